#!/usr/bin/env python3
"""What the one-point statistics of spectral fields cost (spectral.real_moments) on one GPU, written to
profiles/real_moments_ab.txt:

  (a) real_moments of 3 and of 6 fields against that many FFT.ifftn(.., dealias) of the same plan in the same process -- the
      transforms alone, no sweep, no host copy: code the parent commit already has.  256^3 and 512^3, both precisions, '3/2-rule'
      and '2/3-rule'.  The operation writes no real array, so the target is <= 1.00 x outside the yardstick's own spread over the
      processes; with it the plan's stage times nl_x_inv / nl_y_inv / nl_z of the six-field call;
  (b) the plan stage `nl_z` of the six-field moments call against `nl_z` of the cross product over the rows of
      scripts/nlz_bench.py (M = 512, 768, 1024, 1536), through meshes with that many z rows;
  (c) spectral.moments against spectral.absmax over the same (3, n, n, n) real array.

Protocol of scripts/nonlinear_dot_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, medians and the spread over the processes.

    python scripts/real_moments_ab.py [--procs 3] [--out profiles/real_moments_ab.txt] [--sizes 256,512]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nonlinear_absmax_ab import ZROWS, _fields  # noqa: E402
from nonlinear_dot_ab import ROUNDS, WINDOW_S, _alternate, _wall  # noqa: E402

STAGES = ("nl_x_inv", "nl_y_inv", "nl_z")


def _stages(F, fn, reps):
    """ms per call of each of the plan's stages over `reps` calls of fn (HIP events of the plan's stage timers)"""
    F.sync()
    F.reset_timing()
    for _ in range(reps):
        fn()
    F.sync()
    t = F.stage_times()
    return {k: t[k][0] / reps for k in STAGES if k in t}


def worker(sizes):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    res = {"term": {}, "rows": {}, "sweep": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                u = DeviceArray.empty(tuple(F.work_shape(dealias)), F.float)

                def back(x):
                    for i in range(3):
                        F.ifftn(x.component(i), u, dealias)

                sides = {"moments3": lambda: spectral.real_moments(F, a, None, dealias, reduce=False), "ifftn3": lambda: back(a),
                         "moments6": lambda: spectral.real_moments(F, a, b, dealias, reduce=False), "ifftn6": lambda: (back(a), back(b))}
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                F.enable_timing(True)
                st = _stages(F, sides["moments6"], max(3, reps["moments6"] // 2))
                F.enable_timing(False)
                key = "nonlinear_moments_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, stages=st, flag=int(F.plan_info(key)), reps=reps)
                del u
            r3 = DeviceArray.random((3, n, n, n), F.float, seed=5)
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"moments": lambda: spectral.moments(F, r3), "absmax": lambda: spectral.absmax(F, r3)})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, r3
        for M, mesh, dealias in ZROWS:
            F = Slab_R2C(np.array(mesh), L, SelfComm(0), prec)
            a, b = _fields(F)
            out = F.empty_complex(3)
            F.enable_timing(True)
            z, reps = _alternate(lambda fn, k: _stages(F, fn, k)["nl_z"], {
                "moments": lambda: spectral.real_moments(F, a, b, dealias, reduce=False),
                "cross": lambda: spectral.cross_transform(F, a, b, out, dealias)})
            F.enable_timing(False)
            res["rows"]["%s %d" % (prec, M)] = dict(z, mesh=list(mesh), rule=str(dealias), reps=reps)
            del F, a, b, out
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_moments_ab.txt"))
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return worker(sizes)
    runs = []
    for p in range(args.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes", args.sizes], capture_output=True, text=True, timeout=1100)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:       # a process that failed is the end of the run: nothing more is started on the device
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("worker %d failed (rc %d)" % (p, r.returncode))
        runs.append(json.loads(lines[0][7:]))
        print("process %d done" % p, flush=True)

    def stat(vals):
        return statistics.median(vals), min(vals), max(vals)

    def f3(s):
        return "%8.3f [%8.3f .. %8.3f]" % s

    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["One-point statistics of spectral fields: scripts/real_moments_ab.py --procs %d --sizes %s" % (args.procs, args.sizes),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers: real_moments_regs.tsv.", "",
         "(a) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_moments of k fields against k FFT.ifftn(.., dealias)",
         "    into one real array (the transforms alone: no sweep, no host copy).  Target: <= 1.00 x outside the yardstick's spread over the processes.",
         "    %-26s %-2s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "k", "real_moments", "k ifftn", "ratio", "")]
    met = True
    for key in runs[0]["term"]:
        for k in ("3", "6"):
            m = stat([r["term"][key]["wall"]["moments" + k] for r in runs])
            y = stat([r["term"][key]["wall"]["ifftn" + k] for r in runs])
            ok = m[0] <= y[0] + (y[2] - y[1])
            met = met and ok
            o.append("    %-26s %-2s %s  %s  %6.3f  %s (fused flag %d)" % (key, k, f3(m), f3(y), m[0] / y[0], "met" if ok else "NOT met", runs[0]["term"][key]["flag"]))
    o.append("    target (a) at every size measured: %s" % ("MET" if met else "NOT MET"))
    o += ["", "    stages of the six-field call, ms per call (HIP events of the plan's stage timers)",
          "    %-26s %-30s %-30s %s" % ("precision, mesh, rule", "nl_x_inv", "nl_y_inv", "nl_z")]
    for key in runs[0]["term"]:
        o.append("    %-26s %s" % (key, "  ".join(f3(stat([r["term"][key]["stages"][s] for r in runs])) for s in STAGES)))
    o += ["", "(b) plan stage nl_z, ms: the six-field moments kernel and its fold against the cross kernel over the rows of scripts/nlz_bench.py (one batch);",
          "    from the counts: 3 / 4.5 transforms and 6 / 9 rows per (x, y) point",
          "    %-16s %-26s %-30s %-30s %s" % ("precision, M", "mesh, rule", "moments", "cross", "ratio")]
    for key in runs[0]["rows"]:
        t = runs[0]["rows"][key]
        m, c = stat([r["rows"][key]["moments"] for r in runs]), stat([r["rows"][key]["cross"] for r in runs])
        o.append("    %-16s %-26s %s  %s  %6.3f" % (key, "%s %s" % (t["mesh"], t["rule"]), f3(m), f3(c), m[0] / c[0]))
    o += ["", "(c) the sweep, ms: spectral.moments against spectral.absmax over the same (3, n, n, n) real array (no target)",
          "    %-16s %-30s %-30s %s" % ("precision, n", "moments", "absmax", "ratio")]
    for key in runs[0]["sweep"]:
        m, c = stat([r["sweep"][key]["moments"] for r in runs]), stat([r["sweep"][key]["absmax"] for r in runs])
        o.append("    %-16s %s  %s  %6.3f" % (key, f3(m), f3(c), m[0] / c[0]))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
