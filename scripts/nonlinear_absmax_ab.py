#!/usr/bin/env python3
"""What the real-space maxima of the fused nonlinear term cost (spectral.cross_transform(.., absmax=True)) on one GPU, written to
profiles/nonlinear_absmax_ab.txt:

  (a) the plan stage `nl_z` (HIP events, mfft_plan_timing_get) of the statistics call -- the Build::AbsMax z kernel and the two
      small fold launches after it -- against `nl_z` of the plain call of the same library, whose kernels scripts/kernel_regs.py
      --diff shows to be the parent commit's: 256^3 and 512^3, '3/2-rule' and '2/3-rule', both precisions; and the same for
      single launches over the rows of scripts/nlz_bench.py (M = 512, 768, 1024, 1536), through meshes with that many z rows;
  (b) the whole statistics call minus the plain call, against what the three velocity maxima cost without it: three dealiased
      FFT.ifftn into (padded) real arrays and one spectral.absmax sweep over them.

Protocol of scripts/nonlinear_dot_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, medians and the spread over the processes.

    python scripts/nonlinear_absmax_ab.py [--procs 3] [--out profiles/nonlinear_absmax_ab.txt] [--sizes 256,512]"""
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
from nonlinear_dot_ab import ROUNDS, WINDOW_S, _alternate, _wall  # noqa: E402

# (M, mesh, rule): z rows of length M, as many as scripts/nlz_bench.py runs (65536, 73728, 49152, 36864)
ZROWS = [(512, (256, 256, 512), None), (768, (256, 128, 512), "3/2-rule"), (1024, (256, 192, 1024), None), (1536, (128, 128, 1024), "3/2-rule")]


def _stage(F, fn, reps, name="nl_z"):
    """ms per call that the plan's stage `name` takes over `reps` calls of fn (HIP events of the plan's stage timers)"""
    F.sync()
    F.reset_timing()
    for _ in range(reps):
        fn()
    F.sync()
    return F.stage_times()[name][0] / reps


def _fields(F):
    from mpifft4py_amd import DeviceArray
    a, b = F.empty_complex(3), F.empty_complex(3)
    for s, x in enumerate((a, b)):
        for i in range(3):
            F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=100 + 3 * s + i), x.component(i))
    return a, b


def worker(sizes):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    res = {"term": {}, "rows": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            out = F.empty_complex(3)
            for dealias in ("3/2-rule", "2/3-rule"):
                u = DeviceArray.empty((3,) + tuple(F.work_shape(dealias)), F.float)

                def stats():
                    spectral.cross_transform(F, a, b, out, dealias, absmax=True)

                def plain():
                    spectral.cross_transform(F, a, b, out, dealias)

                def today():
                    for i in range(3):
                        F.ifftn(a.component(i), u.component(i), dealias)
                    spectral.absmax(F, u)

                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"stats": stats, "plain": plain, "today": today})
                F.enable_timing(True)
                z, _ = _alternate(lambda fn, k: _stage(F, fn, k), {"stats": stats, "plain": plain})
                F.enable_timing(False)
                got = spectral.nonlinear_absmax(F)
                key = "nonlinear_absmax_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, nl_z=z, flag=int(F.plan_info(key)), reps=reps, umax=float(got[0].max()))
                del u
            del F, a, b, out
        for M, mesh, dealias in ZROWS:
            F = Slab_R2C(np.array(mesh), L, SelfComm(0), prec)
            a, b = _fields(F)
            out = F.empty_complex(3)
            F.enable_timing(True)
            z, reps = _alternate(lambda fn, k: _stage(F, fn, k), {
                "stats": lambda: spectral.cross_transform(F, a, b, out, dealias, absmax=True),
                "plain": lambda: spectral.cross_transform(F, a, b, out, dealias),
                "dot_stats": lambda: spectral.dot_transform(F, a, b, out.component(0), dealias, absmax=True),
                "dot_plain": lambda: spectral.dot_transform(F, a, b, out.component(0), dealias)})
            F.enable_timing(False)
            res["rows"]["%s %d" % (prec, M)] = dict(z, mesh=list(mesh), rule=str(dealias), reps=reps)
            del F, a, b, out
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlinear_absmax_ab.txt"))
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
    o = ["Real-space maxima of the fused nonlinear term: scripts/nonlinear_absmax_ab.py --procs %d --sizes %s" % (args.procs, args.sizes),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers: nonlinear_absmax_regs.tsv.", "",
         "(a) plan stage nl_z, ms per nonlinear term (HIP events of the stage timers): cross_transform(absmax=True) -- the AbsMax z kernel and its two",
         "    fold launches -- against the plain call (the parent commit's kernels: kernel_regs.py --diff, 0 changed)",
         "    %-26s %-30s %-30s %s" % ("precision, mesh, rule", "nl_z with maxima", "nl_z plain", "ratio")]
    for key in runs[0]["term"]:
        s = stat([r["term"][key]["nl_z"]["stats"] for r in runs])
        p = stat([r["term"][key]["nl_z"]["plain"] for r in runs])
        o.append("    %-26s %s  %s  %6.3f" % (key, f3(s), f3(p), s[0] / p[0]))
    o += ["", "    the z kernel's rows of scripts/nlz_bench.py through meshes with that many rows (one batch), nl_z in ms: cross product, dot product",
          "    %-16s %-22s %-30s %-30s %-7s %-30s %-30s %s" % ("precision, M", "mesh, rule", "cross with maxima", "cross plain", "ratio", "dot with maxima", "dot plain", "ratio")]
    for key in runs[0]["rows"]:
        t = runs[0]["rows"][key]
        s, p = stat([r["rows"][key]["stats"] for r in runs]), stat([r["rows"][key]["plain"] for r in runs])
        ds, dp = stat([r["rows"][key]["dot_stats"] for r in runs]), stat([r["rows"][key]["dot_plain"] for r in runs])
        o.append("    %-16s %-22s %s  %s  %6.3f  %s  %s  %6.3f" % (key, "%s %s" % (t["mesh"], t["rule"]), f3(s), f3(p), s[0] / p[0], f3(ds), f3(dp), ds[0] / dp[0]))
    o += ["", "(b) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): what the statistic adds (with maxima - plain,",
          "    per process) against what the three velocity maxima cost without it (three dealiased FFT.ifftn + one spectral.absmax sweep)",
          "    %-26s %-30s %-30s %-30s %-30s %s" % ("precision, mesh, rule", "with maxima", "plain", "added", "three ifftn + absmax", "added / today")]
    met = True
    for key in runs[0]["term"]:
        s = stat([r["term"][key]["wall"]["stats"] for r in runs])
        p = stat([r["term"][key]["wall"]["plain"] for r in runs])
        d = stat([r["term"][key]["wall"]["stats"] - r["term"][key]["wall"]["plain"] for r in runs])
        t = stat([r["term"][key]["wall"]["today"] for r in runs])
        ok = d[2] < t[1]
        met = met and ok
        o.append("    %-26s %s  %s  %s  %s  %7.3f  %s (fused flag %d)" % (key, f3(s), f3(p), f3(d), f3(t), d[0] / t[0],
                                                                         "cheaper in every process" if ok else "NOT cheaper in every process", runs[0]["term"][key]["flag"]))
    o.append("    condition (b) -- the statistic costs less than that composition at every size measured: %s" % ("MET" if met else "NOT MET"))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
