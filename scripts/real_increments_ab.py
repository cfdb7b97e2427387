#!/usr/bin/env python3
"""What the structure functions of spectral fields cost (spectral.real_increments) on one GPU, written to
profiles/real_increments_ab.txt.  256^3 and 512^3, both precisions, '3/2-rule' and '2/3-rule', k = 3 and k = 6 fields:

  (1) the fused call at nsep = 8 against its own composed route: per field one FFT.ifftn(.., dealias) into ONE real work array and
      one spectral.increments sweep of it -- the calls the plan's composed route makes (plan_nonlinear.hip incr_composed), issued
      from the same process, because MFFT_NO_NLZ is read once per process and the two sides have to alternate.  Expectation: the
      fused median <= the composed median + the composed side's spread over the processes (the real array is neither written nor
      read).  With --switch-check one more process per run measures the call itself under MFFT_NO_NLZ=1, recorded beside it.
  (2) the fused call against spectral.real_moments on the same fields at nsep = 1 and nsep = MFFT_INCR_MAXSEP (8: the two other
      counts the issue names coincide).  The ratio is recorded; no expectation, the LDS reads grow with nsep.
  (3) the sweep: spectral.increments against spectral.moments over the same (3, n, n, n) real array at nsep = 1 (expectation:
      level -- median <= the moments side's + its spread) and nsep = 8 (recorded).

Protocol of scripts/real_histogram_ab.py: all sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, the median over the processes [min .. max].

    python scripts/real_increments_ab.py [--procs 3] [--out profiles/real_increments_ab.txt] [--sizes 256,512] [--switch-check]"""
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
from nonlinear_absmax_ab import _fields  # noqa: E402
from nonlinear_dot_ab import ROUNDS, WINDOW_S, _alternate, _wall  # noqa: E402

RULES = ("3/2-rule", "2/3-rule")


def _seps(M, nsep):
    """nsep separations of a row of M points: powers of two below M / 2 (seven at the most), M / 2, odd ones where those run out"""
    s = [x for x in (1, 2, 4, 8, 16, 32, 64) if x < M // 2][:nsep - 1] + [M // 2] if nsep > 1 else [1]
    odd = 3
    while len(s) < nsep:
        s.append(odd)
        odd += 2
    return s[:nsep]


def worker(sizes, switched):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    res = {"term": {}, "sweep": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in RULES:
                M = 3 * n // 2 if dealias == "3/2-rule" else n
                s8, s1 = _seps(M, spectral.INCR_MAXSEP), _seps(M, 1)
                u = None if switched else DeviceArray.empty(tuple(F.work_shape(dealias)), F.float)

                def composed(fields):
                    for x in fields:
                        for i in range(3):
                            F.ifftn(x.component(i), u, dealias)
                            spectral.increments(F, u, s8)
                sides = {}
                for k, bb in ((3, None), (6, b)):
                    sides["incr8_%d" % k] = lambda bb=bb: spectral.real_increments(F, a, bb, dealias, s8, reduce=False)
                    if not switched:
                        sides["incr1_%d" % k] = lambda bb=bb: spectral.real_increments(F, a, bb, dealias, s1, reduce=False)
                        sides["moments_%d" % k] = lambda bb=bb: spectral.real_moments(F, a, bb, dealias, reduce=False)
                        sides["composed8_%d" % k] = lambda bb=bb: composed((a,) if bb is None else (a, bb))
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_increments_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
                del u
            if not switched:
                r3 = DeviceArray.random((3, n, n, n), F.float, seed=5)
                s8, s1 = _seps(n, spectral.INCR_MAXSEP), _seps(n, 1)
                sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"incr1": lambda: spectral.increments(F, r3, s1),
                                                                     "incr8": lambda: spectral.increments(F, r3, s8),
                                                                     "moments": lambda: spectral.moments(F, r3)})
                res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
                del r3
            del F, a, b
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_increments_ab.txt"))
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--switch-check", action="store_true", help="one more process under MFFT_NO_NLZ=1: the call itself on its composed route")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--switched", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return worker(sizes, args.switched)

    def run(extra, env=None):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes=" + args.sizes] + extra, capture_output=True, text=True,
                           timeout=1100, env=dict(os.environ, **(env or {})))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:       # a process that failed is the end of the run: nothing more is started on the device
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("worker failed (rc %d)" % r.returncode)
        return json.loads(lines[0][7:])
    runs = []
    for p in range(args.procs):
        runs.append(run([]))
        print("process %d done" % p, flush=True)
    switched = run(["--switched"], {"MFFT_NO_NLZ": "1"}) if args.switch_check else None

    def stat(vals):
        return statistics.median(vals), min(vals), max(vals)

    def f3(s):
        return "%8.3f [%8.3f .. %8.3f]" % s

    def verdict(h, y):
        return "met" if h[0] <= y[0] + (y[2] - y[1]) else "NOT met"

    from mpifft4py_amd import _lib, spectral
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["Structure functions of spectral fields: scripts/real_increments_ab.py --procs %d --sizes=%s%s" % (args.procs, args.sizes, " --switch-check" if switched else ""),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  MFFT_INCR_MAXSEP = %d." % spectral.INCR_MAXSEP,
         "Registers: real_increments_regs.tsv.  ms, host clock around calls that end in a synchronise of the plan's stream.", "",
         "(1) real_increments of k fields at nsep = 8 against its composed route (per field FFT.ifftn into ONE real work array + spectral.increments,",
         "    the calls of the plan's composed route, same process).  Expectation: fused median <= composed median + the composed side's spread.",
         "    %-26s %-2s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "k", "fused", "composed", "ratio", "")]
    met = {1: True, 3: True}
    for key in runs[0]["term"]:
        for k in ("3", "6"):
            h = stat([r["term"][key]["wall"]["incr8_" + k] for r in runs])
            c = stat([r["term"][key]["wall"]["composed8_" + k] for r in runs])
            met[1] = met[1] and verdict(h, c) == "met"
            extra = "" if not switched else "; the call under MFFT_NO_NLZ=1, one process: %.3f (fused flag %d)" % (
                switched["term"][key]["wall"]["incr8_" + k], switched["term"][key]["flag"])
            o.append("    %-26s %-2s %s  %s  %6.3f  %s (fused flag %d%s)" % (key, k, f3(h), f3(c), h[0] / c[0], verdict(h, c), runs[0]["term"][key]["flag"], extra))
    o.append("    expectation (1) at every case measured: %s" % ("MET" if met[1] else "NOT MET"))
    o += ["", "(2) real_increments at nsep = 1 and nsep = %d (the most one call takes) against real_moments of the same fields; the ratio is recorded, no expectation" % spectral.INCR_MAXSEP,
          "    %-26s %-2s %-30s %-30s %-30s %-8s %s" % ("precision, mesh, rule", "k", "nsep = 1", "nsep = 8", "real_moments", "ratio 1", "ratio 8")]
    for key in runs[0]["term"]:
        for k in ("3", "6"):
            h1 = stat([r["term"][key]["wall"]["incr1_" + k] for r in runs])
            h8 = stat([r["term"][key]["wall"]["incr8_" + k] for r in runs])
            m = stat([r["term"][key]["wall"]["moments_" + k] for r in runs])
            o.append("    %-26s %-2s %s  %s  %s  %7.3f  %7.3f" % (key, k, f3(h1), f3(h8), f3(m), h1[0] / m[0], h8[0] / m[0]))
    o += ["", "(3) the sweep: spectral.increments against spectral.moments over the same (3, n, n, n) real array.  Expectation at nsep = 1: level",
          "    (median <= the moments side's median + its spread); nsep = 8 is recorded",
          "    %-16s %-30s %-30s %-30s %-8s %-8s %s" % ("precision, n", "nsep = 1", "nsep = 8", "moments", "ratio 1", "ratio 8", "")]
    for key in runs[0]["sweep"]:
        h1, h8, m = (stat([r["sweep"][key][w] for r in runs]) for w in ("incr1", "incr8", "moments"))
        met[3] = met[3] and verdict(h1, m) == "met"
        o.append("    %-16s %s  %s  %s  %7.3f  %7.3f  %s" % (key, f3(h1), f3(h8), f3(m), h1[0] / m[0], h8[0] / m[0], verdict(h1, m)))
    o.append("    expectation (3) at every size measured: %s" % ("MET" if met[3] else "NOT MET"))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
