#!/usr/bin/env python3
"""What the statistics of quadratic forms of spectral fields cost (spectral.real_quadratic) on one GPU, written to
profiles/real_quadratic_ab.txt:

  (1) the whole call: spectral.real_quadratic of k = 6 and k = 3 fields with 256 bins (range given) against spectral.real_moments
      of the same fields -- the operation as the parent commit has it, on the same data --, 256^3 and 512^3, both precisions,
      '3/2-rule' and '2/3-rule';
  (2) the z stage alone: mfft_nlz_quad_rows against mfft_nlz_moments_rows on the same rows, six fields, n = 512, 768, 1024, 1536,
      both precisions (both calls allocate, launch, fold, copy back and synchronise);
  (3) the sweep: spectral.quadratic against spectral.moments over the same (3, n, n, n) real array.
Expectation for each line: the median is <= the moments side's median plus that side's own spread over the processes -- both
sides load the same rows and run the same transforms, and the quadratic body keeps less state.

Protocol of scripts/real_histogram_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, the median over the processes [min .. max].

    python scripts/real_quadratic_ab.py [--procs 3] [--out profiles/real_quadratic_ab.txt] [--sizes 256,512]"""
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
from real_histogram_ab import LENGTHS, NBINS, ROWS, _host_wall, _rows  # noqa: E402

DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
W6 = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])


def worker(sizes, lengths):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"rows": {}, "term": {}, "sweep": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        code = _lib.precision_code(prec)
        for n in lengths:
            a, b = DeviceArray.from_numpy(_rows(n, prec, False, 1)), DeviceArray.from_numpy(_rows(n, prec, False, 2))
            valid = n // 2 + 1
            hi = 9.0 * 32.0 / n                     # q = sum of six squares of variance 2 / n, weights 1, 1, 1, 2, 2, 2: mean 18 / n
            mom, out6, cnt = np.zeros(36), np.zeros(6), np.zeros(NBINS + 3, dtype=np.int64)
            sides = {"moments": lambda: _lib.call("mfft_nlz_moments_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, None, mom.ctypes.data_as(DP)),
                     "quad": lambda: _lib.call("mfft_nlz_quad_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, W6.ctypes.data_as(DP), 0.0,
                                               -hi / 8, hi, NBINS, out6.ctypes.data_as(DP), cnt.ctypes.data_as(IP))}
            t, reps = _alternate(_host_wall, sides)
            assert cnt.sum() == ROWS * n and cnt[-1] == 0 and np.all(np.isfinite(out6))
            res["rows"]["%s %d" % (prec, n)] = dict(t, reps=reps, inside=float(cnt[1:-2].sum()) / (ROWS * n))
            del a, b
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                sides = {}
                m6 = spectral.real_quadratic(F, a, b, dealias, weights=W6)[0]
                for k, bb, w in ((3, None, W6[:3]), (6, b, W6)):
                    hi = float(m6.mean()[0]) * 8
                    sides["quad%d" % k] = lambda bb=bb, w=w, hi=hi: spectral.real_quadratic(F, a, bb, dealias, weights=w, bins=NBINS, range=(-hi / 8, hi), reduce=False)
                    sides["moments%d" % k] = lambda bb=bb: spectral.real_moments(F, a, bb, dealias, reduce=False)
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_quadratic_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
            r3 = DeviceArray.random((3, n, n, n), F.float, seed=5)
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"quad": lambda: spectral.quadratic(F, r3, bins=NBINS, range=(-0.375, 3.0)),
                                                                 "moments": lambda: spectral.moments(F, r3)})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, r3
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_quadratic_ab.txt"))
    ap.add_argument("--sizes", default="256,512", help="meshes of (1) and (3); empty: neither")
    ap.add_argument("--lengths", default=",".join(str(n) for n in LENGTHS), help="row lengths of (2); empty: no stage cases")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    lengths = [int(x) for x in args.lengths.split(",") if x]
    if args.worker:
        return worker(sizes, lengths)
    runs = []
    for p in range(args.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes=" + args.sizes, "--lengths=" + args.lengths], capture_output=True, text=True, timeout=1100)
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

    def verdict(h, y):
        return "met" if h[0] <= y[0] + (y[2] - y[1]) else "NOT met"

    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["Statistics of quadratic forms of spectral fields: scripts/real_quadratic_ab.py --procs %d --sizes=%s --lengths=%s" % (args.procs, args.sizes, args.lengths),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers: real_quadratic_regs.tsv.",
         "Expectation on every line: median <= the moments side's median + that side's spread (max - min) over the processes.", "",
         "(1) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_quadratic of k fields, %d bins, range given," % NBINS,
         "    against real_moments of the same fields",
         "    %-26s %-2s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "k", "real_quadratic", "real_moments", "ratio", "")]
    met = {1: True, 2: True, 3: True}
    for key in runs[0]["term"]:
        for k in ("6", "3"):
            h = stat([r["term"][key]["wall"]["quad" + k] for r in runs])
            m = stat([r["term"][key]["wall"]["moments" + k] for r in runs])
            met[1] = met[1] and verdict(h, m) == "met"
            o.append("    %-26s %-2s %s  %s  %6.3f  %s (fused flag %d)" % (key, k, f3(h), f3(m), h[0] / m[0], verdict(h, m), runs[0]["term"][key]["flag"]))
    o.append("    expectation (1) at every size measured: %s" % ("MET" if met[1] else "NOT MET"))
    o += ["", "(2) the z stage alone, ms per call (host clock; each call allocates, launches, folds, copies back and synchronises): %d rows x 6 fields," % ROWS,
          "    Gaussian spectra; quadratic: weights 1, 1, 1, 2, 2, 2, %d bins; inside = the share of the points inside the range" % NBINS,
          "    %-16s %-30s %-30s %-7s %-7s %s" % ("precision, n", "mfft_nlz_quad_rows", "mfft_nlz_moments_rows", "ratio", "inside", "")]
    for key in runs[0]["rows"]:
        m = stat([r["rows"][key]["moments"] for r in runs])
        h = stat([r["rows"][key]["quad"] for r in runs])
        met[2] = met[2] and verdict(h, m) == "met"
        o.append("    %-16s %s  %s  %6.3f  %6.4f  %s" % (key, f3(h), f3(m), h[0] / m[0], runs[0]["rows"][key]["inside"], verdict(h, m)))
    o.append("    expectation (2) at every case measured: %s" % ("MET" if met[2] else "NOT MET"))
    o += ["", "(3) the sweep, ms: spectral.quadratic (%d bins, range given) against spectral.moments over the same (3, n, n, n) real array" % NBINS,
          "    %-16s %-30s %-30s %-7s %s" % ("precision, n", "quadratic", "moments", "ratio", "")]
    for key in runs[0]["sweep"]:
        h, m = stat([r["sweep"][key]["quad"] for r in runs]), stat([r["sweep"][key]["moments"] for r in runs])
        met[3] = met[3] and verdict(h, m) == "met"
        o.append("    %-16s %s  %s  %6.3f  %s" % (key, f3(h), f3(m), h[0] / m[0], verdict(h, m)))
    o.append("    expectation (3) at every size measured: %s" % ("MET" if met[3] else "NOT MET"))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
