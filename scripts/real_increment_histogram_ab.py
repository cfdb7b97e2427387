#!/usr/bin/env python3
"""What the increment PDFs of spectral fields cost (spectral.real_increment_histogram) on one GPU, written to
profiles/real_increment_histogram_ab.txt:

  (1) the whole call: spectral.real_increment_histogram (nsep = 8, 128 bins, ranges given) against spectral.real_increments at the same
      eight separations on the same fields, 256^3 and 512^3, both precisions, '3/2-rule' and '2/3-rule', three and six fields.  Both run
      the same transforms and read the row back shifted; the yardstick holds 48 doubles of accumulators, the new body none and issues
      an LDS add per increment.  Expectation: no slower than real_increments plus that yardstick's own spread over the processes;
  (2) the fused call against its composed route: per field one FFT.ifftn(.., dealias) into ONE real work array and one
      spectral.increment_histogram sweep of it -- the calls the plan's composed route makes (plan_nonlinear.hip reduce_composed),
      issued from the same process, because MFFT_NO_NLZ is read once per process and the two sides have to alternate.
      Expectation: no slower than the composed route plus its spread;
  (3) the z stage alone: mfft_nlz_incr_hist_rows against mfft_nlz_incr_rows on the same rows (36864 rows x 6 fields, eight
      separations, 128 bins over +-4 sigma of Gaussian spectra), 512 / 768 / 1024 / 1536, both precisions.  Expectation: no slower than
      the increments stage plus its spread;
  (4) the sweep: spectral.increment_histogram against spectral.increments of the same (3, n, n, n) real array at the same eight
      separations.  Expectation: no slower than the increments sweep plus its spread.
Several ranks and pencils are tested (tests/test_gpu_real_increment_histogram.py), not timed.

Protocol of scripts/real_joint_ab.py: both sides in the same process, alternating windows of at least half a second after a warm-up
of every shape, several fresh processes, medians and the spread over the processes.

    python scripts/real_increment_histogram_ab.py [--procs 3] [--out profiles/real_increment_histogram_ab.txt] [--sizes 256,512] [--lengths ...]"""
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
from real_histogram_ab import _host_wall  # noqa: E402
from real_increments_ab import _seps  # noqa: E402
from real_joint_ab import _rows  # noqa: E402

LENGTHS = (512, 768, 1024, 1536)
ROWS = 36864
NB = 128
NSEP = 8
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)


def worker(sizes, lengths):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"rows": {}, "term": {}, "sweep": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        code = _lib.precision_code(prec)
        for n in lengths:
            a, b = _rows(DeviceArray, n, prec, 1), _rows(DeviceArray, n, prec, 2)
            valid = n // 2 + 1
            sv = np.ascontiguousarray(_seps(n, NSEP), dtype=np.int64)
            s = 4 * np.sqrt(2.0 / n) * 1.5 * np.sqrt(2.0)
            lo, hi = np.full(6 * NSEP, -s), np.full(6 * NSEP, s)
            cnt, sums = np.zeros((6, NSEP, NB + 3), dtype=np.int64), np.zeros(6 * NSEP * 3)
            sides = {"incr": lambda: _lib.call("mfft_nlz_incr_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, sv.ctypes.data_as(IP), NSEP,
                                               sums.ctypes.data_as(DP)),
                     "incr_hist": lambda: _lib.call("mfft_nlz_incr_hist_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, sv.ctypes.data_as(IP), NSEP,
                                                    lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), NB, cnt.ctypes.data_as(IP))}
            t, reps = _alternate(_host_wall, sides)
            assert np.all(cnt.sum(2) == ROWS * n)
            res["rows"]["%s %d" % (prec, n)] = dict(t, reps=reps, groups=int(_lib.call("mfft_nlz_incr_hist_groups", ROWS, n, code)),
                                                    incr_groups=int(_lib.call("mfft_nlz_incr_groups", ROWS, n, code)),
                                                    outside=float((cnt[:, :, 0].sum() + cnt[:, :, -2:].sum()) / cnt.sum()))
            del a, b
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                M = 3 * n // 2 if dealias == "3/2-rule" else n
                s8 = _seps(M, NSEP)
                u = DeviceArray.empty(tuple(F.work_shape(dealias)), F.float)
                rg = (-0.6, 0.6)

                def composed(fields):
                    for x in fields:
                        for i in range(3):
                            F.ifftn(x.component(i), u, dealias)
                            spectral.increment_histogram(F, u, seps=s8, bins=NB, range=rg)
                sides = {}
                for k, bb in ((3, None), (6, b)):
                    sides["incr_hist_%d" % k] = lambda bb=bb: spectral.real_increment_histogram(F, a, bb, dealias, seps=s8, bins=NB, range=rg, reduce=False)
                    sides["incr_%d" % k] = lambda bb=bb: spectral.real_increments(F, a, bb, dealias, s8, reduce=False)
                    sides["composed_%d" % k] = lambda bb=bb: composed((a,) if bb is None else (a, bb))
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_incr_hist_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
                del u
            r3 = DeviceArray.random((3, n, n, n), F.float, seed=5)
            s8 = _seps(n, NSEP)
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"incr_hist": lambda: spectral.increment_histogram(F, r3, seps=s8, bins=NB, range=(-1.0, 1.0)),
                                                                 "incr": lambda: spectral.increments(F, r3, s8)})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, r3
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_increment_histogram_ab.txt"))
    ap.add_argument("--sizes", default="256,512", help="meshes of (1), (2) and (4); empty: none of them")
    ap.add_argument("--lengths", default=",".join(str(n) for n in LENGTHS), help="row lengths of (3); empty: no stage cases")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    lengths = [int(x) for x in args.lengths.split(",") if x]
    if args.worker:
        return worker(sizes, lengths)
    runs = []
    for p in range(args.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes=" + args.sizes, "--lengths=" + args.lengths], capture_output=True, text=True, timeout=560)
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
    o = ["Increment PDFs of spectral fields: scripts/real_increment_histogram_ab.py --procs %d --sizes=%s --lengths=%s" % (args.procs, args.sizes, args.lengths),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers and LDS:",
         "real_increment_histogram_regs.tsv.  Expectation everywhere: median <= the yardstick's median + the yardstick's spread (max - min) over the",
         "processes.  Several ranks and pencils are tested (tests/test_gpu_real_increment_histogram.py), not timed.", ""]
    for title, side, yard, what in (
            ("(1) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_increment_histogram, nsep = %d, %d bins,\n"
             "    ranges given, against real_increments at the same separations on the same k fields" % (NSEP, NB), "incr_hist_", "incr_", "real_increments"),
            ("(2) the fused call against its composed route, ms (per field FFT.ifftn into ONE real work array + spectral.increment_histogram, same process)",
             "incr_hist_", "composed_", "composed")):
        o += [title, "    %-26s %-2s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "k", "real_increment_histogram", what, "ratio", "")]
        met = True
        for key in runs[0]["term"]:
            for k in ("3", "6"):
                j = stat([r["term"][key]["wall"][side + k] for r in runs])
                h = stat([r["term"][key]["wall"][yard + k] for r in runs])
                met = met and verdict(j, h) == "met"
                o.append("    %-26s %-2s %s  %s  %6.3f  %s (fused flag %d)" % (key, k, f3(j), f3(h), j[0] / h[0], verdict(j, h), runs[0]["term"][key]["flag"]))
        o += ["    expectation at every size measured: %s" % ("MET" if met else "NOT MET"), ""]
    o += ["(3) the z stage alone, ms per call (host clock; each call allocates, launches, folds, copies back and synchronises): %d rows x 6 fields," % ROWS,
          "    %d separations, %d bins; wgs = workgroups of the launch, increment histogram / increments: resident per CU x CUs" % (NSEP, NB),
          "    %-16s %-30s %-30s %-7s %-10s %s" % ("precision, n", "increments stage", "increment-histogram stage", "ratio", "wgs", "")]
    met = True
    for key in runs[0]["rows"]:
        h = stat([r["rows"][key]["incr"] for r in runs])
        j = stat([r["rows"][key]["incr_hist"] for r in runs])
        met = met and verdict(j, h) == "met"
        o.append("    %-16s %s  %s  %6.3f  %-10s %s (outside the range: %.2e)" % (key, f3(h), f3(j), j[0] / h[0], "%d / %d" % (runs[0]["rows"][key]["groups"], runs[0]["rows"][key]["incr_groups"]),
                                                                             verdict(j, h), runs[0]["rows"][key]["outside"]))
    o += ["    expectation (3) at every case measured: %s" % ("MET" if met else "NOT MET"), "",
          "(4) the sweep, ms: spectral.increment_histogram (%d bins) against spectral.increments of the same (3, n, n, n) real array, %d separations" % (NB, NSEP),
          "    %-16s %-30s %-30s %-7s %s" % ("precision, n", "increment_histogram", "increments", "ratio", "")]
    met = True
    for key in runs[0]["sweep"]:
        j, h = stat([r["sweep"][key]["incr_hist"] for r in runs]), stat([r["sweep"][key]["incr"] for r in runs])
        met = met and verdict(j, h) == "met"
        o.append("    %-16s %s  %s  %6.3f  %s" % (key, f3(j), f3(h), j[0] / h[0], verdict(j, h)))
    o.append("    expectation (4) at every size measured: %s" % ("MET" if met else "NOT MET"))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
