#!/usr/bin/env python3
"""What the histograms of spectral fields cost (spectral.real_histogram) on one GPU, written to profiles/real_histogram_ab.txt:

  (a) the z stage alone: mfft_nlz_hist_rows against mfft_nlz_moments_rows on the same rows, six fields, n = 512, 768, 1024, 1536,
      both precisions, two data sets -- random spectra, and a smooth field (rows of a Taylor-Green-like field: one low mode per
      row, the hot-slot worst case: a whole wave adds to one or two slots) -- and two builds of the histogram kernels: the plain
      LDS add (shipped) and, where build/libmpifft4py_amd_nlhmerge.so exists (`make -C mpifft4py_amd/csrc nlh_variant`), the one
      that merges runs of equal slot inside the wave first.  Both calls allocate, launch, fold, copy back and synchronise;
  (b) the whole call: spectral.real_histogram (range given) against spectral.real_moments, 256^3 and 512^3, both precisions,
      '3/2-rule' and '2/3-rule', k = 3 and 6 fields;
  (c) the sweep: spectral.histogram against spectral.moments on the same (3, n, n, n) real array.
Expectation for each: the median is <= the moments side's median plus that yardstick's own spread over the processes.

Protocol of scripts/real_moments_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, medians and the spread over the processes.
  (d) `--append-pmc DIR`: the LDS counters of a counter run of its own are appended to the file:
      rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -- python scripts/real_histogram_ab.py --pmc-worker

    python scripts/real_histogram_ab.py [--procs 3] [--out profiles/real_histogram_ab.txt] [--sizes 256,512]"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nonlinear_absmax_ab import _fields  # noqa: E402
from nonlinear_dot_ab import ROUNDS, WINDOW_S, _alternate, _wall  # noqa: E402

VARIANT = os.environ.get("MFFT_NLH_VARIANT", os.path.join(ROOT, "mpifft4py_amd", "csrc", "build", "libmpifft4py_amd_nlhmerge.so"))
LENGTHS = (512, 768, 1024, 1536)
ROWS = 36864                     # rows of a stage case: 36864 x 1536 x 6 fields in double precision are 2.7 GB
NBINS = 256
DP, IP, V = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p


def _host_wall(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def _rows(n, prec, smooth, seed):
    """(3, ROWS, n / 2 + 1) spectra: Gaussian bins, or ONE low mode per row (amplitude by row, mode 1 .. 3)."""
    ct = np.complex128 if prec == "double" else np.complex64
    rng = np.random.default_rng(seed)
    shape = (3, ROWS, n // 2 + 1)
    if not smooth:
        return rng.standard_normal(shape + (2,), dtype=np.float32).view(np.complex64)[..., 0].astype(ct)
    x = np.zeros(shape, dtype=ct)
    r = np.arange(ROWS)
    for f in range(3):
        x[f, r, 1 + (r + f) % 3] = (0.5 * n * np.cos(2 * np.pi * r / ROWS + f)).astype(ct)
    return x


def worker(sizes, lengths):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"rows": {}, "term": {}, "sweep": {}, "variant": os.path.exists(VARIANT)}
    L = np.array([2 * np.pi] * 3)
    var = None
    if res["variant"]:           # the second build in the same process, its symbols to itself; it runs on the same device arrays
        var = ctypes.CDLL(VARIANT, mode=ctypes.RTLD_LOCAL)
        var.mfft_nlz_hist_rows.argtypes = [V, V, ctypes.c_int] + [ctypes.c_int64] * 5 + [ctypes.c_int, DP, DP, ctypes.c_int, IP]
    for prec in ("double", "single"):
        code = _lib.precision_code(prec)
        for n in lengths:
            for smooth in (False, True):
                a, b = DeviceArray.from_numpy(_rows(n, prec, smooth, 1)), DeviceArray.from_numpy(_rows(n, prec, smooth, 2))
                valid = n // 2 + 1
                s = 0.6 if smooth else 4 * np.sqrt(2.0 / n)
                lo, hi = np.full(6, -s), np.full(6, s)
                mom, cnt = np.zeros(36), np.zeros((6, NBINS + 3), dtype=np.int64)
                hist_args = (a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), NBINS, cnt.ctypes.data_as(IP))
                sides = {"moments": lambda: _lib.call("mfft_nlz_moments_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, None, mom.ctypes.data_as(DP)),
                         "hist": lambda: _lib.call("mfft_nlz_hist_rows", *hist_args)}
                if var is not None:
                    def merged():
                        if var.mfft_nlz_hist_rows(*hist_args) != 0:
                            raise RuntimeError("the variant library refused the call")
                    sides["hist_merge"] = merged
                t, reps = _alternate(_host_wall, sides)
                plain = cnt.copy()
                if var is not None:
                    merged()
                    assert np.array_equal(cnt, plain), "the two builds disagree"
                assert np.all(plain.sum(1) == ROWS * n)
                res["rows"]["%s %d %s" % (prec, n, "smooth" if smooth else "random")] = dict(
                    t, reps=reps, hottest=float(plain[:, 1:-2].max()) / (ROWS * n))
                del a, b
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                sides = {}
                for k, bb in ((3, None), (6, b)):
                    rng = np.tile([-0.6, 0.6], (k, 1))
                    sides["hist%d" % k] = lambda bb=bb, rng=rng: spectral.real_histogram(F, a, bb, dealias, bins=NBINS, range=rng, reduce=False)
                    sides["moments%d" % k] = lambda bb=bb: spectral.real_moments(F, a, bb, dealias, reduce=False)
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_histogram_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
            r3 = DeviceArray.random((3, n, n, n), F.float, seed=5)
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"hist": lambda: spectral.histogram(F, r3, bins=NBINS, range=(0.0, 1.0)),
                                                                 "moments": lambda: spectral.moments(F, r3)})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, r3
    print("RESULT " + json.dumps(res), flush=True)


def pmc_worker():
    """The 512-point double-precision stage kernel on both data sets, a few launches each: the subject of a counter run."""
    from mpifft4py_amd import DeviceArray, _lib
    n, valid = 512, 257
    for smooth in (False, True):
        a, b = DeviceArray.from_numpy(_rows(n, "double", smooth, 1)), DeviceArray.from_numpy(_rows(n, "double", smooth, 2))
        s = 0.6 if smooth else 4 * np.sqrt(2.0 / n)
        lo, hi = np.full(6, -s), np.full(6, s)
        cnt = np.zeros((6, NBINS + 3), dtype=np.int64)
        for _ in range(3):
            _lib.call("mfft_nlz_hist_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, _lib.DOUBLE, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
                      NBINS, cnt.ctypes.data_as(IP))
        del a, b


def append_pmc(out, d):
    """Per kernel launch of the histogram z kernel: the two LDS counters, in launch order (three launches random, three smooth)."""
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        rows += list(csv.DictReader(open(path)))
    per = {}
    for r in rows:
        if "NlzHist" in r.get("Kernel_Name", ""):
            per.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    o = ["", "(d) LDS counters of the 512-point double-precision histogram z kernel (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE, a run of its own:",
         "    scripts/real_histogram_ab.py --pmc-worker): %d rows x 6 fields per launch, three launches on random spectra, then three on the smooth rows" % ROWS,
         "    %-10s %-22s %-22s %s" % ("launch", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "conflict cycles per active cycle")]
    for i, k in enumerate(sorted(per)):
        c, a = per[k].get("SQ_LDS_BANK_CONFLICT", float("nan")), per[k].get("SQ_LDS_IDX_ACTIVE", float("nan"))
        o.append("    %-10s %-22.0f %-22.0f %.3f" % ("%d %s" % (i, "random" if i < len(per) // 2 else "smooth"), c, a, c / a if a else float("nan")))
    if not per:
        o.append("    (no counter rows found under %s)" % d)
    with open(out, "a") as f:
        f.write("\n".join(o) + "\n")
    print("\n".join(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_histogram_ab.txt"))
    ap.add_argument("--sizes", default="256,512", help="meshes of (b) and (c); empty: neither")
    ap.add_argument("--lengths", default=",".join(str(n) for n in LENGTHS), help="row lengths of (a); empty: no stage cases")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--pmc-worker", action="store_true")
    ap.add_argument("--append-pmc", default=None)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    lengths = [int(x) for x in args.lengths.split(",") if x]
    if args.worker:
        return worker(sizes, lengths)
    if args.pmc_worker:
        return pmc_worker()
    if args.append_pmc:
        return append_pmc(args.out, args.append_pmc)
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
    variant = runs[0]["variant"]
    o = ["Histograms of spectral fields: scripts/real_histogram_ab.py --procs %d --sizes=%s --lengths=%s" % (args.procs, args.sizes, args.lengths),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers: real_histogram_regs.tsv.",
         "Expectation everywhere: median <= the moments side's median + that side's spread (max - min) over the processes.", "",
         "(a) the z stage alone, ms per call (host clock; each call allocates, launches, folds, copies back and synchronises): %d rows x 6 fields, %d bins;" % (ROWS, NBINS),
         "    random: Gaussian spectra, +-4 sigma; smooth: one low mode per row (hot slots); hottest = the largest share of a field's points in ONE bin;",
         "    merge = the build that merges runs of equal slot inside the wave before the LDS add%s" % ("" if variant else " (NOT built for this run)"),
         "    %-24s %-30s %-30s %-30s %-8s %-8s %s" % ("precision, n, data", "moments", "histogram (plain add)", "histogram (merge)", "plain/m", "merge/m", "hottest")]
    met_a = True
    plain_wins = merge_wins = 0
    for key in runs[0]["rows"]:
        m = stat([r["rows"][key]["moments"] for r in runs])
        h = stat([r["rows"][key]["hist"] for r in runs])
        g = stat([r["rows"][key]["hist_merge"] for r in runs]) if variant else None
        met_a = met_a and verdict(h, m) == "met"
        if g:
            plain_wins += h[0] <= g[0]
            merge_wins += g[0] < h[0]
        o.append("    %-24s %s  %s  %s  %6.3f   %s   %.3f  %s" % (key, f3(m), f3(h), f3(g) if g else "%-30s" % "-", h[0] / m[0],
                                                                    "%6.3f" % (g[0] / m[0]) if g else "     -", runs[0]["rows"][key]["hottest"], verdict(h, m)))
    o.append("    expectation (a), plain add, at every case measured: %s" % ("MET" if met_a else "NOT MET"))
    if variant:
        o.append("    plain add against merge: the plain add is ahead or even in %d cases, the merge in %d" % (plain_wins, merge_wins))
    o += ["", "(b) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_histogram of k fields, range given, against",
          "    real_moments of the same fields",
          "    %-26s %-2s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "k", "real_histogram", "real_moments", "ratio", "")]
    met_b = True
    for key in runs[0]["term"]:
        for k in ("3", "6"):
            h = stat([r["term"][key]["wall"]["hist" + k] for r in runs])
            m = stat([r["term"][key]["wall"]["moments" + k] for r in runs])
            met_b = met_b and verdict(h, m) == "met"
            o.append("    %-26s %-2s %s  %s  %6.3f  %s (fused flag %d)" % (key, k, f3(h), f3(m), h[0] / m[0], verdict(h, m), runs[0]["term"][key]["flag"]))
    o.append("    expectation (b) at every size measured: %s" % ("MET" if met_b else "NOT MET"))
    o += ["", "(c) the sweep, ms: spectral.histogram (%d bins, range given) against spectral.moments over the same (3, n, n, n) real array" % NBINS,
          "    %-16s %-30s %-30s %-7s %s" % ("precision, n", "histogram", "moments", "ratio", "")]
    met_c = True
    for key in runs[0]["sweep"]:
        h, m = stat([r["sweep"][key]["hist"] for r in runs]), stat([r["sweep"][key]["moments"] for r in runs])
        met_c = met_c and verdict(h, m) == "met"
        o.append("    %-16s %s  %s  %6.3f  %s" % (key, f3(h), f3(m), h[0] / m[0], verdict(h, m)))
    o.append("    expectation (c) at every size measured: %s" % ("MET" if met_c else "NOT MET"))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
