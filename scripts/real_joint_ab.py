#!/usr/bin/env python3
"""What the joint histograms of spectral fields cost (spectral.real_joint_histogram) on one GPU, written to
profiles/real_joint_ab.txt:

  (1) the whole call: spectral.real_joint_histogram (64 x 64 bins, range given) against spectral.real_histogram (64 bins) on the
      same six fields, 256^3 and 512^3, both precisions, '3/2-rule' and '2/3-rule', ncomp = 3.  Both run the same transforms and
      loads; the joint body does one LDS add per point where the histogram body does two.  Expectation: no slower than the
      histogram call plus that yardstick's own spread over the processes;
  (2) the fused call against its composed route: per pair two FFT.ifftn(.., dealias) into TWO real work arrays and one
      spectral.joint_histogram sweep of them -- the calls the plan's composed route makes (plan_nonlinear.hip joint_composed),
      issued from the same process, because MFFT_NO_NLZ is read once per process and the two sides have to alternate.
      Expectation: no slower than the composed route plus its spread;
  (3) the z stage alone: mfft_nlz_joint_rows against mfft_nlz_hist_rows on the same rows (36864 rows x 6 fields, 64 bins per
      field, Gaussian spectra over +-4 sigma), both precisions, and, where build/libmpifft4py_amd_nljtwin.so exists
      (`make -C mpifft4py_amd/csrc nlj_variant`), the alternative build of the joint kernels: (a) = the shipped LDS rule (csrc/
      registry_nlz.h nlj_split: the split exchange where the grid would cost the second resident workgroup, hence a barrier build),
      (b) = the histogram twin's exchange and wave build with the LDS that then takes.  The two differ for the kernels the
      rule changes; everywhere else they are the same code.  Expectation: (a) no slower than the histogram stage plus its spread;
  (4) the sweep: spectral.joint_histogram of two (3, n, n, n) real arrays against spectral.histogram of one (6, n, n, n) array
      over the same bytes.  Expectation: level (no slower than the histogram sweep plus its spread).
Several ranks and pencils are tested (tests/test_gpu_real_joint.py), not timed.

Protocol of scripts/real_histogram_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, medians and the spread over the processes.

    python scripts/real_joint_ab.py [--procs 3] [--out profiles/real_joint_ab.txt] [--sizes 256,512] [--lengths ...]"""
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

VARIANT = os.environ.get("MFFT_NLJ_VARIANT", os.path.join(ROOT, "mpifft4py_amd", "csrc", "build", "libmpifft4py_amd_nljtwin.so"))
# 512: a kernel the rule leaves alone; the others: the kernels whose exchange the rule changes (double precision 768 .. 2304 and
# 4096, single precision 4096; profiles/real_joint_regs.tsv)
LENGTHS = (512, 768, 1296, 1536, 2048, 2304, 4096)
ROWS = 36864
NB = 64
DP, IP, V = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p


def _rows(DeviceArray, n, prec, seed):
    """(3, ROWS, n / 2 + 1) Gaussian spectra on the device: one draw per array, the components scaled apart."""
    ct = np.complex128 if prec == "double" else np.complex64
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((ROWS, n // 2 + 1, 2), dtype=np.float32).view(np.complex64)[..., 0]
    x = DeviceArray.empty((3, ROWS, n // 2 + 1), ct)
    for f in range(3):
        x.component(f).set((base * np.float32(1.0 + 0.25 * f)).astype(ct))
    return x


def worker(sizes, lengths):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"rows": {}, "term": {}, "sweep": {}, "variant": os.path.exists(VARIANT)}
    L = np.array([2 * np.pi] * 3)
    var = None
    if res["variant"]:           # the second build in the same process, its symbols to itself; it runs on the same device arrays
        var = ctypes.CDLL(VARIANT, mode=ctypes.RTLD_LOCAL)
        var.mfft_nlz_joint_rows.argtypes = [V, V, ctypes.c_int] + [ctypes.c_int64] * 5 + [ctypes.c_int, DP, DP, ctypes.c_int, ctypes.c_int, IP]
    for prec in ("double", "single"):
        code = _lib.precision_code(prec)
        for n in lengths:
            a, b = _rows(DeviceArray, n, prec, 1), _rows(DeviceArray, n, prec, 2)
            valid = n // 2 + 1
            s = 4 * np.sqrt(2.0 / n) * 1.5
            lo, hi = np.full(6, -s), np.full(6, s)
            cnt, grid = np.zeros((6, NB + 3), dtype=np.int64), np.zeros((3, NB + 3, NB + 3), dtype=np.int64)
            jargs = (a.ptr, b.ptr, 3, ROWS, n, valid, valid, 0, code, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), NB, NB, grid.ctypes.data_as(IP))
            sides = {"hist": lambda: _lib.call("mfft_nlz_hist_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, lo.ctypes.data_as(DP),
                                               hi.ctypes.data_as(DP), NB, cnt.ctypes.data_as(IP)),
                     "joint": lambda: _lib.call("mfft_nlz_joint_rows", *jargs)}
            if var is not None:
                def twin():
                    if var.mfft_nlz_joint_rows(*jargs) != 0:
                        raise RuntimeError("the variant library refused the call")
                sides["joint_twin"] = twin
            t, reps = _alternate(_host_wall, sides)
            shipped = grid.copy()
            if var is not None:
                twin()
                assert np.array_equal(grid, shipped), "the two builds disagree"
            assert np.all(shipped.sum((1, 2)) == ROWS * n)
            same = bool(np.array_equal(shipped.sum(2), cnt[:3]) and np.array_equal(shipped.sum(1), cnt[3:]))      # (an observation, not a contract)
            res["rows"]["%s %d" % (prec, n)] = dict(t, reps=reps, marginals_equal=same, groups=int(_lib.call("mfft_nlz_joint_groups", ROWS, n, code)),
                                                    hist_groups=int(_lib.call("mfft_nlz_hist_groups", ROWS, n, code)))
            del a, b
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                r1, r2 = DeviceArray.empty(tuple(F.work_shape(dealias)), F.float), DeviceArray.empty(tuple(F.work_shape(dealias)), F.float)
                jr, hr = ((-0.6, 0.6), (-0.6, 0.6)), np.tile([-0.6, 0.6], (6, 1))

                def composed():
                    for p in range(3):
                        F.ifftn(a.component(p), r1, dealias)
                        F.ifftn(b.component(p), r2, dealias)
                        spectral.joint_histogram(F, r1, r2, bins=NB, range=jr)
                sides = {"joint": lambda: spectral.real_joint_histogram(F, a, b, dealias, bins=NB, range=jr, reduce=False),
                         "hist": lambda: spectral.real_histogram(F, a, b, dealias, bins=NB, range=hr, reduce=False),
                         "composed": composed}
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_joint_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
                del r1, r2
            x6 = DeviceArray.random((6, n, n, n), F.float, seed=5)
            half = 3 * n ** 3 * np.dtype(F.float).itemsize
            x, y = (DeviceArray((3, n, n, n), F.float, ptr=x6.ptr + k * half, owner=False) for k in (0, 1))
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"joint": lambda: spectral.joint_histogram(F, x, y, bins=NB, range=((0.0, 1.0), (0.0, 1.0))),
                                                                 "hist": lambda: spectral.histogram(F, x6, bins=NB, range=(0.0, 1.0))})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, x6, x, y
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_joint_ab.txt"))
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
    variant = runs[0]["variant"]
    o = ["Joint histograms of spectral fields: scripts/real_joint_ab.py --procs %d --sizes=%s --lengths=%s" % (args.procs, args.sizes, args.lengths),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers and LDS: real_joint_regs.tsv.",
         "Expectation everywhere: median <= the yardstick's median + the yardstick's spread (max - min) over the processes.",
         "Several ranks and pencils are tested (tests/test_gpu_real_joint.py), not timed.", "",
         "(1) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_joint_histogram, %d x %d bins, three pairs," % (NB, NB),
         "    against real_histogram, %d bins, of the same six fields; ranges given" % NB,
         "    %-26s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "real_joint_histogram", "real_histogram", "ratio", "")]
    met = True
    for key in runs[0]["term"]:
        j = stat([r["term"][key]["wall"]["joint"] for r in runs])
        h = stat([r["term"][key]["wall"]["hist"] for r in runs])
        met = met and verdict(j, h) == "met"
        o.append("    %-26s %s  %s  %6.3f  %s (fused flag %d)" % (key, f3(j), f3(h), j[0] / h[0], verdict(j, h), runs[0]["term"][key]["flag"]))
    o.append("    expectation (1) at every size measured: %s" % ("MET" if met else "NOT MET"))
    o += ["", "(2) the fused call against its composed route, ms (per pair two FFT.ifftn into TWO real work arrays + spectral.joint_histogram, same process)",
          "    %-26s %-30s %-30s %-7s %s" % ("precision, mesh, rule", "fused", "composed", "ratio", "")]
    met = True
    for key in runs[0]["term"]:
        j = stat([r["term"][key]["wall"]["joint"] for r in runs])
        c = stat([r["term"][key]["wall"]["composed"] for r in runs])
        met = met and verdict(j, c) == "met"
        o.append("    %-26s %s  %s  %6.3f  %s" % (key, f3(j), f3(c), j[0] / c[0], verdict(j, c)))
    o.append("    expectation (2) at every size measured: %s" % ("MET" if met else "NOT MET"))
    o += ["", "(3) the z stage alone, ms per call (host clock; each call allocates, launches, folds, copies back and synchronises): %d rows x 6 fields," % ROWS,
          "    %d bins per field; (a) = the shipped LDS rule (nlj_split), (b) = the histogram twin's exchange and wave build%s;" % (NB, "" if variant else " (NOT built for this run)"),
          "    wgs = workgroups of the launch, joint (a) / histogram: resident per CU x CUs",
          "    %-16s %-30s %-30s %-30s %-7s %-7s %-10s %s" % ("precision, n", "histogram stage", "joint (a) shipped rule", "joint (b) twin's exchange", "(a)/h", "(b)/h", "wgs", "")]
    met = True
    for key in runs[0]["rows"]:
        h = stat([r["rows"][key]["hist"] for r in runs])
        j = stat([r["rows"][key]["joint"] for r in runs])
        g = stat([r["rows"][key]["joint_twin"] for r in runs]) if variant else None
        met = met and verdict(j, h) == "met"
        faster = "" if not g else ("; (a) faster" if j[0] < g[0] - (g[2] - g[1]) else "; (b) faster" if g[0] < j[0] - (j[2] - j[1]) else "; (a), (b) level")
        o.append("    %-16s %s  %s  %s  %6.3f  %s  %-10s %s%s" % (key, f3(h), f3(j), f3(g) if g else "%-30s" % "-", j[0] / h[0], "%6.3f" % (g[0] / h[0]) if g else "     -",
                                                                  "%d / %d" % (runs[0]["rows"][key]["groups"], runs[0]["rows"][key]["hist_groups"]), verdict(j, h), faster))
    o.append("    marginals of the joint stage bitwise equal to the histogram stage's counts: %d of %d cases (observed, not a contract)"
             % (sum(all(r["rows"][k]["marginals_equal"] for r in runs) for k in runs[0]["rows"]), len(runs[0]["rows"])))
    o.append("    expectation (3), the shipped build against the histogram stage, at every case measured: %s" % ("MET" if met else "NOT MET"))
    o += ["", "(4) the sweep, ms: spectral.joint_histogram of two (3, n, n, n) real arrays (%d x %d bins) against spectral.histogram of the same bytes as one" % (NB, NB),
          "    (6, n, n, n) array (%d bins); ranges given" % NB,
          "    %-16s %-30s %-30s %-7s %s" % ("precision, n", "joint_histogram", "histogram", "ratio", "")]
    met = True
    for key in runs[0]["sweep"]:
        j, h = stat([r["sweep"][key]["joint"] for r in runs]), stat([r["sweep"][key]["hist"] for r in runs])
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
