#!/usr/bin/env python3
"""What the plane-averaged profiles of spectral fields cost (spectral.real_profiles) on one GPU, written to
profiles/real_profiles_ab.txt:

  (1) the whole call: spectral.real_profiles on three pairs against spectral.real_moments on the same six fields, 256^3 and
      512^3, both precisions, '3/2-rule' and '2/3-rule'.  Both run the same transforms and loads; the profiles body adds five
      sums per point and pair where the moments body adds twelve statistics, and stores and folds one partial profile per row
      slot of the launch.  Expectation: no slower than the moments call plus that yardstick's own spread over the processes;
  (2) the fused call against its composed route: per pair two FFT.ifftn(.., dealias) into TWO real work arrays and one
      spectral.profiles sweep of them -- the calls the plan's composed route makes (plan_nonlinear.hip reduce_composed), issued
      from the same process, because MFFT_NO_NLZ is read once per process and the two sides have to alternate.  Expectation: no
      slower than the composed route plus its spread;
  (3) the z stage alone: mfft_nlz_profile_rows against mfft_nlz_moments_rows on the same rows (36864 rows x 6 fields), both
      precisions.  Expectation: no slower than the moments stage plus its spread;
  (4) the sweep: spectral.profiles of two (3, n, n, n) real arrays against spectral.moments of one (6, n, n, n) array over the
      same bytes.  Expectation: no slower than the moments sweep plus its spread.
Several ranks and pencils are tested (tests/test_gpu_real_profiles.py), not timed.

Protocol of scripts/real_joint_ab.py: both sides in the same process, alternating windows of at least half a second after a
warm-up of every shape, several fresh processes, medians and the spread over the processes.

    python scripts/real_profiles_ab.py [--procs 3] [--out profiles/real_profiles_ab.txt] [--sizes 256,512] [--lengths ...]"""
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
from real_joint_ab import ROWS, _rows  # noqa: E402

LENGTHS = (512, 768, 1024, 1536, 3072)      # 8-values plans (512, 1024) and 12-values plans (768, 1536, 3072: 60 doubles of accumulators)
DP = ctypes.POINTER(ctypes.c_double)


def worker(sizes, lengths):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"rows": {}, "term": {}, "sweep": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in ("double", "single"):
        code = _lib.precision_code(prec)
        for n in lengths:
            a, b = _rows(DeviceArray, n, prec, 1), _rows(DeviceArray, n, prec, 2)
            valid = n // 2 + 1
            mom, prof = np.zeros(36), np.zeros((3, 5, n))
            sides = {"moments": lambda: _lib.call("mfft_nlz_moments_rows", a.ptr, b.ptr, 6, ROWS, n, valid, valid, 0, code, None, mom.ctypes.data_as(DP)),
                     "profiles": lambda: _lib.call("mfft_nlz_profile_rows", a.ptr, b.ptr, 3, ROWS, n, valid, valid, 0, code, None, prof.ctypes.data_as(DP))}
            t, reps = _alternate(_host_wall, sides)
            assert np.all(np.isfinite(prof)) and np.all(prof[:, 2:4] > 0)
            res["rows"]["%s %d" % (prec, n)] = dict(t, reps=reps, groups=int(_lib.call("mfft_nlz_profile_groups", ROWS, n, code)),
                                                    moments_groups=int(_lib.call("mfft_nlz_moments_groups", ROWS, n, code)))
            del a, b
        for n in sizes:
            F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
            a, b = _fields(F)
            for dealias in ("3/2-rule", "2/3-rule"):
                r1, r2 = DeviceArray.empty(tuple(F.work_shape(dealias)), F.float), DeviceArray.empty(tuple(F.work_shape(dealias)), F.float)

                def composed():
                    for p in range(3):
                        F.ifftn(a.component(p), r1, dealias)
                        F.ifftn(b.component(p), r2, dealias)
                        spectral.profiles(F, r1, r2)
                sides = {"profiles": lambda: spectral.real_profiles(F, a, b, dealias, reduce=False),
                         "moments": lambda: spectral.real_moments(F, a, b, dealias, reduce=False),
                         "composed": composed}
                wall, reps = _alternate(lambda fn, k: _wall(F, fn, k), sides)
                key = "nonlinear_profiles_fused_" + ("3_2" if dealias == "3/2-rule" else "2_3")
                res["term"]["%s %d %s" % (prec, n, dealias)] = dict(wall=wall, flag=int(F.plan_info(key)), reps=reps)
                del r1, r2
            x6 = DeviceArray.random((6, n, n, n), F.float, seed=5)
            half = 3 * n ** 3 * np.dtype(F.float).itemsize
            x, y = (DeviceArray((3, n, n, n), F.float, ptr=x6.ptr + k * half, owner=False) for k in (0, 1))
            sw, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"profiles": lambda: spectral.profiles(F, x, y), "moments": lambda: spectral.moments(F, x6)})
            res["sweep"]["%s %d" % (prec, n)] = dict(sw, reps=reps)
            del F, a, b, x6, x, y
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_profiles_ab.txt"))
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
    o = ["Plane-averaged profiles of spectral fields: scripts/real_profiles_ab.py --procs %d --sizes=%s --lengths=%s" % (args.procs, args.sizes, args.lengths),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].  Registers and LDS: real_profiles_regs.tsv.",
         "Expectation everywhere: median <= the yardstick's median + the yardstick's spread (max - min) over the processes.",
         "Several ranks and pencils are tested (tests/test_gpu_real_profiles.py), not timed.", ""]

    def section(title, head, table, mine, yard, extra=lambda key: ""):
        o.extend(title)
        o.append("    %-26s %-30s %-30s %-7s %s" % head)
        met = True
        for key in runs[0][table]:
            get = (lambda r, k: r[table][key]["wall"][k]) if table == "term" else (lambda r, k: r[table][key][k])
            j, h = stat([get(r, mine) for r in runs]), stat([get(r, yard) for r in runs])
            met = met and verdict(j, h) == "met"
            o.append("    %-26s %s  %s  %6.3f  %s%s" % (key, f3(j), f3(h), j[0] / h[0], verdict(j, h), extra(key)))
        o.append("    expectation at every case measured: %s" % ("MET" if met else "NOT MET"))
        o.append("")

    section(["(1) the whole call, ms (host clock around calls that end in a synchronise of the plan's stream): real_profiles, three pairs,",
             "    against real_moments of the same six fields"],
            ("precision, mesh, rule", "real_profiles", "real_moments", "ratio", ""), "term", "profiles", "moments",
            lambda key: " (fused flag %d)" % runs[0]["term"][key]["flag"])
    section(["(2) the fused call against its composed route, ms (per pair two FFT.ifftn into TWO real work arrays + spectral.profiles, same process)"],
            ("precision, mesh, rule", "fused", "composed", "ratio", ""), "term", "profiles", "composed")
    section(["(3) the z stage alone, ms per call (host clock; each call allocates, launches, folds, copies back and synchronises): %d rows x 6 fields;" % ROWS,
             "    wgs = workgroups of the launch, profiles / moments"],
            ("precision, n", "profiles stage", "moments stage", "ratio", ""), "rows", "profiles", "moments",
            lambda key: "  wgs %d / %d" % (runs[0]["rows"][key]["groups"], runs[0]["rows"][key]["moments_groups"]))
    section(["(4) the sweep, ms: spectral.profiles of two (3, n, n, n) real arrays against spectral.moments of the same bytes as one (6, n, n, n) array"],
            ("precision, n", "profiles", "moments", "ratio", ""), "sweep", "profiles", "moments")
    text = "\n".join(o)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
