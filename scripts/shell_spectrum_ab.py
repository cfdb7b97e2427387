#!/usr/bin/env python3
"""A/B of the shell-binned sums (spectral.shell_sums, mfft_ew_shell_sums; csrc/shells.hip) on one GPU against the
library's plain streaming reduction over the same bytes (spectral.sumsq, mfft_ew_sumsq), written to
profiles/shell_spectrum_ab.txt:

  energy_spectrum(U_hat)             (b == a: three components read once)    against   one sumsq sweep over U_hat
  transfer_spectrum(U_hat, N_hat)    (two fields, twice the bytes)           against   two sumsq sweeps, U_hat and N_hat

at 512^3 and 1024^3 in double and 1024^3 in single precision, compact spectra, one rank, slab.  Both calls synchronise the
plan's stream, so the host clock around a window of calls is the time.  Both sides run in the same process, alternating,
every shape warmed up first, each window at least half a second; the whole thing in several fresh processes.  The yardstick's
own spread -- (max - min) / median over its windows in that process -- is what a difference has to exceed.

    python scripts/shell_spectrum_ab.py [--procs 3] [--out profiles/shell_spectrum_ab.txt] [--cases 512:double,1024:double,1024:single]

The profiler's view of the same kernels is appended to that file from two further runs of the worker under rocprofv3, the
counters in a run of their own (scripts/reproduce_profiles.sh shell_spectrum_ab.txt):

    python scripts/shell_spectrum_ab.py --out FILE --append-profiles TRACE_DIR PMC_DIR"""
import argparse
import collections
import csv
import ctypes
import glob
import re
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_S = 0.5
ROUNDS = 3
PEAK_GBS = 8000.0          # HBM3E of one MI355X


def _window(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def _alternate(sides):
    reps = {}
    for name, fn in sides.items():
        _window(fn, 2)
        reps[name] = max(3, int(1e3 * WINDOW_S / max(_window(fn, 3), 1e-3)) + 1)
    out = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            out[name].append(_window(fn, reps[name]))
    return out


def worker(cases):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    L = np.array([2 * np.pi] * 3)
    res = {}
    for n, prec in cases:
        F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
        K = spectral.Wavenumbers(F)
        cs = tuple(F.complex_shape())
        U = DeviceArray.random((3,) + cs, F.complex, seed=1)
        N = DeviceArray.random((3,) + cs, F.complex, seed=2)
        want = spectral.sumsq(F, U)
        got = spectral.shell_sums(F, K, U)                 # with random numbers on every stored mode, weights 1 and 2
        assert got.shape == (K.nshell,) and np.all(np.isfinite(got)) and want < got.sum() < 2 * want, (got.sum(), want)
        w = _alternate({"energy": lambda: spectral.energy_spectrum(F, K, U),
                        "sumsq": lambda: spectral.sumsq(F, U),
                        "transfer": lambda: spectral.transfer_spectrum(F, K, U, N),
                        "sumsq2": lambda: (spectral.sumsq(F, U), spectral.sumsq(F, N))})
        res["%d %s" % (n, prec)] = dict(windows=w, bytes=U.nbytes, nshell=K.nshell)
        del U, N, F, K
    print("RESULT " + json.dumps(res), flush=True)


KERNELS = re.compile(r"(shell_kernel<[^>]*>|shell_sum_kernel|sumsq_kernel<\w+>)")


def append_profiles(out, trace_dir, pmc_dir):
    """The kernels' lines of `rocprofv3 --kernel-trace --stats` and the per-launch means of the counters of
    `rocprofv3 --pmc ...`, both written with --output-format csv, appended to `out`."""
    o = ["", "rocprofv3 --kernel-trace --stats -- python scripts/shell_spectrum_ab.py --worker --cases 512:double,1024:double,1024:single",
         "(every launch of the A/B windows of one process, the three meshes of a precision together: calls, ns)", ""]
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            m = KERNELS.search(r["Name"])
            if m:
                o.append("   %-36s calls %6s   average %12.0f   min %10s   max %10s   %5s %% of the run's kernel time"
                         % (m.group(1), r["Calls"], float(r["AverageNs"]), r["MinNs"], r["MaxNs"], r["Percentage"]))
    o += ["", "rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -- python scripts/shell_spectrum_ab.py --worker --cases 512:double",
          "(a run of its own; mean per launch, and the share of the LDS cycles that are bank conflicts)", ""]
    tot, cnt = collections.defaultdict(float), collections.Counter()
    for f in sorted(glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            m = KERNELS.search(r["Kernel_Name"])
            if m:
                tot[(m.group(1), r["Counter_Name"])] += float(r["Counter_Value"])
                cnt[(m.group(1), r["Counter_Name"])] += 1
    for k in sorted({k for k, _ in tot}):
        conf, act = (tot[(k, c)] / max(cnt[(k, c)], 1) for c in ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"))
        o.append("   %-36s launches %6d   SQ_LDS_BANK_CONFLICT %.4e   SQ_LDS_IDX_ACTIVE %.4e   %.2f %%"
                 % (k, cnt[(k, "SQ_LDS_IDX_ACTIVE")], conf, act, 100 * conf / max(act, 1.0)))
    with open(out, "a") as f:
        f.write("\n".join(o) + "\n")
    print("\n".join(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shell_spectrum_ab.txt"))
    ap.add_argument("--cases", default="512:double,1024:double,1024:single")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--append-profiles", nargs=2, metavar=("TRACE_DIR", "PMC_DIR"))
    args = ap.parse_args()
    if args.append_profiles:
        return append_profiles(args.out, *args.append_profiles)
    cases = [(int(c.split(":")[0]), c.split(":")[1]) for c in args.cases.split(",") if c]
    if args.worker:
        return worker(cases)
    runs = []
    for p in range(args.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--cases", args.cases], capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:       # a process that failed is the end of the run: nothing more is started on the device
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("worker %d failed (rc %d)" % (p, r.returncode))
        runs.append(json.loads(lines[0][7:]))
        print("process %d done" % p, flush=True)

    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["Shell-binned sums against the plain streaming reduction over the same bytes: scripts/shell_spectrum_ab.py --procs %d --cases %s" % (args.procs, args.cases),
         "%s; one rank, slab, compact spectra of random numbers; %d fresh processes, in each %d alternating rounds of windows >= %.1f s"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per side after a warm-up; host clock around synchronous calls.  Per process: median of its windows; GB/s of algorithmic bytes",
         "(every component of every field read once) and their share of %.0f GB/s; spread = (max - min) / median of the yardstick's windows" % PEAK_GBS,
         "in that process.  Met: the shell sums' median is not slower than the yardstick's by more than that spread.",
         "Several ranks and the pencil layouts were not timed.", ""]
    for key in runs[0]:
        for shell, yard, mult, what in (("energy", "sumsq", 1, "energy_spectrum(U) against sumsq(U)"),
                                        ("transfer", "sumsq2", 2, "transfer_spectrum(U, N) against sumsq(U) + sumsq(N)")):
            o.append("%s, %d shells: %s, %.2f GB" % (key, runs[0][key]["nshell"], what, mult * runs[0][key]["bytes"] / 1e9))
            for p, r in enumerate(runs):
                w = r[key]["windows"]
                gb = mult * r[key]["bytes"] / 1e9
                s, y = statistics.median(w[shell]), statistics.median(w[yard])
                spread = (max(w[yard]) - min(w[yard])) / y
                o.append("   process %d   shell sums %8.3f ms  %6.0f GB/s  %4.1f %%   |  sumsq %8.3f ms  %6.0f GB/s  %4.1f %%  spread %4.1f %%   |  ratio %5.3f  %s"
                         % (p, s, gb / (s * 1e-3), 100 * gb / (s * 1e-3) / PEAK_GBS, y, gb / (y * 1e-3), 100 * gb / (y * 1e-3) / PEAK_GBS,
                            100 * spread, s / y, "met" if s <= y * (1 + spread) else "NOT met"))
            o.append("")
    text = "\n".join(o)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
