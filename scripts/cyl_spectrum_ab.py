#!/usr/bin/env python3
"""A/B of the (k_perp, k_z) sums (spectral.cyl_sums, mfft_ew_cyl_sums; csrc/cylspec.hip) on one GPU against the shell-binned sums
(spectral.shell_sums, mfft_ew_shell_sums; csrc/shells.hip) over the same fields in the same process, written to
profiles/cyl_spectrum_ab.txt by the protocol of profiles/shell_spectrum_ab.txt:

  cyl_sums(s)       (one scalar field, b == a: read once)            against   shell_sums(s)
  cyl_sums(U, N)    (three components of two fields)                 against   shell_sums(U, N)

at 512^3 and 1024^3 in double and single precision, compact spectra, one rank, slab.  Both calls synchronise the plan's stream and
copy their result to the host (nperp x npar doubles against nshell), so the host clock around a window of calls is the time.  Both
sides run in the same process, alternating, every shape warmed up first, each window at least half a second; the whole thing in
several fresh processes.  The expectation per line: the cylindrical sums' median over the processes is not slower than the
yardstick's by more than the yardstick's own spread ACROSS the processes, (max - min) / median of its per-process medians.

    python scripts/cyl_spectrum_ab.py [--procs 3] [--out profiles/cyl_spectrum_ab.txt] [--cases 512:double,512:single,1024:double,1024:single]

--segs 64,128,256,512 adds, in ONE further process and at the largest double-precision case, the time of cyl_sums(U, N) for
each of these segment lengths (the values MFFT_CYL_SEG_ROWS was chosen among), alternating."""
import argparse
import ctypes
import json
import os
import re
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


def default_seg():
    txt = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    return int(re.search(r"#define MFFT_CYL_SEG_ROWS (\d+)", txt).group(1))


def worker(cases, segs):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    L = np.array([2 * np.pi] * 3)
    res = {}
    for n, prec in cases:
        F = Slab_R2C(np.array([n, n, n]), L, SelfComm(0), prec)
        K = spectral.Wavenumbers(F)
        cs = tuple(F.complex_shape())
        U = DeviceArray.random((3,) + cs, F.complex, seed=1)
        N = DeviceArray.random((3,) + cs, F.complex, seed=2)
        s = U.component(0)
        # the same numbers binned two ways: the totals agree (random numbers on every stored mode)
        for a, b in ((s, None), (U, N)):
            R, S = spectral.cyl_sums(F, K, a, b), spectral.shell_sums(F, K, a, b)
            scale = spectral.shell_sums(F, K, a).sum() if b is None else np.sqrt(spectral.shell_sums(F, K, a).sum() * spectral.shell_sums(F, K, b).sum())
            assert R.shape == (K.nperp, K.npar) and np.all(np.isfinite(R)) and abs(R.sum() - S.sum()) <= 1e-9 * scale, (R.sum(), S.sum(), scale)
        nseg = int(sum(-(-int(c) // default_seg()) for c in np.diff(K.perp_start)))
        if segs:
            w = _alternate({"seg %d" % g: (lambda g=g: spectral.cyl_sums(F, K, U, N, seg_rows=g)) for g in segs})
            res["%d %s" % (n, prec)] = dict(segs=w, bytes=U.nbytes)
        else:
            w = _alternate({"cyl1": lambda: spectral.cyl_sums(F, K, s),
                            "shell1": lambda: spectral.shell_sums(F, K, s),
                            "cyl6": lambda: spectral.cyl_sums(F, K, U, N),
                            "shell6": lambda: spectral.shell_sums(F, K, U, N)})
            res["%d %s" % (n, prec)] = dict(windows=w, bytes=U.nbytes, nperp=K.nperp, npar=K.npar, nshell=K.nshell,
                                            part_bytes=8 * (nseg * cs[2] + K.nperp * K.npar), nseg=nseg)
        del U, N, s, F, K
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(args, extra):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + extra, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not lines:       # a process that failed is the end of the run: nothing more is started on the device
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("worker failed (rc %d)" % r.returncode)
    return json.loads(lines[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyl_spectrum_ab.txt"))
    ap.add_argument("--cases", default="512:double,512:single,1024:double,1024:single")
    ap.add_argument("--segs", default="")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    cases = [(int(c.split(":")[0]), c.split(":")[1]) for c in args.cases.split(",") if c]
    segs = [int(g) for g in args.segs.split(",") if g]
    if args.worker:
        return worker(cases, segs)
    runs = []
    for p in range(args.procs):
        runs.append(run_worker(args, ["--cases", args.cases]))
        print("process %d done" % p, flush=True)
    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["(k_perp, k_z) sums against the shell-binned sums over the same fields: scripts/cyl_spectrum_ab.py --procs %d --cases %s" % (args.procs, args.cases),
         "%s; one rank, slab, compact spectra of random numbers; %d fresh processes, in each %d alternating rounds of windows >= %.1f s"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per side after a warm-up; host clock around synchronous calls, the copy of the result to the host included.  Per process: median of",
         "its windows; GB/s of algorithmic bytes (every component of every field read once) and their share of %.0f GB/s.  Per line: the" % PEAK_GBS,
         "medians over the processes, spread = (max - min) / median of the yardstick's per-process medians.  Met: the cylindrical sums'",
         "median is not slower than the yardstick's by more than that spread.  MFFT_CYL_SEG_ROWS = %d.  Several ranks and the pencil" % default_seg(),
         "layouts were not timed.", ""]
    for key in runs[0]:
        r0 = runs[0][key]
        o.append("%s: %d x %d bins against %d shells; %d segments, %.1f MB of partial rows and result in the plan's buffer"
                 % (key, r0["nperp"], r0["npar"], r0["nshell"], r0["nseg"], r0["part_bytes"] / 1e6))
        for cyl, yard, frac, what in (("cyl1", "shell1", 1.0 / 3.0, "cyl_sums(s) against shell_sums(s), one scalar field"),
                                      ("cyl6", "shell6", 2.0, "cyl_sums(U, N) against shell_sums(U, N), three components of two fields")):
            gb = frac * r0["bytes"] / 1e9
            o.append("  %s, %.2f GB" % (what, gb))
            cm, ym = [], []
            for p, r in enumerate(runs):
                c, y = statistics.median(r[key]["windows"][cyl]), statistics.median(r[key]["windows"][yard])
                cm.append(c)
                ym.append(y)
                o.append("     process %d   cyl sums %8.3f ms  %6.0f GB/s  %4.1f %%   |  shell sums %8.3f ms  %6.0f GB/s  %4.1f %%   |  ratio %5.3f"
                         % (p, c, gb / (c * 1e-3), 100 * gb / (c * 1e-3) / PEAK_GBS, y, gb / (y * 1e-3), 100 * gb / (y * 1e-3) / PEAK_GBS, c / y))
            c, y = statistics.median(cm), statistics.median(ym)
            spread = (max(ym) - min(ym)) / y
            o.append("     medians     cyl sums %8.3f ms  %6.0f GB/s  |  shell sums %8.3f ms  %6.0f GB/s  spread %4.1f %%  |  ratio %5.3f  %s"
                     % (c, gb / (c * 1e-3), y, gb / (y * 1e-3), 100 * spread, c / y, "met" if c <= y * (1 + spread) else "NOT met"))
        o.append("")
    if segs:
        big = [c for c in cases if c[1] == "double"] or cases
        n, prec = max(big)
        r = run_worker(args, ["--cases", "%d:%s" % (n, prec), "--segs", args.segs])["%d %s" % (n, prec)]
        o.append("Segment length, %d %s, cyl_sums(U, N), one further process, alternating windows: median ms (min .. max)" % (n, prec))
        for g in segs:
            w = r["segs"]["seg %d" % g]
            o.append("   seg_rows %5d   %8.3f ms  (%.3f .. %.3f)" % (g, statistics.median(w), min(w), max(w)))
        o.append("")
    text = "\n".join(o)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
