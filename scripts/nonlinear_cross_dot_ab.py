#!/usr/bin/env python3
"""A/B of the fused velocity + scalar nonlinear term (spectral.cross_dot_transform, mfft_nonlinear_cross_dot) on one GPU, written
to profiles/nonlinear_cross_dot_ab.txt:

  1. cross_dot_transform against cross_transform followed by dot_transform on the same plan (the two calls a coupled loop makes
     without it) at 256^3 and 512^3, double precision, '3/2-rule' and '2/3-rule';
  2. the z kernel alone (mfft_nlz_cross_dot_rows) against mfft_nlz_rows + mfft_nlz_dot_rows on the same rows at M = 512, 768, 1024,
     1536, in ms per launch and GB/s of algorithmic bytes (13 against 9 + 7 = 16 rows of `valid` bins per (x, y) point).

Both sides of a pair run in the same process on the same build, alternating, every shape warmed up first, each window at
least half a second of device time; the whole thing in several fresh processes (the x-pass rate of this card differs from
process to process: profiles/r02_run_to_run_spread.txt), medians and the spread over the processes reported.

    python scripts/nonlinear_cross_dot_ab.py [--procs 3] [--out profiles/nonlinear_cross_dot_ab.txt] [--sizes 256,512]"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from nonlinear_dot_ab import ROUNDS, ROWS, WINDOW_S, _alternate, _events, _wall  # noqa: E402  (the protocol is that script's)

KEY = {"3/2-rule": "nonlinear_cross_dot_fused_3_2", "2/3-rule": "nonlinear_cross_dot_fused_2_3"}


def worker(sizes):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"transform": {}, "rows": {}}
    L = np.array([2 * np.pi] * 3)
    for n in sizes:
        N = np.array([n, n, n])
        F = Slab_R2C(N, L, SelfComm(0), "double")
        a, b, c = F.empty_complex(3), F.empty_complex(3), F.empty_complex(3)
        for s, x in enumerate((a, b, c)):
            for i in range(3):
                F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=100 + 3 * s + i), x.component(i))
        out, sc = F.empty_complex(3), F.empty_complex()
        for dealias in ("3/2-rule", "2/3-rule"):
            def one():
                spectral.cross_dot_transform(F, a, b, c, out, sc, dealias)

            def two():
                spectral.cross_transform(F, a, b, out, dealias)
                spectral.dot_transform(F, a, c, sc, dealias)

            med, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"one": one, "two": two})
            res["transform"]["%d %s" % (n, dealias)] = dict(med, fused_flag=int(F.plan_info(KEY[dealias])), reps=reps,
                                                            nonlinear_bytes=int(F.plan_info("nonlinear_bytes")))
        del F, a, b, c, out, sc
    code = _lib.precision_code("double")
    for M, valid, nrows in ROWS:
        line = 128 // 16
        pitch = (valid + line - 1) // line * line
        a = DeviceArray.random((3, nrows, pitch), np.complex128, seed=1)
        b = DeviceArray.random((3, nrows, pitch), np.complex128, seed=2)
        c = DeviceArray.random((3, nrows, pitch), np.complex128, seed=3)
        s = DeviceArray.random((nrows, pitch), np.complex128, seed=4)
        b0 = b.component(0)

        def two_launches():      # in place on the first field / out of place into a row array, as the two calls' routes run them
            _lib.call("mfft_nlz_rows", a.ptr, b.ptr, a.ptr, nrows, M, pitch, valid, code, 0)
            _lib.call("mfft_nlz_dot_rows", a.ptr, c.ptr, s.ptr, nrows, M, pitch, valid, code, 0)

        med, reps = _alternate(_events, {
            # in place on the first field and the second's first component, as the plan runs it
            "one": lambda: _lib.call("mfft_nlz_cross_dot_rows", a.ptr, b.ptr, c.ptr, a.ptr, b0.ptr, nrows, M, pitch, valid, code, 0),
            "two": two_launches})
        _lib.call("mfft_device_sync")
        gb = nrows * valid * 16 / 1e9
        res["rows"]["%d" % M] = dict(med, valid=valid, nrows=nrows, one_gbs=13 * gb / (med["one"] * 1e-3), two_gbs=16 * gb / (med["two"] * 1e-3), reps=reps)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlinear_cross_dot_ab.txt"))
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return worker(sizes)
    runs = []
    for p in range(args.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes", args.sizes], capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:       # a process that failed is the end of the run: nothing more is started on the device
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("worker %d failed (rc %d)" % (p, r.returncode))
        runs.append(json.loads(lines[0][7:]))
        print("process %d done" % p, flush=True)

    def stat(vals):
        return statistics.median(vals), min(vals), max(vals)

    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["Fused velocity + scalar nonlinear term, fftn(ifftn(a) x ifftn(b)) and fftn(sum_f ifftn(a_f) ifftn(c_f)): "
         "scripts/nonlinear_cross_dot_ab.py --procs %d --sizes %s" % (args.procs, args.sizes),
         "%s; double precision; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].", "",
         "1. spectral.cross_dot_transform (one plan operation) against spectral.cross_transform + spectral.dot_transform on the same plan, ms per pair of terms",
         "   (host clock around calls that end in a synchronise of the plan's stream)",
         "   %-14s %-28s %-28s %-9s %s" % ("mesh, rule", "one operation", "two calls", "ratio", "fused flag, plan work buffers")]
    for key in runs[0]["transform"]:
        f = stat([r["transform"][key]["one"] for r in runs])
        c = stat([r["transform"][key]["two"] for r in runs])
        t = runs[0]["transform"][key]
        verdict = "one operation ahead by more than the spread" if f[2] < c[1] else ("one operation's median below" if f[0] < c[0] else "one operation's median NOT below")
        o.append("   %-14s %7.3f [%7.3f .. %7.3f]  %7.3f [%7.3f .. %7.3f]  %6.3f    %d, %.2f GB   %s"
                 % (key, f[0], f[1], f[2], c[0], c[1], c[2], f[0] / c[0], t["fused_flag"], t["nonlinear_bytes"] / 1e9, verdict))
    o += ["", "2. the z kernel alone on rows of `valid` bins (pitch: whole cache lines), ms and GB/s of algorithmic bytes; HIP events around the window",
          "   (one: mfft_nlz_cross_dot_rows, 9 rows in + 4 out = 13 rows of valid bins per (x, y) point; two: mfft_nlz_rows + mfft_nlz_dot_rows, 9 + 7 = 16)",
          "   %-6s %-6s %-8s %-28s %-28s %-8s %-22s %s" % ("M", "valid", "rows", "one launch, ms", "two launches, ms", "ratio", "one GB/s", "two GB/s")]
    for key in runs[0]["rows"]:
        d = stat([r["rows"][key]["one"] for r in runs])
        c = stat([r["rows"][key]["two"] for r in runs])
        dg = stat([r["rows"][key]["one_gbs"] for r in runs])
        cg = stat([r["rows"][key]["two_gbs"] for r in runs])
        t = runs[0]["rows"][key]
        o.append("   %-6s %-6d %-8d %7.4f [%7.4f .. %7.4f]  %7.4f [%7.4f .. %7.4f]  %6.3f   %5.0f [%5.0f .. %5.0f]  %5.0f [%5.0f .. %5.0f]"
                 % (key, t["valid"], t["nrows"], d[0], d[1], d[2], c[0], c[1], c[2], d[0] / c[0], dg[0], dg[1], dg[2], cg[0], cg[1], cg[2]))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
