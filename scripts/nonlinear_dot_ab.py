#!/usr/bin/env python3
"""A/B of the fused scalar-advection term (spectral.dot_transform, mfft_nonlinear_dot) on one GPU, written to
profiles/nonlinear_dot_ab.txt:

  1. dot_transform against the caller-side composition (six FFT.ifftn, spectral.dot, one FFT.fftn) at 256^3 and 512^3, double
     precision, '3/2-rule' and '2/3-rule';
  2. the z kernel alone (mfft_nlz_dot_rows) against the cross-product kernel (mfft_nlz_rows) on the same rows at M = 512, 768,
     1024, 1536, in GB/s of algorithmic bytes (7 against 9 rows of `valid` bins per (x, y) point).

Both sides of a pair run in the same process on the same build, alternating, every shape warmed up first, each window at
least half a second of device time; the whole thing in several fresh processes (the x-pass rate of this card differs from
process to process: profiles/r02_run_to_run_spread.txt), medians and the spread over the processes reported.

    python scripts/nonlinear_dot_ab.py [--procs 3] [--out profiles/nonlinear_dot_ab.txt] [--sizes 256,512]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(512, 257, 512 * 128), (768, 257, 768 * 96), (1024, 513, 1024 * 48), (1536, 513, 1536 * 24)]      # (M, valid, rows): scripts/nlz_bench.py's
WINDOW_S = 0.5
ROUNDS = 3


def _events(fn, reps):
    """ms per call of fn over `reps` enqueued calls, HIP events on the default stream"""
    from mpifft4py_amd import _lib
    t = ctypes.c_void_p()
    _lib.call("mfft_timer_create", ctypes.byref(t))
    _lib.call("mfft_timer_start", t)
    for _ in range(reps):
        fn()
    ms = ctypes.c_float(0)
    _lib.call("mfft_timer_stop", t, ctypes.byref(ms))
    _lib.call("mfft_timer_destroy", t)
    return ms.value / reps


def _wall(F, fn, reps):
    """ms per call: host clock around `reps` calls that end in a synchronise of the plan's stream"""
    F.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    F.sync()
    return 1e3 * (time.perf_counter() - t0) / reps


def _alternate(timer, sides):
    """sides: {name: fn}.  Warm up, size the windows, then ROUNDS rounds of one window per side, alternating."""
    reps = {}
    for name, fn in sides.items():
        timer(fn, 2)
        one = timer(fn, 3)
        reps[name] = max(3, int(1e3 * WINDOW_S / max(one, 1e-3)) + 1)
    out = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            out[name].append(timer(fn, reps[name]))
    return {name: statistics.median(v) for name, v in out.items()}, reps


def worker(sizes):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"transform": {}, "rows": {}}
    L = np.array([2 * np.pi] * 3)
    for n in sizes:
        N = np.array([n, n, n])
        F = Slab_R2C(N, L, SelfComm(0), "double")
        cs = tuple(F.complex_shape())
        a, b = F.empty_complex(3), F.empty_complex(3)
        for s, x in enumerate((a, b)):
            for i in range(3):
                F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=100 + 3 * s + i), x.component(i))
        out = DeviceArray.empty(cs, F.complex)
        for dealias in ("3/2-rule", "2/3-rule"):
            ws = tuple(F.work_shape(dealias))
            ua, ub = DeviceArray.empty((3,) + ws, F.float), DeviceArray.empty((3,) + ws, F.float)
            r = DeviceArray.empty(ws, F.float)

            def fused():
                spectral.dot_transform(F, a, b, out, dealias)

            def composed():
                for i in range(3):
                    F.ifftn(a.component(i), ua.component(i), dealias)
                    F.ifftn(b.component(i), ub.component(i), dealias)
                spectral.dot(F, ua, ub, r)
                F.fftn(r, out, None if dealias == "2/3-rule" else dealias)

            med, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"fused": fused, "composed": composed})
            key = {"3/2-rule": "nonlinear_dot_fused_3_2", "2/3-rule": "nonlinear_dot_fused_2_3"}[dealias]
            res["transform"]["%d %s" % (n, dealias)] = dict(med, fused_flag=int(F.plan_info(key)), reps=reps,
                                                            nonlinear_bytes=int(F.plan_info("nonlinear_bytes")))
            del ua, ub, r
        del F, a, b, out
    code = _lib.precision_code("double")
    for M, valid, nrows in ROWS:
        line = 128 // 16
        pitch = (valid + line - 1) // line * line
        a = DeviceArray.random((3, nrows, pitch), np.complex128, seed=1)
        b = DeviceArray.random((3, nrows, pitch), np.complex128, seed=2)
        # in place on the first field / its first component, as the plan runs them
        med, reps = _alternate(_events, {
            "dot": lambda: _lib.call("mfft_nlz_dot_rows", a.ptr, b.ptr, a.ptr, nrows, M, pitch, valid, code, 0),
            "cross": lambda: _lib.call("mfft_nlz_rows", a.ptr, b.ptr, a.ptr, nrows, M, pitch, valid, code, 0)})
        _lib.call("mfft_device_sync")
        gb = nrows * valid * 16 / 1e9
        res["rows"]["%d" % M] = dict(med, valid=valid, nrows=nrows, dot_gbs=7 * gb / (med["dot"] * 1e-3), cross_gbs=9 * gb / (med["cross"] * 1e-3), reps=reps)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlinear_dot_ab.txt"))
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
    o = ["Fused scalar-advection term, fftn(sum_f ifftn(a_f) ifftn(b_f)): scripts/nonlinear_dot_ab.py --procs %d --sizes %s" % (args.procs, args.sizes),
         "%s; double precision; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].", "",
         "1. spectral.dot_transform (one plan operation) against the caller-side composition (six ifftn, spectral.dot, one fftn), ms per term",
         "   (host clock around calls that end in a synchronise of the plan's stream)",
         "   %-14s %-28s %-28s %-9s %s" % ("mesh, rule", "fused", "composed", "ratio", "fused flag, plan work buffers")]
    for key in runs[0]["transform"]:
        f = stat([r["transform"][key]["fused"] for r in runs])
        c = stat([r["transform"][key]["composed"] for r in runs])
        t = runs[0]["transform"][key]
        verdict = "fused ahead by more than the spread" if f[2] < c[1] else "NOT separated by the spread"
        o.append("   %-14s %7.3f [%7.3f .. %7.3f]  %7.3f [%7.3f .. %7.3f]  %6.3f    %d, %.2f GB   %s"
                 % (key, f[0], f[1], f[2], c[0], c[1], c[2], f[0] / c[0], t["fused_flag"], t["nonlinear_bytes"] / 1e9, verdict))
    o += ["", "2. the z kernel alone, in place on rows of `valid` bins (pitch: whole cache lines), ms per launch and GB/s of algorithmic bytes",
          "   (dot: 6 rows in + 1 out = 7 rows of valid bins per (x, y) point; cross: 6 + 3 = 9); HIP events around the window",
          "   %-6s %-6s %-8s %-28s %-28s %-22s %s" % ("M", "valid", "rows", "dot ms", "cross ms", "dot GB/s", "cross GB/s")]
    for key in runs[0]["rows"]:
        d = stat([r["rows"][key]["dot"] for r in runs])
        c = stat([r["rows"][key]["cross"] for r in runs])
        dg = stat([r["rows"][key]["dot_gbs"] for r in runs])
        cg = stat([r["rows"][key]["cross_gbs"] for r in runs])
        t = runs[0]["rows"][key]
        o.append("   %-6s %-6d %-8d %7.4f [%7.4f .. %7.4f]  %7.4f [%7.4f .. %7.4f]  %5.0f [%5.0f .. %5.0f]  %5.0f [%5.0f .. %5.0f]"
                 % (key, t["valid"], t["nrows"], d[0], d[1], d[2], c[0], c[1], c[2], dg[0], dg[1], dg[2], cg[0], cg[1], cg[2]))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
