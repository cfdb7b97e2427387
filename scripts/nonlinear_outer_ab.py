#!/usr/bin/env python3
"""A/B of the fused outer-product term (spectral.outer_transform, mfft_nonlinear_outer) on one GPU, written to
profiles/nonlinear_outer_ab.txt.  Every yardstick is existing code on the same plan in the same process; every line states its
expectation and is marked met or NOT met:

  1. outer_transform against the caller-side composition (6 FFT.ifftn, 9 spectral.mul, 9 FFT.fftn on seven real arrays) at 256^3
     and 512^3, double and single precision, '3/2-rule' and '2/3-rule'.  Expectation: no slower than the yardstick plus its spread.
  2. outer_transform against three cross_transform calls on the same spectra (u x omega, j x b, u x b: what MHD costs without it).
     Expectation: no slower than the yardstick plus its spread; the transform counts say about 15 / 27.
  3. the z kernel alone (mfft_nlz_outer_rows, in place as the routes run it) against the cross product's (mfft_nlz_rows) on the same
     rows at M = 512, 768, 1024, 1536.  By transform count the ratio would be 7.5 / 4.5; expectation: no more than that times the
     yardstick plus its spread.  The registers of both kernels (profiles/nonlinear_outer_regs.tsv) stand next to the ratio.

Protocol of scripts/nonlinear_dot_ab.py: the sides of a comparison run in the same process on the same build, alternating, every
shape warmed up first, each window at least half a second of device time; the whole thing in several fresh processes, medians
and the spread over the processes reported.

    python scripts/nonlinear_outer_ab.py [--procs 3] [--out profiles/nonlinear_outer_ab.txt] [--sizes 256,512]"""
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

KEY = {"3/2-rule": "nonlinear_outer_fused_3_2", "2/3-rule": "nonlinear_outer_fused_2_3"}
PRECS = ("double", "single")


def worker(sizes):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    res = {"transform": {}, "rows": {}}
    L = np.array([2 * np.pi] * 3)
    for prec in PRECS:
        for n in sizes:
            N = np.array([n, n, n])
            F = Slab_R2C(N, L, SelfComm(0), prec)
            a, b = F.empty_complex(3), F.empty_complex(3)
            for s, x in enumerate((a, b)):
                for i in range(3):
                    F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=100 + 3 * s + i), x.component(i))
            out, c3 = F.empty_complex(9), F.empty_complex(3)
            for dealias in ("3/2-rule", "2/3-rule"):
                ws = tuple(F.work_shape(dealias))
                ra, rb = DeviceArray.empty((3,) + ws, F.float), DeviceArray.empty((3,) + ws, F.float)
                w = DeviceArray.empty(ws, F.float)

                def one():
                    spectral.outer_transform(F, a, b, out, dealias)

                def composed():
                    for f in range(3):
                        F.ifftn(a.component(f), ra.component(f), dealias)
                        F.ifftn(b.component(f), rb.component(f), dealias)
                    for i in range(3):
                        for j in range(3):
                            spectral.mul(F, ra.component(i), rb.component(j), w)
                            F.fftn(w, out.component(3 * i + j), None if dealias == "2/3-rule" else dealias)

                def three():
                    for _ in range(3):
                        spectral.cross_transform(F, a, b, c3, dealias)

                med, reps = _alternate(lambda fn, k: _wall(F, fn, k), {"one": one, "composed": composed, "three": three})
                res["transform"]["%s %d %s" % (prec, n, dealias)] = dict(med, fused_flag=int(F.plan_info(KEY[dealias])), reps=reps,
                                                                         nonlinear_bytes=int(F.plan_info("nonlinear_bytes")))
                del ra, rb, w
            del F, a, b, out, c3
    for prec in PRECS:
        code = _lib.precision_code(prec)
        ct = np.complex128 if prec == "double" else np.complex64
        es = np.dtype(ct).itemsize
        for M, valid, nrows in ROWS:
            line = 128 // es
            pitch = (valid + line - 1) // line * line
            o = DeviceArray.random((9, nrows, pitch), ct, seed=1)      # a = components 0..2, b = 3..5: in place, as the routes run it
            b = o.component(3)
            med, reps = _alternate(_events, {
                "outer": lambda: _lib.call("mfft_nlz_outer_rows", o.ptr, b.ptr, o.ptr, nrows, M, pitch, valid, code, 0),
                "cross": lambda: _lib.call("mfft_nlz_rows", o.ptr, b.ptr, o.ptr, nrows, M, pitch, valid, code, 0)})
            _lib.call("mfft_device_sync")
            gb = nrows * valid * es / 1e9
            res["rows"]["%s %d" % (prec, M)] = dict(med, valid=valid, nrows=nrows, outer_gbs=15 * gb / (med["outer"] * 1e-3),
                                                    cross_gbs=9 * gb / (med["cross"] * 1e-3), reps=reps)
            del o, b
    print("RESULT " + json.dumps(res), flush=True)


def _regs():
    """(precision, M) -> 'cross vgpr/scratch, outer vgpr/scratch' from profiles/nonlinear_outer_regs.tsv"""
    out = {}
    path = os.path.join(ROOT, "profiles", "nonlinear_outer_regs.tsv")
    if not os.path.exists(path):
        return out
    for l in open(path):
        f = l.rstrip("\n").split("\t")
        if l.startswith("#") or f[0] == "precision" or len(f) < 11:
            continue
        out[("double" if f[0] == "double" else "single", int(f[1].split("=")[1]))] = "cross %s VGPRs / %s B scratch, outer %s / %s" % (f[2], f[4], f[8], f[10])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlinear_outer_ab.txt"))
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

    def verdict(ok):
        return "met" if ok else "NOT met"

    from mpifft4py_amd import _lib
    name = ctypes.create_string_buffer(256)
    _lib.call("mfft_device_name", name, 256)
    o = ["Fused outer-product term, out[3 i + j] = fftn(ifftn(a_i) ifftn(b_j)): scripts/nonlinear_outer_ab.py --procs %d --sizes %s" % (args.procs, args.sizes),
         "%s; %d fresh processes, in each %d alternating rounds of windows >= %.1f s per side after a warm-up of every shape;"
         % (name.value.decode(), args.procs, ROUNDS, WINDOW_S),
         "per process the median of its rounds; below the median over the processes [min .. max over the processes].",
         "Expectation of lines 1 and 2: the one operation's median is no more than the yardstick's median plus the yardstick's spread (max - min).", ""]
    for title, side, what in (("1. spectral.outer_transform (one plan operation) against the caller-side composition on the same plan: 6 FFT.ifftn, 9 spectral.mul, 9 FFT.fftn, seven real arrays",
                               "composed", "composition"),
                              ("2. spectral.outer_transform against three spectral.cross_transform calls on the same spectra (18 inverse + 9 forward transforms against 6 + 9: "
                               "the counts say about 15 / 27 = 0.56)", "three", "three cross calls")):
        o += [title, "   ms per call (host clock around calls that end in a synchronise of the plan's stream)",
              "   %-22s %-28s %-28s %-8s %s" % ("precision, mesh, rule", "one operation", what, "ratio", "fused flag, plan work buffers, expectation")]
        for key in runs[0]["transform"]:
            f = stat([r["transform"][key]["one"] for r in runs])
            c = stat([r["transform"][key][side] for r in runs])
            t = runs[0]["transform"][key]
            o.append("   %-22s %7.3f [%7.3f .. %7.3f]  %7.3f [%7.3f .. %7.3f]  %6.3f   %d, %.2f GB   %s"
                     % (key, f[0], f[1], f[2], c[0], c[1], c[2], f[0] / c[0], t["fused_flag"], t["nonlinear_bytes"] / 1e9, verdict(f[0] <= c[0] + (c[2] - c[1]))))
        o.append("")
    regs = _regs()
    o += ["3. the z kernel alone on rows of `valid` bins (pitch: whole cache lines), in place as the routes run it, ms and GB/s of algorithmic bytes; HIP events around the window",
          "   (outer: mfft_nlz_outer_rows, 6 rows in + 9 out = 15 rows of valid bins per (x, y) point, 7.5 transforms; cross: mfft_nlz_rows, 6 + 3 = 9 rows, 4.5 transforms)",
          "   Expectation: outer / cross no more than 7.5 / 4.5 = 1.667 of the yardstick's median plus its spread.",
          "   %-16s %-6s %-8s %-28s %-28s %-7s %-8s %-8s %s" % ("precision, M", "valid", "rows", "outer, ms", "cross, ms", "ratio", "outer GB/s", "cross GB/s", "expectation; registers")]
    for key in runs[0]["rows"]:
        d = stat([r["rows"][key]["outer"] for r in runs])
        c = stat([r["rows"][key]["cross"] for r in runs])
        dg = stat([r["rows"][key]["outer_gbs"] for r in runs])
        cg = stat([r["rows"][key]["cross_gbs"] for r in runs])
        t = runs[0]["rows"][key]
        prec, M = key.split()
        o.append("   %-16s %-6d %-8d %7.4f [%7.4f .. %7.4f]  %7.4f [%7.4f .. %7.4f]  %6.3f  %5.0f      %5.0f      %s; %s"
                 % (key, t["valid"], t["nrows"], d[0], d[1], d[2], c[0], c[1], c[2], d[0] / c[0], dg[0], cg[0],
                    verdict(d[0] <= 7.5 / 4.5 * (c[0] + (c[2] - c[1]))), regs.get((prec, int(M)), "registers: see profiles/nonlinear_outer_regs.tsv")))
    text = "\n".join(o) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
