#!/usr/bin/env python3
"""Sweep of the split-last route "x near" (csrc/plan_slab.hip) on one GPU: directions, the tile G of the pair kernels' slot order and
the block pitch of the transposed work array, against the route without it (profiles/split_last_xnear_ab.txt sections 0 and 1).

    python3 scripts/split_last_xnear_ab.py [--n 1024] [--rounds 3] [--pairs 8] [--set sweep|pads|order]

One process, the candidates one after the other, `rounds` such rounds; per candidate and round a fresh plan, 2 pairs of warm-up and
`pairs` timed pairs with the stage timers on.  Per candidate: the wall time per pair (median, min, max over the rounds), the round
trip error, the medians over the rounds of the six stage times, and whether fftn / ifftn gave the bits of the first candidate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib  # noqa: E402

KEYS = ("MFFT_SPLIT_LAST_XNEAR", "MFFT_SPLIT_LAST_PAIRBLOCK", "MFFT_SPLIT_LAST_PAIRXFAST", "MFFT_SPLIT_LAST_XNEAR_PAD", "MFFT_SPLIT_LAST_YBLOCK",
        "MFFT_SPLIT_LAST_YFIRST", "MFFT_SPLIT_LAST_PAD")


def candidates(which):
    X, G, P = "MFFT_SPLIT_LAST_XNEAR", "MFFT_SPLIT_LAST_PAIRBLOCK", "MFFT_SPLIT_LAST_XNEAR_PAD"
    if which == "sweep":
        out = [("default (no W_T)", {X: "0"}),
               ("B1 yfirst, one array", {X: "0", "MFFT_SPLIT_LAST_YBLOCK": "1", "MFFT_SPLIT_LAST_YFIRST": "1"}),
               ("default, G16", {X: "0", G: "16"})]
        out += [("xnear both G%d" % g, {X: "1", G: str(g)}) for g in (0, 8, 16, 32)]
        # one direction alone, G by rule (tiles where the z pass runs on W_T, row order on W)
        out += [("xnear fwd  G rule", {X: "2"}), ("xnear inv  G rule", {X: "3"})]
        return out
    if which == "order":      # which index runs fastest inside a tile: ky (0), kx in the forward (1), the inverse (2), both z passes (3)
        return [("default (no W_T)", {X: "0"})] + [("xnear both G%d xfast%d" % (g, m), {X: "1", G: str(g), "MFFT_SPLIT_LAST_PAIRXFAST": str(m)})
                                                   for g in (16, 32) for m in (0, 1, 2, 3)]
    return [("default (no W_T)", {X: "0"})] + [("xnear both G16 pad%d" % p, {X: "1", G: "16", P: str(p)})
                                               for p in (0, 128, 4096, 16384, 65536 + 128)]


def run(N, env, pairs, u, fu, u2):
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    F = Slab_R2C(np.array(N), np.array([2 * np.pi] * 3), SelfComm(0), "double")
    F.enable_timing(True)
    for _ in range(2):
        F.fftn(u, fu)
        F.ifftn(fu, u2)
    F.sync()
    _lib.call("mfft_device_sync")
    F.reset_timing()
    t0 = time.perf_counter()
    for _ in range(pairs):
        F.fftn(u, fu)
        F.ifftn(fu, u2)
    F.sync()
    _lib.call("mfft_device_sync")
    dt = (time.perf_counter() - t0) / pairs * 1e3
    st = {k: v[0] / max(v[1], 1) for k, v in F.stage_times().items()}
    info = tuple(F.plan_info(k) for k in ("split_last", "split_last_xnear", "split_last_pairblock", "split_last_yblock",
                                          "split_last_row_pitch", "split_last_xnear_block_pitch"))
    return dt, st, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--set", default="sweep", choices=["sweep", "pads", "order"])
    a = ap.parse_args()
    N = [a.n] * 3
    u = DeviceArray.random(tuple(N), np.float64, seed=1234)
    fu = DeviceArray.empty((a.n, a.n, a.n // 2 + 1), np.complex128)
    u2 = DeviceArray.empty(tuple(N), np.float64)
    cands = candidates(a.set)
    res = {name: [] for name, _ in cands}
    ref = None
    for r in range(a.rounds):
        for name, env in cands:
            dt, st, info = run(N, env, a.pairs, u, fu, u2)
            k = min(2, a.n)
            sample = (fu.leading(0, k).get(), u2.leading(0, k).get())
            if ref is None:
                ref = sample
            same = all(np.array_equal(x, y) for x, y in zip(sample, ref))
            a0 = u.leading(0, k).get()
            rt = float(np.linalg.norm((a0 - sample[1]).ravel()) / np.linalg.norm(a0.ravel()))
            res[name].append((dt, st, info, rt, same))
            print("round %d  %-28s pair %.3f ms" % (r, name, dt), flush=True)
    print("== medians of %d rounds of %d pairs, n = %d; (sl, xnear, G, B, SR, SB_T); stages fwd / bwd in ms" % (a.rounds, a.pairs, a.n))
    for name, _ in cands:
        rr = res[name]
        dts = [x[0] for x in rr]
        med = {k: statistics.median(x[1].get(k, float("nan")) for x in rr) for k in ("fwd_x", "fwd_y", "fwd_z", "bwd_x", "bwd_y", "bwd_z")}
        print("%-28s %s pair med %.3f min %.3f max %.3f rt %.1e bits %s  x %.3f/%.3f y %.3f/%.3f z %.3f/%.3f  fwd %.3f bwd %.3f" % (
            name, rr[0][2], statistics.median(dts), min(dts), max(dts), max(x[3] for x in rr),
            "same" if all(x[4] for x in rr) else "DIFFER", med["fwd_x"], med["bwd_x"], med["fwd_y"], med["bwd_y"], med["fwd_z"], med["bwd_z"],
            med["fwd_x"] + med["fwd_y"] + med["fwd_z"], med["bwd_x"] + med["bwd_y"] + med["bwd_z"]))


if __name__ == "__main__":
    main()
