"""CPU: the pieces of the split-last route "x near" (csrc/plan_slab.hip) that need no device.

The launch-index -> slot map of the pair-row kernels (csrc/fft_kernels.h pair_slot) is a bijection for every n0, n1 <= 20 and
G in {1, 2, 3, 4, 8, 16, 32}, with ky or kx fastest inside a tile (and the row order for G = 0), and the pair kernels with tiled order
on the transposed work array W_T meet the long-double reference of csrc/emu/test_row.h -- emulator group `pairslot`.  The layout
arithmetic of both work arrays, the plain W and W_T (one y row per block): every element inside its buffer, no two on one address."""
import re

import pytest

from emu_util import run_group
from test_gpu_split_last_blocked import _rule, layout_problems

MESHES = [[2, 2, 64], [5, 3, 256], [9, 15, 64], [12, 20, 64], [16, 32, 64], [32, 16, 2048], [34, 18, 64]]


def _id(v):
    return "x".join(str(i) for i in v)


def test_slot_map_is_a_bijection():
    r = run_group("pairslot")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("pair_slot bijection")]
    for order in (False, True):      # ky fastest inside a tile, kx fastest
        mine = [l for l in lines if (" xfast" in l) == order]
        assert sorted(int(re.search(r"G=(\d+)", l).group(1)) for l in mine) == [0, 1, 2, 3, 4, 8, 16, 32], mine
        assert all(l.rstrip().endswith("ok") for l in mine), mine


def test_pair_kernels_tiled_on_the_transposed_array():
    r = run_group("pairslot")
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if re.match(r"(r2c|c2r) pair ", l)]
    tiled_t = [l for l in lines if re.search(r" b1 g[1-9]", l)]
    assert len(tiled_t) >= 20 and all(l.rstrip().endswith("ok") for l in lines), lines
    assert any(l.startswith("r2c") and "34x18 b1 g4" in l for l in tiled_t)      # partial edge tiles in both directions
    assert any(l.startswith("c2r") and "34x18 b1 g4" in l for l in tiled_t)
    assert any(l.startswith("r2c") and "34x18 b1 g4x" in l for l in tiled_t)      # ... and kx fastest inside the tiles
    assert any(l.startswith("c2r") and "34x18 b1 g4x" in l for l in tiled_t)
    assert any("single" in l for l in tiled_t) and any("N=1024 " in l for l in tiled_t) and any("N=2048 " in l for l in tiled_t)


@pytest.mark.parametrize("N", MESHES, ids=_id)
def test_layout_arithmetic_of_both_arrays(N):
    for block in (N[1], 1):      # the plain array W, the transposed array W_T
        B, SR, SB = _rule(N, block)
        assert B == block
        need = N[1] // B * SB * 16
        assert layout_problems(N, B, SR, SB, need) == []
        assert layout_problems(N, B, SR, SB, need - 16) != []      # one element short: the check notices
    _, SR, SB = _rule(N, 1)
    assert "two elements on one address" in layout_problems(N, 1, SR, N[0] * SR - 8, 1 << 40)      # blocks that overlap: noticed


def test_layout_arithmetic_1024_cubed():
    """The mesh the route is made for: W with its planes 16 KiB further apart, W_T with rows of 8 KiB and blocks of 8 MiB + one
    line; each a compact array plus pads of at most a line per block or 16 KiB per plane."""
    N = [1024, 1024, 1024]
    compact = 1024 * 1024 * 512 * 16
    SRp = 1024 * 512 + 16384 // 16
    assert layout_problems(N, 1024, SRp, 1024 * SRp, 1024 * SRp * 16, exhaustive=False) == []
    assert 1024 * SRp * 16 <= compact + 1024 * 16384
    B, SR, SB = _rule(N, 1)
    assert (B, SR, SB) == (1, 512, 1024 * 512 + 8)
    assert layout_problems(N, 1, SR, SB, 1024 * SB * 16, exhaustive=False) == []
    assert 1024 * SB * 16 <= compact + 1024 * 128
