"""CPU: the device-free half of the shell spectra (spectral.shell_sums): `_mesh.Block.shell_of` against the exact integer
rule, the shell count, the int32 mode vectors and the Hermitian weights of every rank's block of slab and pencil layouts
(built on a LayoutComm: no device, no plan), and -- numpy only -- that the weighted half-spectrum sums of a real field are
the full-spectrum sums.  The reference is plain numpy and integer arithmetic written here, never the helpers under test."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mpifft4py_amd import LayoutComm, Pencil_R2C, Slab_C2C, Slab_R2C
from mpifft4py_amd._mesh import Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.array([2 * np.pi] * 3)
TOL = 1e-10                                  # gpu_util.TOL["double"]
MESHES = [(16, 12, 20), (12, 10, 9), (7, 9, 15), (8, 16, 6)]


def exact_shell(m):
    """The unique integer s with |sqrt(m) - s| <= 1/2, in exact integers: (2s-1)^2 <= 4m < (2s+1)^2 (no integer m lies on
    a boundary: (2s+1)^2 is odd), 0 for m = 0."""
    m = int(m)
    if m == 0:
        return 0
    s = math.isqrt(m)                        # floor(sqrt(m)) exactly
    if 4 * m >= (2 * s + 1) ** 2:
        s += 1
    assert (2 * s - 1) ** 2 <= 4 * m < (2 * s + 1) ** 2 and s >= 1
    return s


def full_modes(n):
    k = np.arange(n, dtype=np.int64)
    k[(n + 1) // 2:] -= n                    # the Nyquist mode of an even axis is -n/2
    return k


def global_half_tables(N):
    """(shell, weight) of every mode of the rfftn layout (N0, N1, N2//2 + 1), from integers alone."""
    k0, k1, k2 = full_modes(N[0]), full_modes(N[1]), np.arange(N[2] // 2 + 1, dtype=np.int64)
    m = k0[:, None, None] ** 2 + k1[None, :, None] ** 2 + k2[None, None, :] ** 2
    sh = np.vectorize(exact_shell, otypes=[np.int64])(m)
    h = np.full(len(k2), 2, dtype=np.int64)
    h[0] = 1
    if N[2] % 2 == 0:
        h[-1] = 1
    return sh, h


def one_rank_half_block(N):
    """A one-rank block of the real transform's layout, odd N2 included (the R2C plans themselves take even N2 only)."""
    nf = N[2] // 2 + 1
    return Block(N, L, [(0, N[0]), (0, N[1]), (0, N[2])], [(0, N[0]), (0, N[1]), (0, nf)], 2)


def blocks_of(kind, N):
    N = np.array(N)
    if kind == "slab1":
        return [Slab_R2C(N, L, LayoutComm(1, 0), "double")._mesh]
    if kind == "slab4":
        return [Slab_R2C(N, L, LayoutComm(4, r), "double")._mesh for r in range(4)]
    if kind == "c2c1":
        return [Slab_C2C(N, L, LayoutComm(1, 0), "double")._mesh]
    return [Pencil_R2C(N, L, LayoutComm(4, r), "double", P1=2, alignment=kind[-1])._mesh for r in range(4)]


def test_shell_of_matches_the_exact_rule_everywhere():
    top = 3 * 1024 ** 2
    got = Block.shell_of(np.arange(top + 1, dtype=np.int64))
    want = np.zeros(top + 1, dtype=np.int64)
    s = 1
    while (2 * s - 1) ** 2 <= 4 * top:                       # shell s holds ceil((2s-1)^2 / 4) .. floor(((2s+1)^2 - 1) / 4)
        lo, hi = ((2 * s - 1) ** 2 + 3) // 4, ((2 * s + 1) ** 2 - 1) // 4
        want[lo:min(hi, top) + 1] = s
        s += 1
    assert got.dtype.kind == "i" and np.array_equal(got, want)
    for m in (0, 1, 2, 3, 4, 6, 7, 12, 13, top):
        assert int(Block.shell_of(m)) == exact_shell(m) == want[m]
    for s in range(1, 1774):                                  # the boundary values m = s^2 +- s: sqrt(m) ~ s +- 1/2
        for m, t in ((s * s - s, s - 1 if s > 1 else 0), (s * s - s + 1, s), (s * s + s, s), (s * s + s + 1, s + 1)):
            if m <= top:
                assert exact_shell(m) == t and int(Block.shell_of(m)) == t, (s, m)
    assert int(Block.shell_of(0)) == 0 and int(Block.shell_of(np.int64(1))) == 1


LAYOUTS = [("slab1", (16, 12, 20)), ("slab1", (8, 16, 6)), ("slab1", (32, 64, 128)), ("slab4", (16, 12, 20)), ("slab4", (8, 16, 6)),
           ("slab4", (12, 8, 10)), ("pencilX", (16, 12, 20)), ("pencilY", (16, 12, 20)), ("pencilX", (8, 16, 12)),
           ("pencilY", (8, 16, 12))]


@pytest.mark.parametrize("kind,N", LAYOUTS)
def test_block_vectors_of_every_rank(kind, N):
    """The blocks' vectors tile the global tables exactly: every mode is binned once, with the weight the rfftn layout needs."""
    sh, h = global_half_tables(N)
    nshell = exact_shell(sum((n // 2) ** 2 for n in N)) + 1
    seen = np.zeros(sh.shape, dtype=np.int64)
    for b in blocks_of(kind, N):
        assert b.shell_count() == nshell
        iv, w = b.shell_index_vectors(), b.hermitian_weights()
        assert len(iv) == 3 and all(v.dtype == np.int32 and v.flags["C_CONTIGUOUS"] for v in iv) and w.dtype == np.uint8
        assert tuple(len(v) for v in iv) == b.spectral_shape() and len(w) == b.spectral_shape()[2]
        sl = tuple(slice(s, s + l) for s, l in b.spectral_window)
        m = iv[0].astype(np.int64)[:, None, None] ** 2 + iv[1].astype(np.int64)[None, :, None] ** 2 + iv[2].astype(np.int64)[None, None, :] ** 2
        assert np.array_equal(Block.shell_of(m), sh[sl])
        assert np.array_equal(w.astype(np.int64), h[sl[2]])
        seen[sl] += 1
    assert np.all(seen == 1)
    assert sh.max() == nshell - 1                            # the corner mode (N0//2, N1//2, N2//2) is stored


@pytest.mark.parametrize("N", MESHES)
def test_one_rank_half_blocks_even_and_odd(N):
    """Even and odd N2 through a hand-built block of the rfftn layout, and the complex plans' full layout (weights 1)."""
    sh, h = global_half_tables(N)
    b = one_rank_half_block(N)
    iv, w = b.shell_index_vectors(), b.hermitian_weights()
    assert np.array_equal(iv[0], full_modes(N[0])) and np.array_equal(iv[1], full_modes(N[1]))
    assert np.array_equal(iv[2], np.arange(N[2] // 2 + 1)) and np.array_equal(w.astype(np.int64), h)
    assert b.shell_count() == exact_shell(sum((n // 2) ** 2 for n in N)) + 1 == sh.max() + 1
    c = blocks_of("c2c1", N)[0]
    assert c.half_axis is None and np.array_equal(c.hermitian_weights(), np.ones(N[2], dtype=np.uint8))
    assert [v.tolist() for v in c.shell_index_vectors()] == [full_modes(n).tolist() for n in N]
    assert c.shell_count() == b.shell_count()


def binned(sh, wgt, a, b, nshell):
    """(S, A, cnt) per shell: sums of wgt * Re(conj(a) b), of wgt * |a| |b|, and the number of elements."""
    t = wgt * (a.real * b.real + a.imag * b.imag)
    S = np.bincount(sh.ravel(), weights=t.ravel(), minlength=nshell)
    A = np.bincount(sh.ravel(), weights=(wgt * np.abs(a) * np.abs(b)).ravel(), minlength=nshell)
    cnt = np.bincount(sh.ravel(), minlength=nshell)
    return S, A, cnt


@pytest.mark.parametrize("k2", [False, True])
@pytest.mark.parametrize("N", MESHES)
def test_half_spectrum_sums_are_the_full_spectrum_sums(N, k2):
    """numpy only: rfftn with the block's weights and shells against fftn with weight 1 and the exact rule, per shell within
    4 TOL A_s; the sum over the shells is the Parseval sum N0 N1 N2 sum(u w)."""
    rng = np.random.default_rng(sum(N))
    u, w = rng.random(N) - 0.5, rng.random(N) - 0.5
    blk = one_rank_half_block(N)
    nshell = blk.shell_count()
    iv, hw = blk.shell_index_vectors(), blk.hermitian_weights()
    mh = iv[0].astype(np.int64)[:, None, None] ** 2 + iv[1].astype(np.int64)[None, :, None] ** 2 + iv[2].astype(np.int64)[None, None, :] ** 2
    kf = [full_modes(n) for n in N]
    mf = kf[0][:, None, None] ** 2 + kf[1][None, :, None] ** 2 + kf[2][None, None, :] ** 2
    shf = np.vectorize(exact_shell, otypes=[np.int64])(mf)
    wh = hw.astype(np.float64)[None, None, :] * (mh.astype(np.float64) if k2 else 1.0) * np.ones(mh.shape)
    wf = (mf.astype(np.float64) if k2 else 1.0) * np.ones(mf.shape)
    for a, b in ((u, u), (u, w)):
        Sh, Ah, _ = binned(Block.shell_of(mh), wh, np.fft.rfftn(a), np.fft.rfftn(b), nshell)
        Sf, Af, _ = binned(shf, wf, np.fft.fftn(a), np.fft.fftn(b), nshell)
        assert len(Sh) == len(Sf) == nshell
        d = np.abs(Sh - Sf)
        print("N", N, "k2", k2, "max |half - full| / A_s = %.3e" % np.max(d / np.maximum(Ah, 1e-300)))
        assert np.all(d <= 4 * TOL * Ah), (d, Ah)
        assert np.all(np.abs(Ah - Af) <= 4 * TOL * Af)
        if not k2:
            want = float(np.prod(N)) * np.sum(a * b)
            print("   Parseval residual %.3e of %.3e" % (abs(Sh.sum() - want), Ah.sum()))
            assert abs(Sh.sum() - want) <= 4 * TOL * Ah.sum()


def test_the_entry_point_is_declared_bound_and_exported():
    from mpifft4py_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    assert "mfft_ew_shell_sums" in re.findall(r"MFFT_API\s+[\w\s\*]+?\b(mfft_\w+)\s*\(", txt)
    assert "mfft_ew_shell_sums" in _lib.exported_symbols()
    assert hasattr(_lib.load(), "mfft_ew_shell_sums")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert any(l.split()[-1] == "mfft_ew_shell_sums" and " T " in l for l in out.splitlines())
