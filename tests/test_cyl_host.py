"""CPU: the device-free half of the (k_perp, k_z) spectra (spectral.cyl_sums): the row lists `_mesh.Block.perp_row_lists` and
`mfft_cyl_row_lists` build for every rank's spectral window of slab and pencil layouts (on a LayoutComm: no device, no plan), and
the perp shell count.  The judge of a row's shell is math.isqrt on integers, never the helpers under test."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mpifft4py_amd import LayoutComm, Pencil_R2C, Slab_C2C, Slab_R2C, _lib
from mpifft4py_amd._mesh import Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.array([2 * np.pi] * 3)
I32 = ctypes.POINTER(ctypes.c_int32)


def exact_shell(m):
    m = int(m)
    if m == 0:
        return 0
    s = math.isqrt(m)
    if 4 * m >= (2 * s + 1) ** 2:
        s += 1
    assert (2 * s - 1) ** 2 <= 4 * m < (2 * s + 1) ** 2 and s >= 1
    return s


def blocks_of(kind, N):
    N = np.array(N)
    if kind == "slab1":
        return [Slab_R2C(N, L, LayoutComm(1, 0), "double")._mesh]
    if kind == "slab4":
        return [Slab_R2C(N, L, LayoutComm(4, r), "double")._mesh for r in range(4)]
    if kind == "c2c1":
        return [Slab_C2C(N, L, LayoutComm(1, 0), "double")._mesh]
    return [Pencil_R2C(N, L, LayoutComm(4, r), "double", P1=2, alignment=kind[-1])._mesh for r in range(4)]


LAYOUTS = [("slab1", (16, 12, 20)), ("slab1", (12, 10, 16)), ("c2c1", (7, 9, 15)), ("slab4", (16, 12, 20)), ("pencilX", (16, 12, 20)),
           ("pencilY", (16, 12, 20))]


def c_row_lists(ikx, iky, nperp):
    rows = np.full(len(ikx) * len(iky), -1, dtype=np.int32)
    start = np.full(nperp + 1, -1, dtype=np.int32)
    rc = _lib.load().mfft_cyl_row_lists(ikx.ctypes.data_as(I32), iky.ctypes.data_as(I32), len(ikx), len(iky), nperp,
                                        rows.ctypes.data_as(I32), start.ctypes.data_as(I32))
    return rc, rows, start


@pytest.mark.parametrize("kind,N", LAYOUTS)
def test_row_lists_of_every_rank(kind, N):
    """Every local row once, grouped by the exact shell of kx^2 + ky^2, (l, j) order inside a shell, monotone offsets; some
    rank of a distributed layout has empty shells, and over the ranks every mode of the global spectrum lies in one listed row."""
    nperp = exact_shell((N[0] // 2) ** 2 + (N[1] // 2) ** 2) + 1
    seen = np.zeros((N[0], N[1], N[2] // 2 + 1 if kind != "c2c1" else N[2]), dtype=np.int64)      # (pencils split z too)
    empties = 0
    for b in blocks_of(kind, N):
        assert b.perp_shell_count() == nperp
        rows, start = b.perp_row_lists()
        s0, s1, _ = b.spectral_shape()
        assert rows.dtype == np.int32 and start.dtype == np.int32 and rows.shape == (s0 * s1,) and start.shape == (nperp + 1,)
        assert sorted(rows.tolist()) == list(range(s0 * s1))                         # every local row exactly once
        assert start[0] == 0 and start[-1] == s0 * s1 and np.all(np.diff(start) >= 0)
        kx, ky = b.mode_vectors()[:2]
        for p in range(nperp):
            mine = rows[start[p]:start[p + 1]].tolist()
            assert all(exact_shell(int(kx[r // s1]) ** 2 + int(ky[r % s1]) ** 2) == p for r in mine), (kind, p)
            assert mine == sorted(mine)                                              # l * s1 + j ascending = (l, j) order
            empties += not mine
        # the C entry builds the same lists
        ikx, iky = b.shell_index_vectors()[:2]
        rc, crows, cstart = c_row_lists(ikx, iky, nperp)
        assert rc == 0 and np.array_equal(crows, rows) and np.array_equal(cstart, start)
        seen[tuple(slice(a, a + n) for a, n in b.spectral_window)] += 1
    assert np.all(seen == 1)
    if kind != "slab1" and kind != "c2c1":
        assert empties > 0, "no rank of %s has an empty shell: the case is not exercised" % kind


def test_row_lists_error_returns():
    ikx = np.array([0, 1, 2, -3, -2, -1], dtype=np.int32)
    iky = np.array([0, 1, -2, -1], dtype=np.int32)
    nperp = exact_shell(9 + 4) + 1
    rc, rows, start = c_row_lists(ikx, iky, nperp)
    assert rc == 0 and start[-1] == 24
    rc, _, _ = c_row_lists(ikx, iky, nperp - 1)                                      # a row's shell is >= nperp: MFFT_ERR_INVALID
    assert rc == -1 and b"nperp" in _lib.load().mfft_last_error()
    lib = _lib.load()
    assert lib.mfft_cyl_row_lists(None, iky.ctypes.data_as(I32), 6, 4, nperp, rows.ctypes.data_as(I32), start.ctypes.data_as(I32)) == -1
    assert lib.mfft_cyl_row_lists(ikx.ctypes.data_as(I32), iky.ctypes.data_as(I32), 0, 4, nperp, rows.ctypes.data_as(I32), start.ctypes.data_as(I32)) == -1


@pytest.mark.parametrize("N01,want", [((12, 10), 9), ((160, 160), 114), ((1024, 1024), 725)])
def test_perp_shell_count(N01, want):
    b = Block(list(N01) + [8], L, [(0, N01[0]), (0, N01[1]), (0, 8)], [(0, N01[0]), (0, N01[1]), (0, 5)], 2)
    assert b.perp_shell_count() == want == exact_shell((N01[0] // 2) ** 2 + (N01[1] // 2) ** 2) + 1


def test_largest_list_of_160_squared_exceeds_the_default_segment():
    """What tests/test_gpu_cyl_spectrum.py relies on for its fold over several segments."""
    b = Block([160, 160, 8], L, [(0, 160), (0, 160), (0, 8)], [(0, 160), (0, 160), (0, 5)], 2)
    _, start = b.perp_row_lists()
    txt = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    seg = int(re.search(r"#define MFFT_CYL_SEG_ROWS (\d+)", txt).group(1))
    assert np.diff(start).max() == 500 > seg


def test_the_entry_points_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("mfft_cyl_row_lists", "mfft_ew_cyl_sums"):
        assert name in re.findall(r"MFFT_API\s+[\w\s\*]+?\b(mfft_\w+)\s*\(", txt)
        assert name in _lib.exported_symbols() and hasattr(_lib.load(), name)
        assert any(l.split()[-1] == name and " T " in l for l in out.splitlines())
