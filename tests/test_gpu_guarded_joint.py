"""GPU: guard bands and poison for the joint-histogram operations (tests/guard_util.py): mfft_real_joint_histogram on the fused and
the composed route, mfft_ew_joint_histogram and mfft_nlz_joint_rows run with their inputs between guard bands and their outputs
poisoned.  No guard byte changes (no stray write below or above an input), every cell of the result is written (none keeps its
poison), the inputs come back bit for bit.  The counts themselves are judged in tests/test_gpu_real_joint.py; here every pair's
cells must sum to the number of points, which no unwritten or doubly written cell survives."""
import ctypes

import numpy as np
import pytest

import test_gpu_real_joint as rj
from gpu_util import L, cdtype, have_gpu, rdtype
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
POISON = -0x0101010101010102          # int64 of a host result nobody has written (no count is negative)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(npairs, nba, nbb):
    """The host array a call fills, between two guard bands of its own: (whole buffer, view of the result)."""
    g = 4096
    buf = np.empty(2 * g + npairs * (nba + 3) * (nbb + 3) * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.int64).reshape(npairs, nba + 3, nbb + 3)
    out[:] = POISON
    return buf, out, g


def _check_host(buf, out, g, count, what):
    assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
    assert not np.any(out == POISON), "%s: cells of the result never written: %s" % (what, np.argwhere(out == POISON)[:4])
    assert np.all(out >= 0) and np.all(out.sum((1, 2)) == count), (what, out.sum((1, 2)), count)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_joint_histogram_guarded(N, fused, ncomp, dealias, prec):
    """mfft_real_joint_histogram through the C interface: one and three pairs, the fused route (the z stage ends in the grid) and
    the composed one ([24, 40, 20] has no fused kernels: a_p and b_p into two work arrays, then the sweep)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    cs = tuple(int(x) for x in F.complex_shape())
    a, b = rj.nl.spectra(cs, np.array(N), prec, 5 + N[2], True)
    if ncomp == 1:
        da, db = guarded(cs, F.complex, fill=a[0]), guarded(cs, F.complex, fill=b[0])
    else:
        da, db = guarded((3,) + cs, F.complex, fill=a), guarded((3,) + cs, F.complex, fill=b)
    nba, nbb = 37, 64
    lo, hi = np.full(2 * ncomp, -0.45), np.full(2 * ncomp, 0.40)
    buf, out, g = _host_result(ncomp, nba, nbb)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    F.comm.use_device()
    _lib.call("mfft_real_joint_histogram", F._plan, da.ptr, db.ptr, ncomp, _DEALIAS[dealias], lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
              nba, nbb, out.ctypes.data_as(IP), ctypes.byref(count))
    assert F.plan_info(rj.INFO(dealias)) == (1 if fused else 0)
    check(da, "real_joint_histogram a_hat")
    check(db, "real_joint_histogram b_hat")
    points = int(np.prod([3 * n // 2 for n in N])) if dealias == "3/2-rule" else int(np.prod(N))
    assert count.value == points
    _check_host(buf, out, g, points, "real_joint_histogram %s %s ncomp=%d" % (N, dealias, ncomp))
    assert np.all(out[:, -1, :] == 0) and np.all(out[:, :, -1] == 0) and np.all(out[:, 1:-2, 1:-2].sum((1, 2)) > 0)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15), (3, 5, 7, 31)])
def test_ew_joint_histogram_guarded(shape, prec):
    """mfft_ew_joint_histogram: the real arrays between guard bands (odd sizes: components that start off 16 bytes, heads and tails)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(sum(shape))
    x, y = rng.standard_normal(shape).astype(rdtype(prec)), rng.standard_normal(shape).astype(rdtype(prec))
    dx, dy = guarded(shape, rdtype(prec), fill=x), guarded(shape, rdtype(prec), fill=y)
    ncomp, n, nba, nbb = shape[0], int(np.prod(shape[1:])), 29, 64
    lo = np.concatenate([np.full(ncomp, -2.0), np.full(ncomp, -1.5)])
    hi = np.concatenate([np.full(ncomp, 2.5), np.full(ncomp, 1.0)])
    buf, out, g = _host_result(ncomp, nba, nbb)
    F.comm.use_device()
    _lib.call("mfft_ew_joint_histogram", F._plan, dx.ptr, dy.ptr, ncomp, n, _lib.precision_code(prec), lo.ctypes.data_as(DP),
              hi.ctypes.data_as(DP), nba, nbb, out.ctypes.data_as(IP))
    check(dx, "ew_joint_histogram x")
    check(dy, "ew_joint_histogram y")
    _check_host(buf, out, g, n, "ew_joint_histogram %s" % (shape,))
    assert np.array_equal(out, np.stack([rj._grid(x[c], y[c], (-2.0, -1.5), (2.5, 1.0), nba, nbb) for c in range(ncomp)]))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,ncomp,nrows", [(16, 3, 301), (512, 3, 9), (768, 1, 5), (3072, 1, 3)])
def test_nlz_joint_rows_guarded(n, ncomp, nrows, prec):
    """mfft_nlz_joint_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in the transform -- the non-finite row and column stay 0."""
    from mpifft4py_amd import _lib
    valid = n // 2 + 1
    pitch = valid + 5
    shape = (ncomp, nrows, valid)
    rng = np.random.default_rng(n + ncomp)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
    da = guarded(shape, cdtype(prec), pitch=pitch, fill=draw())
    db = guarded(shape, cdtype(prec), pitch=pitch, fill=draw())
    nba, nbb = 64, 64
    s = 4 * np.sqrt(2.0 / n)
    lo, hi = np.full(2 * ncomp, -s), np.full(2 * ncomp, s)
    buf, out, g = _host_result(ncomp, nba, nbb)
    _lib.call("mfft_nlz_joint_rows", da.ptr, db.ptr, ncomp, nrows, n, pitch, valid, 0, _lib.precision_code(prec),
              lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nba, nbb, out.ctypes.data_as(IP))
    check(da, "nlz_joint_rows a")
    check(db, "nlz_joint_rows b")
    _check_host(buf, out, g, nrows * n, "nlz_joint_rows n=%d ncomp=%d" % (n, ncomp))
    assert np.all(out[:, -1, :] == 0) and np.all(out[:, :, -1] == 0), (out[:, -1, :].sum(), out[:, :, -1].sum())
