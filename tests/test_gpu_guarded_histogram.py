"""GPU: guard bands and poison for the histogram operations (tests/guard_util.py): mfft_real_histogram on the fused and the composed
route, mfft_ew_histogram and mfft_nlz_hist_rows run with their inputs between guard bands and their outputs poisoned.  No guard
byte changes (no stray write below or above an input), every slot of the result is written (none keeps its poison), the inputs
come back bit for bit.  The counts themselves are judged in tests/test_gpu_real_histogram.py; here every field's slots must sum
to the number of points, which no unwritten or doubly written slot survives."""
import ctypes

import numpy as np
import pytest

import test_gpu_real_histogram as rh
from gpu_util import L, have_gpu, rdtype
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
POISON = -0x0101010101010102          # int64 of a host result nobody has written (no count is negative)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(nfields, nbins):
    """The host array a call fills, between two guard bands of its own: (whole buffer, view of the result)."""
    g = 4096
    buf = np.empty(2 * g + nfields * (nbins + 3) * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.int64).reshape(nfields, nbins + 3)
    out[:] = POISON
    return buf, out, g


def _check_host(buf, out, g, count, what):
    assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
    assert not np.any(out == POISON), "%s: slots of the result never written: %s" % (what, np.argwhere(out == POISON)[:4])
    assert np.all(out >= 0) and np.all(out.sum(1) == count), (what, out.sum(1), count)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_histogram_guarded(N, fused, nfields, dealias, prec):
    """mfft_real_histogram through the C interface: 1, 3 and 6 fields, the fused route (the z stage ends in a histogram) and the
    composed one ([24, 40, 20] has no fused kernels: one field at a time into one work array, then the sweep)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    cs = tuple(int(x) for x in F.complex_shape())
    a, b = rh.nl.spectra(cs, np.array(N), prec, 5 + N[2], True)
    if nfields == 1:
        da, db = guarded(cs, F.complex, fill=a[0]), None
    else:
        da = guarded((3,) + cs, F.complex, fill=a)
        db = guarded((3,) + cs, F.complex, fill=b) if nfields == 6 else None
    nbins = 37
    lo, hi = np.full(nfields, -0.45), np.full(nfields, 0.40)
    buf, out, g = _host_result(nfields, nbins)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    _lib.call("mfft_real_histogram", F._plan, da.ptr, db.ptr if db is not None else None, 1 if nfields == 1 else 3, _DEALIAS[dealias],
              lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP), ctypes.byref(count))
    assert F.plan_info(rh.INFO(dealias)) == (1 if fused else 0)
    check(da, "real_histogram a_hat")
    if db is not None:
        check(db, "real_histogram b_hat")
    points = int(np.prod([3 * n // 2 for n in N])) if dealias == "3/2-rule" else int(np.prod(N))
    assert count.value == points
    _check_host(buf, out, g, points, "real_histogram %s %s nfields=%d" % (N, dealias, nfields))
    assert np.all(out[:, -1] == 0) and np.all(out[:, 1:-2].sum(1) > 0)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15), (6, 5, 7, 31)])
def test_ew_histogram_guarded(shape, prec):
    """mfft_ew_histogram: the real array between guard bands (odd sizes: components that start off 16 bytes, heads and tails)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    x = (np.random.default_rng(sum(shape)).standard_normal(shape)).astype(rdtype(prec))
    dx = guarded(shape, rdtype(prec), fill=x)
    ncomp, n, nbins = shape[0], int(np.prod(shape[1:])), 29
    lo, hi = np.full(ncomp, -2.0), np.full(ncomp, 2.5)
    buf, out, g = _host_result(ncomp, nbins)
    _lib.call("mfft_ew_histogram", F._plan, dx.ptr, ncomp, n, _lib.precision_code(prec), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP),
              nbins, out.ctypes.data_as(IP))
    check(dx, "ew_histogram x")
    _check_host(buf, out, g, n, "ew_histogram %s" % (shape,))
    assert np.array_equal(out, np.stack([rh._hist(x[c], -2.0, 2.5, nbins) for c in range(ncomp)]))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,nfields,nrows", [(16, 6, 301), (512, 3, 9), (768, 1, 5), (3072, 2, 3)])
def test_nlz_hist_rows_guarded(n, nfields, nrows, prec):
    """mfft_nlz_hist_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in the transform -- the non-finite slots stay 0."""
    from mpifft4py_amd import _lib
    valid = n // 2 + 1
    pitch = valid + 5
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = ((ncomp,) if nfields > 2 else ()) + (nrows, valid)
    rng = np.random.default_rng(n + nfields)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(rh.cdtype(prec))
    da = guarded(shape, rh.cdtype(prec), pitch=pitch, fill=draw())
    db = guarded(shape, rh.cdtype(prec), pitch=pitch, fill=draw()) if nfields % 2 == 0 else None
    nbins = 64
    s = 4 * np.sqrt(2.0 / n)
    lo, hi = np.full(nfields, -s), np.full(nfields, s)
    buf, out, g = _host_result(nfields, nbins)
    _lib.call("mfft_nlz_hist_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, 0,
              _lib.precision_code(prec), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP))
    check(da, "nlz_hist_rows a")
    if db is not None:
        check(db, "nlz_hist_rows b")
    _check_host(buf, out, g, nrows * n, "nlz_hist_rows n=%d nfields=%d" % (n, nfields))
    assert np.all(out[:, -1] == 0), out[:, -1]
