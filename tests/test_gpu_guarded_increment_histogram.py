"""GPU: guard bands and poison for the increment PDFs (tests/guard_util.py): mfft_real_increment_histogram on the fused and the composed
route, mfft_ew_increment_histogram and mfft_nlz_incr_hist_rows run with their inputs between guard bands and their host results
between guard bands of their own, poisoned.  No guard byte changes (no stray write below or above an input or a result), every slot
of the result is written (none keeps its poison), the inputs come back bit for bit.  The counts themselves are judged in
tests/test_gpu_real_increment_histogram.py; here every (field, separation) must sum to the points and hold no non-finite count --
pitched rows have poison between them: a value read beside a row would be a NaN in a difference."""
import ctypes

import numpy as np
import pytest

import incr_hist_util as ih
import nonlinear_util as nl
from gpu_util import L, cdtype, have_gpu, rdtype
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
IPOISON = -0x5A5A5A5A5A5A5A5A         # an int64 no count takes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(nfields, nsep, nbins):
    """The host array a call fills, between two guard bands of its own: (buffer, view, guard)."""
    g = 4096
    buf = np.empty(2 * g + nfields * nsep * (nbins + 3) * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.int64)
    out[:] = IPOISON
    return buf, out.reshape(nfields, nsep, nbins + 3), g


def _check_host(res, points, what):
    buf, out, g = res
    assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
    assert not np.any(out == IPOISON), "%s: counts never written: %s" % (what, np.argwhere(out == IPOISON)[:4])
    assert np.all(out >= 0) and np.all(out.sum(2) == points) and np.all(out[:, :, -1] == 0), (what, out.sum(2), points, out[:, :, -1])


def _seps(M, nsep):
    return np.ascontiguousarray([1, M - 1, M // 2, (M // 2 - 1) | 1, 2, 1, 3, M - 2][:nsep], dtype=np.int64)


def _ranges(nfields, nsep, scale):
    lo = np.ascontiguousarray(-scale * (1.0 + 0.1 * np.arange(nfields * nsep)))
    return lo, np.ascontiguousarray(-0.9 * lo)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("nfields,nsep,nbins", [(1, 8, 256), (3, 1, 1), (6, 5, 37)])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_increment_histogram_guarded(N, fused, nfields, nsep, nbins, dealias, prec):
    """mfft_real_increment_histogram through the C interface: 1, 3 and 6 fields, one separation, some and all a call takes, 1, 37 and
    256 bins, the fused route (the z stage ends in the counts) and the composed one ([24, 40, 20] has no fused kernels: one field at
    a time into one work array, one sweep each)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    cs = tuple(int(x) for x in F.complex_shape())
    a, b = nl.spectra(cs, np.array(N), prec, 5 + N[2], True)
    if nfields == 1:
        da, db = guarded(cs, F.complex, fill=a[0]), None
    else:
        da = guarded((3,) + cs, F.complex, fill=a)
        db = guarded((3,) + cs, F.complex, fill=b) if nfields == 6 else None
    M = 3 * N[2] // 2 if dealias == "3/2-rule" else N[2]
    seps = _seps(M, nsep)
    lo, hi = _ranges(nfields, nsep, 0.5)
    res = _host_result(nfields, nsep, nbins)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    _lib.call("mfft_real_increment_histogram", F._plan, da.ptr, db.ptr if db is not None else None, 1 if nfields == 1 else 3, _DEALIAS[dealias],
              seps.ctypes.data_as(IP), nsep, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, res[1].ctypes.data_as(IP), ctypes.byref(count))
    assert F.plan_info("nonlinear_incr_hist_fused_%s" % nl.RULE[dealias]) == (1 if fused else 0)
    check(da, "real_increment_histogram a_hat")
    if db is not None:
        check(db, "real_increment_histogram b_hat")
    points = int(np.prod([3 * n // 2 for n in N])) if dealias == "3/2-rule" else int(np.prod(N))
    assert count.value == points
    _check_host(res, points, "real_increment_histogram %s %s nfields=%d" % (N, dealias, nfields))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape,pitch,nsep,nbins", [((3, 8, 16, 32), None, 8, 256), ((1, 7, 9, 15), None, 5, 37), ((6, 5, 7, 31), 37, 1, 1),
                                                    ((2, 5, 7, 32), 40, 8, 64), ((1, 1, 3, 300), 301, 4, 16)])
def test_ew_increment_histogram_guarded(shape, pitch, nsep, nbins, prec):
    """mfft_ew_increment_histogram: the real array between guard bands (odd sizes, and pitched rows with poison between them); the
    counts EQUAL numpy's by the rule."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    x = (np.random.default_rng(sum(shape)).standard_normal(shape)).astype(rdtype(prec))
    dx = guarded(shape, rdtype(prec), fill=x, **(dict(pitch=pitch) if pitch else {}))
    ncomp, n = shape[0], shape[-1]
    nrows = int(np.prod(shape[1:-1]))
    seps = _seps(n, nsep)
    lo, hi = _ranges(ncomp, nsep, 2.0)
    res = _host_result(ncomp, nsep, nbins)
    _lib.call("mfft_ew_increment_histogram", F._plan, dx.ptr, ncomp, nrows, n, pitch or n, _lib.precision_code(prec), seps.ctypes.data_as(IP), nsep,
              lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, res[1].ctypes.data_as(IP))
    check(dx, "ew_increment_histogram x")
    _check_host(res, nrows * n, "ew_increment_histogram %s" % (shape,))
    l2, h2 = lo.reshape(ncomp, nsep), hi.reshape(ncomp, nsep)
    want = np.stack([ih.counts(x[c].astype(np.float64), seps, l2[c], h2[c], nbins) for c in range(ncomp)])
    assert np.array_equal(res[1], want)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,nfields,nrows,nsep,nbins", [(16, 6, 301, 8, 256), (12, 3, 9, 1, 1), (768, 1, 5, 8, 64), (1024, 2, 3, 5, 37),
                                                        (1536, 6, 3, 8, 256)])
def test_nlz_incr_hist_rows_guarded(n, nfields, nrows, nsep, nbins, prec):
    """mfft_nlz_incr_hist_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in a difference -- the non-finite slots stay empty."""
    from mpifft4py_amd import _lib
    valid = n // 2 + 1
    pitch = valid + 5
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = ((ncomp,) if nfields > 2 else ()) + (nrows, valid)
    rng = np.random.default_rng(n + nfields)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
    da = guarded(shape, cdtype(prec), pitch=pitch, fill=draw())
    db = guarded(shape, cdtype(prec), pitch=pitch, fill=draw()) if nfields % 2 == 0 else None
    seps = _seps(n, nsep)
    lo, hi = _ranges(nfields, nsep, 4.0 / np.sqrt(n))
    res = _host_result(nfields, nsep, nbins)
    _lib.call("mfft_nlz_incr_hist_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, 0,
              _lib.precision_code(prec), seps.ctypes.data_as(IP), nsep, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, res[1].ctypes.data_as(IP))
    check(da, "nlz_incr_hist_rows a")
    if db is not None:
        check(db, "nlz_incr_hist_rows b")
    _check_host(res, nrows * n, "nlz_incr_hist_rows n=%d nfields=%d" % (n, nfields))
