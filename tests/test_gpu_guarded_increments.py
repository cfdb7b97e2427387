"""GPU: guard bands and poison for the structure functions (tests/guard_util.py): mfft_real_increments on the fused and the composed
route, mfft_ew_increments and mfft_nlz_incr_rows run with their inputs between guard bands and their host results between guard
bands of their own, poisoned.  No guard byte changes (no stray write below or above an input or a result), every slot of the
result is written (none keeps its poison), the inputs come back bit for bit.  The values themselves are judged in
tests/test_gpu_real_increments.py; here the sums must be finite, S2 and S4 not negative, and -- pitched rows with poison between
them -- no value beside a row may have been read."""
import ctypes

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, cdtype, have_gpu, rdtype
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
DPOISON = -7.25e300                   # a double no sum of these fields takes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(nvals):
    """The host array a call fills, between two guard bands of its own: (buffer, view, guard)."""
    g = 4096
    buf = np.empty(2 * g + nvals * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.float64)
    out[:] = DPOISON
    return buf, out, g


def _check_host(res, what):
    buf, out, g = res
    assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
    assert not np.any(out == DPOISON), "%s: sums never written: %s" % (what, np.argwhere(out == DPOISON)[:4])
    s = out.reshape(-1, 3)
    assert np.all(np.isfinite(s)) and np.all(s[:, 0] >= 0) and np.all(s[:, 2] >= 0), (what, s)
    # Cauchy-Schwarz over the points: S3^2 <= S2 S4
    assert np.all(s[:, 1] ** 2 <= s[:, 0] * s[:, 2] * (1 + 1e-9) + 1e-300), (what, s)


def _seps(M, nsep):
    return np.ascontiguousarray([1, M - 1, M // 2, (M // 2 - 1) | 1, 2, 1, 3, M - 2][:nsep], dtype=np.int64)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("nfields,nsep", [(1, 8), (3, 1), (6, 5)])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_increments_guarded(N, fused, nfields, nsep, dealias, prec):
    """mfft_real_increments through the C interface: 1, 3 and 6 fields, one separation, some and all a call takes, the fused route
    (the z stage ends in the sums) and the composed one ([24, 40, 20] has no fused kernels: one field at a time into one work
    array, one sweep each)."""
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
    res = _host_result(nfields * nsep * 3)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    _lib.call("mfft_real_increments", F._plan, da.ptr, db.ptr if db is not None else None, 1 if nfields == 1 else 3, _DEALIAS[dealias],
              seps.ctypes.data_as(IP), nsep, res[1].ctypes.data_as(DP), ctypes.byref(count))
    assert F.plan_info("nonlinear_increments_fused_%s" % nl.RULE[dealias]) == (1 if fused else 0)
    check(da, "real_increments a_hat")
    if db is not None:
        check(db, "real_increments b_hat")
    points = int(np.prod([3 * n // 2 for n in N])) if dealias == "3/2-rule" else int(np.prod(N))
    assert count.value == points
    _check_host(res, "real_increments %s %s nfields=%d" % (N, dealias, nfields))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape,pitch,nsep", [((3, 8, 16, 32), None, 8), ((1, 7, 9, 15), None, 5), ((6, 5, 7, 31), 37, 1), ((2, 5, 7, 32), 40, 8)])
def test_ew_increments_guarded(shape, pitch, nsep, prec):
    """mfft_ew_increments: the real array between guard bands (odd sizes, and pitched rows with poison between them: a read beside a
    row would be a NaN in the sums)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    x = (np.random.default_rng(sum(shape)).standard_normal(shape)).astype(rdtype(prec))
    dx = guarded(shape, rdtype(prec), fill=x, **(dict(pitch=pitch) if pitch else {}))
    ncomp, n = shape[0], shape[-1]
    nrows = int(np.prod(shape[1:-1]))
    seps = _seps(n, nsep)
    res = _host_result(ncomp * nsep * 3)
    _lib.call("mfft_ew_increments", F._plan, dx.ptr, ncomp, nrows, n, pitch or n, _lib.precision_code(prec), seps.ctypes.data_as(IP), nsep,
              res[1].ctypes.data_as(DP))
    check(dx, "ew_increments x")
    _check_host(res, "ew_increments %s" % (shape,))
    want = np.stack([spectral.incr_rule(x[c].astype(np.float64), seps) for c in range(ncomp)])
    assert np.allclose(res[1].reshape(ncomp, nsep, 3), want, rtol=1e-9, atol=1e-12 * float(np.abs(want).max()))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,nfields,nrows,nsep", [(16, 6, 301, 8), (12, 3, 9, 1), (768, 1, 5, 8), (1024, 2, 3, 5), (1536, 6, 3, 8)])
def test_nlz_incr_rows_guarded(n, nfields, nrows, nsep, prec):
    """mfft_nlz_incr_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in the sums -- they stay finite."""
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
    res = _host_result(nfields * nsep * 3)
    _lib.call("mfft_nlz_incr_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, 0,
              _lib.precision_code(prec), seps.ctypes.data_as(IP), nsep, res[1].ctypes.data_as(DP))
    check(da, "nlz_incr_rows a")
    if db is not None:
        check(db, "nlz_incr_rows b")
    _check_host(res, "nlz_incr_rows n=%d nfields=%d" % (n, nfields))
