"""GPU: guard bands and poison for the operations on quadratic forms (tests/guard_util.py): mfft_real_quadratic on the fused and the
composed route, mfft_ew_quadratic, mfft_ew_strain_hat and mfft_nlz_quad_rows run with their inputs between guard bands and their
outputs poisoned.  No guard byte changes (no stray write below or above an input or an output), every slot of the result is
written (none keeps its poison), the inputs come back bit for bit.  The values themselves are judged in
tests/test_gpu_real_quadratic.py; here the slots must sum to the number of points, which no unwritten or doubly written slot
survives, and the six statistics must be finite."""
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
DPOISON = -7.25e300                   # ... and a double no statistic of these fields takes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(nbins):
    """The two host arrays a call fills, each between two guard bands of its own: (buffer, view, guard) for out6 and for counts."""
    g = 4096
    res = []
    for nbytes, dt, poison in ((6 * 8, np.float64, DPOISON), ((nbins + 3) * 8, np.int64, POISON)):
        buf = np.empty(2 * g + nbytes, dtype=np.uint8)
        buf[:g] = pattern(g)
        buf[-g:] = pattern(g)
        out = buf[g:-g].view(dt)
        out[:] = poison
        res.append((buf, out, g))
    return res


def _check_host(res, count, nbins, what):
    (b6, out6, g), (bc, counts, _) = res
    for buf in (b6, bc):
        assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside a host result" % what
    assert not np.any(out6 == DPOISON) and np.all(np.isfinite(out6)), (what, out6)
    assert out6[0] <= out6[1]
    if nbins:
        assert not np.any(counts == POISON), "%s: slots of the counts never written: %s" % (what, np.argwhere(counts == POISON)[:4])
        assert np.all(counts >= 0) and counts.sum() == count and counts[-1] == 0, (what, counts.sum(), count)
    else:
        assert np.all(counts == POISON), "%s: counts written without bins" % what


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("nfields,nbins", [(1, 37), (3, 0), (6, 37)])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_quadratic_guarded(N, fused, nfields, nbins, dealias, prec):
    """mfft_real_quadratic through the C interface: 1, 3 and 6 fields, with and without bins, the fused route (the z stage ends in
    the statistics) and the composed one ([24, 40, 20] has no fused kernels: one field at a time into one work array, its term
    into one array of doubles, one sweep)."""
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
    w = np.array([1.0, 0.5, -0.25, 2.0, 1.0, 3.0][:nfields])
    res = _host_result(nbins)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    _lib.call("mfft_real_quadratic", F._plan, da.ptr, db.ptr if db is not None else None, 1 if nfields == 1 else 3, _DEALIAS[dealias],
              w.ctypes.data_as(DP), 0.01, -0.05, 0.40, nbins, res[0][1].ctypes.data_as(DP), res[1][1].ctypes.data_as(IP), ctypes.byref(count))
    assert F.plan_info("nonlinear_quadratic_fused_%s" % rh.nl.RULE[dealias]) == (1 if fused else 0)
    check(da, "real_quadratic a_hat")
    if db is not None:
        check(db, "real_quadratic b_hat")
    points = int(np.prod([3 * n // 2 for n in N])) if dealias == "3/2-rule" else int(np.prod(N))
    assert count.value == points
    _check_host(res, points, nbins, "real_quadratic %s %s nfields=%d" % (N, dealias, nfields))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape,nbins", [((3, 8, 16, 32), 29), ((1, 7, 9, 15), 29), ((6, 5, 7, 31), 0), ((2, 5, 7, 32), 512)])
def test_ew_quadratic_guarded(shape, nbins, prec):
    """mfft_ew_quadratic: the real array between guard bands (odd sizes: components that start off 16 bytes take the scalar build)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    x = (np.random.default_rng(sum(shape)).standard_normal(shape)).astype(rdtype(prec))
    dx = guarded(shape, rdtype(prec), fill=x)
    ncomp, n = shape[0], int(np.prod(shape[1:]))
    w = np.array([1.0, 0.5, -0.25, 2.0, 1.0, 3.0][:ncomp])
    res = _host_result(nbins)
    _lib.call("mfft_ew_quadratic", F._plan, dx.ptr, ncomp, n, _lib.precision_code(prec), w.ctypes.data_as(DP), 0.0, -1.0, 9.0, nbins,
              res[0][1].ctypes.data_as(DP), res[1][1].ctypes.data_as(IP))
    check(dx, "ew_quadratic x")
    _check_host(res, n, nbins, "ew_quadratic %s" % (shape,))
    q = spectral.quad_rule(x.reshape(ncomp, -1).astype(np.float64), w)
    assert res[0][1][0] == q.min() and res[0][1][1] == q.max()
    if nbins:
        assert np.array_equal(res[1][1], rh._hist(q, -1.0, 9.0, nbins))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N,pitch", [([8, 16, 32], None), ([32, 64, 128], "auto")])
def test_ew_strain_hat_guarded(N, pitch, prec):
    """mfft_ew_strain_hat: U_hat between guard bands and preserved, both outputs poisoned and written everywhere."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch=pitch)
    K = spectral.Wavenumbers(F)
    cs = tuple(int(x) for x in F.complex_shape())
    rng = np.random.default_rng(N[0])
    u = (rng.standard_normal((3,) + cs) + 1j * rng.standard_normal((3,) + cs)).astype(rh.cdtype(prec))
    kw = dict(pitch=F.complex_pitch) if pitch else {}
    U = guarded((3,) + cs, F.complex, fill=u, **kw)
    diag, off = guarded((3,) + cs, F.complex, **kw), guarded((3,) + cs, F.complex, **kw)
    spectral.strain_hat(F, K, U, diag, off)
    F.sync()
    check(U, "strain_hat U_hat")
    check(diag, "strain_hat diag", "output")
    check(off, "strain_hat off", "output")


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,nfields,nrows,nbins", [(16, 6, 301, 64), (512, 3, 9, 0), (768, 1, 5, 64), (3072, 2, 3, 512)])
def test_nlz_quad_rows_guarded(n, nfields, nrows, nbins, prec):
    """mfft_nlz_quad_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in q -- the statistics stay finite and the non-finite slot 0."""
    from mpifft4py_amd import _lib
    valid = n // 2 + 1
    pitch = valid + 5
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = ((ncomp,) if nfields > 2 else ()) + (nrows, valid)
    rng = np.random.default_rng(n + nfields)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(rh.cdtype(prec))
    da = guarded(shape, rh.cdtype(prec), pitch=pitch, fill=draw())
    db = guarded(shape, rh.cdtype(prec), pitch=pitch, fill=draw()) if nfields % 2 == 0 else None
    w = np.array([1.0, 0.5, -0.25, 2.0, 1.0, 3.0][:nfields])
    res = _host_result(nbins)
    _lib.call("mfft_nlz_quad_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, 0,
              _lib.precision_code(prec), w.ctypes.data_as(DP), 0.0, -8.0 / n, 64.0 / n, nbins, res[0][1].ctypes.data_as(DP), res[1][1].ctypes.data_as(IP))
    check(da, "nlz_quad_rows a")
    if db is not None:
        check(db, "nlz_quad_rows b")
    _check_host(res, nrows * n, nbins, "nlz_quad_rows n=%d nfields=%d" % (n, nfields))
