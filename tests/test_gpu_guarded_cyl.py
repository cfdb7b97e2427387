"""GPU: guard bands and poison for the (k_perp, k_z) sums (tests/guard_util.py): mfft_ew_cyl_sums runs with its two fields between
guard bands and its host result poisoned between guard bands of its own.  No guard byte changes (no stray write below or above an
input), the inputs come back bit for bit, and every double of the result is written (none keeps its poison).  The sums themselves
are judged in tests/test_gpu_cyl_spectrum.py; here they must be finite, the bins of a field with itself not negative, and their
total the Parseval sum of the downloaded field to 1e-12."""
import ctypes

import numpy as np
import pytest

from gpu_util import L, cdtype, have_gpu
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
I32 = ctypes.POINTER(ctypes.c_int32)
POISON = np.frombuffer(np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).tobytes(), dtype=np.float64)[0]      # a NaN nobody computes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(nperp, npar):
    """The host array a call fills, between two guard bands of its own: (whole buffer, view of the result, guard size)."""
    g = 4096
    buf = np.empty(2 * g + nperp * npar * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.float64).reshape(nperp, npar)
    out[:] = POISON
    return buf, out, g


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("N", [(12, 10, 16), (8, 6, 130)])
def test_ew_cyl_sums_guarded(N, same, ncomp, prec):
    """Rows of 9 (one partial wave; odd, so fp32 loads 8 bytes) and of 66 (a run of 2 behind a whole wave), one and three components,
    b is a and b of its own, with and without |K|^2."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    K = spectral.Wavenumbers(F)
    cs = tuple(int(x) for x in F.complex_shape())
    shape = cs if ncomp == 1 else (3,) + cs
    rng = np.random.default_rng(sum(N) + ncomp)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
    ha = draw()
    da = guarded(shape, F.complex, fill=ha)
    db = da if same else guarded(shape, F.complex, fill=draw())
    F.comm.use_device()
    for k2 in (0, 1):
        buf, out, g = _host_result(K.nperp, K.npar)
        _lib.call("mfft_ew_cyl_sums", F._plan, da.ptr, db.ptr, ncomp, K.perp_rows.ptr, K.perp_start.ctypes.data_as(I32), K.nperp, K.idev[2].ptr,
                  K.hdev.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr, k2, K.cshape, K.npar, 0, _lib.precision_code(prec), out.ctypes.data_as(DP))
        what = "ew_cyl_sums %s %s ncomp=%d same=%d k2=%d" % (list(N), prec, ncomp, same, k2)
        check(da, what + " a")
        if not same:
            check(db, what + " b")
        assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
        poison = out.view(np.uint64) == np.array([POISON]).view(np.uint64)[0]
        assert not np.any(poison), "%s: doubles of the result never written: %s" % (what, np.argwhere(poison)[:4])
        assert np.all(np.isfinite(out)), what
        if same:
            assert np.all(out >= 0), what
            if not k2:
                h = K._mesh.hermitian_weights().astype(np.float64)
                want = float((np.abs(ha.astype(np.complex128)) ** 2 * h).sum())
                assert abs(out.sum() - want) <= 1e-12 * want, (what, out.sum(), want)
