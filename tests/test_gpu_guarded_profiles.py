"""GPU: guard bands and poison for the profile operations (tests/guard_util.py): mfft_real_profiles on the fused and the composed
route, mfft_ew_profiles and mfft_nlz_profile_rows run with their inputs between guard bands and their outputs poisoned.  No guard
byte changes (no stray write below or above an input), every double of the result is written (none keeps its poison), the inputs
come back bit for bit.  The sums themselves are judged in tests/test_gpu_real_profiles.py; here they must be finite, the sums of
squares not negative, and |sum d_a d_b| <= sqrt(sum d_a^2 sum d_b^2) (Cauchy-Schwarz, with the rounding of the three sums), which
no unwritten or doubly folded slot survives together with the count."""
import ctypes

import numpy as np
import pytest

import test_gpu_real_profiles as rp
from gpu_util import L, cdtype, have_gpu, rdtype
from guard_util import check, guarded, pattern

pytestmark = pytest.mark.gpu
DP = ctypes.POINTER(ctypes.c_double)
POISON = np.frombuffer(np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).tobytes(), dtype=np.float64)[0]      # a NaN nobody computes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _host_result(npairs, M):
    """The host array a call fills, between two guard bands of its own: (whole buffer, view of the result)."""
    g = 4096
    buf = np.empty(2 * g + npairs * 5 * M * 8, dtype=np.uint8)
    buf[:g] = pattern(g)
    buf[-g:] = pattern(g)
    out = buf[g:-g].view(np.float64).reshape(npairs, 5, M)
    out[:] = POISON
    return buf, out, g


def _check_host(buf, out, g, what):
    assert np.array_equal(buf[:g], pattern(g)) and np.array_equal(buf[-g:], pattern(g)), "%s: stray write beside the host result" % what
    poison = out.view(np.uint64) == np.array([POISON]).view(np.uint64)[0]
    assert not np.any(poison), "%s: doubles of the result never written: %s" % (what, np.argwhere(poison)[:4])
    assert np.all(np.isfinite(out)) and np.all(out[:, 2:4] >= 0), what
    assert np.all(np.abs(out[:, 4]) <= np.sqrt(out[:, 2] * out[:, 3]) * (1 + 1e-5) + 1e-300), what
    assert np.all(out[:, 2] > 0) and np.all(out[:, 3] > 0), what


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)])
def test_real_profiles_guarded(N, fused, ncomp, dealias, prec):
    """mfft_real_profiles through the C interface: one and three pairs, the fused route (the z stage ends in the plane sums) and the
    composed one ([24, 40, 20] has no fused kernels: a_p and b_p into two work arrays, then the sweep)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    cs = tuple(int(x) for x in F.complex_shape())
    a, b = rp.nl.spectra(cs, np.array(N), prec, 5 + N[2], True)
    if ncomp == 1:
        da, db = guarded(cs, F.complex, fill=a[0]), guarded(cs, F.complex, fill=b[0])
    else:
        da, db = guarded((3,) + cs, F.complex, fill=a), guarded((3,) + cs, F.complex, fill=b)
    M = 3 * N[2] // 2 if dealias == "3/2-rule" else N[2]
    center = np.linspace(-0.02, 0.03, 2 * ncomp)
    buf, out, g = _host_result(ncomp, M)
    count = ctypes.c_int64(-1)
    if dealias == "2/3-rule":
        F._ensure_mask()
    F.comm.use_device()
    _lib.call("mfft_real_profiles", F._plan, da.ptr, db.ptr, ncomp, _DEALIAS[dealias], center.ctypes.data_as(DP), out.ctypes.data_as(DP), ctypes.byref(count))
    assert F.plan_info(rp.INFO(dealias)) == (1 if fused else 0)
    check(da, "real_profiles a_hat")
    check(db, "real_profiles b_hat")
    plane = (3 * N[0] // 2) * (3 * N[1] // 2) if dealias == "3/2-rule" else N[0] * N[1]
    assert count.value == plane
    _check_host(buf, out, g, "real_profiles %s %s ncomp=%d" % (N, dealias, ncomp))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15), (3, 5, 7, 131)])
def test_ew_profiles_guarded(shape, prec):
    """mfft_ew_profiles: the real arrays between guard bands (odd row lengths, a row longer than two column blocks of the sweep)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(sum(shape))
    x, y = rng.standard_normal(shape).astype(rdtype(prec)), rng.standard_normal(shape).astype(rdtype(prec))
    dx, dy = guarded(shape, rdtype(prec), fill=x), guarded(shape, rdtype(prec), fill=y)
    ncomp, nrows, M = shape[0], shape[1] * shape[2], shape[3]
    center = np.linspace(-0.5, 0.5, 2 * ncomp)
    buf, out, g = _host_result(ncomp, M)
    F.comm.use_device()
    _lib.call("mfft_ew_profiles", F._plan, dx.ptr, dy.ptr, ncomp, nrows, M, _lib.precision_code(prec), center.ctypes.data_as(DP), out.ctypes.data_as(DP))
    check(dx, "ew_profiles x")
    check(dy, "ew_profiles y")
    _check_host(buf, out, g, "ew_profiles %s" % (shape,))
    c = center.reshape(2, ncomp).T
    want = np.stack([spectral.profile_rule(x[p], y[p], c[p]) for p in range(ncomp)])
    assert np.allclose(out, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,ncomp,nrows", [(16, 3, 301), (512, 3, 9), (768, 1, 5), (3072, 1, 3)])
def test_nlz_profile_rows_guarded(n, ncomp, nrows, prec):
    """mfft_nlz_profile_rows: pitched rows with poison between them, guard bands around the fields; a row past the end or a bin past
    `valid` that the kernel read would be a NaN in the transform -- every sum stays finite."""
    from mpifft4py_amd import _lib
    valid = n // 2 + 1
    pitch = valid + 5
    shape = (ncomp, nrows, valid)
    rng = np.random.default_rng(n + ncomp)
    draw = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
    da = guarded(shape, cdtype(prec), pitch=pitch, fill=draw())
    db = guarded(shape, cdtype(prec), pitch=pitch, fill=draw())
    center = np.linspace(-0.01, 0.01, 2 * ncomp)
    buf, out, g = _host_result(ncomp, n)
    _lib.call("mfft_nlz_profile_rows", da.ptr, db.ptr, ncomp, nrows, n, pitch, valid, 0, _lib.precision_code(prec),
              center.ctypes.data_as(DP), out.ctypes.data_as(DP))
    check(da, "nlz_profile_rows a")
    check(db, "nlz_profile_rows b")
    _check_host(buf, out, g, "nlz_profile_rows n=%d ncomp=%d" % (n, ncomp))
