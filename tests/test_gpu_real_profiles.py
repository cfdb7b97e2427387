"""GPU: plane-averaged profiles along z of spectral fields without the real-space arrays (mfft_real_profiles,
mfft_nlz_profile_rows, mfft_ew_profiles; csrc/nlz_prof.h NlzProf::body, csrc/profiles.hip) -- the sweep against the numpy rule, the z
stage on its own against numpy, the plan operation against the ORACLE's backward transforms of the same spectra on every route
(fused on one rank and several, batches, composed, pencils, pitched), `a_hat is b_hat`, `center`, known answers, the consistency
with `real_moments` and the example's --profiles.

Tolerances, per plane (the form of test_gpu_real_moments._check): tol = 4 TOL[prec] (0 for the sweep of real inputs), R the rows of
the plane, |.| the 2-norm of the WHOLE reference field, d the centred reference values of the plane in long double:
  sum d_a       tol sqrt(R) |a|                                   + (R + 8) 2^-52 sum |d_a|
  sum d_a^2     2 tol sqrt(sum d_a^2) |a|                         + (R + 8) 2^-52 sum d_a^2
  sum d_a d_b   tol (sqrt(sum d_b^2) |a| + sqrt(sum d_a^2) |b|)   + (R + 8) 2^-52 sum |d_a d_b|
the 4 TOL relative-L2 bound of a transform pushed through the sums by Cauchy-Schwarz, plus the bound of a double sum in any order."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
import test_gpu_real_moments as rm
from gpu_util import L, TOL, cdtype, have_gpu, rdtype, run_ranks
from test_gpu_real_moments import _irfft_rows, _reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
EPS = 2.0 ** -52
NAMES = ("sum d_a", "sum d_b", "sum d_a^2", "sum d_b^2", "sum d_a d_b")


def INFO(dealias):
    return "nonlinear_profiles_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


_WANT = {}


def _want(xa, xb, ca, cb, key=None):
    """(the five reference sums (5, M) in long double, their bounds' two terms (5, M) each, without tol) of one pair; xa, xb of
    shape (..., M).  `key`: computed once per key and shared between the tests."""
    k = (key, float(ca), float(cb))
    if key is not None and k in _WANT:
        return _WANT[k]
    M = xa.shape[-1]
    a, b = np.asarray(xa, dtype=np.float64).reshape(-1, M).astype(np.longdouble), np.asarray(xb, dtype=np.float64).reshape(-1, M).astype(np.longdouble)
    R = a.shape[0]
    na, nb = float(np.sqrt(np.sum(a * a))), float(np.sqrt(np.sum(b * b)))
    da, db = a - np.longdouble(ca), b - np.longdouble(cb)
    s = np.stack([da.sum(0), db.sum(0), (da * da).sum(0), (db * db).sum(0), (da * db).sum(0)])
    ra, rb = np.sqrt(s[2].astype(np.float64)), np.sqrt(s[3].astype(np.float64))
    first = np.stack([np.full(M, np.sqrt(R) * na), np.full(M, np.sqrt(R) * nb), 2 * ra * na, 2 * rb * nb, rb * na + ra * nb])
    mag = np.stack([np.abs(da).sum(0), np.abs(db).sum(0), s[2], s[3], np.abs(da * db).sum(0)]).astype(np.float64)
    res = (s, first, (R + 8) * EPS * mag)
    if key is not None:
        _WANT[k] = res
    return res


def _bounds(xa, xb, ca, cb, prec, spectral_input=True, key=None):
    s, first, second = _want(xa, xb, ca, cb, key)
    return s, (4 * TOL[prec] if spectral_input else 0.0) * first + second


def _check(sums, pairs, centers, prec, what, spectral_input=True, keys=None):
    """sums: (npairs, 5, M); pairs: [(xa, xb)] reference fields of shape (..., M); centers: (npairs, 2).  Every figure is printed
    before it is asserted: per sum the worst error over the planes, its bound there, and the worst ratio."""
    sums = np.asarray(sums, dtype=np.float64)
    assert sums.shape == (len(pairs), 5, pairs[0][0].shape[-1]), (sums.shape, len(pairs))
    for p, (xa, xb) in enumerate(pairs):
        ref, bound = _bounds(xa, xb, centers[p][0], centers[p][1], prec, spectral_input, keys[p] if keys is not None else None)
        err = np.abs(sums[p].astype(np.longdouble) - ref).astype(np.float64)
        for k in range(5):
            w = int(np.argmax(err[k] - bound[k]))
            print("profiles %s %s pair %d %-11s worst plane %d: err %.3e bound %.3e (max err / bound %.3g)"
                  % (what, prec, p, NAMES[k], w, err[k, w], bound[k, w], float(np.max(err[k] / np.maximum(bound[k], 1e-300)))))
        assert np.all(np.isfinite(sums[p])) and np.all(err <= bound), (what, p, np.argwhere(err > bound)[:4])


# ---- the sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15)])
def test_sweep_against_the_rule(shape, prec):
    """spectral.profiles of random real arrays against spectral.profile_rule within the summation term alone (the inputs are
    exact); two calls return identical bytes; (1, 7, 9, 15) has an odd row length and 63 rows."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(29 + shape[0])
    x = (3.0 * rng.standard_normal(shape) + 2.0).astype(rdtype(prec))
    y = (0.5 * rng.standard_normal(shape) - 1.0).astype(rdtype(prec))
    ncomp, M = shape[0], shape[-1]
    dx, dy = DeviceArray.from_numpy(x), DeviceArray.from_numpy(y)
    for center in (None, [[2.0, -1.0]] * ncomp if ncomp == 1 else [[2.0, -1.0], [0.0, 0.5], [-3.0, 7.0]]):
        h = spectral.profiles(F, dx, dy, center=center)
        c = np.zeros((ncomp, 2)) if center is None else np.asarray(center)
        assert h.count == shape[1] * shape[2] and h.sums.shape == (ncomp, 5, M) and np.array_equal(h.center, c)
        for p in range(ncomp):
            want = spectral.profile_rule(x[p], y[p], c[p])
            _, bound = _bounds(x[p], y[p], c[p][0], c[p][1], prec, spectral_input=False)
            err = np.abs(h.sums[p] - want)
            print("sweep %s %s center %s pair %d: max err / bound per sum %s" % (shape, prec, c[p], p, (err / bound).max(axis=1)))
            assert np.all(err <= bound), (shape, p, np.argwhere(err > bound)[:4])
        again = spectral.profiles(F, dx, dy, center=center)
        assert again.sums.tobytes() == h.sums.tobytes() and again.count == h.count
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    view = DeviceArray(dx.shape, dx.dtype, ptr=dx.ptr, owner=False)
    view.pitch = shape[-1] + 8
    with pytest.raises(ValueError):                  # pitched views are refused
        spectral.profiles(F, view, dy)
    with pytest.raises(ValueError):                  # a centre that is not finite
        spectral.profiles(F, dx, dy, center=(np.nan, 0.0))


# ---- the stage alone --------------------------------------------------------------------------------------------------
# One length of each build kind of the registry, as the moments tests list them: 16 and 512 wave-synchronous, 1024 a barrier build,
# 768 a 12-values plan, 3072 256 threads per row (in double precision the split exchange).
LENGTHS = [16, 512, 768, 1024, 3072]


def _rows_call(a, b, ncomp, nrows, n, pitch, valid, valid_in, prec, center):
    from mpifft4py_amd import DeviceArray, _lib
    da, db = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b)
    got = np.full((ncomp, 5, n), -7.0)
    c = np.ascontiguousarray(center, dtype=np.float64) if center is not None else None
    _lib.call("mfft_nlz_profile_rows", da.ptr, db.ptr, ncomp, nrows, n, pitch, valid, valid_in, _lib.precision_code(prec),
              c.ctypes.data_as(DP) if c is not None else None, got.ctypes.data_as(DP))
    assert da.get().tobytes() == a.tobytes() and db.get().tobytes() == b.tobytes()      # inputs preserved
    return got


def _stage(n, prec, nfields, nrows, valid, valid_in=0, center=None):
    """The draws of the moments test's _stage (a mean of 0.75 in every row); center: a_0.., then b_0..."""
    rng = np.random.default_rng(1000 * n + 10 * nrows % 1000 + valid + nfields)
    pitch = valid + 3
    ncomp = nfields // 2
    shape = (ncomp, nrows, pitch)
    draw = lambda: (np.sqrt(n) * (rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5))).astype(cdtype(prec))
    a, b = draw(), draw()
    for x in (a, b):
        x[..., 0] += n * 0.75
    got = _rows_call(a, b, ncomp, nrows, n, pitch, valid, valid_in, prec, center)
    vin = valid_in or valid
    ra, rb = _irfft_rows(a, n, vin), _irfft_rows(b, n, vin)
    c = np.zeros((ncomp, 2)) if center is None else np.asarray(center, dtype=np.float64).reshape(2, ncomp).T
    _check(got, [(ra[p], rb[p]) for p in range(ncomp)], c, prec, "stage n=%d nfields=%d nrows=%d valid=%d/%d" % (n, nfields, nrows, vin, valid))
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_nlz_profile_rows_against_numpy(n, prec):
    """mfft_nlz_profile_rows against numpy.fft.irfft of the rows in double: 2 and 6 fields, 37 rows and one, the n/2 + 1 bins and
    the n/3 + 1 of the 3/2-rule, pruned valid_in, centres; a second call gives the same bits."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage(n, prec, 6, 37, full)
    assert _stage(n, prec, 6, 37, full).tobytes() == first.tobytes()
    _stage(n, prec, 2, 37, lim, center=[0.75, 0.5])
    _stage(n, prec, 6, 37, full, valid_in=lim, center=[0.75, 0.5, 1.0, 0.0, 0.75, -2.0])
    _stage(n, prec, 2, 1, full)


@pytest.mark.parametrize("prec", ["double", "single"])
def test_nlz_profile_rows_more_than_two_passes_of_the_grid(prec):
    """n = 16: more than two passes of mfft_nlz_profile_groups workgroups and a ragged rest: every workgroup strides, the last pass
    is partial, and the fold adds every row slot of every workgroup."""
    from mpifft4py_amd import _lib
    code = _lib.precision_code(prec)
    cap = _lib.call("mfft_nlz_profile_groups", 1 << 40, 16, code)
    assert cap >= 1
    per = 1
    while _lib.call("mfft_nlz_profile_groups", per + 1, 16, code) == 1:      # rows per workgroup and pass: a power of two
        per *= 2
    nrows = 2 * cap * per + per // 2 + 3
    assert _lib.call("mfft_nlz_profile_groups", nrows, 16, code) == cap and nrows > 2 * cap * per and nrows % (cap * per) != 0
    _stage(16, prec, 2, nrows, 9, center=[0.75, 0.7])


def test_nlz_profile_rows_nonfinite_bins():
    """A NaN or an Inf bin in a_1 or in b_1: that field's `finite` is False and nothing else's; its partner's two own sums and
    every other pair have the bytes of the clean run -- the run with that bin zero, which is what the transform sees."""
    from mpifft4py_amd import spectral
    n, nrows, valid = 128, 5, 65
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    b = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    center = [0.1, 0.0, -0.1, 0.2, 0.0, 0.3]
    for bad in (np.nan, np.inf):
        for which in (0, 1):
            an, bn = a.copy(), b.copy()
            (an, bn)[which][1, 3, 7] = 0.0
            clean = _rows_call(an, bn, 3, nrows, n, valid, valid, 0, "double", center)
            assert np.all(np.isfinite(clean))
            (an, bn)[which][1, 3, 7] = bad
            got = _rows_call(an, bn, 3, nrows, n, valid, valid, 0, "double", center)
            h = spectral.Profiles(nrows, got, np.asarray(center).reshape(2, 3).T)
            want = np.ones((3, 2), dtype=bool)
            want[1, which] = False
            print("bad bin %r in %s_1: finite %s, NaNs per sum of the pair %s" % (bad, "ab"[which], h.finite.tolist(), np.isnan(got[1]).sum(axis=1)))
            assert np.array_equal(h.finite, want)
            assert got[1, 1 - which].tobytes() == clean[1, 1 - which].tobytes() and got[1, 3 - which].tobytes() == clean[1, 3 - which].tobytes()
            assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
            for s in (which, 2 + which, 4):
                assert np.isnan(got[1, s]).any() and not np.isinf(got[1, s]).any()


def test_error_cases_leave_the_outputs_untouched():
    """MFFT_ERR_UNSUPPORTED for a length without a kernel (stage call); MFFT_ERR_INVALID for ncomp outside {1, 3}, a NULL b, a centre
    that is not finite and valid > n / 2 + 1: the status codes themselves, out and count untouched."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    assert int(re.search(r"#define MFFT_PROFILE_STATS (\d+)", header).group(1)) == 5
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    out = np.full((3, 5, 128), -7.0)
    zero, nan, inf = np.zeros(6), np.array([0, 0, np.nan, 0, 0, 0.0]), np.array([0, 0, 0, 0, np.inf, 0.0])
    fn = getattr(_lib.load(), "mfft_nlz_profile_rows")

    def status(n, valid, ncomp, center, b=z.ptr):
        return fn(z.ptr, b, ncomp, 4, n, 65, valid, 0, _lib.DOUBLE, center.ctypes.data_as(DP), out.ctypes.data_as(DP))
    cases = [((100, 51, 3, zero), "MFFT_ERR_UNSUPPORTED"), ((128, 65, 2, zero), "MFFT_ERR_INVALID"), ((128, 65, 0, zero), "MFFT_ERR_INVALID"),
             ((128, 65, 3, nan), "MFFT_ERR_INVALID"), ((128, 65, 3, inf), "MFFT_ERR_INVALID"), ((64, 51, 3, zero), "MFFT_ERR_INVALID"),
             ((128, 65, 3, zero, None), "MFFT_ERR_INVALID")]
    for args, name in cases:
        rc = status(*args)
        print(args[:3], "->", rc)
        assert rc == codes[name], (args[:3], rc, name)
    assert np.all(out == -7.0)
    assert status(128, 65, 3, zero) == 0 and np.all(out == 0.0)                       # rows of zeros
    assert _lib.call("mfft_nlz_profile_groups", 4, 100, _lib.DOUBLE) == 0
    # the plan operation
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    d = F.empty_complex(3).set(np.zeros((3,) + tuple(F.complex_shape()), dtype=np.complex128))
    pout = np.full((3, 5, 32), -7.0)
    count = ctypes.c_int64(-5)
    pfn = getattr(_lib.load(), "mfft_real_profiles")
    F.comm.use_device()

    def pstatus(b, ncomp, center):
        return pfn(F._plan, d.ptr, b, ncomp, _DEALIAS[None], center.ctypes.data_as(DP), pout.ctypes.data_as(DP), ctypes.byref(count))
    for args in ((None, 3, zero), (d.ptr, 2, zero), (d.ptr, 3, nan), (d.ptr, 3, inf)):
        rc = pstatus(*args)
        print("plan", args[1], "->", rc)
        assert rc == codes["MFFT_ERR_INVALID"], (args[1], rc)
    assert np.all(pout == -7.0) and count.value == -5
    assert pstatus(d.ptr, 3, zero) == 0 and np.all(pout == 0.0) and count.value == 8 * 16


# ---- the plan operation, one rank ---------------------------------------------------------------------------------------
def _keys(N, prec, dealias, other="b"):
    return [(tuple(int(n) for n in N), prec, dealias, p, other) for p in range(3)]


def _call(F, a, b, ncomp, dealias, center=None, reduce=True, same=False):
    from mpifft4py_amd import spectral
    if ncomp == 1:
        da = F.empty_complex().set(a[0])
        db = da if same else F.empty_complex().set(b[0])
    else:
        da = F.empty_complex(3).set(a)
        db = da if same else F.empty_complex(3).set(b)
    return spectral.real_profiles(F, da, db, dealias, center, reduce), da, db


def _plan_case(F, N, prec, dealias, ncomp, fused, center=None):
    from mpifft4py_amd import spectral
    a, b, ua, ub = _reference(N, prec, dealias)
    h, da, db = _call(F, a, b, ncomp, dealias, center)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    M = ua.shape[-1]
    assert h.count == ua[0].size // M and h.sums.shape == (ncomp, 5, M) and h.M == M
    c = np.zeros((ncomp, 2)) if center is None else np.tile(np.asarray(center, dtype=np.float64), (ncomp, 1))
    assert np.array_equal(h.center, c) and h.finite.all()
    _check(h.sums, [(ua[p], ub[p]) for p in range(ncomp)], c, prec, "%s %s ncomp=%d" % (list(N), dealias, ncomp), keys=_keys(N, prec, dealias)[:ncomp])
    assert np.array_equal(da.get(), a[0] if ncomp == 1 else a) and np.array_equal(db.get(), b[0] if ncomp == 1 else b)      # inputs preserved
    again = spectral.real_profiles(F, da, db, dealias, center)
    assert again.sums.tobytes() == h.sums.tobytes() and again.count == h.count                                        # bitwise reproducible
    return h


@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,prec", [([24, 20, 32], "double"), ([24, 20, 32], "single"), ([48, 40, 96], "double")])
def test_real_profiles_one_rank_fused(N, prec, dealias, ncomp):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, ncomp, True, center=(0.01, -0.02) if ncomp == 3 else None)


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_a_hat_is_b_hat(dealias):
    """The same array as both fields: the two own sums are the same bits pairwise, and the cross sum is the sum of squares."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [24, 20, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, _, ua, _ = _reference(N, prec, dealias)
    h, da, db = _call(F, a, a, 3, dealias, center=(0.25, 0.25), same=True)
    assert da is db and F.plan_info(INFO(dealias)) == 1
    _check(h.sums, [(ua[p], ua[p]) for p in range(3)], [(0.25, 0.25)] * 3, prec, "a_hat is b_hat %s" % dealias, keys=_keys(N, prec, dealias, "a"))
    assert np.array_equal(da.get(), a)


def _var_bounds(xa, xb, ca, cb, prec):
    """Bounds of the plane variance of a and of the covariance formed from the raw sums of a call about (ca, cb): the bounds of the
    raw means pushed through var = m2 - m1^2, cov = m4 - m0 m1."""
    s, bound = _bounds(xa, xb, ca, cb, prec)
    R = xa.reshape(-1, xa.shape[-1]).shape[0]
    e, m = bound / R, np.abs(s.astype(np.float64)) / R
    return e[2] + 2 * m[0] * e[0] + e[0] ** 2, e[4] + m[0] * e[1] + m[1] * e[0] + e[0] * e[1]


@pytest.mark.parametrize("prec", ["double", "single"])
def test_center_keeps_the_digits_of_a_field_with_a_large_mean(prec):
    """A scalar of mean 300 and deviation 0.1 against a scalar of mean -40: the plane variances and covariances from the centres
    (300, -40) and from centre 0 agree within the bounds of the two calls pushed through the shift, those about the centre agree
    with the reference within THEIR bound alone -- and that bound is far below the centre-0 call's: the digits the centre keeps."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array([24, 20, 32])
    F = Slab_R2C(N, L, SelfComm(0), prec)
    rng = np.random.default_rng(21)
    x = 300.0 + 0.1 * rng.standard_normal(tuple(N))
    y = -40.0 + 0.05 * rng.standard_normal(tuple(N)) + 0.2 * (x - 300.0)
    hats = [np.fft.rfftn(v).astype(cdtype(prec)) for v in (x, y)]
    xr, yr = [np.fft.irfftn(v.astype(np.complex128), s=tuple(N), axes=(0, 1, 2)) for v in hats]      # the fields the (rounded) spectra stand for
    da, db = F.empty_complex().set(hats[0]), F.empty_complex().set(hats[1])
    h0 = spectral.real_profiles(F, da, db, None, center=None)
    hc = spectral.real_profiles(F, da, db, None, center=(300.0, -40.0))
    _check(h0.sums, [(xr, yr)], [(0.0, 0.0)], prec, "centre 0")
    _check(hc.sums, [(xr, yr)], [(300.0, -40.0)], prec, "centre (300, -40)")
    v0, c0 = _var_bounds(xr, yr, 0.0, 0.0, prec)
    vc, cc = _var_bounds(xr, yr, 300.0, -40.0, prec)
    var0, varc = np.asarray(h0.variance()[0], dtype=np.float64), np.asarray(hc.variance()[0], dtype=np.float64)
    cov0, covc = np.asarray(h0.covariance(), dtype=np.float64), np.asarray(hc.covariance(), dtype=np.float64)
    a2 = xr.reshape(-1, N[2])
    b2 = yr.reshape(-1, N[2])
    ref_var = a2.var(axis=0)
    ref_cov = ((a2 - a2.mean(0)) * (b2 - b2.mean(0))).mean(0)
    print("variance about 0: worst |diff to centre| %.3e bound %.3e; about the centre: err %.3e bound %.3e; bound ratio %.3g"
          % (np.abs(var0 - varc).max(), (v0 + vc).max(), np.abs(varc - ref_var).max(), vc.max(), (v0 / vc).min()))
    print("covariance about 0: worst |diff to centre| %.3e bound %.3e; about the centre: err %.3e bound %.3e"
          % (np.abs(cov0 - covc).max(), (c0 + cc).max(), np.abs(covc - ref_cov).max(), cc.max()))
    assert np.all(np.abs(var0 - varc) <= v0 + vc) and np.all(np.abs(cov0 - covc) <= c0 + cc)
    assert np.all(np.abs(varc - ref_var) <= vc) and np.all(np.abs(covc - ref_cov) <= cc)
    assert np.all(vc * 100 <= v0)                    # the centre's bound: at least two digits below the centre-0 call's
    mean = np.asarray(hc.mean(), dtype=np.float64)
    assert np.all(np.abs(mean[0] - a2.mean(0)) <= _bounds(xr, yr, 300.0, -40.0, prec)[1][0] / a2.shape[0] + 4 * EPS * 300.0)


def test_real_profiles_pitched_plan_with_nans_between_rows():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert F.complex_pitch > F.complex_shape()[-1]
    for dealias in ("3/2-rule", "2/3-rule", None):
        a, b, ua, ub = _reference(N, prec, dealias)
        da, db = F.empty_complex(3), F.empty_complex(3)
        for d in (da, db):                                                         # NaNs between the rows
            whole = DeviceArray(d.shape[:-1] + (F.complex_pitch,), d.dtype, ptr=d.ptr, owner=False)
            whole.set(np.full(whole.shape, np.nan + 1j * np.nan, dtype=d.dtype))
        da.set(a), db.set(b)
        h = spectral.real_profiles(F, da, db, dealias)
        assert F.plan_info(INFO(dealias)) == 1
        _check(h.sums, [(ua[p], ub[p]) for p in range(3)], np.zeros((3, 2)), prec, "pitched %s" % dealias, keys=_keys(N, prec, dealias))


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    """(the cases and their checks are this module's own: the child imports it beside nonlinear_util)"""
    return nl.run_child("import test_gpu_real_profiles as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_real_profiles_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB: 60 padded x planes in several batches, the last one ragged; the plane
    sums accumulate over the batches."""
    _child("""
N = [40, 32, 64]
F = Slab_R2C(np.array(N), L, SelfComm(0), 'double')
for ncomp in (3, 1):
    t._plan_case(F, N, 'double', '3/2-rule', ncomp, True, center=(0.02, -0.01))
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_real_profiles_composed_kill_switch():
    """MFFT_NO_NLZ=1: a pair at a time through the plan's inverse transform into TWO real work arrays and the sweep; [16, 32, 24]
    and [20, 24, 40] (no fused kernels for 24 / 36, 40 / 60 either)."""
    _child("""
for N in ([16, 32, 24], [20, 24, 40]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for ncomp in (3, 1):
                t._plan_case(F, N, prec, dealias, ncomp, False, center=(0.01, 0.0) if ncomp == 3 else None)
print('ok')
""", MFFT_NO_NLZ="1")


def test_real_profiles_z_length_without_a_kernel():
    """[24, 40, 20]: no fused kernel of 20 or 30 points: the composed route inside the plan, flag 0."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N = [24, 40, 20]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    for dealias in ("3/2-rule", None):
        _plan_case(F, N, "double", dealias, 3, False, center=(0.0, 0.1))


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_real_profiles_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan, flag 0): every rank's profiles against the real fields its own
    ifftn gives, the reduced ones against all of them together; the same bits on every rank."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 24])

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(50 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a, b = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.25), x.component(i))
        u = DeviceArray.empty(ws, F.float)
        mine = []
        for x in (a, b):
            for i in range(3):
                F.ifftn(x.component(i), u, dealias)
                mine.append(u.get().astype(np.float64))
        local = spectral.real_profiles(F, a, b, dealias, center=(0.25, 0.2), reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == mine[0].size // mine[0].shape[-1]
        _check(local.sums, [(mine[p], mine[3 + p]) for p in range(3)], [(0.25, 0.2)] * 3, "double", "pencil rank %d" % comm.Get_rank())
        glob = spectral.real_profiles(F, a, b, dealias, center=(0.25, 0.2))
        return mine, local.sums, glob.sums, glob.count

    res = run_ranks(4, work)
    M = res[0][0][0].shape[-1]
    whole = [np.concatenate([r[0][f].reshape(-1, M) for r in res]) for f in range(6)]
    for _, _, g, cnt in res:
        assert cnt == whole[0].shape[0] and g.tobytes() == res[0][2].tobytes()
        _check(g, [(whole[p], whole[3 + p]) for p in range(3)], [(0.25, 0.2)] * 3, "double", "pencils, reduced")
    assert np.array_equal(np.sum([r[1] for r in res], 0), res[0][2])               # (rank order: what allreduce adds)


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("P", [2, 4])
def test_real_profiles_ranks_fused(P, dealias):
    """2 and 4 slab ranks: every rank's profiles against its own x planes of the one-rank reference, the reduced ones against the
    whole reference; `count` sums to Nx Ny (of the padded grid under the 3/2-rule)."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = [24, 20, 32]
    a, b, ua, ub = _reference(N, "double", dealias)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_profiles(F, da, db, dealias, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_profiles(F, da, db, dealias)
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return local.sums, local.count, glob.sums, glob.count

    out = run_ranks(P, work)
    planes = ua.shape[1] // P                                                      # a rank holds the sums of its own x planes
    for r, (local, lcount, glob, gcount) in enumerate(out):
        mine = [(ua[p][r * planes:(r + 1) * planes], ub[p][r * planes:(r + 1) * planes]) for p in range(3)]
        assert lcount == planes * ua.shape[2] and gcount == ua.shape[1] * ua.shape[2]
        _check(local, mine, np.zeros((3, 2)), "double", "%s P=%d %s rank %d" % (N, P, dealias, r))
        _check(glob, [(ua[p], ub[p]) for p in range(3)], np.zeros((3, 2)), "double", "%s P=%d %s reduced" % (N, P, dealias), keys=_keys(N, "double", dealias))
        assert glob.tobytes() == out[0][2].tobytes()                               # equal on all ranks
    assert sum(o[1] for o in out) == ua.shape[1] * ua.shape[2]
    assert np.array_equal(np.sum(np.stack([o[0] for o in out]), 0), out[0][2])     # local sums add up to the reduced ones


# ---- known answers, consistency ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_known_profiles(dealias):
    """a = cos z (1 + cos x), b = sin 2z + cos y, set as a few modes: <a> = cos z, <b> = sin 2z, <a^2> = (3/2) cos^2 z, <a b> =
    cos z sin 2z.  Then Taylor-Green: <u_x> = 0, <u_x^2> = cos^2 z / 4, <u_x u_y> = 0.  All within 1e-10."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    n3 = float(np.prod(N))
    cs = tuple(F.complex_shape())
    a, b = np.zeros(cs, dtype=np.complex128), np.zeros(cs, dtype=np.complex128)
    a[0, 0, 1] = 0.5 * n3                              # cos z
    a[1, 0, 1] = a[-1, 0, 1] = 0.25 * n3               # cos x cos z
    b[0, 0, 2] = -0.5j * n3                            # sin 2z
    b[0, 1, 0] = b[0, -1, 0] = 0.5 * n3                # cos y
    h = spectral.real_profiles(F, F.empty_complex().set(a), F.empty_complex().set(b), dealias)
    assert F.plan_info(INFO(dealias)) == 1
    M = h.M
    z = np.arange(M) * 2 * np.pi / M
    assert np.allclose(h.z(F), z, rtol=0, atol=1e-14) and h.count == (M * M if dealias == "3/2-rule" else 32 * 32)
    mean, flux = np.asarray(h.mean(), dtype=np.float64), np.asarray(h.flux(), dtype=np.float64)
    a2 = h.sums[0, 2] / h.count
    errs = [np.abs(mean[0] - np.cos(z)).max(), np.abs(mean[1] - np.sin(2 * z)).max(), np.abs(a2 - 1.5 * np.cos(z) ** 2).max(),
            np.abs(flux - np.cos(z) * np.sin(2 * z)).max()]
    print("known profiles (%s): errors of <a>, <b>, <a^2>, <a b>: %s" % (dealias, errs))
    assert max(errs) <= 1e-10, errs
    x = np.arange(32) * 2 * np.pi / 32
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    U = F.empty_complex(3)
    for f, u in enumerate((np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X))):
        F.fftn(DeviceArray.from_numpy(u), U.component(f))
    t = spectral.real_profiles(F, U.component(0), U.component(1), dealias)
    errs = [np.abs(np.asarray(t.mean(), dtype=np.float64)).max(), np.abs(t.sums[0, 2] / t.count - np.cos(z) ** 2 / 4).max(),
            np.abs(np.asarray(t.flux(), dtype=np.float64)).max()]
    print("Taylor-Green (%s): errors of <u_x>, <u_x^2>, <u_x u_y>: %s" % (dealias, errs))
    assert max(errs) <= 1e-10, errs


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_profile_sums_add_up_to_the_moments(dealias, prec):
    """The sum over z of the profile sums equals S1 and S2 of `real_moments` of the same fields about the same centres, within
    the sum of the bounds of the two calls."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = [24, 20, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua, ub = _reference(N, prec, dealias)
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    c = (0.01, -0.02)
    h = spectral.real_profiles(F, da, db, dealias, center=c)
    m = spectral.real_moments(F, da, db, dealias, center=[c[0]] * 3 + [c[1]] * 3)
    for p in range(3):
        _, bound = _bounds(ua[p], ub[p], c[0], c[1], prec, key=_keys(N, prec, dealias)[p])
        for f, x, s1, s2 in ((p, ua[p], 0, 2), (3 + p, ub[p], 1, 3)):
            _, _, first, second = rm._want(x, c[f // 3])
            mb = [4 * TOL[prec] * first[k] + second[k] for k in (0, 1)]
            for k, s in ((0, s1), (1, s2)):
                got, want, bd = float(h.sums[p, s].sum()), float(m.sums[f, k]), float(bound[s].sum()) + mb[k] + 40 * EPS * float(np.abs(h.sums[p, s]).sum())
                print("consistency %s %s field %d S%d: profiles %.12e moments %.12e |diff| %.3e bound %.3e" % (dealias, prec, f, k + 1, got, want, abs(got - want), bd))
                assert abs(got - want) <= bd
    assert h.count * h.M == m.count


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_profiles():
    exe = [sys.executable, os.path.join(ROOT, "examples", "boussinesq_device.py"), "--N", "32", "--steps", "2", "--profiles"]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("profiles step")]
    assert len(lines) == 2, r.stdout
    for l in lines:
        groups = re.findall(r"\[([^\]]+)\]", l)
        assert len(groups) == 3 and all(len(g.split(",")) == 5 for g in groups), l
        vals = np.array([float(v) for g in groups for v in g.split(",")])
        assert np.all(np.isfinite(vals)), l
        m = re.search(r"plane-mean <u_z theta> = (\S+)\s+box <u_z theta> = (\S+)", l)
        assert m, l
        pm, box = float(m.group(1)), float(m.group(2))
        assert abs(pm - box) <= 1e-10 * max(1.0, abs(box)), (pm, box)
