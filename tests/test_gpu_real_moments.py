"""GPU: one-point statistics of spectral fields without the real-space arrays (mfft_real_moments, mfft_nlz_moments_rows,
mfft_ew_moments, mfft_ew_diag_grad_hat; csrc/nlz_moments.h NlzMoments::body, csrc/moments.hip) -- the z stage on its own against numpy,
the plan operation against the ORACLE's backward transforms of the same spectra on every route (fused on one rank and several,
batches, composed, pencils, pitched), spectral.moments, the Taylor-Green known answer, `center`, and the example's --stats.

Tolerances, with x the reference field in float64, cnt its points, d = x - center and TOL = gpu_util.TOL:
  min / max            4 TOL[prec] max|x|                      (the maxima tests' bound)
  S_p from spectra     4 TOL[prec] p sqrt(sum d^(2(p-1)) sum x^2) + (cnt + 8) 2^-52 sum |d|^p
                       the 4 TOL relative-L2 bound of a padded transform pushed through x -> (x - c)^p by Cauchy-Schwarz
                       (|delta (d^p)| <= p |d|^(p-1) |delta x| to first order), plus the shell-sum tests' bound for a double
                       sum in any order; for center = 0 it is the bound with x in place of d
  sweep on real arrays the second term alone, against a long-double numpy sum (the inputs are exact)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, TOL, cdtype, have_gpu, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
DP = ctypes.POINTER(ctypes.c_double)


def INFO(dealias):
    return "nonlinear_moments_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


_WANT = {}


def _want(x, center, key=None):
    """[min, max, S1..S4] of one field in long double, and the quantities of the bounds.  `key`: computed once per key and shared."""
    if key is not None and (key, float(center)) in _WANT:
        return _WANT[(key, float(center))]
    x = np.asarray(x, dtype=np.float64).ravel()
    xl = x.astype(np.longdouble)
    d = xl - np.longdouble(center)
    d2 = d * d
    d3 = d2 * d
    s = [np.sum(d), np.sum(d2), np.sum(d3), np.sum(d2 * d2)]
    sabs = [float(np.sum(np.abs(d))), float(s[1]), float(np.sum(np.abs(d3))), float(s[3])]
    s2p = [float(x.size), float(s[1]), float(s[3]), float(np.sum(d3 * d3))]           # sum d^(2 (p - 1))
    sx2 = float(np.sum(xl * xl))
    first = [p * np.sqrt(s2p[p - 1] * sx2) for p in (1, 2, 3, 4)]
    second = [(x.size + 8) * 2.0 ** -52 * sabs[p - 1] for p in (1, 2, 3, 4)]
    res = ([x.min(), x.max()] + s, float(np.abs(x).max()), first, second)
    if key is not None:
        _WANT[(key, float(center))] = res
    return res


def _check(raw, fields, centers, prec, what, spectral_input=True, keys=None):
    """raw: (nfields, 6) [min, max, S1..S4]; fields: the reference fields (keys: names under which their reference sums are
    shared between tests); every figure is printed before it is asserted."""
    raw = np.asarray(raw, dtype=np.float64).reshape(len(fields), 6)
    for f, x in enumerate(fields):
        ref, amax, first, second = _want(x, centers[f], keys[f] if keys is not None else None)
        tol = 4 * TOL[prec] if spectral_input else 0.0
        bounds = [tol * amax, tol * amax] + [tol * a + b for a, b in zip(first, second)]
        errs = [abs(float(np.longdouble(raw[f, k]) - ref[k])) for k in range(6)]
        print("moments %s %s field %d\n  got   %s\n  err   %s\n  bound %s" % (what, prec, f, raw[f], errs, bounds))
        assert all(np.isfinite(raw[f])) and all(e <= b for e, b in zip(errs, bounds)), (what, f, raw[f], errs, bounds)


# ---- the stage alone --------------------------------------------------------------------------------------------------
# One length of each build kind of the registry (registry_nlz.h nlz_rows / nlz_wave / nlz_split), as the maxima test chooses them:
#   16    two threads per row, 32 rows per wave (wave-synchronous)         512   64 threads per row: one row per wave
#   1024  128 threads per row: two waves per row (barrier build)           768   a 12-values plan (64 threads per row)
#   3072  256 threads per row; in double precision the split (real / imaginary) exchange
def _irfft_rows(x, n, vin):
    x = x[..., :vin].astype(np.complex128)
    x[..., 0] = x[..., 0].real
    if vin == n // 2 + 1 and n % 2 == 0:
        x[..., -1] = x[..., -1].real
    return np.fft.irfft(x, n=n, axis=-1)


def _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, center):
    from mpifft4py_amd import DeviceArray, _lib
    da = DeviceArray.from_numpy(a)
    db = DeviceArray.from_numpy(b) if b is not None else None
    got = np.zeros(nfields * 6)
    c = np.ascontiguousarray(center, dtype=np.float64) if center is not None else None
    _lib.call("mfft_nlz_moments_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, valid_in,
              _lib.precision_code(prec), c.ctypes.data_as(DP) if c is not None else None, got.ctypes.data_as(DP))
    assert da.get().tobytes() == a.tobytes() and (b is None or db.get().tobytes() == b.tobytes())      # inputs preserved
    return got.reshape(nfields, 6)


def _stage(n, prec, nfields, nrows, valid, valid_in=0, center=None):
    rng = np.random.default_rng(1000 * n + 10 * nrows + valid + nfields)
    pitch = valid + 3
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = ((ncomp,) if nfields > 2 else ()) + (nrows, pitch)
    draw = lambda: (np.sqrt(n) * (rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5))).astype(cdtype(prec))
    a = draw()
    b = draw() if nfields % 2 == 0 else None
    for x in (a, b):
        if x is not None:
            x[..., 0] += n * 0.75                      # a mean of 0.75 in every row
    got = _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, center)
    vin = valid_in or valid
    fields = [r for x in (a, b) if x is not None for r in _irfft_rows(x.reshape((ncomp, nrows, pitch)), n, vin)]
    _check(got, fields, center if center is not None else [0.0] * nfields, prec,
           "stage n=%d nfields=%d nrows=%d valid=%d/%d" % (n, nfields, nrows, vin, valid))
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [16, 512, 1024, 3072, 768])
def test_nlz_moments_rows_against_numpy(n, prec):
    """mfft_nlz_moments_rows against numpy.fft.irfft of the rows in double: 37 rows and one, the n/2 + 1 bins and the n/3 + 1 of
    the 3/2-rule, pruned valid_in, field counts 6, 1, 3 and 2, a centre; a second call gives the same bits."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage(n, prec, 6, 37, full)
    assert _stage(n, prec, 6, 37, full).tobytes() == first.tobytes()
    _stage(n, prec, 1, 1, lim)
    _stage(n, prec, 3, 37, lim, center=[0.75, 0.5, 1.0])
    _stage(n, prec, 2, 1, full, valid_in=lim, center=[0.75, 0.0])


@pytest.mark.parametrize("prec", ["double", "single"])
def test_nlz_moments_rows_more_than_one_pass_of_the_grid(prec):
    """n = 16: the launch has at most mfft_nlz_moments_groups workgroups of 2 x 128 rows; twice that many rows and a ragged rest,
    so every workgroup strides and the last pass is partial."""
    from mpifft4py_amd import _lib
    cap = _lib.call("mfft_nlz_moments_groups", 1 << 40, 16, _lib.precision_code(prec))
    assert cap >= 1
    nrows = 2 * cap * 256 + 333
    assert _lib.call("mfft_nlz_moments_groups", nrows, 16, _lib.precision_code(prec)) == cap
    _stage(16, prec, 1, nrows, 9, center=[0.75])


def test_nlz_moments_rows_nan_inf_and_unsupported():
    from mpifft4py_amd import DeviceArray, _lib
    n, nrows, valid = 128, 5, 65
    rng = np.random.default_rng(3)
    a = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    b = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    fields = list(_irfft_rows(a, n, valid)) + list(_irfft_rows(b, n, valid))
    keep = [0, 2, 3, 4, 5]
    a[1, 3, 7] = np.nan
    got = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", None)
    # a_1 holds the NaN: NaN in all six of ITS statistics, b_1 (the other half of its transform) among the five that are right
    assert np.all(np.isnan(got[1])), got
    _check(got[keep], [fields[i] for i in keep], [0.0] * 5, "double", "beside a NaN")
    a[1, 3, 7] = np.inf
    got = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", None)
    assert np.all(np.isnan(got[1, 2:])) and (np.isnan(got[1, 0]) or got[1, 0] == -np.inf) and (np.isnan(got[1, 1]) or got[1, 1] == np.inf), got
    _check(got[keep], [fields[i] for i in keep], [0.0] * 5, "double", "beside an Inf")
    z = DeviceArray.zeros((3, 4, 51), np.complex128)
    out = np.zeros(36)
    with pytest.raises(_lib.MfftError):                # 100 has no fused kernel
        _lib.call("mfft_nlz_moments_rows", z.ptr, z.ptr, 6, 4, 100, 51, 51, 0, _lib.DOUBLE, None, out.ctypes.data_as(DP))
    with pytest.raises(_lib.MfftError):                # more bins than a row of 64 points has
        _lib.call("mfft_nlz_moments_rows", z.ptr, z.ptr, 6, 4, 64, 51, 51, 0, _lib.DOUBLE, None, out.ctypes.data_as(DP))
    with pytest.raises(_lib.MfftError):                # four fields are not a call
        _lib.call("mfft_nlz_moments_rows", z.ptr, z.ptr, 4, 4, 128, 51, 51, 0, _lib.DOUBLE, None, out.ctypes.data_as(DP))


# ---- the plan operation, one rank ---------------------------------------------------------------------------------------
_REF = {}


def _reference(N, prec, dealias):
    """Seeded spectra (those of the maxima tests: seed 11 + N2) and the oracle's six real fields, computed once."""
    key = (tuple(int(n) for n in N), prec, dealias)
    if key not in _REF:
        from mpifft4py_amd import LayoutComm
        from mpifft4py_amd.slab import R2C
        N = np.array(N)
        F = R2C(N, L, LayoutComm(1, 0), prec)
        a, b = nl.spectra(tuple(F.complex_shape()), N, prec, 11 + int(N[2]), True)
        mask = F.get_dealias_filter() if dealias == "2/3-rule" else None
        _REF[key] = (a, b, nl.oracle_back(a, N, prec, dealias, mask), nl.oracle_back(b, N, prec, dealias, mask))
    return _REF[key]


def _keys(N, prec, dealias):
    return [(tuple(int(n) for n in N), prec, dealias, f) for f in range(6)]


def _raw(m):
    return np.concatenate([m.min[:, None], m.max[:, None], m.sums], axis=1)


def _call(F, a, b, nfields, dealias, center=None, reduce=True):
    """real_moments of the first `nfields` of (a, b): 1: a[0]; 3: a; 6: a and b.  Returns (Moments, the device inputs)."""
    from mpifft4py_amd import spectral
    if nfields == 1:
        da, db = F.empty_complex().set(a[0]), None
    else:
        da, db = F.empty_complex(3).set(a), (F.empty_complex(3).set(b) if nfields == 6 else None)
    return spectral.real_moments(F, da, db, dealias, center, reduce), da, db


def _plan_case(F, N, prec, dealias, nfields, fused, center=None):
    a, b, ua, ub = _reference(N, prec, dealias)
    m, da, db = _call(F, a, b, nfields, dealias, center)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    fields = (list(ua) + list(ub))[:nfields]
    assert m.count == fields[0].size and m.min.shape == m.max.shape == (nfields,) and m.sums.shape == (nfields, 4)
    c = np.zeros(nfields) if center is None else np.asarray(center, dtype=np.float64) * np.ones(nfields)
    _check(_raw(m), fields, c, prec, "%s %s nfields=%d" % (list(N), dealias, nfields), keys=_keys(N, prec, dealias)[:nfields])
    assert np.array_equal(da.get(), a[0] if nfields == 1 else a) and (db is None or np.array_equal(db.get(), b))      # inputs preserved
    from mpifft4py_amd import spectral
    again = spectral.real_moments(F, da, db, dealias, center)
    assert _raw(again).tobytes() == _raw(m).tobytes() and again.count == m.count                                      # bitwise reproducible
    return m


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_moments_one_rank_fused(N, dealias, nfields, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, nfields, True, center=0.01 if nfields == 3 else None)


def test_real_moments_pitched_plan_with_nans_between_rows():
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
        m = spectral.real_moments(F, da, db, dealias)
        assert F.plan_info(INFO(dealias)) == 1
        _check(_raw(m), list(ua) + list(ub), np.zeros(6), prec, "pitched %s" % dealias, keys=_keys(N, prec, dealias))


def test_real_moments_nan_marks_its_field_only():
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua, ub = _reference(N, prec, None)
    an = a.copy()
    an[2, 3, 5, 7] = np.nan
    m, _, _ = _call(F, an, b, 6, None)
    raw = _raw(m)
    assert np.all(np.isnan(raw[2])), raw
    keep = [0, 1, 3, 4, 5]
    _check(raw[keep], [(list(ua) + list(ub))[i] for i in keep], np.zeros(5), prec, "beside a NaN field")
    assert np.all(np.isnan(m.skewness()[2])) and np.all(np.isfinite(m.flatness()[keep].astype(np.float64)))


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    """(the cases and their checks are this module's own: the child imports it beside nonlinear_util)"""
    return nl.run_child("import test_gpu_real_moments as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_real_moments_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB: 60 padded x planes in nine or ten batches, the last one ragged; the
    statistics accumulate over the batches.  Six fields (152 kB of rows per plane) and one (more planes per batch)."""
    _child("""
N = [40, 32, 64]
F = Slab_R2C(np.array(N), L, SelfComm(0), 'double')
for nfields in (6, 1, 3):
    t._plan_case(F, N, 'double', '3/2-rule', nfields, True, center=0.02)
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_real_moments_composed_kill_switch():
    """MFFT_NO_NLZ=1: one field at a time through the plan's inverse transform into ONE real work array and the sweep; [16, 32, 24]
    and [20, 24, 40] (no fused kernels for 24 / 36, 40 / 60 either).  The plan's nonlinear buffers hold that one array: the padded
    real field of the 3/2-rule, the first mode run."""
    _child("""
for N in ([16, 32, 24], [20, 24, 40]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for nfields in (6, 1, 3):
                t._plan_case(F, N, prec, dealias, nfields, False, center=0.01 if nfields == 6 else None)
            one = int(np.prod([3 * n // 2 for n in N])) * (8 if prec == 'double' else 4)
            assert F.plan_info('nonlinear_bytes') == one, (F.plan_info('nonlinear_bytes'), one)
print('ok')
""", MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_real_moments_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan, flag 0): every rank's statistics against the real fields its
    own ifftn gives, the reduced ones against all of them together; the same bits on every rank."""
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
                s = spectral.moments(F, u, center=0.25)
                _check(_raw(s), [mine[-1]], [0.25], "double", "sweep, pencil rank %d" % comm.Get_rank(), spectral_input=False)
        local = spectral.real_moments(F, a, b, dealias, center=0.25, reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == mine[0].size
        _check(_raw(local), mine, [0.25] * 6, "double", "pencil rank %d" % comm.Get_rank())
        glob = spectral.real_moments(F, a, b, dealias, center=0.25)
        return mine, _raw(local), _raw(glob), glob.count

    res = run_ranks(4, work)
    whole = [np.concatenate([r[0][f].ravel() for r in res]) for f in range(6)]
    for _, _, g, cnt in res:
        assert cnt == whole[0].size and g.tobytes() == res[0][2].tobytes()
        _check(g, whole, [0.25] * 6, "double", "pencils, reduced")
    assert np.array_equal(np.sum([r[1][:, 2:] for r in res], 0), res[0][2][:, 2:])      # (rank order: what allreduce adds)


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,P", [([32, 64, 128], 2), ([32, 64, 128], 4), ([8, 16, 32], 2), ([8, 16, 32], 4)])
def test_real_moments_ranks_fused(N, P, dealias):
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua, ub = _reference(N, "double", dealias)
    fields = list(ua) + list(ub)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_moments(F, da, db, dealias, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_moments(F, da, db, dealias)
        three = spectral.real_moments(F, da, None, dealias)
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return _raw(local), local.count, _raw(glob), glob.count, _raw(three)

    out = run_ranks(P, work)
    planes = ua.shape[1] // P                                                      # a rank holds the statistics of its own x planes
    for r, (local, lcount, glob, gcount, three) in enumerate(out):
        mine = [x[r * planes:(r + 1) * planes] for x in fields]
        assert lcount == mine[0].size and gcount == fields[0].size
        _check(local, mine, np.zeros(6), "double", "%s P=%d %s rank %d" % (N, P, dealias, r))
        _check(glob, fields, np.zeros(6), "double", "%s P=%d %s reduced" % (N, P, dealias), keys=_keys(N, "double", dealias))
        _check(three, fields[:3], np.zeros(3), "double", "%s P=%d %s three fields" % (N, P, dealias), keys=_keys(N, "double", dealias)[:3])
        assert glob.tobytes() == out[0][2].tobytes()                               # equal on all ranks
    stack = np.stack([o[0] for o in out])
    assert np.array_equal(np.sum(stack[:, :, 2:], 0), out[0][2][:, 2:])            # local sums add up to the reduced ones
    assert np.array_equal(stack[:, :, 0].min(0), out[0][2][:, 0]) and np.array_equal(stack[:, :, 1].max(0), out[0][2][:, 1])


# ---- spectral.moments -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_spectral_moments(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(4)
    shape = (7, 9, 11)                              # 693 elements: odd, so components 1 and 2 of a (3, ...) fp32 array start off 16 bytes
    x = (rng.random(shape) - 0.3).astype(rdtype(prec))
    for where in (0, 692, 333):
        x.reshape(-1)[where] = -3.25
        m = spectral.moments(F, DeviceArray.from_numpy(x))
        assert m.count == 693 and m.min[0] == -3.25 and m.sums.shape == (1, 4)
        _check(_raw(m), [x], [0.0], prec, "sweep %s" % (shape,), spectral_input=False)
    v = (rng.random((3,) + shape) - 0.3).astype(rdtype(prec))
    v[1].reshape(-1)[0] = 2.5
    v[2].reshape(-1)[692] = -4.5
    c = [0.2, 0.0, -1.0]
    m = spectral.moments(F, DeviceArray.from_numpy(v), center=c)
    assert m.max[1] == 2.5 and m.min[2] == -4.5 and m.count == 693
    _check(_raw(m), list(v), c, prec, "sweep (3, 7, 9, 11)", spectral_input=False)
    big = (rng.random((3, 64, 64, 65)) - 0.5).astype(rdtype(prec))     # more than one vector per lane, odd rows
    m = spectral.moments(F, DeviceArray.from_numpy(big), center=0.1)
    _check(_raw(m), list(big), [0.1] * 3, prec, "sweep (3, 64, 64, 65)", spectral_input=False)
    again = spectral.moments(F, DeviceArray.from_numpy(big), center=0.1)
    assert _raw(again).tobytes() == _raw(m).tobytes()
    x = np.zeros(shape, dtype=rdtype(prec))
    assert np.array_equal(_raw(spectral.moments(F, DeviceArray.from_numpy(x))), np.zeros((1, 6)))
    x[3, 4, 5] = np.nan
    assert np.all(np.isnan(_raw(spectral.moments(F, DeviceArray.from_numpy(x)))))
    x[3, 4, 5] = -np.inf
    r = _raw(spectral.moments(F, DeviceArray.from_numpy(x)))[0]
    assert r[0] == -np.inf and r[1] == 0.0 and r[2] == -np.inf and r[3] == np.inf and r[4] == -np.inf and r[5] == np.inf, r
    two = DeviceArray.from_numpy(np.zeros((2, 4, 4, 6), dtype=rdtype(prec)))
    pitched = DeviceArray(two.shape, two.dtype, ptr=two.ptr, owner=False)
    pitched.pitch = 8
    with pytest.raises(ValueError):
        spectral.moments(F, pitched)


# ---- known answer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_taylor_green_known_moments(dealias):
    """u = (sin x cos y cos z, -cos x sin y cos z, 0) at N = 32.  u_0: mean 0, <u^2> = 1/8, <u^3> = 0, <u^4> = 27/512, flatness 27/8,
    min -1, max 1; omega_2 = 2 sin x sin y cos z: <w^2> = 1/2, <w^4> = 27/32; all within 1e-10 (x = pi / 2 lies on the 32- and on
    the 48-point grid)."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    x = np.arange(32) * 2 * np.pi / 32
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    U = F.empty_complex(3)
    for f, u in enumerate((np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X))):
        F.fftn(DeviceArray.from_numpy(u), U.component(f))
    K = spectral.Wavenumbers(F)
    W = F.empty_complex(3)
    spectral.curl_hat(F, K, U, W)
    m = spectral.real_moments(F, U, W, dealias)
    assert F.plan_info(INFO(dealias)) == 1
    mean = m.sums / m.count
    print("Taylor-Green (%s): min %s max %s\n  raw moments %s\n  flatness %s" % (dealias, m.min, m.max, mean, m.flatness()))
    assert np.all(np.abs(mean[0] - [0.0, 0.125, 0.0, 27.0 / 512]) <= 1e-10), mean[0]
    assert abs(float(m.flatness()[0]) - 27.0 / 8) <= 1e-10 and abs(float(m.mean()[0])) <= 1e-10 and abs(float(m.skewness()[0])) <= 1e-10
    assert abs(m.min[0] + 1.0) <= 1e-10 and abs(m.max[0] - 1.0) <= 1e-10
    assert abs(mean[5, 1] - 0.5) <= 1e-10 and abs(mean[5, 3] - 27.0 / 32) <= 1e-10 and abs(m.max[5] - 2.0) <= 1e-10
    # the longitudinal derivatives: du_0/dx_0 = cos x cos y cos z, <.^2> = 1/8, flatness 27/8; du_2/dx_2 = 0
    G = F.empty_complex(3)
    spectral.diag_grad_hat(F, K, U, G)
    g = spectral.real_moments(F, G, None, dealias)
    assert abs(float(g.variance()[0]) - 0.125) <= 1e-10 and abs(float(g.flatness()[1]) - 27.0 / 8) <= 1e-10 and abs(float(g.skewness()[0])) <= 1e-10
    assert g.min[2] == 0.0 and g.max[2] == 0.0
    ref = (1j * np.asarray(K.dev[0].get()).reshape(-1, 1, 1)[:, :, :] * U.get()[0])
    assert np.allclose(G.get()[0], ref, rtol=0, atol=1e-12 * np.abs(ref).max())


# ---- center -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_center_keeps_the_digits_of_a_field_with_a_mean(prec):
    """A scalar of mean 3: the central moments from center = 3 and from center = 0 agree within the bounds of the two calls pushed
    through the shift (mu_p is a polynomial in the raw moments; the bound of every term is added), and mean() is a_hat[0, 0, 0] / N^3."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), prec)
    rng = np.random.default_rng(21)
    x = 3.0 + 0.5 * (rng.random(tuple(N)) ** 2 - 1.0 / 3)
    a_hat = np.fft.rfftn(x).astype(cdtype(prec))
    xr = np.fft.irfftn(a_hat.astype(np.complex128), s=tuple(N), axes=(0, 1, 2))          # the field the (rounded) spectrum stands for
    d = F.empty_complex().set(a_hat)
    m0 = spectral.real_moments(F, d, None, None, center=None)
    m3 = spectral.real_moments(F, d, None, None, center=3.0)
    _check(_raw(m0), [xr], [0.0], prec, "centre 0")
    _check(_raw(m3), [xr], [3.0], prec, "centre 3")
    n = float(np.prod(N))
    mean = float(a_hat[0, 0, 0].real) / n
    for m in (m0, m3):
        assert abs(float(m.mean()[0]) - mean) <= 4 * TOL[prec] * abs(mean) + 16 * 2.0 ** -52 * abs(mean), (float(m.mean()[0]), mean)
    # bounds of the raw means of the two calls, then of the central moments formed from them
    def raw_bounds(c):
        _, _, first, second = _want(xr, c)
        return [(4 * TOL[prec] * a + b) / n for a, b in zip(first, second)]
    def central_bounds(c):
        e = raw_bounds(c)
        dl = abs(float(np.mean(xr)) - c) + e[0]
        mk = [float(np.mean(np.abs(xr - c) ** p)) for p in (1, 2, 3, 4)]
        b2 = e[1] + 2 * dl * e[0]
        b3 = e[2] + 3 * (dl * e[1] + mk[1] * e[0]) + 6 * dl * dl * e[0]
        b4 = e[3] + 4 * (dl * e[2] + mk[2] * e[0]) + 6 * (dl * dl * e[1] + 2 * dl * mk[1] * e[0]) + 12 * dl ** 3 * e[0]
        return np.array([b2, b3, b4])
    b = central_bounds(0.0) + central_bounds(3.0)
    c0, c3 = [np.array([float(v[0]) for v in m._central()[1:]]) for m in (m0, m3)]
    print("central moments about 0: %s\n  about 3: %s\n  bound %s" % (c0, c3, b))
    assert np.all(np.abs(c0 - c3) <= b), (c0, c3, b)
    dd = xr - xr.mean()
    assert np.all(np.abs(c3 - [np.mean(dd ** 2), np.mean(dd ** 3), np.mean(dd ** 4)]) <= central_bounds(3.0))


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_stats():
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--stats"]
    r = subprocess.run(exe + ["--steps", "2"], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    nums = re.findall(r"(?:skewness|flatness|min|max)[^=\n]*= \[([^\]]+)\]", r.stdout)
    assert len(nums) >= 6, r.stdout
    vals = np.array([float(v) for grp in nums for v in grp.split()])
    assert np.all(np.isfinite(vals)), r.stdout
    r0 = subprocess.run(exe + ["--steps", "0"], capture_output=True, text=True, timeout=280)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    flat = re.search(r"u: skewness = \[[^\]]+\]\s+flatness = \[([^\]]+)\]", r0.stdout)
    assert flat, r0.stdout
    f = [float(v) for v in flat.group(1).split()]
    assert abs(f[0] - 27.0 / 8) <= 1e-9 and abs(f[1] - 27.0 / 8) <= 1e-9, f      # Taylor-Green at t = 0
