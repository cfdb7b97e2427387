"""GPU: structure functions along z of spectral fields without the real-space arrays (mfft_real_increments, mfft_nlz_incr_rows,
mfft_ew_increments; csrc/nlz_incr.h NlzIncr::body, csrc/incr.hip) -- the z stage on its own against numpy (np.roll), the plan operation
against the ORACLE's backward transforms of the same spectra on every route (fused on one rank and several, composed, pencils,
pitched), spectral.increments, S_2 against the spectrum of the rows, the Taylor-Green known answer, and the example's --structure.

Tolerance, with x the reference field in float64, cnt its points, d = x(z + s) - x(z) and TOL = gpu_util.TOL -- the moments' rule
with the factor 2 that a difference of two values brings:
  S_p from spectra     2 TOL[prec] p sqrt(sum d^(2(p-1)) sum x^2) + (cnt + 8) 2^-52 sum |d|^p
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
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
POISON = -7.25e300                     # a double no sum of these fields takes: an output nobody wrote


def INFO(dealias):
    return "nonlinear_increments_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


_WANT = {}


def _want(x, seps, key=None):
    """Per separation ([S2, S3, S4] in long double, the first and the second term of the bound before TOL), rows along the last
    axis of x.  `key`: computed once per key and shared."""
    k = (key, tuple(int(s) for s in seps))
    if key is not None and k in _WANT:
        return _WANT[k]
    x = np.asarray(x, dtype=np.float64)
    xl = x.astype(np.longdouble)
    sx2 = float(np.sum(xl * xl))
    res = []
    for s in seps:
        d = np.roll(xl, -int(s), axis=-1) - xl
        d2 = d * d
        d3 = d2 * d
        ref = [np.sum(d2), np.sum(d3), np.sum(d2 * d2)]
        sabs = [float(ref[0]), float(np.sum(np.abs(d3))), float(ref[2])]
        s2p = [float(ref[0]), float(ref[2]), float(np.sum(d3 * d3))]            # sum d^(2 (p - 1)), p = 2, 3, 4
        first = [2 * p * np.sqrt(s2p[p - 2] * sx2) for p in (2, 3, 4)]
        second = [(x.size + 8) * 2.0 ** -52 * sabs[p - 2] for p in (2, 3, 4)]
        res.append((ref, first, second))
    if key is not None:
        _WANT[k] = res
    return res


def _check(got, fields, seps, prec, what, spectral_input=True, keys=None):
    """got: (nfields, nsep, 3); fields: the reference fields, rows along their last axis; every figure is printed before it is
    asserted."""
    got = np.asarray(got, dtype=np.float64).reshape(len(fields), len(seps), 3)
    tol = TOL[prec] if spectral_input else 0.0
    for f, x in enumerate(fields):
        for i, (ref, first, second) in enumerate(_want(x, seps, keys[f] if keys is not None else None)):
            bounds = [tol * a + b for a, b in zip(first, second)]
            errs = [abs(float(np.longdouble(got[f, i, k]) - ref[k])) for k in range(3)]
            print("increments %s %s field %d s=%d\n  got   %s\n  err   %s\n  bound %s" % (what, prec, f, seps[i], got[f, i], errs, bounds))
            assert all(np.isfinite(got[f, i])) and all(e <= b for e, b in zip(errs, bounds)), (what, f, seps[i], got[f, i], errs, bounds)


# ---- the stage alone --------------------------------------------------------------------------------------------------
#   12    the shortest plan (12 values per thread, one thread per row)   16    two threads per row, 32 rows per wave
#   144   a 9 * 2^a plan                                                 768   a 12-values plan, 64 threads per row
#   1024  128 threads per row: two waves per row, the one kernel here that is NOT wave-synchronous (workgroup barriers)
#   1536  128 threads per row with 12 values: the z row of 1024 under the 3/2-rule
def _irfft_rows(x, n, vin):
    x = x[..., :vin].astype(np.complex128)
    x[..., 0] = x[..., 0].real
    if vin == n // 2 + 1 and n % 2 == 0:
        x[..., -1] = x[..., -1].real
    return np.fft.irfft(x, n=n, axis=-1)


def _stage_seps(n):
    """1, a multiple of every thread stride of the plans (16 where the row has it), an odd value near the middle, n / 2, n - 1, a
    duplicate, and two more short ones: eight."""
    return [1, min(16, n - 2), (n // 2 - 1) | 1, n // 2, n - 1, 1, 2, 3]


def _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, seps):
    from mpifft4py_amd import DeviceArray, _lib
    da = DeviceArray.from_numpy(a)
    db = DeviceArray.from_numpy(b) if b is not None else None
    got = np.full(nfields * len(seps) * 3, POISON)
    sv = np.ascontiguousarray(seps, dtype=np.int64)
    _lib.call("mfft_nlz_incr_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, valid_in,
              _lib.precision_code(prec), sv.ctypes.data_as(IP), len(seps), got.ctypes.data_as(DP))
    assert da.get().tobytes() == a.tobytes() and (b is None or db.get().tobytes() == b.tobytes())      # inputs preserved
    assert not np.any(got == POISON)
    return got.reshape(nfields, len(seps), 3)


def _stage(n, prec, nfields, nrows, valid, valid_in=0, seps=None):
    rng = np.random.default_rng(1000 * n + 10 * nrows + valid + nfields)
    pitch = valid + 3
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = ((ncomp,) if nfields > 2 else ()) + (nrows, pitch)
    draw = lambda: (np.sqrt(n) * (rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5))).astype(cdtype(prec))
    a = draw()
    b = draw() if nfields % 2 == 0 else None
    for x in (a, b):
        if x is not None:
            x[..., 0] += n * 0.75                      # a mean of 0.75 in every row: the increments do not see it, the rounding does
    seps = _stage_seps(n) if seps is None else seps
    got = _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, seps)
    vin = valid_in or valid
    fields = [r for x in (a, b) if x is not None for r in _irfft_rows(x.reshape((ncomp, nrows, pitch)), n, vin)]
    _check(got, fields, seps, prec, "stage n=%d nfields=%d nrows=%d valid=%d/%d" % (n, nfields, nrows, vin, valid))
    if len(seps) > 5 and seps[5] == seps[0]:
        assert got[:, 0].tobytes() == got[:, 5].tobytes()               # the duplicate separation: the same bits
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [12, 16, 144, 768, 1024, 1536])
def test_nlz_incr_rows_against_numpy(n, prec):
    """mfft_nlz_incr_rows against np.roll of numpy.fft.irfft of the rows in double: 37 rows and one, the n/2 + 1 bins and the
    n/3 + 1 of the 3/2-rule, pruned valid_in, field counts 6, 1, 3 and 2; a second call gives the same bits."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage(n, prec, 6, 37, full)
    assert _stage(n, prec, 6, 37, full).tobytes() == first.tobytes()
    _stage(n, prec, 1, 1, lim)
    _stage(n, prec, 3, 37, lim)
    _stage(n, prec, 2, 1, full, valid_in=lim)
    _stage(n, prec, 1, 37, full, seps=[n // 2])                        # one separation


@pytest.mark.parametrize("prec", ["double", "single"])
def test_nlz_incr_rows_more_than_two_passes_of_the_grid(prec):
    """n = 16: the launch has at most mfft_nlz_incr_groups workgroups of 2 x 128 rows; twice that many rows and a ragged rest, so
    every workgroup strides and the last pass is partial."""
    from mpifft4py_amd import _lib
    cap = _lib.call("mfft_nlz_incr_groups", 1 << 40, 16, _lib.precision_code(prec))
    assert cap >= 1
    nrows = 2 * cap * 256 + 333
    assert _lib.call("mfft_nlz_incr_groups", nrows, 16, _lib.precision_code(prec)) == cap
    _stage(16, prec, 1, nrows, 9)


def test_nlz_incr_rows_nan_and_inf_mark_their_field_only():
    n, nrows, valid = 128, 5, 65
    rng = np.random.default_rng(3)
    a = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    b = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    fields = list(_irfft_rows(a, n, valid)) + list(_irfft_rows(b, n, valid))
    keep = [0, 2, 3, 4, 5]
    seps = [1, 7, 64, 127]
    for bad in (np.nan, np.inf):
        a[1, 3, 7] = bad
        got = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", seps)
        # a_1 holds the bad bin: NaN in all of ITS sums, b_1 (the other half of its transform) among the five that are right
        assert np.all(np.isnan(got[1])), got
        _check(got[keep], [fields[i] for i in keep], seps, "double", "beside %s" % bad)


def _untouched(fn):
    """fn(out) raises MfftError and leaves `out` as it was; returns the message."""
    from mpifft4py_amd import _lib
    out = np.full(6 * 8 * 3 + 8, POISON)
    with pytest.raises(_lib.MfftError) as e:
        fn(out)
    assert np.all(out == POISON), "an output was written by a call that failed"
    return str(e.value)


def test_error_cases_leave_the_outputs_untouched():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+) = (-\d+)", open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read())}
    inv, uns = "error %d:" % codes["MFFT_ERR_INVALID"], "error %d:" % codes["MFFT_ERR_UNSUPPORTED"]
    maxsep = 8
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    count = ctypes.c_int64(-5)

    def sv(seps):
        return np.ascontiguousarray(seps, dtype=np.int64)

    def stage(seps, nsep=None, n=128, valid=65):
        s = sv(seps)
        return lambda out: _lib.call("mfft_nlz_incr_rows", z.ptr, z.ptr, 6, 4, n, 65, valid, 0, _lib.DOUBLE, s.ctypes.data_as(IP),
                                     len(seps) if nsep is None else nsep, out.ctypes.data_as(DP))
    bad_lists = [([1], 0), ([1] * (maxsep + 1), None), ([0], None), ([-1], None), ([128], None), ([1, 2, 200], None)]
    for seps, nsep in bad_lists:
        assert inv in _untouched(stage(seps, nsep)), (seps, nsep)
    assert uns in _untouched(stage([1], n=100, valid=51))             # 100 has no fused kernel
    assert inv in _untouched(stage([1], n=64))                        # more bins than a row of 64 points has
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), "double")
    x = DeviceArray.zeros((3, 8, 16, 32), np.float64)
    for seps, nsep in [([1], 0), ([1] * (maxsep + 1), None), ([0], None), ([32], None), ([-3], None)]:
        s = sv(seps)
        assert inv in _untouched(lambda out: _lib.call("mfft_ew_increments", F._plan, x.ptr, 3, 128, 32, 32, _lib.DOUBLE, s.ctypes.data_as(IP),
                                                       len(seps) if nsep is None else nsep, out.ctypes.data_as(DP))), seps
    a = F.empty_complex(3).set(np.zeros((3,) + tuple(F.complex_shape()), np.complex128))
    for dealias, M in ((None, 32), ("2/3-rule", 32), ("3/2-rule", 48)):
        if dealias == "2/3-rule":
            F._ensure_mask()
        for seps, nsep in [([1], 0), ([1] * (maxsep + 1), None), ([0], None), ([M], None), ([-3], None)]:
            s = sv(seps)
            assert inv in _untouched(lambda out: _lib.call("mfft_real_increments", F._plan, a.ptr, a.ptr, 3, _DEALIAS[dealias], s.ctypes.data_as(IP),
                                                           len(seps) if nsep is None else nsep, out.ctypes.data_as(DP), ctypes.byref(count))), (dealias, seps)
        assert count.value == -5
        # the last valid separation of the mode is taken
        s, out = sv([M - 1]), np.zeros(18)
        _lib.call("mfft_real_increments", F._plan, a.ptr, a.ptr, 3, _DEALIAS[dealias], s.ctypes.data_as(IP), 1, out.ctypes.data_as(DP), ctypes.byref(count))
        assert np.all(out == 0.0)
        count.value = -5


# ---- the plan operation, one rank ---------------------------------------------------------------------------------------
_REF = {}


def _reference(N, prec, dealias):
    """Seeded spectra (those of the moments tests: seed 11 + N2) and the oracle's six real fields, computed once."""
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


def _call(F, a, b, nfields, dealias, seps=None, reduce=True):
    """real_increments of the first `nfields` of (a, b): 1: a[0]; 3: a; 6: a and b.  Returns (Increments, the device inputs)."""
    from mpifft4py_amd import spectral
    if nfields == 1:
        da, db = F.empty_complex().set(a[0]), None
    else:
        da, db = F.empty_complex(3).set(a), (F.empty_complex(3).set(b) if nfields == 6 else None)
    return spectral.real_increments(F, da, db, dealias, seps, reduce), da, db


def _plan_case(F, N, prec, dealias, nfields, fused, seps=None):
    from mpifft4py_amd import spectral
    a, b, ua, ub = _reference(N, prec, dealias)
    inc, da, db = _call(F, a, b, nfields, dealias, seps)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    fields = (list(ua) + list(ub))[:nfields]
    M = fields[0].shape[-1]
    assert inc.M == M == (3 * N[2] // 2 if dealias == "3/2-rule" else N[2])
    if seps is None:
        assert list(inc.seps) == spectral.default_seps(M) and inc.seps[-1] == M // 2
    assert inc.count == fields[0].size and inc.sums.shape == (nfields, len(inc.seps), 3)
    _check(inc.sums, fields, list(inc.seps), prec, "%s %s nfields=%d" % (list(N), dealias, nfields), keys=_keys(N, prec, dealias)[:nfields])
    assert np.array_equal(da.get(), a[0] if nfields == 1 else a) and (db is None or np.array_equal(db.get(), b))      # inputs preserved
    again = spectral.real_increments(F, da, db, dealias, seps)
    assert again.sums.tobytes() == inc.sums.tobytes() and again.count == inc.count                                    # bitwise reproducible
    assert np.allclose(inc.r(F), inc.seps * 2 * np.pi / M, rtol=1e-6)
    return inc


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_increments_one_rank_fused(N, dealias, nfields, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, nfields, True)


def test_real_increments_long_lists_go_in_chunks():
    """Eleven separations, a duplicate and the two ends of the range among them: two calls of the library, one result."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = [8, 16, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert spectral.INCR_MAXSEP < 11
    for dealias, M in (("3/2-rule", 48), (None, 32)):
        seps = [1, 2, 3, 5, 7, 11, 13, M // 2, M - 1, 1, 17]
        inc = _plan_case(F, N, "double", dealias, 6, True, seps=seps)
        assert inc.sums[:, 0].tobytes() == inc.sums[:, 9].tobytes()
        one = _call(F, *_reference(N, "double", dealias)[:2], 6, dealias, seps=seps[8:])[0]
        assert one.sums.tobytes() == inc.sums[:, 8:].tobytes()


def test_real_increments_pitched_plan_with_nans_between_rows():
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
        inc = spectral.real_increments(F, da, db, dealias)
        assert F.plan_info(INFO(dealias)) == 1
        _check(inc.sums, list(ua) + list(ub), list(inc.seps), prec, "pitched %s" % dealias, keys=_keys(N, prec, dealias))


def test_real_increments_nan_marks_its_field_only():
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua, ub = _reference(N, prec, None)
    an = a.copy()
    an[2, 3, 5, 7] = np.nan
    inc, _, _ = _call(F, an, b, 6, None)
    assert np.all(np.isnan(inc.sums[2])), inc.sums
    keep = [0, 1, 3, 4, 5]
    _check(inc.sums[keep], [(list(ua) + list(ub))[i] for i in keep], list(inc.seps), prec, "beside a NaN field")
    assert np.all(np.isnan(inc.skewness()[2].astype(np.float64))) and np.all(np.isfinite(inc.flatness()[keep].astype(np.float64)))


# ---- composed route: a fresh process (the switch is read once) -------------------------------------------------------------
def test_real_increments_composed_kill_switch():
    """MFFT_NO_NLZ=1: one field at a time through the plan's inverse transform into ONE real work array and the sweep; [8, 16, 32]
    (fused without the switch), [16, 32, 24] and [20, 24, 40] (no fused kernels for 24 / 36, 40 / 60 either).  The plan's nonlinear
    buffers hold that one array: the padded real field of the 3/2-rule, the first mode run."""
    nl.run_child("""
import test_gpu_real_increments as t
for N in ([8, 16, 32], [16, 32, 24], [20, 24, 40]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for nfields in (6, 1, 3):
                t._plan_case(F, N, prec, dealias, nfields, False)
            one = int(np.prod([3 * n // 2 for n in N])) * (8 if prec == 'double' else 4)
            assert F.plan_info('nonlinear_bytes') == one, (F.plan_info('nonlinear_bytes'), one)
print('ok')
""", timeout=280, MFFT_NO_NLZ="1")


def test_real_increments_lengths_without_a_kernel_are_composed():
    """[24, 40, 20]: no fused z kernel of 20 or 30 points, so every mode goes through the one work array and the sweep; [16, 32, 24]
    has one of 24 but none of 36, so only its 3/2-rule does."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N = [24, 40, 20]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    for dealias in ("3/2-rule", "2/3-rule", None):
        _plan_case(F, N, "double", dealias, 6, False)
    N = [16, 32, 24]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "single")
    for dealias in ("3/2-rule", "2/3-rule", None):
        _plan_case(F, N, "single", dealias, 3, dealias != "3/2-rule")


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_real_increments_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan, flag 0; z is whole on every rank): every rank's sums against the
    real fields its own ifftn gives, the reduced ones against all of them together; the same bits on every rank."""
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
                s = spectral.increments(F, u)
                _check(s.sums, [mine[-1]], list(s.seps), "double", "sweep, pencil rank %d" % comm.Get_rank(), spectral_input=False)
        local = spectral.real_increments(F, a, b, dealias, reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == mine[0].size and local.M == ws[-1]
        _check(local.sums, mine, list(local.seps), "double", "pencil rank %d" % comm.Get_rank())
        glob = spectral.real_increments(F, a, b, dealias)
        return mine, local.sums, glob.sums, glob.count, list(glob.seps)

    res = run_ranks(4, work)
    for _, _, g, cnt, seps in res:
        assert cnt == sum(r[0][0].size for r in res) and g.tobytes() == res[0][2].tobytes()
    assert np.array_equal(np.sum([r[1] for r in res], 0), res[0][2])      # (rank order: what allreduce adds)
    # the reduced sums against the ranks' rows together: rows are whole on every rank, so the rows of all ranks are the field's
    whole = [np.concatenate([r[0][f].reshape(-1, r[0][f].shape[-1]) for r in res]) for f in range(6)]
    _check(res[0][2], whole, res[0][4], "double", "pencils, reduced")


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
_ONE = {}


def _one_rank(N, dealias):
    from mpifft4py_amd import SelfComm, Slab_R2C
    key = (tuple(N), dealias)
    if key not in _ONE:
        a, b, _, _ = _reference(N, "double", dealias)
        _ONE[key] = _call(Slab_R2C(np.array(N), L, SelfComm(0), "double"), a, b, 6, dealias)[0]
    return _ONE[key]


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,P", [([32, 64, 128], 2), ([32, 64, 128], 4), ([8, 16, 32], 2), ([8, 16, 32], 4)])
def test_real_increments_ranks_fused(N, P, dealias):
    """The ranks' sums add up to the one-rank result -- to the bits where the reduction is concerned (rank order), within the
    rounding of a double sum in another order where the one-rank call is -- and so do the counts."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua, ub = _reference(N, "double", dealias)
    fields = list(ua) + list(ub)
    one = _one_rank(N, dealias)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_increments(F, da, db, dealias, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_increments(F, da, db, dealias)
        three = spectral.real_increments(F, da, None, dealias)
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return local.sums, local.count, glob.sums, glob.count, three.sums, list(glob.seps)

    out = run_ranks(P, work)
    planes = ua.shape[1] // P                                                      # a rank holds the sums of its own x planes
    seps = out[0][5]
    assert seps == list(one.seps)
    for r, (local, lcount, glob, gcount, three, _) in enumerate(out):
        mine = [x[r * planes:(r + 1) * planes] for x in fields]
        assert lcount == mine[0].size and gcount == fields[0].size == one.count
        _check(local, mine, seps, "double", "%s P=%d %s rank %d" % (N, P, dealias, r))
        _check(glob, fields, seps, "double", "%s P=%d %s reduced" % (N, P, dealias), keys=_keys(N, "double", dealias))
        _check(three, fields[:3], seps, "double", "%s P=%d %s three fields" % (N, P, dealias), keys=_keys(N, "double", dealias)[:3])
        assert glob.tobytes() == out[0][2].tobytes()                               # equal on all ranks
    assert sum(o[1] for o in out) == one.count
    assert np.array_equal(np.sum(np.stack([o[0] for o in out]), 0), out[0][2])     # local sums add up to the reduced ones
    # ... and to the one-rank result: both are within their bound of the same reference, so within twice the bound of each other
    for f in range(6):
        for i, (ref, first, second) in enumerate(_want(fields[f], seps, _keys(N, "double", dealias)[f])):
            for k in range(3):
                assert abs(out[0][2][f, i, k] - one.sums[f, i, k]) <= 2 * (TOL["double"] * first[k] + second[k])


# ---- spectral.increments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_spectral_increments(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(4)
    shape = (7, 9, 11)                              # odd everywhere: rows of 11 start off 16 bytes
    x = (rng.random(shape) - 0.3).astype(rdtype(prec))
    inc = spectral.increments(F, DeviceArray.from_numpy(x))
    assert inc.count == 693 and inc.M == 11 and list(inc.seps) == [1, 2, 4, 5] and inc.sums.shape == (1, 4, 3)
    _check(inc.sums, [x], list(inc.seps), prec, "sweep %s" % (shape,), spectral_input=False)
    seps = [1, 10, 5, 6, 3, 1, 7, 9, 2, 4, 8]       # eleven: two sweeps
    v = (rng.random((3,) + shape) - 0.3).astype(rdtype(prec))
    inc = spectral.increments(F, DeviceArray.from_numpy(v), seps=seps)
    assert inc.count == 693 and inc.sums.shape == (3, 11, 3)
    _check(inc.sums, list(v), seps, prec, "sweep (3, 7, 9, 11)", spectral_input=False)
    assert inc.sums[:, 0].tobytes() == inc.sums[:, 5].tobytes()
    # the rule in numpy float64 agrees with the long-double sums as well
    _check(np.stack([spectral.incr_rule(v[f], seps) for f in range(3)]), list(v), seps, prec, "incr_rule", spectral_input=False)
    big = (rng.random((6, 16, 33, 65)) - 0.5).astype(rdtype(prec))     # more than one element per lane, odd rows, six components
    inc = spectral.increments(F, DeviceArray.from_numpy(big))
    _check(inc.sums, list(big), list(inc.seps), prec, "sweep (6, 16, 33, 65)", spectral_input=False)
    again = spectral.increments(F, DeviceArray.from_numpy(big))
    assert again.sums.tobytes() == inc.sums.tobytes()
    # a pitched array is swept as it lies: NaNs between the rows
    two = (rng.random((2, 4, 5, 6)) - 0.5).astype(rdtype(prec))
    whole = np.full((2, 4, 5, 8), np.nan, dtype=rdtype(prec))
    whole[..., :6] = two
    dw = DeviceArray.from_numpy(whole)
    pitched = DeviceArray(two.shape, two.dtype, ptr=dw.ptr, owner=False, pitch=8)
    inc = spectral.increments(F, pitched, seps=[1, 3, 5])
    _check(inc.sums, list(two), [1, 3, 5], prec, "sweep, pitched", spectral_input=False)
    z = np.zeros(shape, dtype=rdtype(prec))
    assert np.array_equal(spectral.increments(F, DeviceArray.from_numpy(z)).sums, np.zeros((1, 4, 3)))
    z[3, 4, 5] = np.nan
    assert np.all(np.isnan(spectral.increments(F, DeviceArray.from_numpy(z)).sums))


# ---- S_2 against the spectrum: no np.roll ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [12, 144, 1024])
def test_s2_against_the_spectrum_of_the_rows(n, prec):
    """sum_z d^2 = (1 / M) sum_k |X_k|^2 2 (1 - cos 2 pi k s / M), X the full spectrum of the row: with the half-spectrum,
    (1 / M) sum_q h_q |A_q|^2 2 (1 - cos 2 pi q s / M), h = 1 for q = 0 and M / 2, else 2."""
    nrows, valid = 9, n // 2 + 1
    rng = np.random.default_rng(n)
    a = (np.sqrt(n) * (rng.random((nrows, valid)) - 0.5 + 1j * (rng.random((nrows, valid)) - 0.5))).astype(cdtype(prec))
    seps = _stage_seps(n)
    got = _rows_call(a, None, 1, nrows, n, valid, valid, 0, prec, seps)
    al = a.astype(np.complex128)
    al[:, 0] = al[:, 0].real
    al[:, -1] = al[:, -1].real
    h = np.full(valid, 2.0)
    h[0] = h[-1] = 1.0
    p = (np.abs(al) ** 2 * h).astype(np.longdouble).sum(0) / np.longdouble(n) ** 2      # irfft carries 1 / M: |x_k|^2 / M^2, times M / M
    q = np.arange(valid, dtype=np.longdouble)
    sx2 = float(np.sum(p)) * n
    for i, s in enumerate(seps):
        want = np.sum(p * 2 * (1 - np.cos(2 * np.pi * q * s / n))) * n
        bound = TOL[prec] * 2 * 2 * np.sqrt(float(want) * sx2) + (nrows * n + 8) * 2.0 ** -52 * float(want)
        print("S2 from the spectrum n=%d %s s=%d: got %r want %r bound %r" % (n, prec, s, got[0, i, 0], float(want), bound))
        assert abs(got[0, i, 0] - float(want)) <= bound


# ---- known answer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_taylor_green_known_structure_functions(dealias):
    """u = (sin x cos y cos z, -cos x sin y cos z, 0) at N = 32, r = 2 pi s / M: u_0(z + r) - u_0(z) = -2 sin x cos y sin(r/2)
    sin(z + r/2), so S_2 = 4 sin^2(r/2) <sin^2 x><cos^2 y><sin^2> = sin^2(r/2) / 2, S_3 = 0, S_4 = 16 sin^4(r/2) (3/8)^3 = (27/32)
    sin^4(r/2); field 2 is zero.  Within 1e-10 (what the transforms of the plan keep; the sums themselves are exact to 1e-16 on
    grids of 32 and 48 points)."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    x = np.arange(32) * 2 * np.pi / 32
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    U = F.empty_complex(3)
    for f, u in enumerate((np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X))):
        F.fftn(DeviceArray.from_numpy(u), U.component(f))
    inc = spectral.real_increments(F, U, None, dealias)
    assert F.plan_info(INFO(dealias)) == 1
    M = 48 if dealias == "3/2-rule" else 32
    assert inc.M == M and inc.count == M ** 3
    r = inc.r(F)
    assert np.allclose(r, inc.seps * 2 * np.pi / M, rtol=1e-14)
    sh = np.sin(r / 2) ** 2
    S2, S3, S4 = (inc.S(p).astype(np.float64) for p in (2, 3, 4))
    print("Taylor-Green (%s): seps %s\n  S2 %s\n  S3 %s\n  S4 %s" % (dealias, inc.seps, S2, S3, S4))
    for f in (0, 1):
        assert np.all(np.abs(S2[f] - sh / 2) <= 1e-10) and np.all(np.abs(S3[f]) <= 1e-10) and np.all(np.abs(S4[f] - 27.0 / 32 * sh * sh) <= 1e-10)
    assert np.all(np.abs(S2[2]) <= 1e-20) and np.all(np.abs(S3[2]) <= 1e-20) and np.all(np.abs(S4[2]) <= 1e-20)
    flat = inc.flatness().astype(np.float64)
    assert np.all(np.abs(flat[0] - 27.0 / 8) <= 1e-8)


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_structure():
    """--structure prints one line before every step and one of the final state.  At t = 0 (Taylor-Green, the 3/2-rule at 32^3: rows
    of 48 points) S_2 of u_0 is sin^2(r / 2) / 2 and u_2 is zero, so the longitudinal skewness is 0 / 0 there; after two steps every
    figure is finite and the flatness at least 1."""
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--structure"]
    nums = lambda name, line: np.array([float(v) for v in re.search(re.escape(name) + r" = \[([^\]]*)\]", line).group(1).split()])
    r = subprocess.run(exe + ["--steps", "2"], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("structure ")]
    assert len(lines) == 3 and lines[0].startswith("structure step 0:") and lines[2].startswith("structure final:"), r.stdout
    assert list(nums("s", lines[2])) == [1, 2, 4, 8, 16, 24]
    for l in lines:
        assert np.all(np.isfinite(nums("S2(u_0)", l))) and np.all(nums("S2(u_0)", l) > 0) and np.all(nums("S2(u_2)", l) >= 0), l
    last = lines[2]
    assert np.all(nums("S2(u_2)", last) > 0) and np.all(np.isfinite(nums("skewness(du_2)", last))) and np.all(nums("flatness(du_2)", last) >= 1.0), last
    r0 = subprocess.run(exe + ["--steps", "0"], capture_output=True, text=True, timeout=280)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    l0 = [l for l in r0.stdout.splitlines() if l.startswith("structure ")]
    assert len(l0) == 1 and l0[0].startswith("structure final:"), r0.stdout
    got = nums("S2(u_0)", l0[0])
    want = np.sin(np.pi * np.array([1, 2, 4, 8, 16, 24]) / 48) ** 2 / 2
    assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-9), (got, want)      # Taylor-Green at t = 0
    assert np.all(nums("S2(u_2)", l0[0]) == 0.0)
