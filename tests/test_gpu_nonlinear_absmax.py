"""GPU: the real-space maxima of the fused nonlinear term (mfft_nonlinear_cross_absmax / mfft_nonlinear_dot_absmax,
mfft_plan_nonlinear_absmax; csrc/fft_nlz.h NlzAbsMax, csrc/absmax.hip) -- the z stage on its own against numpy, the plan
operation against the ORACLE's backward transforms of the same spectra on every route (fused on one rank and several,
batches, composed, pencils, pitched), spectral.absmax, the Taylor-Green known answer and the example's --cfl.

Tolerance of every maximum: |got - want| <= 4 TOL[prec] want, the project's bound for padded paths (gpu_util.TOL)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, TOL, cdtype, have_gpu, orc, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def INFO(dealias, dot):
    return nl.info_key("dot" if dot else "cross", dealias, absmax=True)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _close(got, want, prec, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("absmax %s %s\n  got  %s\n  want %s\n  rel  %s (bound %.1e)" % (what, prec, got.ravel(), want.ravel(),
                                                                          (np.abs(got - want) / want).ravel(), 4 * TOL[prec]))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= 4 * TOL[prec] * want), (what, got, want)


# ---- the stage alone --------------------------------------------------------------------------------------------------
# One length of each build kind of the registry (registry_nlz.h nlz_rows / nlz_wave / nlz_split; TPT = n / values per thread):
#   16    two threads per row, 32 rows per wave (wave-synchronous)         512   64 threads per row: one row per wave
#   1024  128 threads per row: two waves per row (barrier build)           768   a 12-values plan (64 threads per row)
#   3072  256 threads per row; in double precision the split (real / imaginary) exchange
def _irfft_rows(x, n, valid):
    x = x[..., :valid].astype(np.complex128)
    x[..., 0] = x[..., 0].real
    if valid == n // 2 + 1 and n % 2 == 0:
        x[..., -1] = x[..., -1].real
    return np.fft.irfft(x, n=n, axis=-1)


def _stage(n, prec, dot, nrows, valid, spike):
    from mpifft4py_amd import DeviceArray, _lib
    rng = np.random.default_rng(1000 * n + 10 * nrows + valid)
    pitch = valid + 3
    amp = 0.1 * np.sqrt(n)                         # real rows of about 0.04 rms: a spike of height 0.67 - 1 stands out, its partner stays comparable
    ab = amp * (rng.random((2, 3, nrows, pitch)) - 0.5 + 1j * (rng.random((2, 3, nrows, pitch)) - 0.5))
    if spike is not None:
        s, f, row, pos = spike
        ab[s, f, row, :valid] += np.exp(-2j * np.pi * np.arange(valid) * pos / n)
    ab = ab.astype(cdtype(prec))
    a, b = ab[0], ab[1]
    out = np.full((nrows, pitch) if dot else (3, nrows, pitch), 7 + 7j, dtype=cdtype(prec))
    da, db, do = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b), DeviceArray.from_numpy(out)
    got6 = np.zeros(6)
    _lib.call("mfft_nlz_rows_absmax", da.ptr, db.ptr, do.ptr, nrows, n, pitch, valid, _lib.precision_code(prec), 1 if dot else 0,
              got6.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    ra, rb = _irfft_rows(a, n, valid), _irfft_rows(b, n, valid)
    want6 = np.concatenate([np.abs(ra).max((1, 2)), np.abs(rb).max((1, 2))])
    if spike is not None:                          # the planted extreme IS the maximum of its field, where it was planted
        s, f, row, pos = spike
        r = (ra, rb)[s][f]
        assert np.unravel_index(np.argmax(np.abs(r)), r.shape) == (row, pos) and want6[3 * s + f] > 0.55, (spike, want6)
    _close(got6, want6, prec, "stage n=%d nrows=%d valid=%d dot=%d spike=%s" % (n, nrows, valid, dot, spike))
    want = np.fft.rfft(np.sum(ra * rb, 0) if dot else np.cross(ra, rb, axis=0), axis=-1)[..., :valid]
    g = do.get()
    e = orc.rel_l2(g[..., :valid], want)
    assert e < 4 * TOL[prec], e
    assert np.all(g[..., valid:] == 7 + 7j)
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dot", [0, 1])
@pytest.mark.parametrize("n", [16, 512, 1024, 3072, 768])
def test_nlz_rows_absmax_against_numpy(n, dot, prec):
    """mfft_nlz_rows_absmax: the six maxima against numpy.fft.irfft of the rows in double, the product rows within the
    existing bound; one row, an odd row count, the n/3 + 1 bins of the 3/2-rule; spikes in the first row, in the last row
    (whose partner is inactive) and, with one row, in the only one."""
    full, lim = n // 2 + 1, n // 3 + 1
    _stage(n, prec, dot, 37, full, None)
    _stage(n, prec, dot, 1, lim, None)
    tpt = {16: 2, 512: 64, 1024: 128, 3072: 256, 768: 64}[n]
    for i, pos in enumerate((0, 1, tpt - 1, tpt, n // 2, n - 1)):
        _stage(n, prec, dot, 37, full if i % 2 else lim, (i % 2, i % 3, 0 if i % 2 else 36, pos))
    _stage(n, prec, dot, 1, full, (1, 2, 0, n - 1))


def test_nlz_rows_absmax_nan_and_unsupported():
    from mpifft4py_amd import DeviceArray, _lib
    n, nrows, valid = 128, 5, 65
    rng = np.random.default_rng(3)
    a = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    b = rng.random((3, nrows, valid)) - 0.5 + 1j * (rng.random((3, nrows, valid)) - 0.5)
    want = np.concatenate([np.abs(_irfft_rows(a, n, valid)).max((1, 2)), np.abs(_irfft_rows(b, n, valid)).max((1, 2))])
    a[1, 3, 7] = np.nan
    out = DeviceArray.zeros((3, nrows, valid), np.complex128)
    got = np.zeros(6)
    p6 = got.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    da, db = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b)
    _lib.call("mfft_nlz_rows_absmax", da.ptr, db.ptr, out.ptr, nrows, n, valid, valid, _lib.DOUBLE, 0, p6)
    # a_1 holds the NaN: NaN for that field only, b_1 (the other half of its transform) included in the five that are right
    assert np.isnan(got[1]), got
    _close(got[[0, 2, 3, 4, 5]], want[[0, 2, 3, 4, 5]], "double", "beside a NaN")
    plain = DeviceArray.zeros((3, nrows, valid), np.complex128)      # the product rows: NaN where the plain kernel's are, else its bits
    _lib.call("mfft_nlz_rows", da.ptr, db.ptr, plain.ptr, nrows, n, valid, valid, _lib.DOUBLE, 1)
    g, p = out.get(), plain.get()
    assert np.array_equal(np.isnan(g), np.isnan(p)) and np.isnan(g[0, 3]).all() and np.isfinite(g[:, 0]).all()
    assert np.array_equal(g[~np.isnan(g)], p[~np.isnan(p)])
    a[1, 3, 7] = np.inf
    da = DeviceArray.from_numpy(a)
    _lib.call("mfft_nlz_rows_absmax", da.ptr, db.ptr, out.ptr, nrows, n, valid, valid, _lib.DOUBLE, 1, p6)
    assert got[1] == np.inf, got                   # Inf gives Inf
    _close(got[[0, 2, 3, 4, 5]], want[[0, 2, 3, 4, 5]], "double", "beside an Inf")
    z = DeviceArray.zeros((3, 4, 51), np.complex128)
    with pytest.raises(_lib.MfftError):
        _lib.call("mfft_nlz_rows_absmax", z.ptr, z.ptr, z.ptr, 4, 100, 51, 51, _lib.DOUBLE, 0, p6)


# ---- the plan operation, one rank ---------------------------------------------------------------------------------------
_REF = {}


def _reference(N, prec, dealias):
    """Seeded spectra (those of test_gpu_nonlinear_dot: seed 11 + N2) and the oracle's six real fields, computed once."""
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


def _oracle_out(ua, ub, N, prec, dealias, dot):
    return nl.oracle_product("dot" if dot else "cross", (ua, ub), N, prec, dealias)


def _want6(ua, ub):
    return np.stack([np.abs(ua).max((1, 2, 3)), np.abs(ub).max((1, 2, 3))])


def _plan_case(F, N, prec, dealias, dot, fused):
    from mpifft4py_amd import spectral
    a, b, ua, ub = _reference(N, prec, dealias)
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    out = F.empty_complex() if dot else F.empty_complex(3)
    op = spectral.dot_transform if dot else spectral.cross_transform
    op(F, da, db, out, dealias, absmax=True)
    got = spectral.nonlinear_absmax(F)
    assert got.shape == (2, 3) and got.dtype == np.float64
    assert F.plan_info(INFO(dealias, dot)) == (1 if fused else 0)
    _close(got, _want6(ua, ub), prec, "%s %s dot=%d" % (list(N), dealias, dot))
    e = orc.rel_l2(out.get(), _oracle_out(ua, ub, np.array(N), prec, dealias, dot))
    assert e < 4 * TOL[prec], e
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)          # inputs preserved
    op(F, da, db, out, dealias, absmax=True)
    again = spectral.nonlinear_absmax(F)
    assert again.tobytes() == got.tobytes()                                       # bitwise reproducible
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dot", [0, 1])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_nonlinear_absmax_one_rank_fused(N, dealias, dot, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, dot, True)


def test_nonlinear_absmax_pitched_plan_with_nans_between_rows():
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
        out = F.empty_complex(3)
        spectral.cross_transform(F, da, db, out, dealias, absmax=True)
        got = spectral.nonlinear_absmax(F)
        assert F.plan_info(INFO(dealias, 0)) == 1 and np.all(np.isfinite(got))
        _close(got, _want6(ua, ub), prec, "pitched %s" % dealias)


def test_nonlinear_absmax_semantics():
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    with pytest.raises(_lib.MfftError):
        spectral.nonlinear_absmax(F)                                              # no statistics call yet
    a, b, ua, ub = _reference(N, prec, None)
    da, db, out = F.empty_complex(3).set(a), F.empty_complex(3).set(b), F.empty_complex(3)
    spectral.cross_transform(F, da, db, out, None)
    with pytest.raises(_lib.MfftError):
        spectral.nonlinear_absmax(F)                                              # ... a plain call is none
    spectral.cross_transform(F, da, db, out, None, absmax=True)
    first = spectral.nonlinear_absmax(F)
    spectral.cross_transform(F, F.empty_complex(3).set(2 * a), db, out, None)     # plain: the stored values stay
    spectral.dot_transform(F, da, db, F.empty_complex(), "3/2-rule")
    assert spectral.nonlinear_absmax(F).tobytes() == first.tobytes()
    spectral.cross_transform(F, F.empty_complex(3).set(2 * a), db, out, None, absmax=True)
    _close(spectral.nonlinear_absmax(F), _want6(2 * ua, ub), prec, "second statistics call")
    an = a.copy()
    an[2, 3, 5, 7] = np.nan
    spectral.cross_transform(F, F.empty_complex(3).set(an), db, out, None, absmax=True)
    got = spectral.nonlinear_absmax(F)
    assert np.isnan(got[0, 2]), got                                               # for that field only
    keep = np.ones((2, 3), dtype=bool)
    keep[0, 2] = False
    _close(got[keep], _want6(ua, ub)[keep], prec, "beside a NaN field")


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    """(the cases and their checks are this module's own: the child imports it beside nonlinear_util)"""
    return nl.run_child("import test_gpu_nonlinear_absmax as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_nonlinear_absmax_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB: 60 padded x planes of 6 x 48 rows = 152 kB (ALIGN=1: more) each, so
    nine batches of seven planes, the last one ragged with four (ALIGN=1: ten of six).  Field a_0 has its extreme on padded plane 3 (the first batch), b_2 on
    plane 57 (the last): real fields with planted spikes, transformed with numpy."""
    _child("""
N = np.array([40, 32, 64])
rng = np.random.default_rng(8)
ra = 0.05 * (rng.random((3,) + tuple(N)) - 0.5)
rb = 0.05 * (rng.random((3,) + tuple(N)) - 0.5)
ra[0, 2, 10, 20] = 1.0                     # even indices: the point lies on the padded grid too (index 3 / 2 times as large)
rb[2, 38, 4, 6] = -1.5
a = np.stack([np.fft.rfftn(x) for x in ra]); b = np.stack([np.fft.rfftn(x) for x in rb])
ua = np.stack([orc.slab_r2c_backward_padded([x], N, 'double')[0] for x in a])
ub = np.stack([orc.slab_r2c_backward_padded([x], N, 'double')[0] for x in b])
assert np.unravel_index(np.argmax(np.abs(ua[0])), ua[0].shape) == (3, 15, 30), np.unravel_index(np.argmax(np.abs(ua[0])), ua[0].shape)
assert np.unravel_index(np.argmax(np.abs(ub[2])), ub[2].shape) == (57, 6, 9)
F = Slab_R2C(N, L, SelfComm(0), 'double')
for dot in (0, 1):
    out = F.empty_complex() if dot else F.empty_complex(3)
    (spectral.dot_transform if dot else spectral.cross_transform)(F, F.empty_complex(3).set(a), F.empty_complex(3).set(b), out, '3/2-rule', absmax=True)
    got = spectral.nonlinear_absmax(F)
    assert F.plan_info(t.INFO('3/2-rule', dot)) == 1
    t._close(got, t._want6(ua, ub), 'double', 'batches dot=%d' % dot)
    assert orc.rel_l2(out.get(), t._oracle_out(ua, ub, N, 'double', '3/2-rule', dot)) < 4 * TOL['double']
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_nonlinear_absmax_composed_kill_switch():
    """MFFT_NO_NLZ=1: the plan's composition, the sweep over its six real work arrays, the same contract; [16, 32, 24] and
    [20, 24, 40] (no fused kernels for 24 / 36, 40 / 60 either)."""
    _child("""
for N in ([16, 32, 24], [20, 24, 40]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for dot in (0, 1):
                t._plan_case(F, N, prec, dealias, dot, False)
print('ok')
""", MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_nonlinear_absmax_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan, flag 0): every rank's values against the maxima of the
    real fields its own ifftn gives, and the reduced values against the maximum of those over the ranks."""
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
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.5), x.component(i))
        u = DeviceArray.empty(ws, F.float)
        mine = np.zeros((2, 3))
        for s, x in enumerate((a, b)):
            for i in range(3):
                F.ifftn(x.component(i), u, dealias)
                mine[s, i] = np.abs(u.get()).max()
                assert abs(spectral.absmax(F, u) - mine[s, i]) == 0.0              # the sweep on its own: exact
        for dot in (0, 1):
            out = DeviceArray.empty(cs if dot else (3,) + cs, F.complex)
            (spectral.dot_transform if dot else spectral.cross_transform)(F, a, b, out, dealias, absmax=True)
            assert F.plan_info(INFO(dealias, dot)) == 0
            local = spectral.nonlinear_absmax(F, reduce=False)
            _close(local, mine, "double", "pencil rank %d" % comm.Get_rank())
            glob = spectral.nonlinear_absmax(F)
        return mine, glob

    res = run_ranks(4, work)
    want = np.max(np.stack([m for m, _ in res]), 0)
    for _, g in res:
        _close(g, want, "double", "pencils, reduced")
        assert g.tobytes() == res[0][1].tobytes()


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,P", [([32, 64, 128], 2), ([32, 64, 128], 4), ([8, 16, 32], 2), ([8, 16, 32], 4)])
def test_nonlinear_absmax_ranks_fused(N, P, dealias):
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua, ub = _reference(N, "double", dealias)
    want = _want6(ua, ub)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        res = []
        for dot in (0, 1):
            out = DeviceArray.empty(tuple(F.complex_shape()) if dot else (3,) + tuple(F.complex_shape()), F.complex)
            (spectral.dot_transform if dot else spectral.cross_transform)(F, da, db, out, dealias, absmax=True)
            assert F.plan_info(INFO(dealias, dot)) == F.plan_info(INFO(dealias, dot).replace("absmax_", "")) == 1
            res.append((spectral.nonlinear_absmax(F, reduce=False), spectral.nonlinear_absmax(F)))
        # the reduction keeps NaNs: rank 1's NaN reaches every rank, the other entries are the maxima
        v = np.arange(6.0).reshape(2, 3) + comm.Get_rank()
        if comm.Get_rank() == 1:
            v[1, 2] = np.nan
        return res, spectral._max_over_ranks(F, v)

    out = run_ranks(P, work)
    for res, red in out:
        for local, glob in res:
            assert np.all(local <= glob)                                           # a rank holds the maxima of its own x planes
            _close(glob, want, "double", "%s P=%d %s" % (N, P, dealias))
        for i in (0, 1):                                                           # equal on all ranks
            assert res[i][1].tobytes() == out[0][0][i][1].tobytes()
        assert np.isnan(red[1, 2])
        ref = np.arange(6.0).reshape(2, 3) + P - 1
        assert np.array_equal(np.delete(red.ravel(), 5), np.delete(ref.ravel(), 5))
    stack = np.stack([res[0][0] for res, _ in out])
    assert np.array_equal(stack.max(0), out[0][0][0][1])                          # ... and the reduced value is their maximum


# ---- spectral.absmax --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_spectral_absmax(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(4)
    shape = (7, 9, 11)                              # 693 elements: odd, so components 1 and 2 of a (3, ...) fp32 array start off 16 bytes
    for where in (0, 692, 333, 1, 691):
        x = (rng.random(shape) - 0.5).astype(rdtype(prec))
        x.reshape(-1)[where] = -3.25
        assert spectral.absmax(F, DeviceArray.from_numpy(x)) == 3.25
        v = (rng.random((3,) + shape) - 0.5).astype(rdtype(prec))
        v[1].reshape(-1)[where] = 2.5
        v[2].reshape(-1)[692 - where] = -4.5
        got = spectral.absmax(F, DeviceArray.from_numpy(v))
        assert got.shape == (3,) and np.array_equal(got, np.abs(v.astype(np.float64)).reshape(3, -1).max(1)), got
    big = (rng.random((3, 64, 64, 65)) - 0.5).astype(rdtype(prec))     # more than one wave per lane's stride, odd rows
    assert np.array_equal(spectral.absmax(F, DeviceArray.from_numpy(big)), np.abs(big.astype(np.float64)).reshape(3, -1).max(1))
    x = np.zeros(shape, dtype=rdtype(prec))
    assert spectral.absmax(F, DeviceArray.from_numpy(x)) == 0.0
    x[3, 4, 5] = np.nan
    assert np.isnan(spectral.absmax(F, DeviceArray.from_numpy(x)))
    x[3, 4, 5] = -np.inf
    assert spectral.absmax(F, DeviceArray.from_numpy(x)) == np.inf


# ---- known answer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_taylor_green_known_maxima(dealias):
    """u = (sin x cos y cos z, -cos x sin y cos z, 0) and its curl (.., .., 2 sin x sin y cos z) at N = 32: maxima (1, 1, 0) and
    (1, 1, 2) to 1e-10; x = pi / 2 lies on the 32- and on the 48-point grid."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    x = np.arange(32) * 2 * np.pi / 32
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    U = F.empty_complex(3)
    for f, u in enumerate((np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X))):
        F.fftn(DeviceArray.from_numpy(u), U.component(f))
    W = F.empty_complex(3)
    spectral.curl_hat(F, spectral.Wavenumbers(F), U, W)
    spectral.cross_transform(F, U, W, F.empty_complex(3), dealias, absmax=True)
    got = spectral.nonlinear_absmax(F)
    assert F.plan_info(INFO(dealias, 0)) == 1
    print("Taylor-Green maxima (%s): %s" % (dealias, got))
    assert np.all(np.abs(got - np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 2.0]])) <= 1e-10), got
    assert spectral.advective_dt(F, got[0], 0.5) == pytest.approx(0.5 * 2 * np.pi / (2 * 32), rel=1e-9)


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_cfl():
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--steps", "2"]
    r = subprocess.run(exe + ["--cfl", "0.5"], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = re.findall(r"step (\d+): dt = (\S+)\s+max\|omega\| = (\S+)", r.stdout)
    assert [s[0] for s in steps] == ["0", "1"], r.stdout
    assert float(steps[0][1]) == pytest.approx(0.5 * 2 * np.pi / (2 * 32), rel=1e-9)
    assert float(steps[0][2]) == pytest.approx(2.0, rel=1e-9)
    k = float(re.search(r"k = (\S+)", r.stdout).group(1))
    assert k < 0.125                                                                # the energy decreases (Taylor-Green starts at 1/8)
    plain = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert plain.returncode == 0 and "step 0" not in plain.stdout and "dt =" not in plain.stdout, plain.stdout + plain.stderr
    # ... prints what it printed before the option existed: the two lines of a two-step run, timing and buffer figures masked,
    # with the k of the fixed-dt loop (solve()'s defaults, the loop tests/test_gpu_demo.py holds to the golden value)
    lines = plain.stdout.strip().splitlines()
    assert len(lines) == 2, plain.stdout
    assert re.fullmatch(r"N = 32\^3, 2 RK4 steps, \d+\.\d{3} ms per step \(fused nonlinear z stage, device-resident; "
                        r"plan work buffers \d+\.\d{2} GB\)", lines[0]), lines[0]
    m = re.fullmatch(r"k = ([0-9.e+-]+)", lines[1])
    assert m, lines[1]
    import spectral_dns_device as demo
    from mpifft4py_amd import SelfComm
    want = demo.solve(SelfComm(), steps=2)
    assert abs(float(m.group(1)) - want) < 1e-12 and float(m.group(1)) != pytest.approx(k, abs=1e-9), (lines[1], want, k)
