"""GPU: both nonlinear terms of a velocity that carries a scalar, fftn(ifftn(a) x ifftn(b)) and fftn(sum_f ifftn(a_f) ifftn(c_f)),
as one plan operation (mfft_nonlinear_cross_dot; csrc/fft_nlz.h body_cross_dot) against the ORACLE's transforms -- what a
caller composes from nine FFT.ifftn, np.cross, np.sum(ua * uc, 0) and four FFT.fftn -- on the same seeded spectra, through the C
ABI; against cross_transform + dot_transform of the same plan over several ranks and at 512^3; its z stage on its own against
numpy; and the Boussinesq example, one operation per stage against two calls."""
import os
import sys

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, TOL, cdtype, have_gpu, orc, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
INFO = {d: nl.info_key("cross_dot", d) for d in nl.RULE}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _spectra(cs, N, prec, seed, hermitian):
    return nl.spectra(cs, N, prec, seed, hermitian, 3)


def _oracle(a, b, c, N, prec, dealias, mask=None):
    """(fftn(ifftn(a) x ifftn(b)), fftn(sum_f ifftn(a_f) ifftn(c_f))) with the oracle's one-rank transforms in the mode `dealias`."""
    return nl.oracle("cross_dot", (a, b, c), N, prec, dealias, mask)


def _nlz_lengths():
    """The z lengths with a fused kernel: every plan of MFFT_NLZPLANS_P2 / _3 / _9 (csrc/plans.h)."""
    import re
    txt = open(os.path.join(ROOT, "mpifft4py_amd", "csrc", "plans.h")).read().replace("\\\n", " ")
    out = []
    for group in ("MFFT_NLZPLANS_P2", "MFFT_NLZPLANS_3", "MFFT_NLZPLANS_9"):
        body = re.search(r"#define %s\(X\)(.*)" % group, txt).group(1)
        out += [int(n) for n in re.findall(r"X\((\d+),", body)]
    assert len(out) == 32, out
    return sorted(out)


_REF = {}      # the spectra and the oracle's answer of a case, computed once and left unchanged


def _reference(F, N, prec, dealias, hermitian, seed=None):
    key = (tuple(int(n) for n in N), prec, dealias, hermitian, seed)
    if key not in _REF:
        a, b, c = _spectra(tuple(F.complex_shape()), N, prec, (13 + int(N[2])) if seed is None else seed, hermitian)
        mask = F.get_dealias_filter() if dealias == "2/3-rule" else None
        want, swant = _oracle(a, b, c, np.array(N), prec, dealias, mask)
        for x in (a, b, c, want, swant):
            x.setflags(write=False)
        _REF[key] = (a, b, c, want, swant)
    return _REF[key]


def _one_rank(N, fused, dealias, prec, hermitian, complex_pitch=None):
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=complex_pitch)
    a, b, c, want, swant = _reference(F, N, prec, dealias, hermitian)
    da, db, dc = (F.empty_complex(3).set(x) for x in (a, b, c))
    out, s = F.empty_complex(3), F.empty_complex()
    spectral.cross_dot_transform(F, da, db, dc, out, s, dealias)
    F.sync()
    if fused == "z":      # the composed route wherever the z length the mode works on (the padded one under the 3/2-rule) has no kernel
        if (int(N[2]) * 3 // 2 if dealias == "3/2-rule" else int(N[2])) not in _nlz_lengths():
            assert F.plan_info(INFO[dealias]) == 0
    elif fused is not None:
        assert F.plan_info(INFO[dealias]) == (1 if fused else 0)
    e, es = orc.rel_l2(out.get(), want), orc.rel_l2(s.get(), swant)
    print("cross_dot_transform %s %s %s herm=%s rel-L2 cross %.3e dot %.3e (bound %.1e)" % (list(N), dealias, prec, hermitian, e, es, 4 * TOL[prec]))
    assert e < 4 * TOL[prec] and es < 4 * TOL[prec]
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b) and np.array_equal(dc.get(), c)      # inputs preserved
    spectral.cross_dot_transform(F, da, db, dc, da, dc.component(1), dealias)      # the results over a_hat and one component of c_hat
    F.sync()
    ga, gc = da.get(), dc.get()
    assert orc.rel_l2(ga, want) < 4 * TOL[prec] and orc.rel_l2(gc[1], swant) < 4 * TOL[prec]
    assert np.array_equal(db.get(), b) and np.array_equal(gc[0], c[0]) and np.array_equal(gc[2], c[2])


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([32, 64, 128], True), ([36, 72, 144], True), ([108, 216, 432], True),
                                     ([16, 32, 24], "z"), ([20, 24, 40], "z")])
def test_nonlinear_cross_dot_one_rank(N, fused, dealias, prec):
    """One rank, slab, spectra of real fields: the fused route where every axis has its kernels (flag 1), the plan's own
    composition where a mode's z length has none -- both against the oracle; inputs preserved; then out_hat over a_hat and s_hat over
    c_hat.component(1), the untouched components bitwise."""
    _one_rank(N, fused, dealias, prec, True)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,fused", [([32, 64, 128], True), ([16, 32, 24], None)])
def test_nonlinear_cross_dot_one_rank_arbitrary_spectra(N, fused, dealias, prec):
    """Arbitrary complex spectra: the bins a real field would not have follow the transforms' conventions."""
    _one_rank(N, fused, dealias, prec, False)


def test_nonlinear_cross_dot_pitched_plan():
    """A plan whose spectra have rows a whole number of cache lines apart: the routes run on the pitched rows."""
    for dealias in ("3/2-rule", "2/3-rule", None):
        _one_rank([32, 64, 128], True, dealias, "double", True, complex_pitch="auto")


@pytest.mark.parametrize("batch_mb,align", [("1", "0"), ("1", "1"), ("3", "-1")])
def test_nonlinear_cross_dot_batches(batch_mb, align):
    """Several batches of x planes and both row pitches of the intermediates: a fresh process, the switches are read once.
    (Nine fields of [24, 64, 128] are 14.4 MB: twelve batches of two planes at 1 MB, five of five planes at 3 MB -- the last one
    ragged, four planes.)"""
    nl.check_cases_in_child("cross_dot", (([40, 32, 64], '3/2-rule'), ([24, 64, 128], None)), 1, 4 * TOL["double"],
                            MFFT_NLZ_BATCH_MB=batch_mb, MFFT_NLZ_ALIGN=align)


def test_nonlinear_cross_dot_kill_switch():
    """MFFT_NO_NLZ=1 (read once per process: a fresh one): the same call, the plan's composition, the same answer."""
    nl.check_cases_in_child("cross_dot", [([32, 64, 128], d) for d in ('3/2-rule', '2/3-rule', None)], 0, 4 * TOL["double"], MFFT_NO_NLZ="1")


_RANKS_REF = {}


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_nonlinear_cross_dot_ranks_against_oracle(P, dealias):
    """Several ranks, slab, the fused route (nine inverse exchanges, four forward): gathered results against the oracle's
    one-rank composition on the global spectra."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = np.array([32, 64, 64])
    if dealias not in _RANKS_REF:
        A, B, C = _spectra(None, N, "double", 321, True)
        _RANKS_REF[dealias] = (A, B, C) + _oracle(A, B, C, N, "double", dealias)
    A, B, C, want, swant = _RANKS_REF[dealias]

    def work(comm):
        F = Slab_R2C(N, L, comm, "double")
        sl = tuple(F.complex_local_slice())
        cs = tuple(F.complex_shape())
        out, s = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty(cs, F.complex)
        da, db, dc = (DeviceArray.from_numpy(np.ascontiguousarray(X[(slice(None),) + sl])) for X in (A, B, C))
        spectral.cross_dot_transform(F, da, db, dc, out, s, dealias)
        F.sync()
        assert F.plan_info(INFO[dealias]) == 1
        return sl, out.get(), s.get()

    G, Gs = np.zeros_like(want), np.zeros_like(swant)
    for sl, part, spart in run_ranks(P, work):
        G[(slice(None),) + sl] = part
        Gs[sl] = spart
    e, es = orc.rel_l2(G, want), orc.rel_l2(Gs, swant)
    print("cross_dot_transform P=%d %s: rel-L2 cross %.3e dot %.3e" % (P, dealias, e, es))
    assert e < 4 * TOL["double"] and es < 4 * TOL["double"]


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("decomp,P", [("slab", 4), ("pencilX", 4), ("pencilY", 4)])
def test_nonlinear_cross_dot_ranks(decomp, P, dealias):
    """Several ranks: same results as cross_transform + dot_transform of the same plan (pencils: the plan composes it, the
    fused flag is 0; slab: fused, 2/3-rule included); in place, the untouched inputs bitwise."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = np.array([16, 32, 32])

    def work(comm):
        if decomp == "slab":
            F = Slab_R2C(N, L, comm, "double")
        else:
            F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment=decomp[-1])
        rng = np.random.default_rng(78 + comm.Get_rank())
        cs = tuple(F.complex_shape())
        a, b, c = (DeviceArray.empty((3,) + cs, F.complex) for _ in range(3))
        for x in (a, b, c):                                        # spectra of real fields
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.5), x.component(i))
        want, got = (DeviceArray.empty((3,) + cs, F.complex) for _ in range(2))
        swant, sgot = (DeviceArray.empty(cs, F.complex) for _ in range(2))
        spectral.cross_transform(F, a, b, want, dealias)
        spectral.dot_transform(F, a, c, swant, dealias)
        spectral.cross_dot_transform(F, a, b, c, got, sgot, dealias)
        F.sync()
        assert F.plan_info(INFO[dealias]) == (1 if decomp == "slab" else 0)
        b0, c0 = b.get(), c.get()
        spectral.cross_dot_transform(F, a, b, c, a, c.component(1), dealias)
        F.sync()
        c1 = c.get()
        assert np.array_equal(b.get(), b0) and np.array_equal(c1[0], c0[0]) and np.array_equal(c1[2], c0[2])
        w, sw = want.get(), swant.get()
        return max(orc.rel_l2(got.get(), w), orc.rel_l2(sgot.get(), sw), orc.rel_l2(a.get(), w), orc.rel_l2(c1[1], sw))

    errs = run_ranks(P, work)
    assert max(errs) < 1e-13, errs


def test_plan_info_fused_keys():
    """The smallest mesh the fused route takes: every "nonlinear[_dot|_cross_dot][_absmax]_fused_<mode>" key the plan has -- three
    products and the two with maxima, three modes each, fifteen -- answers 0 or 1; both products with maxima is no key."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), "double")
    keys = nl.fused_keys()
    assert len(set(keys)) == 15, keys
    for key in keys:
        assert F.plan_info(key) in (0, 1), key
    with pytest.raises(_lib.MfftError):
        F.plan_info("nonlinear_cross_dot_absmax_fused_none")


# ---- stage level ----------------------------------------------------------------------------------------------------
def _stage_case(n, prec, valid, inplace):
    from mpifft4py_amd import DeviceArray, _lib
    rng = np.random.default_rng(n + valid)
    nrows = 37
    pitch = valid + 3
    a, b, c = ((rng.random((3, nrows, pitch)) - 0.5 + 1j * (rng.random((3, nrows, pitch)) - 0.5)).astype(cdtype(prec)) for _ in range(3))
    da, db, dc = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b), DeviceArray.from_numpy(c)
    if inplace:
        do, ds = da, dc.component(2)
    else:
        do = DeviceArray.from_numpy(np.full((3, nrows, pitch), 7 + 7j, dtype=cdtype(prec)))
        ds = DeviceArray.from_numpy(np.full((nrows, pitch), 7 + 7j, dtype=cdtype(prec)))
    _lib.call("mfft_nlz_cross_dot_rows", da.ptr, db.ptr, dc.ptr, do.ptr, ds.ptr, nrows, n, pitch, valid, _lib.precision_code(prec), 1)

    def back(x):
        x = x[..., :valid].astype(np.complex128)
        x[..., 0] = x[..., 0].real
        if valid == n // 2 + 1 and n % 2 == 0:
            x[..., -1] = x[..., -1].real
        return np.fft.irfft(x, n=n, axis=-1)
    ua, ub, uc = back(a), back(b), back(c)
    want = np.fft.rfft(np.cross(ua, ub, axis=0), axis=-1)[..., :valid]
    swant = np.fft.rfft(np.sum(ua * uc, 0), axis=-1)[:, :valid]
    got, sgot = do.get(), ds.get()
    e, es = orc.rel_l2(got[..., :valid], want), orc.rel_l2(sgot[:, :valid], swant)
    print("nlz_cross_dot_rows n=%d valid=%d %s%s rel-L2 cross %.3e dot %.3e" % (n, valid, prec, " in place" if inplace else "", e, es))
    assert e < 4 * TOL[prec] and es < 4 * TOL[prec]
    if inplace:      # nothing is stored beyond `valid`; the inputs the results do not lie over are preserved
        assert np.array_equal(got[..., valid:], a[..., valid:]) and np.array_equal(sgot[:, valid:], c[2][:, valid:])
        gc = dc.get()
        assert np.array_equal(db.get(), b) and np.array_equal(gc[0], c[0]) and np.array_equal(gc[1], c[1])
    else:
        assert np.all(got[..., valid:] == 7 + 7j) and np.all(sgot[:, valid:] == 7 + 7j)
        assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b) and np.array_equal(dc.get(), c)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", _nlz_lengths())      # EVERY length with a kernel: 2^a, 3 * 2^a, 9 * 2^a / 27 * 2^a / 81 * 2^a plans
def test_nlz_cross_dot_rows_against_numpy(n, prec):
    """mfft_nlz_cross_dot_rows == rfft(irfft(a) x irfft(b)) and rfft(sum_f irfft(a_f) irfft(c_f)) row by row, every bin and the
    n/3 + 1 bins of the 3/2-rule; an odd number of rows; nothing stored beyond `valid`; once more in place (out over a, s over
    c[2])."""
    for valid in (n // 2 + 1, n // 3 + 1):
        _stage_case(n, prec, valid, False)
        _stage_case(n, prec, valid, True)


def test_nlz_cross_dot_rows_unsupported_length():
    from mpifft4py_amd import DeviceArray, _lib
    a = DeviceArray.zeros((3, 4, 51), np.complex128)
    out = DeviceArray.zeros((3, 4, 51), np.complex128)
    s = DeviceArray.zeros((4, 51), np.complex128)
    with pytest.raises(_lib.MfftError):
        _lib.call("mfft_nlz_cross_dot_rows", a.ptr, a.ptr, a.ptr, out.ptr, s.ptr, 4, 100, 51, 51, _lib.DOUBLE, 1)


# ---- the example ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_boussinesq_one_operation_equals_two_calls(dealias):
    """Taylor-Green velocity and a random scalar at 32^3 over 10 steps: one cross_dot_transform per stage and cross_transform +
    dot_transform agree to rounding on U_hat and theta_hat; without buoyancy the mean of theta (bin 0) does not change (the
    velocity is divergence-free); and the state did change."""
    import boussinesq_device as demo
    from mpifft4py_amd import SelfComm
    N = np.array([32, 32, 32])
    F = demo.make_plan(SelfComm(0), N)
    U0, th0 = demo.taylor_green_hat(F), demo.random_scalar_hat(F, seed=9)
    u0, t0 = U0.get(), th0.get()
    rep = {}
    U1, t1 = demo.solve(SelfComm(0), N, U0, th0, 0.000625, 0.02, 0.01, 10, dealias, one_op=True, FFT=F, report=rep)
    u1, t1 = U1.get(), t1.get()
    U2, t2 = demo.solve(SelfComm(0), N, U0, th0, 0.000625, 0.02, 0.01, 10, dealias, one_op=False, FFT=F)
    u2, t2 = U2.get(), t2.get()
    assert rep["fused"] == 1
    assert np.array_equal(U0.get(), u0) and np.array_equal(th0.get(), t0)
    eu, et = orc.rel_l2(u1, u2), orc.rel_l2(t1, t2)
    d0 = abs(t1[0, 0, 0] - t0[0, 0, 0])
    print("boussinesq, %s: one operation against two calls rel-L2 U %.3e theta %.3e; bin 0 moved by %.3e (largest bin %.3e)"
          % (dealias, eu, et, d0, np.abs(t0).max()))
    assert eu < 1e-12 and et < 1e-12
    # bin 0 receives rounding errors of the transforms, which scale with the largest bin they carry
    assert d0 < 1e-12 * np.abs(t0).max()
    assert orc.rel_l2(u1, u0) > 1e-4 and orc.rel_l2(t1, t0) > 1e-4            # ... and something did happen


def test_boussinesq_buoyancy_one_operation_equals_two_calls():
    """With buoyancy the scalar drives the velocity: both loops still agree to rounding."""
    import boussinesq_device as demo
    from mpifft4py_amd import SelfComm
    N = np.array([32, 32, 32])
    F = demo.make_plan(SelfComm(0), N)
    U0, th0 = demo.taylor_green_hat(F), demo.random_scalar_hat(F, seed=9)
    r1 = demo.solve(SelfComm(0), N, U0, th0, 0.000625, 0.02, 0.01, 10, "3/2-rule", one_op=True, g=1.0, FFT=F)
    r2 = demo.solve(SelfComm(0), N, U0, th0, 0.000625, 0.02, 0.01, 10, "3/2-rule", one_op=False, g=1.0, FFT=F)
    r0 = demo.solve(SelfComm(0), N, U0, th0, 0.000625, 0.02, 0.01, 10, "3/2-rule", one_op=True, g=0.0, FFT=F)
    assert orc.rel_l2(r1[0].get(), r2[0].get()) < 1e-12 and orc.rel_l2(r1[1].get(), r2[1].get()) < 1e-12
    assert orc.rel_l2(r1[0].get(), r0[0].get()) > 1e-6                        # the buoyancy term did act on the velocity


# ---- scale ------------------------------------------------------------------------------------------------------------
def test_nonlinear_cross_dot_512_padded_against_two_calls():
    """512^3 with the 3/2-rule, double: the fused operation against cross_transform + dot_transform of the same plan, and the
    work-buffer bill: below the composition's thirteen real arrays of 768^3 x 8 B = 47.1 GB alone."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([512, 512, 512])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    cs = tuple(F.complex_shape())
    a, b, c = (DeviceArray.empty((3,) + cs, F.complex) for _ in range(3))
    for k, x in enumerate((a, b, c)):
        for i in range(3):
            F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=200 + 3 * k + i), x.component(i))
    got, sgot = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty(cs, F.complex)
    spectral.cross_dot_transform(F, a, b, c, got, sgot, "3/2-rule")
    F.sync()
    assert F.plan_info("nonlinear_cross_dot_fused_3_2") == 1
    nbytes = F.plan_info("nonlinear_bytes")
    print("nonlinear_bytes at 512^3, 3/2-rule, cross and dot: %.3f GB (composition: %.3f GB of real arrays)" % (nbytes / 1e9, 13 * 768 ** 3 * 8 / 1e9))
    assert nbytes < 13 * 768 ** 3 * 8
    want, swant = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty(cs, F.complex)
    spectral.dot_transform(F, a, c, swant, "3/2-rule")
    spectral.cross_transform(F, a, b, want, "3/2-rule")
    # rel-L2 on the device (the arrays are 3.2 GB and 1.1 GB): got <- got - want
    spectral.axpbz(F, got, got, want, 1.0, -1.0)
    spectral.axpbz(F, sgot, sgot, swant, 1.0, -1.0)
    e = np.sqrt(spectral.sumsq(F, got) / spectral.sumsq(F, want))
    es = np.sqrt(spectral.sumsq(F, sgot) / spectral.sumsq(F, swant))
    print("512^3: one operation against two calls rel-L2 cross %.3e dot %.3e" % (e, es))
    assert e < 1e-12 and es < 1e-12
