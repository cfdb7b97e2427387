"""GPU: the advection term of a transported scalar, fftn(sum_f ifftn(a_f) ifftn(b_f)), as one plan operation
(mfft_nonlinear_dot; csrc/fft_nlz.h body_dot) against the ORACLE's transforms -- what a caller composes from six FFT.ifftn,
np.sum(ua * ub, 0) and one FFT.fftn -- on the same seeded spectra, through the C ABI; its stages on their own against numpy;
and the passive-scalar example against the exact RK4 answer of a uniform velocity."""
import ctypes
import os
import sys

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, TOL, cdtype, have_gpu, orc, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
INFO = {d: nl.info_key("dot", d) for d in nl.RULE}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _spectra(F, N, prec, seed, hermitian):
    return nl.spectra(tuple(F.complex_shape()), N, prec, seed, hermitian)


def _oracle_dot(a, b, N, prec, dealias, mask=None):
    """fftn(sum_f ifftn(a_f) ifftn(b_f)) with the oracle's one-rank transforms in the mode `dealias`."""
    return nl.oracle("dot", (a, b), N, prec, dealias, mask)


def _one_rank(N, fused, dealias, prec, hermitian, complex_pitch=None):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=complex_pitch)
    a, b = _spectra(F, N, prec, 11 + int(N[2]), hermitian)
    mask = None
    if dealias == "2/3-rule":
        mask = F.get_dealias_filter()
    want = _oracle_dot(a, b, N, prec, dealias, mask)
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    out = F.empty_complex()
    spectral.dot_transform(F, da, db, out, dealias)
    F.sync()
    if fused:
        assert F.plan_info(INFO[dealias]) == 1
    e = orc.rel_l2(out.get(), want)
    print("dot_transform %s %s %s herm=%s rel-L2 %.3e (bound %.1e)" % (list(N), dealias, prec, hermitian, e, 4 * TOL[prec]))
    assert e < 4 * TOL[prec]
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)          # inputs preserved
    spectral.dot_transform(F, da, db, db.component(1), dealias)                  # the result over one component of the second field
    F.sync()
    got = db.get()
    assert orc.rel_l2(got[1], want) < 4 * TOL[prec]
    assert np.array_equal(da.get(), a) and np.array_equal(got[0], b[0]) and np.array_equal(got[2], b[2])


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,fused", [([32, 64, 128], True), ([8, 16, 32], True), ([128, 128, 128], True), ([36, 72, 144], True),
                                     ([108, 216, 432], True), ([16, 32, 24], None), ([20, 24, 40], None)])
def test_nonlinear_dot_one_rank(N, fused, dealias, prec):
    """One rank, slab, spectra of real fields: the fused route where every axis has its kernels, the plan's own composition
    otherwise -- both against the oracle; inputs preserved; the result over b_hat.component(1)."""
    _one_rank(N, fused, dealias, prec, True)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,fused", [([32, 64, 128], True), ([16, 32, 24], None)])
def test_nonlinear_dot_one_rank_arbitrary_spectra(N, fused, dealias, prec):
    """Arbitrary complex spectra: the bins a real field would not have follow the transforms' conventions."""
    _one_rank(N, fused, dealias, prec, False)


def test_nonlinear_dot_pitched_plan():
    """A plan whose spectra have rows a whole number of cache lines apart: the routes run on the pitched rows."""
    for dealias in ("3/2-rule", "2/3-rule", None):
        _one_rank([32, 64, 128], True, dealias, "double", True, complex_pitch="auto")


@pytest.mark.parametrize("batch_mb,align", [("1", "1"), ("1", "0"), ("4", "-1")])
def test_nonlinear_dot_batches(batch_mb, align):
    """Several batches of x planes (the last one ragged) and both row pitches of the intermediates: a fresh process,
    the switches are read once."""
    nl.check_cases_in_child("dot", (([40, 32, 64], '3/2-rule'), ([24, 64, 128], None)), 1, 4e-10, MFFT_NLZ_BATCH_MB=batch_mb, MFFT_NLZ_ALIGN=align)


def test_nonlinear_dot_kill_switch():
    """MFFT_NO_NLZ=1 (read once per process: a fresh one): the same call, the plan's composition, the same answer."""
    nl.check_cases_in_child("dot", [([32, 64, 128], d) for d in ('3/2-rule', '2/3-rule', None)], 0, 4e-10, MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
@pytest.mark.parametrize("P,pipeline", [(2, 1), (4, 4), (8, -2)])
def test_nonlinear_dot_ranks_against_oracle(P, pipeline, dealias):
    """Several ranks, slab, the fused route (six inverse exchanges, one forward): gathered result against the oracle's
    one-rank composition on the global spectra."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = np.array([32, 64, 64])
    rng = np.random.default_rng(321)
    A = np.stack([np.fft.rfftn(rng.random(tuple(N)) - 0.5) for _ in range(3)])
    B = np.stack([np.fft.rfftn(rng.random(tuple(N)) - 0.5) for _ in range(3)])
    want = _oracle_dot(A, B, N, "double", dealias)

    def work(comm):
        F = Slab_R2C(N, L, comm, "double", pipeline=pipeline)
        sl = tuple(F.complex_local_slice())
        out = DeviceArray.empty(tuple(F.complex_shape()), F.complex)
        spectral.dot_transform(F, DeviceArray.from_numpy(np.ascontiguousarray(A[(slice(None),) + sl])),
                               DeviceArray.from_numpy(np.ascontiguousarray(B[(slice(None),) + sl])), out, dealias)
        F.sync()
        assert F.plan_info(INFO[dealias]) == 1
        return sl, out.get()

    G = np.zeros_like(want)
    for sl, part in run_ranks(P, work):
        G[sl] = part
    assert orc.rel_l2(G, want) < 4 * TOL["double"]


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("decomp,P", [("slab", 4), ("pencilX", 4), ("pencilY", 4)])
def test_nonlinear_dot_ranks(decomp, P, dealias):
    """Several ranks: same call, same result as six ifftn + dot + one fftn issued by the caller (pencils: the plan composes
    it, the fused flag is 0; slab: fused, 2/3-rule included)."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = np.array([16, 32, 32])

    def work(comm):
        if decomp == "slab":
            F = Slab_R2C(N, L, comm, "double")
        else:
            F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment=decomp[-1])
        rng = np.random.default_rng(77 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a = DeviceArray.empty((3,) + cs, F.complex)
        b = DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):                                           # spectra of real fields
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.5), x.component(i))
        ua, ub = (DeviceArray.empty((3,) + ws, F.float) for _ in range(2))
        r = DeviceArray.empty(ws, F.float)
        for i in range(3):
            F.ifftn(a.component(i), ua.component(i), dealias)
            F.ifftn(b.component(i), ub.component(i), dealias)
        spectral.dot(F, ua, ub, r)
        want = DeviceArray.empty(cs, F.complex)
        F.fftn(r, want, None if dealias == "2/3-rule" else dealias)      # (the 2/3-rule filters what goes into the product)
        got = DeviceArray.empty(cs, F.complex)
        spectral.dot_transform(F, a, b, got, dealias)
        F.sync()
        assert F.plan_info(INFO[dealias]) == (1 if decomp == "slab" else 0)
        a0, b0 = a.get(), b.get()
        spectral.dot_transform(F, a, b, b.component(1), dealias)
        F.sync()
        b1 = b.get()
        assert np.array_equal(a.get(), a0) and np.array_equal(b1[0], b0[0]) and np.array_equal(b1[2], b0[2])
        return max(orc.rel_l2(got.get(), want.get()), orc.rel_l2(b1[1], want.get()))

    errs = run_ranks(P, work)
    assert max(errs) < 1e-13, errs


# ---- stage level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [16, 128, 1024, 4096, 12, 96, 768, 144, 432, 1296, 1728])      # 2^a, 3 * 2^a, 9 * 2^a / 27 * 2^a / 81 * 2^a plans
def test_nlz_dot_rows_against_numpy(n, prec):
    """mfft_nlz_dot_rows == rfft(sum_f irfft(a_f) irfft(b_f)) row by row, every bin and the n/3 + 1 bins of the 3/2-rule;
    an odd number of rows; nothing stored beyond `valid`."""
    from mpifft4py_amd import DeviceArray, _lib
    rng = np.random.default_rng(n)
    nrows = 37
    for valid in (n // 2 + 1, n // 3 + 1):
        pitch = valid + 3
        a = (rng.random((3, nrows, pitch)) - 0.5 + 1j * (rng.random((3, nrows, pitch)) - 0.5)).astype(cdtype(prec))
        b = (rng.random((3, nrows, pitch)) - 0.5 + 1j * (rng.random((3, nrows, pitch)) - 0.5)).astype(cdtype(prec))
        out = np.full((nrows, pitch), 7 + 7j, dtype=cdtype(prec))
        da, db, do = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b), DeviceArray.from_numpy(out)
        _lib.call("mfft_nlz_dot_rows", da.ptr, db.ptr, do.ptr, nrows, n, pitch, valid, _lib.precision_code(prec), 1)

        def back(x):
            x = x[..., :valid].astype(np.complex128)
            x[..., 0] = x[..., 0].real
            if valid == n // 2 + 1 and n % 2 == 0:
                x[..., -1] = x[..., -1].real
            return np.fft.irfft(x, n=n, axis=-1)
        want = np.fft.rfft(np.sum(back(a) * back(b), 0), axis=-1)[:, :valid]
        got = do.get()
        e = orc.rel_l2(got[:, :valid], want)
        print("nlz_dot_rows n=%d valid=%d %s rel-L2 %.3e" % (n, valid, prec, e))
        assert e < 4 * TOL[prec]
        assert np.all(got[:, valid:] == 7 + 7j)
        assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)


def test_nlz_dot_rows_unsupported_length():
    from mpifft4py_amd import DeviceArray, _lib
    a = DeviceArray.zeros((3, 4, 51), np.complex128)
    out = DeviceArray.zeros((4, 51), np.complex128)
    with pytest.raises(_lib.MfftError):
        _lib.call("mfft_nlz_dot_rows", a.ptr, a.ptr, out.ptr, 4, 100, 51, 51, _lib.DOUBLE, 1)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("complex_pitch", [None, "auto"])
def test_ew_dot_and_grad_hat_against_numpy(prec, complex_pitch):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([16, 32, 24])
    F = Slab_R2C(N, np.array([2 * np.pi, 4 * np.pi, 2 * np.pi]), SelfComm(0), prec, complex_pitch=complex_pitch)
    rng = np.random.default_rng(5)
    rs, cs = tuple(F.real_shape()), tuple(F.complex_shape())
    a = (rng.random((3,) + rs) - 0.5).astype(rdtype(prec))
    b = (rng.random((3,) + rs) - 0.5).astype(rdtype(prec))
    out = DeviceArray.empty(rs, F.float)
    spectral.dot(F, DeviceArray.from_numpy(a), DeviceArray.from_numpy(b), out)
    F.sync()
    tol = 1e-14 if prec == "double" else 1e-6
    assert np.allclose(out.get(), np.sum(a.astype(np.float64) * b, 0), rtol=tol, atol=tol)
    K = np.array(F.get_local_wavenumbermesh(scaled=True, broadcast=True))
    Kd = spectral.Wavenumbers(F)
    s = (rng.random(cs) - 0.5 + 1j * (rng.random(cs) - 0.5)).astype(cdtype(prec))
    ds, dg = F.empty_complex().set(s), F.empty_complex(3)
    spectral.grad_hat(F, Kd, ds, dg)
    F.sync()
    assert np.allclose(dg.get(), 1j * K * s.astype(np.complex128), rtol=tol, atol=tol)
    assert np.array_equal(ds.get(), s)


# ---- the example ------------------------------------------------------------------------------------------------------
def _no_nyquist(x, N):
    """Zero the Nyquist planes of a half-spectrum: the derivative of a Nyquist mode is not the spectrum of a real field, and the
    real transforms drop what is not (Im of the kz = 0 and kz = N/2 bins), so only the other modes obey the formula below."""
    x = x.copy()
    x[N[0] // 2, :, :] = 0
    x[:, N[1] // 2, :] = 0
    x[:, :, N[2] // 2] = 0
    return x


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_passive_scalar_uniform_velocity_known_answer(dealias):
    """A uniform velocity c (only the k = 0 bin of U_hat is non-zero) couples no two modes: every mode obeys
    theta_k(n dt) = theta_k(0) R(z_k)^n exactly, z_k = (-i k.c - kappa |k|^2) dt, R the RK4 stability polynomial.  Compared on
    the modes the rule keeps (2/3-rule: the filter's; all rules: not the Nyquist planes, see _no_nyquist)."""
    import passive_scalar_device as demo
    from mpifft4py_amd import DeviceArray, SelfComm
    N = np.array([32, 32, 32])
    F = demo.make_plan(SelfComm(0), N)
    c = np.array([0.7, -1.1, 0.4])
    kappa, dt, steps = 0.02, 0.01, 10
    U = F.empty_complex(3)
    for f in range(3):
        F.fftn(DeviceArray.from_numpy(np.full(tuple(N), c[f])), U.component(f))
    rng = np.random.default_rng(2024)
    th0 = F.empty_complex()
    F.fftn(DeviceArray.from_numpy(rng.random(tuple(N)) - 0.5), th0)
    t0 = _no_nyquist(th0.get(), N)
    K = np.array(F.get_local_wavenumbermesh(scaled=True, broadcast=True))
    z = (-1j * np.tensordot(c, K, 1) - kappa * np.sum(K * K, 0)) * dt
    R = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24
    want = t0 * R ** steps
    got = demo.solve(SelfComm(0), N, U, t0, kappa, dt, steps, dealias, fused=True, FFT=F).get()
    assert F.plan_info(INFO[dealias]) == 1
    keep = np.ones(t0.shape, dtype=bool) if dealias != "2/3-rule" else np.asarray(F.get_dealias_filter()).astype(bool)
    e = orc.rel_l2(got[keep], want[keep])
    print("passive scalar, uniform velocity, %s: rel-L2 %.3e (bound %.1e)" % (dealias, e, 4 * TOL["double"]))
    assert e < 4 * TOL["double"]


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_passive_scalar_taylor_green_fused_equals_composed(dealias):
    """Taylor-Green velocity: the plan operation and the caller-side composition agree to rounding, and the mean of theta
    (bin 0) does not change (the velocity is divergence-free)."""
    import passive_scalar_device as demo
    from mpifft4py_amd import SelfComm
    N = np.array([32, 32, 32])
    F = demo.make_plan(SelfComm(0), N)
    U, th0 = demo.taylor_green_hat(F), demo.random_scalar_hat(F, seed=9)
    t0 = th0.get()
    rep = {}
    tf = demo.solve(SelfComm(0), N, U, th0, 0.02, 0.01, 10, dealias, fused=True, FFT=F, report=rep).get()
    tc = demo.solve(SelfComm(0), N, U, th0, 0.02, 0.01, 10, dealias, fused=False, FFT=F).get()
    assert rep["fused_dot"] == 1
    assert np.array_equal(th0.get(), t0)
    assert orc.rel_l2(tf, tc) < 1e-12
    # bin 0 receives rounding errors of the transforms, which scale with the largest bin they carry
    d0 = abs(tf[0, 0, 0] - t0[0, 0, 0])
    print("passive scalar, Taylor-Green, %s: bin 0 moved by %.3e (largest bin %.3e)" % (dealias, d0, np.abs(t0).max()))
    assert d0 < 1e-12 * np.abs(t0).max()
    assert orc.rel_l2(tf, t0) > 1e-4            # ... and something did happen


# ---- scale ------------------------------------------------------------------------------------------------------------
def test_nonlinear_dot_512_padded_against_composition():
    """512^3 with the 3/2-rule: the fused operation against six ifftn + dot + one fftn of the same plan, and the work-buffer
    bill: below the composition's seven real arrays of 768^3 x 8 B = 25.4 GB alone."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([512, 512, 512])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    cs, ws = tuple(F.complex_shape()), tuple(F.work_shape("3/2-rule"))
    a = DeviceArray.empty((3,) + cs, F.complex)
    b = DeviceArray.empty((3,) + cs, F.complex)
    for s, x in enumerate((a, b)):
        for i in range(3):
            F.fftn(DeviceArray.random(F.real_shape(), F.float, seed=100 + 3 * s + i), x.component(i))
    got = DeviceArray.empty(cs, F.complex)
    spectral.dot_transform(F, a, b, got, "3/2-rule")
    F.sync()
    assert F.plan_info("nonlinear_dot_fused_3_2") == 1
    nbytes = F.plan_info("nonlinear_bytes")
    print("nonlinear_bytes at 512^3, 3/2-rule, dot: %.3f GB (composition: %.3f GB of real arrays)" % (nbytes / 1e9, 7 * 768 ** 3 * 8 / 1e9))
    assert nbytes < 7 * 768 ** 3 * 8
    ua, ub = (DeviceArray.empty((3,) + ws, F.float) for _ in range(2))
    for i in range(3):
        F.ifftn(a.component(i), ua.component(i), "3/2-rule")
        F.ifftn(b.component(i), ub.component(i), "3/2-rule")
    r = ua.component(0)                          # the product over the first input (mfft_ew_dot allows it): six real arrays, not seven
    spectral.dot(F, ua, ub, r)
    want = DeviceArray.empty(cs, F.complex)
    F.fftn(r, want, "3/2-rule")
    F.sync()
    assert orc.rel_l2(got.get(), want.get()) < 1e-12
