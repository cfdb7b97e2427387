"""GPU: the outer product of two vector fields, out_hat[3 i + j] = fftn(ifftn(a_hat[i]) ifftn(b_hat[j])), as one plan operation
(mfft_nonlinear_outer; csrc/fft_nlz.h body_outer) against the ORACLE's transforms -- what a caller composes from six FFT.ifftn,
nine products and nine FFT.fftn -- on the same seeded spectra, through the C ABI: one rank fused and composed, pitched spectra,
batches and the kill switch in fresh processes, several slab ranks and a pencil grid; its z stage on its own against numpy; the
Elsasser right-hand side against numpy; and the MHD example, fused against composed and against the Alfven wave it must carry."""
import os
import sys

import numpy as np
import pytest

import nonlinear_util as nl
import outer_util as ou
from gpu_util import L, TOL, cdtype, have_gpu, orc, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
DEALIAS = ["3/2-rule", "2/3-rule", None]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _nlz_lengths():
    from emu_util import nlz_lengths
    out = nlz_lengths()
    assert len(out) == 32, out
    return sorted(out)


_REF = {}      # the spectra and the oracle's answer of a case, computed once and left unchanged


def _reference(F, N, prec, dealias, hermitian):
    key = (tuple(int(n) for n in N), prec, dealias, hermitian)
    if key not in _REF:
        a, b = nl.spectra(tuple(F.complex_shape()), N, prec, 17 + int(N[2]), hermitian, 2)
        mask = F.get_dealias_filter() if dealias == "2/3-rule" else None
        want = ou.oracle(a, b, np.array(N), prec, dealias, mask)
        sym = ou.oracle(a, a, np.array(N), prec, dealias, mask)
        for x in (a, b, want, sym):
            x.setflags(write=False)
        _REF[key] = (a, b, want, sym)
    return _REF[key]


def _one_rank(N, fused, dealias, prec, hermitian, complex_pitch=None):
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=complex_pitch)
    a, b, want, sym = _reference(F, N, prec, dealias, hermitian)
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    out = F.empty_complex(9)
    assert spectral.outer_transform(F, da, db, out, dealias) is out
    F.sync()
    if fused == "z":      # the composed route wherever the z length the mode works on (the padded one under the 3/2-rule) has no kernel
        if (int(N[2]) * 3 // 2 if dealias == "3/2-rule" else int(N[2])) not in _nlz_lengths():
            assert F.plan_info(ou.info_key(dealias)) == 0
    elif fused is not None:
        assert F.plan_info(ou.info_key(dealias)) == (1 if fused else 0)
    got = out.get()
    e = orc.rel_l2(got, want)
    worst = max(orc.rel_l2(got[c], want[c]) for c in range(9))
    print("outer_transform %s %s %s herm=%s rel-L2 %.3e, worst component %.3e (bound %.1e)" % (list(N), dealias, prec, hermitian, e, worst, 4 * TOL[prec]))
    assert e < 4 * TOL[prec] and worst < 4 * TOL[prec]
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)      # inputs preserved, bit for bit
    spectral.outer_transform(F, da, da, out, dealias)                       # a_hat is b_hat: the symmetric tensor, all nine
    F.sync()
    got = out.get()
    assert orc.rel_l2(got, sym) < 4 * TOL[prec]
    assert np.array_equal(da.get(), a)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS)
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([16, 16, 128], True), ([16, 32, 96], True), ([24, 48, 144], True),
                                     ([16, 32, 24], "z"), ([20, 24, 40], "z")])
def test_nonlinear_outer_one_rank(N, fused, dealias, prec):
    """One rank, slab, spectra of real fields: the fused route where every axis has its kernels (flag 1: the 8-values single- and
    multi-pass plans, the 12 / 12.12 / 12.6.3 plans and their padded images), the plan's own composition where a mode's z length
    has none -- both against the oracle; inputs preserved bit for bit; then a_hat is b_hat against the oracle's symmetric tensor."""
    _one_rank(N, fused, dealias, prec, True)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS)
@pytest.mark.parametrize("N,fused", [([16, 16, 128], True), ([16, 32, 24], None)])
def test_nonlinear_outer_one_rank_arbitrary_spectra(N, fused, dealias, prec):
    """Arbitrary complex spectra: the bins a real field would not have follow the transforms' conventions."""
    _one_rank(N, fused, dealias, prec, False)


def test_nonlinear_outer_pitched_plan():
    """A plan whose spectra have rows a whole number of cache lines apart: the routes run on the pitched rows."""
    for dealias in DEALIAS:
        _one_rank([16, 16, 128], True, dealias, "double", True, complex_pitch="auto")


@pytest.mark.parametrize("N", [[8, 16, 32], [20, 24, 40]])
def test_nonlinear_outer_overlap_is_rejected(N):
    """out_hat overlapping an input -- here a_hat, then b_hat, lying inside out_hat -- raises before anything runs: every array
    comes back as it was.  (Fused and composed plan.)"""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib, spectral
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), "double")
    cs = tuple(int(x) for x in F.complex_shape())
    b = nl.spectra(cs, N, "double", 5, True, 1)[0]
    rng = np.random.default_rng(4)
    o = (rng.random((9,) + cs) + 1j * rng.random((9,) + cs)).astype(np.complex128)
    out = F.empty_complex(9).set(o)
    other = F.empty_complex(3).set(b)
    for first in (0, 2, 6):      # the view starts at out_hat's first, third and seventh component
        inside = DeviceArray((3,) + cs, F.complex, ptr=out.component(first).ptr, owner=False, pitch=out.pitch)
        for args in ((inside, other), (other, inside)):
            with pytest.raises(_lib.MfftError):
                spectral.outer_transform(F, args[0], args[1], out, None)
    F.sync()
    assert np.array_equal(out.get(), o) and np.array_equal(other.get(), b)


@pytest.mark.parametrize("align", ["0", "1"])
def test_nonlinear_outer_batches(align):
    """Several batches of x planes and both row pitches of the intermediates: a fresh process, the switches are read once.  The
    batch is sized from max(nin, nout) = 9 fields: [24, 32, 64] is 9 x 16.9 KB per plane with compact rows -- four batches of six
    planes at 1 MB -- and 9 x 20.5 KB with aligned rows: five batches, the last one ragged (four planes of five); [16, 16, 32] under
    the 3/2-rule is two batches of twelve padded planes."""
    ou.check_cases_in_child((([16, 16, 32], '3/2-rule'), ([24, 32, 64], None), ([24, 32, 64], '2/3-rule')), 1, 4 * TOL["double"],
                            MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_nonlinear_outer_kill_switch():
    """MFFT_NO_NLZ=1 (read once per process: a fresh one): the same call, the plan's composition, the same answer."""
    ou.check_cases_in_child([([16, 16, 32], d) for d in ('3/2-rule', '2/3-rule', None)], 0, 4 * TOL["double"], MFFT_NO_NLZ="1")


_RANKS_REF = {}


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
@pytest.mark.parametrize("P", [2, 4])
def test_nonlinear_outer_ranks_against_oracle(P, dealias):
    """Several ranks, slab, the fused route (six inverse exchanges, nine forward): gathered results against the oracle's one-rank
    composition on the global spectra."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    N = np.array([16, 32, 32])
    if dealias not in _RANKS_REF:
        A, B = nl.spectra(None, N, "double", 321, True, 2)
        _RANKS_REF[dealias] = (A, B, ou.oracle(A, B, N, "double", dealias))
    A, B, want = _RANKS_REF[dealias]

    def work(comm):
        F = Slab_R2C(N, L, comm, "double")
        sl = tuple(F.complex_local_slice())
        cs = tuple(F.complex_shape())
        out = DeviceArray.empty((9,) + cs, F.complex)
        da, db = (DeviceArray.from_numpy(np.ascontiguousarray(X[(slice(None),) + sl])) for X in (A, B))
        spectral.outer_transform(F, da, db, out, dealias)
        F.sync()
        assert F.plan_info(ou.info_key(dealias)) == 1
        assert np.array_equal(da.get(), A[(slice(None),) + sl]) and np.array_equal(db.get(), B[(slice(None),) + sl])
        return sl, out.get()

    G = np.zeros_like(want)
    for sl, part in run_ranks(P, work):
        G[(slice(None),) + sl] = part
    e = orc.rel_l2(G, want)
    print("outer_transform P=%d %s: rel-L2 %.3e" % (P, dealias, e))
    assert e < 4 * TOL["double"]


@pytest.mark.parametrize("dealias", DEALIAS)
def test_nonlinear_outer_pencil_grid(dealias):
    """A 2 x 2 pencil grid: the plan composes the operation (flag 0).  Spectra of real fields made by the plan's own fftn, the
    result against the caller's composition from the same plan's ifftn, spectral.mul and fftn."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 32])

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(78 + comm.Get_rank())
        cs, ws = tuple(int(x) for x in F.complex_shape()), tuple(int(x) for x in F.work_shape(dealias))
        a, b = (DeviceArray.empty((3,) + cs, F.complex) for _ in range(2))
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.5), x.component(i))
        ra, rb = (DeviceArray.empty((3,) + ws, F.float) for _ in range(2))
        for x, u in ((a, ra), (b, rb)):
            for i in range(3):
                F.ifftn(x.component(i), u.component(i), dealias)
        w, want = DeviceArray.empty(ws, F.float), DeviceArray.empty((9,) + cs, F.complex)
        for i in range(3):
            for j in range(3):
                spectral.mul(F, ra.component(i), rb.component(j), w)
                F.fftn(w, want.component(3 * i + j), dealias)
        a0, b0 = a.get(), b.get()
        got = DeviceArray.empty((9,) + cs, F.complex)
        spectral.outer_transform(F, a, b, got, dealias)
        F.sync()
        assert F.plan_info(ou.info_key(dealias)) == 0
        assert np.array_equal(a.get(), a0) and np.array_equal(b.get(), b0)
        return orc.rel_l2(got.get(), want.get())

    errs = run_ranks(4, work)
    assert max(errs) < 1e-13, errs


def test_plan_info_outer_keys():
    """The three keys of the operation on the smallest mesh the fused route takes: 1 for the 3/2-rule and None, 0 or 1 for the
    2/3-rule (1 once the plan holds its mask); there is no maxima build."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), "double")
    assert F.plan_info(ou.info_key("3/2-rule")) == 1 and F.plan_info(ou.info_key(None)) == 1
    assert F.plan_info(ou.info_key("2/3-rule")) in (0, 1)
    with pytest.raises(_lib.MfftError):
        F.plan_info("nonlinear_outer_absmax_fused_none")


# ---- stage level ----------------------------------------------------------------------------------------------------
def _stage_case(n, prec, valid, inplace, nrows=37):
    from mpifft4py_amd import DeviceArray, _lib
    rng = np.random.default_rng(n + valid + nrows)
    pitch = valid + 3
    a, b = ((rng.random((3, nrows, pitch)) - 0.5 + 1j * (rng.random((3, nrows, pitch)) - 0.5)).astype(cdtype(prec)) for _ in range(2))
    if inplace:      # components 0..5 of out are the six input components: a and b are the head of ONE array of nine
        hold = np.full((9, nrows, pitch), 7 + 7j, dtype=cdtype(prec))
        hold[:3], hold[3:6] = a, b
        do = DeviceArray.from_numpy(hold)
        pa, pb = do.ptr, do.component(3).ptr
    else:
        da, db = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b)
        do = DeviceArray.from_numpy(np.full((9, nrows, pitch), 7 + 7j, dtype=cdtype(prec)))
        pa, pb = da.ptr, db.ptr
    _lib.call("mfft_nlz_outer_rows", pa, pb, do.ptr, nrows, n, pitch, valid, _lib.precision_code(prec), 1)

    def back(x):
        x = x[..., :valid].astype(np.complex128)
        x[..., 0] = x[..., 0].real
        if valid == n // 2 + 1 and n % 2 == 0:
            x[..., -1] = x[..., -1].real
        return np.fft.irfft(x, n=n, axis=-1)
    ua, ub = back(a), back(b)
    want = np.stack([np.fft.rfft(ua[i] * ub[j], axis=-1)[..., :valid] for i in range(3) for j in range(3)])
    got = do.get()
    e = orc.rel_l2(got[..., :valid], want)
    worst = max(orc.rel_l2(got[c][..., :valid], want[c]) for c in range(9))
    print("nlz_outer_rows n=%d valid=%d rows=%d %s%s rel-L2 %.3e worst component %.3e" % (n, valid, nrows, prec, " in place" if inplace else "", e, worst))
    assert e < 4 * TOL[prec] and worst < 4 * TOL[prec]
    if inplace:      # nothing is stored beyond `valid`
        assert np.array_equal(got[:3, :, valid:], a[..., valid:]) and np.array_equal(got[3:6, :, valid:], b[..., valid:])
        assert np.all(got[6:, :, valid:] == 7 + 7j)
    else:
        assert np.all(got[..., valid:] == 7 + 7j)
        assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", _nlz_lengths())      # EVERY length with a kernel: 2^a, 3 * 2^a, 9 * 2^a / 27 * 2^a / 81 * 2^a plans
def test_nlz_outer_rows_against_numpy(n, prec):
    """mfft_nlz_outer_rows == rfft(irfft(a_i) irfft(b_j)) row by row, every bin and the n/3 + 1 bins of the 3/2-rule; an odd number
    of rows (37) and a single row; out of place nothing is stored beyond `valid` and the inputs are preserved; once more in place,
    components 0..5 over the inputs."""
    for valid in (n // 2 + 1, n // 3 + 1):
        _stage_case(n, prec, valid, False)
        _stage_case(n, prec, valid, True)
    _stage_case(n, prec, n // 2 + 1, True, nrows=1)
    _stage_case(n, prec, n // 3 + 1, False, nrows=1)


def test_nlz_outer_rows_unsupported_length():
    from mpifft4py_amd import DeviceArray, _lib
    a = DeviceArray.zeros((3, 4, 51), np.complex128)
    out = DeviceArray.zeros((9, 4, 51), np.complex128)
    with pytest.raises(_lib.MfftError):
        _lib.call("mfft_nlz_outer_rows", a.ptr, a.ptr, out.ptr, 4, 100, 51, 51, _lib.DOUBLE, 1)


# ---- the right-hand side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("pitch", [None, "auto"])
def test_elsasser_rhs_against_numpy(pitch, prec):
    """elsasser_rhs == the formulas of its docstring in numpy complex128 at [8, 16, 32], compact and pitched spectra; the K = 0 bin
    of both results is exactly zero."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=pitch)
    cs = tuple(int(x) for x in F.complex_shape())
    rng = np.random.default_rng(31)
    rnd = lambda n: (rng.random((n,) + cs) - 0.5 + 1j * (rng.random((n,) + cs) - 0.5)).astype(cdtype(prec))
    T, Zp, Zm = rnd(9), rnd(3), rnd(3)
    nu, eta = 0.03, 0.011
    K = spectral.Wavenumbers(F)
    dT, dZp, dZm = F.empty_complex(9).set(T), F.empty_complex(3).set(Zp), F.empty_complex(3).set(Zm)
    gp, gm = F.empty_complex(3), F.empty_complex(3)
    spectral.elsasser_rhs(F, K, dT, dZp, dZm, gp, gm, nu, eta)
    F.sync()
    Kv = [np.asarray(k, dtype=np.float64) for k in F.get_local_wavenumbermesh(scaled=True)]
    Kv = [np.broadcast_to(k, cs) for k in Kv]
    k2 = Kv[0] ** 2 + Kv[1] ** 2 + Kv[2] ** 2
    T64, Zp64, Zm64 = T.astype(np.complex128), Zp.astype(np.complex128), Zm.astype(np.complex128)
    Np = np.stack([-1j * sum(Kv[j] * T64[3 * i + j] for j in range(3)) for i in range(3)])
    Nm = np.stack([-1j * sum(Kv[j] * T64[3 * j + i] for j in range(3)) for i in range(3)])
    inv = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2))

    def project(X):
        d = sum(Kv[i] * X[i] for i in range(3)) * inv
        return np.stack([np.where(k2 == 0, 0.0, X[i] - Kv[i] * d) for i in range(3)])
    vp, vm = 0.5 * (nu + eta), 0.5 * (nu - eta)
    wp = project(Np) - k2 * (vp * Zp64 + vm * Zm64)
    wm = project(Nm) - k2 * (vp * Zm64 + vm * Zp64)
    hp, hm = gp.get(), gm.get()
    ep, em = orc.rel_l2(hp, wp), orc.rel_l2(hm, wm)
    print("elsasser_rhs %s pitch=%s rel-L2 %.3e %.3e" % (prec, F.complex_pitch, ep, em))
    assert ep < 4 * TOL[prec] and em < 4 * TOL[prec]
    assert np.all(hp[:, 0, 0, 0] == 0) and np.all(hm[:, 0, 0, 0] == 0)
    assert np.array_equal(dT.get(), T) and np.array_equal(dZp.get(), Zp) and np.array_equal(dZm.get(), Zm)


# ---- the example ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", DEALIAS)
def test_mhd_fused_equals_composed(dealias):
    """The Orszag-Tang-like vortex in a mean field at 16^3 over 5 steps: one outer_transform per stage and the 6 + 9 transforms
    issued by the example agree to 1e-12 relative L2 on both Elsasser fields; the initial state is not modified; and the state
    did change."""
    import mhd_device as demo
    from mpifft4py_amd import SelfComm
    N = np.array([16, 16, 16])
    F = demo.make_plan(SelfComm(0), N)
    Zp0, Zm0 = demo.orszag_tang_hat(F, B0=0.5)
    p0, m0 = Zp0.get(), Zm0.get()
    rep = {}
    r1 = demo.solve(SelfComm(0), N, Zp0, Zm0, 0.01, 0.02, 0.005, 5, dealias, fused=True, FFT=F, report=rep)
    p1, m1 = r1[0].get(), r1[1].get()
    r2 = demo.solve(SelfComm(0), N, Zp0, Zm0, 0.01, 0.02, 0.005, 5, dealias, fused=False, FFT=F)
    p2, m2 = r2[0].get(), r2[1].get()
    assert rep["fused"] == 1
    assert np.array_equal(Zp0.get(), p0) and np.array_equal(Zm0.get(), m0)
    ep, em = orc.rel_l2(p1, p2), orc.rel_l2(m1, m2)
    print("mhd, %s: fused against composed rel-L2 z+ %.3e z- %.3e" % (dealias, ep, em))
    assert ep < 1e-12 and em < 1e-12
    assert orc.rel_l2(p1, p0) > 1e-4 and orc.rel_l2(m1, m0) > 1e-4            # ... and something did happen


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("dealias", DEALIAS)
def test_mhd_alfven_wave(dealias, swapped):
    """Known answer at 16^3.  One Elsasser field is the uniform field -B0 e_z (the k = 0 bin only), the other -- the wave -- a
    solenoidal field band-limited to |k| <= 2; nu = eta = 0, dt = 0.01, 10 steps, B0 = 1.  With z- = -B0 e_z the equation of z+ is
    d z+ / dt = -(z- . grad) z+ = +B0 d z+ / dz: every mode of the wave must equal its initial value times exp(+i k_z B0 t) -- the
    convention fixed here: kz the scaled wavenumber of the bin, t = steps * dt -- and the uniform field must stay uniform.  Swapped
    (z+ = -B0 e_z uniform, z- the wave) the same factor holds for z-, through N- instead of N+.  Bound: the RK4 local error of a
    pure rotation exp(i w dt), (w dt)^5 / 120 per step with w = 2 B0 the fastest mode, times two, plus 4 TOL.  A transposed index
    in N+ or N- contracts the wave with its own solenoidal index, the term vanishes, the wave stands still and this fails."""
    import mhd_device as demo
    from mpifft4py_amd import SelfComm
    N = np.array([16, 16, 16])
    B0, dt, steps = 1.0, 0.01, 10
    F = demo.make_plan(SelfComm(0), N)
    cs = tuple(int(x) for x in F.complex_shape())
    k = [np.fft.fftfreq(16, 1.0 / 16), np.fft.fftfreq(16, 1.0 / 16), np.arange(9, dtype=float)]
    KX, KY, KZ = np.meshgrid(*k, indexing="ij")
    k2 = KX ** 2 + KY ** 2 + KZ ** 2
    rng = np.random.default_rng(12)
    w = (rng.random((3,) + cs) - 0.5 + 1j * (rng.random((3,) + cs) - 0.5)) * ((k2 <= 4) & (k2 > 0))
    w = w - np.stack([KX, KY, KZ]) * ((KX * w[0] + KY * w[1] + KZ * w[2]) / np.where(k2 == 0, 1.0, k2))      # solenoidal
    w = np.stack([np.fft.rfftn(np.fft.irfftn(w[i], s=(16, 16, 16), axes=(0, 1, 2))) for i in range(3)])      # ... and the spectrum of a REAL field
    w[np.abs(w) < 1e-13 * np.abs(w).max()] = 0
    assert np.abs(KX * w[0] + KY * w[1] + KZ * w[2]).max() < 1e-10 * np.abs(w).max() and np.abs(w[:, k2 > 4]).max() == 0
    uni = np.zeros((3,) + cs, dtype=np.complex128)
    uni[2, 0, 0, 0] = -B0 * 16 ** 3
    Zp0, Zm0 = (uni, w) if swapped else (w, uni)
    dp, dm = F.empty_complex(3).set(Zp0), F.empty_complex(3).set(Zm0)
    rp, rm = demo.solve(SelfComm(0), N, dp, dm, 0.0, 0.0, dt, steps, dealias, fused=True, FFT=F)
    gp, gm = rp.get(), rm.get()
    wave, still = (gm, gp) if swapped else (gp, gm)
    want = w * np.exp(1j * KZ * B0 * steps * dt)
    bound = 2 * steps * (2 * B0 * dt) ** 5 / 120 + 4 * TOL["double"]
    e, moved = orc.rel_l2(wave, want), orc.rel_l2(wave, w)
    es = orc.rel_l2(still, uni)
    print("alfven wave, %s%s: rel-L2 against the rotated modes %.3e (bound %.3e), against the initial ones %.3e; uniform field %.3e"
          % (dealias, " swapped" if swapped else "", e, bound, moved, es))
    assert e < bound
    assert moved > 1e-2                          # the wave did travel
    assert es < 4 * TOL["double"]                # the uniform field stayed uniform
