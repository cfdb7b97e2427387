"""GPU: shell-binned sums of device-resident spectra (spectral.shell_sums, mfft_ew_shell_sums; csrc/shells.hip) against
plain numpy written here.

Reference A (summation only): the spectra the kernel reads, downloaded, with Hermitian weights and the integer shell
rule formed here from integers, summed per shell in np.longdouble.  With A_s = sum h w sum_c |a_c| |b_c| and cnt_s the
number of contributing elements, |got_s - ref_s| <= (cnt_s + 8) 2^-52 A_s for EVERY shell: a sum of n doubles in any
order errs by at most (n - 1) 2^-53 sum |x|; the + 8 and the factor 2 cover forming each product.  It holds for fp32
fields too, products and sums being in double.

Reference B (end to end): the device transform of real fields, binned on the device, against the FULL np.fft.fftn
spectrum of the same fields binned with weight 1: |got_s - full_s| <= 4 TOL[prec] A_s.

Odd N2 -- (12, 10, 9) and (7, 9, 15) -- runs through the complex slab plan (weight 1 on every mode): the real-to-complex
plans of this library take even N2 only."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import L, TOL, cdtype, have_gpu, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


# ---- the reference: integers and numpy only -------------------------------------------------------------------------
def exact_shell(m):
    m = int(m)
    if m == 0:
        return 0
    s = math.isqrt(m)
    if 4 * m >= (2 * s + 1) ** 2:
        s += 1
    assert (2 * s - 1) ** 2 <= 4 * m < (2 * s + 1) ** 2
    return s


def shells_of(m):
    """exact_shell of an integer array (through a table over its values)."""
    tab = np.array([exact_shell(v) for v in range(int(m.max()) + 1)], dtype=np.int64) if m.max() < 200000 else None
    return tab[m] if tab is not None else np.vectorize(exact_shell, otypes=[np.int64])(m)


def full_modes(n):
    k = np.arange(n, dtype=np.int64)
    k[(n + 1) // 2:] -= n
    return k


def nshell_of(N):
    return exact_shell(sum((int(n) // 2) ** 2 for n in N)) + 1


def block_tables(N, window, half):
    """(shell, h) of the block `window` = [(start, length)] * 3 of the spectrum of an N mesh."""
    ks = [full_modes(N[0]), full_modes(N[1]), np.arange(N[2] // 2 + 1, dtype=np.int64) if half else full_modes(N[2])]
    k = [ks[i][s:s + l] for i, (s, l) in enumerate(window)]
    m = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    if half:
        h = np.where((k[2] == 0) | ((N[2] % 2 == 0) & (k[2] == N[2] // 2)), 1.0, 2.0)
    else:
        h = np.ones(len(k[2]))
    return shells_of(m), np.broadcast_to(h[None, None, :], m.shape)


def ref_a(a, b, sh, h, kvec, nshell, acc=None):
    """Reference A over one block: (S in longdouble, A_s, cnt_s), added to `acc` when given.  a, b: (ncomp, s0, s1, s2)."""
    ld = np.longdouble
    w = np.asarray(h, dtype=ld)
    if kvec is not None:
        kx, ky, kz = (np.asarray(v, dtype=ld) for v in kvec)
        w = w * (kx[:, None, None] ** 2 + ky[None, :, None] ** 2 + kz[None, None, :] ** 2)
    t = np.zeros(sh.shape, dtype=ld)
    absum = np.zeros(sh.shape, dtype=np.float64)
    for c in range(a.shape[0]):
        t += a[c].real.astype(ld) * b[c].real.astype(ld) + a[c].imag.astype(ld) * b[c].imag.astype(ld)
        absum += np.abs(a[c].astype(np.complex128)) * np.abs(b[c].astype(np.complex128))
    S, A, cnt = acc if acc is not None else (np.zeros(nshell, dtype=ld), np.zeros(nshell), np.zeros(nshell))
    np.add.at(S, sh.ravel(), (w * t).ravel())
    A += np.bincount(sh.ravel(), weights=(w.astype(np.float64) * absum).ravel(), minlength=nshell)
    cnt += np.bincount(sh.ravel(), minlength=nshell)
    return S, A, cnt


def check_a(got, ref, tag):
    S, A, cnt = ref
    err = np.abs(got.astype(np.longdouble) - S).astype(np.float64)
    bound = (cnt + 8) * EPS * A
    worst = np.max(err / np.maximum(bound, 1e-300))
    print("%s: reference A  max err / bound = %.3e (max err %.3e, A_s up to %.3e)" % (tag, worst, err.max(), A.max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= bound), (tag, np.nonzero(err > bound)[0][:8], err.max())


def real_fields(N, seed):
    rng = np.random.default_rng(seed)
    return rng.random((3,) + tuple(N)) - 0.5, rng.random((3,) + tuple(N)) - 0.5


def scaled_vectors(F):
    K = F.get_local_wavenumbermesh(scaled=True)
    return [np.asarray(K[i], dtype=F.float).reshape(-1) for i in range(3)]


def spectra_on_device(F, fields, prec, half):
    """The device transforms of three real fields as one (3,) + complex_shape DeviceArray, and their copy on the host."""
    from mpifft4py_amd import DeviceArray
    d = F.empty_complex(3)
    for c in range(3):
        src = fields[c].astype(rdtype(prec)) if half else fields[c].astype(cdtype(prec))
        F.fftn(DeviceArray.from_numpy(src), d.component(c))
    F.sync()
    return d, d.get()


# ---- one rank -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N", [(32, 64, 128), (16, 12, 20), (12, 10, 9), (7, 9, 15), (36, 72, 144)])
def test_shell_sums_one_rank(N, prec):
    """Every mesh and precision: ncomp 1 and 3, b is a and b != a (signed sums), k2 off and on, against both references."""
    from mpifft4py_amd import SelfComm, Slab_C2C, Slab_R2C, spectral
    half = N[2] % 2 == 0
    F = (Slab_R2C if half else Slab_C2C)(np.array(N), L, SelfComm(0), prec)
    K = spectral.Wavenumbers(F)
    nshell = nshell_of(N)
    assert K.nshell == nshell
    u, w = real_fields(N, 7 + sum(N))
    u, w = u.astype(rdtype(prec)).astype(np.float64), w.astype(rdtype(prec)).astype(np.float64)      # what the device is given
    du, hu = spectra_on_device(F, u, prec, half)
    dw, hw = spectra_on_device(F, w, prec, half)
    window = [(0, s) for s in hu.shape[1:]]
    sh, h = block_tables(N, window, half)
    kvec = scaled_vectors(F)
    shf, hf = block_tables(N, [(0, n) for n in N], False)
    kf = [full_modes(n).astype(np.float64) for n in N]
    wfull = kf[0][:, None, None] ** 2 + kf[1][None, :, None] ** 2 + kf[2][None, None, :] ** 2       # L = 2 pi: scale 1
    fu, fw = np.stack([np.fft.fftn(x) for x in u]), np.stack([np.fft.fftn(x) for x in w])
    for ncomp in (1, 3):
        for same in (True, False):
            for k2 in (False, True):
                tag = "%s %s ncomp=%d %s k2=%d" % (list(N), prec, ncomp, "b is a" if same else "b != a", k2)
                if ncomp == 3:
                    a, b, ha, hb, fa, fb = du, (du if same else dw), hu, (hu if same else hw), fu, (fu if same else fw)
                else:
                    a, b = du.component(1), (du.component(1) if same else dw.component(2))
                    ha, hb, fa, fb = hu[1:2], (hu[1:2] if same else hw[2:3]), fu[1:2], (fu[1:2] if same else fw[2:3])
                got = spectral.shell_sums(F, K, a, None if same else b, k2=k2)
                assert got.shape == (nshell,) and got.dtype == np.float64
                ref = ref_a(ha, hb, sh, h, kvec if k2 else None, nshell)
                check_a(got, ref, tag)
                if not same:
                    assert (got < 0).any() and (got > 0).any()                           # signed sums
                t = np.sum(fa.real * fb.real + fa.imag * fb.imag, 0) * (wfull if k2 else 1.0)
                full = np.bincount(shf.ravel(), weights=t.ravel(), minlength=nshell)
                d = np.abs(got - full)
                print("%s: reference B  max |got - full| / A_s = %.3e (bound %.1e)" % (tag, np.max(d / np.maximum(ref[1], 1e-300)), 4 * TOL[prec]))
                assert np.all(d <= 4 * TOL[prec] * ref[1]), (tag, d.max())
    # b passed explicitly as the same array is the same call: the same sums, to reference A's bound (not bit for bit: the
    # order in which a workgroup's waves add to its histogram differs from run to run)
    check_a(spectral.shell_sums(F, K, du, du), ref_a(hu, hu, sh, h, None, nshell), "%s %s b given as a" % (list(N), prec))


@pytest.mark.parametrize("prec", ["double", "single"])
def test_shell_sums_pitched_plan(prec):
    """Rows a whole number of cache lines apart, NaN between them: the elements between the rows are skipped, the sums
    are the compact plan's within reference A's bound."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    N = (32, 64, 128)
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    Fp = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert Fp.complex_pitch and Fp.complex_pitch > Fp.complex_shape()[2]
    u, w = real_fields(N, 5)
    du, hu = spectra_on_device(F, u, prec, True)
    dw, hw = spectra_on_device(F, w, prec, True)
    K, Kp = spectral.Wavenumbers(F), spectral.Wavenumbers(Fp)
    pu, pw = Fp.empty_complex(3), Fp.empty_complex(3)
    for p, hst in ((pu, hu), (pw, hw)):
        _lib.call("mfft_memset", p.ptr, 0xFF, p.nbytes)             # every byte 0xFF: NaN in both precisions
        p.set(hst)
    sh, h = block_tables(N, [(0, s) for s in hu.shape[1:]], True)
    nshell = nshell_of(N)
    for k2 in (False, True):
        for b, hb in ((None, hu), (pw, hw)):
            got_p = spectral.shell_sums(Fp, Kp, pu, b, k2=k2)
            got_c = spectral.shell_sums(F, K, du, None if b is None else dw, k2=k2)
            ref = ref_a(hu, hb, sh, h, scaled_vectors(F) if k2 else None, nshell)
            check_a(got_p, ref, "pitched %s k2=%d" % (prec, k2))
            check_a(got_c, ref, "compact %s k2=%d" % (prec, k2))
            assert np.all(np.abs(got_p - got_c) <= (ref[2] + 8) * EPS * ref[1])


# ---- several ranks ------------------------------------------------------------------------------------------------------
def _ranks_case(kind, P, N, prec):
    from mpifft4py_amd import DeviceArray, Pencil_R2C, Slab_R2C, spectral
    u, w = real_fields(N, 3 + P)

    def work(comm):
        if kind == "slab":
            F = Slab_R2C(np.array(N), L, comm, prec)
        else:
            F = Pencil_R2C(np.array(N), L, comm, prec, P1=2, alignment=kind[-1])
        K = spectral.Wavenumbers(F)
        sl = F.real_local_slice()
        du, dw = F.empty_complex(3), F.empty_complex(3)
        for c in range(3):
            F.fftn(DeviceArray.from_numpy(u[c][sl].astype(rdtype(prec))), du.component(c))
            F.fftn(DeviceArray.from_numpy(w[c][sl].astype(rdtype(prec))), dw.component(c))
        F.sync()
        out = {"uu": spectral.shell_sums(F, K, du), "uw_k2": spectral.shell_sums(F, K, du, dw, k2=True),
               "local": spectral.shell_sums(F, K, du, reduce=False)}
        return out, du.get(), dw.get(), list(F._mesh.spectral_window), scaled_vectors(F)

    res = run_ranks(P, work)
    nshell = nshell_of(N)
    acc_uu = acc_uw = None
    for out, hu, hw, window, kvec in res:
        sh, h = block_tables(N, window, True)
        acc_uu = ref_a(hu, hu, sh, h, None, nshell, acc_uu)
        acc_uw = ref_a(hu, hw, sh, h, kvec, nshell, acc_uw)
        check_a(out["local"], ref_a(hu, hu, sh, h, None, nshell), "%s P=%d %s one rank's partial sums" % (kind, P, prec))
    for out, _, _, _, _ in res:
        assert np.array_equal(out["uu"], res[0][0]["uu"]) and np.array_equal(out["uw_k2"], res[0][0]["uw_k2"])
    check_a(res[0][0]["uu"], acc_uu, "%s P=%d %s %s uu" % (kind, P, list(N), prec))
    check_a(res[0][0]["uw_k2"], acc_uw, "%s P=%d %s %s uw k2" % (kind, P, list(N), prec))
    assert acc_uu[2].sum() == N[0] * N[1] * (N[2] // 2 + 1)                                   # every mode of the spectrum, once


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N", [(16, 12, 20), (32, 64, 128)])
@pytest.mark.parametrize("kind,P", [("slab", 2), ("slab", 4), ("pencilX", 4), ("pencilY", 4)])
def test_shell_sums_ranks(kind, P, N, prec):
    """Slab on 2 and 4 ranks, pencils on 2 x 2 in both alignments: the reduced vector is the same on every rank and meets
    reference A with cnt_s and A_s taken over all ranks."""
    _ranks_case(kind, P, N, prec)


# ---- identities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_parseval_against_sumsq(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = (32, 64, 128)
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    K = spectral.Wavenumbers(F)
    u, _ = real_fields(N, 1)
    U = DeviceArray.from_numpy(u.astype(rdtype(prec)))
    U_hat = F.empty_complex(3)
    for c in range(3):
        F.fftn(U.component(c), U_hat.component(c))
    got = spectral.shell_sums(F, K, U_hat, U_hat).sum()
    want = float(np.prod(N)) * spectral.sumsq(F, U)
    print("Parseval %s: %.15e against %.15e, relative difference %.3e" % (prec, got, want, abs(got - want) / want))
    assert abs(got - want) <= 4 * TOL[prec] * want


def _taylor_green(F):
    """The initial field of examples/spectral_dns_device.py on one rank."""
    from mpifft4py_amd import DeviceArray
    N = [int(n) for n in F.N]
    x, y, z = (np.arange(n, dtype=float) * (2 * np.pi / n) for n in N)
    U = np.zeros((3,) + tuple(N), dtype=F.float)
    U[0] = np.sin(x)[:, None, None] * np.cos(y)[None, :, None] * np.cos(z)[None, None, :]
    U[1] = -np.cos(x)[:, None, None] * np.sin(y)[None, :, None] * np.cos(z)[None, None, :]
    Ud = DeviceArray.from_numpy(U)
    U_hat = F.empty_complex(3)
    for c in range(3):
        F.fftn(Ud.component(c), U_hat.component(c))
    return U_hat


def test_taylor_green_known_spectrum():
    """All the energy of the Taylor-Green field sits in the eight modes |k|^2 = 3: shell 2, E = 1/8."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([64, 64, 64]), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    E = spectral.energy_spectrum(F, K, _taylor_green(F))
    assert E.shape == (nshell_of((64, 64, 64)),) == (56,)
    print("Taylor-Green E[2] - 0.125 = %.3e, largest other shell %.3e" % (E[2] - 0.125, np.delete(E, 2).max()))
    assert abs(E[2] - 0.125) <= 1e-12
    assert np.all(np.abs(np.delete(E, 2)) <= 1e-24)


def test_transfer_sums_to_zero():
    """A few RK4 steps of the example's loop, then T(k) of the projected nonlinear term: the projected advection term
    conserves energy, so the transfer spectrum sums to zero, to 4 TOL sum_s A_s."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N, nu, dt, dealias = (32, 32, 32), 0.000625, 0.01, "3/2-rule"
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    U_hat = _taylor_green(F)
    U0, U1, dU = (F.empty_complex(3) for _ in range(3))
    a, b = [1. / 6., 1. / 3., 1. / 3., 1. / 6.], [0.5, 0.5, 1.]
    spectral.axpbz(F, U0, U_hat, U_hat, 1.0, 0.0)
    spectral.axpbz(F, U1, U_hat, U_hat, 1.0, 0.0)
    spectral.curl_hat(F, K, U_hat, dU)
    for _ in range(4):
        for rk in range(4):
            spectral.cross_transform(F, U_hat, dU, dU, dealias)
            spectral.ns_rk_stage(F, K, dU, U_hat, U0, U1, nu, a[rk] * dt, b[rk] * dt if rk < 3 else 0.0, rk == 3)
    spectral.cross_transform(F, U_hat, dU, dU, dealias)            # dU held curl(U_hat): now fftn(U x curl U)
    spectral.ns_rhs(F, K, dU, U_hat, 0.0)                          # nu = 0: the pressure projection alone
    T = spectral.transfer_spectrum(F, K, U_hat, dU)
    hu, hn = U_hat.get(), dU.get()
    sh, h = block_tables(N, [(0, s) for s in hu.shape[1:]], True)
    ref = ref_a(hu, hn, sh, h, None, nshell_of(N))
    check_a(T * float(np.prod(N)) ** 2, ref, "transfer spectrum")
    scale = ref[1].sum() / float(np.prod(N)) ** 2
    print("sum of T(k) = %.3e, sum of |T| terms %.3e, largest |T(k)| %.3e" % (T.sum(), scale, np.abs(T).max()))
    assert np.abs(T).max() > 1e-9                                   # energy does move between the shells
    assert abs(T.sum()) <= 4 * TOL["double"] * scale


# ---- error paths: every one an error return, none a device fault ------------------------------------------------------
def test_error_returns():
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    N = (16, 12, 20)
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    U_hat = F.empty_complex(3)
    _lib.call("mfft_memset", U_hat.ptr, 0, U_hat.nbytes)
    fn = _lib.load().mfft_ew_shell_sums
    out = np.zeros(9000)
    res = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(ncomp=3, nshell=K.nshell, a=U_hat.ptr):
        return fn(F._plan, a, U_hat.ptr, ncomp, K.idev[0].ptr, K.idev[1].ptr, K.idev[2].ptr, K.hdev.ptr, K.dev[0].ptr,
                  K.dev[1].ptr, K.dev[2].ptr, 0, K.cshape, nshell, 1, res)

    assert call() == 0
    assert call(nshell=K.nshell - 1) == -1 and b"shell" in _lib.load().mfft_last_error()      # a mode beyond the last shell: flagged on the device
    assert call(nshell=2) == -1
    assert call(nshell=0) == -1
    assert call(ncomp=2) == -1                                                                   # MFFT_ERR_INVALID
    assert call(a=None) == -1
    assert call(nshell=8193) == -2 and b"8192" in _lib.load().mfft_last_error()                 # MFFT_ERR_UNSUPPORTED: 64 KiB of LDS
    assert call(nshell=8192) == 0                                                                # the limit itself runs
    assert call() == 0 and np.all(out[:K.nshell] == 0.0)                                         # and the plan still works
    K.nshell -= 1
    with pytest.raises(_lib.MfftError):
        spectral.shell_sums(F, K, U_hat)


def test_line_plans_are_not_supported():
    from mpifft4py_amd import Line_R2C, SelfComm, spectral
    F = Line_R2C(np.array([32, 64]), np.array([2 * np.pi] * 2), SelfComm(0), "double")
    with pytest.raises(NotImplementedError):                  # (the 2-D class has no Wavenumbers either)
        spectral.shell_sums(F, None, F.empty_complex())


# ---- the examples ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,args,said", [
    ("spectral_dns_device.py", ["--M", "5", "--spectrum"], "sum of E(k) equals k to 1e-12"),
    ("spectral_dns_device.py", ["--M", "5", "--spectrum", "--ranks", "2"], "sum of E(k) equals k to 1e-12"),
    ("passive_scalar_device.py", ["--N", "32", "--spectrum"], "sum of the spectrum equals half the mean square to 1e-12")])
def test_examples_print_their_spectra(script, args, said):
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", script)] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT)
    out = p.stdout.decode()
    assert p.returncode == 0 and said in out, out[-3000:]
    if script == "spectral_dns_device.py":
        assert "matches the reference demo's known answer" in out
