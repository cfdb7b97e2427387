"""GPU: (k_perp, k_z) sums of device-resident spectra (spectral.cyl_sums, mfft_ew_cyl_sums; csrc/cylspec.hip) against plain
numpy written here: the spectra the kernel reads, downloaded; the perp shell of a row from the exact integer rule and the z bin
|kz| from integers; the sums per bin in np.longdouble.

The tolerance is the shell test's, per bin: with A = sum h w sum_c |a_c| |b_c| over the bin and cnt its contributing elements,
|got - ref| <= (cnt + 8) 2^-52 A.  A sum of n doubles in any order errs by at most (n - 1) 2^-53 sum |x|; the + 8 and the factor
2 cover forming each product.  It holds for fp32 fields too, products and sums being in double.  Sums of bins (the marginals,
the total) add the bins' bounds and, for the m numbers numpy adds in double, m 2^-52 times the sum of their A."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import L, cdtype, have_gpu, rdtype, run_ranks
from test_gpu_shell_spectrum import (EPS, _taylor_green, block_tables, full_modes, nshell_of, real_fields, ref_a, scaled_vectors,
                                     shells_of, spectra_on_device)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
I32 = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def default_seg():
    txt = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    return int(re.search(r"#define MFFT_CYL_SEG_ROWS (\d+)", txt).group(1))


# ---- the reference: integers and numpy only -------------------------------------------------------------------------
def bins_of(N):
    return int(shells_of(np.array([(N[0] // 2) ** 2 + (N[1] // 2) ** 2]))[0]) + 1, N[2] // 2 + 1


def cyl_tables(N, window, half):
    """(perp shell (s0, s1), |kz| (s2,), h (s2,)) of the block `window` = [(start, length)] * 3 of the spectrum of an N mesh."""
    ks = [full_modes(N[0]), full_modes(N[1]), np.arange(N[2] // 2 + 1, dtype=np.int64) if half else full_modes(N[2])]
    k = [ks[i][s:s + l] for i, (s, l) in enumerate(window)]
    psh = shells_of(k[0][:, None] ** 2 + k[1][None, :] ** 2)
    h = np.where((k[2] == 0) | ((N[2] % 2 == 0) & (k[2] == N[2] // 2)), 1.0, 2.0) if half else np.ones(len(k[2]))
    return psh, np.abs(k[2]), h


def ref_cyl(a, b, tables, kvec, N, acc=None):
    """(R in longdouble, A, cnt), each (nperp, npar), over one block; added to `acc` when given.  a, b: (ncomp, s0, s1, s2)."""
    ld = np.longdouble
    psh, q, h = tables
    nperp, npar = bins_of(N)
    w = np.broadcast_to(np.asarray(h, dtype=ld)[None, None, :], a.shape[1:])
    if kvec is not None:
        kx, ky, kz = (np.asarray(v, dtype=ld) for v in kvec)
        w = w * (kx[:, None, None] ** 2 + ky[None, :, None] ** 2 + kz[None, None, :] ** 2)
    t = np.zeros(a.shape[1:], dtype=ld)
    absum = np.zeros(a.shape[1:], dtype=np.float64)
    for c in range(a.shape[0]):
        t += a[c].real.astype(ld) * b[c].real.astype(ld) + a[c].imag.astype(ld) * b[c].imag.astype(ld)
        absum += np.abs(a[c].astype(np.complex128)) * np.abs(b[c].astype(np.complex128))
    cell = (psh[:, :, None] * npar + q[None, None, :]).ravel()
    assert cell.max() < nperp * npar
    R, A, cnt = acc if acc is not None else (np.zeros(nperp * npar, dtype=ld), np.zeros(nperp * npar), np.zeros(nperp * npar))
    np.add.at(R, cell, (w * t).ravel())
    A += np.bincount(cell, weights=(w.astype(np.float64) * absum).ravel(), minlength=nperp * npar)
    cnt += np.bincount(cell, minlength=nperp * npar)
    return R, A, cnt


def check(got, ref, N, tag):
    R, A, cnt = (x.reshape(bins_of(N)) for x in ref)
    assert got.shape == bins_of(N) and got.dtype == np.float64, (got.shape, bins_of(N))
    err = np.abs(got.astype(np.longdouble) - R).astype(np.float64)
    bound = (cnt + 8) * EPS * A
    print("%s: max err / bound = %.3e (max err %.3e, A up to %.3e)" % (tag, np.max(err / np.maximum(bound, 1e-300)), err.max(), A.max()))
    assert np.all(np.isfinite(got)), tag
    assert np.all(err <= bound), (tag, np.argwhere(err > bound)[:8], err.max())
    assert np.all(got[cnt == 0] == 0.0), tag                      # a bin without a mode is 0.0, not a leftover
    # the marginals against the reference's, the bins' bounds added plus the sum numpy takes in double
    for axis in (0, 1):
        m = got.shape[axis]
        e = np.abs(got.sum(axis=axis).astype(np.longdouble) - R.sum(axis=axis)).astype(np.float64)
        assert np.all(e <= bound.sum(axis=axis) + m * EPS * A.sum(axis=axis)), (tag, axis, e.max())


def variants(du, dw, hu, hw):
    """(tag, a, b or None, host a, host b) for ncomp 1 and 3, b is a and b != a."""
    for ncomp in (1, 3):
        for same in (True, False):
            if ncomp == 3:
                yield "ncomp=3 %s" % ("b is a" if same else "b != a"), du, (None if same else dw), hu, (hu if same else hw)
            else:
                yield ("ncomp=1 %s" % ("b is a" if same else "b != a"), du.component(1), (None if same else dw.component(2)), hu[1:2],
                       (hu[1:2] if same else hw[2:3]))


def one_rank(N, prec, pitch=None):
    from mpifft4py_amd import SelfComm, Slab_C2C, Slab_R2C, spectral
    half = N[2] % 2 == 0
    kw = dict(complex_pitch=pitch) if pitch else {}
    F = (Slab_R2C if half else Slab_C2C)(np.array(N), L, SelfComm(0), prec, **kw)
    return F, spectral.Wavenumbers(F), half


_FIELDS = {}


def fields_of(N, prec):
    """The plan, its wavenumbers, the two device spectra and their host copies of a mesh: made once, shared, never changed."""
    key = (tuple(N), prec)
    if key not in _FIELDS:
        F, K, half = one_rank(N, prec)
        u, w = real_fields(N, 11 + sum(N))
        du, hu = spectra_on_device(F, u, prec, half)
        dw, hw = spectra_on_device(F, w, prec, half)
        tables = cyl_tables(N, [(0, s) for s in hu.shape[1:]], half)
        _FIELDS[key] = (F, K, du, dw, hu, hw, tables)
    return _FIELDS[key]


# ---- one rank -----------------------------------------------------------------------------------------------------------
# (12, 10, 16): rows of 9, one partial wave, odd: fp32 loads 8 bytes.  (12, 10, 18): rows of 10, fp32 loads 16 bytes.  (8, 6, 130): rows of
# 66, a run of 2 behind a whole wave.  (12, 10, 9), (7, 9, 15): the complex slab plan, full z axis, kz and -kz in one bin, odd sizes.
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N", [(12, 10, 16), (12, 10, 18), (8, 6, 130), (12, 10, 9), (7, 9, 15)])
def test_cyl_sums_one_rank(N, prec):
    from mpifft4py_amd import spectral
    F, K, du, dw, hu, hw, tables = fields_of(N, prec)
    assert (K.nperp, K.npar) == bins_of(N)
    kvec = scaled_vectors(F)
    for tag, a, b, ha, hb in variants(du, dw, hu, hw):
        for k2 in (False, True):
            got = spectral.cyl_sums(F, K, a, b, k2=k2)
            check(got, ref_cyl(ha, hb, tables, kvec if k2 else None, N), N, "%s %s %s k2=%d" % (list(N), prec, tag, k2))
            if b is not None and not k2:
                assert (got < 0).any() and (got > 0).any()                           # signed sums
    # b given as the same array is the same call, bit for bit
    assert np.array_equal(spectral.cyl_sums(F, K, du, du), spectral.cyl_sums(F, K, du))


@pytest.mark.parametrize("prec", ["double", "single"])
def test_segment_lengths_and_reproducibility(prec):
    """Segments of 1, 3 and the default number of rows: each within the bound, each bit for bit itself across two calls."""
    from mpifft4py_amd import spectral
    N = (12, 10, 16)
    F, K, du, dw, hu, hw, tables = fields_of(N, prec)
    ref = ref_cyl(hu, hw, tables, scaled_vectors(F), N)
    for seg in (1, 3, 0):
        got = spectral.cyl_sums(F, K, du, dw, k2=True, seg_rows=seg)
        check(got, ref, N, "%s seg_rows=%d" % (prec, seg))
        assert np.array_equal(got, spectral.cyl_sums(F, K, du, dw, k2=True, seg_rows=seg)), seg


@pytest.mark.parametrize("prec", ["double", "single"])
def test_shell_of_several_segments(prec):
    """(160, 160, 8): the largest perp shell holds 500 rows, more than MFFT_CYL_SEG_ROWS, so the fold adds several segments."""
    from mpifft4py_amd import spectral
    N = (160, 160, 8)
    F, K, du, dw, hu, hw, tables = fields_of(N, prec)
    assert np.diff(K.perp_start).max() == 500 > default_seg()
    check(spectral.cyl_sums(F, K, du), ref_cyl(hu, hu, tables, None, N), N, "%s %s uu" % (list(N), prec))
    check(spectral.cyl_sums(F, K, du, dw, k2=True), ref_cyl(hu, hw, tables, scaled_vectors(F), N), N, "%s %s uw k2" % (list(N), prec))


@pytest.mark.parametrize("prec", ["double", "single"])
def test_cyl_sums_pitched_plan(prec):
    """Rows a whole number of cache lines apart, NaN between them: the elements between the rows are skipped."""
    from mpifft4py_amd import _lib, spectral
    N = (32, 64, 128)
    F, K, du, dw, hu, hw, tables = fields_of(N, prec)
    Fp, Kp, _ = one_rank(N, prec, pitch="auto")
    assert Fp.complex_pitch and Fp.complex_pitch > Fp.complex_shape()[2]
    pu, pw = Fp.empty_complex(3), Fp.empty_complex(3)
    for p, hst in ((pu, hu), (pw, hw)):
        _lib.call("mfft_memset", p.ptr, 0xFF, p.nbytes)             # every byte 0xFF: NaN in both precisions
        p.set(hst)
    for k2 in (False, True):
        for b, hb in ((None, hu), (pw, hw)):
            ref = ref_cyl(hu, hb, tables, scaled_vectors(F) if k2 else None, N)
            check(spectral.cyl_sums(Fp, Kp, pu, b, k2=k2), ref, N, "pitched %s k2=%d" % (prec, k2))
            check(spectral.cyl_sums(F, K, du, None if b is None else dw, k2=k2), ref, N, "compact %s k2=%d" % (prec, k2))


# ---- several ranks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("kind,P", [("slab", 2), ("slab", 4), ("pencilX", 4), ("pencilY", 4)])
def test_cyl_sums_ranks(kind, P, prec):
    """The reduced array is the same on every rank and meets the ONE-RANK reference of the assembled global spectrum; a rank's own
    sums meet the reference of its block, and its shells without a row are zeros."""
    from mpifft4py_amd import DeviceArray, Pencil_R2C, Slab_R2C, spectral
    N = (16, 12, 20)
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
        out = {"uu": spectral.cyl_sums(F, K, du), "uw_k2": spectral.cyl_sums(F, K, du, dw, k2=True),
               "local": spectral.cyl_sums(F, K, du, reduce=False)}
        return out, du.get(), dw.get(), list(F._mesh.spectral_window), scaled_vectors(F), np.array(K.perp_start)

    res = run_ranks(P, work)
    gshape = (3, N[0], N[1], N[2] // 2 + 1)
    gu, gw = np.zeros(gshape, dtype=cdtype(prec)), np.zeros(gshape, dtype=cdtype(prec))
    gk = [np.zeros(n, dtype=rdtype(prec)) for n in gshape[1:]]
    empties = 0
    for out, hu, hw, window, kvec, start in res:
        sl = tuple(slice(s, s + l) for s, l in window)
        gu[(slice(None),) + sl], gw[(slice(None),) + sl] = hu, hw
        for i in range(3):
            gk[i][sl[i]] = kvec[i]
        check(out["local"], ref_cyl(hu, hu, cyl_tables(N, window, True), None, N), N, "%s P=%d %s one rank's own sums" % (kind, P, prec))
        empty = np.diff(start) == 0
        empties += int(empty.sum())
        assert np.all(out["local"][empty] == 0.0)
        assert np.array_equal(out["uu"], res[0][0]["uu"]) and np.array_equal(out["uw_k2"], res[0][0]["uw_k2"])
    assert empties > 0, "no rank has a shell without rows: the case is not exercised"
    tables = cyl_tables(N, [(0, n) for n in gshape[1:]], True)
    check(res[0][0]["uu"], ref_cyl(gu, gu, tables, None, N), N, "%s P=%d %s uu" % (kind, P, prec))
    check(res[0][0]["uw_k2"], ref_cyl(gu, gw, tables, gk, N), N, "%s P=%d %s uw k2" % (kind, P, prec))


# ---- identities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N", [(12, 10, 16), (7, 9, 15)])
def test_sum_is_the_shell_sums_sum(N, prec):
    """R.sum() against shell_sums(...).sum(): each within the sum of its bins' bounds of the exact total, plus the two sums numpy
    takes in double over m numbers (m 2^-52 sum A each)."""
    from mpifft4py_amd import spectral
    F, K, du, dw, hu, hw, tables = fields_of(N, prec)
    half = N[2] % 2 == 0
    sh, h = block_tables(N, [(0, s) for s in hu.shape[1:]], half)
    for k2 in (False, True):
        kvec = scaled_vectors(F) if k2 else None
        R, S = spectral.cyl_sums(F, K, du, dw, k2=k2), spectral.shell_sums(F, K, du, dw, k2=k2)
        _, A2, c2 = ref_cyl(hu, hw, tables, kvec, N)
        _, A1, c1 = ref_a(hu, hw, sh, h, kvec, nshell_of(N))
        bound = ((c2 + 8) * EPS * A2).sum() + ((c1 + 8) * EPS * A1).sum() + (R.size + S.size) * EPS * A1.sum()
        print("%s %s k2=%d: R.sum() - S.sum() = %.3e, bound %.3e" % (list(N), prec, k2, R.sum() - S.sum(), bound))
        assert abs(R.sum() - S.sum()) <= bound


def test_taylor_green_known_spectrum_2d():
    """All the energy of the Taylor-Green field sits in the modes (+-1, +-1, +-1): perp shell(1 + 1) = 1, |kz| = 1, E = 1/8."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([64, 64, 64]), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    E = spectral.energy_spectrum_2d(F, K, _taylor_green(F))
    assert E.shape == (46, 33) == bins_of((64, 64, 64))
    rest = E.copy()
    rest[1, 1] = 0.0
    print("Taylor-Green E[1, 1] - 0.125 = %.3e, largest other bin %.3e" % (E[1, 1] - 0.125, np.abs(rest).max()))
    assert abs(E[1, 1] - 0.125) <= 1e-12
    assert np.all(np.abs(rest) <= 1e-24)
    T = spectral.transfer_spectrum_2d(F, K, _taylor_green(F), _taylor_green(F))          # <U*, U> / N^6 = 2 E
    assert abs(T[1, 1] - 0.25) <= 1e-12 and T.shape == E.shape


# ---- error paths: every one an error return, none a device fault ------------------------------------------------------
def test_error_returns():
    from mpifft4py_amd import _lib, spectral
    N = (16, 12, 20)
    F, K, half = one_rank(N, "double")
    U_hat = F.empty_complex(3)
    _lib.call("mfft_memset", U_hat.ptr, 0, U_hat.nbytes)
    fn = _lib.load().mfft_ew_cyl_sums
    poison = -12345.5
    out = np.full(K.nperp * K.npar, poison)
    good = np.array(K.perp_start)
    bad_order, bad_end, bad_first = good.copy(), good.copy(), good.copy()
    bad_order[3], bad_order[4] = good[4], good[3]
    assert bad_order[3] > bad_order[4]
    bad_end[-1] -= 1
    bad_first[0] = 1
    empty = (ctypes.c_int64 * 3)(16, 0, 11)

    def call(a=U_hat.ptr, ncomp=3, start=good, k2=0, kx=K.dev[0].ptr, shape=K.cshape, npar=K.npar, seg=0, prec=1, rows=K.perp_rows.ptr, res=out, nperp=K.nperp):
        return fn(F._plan, a, U_hat.ptr, ncomp, rows, None if start is None else start.ctypes.data_as(I32), nperp, K.idev[2].ptr,
                  K.hdev.ptr, kx, K.dev[1].ptr, K.dev[2].ptr, k2, shape, npar, seg, prec, None if res is None else res.ctypes.data_as(DP))

    assert call() == 0 and np.all(out == 0.0)
    out[:] = poison
    for what, kw in (("null a", dict(a=None)), ("null rows", dict(rows=None)), ("null row_start", dict(start=None)), ("null result", dict(res=None)),
                     ("ncomp", dict(ncomp=2)), ("precision", dict(prec=7)), ("empty block", dict(shape=empty)), ("row_start not monotone", dict(start=bad_order)),
                     ("row_start ends early", dict(start=bad_end)), ("row_start begins late", dict(start=bad_first)), ("k2 without vectors", dict(k2=1, kx=None)),
                     ("seg_rows < 0", dict(seg=-1)), ("nperp", dict(nperp=0)), ("npar", dict(npar=0))):
        assert call(**kw) == -1, what                                                        # MFFT_ERR_INVALID, before anything is enqueued
        assert np.all(out == poison), what
    assert call(npar=K.npar - 1) == -1 and b"npar" in _lib.load().mfft_last_error()          # found on the device: reported, nothing out of range
    assert np.all(out == poison)
    assert call() == 0 and np.all(out == 0.0)                                                # and the plan still works
    K._perp = (K.nperp, K.npar - 1, K.perp_rows, K.perp_start)
    with pytest.raises(_lib.MfftError):
        spectral.cyl_sums(F, K, U_hat)


def test_line_plans_are_not_supported():
    from mpifft4py_amd import Line_R2C, SelfComm, spectral
    F = Line_R2C(np.array([32, 64]), np.array([2 * np.pi] * 2), SelfComm(0), "double")
    with pytest.raises(NotImplementedError):
        spectral.cyl_sums(F, None, F.empty_complex())


# ---- the examples ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,args,what", [
    ("boussinesq_device.py", ["--N", "16", "--steps", "2", "--g", "1.0", "--spectrum2d"], "kinetic energy"),
    ("mhd_device.py", ["--N", "16", "--steps", "2", "--B0", "1.0", "--spectrum2d"], "total energy")])
def test_examples_print_their_2d_spectra(script, args, what):
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", script)] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    for said in ("%s E(k_perp) = [" % what, "%s E(k_z) = [" % what, "%s share of k_z = 0: " % what, "equals the sum of E(k) to 1e-12"):
        assert said in out, out[-3000:]
