"""GPU: the outer product between guard bands (tests/guard_util.py, as tests/test_gpu_guarded.py): mfft_nonlinear_outer on the
fused and on the composed route, its z stage mfft_nlz_outer_rows, and mfft_ew_elsasser_rhs.  Inputs lie in guarded arrays, outputs
in guarded, poisoned ones; after one operation no guard byte has changed, every output slot has been written, the inputs come
back bit for bit, and the result meets the bound of the operation's own test (4 TOL against the oracle / numpy)."""
import numpy as np
import pytest

import nonlinear_util as nl
import outer_util as ou
from gpu_util import L, TOL, cdtype, have_gpu, orc, run_ranks
from guard_util import check, collect, guarded

pytestmark = pytest.mark.gpu
DEALIAS = [None, "2/3-rule", "3/2-rule"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, (list, tuple)) else str(v)


_REF = {}


def _reference(N, prec, dealias):
    key = (tuple(N), prec, dealias)
    if key not in _REF:
        from mpifft4py_amd import SelfComm, Slab_R2C
        H = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        a, b = nl.spectra(tuple(H.complex_shape()), np.array(N), prec, 13 + N[2], True, 2)
        mask = H.get_dealias_filter() if dealias == "2/3-rule" else None
        _REF[key] = (a, b, ou.oracle(a, b, np.array(N), prec, dealias, mask))
    return _REF[key]


def _case(N, P, prec, dealias, fused, complex_pitch=None):
    from mpifft4py_amd import Slab_R2C, spectral
    a, b, want = _reference(N, prec, dealias)

    def body(comm):
        F = Slab_R2C(np.array(N), L, comm, prec, complex_pitch=complex_pitch)
        cs = tuple(int(x) for x in F.complex_shape())
        sl = (slice(None),) + tuple(F.complex_local_slice())
        d = [guarded((3,) + cs, F.complex, pitch=F.complex_pitch, fill=X[sl]) for X in (a, b)]
        out = guarded((9,) + cs, F.complex, pitch=F.complex_pitch)
        spectral.outer_transform(F, d[0], d[1], out, dealias)
        F.sync()
        problems = []
        collect(problems, out, "rank %d outer output" % comm.Get_rank())
        for i, x in enumerate(d):
            collect(problems, x, "rank %d outer input %d" % (comm.Get_rank(), i))
        return problems, orc.rel_l2(out.get(), want[sl]), F.plan_info(ou.info_key(dealias))
    res = run_ranks(P, body)
    problems = [p for r in res for p in r[0]]
    assert not problems, "\n".join(problems)
    for _, err, flag in res:
        print("outer P=%d %s %s %s: rel-L2 %.3e (bound %.1e), fused flag %d" % (P, N, dealias, prec, err, 4 * TOL[prec], flag))
        assert flag == (1 if fused else 0), (flag, fused)
        assert err < 4 * TOL[prec], err


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)], ids=_id)
def test_outer_one_rank(N, fused, dealias, prec):
    """One rank: the fused route on [8, 16, 32] (flag 1) and the plan's own composition on [24, 40, 20] (no fused z kernel of length
    20 or 30: flag 0)."""
    _case(N, 1, prec, dealias, fused)


@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
def test_outer_two_slab_ranks(dealias):
    """Two slab ranks, the fused route behind the exchanges: nine results through buffers sized for nine fields."""
    _case([8, 16, 32], 2, "double", dealias, True)


@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
def test_outer_pitched_plan(dealias):
    _case([8, 16, 32], 1, "double", dealias, True, complex_pitch="auto")


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n,nrows", [(32, 37), (48, 1), (144, 5), (216, 37), (1024, 3)])
def test_nlz_outer_rows(n, nrows, prec):
    """The z stage on its own, out of place: a wave-synchronous 8-values plan, the 12-values plans and a multi-wave row; odd row
    counts and a single row; `valid` the bins of the 3/2-rule, so the rows' tails (pitch = valid + 3) must stay poisoned."""
    from mpifft4py_amd import _lib
    valid = n // 3 + 1
    pitch = valid + 3
    rng = np.random.default_rng(n + nrows)
    a, b = ((rng.random((3, nrows, pitch)) - 0.5 + 1j * (rng.random((3, nrows, pitch)) - 0.5)).astype(cdtype(prec)) for _ in range(2))
    da, db = guarded(a.shape, cdtype(prec), fill=a), guarded(b.shape, cdtype(prec), fill=b)
    out = guarded((9, nrows, pitch), cdtype(prec))
    _lib.call("mfft_nlz_outer_rows", da.ptr, db.ptr, out.ptr, nrows, n, pitch, valid, _lib.precision_code(prec), 1)
    check(da, "nlz_outer_rows a")
    check(db, "nlz_outer_rows b")
    check(out, "nlz_outer_rows out", expect="guards")
    got = out.get()
    assert not np.isnan(got[..., :valid]).any()                      # every slot of the valid bins written
    assert np.isnan(got[..., valid:].real).all() and np.isnan(got[..., valid:].imag).all()      # ... and nothing beyond them

    def back(x):
        x = x[..., :valid].astype(np.complex128)
        x[..., 0] = x[..., 0].real
        return np.fft.irfft(x, n=n, axis=-1)
    ua, ub = back(a), back(b)
    want = np.stack([np.fft.rfft(ua[i] * ub[j], axis=-1)[..., :valid] for i in range(3) for j in range(3)])
    assert orc.rel_l2(got[..., :valid], want) < 4 * TOL[prec]


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("pitch", [None, "auto"], ids=_id)
def test_elsasser_rhs(pitch, prec):
    """mfft_ew_elsasser_rhs: both results written everywhere, the three inputs bit for bit, no guard byte changed; the K = 0 bin is
    exactly zero.  (Its values against numpy: tests/test_gpu_nonlinear_outer.py.)"""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=pitch)
    cs = tuple(int(x) for x in F.complex_shape())
    rng = np.random.default_rng(7)
    rnd = lambda n: (rng.random((n,) + cs) - 0.5 + 1j * (rng.random((n,) + cs) - 0.5)).astype(cdtype(prec))
    T, Zp, Zm = (guarded(x.shape, F.complex, pitch=F.complex_pitch, fill=x) for x in (rnd(9), rnd(3), rnd(3)))
    gp, gm = guarded((3,) + cs, F.complex, pitch=F.complex_pitch), guarded((3,) + cs, F.complex, pitch=F.complex_pitch)
    spectral.elsasser_rhs(F, spectral.Wavenumbers(F), T, Zp, Zm, gp, gm, 0.02, 0.01)
    F.sync()
    for v, what in ((T, "T_hat"), (Zp, "Zp_hat"), (Zm, "Zm_hat"), (gp, "dZp"), (gm, "dZm")):
        check(v, "elsasser_rhs " + what)
    assert np.all(gp.get()[:, 0, 0, 0] == 0) and np.all(gm.get()[:, 0, 0, 0] == 0)
