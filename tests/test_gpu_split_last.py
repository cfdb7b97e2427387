"""One-rank slab R2C route that splits real / complex at the SPECTRUM end (csrc/plan_slab.hip slab_forward_split_last):
x and y as c2c passes on the real array read as complex pairs, the pair-row z kernels last (csrc/fft_kernels.h PAIR).
Forced on with MFFT_SPLIT_LAST=1 (by rule it runs for the 1024^3 double-precision mesh only) and checked against numpy:
fftn against rfftn, ifftn against irfftn for a consistent spectrum AND for an arbitrary complex one (irfftn ignores the
anti-Hermitian part of the planes kz = 0 and N2/2: the pair-merge pass must do the same), inputs untouched, repeatable bit
for bit, and the switch inert on meshes the rule leaves alone."""
import numpy as np
import pytest

from gpu_util import L, TOL, have_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.skip("no HIP device")


def _rel_l2(a, b):
    """|a - b| / |b| without temporaries of the arrays' size (the 1024^3 case)."""
    a2 = a.reshape(a.shape[0], -1)
    b2 = b.reshape(b.shape[0], -1)
    num = den = 0.0
    for i in range(a2.shape[0]):
        d = a2[i] - b2[i]
        num += float(np.vdot(d, d).real)
        den += float(np.vdot(b2[i], b2[i]).real)
    return (num / den) ** 0.5


def _plan(N, monkeypatch, switch):
    from mpifft4py_amd import SelfComm, Slab_R2C
    if switch is None:
        monkeypatch.delenv("MFFT_SPLIT_LAST", raising=False)
    else:
        monkeypatch.setenv("MFFT_SPLIT_LAST", switch)
    return Slab_R2C(np.array(N), L, SelfComm(0), "double")


def _random_spectrum(shape, seed):
    B = np.empty(shape, dtype=np.complex128)
    np.random.default_rng(seed).random(out=B.view(np.float64))
    B -= 0.5 + 0.5j
    return B


def _check(N, monkeypatch):
    from mpifft4py_amd import DeviceArray
    F = _plan(N, monkeypatch, "1")
    A = np.random.default_rng(sum(N)).random(tuple(N))
    u = DeviceArray.from_numpy(A)
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    F.fftn(u, fu)
    F.sync()
    assert F.plan_info("split_last") == 1
    assert np.array_equal(u.get(), A), "fftn changed its input"
    C = fu.get()
    F.fftn(u, fu)
    F.sync()
    assert np.array_equal(fu.get(), C), "fftn is not repeatable"
    want = np.fft.rfftn(A)
    e = _rel_l2(C, want)
    print("N", N, "fftn vs rfftn", e)
    assert e < TOL["double"], e
    del want
    # (a) the consistent spectrum: back to the field
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(fu.get(), C), "ifftn changed its input"
    a = u2.get()
    e = _rel_l2(a, A)
    print("N", N, "ifftn(fftn) vs field", e)
    assert e < 4 * TOL["double"], e
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(u2.get(), a), "ifftn is not repeatable"
    del a, C, A
    # (b) an arbitrary complex array
    B = _random_spectrum(F.complex_shape(), 5 + sum(N))
    fu.set(B)
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(fu.get(), B), "ifftn changed its input"
    b = u2.get()
    want = np.fft.irfftn(B, s=tuple(N), axes=(0, 1, 2))
    e = _rel_l2(b, want)
    print("N", N, "ifftn vs irfftn, arbitrary spectrum", e)
    assert e < 4 * TOL["double"], e


@pytest.mark.parametrize("N", [[12, 20, 64], [9, 15, 64], [16, 32, 64], [5, 3, 256], [2, 2, 64], [32, 16, 2048], [256, 256, 256]])
def test_split_last_against_numpy(N, monkeypatch):
    _check(N, monkeypatch)


def test_split_last_1024_cubed(monkeypatch):
    """The size the rule turns the route on for; also checks that the rule does (no switch set; the key decides whether the
    work buffer fits when it is asked before the first transform)."""
    F = _plan([1024, 1024, 1024], monkeypatch, None)
    assert F.plan_info("split_last") == 1
    del F
    _check([1024, 1024, 1024], monkeypatch)


@pytest.mark.parametrize("N", [[12, 20, 64], [9, 15, 64], [256, 256, 256]])
def test_switch_off_is_the_regular_route(N, monkeypatch):
    """On meshes the rule leaves alone the switch set to 0 changes nothing (bit for bit the same as no switch: both take the
    regular route, whose own output the existing parity tests hold to the oracle), plan_info says which route a plan
    takes, and the forced route agrees with the regular one to rounding."""
    A = np.random.default_rng(1 + sum(N)).random(tuple(N))
    got = {}
    for switch in (None, "0", "1"):
        F = _plan(N, monkeypatch, switch)
        fu = F.fftn(A.copy(), np.zeros(F.complex_shape(), dtype=np.complex128))
        u = F.ifftn(fu.copy(), np.zeros(F.real_shape(), dtype=np.float64))
        assert F.plan_info("split_last") == (1 if switch == "1" else 0)
        got[switch] = (fu, u)
    assert np.array_equal(got[None][0], got["0"][0]) and np.array_equal(got[None][1], got["0"][1])
    assert _rel_l2(got["1"][0], got["0"][0]) < TOL["double"] and _rel_l2(got["1"][1], got["0"][1]) < TOL["double"]


def test_forced_route_replays_captured_graphs(monkeypatch):
    """Small meshes replay captured hipGraphs (MFFT_GRAPH=1): the forced route must stay capturable."""
    from mpifft4py_amd import DeviceArray
    monkeypatch.setenv("MFFT_GRAPH", "1")
    N = [12, 20, 64]
    F = _plan(N, monkeypatch, "1")
    A = np.random.default_rng(3).random(tuple(N))
    u = DeviceArray.from_numpy(A)
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    for _ in range(4):          # direct, captured, replayed
        F.fftn(u, fu)
        F.ifftn(fu, u2)
    F.sync()
    assert F.plan_info("split_last") == 1
    assert _rel_l2(fu.get(), np.fft.rfftn(A)) < TOL["double"]
    assert _rel_l2(u2.get(), A) < 4 * TOL["double"]
