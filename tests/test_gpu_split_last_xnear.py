"""Split-last route "x near" (csrc/plan_slab.hip): a second, transposed work array W_T -- element (x, y, m) at y * SB + x * SR + m --
so that the x passes run on rows 8 KiB apart, and the pair kernels' slots taken in tiles of G x G (csrc/fft_kernels.h pair_slot).

MFFT_SPLIT_LAST_XNEAR chooses the directions (1 both, 2 forward only, 3 inverse only), MFFT_SPLIT_LAST_PAIRBLOCK forces G;
plan_info("split_last_xnear" / "split_last_pairblock" / "split_last_xnear_row_pitch" / "split_last_xnear_block_pitch") report them.
The kernels and the order of the sums are those of the route without W_T (plain W, y first), so every output must equal that
route's BIT FOR BIT -- fftn, ifftn of the consistent spectrum and ifftn of an arbitrary, non-Hermitian one -- besides meeting numpy
within gpu_util.TOL; inputs stay untouched and a second call repeats the bits.  Meshes: a self-partner row and plane, ky = N1 / 2,
odd meshes, fewer rows than a workgroup holds, rows longer than a wave's threads, and [34, 18, 64] whose 18 x 18 slot grid has partial
edge tiles in both directions for G = 4.  One guarded and poisoned case per direction (tests/guard_util.py).  Without a device:
the slot map and the kernels in the emulator, and the layout arithmetic of both arrays, are in tests/test_split_last_xnear_emu.py."""
import numpy as np
import pytest

from gpu_util import L, TOL, have_gpu
from guard_util import check, guarded
from test_gpu_split_last_blocked import _rule, layout_problems

gpu = pytest.mark.gpu

MESHES = [[2, 2, 64], [5, 3, 256], [9, 15, 64], [12, 20, 64], [16, 32, 64], [32, 16, 2048], [34, 18, 64]]
TILES = [0, 4, 16]
MODES = [1, 2, 3]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, list) else str(v)


@pytest.fixture
def _need_gpu():
    if not have_gpu():
        pytest.skip("no HIP device")


def _rel_l2(a, b):
    d = (a - b).reshape(-1)
    return (float(np.vdot(d, d).real) / float(np.vdot(b.reshape(-1), b.reshape(-1)).real)) ** 0.5


def _plan(N, monkeypatch, mode, tile):
    """Split-last forced on, plain W, y first; the route and the tile as asked (tile None: the rule's own)."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    monkeypatch.setenv("MFFT_SPLIT_LAST", "1")
    monkeypatch.setenv("MFFT_SPLIT_LAST_YFIRST", "1")
    monkeypatch.setenv("MFFT_SPLIT_LAST_XNEAR", str(mode))
    for k in ("MFFT_SPLIT_LAST_YBLOCK", "MFFT_SPLIT_LAST_PAD", "MFFT_SPLIT_LAST_XNEAR_PAD", "MFFT_SPLIT_LAST_PAIRBLOCK",
              "MFFT_SPLIT_LAST_PAIRXFAST"):
        monkeypatch.delenv(k, raising=False)
    if tile is not None:
        monkeypatch.setenv("MFFT_SPLIT_LAST_PAIRBLOCK", str(tile))
    return Slab_R2C(np.array(N), L, SelfComm(0), "double")


def _random_spectrum(shape, seed):
    B = np.empty(shape, dtype=np.complex128)
    np.random.default_rng(seed).random(out=B.view(np.float64))
    B -= 0.5 + 0.5j
    return B


_REF = {}


def _reference(N, monkeypatch):
    """Per mesh, once: the field, an arbitrary spectrum, numpy's transforms of them and what the route WITHOUT W_T (slots in row
    order) stores for them.  Shared by every case of the mesh; nobody changes it."""
    key = tuple(N)
    if key not in _REF:
        from mpifft4py_amd import DeviceArray
        F = _plan(N, monkeypatch, 0, 0)
        A = np.random.default_rng(sum(N)).random(tuple(N))
        S = _random_spectrum(F.complex_shape(), 5 + sum(N))
        u = DeviceArray.from_numpy(A)
        fu = DeviceArray.empty(F.complex_shape(), F.complex)
        u2 = DeviceArray.empty(F.real_shape(), F.float)
        F.fftn(u, fu)
        F.sync()
        assert F.plan_info("split_last") == 1 and F.plan_info("split_last_xnear") == 0 and F.plan_info("split_last_pairblock") == 0
        assert F.plan_info("split_last_yblock") == N[1] and F.plan_info("split_last_yfirst") == 1
        C = fu.get()
        F.ifftn(fu, u2)
        F.sync()
        back = u2.get()
        fu.set(S)
        F.ifftn(fu, u2)
        F.sync()
        _REF[key] = dict(A=A, S=S, C=C, back=back, arb=u2.get(), rfftn=np.fft.rfftn(A),
                         irfftn=np.fft.irfftn(S, s=tuple(N), axes=(0, 1, 2)))
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


def _check_info(F, N, mode, tile, padded=False):
    assert F.plan_info("split_last") == 1
    assert F.plan_info("split_last_xnear") == mode
    assert F.plan_info("split_last_pairblock") == tile
    M = N[2] // 2
    SR, SB = F.plan_info("split_last_xnear_row_pitch"), F.plan_info("split_last_xnear_block_pitch")
    assert SR >= M and SB >= N[0] * SR and (SR * 16) % 128 == 0 and (SB * 16) % 128 == 0, (SR, SB)
    assert padded or (1, SR, SB) == _rule(N, 1), (SR, SB, _rule(N, 1))
    problems = layout_problems(N, 1, SR, SB, F.plan_info("split_last_xnear_work_bytes"))
    assert problems == [], problems
    if mode != 3:      # the forward direction goes through the plain array too
        assert F.plan_info("work_bytes") >= ((N[0] - 1) * F.plan_info("split_last_row_pitch") + N[1] * M) * 16


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N", MESHES, ids=_id)
def test_xnear_bits_and_numpy(N, tile, mode, monkeypatch, _need_gpu):
    from mpifft4py_amd import DeviceArray
    R = _reference(N, monkeypatch)
    F = _plan(N, monkeypatch, mode, tile)
    u = DeviceArray.from_numpy(R["A"])
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    F.fftn(u, fu)
    F.sync()
    assert np.array_equal(u.get(), R["A"]), "fftn changed its input"
    C = fu.get()
    assert np.array_equal(C, R["C"]), "fftn: not the bits of the route without W_T"
    F.fftn(u, fu)
    F.sync()
    assert np.array_equal(fu.get(), C), "fftn is not repeatable"
    e = _rel_l2(C, R["rfftn"])
    print("N", N, "G", tile, "xnear", mode, "fftn vs rfftn", e)
    assert e < TOL["double"], e
    # (a) the consistent spectrum: back to the field
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    F.ifftn(fu, u2)
    F.sync()
    _check_info(F, N, mode, tile)
    assert np.array_equal(fu.get(), C), "ifftn changed its input"
    a = u2.get()
    assert np.array_equal(a, R["back"]), "ifftn: not the bits of the route without W_T"
    e = _rel_l2(a, R["A"])
    print("N", N, "G", tile, "xnear", mode, "ifftn(fftn) vs field", e)
    assert e < 4 * TOL["double"], e
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(u2.get(), a), "ifftn is not repeatable"
    # (b) an arbitrary complex array (not the transform of a real field)
    fu.set(R["S"])
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(fu.get(), R["S"]), "ifftn changed its input"
    b = u2.get()
    assert np.array_equal(b, R["arb"]), "ifftn, arbitrary spectrum: not the bits of the route without W_T"
    e = _rel_l2(b, R["irfftn"])
    print("N", N, "G", tile, "xnear", mode, "ifftn vs irfftn, arbitrary spectrum", e)
    assert e < 4 * TOL["double"], e


@gpu
def test_rule_tile_and_forward_needs_plain_yfirst(monkeypatch, _need_gpu):
    """Unset, G is the rule's (tiles on the route, row order without it); the forward direction needs the plain W with y first and
    is left out -- reported so -- where the switches choose another layout or order; the inverse runs on W_T alone."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N = [12, 20, 64]
    F = _plan(N, monkeypatch, 1, None)
    assert F.plan_info("split_last_xnear") == 1 and F.plan_info("split_last_pairblock") > 0
    F = _plan(N, monkeypatch, 0, None)
    assert F.plan_info("split_last_xnear") == 0 and F.plan_info("split_last_pairblock") == 0
    assert F.plan_info("split_last_xnear_block_pitch") == 0
    _plan(N, monkeypatch, 1, None)
    monkeypatch.setenv("MFFT_SPLIT_LAST_YBLOCK", "4")
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert F.plan_info("split_last_xnear") == 3
    monkeypatch.delenv("MFFT_SPLIT_LAST_YBLOCK")
    monkeypatch.setenv("MFFT_SPLIT_LAST_YFIRST", "0")
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert F.plan_info("split_last_xnear") == 3
    monkeypatch.setenv("MFFT_SPLIT_LAST_XNEAR", "2")
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert F.plan_info("split_last_xnear") == 0


@gpu
@pytest.mark.parametrize("xfast", [1, 2, 3])
@pytest.mark.parametrize("N,tile", [([34, 18, 64], 4), ([9, 15, 64], 16), ([32, 16, 2048], 4)], ids=_id)
def test_kx_fastest_inside_the_tiles(N, tile, xfast, monkeypatch, _need_gpu):
    """MFFT_SPLIT_LAST_PAIRXFAST: kx instead of ky fastest inside a tile, in the forward (1), the inverse (2) or both z passes (3);
    another order of the same slots, the same bits."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C
    R = _reference(N, monkeypatch)
    _plan(N, monkeypatch, 1, tile)
    monkeypatch.setenv("MFFT_SPLIT_LAST_PAIRXFAST", str(xfast))
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    u = DeviceArray.from_numpy(R["A"])
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    F.fftn(u, fu)
    F.ifftn(fu, u2)
    F.sync()
    assert F.plan_info("split_last_xnear") == 1 and F.plan_info("split_last_pairxfast") == xfast
    assert np.array_equal(fu.get(), R["C"]) and np.array_equal(u2.get(), R["back"])
    fu.set(R["S"])
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(u2.get(), R["arb"])


@gpu
def test_block_pitch_pad(monkeypatch, _need_gpu):
    """MFFT_SPLIT_LAST_XNEAR_PAD: whole cache lines between the y blocks of W_T; the same bits."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C
    N = [9, 15, 64]
    R = _reference(N, monkeypatch)
    _plan(N, monkeypatch, 1, 4)
    monkeypatch.setenv("MFFT_SPLIT_LAST_XNEAR_PAD", "384")
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    u = DeviceArray.from_numpy(R["A"])
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    F.fftn(u, fu)
    F.ifftn(fu, u2)
    F.sync()
    SR = F.plan_info("split_last_xnear_row_pitch")
    assert F.plan_info("split_last_xnear_block_pitch") == N[0] * SR + 384 // 16
    _check_info(F, N, 1, 4, padded=True)
    assert np.array_equal(fu.get(), R["C"]) and np.array_equal(u2.get(), R["back"])


@gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_guarded(mode, monkeypatch, _need_gpu):
    """[34, 18, 64], G = 4, one direction on the route at a time, between guard bands: no stray store, every output element
    written (the outputs start poisoned), inputs kept."""
    N, tile = [34, 18, 64], 4
    R = _reference(N, monkeypatch)
    F = _plan(N, monkeypatch, mode, tile)
    u = guarded(F.real_shape(), F.float, fill=R["A"])
    fu = guarded(F.complex_shape(), F.complex)
    F.fftn(u, fu)
    F.sync()
    check(u, "fftn input")
    check(fu, "fftn output")
    assert np.array_equal(fu.get(), R["C"])
    fi = guarded(F.complex_shape(), F.complex, fill=R["S"])
    uo = guarded(F.real_shape(), F.float)
    F.ifftn(fi, uo)
    F.sync()
    _check_info(F, N, mode, tile)
    check(fi, "ifftn input")
    check(uo, "ifftn output")
    assert np.array_equal(uo.get(), R["arb"])
    assert _rel_l2(uo.get(), R["irfftn"]) < 4 * TOL["double"]
