"""Split-last route (csrc/plan_slab.hip) with its work array W blocked in y and with either order of the strided passes.

Element (x, y, m) of W = (N0, N1, M = N2 / 2) lies at (y / B) * SB + x * SR + (y % B) * M + m; MFFT_SPLIT_LAST_YBLOCK forces B,
MFFT_SPLIT_LAST_YFIRST the order (1: y, x, z forward and z, x, y inverse, both x passes in place on W; 0: x first, the x passes
carry the caller's arrays), plan_info("split_last_yblock" / "split_last_row_pitch" / "split_last_block_pitch") report B, SR, SB.
The checks are those of tests/test_gpu_split_last.py with the same tolerances -- fftn against rfftn, ifftn against irfftn for a
consistent and for an arbitrary spectrum, inputs untouched, repeatable bit for bit -- on meshes chosen for where a blocked layout
can go wrong: partner rows N1 - ky in another block, ky = N1 / 2 on a block start and inside a block, odd meshes, fewer rows than
a workgroup holds, one row per block, rows longer than a wave's threads, and a block that does not divide N1 (plain layout).
One guarded case per direction (tests/guard_util.py): no guard byte changed, no poisoned output element left, inputs unmodified.
The layout arithmetic itself -- every element inside N1 / B * SB, no two on one address -- is also checked without a device."""
import numpy as np
import pytest

from gpu_util import L, TOL, have_gpu
from guard_util import check, guarded

gpu = pytest.mark.gpu

# (mesh, forced block): see the module docstring
CASES = [([12, 20, 64], 4), ([12, 20, 64], 5), ([12, 20, 64], 10), ([9, 15, 64], 3), ([9, 15, 64], 5), ([5, 3, 256], 1),
         ([5, 3, 256], 3), ([2, 2, 64], 1), ([2, 2, 64], 2), ([16, 32, 64], 8), ([32, 16, 2048], 4)]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, list) else str(v)


@pytest.fixture
def _need_gpu():
    if not have_gpu():
        pytest.skip("no HIP device")


def _rel_l2(a, b):
    d = (a - b).reshape(-1)
    return (float(np.vdot(d, d).real) / float(np.vdot(b.reshape(-1), b.reshape(-1)).real)) ** 0.5


def _plan(N, monkeypatch, block, yfirst):
    from mpifft4py_amd import SelfComm, Slab_R2C
    monkeypatch.setenv("MFFT_SPLIT_LAST", "1")
    monkeypatch.setenv("MFFT_SPLIT_LAST_YBLOCK", str(block))
    monkeypatch.setenv("MFFT_SPLIT_LAST_YFIRST", str(yfirst))
    monkeypatch.delenv("MFFT_SPLIT_LAST_PAD", raising=False)
    return Slab_R2C(np.array(N), L, SelfComm(0), "double")


def _random_spectrum(shape, seed):
    B = np.empty(shape, dtype=np.complex128)
    np.random.default_rng(seed).random(out=B.view(np.float64))
    B -= 0.5 + 0.5j
    return B


# ---- the layout arithmetic: no device -------------------------------------------------------------------------------------
def layout_problems(N, B, SR, SB, work_bytes, es=16, exhaustive=True):
    """What is wrong with the blocked layout (B, SR, SB) of W for mesh N in a buffer of work_bytes: a list of strings, empty if
    every element lies inside the buffer and (exhaustive: small meshes) no two elements share an address."""
    N0, N1, M = int(N[0]), int(N[1]), int(N[2]) // 2
    out = []
    if B < 1 or N1 % B:
        return ["block %d does not divide N1 = %d" % (B, N1)]
    if SR < B * M:
        out.append("row pitch %d below a block row of %d" % (SR, B * M))
    if N1 // B > 1 and SB < N0 * SR:
        out.append("block pitch %d below a block of %d" % (SB, N0 * SR))
    if (SR * es) % 128 or (SB * es) % 128:
        out.append("pitches %d / %d are not whole cache lines" % (SR, SB))
    if N1 // B * SB * es > work_bytes:
        out.append("N1 / B * SB = %d elements beyond the %d bytes of the work buffer" % (N1 // B * SB, work_bytes))
    last = (N1 // B - 1) * SB + (N0 - 1) * SR + (B - 1) * M + M - 1
    if (last + 1) * es > work_bytes:
        out.append("last element %d beyond the %d bytes of the work buffer" % (last, work_bytes))
    if exhaustive:
        x, y, m = np.meshgrid(np.arange(N0), np.arange(N1), np.arange(M), indexing="ij")
        off = (y // B) * SB + x * SR + (y % B) * M + m
        if np.unique(off).size != off.size:
            out.append("two elements on one address")
    return out


def _slow_pitch_pad(elems, es=16):
    """csrc/plan_sched.hip slow_pitch_pad: one cache line on top of pitches the strided passes read slowly."""
    b = elems * es
    if b < 65536:
        return 0
    slow = b % 65536 == 0
    if not slow and bin(b).count("1") == 2:
        hi, lo = b.bit_length() - 1, (b & -b).bit_length() - 1
        slow = hi - lo in (7, 8) or (hi - lo == 9 and hi <= 20)
    return 128 // es if slow else 0


def _rule(N, B, es=16):
    """The pitches the plan derives for a forced block B (csrc/plan_slab.hip split_last_layout), in elements."""
    N0, N1, M = N[0], N[1], N[2] // 2
    if B < 1 or B >= N1 or N1 % B:
        B = N1
    if B == N1:
        SR = N1 * M + (128 // es if (N1 * M * es) % 65536 == 0 else 0)
        return B, SR, N0 * SR
    SR = B * M + _slow_pitch_pad(B * M, es)
    return B, SR, N0 * SR + _slow_pitch_pad(N0 * SR, es)


@pytest.mark.parametrize("N,block", CASES + [([12, 20, 64], 7)], ids=_id)
def test_layout_arithmetic(N, block):
    B, SR, SB = _rule(N, block)
    assert layout_problems(N, B, SR, SB, N[1] // B * SB * 16) == []
    assert layout_problems(N, B, SR, SB, N[1] // B * SB * 16 - 16) != []      # one element short: the check notices
    if B > 1 and B < N[1]:
        assert "two elements on one address" in layout_problems(N, B, B * (N[2] // 2) - 8, SB, 1 << 40)


@pytest.mark.parametrize("block", [1024, 256, 64, 32, 16, 8, 4, 1])
def test_layout_arithmetic_1024_cubed(block):
    """The candidates of profiles/split_last_blocked_ab.txt: the work buffer grows by the pads only -- at most one cache line
    per x row of a block, and a row that gets one has 64 KiB or more (0.2 %), and one line per block."""
    N = [1024, 1024, 1024]
    B, SR, SB = _rule(N, block)
    need = N[1] // B * SB * 16
    assert layout_problems(N, B, SR, SB, need, exhaustive=False) == []
    compact = 1024 * 1024 * 512 * 16
    assert need <= compact + compact // 65536 * 128 + N[1] // B * 128


# ---- on the device ------------------------------------------------------------------------------------------------------
def _check_info(F, N, block, yfirst):
    assert F.plan_info("split_last") == 1
    B = F.plan_info("split_last_yblock")
    SR, SB = F.plan_info("split_last_row_pitch"), F.plan_info("split_last_block_pitch")
    assert B == (block if N[1] % block == 0 else N[1]), (B, block)
    assert (B, SR, SB) == _rule(N, block), (B, SR, SB, _rule(N, block))
    assert F.plan_info("split_last_yfirst") == yfirst
    problems = layout_problems(N, B, SR, SB, F.plan_info("work_bytes"))
    assert problems == [], problems


def _check(N, block, yfirst, monkeypatch):
    from mpifft4py_amd import DeviceArray
    F = _plan(N, monkeypatch, block, yfirst)
    A = np.random.default_rng(sum(N)).random(tuple(N))
    u = DeviceArray.from_numpy(A)
    fu = DeviceArray.empty(F.complex_shape(), F.complex)
    F.fftn(u, fu)
    F.sync()
    _check_info(F, N, block, yfirst)
    assert np.array_equal(u.get(), A), "fftn changed its input"
    C = fu.get()
    F.fftn(u, fu)
    F.sync()
    assert np.array_equal(fu.get(), C), "fftn is not repeatable"
    e = _rel_l2(C, np.fft.rfftn(A))
    print("N", N, "B", block, "yfirst", yfirst, "fftn vs rfftn", e)
    assert e < TOL["double"], e
    # (a) the consistent spectrum: back to the field
    u2 = DeviceArray.empty(F.real_shape(), F.float)
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(fu.get(), C), "ifftn changed its input"
    a = u2.get()
    e = _rel_l2(a, A)
    print("N", N, "B", block, "yfirst", yfirst, "ifftn(fftn) vs field", e)
    assert e < 4 * TOL["double"], e
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(u2.get(), a), "ifftn is not repeatable"
    # (b) an arbitrary complex array
    S = _random_spectrum(F.complex_shape(), 5 + sum(N))
    fu.set(S)
    F.ifftn(fu, u2)
    F.sync()
    assert np.array_equal(fu.get(), S), "ifftn changed its input"
    e = _rel_l2(u2.get(), np.fft.irfftn(S, s=tuple(N), axes=(0, 1, 2)))
    print("N", N, "B", block, "yfirst", yfirst, "ifftn vs irfftn, arbitrary spectrum", e)
    assert e < 4 * TOL["double"], e


@gpu
@pytest.mark.parametrize("N,block", CASES, ids=_id)
def test_blocked_against_numpy(N, block, monkeypatch, _need_gpu):
    _check(N, block, 1, monkeypatch)


@gpu
def test_block_that_does_not_divide(monkeypatch, _need_gpu):
    """B = 7 does not divide N1 = 20: the plain layout (split_last_yblock = N1), and still correct."""
    F = _plan([12, 20, 64], monkeypatch, 7, 1)
    assert F.plan_info("split_last_yblock") == 20
    del F
    _check([12, 20, 64], 7, 1, monkeypatch)


@gpu
def test_default_layout_1024_cubed(monkeypatch, _need_gpu):
    """What the rule picks where it turns the route on (profiles/split_last_blocked_ab.txt): the plain array, y first, planes
    16 KiB further apart; x first keeps the one line.  Only the plan is made, nothing is transformed (the transform at this size:
    tests/test_gpu_split_last.py)."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    for k in ("MFFT_SPLIT_LAST", "MFFT_SPLIT_LAST_YBLOCK", "MFFT_SPLIT_LAST_YFIRST", "MFFT_SPLIT_LAST_PAD"):
        monkeypatch.delenv(k, raising=False)
    N = [1024, 1024, 1024]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert F.plan_info("split_last") == 1
    got = tuple(F.plan_info(k) for k in ("split_last_yblock", "split_last_yfirst", "split_last_row_pitch", "split_last_block_pitch"))
    assert got == (1024, 1, 1024 * 512 + 1024, 1024 * (1024 * 512 + 1024)), got
    monkeypatch.setenv("MFFT_SPLIT_LAST_YFIRST", "0")
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    got = tuple(F.plan_info(k) for k in ("split_last_yblock", "split_last_yfirst", "split_last_row_pitch"))
    assert got == (1024, 0, 1024 * 512 + 8), got


@gpu
@pytest.mark.parametrize("yfirst", [0, 1, 2])
@pytest.mark.parametrize("block", [4, 20])
def test_both_orders(block, yfirst, monkeypatch, _need_gpu):
    """The A/B switch: x first (the x passes carry the caller's arrays), y first, and y first in the forward transform only;
    blocked and plain."""
    _check([12, 20, 64], block, yfirst, monkeypatch)


@gpu
@pytest.mark.parametrize("yfirst", [0, 1])
def test_guarded(yfirst, monkeypatch, _need_gpu):
    """[12, 20, 64], B = 4, both directions between guard bands: no stray store, every output element written, inputs kept."""
    N, block = [12, 20, 64], 4
    F = _plan(N, monkeypatch, block, yfirst)
    A = np.random.default_rng(11).random(tuple(N))
    u = guarded(F.real_shape(), F.float, fill=A)
    fu = guarded(F.complex_shape(), F.complex)
    F.fftn(u, fu)
    F.sync()
    _check_info(F, N, block, yfirst)
    check(u, "fftn input")
    check(fu, "fftn output")
    assert _rel_l2(fu.get(), np.fft.rfftn(A)) < TOL["double"]
    S = _random_spectrum(F.complex_shape(), 12)
    fi = guarded(F.complex_shape(), F.complex, fill=S)
    uo = guarded(F.real_shape(), F.float)
    F.ifftn(fi, uo)
    F.sync()
    check(fi, "ifftn input")
    check(uo, "ifftn output")
    assert _rel_l2(uo.get(), np.fft.irfftn(S, s=tuple(N), axes=(0, 1, 2))) < 4 * TOL["double"]
