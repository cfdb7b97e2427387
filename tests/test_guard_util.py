"""CPU self-tests of the guard-band harness (tests/guard_util.py): its comparisons are pure numpy functions of the guards as
copied back, so what `check` reports -- side, offsets relative to the payload's edge, count, a NaN left in an output -- is
tested here without a device.  The device side has one test of its own in tests/test_gpu_guarded.py."""
import numpy as np
import pytest

import guard_util as gu

G = 4096


def _guards():
    p = gu.pattern(G)
    return p.copy(), p.copy(), p


def test_pattern_is_fixed_and_not_zeros():
    p = gu.pattern(G)
    assert p.dtype == np.uint8 and p.size == G and not p.flags.writeable
    assert np.array_equal(p, np.random.default_rng(gu.SEED).integers(0, 256, G, dtype=np.uint8))
    assert np.count_nonzero(p) > G * 0.98 and len(np.unique(p)) == 256


def test_untouched_guards_pass():
    before, after, p = _guards()
    assert gu.guard_report(before, after, p) == []


@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_one_flipped_byte_is_reported_with_side_and_offset(side, where):
    """The first and the last byte of either guard; offsets count from the payload's edge: the guard below it is [-G, -1], the one
    above it [0, G - 1]."""
    before, after, p = _guards()
    i = 0 if where == "first" else G - 1
    (before if side == "before" else after)[i] ^= 0x01
    want = i - G if side == "before" else i
    assert gu.guard_report(before, after, p) == [dict(side=side, first=want, last=want, count=1)]
    text = gu.format_guard_report(gu.guard_report(before, after, p))
    assert ("guard %s the payload" % side) in text and ("offsets %d .. %d" % (want, want)) in text


def test_a_stray_zero_store_shows_and_both_sides_are_listed():
    before, after, p = _guards()
    before[-16:] = 0                       # one complex128 just below the payload
    after[:8] = 0                          # one float64 just above it
    nb = int(np.count_nonzero(p[-16:]))
    na = int(np.count_nonzero(p[:8]))
    rep = gu.guard_report(before, after, p)
    assert [r["side"] for r in rep] == ["before", "after"]
    assert rep[0]["count"] == nb and -16 <= rep[0]["first"] <= rep[0]["last"] <= -1
    assert rep[1]["count"] == na and 0 <= rep[1]["first"] <= rep[1]["last"] <= 7
    assert nb > 8 and na > 4               # (bytes of the pattern that are zero themselves cannot show; there are few)


def test_guard_of_another_size_is_an_error():
    before, after, p = _guards()
    with pytest.raises(ValueError):
        gu.guard_report(before[:-1], after, p)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_poison_is_nan_and_one_nan_left_is_reported(dtype):
    """0xFF bytes are a NaN in both precisions, in the real and in the imaginary part; one element left among written ones is
    found with its flat index; an imaginary part alone counts."""
    poisoned = np.frombuffer(bytes([gu.POISON]) * (24 * np.dtype(dtype).itemsize), dtype=dtype).reshape(2, 3, 4)
    rep = gu.poison_report(poisoned)
    assert rep == dict(count=24, first=0, last=23)
    if np.dtype(dtype).kind == "c":
        assert np.all(np.isnan(poisoned.real)) and np.all(np.isnan(poisoned.imag))
    written = np.ones((2, 3, 4), dtype=dtype)
    assert gu.poison_report(written) is None
    written[1, 2, 3] = poisoned[0, 0, 0]
    assert gu.poison_report(written) == dict(count=1, first=23, last=23)
    if np.dtype(dtype).kind == "c":
        written[1, 2, 3] = 1.0
        written[0, 1, 0] = complex(1.0, np.nan)
        assert gu.poison_report(written) == dict(count=1, first=4, last=4)


def test_guard_size_rule():
    """max(64 KiB, twice the leading-axis plane), rounded up to 256 B; a pitched array counts its whole extent."""
    up = lambda n: -(-n // 256) * 256
    assert gu.guard_size((8, 16, 17), np.complex128) == 64 << 10                         # plane 4352 B
    assert gu.guard_size((36, 60, 51), np.complex128) == up(2 * 60 * 51 * 16) == 98048   # 97920 B rounded up
    assert gu.guard_size((3, 7, 9, 12), np.complex64) == 64 << 10
    assert gu.guard_size((130, 130, 250), np.float64) == up(2 * 130 * 250 * 8) == 520192
    assert gu.guard_size((4100, 8, 4), np.complex128) == 64 << 10
    assert gu.guard_size((3, 130, 130, 126), np.complex128) % 256 == 0
    assert gu.guard_size((3, 130, 130, 126), np.complex128) >= 2 * 130 * 130 * 126 * 16
    assert gu.payload_bytes((8, 16, 17), np.complex128, pitch=24) == 8 * 16 * 24 * 16
    assert gu.payload_bytes((8, 16, 17), np.complex128, pitch=17) == 8 * 16 * 17 * 16
    assert gu.guard_size((2, 5), np.float32) == 64 << 10 and gu.guard_size((), np.float64) == 64 << 10
