"""CPU: the body of the fused z stage that ends in a JOINT histogram (csrc/nlz_joint.h NlzJoint::body, Op::JointHistogram) runs in the
workgroup emulator (`make emu_nlj`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier
builds, whole-complex and split exchanges, with and without LDS twiddles, 2 and 6 fields, one row, odd row counts and row counts
of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, the bin pairs
(1, 1), (7, 33), (64, 64) and (64, 1), a NaN and an Inf in one bin of one field.  Per case (csrc/emu/test_nlj.h): the cells of a
pair sum to the points, no cell of the partial grids is left unwritten, the inputs are preserved; every two-dimensional
cumulative count lies between those of the long-double rows shifted by -+ the worst-case error of the row's transform; both
marginals EQUAL what NlzHist of the same template parameters counts; a bad bin marks its own field only.  Then the entry points of
the feature in the header, the binding and the library, the cell rule of the module and the host arithmetic of
`spectral.JointHistogram`."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_joint_histogram", "mfft_ew_joint_histogram", "mfft_nlz_joint_rows", "mfft_nlz_joint_groups"]


def _case(l):
    m = re.match(r"nlj f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+) b(\d+)x(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v", "ba", "bb"), (int(x) for x in m.groups()))) if m else None


def test_joint_body_in_the_emulator():
    r = run_group("nlj")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlj ")]
    lengths = nlz_lengths()
    assert len(lengths) == 32
    for n in lengths:
        mine = [l for l in lines if re.search(r"N=%d\s" % n, l)]
        assert all(l.rstrip().endswith("ok") for l in mine), mine
        for prec in ("double", "single"):
            p = [l for l in mine if prec in l]
            plain = [l for l in p if " in field" not in l]
            cases = [_case(l) for l in plain]
            assert len(plain) >= 4 and all(cases), (n, prec, plain)
            assert any(" nan in field" in l for l in p) and any(" inf in field" in l for l in p), (n, prec)
            assert any(" split" in l for l in plain) and any(" split" not in l for l in plain), (n, prec)
            assert any(" twlds" in l for l in plain) and any(" twlds" not in l for l in plain), (n, prec)
            assert any(c["n"] == 1 for c in cases), (n, prec)                                   # one row
            assert any(c["n"] > 1 and c["n"] % 2 == 1 for c in cases), (n, prec)                # odd row counts
            # the loop over the rows iterates and ends unevenly: more than two passes of g workgroups of 2 r rows, and a rest
            assert any(c["n"] > 2 * c["g"] * 2 * c["r"] and c["n"] % (c["g"] * 2 * c["r"]) != 0 for c in cases), (n, prec)
            assert any(c["vin"] < c["v"] for c in cases), (n, prec)                             # pruned valid_in
            assert any(c["v"] == n // 3 + 1 for c in cases) and any(c["v"] == n // 2 + 1 for c in cases), (n, prec)
            assert set(c["f"] for c in cases) == {2, 6}, (n, prec)
        cases = [_case(l) for l in mine if " in field" not in l]
        assert {(1, 1), (7, 33), (64, 64), (64, 1)} <= set((c["ba"], c["bb"]) for c in cases), n
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_marks_its_field_only():
    """A NaN or an Inf bin of one field: at least one count in ITS non-finite slot; the partner's marginal and every other pair
    have EXACTLY the counts of the run without the bad bin: the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nlj")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlj ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nlj f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nlj f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def _slot(x, lo, inv, nb):
    """the slot rule of the header, one value at a time"""
    t = (x - lo) * inv
    if x != x:
        return nb + 2
    if t < 0:
        return 0
    if t >= nb:
        return nb + 1
    return 1 + int(t)


def test_cell_rule_of_the_module_is_the_documented_one():
    from mpifft4py_amd import spectral
    assert spectral.JOINT_MAXBINS == 64
    v = np.array([-np.inf, -1.0, -0.5, -0.5 + 1e-16, 0.0, 0.25, 0.4999999, 0.5, 7.0, np.inf, np.nan, 1e308, -1e308])
    xa, xb = (g.ravel() for g in np.meshgrid(v, v, indexing="ij"))
    lo, hi = (-0.5, -1.0), (0.5, 0.25)
    for nba, nbb in ((1, 1), (7, 33), (64, 64), (64, 1)):
        got = spectral.joint_cells(xa, xb, lo, hi, (nba, nbb))
        with np.errstate(all="ignore"):
            want = [_slot(float(a), lo[0], nba / (hi[0] - lo[0]), nba) * (nbb + 3) + _slot(float(b), lo[1], nbb / (hi[1] - lo[1]), nbb)
                    for a, b in zip(xa, xb)]
        assert np.array_equal(got, np.array(want)), (nba, nbb)
        assert got.min() == 0 and got.max() == (nba + 3) * (nbb + 3) - 1                        # (-Inf, -Inf) and (NaN, NaN)
    assert np.array_equal(spectral.joint_cells(xa, xb, lo, hi, 7), spectral.joint_cells(xa, xb, lo, hi, (7, 7)))


def test_joint_histogram_object_host_arithmetic():
    """pdf times the cell area sums to 1 - outside / count, the marginals are the row and column sums with the border slots,
    conditional_mean of a sample with b = 2 a lies within half a bin of 2 x centre."""
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(11)
    n, nba, nbb = 30001, 20, 40
    a = np.stack([rng.standard_normal(n), rng.random(n) * 2 - 1.0])
    b = np.stack([2.0 * a[0], rng.standard_normal(n) ** 3])
    a[1, :4] = np.nan
    b[1, 9] = np.inf
    lo = np.array([[-2.0, -4.0], [-0.75, -2.0]])      # [pair][a, b]
    hi = np.array([[2.0, 4.0], [0.5, 2.5]])
    raw = np.stack([np.bincount(spectral.joint_cells(a[p], b[p], lo[p], hi[p], (nba, nbb)), minlength=(nba + 3) * (nbb + 3)) for p in range(2)])
    h = spectral.JointHistogram(n, raw, lo, hi, (nba, nbb))
    assert h.raw.shape == (2, nba + 3, nbb + 3) and h.counts.shape == (2, nba, nbb) and h.counts.dtype == np.int64
    assert h.count == n and h.npairs == 2 and h.nbins == (nba, nbb)
    for p in range(2):
        assert h.raw[p].sum() == n and h.outside(p) == n - h.counts[p].sum() and h.outside(p) >= 1
        area = (hi[p, 0] - lo[p, 0]) / nba * (hi[p, 1] - lo[p, 1]) / nbb
        assert abs(float(h.pdf(p).sum() * area) - (1.0 - h.outside(p) / n)) <= 1e-12
        for axis, nb in ((0, nba), (1, nbb)):
            e, c = h.edges(p, axis), h.centers(p, axis)
            assert e.shape == (nb + 1,) and e[0] == lo[p, axis] and e[-1] == hi[p, axis] and np.allclose(c, 0.5 * (e[1:] + e[:-1]), rtol=1e-15)
    for axis, x, nb in ((0, a, nba), (1, b, nbb)):
        m = h.marginal(axis)
        assert isinstance(m, spectral.Histogram) and m.count == n and m.nbins == nb
        for p in range(2):
            want = np.bincount(spectral.hist_slots(x[p], lo[p, axis], hi[p, axis], nb), minlength=nb + 3)
            got = np.concatenate([[m.below[p]], m.counts[p], [m.above[p]], [m.nonfinite[p]]])
            assert np.array_equal(got, want), (axis, p)
    assert h.marginal(0).nonfinite.tolist() == [0, 4] and h.marginal(1).above[1] >= 1
    cm = h.conditional_mean(0, of=1)
    filled = h.counts[0].sum(axis=1) > 0
    assert filled.sum() >= nba - 2 and np.all(np.isnan(cm[~filled]))
    # (an a bin maps onto exactly two b bins here, whose centres lie half a b bin either side of 2 x the a bin's centre)
    assert np.all(np.abs(cm[filled] - 2.0 * h.centers(0, 0)[filled]) <= 0.5 * (hi[0, 1] - lo[0, 1]) / nbb + 1e-12)
    empty = spectral.JointHistogram(5, np.zeros((1, 4, 4), dtype=np.int64), [[0.0, 0.0]], [[1.0, 1.0]], 1)
    assert np.all(np.isnan(empty.conditional_mean(0))) and np.all(np.isnan(empty.conditional_mean(0, of=0)))
