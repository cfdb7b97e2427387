"""CPU: the body of the fused z stage that ends in a histogram (csrc/nlz_hist.h NlzHist::body, Op::Histogram) runs in the workgroup
emulator (`make emu_nlh`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier builds,
whole-complex and split exchanges, with and without LDS twiddles, field counts 1, 2, 3 and 6, one row, odd row counts and row
counts of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, bin counts
from 1 to the maximum, a NaN and an Inf in one bin of one field.  Per case every cumulative count lies between those of the
long-double rows shifted by -+ the worst-case error of the row's transform (csrc/emu/test_nlh.h), the slots of a field sum to the
number of points, no slot of the partial histograms is left unwritten and the inputs are preserved.  Then the entry points of the
feature in the header, the binding and the library, and the host arithmetic of `spectral.Histogram`."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_histogram", "mfft_ew_histogram", "mfft_nlz_hist_rows", "mfft_nlz_hist_groups"]


def _case(l):
    m = re.match(r"nlh f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+) b(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v", "b"), (int(x) for x in m.groups()))) if m else None


def test_histogram_body_in_the_emulator():
    r = run_group("nlh")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlh ")]
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
            assert len(set(c["b"] for c in cases)) >= 2, (n, prec)                              # more than one bin count
        cases = [_case(l) for l in mine if " in field" not in l]
        assert set(c["f"] for c in cases) == {1, 2, 3, 6}, n
        assert {1, 512} <= set(c["b"] for c in cases), n                                       # one bin, and the maximum
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_marks_its_field_only():
    """A NaN or an Inf bin of one field: at least one count in ITS non-finite slot, its slots still sum to the points; the other
    fields -- the partner on the same complex transform among them -- have EXACTLY the counts of the run without the bad bin:
    the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nlh")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlh ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nlh f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nlh f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def _slots(x, lo, hi, nbins):
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.asarray(x, dtype=np.float64) - lo) * (np.float64(nbins) / (np.float64(hi) - np.float64(lo)))
    s = np.where(t < 0, 0, np.where(t >= nbins, nbins + 1, 1 + np.where((t >= 0) & (t < nbins), t, 0).astype(np.int64)))
    return np.where(np.isnan(x), nbins + 2, s)


def test_slot_rule_of_the_module_is_the_documented_one():
    from mpifft4py_amd import spectral
    x = np.array([-np.inf, -1.0, -0.5, -0.5 + 1e-16, 0.0, 0.25, 0.4999999, 0.5, 7.0, np.inf, np.nan, 1e308, -1e308])
    for nbins in (1, 7, 64, spectral.HIST_MAXBINS):
        got = spectral.hist_slots(x, -0.5, 0.5, nbins)
        assert np.array_equal(got, _slots(x, -0.5, 0.5, nbins)), (nbins, got)
        assert got[0] == 0 and got[2] == 1 and got[7] == nbins + 1 and got[9] == nbins + 1 and got[10] == nbins + 2


def test_histogram_object_host_arithmetic():
    """pdf integrates to 1 - (below + above + nonfinite) / count, cdf is monotone and ends there too, quantile inverts cdf."""
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(9)
    x = np.stack([rng.standard_normal(20001) ** 3, rng.random(20001) * 3 - 1.0])
    x[0, :5] = np.nan
    x[1, 7] = np.inf
    lo, hi, nbins = np.array([-2.0, -0.5]), np.array([2.5, 1.5]), 50
    raw = np.stack([np.bincount(_slots(x[f], lo[f], hi[f], nbins), minlength=nbins + 3) for f in range(2)])
    h = spectral.Histogram(x.shape[1], raw, lo, hi)
    assert h.counts.shape == (2, nbins) and h.counts.dtype == np.int64 and h.count == 20001 and h.nbins == nbins
    assert h.nonfinite.tolist() == [5, 0] and h.above[1] >= 1 and np.all(h.below >= 1)
    assert np.all(h.counts.sum(1) + h.below + h.above + h.nonfinite == h.count)
    for f in range(2):
        e, c = h.edges(f), h.centers(f)
        assert e.shape == (nbins + 1,) and e[0] == lo[f] and e[-1] == hi[f] and np.allclose(c, 0.5 * (e[1:] + e[:-1]), rtol=1e-15)
        width = (hi[f] - lo[f]) / nbins
        tails = float(h.below[f] + h.above[f] + h.nonfinite[f]) / h.count
        assert abs(float(np.sum(h.pdf(f)) * width) - (1.0 - tails)) <= 1e-12
        cdf = h.cdf(f)
        assert cdf.shape == (nbins + 1,) and np.all(np.diff(cdf) >= 0)
        assert cdf[0] == h.below[f] / h.count and abs(cdf[-1] - (h.count - h.above[f] - h.nonfinite[f]) / h.count) <= 1e-15
        q = np.linspace(cdf[0], cdf[-1], 41)[1:-1]
        xq = h.quantile(f, q)
        assert np.all(np.diff(xq) >= 0) and np.all((xq >= lo[f]) & (xq <= hi[f]))
        assert np.allclose(np.interp(xq, e, cdf), q, rtol=0, atol=1e-12)                        # quantile inverts cdf
        assert np.all(np.isnan(h.quantile(f, [cdf[0] - 1e-3, cdf[-1] + 1e-3])))
        med = float(np.median(x[f][np.isfinite(x[f])]))
        assert abs(float(h.quantile(f, 0.5)) - med) <= 2 * width
