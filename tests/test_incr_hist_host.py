"""CPU: the host arithmetic of the increment PDFs -- `spectral.incr_hist_rule`, the rule of include/mpifft4py_amd.h in numpy, against a
plain Python loop (values exactly on edges, s = 1 and s = M - 1, +-Inf and NaN), and the result class `spectral.IncrementHistogram`
(every histogram sums to the count, its second moment against S_2 of `incr_rule`, the standardised PDF)."""
import numpy as np
import pytest

import incr_hist_util as ih


def _rows(seed, nrows, M):
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal((nrows, M)) * 8) / 8          # multiples of 1/8: increments land exactly on edges


@pytest.mark.parametrize("M", [2, 5, 16, 33])
def test_rule_against_a_plain_loop(M):
    from mpifft4py_amd import spectral
    r = _rows(M, 7, M)
    seps = sorted({1, M - 1, max(1, M // 2)}) + [1]                   # the two ends, the middle and a duplicate
    for bins, lo, hi in ((16, -2.0, 2.0), (1, -0.5, 0.5), (37, -1.3, 2.9)):
        lov, hiv = np.full(len(seps), lo), np.full(len(seps), hi)
        got = spectral.incr_hist_rule(r, seps, lov, hiv, bins)
        want = ih.counts_py(r, seps, lov, hiv, bins)
        assert got.dtype == np.int64 and got.shape == (len(seps), bins + 3)
        assert np.array_equal(got, want), (M, bins, np.argwhere(got != want))
        assert np.all(got.sum(1) == r.size) and np.array_equal(got[0], got[-1])
        assert np.array_equal(got, ih.counts(r, seps, lov, hiv, bins))      # the tests' own restatement agrees
    d = ih.incr(r, 1)
    if M > 2:
        on_edge = np.mean((d * 4 == np.round(d * 4)) & (np.abs(d) < 2))
        assert on_edge > 0.2, on_edge                                 # (16 bins over +-2: edges at multiples of 1/4 -- many values sit ON them)


def test_rule_per_separation_ranges_broadcast():
    from mpifft4py_amd import spectral
    r = _rows(3, 4, 12)
    seps = [1, 11, 6]
    lo, hi = np.array([-1.0, -2.0, -0.25]), np.array([1.0, 2.5, 0.25])
    got = spectral.incr_hist_rule(r, seps, lo, hi, 9)
    assert np.array_equal(got, ih.counts_py(r, seps, lo, hi, 9))
    one = spectral.incr_hist_rule(r, seps, -1.0, 1.0, 9)
    assert np.array_equal(one[0], got[0])


def test_rule_nonfinite_values():
    """An Inf or a NaN in a row makes the two increments that touch it non-finite (Inf - x = Inf counts as above, x - Inf below,
    Inf - Inf and anything with NaN in the non-finite slot), by the histograms' slot rule."""
    from mpifft4py_amd import spectral
    r = _rows(9, 3, 10)
    r[0, 0], r[1, 4], r[2, 9], r[2, 0] = np.inf, np.nan, -np.inf, -np.inf
    seps = [1, 9, 5]
    lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    got = spectral.incr_hist_rule(r, seps, lo, hi, 8)
    want = ih.counts_py(r, seps, lo, hi, 8)
    assert np.array_equal(got, want)
    assert np.all(got.sum(1) == 30)
    # s = 1: NaN row: 2 non-finite; the -Inf, -Inf neighbours (positions 9, 0 of a periodic row): one -Inf - -Inf = NaN
    assert got[0, -1] == 3 and got[0, 0] >= 2 and got[0, -2] >= 2


def _result(seed=5, nf=2, nrows=2048, M=32, bins=256, sig=8.0):
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(seed)
    k = np.arange(M // 2 + 1)
    amp = 1.0 / np.maximum(k, 1.0)                                      # periodic rows with a falling spectrum
    x = np.fft.irfft((rng.standard_normal((nf, nrows, M // 2 + 1)) + 1j * rng.standard_normal((nf, nrows, M // 2 + 1))) * amp, n=M, axis=-1) * M
    seps = [1, 2, 4, 16, 31]
    sums = np.stack([spectral.incr_rule(x[f], seps) for f in range(nf)])
    s = np.sqrt(sums[:, :, 0] / (nrows * M))
    lo, hi = -sig * s, sig * s
    raw = np.stack([spectral.incr_hist_rule(x[f], seps, lo[f], hi[f], bins) for f in range(nf)])
    return spectral.IncrementHistogram(nrows * M, seps, raw, lo, hi, M), sums, x


def test_increment_histogram_class():
    from mpifft4py_amd import spectral
    H, sums, x = _result()
    assert H.raw.shape == (2, 5, 259) and H.raw.dtype == np.int64 and H.nbins == 256 and H.lo.shape == H.hi.shape == (2, 5)
    for i in range(5):
        h = H.hist(i)
        assert isinstance(h, spectral.Histogram) and h.count == H.count
        assert np.all(h.counts.sum(1) + h.below + h.above + h.nonfinite == H.count)
        assert np.array_equal(h.counts, H.raw[:, i, 1:-2]) and np.all(h.nonfinite == 0)
        for f in range(2):
            assert np.array_equal(H.pdf(f, i), h.pdf(f)) and np.array_equal(H.centers(f, i), h.centers(f))
    # moment(2) against S2 of incr_rule: a value moves by at most half a bin width w to its centre, so |c^2 - d^2| <= |d| w + w^2/4;
    # averaged over the points that is within w sqrt(S2) + w^2 / 4 -- and the range of +-8 sigma leaves nothing outside here
    assert np.all(H.raw[:, :, 0] == 0) and np.all(H.raw[:, :, -2] == 0)
    w = (H.hi - H.lo) / H.nbins
    S2 = sums[:, :, 0] / H.count
    m2 = H.moment(2)
    print("moment(2)", m2, "S2", S2, "half a bin width squared", (w / 2) ** 2)
    assert m2.shape == (2, 5) and np.all(np.abs(m2 - S2) <= w * np.sqrt(S2) + (w / 2) ** 2)
    # ... and to half a bin width squared: the first-order term (c - d) d averages out over a bin of a smooth density (what is left
    # is -w^2 / 12 and the sampling noise of 65536 points, w sigma / sqrt(3 count)); 256 bins over +-8 sigma: w^2 / 4 = sigma^2 / 1024
    assert np.all(np.abs(m2 - S2) <= (w / 2) ** 2), (m2 - S2, (w / 2) ** 2)
    # any real order with absolute=True; odd orders keep their sign without it
    m3, a3, a05 = H.moment(3), H.moment(3, absolute=True), H.moment(0.5, absolute=True)
    assert np.all(a3 >= np.abs(m3)) and np.all(a05 > 0) and np.all(np.isfinite(a05))
    S3, S4 = sums[:, :, 1] / H.count, sums[:, :, 2] / H.count
    # |c^3 - d^3| <= |c - d| (c^2 + |c d| + d^2) <= (w / 2) 1.5 (c^2 + d^2) per point: the means within 0.75 w (m2 + S2)
    assert np.all(np.abs(m3 - S3) <= 0.75 * w * (m2 + S2))
    # |c^4 - d^4| <= |c - d| (|c| + |d|)(c^2 + d^2) with |c| <= |d| + w / 2, evaluated on the increments themselves
    for f in range(2):
        for i, sep in enumerate(H.seps):
            d = np.abs(np.roll(x[f], -int(sep), axis=-1) - x[f])
            c = d + w[f, i] / 2
            bound = float(np.mean((w[f, i] / 2) * (c + d) * (c * c + d * d)))
            assert abs(H.moment(4)[f, i] - S4[f, i]) <= bound, (f, i, H.moment(4)[f, i], S4[f, i], bound)
    assert np.allclose(H.moment(0), 1.0, rtol=0, atol=1e-15)          # nothing outside: the counts are all there


def test_standardized_integrates_to_the_inside_share():
    H, sums, x = _result(bins=64, sig=2.0)                            # +-2 sigma: a few per cent of the increments lie outside
    for f in range(2):
        for i in range(5):
            xs, ps = H.standardized(f, i)
            inside = H.raw[f, i, 1:-2].sum() / H.count
            outside = (H.raw[f, i, 0] + H.raw[f, i, -2] + H.raw[f, i, -1]) / H.count
            assert outside > 0.01 and abs(inside + outside - 1.0) <= 1e-15
            dx = xs[1] - xs[0]
            assert abs(float(np.sum(ps) * dx) - (1.0 - outside)) <= 1e-12
            # sigma is the histogram's own: the standardised centres have unit variance under the counts
            wgt = H.raw[f, i, 1:-2] / H.raw[f, i, 1:-2].sum()
            mean = float(np.sum(wgt * xs))
            assert abs(float(np.sum(wgt * (xs - mean) ** 2)) - 1.0) <= 1e-12


def test_r_and_shapes():
    from mpifft4py_amd import spectral

    class FakeFFT(object):
        L = np.array([2 * np.pi, 2 * np.pi, 4 * np.pi])
    H = spectral.IncrementHistogram(10, [1, 5], np.zeros((3, 2, 7), dtype=np.int64), np.zeros((3, 2)), np.ones((3, 2)), 10)
    assert np.allclose(H.r(FakeFFT()), np.array([1, 5]) * 4 * np.pi / 10)
    assert H.nfields == 3 and H.nbins == 4 and H.hist(1).counts.shape == (3, 4)
    assert spectral.INCR_HIST_MAXBINS == 256
