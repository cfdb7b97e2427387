"""CPU: the body of the fused z stage that ends in a reduction (csrc/nlz_moments.h NlzMoments::body, Op::Moments) runs in the workgroup
emulator (`make emu_nls`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier builds,
whole-complex and split exchanges, with and without LDS twiddles, field counts 1, 2, 3 and 6, one row, odd row counts and row
counts of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, a non-zero
centre, a NaN and an Inf in one bin of one field.  Per case min, max and the four power sums of every field agree with
long-double transforms of the rows: extremes within tol * max|x|, S_p within tol * p * sqrt(sum d^(2(p-1)) * sum x^2) +
(count + 8) * 2^-52 * sum |d|^p (d = x - centre; tol = 4e-14 / 2e-5, the tolerance emu_nld applies to rows).  Then the entry
points of the feature in the header, the binding and the library, and the host arithmetic of `spectral.Moments`."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_moments", "mfft_ew_moments", "mfft_nlz_moments_rows", "mfft_nlz_moments_groups", "mfft_ew_diag_grad_hat"]


def _case(l):
    m = re.match(r"nls f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v"), (int(x) for x in m.groups()))) if m else None


def test_moments_body_in_the_emulator():
    r = run_group("nls")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nls ")]
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
            assert any(" centre" in l for l in plain) and any(" centre" not in l for l in plain), (n, prec)
            assert any(c["n"] == 1 for c in cases), (n, prec)                                   # one row
            assert any(c["n"] > 1 and c["n"] % 2 == 1 for c in cases), (n, prec)                # odd row counts
            # the loop over the rows iterates and ends unevenly: more than two passes of g workgroups of 2 r rows, and a rest
            assert any(c["n"] > 2 * c["g"] * 2 * c["r"] and c["n"] % (c["g"] * 2 * c["r"]) != 0 for c in cases), (n, prec)
            assert any(c["vin"] < c["v"] for c in cases), (n, prec)                             # pruned valid_in
            assert any(c["v"] == n // 3 + 1 for c in cases) and any(c["v"] == n // 2 + 1 for c in cases), (n, prec)
        assert set(c["f"] for c in (_case(l) for l in mine if " in field" not in l)) == {1, 2, 3, 6}, n
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_marks_its_field_only():
    """A NaN bin of one field: NaN in all six of its statistics; an Inf bin: NaN sums, extremes -Inf / +Inf or NaN.  The other
    fields -- the partner on the same complex transform among them -- against their long-double references as before
    (fft_nlz.h take_out_nonfinite): the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nls")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nls ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    # fields with a partner on their transform and both halves of a pair are met
    assert any(re.match(r"nls f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nls f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def test_moments_object_host_arithmetic():
    """mean, variance, skewness and flatness from raw sums about a centre are those about the mean, whatever the centre."""
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(5)
    x = np.stack([rng.standard_normal(4001) ** 3 + 2.0, rng.random(4001) - 7.0]).astype(np.longdouble)
    want_mean = x.mean(1)
    d = x - want_mean[:, None]
    mu = [np.mean(d ** p, axis=1) for p in (2, 3, 4)]
    for center in ([0.0, 0.0], [2.0, -6.5], [100.0, 3.0]):
        c = np.asarray(center, dtype=np.float64)
        e = x - c.astype(np.longdouble)[:, None]
        sums = np.stack([np.sum(e ** p, axis=1) for p in (1, 2, 3, 4)], axis=1).astype(np.float64)
        m = spectral.Moments(x.shape[1], x.min(1), x.max(1), sums, c)
        loss = float(np.max(np.abs(c - want_mean.astype(np.float64)) / np.sqrt(mu[0].astype(np.float64)))) + 1.0
        tol = 64 * 2.0 ** -52 * loss ** 4               # the raw sums are rounded to double: digits go as (|mean - c| / sigma)^p
        assert m.count == 4001 and m.sums.shape == (2, 4) and m.min.shape == m.max.shape == (2,)
        assert np.all(np.abs(m.mean() - want_mean) <= tol * np.abs(want_mean))
        assert np.all(np.abs(m.variance() - mu[0]) <= tol * mu[0])
        assert np.all(np.abs(m.skewness() - mu[1] / mu[0] ** 1.5) <= tol * 10)
        assert np.all(np.abs(m.flatness() - mu[2] / mu[0] ** 2) <= tol * 30)
