"""CPU: the body of the fused z stage that ends in structure functions (csrc/nlz_incr.h NlzIncr::body, Op::Increments) runs in the
workgroup emulator (`make emu_nli`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier
builds, whole-complex and split exchanges, with and without LDS twiddles, field counts 1, 2, 3 and 6, one row, odd row counts and
row counts of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, a NaN
and an Inf in one bin of one field; separations 1, a multiple of the threads' stride, an odd one near the middle, n/2, n-1 and a
duplicate.  Per case the sums S2, S3, S4 of every field and separation agree with long-double rows within
2 * tol * p * sqrt(sum d^(2(p-1)) * sum x^2) + (count + 8) * 2^-52 * sum |d|^p (tol = 4e-14 / 2e-5, the tolerance of the moments).
Then the entry points of the feature in the header, the binding and the library, and the host arithmetic of
`spectral.Increments`."""
import re

import numpy as np
import pytest

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_increments", "mfft_ew_increments", "mfft_nlz_incr_rows", "mfft_nlz_incr_groups"]


def _case(l):
    m = re.match(r"nli f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v"), (int(x) for x in m.groups()))) if m else None


def test_increments_body_in_the_emulator():
    r = run_group("nli")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nli ")]
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
        assert set(c["f"] for c in (_case(l) for l in mine if " in field" not in l)) == {1, 2, 3, 6}, n
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_marks_its_field_only():
    """A NaN or Inf bin of one field: NaN in all of its sums; the other fields -- the partner on the same complex transform among
    them -- against their long-double references as before: the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nli")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nli ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nli f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nli f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def test_maxsep_is_one_number():
    from mpifft4py_amd import spectral
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mpifft4py_amd.h")).read()
    kernel = open(os.path.join(root, "mpifft4py_amd", "csrc", "nlz_incr.h")).read()
    h = int(re.search(r"#define MFFT_INCR_MAXSEP (\d+)", header).group(1))
    k = int(re.search(r"NLI_MAXSEP = (\d+)", kernel).group(1))
    assert h == k == spectral.INCR_MAXSEP and h >= 8


def test_default_separations():
    from mpifft4py_amd import spectral
    assert spectral.default_seps(32) == [1, 2, 4, 8, 16]
    assert spectral.default_seps(48) == [1, 2, 4, 8, 16, 24]
    assert spectral.default_seps(12) == [1, 2, 4, 6]
    assert spectral.default_seps(2) == [1]
    assert spectral.default_seps(11) == [1, 2, 4, 5]
    for M in range(2, 200):
        s = spectral.default_seps(M)
        assert s and all(1 <= x <= M - 1 for x in s) and s == sorted(set(s)), (M, s)


def test_increments_object_host_arithmetic():
    """S(p), skewness, flatness and r from raw sums are those of the rows' increments, and the rule in numpy is np.roll's."""
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 5, 7, 24)) ** 3
    seps = [1, 5, 12, 23, 1]
    sums = np.stack([spectral.incr_rule(x[f], seps) for f in range(2)])
    inc = spectral.Increments(5 * 7 * 24, seps, sums, 24)
    assert inc.count == 840 and inc.sums.shape == (2, 5, 3) and list(inc.seps) == seps
    xl = x.astype(np.longdouble)
    for i, s in enumerate(seps):
        d = np.roll(xl, -s, axis=-1) - xl
        mu = [np.mean(d ** p, axis=(1, 2, 3)) for p in (2, 3, 4)]
        scale = [np.mean(np.abs(d) ** p, axis=(1, 2, 3)) for p in (2, 3, 4)]
        for p in (2, 3, 4):
            assert np.all(np.abs(inc.S(p)[:, i] - mu[p - 2]) <= 900 * 2.0 ** -52 * scale[p - 2]), (s, p)
        assert np.all(np.abs(inc.skewness()[:, i] - mu[1] / mu[0] ** 1.5) <= 1e-11)
        assert np.all(np.abs(inc.flatness()[:, i] - mu[2] / mu[0] ** 2) <= 1e-11)
    assert np.array_equal(inc.sums[:, 0], inc.sums[:, 4])          # a duplicate separation: the same bits
    # periodic rows: the sums at s and M - s are the same but for the sign of the odd one
    a, b = spectral.incr_rule(x[0], [5])[0], spectral.incr_rule(x[0], [19])[0]
    assert abs(a[0] - b[0]) <= 1e-12 * a[0] and abs(a[1] + b[1]) <= 1e-12 * a[2] ** 0.75 * 840 ** 0.25 + 1e-9 and abs(a[2] - b[2]) <= 1e-12 * a[2]

    class F(object):
        L = np.array([2 * np.pi, 2 * np.pi, 4 * np.pi])
    assert np.allclose(inc.r(F), np.asarray(seps) * 4 * np.pi / 24, rtol=1e-15)
    with pytest.raises(ValueError):
        inc.S(1)
    with pytest.raises(ValueError):
        inc.S(5)
