"""CPU: the body of the fused z stage that ends in plane-averaged PROFILES (csrc/nlz_prof.h NlzProf::body, Op::Profiles) runs in the
workgroup emulator (`make emu_nlp`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier
builds, whole-complex and split exchanges, with and without LDS twiddles, 2 and 6 fields, one row, odd row counts and row counts
of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, a NaN and an Inf
in one bin of one field.  Per case (csrc/emu/test_nlp.h): the five sums of every pair at every position of the row against
long-double rows within the per-plane bound of the moments, no slot of the partial profiles left unwritten, the inputs
preserved; a bad bin makes its own field's sums and the cross sum NaN and leaves every other sum the bytes of the run without it.
Then the entry points of the feature in the header, the binding and the library, the rule of the module and the host arithmetic
of `spectral.Profiles`."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_profiles", "mfft_ew_profiles", "mfft_nlz_profile_rows", "mfft_nlz_profile_groups"]


def _case(l):
    m = re.match(r"nlp f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v"), (int(x) for x in m.groups()))) if m else None


def test_profile_body_in_the_emulator():
    r = run_group("nlp")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlp ")]
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
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_marks_its_field_only():
    """A NaN or an Inf bin of one field: NaNs in ITS two sums and in the cross sum; the partner's two sums and every other pair
    have EXACTLY the bytes of the run with that bin taken out: the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nlp")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlp ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nlp f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nlp f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def test_profile_rule_of_the_module_is_the_documented_one():
    """spectral.profile_rule against a direct long-double evaluation: within (R + 8) 2^-52 of the sums of absolute values."""
    from mpifft4py_amd import spectral
    assert spectral.PROFILE_STATS == 5
    rng = np.random.default_rng(5)
    R, M = 37, 19
    x = rng.standard_normal((R, M)) + 3.0
    y = rng.standard_normal((R, M)) * 0.01 - 2.0
    eps = 2.0 ** -52
    for center in (None, (3.0, -2.0), (0.5, 7.25)):
        got = spectral.profile_rule(x.reshape(1, R, M), y.reshape(1, R, M), center)
        assert got.shape == (5, M) and got.dtype == np.float64
        ca, cb = (0.0, 0.0) if center is None else center
        # (the subtraction of the centre is ONE rounded operation of the rule: the reference starts from the same doubles)
        dx, dy = (x - ca).astype(np.longdouble), (y - cb).astype(np.longdouble)
        terms = [dx, dy, dx * dx, dy * dy, dx * dy]
        for k in range(5):
            want, mag = terms[k].sum(axis=0), np.abs(terms[k]).sum(axis=0)
            err = np.abs(got[k].astype(np.longdouble) - want)
            print("rule center=%r sum %d: worst err / bound = %.3g" % (center, k, float((err / ((R + 8) * eps * mag)).max())))
            assert np.all(err <= (R + 8) * eps * mag), (center, k)


def test_profiles_object_host_arithmetic():
    """mean, variance, covariance, correlation and flux of a constructed sample against numpy on the same sample; a constant
    plane has no correlation (nan); `finite` marks the field whose sums are not finite and nothing else."""
    from mpifft4py_amd import spectral
    rng = np.random.default_rng(23)
    R, M = 4001, 6
    x = rng.standard_normal((2, R, M)) * np.linspace(0.5, 2.0, M) + np.linspace(-1.0, 1.0, M)
    y = 0.75 * x + 0.5 * rng.standard_normal((2, R, M)) + 4.0
    x[1, :, 2] = 1.25                                  # a constant plane of pair 1's first field
    center = np.array([[0.1, 4.0], [1.25, 3.5]])
    sums = np.stack([spectral.profile_rule(x[p], y[p], center[p]) for p in range(2)])
    h = spectral.Profiles(R, sums, center)
    assert h.count == R and h.M == M and h.sums.shape == (2, 5, M) and h.center.shape == (2, 2)
    for p in range(2):
        mean, var, cov, flux = h.mean(p), h.variance(p), h.covariance(p), h.flux(p)
        assert mean.shape == (2, M) and var.shape == (2, M) and cov.shape == (M,) and flux.shape == (M,)
        assert np.allclose(np.asarray(mean, dtype=np.float64), [x[p].mean(axis=0), y[p].mean(axis=0)], rtol=0, atol=1e-12)
        assert np.allclose(np.asarray(var, dtype=np.float64), [x[p].var(axis=0), y[p].var(axis=0)], rtol=1e-10, atol=1e-12)
        want_cov = ((x[p] - x[p].mean(axis=0)) * (y[p] - y[p].mean(axis=0))).mean(axis=0)
        assert np.allclose(np.asarray(cov, dtype=np.float64), want_cov, rtol=1e-10, atol=1e-12)
        assert np.allclose(np.asarray(flux, dtype=np.float64), (x[p] * y[p]).mean(axis=0), rtol=1e-11, atol=1e-12)
        corr = np.asarray(h.correlation(p), dtype=np.float64)
        for m in range(M):
            if p == 1 and m == 2:
                assert np.isnan(corr[m])               # the constant plane: its variance is 0
            else:
                assert abs(corr[m] - np.corrcoef(x[p, :, m], y[p, :, m])[0, 1]) <= 1e-10, (p, m)
    assert h.finite.shape == (2, 2) and h.finite.all()
    assert np.array_equal(h.z(type("F", (), {"L": (1.0, 1.0, 3.0)})()), np.arange(M) * 3.0 / M)
    bad = sums.copy()
    bad[1, 1, 3] = np.nan                              # sum d_y of pair 1: its second field
    assert spectral.Profiles(R, bad, center).finite.tolist() == [[True, True], [True, False]]
    bad = sums.copy()
    bad[0, 2, 0] = np.inf                              # sum d_x^2 of pair 0: its first field
    assert spectral.Profiles(R, bad, center).finite.tolist() == [[False, True], [True, True]]
