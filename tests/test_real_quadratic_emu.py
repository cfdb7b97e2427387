"""CPU: the body of the fused z stage that ends in the statistics of a quadratic form (csrc/nlz_quad.h NlzQuad::body, Op::Quadratic)
runs in the workgroup emulator (`make emu_nlq`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and
barrier builds, whole-complex and split exchanges, with and without LDS twiddles, field counts 1, 2, 3 and 6, one row, odd row
counts and row counts of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned
`valid_in`, bin counts 0, 1 and 512, a negative weight, a NaN and an Inf in one bin of one field.  Per case (csrc/emu/test_nlq.h)
min, max and the four sums of q lie within the pointwise bound dq of the long-double rows pushed through them, every cumulative
count lies between those of q_ref + dq and q_ref - dq, the slots sum to the number of points, no slot of either partial array is
left unwritten and the inputs are preserved.  Then the entry points of the feature in the header, the binding and the library, and
the evaluation rule of q: the module's against the documented one, on values where a fused multiply-add would differ."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_quadratic", "mfft_ew_quadratic", "mfft_ew_strain_hat", "mfft_nlz_quad_rows", "mfft_nlz_quad_groups"]


def _case(l):
    m = re.match(r"nlq f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+) b(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v", "b"), (int(x) for x in m.groups()))) if m else None


def test_quadratic_body_in_the_emulator():
    r = run_group("nlq")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlq f")]
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
            assert any(" neg" in l for l in plain) and any(" neg" not in l for l in plain), (n, prec)      # a negative weight
            assert any(c["n"] == 1 for c in cases), (n, prec)                                   # one row
            assert any(c["n"] > 1 and c["n"] % 2 == 1 for c in cases), (n, prec)                # odd row counts
            # the loop over the rows iterates and ends unevenly: more than two passes of g workgroups of 2 r rows, and a rest
            assert any(c["n"] > 2 * c["g"] * 2 * c["r"] and c["n"] % (c["g"] * 2 * c["r"]) != 0 for c in cases), (n, prec)
            assert any(c["vin"] < c["v"] for c in cases), (n, prec)                             # pruned valid_in
            assert any(c["v"] == n // 3 + 1 for c in cases) and any(c["v"] == n // 2 + 1 for c in cases), (n, prec)
        cases = [_case(l) for l in mine if " in field" not in l]
        assert set(c["f"] for c in cases) == {1, 2, 3, 6}, n
        assert {0, 1, 512} <= set(c["b"] for c in cases), n                                    # no bins, one bin, the maximum
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)


def test_nonfinite_bin_in_any_field_makes_q_nan():
    """A NaN or an Inf bin in one of the fields: NaN sums, NaN minimum and maximum, at least one count in the non-finite slot and
    slots that still sum to the points: the "nan in field k" / "inf in field k" lines of the run."""
    r = run_group("nlq")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlq f") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nlq f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nlq f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def _documented_rule(r, w):
    """include/mpifft4py_amd.h, written out with Python floats (IEEE doubles, every operation rounded on its own)."""
    q = 0.0
    for rf, wf in zip(r, w):
        q = q + (float(wf) * float(rf)) * float(rf)
    return q


def test_q_rule_of_the_module_is_the_documented_one():
    from mpifft4py_amd import spectral
    # the emulator's own check of the device code's rule on the same values (csrc/emu/test_nlq.h test_nlq_rule): the contracted
    # sum ends in ..ced7, the rule's in ..ced8
    r, w = [1.1, 2.3, 0.7], [0.9, -1.7, 3.3]
    q = float.fromhex("-0x1.925e353f7ced8p+2")
    assert _documented_rule(r, w) == q
    assert spectral.quad_rule(np.array(r), np.array(w)).item() == q
    out = run_group("nlq").stdout
    assert re.search(r"nlq rule .* ok", out) and ("nlq-rule q = %s" % q.hex()) in out, out[:400]
    # hand-picked values: signs, zeros, a negative weight, sums that cancel, values that overflow, NaN and Inf
    vals = np.array([[0.0, -0.0, 1.0, -3.0, 1e-170, 1e160, 0.1, np.nan, np.inf, 1.0 / 3.0],
                     [2.0, 0.5, -1.0, 3.0, 1e-170, 1e160, 0.7, 1.0, 1.0, -2.0 / 3.0],
                     [1.5, 0.0, 1e-8, 3.0, 0.0, -1e160, 0.3, 1.0, -np.inf, 1e-3]])
    for weights in ([1.0, 1.0, 1.0], [2.0, -1.0, 0.25], [-0.1, 0.7, 1e10]):
        got = spectral.quad_rule(vals, weights)
        with np.errstate(all="ignore"):
            want = np.array([_documented_rule(vals[:, i], weights) for i in range(vals.shape[1])])
        assert np.array_equal(got, want, equal_nan=True), (weights, got, want)
        assert np.isnan(got[7]) and not np.isfinite(got[8])
    assert spectral.quad_rule(vals[:, :1], [1.0, 1.0, 1.0])[0] == 6.25
    # the order of the fields: a alone as they come, a and b pair by pair
    assert spectral.quad_slot_order(3, False) == [0, 1, 2] and spectral.quad_slot_order(6, True) == [0, 3, 1, 4, 2, 5]
    assert spectral.quad_slot_order(2, True) == [0, 1] and spectral.quad_slot_order(1, False) == [0]
