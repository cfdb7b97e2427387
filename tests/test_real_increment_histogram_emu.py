"""CPU: the body of the fused z stage that ends in increment histograms (csrc/nlz_incr_hist.h NlzIncrHist::body, Op::IncrementHistogram) runs
in the workgroup emulator (`make emu_nlk`): every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and barrier
builds, whole-complex and split exchanges, with and without LDS twiddles, field counts 1, 2, 3 and 6, one row, odd row counts and
row counts of several passes of the launch's workgroups plus a ragged rest, `valid` = n/2+1 and n/3+1, pruned `valid_in`, bin counts
1, 37, 64 and 256, a NaN and an Inf in one bin of one field; eight separations: 1, a multiple of the threads' stride, an odd one near
the middle, n/2, n-1, a duplicate and two more.  Per case every (field, separation) sums to the points, its cumulative counts lie
between those of the long-double rows' increments shifted by -+2 delta through the same slot rule (csrc/emu/test_nlk.h), the
duplicate repeats its twin and a non-finite bin marks its own field only.  Then the entry points of the feature in the header, the
binding and the library, and that the limits are one number everywhere."""
import os
import re

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_real_increment_histogram", "mfft_ew_increment_histogram", "mfft_nlz_incr_hist_rows", "mfft_nlz_incr_hist_groups"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(l):
    m = re.match(r"nlk f(\d) r(\d+) n(\d+) g(\d+) v(\d+)/(\d+) b(\d+)", l)
    return dict(zip(("f", "r", "n", "g", "vin", "v", "b"), (int(x) for x in m.groups()))) if m else None


def test_increment_histogram_body_in_the_emulator():
    r = run_group("nlk")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlk ")]
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
            assert any(" split" in l for l in plain) and any(" split" not in l for l in plain), (n, prec)         # both exchanges
            assert any(" twlds" in l for l in plain) and any(" twlds" not in l for l in plain), (n, prec)
            assert any(c["n"] == 1 for c in cases), (n, prec)                                   # one row
            assert any(c["n"] > 1 and c["n"] % 2 == 1 for c in cases), (n, prec)                # odd row counts
            # the loop over the rows iterates and ends unevenly: more than two passes of g workgroups of 2 r rows, and a rest
            assert any(c["n"] > 2 * c["g"] * 2 * c["r"] and c["n"] % (c["g"] * 2 * c["r"]) != 0 for c in cases), (n, prec)
            assert any(c["vin"] < c["v"] for c in cases), (n, prec)                             # pruned valid_in
            assert any(c["v"] == n // 3 + 1 for c in cases) and any(c["v"] == n // 2 + 1 for c in cases), (n, prec)
        every = [_case(l) for l in mine if " in field" not in l]
        assert set(c["f"] for c in every) == {1, 2, 3, 6}, n
        assert {1, 256} <= set(c["b"] for c in every), n                                        # the two ends of the bin counts
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)             # a wave build among the cases


def test_nonfinite_bin_marks_its_field_only():
    """A NaN or Inf bin of one field: its non-finite slot is met and every (field, separation) still sums to the points; the other
    fields -- the partner on the same complex transform among them -- have the counts of the run without it, exactly: the "nan in
    field k" / "inf in field k" lines of the run."""
    r = run_group("nlk")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlk ") and " in field" in l]
    assert len(lines) >= 3 * 32, len(lines)
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]
    assert any(re.match(r"nlk f6 .* in field [0-2]", l) for l in lines) and any(re.match(r"nlk f6 .* in field [3-5]", l) for l in lines)


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def test_limits_are_one_number():
    from mpifft4py_amd import spectral
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    kernel = open(os.path.join(ROOT, "mpifft4py_amd", "csrc", "nlz_incr_hist.h")).read()
    h = int(re.search(r"#define MFFT_INCR_HIST_MAXBINS (\d+)", header).group(1))
    k = int(re.search(r"NLK_MAXBINS = (\d+)", kernel).group(1))
    assert h == k == spectral.INCR_HIST_MAXBINS == 256
    assert int(re.search(r"#define MFFT_INCR_MAXSEP (\d+)", header).group(1)) == spectral.INCR_MAXSEP == 8
    # a pair's histograms fit under the joint grid, whose exchange rule the kernels take
    cells = 2 * 8 * (k + 3)
    joint = int(re.search(r"NLJ_MAXBINS = (\d+)", open(os.path.join(ROOT, "mpifft4py_amd", "csrc", "nlz_joint.h")).read()).group(1))
    assert cells == 4144 and cells <= (joint + 3) ** 2
