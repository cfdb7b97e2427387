"""CPU: the outer-product bodies of the fused nonlinear z stage (csrc/fft_nlz.h NlzFft::body_outer) run in the workgroup emulator
against long-double DFTs of irfft(a_i) irfft(b_j), all nine -- every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions,
wave-synchronous and barrier builds, whole-complex and split exchanges, with and without LDS twiddles, limited `valid`, pruned
`valid_in`, out of place and in place over the six inputs, an odd row count, and an odd row count in place with NaNs behind the
last row -- and the entry points of the operation are in the header, the binding and the library."""
import re

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_nonlinear_outer", "mfft_nlz_outer_rows", "mfft_ew_elsasser_rhs", "mfft_ew_mul"]


def test_outer_bodies_in_the_emulator():
    r = run_group("nlo")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlo ")]
    lengths = nlz_lengths()
    assert len(lengths) == 32
    for n in lengths:
        mine = [l for l in lines if re.search(r"N=%d\s" % n, l)]
        assert len(mine) >= 12, (n, mine)
        assert all(l.rstrip().endswith("ok") for l in mine), mine
        for prec in ("double", "single"):
            p = [l for l in mine if prec in l]
            assert any(" split" in l for l in p) and any(" split" not in l for l in p), (n, prec)
            assert any(" twlds" in l for l in p) and any(" twlds" not in l for l in p), (n, prec)
            assert any(" inpl" in l for l in p) and any(" inpl" not in l for l in p), (n, prec)
            assert any(" poison" in l for l in p), (n, prec)      # in place, NaNs behind the odd last row


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)
