"""CPU: the bodies of the fused nonlinear z stage that also emit the real-space maxima (csrc/fft_nlz.h NlzAbsMax) run in the
workgroup emulator -- cross and dot product, every plan of MFFT_NLZPLANS_P2 / _3 / _9, both precisions, wave-synchronous and
barrier builds, whole-complex and split exchanges, with and without LDS twiddles, limited `valid`, pruned `valid_in`, odd row
counts and one row.  Per case the product rows are bit for bit those of the plain body in the same emulator, and the six
maxima agree with long-double transforms of the six rows (tolerance: the one emu_nld applies to rows, 4e-14 / 2e-5, relative
to the field's own maximum.  One deviation from that wording: in the planted-extreme cases the PARTNER of the spiked field --
noise of 1e-3 that shares one complex transform with a spike near 1 -- is taken relative to the maximum of the pair, because
the transform's rounding errors scale with the larger of its two fields; the spiked field itself, every field in turn, is held
to its own maximum).  Planted extremes: at every z position for rows of up to 64
points, else at 0, 1, TPT - 1, TPT, M/2, M - 1, in the first row and in the last row of an odd count.  Then the five entry
points of the feature in the header, the binding and the library, and advective_dt on a plan without a device.  A NaN in
one input bin: NaN for that field only, NaNs in the product rows where the plain body has them."""
import re

import numpy as np

from emu_util import assert_entry_points, nlz_lengths, run_group

NEW = ["mfft_nonlinear_cross_absmax", "mfft_nonlinear_dot_absmax", "mfft_plan_nonlinear_absmax", "mfft_nlz_rows_absmax",
       "mfft_ew_absmax"]


def test_absmax_bodies_in_the_emulator():
    r = run_group("nlm")
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlm ")]
    lengths = nlz_lengths()
    assert len(lengths) == 32
    for n in lengths:
        mine = [l for l in lines if re.search(r"N=%d\s" % n, l)]
        assert all(l.rstrip().endswith("ok") for l in mine), mine
        for prod in ("cross", "dot"):                  # each product: a NaN case and planted extremes at every length
            assert any(l.startswith("nlm %s " % prod) and " nan in field" in l for l in mine), (n, prod)
            assert any(l.startswith("nlm %s " % prod) and " spikes" in l for l in mine), (n, prod)
        for prec in ("double", "single"):
            p = [l for l in mine if prec in l]
            plain = [l for l in p if " nan in field" not in l and " spikes" not in l]
            assert len(plain) >= 3, (n, prec, plain)
            assert any(" nan in field" in l for l in p) and any(" spikes" in l for l in p), (n, prec)
            for prod in ("cross", "dot"):
                assert any(l.startswith("nlm %s " % prod) for l in plain), (n, prec, prod)
            assert any(" split" in l for l in plain) and any(" split" not in l for l in plain), (n, prec)
            assert any(" twlds" in l for l in plain) and any(" twlds" not in l for l in plain), (n, prec)
            assert any(" n1 " in l for l in plain), (n, prec)                        # one row
            assert any(re.search(r" n[3579] ", l) for l in plain), (n, prec)         # odd row counts
            vs = [tuple(int(x) for x in re.search(r" v(\d+)/(\d+)", l).groups()) for l in plain]
            assert any(vin < v for vin, v in vs), (n, prec)                           # pruned valid_in
            assert any(v == n // 3 + 1 for _, v in vs) and any(v == n // 2 + 1 for _, v in vs), (n, prec)
    assert any(" wave" in l for l in lines) and any(" wave" not in l for l in lines)
    # every z position of the short rows: N + N spikes (first and last row) per line
    for n in (12, 16, 24, 32, 48, 64):
        sp = [l for l in lines if re.search(r"N=%d\s" % n, l) and " spikes" in l]
        assert sp and all(int(re.search(r" (\d+) spikes", l).group(1)) == 2 * n for l in sp), (n, sp)


def test_nan_in_one_field_gives_nan_for_that_field_only():
    """A NaN in one input bin gives a NaN maximum for THAT field only: the "nan in field k" lines of the run.  ifft(a_f)
    and ifft(b_f) are the two halves of one complex transform, so the bodies with maxima take non-finite input values out of
    it (fft_nlz.h take_out_nonfinite) and give them back to their own field after it: the emulator asserts NaN for field k,
    the other FIVE maxima against their long-double references, and NaNs in the product rows exactly where the plain body
    has them."""
    r = run_group("nlm")
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlm ") and " nan in field" in l]
    fields = set(int(re.search(r"nan in field (\d)", l).group(1)) for l in lines)
    assert len(lines) >= 2 * 32 and min(fields) < 3 <= max(fields), (len(lines), fields)      # first-field and second-field cases
    assert r.returncode == 0 and all(l.rstrip().endswith("ok") for l in lines), r.stdout[-2000:]


def test_new_entry_points_in_header_binding_and_library():
    assert_entry_points(NEW)


def test_advective_dt_on_a_layout_plan():
    from mpifft4py_amd import LayoutComm, spectral
    from mpifft4py_amd.slab import R2C
    N = np.array([32, 64, 48], dtype=int)
    L = np.array([2 * np.pi, 4 * np.pi, 1.0])
    FFT = R2C(N, L, LayoutComm(1, 0), "double")
    umax = np.array([1.5, 0.25, 3.0])
    want = 0.5 / (1.5 * 32 / (2 * np.pi) + 0.25 * 64 / (4 * np.pi) + 3.0 * 48 / 1.0)
    got = spectral.advective_dt(FFT, umax, 0.5)
    assert abs(got - want) <= 1e-15 * want, (got, want)
    assert spectral.advective_dt(FFT, [0.0, 0.0, 0.0], 0.5) == float("inf")          # a field at rest
    assert spectral.advective_dt(FFT, [0.0, 2.0, 0.0], 1.0) == 1.0 / (2.0 * 64 / (4 * np.pi))
    assert np.isnan(spectral.advective_dt(FFT, [1.0, np.nan, 0.0], 0.5))
    assert spectral.advective_dt(FFT, [1.0, 0.0, np.inf], 0.5) == 0.0
