"""GPU: PDFs of the increments along z of spectral fields without the real-space arrays (mfft_real_increment_histogram,
mfft_nlz_incr_hist_rows, mfft_ew_increment_histogram; csrc/nlz_incr_hist.h NlzIncrHist::body, csrc/incrhist.hip) -- the sweep against numpy
exactly, the z stage on known answers exactly and on random spectra by brackets, its consistency with mfft_nlz_incr_rows, non-finite
bins and every error code, the plan operation on every route (fused on one rank and several, chunks, composed, pencils, pitched),
`range=None`, the Taylor-Green known answer and the example's --structure-pdf.

Counts have no tolerance.  Where the values come from a transform they are compared by BRACKETS on the increments with 2 delta
(tests/incr_hist_util.py explains the method and states the 1 % cap, which is asserted from the numpy reference alone).  delta is
the histogram tests' worst-case bound: per transform 8 eps_T log2(n) sum_k h_k (|A_k| + |B_k|) / n over BOTH fields of a pair."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import incr_hist_util as ih
import nonlinear_util as nl
from gpu_util import L, cdtype, have_gpu, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
MAXBINS, MAXSEP = 256, 8
POISON = -7


def INFO(dealias):
    return "nonlinear_incr_hist_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _ranges(fields, seps, k=4.0):
    """+-k sigma of every field's increments at every separation, from the reference: (nfields, nsep) lo and hi."""
    sg = np.array([[float(np.sqrt(np.mean(ih.incr(x, s) ** 2))) for s in seps] for x in fields])
    sg[~(sg > 0)] = 0.5 / k
    return -k * sg, k * sg


# ---- 1. the sweep: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15)])
def test_sweep_equals_numpy(shape, prec):
    """spectral.increment_histogram of real arrays whose values are multiples of 1/8 -- so that increments sit exactly ON edges --
    with +-Inf and NaN among them EQUALS numpy evaluating the rule in float64; separations 1, M - 1 and a duplicate; then one range
    per (component, separation) with an odd bin count, a list of more than eight separations, and a pitched array with NaNs
    between its rows."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(7 + shape[0])
    x = (np.round(3.0 * rng.standard_normal(shape) * 8) / 8).astype(rdtype(prec))
    M = shape[-1]
    flat = x.reshape(shape[0], -1)
    n = flat.shape[1]
    for c in range(shape[0]):
        special = [np.inf, -np.inf, np.nan, np.nan, 4.0, -4.0]
        where = rng.choice(n, len(special), replace=False)
        where[:3] = [0, n - 1, n // 2]               # the first, the last and a middle element among them
        flat[c, where] = special
    seps = [1, M - 1, M // 2, 1]
    lo, hi, nbins = -4.0, 4.0, 64                    # edges at multiples of 1/8: exact in both precisions
    want = np.stack([ih.counts(x[c], seps, [lo] * 4, [hi] * 4, nbins) for c in range(shape[0])])
    h = spectral.increment_histogram(F, DeviceArray.from_numpy(x), seps=seps, bins=nbins, range=(lo, hi))
    on_edge = float(np.mean(ih.incr(x, 1) * 8 == np.round(ih.incr(x, 1) * 8)))
    print("sweep %s %s: on an edge %.3f, below %s above %s nonfinite %s" % (shape, prec, on_edge, h.raw[:, 0, 0], h.raw[:, 0, -2], h.raw[:, 0, -1]))
    assert h.count == n and h.raw.dtype == np.int64 and h.raw.shape == (shape[0], 4, nbins + 3) and list(h.seps) == seps
    assert np.array_equal(h.raw, want), np.argwhere(h.raw != want)[:8]
    assert np.all(h.raw[:, :, -1] >= 2) and np.all(h.raw.sum(2) == n) and on_edge > 0.9
    assert np.array_equal(h.raw[:, 0], h.raw[:, 3])                                   # the duplicate
    assert np.array_equal(h.raw, np.stack([spectral.incr_hist_rule(x[c], seps, lo, hi, nbins) for c in range(shape[0])]))
    # one range per (component, separation), an odd bin count, eleven separations (two sweeps)
    seps = [1, M - 1, 2, 3, 5, 7, M // 2, 1, M - 2, 4, 6]
    r = np.array([[(-1.0 - 0.1 * c - 0.05 * i, 2.0 + 0.3 * c + 0.07 * i) for i in range(len(seps))] for c in range(shape[0])])
    h = spectral.increment_histogram(F, DeviceArray.from_numpy(x), seps=seps, bins=37, range=r)
    want = np.stack([ih.counts(x[c], seps, r[c, :, 0], r[c, :, 1], 37) for c in range(shape[0])])
    assert h.raw.shape == (shape[0], 11, 40) and np.array_equal(h.raw, want), np.argwhere(h.raw != want)[:8]
    # a pitched array is swept as it lies: NaNs between the rows
    whole = np.full(shape[:-1] + (M + 5,), np.nan, dtype=rdtype(prec))
    whole[..., :M] = x
    dw = DeviceArray.from_numpy(whole)
    pitched = DeviceArray(x.shape, x.dtype, ptr=dw.ptr, owner=False, pitch=M + 5)
    hp = spectral.increment_histogram(F, pitched, seps=seps, bins=37, range=r)
    assert np.array_equal(hp.raw, want)


@pytest.mark.parametrize("prec", ["double", "single"])
def test_sweep_every_path_of_the_kernel(prec):
    """Rows of 2 points; 255, 256 and 257 (several rows per pass of a workgroup / one); the longest row that is staged in LDS and the
    first that is not (49152 bytes); more rows than one pass of the grid; six components."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    staged = 49152 // np.dtype(rdtype(prec)).itemsize
    rng = np.random.default_rng(11)
    # (four axes: the first counts the components)
    for shape in [(1, 1, 33, 2), (2, 1, 5, 255), (2, 1, 5, 256), (2, 1, 5, 257), (1, 1, 3, staged), (1, 1, 3, staged + 1), (6, 1, 4100, 3),
                  (1, 3, 2049, 85)]:
        x = (np.round(rng.standard_normal(shape) * 16) / 16).astype(rdtype(prec))
        M = shape[-1]
        seps = [1] if M == 2 else [1, M - 1, M // 2, 2]
        h = spectral.increment_histogram(F, DeviceArray.from_numpy(x), seps=seps, bins=48, range=(-3.0, 3.0))
        want = np.stack([ih.counts(x[c], seps, [-3.0] * len(seps), [3.0] * len(seps), 48) for c in range(shape[0])])
        assert np.array_equal(h.raw, want), (shape, np.argwhere(h.raw != want)[:8])


# ---- the stage alone --------------------------------------------------------------------------------------------------
#   12    the shortest plan (12 values per thread, one thread per row)   16    two threads per row, 32 rows per wave
#   144   a 9 * 2^a plan                                                 768   a 12-values plan; in double precision nlj_split halves
#   1024  128 threads per row: two waves per row, a barrier build              its exchange: a barrier build with two rounds per pair
#   1536  128 threads per row with 12 values: the z row of 1024 under the 3/2-rule
#   2048  double: the split exchange chosen by nlj_split                 4096  double: the histogram twin's exchange is kept
def _irfft_rows(x, n, vin):
    x = x[..., :vin].astype(np.complex128)
    x[..., 0] = x[..., 0].real
    if vin == n // 2 + 1 and n % 2 == 0:
        x[..., -1] = x[..., -1].real
    return np.fft.irfft(x, n=n, axis=-1)


def _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, seps, lo, hi, nbins):
    from mpifft4py_amd import DeviceArray, _lib
    da = DeviceArray.from_numpy(a)
    db = DeviceArray.from_numpy(b) if b is not None else None
    got = np.full((nfields, len(seps), nbins + 3), POISON, dtype=np.int64)
    sv = np.ascontiguousarray(seps, dtype=np.int64)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (nfields, len(seps))))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (nfields, len(seps))))
    _lib.call("mfft_nlz_incr_hist_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, valid_in,
              _lib.precision_code(prec), sv.ctypes.data_as(IP), len(seps), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins,
              got.ctypes.data_as(IP))
    assert da.get().tobytes() == a.tobytes() and (b is None or db.get().tobytes() == b.tobytes())      # inputs preserved
    assert not np.any(got == POISON)
    return got


KNOWN_SEPS = lambda n: [1, 2, 3, 4, n // 2, n - 1, 1, n - 2]


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [12, 16, 144, 768, 1024, 1536])
def test_stage_known_answers_exact(n, prec):
    """Three fields whose real rows are known without a transform: the constant 2 (every increment 0), 1 + 2 (-1)^j (bins 0 and
    n / 2: increments 0 and -+4) and the single cosine mode n / 4, 3 cos(pi j / 2) = {3, 0, -3, 0} (increments in {0, +-3, +-6}).
    Thirteen bins of width 1 over [-6.5, 6.5): every increment sits half a bin from every edge, so the counts are exact; they are
    written down from the integer rows, not from a transform."""
    nrows, valid, nbins = 5, n // 2 + 1, 13
    a = np.zeros((3, nrows, valid + 3), dtype=cdtype(prec))
    a[0, :, 0] = 2.0 * n
    a[1, :, 0] = 1.0 * n
    a[1, :, n // 2] = 2.0 * n
    a[2, :, n // 4] = 1.5 * n
    j = np.arange(n)
    rows = [np.full(n, 2.0), 1.0 + 2.0 * (-1.0) ** j, np.array([3.0, 0.0, -3.0, 0.0])[j % 4]]
    seps = KNOWN_SEPS(n)
    got = _rows_call(a, None, 3, nrows, n, valid + 3, valid, 0, prec, seps, -6.5, 6.5, nbins)
    want = np.stack([nrows * ih.counts(r, seps, [-6.5] * 8, [6.5] * 8, nbins) for r in rows])
    print("known answers n=%d %s:\n%s" % (n, prec, got[2]))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    slot = lambda v: 1 + int(v + 6.5)
    assert got[0, :, slot(0)].tolist() == [nrows * n] * 8
    assert got[1, 0, slot(4)] == got[1, 0, slot(-4)] == nrows * n // 2 and got[1, 1, slot(0)] == nrows * n
    assert got[2, 0, slot(3)] == got[2, 0, slot(-3)] == nrows * n // 2                 # s = 1: {-3, -3, 3, 3}
    assert got[2, 1, slot(6)] == got[2, 1, slot(-6)] == nrows * n // 4 and got[2, 1, slot(0)] == nrows * n // 2      # s = 2: {-6, 0, 6, 0}
    assert got[2, 3, slot(0)] == nrows * n                                             # s = 4: a whole period
    assert np.allclose(np.stack(rows), _irfft_rows(a, n, valid)[:, 0], atol=1e-12)     # (the spectra are those rows)


def _spectra(rng, shape, n, valid, prec):
    z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
    z[..., 0] = z[..., 0].real
    if n % 2 == 0 and valid == n // 2 + 1:
        z[..., valid - 1] = z[..., valid - 1].real
    return z


def _stage_case(n, prec, nfields, nrows, valid, valid_in, seps, nbins):
    """(a, b, fields, deltas, lo, hi) of a stage case from the seed alone: Gaussian spectra with real end bins, every (field,
    separation) over +-4 sigma of the reference increments."""
    rng = np.random.default_rng(100 * n + 7 * nrows % 1000 + valid + nfields + 31 * len(seps) + nbins)
    pitch = valid + 3
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = (ncomp, nrows, pitch)
    a = _spectra(rng, shape, n, valid, prec)
    b = _spectra(rng, shape, n, valid, prec) if nfields % 2 == 0 else None
    vin = valid_in or valid
    fields = [r for x in (a, b) if x is not None for r in _irfft_rows(x, n, vin)]
    dl = [r for x in (a, b) if x is not None for r in ih.delta_rows(x, n, vin, prec)]
    deltas = []
    for f in range(nfields):
        # the partner on the transform: b_f for a_f where there are two arrays; among a's components the next / previous one
        g = (f + ncomp) % nfields if b is not None else (f ^ 1 if (f ^ 1) < nfields else None)
        deltas.append((dl[f] + (dl[g] if g is not None else 0.0))[:, None])
    lo, hi = _ranges(fields, seps)
    return a, b, fields, deltas, lo, hi


def _stage_random(n, prec, nfields, nrows, valid, valid_in=0, seps=None, nbins=64):
    seps = _stage_seps(n) if seps is None else seps
    a, b, fields, deltas, lo, hi = _stage_case(n, prec, nfields, nrows, valid, valid_in, seps, nbins)
    flat = lambda x: x if nfields > 2 else x[0]
    got = _rows_call(flat(a), flat(b) if b is not None else None, nfields, nrows, n, valid + 3, valid, valid_in, prec, seps, lo, hi, nbins)
    for f in range(nfields):
        for i, s in enumerate(seps):
            ih.bracket(got[f, i], fields[f], deltas[f], s, lo[f, i], hi[f, i], nbins,
                       "stage n=%d %s nfields=%d nrows=%d valid=%d/%d bins=%d field %d" % (n, prec, nfields, nrows, valid_in or valid, valid, nbins, f))
    if len(seps) > 5 and seps[5] == seps[0]:
        assert np.array_equal(got[:, 0], got[:, 5])                                    # the duplicate separation (same range)
    return got


def _stage_seps(n):
    """1, a multiple of every thread stride of the plans (16 where the row has it), an odd value near the middle, n / 2, n - 1, a
    duplicate, and two more short ones: eight."""
    return [1, min(16, n - 2), (n // 2 - 1) | 1, n // 2, n - 1, 1, 2, 3]


STAGE = [(n, p) for n in (12, 16, 144, 768, 1536) for p in ("double", "single")] + [(4096, "double"), (2048, "double")]


@pytest.mark.parametrize("n,prec", STAGE)
def test_stage_random_spectra_bracket(n, prec):
    """6, 3, 2 and 1 fields (the odd counts exercise the pair without a partner); eight separations and one; the n/2 + 1 bins, the
    n/3 + 1 of the 3/2-rule and pruned valid_in; 37 rows (odd) and one; 64 bins, 1 and -- in double precision, where 2 delta is far
    below a bin of 8 sigma / 256 -- 256; a second call gives identical arrays."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage_random(n, prec, 6, 37, full)
    assert np.array_equal(_stage_random(n, prec, 6, 37, full), first)
    _stage_random(n, prec, 3, 37, lim, nbins=256 if prec == "double" else 64)
    _stage_random(n, prec, 2, 37, full, valid_in=lim, seps=[n // 2])
    _stage_random(n, prec, 1, 37, full, nbins=1)
    if n > 16:                                       # (one row of 16 points has no 64-bin PDF to bracket: the odd count covers 16)
        _stage_random(n, prec, 1, 1, full, seps=[1, n - 1])
    else:
        _stage_random(n, prec, 1, 1, full, seps=[1, n - 1], nbins=4)


@pytest.mark.parametrize("prec", ["double", "single"])
def test_stage_more_than_two_passes_of_the_grid(prec):
    """n = 16: more than two passes of mfft_nlz_incr_hist_groups workgroups and a ragged rest: every workgroup strides, the last pass
    is partial."""
    from mpifft4py_amd import _lib
    code = _lib.precision_code(prec)
    cap = _lib.call("mfft_nlz_incr_hist_groups", 1 << 40, 16, code)
    per = 1
    while _lib.call("mfft_nlz_incr_hist_groups", per + 1, 16, code) == 1:      # rows per workgroup: a power of two
        per *= 2
    assert cap >= 1
    nrows = 2 * cap * per + per // 2 + 3
    assert _lib.call("mfft_nlz_incr_hist_groups", nrows, 16, code) == cap
    _stage_random(16, prec, 1, nrows, 9, seps=[1, 8])


# ---- 4. consistency with the increment sums on the same rows ------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", [16, 768, 1024])
def test_stage_consistent_with_incr_rows(n, prec):
    """The same rows through mfft_nlz_incr_rows and mfft_nlz_incr_hist_rows, 256 bins over a range that holds every increment: every
    row of counts sums to nrows n, and sum counts centre^2 agrees with S2 to half a bin -- a value lies within w / 2 of its bin's
    centre, |c^2 - d^2| <= (w / 2)(2 |d| + w / 2), summed: w sqrt(count S2) + count w^2 / 4 (Cauchy-Schwarz)."""
    from mpifft4py_amd import DeviceArray, _lib
    nrows, valid, nbins = 37, n // 2 + 1, 256
    seps = _stage_seps(n)
    a, b, fields, _, _, _ = _stage_case(n, prec, 6, nrows, valid, 0, seps, nbins)
    top = np.array([[1.01 * float(np.max(np.abs(ih.incr(x, s)))) for s in seps] for x in fields])
    got = _rows_call(a, b, 6, nrows, n, valid + 3, valid, 0, prec, seps, -top, top, nbins)
    sums = np.zeros(6 * 8 * 3)
    sv = np.ascontiguousarray(seps, dtype=np.int64)
    da, db = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b)
    _lib.call("mfft_nlz_incr_rows", da.ptr, db.ptr, 6, nrows, n, valid + 3, valid, 0, _lib.precision_code(prec), sv.ctypes.data_as(IP), 8,
              sums.ctypes.data_as(DP))
    S2 = sums.reshape(6, 8, 3)[:, :, 0]
    count = nrows * n
    assert np.all(got.sum(2) == count) and np.all(got[:, :, 0] == 0) and np.all(got[:, :, -2:] == 0)
    w = 2 * top / nbins
    centres = -top[:, :, None] + (np.arange(nbins) + 0.5) * w[:, :, None]
    m2 = (got[:, :, 1:-2] * centres ** 2).sum(2)
    bound = w * np.sqrt(count * S2) + count * w * w / 4
    print("consistency n=%d %s: max |sum c^2 - S2| / bound %.3f" % (n, prec, float(np.max(np.abs(m2 - S2) / bound))))
    assert np.all(np.abs(m2 - S2) <= bound)


# ---- 5. non-finite bins, error codes ---------------------------------------------------------------------------------------
def test_stage_nonfinite_bins_mark_their_field_only():
    n, nrows, valid, nbins = 128, 5, 65, 31
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    b = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    seps = [1, 7, 64, 127]
    clean = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", seps, -0.5, 0.5, nbins)
    assert np.all(clean.sum(2) == nrows * n) and np.all(clean[:, :, -1] == 0)
    keep = [0, 2, 3, 4, 5]
    for bad in (np.nan, np.inf):
        an = a.copy()
        an[1, 3, 7] = bad
        got = _rows_call(an, b, 6, nrows, n, valid, valid, 0, "double", seps, -0.5, 0.5, nbins)
        print("bad bin %r: field 1, s = 1: %s" % (bad, got[1, 0]))
        assert np.all(got[1, :, -1] >= 1) and np.all(got[1].sum(1) == nrows * n)
        assert np.array_equal(got[keep], clean[keep])      # b_1 rides on the same transform: exactly the counts of the clean run


def test_error_codes_and_untouched_outputs():
    """MFFT_ERR_UNSUPPORTED for a length without a kernel (the stage call); MFFT_ERR_INVALID for nbins of 0 or above 256, nsep of 0 or
    above 8, a separation < 1 or >= M, hi <= lo, a range that is not finite and valid > n / 2 + 1 -- the status codes themselves, on
    the stage call, the sweep and the plan call; a refused call writes nothing, byte for byte."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, _lib
    from mpifft4py_amd._base import _DEALIAS
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    INV, UNS = codes["MFFT_ERR_INVALID"], codes["MFFT_ERR_UNSUPPORTED"]
    assert int(re.search(r"#define MFFT_INCR_HIST_MAXBINS (\d+)", header).group(1)) == MAXBINS
    lib = _lib.load()
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    out = np.full((6, MAXSEP + 1, MAXBINS + 4), POISON, dtype=np.int64)
    before = out.tobytes()
    count = ctypes.c_int64(-5)
    arr = lambda v, n: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))

    def bad_cases(M):
        """(seps, nsep or None, nbins, lo, hi) that must be refused for a row of M points."""
        return [([1], None, 0, -1, 1), ([1], None, MAXBINS + 1, -1, 1), ([1], 0, 31, -1, 1), ([1] * (MAXSEP + 1), None, 31, -1, 1),
                ([0], None, 31, -1, 1), ([-1], None, 31, -1, 1), ([M], None, 31, -1, 1), ([1, 2, M + 70], None, 31, -1, 1),
                ([1], None, 31, 1, 1), ([1], None, 31, 1, -1), ([1], None, 31, -np.inf, 1), ([1], None, 31, -1, np.nan),
                ([1, 2], None, 31, [-1, 3], [1, 2])]

    def stage(seps, nsep, nbins, lo, hi, n=128, valid=65):
        s = np.ascontiguousarray(seps, dtype=np.int64)
        k = len(seps)
        l, h = arr(lo, 6 * k) if np.ndim(lo) == 0 else np.tile(arr(lo, k), 6), arr(hi, 6 * k) if np.ndim(hi) == 0 else np.tile(arr(hi, k), 6)
        return lib.mfft_nlz_incr_hist_rows(z.ptr, z.ptr, 6, 4, n, 65, valid, 0, _lib.DOUBLE, s.ctypes.data_as(IP), k if nsep is None else nsep,
                                           l.ctypes.data_as(DP), h.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP))
    for case in bad_cases(128):
        rc = stage(*case)
        print("stage", case, "->", rc)
        assert rc == INV, (case, rc)
    assert stage([1], None, 31, -1, 1, n=100, valid=51) == UNS         # 100 has no fused kernel
    assert stage([1], None, 31, -1, 1, n=64) == INV                    # more bins than a row of 64 points has
    assert _lib.call("mfft_nlz_incr_hist_groups", 4, 100, _lib.DOUBLE) == 0
    assert out.tobytes() == before
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), "double")
    x = DeviceArray.zeros((3, 8, 16, 32), np.float64)

    def sweep(seps, nsep, nbins, lo, hi):
        s = np.ascontiguousarray(seps, dtype=np.int64)
        k = len(seps)
        l, h = arr(lo, 3 * k) if np.ndim(lo) == 0 else np.tile(arr(lo, k), 3), arr(hi, 3 * k) if np.ndim(hi) == 0 else np.tile(arr(hi, k), 3)
        return lib.mfft_ew_increment_histogram(F._plan, x.ptr, 3, 128, 32, 32, _lib.DOUBLE, s.ctypes.data_as(IP), k if nsep is None else nsep,
                                               l.ctypes.data_as(DP), h.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP))
    for case in bad_cases(32):
        rc = sweep(*case)
        assert rc == INV, ("sweep", case, rc)
    assert out.tobytes() == before
    a = F.empty_complex(3).set(np.zeros((3,) + tuple(F.complex_shape()), np.complex128))
    for dealias, M in ((None, 32), ("2/3-rule", 32), ("3/2-rule", 48)):
        if dealias == "2/3-rule":
            F._ensure_mask()

        def plan(seps, nsep, nbins, lo, hi):
            s = np.ascontiguousarray(seps, dtype=np.int64)
            k = len(seps)
            l, h = arr(lo, 6 * k) if np.ndim(lo) == 0 else np.tile(arr(lo, k), 6), arr(hi, 6 * k) if np.ndim(hi) == 0 else np.tile(arr(hi, k), 6)
            return lib.mfft_real_increment_histogram(F._plan, a.ptr, a.ptr, 3, _DEALIAS[dealias], s.ctypes.data_as(IP), k if nsep is None else nsep,
                                                     l.ctypes.data_as(DP), h.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP), ctypes.byref(count))
        for case in bad_cases(M):
            rc = plan(*case)
            assert rc == INV, (dealias, case, rc)
        assert out.tobytes() == before and count.value == -5
        # the last valid separation of the mode is taken: rows of zeros, every increment in the bin that holds 0
        assert plan([M - 1], None, 31, -1, 1) == 0
        pts = int(np.prod([3 * n // 2 for n in (8, 16, 32)])) if dealias == "3/2-rule" else 8 * 16 * 32
        got = out.reshape(-1)[:6 * 34].reshape(6, 34)
        assert count.value == pts and got[:, 16].tolist() == [pts] * 6 and got.sum() == 6 * pts
        out[:] = POISON
        count.value = -5


# ---- 6. the plan operation ------------------------------------------------------------------------------------------------
_REF = {}


def _reference(N, prec, dealias):
    """The moments tests' seeded spectra (seed 11 + N2), the oracle's six real fields, and per field the 3-D sum of the bound."""
    key = (tuple(int(n) for n in N), prec, dealias)
    if key not in _REF:
        from mpifft4py_amd import LayoutComm
        from mpifft4py_amd.slab import R2C
        N = np.array(N)
        F = R2C(N, L, LayoutComm(1, 0), prec)
        a, b = nl.spectra(tuple(F.complex_shape()), N, prec, 11 + int(N[2]), True)
        mask = F.get_dealias_filter() if dealias == "2/3-rule" else None
        ua, ub = nl.oracle_back(a, N, prec, dealias, mask), nl.oracle_back(b, N, prec, dealias, mask)
        h = np.full(a.shape[-1], 2.0)
        h[0] = 1.0
        if N[2] % 2 == 0:
            h[-1] = 1.0
        grid = np.array([3 * n // 2 for n in N]) if dealias == "3/2-rule" else N
        scale = 8 * ih.EPS[prec] * np.log2(float(np.prod(grid))) / float(np.prod(N))
        m = 1.0 if mask is None else np.asarray(mask, dtype=np.float64)
        sums = [scale * float(np.sum(np.abs(x[i].astype(np.complex128)) * m * h)) for x in (a, b) for i in range(3)]
        _REF[key] = (a, b, ua, ub, sums)
    return _REF[key]


def _partner(f, nfields):
    """The field that shares field f's transform on the fused routes (None: alone)."""
    if nfields == 6:
        return (f + 3) % 6
    g = f ^ 1
    return g if g < nfields else None


_SETUP = {}
LADDER = (64, 32, 16, 8, 4, 3, 2, 1)


def _setup(N, prec, dealias, nfields, seps=None):
    """(fields, seps, lo, hi, nbins, deltas) of a plan case, from the reference alone.  Every (field, separation) over +-4 sigma of its
    increments.  The worst-case delta of a 3-D transform grows with sqrt(points), so in single precision on the larger meshes 64
    bins cannot meet the 1 % condition whatever the device computes -- least of all at s = 1, where the increments are small and
    delta is the whole field's: nbins is the first of 64, 32, 16, 8, 4, 3, 2, 1 at which every field and separation of the case meets
    it (3 before 2: its edges lie at +-4/3 sigma, where the density is lower than at 0) -- 64 throughout in double precision.  The
    condition itself is asserted in ih.bracket."""
    from mpifft4py_amd import spectral
    key = (tuple(int(n) for n in N), prec, dealias, nfields, None if seps is None else tuple(seps))
    if key not in _SETUP:
        a, b, ua, ub, sums = _reference(N, prec, dealias)
        fields = (list(ua) + list(ub))[:nfields]
        sp = spectral.default_seps(fields[0].shape[-1]) if seps is None else list(seps)
        lo, hi = _ranges(fields, sp)
        deltas = [sums[f] + (sums[_partner(f, nfields)] if _partner(f, nfields) is not None else 0.0) for f in range(nfields)]
        nbins = LADDER[-1]
        for nb in LADDER:
            if all(np.mean(ih.slots(ih.incr(x, s) + 2 * d, lo[f, i], hi[f, i], nb) != ih.slots(ih.incr(x, s) - 2 * d, lo[f, i], hi[f, i], nb)) <= 0.01
                   for f, (x, d) in enumerate(zip(fields, deltas)) for i, s in enumerate(sp)):
                nbins = nb
                break
        assert prec == "single" or nbins == 64, (key, nbins)
        _SETUP[key] = (fields, sp, lo, hi, nbins, deltas)
    return _SETUP[key]


def _call(F, a, b, nfields, dealias, seps, lo, hi, nbins, reduce=True):
    from mpifft4py_amd import spectral
    if nfields == 1:
        da, db = F.empty_complex().set(a[0]), None
    else:
        da, db = F.empty_complex(3).set(a), (F.empty_complex(3).set(b) if nfields == 6 else None)
    return spectral.real_increment_histogram(F, da, db, dealias, seps=seps, bins=nbins, range=np.stack([lo, hi], 2), reduce=reduce), da, db


def _plan_case(F, N, prec, dealias, nfields, fused, seps=None):
    from mpifft4py_amd import spectral
    a, b = _reference(N, prec, dealias)[:2]
    fields, sp, lo, hi, nbins, deltas = _setup(N, prec, dealias, nfields, seps)
    h, da, db = _call(F, a, b, nfields, dealias, seps, lo, hi, nbins)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    M = fields[0].shape[-1]
    assert h.M == M == (3 * N[2] // 2 if dealias == "3/2-rule" else N[2]) and list(h.seps) == sp
    assert h.count == fields[0].size and h.raw.shape == (nfields, len(sp), nbins + 3) and h.raw.dtype == np.int64
    for f in range(nfields):
        for i, s in enumerate(sp):
            ih.bracket(h.raw[f, i], fields[f], deltas[f], s, lo[f, i], hi[f, i], nbins, "%s %s %s nfields=%d field %d" % (list(N), prec, dealias, nfields, f))
    assert np.array_equal(da.get(), a[0] if nfields == 1 else a) and (db is None or np.array_equal(db.get(), b))      # inputs preserved
    again = spectral.real_increment_histogram(F, da, db, dealias, seps=seps, bins=nbins, range=np.stack([lo, hi], 2))
    assert np.array_equal(again.raw, h.raw) and again.count == h.count                                              # identical arrays
    return h


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_increment_histogram_one_rank_fused(N, dealias, nfields, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, nfields, True)


def test_real_increment_histogram_long_lists_go_in_chunks():
    """Eleven separations, a duplicate and the two ends of the range among them: two calls of the library, one result."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = [8, 16, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    assert spectral.INCR_MAXSEP < 11
    for dealias, M in (("3/2-rule", 48), (None, 32)):
        seps = [1, 2, 3, 5, 7, 11, 13, M // 2, M - 1, 1, 17]
        h = _plan_case(F, N, "double", dealias, 6, True, seps=seps)
        assert np.array_equal(h.raw[:, 0], h.raw[:, 9])
        fields, sp, lo, hi, nbins, _ = _setup(N, "double", dealias, 6, seps)
        one = _call(F, *_reference(N, "double", dealias)[:2], 6, dealias, seps[8:], lo[:, 8:], hi[:, 8:], nbins)[0]
        assert np.array_equal(one.raw, h.raw[:, 8:])


def test_real_increment_histogram_pitched_plan_with_nans_between_rows():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert F.complex_pitch > F.complex_shape()[-1]
    for dealias in ("3/2-rule", "2/3-rule", None):
        a, b = _reference(N, prec, dealias)[:2]
        fields, sp, lo, hi, nbins, deltas = _setup(N, prec, dealias, 6)
        da, db = F.empty_complex(3), F.empty_complex(3)
        for d in (da, db):                                                         # NaNs between the rows
            whole = DeviceArray(d.shape[:-1] + (F.complex_pitch,), d.dtype, ptr=d.ptr, owner=False)
            whole.set(np.full(whole.shape, np.nan + 1j * np.nan, dtype=d.dtype))
        da.set(a), db.set(b)
        h = spectral.real_increment_histogram(F, da, db, dealias, bins=nbins, range=np.stack([lo, hi], 2))
        assert F.plan_info(INFO(dealias)) == 1
        for f in range(6):
            for i, s in enumerate(sp):
                ih.bracket(h.raw[f, i], fields[f], deltas[f], s, lo[f, i], hi[f, i], nbins, "pitched %s field %d" % (dealias, f))


def test_real_increment_histogram_nan_marks_its_field_only():
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b = _reference(N, prec, None)[:2]
    fields, sp, lo, hi, nbins, _ = _setup(N, prec, None, 6)
    clean = _call(F, a, b, 6, None, None, lo, hi, nbins)[0]
    an = a.copy()
    an[2, 3, 5, 7] = np.nan
    h = _call(F, an, b, 6, None, None, lo, hi, nbins)[0]
    keep = [0, 1, 3, 4, 5]
    assert np.all(h.raw[2, :, -1] >= 1) and np.all(h.raw.sum(2) == h.count)
    assert np.array_equal(h.raw[keep], clean.raw[keep])


# ---- composed route: a fresh process (the switch is read once) -------------------------------------------------------------
def test_real_increment_histogram_composed_kill_switch():
    """MFFT_NO_NLZ=1: one field at a time through the plan's inverse transform into ONE real work array and the sweep; [8, 16, 32]
    (fused without the switch), [16, 32, 24] and [20, 24, 40] (no fused kernels for 24 / 36, 40 / 60 either).  The plan's nonlinear
    buffers hold that one array: the padded real field of the 3/2-rule, the first mode run (the histogram test's check)."""
    nl.run_child("""
import test_gpu_real_increment_histogram as t
for N in ([8, 16, 32], [16, 32, 24], [20, 24, 40]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for nfields in (6, 1, 3):
                t._plan_case(F, N, prec, dealias, nfields, False)
            one = int(np.prod([3 * n // 2 for n in N])) * (8 if prec == 'double' else 4)
            assert F.plan_info('nonlinear_bytes') == one, (F.plan_info('nonlinear_bytes'), one)
print('ok')
""", timeout=280, MFFT_NO_NLZ="1")


def test_real_increment_histogram_lengths_without_a_kernel_are_composed():
    """[24, 40, 20]: no fused z kernel of 20 or 30 points, so every mode goes through the one work array and the sweep; [16, 32, 24]
    has one of 24 but none of 36, so only its 3/2-rule does."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N = [24, 40, 20]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "double")
    for dealias in ("3/2-rule", "2/3-rule", None):
        _plan_case(F, N, "double", dealias, 6, False)
    N = [16, 32, 24]
    F = Slab_R2C(np.array(N), L, SelfComm(0), "single")
    for dealias in ("3/2-rule", "2/3-rule", None):
        _plan_case(F, N, "single", dealias, 3, dealias != "3/2-rule")


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_real_increment_histogram_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan, flag 0; z is whole on every rank): every rank's counts EQUAL the
    sweep of the real fields its own ifftn gives (the composed route IS that transform and that sweep), which equals numpy on them;
    the reduced counts are the ranks' sum, the same on every rank."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 24])

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(50 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a, b = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.25), x.component(i))
        seps = spectral.default_seps(ws[-1])
        rngs = np.array([[(-0.3 - 0.01 * f - 0.02 * i, 0.3 + 0.02 * f + 0.01 * i) for i in range(len(seps))] for f in range(6)])
        u = DeviceArray.empty(ws, F.float)
        mine = []
        for f, (x, i) in enumerate([(x, i) for x in (a, b) for i in range(3)]):
            F.ifftn(x.component(i), u, dealias)
            s = spectral.increment_histogram(F, u, bins=50, range=rngs[f:f + 1])
            assert np.array_equal(s.raw[0], ih.counts(u.get().astype(np.float64), seps, rngs[f, :, 0], rngs[f, :, 1], 50))
            mine.append(s.raw[0])
        local = spectral.real_increment_histogram(F, a, b, dealias, bins=50, range=rngs, reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == int(np.prod(ws)) and local.M == ws[-1]
        assert np.array_equal(local.raw, np.stack(mine))
        glob = spectral.real_increment_histogram(F, a, b, dealias, bins=50, range=rngs)
        return local.raw, local.count, glob.raw, glob.count

    res = run_ranks(4, work)
    for _, _, g, cnt in res:
        assert cnt == sum(r[1] for r in res) and np.array_equal(g, res[0][2])
    assert np.array_equal(np.sum([r[0] for r in res], 0), res[0][2]) and np.all(res[0][2].sum(2) == res[0][3])


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
_ONE = {}


def _one_rank(N, dealias):
    from mpifft4py_amd import SelfComm, Slab_R2C
    key = (tuple(N), dealias)
    if key not in _ONE:
        a, b = _reference(N, "double", dealias)[:2]
        fields, sp, lo, hi, nbins, _ = _setup(N, "double", dealias, 6)
        _ONE[key] = _call(Slab_R2C(np.array(N), L, SelfComm(0), "double"), a, b, 6, dealias, None, lo, hi, nbins)[0]
    return _ONE[key]


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N,P", [([32, 64, 128], 2), ([32, 64, 128], 4), ([8, 16, 32], 2), ([8, 16, 32], 4)])
def test_real_increment_histogram_ranks_fused(N, P, dealias):
    """The ranks' counts add up to the reduced ones, and those are IDENTICAL to the one-rank result: the fused routes compute the same
    values on every number of ranks, and counts are integers."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua, ub, _ = _reference(N, "double", dealias)
    fields, sp, lo, hi, nbins, deltas = _setup(N, "double", dealias, 6)
    one = _one_rank(N, dealias)
    rngs = np.stack([lo, hi], 2)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_increment_histogram(F, da, db, dealias, bins=nbins, range=rngs, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_increment_histogram(F, da, db, dealias, bins=nbins, range=rngs)
        three = spectral.real_increment_histogram(F, da, None, dealias, bins=nbins, range=rngs[:3])
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return local.raw, local.count, glob.raw, glob.count, three.raw

    out = run_ranks(P, work)
    planes = ua.shape[1] // P                                                      # a rank holds the counts of its own x planes
    for r, (local, lcount, glob, gcount, three) in enumerate(out):
        assert lcount == fields[0][r * planes:(r + 1) * planes].size and gcount == fields[0].size == one.count
        assert np.array_equal(glob, out[0][2])                                     # equal on all ranks
    assert np.array_equal(np.sum(np.stack([o[0] for o in out]), 0), out[0][2])     # local counts add up to the reduced ones
    assert np.array_equal(out[0][2], one.raw), np.argwhere(out[0][2] != one.raw)[:8]      # ... and are the one-rank counts, exactly
    for f in range(3):                                                              # three fields pair up differently: brackets
        for i, s in enumerate(sp):
            d3 = _reference(N, "double", dealias)[4]
            delta = d3[f] + (d3[f ^ 1] if (f ^ 1) < 3 else 0.0)
            ih.bracket(out[0][4][f, i], fields[f], delta, s, lo[f, i], hi[f, i], nbins, "%s P=%d %s three fields, field %d" % (N, P, dealias, f))


# ---- 7. range=None --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_range_none_takes_sigmas_from_real_increments(dealias):
    """The ranges are +-sigmas sigma(f, s) with sigma from `real_increments` on the same separations; a single sine mode has
    |d| <= sqrt(2) sigma_d, so nothing lands outside +-10 or +-4 sigma; a field without increments (zero) gets +-0.5."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    x = np.arange(32) * 2 * np.pi / 32
    U = F.empty_complex(3)
    fields = [np.broadcast_to(np.sin(x), (8, 16, 32)).copy(), np.broadcast_to(2.5 * np.cos(x) + 1.0, (8, 16, 32)).copy(), np.zeros((8, 16, 32))]
    for f, u in enumerate(fields):
        F.fftn(DeviceArray.from_numpy(u), U.component(f))
    inc = spectral.real_increments(F, U, None, dealias)
    for sigmas in (10.0, 4.0):
        h = spectral.real_increment_histogram(F, U, None, dealias, sigmas=sigmas)
        assert F.plan_info(INFO(dealias)) == 1 and h.nbins == 128 and list(h.seps) == list(inc.seps)
        sg = np.sqrt(inc.sums[:, :, 0] / inc.count)
        want = sigmas * sg
        want[2] = 0.5
        print("range=None (%s, %g sigma): hi %s" % (dealias, sigmas, h.hi))
        assert np.array_equal(h.hi[:2], want[:2]) and np.array_equal(h.lo, -h.hi) and np.all(h.hi[2] == 0.5)
        assert np.all(h.raw[:, :, 0] == 0) and np.all(h.raw[:, :, -2:] == 0) and np.all(h.raw.sum(2) == h.count)
        assert np.all(h.raw[2, :, 1 + 64] == h.count)                              # the constant field: every increment 0, the bin that holds 0
    # the sweep takes its sigmas from `increments`
    u = DeviceArray.from_numpy(np.stack(fields))
    hs = spectral.increment_histogram(F, u)
    si = spectral.increments(F, u)
    assert np.array_equal(hs.hi[:2], 10.0 * np.sqrt(si.sums[:2, :, 0] / si.count)) and np.all(hs.raw[:, :, 0] == 0) and np.all(hs.raw[:, :, -2:] == 0)


# ---- 8. known answer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_taylor_green_known_moments(dealias):
    """u = sin x cos y cos z at N = 32, r = 2 pi s / M: the increments along z are -2 sin x cos y sin(r/2) sin(z + r/2), so
    S_2 = sin^2(r/2) / 2 and S_4 = (27/32) sin^4(r/2).  The moments of the PDF agree to bin-width accuracy: a value lies within w / 2
    of its centre, |c^p - d^p| <= p (w / 2) max(|c|, |d|)^(p-1) with |c|, |d| <= 1.03 A, A = 2 sin(r/2): p (w / 2) (1.03 A)^(p-1).  The counts
    themselves EQUAL numpy's on the exact field: 251 bins (odd: 0 sits in the middle of one) over +-1.03 A, for which no increment sits within 1e-6 bins of an edge
    (asserted), so a transform's rounding cannot move one."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    M = 48 if dealias == "3/2-rule" else 32
    x = np.arange(32) * 2 * np.pi / 32
    xm = np.arange(M) * 2 * np.pi / M
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    U = F.empty_complex()
    F.fftn(DeviceArray.from_numpy(np.sin(X) * np.cos(Y) * np.cos(Z)), U)
    Xm, Ym, Zm = np.meshgrid(xm, xm, xm, indexing="ij")
    u = np.sin(Xm) * np.cos(Ym) * np.cos(Zm)                                       # the field on the grid the mode is formed on
    seps = spectral.default_seps(M)
    r = np.array(seps) * 2 * np.pi / M
    A = 2 * np.sin(r / 2)
    nbins = 251
    lo, hi = -1.03 * A, 1.03 * A
    edge = 1.0
    for i, s in enumerate(seps):
        t = (ih.incr(u, s) - lo[i]) * (nbins / (hi[i] - lo[i]))
        edge = min(edge, float(np.min(np.abs(t - np.round(t)))))
    print("Taylor-Green: nearest increment to an edge, in bins: %.3e" % edge)
    assert edge > 1e-6
    h = spectral.real_increment_histogram(F, U, None, dealias, seps=seps, bins=nbins, range=np.stack([lo, hi], 1)[None])
    assert F.plan_info(INFO(dealias)) == 1 and h.count == M ** 3
    want = ih.counts(u, seps, lo, hi, nbins)
    assert np.array_equal(h.raw[0], want), np.argwhere(h.raw[0] != want)[:8]
    w = (hi - lo) / nbins
    m2, m4, m3 = h.moment(2)[0], h.moment(4)[0], h.moment(3)[0]
    sh = np.sin(r / 2) ** 2
    print("Taylor-Green (%s): m2 %s want %s\n  m4 %s want %s" % (dealias, m2, sh / 2, m4, 27.0 / 32 * sh * sh))
    assert np.all(np.abs(m2 - sh / 2) <= 2 * (w / 2) * 1.03 * A) and np.all(np.abs(m4 - 27.0 / 32 * sh * sh) <= 4 * (w / 2) * (1.03 * A) ** 3)
    assert np.all(np.abs(m3) <= 3 * (w / 2) * (1.03 * A) ** 2)


# ---- 9. the example -------------------------------------------------------------------------------------------------------
def test_example_structure_pdf():
    """--structure-pdf prints, per separation, the longitudinal increment flatness from the PDF next to the one from real_increments;
    after two steps of the Taylor-Green flow both are finite, at least 1, and within a tenth of each other (128 bins over +-10
    sigma: a bin is 0.16 sigma wide)."""
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--structure-pdf", "--steps", "2"]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"^structure-pdf s = (\d+)\s+flatness from the PDF ([0-9.eE+-]+)\s+from the sums ([0-9.eE+-]+)", r.stdout, re.M)
    assert [int(s) for s, _, _ in rows] == [1, 2, 4, 8, 16, 24], r.stdout
    p, q = np.array([float(a) for _, a, _ in rows]), np.array([float(b) for _, _, b in rows])
    print("example --structure-pdf: flatness from the PDF %s, from the sums %s" % (p, q))
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(q)) and np.all(q >= 1.0) and np.all(p >= 1.0) and np.all(np.abs(p - q) <= 0.1 * q)
