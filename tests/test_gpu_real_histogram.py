"""GPU: histograms of spectral fields without the real-space arrays (mfft_real_histogram, mfft_nlz_hist_rows, mfft_ew_histogram;
csrc/nlz_hist.h NlzHist::body, csrc/hist.hip) -- the sweep against numpy exactly, the z stage on known answers exactly and on random
spectra by brackets, the plan operation on every route (fused on one rank and several, batches, composed, pencils, pitched),
`range=None`, the Taylor-Green known answer and the example's --pdf.

Counts have no tolerance.  Where the values come from a transform they are compared by BRACKETS: the slot rule (`_slots`, the
rule of include/mpifft4py_amd.h evaluated by numpy in float64) is monotone in x, so with |x_device - x_ref| <= delta every
cumulative count obeys  C_j(x_ref + delta) <= C_j(device) <= C_j(x_ref - delta),  j = 0 .. nbins + 1; the total equals the
number of points and the non-finite slot is 0.  delta is a worst-case bound, not a measurement: per transform
    delta = 8 eps_T log2(n) sum_k h_k (|A_k| + |B_k|) / n,      eps_T = 2^-53 / 2^-24, h the Hermitian weights,
over BOTH fields of a pair (they share the transform); for a plan the sum runs over the 3-D spectrum, n is the number of points
of the grid the transform runs on (the padded one under the 3/2-rule) and the divisor the points of the mesh.  Asserted from the
reference alone: at most 1 % of the points change their slot between x_ref - delta and x_ref + delta, so a shift by one bin --
which moves whole bins -- cannot pass."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, cdtype, have_gpu, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
EPS = {"double": 2.0 ** -53, "single": 2.0 ** -24}
MAXBINS = 512


def INFO(dealias):
    return "nonlinear_histogram_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _slots(x, lo, hi, nbins):
    """The slot rule, numpy float64."""
    x = np.asarray(x, dtype=np.float64)
    inv = np.float64(nbins) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - np.float64(lo)) * inv
        nan, below, above = x != x, t < 0, t >= nbins
        mid = ~(nan | below | above)
        s = np.zeros(x.shape, dtype=np.int64)
        s[mid] = 1 + t[mid].astype(np.int64)
    s[above & ~below & ~nan] = nbins + 1
    s[below & ~nan] = 0
    s[nan] = nbins + 2
    return s


def _hist(x, lo, hi, nbins):
    return np.bincount(_slots(x, lo, hi, nbins).ravel(), minlength=nbins + 3).astype(np.int64)


def _raw(h):
    return np.concatenate([h.below[:, None], h.counts, h.above[:, None], h.nonfinite[:, None]], axis=1)


def _bracket(counts, x, delta, lo, hi, nbins, what):
    """counts: the nbins + 3 device counts of one field; x: its reference values; delta: the bound, broadcastable to x."""
    x = np.asarray(x, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    su, sd = _slots(x + delta, lo, hi, nbins), _slots(x - delta, lo, hi, nbins)
    share = float(np.mean(su != sd))
    outside = float(np.mean((x < lo) | (x >= hi)))
    cu = np.cumsum(np.bincount(su.ravel(), minlength=nbins + 3))[:nbins + 2]
    cd = np.cumsum(np.bincount(sd.ravel(), minlength=nbins + 3))[:nbins + 2]
    cg = np.cumsum(counts)[:nbins + 2]
    print("histogram %s: %d points, delta max %.3e, slot changes within +-delta %.4f %%, outside the range %.4f %%, "
          "cumulative slack below %d above %d" % (what, x.size, float(np.max(delta)), 100 * share, 100 * outside,
                                                 int(np.min(cg - cu)), int(np.min(cd - cg))))
    assert share <= 0.01, (what, share)
    assert counts.sum() == x.size and counts[nbins + 2] == 0, (what, counts.sum(), x.size, counts[nbins + 2])
    assert np.all(cu <= cg) and np.all(cg <= cd), (what, np.flatnonzero((cu > cg) | (cg > cd)))


# ---- 1. the sweep: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15)])
def test_sweep_equals_numpy(shape, prec):
    """spectral.histogram of random real arrays with values placed exactly on edges, at lo, at hi, +-Inf and NaN EQUALS numpy
    evaluating the slot rule in float64; (1, 7, 9, 15) has 945 elements, so heads and tails of the 16-byte lanes are met."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(7 + shape[0])
    x = (3.0 * rng.standard_normal(shape)).astype(rdtype(prec))
    lo, hi, nbins = -4.0, 4.0, 64                    # edges at multiples of 1/8: exact in both precisions
    flat = x.reshape(shape[0], -1)
    n = flat.shape[1]
    for c in range(shape[0]):
        special = [lo, hi, -3.875, 0.0, 0.125, 3.875, np.nextafter(rdtype(prec)(hi), rdtype(prec)(0)), np.inf, -np.inf, np.nan, np.nan]
        where = rng.choice(n, len(special), replace=False)
        where[:3] = [0, n - 1, n // 2]               # the first, the last and a middle element among them
        flat[c, where] = special
    want = np.stack([_hist(flat[c], lo, hi, nbins) for c in range(shape[0])])
    h = spectral.histogram(F, DeviceArray.from_numpy(x), bins=nbins, range=(lo, hi))
    got = _raw(h)
    print("sweep %s %s: below %s above %s nonfinite %s" % (shape, prec, h.below, h.above, h.nonfinite))
    assert h.count == n and got.dtype == np.int64 and got.shape == (shape[0], nbins + 3)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert np.all(h.nonfinite >= 1) and np.all(got.sum(1) == n)
    # one range per component, an odd bin count, bins that are not binary fractions: still the same expressions in the same order
    rngs = [(-1.0 - 0.1 * c, 2.0 + 0.3 * c) for c in range(shape[0])]
    h = spectral.histogram(F, DeviceArray.from_numpy(x), bins=37, range=rngs)
    want = np.stack([_hist(flat[c], rngs[c][0], rngs[c][1], 37) for c in range(shape[0])])
    assert np.array_equal(_raw(h), want)
    if shape[0] == 3:
        pitched = DeviceArray.from_numpy(x)
        view = DeviceArray(pitched.shape, pitched.dtype, ptr=pitched.ptr, owner=False)
        view.pitch = 40
        with pytest.raises(ValueError):
            spectral.histogram(F, view, bins=8, range=(lo, hi))


# ---- the stage alone --------------------------------------------------------------------------------------------------
# The lengths of the moments tests: 16 (two threads per row, wave-synchronous), 512 (one row per wave), 1024 (two waves per row,
# barrier build), 768 (a 12-values plan), 3072 (256 threads per row; in double precision the split exchange).
LENGTHS = [16, 512, 768, 1024, 3072]


def _irfft_rows(x, n, vin):
    x = x[..., :vin].astype(np.complex128)
    x[..., 0] = x[..., 0].real
    if vin == n // 2 + 1 and n % 2 == 0:
        x[..., -1] = x[..., -1].real
    return np.fft.irfft(x, n=n, axis=-1)


def _row_delta(x, n, vin, prec):
    """8 eps log2(n) sum_k h_k |A_k| / n per row of the stored spectra x[..., :vin] (Im of the self-conjugate bins is not read)."""
    a = np.abs(x[..., :vin].astype(np.complex128))
    a[..., 0] = np.abs(x[..., 0].real)
    h = np.full(vin, 2.0)
    h[0] = 1.0
    if vin == n // 2 + 1 and n % 2 == 0:
        a[..., -1] = np.abs(x[..., vin - 1].real)
        h[-1] = 1.0
    return 8 * EPS[prec] * np.log2(n) * (a * h).sum(-1) / n


def _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, lo, hi, nbins, da=None, db=None):
    from mpifft4py_amd import DeviceArray, _lib
    da = DeviceArray.from_numpy(a) if da is None else da
    db = (DeviceArray.from_numpy(b) if b is not None else None) if db is None else db
    got = np.full((nfields, nbins + 3), -1, dtype=np.int64)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (nfields,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (nfields,)))
    _lib.call("mfft_nlz_hist_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, valid_in,
              _lib.precision_code(prec), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, got.ctypes.data_as(IP))
    assert da.get().tobytes() == a.tobytes() and (b is None or db.get().tobytes() == b.tobytes())      # inputs preserved
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_stage_known_answers_exact(n, prec):
    """Three fields whose real rows are known: only bin 0 set (the constant 2: all nrows n points in one slot), bins 0 and n/2 set
    (1 + 2 (-1)^j: two slots, nrows n / 2 each), the single bin n/4 (3 cos(pi j / 2) = {3, 0, -3, 0}).  Nine bins of width 1 over
    [-4.5, 4.5): 0 sits in the middle of bin 4 and every value half a bin from an edge, so the counts are exact."""
    nrows, valid, nbins = 5, n // 2 + 1, 9
    a = np.zeros((3, nrows, valid + 3), dtype=cdtype(prec))
    a[0, :, 0] = 2.0 * n
    a[1, :, 0] = 1.0 * n
    a[1, :, n // 2] = 2.0 * n
    a[2, :, n // 4] = 1.5 * n
    got = _rows_call(a, None, 3, nrows, n, valid + 3, valid, 0, prec, -4.5, 4.5, nbins)
    want = np.zeros((3, nbins + 3), dtype=np.int64)
    slot = lambda v: 1 + int(v + 4.5)
    want[0, slot(2)] = nrows * n
    want[1, slot(3)] = want[1, slot(-1)] = nrows * n // 2
    want[2, slot(3)] = want[2, slot(-3)] = nrows * n // 4
    want[2, slot(0)] = nrows * n // 2
    print("known answers n=%d %s:\n%s" % (n, prec, got))
    assert np.array_equal(got, want)
    assert np.array_equal(want, np.stack([_hist(r, -4.5, 4.5, nbins) for r in _irfft_rows(a, n, valid)]))      # (the reference agrees)


_ROWS_PER_PASS = {}


def _pass_shape(n, prec):
    """(workgroups of a full launch, rows one workgroup takes per pass) from mfft_nlz_hist_groups alone."""
    from mpifft4py_amd import _lib
    if (n, prec) not in _ROWS_PER_PASS:
        code = _lib.precision_code(prec)
        cap = _lib.call("mfft_nlz_hist_groups", 1 << 40, n, code)
        per = 1
        while _lib.call("mfft_nlz_hist_groups", per + 1, n, code) == 1:      # rows per workgroup: a power of two
            per *= 2
        _ROWS_PER_PASS[(n, prec)] = (cap, per)
    return _ROWS_PER_PASS[(n, prec)]


def _stage_random(n, prec, nfields, nrows, valid, valid_in=0, nbins=64):
    """Seeded Gaussian spectra with real end bins, 64 bins over +-4 sigma of the reference rows."""
    rng = np.random.default_rng(100 * n + 7 * nrows % 1000 + valid + nfields)
    pitch = valid + 3
    ncomp = nfields // 2 if nfields % 2 == 0 else nfields
    shape = (ncomp, nrows, pitch)

    def draw():
        z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
        z[..., 0] = z[..., 0].real
        if n % 2 == 0 and valid == n // 2 + 1:
            z[..., valid - 1] = z[..., valid - 1].real
        return z
    a = draw()
    b = draw() if nfields % 2 == 0 else None
    vin = valid_in or valid
    fields = [r for x in (a, b) if x is not None for r in _irfft_rows(x, n, vin)]
    dl = [r for x in (a, b) if x is not None for r in _row_delta(x, n, vin, prec)]
    sig = [float(np.std(x)) for x in fields]
    lo, hi = np.array([-4 * s for s in sig]), np.array([4 * s for s in sig])
    flat = lambda x: x if nfields > 2 else x[0]
    got = _rows_call(flat(a), flat(b) if b is not None else None, nfields, nrows, n, pitch, valid, valid_in, prec, lo, hi, nbins)
    for f in range(nfields):
        # the partner on the transform: b_f for a_f where there are two arrays; among a's components the next / previous one
        g = (f + ncomp) % nfields if b is not None else (f ^ 1 if (f ^ 1) < nfields else None)
        delta = dl[f] + (dl[g] if g is not None else 0.0)
        outside = float(np.mean(np.abs(fields[f]) >= 4 * sig[f]))
        assert outside < 2e-4, outside
        _bracket(got[f], fields[f], delta[:, None], lo[f], hi[f], nbins,
                 "stage n=%d %s nfields=%d nrows=%d valid=%d/%d field %d" % (n, prec, nfields, nrows, vin, valid, f))
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_stage_random_spectra_bracket(n, prec):
    """1, 2, 3 and 6 fields; one row, an odd count, pruned valid_in; a second call gives identical arrays."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage_random(n, prec, 6, 37, full)
    assert np.array_equal(_stage_random(n, prec, 6, 37, full), first)
    _stage_random(n, prec, 3, 37, lim)
    _stage_random(n, prec, 2, 37, full, valid_in=lim)
    if n > 16:                                       # (one row of 16 points has no 64-bin PDF to bracket: the odd count covers 16)
        _stage_random(n, prec, 1, 1, full)
    else:
        _stage_random(n, prec, 1, 1, full, nbins=4)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_stage_more_than_two_passes_of_the_grid(n, prec):
    """More than two passes of mfft_nlz_hist_groups workgroups and a ragged rest: every workgroup strides, the last pass is partial."""
    from mpifft4py_amd import _lib
    cap, per = _pass_shape(n, prec)
    assert cap >= 1
    nrows = 2 * cap * per + per // 2 + 3
    assert _lib.call("mfft_nlz_hist_groups", nrows, n, _lib.precision_code(prec)) == cap
    _stage_random(n, prec, 1, nrows, n // 2 + 1)


def test_stage_nonfinite_bins_and_errors():
    from mpifft4py_amd import DeviceArray, _lib
    n, nrows, valid, nbins = 128, 5, 65, 31
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    b = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    clean = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", -0.5, 0.5, nbins)
    assert np.all(clean.sum(1) == nrows * n) and np.all(clean[:, -1] == 0)
    keep = [0, 2, 3, 4, 5]
    for bad in (np.nan, np.inf):
        an = a.copy()
        an[1, 3, 7] = bad
        got = _rows_call(an, b, 6, nrows, n, valid, valid, 0, "double", -0.5, 0.5, nbins)
        print("bad bin %r: field 1 %s" % (bad, got[1]))
        assert got[1, -1] >= 1 and got[1].sum() == nrows * n
        assert np.array_equal(got[keep], clean[keep])      # b_1 rides on the same transform: exactly the counts of the clean run


def test_stage_error_codes():
    """MFFT_ERR_UNSUPPORTED for a length without a kernel; MFFT_ERR_INVALID for nbins of 0 or above the maximum, hi <= lo and
    valid > n / 2 + 1: the status codes themselves, and a refused call writes nothing."""
    from mpifft4py_amd import DeviceArray, _lib
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    assert int(re.search(r"#define MFFT_HIST_MAXBINS (\d+)", header).group(1)) == MAXBINS
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    out = np.full((6, 34), -7, dtype=np.int64)
    one, mone = np.ones(6), -np.ones(6)
    fn = getattr(_lib.load(), "mfft_nlz_hist_rows")

    def status(n, valid, nbins, lo, hi):
        return fn(z.ptr, z.ptr, 6, 4, n, 65, valid, 0, _lib.DOUBLE, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nbins, out.ctypes.data_as(IP))
    cases = [((100, 51, 31, mone, one), "MFFT_ERR_UNSUPPORTED"), ((128, 65, 0, mone, one), "MFFT_ERR_INVALID"),
             ((128, 65, MAXBINS + 1, mone, one), "MFFT_ERR_INVALID"), ((128, 65, 31, one, one), "MFFT_ERR_INVALID"),
             ((128, 65, 31, one, mone), "MFFT_ERR_INVALID"), ((64, 51, 31, mone, one), "MFFT_ERR_INVALID")]
    for args, name in cases:
        rc = status(*args)
        print(args[:3], "->", rc)
        assert rc == codes[name], (args[:3], rc, name)
    assert np.all(out == -7)
    assert status(128, 65, 31, mone, one) == 0 and out[:, 16].tolist() == [4 * 128] * 6      # rows of zeros: the bin that holds 0
    assert _lib.call("mfft_nlz_hist_groups", 4, 100, _lib.DOUBLE) == 0


# ---- the plan operation ---------------------------------------------------------------------------------------------------
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
        scale = 8 * EPS[prec] * np.log2(float(np.prod(grid))) / float(np.prod(N))
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
LADDER = (64, 32, 16, 8, 4, 2)


def _setup(N, prec, dealias, nfields):
    """(fields, lo, hi, nbins, deltas) of a plan case, from the reference alone.  The range is +-4 sigma about each field's mean.
    The worst-case delta of a 3-D transform grows with sqrt(points) (the sum of |A_k|), so in single precision on the larger meshes
    64 bins cannot meet the 1 % condition whatever the device computes: nbins is the largest of 64, 32, .., 2 at which every field
    of the case meets it -- 64 throughout in double precision.  The condition itself is asserted in _bracket."""
    key = (tuple(int(n) for n in N), prec, dealias, nfields)
    if key not in _SETUP:
        a, b, ua, ub, sums = _reference(N, prec, dealias)
        fields = (list(ua) + list(ub))[:nfields]
        lo = np.array([float(np.mean(x) - 4 * np.std(x)) for x in fields])
        hi = np.array([float(np.mean(x) + 4 * np.std(x)) for x in fields])
        deltas = [sums[f] + (sums[_partner(f, nfields)] if _partner(f, nfields) is not None else 0.0) for f in range(nfields)]
        nbins = LADDER[-1]
        for nb in LADDER:
            if all(np.mean(_slots(x + d, l, h, nb) != _slots(x - d, l, h, nb)) <= 0.01 for x, d, l, h in zip(fields, deltas, lo, hi)):
                nbins = nb
                break
        assert prec == "single" or nbins == 64, (key, nbins)
        _SETUP[key] = (fields, lo, hi, nbins, deltas)
    return _SETUP[key]


def _call(F, a, b, nfields, dealias, lo, hi, nbins, reduce=True):
    from mpifft4py_amd import spectral
    if nfields == 1:
        da, db = F.empty_complex().set(a[0]), None
    else:
        da, db = F.empty_complex(3).set(a), (F.empty_complex(3).set(b) if nfields == 6 else None)
    return spectral.real_histogram(F, da, db, dealias, bins=nbins, range=np.stack([lo, hi], 1), reduce=reduce), da, db


def _plan_case(F, N, prec, dealias, nfields, fused):
    a, b = _reference(N, prec, dealias)[:2]
    fields, lo, hi, nbins, deltas = _setup(N, prec, dealias, nfields)
    h, da, db = _call(F, a, b, nfields, dealias, lo, hi, nbins)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    got = _raw(h)
    assert h.count == fields[0].size and got.shape == (nfields, nbins + 3) and h.counts.dtype == np.int64
    for f in range(nfields):
        _bracket(got[f], fields[f], deltas[f], lo[f], hi[f], nbins, "%s %s %s nfields=%d field %d" % (list(N), prec, dealias, nfields, f))
    assert np.array_equal(da.get(), a[0] if nfields == 1 else a) and (db is None or np.array_equal(db.get(), b))      # inputs preserved
    from mpifft4py_amd import spectral
    again = spectral.real_histogram(F, da, db, dealias, bins=nbins, range=np.stack([lo, hi], 1))
    assert np.array_equal(_raw(again), got) and again.count == h.count                                              # identical arrays
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_histogram_one_rank_fused(N, dealias, nfields, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, nfields, True)


def test_real_histogram_pitched_plan_with_nans_between_rows():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert F.complex_pitch > F.complex_shape()[-1]
    G = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    for dealias in ("3/2-rule", "2/3-rule", None):
        a, b = _reference(N, prec, dealias)[:2]
        fields, lo, hi, nbins, deltas = _setup(N, prec, dealias, 6)
        da, db = F.empty_complex(3), F.empty_complex(3)
        for d in (da, db):                                                         # NaNs between the rows
            whole = DeviceArray(d.shape[:-1] + (F.complex_pitch,), d.dtype, ptr=d.ptr, owner=False)
            whole.set(np.full(whole.shape, np.nan + 1j * np.nan, dtype=d.dtype))
        da.set(a), db.set(b)
        h = spectral.real_histogram(F, da, db, dealias, bins=nbins, range=np.stack([lo, hi], 1))
        assert F.plan_info(INFO(dealias)) == 1
        got = _raw(h)
        for f in range(6):
            _bracket(got[f], fields[f], deltas[f], lo[f], hi[f], nbins, "pitched %s field %d" % (dealias, f))
        compact, _, _ = _call(G, a, b, 6, dealias, lo, hi, nbins)
        print("pitched against compact rows (%s): %d counts differ" % (dealias, int(np.sum(_raw(compact) != got))))


def test_real_histogram_nonfinite_marks_its_field_only():
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua = _reference(N, prec, None)[:3]
    _, lo, hi, nbins, _ = _setup(N, prec, None, 6)
    clean = _raw(_call(F, a, b, 6, None, lo, hi, nbins)[0])
    keep = [0, 1, 3, 4, 5]
    for bad in (np.nan, np.inf):
        an = a.copy()
        an[2, 3, 5, 7] = bad
        got = _raw(_call(F, an, b, 6, None, lo, hi, nbins)[0])
        assert got[2, -1] >= 1 and got[2].sum() == ua[0].size, got[2]
        # every z row whose (x, y) transforms met the bad bin is non-finite in ITS field; the others: the clean run's counts
        assert np.array_equal(got[keep], clean[keep])


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    return nl.run_child("import test_gpu_real_histogram as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_real_histogram_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB (nine or ten batches, the last one ragged): the counts accumulate over the
    batches; totals exact."""
    _child("""
N = [40, 32, 64]
F = Slab_R2C(np.array(N), L, SelfComm(0), 'double')
for nfields in (6, 1, 3):
    t._plan_case(F, N, 'double', '3/2-rule', nfields, True)
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_real_histogram_composed_kill_switch():
    """MFFT_NO_NLZ=1: one field at a time through the plan's inverse transform into ONE real work array and the sweep."""
    _child("""
for N in ([8, 16, 32], [16, 32, 24]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for nfields in (6, 1, 3):
                t._plan_case(F, N, prec, dealias, nfields, False)
            one = int(np.prod([3 * n // 2 for n in N])) * (8 if prec == 'double' else 4)
            assert F.plan_info('nonlinear_bytes') == one, (F.plan_info('nonlinear_bytes'), one)
print('ok')
""", MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_real_histogram_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan): every rank's counts EQUAL numpy's of the real fields its own
    ifftn gives (the sweep is exact), the reduced ones are their sum and identical on every rank."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 24])
    lo, hi, nbins = np.full(6, -0.02), np.full(6, 0.06), 48

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(50 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a, b = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.25), x.component(i))
        u = DeviceArray.empty(ws, F.float)
        mine = []
        for x in (a, b):
            for i in range(3):
                F.ifftn(x.component(i), u, dealias)
                mine.append(_hist(u.get(), lo[0], hi[0], nbins))
        local = spectral.real_histogram(F, a, b, dealias, bins=nbins, range=(lo[0], hi[0]), reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == int(np.prod(ws))
        glob = spectral.real_histogram(F, a, b, dealias, bins=nbins, range=(lo[0], hi[0]))
        return np.stack(mine), _raw(local), _raw(glob), glob.count, local.count

    res = run_ranks(4, work)
    for mine, local, g, cnt, lcnt in res:
        assert np.array_equal(local, mine)
        assert np.array_equal(g, res[0][2]) and cnt == sum(r[4] for r in res)
    assert np.array_equal(np.sum([r[1] for r in res], 0), res[0][2])
    assert np.all(res[0][2].sum(1) == res[0][3])


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[32, 64, 128], [8, 16, 32]])
def test_real_histogram_ranks_fused_identical_to_one_rank(N, dealias):
    """Fused P = 1, 2 and 4 give IDENTICAL int64 arrays (each row's transforms are the same arithmetic whichever rank runs
    them), bracketed once; `reduce` gives the same arrays on every rank, the local ones add up to them."""
    from mpifft4py_amd import DeviceArray, SelfComm, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua = _reference(N, "double", dealias)[:3]
    fields, lo, hi, nbins, _ = _setup(N, "double", dealias, 6)
    rngs = np.stack([lo, hi], 1)
    one = _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), "double"), N, "double", dealias, 6, True)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_histogram(F, da, db, dealias, bins=nbins, range=rngs, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_histogram(F, da, db, dealias, bins=nbins, range=rngs)
        three = spectral.real_histogram(F, da, None, dealias, bins=nbins, range=rngs[:3])
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return _raw(local), local.count, _raw(glob), glob.count, _raw(three)

    for P in (2, 4):
        out = run_ranks(P, work)
        planes = ua.shape[1] // P
        for r, (local, lcount, glob, gcount, three) in enumerate(out):
            assert lcount == fields[0][r * planes:(r + 1) * planes].size and gcount == fields[0].size
            assert np.all(local.sum(1) == lcount) and np.all(three.sum(1) == gcount)
            assert np.array_equal(glob, out[0][2])                               # identical on all ranks
        assert np.array_equal(np.sum([o[0] for o in out], 0), out[0][2])         # local counts add up to the reduced ones
        differ = int(np.sum(out[0][2] != one))
        print("%s %s P=%d against P=1: %d counts differ" % (N, dealias, P, differ))
        assert np.array_equal(out[0][2], one)


# ---- range=None -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_range_none_takes_the_extremes(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = [8, 16, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua, ub, _ = _reference(N, prec, None)
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    h = spectral.real_histogram(F, da, db, None, bins=16)
    m = spectral.real_moments(F, da, db, None)
    print("range=None %s: lo %s hi %s first bins %s last bins %s" % (prec, h.lo, h.hi, h.counts[:, 0], h.counts[:, -1]))
    assert np.all(h.below == 0) and np.all(h.above == 0) and np.all(h.nonfinite == 0)
    assert np.all(h.counts[:, 0] >= 1) and np.all(h.counts[:, -1] >= 1) and np.all(h.counts.sum(1) == h.count)
    assert np.array_equal(h.lo, m.min) and np.all(h.hi > m.max)
    const = F.empty_complex().set(np.zeros(tuple(F.complex_shape()), dtype=cdtype(prec)))
    const_host = const.get()
    const_host[0, 0, 0] = 2.5 * np.prod(N)
    h = spectral.real_histogram(F, const.set(const_host), None, None, bins=5)
    assert h.lo[0] == 2.0 and h.hi[0] == 3.0 and h.counts[0, 2] == h.count and h.below[0] == h.above[0] == 0
    x = DeviceArray.from_numpy((np.random.default_rng(1).random((3, 8, 16, 32)) - 0.5).astype(rdtype(prec)))
    hs = spectral.histogram(F, x, bins=16)
    assert np.all(hs.below == 0) and np.all(hs.above == 0) and np.all(hs.counts[:, 0] >= 1) and np.all(hs.counts[:, -1] >= 1)


# ---- known answer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["2/3-rule", None])
def test_taylor_green_known_histogram(dealias):
    """u_0 = sin x cos y cos z at N = 32: the histogram over [-1, 1] matches the counts of the analytic field on the grid.  With 8
    bins the 0 of the field -- half of all points -- sits on an edge and rounding decides its side; 7 bins avoid that tie, and a
    range wider than [-1, 1] by 2^-20 at either end the ties of the extremes -1 and 1 with lo and hi.  The distance of the analytic
    values from the nearest edge is asserted (in bins: 1e-6 at least); the transform's error is 1e-15."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([32, 32, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    x = np.arange(32) * 2 * np.pi / 32
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    u = np.sin(X) * np.cos(Y) * np.cos(Z)
    U = F.empty_complex()
    F.fftn(DeviceArray.from_numpy(u), U)
    lo, hi, nbins = -1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 7
    t = (u - lo) * (nbins / (hi - lo))
    edge = float(np.min(np.abs(t - np.rint(t))))
    print("Taylor-Green: nearest value to an edge, in bins: %.3e" % edge)
    assert edge > 1e-6
    h = spectral.real_histogram(F, U, None, dealias, bins=nbins, range=(lo, hi))
    assert F.plan_info(INFO(dealias)) == 1
    want = _hist(u, lo, hi, nbins)
    print("Taylor-Green (%s): %s" % (dealias, _raw(h)[0]))
    assert np.array_equal(_raw(h)[0], want) and h.count == 32 ** 3
    assert np.array_equal(h.counts[0], h.counts[0][::-1])      # an odd field on a symmetric grid


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_pdf():
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--pdf", "--steps", "2"]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"^pdf\s+(\S+)\s+(\S+)\s*$", r.stdout, re.M)
    tails = re.search(r"outside the range: ([0-9.eE+-]+)", r.stdout)
    width = re.search(r"bin width ([0-9.eE+-]+)", r.stdout)
    assert len(rows) >= 8 and tails and width, r.stdout
    p = np.array([float(v) for _, v in rows])
    integral = float(np.sum(p) * float(width.group(1)))
    print("example --pdf: integral %.15f, tails %s" % (integral, tails.group(1)))
    assert np.all(p >= 0) and abs(integral - (1.0 - float(tails.group(1)))) <= 1e-12
    # no other output changes: the lines of the run without --pdf come first and unchanged -- the timing apart, and numbers to nine
    # digits (the example's energy is summed in an order that varies from run to run in the last two)
    plain = subprocess.run(exe[:4] + exe[5:], capture_output=True, text=True, timeout=280)
    assert plain.returncode == 0 and "pdf" not in plain.stdout.lower(), plain.stdout + plain.stderr
    nine = lambda l: re.sub(r"-?\d+\.\d+(?:[eE][-+]?\d+)?", lambda m: "%.9g" % float(m.group(0)), l)
    steady = lambda out: [nine(l) for l in out.splitlines() if "ms per step" not in l]
    assert steady(r.stdout)[:len(steady(plain.stdout))] == steady(plain.stdout)
