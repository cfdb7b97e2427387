"""GPU: joint histograms of two spectral fields without the real-space arrays (mfft_real_joint_histogram, mfft_nlz_joint_rows,
mfft_ew_joint_histogram; csrc/nlz_joint.h NlzJoint::body, csrc/joint.hip) -- the sweep against numpy exactly, the z stage on known
answers exactly and on random spectra by brackets, the plan operation on every route (fused on one rank and several, batches,
composed, pencils, pitched), `range=None`, `a_hat is b_hat`, the marginals against `real_histogram` and the example's --joint.

Counts have no tolerance.  Where the values come from a transform they are compared by TWO-DIMENSIONAL BRACKETS: the cell rule
(include/mpifft4py_amd.h: cell = sa (nbb + 3) + sb, the slots by the rule of the histograms) is monotone in each argument, so with
|x_device - x_ref| <= delta on both fields every cumulative count obeys
    C_ij(x_ref + delta) <= C_ij(device) <= C_ij(x_ref - delta),   i <= nba + 1,  j <= nbb + 1,
C_ij = the points with sa <= i and sb <= j; the total equals the number of points and the non-finite row and column are 0.  delta
is the worst-case bound of tests/test_gpu_real_histogram.py over BOTH fields of the pair (they share the transform).  Asserted
from the reference alone: at most 2 % of the points change their CELL between x_ref - delta and x_ref + delta -- the union of the
two fields' one-dimensional shares, each of which the histogram tests hold to 1 % on these draws and bin counts."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
import test_gpu_real_histogram as rh
from gpu_util import L, cdtype, have_gpu, rdtype, run_ranks
from test_gpu_real_histogram import _irfft_rows, _row_delta, _slots

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
MAXBINS = 64


def INFO(dealias):
    return "nonlinear_joint_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _cells(xa, xb, lo, hi, nba, nbb):
    """The cell rule, numpy float64: lo, hi = (a, b)."""
    return _slots(xa, lo[0], hi[0], nba) * (nbb + 3) + _slots(xb, lo[1], hi[1], nbb)


def _grid(xa, xb, lo, hi, nba, nbb):
    return np.bincount(_cells(xa, xb, lo, hi, nba, nbb).ravel(), minlength=(nba + 3) * (nbb + 3)).astype(np.int64).reshape(nba + 3, nbb + 3)


def _cum(g):
    return np.cumsum(np.cumsum(g, axis=0), axis=1)


def _bracket2(got, xa, xb, delta, lo, hi, nba, nbb, what):
    """got: the (nba + 3, nbb + 3) device counts of one pair; xa, xb: its reference values; delta: the bound, broadcastable."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    got = np.asarray(got, dtype=np.int64)
    cu, cd = _cells(xa + delta, xb + delta, lo, hi, nba, nbb), _cells(xa - delta, xb - delta, lo, hi, nba, nbb)
    share = float(np.mean(cu != cd))
    ncell = (nba + 3) * (nbb + 3)
    up = _cum(np.bincount(cu.ravel(), minlength=ncell).reshape(nba + 3, nbb + 3))[:nba + 2, :nbb + 2]
    dn = _cum(np.bincount(cd.ravel(), minlength=ncell).reshape(nba + 3, nbb + 3))[:nba + 2, :nbb + 2]
    cg = _cum(got)[:nba + 2, :nbb + 2]
    print("joint %s: %d points, delta max %.3e, cell changes within +-delta %.4f %%, cumulative slack below %d above %d"
          % (what, xa.size, float(np.max(delta)), 100 * share, int(np.min(cg - up)), int(np.min(dn - cg))))
    assert share <= 0.02, (what, share)
    assert got.sum() == xa.size and got[nba + 2].sum() == 0 and got[:, nbb + 2].sum() == 0, (what, got.sum(), xa.size)
    assert np.all(up <= cg) and np.all(cg <= dn), (what, np.argwhere((up > cg) | (cg > dn))[:4])


# ---- 1. the sweep: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape", [(3, 8, 16, 32), (1, 7, 9, 15)])
def test_sweep_equals_numpy(shape, prec):
    """spectral.joint_histogram of random real arrays with values placed exactly on edges, at lo, at hi, +-Inf and NaN in either
    array EQUALS numpy evaluating the cell rule in float64; (1, 7, 9, 15) has 945 elements, so heads and tails of the 16-byte
    lanes are met."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(17 + shape[0])
    x = (3.0 * rng.standard_normal(shape)).astype(rdtype(prec))
    y = (2.0 * rng.standard_normal(shape)).astype(rdtype(prec))
    lo, hi = (-4.0, -2.0), (4.0, 6.0)                 # edges at multiples of 1/8: exact in both precisions
    fx, fy = x.reshape(shape[0], -1), y.reshape(shape[0], -1)
    n = fx.shape[1]
    for c in range(shape[0]):
        for f, l, h in ((fx, lo[0], hi[0]), (fy, lo[1], hi[1])):
            special = [l, h, l + 0.125, 0.0, 0.125, h - 0.125, np.nextafter(rdtype(prec)(h), rdtype(prec)(0)), np.inf, -np.inf, np.nan, np.nan]
            where = rng.choice(n, len(special), replace=False)
            where[:3] = [0, n - 1, n // 2]               # the first, the last and a middle element among them
            f[c, where] = special
    for bins, rngs in (((64, 64), [(lo, hi)] * shape[0]), ((37, 5), [((-1.0 - 0.1 * c, -0.7), (2.0 + 0.3 * c, 1.9)) for c in range(shape[0])])):
        nba, nbb = bins
        r = np.array([[[l[0], h[0]], [l[1], h[1]]] for l, h in rngs])      # [pair][a, b][lo, hi]
        want = np.stack([_grid(fx[c], fy[c], rngs[c][0], rngs[c][1], nba, nbb) for c in range(shape[0])])
        assert np.array_equal(want, np.stack([np.bincount(spectral.joint_cells(fx[c], fy[c], rngs[c][0], rngs[c][1], bins),
                                                          minlength=want[c].size).reshape(want[c].shape) for c in range(shape[0])]))
        h = spectral.joint_histogram(F, DeviceArray.from_numpy(x), DeviceArray.from_numpy(y), bins=bins, range=r)
        print("sweep %s %s %s: outside %s" % (shape, prec, bins, [h.outside(p) for p in range(shape[0])]))
        assert h.count == n and h.raw.dtype == np.int64 and h.raw.shape == (shape[0], nba + 3, nbb + 3)
        assert np.array_equal(h.raw, want), np.argwhere(h.raw != want)[:5]
        assert np.all(h.raw.sum((1, 2)) == n) and np.all(h.raw[:, -1, :].sum(1) >= 1) and np.all(h.raw[:, :, -1].sum(1) >= 1)
    if shape[0] == 3:
        # an array that starts off 16 bytes from its partner: taken singly, the same counts
        off = DeviceArray.from_numpy(np.concatenate([np.zeros(1, dtype=x.dtype), x.ravel()]))
        view = DeviceArray(x.shape, x.dtype, ptr=off.ptr + x.dtype.itemsize, owner=False)
        h2 = spectral.joint_histogram(F, view, DeviceArray.from_numpy(y), bins=bins, range=r)
        assert np.array_equal(h2.raw, want)
        pitched = DeviceArray.from_numpy(x)
        view = DeviceArray(pitched.shape, pitched.dtype, ptr=pitched.ptr, owner=False)
        view.pitch = 40
        with pytest.raises(ValueError):
            spectral.joint_histogram(F, view, DeviceArray.from_numpy(y), bins=8, range=r)
        with pytest.raises(ValueError):
            spectral.joint_histogram(F, DeviceArray.from_numpy(x), DeviceArray.from_numpy(y), bins=(65, 8), range=r)


# ---- the stage alone --------------------------------------------------------------------------------------------------
# The lengths of the histogram tests: 16 and 512 are wave-synchronous builds, 1024 a barrier build; 768 in double precision is a
# kernel whose exchange the LDS rule of the joint kernels changes (csrc/registry_nlz.h nlj_split: split, hence a barrier build),
# 3072 in double precision the split kernel that keeps one resident workgroup next to the grid.
LENGTHS = [16, 512, 768, 1024, 3072]


def _rows_call(a, b, ncomp, nrows, n, pitch, valid, valid_in, prec, lo, hi, nba, nbb):
    """a, b: (ncomp, nrows, pitch) (or (nrows, pitch)); lo, hi: (2 ncomp,), a_0.., then b_0..  Returns (ncomp, nba + 3, nbb + 3)."""
    from mpifft4py_amd import DeviceArray, _lib
    da, db = DeviceArray.from_numpy(a), DeviceArray.from_numpy(b)
    got = np.full((ncomp, nba + 3, nbb + 3), -1, dtype=np.int64)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (2 * ncomp,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (2 * ncomp,)))
    _lib.call("mfft_nlz_joint_rows", da.ptr, db.ptr, ncomp, nrows, n, pitch, valid, valid_in, _lib.precision_code(prec),
              lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nba, nbb, got.ctypes.data_as(IP))
    assert da.get().tobytes() == a.tobytes() and db.get().tobytes() == b.tobytes()      # inputs preserved
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS + [4096])          # (4096: in double precision the one kernel that keeps its twin's exchange by exception)
def test_stage_known_answers_exact(n, prec):
    """The three known rows of the histogram test as a -- the constant 2, 1 + 2 (-1)^j, 3 cos(pi j / 2) = {3, 0, -3, 0} -- and
    the same set rotated by one component as b.  9 x 9 bins of width 1 over [-4.5, 4.5)^2: every value sits half a bin from an
    edge, so the cells are exact.  Pair 0 = (2, 3 | -1): two cells of nrows n / 2; pair 1 = (3 | -1, {3, 0, -3, 0}): (3, 3) and
    (3, -3) hold nrows n / 4 each, (-1, 0) nrows n / 2; pair 2 = ({3, 0, -3, 0}, 2): (3, 2) and (-3, 2) nrows n / 4, (0, 2) nrows n / 2."""
    nrows, valid, nb = 5, n // 2 + 1, 9
    a = np.zeros((3, nrows, valid + 3), dtype=cdtype(prec))
    a[0, :, 0] = 2.0 * n
    a[1, :, 0] = 1.0 * n
    a[1, :, n // 2] = 2.0 * n
    a[2, :, n // 4] = 1.5 * n
    b = np.ascontiguousarray(np.roll(a, -1, axis=0))
    got = _rows_call(a, b, 3, nrows, n, valid + 3, valid, 0, prec, -4.5, 4.5, nb, nb)
    want = np.zeros((3, nb + 3, nb + 3), dtype=np.int64)
    slot = lambda v: 1 + int(v + 4.5)
    P = nrows * n
    want[0, slot(2), slot(3)] = want[0, slot(2), slot(-1)] = P // 2
    want[1, slot(3), slot(3)] = want[1, slot(3), slot(-3)] = P // 4
    want[1, slot(-1), slot(0)] = P // 2
    want[2, slot(3), slot(2)] = want[2, slot(-3), slot(2)] = P // 4
    want[2, slot(0), slot(2)] = P // 2
    print("known answers n=%d %s: cells %s" % (n, prec, [np.argwhere(g).tolist() for g in got]))
    assert np.array_equal(got, want)
    ra, rb = _irfft_rows(a, n, valid), _irfft_rows(b, n, valid)
    assert np.array_equal(want, np.stack([_grid(ra[p], rb[p], (-4.5, -4.5), (4.5, 4.5), nb, nb) for p in range(3)]))      # (the reference agrees)


_ROWS_PER_PASS = {}


def _pass_shape(n, prec):
    """(workgroups of a full launch, rows one workgroup takes per pass) from mfft_nlz_joint_groups alone."""
    from mpifft4py_amd import _lib
    if (n, prec) not in _ROWS_PER_PASS:
        code = _lib.precision_code(prec)
        cap = _lib.call("mfft_nlz_joint_groups", 1 << 40, n, code)
        per = 1
        while _lib.call("mfft_nlz_joint_groups", per + 1, n, code) == 1:      # rows per workgroup: a power of two
            per *= 2
        _ROWS_PER_PASS[(n, prec)] = (cap, per)
    return _ROWS_PER_PASS[(n, prec)]


def _stage_random(n, prec, nfields, nrows, valid, valid_in=0, nbins=64):
    """The draws of the histogram test's _stage_random (the same generator and order: seeded Gaussian spectra with real end bins),
    nbins x nbins bins over +-4 sigma of the reference rows; nfields = 2 or 6."""
    rng = np.random.default_rng(100 * n + 7 * nrows % 1000 + valid + nfields)
    pitch = valid + 3
    ncomp = nfields // 2
    shape = (ncomp, nrows, pitch)

    def draw():
        z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype(prec))
        z[..., 0] = z[..., 0].real
        if n % 2 == 0 and valid == n // 2 + 1:
            z[..., valid - 1] = z[..., valid - 1].real
        return z
    a, b = draw(), draw()
    vin = valid_in or valid
    ra, rb = _irfft_rows(a, n, vin), _irfft_rows(b, n, vin)
    delta = _row_delta(a, n, vin, prec) + _row_delta(b, n, vin, prec)      # per pair and row: both fields share the transform
    lo = np.array([-4 * float(np.std(x)) for x in list(ra) + list(rb)])
    hi = -lo
    got = _rows_call(a, b, ncomp, nrows, n, pitch, valid, valid_in, prec, lo, hi, nbins, nbins)
    for p in range(ncomp):
        _bracket2(got[p], ra[p], rb[p], delta[p][:, None], (lo[p], lo[ncomp + p]), (hi[p], hi[ncomp + p]), nbins, nbins,
                  "stage n=%d %s nfields=%d nrows=%d valid=%d/%d pair %d" % (n, prec, nfields, nrows, vin, valid, p))
    return got


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_stage_random_spectra_bracket(n, prec):
    """2 and 6 fields; one row, an odd count, pruned valid_in; a second call gives identical arrays."""
    full, lim = n // 2 + 1, n // 3 + 1
    first = _stage_random(n, prec, 6, 37, full)
    assert np.array_equal(_stage_random(n, prec, 6, 37, full), first)
    _stage_random(n, prec, 2, 37, lim)
    _stage_random(n, prec, 2, 37, full, valid_in=lim)
    if n > 16:                                       # (one row of 16 points has no 64 x 64 PDF to bracket: the odd count covers 16)
        _stage_random(n, prec, 2, 1, full)
    else:
        _stage_random(n, prec, 2, 1, full, nbins=4)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", LENGTHS)
def test_stage_more_than_two_passes_of_the_grid(n, prec):
    """More than two passes of mfft_nlz_joint_groups workgroups and a ragged rest: every workgroup strides, the last pass is partial."""
    from mpifft4py_amd import _lib
    cap, per = _pass_shape(n, prec)
    assert cap >= 1
    nrows = 2 * cap * per + per // 2 + 3
    assert _lib.call("mfft_nlz_joint_groups", nrows, n, _lib.precision_code(prec)) == cap
    _stage_random(n, prec, 2, nrows, n // 2 + 1)


def test_stage_nonfinite_bins():
    """A NaN or an Inf bin in a_1 or in b_1: the bad field's marginal has counts in its non-finite slot, the partner's marginal and
    every other pair EQUAL the clean run."""
    n, nrows, valid, nba, nbb = 128, 5, 65, 31, 17
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    b = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    clean = _rows_call(a, b, 3, nrows, n, valid, valid, 0, "double", -0.5, 0.5, nba, nbb)
    assert np.all(clean.sum((1, 2)) == nrows * n) and np.all(clean[:, -1, :] == 0) and np.all(clean[:, :, -1] == 0)
    for bad in (np.nan, np.inf):
        for which in (0, 1):
            an, bn = a.copy(), b.copy()
            (an, bn)[which][1, 3, 7] = bad
            got = _rows_call(an, bn, 3, nrows, n, valid, valid, 0, "double", -0.5, 0.5, nba, nbb)
            mine, partner = got[1].sum(1 - which), got[1].sum(which)      # marginals of the bad field and of its partner
            print("bad bin %r in %s_1: non-finite slot %d" % (bad, "ab"[which], mine[-1]))
            assert mine[-1] >= 1 and got[1].sum() == nrows * n
            assert np.array_equal(partner, clean[1].sum(which))
            assert np.array_equal(got[[0, 2]], clean[[0, 2]])


def test_stage_error_codes():
    """MFFT_ERR_UNSUPPORTED for a length without a kernel; MFFT_ERR_INVALID for a bin count of 0 or above the maximum (either
    field), hi <= lo, ranges that are not finite, a NULL b and valid > n / 2 + 1: the status codes themselves, and a refused call
    writes nothing."""
    from mpifft4py_amd import DeviceArray, _lib
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    assert int(re.search(r"#define MFFT_JOINT_MAXBINS (\d+)", header).group(1)) == MAXBINS
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    out = np.full((3, 34, 34), -7, dtype=np.int64)
    one, mone = np.ones(6), -np.ones(6)
    inf, nan = np.full(6, np.inf), np.full(6, np.nan)
    fn = getattr(_lib.load(), "mfft_nlz_joint_rows")

    def status(n, valid, nba, nbb, lo, hi, b=z.ptr):
        return fn(z.ptr, b, 3, 4, n, 65, valid, 0, _lib.DOUBLE, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nba, nbb, out.ctypes.data_as(IP))
    cases = [((100, 51, 31, 31, mone, one), "MFFT_ERR_UNSUPPORTED"), ((128, 65, 0, 31, mone, one), "MFFT_ERR_INVALID"),
             ((128, 65, 31, 0, mone, one), "MFFT_ERR_INVALID"), ((128, 65, MAXBINS + 1, 31, mone, one), "MFFT_ERR_INVALID"),
             ((128, 65, 31, MAXBINS + 1, mone, one), "MFFT_ERR_INVALID"), ((128, 65, 31, 31, one, one), "MFFT_ERR_INVALID"),
             ((128, 65, 31, 31, one, mone), "MFFT_ERR_INVALID"), ((128, 65, 31, 31, mone, inf), "MFFT_ERR_INVALID"),
             ((128, 65, 31, 31, nan, one), "MFFT_ERR_INVALID"), ((64, 51, 31, 31, mone, one), "MFFT_ERR_INVALID"),
             ((128, 65, 31, 31, mone, one, None), "MFFT_ERR_INVALID")]
    for args, name in cases:
        rc = status(*args)
        print(args[:4], "->", rc)
        assert rc == codes[name], (args[:4], rc, name)
    assert np.all(out == -7)
    assert status(128, 65, 31, 31, mone, one) == 0
    assert out[:, 16, 16].tolist() == [4 * 128] * 3 and out.sum() == 3 * 4 * 128      # rows of zeros: the cell that holds (0, 0)
    assert _lib.call("mfft_nlz_joint_groups", 4, 100, _lib.DOUBLE) == 0


# ---- the plan operation ---------------------------------------------------------------------------------------------------
def _setup(N, prec, dealias):
    """(fields, lo, hi, nbins, deltas) of the histogram tests' six-field case, from the reference alone: +-4 sigma about each
    field's mean, nbins the largest of 64, 32, .., 2 at which every field meets the 1 % condition with the 3-D delta of its PAIR
    (64 throughout in double precision).  The joint call takes nbins x nbins."""
    return rh._setup(N, prec, dealias, 6)


def _ranges(lo, hi, ncomp):
    """[pair][a, b][lo, hi] for the pairs (field p, field 3 + p) of the six-field setup."""
    return np.array([[[lo[p], hi[p]], [lo[3 + p], hi[3 + p]]] for p in range(ncomp)])


def _call(F, a, b, ncomp, dealias, lo, hi, nbins, reduce=True):
    from mpifft4py_amd import spectral
    if ncomp == 1:
        da, db = F.empty_complex().set(a[0]), F.empty_complex().set(b[0])
    else:
        da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    return spectral.real_joint_histogram(F, da, db, dealias, bins=nbins, range=_ranges(lo, hi, ncomp), reduce=reduce), da, db


def _plan_case(F, N, prec, dealias, ncomp, fused):
    from mpifft4py_amd import spectral
    a, b = rh._reference(N, prec, dealias)[:2]
    fields, lo, hi, nbins, deltas = _setup(N, prec, dealias)
    h, da, db = _call(F, a, b, ncomp, dealias, lo, hi, nbins)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    assert h.count == fields[0].size and h.raw.shape == (ncomp, nbins + 3, nbins + 3) and h.raw.dtype == np.int64
    for p in range(ncomp):
        _bracket2(h.raw[p], fields[p], fields[3 + p], deltas[p], (lo[p], lo[3 + p]), (hi[p], hi[3 + p]), nbins, nbins,
                  "%s %s %s ncomp=%d pair %d" % (list(N), prec, dealias, ncomp, p))
    assert np.array_equal(da.get(), a[0] if ncomp == 1 else a) and np.array_equal(db.get(), b[0] if ncomp == 1 else b)      # inputs preserved
    again = spectral.real_joint_histogram(F, da, db, dealias, bins=nbins, range=_ranges(lo, hi, ncomp))
    assert np.array_equal(again.raw, h.raw) and again.count == h.count                                            # identical arrays
    return h.raw


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_joint_one_rank_fused(N, dealias, ncomp, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, ncomp, True)


def test_real_joint_pitched_plan_with_nans_between_rows():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert F.complex_pitch > F.complex_shape()[-1]
    for dealias in ("3/2-rule", "2/3-rule", None):
        a, b = rh._reference(N, prec, dealias)[:2]
        fields, lo, hi, nbins, deltas = _setup(N, prec, dealias)
        da, db = F.empty_complex(3), F.empty_complex(3)
        for d in (da, db):                                                         # NaNs between the rows
            whole = DeviceArray(d.shape[:-1] + (F.complex_pitch,), d.dtype, ptr=d.ptr, owner=False)
            whole.set(np.full(whole.shape, np.nan + 1j * np.nan, dtype=d.dtype))
        da.set(a), db.set(b)
        h = spectral.real_joint_histogram(F, da, db, dealias, bins=nbins, range=_ranges(lo, hi, 3))
        assert F.plan_info(INFO(dealias)) == 1
        for p in range(3):
            _bracket2(h.raw[p], fields[p], fields[3 + p], deltas[p], (lo[p], lo[3 + p]), (hi[p], hi[3 + p]), nbins, nbins,
                      "pitched %s pair %d" % (dealias, p))


def test_real_joint_errors_leave_the_outputs_untouched():
    """mfft_real_joint_histogram through the C interface: a NULL b_hat, bins outside 1 .. 64, hi <= lo and ranges that are not
    finite are MFFT_ERR_INVALID, reported before anything is enqueued: out and count keep their values."""
    from mpifft4py_amd import SelfComm, Slab_R2C, _lib, spectral
    from mpifft4py_amd._base import _DEALIAS
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), "double")
    F.comm.use_device()
    da = F.empty_complex(3).set(np.zeros((3,) + tuple(F.complex_shape()), dtype=np.complex128))
    out = np.full((3, 11, 11), -7, dtype=np.int64)
    count = ctypes.c_int64(-5)
    fn = getattr(_lib.load(), "mfft_real_joint_histogram")
    one, mone = np.ones(6), -np.ones(6)

    def status(b, nba, nbb, lo, hi):
        return fn(F._plan, da.ptr, b, 3, _DEALIAS[None], lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), nba, nbb, out.ctypes.data_as(IP), ctypes.byref(count))
    for args in ((None, 8, 8, mone, one), (da.ptr, 0, 8, mone, one), (da.ptr, 8, 65, mone, one), (da.ptr, 8, 8, one, mone),
                 (da.ptr, 8, 8, one, one), (da.ptr, 8, 8, mone, np.full(6, np.inf)), (da.ptr, 8, 8, np.full(6, np.nan), one)):
        assert status(*args) == codes["MFFT_ERR_INVALID"], args[:3]
    assert np.all(out == -7) and count.value == -5
    assert status(da.ptr, 8, 8, mone, one) == 0 and count.value == 8 * 16 * 32 and out[:, 5, 5].tolist() == [count.value] * 3
    with pytest.raises(ValueError):
        spectral.real_joint_histogram(F, da, None, None, bins=8, range=((-1, 1), (-1, 1)))
    with pytest.raises(ValueError):
        spectral.real_joint_histogram(F, da, da, None, bins=(8, 65), range=((-1, 1), (-1, 1)))


def test_real_joint_nonfinite_marks_its_field_only():
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec = [8, 16, 32], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua = rh._reference(N, prec, None)[:3]
    _, lo, hi, nbins, _ = _setup(N, prec, None)
    clean = _call(F, a, b, 3, None, lo, hi, nbins)[0].raw
    for bad in (np.nan, np.inf):
        an = a.copy()
        an[2, 3, 5, 7] = bad
        got = _call(F, an, b, 3, None, lo, hi, nbins)[0].raw
        assert got[2].sum(1)[-1] >= 1 and got[2].sum() == ua[0].size
        assert np.array_equal(got[2].sum(0), clean[2].sum(0))      # b_2 rides on the same transform: exactly its clean marginal
        assert np.array_equal(got[:2], clean[:2])


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    return nl.run_child("import test_gpu_real_joint as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_real_joint_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB (the last one ragged): the counts accumulate over the batches."""
    _child("""
N = [40, 32, 64]
F = Slab_R2C(np.array(N), L, SelfComm(0), 'double')
for ncomp in (3, 1):
    t._plan_case(F, N, 'double', '3/2-rule', ncomp, True)
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_real_joint_composed_kill_switch():
    """MFFT_NO_NLZ=1: a_p and b_p through the plan's inverse transform into TWO real work arrays, then the sweep; the same brackets."""
    _child("""
for N in ([8, 16, 32], [16, 32, 24]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for ncomp in (3, 1):
                t._plan_case(F, N, prec, dealias, ncomp, False)
print('ok')
""", MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_real_joint_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan): every rank's counts EQUAL numpy's of the real fields its own
    ifftn gives (the sweep is exact), the reduced ones are their sum and identical on every rank."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 24])
    lo, hi, bins = (-0.02, -0.03), (0.06, 0.05), (48, 11)
    r = ((lo[0], hi[0]), (lo[1], hi[1]))

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(50 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a, b = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.25), x.component(i))
        u = DeviceArray.empty(ws, F.float)
        real = []
        for x in (a, b):
            for i in range(3):
                F.ifftn(x.component(i), u, dealias)
                real.append(u.get().copy())
        mine = np.stack([_grid(real[p], real[3 + p], lo, hi, *bins) for p in range(3)])
        local = spectral.real_joint_histogram(F, a, b, dealias, bins=bins, range=r, reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and local.count == int(np.prod(ws))
        glob = spectral.real_joint_histogram(F, a, b, dealias, bins=bins, range=r)
        return mine, local.raw, glob.raw, glob.count, local.count

    res = run_ranks(4, work)
    for mine, local, g, cnt, lcnt in res:
        assert np.array_equal(local, mine)
        assert np.array_equal(g, res[0][2]) and cnt == sum(x[4] for x in res)
    assert np.array_equal(np.sum([x[1] for x in res], 0), res[0][2])
    assert np.all(res[0][2].sum((1, 2)) == res[0][3])


# ---- several ranks, fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[32, 64, 128], [8, 16, 32]])
def test_real_joint_ranks_fused_identical_to_one_rank(N, dealias):
    """Fused P = 1, 2 and 4 give IDENTICAL int64 arrays, bracketed once; `reduce` gives the same arrays on every rank, the local
    ones add up to them."""
    from mpifft4py_amd import DeviceArray, SelfComm, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b, ua = rh._reference(N, "double", dealias)[:3]
    fields, lo, hi, nbins, _ = _setup(N, "double", dealias)
    rngs = _ranges(lo, hi, 3)
    one = _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), "double"), N, "double", dealias, 3, True)

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        local = spectral.real_joint_histogram(F, da, db, dealias, bins=nbins, range=rngs, reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        glob = spectral.real_joint_histogram(F, da, db, dealias, bins=nbins, range=rngs)
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return local.raw, local.count, glob.raw, glob.count

    for P in (2, 4):
        out = run_ranks(P, work)
        planes = ua.shape[1] // P
        for r, (local, lcount, glob, gcount) in enumerate(out):
            assert lcount == fields[0][r * planes:(r + 1) * planes].size and gcount == fields[0].size
            assert np.all(local.sum((1, 2)) == lcount)
            assert np.array_equal(glob, out[0][2])                               # identical on all ranks
        assert np.array_equal(np.sum([o[0] for o in out], 0), out[0][2])         # local counts add up to the reduced ones
        print("%s %s P=%d against P=1: %d counts differ" % (N, dealias, P, int(np.sum(out[0][2] != one))))
        assert np.array_equal(out[0][2], one)


# ---- range=None, a_hat is b_hat, marginals -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_range_none_puts_every_point_inside(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = [8, 16, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b = rh._reference(N, prec, None)[:2]
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    h = spectral.real_joint_histogram(F, da, db, None, bins=(16, 9))
    m = spectral.real_moments(F, da, db, None)
    print("range=None %s: lo %s hi %s" % (prec, h.lo.tolist(), h.hi.tolist()))
    assert all(h.outside(p) == 0 for p in range(3)) and np.all(h.counts.sum((1, 2)) == h.count)
    assert np.array_equal(h.lo[:, 0], m.min[:3]) and np.array_equal(h.lo[:, 1], m.min[3:]) and np.all(h.hi[:, 0] > m.max[:3]) and np.all(h.hi[:, 1] > m.max[3:])
    assert np.all(h.counts.sum(2)[:, 0] >= 1) and np.all(h.counts.sum(2)[:, -1] >= 1) and np.all(h.counts.sum(1)[:, 0] >= 1) and np.all(h.counts.sum(1)[:, -1] >= 1)
    x = DeviceArray.from_numpy((np.random.default_rng(1).random((3, 8, 16, 32)) - 0.5).astype(rdtype(prec)))
    y = DeviceArray.from_numpy((np.random.default_rng(2).random((3, 8, 16, 32)) * 3).astype(rdtype(prec)))
    hs = spectral.joint_histogram(F, x, y, bins=16)
    assert all(hs.outside(p) == 0 for p in range(3)) and hs.count == 8 * 16 * 32


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_a_hat_is_b_hat(dealias):
    """The same array as both fields is accepted; the marginals bracket as usual."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, sums = rh._reference(N, prec, dealias)[0], rh._reference(N, prec, dealias)[4]
    fields, lo, hi, nbins, _ = _setup(N, prec, dealias)
    da = F.empty_complex(3).set(a)
    r = np.array([[[lo[p], hi[p]], [lo[p], hi[p]]] for p in range(3)])
    h = spectral.real_joint_histogram(F, da, da, dealias, bins=nbins, range=r)
    assert F.plan_info(INFO(dealias)) == 1 and np.array_equal(da.get(), a)
    for p in range(3):
        # (the real and the imaginary part of the transform of a + i a are not the same arithmetic: a point next to an edge may
        # leave the diagonal by one bin; counted and printed)
        print("a_hat is b_hat %s pair %d: %d points off the diagonal" % (dealias, p, h.raw[p].sum() - np.trace(h.raw[p])))
        assert h.raw[p].sum() == h.count
        for axis in (0, 1):                              # the pair's delta: the field rides with itself
            rh._bracket(h.raw[p].sum(1 - axis), fields[p], 2 * sums[p], lo[p], hi[p], nbins, "a is b %s pair %d axis %d" % (dealias, p, axis))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
def test_marginals_against_real_histogram(dealias, prec):
    """The marginals of the fused joint result and spectral.real_histogram on the same fields, ranges and bins lie inside the same
    brackets; whether they are bitwise equal is PRINTED, not asserted (both bodies run the same transform code, but the compiler's
    contraction choices across two instantiations are not under the test's control)."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = [32, 64, 128]
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b = rh._reference(N, prec, dealias)[:2]
    fields, lo, hi, nbins, deltas = _setup(N, prec, dealias)
    hj, da, db = _call(F, a, b, 3, dealias, lo, hi, nbins)
    h1 = rh._raw(spectral.real_histogram(F, da, db, dealias, bins=nbins, range=np.stack([lo, hi], 1)))
    mj = np.concatenate([rh._raw(hj.marginal(0)), rh._raw(hj.marginal(1))])
    for f in range(6):
        rh._bracket(mj[f], fields[f], deltas[f], lo[f], hi[f], nbins, "marginal %s %s field %d" % (dealias, prec, f))
        rh._bracket(h1[f], fields[f], deltas[f], lo[f], hi[f], nbins, "real_histogram %s %s field %d" % (dealias, prec, f))
    print("marginals of the joint result against real_histogram (%s, %s, %d bins): bitwise equal: %s (%d counts differ)"
          % (dealias, prec, nbins, np.array_equal(mj, h1), int(np.sum(mj != h1))))


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_joint():
    exe = [sys.executable, os.path.join(ROOT, "examples", "boussinesq_device.py"), "--M", "5", "--joint", "--steps", "2"]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"^joint step (\d+): corr\(u_z, theta\) = (\S+)\s+<u_z \| theta> = \[([^\]]*)\]\s+total = (\d+)\s*$", r.stdout, re.M)
    print(r.stdout)
    assert len(rows) == 2, r.stdout
    points = (3 * 32 // 2) ** 3                      # the example's default is the 3/2-rule: the padded grid is counted
    for step, corr, cond, total in rows:
        assert int(total) == points and -1.0 <= float(corr) <= 1.0 and len(cond.split(",")) == 5
    none = subprocess.run(exe + ["--dealias", "None"], capture_output=True, text=True, timeout=280)
    assert none.returncode == 0 and [int(t) for t in re.findall(r"total = (\d+)", none.stdout)] == [32 ** 3] * 2, none.stdout + none.stderr
