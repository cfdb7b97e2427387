"""GPU: moments and PDFs of quadratic forms q = sum_f w_f ifftn(field f)^2 without the real-space arrays (mfft_real_quadratic,
mfft_nlz_quad_rows, mfft_ew_quadratic, mfft_ew_strain_hat; csrc/nlz_quad.h NlzQuad::body, csrc/quad.hip) -- the sweep against numpy
(counts exactly), the z stage on known answers exactly and on random spectra by bounds, the plan operation on every route (fused
on one rank and several, batches, composed, pencils, pitched), `range=None`, Taylor-Green known answers, the strain tensor, the
identity with the enstrophy spectrum and the example's --dissipation.

Bounds, from the reference alone.  With r the oracle's float64 fields and delta_f the worst-case bound of field f's transform
(test_gpu_real_histogram.py: `_row_delta` for rows, the 3-D sum for plans, the partner on the transform included), pointwise
    dq = sum_f |w_f| (2 |r_f| delta_f + delta_f^2) + (n + 1) 2^-53 sum_f |w_f| r_f^2          (n fields)
and with d = q - c:  min and max within max dq;  |S_p - ref| <= sum p dq (|d| + dq)^(p - 1) + (cnt + 8) 2^-52 sum |d|^p;  the
cumulative counts lie between those of q + dq and q - dq (the slot rule is monotone).  Asserted from the reference alone: at most
1 % of the points change their slot between q - dq and q + dq.  Ranges are hi = mean + 4 sigma, lo = -hi / 8: zero is the mode of
q and must not be a bin edge."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nonlinear_util as nl
import test_gpu_real_histogram as th
from gpu_util import L, cdtype, have_gpu, rdtype, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int64)
LD = np.longdouble
WEIGHTS = {1: [1.0], 2: [1.0, 3.0], 3: [1.0, 1.0, 1.0], 6: [1.0, 1.0, 1.0, 2.0, 2.0, 2.0]}


def INFO(dealias):
    return "nonlinear_quadratic_fused_%s" % nl.RULE[dealias]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _q_and_dq(fields, w, deltas):
    """(q in long double, dq in float64) of the reference fields r_f (float64), weights and per-field bounds (broadcastable)."""
    q = np.zeros(np.shape(fields[0]), dtype=LD)
    dq = np.zeros(np.shape(fields[0]), dtype=np.float64)
    wr2 = np.zeros(np.shape(fields[0]), dtype=np.float64)
    for r, wf, d in zip(fields, w, deltas):
        r = np.asarray(r, dtype=np.float64)
        q += LD(wf) * r.astype(LD) ** 2
        wr2 += abs(wf) * r * r
        dq += abs(wf) * (2 * np.abs(r) * d + d * d)
    return q, dq + (len(fields) + 1) * 2.0 ** -53 * wr2


def _raw(h):
    return np.concatenate([h.below, h.counts[0], h.above, h.nonfinite]).astype(np.int64)


def _check_moments(got6, q, dq, center, what):
    """got6 = [min, max, S1 .. S4] of the device against q (long double) within the bound above."""
    q, dq = np.asarray(q, dtype=LD).ravel(), np.asarray(dq, dtype=LD).ravel()
    cnt, dmax = q.size, float(np.max(dq))
    d = q - LD(center)
    ad = np.abs(d) + dq
    print("quadratic %s: %d points, dq max %.3e; min %.17g (ref %.17g) max %.17g (ref %.17g)" % (what, cnt, dmax, got6[0], float(q.min()), got6[1], float(q.max())))
    assert np.all(np.isfinite(got6)), (what, got6)
    assert abs(LD(got6[0]) - q.min()) <= dmax and abs(LD(got6[1]) - q.max()) <= dmax, (what, got6[:2], float(q.min()), float(q.max()), dmax)
    dp, ap = np.ones_like(d), np.ones_like(d)         # d^p and (|d| + dq)^(p - 1), by repeated products
    for p in (1, 2, 3, 4):
        slope = np.sum(p * dq * ap)
        dp, ap = dp * d, ap * ad
        ref = np.sum(dp)
        bound = slope + (cnt + 8) * LD(2.0) ** -52 * np.sum(np.abs(dp))
        err = abs(LD(got6[1 + p]) - ref)
        print("   S%d %.17g ref %.17g err %.3e bound %.3e" % (p, got6[1 + p], float(ref), float(err), float(bound)))
        assert err <= bound, (what, p, float(err), float(bound))


def _check_counts(counts, q, dq, lo, hi, nbins, what):
    q = np.asarray(q, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    su, sd = th._slots(q + dq, lo, hi, nbins), th._slots(q - dq, lo, hi, nbins)
    share = float(np.mean(su != sd))
    cu = np.cumsum(np.bincount(su.ravel(), minlength=nbins + 3))[:nbins + 2]
    cd = np.cumsum(np.bincount(sd.ravel(), minlength=nbins + 3))[:nbins + 2]
    cg = np.cumsum(counts)[:nbins + 2]
    print("   counts %s: %d bins, slot changes within +-dq %.4f %%, cumulative slack below %d above %d"
          % (what, nbins, 100 * share, int(np.min(cg - cu)), int(np.min(cd - cg))))
    assert share <= 0.01, (what, share)
    assert counts.sum() == q.size and counts[nbins + 2] == 0, (what, counts.sum(), q.size, counts[nbins + 2])
    assert np.all(cu <= cg) and np.all(cg <= cd), (what, np.flatnonzero((cu > cg) | (cg > cd)))


def _range(q):
    q = np.asarray(q, dtype=np.float64)
    hi = float(np.mean(q) + 4 * np.std(q))
    return -hi / 8, hi


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("shape,weights", [((3, 8, 16, 32), [1.0, 1.0, 1.0]), ((6, 8, 16, 32), [2.0, 2.0, 2.0, 4.0, 4.0, 4.0]),
                                           ((6, 8, 16, 32), [1.5, -0.75, 0.1, -3.0, 2.0, 0.3]), ((1, 7, 9, 15), [1.0]), ((1, 7, 9, 15), [-2.5])])
def test_sweep_counts_equal_numpy(shape, weights, prec):
    """spectral.quadratic of random real arrays with edge values, +-Inf and NaN placed: the counts EQUAL numpy evaluating the q rule
    and the slot rule in float64; the sums against a long-double sum of numpy's q within the summation term of the bound.
    (1, 7, 9, 15) has 945 elements: the scalar build of the sweep; the others its 16-byte build."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array([8, 16, 32]), L, SelfComm(0), prec)
    rng = np.random.default_rng(17 + shape[0] + int(weights[0] < 0))
    x = rng.standard_normal(shape).astype(rdtype(prec))
    flat = x.reshape(shape[0], -1)
    n = flat.shape[1]
    flat[:, 5] = 0.0                                  # q = 0 exactly
    flat[0, 6] = 2.0
    flat[1:, 6] = 0.0                                 # q = 4 w_0: on an edge of the range below where w_0 = 1
    clean = spectral.quad_rule(flat.astype(np.float64), weights)
    lo, hi, nbins = -8.0, 8.0, 64                     # edges at multiples of 1/4
    m, h = spectral.quadratic(F, DeviceArray.from_numpy(x), weights=weights, center=0.25, bins=nbins, range=(lo, hi))
    got6 = np.concatenate([m.min, m.max, m.sums[0]])
    assert h.count == m.count == n and np.array_equal(_raw(h), th._hist(clean, lo, hi, nbins)), np.flatnonzero(_raw(h) != th._hist(clean, lo, hi, nbins))
    assert got6[0] == clean.min() and got6[1] == clean.max()
    d = clean.astype(LD) - LD(0.25)
    for p in (1, 2, 3, 4):                            # q is numpy's to the bit: what is left is (q - c)^p and the summation
        ref, mag = np.sum(d ** p), np.sum(np.abs(d) ** p)
        err = abs(LD(got6[1 + p]) - ref)
        print("sweep %s %s %s S%d err %.3e bound %.3e" % (shape, weights, prec, p, float(err), float((n + 8) * 2.0 ** -52 * mag)))
        assert err <= (n + 8) * LD(2.0) ** -52 * mag
    # special values: NaN and Inf make q NaN or +-Inf; counts still equal numpy
    for c in range(shape[0]):
        where = rng.choice(np.arange(8, n), 3, replace=False)
        flat[c, where] = [np.inf, -np.inf, np.nan]
    bad = spectral.quad_rule(flat.astype(np.float64), weights)
    m, h = spectral.quadratic(F, DeviceArray.from_numpy(x), weights=weights, bins=37, range=(-1.1, 5.3))
    assert np.array_equal(_raw(h), th._hist(bad, -1.1, 5.3, 37)) and h.nonfinite[0] >= 1 and _raw(h).sum() == n
    assert np.isnan(m.min[0]) and np.isnan(m.max[0]) and np.all(np.isnan(m.sums))
    m0, h0 = spectral.quadratic(F, DeviceArray.from_numpy(x), weights=weights)
    assert h0 is None and np.isnan(m0.min[0])
    if shape[0] == 3:
        pitched = DeviceArray.from_numpy(x)
        view = DeviceArray(pitched.shape, pitched.dtype, ptr=pitched.ptr, owner=False)
        view.pitch = 40
        with pytest.raises(ValueError):
            spectral.quadratic(F, view, bins=8, range=(lo, hi))


# ---- 2. the stage alone ---------------------------------------------------------------------------------------------------
def _rows_call(a, b, nfields, nrows, n, pitch, valid, valid_in, prec, w, center, lo, hi, nbins):
    from mpifft4py_amd import DeviceArray, _lib
    da = DeviceArray.from_numpy(a)
    db = DeviceArray.from_numpy(b) if b is not None else None
    out6 = np.full(6, -7.0)
    counts = np.full(nbins + 3, -1, dtype=np.int64)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    _lib.call("mfft_nlz_quad_rows", da.ptr, db.ptr if db is not None else None, nfields, nrows, n, pitch, valid, valid_in,
              _lib.precision_code(prec), w.ctypes.data_as(DP), float(center), float(lo), float(hi), nbins, out6.ctypes.data_as(DP),
              counts.ctypes.data_as(IP) if nbins else None)
    assert da.get().tobytes() == a.tobytes() and (b is None or db.get().tobytes() == b.tobytes())      # inputs preserved
    return out6, counts


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", th.LENGTHS)
def test_stage_known_answers_exact(n, prec):
    """Three fields whose real rows are known: only bin 0 set (the constant 2), bins 0 and n/2 set (1 + 2 (-1)^j = 3, -1), the
    single bin n/4 (3 cos(pi j / 2) = 3, 0, -3, 0).  With weights (1, 2, -1): q = 4 + 2 r_1^2 - r_2^2 over j mod 4 is 13, 6, 13, 6:
    exactly representable, mid-bin in 16 bins of width 1 over [-0.5, 15.5).  Counts, min, max and S1 are exact."""
    nrows, valid, nbins = 5, n // 2 + 1, 16
    a = np.zeros((3, nrows, valid + 3), dtype=cdtype(prec))
    a[0, :, 0] = 2.0 * n
    a[1, :, 0] = 1.0 * n
    a[1, :, n // 2] = 2.0 * n
    a[2, :, n // 4] = 1.5 * n
    w = [1.0, 2.0, -1.0]
    out6, counts = _rows_call(a, None, 3, nrows, n, valid + 3, valid, 0, prec, w, 0.0, -0.5, 15.5, nbins)
    want = np.zeros(nbins + 3, dtype=np.int64)
    want[1 + 13] = want[1 + 6] = nrows * n // 2
    print("known answers n=%d %s: %s %s" % (n, prec, out6, counts))
    assert np.array_equal(counts, want)
    assert out6[0] == 6.0 and out6[1] == 13.0 and out6[2] == 19.0 * nrows * n / 2
    rows = th._irfft_rows(a, n, valid)
    assert np.array_equal(want, th._hist(w[0] * rows[0] ** 2 + w[1] * rows[1] ** 2 + w[2] * rows[2] ** 2, -0.5, 15.5, nbins))      # (the reference agrees)
    # a and b: six fields, q = 4 + 9 + .. in slot order; small integer weights
    b = a.copy()
    out6, counts = _rows_call(a, b, 6, nrows, n, valid + 3, valid, 0, prec, [1, 2, -1, 1, 1, 1], 0.0, -0.5, 63.5, 64)
    q4 = np.array([13 + 4 + 9 + 9, 6 + 4 + 1, 13 + 4 + 9 + 9, 6 + 4 + 1])      # 4 + 2 r_1^2 - r_2^2 + 4 + r_1^2 + r_2^2 = 8 + 3 r_1^2
    want = np.bincount(1 + q4, minlength=67) * (nrows * n // 4)
    assert np.array_equal(counts, want) and out6[0] == 11.0 and out6[1] == 35.0 and out6[2] == float(q4.sum()) * nrows * n / 4


def _stage_random(n, prec, nfields, nrows, valid, valid_in=0, nbins=64, w=None):
    """Seeded Gaussian spectra with real end bins; the reference rows, their bound, the range of the module's docstring."""
    rng = np.random.default_rng(200 * n + 7 * nrows % 1000 + valid + nfields)
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
    w = WEIGHTS[nfields] if w is None else w
    fields = [r for x in (a, b) if x is not None for r in th._irfft_rows(x, n, vin)]
    dl = [r for x in (a, b) if x is not None for r in th._row_delta(x, n, vin, prec)]
    deltas = []
    for f in range(nfields):                          # the partner on the transform (test_gpu_real_histogram._stage_random)
        g = (f + ncomp) % nfields if b is not None else (f ^ 1 if (f ^ 1) < nfields else None)
        deltas.append((dl[f] + (dl[g] if g is not None else 0.0))[:, None])
    q, dq = _q_and_dq(fields, w, deltas)
    lo, hi = _range(q)
    center = float(np.mean(q.astype(np.float64))) if nrows % 2 else 0.0
    flat = lambda x: x if nfields > 2 else x[0]
    out6, counts = _rows_call(flat(a), flat(b) if b is not None else None, nfields, nrows, n, pitch, valid, valid_in, prec, w, center, lo, hi, nbins)
    what = "stage n=%d %s nfields=%d nrows=%d valid=%d/%d" % (n, prec, nfields, nrows, vin, valid)
    _check_moments(out6, q, dq, center, what)
    if nbins:
        _check_counts(counts, q, dq, lo, hi, nbins, what)
    return out6, counts


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", th.LENGTHS)
def test_stage_random_spectra_bounds(n, prec):
    """1, 2, 3 and 6 fields; one row, an odd count, pruned valid_in, a signed set of weights; a second call gives identical results."""
    full, lim = n // 2 + 1, n // 3 + 1
    nb = 64 if prec == "double" else 16
    first = _stage_random(n, prec, 6, 37, full, nbins=nb)
    again = _stage_random(n, prec, 6, 37, full, nbins=nb)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    _stage_random(n, prec, 3, 37, lim, nbins=nb, w=[1.5, -0.5, 0.25])
    _stage_random(n, prec, 2, 37, full, valid_in=lim, nbins=nb)
    _stage_random(n, prec, 1, 1, full, nbins=0)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", th.LENGTHS)
def test_stage_more_than_two_passes_of_the_grid(n, prec):
    """More than two passes of mfft_nlz_quad_groups workgroups and a ragged rest: every workgroup strides, the last pass is partial."""
    from mpifft4py_amd import _lib
    code = _lib.precision_code(prec)
    cap = _lib.call("mfft_nlz_quad_groups", 1 << 40, n, code)
    per = 1
    while _lib.call("mfft_nlz_quad_groups", per + 1, n, code) == 1:      # rows per workgroup: a power of two
        per *= 2
    assert cap >= 1
    nrows = 2 * cap * per + per // 2 + 3
    assert _lib.call("mfft_nlz_quad_groups", nrows, n, code) == cap
    _stage_random(n, prec, 1, nrows, n // 2 + 1, nbins=64 if prec == "double" else 16)


def test_stage_nonfinite_bins_and_error_codes():
    """A NaN or Inf bin in ANY field: NaN sums, NaN min and max, counts in the non-finite slot, slots still sum to the points.
    MFFT_ERR_UNSUPPORTED for a length without a kernel; MFFT_ERR_INVALID for bins outside 0 .. 512, a non-finite weight and
    lo >= hi: the status codes themselves, and a refused call writes nothing."""
    from mpifft4py_amd import DeviceArray, _lib
    n, nrows, valid, nbins = 128, 5, 65, 31
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    b = rng.standard_normal((3, nrows, valid)) + 1j * rng.standard_normal((3, nrows, valid))
    w = WEIGHTS[6]
    out6, clean = _rows_call(a, b, 6, nrows, n, valid, valid, 0, "double", w, 0.0, -0.1, 0.7, nbins)
    assert clean.sum() == nrows * n and clean[-1] == 0 and np.all(np.isfinite(out6))
    for bad in (np.nan, np.inf):
        for which in (0, 1):
            an, bn = a.copy(), b.copy()
            (an, bn)[which][1, 3, 7] = bad
            out6, got = _rows_call(an, bn, 6, nrows, n, valid, valid, 0, "double", w, 0.0, -0.1, 0.7, nbins)
            print("bad bin %r in %s: %s nonfinite %d" % (bad, "ab"[which], out6, got[-1]))
            assert np.all(np.isnan(out6)) and got[-1] >= 1 and got.sum() == nrows * n
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(MFFT_ERR_\w+)\s*=\s*(-?\d+)", header)}
    z = DeviceArray.zeros((3, 4, 65), np.complex128)
    out = np.full(6, -7.0)
    cnt = np.full(515, -7, dtype=np.int64)
    fn = getattr(_lib.load(), "mfft_nlz_quad_rows")
    one = np.ones(6)
    wnan, winf = one.copy(), one.copy()
    wnan[4], winf[0] = np.nan, np.inf

    def status(nn, nb, ww, lo, hi):
        return fn(z.ptr, z.ptr, 6, 4, nn, 65, min(65, nn // 2 + 1), 0, _lib.DOUBLE, ww.ctypes.data_as(DP), 0.0, lo, hi, nb, out.ctypes.data_as(DP), cnt.ctypes.data_as(IP))
    cases = [((100, 31, one, -1.0, 1.0), "MFFT_ERR_UNSUPPORTED"), ((128, -1, one, -1.0, 1.0), "MFFT_ERR_INVALID"),
             ((128, 513, one, -1.0, 1.0), "MFFT_ERR_INVALID"), ((128, 31, wnan, -1.0, 1.0), "MFFT_ERR_INVALID"),
             ((128, 0, winf, -1.0, 1.0), "MFFT_ERR_INVALID"), ((128, 31, one, 1.0, 1.0), "MFFT_ERR_INVALID"),
             ((128, 31, one, 1.0, -1.0), "MFFT_ERR_INVALID")]
    for args, name in cases:
        rc = status(*args)
        print(args[:2], args[3:], "->", rc)
        assert rc == codes[name], (args[:2], rc, name)
    assert np.all(out == -7.0) and np.all(cnt == -7)
    assert status(128, 31, one, -1.0, 1.0) == 0 and cnt[16] == 4 * 128 and out[0] == out[1] == 0.0      # rows of zeros: the bin that holds 0
    assert status(128, 0, one, 1.0, 1.0) == 0                        # no bins: the range is not looked at
    assert _lib.call("mfft_nlz_quad_groups", 4, 100, _lib.DOUBLE) == 0


# ---- 3. the plan operation ------------------------------------------------------------------------------------------------
_SPARSE = {}


def _sparse_reference(N, prec, dealias):
    """Single precision on the larger meshes: 32 modes per field with 1 <= kz <= N2/2 - 1 and Gaussian amplitudes (no
    self-conjugate bin: any complex amplitude stands for a real field), the oracle's real fields and the 3-D sums of the bound
    (of the masked spectrum under the 2/3-rule)."""
    key = (tuple(int(n) for n in N), prec, dealias)
    if key not in _SPARSE:
        from mpifft4py_amd import LayoutComm
        from mpifft4py_amd.slab import R2C
        N = np.array(N)
        F = R2C(N, L, LayoutComm(1, 0), prec)
        cs = tuple(F.complex_shape())
        rng = np.random.default_rng(31 + int(N[2]))
        tot = float(np.prod(N))

        def draw():
            x = np.zeros((3,) + cs, dtype=cdtype(prec))
            for i in range(3):
                kx, ky = rng.integers(0, N[0], 32), rng.integers(0, N[1], 32)
                kz = rng.integers(1, N[2] // 2, 32)
                x[i, kx, ky, kz] = (rng.standard_normal(32) + 1j * rng.standard_normal(32)) * tot / 16
            return x
        a, b = draw(), draw()
        mask = F.get_dealias_filter() if dealias == "2/3-rule" else None
        ua, ub = nl.oracle_back(a, N, prec, dealias, mask), nl.oracle_back(b, N, prec, dealias, mask)
        grid = np.array([3 * n // 2 for n in N]) if dealias == "3/2-rule" else N
        scale = 8 * th.EPS[prec] * np.log2(float(np.prod(grid))) / tot
        m = 1.0 if mask is None else np.asarray(mask, dtype=np.float64)
        sums = [scale * float(np.sum(np.abs(x[i].astype(np.complex128)) * m * 2.0)) for x in (a, b) for i in range(3)]
        _SPARSE[key] = (a, b, ua, ub, sums)
    return _SPARSE[key]


def _reference(N, prec, dealias):
    if prec == "single" and int(np.prod(N)) > 8 * 16 * 32:
        return _sparse_reference(N, prec, dealias)
    return th._reference(N, prec, dealias)


_SETUP = {}


def _setup(N, prec, dealias, nfields):
    """(fields, w, q, dq, lo, hi, nbins) of a plan case, from the reference alone: 64 bins, but in single precision with the dense
    spectra of [8, 16, 32], and under the 2/3-rule with the sparse ones, the largest of 64 .. 2 at which the 1 % condition holds."""
    key = (tuple(int(n) for n in N), prec, dealias, nfields)
    if key not in _SETUP:
        a, b, ua, ub, sums = _reference(N, prec, dealias)
        fields = (list(ua) + list(ub))[:nfields]
        w = WEIGHTS[nfields]
        deltas = [sums[f] + (sums[th._partner(f, nfields)] if th._partner(f, nfields) is not None else 0.0) for f in range(nfields)]
        q, dq = _q_and_dq(fields, w, deltas)
        lo, hi = _range(q)
        q64 = q.astype(np.float64)
        nbins = th.LADDER[-1]
        for nb in th.LADDER:
            if np.mean(th._slots(q64 + dq, lo, hi, nb) != th._slots(q64 - dq, lo, hi, nb)) <= 0.01:
                nbins = nb
                break
        dense_single = prec == "single" and int(np.prod(N)) <= 8 * 16 * 32
        assert nbins == 64 or dense_single or (prec == "single" and dealias == "2/3-rule"), (key, nbins)
        _SETUP[key] = (fields, w, q, dq, lo, hi, nbins)
    return _SETUP[key]


def _call(F, a, b, nfields, dealias, w, center, lo, hi, nbins, reduce=True):
    from mpifft4py_amd import spectral
    if nfields == 1:
        da, db = F.empty_complex().set(a[0]), None
    else:
        da, db = F.empty_complex(3).set(a), (F.empty_complex(3).set(b) if nfields == 6 else None)
    m, h = spectral.real_quadratic(F, da, db, dealias, weights=w, center=center, bins=nbins, range=(lo, hi), reduce=reduce)
    return m, h, da, db


def _plan_case(F, N, prec, dealias, nfields, fused):
    from mpifft4py_amd import spectral
    a, b = _reference(N, prec, dealias)[:2]
    fields, w, q, dq, lo, hi, nbins = _setup(N, prec, dealias, nfields)
    center = float(np.mean(q.astype(np.float64)))
    m, h, da, db = _call(F, a, b, nfields, dealias, w, center, lo, hi, nbins)
    assert F.plan_info(INFO(dealias)) == (1 if fused else 0)
    got6 = np.concatenate([m.min, m.max, m.sums[0]])
    what = "%s %s %s nfields=%d" % (list(N), prec, dealias, nfields)
    assert m.count == h.count == q.size
    _check_moments(got6, q, dq, center, what)
    _check_counts(_raw(h), q, dq, lo, hi, nbins, what)
    assert np.array_equal(da.get(), a[0] if nfields == 1 else a) and (db is None or np.array_equal(db.get(), b))      # inputs preserved
    m2, h2 = spectral.real_quadratic(F, da, db, dealias, weights=w, center=center, bins=nbins, range=(lo, hi))
    assert np.array_equal(_raw(h2), _raw(h)) and np.array_equal(np.concatenate([m2.min, m2.max, m2.sums[0]]), got6)      # identical arrays
    return got6, _raw(h)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[8, 16, 32], [32, 64, 128], [36, 72, 144]])
def test_real_quadratic_one_rank_fused(N, dealias, nfields, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), prec), N, prec, dealias, nfields, True)


def test_real_quadratic_pitched_plan_with_nans_between_rows():
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N, prec = [32, 64, 128], "double"
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec, complex_pitch="auto")
    assert F.complex_pitch > F.complex_shape()[-1]
    for dealias in ("3/2-rule", "2/3-rule", None):
        a, b = _reference(N, prec, dealias)[:2]
        fields, w, q, dq, lo, hi, nbins = _setup(N, prec, dealias, 6)
        da, db = F.empty_complex(3), F.empty_complex(3)
        for d in (da, db):                                                         # NaNs between the rows
            whole = DeviceArray(d.shape[:-1] + (F.complex_pitch,), d.dtype, ptr=d.ptr, owner=False)
            whole.set(np.full(whole.shape, np.nan + 1j * np.nan, dtype=d.dtype))
        da.set(a), db.set(b)
        m, h = spectral.real_quadratic(F, da, db, dealias, weights=w, bins=nbins, range=(lo, hi))
        assert F.plan_info(INFO(dealias)) == 1
        _check_moments(np.concatenate([m.min, m.max, m.sums[0]]), q, dq, 0.0, "pitched %s" % dealias)
        _check_counts(_raw(h), q, dq, lo, hi, nbins, "pitched %s" % dealias)


# ---- batches, composed route: fresh processes (the switches are read once) ------------------------------------------------
def _child(code, **env):
    return nl.run_child("import test_gpu_real_quadratic as t\n" + code, timeout=280, **env)


@pytest.mark.parametrize("align", ["0", "1"])
def test_real_quadratic_batches(align):
    """[40, 32, 64] with the 3/2-rule in batches of 1 MB (nine or ten batches, the last one ragged): moments and counts accumulate
    over the batches."""
    _child("""
N = [40, 32, 64]
F = Slab_R2C(np.array(N), L, SelfComm(0), 'double')
for nfields in (6, 1, 3):
    t._plan_case(F, N, 'double', '3/2-rule', nfields, True)
print('ok')
""", MFFT_NLZ_BATCH_MB="1", MFFT_NLZ_ALIGN=align)


def test_real_quadratic_composed_kill_switch():
    """MFFT_NO_NLZ=1: one field at a time through the plan's inverse transform into ONE real work array, its term added into ONE
    array of doubles, one sweep: plan_info 0, the same bounds."""
    _child("""
for N in ([8, 16, 32], [16, 32, 24]):
    for prec in ('double', 'single'):
        F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
        for dealias in ('3/2-rule', '2/3-rule', None):
            for nfields in (6, 1, 3):
                t._plan_case(F, N, prec, dealias, nfields, False)
            points = int(np.prod([3 * n // 2 for n in N]))          # ONE real work array and ONE array of doubles, sized by the 3/2-rule's grid
            want = points * (8 if prec == 'double' else 4) + points * 8
            assert F.plan_info('nonlinear_bytes') == want, (F.plan_info('nonlinear_bytes'), want)
print('ok')
""", MFFT_NO_NLZ="1")


@pytest.mark.parametrize("dealias", ["3/2-rule", None])
def test_real_quadratic_pencils(dealias):
    """Pencil_R2C on 2 x 2 virtual ranks (composed inside the plan): every rank's counts EQUAL numpy's rule on the real fields its
    own ifftn gives (fields in slot order), the reduced ones are their sum and identical on every rank."""
    from mpifft4py_amd import DeviceArray, spectral
    from mpifft4py_amd.pencil import R2C as Pencil_R2C
    N = np.array([16, 32, 24])
    w, lo, hi, nbins = np.array(WEIGHTS[6]), -0.001, 0.02, 48

    def work(comm):
        F = Pencil_R2C(N, L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(50 + comm.Get_rank())
        cs, ws = tuple(F.complex_shape()), tuple(F.work_shape(dealias))
        a, b = DeviceArray.empty((3,) + cs, F.complex), DeviceArray.empty((3,) + cs, F.complex)
        for x in (a, b):
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.25), x.component(i))
        u = DeviceArray.empty(ws, F.float)
        r = []
        for x in (a, b):
            for i in range(3):
                F.ifftn(x.component(i), u, dealias)
                r.append(u.get().copy())
        order = spectral.quad_slot_order(6, True)
        q = spectral.quad_rule(np.stack([r[i] for i in order]), w[order])
        ml, hl = spectral.real_quadratic(F, a, b, dealias, weights=w, bins=nbins, range=(lo, hi), reduce=False)
        assert F.plan_info(INFO(dealias)) == 0 and hl.count == int(np.prod(ws))
        assert np.array_equal(_raw(hl), th._hist(q, lo, hi, nbins)) and ml.min[0] == q.min() and ml.max[0] == q.max()
        mg, hg = spectral.real_quadratic(F, a, b, dealias, weights=w, bins=nbins, range=(lo, hi))
        return _raw(hl), _raw(hg), hg.count, hl.count, float(ml.sums[0, 0]), float(mg.sums[0, 0]), float(np.sum(q.astype(LD))), float(np.sum(np.abs(q)))

    res = run_ranks(4, work)
    for hl, hg, cnt, lcnt, s1l, s1g, ref, mag in res:
        assert np.array_equal(hg, res[0][1]) and cnt == sum(r[3] for r in res) and s1g == res[0][5]
        assert abs(s1l - ref) <= (lcnt + 8) * 2.0 ** -52 * mag
    assert np.array_equal(np.sum([r[0] for r in res], 0), res[0][1])
    assert res[0][1].sum() == res[0][2]
    assert abs(res[0][5] - sum(r[6] for r in res)) <= (res[0][2] + 8) * 2.0 ** -52 * sum(r[7] for r in res)


@pytest.mark.parametrize("dealias", ["3/2-rule", "2/3-rule", None])
@pytest.mark.parametrize("N", [[32, 64, 128], [8, 16, 32]])
def test_real_quadratic_ranks_fused_counts_identical_to_one_rank(N, dealias):
    """Fused P = 1, 2 and 4: the counts are IDENTICAL (each row's transforms and its q are the same arithmetic whichever rank runs
    them), min and max too; the sums differ by the order of a double sum only."""
    from mpifft4py_amd import DeviceArray, SelfComm, spectral
    from mpifft4py_amd.slab import R2C as Slab_R2C
    a, b = _reference(N, "double", dealias)[:2]
    fields, w, q, dq, lo, hi, nbins = _setup(N, "double", dealias, 6)
    center = float(np.mean(q.astype(np.float64)))
    one6, one = _plan_case(Slab_R2C(np.array(N), L, SelfComm(0), "double"), N, "double", dealias, 6, True)
    d = np.abs(q - LD(center))

    def work(comm):
        F = Slab_R2C(np.array(N), L, comm, "double")
        sl = (slice(None),) + tuple(F.complex_local_slice())
        da, db = DeviceArray.from_numpy(np.ascontiguousarray(a[sl])), DeviceArray.from_numpy(np.ascontiguousarray(b[sl]))
        ml, hl = spectral.real_quadratic(F, da, db, dealias, weights=w, center=center, bins=nbins, range=(lo, hi), reduce=False)
        assert F.plan_info(INFO(dealias)) == 1
        mg, hg = spectral.real_quadratic(F, da, db, dealias, weights=w, center=center, bins=nbins, range=(lo, hi))
        assert np.array_equal(da.get(), a[sl]) and np.array_equal(db.get(), b[sl])
        return _raw(hl), hl.count, _raw(hg), hg.count, np.concatenate([mg.min, mg.max, mg.sums[0]])

    for P in (2, 4):
        out = run_ranks(P, work)
        for r, (local, lcount, glob, gcount, g6) in enumerate(out):
            assert gcount == q.size and local.sum() == lcount and lcount * P == gcount
            assert np.array_equal(glob, out[0][2]) and np.array_equal(g6, out[0][4])      # identical on all ranks
        assert np.array_equal(np.sum([o[0] for o in out], 0), out[0][2])                   # local counts add up to the reduced ones
        assert np.array_equal(out[0][2], one)                                              # ... and EQUAL one rank's
        g6 = out[0][4]
        assert g6[0] == one6[0] and g6[1] == one6[1]
        for p in (1, 2, 3, 4):
            bound = 2 * (q.size + 8) * 2.0 ** -52 * float(np.sum(d ** p))
            print("%s %s P=%d S%d: %.17g against %.17g, bound %.3e" % (N, dealias, P, p, g6[1 + p], one6[1 + p], bound))
            assert abs(g6[1 + p] - one6[1 + p]) <= bound


@pytest.mark.parametrize("prec", ["double", "single"])
def test_range_none_takes_the_extremes(prec):
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = [8, 16, 32]
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b = th._reference(N, prec, None)[:2]
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    m, h = spectral.real_quadratic(F, da, db, None, bins=16)
    print("range=None %s: lo %s hi %s first %d last %d" % (prec, h.lo, h.hi, h.counts[0, 0], h.counts[0, -1]))
    assert h.below[0] == h.above[0] == h.nonfinite[0] == 0 and h.counts.sum() == h.count
    assert h.counts[0, 0] >= 1 and h.counts[0, -1] >= 1 and h.lo[0] == m.min[0] and h.hi[0] > m.max[0]
    x = DeviceArray.from_numpy((np.random.default_rng(1).random((3, 8, 16, 32)) - 0.5).astype(rdtype(prec)))
    ms, hs = spectral.quadratic(F, x, bins=16)
    assert hs.below[0] == hs.above[0] == 0 and hs.counts[0, 0] >= 1 and hs.counts[0, -1] >= 1 and hs.lo[0] == ms.min[0]
    for kw in (dict(bins=513), dict(bins=-1), dict(bins=4, range=(1.0, 1.0)), dict(weights=[1.0, np.nan, 1.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            spectral.real_quadratic(F, da, db, None, **kw)


# ---- known answers --------------------------------------------------------------------------------------------------------
def _taylor_green(F, N):
    from mpifft4py_amd import DeviceArray
    x = np.arange(N) * 2 * np.pi / N
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    u = np.stack([np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X)])
    U = F.empty_complex(3)
    for i in range(3):
        F.fftn(DeviceArray.from_numpy(u[i]), U.component(i))
    return U


@pytest.mark.parametrize("dealias", ["2/3-rule", None])
def test_taylor_green_enstrophy(dealias):
    """u = (sin x cos y cos z, -cos x sin y cos z, 0) at N = 16: omega^2 of the curl with weights 1 has mean 0.75, min 0, max 4."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    N = 16
    F = Slab_R2C(np.array([N] * 3), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    U = _taylor_green(F, N)
    W = spectral.curl_hat(F, K, U, F.empty_complex(3))
    m, h = spectral.real_quadratic(F, W, None, dealias, bins=8, range=(-0.25, 4.25))
    assert F.plan_info(INFO(dealias)) == 1
    print("Taylor-Green omega^2 (%s): mean %.17g min %.3e max %.17g" % (dealias, float(m.mean()[0]), m.min[0], m.max[0]))
    assert abs(float(m.mean()[0]) - 0.75) <= 1e-13 and abs(m.min[0]) <= 1e-13 and abs(m.max[0] - 4.0) <= 1e-13
    assert h.below[0] == h.above[0] == h.nonfinite[0] == 0 and h.counts.sum() == N ** 3


def test_strain_against_numpy_and_dissipation():
    """strain_hat against numpy on random spectra (pitched and compact); Taylor-Green: <eps> = 2 nu <S_ij S_ij> = 0.75 nu."""
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    for prec, tol in (("double", 1e-14), ("single", 1e-5)):
        for pitch in (None, "auto"):
            N = np.array([8, 16, 32]) if pitch is None else np.array([32, 64, 128])
            F = Slab_R2C(N, L, SelfComm(0), prec, complex_pitch=pitch)
            K = spectral.Wavenumbers(F)
            cs = tuple(F.complex_shape())
            rng = np.random.default_rng(5)
            u = (rng.standard_normal((3,) + cs) + 1j * rng.standard_normal((3,) + cs)).astype(cdtype(prec))
            U = F.empty_complex(3).set(u)
            diag, off = spectral.strain_hat(F, K, U, F.empty_complex(3), F.empty_complex(3))
            k = [np.fft.fftfreq(N[0], 1.0 / N[0])[:, None, None], np.fft.fftfreq(N[1], 1.0 / N[1])[None, :, None],
                 np.fft.rfftfreq(N[2], 1.0 / N[2])[None, None, :]]
            u = u.astype(np.complex128)
            wd = np.stack([1j * k[i] * u[i] for i in range(3)])
            wo = np.stack([0.5j * (k[i] * u[j] + k[j] * u[i]) for i, j in ((0, 1), (0, 2), (1, 2))])
            scale = float(np.max(np.abs(wd)))
            ed, eo = float(np.max(np.abs(diag.get() - wd))) / scale, float(np.max(np.abs(off.get() - wo))) / scale
            print("strain_hat %s pitch %s: %.3e %.3e" % (prec, pitch, ed, eo))
            assert ed <= tol and eo <= tol and np.array_equal(U.get(), u.astype(cdtype(prec)))
    N, nu = 16, 0.01
    F = Slab_R2C(np.array([N] * 3), L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    U = _taylor_green(F, N)
    diag, off = spectral.strain_hat(F, K, U, F.empty_complex(3), F.empty_complex(3))
    m, _ = spectral.real_quadratic(F, diag, off, None, weights=2 * nu * np.array([1, 1, 1, 2, 2, 2.0]))
    mw, _ = spectral.real_quadratic(F, spectral.curl_hat(F, K, U, F.empty_complex(3)), None, None)
    print("Taylor-Green <eps> / nu = %.17g, nu <omega^2> / <eps> = %.17g" % (float(m.mean()[0]) / nu, nu * float(mw.mean()[0]) / float(m.mean()[0])))
    assert abs(float(m.mean()[0]) - 0.75 * nu) <= 1e-14 and abs(nu * float(mw.mean()[0]) / float(m.mean()[0]) - 1.0) <= 1e-12


def test_enstrophy_equals_the_k2_spectrum():
    """Random solenoidal spectra, dealias None: S1 / count of omega^2 equals shell_sums(k2=True).sum() / N^6 -- Parseval, through
    two independent code paths (the fused z kernel, the shell-binning sweep) -- within the bound of this file."""
    from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
    N = np.array([8, 16, 32])
    F = Slab_R2C(N, L, SelfComm(0), "double")
    K = spectral.Wavenumbers(F)
    rng = np.random.default_rng(23)
    U = F.empty_complex(3)
    for i in range(3):
        F.fftn(DeviceArray.from_numpy(rng.standard_normal(tuple(F.real_shape()))), U.component(i))
    u = U.get().astype(np.complex128)
    u[:, N[0] // 2], u[:, :, N[1] // 2], u[:, :, :, N[2] // 2] = 0, 0, 0      # (i k u_hat of a Nyquist mode is not the transform of a real field)
    k = [np.fft.fftfreq(N[0], 1.0 / N[0])[:, None, None] + 0 * u[0].real, np.fft.fftfreq(N[1], 1.0 / N[1])[None, :, None] + 0 * u[0].real,
         np.fft.rfftfreq(N[2], 1.0 / N[2])[None, None, :] + 0 * u[0].real]
    k2 = k[0] ** 2 + k[1] ** 2 + k[2] ** 2
    div = (k[0] * u[0] + k[1] * u[1] + k[2] * u[2]) / np.where(k2 == 0, 1.0, k2)
    U.set(np.stack([u[i] - k[i] * div for i in range(3)]))        # solenoidal: K . U_hat = 0
    W = spectral.curl_hat(F, K, U, F.empty_complex(3))
    m, _ = spectral.real_quadratic(F, W, None, None)
    assert F.plan_info(INFO(None)) == 1
    spec = np.asarray(spectral.shell_sums(F, K, U, k2=True), dtype=np.float64)
    lhs, rhs = float(m.sums[0, 0]) / m.count, float(spec.sum()) / float(np.prod(N)) ** 2
    w = W.get()
    fields = [np.fft.irfftn(w[i], s=tuple(N), axes=(0, 1, 2)) for i in range(3)]
    h = np.full(w.shape[-1], 2.0)
    h[0] = h[-1] = 1.0
    sums = [8 * 2.0 ** -53 * np.log2(float(np.prod(N))) * float(np.sum(np.abs(w[i]) * h)) / float(np.prod(N)) for i in range(3)]
    deltas = [sums[f] + (sums[f ^ 1] if (f ^ 1) < 3 else 0.0) for f in range(3)]
    q, dq = _q_and_dq(fields, [1.0] * 3, deltas)
    bound = float(np.sum(dq) + (q.size + 8) * 2.0 ** -52 * np.sum(np.abs(q))) / q.size
    print("<omega^2> = %.17g, sum k^2 |u|^2 / N^6 = %.17g, difference %.3e, bound %.3e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound + 64 * 2.0 ** -52 * abs(rhs)


# ---- the example ----------------------------------------------------------------------------------------------------------
def test_example_dissipation():
    exe = [sys.executable, os.path.join(ROOT, "examples", "spectral_dns_device.py"), "--M", "5", "--dissipation", "--pdf", "--steps", "2"]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout + r.stderr
    ratios = [float(v) for v in re.findall(r"nu <omega\^2> / <eps> = (\S+)", r.stdout)]
    print(r.stdout[-1500:])
    assert ratios and all(abs(v - 1.0) <= 1e-10 for v in ratios), r.stdout
    assert re.search(r"<eps> = \S+\s+<omega\^2> = \S+", r.stdout) and re.search(r"flatness of eps = \S+\s+of omega\^2 = \S+", r.stdout)
    assert len(re.findall(r"^pdf_eps\s+\S+\s+\S+\s*$", r.stdout, re.M)) >= 8 and len(re.findall(r"^pdf_omega2\s+\S+\s+\S+\s*$", r.stdout, re.M)) >= 8
