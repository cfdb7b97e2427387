"""What the increment-PDF tests share: the slot rule and the bracket comparison of tests/test_gpu_real_histogram.py, restated for
increments, and a plain-Python evaluation of the rule of include/mpifft4py_amd.h.

Counts have no tolerance.  Where the values come from a transform they are compared by BRACKETS: the slot rule is monotone in d,
and an increment is a difference of two values that each carry |x_device - x_ref| <= delta, so |d_device - d_ref| <= 2 delta and
every cumulative count obeys  C_j(d_ref + 2 delta) <= C_j(device) <= C_j(d_ref - 2 delta),  j = 0 .. nbins + 1; the total equals
the number of points and the non-finite slot is 0.  delta is the worst-case bound of the histogram tests, not a measurement.  The
cap is a condition on the case, asserted from the numpy reference alone: at most 1 % of the increments change their slot between
d - 2 delta and d + 2 delta, so a shift by one bin -- which moves whole bins -- cannot pass."""
import numpy as np

EPS = {"double": 2.0 ** -53, "single": 2.0 ** -24}


def slots(x, lo, hi, nbins):
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


def incr(x, s):
    """d = x[(z + s) mod M] - x[z] along the last axis, float64."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.roll(x, -int(s), axis=-1) - x


def counts(x, seps, lo, hi, nbins):
    """(nsep, nbins + 3) counts of the increments of x (rows along its last axis); lo, hi: per separation."""
    return np.stack([np.bincount(slots(incr(x, s), lo[i], hi[i], nbins).ravel(), minlength=nbins + 3) for i, s in enumerate(seps)]).astype(np.int64)


def slot_py(d, lo, hi, nbins):
    """The rule once more, in plain Python floats."""
    inv = float(nbins) / (float(hi) - float(lo))
    if d != d:
        return nbins + 2
    t = (d - float(lo)) * inv
    if t < 0.0:
        return 0
    if t >= float(nbins):
        return nbins + 1
    return 1 + int(t)


def counts_py(rows, seps, lo, hi, nbins):
    """A plain loop over rows (a 2-D array, already float64), positions and separations."""
    out = np.zeros((len(seps), nbins + 3), dtype=np.int64)
    for r in rows:
        r = [float(v) for v in r]
        M = len(r)
        for i, s in enumerate(seps):
            for z in range(M):
                out[i, slot_py(r[(z + int(s)) % M] - r[z], lo[i], hi[i], nbins)] += 1
    return out


def delta_rows(x, n, vin, prec):
    """The per-row bound of the stored spectra x[..., :vin]: 8 eps log2(n) sum_k h_k |A_k| / n (Im of the self-conjugate bins is not
    read); the deltas of the two fields of a pair ADD (they share the transform)."""
    a = np.abs(x[..., :vin].astype(np.complex128))
    a[..., 0] = np.abs(x[..., 0].real)
    h = np.full(vin, 2.0)
    h[0] = 1.0
    if vin == n // 2 + 1 and n % 2 == 0:
        a[..., -1] = np.abs(x[..., vin - 1].real)
        h[-1] = 1.0
    return 8 * EPS[prec] * np.log2(n) * (a * h).sum(-1) / n


def bracket(got, x, delta, s, lo, hi, nbins, what):
    """got: the nbins + 3 device counts of one field at separation s; x: the reference field, rows along the last axis; delta: the
    bound on ONE value, broadcastable to x -- the increments are bracketed with 2 delta."""
    got = np.asarray(got, dtype=np.int64)
    d = incr(x, s)
    dd = 2.0 * np.broadcast_to(np.asarray(delta, dtype=np.float64), d.shape)
    su, sd = slots(d + dd, lo, hi, nbins), slots(d - dd, lo, hi, nbins)
    share = float(np.mean(su != sd))
    outside = float(np.mean((d < lo) | (d >= hi)))
    cu = np.cumsum(np.bincount(su.ravel(), minlength=nbins + 3))[:nbins + 2]
    cd = np.cumsum(np.bincount(sd.ravel(), minlength=nbins + 3))[:nbins + 2]
    cg = np.cumsum(got)[:nbins + 2]
    print("increment histogram %s s=%d: %d points, 2 delta max %.3e, slot changes within +-2 delta %.4f %%, outside the range %.4f %%, "
          "cumulative slack below %d above %d" % (what, s, d.size, float(np.max(dd)), 100 * share, 100 * outside, int(np.min(cg - cu)),
                                                 int(np.min(cd - cg))))
    assert share <= 0.01, (what, s, share)
    assert got.sum() == d.size and got[nbins + 2] == 0, (what, s, got.sum(), d.size, got[nbins + 2])
    assert np.all(cu <= cg) and np.all(cg <= cd), (what, s, np.flatnonzero((cu > cg) | (cg > cd)))
