"""Element-wise pieces of a pseudo-spectral Navier-Stokes step on DeviceArrays
(mfft_ew_* of the C ABI).  They are enqueued on the FFT object's own stream, so a
whole RK4 step -- 36 transforms plus these kernels -- runs without a host copy
or a host synchronisation.  Vector fields are DeviceArrays of shape (3,) + local
shape; `Wavenumbers` holds the three 1-D scaled wavenumber vectors on the device."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray


class Wavenumbers(object):
    """Scaled local wavenumbers (2*pi/L * k) of an FFT object's complex layout; for the shell spectra (`shell_sums`) of
    3-D plans also the integer ones (`idev`, int32), the Hermitian weights along z (`hdev`, uint8) and `nshell`.  For the
    (k_perp, k_z) spectra (`cyl_sums`) `nperp`, `npar`, `perp_rows` (device, int32) and `perp_start` (host, int32) are built on
    first use: the rows of the block sorted by perp shell (`_mesh.Block.perp_row_lists`)."""

    def __init__(self, FFT):
        K = FFT.get_local_wavenumbermesh(scaled=True)
        self.shape = tuple(int(s) for s in FFT.complex_shape())
        vecs = [np.ascontiguousarray(np.asarray(K[i], dtype=FFT.float).reshape(-1)) for i in range(3)]
        assert tuple(len(v) for v in vecs) == self.shape
        # pitched spectra (FFT.complex_pitch): the element-wise kernels sweep the rows as they lie in memory, the elements
        # between the rows included (wavenumber 0 there; nothing reads what they compute)
        pitch = getattr(FFT, "complex_pitch", None)
        if pitch:
            vecs[2] = np.concatenate([vecs[2], np.zeros(pitch - len(vecs[2]), dtype=vecs[2].dtype)])
        self.dev = [DeviceArray.from_numpy(v) for v in vecs]
        self.cshape = (ctypes.c_int64 * 3)(self.shape[0], self.shape[1], len(vecs[2]))
        self.idev = self.hdev = self.nshell = None
        mesh = getattr(FFT, "_mesh", None)
        if mesh is not None and mesh.nd == 3:
            ivecs, h = mesh.shell_index_vectors(), mesh.hermitian_weights()
            assert tuple(len(v) for v in ivecs) == self.shape and len(h) == self.shape[2]
            pad = len(vecs[2]) - self.shape[2]                 # pitched spectra: weight 0 between the rows = skipped
            ivecs[2] = np.concatenate([ivecs[2], np.zeros(pad, dtype=np.int32)])
            h = np.concatenate([h, np.zeros(pad, dtype=np.uint8)])
            self.idev = [DeviceArray.from_numpy(v) for v in ivecs]
            self.hdev = DeviceArray.from_numpy(h)
            self.nshell = mesh.shell_count()
        self._mesh = mesh if self.idev is not None else None
        self._perp = None

    def _perp_lists(self):
        if self._perp is None:
            if self._mesh is None:
                raise NotImplementedError("(k_perp, k_z) spectra need a 3-D plan (slab or pencil)")
            rows, start = self._mesh.perp_row_lists()
            self._perp = (self._mesh.perp_shell_count(), self._mesh.N[2] // 2 + 1, DeviceArray.from_numpy(rows), start)
        return self._perp

    nperp = property(lambda self: self._perp_lists()[0])
    npar = property(lambda self: self._perp_lists()[1])
    perp_rows = property(lambda self: self._perp_lists()[2])
    perp_start = property(lambda self: self._perp_lists()[3])


def _prec(FFT):
    return _lib.precision_code(FFT.precision)


def cross(FFT, a, b, out):
    """out = a x b for real vector fields of shape (3,) + real shape."""
    assert a.pitch is None and b.pitch is None and out.pitch is None
    n = a.size // 3
    _lib.call("mfft_ew_cross", FFT._plan, a.ptr, b.ptr, out.ptr, n, _prec(FFT))
    return out


def curl_hat(FFT, K, U_hat, out):
    """out = i K x U_hat."""
    _lib.call("mfft_ew_curl_hat", FFT._plan, U_hat.ptr, out.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr,
              K.cshape, _prec(FFT))
    return out


def ns_rhs(FFT, K, dU, U_hat, nu):
    """Pressure projection and viscous term, in place on dU."""
    _lib.call("mfft_ew_ns_rhs", FFT._plan, dU.ptr, U_hat.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr,
              K.cshape, float(nu), _prec(FFT))
    return dU


def _nonlinear(FFT, name, fields, dealias, head=None, tail=()):
    """One nonlinear operation of the plan, mfft_<name>: `fields` are its (DeviceArray, is_vector) pairs in the order of the
    call's arguments, each of shape FFT.complex_shape() -- (3,) + that for a vector field, (n,) + that where `is_vector` is a
    component count n (the nine of the outer product) -- and of the plan's pitch.
    `head`: the arguments before the dealias code where they are not just the fields' pointers; `tail`: those after it."""
    from ._base import _DEALIAS
    assert dealias in ('3/2-rule', '2/3-rule', 'None', None)
    cs = tuple(int(s) for s in FFT.complex_shape())
    for x, is_vector in fields:
        shape = (3 if is_vector is True else int(is_vector),) + cs if is_vector else cs
        assert x.shape == shape and x.dtype == np.dtype(FFT.complex), (x.shape, x.dtype, shape)
        FFT._check_pitch(x, FFT.complex_pitch)
    code = _DEALIAS[dealias]
    FFT.comm.use_device()
    if code == _lib.DEALIAS_2_3:
        FFT._ensure_mask()
    _lib.call("mfft_" + name, FFT._plan, *(tuple(x.ptr for x, _ in fields) if head is None else head), code, *tail)


def cross_transform(FFT, a_hat, b_hat, out_hat, dealias=None, absmax=False):
    """out_hat = fftn(ifftn(a_hat) x ifftn(b_hat)), the nonlinear term of a pseudo-spectral step as ONE operation of the
    plan (mfft_nonlinear_cross): what the reference demo composes from six `FFT.ifftn(.., dealias)`, a cross product of
    numpy arrays and three `FFT.fftn(.., dealias)` (demo/spectral_dns_solver.py:53-71).  All three are DeviceArrays of
    shape (3,) + FFT.complex_shape(); out_hat may be a_hat or b_hat.  On one rank (slab) the z stages are one fused kernel
    and no real-space work array exists (`FFT.plan_info("nonlinear_fused_3_2")`); elsewhere the plan composes it.
    With `absmax` the call also records max |ifftn(a_hat[f])| and max |ifftn(b_hat[f])| -- velocity and vorticity -- on the
    device (mfft_nonlinear_cross_absmax); `nonlinear_absmax(FFT)` fetches them."""
    _nonlinear(FFT, "nonlinear_cross_absmax" if absmax else "nonlinear_cross", [(a_hat, True), (b_hat, True), (out_hat, True)], dealias)
    return out_hat


def dot(FFT, a, b, out):
    """out = sum_f a[f] * b[f] for real vector fields a, b of shape (3,) + real shape; out has the real shape (and may be
    a component of a or b).  What a caller writes as np.sum(a * b, 0) (mfft_ew_dot)."""
    assert a.pitch is None and b.pitch is None and out.pitch is None
    n = a.size // 3
    assert b.size == 3 * n and out.size == n, (a.shape, b.shape, out.shape)
    _lib.call("mfft_ew_dot", FFT._plan, a.ptr, b.ptr, out.ptr, n, _prec(FFT))
    return out


def mul(FFT, a, b, out):
    """out = a * b for real fields of the real shape (out may be a or b): one product a_i b_j of a composed outer product
    (mfft_ew_mul)."""
    assert a.pitch is None and b.pitch is None and out.pitch is None
    assert a.size == b.size == out.size and a.dtype == b.dtype == out.dtype == np.dtype(FFT.float), (a.shape, b.shape, out.shape)
    _lib.call("mfft_ew_mul", FFT._plan, a.ptr, b.ptr, out.ptr, a.size, _prec(FFT))
    return out


def grad_hat(FFT, K, s_hat, out):
    """out[f] = i K[f] s_hat: the gradient of a scalar in spectral space (mfft_ew_grad_hat).  s_hat has
    FFT.complex_shape(), out is (3,) + that; pitched spectra are swept as they lie in memory, like curl_hat."""
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert s_hat.shape == cs and out.shape == (3,) + cs, (s_hat.shape, out.shape, cs)
    assert s_hat.dtype == out.dtype == np.dtype(FFT.complex) and s_hat.pitch == out.pitch, (s_hat.dtype, s_hat.pitch, out.pitch)
    _lib.call("mfft_ew_grad_hat", FFT._plan, s_hat.ptr, out.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr,
              K.cshape, _prec(FFT))
    return out


def diag_grad_hat(FFT, K, U_hat, out):
    """out[f] = i K[f] U_hat[f]: the three LONGITUDINAL derivatives du_f/dx_f of a vector field in spectral space
    (mfft_ew_diag_grad_hat) -- the field whose skewness, about -0.5 in developed turbulence, a DNS is judged by
    (`real_moments`).  U_hat and out are (3,) + FFT.complex_shape(); pitched spectra are swept as they lie in memory."""
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert U_hat.shape == out.shape == (3,) + cs, (U_hat.shape, out.shape, cs)
    assert U_hat.dtype == out.dtype == np.dtype(FFT.complex) and U_hat.pitch == out.pitch, (U_hat.dtype, U_hat.pitch, out.pitch)
    _lib.call("mfft_ew_diag_grad_hat", FFT._plan, U_hat.ptr, out.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr,
              K.cshape, _prec(FFT))
    return out


def dot_transform(FFT, a_hat, b_hat, out_hat, dealias=None, absmax=False):
    """out_hat = fftn(sum_f ifftn(a_hat[f]) * ifftn(b_hat[f])), the advection term u . grad(theta) of a transported scalar
    as ONE operation of the plan (mfft_nonlinear_dot): what a caller composes from six `FFT.ifftn(.., dealias)`,
    np.sum(A * B, 0) and one `FFT.fftn(.., dealias)`.  a_hat and b_hat are DeviceArrays of shape (3,) +
    FFT.complex_shape(), out_hat has FFT.complex_shape() and may be any one component of a_hat or b_hat
    (`b_hat.component(1)`); the inputs are otherwise preserved.  On slab plans with radix kernels on every axis the z
    stages are one fused kernel and no real-space work array exists (`FFT.plan_info("nonlinear_dot_fused_3_2")`);
    elsewhere the plan composes it on seven work arrays of its own.  With `absmax` the call also records
    max |ifftn(a_hat[f])| and max |ifftn(b_hat[f])| (mfft_nonlinear_dot_absmax; see `nonlinear_absmax`)."""
    _nonlinear(FFT, "nonlinear_dot_absmax" if absmax else "nonlinear_dot", [(a_hat, True), (b_hat, True), (out_hat, False)], dealias)
    return out_hat


def cross_dot_transform(FFT, a_hat, b_hat, c_hat, out_hat, s_hat, dealias=None):
    """out_hat = fftn(ifftn(a_hat) x ifftn(b_hat)) AND s_hat = fftn(sum_f ifftn(a_hat[f]) * ifftn(c_hat[f])) as ONE operation
    of the plan (mfft_nonlinear_cross_dot): u x omega and u . grad(theta) of a velocity that carries a scalar, =
    `cross_transform(FFT, a_hat, b_hat, out_hat)` and `dot_transform(FFT, a_hat, c_hat, s_hat)` with ifftn(a_hat) computed
    once -- nine inverse and four forward transforms instead of twelve and four.  a_hat, b_hat, c_hat and out_hat are
    DeviceArrays of shape (3,) + FFT.complex_shape(), s_hat has FFT.complex_shape().  out_hat may be a_hat or b_hat, s_hat
    may be any one component of c_hat (`c_hat.component(1)`); the inputs are otherwise preserved.  On slab plans with radix
    kernels on every axis the z stages are one fused kernel and no real-space work array exists
    (`FFT.plan_info("nonlinear_cross_dot_fused_3_2")`); elsewhere the plan composes it on twelve work arrays of its own.
    There is no `absmax` here: take the maxima of a CFL step from one `cross_transform(.., absmax=True)`."""
    _nonlinear(FFT, "nonlinear_cross_dot", [(a_hat, True), (b_hat, True), (c_hat, True), (out_hat, True), (s_hat, False)], dealias)
    return out_hat, s_hat


def outer_transform(FFT, a_hat, b_hat, out_hat, dealias=None):
    """out_hat[3 * i + j] = fftn(ifftn(a_hat[i]) * ifftn(b_hat[j])), all nine products of two vector fields as ONE operation of
    the plan (mfft_nonlinear_outer): the Elsasser products z+_i z-_j of incompressible MHD, a convective term in conservative
    form, a stress u_i u_j -- what a caller composes from six `FFT.ifftn(.., dealias)`, nine products of numpy arrays and nine
    `FFT.fftn(.., dealias)`, or today from three `cross_transform` calls (eighteen inverse and nine forward transforms instead
    of six and nine).  a_hat and b_hat are DeviceArrays of shape (3,) + FFT.complex_shape(), out_hat = FFT.empty_complex(9) has
    shape (9,) + FFT.complex_shape(): component 3 * i + j belongs to a_hat[i] and b_hat[j].  a_hat may be b_hat (the symmetric
    tensor, all nine components computed).  out_hat may NOT overlap a_hat or b_hat: the call raises before anything runs; the
    inputs are preserved.  On slab plans with radix kernels on every axis the z stages are one fused kernel and no real-space
    work array exists (`FFT.plan_info("nonlinear_outer_fused_3_2")`); elsewhere the plan composes it on seven work arrays of
    its own."""
    _nonlinear(FFT, "nonlinear_outer", [(a_hat, True), (b_hat, True), (out_hat, 9)], dealias)
    return out_hat


def elsasser_rhs(FFT, K, T_hat, Zp_hat, Zm_hat, dZp, dZm, nu, eta):
    """The right-hand sides of incompressible MHD in Elsasser variables z+- = u +- b in one sweep (mfft_ew_elsasser_rhs).
    T_hat = outer_transform(FFT, Zp_hat, Zm_hat, ..), shape (9,) + FFT.complex_shape(); the others (3,) + that.  Per bin
        N+[i] = -1j * sum_j K[j] * T_hat[3 * i + j],    N-[i] = -1j * sum_j K[j] * T_hat[3 * j + i],
    both projected, N - K (K . N) / |K|^2 with the K = 0 bin set to 0, and
        dZp[i] = N+[i] - |K|^2 ((nu + eta) / 2 * Zp_hat[i] + (nu - eta) / 2 * Zm_hat[i]),   dZm likewise with Zp_hat, Zm_hat swapped.
    dZp and dZm are arrays of their own; pitched spectra are swept as they lie in memory, like `ns_rhs`.  Returns (dZp, dZm)."""
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert T_hat.shape == (9,) + cs, (T_hat.shape, cs)
    for x in (Zp_hat, Zm_hat, dZp, dZm):
        assert x.shape == (3,) + cs and x.pitch == T_hat.pitch, (x.shape, x.pitch, cs, T_hat.pitch)
    for x in (T_hat, Zp_hat, Zm_hat, dZp, dZm):
        assert x.dtype == np.dtype(FFT.complex), (x.dtype, FFT.complex)
    _lib.call("mfft_ew_elsasser_rhs", FFT._plan, T_hat.ptr, Zp_hat.ptr, Zm_hat.ptr, dZp.ptr, dZm.ptr, K.dev[0].ptr, K.dev[1].ptr,
              K.dev[2].ptr, K.cshape, float(nu), float(eta), _prec(FFT))
    return dZp, dZm


def _max_over_ranks(FFT, v):
    """Maximum over FFT.comm that keeps NaNs: the NaN flags are reduced beside the values and the NaNs put back."""
    from .comm import MAX
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    both = np.concatenate([np.where(nan, 0.0, v).ravel(), nan.astype(np.float64).ravel()])
    both = np.asarray(FFT.comm.allreduce(both, op=MAX)).reshape(2, -1)
    return np.where(both[1] > 0.0, np.nan, both[0]).reshape(v.shape)


def nonlinear_absmax(FFT, reduce=True):
    """The six real-space maxima of the LAST `cross_transform` / `dot_transform` with `absmax=True`, a (2, 3) float64
    array: [0][f] = max |ifftn(a_hat[f], dealias)|, [1][f] = max |ifftn(b_hat[f], dealias)| over the grid the product
    was formed on (the padded grid under the 3/2-rule, the masked field under the 2/3-rule).  One synchronisation of the
    plan's stream; with `reduce` the maximum over FFT.comm (every rank calls it), else this rank's x planes only.  A NaN
    anywhere in a field gives NaN; the values are bitwise reproducible.  Raises if no such call has run on the plan."""
    FFT.comm.use_device()
    out = np.zeros(6, dtype=np.float64)
    _lib.call("mfft_plan_nonlinear_absmax", FFT._plan, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    out = out.reshape(2, 3)
    return _max_over_ranks(FFT, out) if reduce else out


def absmax(FFT, x, reduce=False):
    """max |x| of a real DeviceArray (mfft_ew_absmax, the companion of `sumsq`): a float for an array of the real shape,
    a float64 vector of three for (3,) + the real shape (any leading extent of 1, 2, 3 or 6 is taken as components).
    NaNs are kept.  With `reduce` the maximum over FFT.comm."""
    if x.pitch is not None:
        raise ValueError("absmax of a pitched array would look at the elements between its rows")
    assert x.dtype == np.dtype(FFT.float), (x.dtype, FFT.float)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    FFT.comm.use_device()
    out = np.zeros(6, dtype=np.float64)
    _lib.call("mfft_ew_absmax", FFT._plan, x.ptr, ncomp, x.size // ncomp, _prec(FFT), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    out = out[:ncomp]
    if reduce:
        out = _max_over_ranks(FFT, out)
    return float(out[0]) if len(x.shape) != 4 else out


class Moments(object):
    """Raw one-point statistics of `nfields` real fields over `count` points: `min`, `max` of shape (nfields,), `sums` of
    shape (nfields, 4) with sums[f, p - 1] = sum (x - center[f])^p, and the `center` they were taken about.  The derived
    numbers are formed on the host in np.longdouble from the raw sums, about the MEAN whatever the centre was."""

    def __init__(self, count, mn, mx, sums, center):
        self.count = int(count)
        self.min = np.asarray(mn, dtype=np.float64)
        self.max = np.asarray(mx, dtype=np.float64)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, 4)
        self.center = np.asarray(center, dtype=np.float64)

    def _central(self):
        """(delta, mu2, mu3, mu4): the mean minus the centre and the central moments, long double."""
        m = self.sums.astype(np.longdouble) / np.longdouble(self.count)
        d = m[:, 0]
        mu2 = m[:, 1] - d * d
        mu3 = m[:, 2] - 3 * d * m[:, 1] + 2 * d ** 3
        mu4 = m[:, 3] - 4 * d * m[:, 2] + 6 * d * d * m[:, 1] - 3 * d ** 4
        return d, mu2, mu3, mu4

    def mean(self):
        return self.center.astype(np.longdouble) + self._central()[0]

    def variance(self):
        return self._central()[1]

    def skewness(self):
        _, mu2, mu3, _ = self._central()
        with np.errstate(divide="ignore", invalid="ignore"):      # (a field that is constant has none: nan)
            return mu3 / mu2 ** np.longdouble(1.5)

    def flatness(self):
        _, mu2, _, mu4 = self._central()
        with np.errstate(divide="ignore", invalid="ignore"):
            return mu4 / (mu2 * mu2)


def _moments_result(FFT, raw, count, center, reduce):
    raw = np.asarray(raw, dtype=np.float64).reshape(-1, 6)
    mn, mx, sums = raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2:].copy()
    if reduce:
        # sums and count: comm.allreduce adds in rank order, the same bits on every rank; the extremes keep their NaNs
        tot = np.asarray(FFT.comm.allreduce(np.concatenate([sums.ravel(), [float(count)]])))
        sums, count = tot[:-1].reshape(-1, 4), int(round(float(tot[-1])))
        mx = _max_over_ranks(FFT, mx)
        mn = -_max_over_ranks(FFT, -mn)
    return Moments(count, mn, mx, sums, center)


def _centers(center, nfields):
    c = np.zeros(nfields, dtype=np.float64) if center is None else np.asarray(center, dtype=np.float64).reshape(-1) * np.ones(nfields)
    assert c.shape == (nfields,), (c.shape, nfields)
    return np.ascontiguousarray(c)


def _real_fields(FFT, a_hat, b_hat):
    """The opening of the `real_*` statistics: a_hat of FFT.complex_shape() or (3,) + that, b_hat None or of the same shape.
    Returns the fields as `_nonlinear` takes them, the components per field, the number of fields (a's first) and the head of
    the library call's arguments."""
    cs = tuple(int(s) for s in FFT.complex_shape())
    assert a_hat.shape in (cs, (3,) + cs), (a_hat.shape, cs)
    vec = len(a_hat.shape) == 4
    fields = [(a_hat, vec)] + ([(b_hat, vec)] if b_hat is not None else [])
    ncomp = 3 if vec else 1
    return fields, ncomp, ncomp * len(fields), (a_hat.ptr, b_hat.ptr if b_hat is not None else None, ncomp)


def real_moments(FFT, a_hat, b_hat=None, dealias=None, center=None, reduce=True):
    """One-point statistics of fields that exist as SPECTRA only (mfft_real_moments): minimum, maximum and the sums of the
    first four powers of ifftn(a_hat[f], dealias) -- and of ifftn(b_hat[f], dealias) where b_hat is given -- without a real
    array: on slab plans with radix kernels on every axis the z stage ends in a reduction
    (`FFT.plan_info("nonlinear_moments_fused_3_2")`); elsewhere the plan transforms one field at a time into ONE work array
    and sweeps it.  a_hat is a DeviceArray of FFT.complex_shape() or (3,) + that, b_hat None or of the same shape: 1, 2, 3 or
    6 fields, a's first.  The grid is the one a product would be formed on (the padded one under the 3/2-rule, the masked
    field under the 2/3-rule, as `nonlinear_absmax`).  Returns a `Moments`; with `reduce` over FFT.comm (every rank calls it,
    every rank gets the same bits), else this rank's x planes.  `center` (a float or one per field): the sums are taken about
    it.  Moments about a centre far from the mean lose digits as (mean / sigma)^p when the central moments are formed from
    them -- a scalar of mean 3 and deviation 1e-3 keeps nothing of its flatness about 0 -- and that is what `center` is
    for: pass the mean (a_hat[0, 0, 0] / N^3 on the rank that holds it).  A NaN or Inf anywhere in a field gives NaN sums for
    that field; the values are bitwise reproducible.  Synchronises the plan's stream; the inputs are preserved."""
    fields, ncomp, nfields, head = _real_fields(FFT, a_hat, b_hat)
    c = _centers(center, nfields)
    out = np.zeros(nfields * 6, dtype=np.float64)
    count = ctypes.c_int64(0)
    dp = ctypes.POINTER(ctypes.c_double)
    _nonlinear(FFT, "real_moments", fields, dealias, head=head,
               tail=(c.ctypes.data_as(dp), out.ctypes.data_as(dp), ctypes.byref(count)))
    return _moments_result(FFT, out, count.value, c, reduce)


def moments(FFT, x, center=None, reduce=False):
    """The same statistics of a real DeviceArray (mfft_ew_moments, the companion of `absmax` and `sumsq`): an array of the
    real shape is one field, (3,) + the real shape three (any leading extent of 1, 2, 3 or 6 is taken as components).
    Returns a `Moments`; with `reduce` over FFT.comm."""
    if x.pitch is not None:
        raise ValueError("moments of a pitched array would count the elements between its rows")
    assert x.dtype == np.dtype(FFT.float), (x.dtype, FFT.float)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    c = _centers(center, ncomp)
    FFT.comm.use_device()
    out = np.zeros(36, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.call("mfft_ew_moments", FFT._plan, x.ptr, ncomp, x.size // ncomp, _prec(FFT), c.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return _moments_result(FFT, out[:ncomp * 6], x.size // ncomp, c, reduce)


HIST_MAXBINS = 512      # bins per field of one call (MFFT_HIST_MAXBINS: what a workgroup's LDS histograms hold)


def hist_slots(x, lo, hi, nbins):
    """The slot rule of the histograms, in numpy float64 (include/mpifft4py_amd.h): 0 below lo, 1 .. nbins the equal bins of
    [lo, hi), nbins + 1 at or above hi, nbins + 2 not a number.  The device evaluates the same expressions in the same order."""
    x = np.asarray(x, dtype=np.float64)
    inv = np.float64(nbins) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - np.float64(lo)) * inv
        inside = ~(x != x) & ~(t < 0) & ~(t >= nbins)
        s = np.where(inside, 1 + np.where(inside, t, 0.0).astype(np.int64), 0)
    s = np.where(t >= nbins, nbins + 1, s)
    s = np.where(t < 0, 0, s)
    return np.where(x != x, nbins + 2, s)


class Histogram(object):
    """Counts of `nfields` real fields over `count` points in `nbins` equal bins of [lo[f], hi[f]): `counts` of shape
    (nfields, nbins), int64; `below` (x < lo), `above` (x >= hi) and `nonfinite` (NaN) of shape (nfields,).  For every field
    counts[f].sum() + below[f] + above[f] + nonfinite[f] == count."""

    def __init__(self, count, raw, lo, hi):
        raw = np.asarray(raw, dtype=np.int64)
        raw = raw.reshape(len(np.atleast_1d(lo)), -1)
        self.count = int(count)
        self.below = raw[:, 0].copy()
        self.counts = raw[:, 1:-2].copy()
        self.above = raw[:, -2].copy()
        self.nonfinite = raw[:, -1].copy()
        self.lo = np.atleast_1d(np.asarray(lo, dtype=np.float64)).copy()
        self.hi = np.atleast_1d(np.asarray(hi, dtype=np.float64)).copy()

    @property
    def nbins(self):
        return int(self.counts.shape[1])

    def edges(self, f=0):
        """The nbins + 1 edges of field f's bins."""
        return self.lo[f] + (self.hi[f] - self.lo[f]) * (np.arange(self.nbins + 1, dtype=np.float64) / self.nbins)

    def centers(self, f=0):
        e = self.edges(f)
        return 0.5 * (e[:-1] + e[1:])

    def pdf(self, f=0):
        """The density over [lo, hi), normalised by ALL `count` points: it integrates to 1 - (below + above + nonfinite) / count."""
        return self.counts[f] / (float(self.count) * (self.hi[f] - self.lo[f]) / self.nbins)

    def cdf(self, f=0):
        """P(x < edge) at the nbins + 1 edges: below / count at lo, (count - above - nonfinite) / count at hi."""
        c = np.concatenate([[self.below[f]], self.below[f] + np.cumsum(self.counts[f])])
        return c / float(self.count)

    def quantile(self, f, q):
        """The x with cdf(x) = q, the counts taken as uniform inside their bin; nan where q lies in a tail outside [lo, hi)."""
        c, e = self.cdf(f), self.edges(f)
        q = np.asarray(q, dtype=np.float64)
        j = np.clip(np.searchsorted(c, q, side="right") - 1, 0, self.nbins - 1)
        d = c[j + 1] - c[j]
        x = e[j] + np.where(d > 0, (q - c[j]) / np.where(d > 0, d, 1.0), 0.0) * (e[j + 1] - e[j])
        return np.where((q < c[0]) | (q > c[-1]), np.nan, x)


def _add_over_ranks(FFT, v):
    """int64 counts added over FFT.comm exactly: the communicator adds doubles, so 24 low bits and the rest travel apart."""
    v = np.asarray(v, dtype=np.int64)
    if FFT.comm.Get_size() == 1:
        return v.copy()
    parts = np.concatenate([(v & 0xFFFFFF).ravel(), (v >> 24).ravel()]).astype(np.float64)
    tot = np.rint(np.asarray(FFT.comm.allreduce(parts))).astype(np.int64)
    return (tot[:v.size] + (tot[v.size:] << 24)).reshape(v.shape)


def _hist_ranges(rng, nfields):
    r = np.asarray(rng, dtype=np.float64)
    if r.shape == (2,):
        r = np.tile(r, (nfields, 1))
    assert r.shape == (nfields, 2), (r.shape, nfields)
    return np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])


def _hist_check(lo, hi, bins):
    if not 1 <= int(bins) <= HIST_MAXBINS:
        raise ValueError("bins must be 1 .. %d, not %r" % (HIST_MAXBINS, bins))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("every range needs finite lo < hi, not %r .. %r" % (lo, hi))


def _range_of_moments(m, what):
    """Every field's [min, max] as a histogram range: hi widened by (max - min) * 2^-20 so that the maximum falls inside; a
    constant field gets a range of width 1 about its value."""
    if not (np.all(np.isfinite(m.min)) and np.all(np.isfinite(m.max))):
        raise ValueError("a %s is not finite (min %r, max %r): give `range`" % (what, m.min, m.max))
    lo, hi = m.min.copy(), np.maximum(m.max + (m.max - m.min) * 2.0 ** -20, np.nextafter(m.max, np.inf))
    const = ~(m.min < m.max)
    lo[const], hi[const] = m.min[const] - 0.5, m.min[const] + 0.5
    return lo, hi


def real_histogram(FFT, a_hat, b_hat=None, dealias=None, bins=256, range=None, reduce=True):
    """Histograms of fields that exist as SPECTRA only (mfft_real_histogram): the counts of ifftn(a_hat[f], dealias) -- and of
    ifftn(b_hat[f], dealias) where b_hat is given -- in `bins` equal bins per field, without a real array: on slab plans with
    radix kernels on every axis the z stage ends in a histogram (`FFT.plan_info("nonlinear_histogram_fused_3_2")`), elsewhere
    the plan transforms one field at a time into ONE work array and sweeps it.  Fields and grid as `real_moments`.  `range` is
    (lo, hi) for all fields or one pair per field; None: a `real_moments` call runs first and every field gets its own
    [min, max] over FFT.comm, hi widened by (max - min) * 2^-20 so that the maximum falls inside (a constant field: a range
    of width 1 about its value).  Returns a `Histogram`; with `reduce` the int64 counts are added over FFT.comm (every rank
    calls it, every rank gets the same arrays).  Counts are integers: the result is the same bits run to run, on every device
    and for every number of ranks that computes the same values.  Synchronises the plan's stream; the inputs are preserved."""
    fields, ncomp, nfields, head = _real_fields(FFT, a_hat, b_hat)
    if range is None:
        m = real_moments(FFT, a_hat, b_hat, dealias, reduce=True)
        lo, hi = _range_of_moments(m, "field")
    else:
        lo, hi = _hist_ranges(range, nfields)
    _hist_check(lo, hi, bins)
    out = np.zeros((nfields, int(bins) + 3), dtype=np.int64)
    count = ctypes.c_int64(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _nonlinear(FFT, "real_histogram", fields, dealias, head=head,
               tail=(lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), int(bins), out.ctypes.data_as(ip), ctypes.byref(count)))
    n = count.value
    if reduce:
        out, n = _add_over_ranks(FFT, out), int(_add_over_ranks(FFT, [n])[0])
    return Histogram(n, out, lo, hi)


def histogram(FFT, x, bins=256, range=None, reduce=False):
    """The histogram of a real DeviceArray (mfft_ew_histogram, the companion of `moments`): an array of the real shape is one
    field, a leading extent of 1, 2, 3 or 6 is taken as components.  `range` as in `real_histogram`; None: the components'
    [min, max] from `moments` (over FFT.comm with `reduce`).  Returns a `Histogram`; with `reduce` over FFT.comm."""
    if x.pitch is not None:
        raise ValueError("a histogram of a pitched array would count the elements between its rows")
    assert x.dtype == np.dtype(FFT.float), (x.dtype, FFT.float)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    if range is None:
        m = moments(FFT, x, reduce=reduce)
        lo, hi = _range_of_moments(m, "component")
    else:
        lo, hi = _hist_ranges(range, ncomp)
    _hist_check(lo, hi, bins)
    FFT.comm.use_device()
    out = np.zeros((ncomp, int(bins) + 3), dtype=np.int64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _lib.call("mfft_ew_histogram", FFT._plan, x.ptr, ncomp, x.size // ncomp, _prec(FFT), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
              int(bins), out.ctypes.data_as(ip))
    n = x.size // ncomp
    if reduce:
        out, n = _add_over_ranks(FFT, out), int(_add_over_ranks(FFT, [n])[0])
    return Histogram(n, out, lo, hi)


JOINT_MAXBINS = 64      # bins per field of one joint call (MFFT_JOINT_MAXBINS: (64 + 3)^2 cells are what a workgroup's LDS holds)


def joint_cells(xa, xb, lo, hi, bins):
    """The cell rule of the joint histograms, in numpy float64 (include/mpifft4py_amd.h): cell = sa * (nbb + 3) + sb with
    sa = hist_slots(xa, lo[0], hi[0], nba), sb = hist_slots(xb, lo[1], hi[1], nbb); `bins` is an int or (nba, nbb)."""
    nba, nbb = _joint_bins(bins)
    return hist_slots(xa, lo[0], hi[0], nba) * (nbb + 3) + hist_slots(xb, lo[1], hi[1], nbb)


def _joint_bins(bins):
    nba, nbb = (int(bins), int(bins)) if np.ndim(bins) == 0 else (int(bins[0]), int(bins[1]))
    return nba, nbb


def _joint_check(lo, hi, nba, nbb):
    if not (1 <= nba <= JOINT_MAXBINS and 1 <= nbb <= JOINT_MAXBINS):
        raise ValueError("bins must be 1 .. %d per field, not %r: a finer PDF is a second call on a narrower range" % (JOINT_MAXBINS, (nba, nbb)))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("every range needs finite lo < hi, not %r .. %r" % (lo, hi))


class JointHistogram(object):
    """Counts of `npairs` pairs of real fields (a_p, b_p) over `count` points in nba x nbb equal bins of [lo[p, 0], hi[p, 0]) x
    [lo[p, 1], hi[p, 1]): `raw` of shape (npairs, nba + 3, nbb + 3), int64, rows and columns in slot order (0 below, 1 .. nb the
    bins, nb + 1 at or above hi, nb + 2 not a number); `counts` = raw[:, 1:-2, 1:-2] of shape (npairs, nba, nbb).  For every
    pair raw[p].sum() == count."""

    def __init__(self, count, raw, lo, hi, bins):
        nba, nbb = _joint_bins(bins)
        self.count = int(count)
        self.raw = np.asarray(raw, dtype=np.int64).reshape(-1, nba + 3, nbb + 3).copy()
        self.counts = self.raw[:, 1:-2, 1:-2].copy()
        self.lo = np.asarray(lo, dtype=np.float64).reshape(self.raw.shape[0], 2).copy()      # [pair][a, b]
        self.hi = np.asarray(hi, dtype=np.float64).reshape(self.raw.shape[0], 2).copy()

    @property
    def npairs(self):
        return int(self.raw.shape[0])

    @property
    def nbins(self):
        return (int(self.counts.shape[1]), int(self.counts.shape[2]))

    def outside(self, p=0):
        """The points of pair p with either value below, above or not a number: count - counts[p].sum()."""
        return int(self.raw[p].sum() - self.counts[p].sum())

    def edges(self, p=0, axis=0):
        """The nb + 1 edges of the bins of pair p's field a (axis 0) or b (axis 1)."""
        nb = self.nbins[axis]
        return self.lo[p, axis] + (self.hi[p, axis] - self.lo[p, axis]) * (np.arange(nb + 1, dtype=np.float64) / nb)

    def centers(self, p=0, axis=0):
        e = self.edges(p, axis)
        return 0.5 * (e[:-1] + e[1:])

    def pdf(self, p=0):
        """The density over the rectangle, normalised by ALL `count` points: times the cell area it sums to 1 - outside(p) / count."""
        area = (self.hi[p, 0] - self.lo[p, 0]) / self.nbins[0] * (self.hi[p, 1] - self.lo[p, 1]) / self.nbins[1]
        return self.counts[p] / (float(self.count) * area)

    def marginal(self, axis=0):
        """The `Histogram` of the a fields (axis 0) or the b fields (axis 1): the row or column sums, border slots included, so
        that below, above and nonfinite are those of the one-dimensional histogram of the same range and bins."""
        return Histogram(self.count, self.raw.sum(axis=2 - axis), self.lo[:, axis], self.hi[:, axis])

    def conditional_mean(self, p=0, of=1):
        """<b | a in bin i> (of=1; of=0: <a | b in bin j>) from the bin centres of the averaged field, over the points inside the
        rectangle; NaN where a row is empty.  Exact only to half a bin width of the averaged field."""
        c = self.counts[p] if of == 1 else self.counts[p].T
        n = c.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, (c * self.centers(p, of)[None, :]).sum(axis=1) / np.where(n > 0, n, 1), np.nan)


def _joint_ranges(rng, ncomp):
    """(lo, hi) in the order of the C interface, a_0.., then b_0..: `rng` is ((lo_a, hi_a), (lo_b, hi_b)) for all pairs, or
    of shape (npairs, 2, 2), [pair][a, b][lo, hi]."""
    r = np.asarray(rng, dtype=np.float64)
    if r.shape == (2, 2):
        r = np.tile(r, (ncomp, 1, 1))
    assert r.shape == (ncomp, 2, 2), (r.shape, ncomp)
    return np.ascontiguousarray(r[:, :, 0].T.ravel()), np.ascontiguousarray(r[:, :, 1].T.ravel())


def _joint_result(FFT, n, out, lo, hi, ncomp, nba, nbb, reduce):
    if reduce:
        out, n = _add_over_ranks(FFT, out), int(_add_over_ranks(FFT, [n])[0])
    return JointHistogram(n, out, lo.reshape(2, ncomp).T, hi.reshape(2, ncomp).T, (nba, nbb))


def real_joint_histogram(FFT, a_hat, b_hat, dealias=None, bins=64, range=None, reduce=True):
    """Joint histograms of fields that exist as SPECTRA only (mfft_real_joint_histogram): the counts of the points
    (ifftn(a_hat[p], dealias), ifftn(b_hat[p], dealias)) in a grid of `bins` = nba x nbb equal bins per pair (an int: the same for
    both), p over the 1 or 3 components -- the joint PDF of two fields at the same grid point, which no pair of marginal
    histograms gives.  On slab plans with radix kernels on every axis the z stage ends in the grid
    (`FFT.plan_info("nonlinear_joint_fused_3_2")`): a pair rides ONE inverse transform, one thread holds both values, no real
    array exists.  Elsewhere the plan transforms a_p and b_p into TWO real work arrays -- the least a pair can do with -- and
    sweeps them.  At most JOINT_MAXBINS = 64 bins per field ((64 + 3)^2 cells are what a workgroup's LDS holds next to its
    exchange buffers): a finer PDF is a second call on a narrower `range`.  `range` is ((lo_a, hi_a), (lo_b, hi_b)) for all
    pairs or of shape (npairs, 2, 2); None: ONE `real_moments` call runs first and every field gets its own [min, max] over
    FFT.comm, widened as in `real_histogram`, so every point falls inside.  b_hat may be a_hat.  Returns a `JointHistogram`;
    with `reduce` the int64 counts are added over FFT.comm.  Counts are integers: the same bits run to run and for every number
    of ranks of a fused slab plan.  Synchronises the plan's stream; the inputs are preserved."""
    if b_hat is None:
        raise ValueError("a joint histogram counts pairs of fields: b_hat must be given")
    assert b_hat.shape == a_hat.shape, (a_hat.shape, b_hat.shape)
    fields, ncomp, _, head = _real_fields(FFT, a_hat, b_hat)
    nba, nbb = _joint_bins(bins)
    if range is None:
        lo, hi = _range_of_moments(real_moments(FFT, a_hat, b_hat, dealias, reduce=True), "field")      # (a_0.., then b_0..)
    else:
        lo, hi = _joint_ranges(range, ncomp)
    _joint_check(lo, hi, nba, nbb)
    out = np.zeros((ncomp, nba + 3, nbb + 3), dtype=np.int64)
    count = ctypes.c_int64(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _nonlinear(FFT, "real_joint_histogram", fields, dealias, head=head,
               tail=(lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), nba, nbb, out.ctypes.data_as(ip), ctypes.byref(count)))
    return _joint_result(FFT, count.value, out, lo, hi, ncomp, nba, nbb, reduce)


def joint_histogram(FFT, x, y, bins=64, range=None, reduce=False):
    """The joint histogram of two real DeviceArrays of the same shape (mfft_ew_joint_histogram, the companion of `histogram`):
    arrays of the real shape are one pair, a leading extent of 1 or 3 is taken as components, pair p = (x[p], y[p]).  `bins`
    and `range` as in `real_joint_histogram`; None: the components' [min, max] from `moments` (over FFT.comm with `reduce`).
    Returns a `JointHistogram`; with `reduce` over FFT.comm."""
    if x.pitch is not None or y.pitch is not None:
        raise ValueError("a histogram of a pitched array would count the elements between its rows")
    assert x.dtype == np.dtype(FFT.float) and y.dtype == x.dtype and x.shape == y.shape, (x.dtype, y.dtype, x.shape, y.shape)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    assert ncomp in (1, 3), ncomp
    nba, nbb = _joint_bins(bins)
    if range is None:
        lx, hx = _range_of_moments(moments(FFT, x, reduce=reduce), "component")
        ly, hy = _range_of_moments(moments(FFT, y, reduce=reduce), "component")
        lo, hi = np.concatenate([lx, ly]), np.concatenate([hx, hy])
    else:
        lo, hi = _joint_ranges(range, ncomp)
    _joint_check(lo, hi, nba, nbb)
    FFT.comm.use_device()
    out = np.zeros((ncomp, nba + 3, nbb + 3), dtype=np.int64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _lib.call("mfft_ew_joint_histogram", FFT._plan, x.ptr, y.ptr, ncomp, x.size // ncomp, _prec(FFT), lo.ctypes.data_as(dp),
              hi.ctypes.data_as(dp), nba, nbb, out.ctypes.data_as(ip))
    return _joint_result(FFT, x.size // ncomp, out, lo, hi, ncomp, nba, nbb, reduce)


def quad_rule(r, weights):
    """The evaluation rule of the quadratic forms, in numpy float64 (include/mpifft4py_amd.h): r of shape (n, ...) holds the
    fields' values in SLOT order (`quad_slot_order`), q = 0, then q = q + (w_f * r_f) * r_f field by field -- every product
    and sum rounded on its own (numpy never contracts), which is what the device computes."""
    r = np.asarray(r, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    assert r.shape[0] == w.shape[0], (r.shape, w.shape)
    q = np.zeros(r.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(r.shape[0]):
            q = q + (w[f] * r[f]) * r[f]
    return q


def quad_slot_order(nfields, two):
    """The order in which `real_quadratic` adds its fields: a's components as they come where a_hat stands alone; with b_hat,
    a_f and b_f share a transform and the order is a_0, b_0, a_1, b_1, a_2, b_2 (indices into a's fields, then b's)."""
    if not two:
        return list(range(nfields))
    ncomp = nfields // 2
    return [i for f in range(ncomp) for i in (f, ncomp + f)]


def _quad_args(weights, nfields, center, bins, rng):
    w = np.ones(nfields, dtype=np.float64) if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.shape != (nfields,):
        raise ValueError("%d weights for %d fields" % (w.size, nfields))
    if not np.all(np.isfinite(w)):
        raise ValueError("every weight must be finite, not %r" % (w,))
    if not 0 <= int(bins) <= HIST_MAXBINS:
        raise ValueError("bins must be 0 .. %d, not %r" % (HIST_MAXBINS, bins))
    lo, hi = (0.0, 1.0) if rng is None else (float(rng[0]), float(rng[1]))
    if int(bins) > 0 and not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("the range needs finite lo < hi, not %r .. %r" % (lo, hi))
    return w, float(center), lo, hi


def _quad_range(m):
    """[min, max] of a first call without bins, widened as in `real_histogram`."""
    mn, mx = float(m.min[0]), float(m.max[0])
    if not (np.isfinite(mn) and np.isfinite(mx)):
        raise ValueError("q is not finite (min %r, max %r): give `range`" % (mn, mx))
    if not mn < mx:
        return mn - 0.5, mn + 0.5
    return mn, float(max(mx + (mx - mn) * 2.0 ** -20, np.nextafter(mx, np.inf)))


def _quad_result(FFT, out6, counts, n, center, bins, lo, hi, reduce):
    m = _moments_result(FFT, out6, n, np.array([center]), reduce)
    if not bins:
        return m, None
    if reduce:
        counts, n = _add_over_ranks(FFT, counts), int(_add_over_ranks(FFT, [n])[0])
    return m, Histogram(n, counts.reshape(1, -1), [lo], [hi])


def real_quadratic(FFT, a_hat, b_hat=None, dealias=None, weights=None, center=0.0, bins=0, range=None, reduce=True):
    """Statistics of a QUADRATIC FORM of fields that exist as spectra only (mfft_real_quadratic):
        q(x) = sum_f weights[f] * ifftn(field f, dealias)(x)**2
    over the components of a_hat and, where given, of b_hat (1, 2, 3 or 6 fields, a's first; `weights` None: all ones) --
    enstrophy density (the curl, weights 1), dissipation (`strain_hat`, weights 2 nu (1, 1, 1, 2, 2, 2)), energy density --
    whose moments and PDF do not follow from those of the single fields.  Returns (`Moments`, `Histogram` or None), each of ONE
    field: min, max and the sums of (q - center)**p, p = 1..4, and with `bins` > 0 the counts of q in `bins` equal bins of
    `range` = (lo, hi) by the slot rule of `real_histogram`.  bins > 0 with range None: a first call without bins gives
    [min, max] over FFT.comm, widened as in `real_histogram`.  Fields, grid and routes as `real_moments`
    (`FFT.plan_info("nonlinear_quadratic_fused_3_2")`): fused, the z kernel accumulates q in registers across the inverse
    transforms of a row and no real array exists; elsewhere one field at a time goes through ONE work array into ONE array of
    doubles.  q follows ONE rule on every route (`quad_rule`, fields in `quad_slot_order`).  A NaN or Inf in any field gives
    NaN statistics and counts in the non-finite slot.  With `reduce` over FFT.comm; bitwise reproducible.  Synchronises the
    plan's stream; the inputs are preserved."""
    fields, ncomp, nfields, head = _real_fields(FFT, a_hat, b_hat)
    w, center, lo, hi = _quad_args(weights, nfields, center, bins, range)
    if int(bins) > 0 and range is None:
        lo, hi = _quad_range(real_quadratic(FFT, a_hat, b_hat, dealias, w, center, 0, None, True)[0])
    out6 = np.zeros(6, dtype=np.float64)
    counts = np.zeros(int(bins) + 3, dtype=np.int64)
    count = ctypes.c_int64(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _nonlinear(FFT, "real_quadratic", fields, dealias, head=head,
               tail=(w.ctypes.data_as(dp), center, lo, hi, int(bins), out6.ctypes.data_as(dp), counts.ctypes.data_as(ip), ctypes.byref(count)))
    return _quad_result(FFT, out6, counts, count.value, center, int(bins), lo, hi, reduce)


def quadratic(FFT, x, weights=None, center=0.0, bins=0, range=None, reduce=False):
    """The same statistics of q = sum_c weights[c] * x[c]**2 of a real DeviceArray (mfft_ew_quadratic, the companion of `moments`
    and `histogram`): an array of the real shape is one field, a leading extent of 1, 2, 3 or 6 is taken as components, added
    in that order.  q is formed on the fly in one sweep; there is no q array.  Returns (`Moments`, `Histogram` or None)."""
    if x.pitch is not None:
        raise ValueError("a quadratic form of a pitched array would count the elements between its rows")
    assert x.dtype == np.dtype(FFT.float), (x.dtype, FFT.float)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    w, center, lo, hi = _quad_args(weights, ncomp, center, bins, range)
    if int(bins) > 0 and range is None:
        lo, hi = _quad_range(quadratic(FFT, x, w, center, 0, None, reduce)[0])
    FFT.comm.use_device()
    out6 = np.zeros(6, dtype=np.float64)
    counts = np.zeros(int(bins) + 3, dtype=np.int64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _lib.call("mfft_ew_quadratic", FFT._plan, x.ptr, ncomp, x.size // ncomp, _prec(FFT), w.ctypes.data_as(dp), center, lo, hi, int(bins),
              out6.ctypes.data_as(dp), counts.ctypes.data_as(ip))
    return _quad_result(FFT, out6, counts, x.size // ncomp, center, int(bins), lo, hi, reduce)


INCR_MAXSEP = 8         # separations of one call (MFFT_INCR_MAXSEP: what one launch's accumulators hold); longer lists go in chunks


def incr_rule(r, seps):
    """The rule of the increments, in numpy float64 (include/mpifft4py_amd.h): r of shape (..., M) holds periodic rows along its
    last axis (normalised values, already double); returns sums[i] = [S2, S3, S4] of d = r[(z + seps[i]) mod M] - r[z] over all
    rows and positions, shape (len(seps), 3)."""
    r = np.asarray(r, dtype=np.float64)
    out = np.zeros((len(seps), 3), dtype=np.float64)
    for i, s in enumerate(seps):
        d = np.roll(r, -int(s), axis=-1) - r
        d2 = d * d
        out[i] = (d2.sum(), (d2 * d).sum(), (d2 * d2).sum())
    return out


def default_seps(M):
    """The separations a call takes where none are given: the powers of two below M / 2, then M / 2."""
    M = int(M)
    seps, s = [], 1
    while s < M // 2:
        seps.append(s)
        s *= 2
    if M // 2 >= 1 and (not seps or seps[-1] != M // 2):
        seps.append(M // 2)
    return seps


class Increments(object):
    """Raw two-point statistics along z of `nfields` real fields over `count` points per field: `seps` (grid points of the z row
    of `M` points) and `sums` of shape (nfields, nsep, 3) with sums[f, i] = [S2, S3, S4], S_p = sum (x(z + s) - x(z))^p.  The
    derived numbers are formed on the host in np.longdouble.  On a velocity field 2 is the LONGITUDINAL structure function (the
    increment runs along z), fields 0 and 1 the transverse ones."""

    def __init__(self, count, seps, sums, M):
        self.count = int(count)
        self.seps = np.asarray(seps, dtype=np.int64).reshape(-1)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, self.seps.size, 3)
        self.M = int(M)

    def S(self, p):
        """The structure function of order p = 2, 3 or 4: <(x(z + s) - x(z))^p>, shape (nfields, nsep)."""
        if p not in (2, 3, 4):
            raise ValueError("orders 2, 3 and 4 are computed, not %r" % (p,))
        return self.sums[:, :, p - 2].astype(np.longdouble) / np.longdouble(self.count)

    def skewness(self):
        with np.errstate(divide="ignore", invalid="ignore"):      # (a field without increments has none: nan)
            return self.S(3) / self.S(2) ** np.longdouble(1.5)

    def flatness(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.S(4) / (self.S(2) * self.S(2))

    def r(self, FFT):
        """The separations as lengths: s * L_z / M."""
        return self.seps.astype(np.float64) * float(FFT.L[2]) / self.M


def _incr_chunks(seps, M):
    seps = default_seps(M) if seps is None else [int(s) for s in np.asarray(seps).reshape(-1)]
    if not seps:
        raise ValueError("no separations")
    return seps, [seps[i:i + INCR_MAXSEP] for i in range(0, len(seps), INCR_MAXSEP)]


def _incr_result(FFT, sums, count, seps, M, reduce):
    if reduce:      # sums and count: comm.allreduce adds in rank order, the same bits on every rank
        tot = np.asarray(FFT.comm.allreduce(np.concatenate([sums.ravel(), [float(count)]])))
        sums, count = tot[:-1].reshape(sums.shape), int(round(float(tot[-1])))
    return Increments(count, seps, sums, M)


def real_increments(FFT, a_hat, b_hat=None, dealias=None, seps=None, reduce=True):
    """Structure functions along z of fields that exist as SPECTRA only (mfft_real_increments): for every separation s in
    `seps` (grid points of the z row of M points: M = N[2], or 3 N[2] / 2 under the 3/2-rule; 1 <= s <= M - 1, periodic) the
    sums of the second, third and fourth powers of ifftn(field, dealias)(z + s) - ifftn(field, dealias)(z) -- the first
    two-point statistic, what the 4/5 law, the increment skewness and flatness and the intermittency exponents are read from --
    without a real array: on slab plans with radix kernels on every axis the z kernel keeps the real row in its exchange buffer
    and reads it back shifted (`FFT.plan_info("nonlinear_increments_fused_3_2")`); elsewhere the plan transforms one field at a
    time into ONE work array and sweeps it.  z is whole on every rank, so no halo is exchanged.  Fields as `real_moments`: 1, 2,
    3 or 6, a's first.  `seps=None`: the powers of two below M / 2, then M / 2.  One call of the library takes INCR_MAXSEP
    separations; a longer list is issued in chunks, and EACH CHUNK REPEATS THE TRANSFORMS.  Returns an `Increments`; with
    `reduce` the raw sums and the count are added over FFT.comm.  A NaN or Inf anywhere in a field gives NaN sums for that
    field; the values are bitwise reproducible.  Synchronises the plan's stream; the inputs are preserved."""
    fields, ncomp, nfields, head = _real_fields(FFT, a_hat, b_hat)
    M = int(FFT.N[2]) * 3 // 2 if dealias == '3/2-rule' else int(FFT.N[2])
    seps, chunks = _incr_chunks(seps, M)
    count = ctypes.c_int64(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    parts = []
    for ch in chunks:
        sv = np.ascontiguousarray(ch, dtype=np.int64)
        out = np.zeros(nfields * len(ch) * 3, dtype=np.float64)
        _nonlinear(FFT, "real_increments", fields, dealias, head=head,
                   tail=(sv.ctypes.data_as(ip), len(ch), out.ctypes.data_as(dp), ctypes.byref(count)))
        parts.append(out.reshape(nfields, len(ch), 3))
    return _incr_result(FFT, np.concatenate(parts, axis=1), count.value, seps, M, reduce)


def increments(FFT, u, seps=None, reduce=False):
    """The same sums of a real DeviceArray along its LAST axis (mfft_ew_increments, the companion of `moments`): an array of
    four axes is taken as (components, ..) with 1, 2, 3 or 6 components, any other as one field; the rows of the last axis are
    periodic, M = u.shape[-1], and a pitched array is swept as it lies.  `seps` and the chunks as `real_increments` (each chunk
    is one more sweep).  Returns an `Increments`; with `reduce` over FFT.comm."""
    assert u.dtype == np.dtype(FFT.float), (u.dtype, FFT.float)
    ncomp = int(u.shape[0]) if len(u.shape) == 4 else 1
    M = int(u.shape[-1])
    nrows = u.size // (ncomp * M)
    seps, chunks = _incr_chunks(seps, M)
    FFT.comm.use_device()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    parts = []
    for ch in chunks:
        sv = np.ascontiguousarray(ch, dtype=np.int64)
        out = np.zeros(ncomp * len(ch) * 3, dtype=np.float64)
        _lib.call("mfft_ew_increments", FFT._plan, u.ptr, ncomp, nrows, M, M if u.pitch is None else int(u.pitch), _prec(FFT),
                  sv.ctypes.data_as(ip), len(ch), out.ctypes.data_as(dp))
        parts.append(out.reshape(ncomp, len(ch), 3))
    return _incr_result(FFT, np.concatenate(parts, axis=1), nrows * M, seps, M, reduce)


INCR_HIST_MAXBINS = 256   # bins per field and separation of one call (MFFT_INCR_HIST_MAXBINS: 2 x 8 x 259 counts are a pair's share of LDS)


def incr_hist_rule(r, seps, lo, hi, bins):
    """The rule of the increment PDFs, in numpy float64 (include/mpifft4py_amd.h): r of shape (..., M) holds periodic rows along
    its last axis (normalised values, already double); lo, hi broadcastable to (len(seps),).  Returns the int64 counts of
    d = r[(z + seps[i]) mod M] - r[z] by the histograms' slot rule (`hist_slots`), shape (len(seps), bins + 3)."""
    r = np.asarray(r, dtype=np.float64)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (len(seps),))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (len(seps),))
    out = np.zeros((len(seps), int(bins) + 3), dtype=np.int64)
    for i, s in enumerate(seps):
        with np.errstate(invalid="ignore"):
            d = np.roll(r, -int(s), axis=-1) - r
        out[i] = np.bincount(hist_slots(d, lo[i], hi[i], int(bins)).ravel(), minlength=int(bins) + 3)
    return out


class IncrementHistogram(object):
    """PDFs of the increments along z of `nfields` real fields over `count` points per field: `seps` (grid points of the z row of
    `M` points), `raw` of shape (nfields, nsep, bins + 3), int64 -- per field and separation [below lo, the bins of [lo, hi), at or
    above hi, not finite], summing to `count` -- and `lo`, `hi` of shape (nfields, nsep).  On a velocity field 2 is the
    LONGITUDINAL increment (it runs along z), fields 0 and 1 the transverse ones."""

    def __init__(self, count, seps, raw, lo, hi, M):
        self.count = int(count)
        self.seps = np.asarray(seps, dtype=np.int64).reshape(-1)
        raw = np.asarray(raw, dtype=np.int64)
        self.raw = raw.reshape(-1, self.seps.size, raw.shape[-1]).copy()
        self.lo = np.asarray(lo, dtype=np.float64).reshape(self.raw.shape[:2]).copy()
        self.hi = np.asarray(hi, dtype=np.float64).reshape(self.raw.shape[:2]).copy()
        self.M = int(M)

    @property
    def nbins(self):
        return int(self.raw.shape[2]) - 3

    @property
    def nfields(self):
        return int(self.raw.shape[0])

    def hist(self, i):
        """The `Histogram` of separation i over the fields: pdf, cdf, quantile, below, above and nonfinite come with it."""
        return Histogram(self.count, self.raw[:, i, :], self.lo[:, i], self.hi[:, i])

    def centers(self, f, i):
        return self.hist(i).centers(f)

    def pdf(self, f, i):
        """The density of the increments of field f at separation i over [lo, hi), normalised by ALL `count` points."""
        return self.hist(i).pdf(f)

    def _sigma(self, f, i):
        c, w = self.centers(f, i), self.raw[f, i, 1:-2].astype(np.float64)
        n = w.sum()
        if not n > 0:
            return np.nan
        mean = (w * c).sum() / n
        return float(np.sqrt((w * (c - mean) ** 2).sum() / n))

    def standardized(self, f, i):
        """(d / sigma, sigma * pdf): the PDF in units of its own standard deviation, sigma from the histogram's bins (bin centres,
        the counts inside [lo, hi)).  It integrates to 1 minus the share outside the range, as `pdf` does."""
        sg = self._sigma(f, i)
        return self.centers(f, i) / sg, self.pdf(f, i) * sg

    def moment(self, p, absolute=False):
        """<d^p> (or <|d|^p>, any real p, with `absolute`) from the bin centres, shape (nfields, nsep); the counts outside [lo, hi)
        contribute nothing, the divisor is `count`."""
        out = np.zeros(self.raw.shape[:2], dtype=np.float64)
        for f in range(self.nfields):
            for i in range(self.seps.size):
                c, w = self.centers(f, i), self.raw[f, i, 1:-2].astype(np.float64)
                out[f, i] = (w * (np.abs(c) ** p if absolute else c ** p)).sum() / float(self.count)
        return out

    def r(self, FFT):
        """The separations as lengths: s * L_z / M."""
        return self.seps.astype(np.float64) * float(FFT.L[2]) / self.M


def _incr_hist_ranges(rng, nfields, nsep):
    r = np.asarray(rng, dtype=np.float64)
    r = np.ascontiguousarray(np.broadcast_to(r, (nfields, nsep, 2)))
    return np.ascontiguousarray(r[:, :, 0]), np.ascontiguousarray(r[:, :, 1])


def _incr_hist_check(lo, hi, bins):
    if not 1 <= int(bins) <= INCR_HIST_MAXBINS:
        raise ValueError("bins must be 1 .. %d, not %r" % (INCR_HIST_MAXBINS, bins))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("every range needs finite lo < hi, not %r .. %r" % (lo, hi))


def _range_of_increments(inc, sigmas):
    """+-sigmas * sigma(f, s), sigma = sqrt(S2 / count) of an `Increments`; a field without increments (constant along z) gets
    a range of width 1 about 0, as `_range_of_moments` gives a constant field."""
    with np.errstate(invalid="ignore"):
        sg = np.sqrt(inc.sums[:, :, 0] / float(inc.count))
    if not np.all(np.isfinite(sg)):
        raise ValueError("an increment variance is not finite (%r): give `range`" % (sg,))
    hi = float(sigmas) * sg
    hi[~(hi > 0)] = 0.5
    return -hi, hi.copy()


def _incr_hist_result(FFT, raw, count, seps, lo, hi, M, reduce):
    if reduce:
        raw, count = _add_over_ranks(FFT, raw), int(_add_over_ranks(FFT, [count])[0])
    return IncrementHistogram(count, seps, raw, lo, hi, M)


def real_increment_histogram(FFT, a_hat, b_hat=None, dealias=None, seps=None, bins=128, range=None, sigmas=10.0, reduce=True):
    """PDFs of the increments along z of fields that exist as SPECTRA only (mfft_real_increment_histogram): for every field and
    every separation s in `seps` the counts of ifftn(field, dealias)(z + s) - ifftn(field, dealias)(z) in `bins` equal bins of a
    range of its own -- every order of structure function, |d|^p for any p, the tails and the asymmetry of the longitudinal PDF --
    without a real array: on slab plans with radix kernels on every axis the z kernel keeps the real row in its exchange buffer,
    reads it back shifted and counts into LDS (`FFT.plan_info("nonlinear_incr_hist_fused_3_2")`); elsewhere the plan transforms
    one field at a time into ONE work array and sweeps it.  Fields, `seps`, M and the chunks as `real_increments` (at most
    INCR_MAXSEP separations per call of the library, EACH CHUNK REPEATS THE TRANSFORMS); `bins` 1 .. INCR_HIST_MAXBINS; increments
    along z only.  `range`: (lo, hi) for all, or an array broadcastable to (nfields, nsep, 2); None: one `real_increments` call on
    the same separations gives sigma(f, s) = sqrt(S2 / count) over FFT.comm and the range is +-`sigmas` sigma (a field that is
    constant along z: +-0.5).  Returns an `IncrementHistogram`; with `reduce` the int64 counts are added over FFT.comm.  Counts are
    integers: the same bits run to run and for every number of ranks that computes the same values.  Synchronises the plan's
    stream; the inputs are preserved."""
    fields, ncomp, nfields, head = _real_fields(FFT, a_hat, b_hat)
    M = int(FFT.N[2]) * 3 // 2 if dealias == '3/2-rule' else int(FFT.N[2])
    seps, chunks = _incr_chunks(seps, M)
    if range is None:
        lo, hi = _range_of_increments(real_increments(FFT, a_hat, b_hat, dealias, seps=seps, reduce=True), sigmas)
    else:
        lo, hi = _incr_hist_ranges(range, nfields, len(seps))
    _incr_hist_check(lo, hi, bins)
    count = ctypes.c_int64(0)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    parts, i0 = [], 0
    for ch in chunks:
        sv = np.ascontiguousarray(ch, dtype=np.int64)
        l, h = np.ascontiguousarray(lo[:, i0:i0 + len(ch)]), np.ascontiguousarray(hi[:, i0:i0 + len(ch)])
        out = np.zeros((nfields, len(ch), int(bins) + 3), dtype=np.int64)
        _nonlinear(FFT, "real_increment_histogram", fields, dealias, head=head,
                   tail=(sv.ctypes.data_as(ip), len(ch), l.ctypes.data_as(dp), h.ctypes.data_as(dp), int(bins), out.ctypes.data_as(ip),
                         ctypes.byref(count)))
        parts.append(out)
        i0 += len(ch)
    return _incr_hist_result(FFT, np.concatenate(parts, axis=1), count.value, seps, lo, hi, M, reduce)


def increment_histogram(FFT, u, seps=None, bins=128, range=None, sigmas=10.0, reduce=False):
    """The same counts of a real DeviceArray along its LAST axis (mfft_ew_increment_histogram, the companion of `increments`):
    components, rows, M, pitch, `seps` and the chunks as `increments` (each chunk is one more sweep); `bins`, `range` and `sigmas`
    as `real_increment_histogram`, the sigmas of `range=None` from `increments` (over FFT.comm with `reduce`).  Returns an
    `IncrementHistogram`; with `reduce` over FFT.comm."""
    assert u.dtype == np.dtype(FFT.float), (u.dtype, FFT.float)
    ncomp = int(u.shape[0]) if len(u.shape) == 4 else 1
    M = int(u.shape[-1])
    nrows = u.size // (ncomp * M)
    seps, chunks = _incr_chunks(seps, M)
    if range is None:
        lo, hi = _range_of_increments(increments(FFT, u, seps=seps, reduce=reduce), sigmas)
    else:
        lo, hi = _incr_hist_ranges(range, ncomp, len(seps))
    _incr_hist_check(lo, hi, bins)
    FFT.comm.use_device()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    parts, i0 = [], 0
    for ch in chunks:
        sv = np.ascontiguousarray(ch, dtype=np.int64)
        l, h = np.ascontiguousarray(lo[:, i0:i0 + len(ch)]), np.ascontiguousarray(hi[:, i0:i0 + len(ch)])
        out = np.zeros((ncomp, len(ch), int(bins) + 3), dtype=np.int64)
        _lib.call("mfft_ew_increment_histogram", FFT._plan, u.ptr, ncomp, nrows, M, M if u.pitch is None else int(u.pitch), _prec(FFT),
                  sv.ctypes.data_as(ip), len(ch), l.ctypes.data_as(dp), h.ctypes.data_as(dp), int(bins), out.ctypes.data_as(ip))
        parts.append(out)
        i0 += len(ch)
    return _incr_hist_result(FFT, np.concatenate(parts, axis=1), nrows * M, seps, lo, hi, M, reduce)


PROFILE_STATS = 5       # sums per pair and z index (MFFT_PROFILE_STATS): d_a, d_b, d_a^2, d_b^2, d_a d_b


def profile_rule(x, y, center=None):
    """The rule of the profiles, in numpy float64 (include/mpifft4py_amd.h): x and y of shape (..., M) hold rows along their
    last axis (normalised values, already double); with d_x = x - center[0], d_y = y - center[1] returns the five sums over all
    rows [sum d_x, sum d_y, sum d_x^2, sum d_y^2, sum d_x d_y] per position, shape (5, M).  Products and sums in double."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape, (x.shape, y.shape)
    ca, cb = (0.0, 0.0) if center is None else (float(center[0]), float(center[1]))
    M = x.shape[-1]
    dx, dy = x.reshape(-1, M) - ca, y.reshape(-1, M) - cb
    return np.stack([dx.sum(axis=0), dy.sum(axis=0), (dx * dx).sum(axis=0), (dy * dy).sum(axis=0), (dx * dy).sum(axis=0)])


class Profiles(object):
    """Raw plane sums along z of `npairs` pairs of real fields (x_p, y_p): `count` points per plane, `sums` of shape
    (npairs, 5, M) with sums[p, :, m] = [sum d_x, sum d_y, sum d_x^2, sum d_y^2, sum d_x d_y] over the plane z = m,
    d = value - center[p], and the `center` (npairs, 2) they were taken about.  The derived profiles are formed on the host in
    np.longdouble from the raw sums, about the plane MEAN whatever the centre was."""

    def __init__(self, count, sums, center):
        self.count = int(count)
        self.sums = np.asarray(sums, dtype=np.float64)
        assert self.sums.ndim == 3 and self.sums.shape[1] == PROFILE_STATS, self.sums.shape
        self.center = np.asarray(center, dtype=np.float64).reshape(self.sums.shape[0], 2)
        self.M = int(self.sums.shape[2])

    def _m(self, p):
        return self.sums[p].astype(np.longdouble) / np.longdouble(self.count)

    def mean(self, p=0):
        """<x_p>(z), <y_p>(z): shape (2, M)."""
        return self.center[p].astype(np.longdouble)[:, None] + self._m(p)[:2]

    def variance(self, p=0):
        """<x'^2>(z), <y'^2>(z) about the plane means: shape (2, M)."""
        m = self._m(p)
        return m[2:4] - m[:2] * m[:2]

    def covariance(self, p=0):
        """<x' y'>(z) about the plane means: shape (M,)."""
        m = self._m(p)
        return m[4] - m[0] * m[1]

    def correlation(self, p=0):
        """<x' y'> / sqrt(<x'^2> <y'^2>) per plane; nan where a variance is 0."""
        v = self.variance(p)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((v[0] > 0) & (v[1] > 0), self.covariance(p) / np.sqrt(np.abs(v[0] * v[1])), np.nan)

    def flux(self, p=0):
        """The raw <x y>(z), means included: the vertical heat flux <u_z theta>(z) of (u_z, theta)."""
        m, (ca, cb) = self._m(p), self.center[p].astype(np.longdouble)
        return m[4] + ca * m[1] + cb * m[0] + ca * cb

    def z(self, FFT):
        """The heights of the planes: m * L_z / M."""
        return np.arange(self.M, dtype=np.float64) * float(FFT.L[2]) / self.M

    @property
    def finite(self):
        """Per field (npairs, 2): all its own sums, sum d and sum d^2 at every z, are finite (the cross sum of a pair is finite
        where both of its fields are)."""
        f = np.isfinite(self.sums).all(axis=2)
        return np.stack([f[:, 0] & f[:, 2], f[:, 1] & f[:, 3]], axis=1)


def _profile_centers(center, ncomp):
    """The centres in the order of the C interface, a_0.., then b_0..: `center` is None, (c_a, c_b) for all pairs, or of shape
    (npairs, 2)."""
    c = np.zeros((ncomp, 2), dtype=np.float64) if center is None else np.asarray(center, dtype=np.float64)
    if c.shape == (2,):
        c = np.tile(c, (ncomp, 1))
    assert c.shape == (ncomp, 2), (c.shape, ncomp)
    if not np.isfinite(c).all():
        raise ValueError("the centres must be finite, not %r" % (c,))
    return np.ascontiguousarray(c.T.ravel())


def _profiles_result(FFT, sums, count, c, ncomp, reduce):
    if reduce:      # sums and count: comm.allreduce adds in rank order, the same bits on every rank
        tot = np.asarray(FFT.comm.allreduce(np.concatenate([sums.ravel(), [float(count)]])))
        sums, count = tot[:-1].reshape(sums.shape), int(round(float(tot[-1])))
    return Profiles(count, sums, c.reshape(2, ncomp).T)


def real_profiles(FFT, a_hat, b_hat, dealias=None, center=None, reduce=True):
    """Plane-averaged profiles along z of fields that exist as SPECTRA only (mfft_real_profiles): with x = ifftn(a_hat[p],
    dealias), y = ifftn(b_hat[p], dealias), p over the 1 or 3 components, the five sums over every (x, y) plane of the real grid
    [sum d_x, sum d_y, sum d_x^2, sum d_y^2, sum d_x d_y] for each of the M z indices (M = N[2], or 3 N[2] / 2 under the
    3/2-rule) -- <theta>(z), <theta'^2>(z) and the heat flux <u_z theta>(z) of a stratified run, the mean profile and the
    Reynolds stress of a Kolmogorov flow -- without a real array: on slab plans with radix kernels on every axis
    (`FFT.plan_info("nonlinear_profiles_fused_3_2")`) a thread of the z kernel holds the same z positions for every row it meets,
    so the plane sums are its running sums and need no exchange at all.  Elsewhere the plan transforms a_p and b_p into TWO real
    work arrays and sweeps them.  z is whole on every rank.  b_hat may be a_hat.  `center`: None, (c_a, c_b) for all pairs or of
    shape (npairs, 2); the sums are taken about it, and a centre near the mean keeps the digits of the variances.  Returns a
    `Profiles`; with `reduce` the raw sums and the count are added over FFT.comm.  A NaN or Inf in a field gives sums of that
    field that are not finite (`Profiles.finite`); the values are bitwise reproducible run to run, and are NOT claimed identical
    for different numbers of ranks (they are sums of doubles).  Synchronises the plan's stream; the inputs are preserved."""
    if b_hat is None:
        raise ValueError("a profile takes pairs of fields: b_hat must be given (it may be a_hat)")
    assert b_hat.shape == a_hat.shape, (a_hat.shape, b_hat.shape)
    fields, ncomp, _, head = _real_fields(FFT, a_hat, b_hat)
    c = _profile_centers(center, ncomp)
    M = int(FFT.N[2]) * 3 // 2 if dealias == '3/2-rule' else int(FFT.N[2])
    out = np.zeros((ncomp, PROFILE_STATS, M), dtype=np.float64)
    count = ctypes.c_int64(0)
    dp = ctypes.POINTER(ctypes.c_double)
    _nonlinear(FFT, "real_profiles", fields, dealias, head=head, tail=(c.ctypes.data_as(dp), out.ctypes.data_as(dp), ctypes.byref(count)))
    return _profiles_result(FFT, out, count.value, c, ncomp, reduce)


def profiles(FFT, x, y, center=None, reduce=False):
    """The same sums of two real DeviceArrays of the same shape along their LAST axis (mfft_ew_profiles, the companion of
    `joint_histogram`): arrays of four axes are taken as (components, ..) with 1 or 3 components, pair p = (x[p], y[p]), any
    other as one pair; M = x.shape[-1].  `center` as in `real_profiles`.  Returns a `Profiles`; with `reduce` over FFT.comm."""
    if x.pitch is not None or y.pitch is not None:
        raise ValueError("a profile of a pitched array would read the elements between its rows")
    assert x.dtype == np.dtype(FFT.float) and y.dtype == x.dtype and x.shape == y.shape, (x.dtype, y.dtype, x.shape, y.shape)
    ncomp = int(x.shape[0]) if len(x.shape) == 4 else 1
    assert ncomp in (1, 3), ncomp
    M = int(x.shape[-1])
    nrows = x.size // (ncomp * M)
    c = _profile_centers(center, ncomp)
    FFT.comm.use_device()
    out = np.zeros((ncomp, PROFILE_STATS, M), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.call("mfft_ew_profiles", FFT._plan, x.ptr, y.ptr, ncomp, nrows, M, _prec(FFT), c.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return _profiles_result(FFT, out, nrows, c, ncomp, reduce)


def strain_hat(FFT, K, U_hat, diag, off):
    """The strain-rate tensor S_ij = (du_i/dx_j + du_j/dx_i) / 2 of a vector field in spectral space (mfft_ew_strain_hat), U_hat
    read once: diag[f] = i K[f] U_hat[f] (S_00, S_11, S_22) and off = (S_01, S_02, S_12), S_ij = i (K[i] U_hat[j] + K[j] U_hat[i]) / 2.
    All three are distinct arrays of shape (3,) + FFT.complex_shape(); pitched spectra are swept as they lie in memory.  The
    dissipation 2 nu S_ij S_ij is `real_quadratic(FFT, diag, off, weights=2 * nu * np.array([1, 1, 1, 2, 2, 2]))`.
    Returns (diag, off)."""
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert U_hat.shape == diag.shape == off.shape == (3,) + cs, (U_hat.shape, diag.shape, off.shape, cs)
    assert U_hat.dtype == diag.dtype == off.dtype == np.dtype(FFT.complex), (U_hat.dtype, diag.dtype, off.dtype)
    assert U_hat.pitch == diag.pitch == off.pitch, (U_hat.pitch, diag.pitch, off.pitch)
    _lib.call("mfft_ew_strain_hat", FFT._plan, U_hat.ptr, diag.ptr, off.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr, K.cshape, _prec(FFT))
    return diag, off


def advective_dt(FFT, umax, cfl):
    """cfl / sum_f umax[f] N[f] / L[f]: the advective (CFL) time step of a velocity whose components reach umax[f], on
    the mesh FFT.N of the box FFT.L -- the mesh of the run, not the padded one of a 3/2-rule product.  Pure host
    arithmetic; inf for a field at rest, nan if a maximum is."""
    umax = np.asarray(umax, dtype=np.float64).reshape(-1)
    N, L = np.asarray(FFT.N, dtype=np.float64), np.asarray(FFT.L, dtype=np.float64)
    assert umax.size == N.size == L.size, (umax.size, N.size, L.size)
    rate = float(np.sum(umax * N / L))
    if rate != rate:
        return float("nan")
    return float("inf") if rate == 0.0 else float(cfl) / rate


def ns_rk_stage(FFT, K, N_hat, U_hat, U_hat0, U_hat1, nu, a_dt, b_dt, last):
    """One Runge-Kutta stage in one sweep (mfft_ew_ns_rk_stage): N_hat holds the nonlinear term on entry and the curl of
    the updated U_hat on return; U_hat1 += a_dt dU; U_hat = U_hat0 + b_dt dU, or (last) U_hat = U_hat0 = U_hat1."""
    _lib.call("mfft_ew_ns_rk_stage", FFT._plan, N_hat.ptr, U_hat.ptr, U_hat0.ptr, U_hat1.ptr, K.dev[0].ptr, K.dev[1].ptr,
              K.dev[2].ptr, K.cshape, float(nu), float(a_dt), float(b_dt), 1 if last else 0, _prec(FFT))
    return U_hat


def axpbz(FFT, y, x, z, alpha, beta):
    """y = alpha * x + beta * z (element-wise over the raw real storage; aliasing allowed)."""
    assert x.nbytes == y.nbytes == z.nbytes and x.pitch == y.pitch == z.pitch
    n_real = y.nbytes // np.dtype(FFT.float).itemsize          # the rows as they lie in memory (pitched arrays: all of it)
    _lib.call("mfft_ew_axpbz", FFT._plan, y.ptr, x.ptr, z.ptr, float(alpha), float(beta), n_real, _prec(FFT))
    return y


def sumsq(FFT, x):
    if x.pitch is not None:
        raise ValueError("sumsq of a pitched array would count the elements between its rows")
    n_real = x.size * (2 if x.dtype.kind == "c" else 1)
    r = ctypes.c_double(0.0)
    _lib.call("mfft_ew_sumsq", FFT._plan, x.ptr, n_real, _prec(FFT), ctypes.byref(r))
    return r.value


def dft_bins(FFT, u, bins, start, is_input=True, inverse=False):
    """Partial sums of DFT bins over this rank's block of a field (mfft_ew_dft_bins): `u` a DeviceArray holding the
    block whose first element sits at the global index `start`; bins an (nb, 3) integer array.  Returns a complex
    vector of length nb; the global bin is the sum over the ranks.  Evaluated by definition in double precision --
    an independent check of a transform too large for any host FFT."""
    bins = np.ascontiguousarray(np.asarray(bins, dtype=np.int64).reshape(-1, 3))
    N = FFT.global_shape() if hasattr(FFT, "global_shape") else FFT.global_real_shape()
    out = np.zeros(len(bins), dtype=np.complex128)
    shape = (ctypes.c_int64 * 3)(*[int(x) for x in u.shape])
    st = (ctypes.c_int64 * 3)(*[int(x) for x in start])
    n3 = (ctypes.c_int64 * 3)(*[int(x) for x in N])
    for i in range(0, len(bins), 16):
        chunk = bins[i:i + 16]
        res = (ctypes.c_double * (2 * len(chunk)))()
        _lib.call("mfft_ew_dft_bins", FFT._plan, u.ptr, 1 if u.dtype.kind == "c" else 0, shape, st, n3,
                  1 if inverse else 0, len(chunk), chunk.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _prec(FFT), res)
        out[i:i + len(chunk)] = np.array(res[:]).view(np.complex128)
    return out


def shell_sums(FFT, K, a_hat, b_hat=None, k2=False, reduce=True):
    """Shell-binned sums of spectra on the device (mfft_ew_shell_sums):
        S[s] = sum over the modes k with shell(k) = s of  h(k) w(k) sum_c Re(conj(a_hat_c[k]) b_hat_c[k])
    shell(k) the integer nearest to |k| of the integer wave numbers (`_mesh.Block.shell_of`), h the Hermitian weight of
    the half axis (so the sum runs over the FULL spectrum of a real field), w = |K|^2 of the scaled wave numbers with
    k2, else 1.  a_hat, b_hat (default a_hat, read once): DeviceArrays of FFT.complex_shape() or (3,) + that.  Returns
    a float64 vector of K.nshell entries -- the corner modes included, so its sum is the Parseval sum --, added over
    FFT.comm with `reduce`.  Products and sums in double whatever the precision; synchronises the plan's stream."""
    if getattr(getattr(FFT, "_mesh", None), "nd", 0) != 3 or K is None or K.idev is None:
        raise NotImplementedError("shell spectra need a 3-D plan (slab or pencil), not %s" % type(FFT).__name__)
    if b_hat is None:
        b_hat = a_hat
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert a_hat.shape in (cs, (3,) + cs), (a_hat.shape, cs)
    for x in (a_hat, b_hat):
        assert x.shape == a_hat.shape and x.dtype == np.dtype(FFT.complex), (x.shape, x.dtype, a_hat.shape)
        FFT._check_pitch(x, FFT.complex_pitch)
    FFT.comm.use_device()
    out = np.zeros(K.nshell, dtype=np.float64)
    _lib.call("mfft_ew_shell_sums", FFT._plan, a_hat.ptr, b_hat.ptr, 3 if len(a_hat.shape) == 4 else 1,
              K.idev[0].ptr, K.idev[1].ptr, K.idev[2].ptr, K.hdev.ptr, K.dev[0].ptr, K.dev[1].ptr, K.dev[2].ptr,
              1 if k2 else 0, K.cshape, K.nshell, _prec(FFT), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return FFT.comm.allreduce(out) if reduce else out


def _points(FFT):
    return float(FFT.N[0]) * float(FFT.N[1]) * float(FFT.N[2])


def energy_spectrum(FFT, K, U_hat):
    """E[s] = shell_sums(U_hat, U_hat) / (2 (N0 N1 N2)^2): the forward transform is unnormalised (numpy's convention), so
    E.sum() is the mean kinetic energy sum(U * U) / (2 N0 N1 N2) the examples print (half the variance for a scalar)."""
    return shell_sums(FFT, K, U_hat) / (2.0 * _points(FFT) ** 2)


def transfer_spectrum(FFT, K, U_hat, N_hat):
    """T[s] = shell_sums(U_hat, N_hat) / (N0 N1 N2)^2 = Re <U_hat*, N_hat> per shell."""
    return shell_sums(FFT, K, U_hat, N_hat) / _points(FFT) ** 2


def cyl_sums(FFT, K, a_hat, b_hat=None, k2=False, reduce=True, seg_rows=0):
    """(k_perp, k_z) sums of spectra on the device (mfft_ew_cyl_sums; the rule of include/mpifft4py_amd.h):
        R[p, q] = sum over the modes k with shell(kx^2 + ky^2) = p and |kz| = q of  h(k) w(k) sum_c Re(conj(a_hat_c[k]) b_hat_c[k])
    shell the integer rule of `shell_sums` applied to the two perpendicular integer wave numbers, h the Hermitian weight of the
    half axis, w = |K|^2 of the scaled wave numbers with k2, else 1.  a_hat, b_hat (default a_hat, read once): DeviceArrays of
    FFT.complex_shape() or (3,) + that.  Returns a float64 array of shape (K.nperp, K.npar), added over FFT.comm with `reduce`:
    R.sum(axis=1) is the k_perp spectrum, R.sum(axis=0) the k_z spectrum (R[:, 0] the 2-D modes), R.sum() the Parseval sum,
    shell_sums(...).sum().  Products and sums in double whatever the precision; bitwise reproducible run to run; synchronises
    the plan's stream.  seg_rows: rows per partial sum, 0 for the library's default (tests)."""
    if getattr(getattr(FFT, "_mesh", None), "nd", 0) != 3 or K is None or K.idev is None:
        raise NotImplementedError("(k_perp, k_z) spectra need a 3-D plan (slab or pencil), not %s" % type(FFT).__name__)
    if b_hat is None:
        b_hat = a_hat
    cs = tuple(int(x) for x in FFT.complex_shape())
    assert a_hat.shape in (cs, (3,) + cs), (a_hat.shape, cs)
    for x in (a_hat, b_hat):
        assert x.shape == a_hat.shape and x.dtype == np.dtype(FFT.complex), (x.shape, x.dtype, a_hat.shape)
        FFT._check_pitch(x, FFT.complex_pitch)
    FFT.comm.use_device()
    out = np.zeros((K.nperp, K.npar), dtype=np.float64)
    _lib.call("mfft_ew_cyl_sums", FFT._plan, a_hat.ptr, b_hat.ptr, 3 if len(a_hat.shape) == 4 else 1, K.perp_rows.ptr,
              K.perp_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), K.nperp, K.idev[2].ptr, K.hdev.ptr, K.dev[0].ptr,
              K.dev[1].ptr, K.dev[2].ptr, 1 if k2 else 0, K.cshape, K.npar, int(seg_rows), _prec(FFT),
              out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return FFT.comm.allreduce(out) if reduce else out


def energy_spectrum_2d(FFT, K, U_hat):
    """E[p, q] = cyl_sums(U_hat, U_hat) / (2 (N0 N1 N2)^2), the normalisation of `energy_spectrum`: E.sum() is the mean kinetic
    energy, E.sum(axis=1) the k_perp spectrum, E.sum(axis=0) the k_z spectrum, E[:, 0].sum() the energy of the modes k_z = 0."""
    return cyl_sums(FFT, K, U_hat) / (2.0 * _points(FFT) ** 2)


def transfer_spectrum_2d(FFT, K, U_hat, N_hat):
    """T[p, q] = cyl_sums(U_hat, N_hat) / (N0 N1 N2)^2, the normalisation of `transfer_spectrum`: T.sum(axis=1) is the transfer
    across k_perp, T.sum(axis=0) the transfer across k_z."""
    return cyl_sums(FFT, K, U_hat, N_hat) / _points(FFT) ** 2
