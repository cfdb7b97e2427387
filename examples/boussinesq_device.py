"""A velocity that carries a scalar (Boussinesq convection, stratified turbulence, a tracer in a DNS), pseudo-spectral RK4 --
DEVICE-RESIDENT:

    d u / dt     = u x omega - grad(p) + nu laplace(u) + g theta e_z,      div u = 0
    d theta / dt = - u . grad(theta) + kappa laplace(theta)

Velocity, scalar, their spectra and the RK4 work arrays live in HBM.  Per Runge-Kutta stage: the scalar's gradient in spectral
space (spectral.grad_hat), BOTH nonlinear terms as ONE plan operation (spectral.cross_dot_transform: nine inverse transforms,
the cross and the dot product, four forward transforms -- on slab plans with the z stages in one kernel and no real-space array;
ifftn(U_hat) is computed once, where cross_transform + dot_transform compute it twice), the buoyancy added to the vertical
component (spectral.axpbz), the velocity's stage in one sweep (spectral.ns_rk_stage) and the scalar's updates as in
examples/passive_scalar_device.py (whose note on the diffusion term's sweeps applies here as well).

    python examples/boussinesq_device.py --N 32                  # Taylor-Green velocity, a random scalar, ten steps
    python examples/boussinesq_device.py --N 256 --stages        # ms per step by plan stage
    python examples/boussinesq_device.py --N 256 --two-calls     # cross_transform + dot_transform instead: the A/B partner
    python examples/boussinesq_device.py --N 64 --g 1.0          # with buoyancy
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpifft4py_amd import DeviceArray, spectral  # noqa: E402
from mpifft4py_amd.slab import R2C as Slab_R2C  # noqa: E402

INFO = {"3/2-rule": "nonlinear_cross_dot_fused_3_2", "2/3-rule": "nonlinear_cross_dot_fused_2_3", None: "nonlinear_cross_dot_fused_none"}


def make_plan(comm, N, precision="double", complex_pitch=None):
    N = np.array([N] * 3 if np.isscalar(N) else N, dtype=int)
    return Slab_R2C(N, np.array([2 * np.pi] * 3, dtype=float), comm, precision, complex_pitch=complex_pitch)


def _copy(FFT, dst, src):
    return spectral.axpbz(FFT, dst, src, src, 1.0, 0.0)      # (both operands initialised: 0 * garbage may be NaN)


def solve(comm, N, U0_hat, theta0_hat, nu, kappa, dt, steps, dealias, one_op=True, g=0.0, precision="double", report=None,
          timing=False, FFT=None, joint=False, profiles=False):
    """Advance (U_hat, theta_hat) by `steps` RK4 steps and return them (DeviceArrays of (3,) + FFT.complex_shape() and
    FFT.complex_shape()); U0_hat and theta0_hat (DeviceArrays of the plan) are not modified.
    one_op=True: both nonlinear terms are ONE spectral.cross_dot_transform per stage.  one_op=False (--two-calls):
    spectral.dot_transform and spectral.cross_transform, the same arithmetic with ifftn(U_hat) done twice -- the parity and A/B
    partner.  g: buoyancy, N_hat[2] += g theta_hat before the velocity's stage (0: the scalar is passive).
    joint=True: after every step report["joint"] gains the `spectral.JointHistogram` of (u_z, theta) in 64 x 64 bins over the
    fields' extremes, from ONE spectral.real_joint_histogram call on the two spectra (fused, the z kernel ends in the grid: no
    real-space array); the timing then includes it.
    profiles=True: after every step report["profiles"] gains the pair (`spectral.Profiles` of (u_z, theta) from ONE
    spectral.real_profiles call on the two spectra -- <theta>(z), <theta'^2>(z) and the heat flux <u_z theta>(z), no real-space
    array --, the box value of <u_z theta> from the spectra by Parseval); the timing then includes both."""
    if FFT is None:
        FFT = make_plan(comm, N, precision)
    K = spectral.Wavenumbers(FFT)
    U_hat, U_hat0, U_hat1, dU, G, W = (FFT.empty_complex(3) for _ in range(6))
    th, th0, th1, lap, adv = (FFT.empty_complex() for _ in range(5))
    _copy(FFT, U_hat, U0_hat)
    _copy(FFT, th, theta0_hat)
    a = [1. / 6., 1. / 3., 1. / 3., 1. / 6.]
    b = [0.5, 0.5, 1.]

    def nonlinear():
        """dU (the curl of U_hat on entry) <- fftn(U x curl U), adv <- fftn(U . grad theta), lap <- -|K|^2 theta"""
        spectral.grad_hat(FFT, K, th, G)
        for f in range(3):                       # laplace(theta) = div(grad theta), with the sweeps there are
            spectral.grad_hat(FFT, K, G.component(f), W)
            if f == 0:
                _copy(FFT, lap, W.component(0))
            else:
                spectral.axpbz(FFT, lap, lap, W.component(f), 1.0, 1.0)
        if one_op:
            spectral.cross_dot_transform(FFT, U_hat, dU, G, dU, adv, dealias)
        else:
            spectral.dot_transform(FFT, U_hat, G, adv, dealias)
            spectral.cross_transform(FFT, U_hat, dU, dU, dealias)

    def stage(rk):
        nonlinear()
        if g != 0.0:
            spectral.axpbz(FFT, dU.component(2), dU.component(2), th, 1.0, float(g))
        # the velocity: projection, viscous term, both updates and the curl of the NEW U_hat (into dU) in one sweep
        spectral.ns_rk_stage(FFT, K, dU, U_hat, U_hat0, U_hat1, nu, a[rk] * dt, b[rk] * dt if rk < 3 else 0.0, rk == 3)
        # the scalar, advected by the velocity the stage started from
        spectral.axpbz(FFT, adv, adv, lap, -1.0, float(kappa))
        if rk < 3:
            spectral.axpbz(FFT, th, th0, adv, 1.0, b[rk] * dt)
        spectral.axpbz(FFT, th1, th1, adv, 1.0, a[rk] * dt)

    # warm-up outside the timed loop: the plan allocates its buffers at the first call; the state is restored
    spectral.curl_hat(FFT, K, U_hat, dU)
    nonlinear()
    _copy(FFT, U_hat0, U_hat)
    _copy(FFT, U_hat1, U_hat)
    spectral.curl_hat(FFT, K, U_hat, dU)
    FFT.sync()
    if timing:
        FFT.enable_timing(True)
        FFT.reset_timing()
    t0 = time.perf_counter()
    Kw = spectral.Wavenumbers(FFT) if profiles else None
    for _ in range(steps):
        _copy(FFT, th0, th)
        _copy(FFT, th1, th)
        for rk in range(4):
            stage(rk)
        _copy(FFT, th, th1)
        if joint and report is not None:                 # (collective: a moments call for the ranges, then the joint histogram)
            report.setdefault("joint", []).append(spectral.real_joint_histogram(FFT, U_hat.component(2), th, dealias, bins=64))
        if profiles and report is not None:              # (collective: the plane sums are added over the ranks)
            report.setdefault("profiles", []).append((spectral.real_profiles(FFT, U_hat.component(2), th, dealias),
                                                      float(spectral.transfer_spectrum(FFT, Kw, U_hat.component(2), th).sum())))
    FFT.sync()
    wall = time.perf_counter() - t0
    if report is not None:
        report["ms_per_step"] = 1e3 * wall / max(steps, 1)
        report["fused"] = FFT.plan_info(INFO[dealias]) if one_op else 0
        report["work_bytes"] = FFT.plan_info("nonlinear_bytes") + FFT.workspace_bytes()
        if timing:
            report["stages"] = {k: (v[0] / max(steps, 1), v[1] // max(steps, 1)) for k, v in FFT.stage_times().items()}
    return U_hat, th


def taylor_green_hat(FFT):
    """The spectrum of the Taylor-Green velocity (sin x cos y cos z, -cos x sin y cos z, 0) on this rank's block."""
    N = FFT.N
    sl = FFT.real_local_slice()
    x, y, z = (np.arange(s_.start, s_.stop, dtype=float) * (2 * np.pi / int(N[i])) for i, s_ in enumerate(sl))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    U = FFT.empty_complex(3)
    fields = (np.sin(X) * np.cos(Y) * np.cos(Z), -np.cos(X) * np.sin(Y) * np.cos(Z), np.zeros_like(X))
    for f in range(3):
        FFT.fftn(DeviceArray.from_numpy(fields[f].astype(FFT.float)), U.component(f))
    return U


def random_scalar_hat(FFT, seed=0):
    rng = np.random.default_rng(seed + FFT.rank)
    th = FFT.empty_complex()
    FFT.fftn(DeviceArray.from_numpy((rng.random(tuple(FFT.real_shape())) - 0.5).astype(FFT.float)), th)
    return th


def joint_summary(h):
    """(correlation coefficient of (a, b) from the bin centres, <a | b> at five b bins, the counted total) of pair 0 of a
    JointHistogram: what the heat flux <u_z theta> looks like as a PDF.  The coefficient is 0 where a field has no variance."""
    w = h.counts[0].astype(np.float64)
    ca, cb = h.centers(0, 0), h.centers(0, 1)
    tot = w.sum()
    ma, mb = (w.sum(1) * ca).sum() / tot, (w.sum(0) * cb).sum() / tot
    va, vb = (w.sum(1) * (ca - ma) ** 2).sum() / tot, (w.sum(0) * (cb - mb) ** 2).sum() / tot
    cov = (w * np.outer(ca - ma, cb - mb)).sum() / tot
    corr = cov / np.sqrt(va * vb) if va > 0 and vb > 0 else 0.0
    five = np.linspace(0, h.nbins[1] - 1, 7)[1:-1].astype(int)
    return float(corr), h.conditional_mean(0, of=0)[five], int(h.raw[0].sum())


def profiles_summary(h):
    """(<theta>, <theta'^2>, <u_z theta> at five heights, the mean over the planes of <u_z theta>) of pair 0 = (u_z, theta) of a
    Profiles."""
    five = np.linspace(0, h.M - 1, 7)[1:-1].astype(int)
    flux = np.asarray(h.flux(0), dtype=np.float64)
    return (np.asarray(h.mean(0)[1], dtype=np.float64)[five], np.asarray(h.variance(0)[1], dtype=np.float64)[five], flux[five], float(flux.mean()))


def print_spectrum2d(what, E, total):
    """The two reduced spectra of E[k_perp, k_z], the share of the modes k_z = 0 (the 2-D, "vortical" ones) and the sum next to the
    shell spectrum's."""
    fmt = lambda v: ", ".join("%.6e" % c for c in v)
    print("%s E(k_perp) = [%s]" % (what, fmt(E.sum(axis=1))))
    print("%s E(k_z) = [%s]" % (what, fmt(E.sum(axis=0))))
    print("%s share of k_z = 0: %.12f" % (what, E[:, 0].sum() / E.sum()))
    ok = abs(E.sum() - total) <= 1e-12 * abs(total)
    print("%s sum of E(k_perp, k_z) = %.15e: %s the sum of E(k) to 1e-12" % (what, E.sum(), "equals" if ok else "DIFFERS FROM"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=32, help="mesh edge")
    ap.add_argument("--M", type=int, default=0, help="mesh edge 2^M (overrides --N)")
    ap.add_argument("--joint", action="store_true", help="print per step the correlation coefficient of (u_z, theta), <u_z | theta> at five "
                    "theta bins and the counted total, from ONE spectral.real_joint_histogram call on the spectra (no real-space array)")
    ap.add_argument("--profiles", action="store_true", help="print per step <theta>, <theta'^2> and the heat flux <u_z theta> at five heights z, "
                    "and the plane-mean of <u_z theta> next to the box value, from ONE spectral.real_profiles call on the spectra (no real-space array)")
    ap.add_argument("--spectrum2d", action="store_true", help="print the final kinetic energy as E(k_perp) and E(k_z) -- gravity is along z --, the "
                    "share of the modes k_z = 0 and the sum, from ONE spectral.energy_spectrum_2d call on the spectrum (no host copy of it)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.0, help="time step; default: inside the explicit scheme's stability bounds for this mesh")
    ap.add_argument("--nu", type=float, default=0.000625)
    ap.add_argument("--kappa", type=float, default=0.01)
    ap.add_argument("--g", type=float, default=0.0, help="buoyancy: g theta is added to the vertical momentum equation (0: a passive scalar)")
    ap.add_argument("--dealias", default="3/2-rule", choices=["3/2-rule", "2/3-rule", "None"])
    ap.add_argument("--precision", default="double")
    ap.add_argument("--two-calls", action="store_true", help="cross_transform + dot_transform per stage instead of one cross_dot_transform")
    ap.add_argument("--stages", action="store_true", help="print ms per step by plan stage (HIP events)")
    args = ap.parse_args()
    if args.M:
        args.N = 2 ** args.M
    dealias = None if args.dealias == "None" else args.dealias
    # RK4 is explicit: kappa |k|^2 dt and |u| |k| dt must stay inside its stability region (|u| <= 1 for Taylor-Green)
    dt = args.dt or 1.0 / (max(args.kappa, args.nu) * 3 * (args.N / 2) ** 2 + 1.5 * args.N)
    from mpifft4py_amd import SelfComm
    comm = SelfComm()
    FFT = make_plan(comm, args.N, args.precision)
    U0, th0 = taylor_green_hat(FFT), random_scalar_hat(FFT)
    rep = {}
    U, th = solve(comm, args.N, U0, th0, args.nu, args.kappa, dt, args.steps, dealias, one_op=not args.two_calls, g=args.g,
                  precision=args.precision, report=rep, timing=args.stages, FFT=FFT, joint=args.joint, profiles=args.profiles)
    print("N = %d^3, %d RK4 steps of dt = %.3g, %.3f ms per step (%s; plan work buffers %.2f GB)"
          % (args.N, args.steps, dt, rep["ms_per_step"],
             "two calls per stage: cross_transform + dot_transform" if args.two_calls else
             ("one operation per stage, fused cross-and-dot z stage" if rep["fused"] else "one operation per stage, composed inside the plan"),
             rep["work_bytes"] / 1e9))
    for name, (ms, calls) in sorted(rep.get("stages", {}).items()):
        print("  %-10s %8.3f ms per step  (%d launches)" % (name, ms, calls))
    for step, h in enumerate(rep.get("joint", [])):
        corr, cond, total = joint_summary(h)
        print("joint step %d: corr(u_z, theta) = %+.9e  <u_z | theta> = [%s]  total = %d" % (step + 1, corr, ", ".join("%+.6e" % c for c in cond), total))
    for step, (h, box) in enumerate(rep.get("profiles", [])):
        mean, var, flux, pm = profiles_summary(h)
        fmt = lambda v: ", ".join("%+.6e" % c for c in v)
        print("profiles step %d: <theta> = [%s]  <theta'^2> = [%s]  <u_z theta> = [%s]  plane-mean <u_z theta> = %+.12e  box <u_z theta> = %+.12e"
              % (step + 1, fmt(mean), fmt(var), fmt(flux), pm, box))
    Kw = spectral.Wavenumbers(FFT)
    print("kinetic energy: %.15e -> %.15e" % (spectral.energy_spectrum(FFT, Kw, U0).sum(), spectral.energy_spectrum(FFT, Kw, U).sum()))
    print("mean of theta: %.15e -> %.15e" % (th0.get()[0, 0, 0].real, th.get()[0, 0, 0].real))
    if args.spectrum2d:
        print_spectrum2d("kinetic energy", spectral.energy_spectrum_2d(FFT, Kw, U), spectral.energy_spectrum(FFT, Kw, U).sum())


if __name__ == "__main__":
    main()
