"""Incompressible magnetohydrodynamics in Elsasser variables z+- = u +- b, pseudo-spectral RK4 -- DEVICE-RESIDENT:

    d z+ / dt = - (z- . grad) z+ - grad(P) + (nu + eta) / 2 laplace(z+) + (nu - eta) / 2 laplace(z-),      div z+- = 0
    d z- / dt = - (z+ . grad) z- - grad(P) + (nu + eta) / 2 laplace(z-) + (nu - eta) / 2 laplace(z+)

Both fields, their spectra and the RK4 work arrays live in HBM.  Per Runge-Kutta stage: all nine products z+_i z-_j as ONE plan
operation (spectral.outer_transform: six inverse transforms, the nine products, nine forward transforms -- on slab plans with
the z stages in one kernel and no real-space array), both right-hand sides in one sweep (spectral.elsasser_rhs: the two
divergences, the projections, the dissipation) and the RK updates (spectral.axpbz).  Three cross_transform calls (u x omega,
j x b, u x b) would take eighteen inverse and nine forward transforms per stage.

A uniform field B0 e_z is the k = 0 bin of the spectra: z+ carries + B0, z- carries - B0.

    python examples/mhd_device.py --N 32                     # Orszag-Tang-like vortex, ten steps
    python examples/mhd_device.py --N 256 --B0 1.0           # ... in a mean field
    python examples/mhd_device.py --N 256 --composed         # the 6 + 9 transforms and the products issued here: the A/B partner
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpifft4py_amd import DeviceArray, spectral  # noqa: E402
from mpifft4py_amd.slab import R2C as Slab_R2C  # noqa: E402

INFO = {"3/2-rule": "nonlinear_outer_fused_3_2", "2/3-rule": "nonlinear_outer_fused_2_3", None: "nonlinear_outer_fused_none"}


def make_plan(comm, N, precision="double", complex_pitch=None):
    N = np.array([N] * 3 if np.isscalar(N) else N, dtype=int)
    return Slab_R2C(N, np.array([2 * np.pi] * 3, dtype=float), comm, precision, complex_pitch=complex_pitch)


def _copy(FFT, dst, src):
    return spectral.axpbz(FFT, dst, src, src, 1.0, 0.0)      # (both operands initialised: 0 * garbage may be NaN)


def energies(FFT, K, Zp_hat, Zm_hat):
    """(total energy, cross helicity) = (<|z+|^2 + |z-|^2> / 4, <|z+|^2 - |z-|^2> / 4) = (<u.u + b.b> / 2, <u.b>)."""
    ep, em = spectral.energy_spectrum(FFT, K, Zp_hat).sum(), spectral.energy_spectrum(FFT, K, Zm_hat).sum()      # <z.z> / 2 each
    return 0.5 * (ep + em), 0.5 * (ep - em)


def solve(comm, N, Zp0_hat, Zm0_hat, nu, eta, dt, steps, dealias, fused=True, precision="double", report=None, FFT=None, trace=None):
    """Advance (Zp_hat, Zm_hat) by `steps` RK4 steps and return them (DeviceArrays of (3,) + FFT.complex_shape()); Zp0_hat and
    Zm0_hat (DeviceArrays of the plan) are not modified.  fused=True: the nine products are ONE spectral.outer_transform per
    stage.  fused=False (--composed): six FFT.ifftn, nine spectral.mul and nine FFT.fftn issued here, the same arithmetic on
    seven real arrays of this loop -- the parity and A/B partner.  trace: a list that receives (energy, cross helicity) per step."""
    if FFT is None:
        FFT = make_plan(comm, N, precision)
    K = spectral.Wavenumbers(FFT)
    Zp, Zm, Zp0, Zm0, Zp1, Zm1, dZp, dZm = (FFT.empty_complex(3) for _ in range(8))
    T = FFT.empty_complex(9)
    if not fused:
        ws = tuple(FFT.work_shape(dealias))
        Rp, Rm = DeviceArray.empty((3,) + ws, FFT.float), DeviceArray.empty((3,) + ws, FFT.float)
        W = DeviceArray.empty(ws, FFT.float)
    _copy(FFT, Zp, Zp0_hat)
    _copy(FFT, Zm, Zm0_hat)
    a = [1. / 6., 1. / 3., 1. / 3., 1. / 6.]
    b = [0.5, 0.5, 1.]

    def nonlinear():
        """T[3 i + j] <- fftn(ifftn(Zp[i]) ifftn(Zm[j]))"""
        if fused:
            spectral.outer_transform(FFT, Zp, Zm, T, dealias)
            return
        for f in range(3):
            FFT.ifftn(Zp.component(f), Rp.component(f), dealias)
            FFT.ifftn(Zm.component(f), Rm.component(f), dealias)
        for i in range(3):
            for j in range(3):
                spectral.mul(FFT, Rp.component(i), Rm.component(j), W)
                FFT.fftn(W, T.component(3 * i + j), None if dealias == "2/3-rule" else dealias)      # (the 2/3-rule filters what goes INTO a product)

    def stage(rk):
        nonlinear()
        spectral.elsasser_rhs(FFT, K, T, Zp, Zm, dZp, dZm, nu, eta)
        for Z, Z0, Z1, dZ in ((Zp, Zp0, Zp1, dZp), (Zm, Zm0, Zm1, dZm)):
            if rk < 3:
                spectral.axpbz(FFT, Z, Z0, dZ, 1.0, b[rk] * dt)
            spectral.axpbz(FFT, Z1, Z1, dZ, 1.0, a[rk] * dt)

    nonlinear()      # warm-up outside the timed loop: the plan allocates its buffers at the first call; the state is untouched
    FFT.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        for Z, Z0, Z1 in ((Zp, Zp0, Zp1), (Zm, Zm0, Zm1)):
            _copy(FFT, Z0, Z)
            _copy(FFT, Z1, Z)
        for rk in range(4):
            stage(rk)
        _copy(FFT, Zp, Zp1)
        _copy(FFT, Zm, Zm1)
        if trace is not None:
            trace.append(energies(FFT, K, Zp, Zm))
    FFT.sync()
    wall = time.perf_counter() - t0
    if report is not None:
        report["ms_per_step"] = 1e3 * wall / max(steps, 1)
        report["fused"] = FFT.plan_info(INFO[dealias]) if fused else 0
        report["work_bytes"] = FFT.plan_info("nonlinear_bytes") + FFT.workspace_bytes() + (0 if fused else Rp.nbytes + Rm.nbytes + W.nbytes)
    return Zp, Zm


def orszag_tang_hat(FFT, B0=0.0):
    """(Zp_hat, Zm_hat) of a three-dimensional Orszag-Tang-like vortex, u = (-sin y, sin x, 0) + 0.2 (sin z, 0, 0) and
    b = (-sin y, sin 2x, 0) + B0 e_z -- both solenoidal -- on this rank's block."""
    N = FFT.N
    sl = FFT.real_local_slice()
    x, y, z = (np.arange(s_.start, s_.stop, dtype=float) * (2 * np.pi / int(N[i])) for i, s_ in enumerate(sl))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    u = (-np.sin(Y) + 0.2 * np.sin(Z), np.sin(X), np.zeros_like(X))
    bb = (-np.sin(Y), np.sin(2 * X), np.full_like(X, float(B0)))
    Zp, Zm = FFT.empty_complex(3), FFT.empty_complex(3)
    for f in range(3):
        FFT.fftn(DeviceArray.from_numpy((u[f] + bb[f]).astype(FFT.float)), Zp.component(f))
        FFT.fftn(DeviceArray.from_numpy((u[f] - bb[f]).astype(FFT.float)), Zm.component(f))
    return Zp, Zm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=32, help="mesh edge")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.0, help="time step; default: inside the explicit scheme's stability bounds for this mesh")
    ap.add_argument("--nu", type=float, default=0.005)
    ap.add_argument("--eta", type=float, default=0.005)
    ap.add_argument("--B0", type=float, default=0.0, help="uniform field along z")
    ap.add_argument("--dealias", default="3/2-rule", choices=["3/2-rule", "2/3-rule", "None"])
    ap.add_argument("--precision", default="double")
    ap.add_argument("--composed", action="store_true", help="six ifftn, nine products and nine fftn per stage instead of one outer_transform")
    ap.add_argument("--spectrum2d", action="store_true", help="print the final total energy as E(k_perp) and E(k_z) -- the mean field is along z --, "
                    "the share of the modes k_z = 0 and the sum, from spectral.energy_spectrum_2d on the spectra (no host copy of them)")
    args = ap.parse_args()
    dealias = None if args.dealias == "None" else args.dealias
    # RK4 is explicit: nu |k|^2 dt and |z| |k| dt must stay inside its stability region (|z| <= 3.2 + B0 here)
    dt = args.dt or 1.0 / (max(args.nu, args.eta) * 3 * (args.N / 2) ** 2 + (3.2 + abs(args.B0)) * 1.5 * args.N)
    from mpifft4py_amd import SelfComm
    comm = SelfComm()
    FFT = make_plan(comm, args.N, args.precision)
    Zp0, Zm0 = orszag_tang_hat(FFT, args.B0)
    rep, trace = {}, []
    Kw = spectral.Wavenumbers(FFT)
    e0 = energies(FFT, Kw, Zp0, Zm0)
    Zp, Zm = solve(comm, args.N, Zp0, Zm0, args.nu, args.eta, dt, args.steps, dealias, fused=not args.composed, precision=args.precision,
          report=rep, FFT=FFT, trace=trace)
    print("N = %d^3, %d RK4 steps of dt = %.3g, %.3f ms per step (%s; plan work buffers %.2f GB)"
          % (args.N, args.steps, dt, rep["ms_per_step"],
             "composed here: 6 ifftn, 9 products, 9 fftn per stage" if args.composed else
             ("one operation per stage, fused outer-product z stage" if rep["fused"] else "one operation per stage, composed inside the plan"),
             rep["work_bytes"] / 1e9))
    print("step %4d  total energy %.15e  cross helicity %.15e" % ((0,) + e0))
    for i, (e, h) in enumerate(trace):
        print("step %4d  total energy %.15e  cross helicity %.15e" % (i + 1, e, h))
    if args.spectrum2d:      # total energy = (<|z+|^2> + <|z-|^2>) / 4, as in energies()
        E = 0.5 * (spectral.energy_spectrum_2d(FFT, Kw, Zp) + spectral.energy_spectrum_2d(FFT, Kw, Zm))
        fmt = lambda v: ", ".join("%.6e" % c for c in v)
        print("total energy E(k_perp) = [%s]" % fmt(E.sum(axis=1)))
        print("total energy E(k_z) = [%s]" % fmt(E.sum(axis=0)))
        print("total energy share of k_z = 0: %.12f" % (E[:, 0].sum() / E.sum()))
        total = energies(FFT, Kw, Zp, Zm)[0]
        ok = abs(E.sum() - total) <= 1e-12 * abs(total)
        print("total energy sum of E(k_perp, k_z) = %.15e: %s the sum of E(k) to 1e-12" % (E.sum(), "equals" if ok else "DIFFERS FROM"))


if __name__ == "__main__":
    main()
