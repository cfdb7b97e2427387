"""Passive scalar in a prescribed velocity field, pseudo-spectral RK4 -- DEVICE-RESIDENT:

    d theta / dt = - u . grad(theta) + kappa laplace(theta)

The velocity is given by its spectrum and does not change; theta, its spectrum and the RK4 work arrays live in HBM.  Per
Runge-Kutta stage: the gradient in spectral space (spectral.grad_hat), the advection term as ONE plan operation
(spectral.dot_transform: six inverse transforms, the dot product, one forward transform -- on slab plans with the z stages
in one kernel and no real-space array), and the updates with spectral.axpbz.

The diffusion term has no kernel of its own: -|K|^2 theta is taken from three more grad_hat sweeps over the gradient and
three axpbz sums (12 field writes per stage).  On small meshes these sweeps, not the transforms, dominate the ms per step
this example prints; the plan stages of `--stages` (nl_*) are the advection term alone.

    python examples/passive_scalar_device.py --N 32               # Taylor-Green velocity, ten steps
    python examples/passive_scalar_device.py --N 256 --stages     # ms per step by plan stage
    python examples/passive_scalar_device.py --N 256 --composed   # the caller-side composition instead
    python examples/passive_scalar_device.py --N 64 --spectrum    # the variance spectrum of the real field theta after the last step
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpifft4py_amd import DeviceArray, spectral  # noqa: E402
from mpifft4py_amd.slab import R2C as Slab_R2C  # noqa: E402

INFO = {"3/2-rule": "nonlinear_dot_fused_3_2", "2/3-rule": "nonlinear_dot_fused_2_3", None: "nonlinear_dot_fused_none"}


def make_plan(comm, N, precision="double", complex_pitch=None):
    N = np.array([N] * 3 if np.isscalar(N) else N, dtype=int)
    return Slab_R2C(N, np.array([2 * np.pi] * 3, dtype=float), comm, precision, complex_pitch=complex_pitch)


def _to_device(FFT, x, components=None):
    """A numpy spectrum (compact rows, this rank's block) or a DeviceArray as a DeviceArray of the plan's pitch."""
    if isinstance(x, DeviceArray):
        return x
    d = FFT.empty_complex(components)
    return d.set(np.ascontiguousarray(x, dtype=FFT.complex))


def solve(comm, N, U_hat, theta0_hat, kappa, dt, steps, dealias, fused=True, precision="double", complex_pitch=None,
          report=None, timing=False, FFT=None, cfl=None, dt_max=None):
    """Advance theta_hat by `steps` RK4 steps and return it (a DeviceArray of FFT.complex_shape()).  U_hat: (3,) + the local
    complex shape, theta0_hat: the local complex shape (numpy arrays or DeviceArrays; neither is modified).
    fused=True: the advection term is spectral.dot_transform.  fused=False: the composition a caller would write -- six
    FFT.ifftn, spectral.dot on the real fields, one FFT.fftn -- kept for A/B timing and as the parity partner.
    cfl=C (fused only): the first Runge-Kutta stage of a step runs dot_transform with absmax=True and the step's
    dt = min(dt_max, C / sum_f max|u_f| N_f / L_f) is fetched right after it (one synchronisation of the plan's stream per
    step); `dt` is then not used.  report["dt"] lists the steps' dt; rank 0 prints them."""
    if cfl is not None and not fused:
        raise ValueError("cfl needs the plan operation: the composition has no statistics call")
    if FFT is None:
        FFT = make_plan(comm, N, precision, complex_pitch)
    K = spectral.Wavenumbers(FFT)
    U = _to_device(FFT, U_hat, 3)
    th, th_in = FFT.empty_complex(), _to_device(FFT, theta0_hat)
    spectral.axpbz(FFT, th, th_in, th_in, 1.0, 0.0)      # a copy (both operands initialised: 0 * garbage may be NaN)
    th0, th1, lap, adv = (FFT.empty_complex() for _ in range(4))
    G, W = FFT.empty_complex(3), FFT.empty_complex(3)
    if not fused:
        ws = tuple(FFT.work_shape(dealias))
        Ur, Gr = DeviceArray.empty((3,) + ws, FFT.float), DeviceArray.empty((3,) + ws, FFT.float)
        Sr = DeviceArray.empty(ws, FFT.float)
    a = [1. / 6., 1. / 3., 1. / 3., 1. / 6.]
    b = [0.5, 0.5, 1.]

    def rhs(stats=False):
        """adv <- d theta / dt of the current th"""
        spectral.grad_hat(FFT, K, th, G)
        # laplace(theta) is the divergence of the gradient the stage holds anyway: -|K|^2 theta = sum_f (i K_f)(i K_f theta),
        # the f-th component of grad_hat(G_f).  Three more sweeps with the kernels there are; no kernel of its own.
        for f in range(3):
            spectral.grad_hat(FFT, K, G.component(f), W)
            if f == 0:
                spectral.axpbz(FFT, lap, W.component(0), W.component(0), 1.0, 0.0)
            else:
                spectral.axpbz(FFT, lap, lap, W.component(f), 1.0, 1.0)
        if fused:
            spectral.dot_transform(FFT, U, G, adv, dealias, absmax=stats)
        else:
            for f in range(3):
                FFT.ifftn(U.component(f), Ur.component(f), dealias)
                FFT.ifftn(G.component(f), Gr.component(f), dealias)
            spectral.dot(FFT, Ur, Gr, Sr)
            FFT.fftn(Sr, adv, None if dealias == "2/3-rule" else dealias)      # (the 2/3-rule filters what goes INTO a product)
        spectral.axpbz(FFT, adv, adv, lap, -1.0, float(kappa))

    rhs()                                  # warm-up outside the timed loop: the plan allocates its buffers at the first call
    FFT.sync()
    if timing:
        FFT.enable_timing(True)
        FFT.reset_timing()
    t0 = time.perf_counter()
    for step_ in range(steps):
        spectral.axpbz(FFT, th0, th, th, 1.0, 0.0)
        spectral.axpbz(FFT, th1, th, th, 1.0, 0.0)
        for rk in range(4):
            rhs(stats=(cfl is not None and rk == 0))
            if cfl is not None and rk == 0:        # max |u_f| (and max |d theta / dx_f|) of the step's first stage: one synchronisation
                am = spectral.nonlinear_absmax(FFT)
                dt = spectral.advective_dt(FFT, am[0], cfl)
                if dt_max is not None:
                    dt = min(dt, dt_max)
                if report is not None:
                    report.setdefault("dt", []).append(dt)
                if comm.Get_rank() == 0:
                    print("step %d: dt = %.15e  max|grad theta| = %.6e" % (step_, dt, float(am[1].max())))
            if rk < 3:
                spectral.axpbz(FFT, th, th0, adv, 1.0, b[rk] * dt)
            spectral.axpbz(FFT, th1, th1, adv, 1.0, a[rk] * dt)
        spectral.axpbz(FFT, th, th1, th1, 1.0, 0.0)
    FFT.sync()
    wall = time.perf_counter() - t0
    if report is not None:
        report["ms_per_step"] = 1e3 * wall / max(steps, 1)
        report["fused_dot"] = FFT.plan_info(INFO[dealias]) if fused else 0
        report["work_bytes"] = FFT.plan_info("nonlinear_bytes") + FFT.workspace_bytes() + (0 if fused else Ur.nbytes + Gr.nbytes + Sr.nbytes)
        if timing:
            report["stages"] = {k: (v[0] / max(steps, 1), v[1] // max(steps, 1)) for k, v in FFT.stage_times().items()}
    return th


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=32, help="mesh edge")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.0, help="time step; default: inside the explicit scheme's stability bounds for this mesh")
    ap.add_argument("--kappa", type=float, default=0.01)
    ap.add_argument("--dealias", default="3/2-rule", choices=["3/2-rule", "2/3-rule", "None"])
    ap.add_argument("--precision", default="double")
    ap.add_argument("--composed", action="store_true", help="six ifftn + dot + one fftn issued here instead of the plan operation")
    ap.add_argument("--stages", action="store_true", help="print ms per step by plan stage (HIP events)")
    ap.add_argument("--spectrum", action="store_true", help="print the variance spectrum of theta after the last step (shells of integer |k|, binned on the device)")
    ap.add_argument("--cfl", type=float, default=None, help="advective time step dt = CFL / sum_f max|u_f| N_f / L_f from the fused advection "
                    "term's real-space maxima (one stream synchronisation per step) instead of --dt; prints dt per step")
    ap.add_argument("--dt-max", type=float, default=None, help="with --cfl: dt = min(DT_MAX, advective dt)")
    args = ap.parse_args()
    dealias = None if args.dealias == "None" else args.dealias
    # RK4 is explicit: kappa |k|^2 dt and |u| |k| dt must stay inside its stability region (|u| <= 1 for Taylor-Green)
    dt = args.dt or 1.0 / (args.kappa * 3 * (args.N / 2) ** 2 + 1.5 * args.N)
    from mpifft4py_amd import SelfComm
    comm = SelfComm()
    FFT = make_plan(comm, args.N, args.precision)
    U, th0 = taylor_green_hat(FFT), random_scalar_hat(FFT)
    rep = {}
    th = solve(comm, args.N, U, th0, args.kappa, dt, args.steps, dealias, fused=not args.composed, precision=args.precision,
               report=rep, timing=args.stages, FFT=FFT, cfl=args.cfl, dt_max=args.dt_max)
    print("N = %d^3, %d RK4 steps of dt = %.3g, %.3f ms per step (%s; plan work buffers %.2f GB)"
          % (args.N, args.steps, dt, rep["ms_per_step"],
             "composed here: 28 transforms + element-wise kernels" if args.composed else
             ("fused dot z stage" if rep["fused_dot"] else "one plan operation per advection term, composed inside"),
             rep["work_bytes"] / 1e9))
    for name, (ms, calls) in sorted(rep.get("stages", {}).items()):
        print("  %-10s %8.3f ms per step  (%d launches)" % (name, ms, calls))
    a, b = th0.get(), th.get()
    print("mean of theta: %.15e -> %.15e" % (a[0, 0, 0].real, b[0, 0, 0].real))
    if args.spectrum:
        # E[s] = sum over shell s of |theta_hat|^2 / (2 N^6): its sum is half the mean square of theta, taken here from the
        # real field by the streaming reduction the library had before (spectral.sumsq).  It is the spectrum of the REAL
        # field: the random theta has Nyquist modes, on which i k theta_hat is not the spectrum of a real field (and the
        # planes kz = 0, N/2 of the stepped half spectrum are not kept conjugate-symmetric); the complex-to-real transform
        # drops that part, so the stepped array itself sums to a little more than the field holds.
        Kw = spectral.Wavenumbers(FFT)
        stepped = spectral.energy_spectrum(FFT, Kw, th).sum()
        theta = DeviceArray.empty(tuple(FFT.real_shape()), FFT.float)
        FFT.ifftn(th, theta)
        k = FFT.comm.allreduce(spectral.sumsq(FFT, theta)) / float(args.N) ** 3 / 2
        th_real = FFT.empty_complex()                    # the stepped state th stays as it is
        FFT.fftn(theta, th_real)
        E = spectral.energy_spectrum(FFT, Kw, th_real)
        print("variance spectrum of the REAL field theta = ifftn(theta_hat) after the last step, shells of integer |k| (sum %.15e, "
              "half the mean square %.15e).  The stepped array theta_hat itself sums to %.15e: the excess is its part in the "
              "Nyquist planes that is the spectrum of no real field, which the complex-to-real transform drops:" % (E.sum(), k, stepped))
        for s_, e in enumerate(E):
            if e > 0:
                print("  %4d  %.6e" % (s_, e))
        if args.precision == "double":
            assert abs(E.sum() - k) <= 1e-12 * k, (E.sum(), k)
            print("sum of the spectrum equals half the mean square to 1e-12")


if __name__ == "__main__":
    main()
