"""Taylor-Green vortex, pseudo-spectral RK4 -- DEVICE-RESIDENT version: velocity,
spectra and all RK4 work arrays live in HBM, the transforms are mpifft4py_amd
plans and everything between them is a fused element-wise HIP kernel
(mpifft4py_amd.spectral).  Same equations, parameters and known answer as the
reference's demo/spectral_dns_solver.py (k = 0.124953117517 at 32^3, 10 steps).

    python examples/spectral_dns_device.py --M 5            # the reference demo's case
    python examples/spectral_dns_device.py --M 8 --steps 5  # 256^3, prints ms per RK4 step
    python examples/spectral_dns_device.py --M 6 --spectrum # the energy spectrum E(k) after the last step
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpifft4py_amd import DeviceArray, spectral  # noqa: E402
from mpifft4py_amd.pencil import R2C as Pencil_R2C  # noqa: E402
from mpifft4py_amd.slab import R2C as Slab_R2C  # noqa: E402


def _zero(a):
    from mpifft4py_amd import _lib
    _lib.call("mfft_memset", a.ptr, 0, a.nbytes)
    return a


def solve(comm, M=5, dealias='3/2-rule', decomposition='slab', precision="double", nu=0.000625, dt=0.01, steps=10,
          report=None, fused=True, timing=False, complex_pitch="default", edge=None, spectrum=False, cfl=None, dt_max=None,
          stats=False, pdf=False, dissipation=False, structure=False, structure_pdf=False):
    """fused=True (round 6): the nonlinear term is ONE plan operation (spectral.cross_transform: no real-space work
    arrays, the z stages one kernel) and a Runge-Kutta stage's projection, viscous term, both updates and the next
    curl are ONE sweep (spectral.ns_rk_stage).  fused=False: the composition of rounds 3 - 5 (nine transforms, cross,
    curl, rhs and axpbz kernels per stage), kept for A/B timing and as the parity partner of the fused path.
    spectrum=True: report["spectrum"] is the energy spectrum E(k) of the final state, binned on the device
    (spectral.energy_spectrum; the sum over the ranks), whose sum is the k returned.
    cfl=C (fused loop): an advective time step.  The first Runge-Kutta stage of a step runs with absmax=True, so the
    fused z kernel also leaves max |u_f| and max |omega_f| on the device; dt = min(dt_max, C / sum_f max|u_f| N_f / L_f)
    is fetched right after it -- ONE synchronisation of the plan's stream per step -- and the step's four stages use
    it.  report["dt"] lists the steps' dt, report["wmax"] their max |omega|; rank 0 prints both.
    stats=True (fused loop): report["stats"] holds the one-point statistics of the final state -- spectral.Moments of the three
    longitudinal derivatives du_f/dx_f ("grad"), and of u and omega together ("u_omega": six fields) -- from
    spectral.real_moments: the fields exist as spectra only, no real array is written for them.
    pdf=True (fused loop): report["pdf"] = (Histogram, mean, sigma) of du_0/dx_0 of the final state over +-8 of its standard deviations
    in 32 bins, from spectral.real_histogram on the same spectrum (the z kernel ends in a histogram).
    dissipation=True (fused loop): before every step and of the final state, the statistics of the dissipation eps = 2 nu S_ij S_ij
    and of the enstrophy density omega^2 -- quadratic forms of six and of three fields that exist as spectra only
    (spectral.strain_hat, spectral.real_quadratic): report["dissipation"] lists (<eps>, <omega^2>, <eps^2> / <eps>^2,
    <omega^4> / <omega^2>^2) and rank 0 prints them with nu <omega^2> / <eps>, which is 1 for a periodic solenoidal field; with pdf
    also the two histograms of the final state, report["dissipation_pdf"].
    structure=True (fused loop): before every step and of the final state, the structure functions of the velocity along z at the
    default separations (the powers of two below M / 2, then M / 2) -- a two-point statistic of fields that exist as spectra only
    (spectral.real_increments: the z kernel reads the real row back shifted, no real-space array): report["structure"] lists the
    spectral.Increments and rank 0 prints S_2 of u_0 (transverse) and of u_2 (longitudinal: the increment runs along z) and the
    skewness and flatness of the longitudinal increment.
    structure_pdf=True (fused loop): of the final state, the PDFs of the velocity increments along z at the same separations, 128 bins
    over +-10 standard deviations of each (spectral.real_increment_histogram: the z kernel counts the shifted differences into LDS, no
    real-space array): report["structure_pdf"] = (IncrementHistogram, Increments) and rank 0 prints, per separation, the flatness of
    the longitudinal increment obtained from the PDF next to the one from the power sums of spectral.real_increments."""
    if complex_pitch == "default":       # the fused loop on ONE rank keeps its spectra pitched (rows a whole number of cache lines
        # apart: every pass runs on them); several ranks and the composition of rounds 3 - 5 keep compact rows
        complex_pitch = "auto" if (fused and comm.Get_size() == 1) else None
    N = np.array([edge or 2 ** M] * 3, dtype=int)        # edge: a mesh that is not a power of two (576, 1152 ...)
    L = np.array([2 * np.pi] * 3, dtype=float)
    if cfl is not None and not fused:
        raise ValueError("cfl needs the fused loop: the composition has no statistics call")
    if stats and not fused:
        raise ValueError("stats needs the fused loop: the composition holds no curl of the final state")
    if pdf and not fused:
        raise ValueError("pdf needs the fused loop")
    if dissipation and not fused:
        raise ValueError("dissipation needs the fused loop")
    if (structure or structure_pdf) and not fused:
        raise ValueError("structure needs the fused loop")
    if decomposition == 'slab':
        FFT = Slab_R2C(N, L, comm, precision, complex_pitch=complex_pitch)
    else:
        FFT = Pencil_R2C(N, L, comm, precision, communication="Alltoallw", alignment="X", complex_pitch=complex_pitch)
    rs, cs, ws = FFT.real_shape(), FFT.complex_shape(), FFT.work_shape(dealias)
    fl, cx = FFT.float, FFT.complex
    K = spectral.Wavenumbers(FFT)

    # Taylor-Green initial condition (demo:81-84), built on the host in chunks of x planes (a 1024^3 field is 26 GB: the
    # chunks keep the host side at a few hundred MB) from the 1-D coordinates of this rank's block; everything else on the device
    sl = FFT.real_local_slice()
    x, y, z = (np.arange(s_.start, s_.stop, dtype=float) * (L[i] / N[i]) for i, s_ in enumerate(sl))
    U = DeviceArray.empty((3,) + rs, fl)
    cyz = np.cos(y)[:, None] * np.cos(z)[None, :]
    syz = np.sin(y)[:, None] * np.cos(z)[None, :]
    step = max(1, (64 << 20) // (8 * rs[1] * rs[2]))
    for i0 in range(0, rs[0], step):
        i1 = min(rs[0], i0 + step)
        U.component(0).leading(i0, i1).set((np.sin(x[i0:i1])[:, None, None] * cyz[None]).astype(fl))
        U.component(1).leading(i0, i1).set((-np.cos(x[i0:i1])[:, None, None] * syz[None]).astype(fl))
    _zero(U.component(2))
    U_hat, U_hat0, U_hat1, dU = (FFT.empty_complex(3) for _ in range(4))      # (3,) + cs, rows `complex_pitch` apart if asked for
    a = [1. / 6., 1. / 3., 1. / 3., 1. / 6.]
    b = [0.5, 0.5, 1.]
    if timing:
        FFT.enable_timing(True)

    if fused:
        for i in range(3):
            FFT.fftn(U.component(i), U_hat.component(i))
        spectral.axpbz(FFT, U_hat0, U_hat, U_hat, 1.0, 0.0)
        spectral.axpbz(FFT, U_hat1, U_hat, U_hat, 1.0, 0.0)
        spectral.curl_hat(FFT, K, U_hat, dU)               # dU doubles as the curl's spectrum between the stages
        # warm-up outside the timed loop: the plan allocates its buffers (25 GB at 512^3) at the first call; the state is restored
        spectral.cross_transform(FFT, U_hat, dU, dU, dealias)
        spectral.curl_hat(FFT, K, U_hat, dU)
        FFT.sync()
        if timing:
            FFT.reset_timing()
        t0 = time.perf_counter()
        def dissipation_report(label, bins=0):       # (collective: every rank calls it; three sweeps and two plan operations)
            if not dis_work:
                dis_work.extend(FFT.empty_complex(3) for _ in range(3))
            diag, off, W = dis_work
            spectral.strain_hat(FFT, K, U_hat, diag, off)
            spectral.curl_hat(FFT, K, U_hat, W)
            me, he = spectral.real_quadratic(FFT, diag, off, dealias, weights=2 * nu * np.array([1, 1, 1, 2, 2, 2.0]), bins=bins)
            mw, hw = spectral.real_quadratic(FFT, W, None, dealias, bins=bins)
            eps, w2 = float(me.sums[0, 0]) / me.count, float(mw.sums[0, 0]) / mw.count
            fe, fw = float(me.sums[0, 1]) / me.count / eps ** 2, float(mw.sums[0, 1]) / mw.count / w2 ** 2
            if report is not None:
                report.setdefault("dissipation", []).append((eps, w2, fe, fw))
                if bins:
                    report["dissipation_pdf"] = (he, hw)
            if comm.Get_rank() == 0:
                print("%s: <eps> = %.15e  <omega^2> = %.15e  nu <omega^2> / <eps> = %.15f  flatness of eps = %.9f  of omega^2 = %.9f"
                      % (label, eps, w2, nu * w2 / eps, fe, fw))

        def structure_report(label):                 # (collective: every rank calls it; one plan operation)
            inc = spectral.real_increments(FFT, U_hat, None, dealias)
            if report is not None:
                report.setdefault("structure", []).append(inc)
            if comm.Get_rank() == 0:
                fmt = lambda v: "[" + " ".join("%.12e" % float(x) for x in v) + "]"
                S2 = inc.S(2)
                print("structure %s: s = [%s]  S2(u_0) = %s  S2(u_2) = %s  skewness(du_2) = %s  flatness(du_2) = %s"
                      % (label, " ".join(str(int(x)) for x in inc.seps), fmt(S2[0]), fmt(S2[2]), fmt(inc.skewness()[2]), fmt(inc.flatness()[2])))

        dis_work = []
        for step_ in range(steps):
            if dissipation:
                dissipation_report("step %d" % step_)
            if structure:
                structure_report("step %d" % step_)
            for rk in range(4):
                spectral.cross_transform(FFT, U_hat, dU, dU, dealias, absmax=(cfl is not None and rk == 0))      # dU = fftn(U x curl U)
                if cfl is not None and rk == 0:      # max |u_f|, max |omega_f| of the state the step starts from (one stream synchronisation)
                    am = spectral.nonlinear_absmax(FFT)
                    dt = spectral.advective_dt(FFT, am[0], cfl)
                    if dt_max is not None:
                        dt = min(dt, dt_max)
                    if report is not None:
                        report.setdefault("dt", []).append(dt)
                        report.setdefault("wmax", []).append(float(am[1].max()))
                    if comm.Get_rank() == 0:
                        print("step %d: dt = %.15e  max|omega| = %.6e" % (step_, dt, float(am[1].max())))
                spectral.ns_rk_stage(FFT, K, dU, U_hat, U_hat0, U_hat1, nu, a[rk] * dt, b[rk] * dt if rk < 3 else 0.0, rk == 3)
        FFT.sync()
        wall = time.perf_counter() - t0
        if report is not None:
            report["ms_per_step"] = 1e3 * wall / max(steps, 1)
            report["fused_nonlinear"] = FFT.plan_info({"3/2-rule": "nonlinear_fused_3_2", "2/3-rule": "nonlinear_fused_2_3"}.get(
                dealias, "nonlinear_fused_none"))
            report["work_bytes"] = FFT.plan_info("nonlinear_bytes") + FFT.workspace_bytes()
            if timing:
                report["stages"] = {k: (v[0] / steps, v[1] // steps) for k, v in FFT.stage_times().items()}
        if spectrum:
            E = spectral.energy_spectrum(FFT, K, U_hat)         # (collective: every rank calls it)
            if report is not None:
                report["spectrum"] = E
        if stats:                                               # (collective too; dU holds the curl of the final state)
            uw = spectral.real_moments(FFT, U_hat, dU, dealias)
            grad = spectral.real_moments(FFT, spectral.diag_grad_hat(FFT, K, U_hat, FFT.empty_complex(3)), None, dealias)
            if report is not None:
                report["stats"] = {"u_omega": uw, "grad": grad}
        if pdf:                                                 # (collective: a moments call for sigma, then the histogram)
            G = spectral.diag_grad_hat(FFT, K, U_hat, FFT.empty_complex(3))
            g0 = G.component(0)
            m = spectral.real_moments(FFT, g0, None, dealias)
            mean, sigma = float(m.mean()[0]), float(np.sqrt(m.variance()[0]))
            h = spectral.real_histogram(FFT, g0, None, dealias, bins=32, range=(mean - 8 * sigma, mean + 8 * sigma))
            if report is not None:
                report["pdf"] = (h, mean, sigma)
        if dissipation:
            dissipation_report("final", bins=32 if pdf else 0)
        if structure:
            structure_report("final")
        if structure_pdf:                                       # (collective: the sums for sigma, then the histograms)
            inc = spectral.real_increments(FFT, U_hat, None, dealias)
            ih = spectral.real_increment_histogram(FFT, U_hat, None, dealias, seps=list(inc.seps), bins=128, sigmas=10.0)
            if report is not None:
                report["structure_pdf"] = (ih, inc)
            if comm.Get_rank() == 0:
                with np.errstate(divide="ignore", invalid="ignore"):
                    fp = ih.moment(4)[2] / ih.moment(2)[2] ** 2
                fs = inc.flatness()[2]
                for i, sep in enumerate(inc.seps):
                    print("structure-pdf s = %d  flatness from the PDF %.9f  from the sums %.9f  (outside the range: %.3e)"
                          % (int(sep), float(fp[i]), float(fs[i]), float(ih.raw[2, i, [0, -2, -1]].sum()) / ih.count))
        for i in range(3):
            FFT.ifftn(U_hat.component(i), U.component(i))
        return FFT.comm.reduce(spectral.sumsq(FFT, U) / float(N[0]) / float(N[1]) / float(N[2]) / 2)

    W_hat = FFT.empty_complex(3)
    Ud = DeviceArray.empty((3,) + ws, fl)
    Cd = DeviceArray.empty((3,) + ws, fl)
    Rd = DeviceArray.empty((3,) + ws, fl)

    def compute_rhs():
        for i in range(3):
            FFT.ifftn(U_hat.component(i), Ud.component(i), dealias)
        spectral.curl_hat(FFT, K, U_hat, W_hat)
        for i in range(3):
            FFT.ifftn(W_hat.component(i), Cd.component(i), dealias)
        spectral.cross(FFT, Ud, Cd, Rd)
        for i in range(3):
            FFT.fftn(Rd.component(i), dU.component(i), dealias)
        spectral.ns_rhs(FFT, K, dU, U_hat, nu)

    for i in range(3):
        FFT.fftn(U.component(i), U_hat.component(i))
    compute_rhs()                      # warm-up outside the timed loop (work buffers of the padded transforms); writes dU only
    FFT.sync()
    if timing:
        FFT.reset_timing()
    t0 = time.perf_counter()
    for _ in range(steps):
        spectral.axpbz(FFT, U_hat0, U_hat, U_hat, 1.0, 0.0)
        spectral.axpbz(FFT, U_hat1, U_hat, U_hat, 1.0, 0.0)
        for rk in range(4):
            compute_rhs()
            if rk < 3:
                spectral.axpbz(FFT, U_hat, U_hat0, dU, 1.0, b[rk] * dt)
            spectral.axpbz(FFT, U_hat1, U_hat1, dU, 1.0, a[rk] * dt)
        spectral.axpbz(FFT, U_hat, U_hat1, U_hat1, 1.0, 0.0)
    FFT.sync()
    wall = time.perf_counter() - t0
    if spectrum:
        E = spectral.energy_spectrum(FFT, K, U_hat)
        if report is not None:
            report["spectrum"] = E
    for i in range(3):
        FFT.ifftn(U_hat.component(i), U.component(i))
    k = FFT.comm.reduce(spectral.sumsq(FFT, U) / float(N[0]) / float(N[1]) / float(N[2]) / 2)
    if report is not None:
        report["ms_per_step"] = 1e3 * wall / steps
        report["fused_nonlinear"] = 0
        report["work_bytes"] = FFT.workspace_bytes() + 3 * Ud.nbytes
        if timing:
            report["stages"] = {k: (v[0] / steps, v[1] // steps) for k, v in FFT.stage_times().items()}
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=5)
    ap.add_argument("--N", type=int, default=0, help="mesh edge instead of 2**M (576, 1152 ...: any length with radix plans)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--dealias", default="3/2-rule", choices=["3/2-rule", "2/3-rule", "None"])
    ap.add_argument("--precision", default="double")
    ap.add_argument("--composed", action="store_true", help="the nine-transform composition of rounds 3 - 5 instead of the fused operations")
    ap.add_argument("--stages", action="store_true", help="print the per-stage HIP-event times")
    ap.add_argument("--spectrum", action="store_true", help="print the energy spectrum E(k) of the final state (shells of integer |k|, binned on the device)")
    ap.add_argument("--compact", action="store_true", help="compact spectra (rows of Nf bins) instead of the fused loop's default, rows a whole number of cache lines apart")
    ap.add_argument("--cfl", type=float, default=None, help="advective time step dt = CFL / sum_f max|u_f| N_f / L_f from the fused nonlinear term's "
                    "real-space maxima (one stream synchronisation per step) instead of the fixed dt = 0.01; prints dt and max|omega| per step")
    ap.add_argument("--dt-max", type=float, default=None, help="with --cfl: dt = min(DT_MAX, advective dt)")
    ap.add_argument("--stats", action="store_true", help="print skewness and flatness of du_f/dx_f and of u_f and min / max of omega_f of the final "
                    "state, from the spectra (spectral.real_moments: no real-space array)")
    ap.add_argument("--pdf", action="store_true", help="print the PDF of du_0/dx_0 of the final state in units of its standard deviation, from "
                    "the spectrum (spectral.real_histogram: no real-space array)")
    ap.add_argument("--dissipation", action="store_true", help="print before every step and of the final state <eps>, <omega^2>, nu <omega^2> / <eps> "
                    "(1 for a periodic solenoidal field) and the flatness <eps^2> / <eps>^2, <omega^4> / <omega^2>^2, from the spectra "
                    "(spectral.real_quadratic: no real-space array); with --pdf also the two histograms of the final state")
    ap.add_argument("--structure", action="store_true", help="print before every step and of the final state the structure functions along z "
                    "at the separations 1, 2, 4, .. M / 2: S_2 of u_0 and u_2 and the skewness and flatness of the longitudinal increment "
                    "of u_2, from the spectra (spectral.real_increments: no real-space array)")
    ap.add_argument("--structure-pdf", action="store_true", help="print of the final state, per separation, the flatness of the longitudinal "
                    "increment of u_2 from its PDF (128 bins over +-10 sigma) next to the one from the power sums, both from the spectra "
                    "(spectral.real_increment_histogram, spectral.real_increments: no real-space array)")
    args = ap.parse_args()
    dealias = None if args.dealias == "None" else args.dealias
    from mpifft4py_amd import LocalGroup, SelfComm
    rep = {}
    if args.ranks > 1:
        ks = LocalGroup(args.ranks).run(lambda c: solve(c, args.M, dealias, steps=args.steps, precision=args.precision,
                                                        report=rep if c.Get_rank() == 0 else None, fused=not args.composed,
                                                        timing=args.stages, complex_pitch=None if args.compact else "default",
                                                        edge=args.N or None, spectrum=args.spectrum, cfl=args.cfl, dt_max=args.dt_max, stats=args.stats, pdf=args.pdf, dissipation=args.dissipation, structure=args.structure, structure_pdf=args.structure_pdf))
    else:
        ks = [solve(SelfComm(), args.M, dealias, steps=args.steps, precision=args.precision, report=rep,
                    fused=not args.composed, timing=args.stages, complex_pitch=None if args.compact else "default",
                    edge=args.N or None, spectrum=args.spectrum, cfl=args.cfl, dt_max=args.dt_max, stats=args.stats, pdf=args.pdf, dissipation=args.dissipation, structure=args.structure, structure_pdf=args.structure_pdf)]
    print("N = %d^3, %d RK4 steps, %.3f ms per step (%s, device-resident; plan work buffers %.2f GB)"
          % (args.N or 2 ** args.M, args.steps, rep.get("ms_per_step", float("nan")),
             "composed: 36 transforms + element-wise kernels" if args.composed else
             ("fused nonlinear z stage" if rep.get("fused_nonlinear") else "one plan operation per nonlinear term, composed inside"),
             rep.get("work_bytes", 0) / 1e9))
    for name, (ms, calls) in sorted(rep.get("stages", {}).items()):
        print("  %-10s %8.3f ms per step  (%d launches)" % (name, ms, calls))
    print("k =", repr(ks[0]))
    if args.spectrum:
        E = rep["spectrum"]
        print("E(k), shells of integer |k| (sum %.15e):" % E.sum())
        for s_, e in enumerate(E):
            if e > 0:
                print("  %4d  %.6e" % (s_, e))
        if args.precision == "double":
            assert abs(E.sum() - ks[0]) <= 1e-12 * ks[0], (E.sum(), ks[0])
            print("sum of E(k) equals k to 1e-12")
    if args.stats:
        fmt = lambda v: "[" + " ".join("%.9f" % float(x) for x in v) + "]"
        uw, grad = rep["stats"]["u_omega"], rep["stats"]["grad"]
        print("du_f/dx_f: skewness = %s  flatness = %s" % (fmt(grad.skewness()), fmt(grad.flatness())))
        print("u: skewness = %s  flatness = %s" % (fmt(uw.skewness()[:3]), fmt(uw.flatness()[:3])))
        print("omega: min = %s  max = %s" % (fmt(uw.min[3:]), fmt(uw.max[3:])))
    if args.pdf:
        h, mean, sigma = rep["pdf"]
        width = (h.hi[0] - h.lo[0]) / h.nbins / sigma              # in units of sigma: the density below is that of (x - mean) / sigma
        tails = float(h.below[0] + h.above[0] + h.nonfinite[0]) / h.count
        print("PDF of du_0/dx_0 in units of its sigma = %.9e (%d points, bin width %.17g, outside the range: %.17g)" % (sigma, h.count, width, tails))
        for c, p in zip((h.centers(0) - mean) / sigma, h.pdf(0) * sigma):
            print("pdf %+.4f %.17g" % (c, p))
    if args.dissipation and args.pdf:
        for name, h in zip(("eps", "omega2"), rep["dissipation_pdf"]):
            print("PDF of %s over [%.9e, %.9e) (%d points)" % (name, h.lo[0], h.hi[0], h.count))
            for c, p in zip(h.centers(0), h.pdf(0)):
                print("pdf_%s %.9e %.17g" % (name, c, p))
    if args.M == 5 and not args.N and args.steps == 10 and args.precision == "double" and args.cfl is None:
        assert round(ks[0] - 0.124953117517, 7) == 0
        print("matches the reference demo's known answer 0.124953117517")


if __name__ == "__main__":
    main()
