#!/usr/bin/env python3
"""Registers and scratch of the dot-product kernels of the fused nonlinear z stage next to their cross-product counterparts
(developer tool, no GPU needed): reads the built objects like scripts/kernel_regs.py.

    python3 scripts/nonlinear_dot_regs.py > profiles/nonlinear_dot_regs.tsv           # the shipped build
    python3 scripts/nonlinear_dot_regs.py --caps >> profiles/nonlinear_dot_regs.tsv   # + the dot kernels compiled under forced caps

--caps compiles the four kernels_nld*.hip units with -DMFFT_NLD_OCC=2, 3 and 4 (every plan under ONE cap of that many waves
per SIMD) into a temporary directory: the table behind registry_nlz.h nld_occ."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

CSRC = os.path.join(kernel_regs.ROOT, "mpifft4py_amd", "csrc")
PAT = re.compile(r"mfft_kern(?:_occ)?<(mfft::NlzProd<)?mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r"(?:, \(mfft::NlzProduct\)1>)?, mfft::NlzParams<\w+>(?:, (\d+))?>")


def table(objs):
    rows = {}
    for obj in objs:
        ks = kernel_regs.kernels_of(obj)
        names = subprocess.run(["c++filt"], input="\n".join(k[4] for k in ks), stdout=subprocess.PIPE, text=True).stdout.split("\n")
        for (v, a, s, lds, _), nm in zip(ks, names):
            m = PAT.search(nm)
            if not m:
                continue
            key = (m.group(3), tuple(int(x) for x in m.group(2).split(",")))
            cfg = "rows %s%s%s%s" % (m.group(4), " twlds" if m.group(5) == "true" else "", " split" if m.group(6) == "true" else "",
                                      " wave" if m.group(7) == "true" else "")
            cap = int(m.group(8)) - 16 if m.group(8) else 0
            rows.setdefault(key, {})["dot" if m.group(1) else "cross"] = (v, a, s, lds, cap, cfg)
    return rows


def fmt(r):
    return "%d\t%d\t%d\t%d\t%d\t%s" % r if r else "-\t-\t-\t-\t-\t-"


def main():
    build = os.path.join(CSRC, "build")
    if "--caps" not in sys.argv:
        rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nlz", "nlz9", "nld", "nld9") for p in "ds"])
        print("# NlzFft kernels, gfx950: cross product (kernels_nlz*.hip) | dot product (kernels_nld*.hip), shipped build")
        print("# cap = waves per SIMD the launch bounds ask for; scratch in bytes per lane; lds = static bytes (the exchange buffers are dynamic)")
        print("precision\tplan\t" + "\t".join("%s_%s" % (w, c) for w in ("cross", "dot") for c in ("vgpr", "agpr", "scratch", "lds", "cap", "config")))
        for (prec, plan), d in sorted(rows.items()):
            print("%s\t%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), fmt(d.get("cross")), fmt(d.get("dot"))))
        return
    print("# the dot kernels with every plan under ONE forced cap (-DMFFT_NLD_OCC=n): vgpr+agpr / scratch bytes per lane")
    print("precision\tplan\tcap2\tcap3\tcap4")
    caps = {}
    with tempfile.TemporaryDirectory() as d:
        for occ in (2, 3, 4):
            objs = []
            procs = []
            for u in ("nld", "nld9"):
                for p in "ds":
                    o = os.path.join(d, "occ%d_%s_%s.o" % (occ, u, p))
                    objs.append(o)
                    procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include",
                                                   "-Wno-unknown-pragmas", "-DMFFT_NLD_OCC=%d" % occ, "-c", os.path.join(CSRC, "kernels_%s_%s.hip" % (u, p)),
                                                   "-o", o]))
            for pr in procs:
                assert pr.wait() == 0
            for key, r in table(objs).items():
                caps.setdefault(key, {})[occ] = r["dot"]
    for (prec, plan), d in sorted(caps.items()):
        print("%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]),
                              "\t".join("%d+%d / %d%s" % (d[o][0], d[o][1], d[o][2], " split" if " split" in d[o][5] else "") for o in (2, 3, 4))))


if __name__ == "__main__":
    main()
