#!/usr/bin/env python3
"""Registers and scratch of the outer-product kernels of the fused nonlinear z stage (kernels_nlo*.hip) next to their
cross-product (kernels_nlz*.hip) and cross-and-dot (kernels_nlc*.hip) twins (developer tool, no GPU needed): reads the built
objects like scripts/kernel_regs.py.

    python3 scripts/nonlinear_outer_regs.py > profiles/nonlinear_outer_regs.tsv"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

CSRC = os.path.join(kernel_regs.ROOT, "mpifft4py_amd", "csrc")
PAT = re.compile(r"mfft_kern(?:_occ)?<(?:mfft::NlzProd<)?mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r"(?:, \(mfft::NlzProduct\)([23])>)?, mfft::Nl[zco]Params<\w+>(?:, (\d+))?>")
WHICH = {None: "cross", "2": "cross_dot", "3": "outer"}


def table(objs):
    rows = {}
    for obj in objs:
        ks = kernel_regs.kernels_of(obj)
        names = subprocess.run(["c++filt"], input="\n".join(k[4] for k in ks), stdout=subprocess.PIPE, text=True).stdout.split("\n")
        for (v, a, s, lds, _), nm in zip(ks, names):
            m = PAT.search(nm)
            if not m:
                continue
            key = (m.group(2), tuple(int(x) for x in m.group(1).split(",")))
            cfg = "rows %s%s%s%s" % (m.group(3), " twlds" if m.group(4) == "true" else "", " split" if m.group(5) == "true" else "",
                                      " wave" if m.group(6) == "true" else "")
            cap = int(m.group(8)) - 16 if m.group(8) else 0
            rows.setdefault(key, {})[WHICH[m.group(7)]] = (v, a, s, lds, cap, cfg)
    return rows


def fmt(r, config):
    if not r:
        return "-\t-\t-" + ("\t-\t-\t-" if config else "")
    return "%d\t%d\t%d" % r[:3] + ("\t%d\t%d\t%s" % r[3:] if config else "")


def main():
    build = os.path.join(CSRC, "build")
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nlz", "nlz9", "nlc", "nlc9", "nlo", "nlo9") for p in "ds"])
    print("# NlzFft kernels, gfx950: cross product (kernels_nlz*.hip) | cross and dot product (kernels_nlc*.hip) | outer product (kernels_nlo*.hip), shipped build")
    print("# cap = waves per SIMD the launch bounds ask for; scratch in bytes per lane; lds = static bytes (the exchange buffers are dynamic)")
    print("precision\tplan\t" + "\t".join("%s_%s" % (w, c) for w in ("cross", "cross_dot") for c in ("vgpr", "agpr", "scratch")) + "\t" +
          "\t".join("outer_%s" % c for c in ("vgpr", "agpr", "scratch", "lds", "cap", "config")))
    n = spill = 0
    for (prec, plan), d in sorted(rows.items()):
        print("%s\t%s\t%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), fmt(d.get("cross"), False),
                                      fmt(d.get("cross_dot"), False), fmt(d.get("outer"), True)))
        if d.get("outer"):
            n += 1
            spill += d["outer"][2] > 0
    print("# %d outer-product kernels, %d of them with scratch" % (n, spill))


if __name__ == "__main__":
    main()
