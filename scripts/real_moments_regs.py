#!/usr/bin/env python3
"""Registers and scratch of the kernels of the fused z stage that ends in a reduction (kernels_nls*.hip) next to their
cross-product twins (kernels_nlz*.hip) (developer tool, no GPU needed): reads the built objects like scripts/kernel_regs.py.

    python3 scripts/real_moments_regs.py > profiles/real_moments_regs.tsv"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

CSRC = os.path.join(kernel_regs.ROOT, "mpifft4py_amd", "csrc")
PAT = re.compile(r"mfft_kern(?:_occ)?<(mfft::NlzMoments<)?mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r" ?>?, mfft::Nl[zs]Params<\w+>(?:, (\d+))?>")


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
            rows.setdefault(key, {})["moments" if m.group(1) else "cross"] = (v, a, s, lds, cap, cfg)
    return rows


def fmt(r):
    return "%d\t%d\t%d\t%d\t%d\t%s" % r if r else "-\t-\t-\t-\t-\t-"


def main():
    build = os.path.join(CSRC, "build")
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nlz", "nlz9", "nls", "nls9") for p in "ds"])
    print("# NlzFft kernels, gfx950: cross product (kernels_nlz*.hip) | moments (kernels_nls*.hip), shipped build")
    print("# cap = waves per SIMD the launch bounds ask for; scratch in bytes per lane; lds = static bytes (the exchange buffers are dynamic)")
    print("precision\tplan\t" + "\t".join("%s_%s" % (w, c) for w in ("cross", "moments") for c in ("vgpr", "agpr", "scratch", "lds", "cap", "config")))
    more = less = same = 0
    for (prec, plan), d in sorted(rows.items()):
        print("%s\t%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), fmt(d.get("cross")), fmt(d.get("moments"))))
        if d.get("cross") and d.get("moments"):
            more += d["moments"][2] > d["cross"][2]
            less += d["moments"][2] < d["cross"][2]
            same += d["moments"][2] == d["cross"][2]
    print("# scratch against the cross-product twin: %d kernels more, %d less, %d the same" % (more, less, same))


if __name__ == "__main__":
    main()
