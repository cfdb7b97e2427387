#!/usr/bin/env python3
"""Registers and scratch of the fused nonlinear z kernels that also emit the real-space maxima (Build::AbsMax, kernels_nlm*.hip)
next to the kernels they shadow, cross and dot product (developer tool, no GPU needed): reads the built objects like
scripts/kernel_regs.py.

    python3 scripts/nonlinear_absmax_regs.py > profiles/nonlinear_absmax_regs.tsv"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

CSRC = os.path.join(kernel_regs.ROOT, "mpifft4py_amd", "csrc")
FFT = r"mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
PLAIN = re.compile(r"mfft_kern(?:_occ)?<(mfft::NlzProd<)?" + FFT + r"(?:, \(mfft::NlzProduct\)1>)?, mfft::NlzParams<\w+>(?:, (\d+))?>")
STATS = re.compile(r"mfft_kern(?:_occ)?<mfft::NlzAbsMax<" + FFT + r", \(mfft::NlzProduct\)([01])>, mfft::NlmParams<\w+>(?:, (\d+))?>")


def main():
    build = os.path.join(CSRC, "build")
    rows = {}
    for u in ("nlz", "nlz9", "nld", "nld9", "nlm", "nlm9"):
        for p in "ds":
            ks = kernel_regs.kernels_of(os.path.join(build, "kernels_%s_%s.o" % (u, p)))
            names = subprocess.run(["c++filt"], input="\n".join(k[4] for k in ks), stdout=subprocess.PIPE, text=True).stdout.split("\n")
            for (v, a, s, _, _), nm in zip(ks, names):
                m = PLAIN.search(nm)
                if m:
                    which, g = ("dot" if m.group(1) else "cross"), m.groups()[1:7]
                else:
                    m = STATS.search(nm)
                    if not m:
                        continue
                    which, g = ("dot_absmax" if m.group(7) == "1" else "cross_absmax"), m.groups()[0:6]
                key = (g[1], tuple(int(x) for x in g[0].split(",")))
                rows.setdefault(key, {})[which] = (v, a, s)
    print("# NlzFft kernels, gfx950: the plain kernels (kernels_nlz*.hip, kernels_nld*.hip) | the same with the six maxima (kernels_nlm*.hip)")
    print("# vgpr+agpr / bytes of scratch per lane; rows, exchange, twiddle placement and register cap are the plain kernel's")
    print("# (one exception to the cap: the single-precision dot_absmax kernels of 1024 and 2048 take three waves where dot takes four)")
    print("precision\tplan\tcross\tcross_absmax\tdot\tdot_absmax")
    for (prec, plan), d in sorted(rows.items()):
        print("%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]),
                              "\t".join("%d+%d / %d" % d[w] if w in d else "-" for w in ("cross", "cross_absmax", "dot", "dot_absmax"))))


if __name__ == "__main__":
    main()
