#!/usr/bin/env python3
"""Registers, scratch, LDS and resident workgroups of the kernels of the fused z stage that ends in structure functions
(kernels_nli*.hip) next to their moments twins (kernels_nls*.hip) (developer tool, no GPU needed): reads the built objects like
scripts/kernel_regs.py.  The increments body takes no LDS beyond the exchange buffers, so both twins launch with the same bytes.

    python3 scripts/real_increments_regs.py > profiles/real_increments_regs.tsv

Resident workgroups per CU as in scripts/real_histogram_regs.py: min(by LDS: 160 KiB / bytes; by registers: the waves per SIMD the
VGPRs allow / ceil(waves of a workgroup / 4); 4: what the launch asks for at most, core.hip NLS_WG_PER_CU)."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402
from real_histogram_regs import CSRC, resident  # noqa: E402
from real_quadratic_regs import lds_table  # noqa: E402

PAT = re.compile(r"mfft_kern(?:_occ)?<mfft::Nlz(Moments|Incr)<mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r" ?>, mfft::Nl[si]Params<\w+>(?:, (\d+))?>")
NAMES = {"Moments": "moments", "Incr": "incr"}


def table(objs):
    rows = {}
    for obj in objs:
        ks = kernel_regs.kernels_of(obj)
        names = subprocess.run(["c++filt"], input="\n".join(k[4] for k in ks), stdout=subprocess.PIPE, text=True).stdout.split("\n")
        for (v, a, s, _, _), nm in zip(ks, names):
            m = PAT.search(nm)
            if not m:
                continue
            key = (m.group(3), tuple(int(x) for x in m.group(2).split(",")))
            cfg = "rows %s%s%s%s" % (m.group(4), " twlds" if m.group(5) == "true" else "", " split" if m.group(6) == "true" else "",
                                      " wave" if m.group(7) == "true" else "")
            rows.setdefault(key, {})[NAMES[m.group(1)]] = (v, a, s, cfg)
    return rows


def main():
    build = os.path.join(CSRC, "build")
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nls", "nls9", "nli", "nli9") for p in "ds"])
    lds = lds_table()
    header = open(os.path.join(CSRC, "nlz_incr.h")).read()
    maxsep = int(re.search(r"NLI_MAXSEP = (\d+)", header).group(1))
    kinds = ("moments", "incr")
    print("# NlzFft kernels, gfx950: moments (kernels_nls*.hip) | increments (kernels_nli*.hip), NLI_MAXSEP = %d: one pair's 2 x %d x 3 = %d doubles of" % (maxsep, maxsep, 6 * maxsep))
    print("# accumulators in registers across a transform (the moments body holds 36); scratch in bytes per lane; lds = dynamic bytes of the")
    print("# launch (the same for both: the row is read back out of the exchange buffer); wgs = resident workgroups per CU")
    print("precision\tplan\tthreads\tconfig\t" + "\t".join("%s_%s" % (w, c) for w in kinds for c in ("vgpr", "agpr", "scratch", "lds", "wgs")))
    more = less = same = lost = spill = 0
    spill12 = []
    for (prec, plan), d in sorted(rows.items()):
        threads, l = lds[(prec, plan)]
        cells, wgs = [], {}
        for w in kinds:
            v, a, s, _ = d[w]
            wgs[w] = resident(v, a, threads, l["moments"])
            cells.append("%d\t%d\t%d\t%d\t%d" % (v, a, s, l["moments"], wgs[w]))
        print("%s\t%s\t%d\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), threads, d["incr"][3], "\t".join(cells)))
        more += d["incr"][2] > d["moments"][2]
        less += d["incr"][2] < d["moments"][2]
        same += d["incr"][2] == d["moments"][2]
        lost += wgs["incr"] < wgs["moments"]
        spill += d["incr"][2] > 0
        if d["incr"][2] > 0:
            spill12.append("%s %d: %d" % (prec, plan[0], d["incr"][2]))
    print("# scratch against the moments twin: %d kernels more, %d less, %d the same (of %d)" % (more, less, same, len(rows)))
    print("# increments kernels with scratch: %d of %d%s" % (spill, len(rows), (" (" + "; ".join(spill12) + ")") if spill12 else ""))
    print("# resident workgroups against the moments twin: %d of %d kernels lose one" % (lost, len(rows)))


if __name__ == "__main__":
    main()
