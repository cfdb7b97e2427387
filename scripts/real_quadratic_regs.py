#!/usr/bin/env python3
"""Registers, scratch, LDS and resident workgroups of the kernels of the fused z stage that ends in the statistics of a quadratic
form (kernels_nlq*.hip) next to their moments and histogram twins (kernels_nls*.hip, kernels_nlh*.hip) (developer tool, no GPU
needed): reads the built objects like scripts/kernel_regs.py, and asks the registration templates themselves for the LDS bytes (a
host-only program of a few lines, compiled on the fly: the exchange buffers are dynamic LDS, which the code objects do not record).

    python3 scripts/real_quadratic_regs.py > profiles/real_quadratic_regs.tsv

Resident workgroups per CU as in scripts/real_histogram_regs.py: min(by LDS: 160 KiB / bytes; by registers: the waves per SIMD the
VGPRs allow / ceil(waves of a workgroup / 4); 4: what the launch asks for at most, core.hip NLS_WG_PER_CU)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402
from real_histogram_regs import CSRC, resident  # noqa: E402

PAT = re.compile(r"mfft_kern(?:_occ)?<mfft::Nlz(Moments|Hist|Quad)<mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r"(?:, false)? ?>, mfft::Nl[shq]Params<\w+>(?:, (\d+))?>")
NAMES = {"Moments": "moments", "Hist": "hist", "Quad": "quad"}
PROBE = r"""
#include <cstdio>
#include "registry_nlz.h"
#include "plans.h"
using namespace mfft;
template <class S, typename T> void row(const char* plan, const char* prec) {
  typedef NlzFft<S, T, nlz_rows<S, T>(), nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()> K;
  printf("%s\t%s\t%d\t%d\t%d\t%d\n", prec, plan, K::THREADS, NlzMoments<K>::LDS_BYTES, NlzHist<K>::LDS_BYTES, NlzQuad<K>::LDS_BYTES);
}
#define ROW(N, ...) row<Spec<N, __VA_ARGS__>, double>(#N "," #__VA_ARGS__, "double"); row<Spec<N, __VA_ARGS__>, float>(#N "," #__VA_ARGS__, "float");
int main() { MFFT_NLZPLANS_P2(ROW) MFFT_NLZPLANS_3(ROW) MFFT_NLZPLANS_9(ROW) return 0; }
"""


def lds_table():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.hip"), os.path.join(d, "probe")
        open(src, "w").write(PROBE)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-std=c++17", "-O0", "-I" + CSRC, "-I/opt/rocm/include", src, "-o", exe], check=True)
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    t = {}
    for l in out.splitlines():
        prec, plan, threads, lm, lh, lq = l.split("\t")
        t[(prec, tuple(int(x) for x in plan.replace(" ", "").split(",")))] = (int(threads), {"moments": int(lm), "hist": int(lh), "quad": int(lq)})
    return t


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
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nls", "nls9", "nlh", "nlh9", "nlq", "nlq9") for p in "ds"])
    lds = lds_table()
    kinds = ("moments", "hist", "quad")
    print("# NlzFft kernels, gfx950: moments (kernels_nls*.hip) | histogram (kernels_nlh*.hip) | quadratic form (kernels_nlq*.hip), NLH_MAXBINS = 512")
    print("# scratch in bytes per lane; lds = dynamic bytes of the launch (histogram: the moments twin's + 2 x 515 x 4, quadratic: + 515 x 4); wgs = resident workgroups per CU")
    print("precision\tplan\tthreads\tconfig\t" + "\t".join("%s_%s" % (w, c) for w in kinds for c in ("vgpr", "agpr", "scratch", "lds", "wgs")))
    cmp = {"moments": [0, 0, 0], "hist": [0, 0, 0]}
    lost = {"moments": 0, "hist": 0}
    for (prec, plan), d in sorted(rows.items()):
        threads, l = lds[(prec, plan)]
        cells, wgs = [], {}
        for w in kinds:
            v, a, s, _ = d[w]
            wgs[w] = resident(v, a, threads, l[w])
            cells.append("%d\t%d\t%d\t%d\t%d" % (v, a, s, l[w], wgs[w]))
        print("%s\t%s\t%d\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), threads, d["quad"][3], "\t".join(cells)))
        for w in ("moments", "hist"):
            cmp[w][0] += d["quad"][2] > d[w][2]
            cmp[w][1] += d["quad"][2] < d[w][2]
            cmp[w][2] += d["quad"][2] == d[w][2]
            lost[w] += wgs["quad"] < wgs[w]
    for w in ("moments", "hist"):
        print("# scratch against the %s twin: %d kernels more, %d less, %d the same (of %d)" % (w, cmp[w][0], cmp[w][1], cmp[w][2], len(rows)))
        print("# resident workgroups against the %s twin: %d of %d kernels lose one" % (w, lost[w], len(rows)))


if __name__ == "__main__":
    main()
