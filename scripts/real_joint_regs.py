#!/usr/bin/env python3
"""Registers, scratch, LDS and resident workgroups of the kernels of the fused z stage that ends in a JOINT histogram
(kernels_nlj*.hip) next to their histogram twins (kernels_nlh*.hip) (developer tool, no GPU needed): reads the built objects like
scripts/kernel_regs.py, and asks the registration templates themselves for the LDS bytes (a host-only program of a few lines,
compiled on the fly: the exchange buffers are dynamic LDS, which the code objects do not record).  The joint kernels choose
their exchange by a rule of their own (csrc/registry_nlz.h nlj_split): the config column names both builds where they differ.

    python3 scripts/real_joint_regs.py > profiles/real_joint_regs.tsv

Resident workgroups per CU = min(by LDS: 160 KiB / bytes; by registers: the waves per SIMD the VGPRs allow / ceil(waves of a
workgroup / 4), the dispatcher's rule of csrc/registry.h; 4: what the launch asks for at most, core.hip NLS_WG_PER_CU)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

CSRC = os.path.join(kernel_regs.ROOT, "mpifft4py_amd", "csrc")
PAT = re.compile(r"mfft_kern(?:_occ)?<mfft::Nlz(Hist|Joint)<mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r"(?:, false)? ?>, mfft::Nl[hj]Params<\w+>(?:, (\d+))?>")
LDS_CU = 160 * 1024
PROBE = r"""
#include <cstdio>
#include "registry_nlz.h"
#include "plans.h"
using namespace mfft;
template <class S, typename T> void row(const char* plan, const char* prec) {
  typedef NlzFft<S, T, nlz_rows<S, T>(), nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()> K;
  typedef NlzFft<S, T, nlz_rows<S, T>(), nlz_twlds<S, T>(), nlj_split<S, T>(), nlj_wave<S, T>()> J;
  printf("%s\t%s\t%d\t%d\t%d\n", prec, plan, K::THREADS, NlzHist<K>::LDS_BYTES, NlzJoint<J>::LDS_BYTES);
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
        prec, plan, threads, lm, lh = l.split("\t")
        t[(prec, tuple(int(x) for x in plan.replace(" ", "").split(",")))] = (int(threads), int(lm), int(lh))
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
            rows.setdefault(key, {})["joint" if m.group(1) == "Joint" else "hist"] = (v, a, s, cfg)
    return rows


def resident(v, a, threads, lds):
    by_regs = kernel_regs.waves(v, a) // (((threads + 63) // 64 + 3) // 4)
    return max(0, min(LDS_CU // lds, by_regs, 4))


def main():
    build = os.path.join(CSRC, "build")
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nlh", "nlh9", "nlj", "nlj9") for p in "ds"])
    lds = lds_table()
    print("# NlzFft kernels, gfx950: histogram (kernels_nlh*.hip) | joint histogram (kernels_nlj*.hip), shipped build, NLJ_MAXBINS = 64")
    print("# scratch in bytes per lane; lds = dynamic bytes of the launch (joint: its own exchange + 4489 x 4); wgs = resident workgroups per CU")
    print("precision\tplan\tthreads\thist_config\tjoint_config\t" + "\t".join("%s_%s" % (w, c) for w in ("hist", "joint") for c in ("vgpr", "agpr", "scratch", "lds", "wgs")))
    lost = more = less = same = changed = fp32_scratch = 0
    for (prec, plan), d in sorted(rows.items()):
        threads, lh, lj = lds[(prec, plan)]
        cells = []
        wgs = {}
        for w, l in (("hist", lh), ("joint", lj)):
            v, a, s, _ = d[w]
            wgs[w] = resident(v, a, threads, l)
            cells.append("%d\t%d\t%d\t%d\t%d" % (v, a, s, l, wgs[w]))
        print("%s\t%s\t%d\t%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), threads, d["hist"][3], d["joint"][3], "\t".join(cells)))
        lost += wgs["joint"] < wgs["hist"]
        changed += d["joint"][3] != d["hist"][3]
        more += d["joint"][2] > d["hist"][2]
        less += d["joint"][2] < d["hist"][2]
        same += d["joint"][2] == d["hist"][2]
        fp32_scratch += prec == "float" and d["joint"][2] > 0
    print("# exchange or wave build differs from the histogram twin: %d of %d kernels" % (changed, len(rows)))
    print("# resident workgroups against the histogram twin: %d of %d kernels lose one" % (lost, len(rows)))
    print("# scratch against the histogram twin: %d kernels more, %d less, %d the same" % (more, less, same))
    print("# expectation: no scratch in fp32: %s (%d kernels with scratch)" % ("met" if fp32_scratch == 0 else "NOT met", fp32_scratch))
    more64 = sum(1 for (prec, _), d in rows.items() if prec == "double" and d["joint"][2] > d["hist"][2])
    print("# expectation: no more scratch in fp64 than the twin: %s (%d kernels with more)" % ("met" if more64 == 0 else "NOT met", more64))


if __name__ == "__main__":
    main()
