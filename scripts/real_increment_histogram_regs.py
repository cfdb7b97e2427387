#!/usr/bin/env python3
"""Registers, scratch, LDS and resident workgroups of the kernels of the fused z stage that ends in increment histograms
(kernels_nlk*.hip) next to the increments kernels (kernels_nli*.hip: the same skeleton, 48 doubles of accumulators) and the joint
histogram kernels (kernels_nlj*.hip: the same exchange rule and the same ending, counts in LDS) (developer tool, no GPU needed):
reads the built objects like scripts/kernel_regs.py, and asks the registration templates themselves for the LDS bytes, as
scripts/real_joint_regs.py does.

    python3 scripts/real_increment_histogram_regs.py > profiles/real_increment_histogram_regs.tsv

Resident workgroups per CU as in scripts/real_joint_regs.py: min(by LDS: 160 KiB / bytes; by registers: the waves per SIMD the
VGPRs allow / ceil(waves of a workgroup / 4); 4: what the launch asks for at most, core.hip NLS_WG_PER_CU)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402
from real_joint_regs import CSRC, resident  # noqa: E402

PAT = re.compile(r"mfft_kern(?:_occ)?<mfft::Nlz(Incr|Joint|IncrHist)<mfft::NlzFft<mfft::Spec<([0-9, ]+)>, (double|float), (\d+), (true|false), (true|false), (true|false)>"
                 r" ?>, mfft::Nl[ijk]Params<\w+>(?:, (\d+))?>")
NAMES = {"Incr": "incr", "Joint": "joint", "IncrHist": "incr_hist"}
PROBE = r"""
#include <cstdio>
#include "registry_nlz.h"
#include "plans.h"
using namespace mfft;
template <class S, typename T> void row(const char* plan, const char* prec) {
  typedef NlzFft<S, T, nlz_rows<S, T>(), nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()> K;
  typedef NlzFft<S, T, nlz_rows<S, T>(), nlz_twlds<S, T>(), nlj_split<S, T>(), nlj_wave<S, T>()> J;
  printf("%s\t%s\t%d\t%d\t%d\t%d\n", prec, plan, K::THREADS, NlzIncr<K>::LDS_BYTES, NlzJoint<J>::LDS_BYTES, NlzIncrHist<J>::LDS_BYTES);
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
        prec, plan, threads, li, lj, lk = l.split("\t")
        t[(prec, tuple(int(x) for x in plan.replace(" ", "").split(",")))] = (int(threads), {"incr": int(li), "joint": int(lj), "incr_hist": int(lk)})
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
    rows = table([os.path.join(build, "kernels_%s_%s.o" % (u, p)) for u in ("nli", "nli9", "nlj", "nlj9", "nlk", "nlk9") for p in "ds"])
    lds = lds_table()
    kinds = ("incr", "joint", "incr_hist")
    print("# NlzFft kernels, gfx950: increments (kernels_nli*.hip) | joint histogram (kernels_nlj*.hip) | increment histogram (kernels_nlk*.hip),")
    print("# NLK_MAXBINS = 256, NLI_MAXSEP = 8.  The increment-histogram body holds NO accumulators (the increments body holds 48 doubles): a slot and an")
    print("# LDS add per increment; it takes the joint kernels' exchange and wave build (nlj_split, nlj_wave: config) and 2 x 8 x 259 x 4 = 16576")
    print("# bytes of LDS behind the exchange (the joint grid: 17956).  scratch in bytes per lane; lds = dynamic bytes of the launch; wgs = resident")
    print("# workgroups per CU")
    print("precision\tplan\tthreads\tincr_config\tconfig\t" + "\t".join("%s_%s" % (w, c) for w in kinds for c in ("vgpr", "agpr", "scratch", "lds", "wgs")))
    spill, spill_incr, lost_j, lost_i, worse = [], 0, 0, 0, 0
    for (prec, plan), d in sorted(rows.items()):
        threads, l = lds[(prec, plan)]
        cells, wgs = [], {}
        for w in kinds:
            v, a, s, _ = d[w]
            wgs[w] = resident(v, a, threads, l[w])
            cells.append("%d\t%d\t%d\t%d\t%d" % (v, a, s, l[w], wgs[w]))
        assert d["incr_hist"][3] == d["joint"][3], (prec, plan)      # one exchange rule
        print("%s\t%s\t%d\t%s\t%s\t%s" % (prec, "x".join(str(x) for x in plan[1:]) + "=" + str(plan[0]), threads, d["incr"][3], d["incr_hist"][3], "\t".join(cells)))
        if d["incr_hist"][2] > 0:
            spill.append("%s %d: %d" % (prec, plan[0], d["incr_hist"][2]))
        spill_incr += d["incr"][2] > 0
        worse += d["incr_hist"][2] > d["joint"][2]
        lost_j += wgs["incr_hist"] < wgs["joint"]
        lost_i += wgs["incr_hist"] < wgs["incr"]
    n = len(rows)
    print("# increment-histogram kernels with scratch: %d of %d%s; increments kernels with scratch: %d" % (len(spill), n, (" (" + "; ".join(spill) + ")") if spill else "", spill_incr))
    print("# expectation: the register picture of the histogram kernels, not of the increments kernels -- no more scratch than the joint twin: %s (%d kernels with more)"
          % ("met" if worse == 0 else "NOT met", worse))
    print("# resident workgroups: %d of %d kernels hold fewer than the joint twin, %d fewer than the increments kernel" % (lost_j, n, lost_i))


if __name__ == "__main__":
    main()
