#!/usr/bin/env python3
"""Registers and scratch of every gfx950 kernel in the built objects (developer tool, no GPU needed).

    python3 scripts/kernel_regs.py [build dir] > regs.tsv          # one line per kernel: vgpr agpr scratch lds symbol
    python3 scripts/kernel_regs.py --diff old.tsv new.tsv          # kernels whose numbers changed, worst first
    python3 scripts/kernel_regs.py --code [build dir] > code.tsv   # ... with a sixth column: a hash of the kernel's machine code

Reads the code-object metadata (clang-offload-bundler --unbundle, llvm-readelf --notes) of mpifft4py_amd/csrc/build/*.o.
Why it exists: in round 4 an edit that did not concern them moved the c2r kernels of the 7 * 2^a plans from 248 to 262
VGPRs -- from two waves per SIMD to one, 2 x the time -- and no test or benchmark noticed (profiles/r05_radix7_c2r_bisect.txt).
Run before and after a change to a kernel header; `--diff` lists what moved across an occupancy step (512 / n waves:
128, 168, 256 VGPRs) or started to spill.
--code is for a change that should move code without changing it (a body into another header, a wrapper around a kernel): the hash
is over the bytes of the kernel's function symbol in the gfx950 code object (llvm-readelf: the symbol's address and size, its
section's address and file offset), so two builds give equal hashes exactly where the instruction stream is the same.  `--diff`
of two such files also lists the kernels whose registers are what they were and whose code is not, and counts them in a
second summary line."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def code_hashes(co):
    """{function symbol: hash of its bytes} of a code object file"""
    elf = open(co, "rb").read()
    secs = {}
    for l in subprocess.run([LLVM + "/llvm-readelf", "-S", "--wide", co], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n"):
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+([0-9a-f]+)", l)
        if m:
            secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for l in subprocess.run([LLVM + "/llvm-readelf", "--symbols", "--wide", co], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n"):
        f = l.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, off = secs[int(f[6])]
            start = int(f[1], 16) - addr + off
            out[f[7]] = hashlib.sha1(elf[start:start + int(f[2])]).hexdigest()[:16]
    return out


def kernels_of(obj, code=False):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        if not os.path.exists(fat) or os.path.getsize(fat) == 0:
            return []
        subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, stderr=subprocess.DEVNULL)
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], stdout=subprocess.PIPE, check=True).stdout.decode()
        hashes = code_hashes(co) if code else {}
    out = []
    for blk in notes.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk))
        if "name" in f:
            out.append((int(f.get("vgpr_count", 0)), int(f.get("agpr_count", 0)), int(f.get("private_segment_fixed_size", 0)),
                        int(f.get("group_segment_fixed_size", 0)), f["name"]) + ((hashes[f["name"]],) if code else ()))
    return out


def waves(v, a):
    tot = (v + a + 7) // 8 * 8
    return max(1, min(8, 512 // max(tot, 1)))


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--diff":
        def load(p):
            return {l.split("\t")[4].strip(): tuple(int(x) for x in l.split("\t")[:4]) for l in open(p) if l.strip()}

        def load_code(p):
            return {f[4].strip(): f[5].strip() for f in (l.split("\t") for l in open(p) if l.strip()) if len(f) > 5}
        old, new = load(sys.argv[2]), load(sys.argv[3])
        oldc, newc = load_code(sys.argv[2]), load_code(sys.argv[3])
        rows = []
        for k in sorted(set(old) & set(new)):
            o, n = old[k], new[k]
            if o[:3] != n[:3]:
                rows.append((waves(n[0], n[1]) - waves(o[0], o[1]), n[2] - o[2], k, o, n))
        rows.sort()
        names = subprocess.run(["c++filt"], input="\n".join(r[2] for r in rows), stdout=subprocess.PIPE, text=True).stdout.split("\n")
        for (dw, ds, k, o, n), nm in zip(rows, names):
            print("waves/SIMD %d -> %d  vgpr+agpr %d+%d -> %d+%d  scratch %d -> %d  %s" % (
                waves(o[0], o[1]), waves(n[0], n[1]), o[0], o[1], n[0], n[1], o[2], n[2], nm[:170]))
        print("# %d kernels changed (of %d common; %d only old, %d only new)" % (len(rows), len(set(old) & set(new)),
                                                                                  len(set(old) - set(new)), len(set(new) - set(old))))
        if oldc and newc:
            both = sorted(set(oldc) & set(newc))
            moved = [k for k in both if oldc[k] != newc[k]]
            same_regs = [k for k in moved if old[k][:3] == new[k][:3]]
            names = subprocess.run(["c++filt"], input="\n".join(same_regs), stdout=subprocess.PIPE, text=True).stdout.split("\n")
            for k, nm in zip(same_regs, names):
                print("code differs, registers and scratch as they were  %s" % nm[:170])
            print("# %d kernels differ in code (of %d with a code hash in both files)" % (len(moved), len(both)))
        return
    code = len(sys.argv) > 1 and sys.argv[1] == "--code"
    args = sys.argv[2:] if code else sys.argv[1:]
    build = args[0] if args else os.path.join(ROOT, "mpifft4py_amd", "csrc", "build")
    for obj in sorted(glob.glob(os.path.join(build, "*.o"))):
        for k in kernels_of(obj, code):
            print("\t".join(str(x) for x in k))


if __name__ == "__main__":
    main()
