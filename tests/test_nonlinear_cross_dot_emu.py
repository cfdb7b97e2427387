"""CPU: the cross-and-dot bodies of the fused nonlinear z stage (csrc/fft_nlz.h NlzFft::body_cross_dot) run in the workgroup
emulator against long-double DFTs of irfft(a) x irfft(b) and sum_f irfft(a_f) irfft(c_f) -- every plan of MFFT_NLZPLANS_P2 / _3 /
_9, both precisions, wave-synchronous and barrier builds, whole-complex and split exchanges, with and without LDS twiddles,
limited `valid`, pruned `valid_in`, out of place and in place, an odd row count, and an odd row count in place with NaNs behind
the last row -- and the two entry points of the operation are in the header, the binding and the library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpifft4py_amd", "csrc")
NEW = ["mfft_nonlinear_cross_dot", "mfft_nlz_cross_dot_rows"]


def _nlz_lengths():
    txt = open(os.path.join(CSRC, "plans.h")).read().replace("\\\n", " ")
    out = []
    for group in ("MFFT_NLZPLANS_P2", "MFFT_NLZPLANS_3", "MFFT_NLZPLANS_9"):
        body = re.search(r"#define %s\(X\)(.*)" % group, txt).group(1)
        out += [int(n) for n in re.findall(r"X\((\d+),", body)]
    return out


def test_cross_dot_bodies_in_the_emulator():
    subprocess.check_call(["make", "-C", CSRC, "emu_nlc"])
    exe = os.path.join(CSRC, "build", "emu_nlc")
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "EMU TESTS PASSED" in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("nlc ")]
    lengths = _nlz_lengths()
    assert len(lengths) == 32
    for n in lengths:
        mine = [l for l in lines if re.search(r"N=%d\s" % n, l)]
        assert len(mine) >= 12, (n, mine)
        assert all(l.rstrip().endswith("ok") for l in mine), mine
        for prec in ("double", "single"):
            p = [l for l in mine if prec in l]
            assert any(" split" in l for l in p) and any(" split" not in l for l in p), (n, prec)
            assert any(" twlds" in l for l in p) and any(" twlds" not in l for l in p), (n, prec)
            assert any(" inpl" in l for l in p) and any(" inpl" not in l for l in p), (n, prec)
            assert any(" poison" in l for l in p), (n, prec)      # in place, NaNs behind the odd last row


def test_new_entry_points_in_header_binding_and_library():
    from mpifft4py_amd import _lib
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    declared = set(re.findall(r"MFFT_API\s+[\w\s\*]+?\b(mfft_\w+)\s*\(", header))
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in nm.splitlines() if " T " in l)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert name in exported, name
