"""What the tests of the CPU workgroup emulator (csrc/emu/) share: building and running one group, the lengths of the plans of
the fused nonlinear z stage, and the check that an operation's entry points are in the header, the binding and the library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpifft4py_amd", "csrc")

_RUNS = {}


def run_group(name):
    """Build group `name` (csrc/emu/group_<name>.cpp) and run it: once per session, whoever asks."""
    if name not in _RUNS:
        subprocess.check_call(["make", "-C", CSRC, "emu_" + name])
        _RUNS[name] = subprocess.run([os.path.join(CSRC, "build", "emu_" + name)], stdout=subprocess.PIPE, text=True)
    return _RUNS[name]


def plan_lengths(*groups):
    """The lengths N of every X(N, ...) of the plan-list macros `groups` of plans.h."""
    txt = open(os.path.join(CSRC, "plans.h")).read().replace("\\\n", " ")
    out = []
    for group in groups:
        body = re.search(r"#define %s\(X\)(.*)" % group, txt).group(1)
        out += [int(n) for n in re.findall(r"X\((\d+),", body)]
    return out


def nlz_lengths():
    return plan_lengths("MFFT_NLZPLANS_P2", "MFFT_NLZPLANS_3", "MFFT_NLZPLANS_9")


def assert_entry_points(names):
    from mpifft4py_amd import _lib
    header = open(os.path.join(ROOT, "include", "mpifft4py_amd.h")).read()
    declared = set(re.findall(r"MFFT_API\s+[\w\s\*]+?\b(mfft_\w+)\s*\(", header))
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j8"])
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in nm.splitlines() if " T " in l)
    for name in names:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert name in exported, name
