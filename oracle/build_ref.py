"""Build the ONLY native source of the reference -- mpiFFT4py/cython/maths.pyx
(transpose_Uc, dealias_filter, transpose_Umpi) -- from where it lies under
/root/reference into oracle/_ref/ (git-ignored; travels to the GPU box with the
snapshot).  Nothing of the reference is copied into the tracked tree: the .pyx
is read in place, cython writes its generated C file and gcc the extension
module into oracle/_ref/ only.

    python oracle/build_ref.py          # no-op when /root/reference is absent

The resulting module is test infrastructure: tests compare the oracle's
slab_unpack / apply_mask and the HIP mfft_slab_unpack / mfft_dealias_filter with
the reference's own compiled loops.
"""
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
PYX = "/root/reference/mpiFFT4py/cython/maths.pyx"


def build(verbose=False):
    if not os.path.exists(PYX):
        return None
    import numpy as np
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "ref_maths" + sysconfig.get_config_var("EXT_SUFFIX"))
    if os.path.exists(so) and os.path.getmtime(so) >= os.path.getmtime(PYX):
        return so
    c_file = os.path.join(OUT, "ref_maths.c")
    # module name must match the file name: cython derives PyInit_<name> from --module-name
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "--module-name", "ref_maths", PYX, "-o", c_file],
                          stdout=None if verbose else subprocess.DEVNULL, stderr=subprocess.STDOUT)
    inc = [sysconfig.get_paths()["include"], np.get_include()]
    cmd = ["gcc", "-O2", "-shared", "-fPIC", "-w", "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION"]
    cmd += ["-I" + i for i in inc] + [c_file, "-o", so]
    subprocess.check_call(cmd)
    os.remove(c_file)            # keep only the binary
    return so


def load():
    """Import oracle/_ref/ref_maths if it has been built (returns None otherwise)."""
    import glob
    import importlib.util
    cands = glob.glob(os.path.join(OUT, "ref_maths*.so"))
    if not cands:
        return None
    spec = importlib.util.spec_from_file_location("ref_maths", cands[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GOLDEN = os.path.join(HERE, "..", "tests", "golden", "ref_maths_loops.npz")


def loop_cases():
    """The seeded inputs of the tests that compare with the compiled loops (tests/test_oracle_golden.py: "cpu_*",
    tests/test_gpu_stages.py: "gpu_*"), keyed <case>_<dtype>_<array>."""
    import numpy as np
    cases = {}
    for tag, seed, P, Np0, Np1, Nf, fshape in (("cpu", 8, 4, 3, 5, 9, (6, 7, 5)), ("gpu", 12, 8, 4, 6, 33, (16, 8, 33))):
        rng = np.random.default_rng(seed)
        for dt in (np.complex128, np.complex64):
            key = "%s_%s_" % (tag, np.dtype(dt).name)
            cases[key + "U"] = (rng.random((P, Np0, Np1, Nf)) + 1j * rng.random((P, Np0, Np1, Nf))).astype(dt)
            cases[key + "fu"] = (rng.random(fshape) + 1j * rng.random(fshape)).astype(dt)
            cases[key + "mask"] = (rng.random(fshape) > 0.5).astype(np.uint8)
    return cases


def run_loops(ref, cases):
    """What the compiled loops return for `cases`: <case>_<dtype>_T (transpose_Uc) and _filtered (dealias_filter)."""
    import numpy as np
    out = {}
    for key in [k[:-1] for k in cases if k.endswith("_U")]:
        U = cases[key + "U"]
        P, Np0, Np1, Nf = U.shape
        T = np.zeros((Np0, P * Np1, Nf), dtype=U.dtype)
        ref.transpose_Uc(T, U, P, Np0, Np1, Nf)                      # maths.pyx:21-31
        out[key + "T"] = T
        out[key + "filtered"] = np.asarray(ref.dealias_filter(cases[key + "fu"].copy(), cases[key + "mask"]))   # maths.pyx:9-19
    return out


def write_golden():
    """tests/golden/ref_maths_loops.npz: the inputs of loop_cases and the compiled loops' outputs for them, so that the
    tests that compare with the loops also run where the reference is absent."""
    import numpy as np
    build()
    ref = load()
    cases = loop_cases()
    np.savez_compressed(GOLDEN, **cases, **run_loops(ref, cases))
    return os.path.abspath(GOLDEN)


if __name__ == "__main__":
    print(write_golden() if sys.argv[1:] == ["golden"] else build(verbose=True))
