#!/usr/bin/env python3
"""The dot-product z kernel (mfft_nlz_dot_rows) of TWO builds of the library against each other: both loaded into one process,
alternating windows of >= 0.3 s on the same rows, HIP events.  How the register caps of registry_nlz.h nld_occ were chosen
(profiles/nonlinear_dot_ab.txt, section 3).  A variant build is the four kernels_nld*.hip units compiled with
-DMFFT_NLD_OCC=n (every plan under a cap of n waves per SIMD) and linked with the other objects of csrc/build:

    make -C mpifft4py_amd/csrc nld_variant OCC=2
    python scripts/nonlinear_dot_occ_ab.py shipped=mpifft4py_amd/libmpifft4py_amd.so occ2=mpifft4py_amd/csrc/build/libmpifft4py_amd_nldocc2.so"""
import ctypes, os, statistics, sys
if len(sys.argv) != 3:
    sys.exit(__doc__)
libs = {a.split("=", 1)[0]: ctypes.CDLL(os.path.abspath(a.split("=", 1)[1]), mode=ctypes.RTLD_LOCAL) for a in sys.argv[1:3]}
V = ctypes.c_void_p
for l in libs.values():
    l.mfft_malloc.argtypes = [ctypes.POINTER(V), ctypes.c_size_t]
    l.mfft_fill_uniform.argtypes = [V, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64]
    l.mfft_nlz_dot_rows.argtypes = [V, V, V] + [ctypes.c_int64] * 4 + [ctypes.c_int, ctypes.c_int]
    l.mfft_timer_create.argtypes = [ctypes.POINTER(V)]
    l.mfft_timer_start.argtypes = [V]
    l.mfft_timer_stop.argtypes = [V, ctypes.POINTER(ctypes.c_float)]
    l.mfft_last_error.restype = ctypes.c_char_p
A = list(libs.values())[0]
def ck(l, rc):
    if rc < 0:
        sys.exit("error %d: %s" % (rc, l.mfft_last_error()))
def timed(l, args, reps):
    t = V(); ck(l, l.mfft_timer_create(ctypes.byref(t))); ck(l, l.mfft_timer_start(t))
    for _ in range(reps):
        ck(l, l.mfft_nlz_dot_rows(*args))
    ms = ctypes.c_float(0); ck(l, l.mfft_timer_stop(t, ctypes.byref(ms)))
    return ms.value / reps
for prec, es in ((1, 16), (0, 8)):
    for M, valid, nrows in ((512, 257, 512 * 128), (1024, 513, 1024 * 48), (2048, 1025, 2048 * 12), (256, 129, 256 * 256), (768, 257, 768 * 96)):
        line = 128 // es
        pitch = (valid + line - 1) // line * line
        n = 3 * nrows * pitch
        a, b = V(), V()
        ck(A, A.mfft_malloc(ctypes.byref(a), n * es)); ck(A, A.mfft_malloc(ctypes.byref(b), n * es))
        ck(A, A.mfft_fill_uniform(a, 2 * n, prec, 1)); ck(A, A.mfft_fill_uniform(b, 2 * n, prec, 2))
        args = (a, b, a, nrows, M, pitch, valid, prec, 0)
        res = {k: [] for k in libs}
        reps = {}
        for k, l in libs.items():
            timed(l, args, 2)
            reps[k] = max(3, int(300.0 / timed(l, args, 3)))
        for r in range(3):
            for k, l in libs.items():
                res[k].append(timed(l, args, reps[k]))
        gb = 7 * nrows * valid * es / 1e9
        print("M=%-5d %s  " % (M, "fp64" if prec else "fp32") + "   ".join("%s %.4f ms [%s] %5.0f GB/s" % (k, statistics.median(v), " ".join("%.4f" % x for x in v), gb / statistics.median(v) * 1e3) for k, v in res.items()), flush=True)
        A.mfft_free(a); A.mfft_free(b)
