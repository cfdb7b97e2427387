// nlz_reduce.h -- what the endings of the fused z stage that reduce instead of transforming forward share (nlz_*.h).
#pragma once
#include "fft_nlz.h"

namespace mfft {

// Up to six real fields per launch: pair p is a[p] + i b[p] on one complex transform, p < npairs <= NLS_PAIRS.
constexpr int NLS_PAIRS = 3, NLS_STATS = 6;                     // per field: min, max, S1 .. S4

// What a body needs of the kernel K = NlzFft<..> it is built around, under the names NlzFft itself uses, so that a body reads
// inside its wrapper as the product bodies read inside NlzFft.  (A macro: a dependent base's names are not found unqualified.)
#define MFFT_NLZ_NAMES_OF(K)                                                                                             \
  typedef typename K::Plan S; typedef typename K::Real T; typedef typename K::XE XE; typedef typename K::Xch Xch;         \
  static constexpr int M = K::M, E = K::E, ROWS = K::NROWS, PD = K::PD, PLEN = K::PLEN, TW_BYTES = K::TW_BYTES;            \
  static constexpr bool TWLDS = K::TW_LDS, SPLIT = K::SPLIT_XCH, WAVE = K::WAVE_XCH

// The slot of a value.  NaN first, before any cast; the upper end compared BEFORE the cast to int (an Inf or a huge t never
// reaches it); a subtraction, then a multiplication: nothing for the compiler to contract, so host and device agree to the bit.
// The result is clamped once more: no index reaches LDS or memory on the strength of the caller's lo and inv alone.
MFFT_D int hist_slot(double x, double lo, double inv, int nbins) {
  const double t = (x - lo) * inv;
  const int s = x != x ? nbins + 2 : t < 0.0 ? 0 : t >= (double)nbins ? nbins + 1 : 1 + (int)t;
  return s < 0 ? 0 : s > nbins + 2 ? nbins + 2 : s;
}
// one count into a workgroup's LDS histogram: an atomic add whose result nobody reads (ds_add_u32); the emulator's threads are
// fibres of one host thread, a plain add there
#if defined(__HIPCC__)
#define MFFT_LDS_COUNT(p) ((void)atomicAdd((p), 1u))
#else
#define MFFT_LDS_COUNT(p) ((void)(*(p) += 1u))
#endif

// The evaluation rule of q (include/mpifft4py_amd.h states it): every product and every sum rounded on its own, in double.  hipcc
// contracts a * b + c into an FMA by default, which rounds once -- the host, numpy and the emulator round twice.  HIP's __dmul_rn
// and __dadd_rn are a plain `*` and `+` in this toolchain's headers and would be contracted all the same once inlined, so the two
// operations are compiled with contraction off instead (the pragma takes the `contract` flag off the instruction itself, wherever
// it is inlined; checked in the kernels' code: v_mul_f64 and v_add_f64, no v_fma_f64 in the accumulation of q).  The emulator is
// built with -ffp-contract=off (Makefile).
MFFT_D double quad_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
MFFT_D double quad_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// The rule of the increments (include/mpifft4py_amd.h states it; kernel, sweep, emulator and tests share it): the value in the
// rows' precision taken to double and normalised THERE -- one rounded product, never contracted into the difference --, the
// difference, its powers and the sums in double.
MFFT_D double incr_value(double x, double norm) { return quad_mul(x, norm); }

// N plain sums over the WHOLE wave by a fixed butterfly (the same order of additions every run: the sums are bitwise reproducible);
// lane 0 stores them.  Lanes past the workgroup's last thread are left out (fft_nlz.h wave_absmax_store).
template <int THREADS, int N>
MFFT_D void wave_sums_store(double (&m)[N], int tid, double* slot) {
  const int lane = tid & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double other = wave_shfl(m[k], lane ^ o);
      if (THREADS % 64 == 0 || (tid ^ o) < THREADS) m[k] += other;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) slot[k] = m[k];
  }
}

}  // namespace mfft
