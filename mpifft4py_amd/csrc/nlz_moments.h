// nlz_moments.h -- the fused z stage that ends in one-point MOMENTS (Op::Moments; kernels_nls*.hip).
#pragma once
#include "nlz_reduce.h"

namespace mfft {

// ... of the kernel that ends in a REDUCTION instead of a product (NlzMoments::body below): min, max and the sums of the first
// four powers of up to six real fields.  Pair p is a[p] + i b[p] on one complex transform, p < npairs; b[p] may be null (an odd
// field count: the partner reads as zeros and its statistics mean nothing).  out[], scale and valid are not used.
constexpr int NLS_SLOTS = 2 * NLS_PAIRS * NLS_STATS;            // doubles per wave in NlsParams::part: [pair][a, b][statistic]
template <typename T>
struct NlsParams : NlzParams<T> {
  double* part;                // (waves of the launch, NLS_SLOTS) partial statistics, every slot written
  double center[2 * NLS_PAIRS];   // [pair][a, b]: S_p = sum (x - center)^p, x the normalised value
  double norm;                 // x = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};

// one value into the six statistics of its field (double whatever the rows' precision): m = [min, max, S1, S2, S3, S4]
MFFT_D void moments_add(double (&m)[NLS_STATS], double x, double c) {
  m[0] = nan_min(m[0], x);
  m[1] = nan_max(m[1], x);
  const double d = x - c, d2 = d * d;
  m[2] += d;
  m[3] += d2;
  m[4] += d2 * d;
  m[5] += d2 * d2;
}
MFFT_D void moments_clear(double (&m)[NLS_STATS]) {
  m[0] = __builtin_inf();
  m[1] = -__builtin_inf();
  m[2] = m[3] = m[4] = m[5] = 0.0;
}
MFFT_D void moments_merge(double (&m)[NLS_STATS], const double (&o)[NLS_STATS]) {
  m[0] = nan_min(m[0], o[0]);
  m[1] = nan_max(m[1], o[1]);
#pragma unroll
  for (int k = 2; k < NLS_STATS; ++k) m[k] += o[k];
}

// The six statistics of one field over the WHOLE wave, by a fixed butterfly (the same order of additions every run: the sums are
// bitwise reproducible); lane 0 stores them.  Missing lanes of a workgroup's last wave are left out as above.
template <int THREADS>
MFFT_D void wave_moments_store(double (&m)[NLS_STATS], int tid, double* slot) {
  const int lane = tid & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    double other[NLS_STATS];
#pragma unroll
    for (int k = 0; k < NLS_STATS; ++k) other[k] = wave_shfl(m[k], lane ^ o);
    if (THREADS % 64 == 0 || (tid ^ o) < THREADS) moments_merge(m, other);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NLS_STATS; ++k) slot[k] = m[k];
  }
}

// The stage that ends in a REDUCTION: min, max and S_p = sum (x - c)^p, p = 1..4, of up to six real fields over all rows and all
// M positions -- the one-point statistics of a field that never exists in real space.  ceil(nfields / 2) inverse transforms per
// row, nothing forward, nothing stored but the partials; nothing is parked next to a transform's working set but the
// accumulators, 2 x 6 doubles per pair.  The maxima bodies (fft_nlz.h NlzFft::stats) reduce over the wave after every transform; with twelve 64-bit
// values per pair that would be some 140 shuffles per transform, so here a workgroup strides over the pairs of rows
// (unit += ngroups * ROWS), every thread keeps its accumulators for the whole launch, and ONE wave reduction runs at the end:
// lane 0 of every wave stores NLS_SLOTS doubles with plain stores, a fold kernel adds the waves' slots in a fixed order.  Which
// rows a thread meets and the order it adds them in depend on (nrows, ngroups) only: the results are bitwise reproducible.
// Powers and sums in double in both precisions.  Non-finite inputs leave the transform on load (take_out_nonfinite) and come back
// as NaN sums and NaN / +-Inf extremes of THEIR field; the partner of the pair stays what it is.
// ONE transform is inlined, in a loop over the pairs that is not unrolled -- inlined transforms keep each other's LDS
// addresses and twiddle indices live, and the 12-values plans have no registers for that --, and only the accumulation is
// written out per pair, so that the accumulators are indexed statically: registers.  npairs is uniform over the launch, so the
// barriers inside a transform are met by everybody or nobody.
// K's rows, exchanges and inverse transforms around it, NlsParams.
template <class K> struct NlzMoments {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLS_SLOTS doubles in NlsParams::part per workgroup
  template <class PP>
  static MFFT_D void body(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    double acc[NLS_PAIRS][2][NLS_STATS];
#pragma unroll
    for (int p = 0; p < NLS_PAIRS; ++p) {
      moments_clear(acc[p][0]);
      moments_clear(acc[p][1]);
    }
    const i64 last = P.nrows - 1;
    // the values of one pair into its accumulators (swapped results: .y = a_p, .x = b_p at position j + k TPT), and what the load
    // took out of either spectrum (Inf or NaN) into that field's
    auto add = [&](double (&m)[2][NLS_STATS], const cx<T> (&v)[E], const T (&bad)[2], double ca, double cb) {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        moments_add(m[0], (double)v[k].y * P.norm, ca);
        moments_add(m[1], (double)v[k].x * P.norm, cb);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (bad[i] != (T)0) {
          const double w = (double)bad[i], nn = w * 0.0;
          m[i][0] = nan_min(m[i][0], -w);
          m[i][1] = nan_max(m[i][1], w);
#pragma unroll
          for (int k = 2; k < NLS_STATS; ++k) m[i][k] += nn;
        }
    };
#pragma unroll 1
    for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
      const i64 unit = base + rl;                  // a pair of rows
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const i64 row = 2 * unit + h;
        const bool active = row < P.nrows;         // rows past the end re-read the last row and count nothing
        const i64 io = (active ? row : last) * P.in_stride;
#pragma unroll 1
        for (int p = 0; p < P.npairs; ++p) {
          cx<T> v[E];
          T bad[2];
          const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
          const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
          const bool hb = pb != nullptr;
          K::template load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          if (active) {
            if (p == 0) add(acc[0], v, bad, P.center[0], P.center[1]);
            else if (p == 1) add(acc[1], v, bad, P.center[2], P.center[3]);
            else add(acc[2], v, bad, P.center[4], P.center[5]);
          }
        }
      }
    }
    constexpr int NW = (THREADS + 63) / 64;
    double* slot = P.part + ((i64)bid * NW + tid / 64) * NLS_SLOTS;
#pragma unroll
    for (int p = 0; p < NLS_PAIRS; ++p) {
      if (p < P.npairs) {
        wave_moments_store<THREADS>(acc[p][0], tid, slot + (2 * p) * NLS_STATS);
        wave_moments_store<THREADS>(acc[p][1], tid, slot + (2 * p + 1) * NLS_STATS);
      } else if ((tid & 63) == 0) {                // every slot written: the fold reads them all
#pragma unroll
        for (int k = 0; k < NLS_STATS; ++k) slot[(2 * p) * NLS_STATS + k] = slot[(2 * p + 1) * NLS_STATS + k] = acc[p][0][k];
      }
    }
  }
};

}  // namespace mfft
