// nlz_incr.h -- the fused z stage that ends in STRUCTURE FUNCTIONS along z (Op::Increments; kernels_nli*.hip).
#pragma once
#include "nlz_reduce.h"

namespace mfft {

// ... of the kernel that ends in STRUCTURE FUNCTIONS (NlzIncr::body below): the sums of the second, third and fourth powers of
// the increments along z, d = r(z + s) - r(z), of up to six real fields for up to NLI_MAXSEP separations s -- the first two-point
// statistic.  Pairs as in NlsParams.  Per field and separation NLI_STATS sums: S2, S3, S4 (S1 is zero on a periodic row).
constexpr int NLI_MAXSEP = 8, NLI_STATS = 3;                    // separations per launch (include/mpifft4py_amd.h MFFT_INCR_MAXSEP)
constexpr int NLI_FIELD = NLI_MAXSEP * NLI_STATS;               // doubles per field: [separation][S2, S3, S4]
constexpr int NLI_SLOTS = 2 * NLS_PAIRS * NLI_FIELD;            // doubles per wave in NliParams::part: [pair][a, b][separation][sum]
template <typename T>
struct NliParams : NlzParams<T> {
  double* part;                // (waves of the launch, NLI_SLOTS) partial sums, every slot written (zeros where nothing was added)
  double norm;                 // r = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int sep[NLI_MAXSEP];         // 1 <= sep[i] <= M - 1, in grid points of the row, i < nsep; duplicates allowed
  int nsep;                    // 1 .. NLI_MAXSEP
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The sums of one increment (the rule of the increments: nlz_reduce.h incr_value).
MFFT_D void incr_add(double* m, double r1, double r0) {      // m: the NLI_STATS sums of one field and separation
  const double d = r1 - r0, d2 = d * d;
  m[0] += d2;
  m[1] += d2 * d;
  m[2] += d2 * d2;
}
// position (pos + s) mod M of a periodic row, 0 <= pos < M, 1 <= s < M
MFFT_D int incr_pos(int pos, int s, int M) {
  const int q = pos + s;
  return q >= M ? q - M : q;
}

// The stage that ends in STRUCTURE FUNCTIONS: S_p(s) = sum (r(z + s) - r(z))^p, p = 2, 3, 4, over all rows and all M positions of
// up to six real fields, for up to NLI_MAXSEP separations along z -- a two-point statistic of fields that never exist in real
// space.  Increments along z are local to a row, and after run_passes a thread group holds the whole real row of two fields
// (positions j + k TPT): the row goes into the row's own exchange buffer at its natural positions, and every thread reads its E
// positions back shifted by s, once per separation.  The skeleton is NlzHist::body's with the loop over the PAIRS outermost, so that
// only one pair's accumulators are live: 2 fields x NLI_MAXSEP x 3 doubles in registers (statically indexed: the loop over the
// separations is unrolled and guarded by nsep), kept over all rows of the workgroup, ONE wave reduction per pair at the end,
// plain stores of every slot; incr_fold (incr.hip) adds the waves' slots in fixed order: bitwise reproducible, no atomics.
// With the whole-complex exchange the buffer holds both fields of the pair at once; with the split exchange it holds ONE real
// value per position, so the two fields take two rounds.  Synchronisation as the build requires (nlz_sync): before the store
// everybody has left the transform's last gather and the reads of the round before; after it the row is there; the sync before
// the next transform's passes (below, as in NlzMoments::body) keeps its scatter behind the last reads.  All of them sit where every
// thread of the workgroup arrives -- nsep and npairs are uniform, a row past the end runs the same code and adds nothing.
// Non-finite bins leave the transform on load; the thread that met one adds NaN to every sum of THAT field, the partner stays exact.
// K's rows, exchanges and inverse transforms around it, NliParams; no LDS beyond K's own.
template <class K> struct NlzIncr {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLI_SLOTS doubles in NliParams::part per workgroup
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
    const i64 last = P.nrows - 1;
    const int nsep = P.nsep < NLI_MAXSEP ? P.nsep : NLI_MAXSEP;
    constexpr int NW = (THREADS + 63) / 64;
    double* slot = P.part + ((i64)bid * NW + tid / 64) * NLI_SLOTS;
    // one separation's clamped value: no index reaches LDS on the strength of the caller's list alone
    // (hidden from the optimiser inside the row loop: left alone, hipcc hoists the E LDS addresses of every separation out of the
    // loop over the rows -- 8 E registers next to 48 doubles of accumulators, 150 - 850 bytes of scratch in every kernel)
    auto sep_of = [&](int i) {
      int s = P.sep[i];
      s = s < 1 ? 1 : s > M - 1 ? M - 1 : s;
      MFFT_HIDE_RANGE(s);
      return s;
    };
#pragma unroll 1
    for (int p = 0; p < NLS_PAIRS; ++p) {
      double acc[2][NLI_FIELD];                    // [a_p, b_p][separation][S2, S3, S4]
#pragma unroll
      for (int i = 0; i < NLI_FIELD; ++i) acc[0][i] = acc[1][i] = 0.0;
      if (p < P.npairs) {                          // (uniform over the launch)
        const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
        const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
        const bool hb = pb != nullptr;
#pragma unroll 1
        for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
          const i64 unit = base + rl;              // a pair of rows
#pragma unroll 1
          for (int h = 0; h < 2; ++h) {
            const i64 row = 2 * unit + h;
            const bool active = row < P.nrows;     // rows past the end re-read the last row and add nothing
            const i64 io = (active ? row : last) * P.in_stride;
            cx<T> v[E];
            T bad[2];
            K::template load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
            nlz_sync<WAVE>();
            run_passes<S, 0, T>(v, j, tw, xc);
            // swapped results: .y = a_p, .x = b_p at position j + k TPT
            if constexpr (SPLIT) {
#pragma unroll
              for (int f = 0; f < 2; ++f) {
                nlz_sync<WAVE>();
#pragma unroll
                for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = f == 0 ? v[k].y : v[k].x;
                nlz_sync<WAVE>();
                if (active) {
#pragma unroll
                  for (int i = 0; i < NLI_MAXSEP; ++i)
                    if (i < nsep) {
                      const int s = sep_of(i);
#pragma unroll
                      for (int k = 0; k < E; ++k) {
                        const T x1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                        incr_add(acc[f] + i * NLI_STATS, incr_value((double)x1, P.norm), incr_value((double)(f == 0 ? v[k].y : v[k].x), P.norm));
                      }
                    }
                }
              }
            } else {
              nlz_sync<WAVE>();
#pragma unroll
              for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k];
              nlz_sync<WAVE>();
              if (active) {
#pragma unroll
                for (int i = 0; i < NLI_MAXSEP; ++i)
                  if (i < nsep) {
                    const int s = sep_of(i);
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                      const cx<T> z1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                      incr_add(acc[0] + i * NLI_STATS, incr_value((double)z1.y, P.norm), incr_value((double)v[k].y, P.norm));
                      incr_add(acc[1] + i * NLI_STATS, incr_value((double)z1.x, P.norm), incr_value((double)v[k].x, P.norm));
                    }
                  }
              }
            }
            if (active) {
#pragma unroll
              for (int f = 0; f < 2; ++f)
                if (bad[f] != (T)0) {              // what the load took out of this field: all its sums are NaN
                  const double nn = (double)bad[f] * 0.0;
#pragma unroll
                  for (int i = 0; i < NLI_FIELD; ++i)
                    if (i < nsep * NLI_STATS) acc[f][i] += nn;
                }
            }
          }
        }
      }
      // every slot written, the pairs the launch does not have with zeros: the fold reads them all
      wave_sums_store<THREADS, NLI_FIELD>(acc[0], tid, slot + (2 * p) * NLI_FIELD);
      wave_sums_store<THREADS, NLI_FIELD>(acc[1], tid, slot + (2 * p + 1) * NLI_FIELD);
    }
  }
};

}  // namespace mfft
