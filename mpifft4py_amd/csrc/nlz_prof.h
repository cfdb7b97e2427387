// nlz_prof.h -- the fused z stage that ends in plane-averaged PROFILES along z (Op::Profiles; kernels_nlp*.hip).
#pragma once
#include "nlz_reduce.h"

namespace mfft {

// ... of the kernel that ends in plane-averaged PROFILES along z (NlzProf::body below): per pair (a_p, b_p) and per position m
// of the row NLP_STATS sums over all rows -- a row is one (x, y) point, so a sum over the rows at a fixed position is a sum over
// the plane z = m.  The first reduction whose result is a vector in z.  Every pair has both fields, as in NljParams.
constexpr int NLP_STATS = 5;                                    // per pair and position: d_a, d_b, d_a^2, d_b^2, d_a d_b (MFFT_PROFILE_STATS)
template <typename T>
struct NlpParams : NlzParams<T> {
  double* part;                // (ngroups x ROWS row slots, npairs, NLP_STATS, M) partial profiles, every slot written
  double center[2 * NLS_PAIRS];   // [pair][a, b]: d = x - center, x the normalised value
  double norm;                 // x = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The rule of the profiles (include/mpifft4py_amd.h states it; kernel, sweep, emulator and tests share it): the value in the rows'
// precision taken to double and normalised THERE by one rounded product (incr_value), the centre subtracted, products and sums in
// double.  m: the NLP_STATS sums of one pair at one position; da, db: the centred values.
MFFT_D void prof_add(double* m, double da, double db) {
  m[0] += da;
  m[1] += db;
  m[2] += da * da;
  m[3] += db * db;
  m[4] += da * db;
}

// The stage that ends in plane-averaged PROFILES along z: per pair (a_p, b_p) and per position m of the row the sums over all rows
// of d_a, d_b, d_a^2, d_b^2, d_a d_b (prof_add) -- <theta>(z), <theta'^2>(z), <u_z theta>(z) of fields that never exist in real
// space.  After run_passes thread (rl, j) holds both values of a pair (.y = a_p, .x = b_p) at the positions j + k TPT, k < E, and
// it holds the SAME positions for every row it meets: a per-position sum over a thread's rows is a plane sum and needs no
// exchange between threads at all, not even a wave reduction.  The skeleton is NlzIncr::body's with the loop over the PAIRS outermost,
// so that only one pair's accumulators are live: E x NLP_STATS doubles in registers, statically indexed, kept over all rows of
// the workgroup.  After the rows of a pair every thread stores its E x NLP_STATS sums with plain stores into the row slot
// (bid ROWS + rl) of P.part, laid out [row slot][pair][sum][position]: lanes with neighbouring j write neighbouring doubles, every
// slot of every row slot and every pair of the launch is written (zeros where nothing was added), and prof_fold (profiles.hip)
// adds the ngroups x ROWS partial profiles in fixed order: bitwise reproducible, no atomics.  No LDS beyond the transform's own.
// Non-finite bins leave the transform on load; the thread that met one adds NaN to ITS positions of that field's two sums and of
// the cross sum, the partner's own two sums stay what they are.  Rows past the end re-read the last row and add nothing; npairs
// is uniform over the launch, so the barriers inside a transform are met by everybody or nobody.  Every pair has both fields
// (the host refuses a null b).
// K's rows, exchanges and inverse transforms around it, NlpParams; no LDS beyond K's own.
template <class K> struct NlzProf {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  // (body forwards: with the text below as `body` itself, one call level fewer to inline, hipcc allocates the registers of one kernel
  // of the library differently -- same counts, other code; scripts/kernel_regs.py --code.  The other endings do not care.)
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { body_prof(p, bid, tid, lds); }
  template <class PP>
  static MFFT_D void body_prof(const PP& P, int bid, int tid, char* lds) {
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
    const int npairs = P.npairs < NLS_PAIRS ? P.npairs : NLS_PAIRS;
#pragma unroll 1
    for (int p = 0; p < npairs; ++p) {
      double acc[E][NLP_STATS];                    // [position j + k TPT][d_a, d_b, d_a^2, d_b^2, d_a d_b]
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int s = 0; s < NLP_STATS; ++s) acc[k][s] = 0.0;
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double ca = p == 0 ? P.center[0] : p == 1 ? P.center[2] : P.center[4];
      const double cb = p == 0 ? P.center[1] : p == 1 ? P.center[3] : P.center[5];
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and add nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          K::template load_pair_rows<true>(v, pa + io, pb + io, j, P.valid_in, P.valid_in, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          if (active) {                            // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) prof_add(acc[k], incr_value((double)v[k].y, P.norm) - ca, incr_value((double)v[k].x, P.norm) - cb);
#pragma unroll
            for (int f = 0; f < 2; ++f)
              if (bad[f] != (T)0) {                // what the load took out of this field: its own sums and the cross sum are NaN
                const double nn = (double)bad[f] * 0.0;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                  acc[k][f] += nn;
                  acc[k][2 + f] += nn;
                  acc[k][4] += nn;
                }
              }
          }
        }
      }
      // row slot bid ROWS + rl < ngroups ROWS, pair p < npairs, position j + k TPT < M: inside (ngroups ROWS, npairs, NLP_STATS, M)
      double* dst = P.part + (((i64)bid * ROWS + rl) * npairs + p) * (NLP_STATS * M) + j;
#pragma unroll
      for (int s = 0; s < NLP_STATS; ++s)
#pragma unroll
        for (int k = 0; k < E; ++k) dst[s * M + k * S::TPT] = acc[k][s];
    }
  }
};

}  // namespace mfft
