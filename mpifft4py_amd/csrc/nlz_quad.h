// nlz_quad.h -- the fused z stage that ends in the statistics of a QUADRATIC FORM (Op::Quadratic; kernels_nlq*.hip).
#pragma once
#include "nlz_moments.h"
#include "nlz_hist.h"

namespace mfft {

// ... of the kernel that ends in the statistics of a QUADRATIC FORM of its fields (NlzQuad::body below): q = sum_f w_f r_f^2 over
// up to six real fields r_f -- enstrophy, dissipation, energy density -- reduced to [min, max, S1 .. S4] about `center` and, with
// nbins > 0, counted in nbins equal bins of [lo, hi) (hist_slot).  Pairs as in NlsParams; w in slot order, [pair][a, b].
template <typename T>
struct NlqParams : NlzParams<T> {
  double* mpart;               // (waves of the launch, NLS_STATS) partial statistics of q, every slot written
  unsigned* hpart;             // (workgroups of the launch, nbins + 3) counts of q, every slot written (zeros where nbins == 0)
  double w[2 * NLS_PAIRS];     // [pair][a, b]: the weight of the field's square; 0 where the pair has no partner
  double center;               // S_p = sum (q - center)^p
  double norm;                 // r = norm * (the un-normalised result of the inverse transform)
  double lo, inv;              // the lower edge of the first bin and nbins / (hi - lo), formed once on the host
  int nbins;                   // 0 .. NLH_MAXBINS; 0: no histogram
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// q + (w r) r: one field's term
MFFT_D double quad_term(double q, double w, double r) { return quad_add(q, quad_mul(quad_mul(w, r), r)); }

// The stage that ends in the statistics of a QUADRATIC FORM: q = sum_f w_f r_f^2 of up to six real fields at every position of
// every row -- enstrophy density, dissipation, energy density -- reduced to [min, max, S1 .. S4] and, with nbins > 0, counted in
// nbins equal bins: the statistics of a combination of fields none of which exists in real space.  The accumulation of body_dot
// (a running sum in registers across the inverse transforms of a row) under the ending of NlzMoments::body and NlzHist::body, on the
// skeleton of NlzMoments::body: a workgroup strides over the pairs of rows, ONE transform is inlined in a loop over the pairs that is
// not unrolled, non-finite bins leave the transform on load.  After each transform the pair's two fields go into q[E] by the one
// rule (quad_term: q = q + (w r) r, slot order, every operation rounded on its own); after the last pair of an active row q goes
// into ONE set of six accumulators and ONE LDS histogram of nbins + 3 counts behind the exchange buffers.  State across a
// transform: E doubles of q and 6 accumulators, where NlzMoments::body holds 36.  A partner that is not there reads as zeros and has
// weight 0: its term is +-0 and changes no q.  A thread whose load took a non-finite bin out of ANY field has a NaN q in that
// row.  The histogram is cleared once before the row loop and stored once after it, the barriers where NlzHist::body has them (the
// first also covers the twiddles); nbins is uniform over the launch; the wave-synchronous builds keep their row loop free of
// workgroup barriers.  Rows past the end re-read the last row and count nothing.  Plain stores of every slot of the launch's
// mpart and hpart; the folds of moments.hip and hist.hip add them in fixed order: bitwise reproducible.
// K's rows, exchanges and inverse transforms around it, NlqParams; ONE histogram lies behind K's own LDS, 2060 bytes where NlzHist
// takes 4120.
template <class K> struct NlzQuad {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + (NLH_MAXBINS + 3) * 4;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLS_STATS doubles in NlqParams::mpart per workgroup
  template <class PP>
  static MFFT_D void body(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + K::LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nb3 = P.nbins + 3;
    double acc[NLS_STATS];
    moments_clear(acc);
    for (int i = tid; i < nb3; i += THREADS) hist[i] = 0u;
    MFFT_BARRIER();
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
      const i64 unit = base + rl;                  // a pair of rows
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const i64 row = 2 * unit + h;
        const bool active = row < P.nrows;         // rows past the end re-read the last row and count nothing
        const i64 io = (active ? row : last) * P.in_stride;
        double q[E];
#pragma unroll
        for (int k = 0; k < E; ++k) q[k] = 0.0;
        bool anybad = false;
#pragma unroll 1
        for (int p = 0; p < P.npairs; ++p) {
          cx<T> v[E];
          T bad[2];
          const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
          const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
          const double wa = p == 0 ? P.w[0] : p == 1 ? P.w[2] : P.w[4], wb = p == 0 ? P.w[1] : p == 1 ? P.w[3] : P.w[5];
          const bool hb = pb != nullptr;
          K::template load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
#pragma unroll
          for (int k = 0; k < E; ++k) {            // swapped results: .y = a_p, .x = b_p at position j + k TPT; slot 2 p, then 2 p + 1
            q[k] = quad_term(q[k], wa, quad_mul((double)v[k].y, P.norm));
            q[k] = quad_term(q[k], wb, quad_mul((double)v[k].x, P.norm));
          }
          anybad = anybad || bad[0] != (T)0 || bad[1] != (T)0;
        }
        if (active) {
#pragma unroll
          for (int k = 0; k < E; ++k) {
            const double x = anybad ? __builtin_nan("") : q[k];
            moments_add(acc, x, P.center);
            if (P.nbins > 0) MFFT_LDS_COUNT(hist + hist_slot(x, P.lo, P.inv, P.nbins));
          }
        }
      }
    }
    MFFT_BARRIER();
    unsigned* dst = P.hpart + (i64)bid * nb3;
    for (int i = tid; i < nb3; i += THREADS) dst[i] = hist[i];
    constexpr int NW = (THREADS + 63) / 64;
    wave_moments_store<THREADS>(acc, tid, P.mpart + ((i64)bid * NW + tid / 64) * NLS_STATS);
  }
};

}  // namespace mfft
