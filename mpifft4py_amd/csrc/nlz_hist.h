// nlz_hist.h -- the fused z stage that ends in HISTOGRAMS (Op::Histogram; kernels_nlh*.hip).
#pragma once
#include "nlz_reduce.h"

namespace mfft {

// ... of the kernel that ends in a HISTOGRAM (NlzHist::body below): counts of the values of up to six real fields in nbins
// equal bins over [lo, hi) of each field.  Pairs as in NlsParams.  Per field nbins + 3 slots: [0] below lo, [1 .. nbins] the bins,
// [nbins + 1] at or above hi, [nbins + 2] not finite (nlz_reduce.h hist_slot: the ONE rule of host, sweep, kernel and tests).
constexpr int NLH_MAXBINS = 512;                                // bins per field a workgroup's LDS histograms hold
template <typename T>
struct NlhParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, 2, nbins + 3) counts, every slot of the launch's pairs written
  double lo[2 * NLS_PAIRS];    // [pair][a, b]: the lower edge of the field's first bin
  double inv[2 * NLS_PAIRS];   // ... and nbins / (hi - lo), formed once on the host
  double norm;                 // x = norm * (the un-normalised result of the inverse transform)
  int nbins;                   // 1 .. NLH_MAXBINS
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The same with runs of equal slot merged inside the wave first (NlzHist MERGE; the build that was measured against the plain add,
// profiles/real_histogram_ab.txt): neighbouring lanes hold neighbouring z positions, a smooth field puts whole runs of them into
// one slot and the LDS serialises those adds.  Every lane contributes ONE, so a run's sum is its length: the head of a run (its
// slot differs from the lane's before it) adds the distance to the next head -- one shuffle and one ballot, no reduction tree, the
// head-and-ballot scheme of shells.hip.  EVERY lane of the wave calls it (s < 0: the lane counts nothing and breaks a run).
#if defined(__HIPCC__)
MFFT_D void lds_count_runs(unsigned* hist, int s, int lane) {
  const int sprev = __shfl_up(s, 1, 64);
  const unsigned long long live = __ballot(1), heads = __ballot(lane == 0 || s != sprev);
  const unsigned long long above = heads & ~((2ull << lane) - 1ull);
  const int end = above ? __builtin_ctzll(above) : __builtin_popcountll(live);      // (a workgroup's last wave may be short)
  if (((heads >> lane) & 1ull) && s >= 0) (void)atomicAdd(hist + s, (unsigned)(end - lane));
}
#else
MFFT_D void lds_count_runs(unsigned* hist, int s, int lane) {
  if (s >= 0) hist[s] += 1u;
}
#endif

// The stage that ends in a HISTOGRAM: the counts of the values of up to six real fields in nbins equal bins per field -- the PDF
// of a field that never exists in real space.  The skeleton is NlzMoments::body's: a workgroup strides over the pairs of rows, pairs of
// fields ride on one inverse transform, ONE transform is inlined, non-finite bins leave the transform on load.  What differs is
// where the state lives: two histograms of nbins + 3 unsigned counts in LDS behind the exchange buffers (NlzHist::LDS_BYTES), no
// accumulator in a register.  So the loop over the PAIRS is the outer one: clear the two histograms, barrier, all rows of this
// workgroup for this pair -- every value to its slot (hist_slot) with an LDS add --, barrier, plain stores of the two histograms
// into the workgroup's row of P.part.  Every (row, pair) is still loaded once; the barriers sit where every thread of the
// workgroup arrives (the bound of the row loop is the workgroup's), so the wave-synchronous builds keep their row loop free of
// them.  A thread clears and stores the slots tid, tid + THREADS, ..: what it clears for the next pair it has stored itself.
// Counts are integers: whatever order the adds land in, the result is the same bits.  A thread whose load took a non-finite
// bin out of a field counts ITS values of that field in the non-finite slot (the row is NaN there); the partner stays exact.
// A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M values per field: the host keeps that below 2^32.
// MERGE: runs of equal slot inside the wave are merged before the add (lds_count_runs); every lane of the wave takes part, a lane
// of a row past the end with slot -1.
// K's rows, exchanges and inverse transforms around it, NlhParams; the two histograms of the pair at hand lie behind K's own LDS.
template <class K, bool MERGE = false> struct NlzHist {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + 2 * (NLH_MAXBINS + 3) * 4;
  template <class PP>
  static MFFT_D void body(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + K::LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nb3 = P.nbins + 3;
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (int p = 0; p < P.npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double loa = p == 0 ? P.lo[0] : p == 1 ? P.lo[2] : P.lo[4], lob = p == 0 ? P.lo[1] : p == 1 ? P.lo[3] : P.lo[5];
      const double iva = p == 0 ? P.inv[0] : p == 1 ? P.inv[2] : P.inv[4], ivb = p == 0 ? P.inv[1] : p == 1 ? P.inv[3] : P.inv[5];
      const bool hb = pb != nullptr;
      for (int i = tid; i < 2 * nb3; i += THREADS) hist[i] = 0u;
      MFFT_BARRIER();
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and count nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          K::template load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
          if constexpr (MERGE) {
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? P.nbins + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, P.nbins);
              const int sb = bb ? P.nbins + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, P.nbins);
              lds_count_runs(hist, active ? sa : -1, tid & 63);
              lds_count_runs(hist + nb3, active ? sb : -1, tid & 63);
            }
          } else if (active) {                     // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? P.nbins + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, P.nbins);
              const int sb = bb ? P.nbins + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, P.nbins);
              MFFT_LDS_COUNT(hist + sa);
              MFFT_LDS_COUNT(hist + nb3 + sb);
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * P.npairs + p) * (2 * nb3);
      for (int i = tid; i < 2 * nb3; i += THREADS) dst[i] = hist[i];
    }
  }
};

}  // namespace mfft
