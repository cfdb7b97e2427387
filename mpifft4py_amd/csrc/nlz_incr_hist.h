// nlz_incr_hist.h -- the fused z stage that ends in INCREMENT HISTOGRAMS (Op::IncrementHistogram; kernels_nlk*.hip).
#pragma once
#include "nlz_incr.h"
#include "nlz_joint.h"

namespace mfft {

// ... of the kernel that ends in INCREMENT HISTOGRAMS (NlzIncrHist::body below): the counts of the increments along z,
// d = r(z + s) - r(z), of up to six real fields for up to NLI_MAXSEP separations s, in nbins equal bins over a range of its own per
// field and separation.  Pairs as in NlsParams.  The ONE rule (include/mpifft4py_amd.h states it; kernel, sweep, emulator, numpy and
// tests share it): r = incr_value((double)x, norm), d = r(pos + s mod M) - r(pos) in double, slot = hist_slot(d, lo, inv, nbins).  Per
// field and separation nbins + 3 slots, as in NlhParams.
constexpr int NLK_MAXBINS = 256;                                // bins per field and separation (MFFT_INCR_HIST_MAXBINS)
constexpr int NLK_MAXCELLS = 2 * NLI_MAXSEP * (NLK_MAXBINS + 3);      // 4144 counts, 16576 bytes: a pair's histograms in LDS
static_assert(NLK_MAXCELLS <= NLJ_MAXCELLS, "the increment histograms take the joint kernels' exchange rule: they fit under its grid");
template <typename T>
struct NlkParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, 2, nsep, nbins + 3) counts, every slot of the launch's pairs written
  double lo[2 * NLS_PAIRS][NLI_MAXSEP];    // [pair][a, b][separation]: the lower edge of the first bin
  double inv[2 * NLS_PAIRS][NLI_MAXSEP];   // ... and nbins / (hi - lo), formed once on the host
  double norm;                 // r = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int sep[NLI_MAXSEP];         // 1 <= sep[i] <= M - 1, in grid points of the row, i < nsep; duplicates allowed
  int nsep;                    // 1 .. NLI_MAXSEP
  int nbins;                   // 1 .. NLK_MAXBINS
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The count of one increment.  hist_slot clamps the slot to nbins + 2; the cell of (field of the pair, separation, slot) is clamped
// once more to what the kernel reserves, so that no LDS index rests on the caller's nbins, nsep or separations alone.
MFFT_D int incr_hist_cell(int f, int i, int nsep, int nb3, int slot) {
  const int c = (f * nsep + i) * nb3 + slot;
  return c < 0 ? 0 : c > NLK_MAXCELLS - 1 ? NLK_MAXCELLS - 1 : c;
}
MFFT_D int incr_hist_slot(double r1, double r0, double lo, double inv, int nbins) { return hist_slot(r1 - r0, lo, inv, nbins); }

// The stage that ends in INCREMENT HISTOGRAMS: the counts of d = r(z + s) - r(z) over all rows and all M positions of up to six
// real fields, for up to NLI_MAXSEP separations along z, in nbins equal bins of a range per field and separation -- the PDFs of
// the increments of fields that never exist in real space.  The skeleton is NlzIncr::body's: the loop over the PAIRS outermost, the
// real row into the row's own exchange buffer at its natural positions, read back shifted once per separation; with the split
// exchange the two fields of a pair take two rounds; the separation clamped and hidden from the optimiser inside the row loop;
// the syncs where NlzIncr::body has them.  The ending is NlzHist::body's: NO accumulator in a register -- a thread computes a slot
// (incr_hist_slot) and issues an LDS add; the pair's 2 x nsep x (nbins + 3) unsigned counts lie behind the exchange buffers
// (NlzIncrHist::LDS_BYTES reserves NLK_MAXCELLS), cleared once per pair, barrier, all rows of this workgroup, barrier, plain
// stores into the workgroup's row of P.part; the barriers sit where every thread of the workgroup arrives.  nsep, nbins and every
// cell are clamped here (incr_hist_cell): no LDS index rests on the caller's numbers alone.  A thread whose load took a non-finite
// bin out of a field counts ITS E x nsep increments of that field in the non-finite slot; the partner stays exact.  Rows past the
// end re-read the last row and count nothing.  A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M
// increments per field and separation: the host keeps that below 2^32.
// K's rows, exchanges and inverse transforms around it, NlkParams; the histograms of the pair at hand lie behind K's own LDS,
// 16576 bytes where NlzJoint takes 17956.
template <class K> struct NlzIncrHist {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + NLK_MAXCELLS * 4;
  // (body forwards: with the text below as `body` itself, one call level fewer to inline, hipcc allocates the registers of eight kernels
  // of the library differently -- same counts, other code; scripts/kernel_regs.py --code.  The other endings do not care.)
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { body_incr_hist(p, bid, tid, lds); }
  template <class PP>
  static MFFT_D void body_incr_hist(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + K::LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 last = P.nrows - 1;
    const int nsep = P.nsep < 1 ? 1 : P.nsep > NLI_MAXSEP ? NLI_MAXSEP : P.nsep;
    const int nbins = P.nbins < 1 ? 1 : P.nbins > NLK_MAXBINS ? NLK_MAXBINS : P.nbins;
    const int nb3 = nbins + 3;
    const int cells = 2 * nsep * nb3;              // <= NLK_MAXCELLS
    const int npairs = P.npairs < NLS_PAIRS ? P.npairs : NLS_PAIRS;
    // one separation's clamped value, hidden from the optimiser inside the row loop (NlzIncr::body's sep_of: left alone, hipcc hoists
    // the E LDS addresses of every separation out of the loop over the rows)
    auto sep_of = [&](int i) {
      int s = P.sep[i];
      s = s < 1 ? 1 : s > M - 1 ? M - 1 : s;
      MFFT_HIDE_RANGE(s);
      return s;
    };
#pragma unroll 1
    for (int p = 0; p < npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const bool hb = pb != nullptr;
      // the ranges of the two fields of this pair: selects between unconditional loads at constant offsets, as above -- read where
      // they are used, under `i < nsep`, the loads of the three pairs merge into ONE load of a selected address, and the whole
      // argument block goes to scratch for it (968 bytes in every kernel)
      double plo[2][NLI_MAXSEP], piv[2][NLI_MAXSEP];
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int i = 0; i < NLI_MAXSEP; ++i) {
          plo[f][i] = p == 0 ? P.lo[f][i] : p == 1 ? P.lo[2 + f][i] : P.lo[4 + f][i];
          piv[f][i] = p == 0 ? P.inv[f][i] : p == 1 ? P.inv[2 + f][i] : P.inv[4 + f][i];
        }
      for (int c = tid; c < cells; c += THREADS) hist[c] = 0u;
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
          // swapped results: .y = a_p, .x = b_p at position j + k TPT
          if constexpr (SPLIT) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              nlz_sync<WAVE>();
#pragma unroll
              for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = f == 0 ? v[k].y : v[k].x;
              nlz_sync<WAVE>();
              if (active) {
                const bool bf = f == 0 ? ba : bb;
#pragma unroll
                for (int i = 0; i < NLI_MAXSEP; ++i)
                  if (i < nsep) {
                    const int s = sep_of(i);
                    const double lo = plo[f][i], iv = piv[f][i];
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                      const T x1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                      const int sl = bf ? nbins + 2
                                        : incr_hist_slot(incr_value((double)x1, P.norm), incr_value((double)(f == 0 ? v[k].y : v[k].x), P.norm), lo, iv, nbins);
                      MFFT_LDS_COUNT(hist + incr_hist_cell(f, i, nsep, nb3, sl));
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
                  const double loa = plo[0][i], iva = piv[0][i], lob = plo[1][i], ivb = piv[1][i];
#pragma unroll
                  for (int k = 0; k < E; ++k) {
                    const cx<T> z1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                    const int sa = ba ? nbins + 2 : incr_hist_slot(incr_value((double)z1.y, P.norm), incr_value((double)v[k].y, P.norm), loa, iva, nbins);
                    const int sb = bb ? nbins + 2 : incr_hist_slot(incr_value((double)z1.x, P.norm), incr_value((double)v[k].x, P.norm), lob, ivb, nbins);
                    MFFT_LDS_COUNT(hist + incr_hist_cell(0, i, nsep, nb3, sa));
                    MFFT_LDS_COUNT(hist + incr_hist_cell(1, i, nsep, nb3, sb));
                  }
                }
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * npairs + p) * cells;
      for (int c = tid; c < cells; c += THREADS) dst[c] = hist[c];
    }
  }
};

}  // namespace mfft
