// nlz_joint.h -- the fused z stage that ends in JOINT HISTOGRAMS (Op::JointHistogram; kernels_nlj*.hip).
#pragma once
#include "nlz_reduce.h"

namespace mfft {

// ... of the kernel that ends in a JOINT HISTOGRAM (NlzJoint::body below): the two fields of a pair ride one transform, so one
// thread holds both real values of a grid point; it counts the point into ONE cell of a two-dimensional grid.  Per pair
// (nba + 3) x (nbb + 3) cells, cell = sa * (nbb + 3) + sb with sa, sb the fields' slots by hist_slot (joint_cell below: the ONE
// rule of host, sweep, kernel and tests).  Every pair has both fields: a pair without a partner is an error on the host.
constexpr int NLJ_MAXBINS = 64;                                 // bins per field: (64 + 3)^2 cells are what a workgroup's LDS holds
constexpr int NLJ_MAXCELLS = (NLJ_MAXBINS + 3) * (NLJ_MAXBINS + 3);      // 4489 cells, 17956 bytes
template <typename T>
struct NljParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, (nba + 3)(nbb + 3)) counts, every cell of the launch's pairs written
  double lo[2 * NLS_PAIRS];    // [pair][a, b]: the lower edge of the field's first bin
  double inv[2 * NLS_PAIRS];   // ... and nb / (hi - lo) of the field, formed once on the host
  double norm;                 // x = norm * (the un-normalised result of the inverse transform)
  int nba, nbb;                // 1 .. NLJ_MAXBINS each: the bins of the a fields and of the b fields
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The cell of a pair of slots.  hist_slot clamps each slot to its nb + 2; the product is clamped once more to the grid that the
// kernel reserves, so that no LDS index rests on the caller's bin counts alone.
MFFT_D int joint_cell(int sa, int sb, int nbb) {
  const int c = sa * (nbb + 3) + sb;
  return c < 0 ? 0 : c > NLJ_MAXCELLS - 1 ? NLJ_MAXCELLS - 1 : c;
}

// The stage that ends in a JOINT HISTOGRAM: the skeleton of NlzHist::body, but the pairing that NlzHist::body throws away is kept.  After
// run_passes a thread holds .y = a_p and .x = b_p of the SAME grid point; it counts the point into one cell of the pair's grid,
// cell = sa (nbb + 3) + sb (joint_cell), with ONE LDS add where NlzHist::body issues two.  The grid of (nba + 3)(nbb + 3) unsigned
// cells lies behind the exchange buffers (NlzJoint::LDS_BYTES reserves NLJ_MAXCELLS).  The loop over the pairs is outermost:
// clear the grid, barrier, all rows of this workgroup for this pair, barrier, plain stores of the used cells into the workgroup's
// row of P.part; the barriers sit where every thread of the workgroup arrives, so the wave-synchronous builds keep their row loop
// free of them.  A thread clears and stores the cells tid, tid + THREADS, ..: what it clears for the next pair it has stored
// itself.  A non-finite bin met on load marks ITS field's slot only: the partner keeps its exact slot.  Rows past the end re-read
// the last row and count nothing.  A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M points: the host keeps
// that below 2^32.  Every pair has both fields (the host refuses a null b).
// K's rows, exchanges and inverse transforms around it, NljParams; the grid of the pair at hand lies behind K's own LDS, 17956
// bytes where NlzHist takes 4120.
template <class K> struct NlzJoint {
  MFFT_NLZ_NAMES_OF(K);
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + NLJ_MAXCELLS * 4;
  template <class PP>
  static MFFT_D void body(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* grid = reinterpret_cast<unsigned*>(lds + K::LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nba = P.nba < 1 ? 1 : P.nba > NLJ_MAXBINS ? NLJ_MAXBINS : P.nba;
    const int nbb = P.nbb < 1 ? 1 : P.nbb > NLJ_MAXBINS ? NLJ_MAXBINS : P.nbb;
    const int cells = (nba + 3) * (nbb + 3);       // <= NLJ_MAXCELLS
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (int p = 0; p < P.npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double loa = p == 0 ? P.lo[0] : p == 1 ? P.lo[2] : P.lo[4], lob = p == 0 ? P.lo[1] : p == 1 ? P.lo[3] : P.lo[5];
      const double iva = p == 0 ? P.inv[0] : p == 1 ? P.inv[2] : P.inv[4], ivb = p == 0 ? P.inv[1] : p == 1 ? P.inv[3] : P.inv[5];
      for (int i = tid; i < cells; i += THREADS) grid[i] = 0u;
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
          K::template load_pair_rows<true>(v, pa + io, pb + io, j, P.valid_in, P.valid_in, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
          if (active) {                            // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? nba + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, nba);
              const int sb = bb ? nbb + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, nbb);
              MFFT_LDS_COUNT(grid + joint_cell(sa, sb, nbb));
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * P.npairs + p) * cells;
      for (int i = tid; i < cells; i += THREADS) dst[i] = grid[i];
    }
  }
};

}  // namespace mfft
