// incrhist.hip -- PDFs of the increments along z on the device: per field and separation s the nbins + 3 int64 counts of
// d = r(z + s) - r(z) over periodic rows, each (field, separation) over a range of its own (the rule: include/mpifft4py_amd.h;
// nlz_reduce.h incr_value and hist_slot, nlz_incr_hist.h incr_hist_slot).  The streaming sweep mfft_ew_increment_histogram over real rows (the composed
// route of mfft_real_increment_histogram, and the caller's own arrays) and the plan's accumulator; the partial histograms that the
// fused z stage emits (nlz_incr_hist.h NlzIncrHist::body) are rows of nsep (nbins + 3) counts per field and go through the histograms' fold
// (hist.hip hist_fold_slots), as the sweep's do.
// No global atomics anywhere: a workgroup counts in LDS (unsigned), stores its histograms with plain stores, one small launch adds the
// workgroups' rows in a FIXED order into int64.
#include <math.h>
#include "plan_impl.h"
#include "nlz_incr_hist.h"

using namespace mfft;

namespace {

constexpr int KS_BLOCK = 256;
constexpr int KS_CELLS = NLI_MAXSEP * (NLK_MAXBINS + 3);        // one component's histograms in a workgroup's LDS: 8288 bytes
constexpr int KS_ROW_BYTES = 49152;                             // the staged rows of a pass: rows of up to 6144 doubles, 12288 floats
constexpr unsigned KS_MAXGRID = 2048;

struct IncrHistCall {
  double lo[6][NLI_MAXSEP], inv[6][NLI_MAXSEP];    // [component][separation]
  int sep[NLI_MAXSEP];
  int nsep, nbins;
};

// One component per blockIdx.y; a workgroup takes a stripe of rows, blockIdx.x, + gridDim.x, ..: KS_BLOCK / n whole rows per pass
// where rows are short, one row otherwise.  STAGED: the rows of a pass are copied into LDS once (every element is read from memory
// once, coalesced), the value and its nsep shifted partners come from there; rows too long for that are read through the caches.
// A thread knows its row of the pass and its first position from ONE 32-bit division before the loop: nothing is divided per
// element.  Every count goes into the workgroup's LDS histograms; plain stores of them into part[(workgroup, component, cells)].
template <typename T, bool STAGED>
__global__ __launch_bounds__(KS_BLOCK) void incr_hist_kernel(const T* __restrict__ x, int64_t nrows, int n, int64_t pitch, int ncomp,
                                                            const IncrHistCall L, unsigned* __restrict__ part) {
  __shared__ unsigned hist[KS_CELLS];
  extern __shared__ __attribute__((aligned(16))) char staged_rows[];      // STAGED: the rows of a pass, max(n, rows per pass x n) values
  T* rows = reinterpret_cast<T*>(staged_rows);
  const int c = blockIdx.y, t = (int)threadIdx.x;
  const int nsep = L.nsep < 1 ? 1 : L.nsep > NLI_MAXSEP ? NLI_MAXSEP : L.nsep;
  const int nbins = L.nbins < 1 ? 1 : L.nbins > NLK_MAXBINS ? NLK_MAXBINS : L.nbins;
  const int nb3 = nbins + 3, cells = nsep * nb3;
  for (int i = t; i < cells; i += KS_BLOCK) hist[i] = 0u;
  const int rp = n >= KS_BLOCK ? 1 : KS_BLOCK / n;            // rows per pass
  const int lr = rp > 1 ? t / n : 0, z0 = t - lr * n;         // this thread's row of the pass and its first position
  const int step = rp > 1 ? n : KS_BLOCK;                     // (short rows: one position per thread)
  const T* p = x + (size_t)c * (size_t)nrows * (size_t)pitch;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * rp; base < nrows; base += (int64_t)gridDim.x * rp) {      // (the bound is the workgroup's)
    const int64_t row = base + lr;
    const bool active = lr < rp && row < nrows;
    const T* r = p + (size_t)(active ? row : nrows - 1) * (size_t)pitch;
    const T* src = r;
    if constexpr (STAGED) {
      __syncthreads();                               // the reads of the pass before are done
      if (active)
        for (int z = z0; z < n; z += step) rows[lr * n + z] = r[z];
      __syncthreads();
      src = rows + lr * n;
    }
    if (active)
      for (int z = z0; z < n; z += step) {
        const double r0 = incr_value((double)src[z], 1.0);
#pragma unroll
        for (int i = 0; i < NLI_MAXSEP; ++i)
          if (i < nsep) {
            int s = L.sep[i];
            s = s < 1 ? 1 : s > n - 1 ? n - 1 : s;
            const double r1 = incr_value((double)src[incr_pos(z, s, n)], 1.0);
            const int cell = i * nb3 + incr_hist_slot(r1, r0, L.lo[c][i], L.inv[c][i], nbins);
            MFFT_LDS_COUNT(hist + (cell < 0 ? 0 : cell > KS_CELLS - 1 ? KS_CELLS - 1 : cell));
          }
      }
  }
  __syncthreads();
  unsigned* dst = part + ((size_t)blockIdx.x * ncomp + c) * (size_t)cells;
  for (int i = t; i < cells; i += KS_BLOCK) dst[i] = hist[i];
}

}  // namespace

namespace mfft {

static_assert(NLK_MAXBINS == MFFT_INCR_HIST_MAXBINS, "the public header states the kernels' limit");

size_t incr_hist_part_bytes(int ngroups, int nslots, int nsep, int nbins) {
  return (size_t)ngroups * (size_t)nslots * (size_t)nsep * (size_t)(nbins + 3) * sizeof(unsigned);
}

int incr_hist_range(double lo, double hi, int nbins, double* inv) {
  if (nbins < 1 || nbins > NLK_MAXBINS) return set_error(MFFT_ERR_INVALID, "nbins must be 1 .. %d, not %d", NLK_MAXBINS, nbins);
  if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g): lo < hi, both finite", lo, hi);
  const double v = (double)nbins / (hi - lo);
  if (!isfinite(v) || !(v > 0.0)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g) is too narrow or too wide", lo, hi);
  *inv = v;
  return 0;
}

}  // namespace mfft

// acc[(c * nsep + i) * (nbins + 3) + slot] += the counts of component c of x (ncomp x nrows rows of n elements, pitch apart), c < ncomp
// <= 6, at the plan's separations, with the ranges of the slots slot0 + c (incr_hist_begin), on the plan's stream
int mfft_plan_s::incr_hist_sweep(const void* x, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int slot0, int64_t* acc) {
  const NlrCall& q = nlcall;
  IncrHistCall L;
  for (int c = 0; c < 6; ++c)
    for (int i = 0; i < NLI_MAXSEP; ++i) {
      const bool used = c < ncomp && slot0 + c < 6 && i < q.nsep;
      L.lo[c][i] = used ? q.ilo[slot0 + c][i] : 0.0;
      L.inv[c][i] = used ? q.iinv[slot0 + c][i] : 1.0;
    }
  for (int i = 0; i < NLI_MAXSEP; ++i) L.sep[i] = i < q.nsep ? q.sep[i] : 1;
  L.nsep = q.nsep;
  L.nbins = q.nbins;
  const int cells = q.nsep * (q.nbins + 3);
  const int rp = n >= KS_BLOCK ? 1 : (int)(KS_BLOCK / n);
  const bool staged = (size_t)n * rs <= (size_t)KS_ROW_BYTES;
  const size_t lds = staged ? (size_t)rp * (size_t)n * rs : 0;      // (rp x n <= KS_BLOCK values where rp > 1)
  // a workgroup's share of one launch stays below 2^32 increments per separation: passes x rows per pass x n
  const int64_t wg_rows = (((int64_t)1 << 32) - 1) / n / rp * rp;
  for (int64_t r0 = 0; r0 < nrows;) {
    const int64_t passes = (nrows - r0 + rp - 1) / rp;
    const unsigned grid = (unsigned)std::min<int64_t>(passes, KS_MAXGRID);
    const int64_t len = std::min(nrows - r0, (int64_t)grid * wg_rows);
    MFFT_TRY(ensure(nlm, incr_hist_part_bytes((int)grid, ncomp, q.nsep, q.nbins)));
    unsigned* part = static_cast<unsigned*>(nlm.p);
    // (the components of the caller's array are nrows * pitch apart: a launch over some of the rows is a launch per component)
    for (int c = 0; c < (len == nrows ? 1 : ncomp); ++c) {
      const int nc = len == nrows ? ncomp : 1;
      IncrHistCall Lc = L;
      if (nc == 1 && c > 0)
        for (int i = 0; i < NLI_MAXSEP; ++i) { Lc.lo[0][i] = L.lo[c][i]; Lc.inv[0][i] = L.inv[c][i]; }
      const size_t off = ((size_t)c * (size_t)nrows + (size_t)r0) * (size_t)pitch;
      const dim3 g(grid, nc), b(KS_BLOCK);
      if (prec == MFFT_DOUBLE) {
        const double* px = static_cast<const double*>(x) + off;
        if (staged) hipLaunchKernelGGL((incr_hist_kernel<double, true>), g, b, lds, stream, px, len, (int)n, pitch, nc, Lc, part);
        else hipLaunchKernelGGL((incr_hist_kernel<double, false>), g, b, lds, stream, px, len, (int)n, pitch, nc, Lc, part);
      } else {
        const float* px = static_cast<const float*>(x) + off;
        if (staged) hipLaunchKernelGGL((incr_hist_kernel<float, true>), g, b, lds, stream, px, len, (int)n, pitch, nc, Lc, part);
        else hipLaunchKernelGGL((incr_hist_kernel<float, false>), g, b, lds, stream, px, len, (int)n, pitch, nc, Lc, part);
      }
      MFFT_HIP(hipGetLastError());
      MFFT_TRY(hist_fold_slots(part, grid, nc, cells, acc + (size_t)c * cells, stream));
    }
    r0 += len;
  }
  return 0;
}

// the plan's accumulator of an increment-histogram call: nlkacc = 6 x MFFT_INCR_MAXSEP x (MFFT_INCR_HIST_MAXBINS + 3) int64 in slot
// order, rows nsep (nbins + 3) apart, cleared on the stream; the call's separations (checked by the caller: incr_check), bin count
// and ranges in slot order
int mfft_plan_s::incr_hist_begin(const int64_t* seps, int nsep, const double (*lo_slots)[MFFT_INCR_MAXSEP], const double (*inv_slots)[MFFT_INCR_MAXSEP],
                                 int nbins) {
  const size_t bytes = (size_t)6 * NLI_MAXSEP * (NLK_MAXBINS + 3) * sizeof(int64_t);
  MFFT_TRY(ensure(nlkacc, bytes));
  MFFT_HIP(hipMemsetAsync(nlkacc.p, 0, bytes, stream));
  for (int i = 0; i < NLI_MAXSEP; ++i) nlcall.sep[i] = i < nsep ? (int)seps[i] : 1;
  nlcall.nsep = nsep;
  nlcall.nbins = nbins;
  for (int f = 0; f < 6; ++f)
    for (int i = 0; i < NLI_MAXSEP; ++i) { nlcall.ilo[f][i] = lo_slots[f][i]; nlcall.iinv[f][i] = inv_slots[f][i]; }
  return 0;
}
int mfft_plan_s::incr_hist_end(int64_t* host, int nslots) {
  MFFT_HIP(hipMemcpyAsync(host, nlkacc.p, (size_t)nslots * nlcall.nsep * (nlcall.nbins + 3) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[(c * nsep + i) * (nbins + 3) + slot]: see include/mpifft4py_amd.h.  Synchronises the plan's stream.
int mfft_ew_increment_histogram(mfft_plan_t plan, const void* x, int ncomp, int64_t nrows, int64_t n, int64_t row_pitch, int precision,
                                const int64_t* seps, int nsep, const double* lo, const double* hi, int nbins, int64_t* out_host) {
  if (!plan || !x || !out_host || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (nrows < 1 || n < 2 || n >= ((int64_t)1 << 30) || row_pitch < n) return set_error(MFFT_ERR_INVALID, "bad rows: %lld of %lld elements, pitch %lld", (long long)nrows, (long long)n, (long long)row_pitch);
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  MFFT_TRY(incr_check(seps, nsep, n));
  double l6[6][MFFT_INCR_MAXSEP] = {}, i6[6][MFFT_INCR_MAXSEP] = {};
  for (int c = 0; c < ncomp; ++c)
    for (int i = 0; i < nsep; ++i) {
      MFFT_TRY(incr_hist_range(lo[c * nsep + i], hi[c * nsep + i], nbins, &i6[c][i]));
      l6[c][i] = lo[c * nsep + i];
    }
  MFFT_TRY(plan->incr_hist_begin(seps, nsep, l6, i6, nbins));
  MFFT_TRY(plan->incr_hist_sweep(x, ncomp, nrows, n, row_pitch, 0, static_cast<int64_t*>(plan->nlkacc.p)));
  return plan->incr_hist_end(out_host, ncomp);
}

}  // extern "C"
