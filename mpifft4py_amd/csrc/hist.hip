// hist.hip -- histograms on the device: per field nbins + 3 int64 counts, [0] below lo, [1 .. nbins] the equal bins of [lo, hi),
// [nbins + 1] at or above hi, [nbins + 2] not finite (nlz_reduce.h hist_slot: the one rule of host, sweep, fused kernel and tests).
// The fold of the partial histograms that the fused z stage emits (nlz_hist.h NlzHist::body) and the streaming sweep mfft_ew_histogram
// over real fields (the composed route of mfft_real_histogram, and the caller's own arrays), the companion of mfft_ew_moments.
// No global atomics anywhere: a workgroup counts in LDS (unsigned), stores its histogram with plain stores, one small launch adds
// the workgroups' rows in a FIXED order into int64.  Counts are integers, so the order would not matter anyway: the result is
// the same bits run to run, device to device and for every number of ranks.
#include <math.h>
#include "plan_impl.h"
#include "nlz_hist.h"

using namespace mfft;

namespace {

constexpr int HS_BLOCK = 256;
constexpr int HF_BLOCK = 256;
constexpr int NB3_MAX = NLH_MAXBINS + 3;
static_assert(NLH_MAXBINS == MFFT_HIST_MAXBINS, "the public header states the kernels' limit");
constexpr size_t HS_CHUNK = (size_t)1 << 40;      // elements per component of one sweep launch: 2^40 / 1024 workgroups < 2^32 each

// acc[f][s] += sum_g part[g][f][s] for the HF_SLOTS slots of field blockIdx.y that the workgroup holds: consecutive threads on
// consecutive counts (128-byte segments), HF_LANES threads per slot that take the groups gy, gy + HF_LANES, .. in that order --
// a launch of a thousand workgroups is a thousand rows, which ONE thread per slot read one after the other in 0.2 - 0.4 ms
// (profiles/real_histogram_ab.txt, first take) --, then the first of them adds the HF_LANES partial sums in order, and the accumulator.
constexpr int HF_SLOTS = 32, HF_LANES = HF_BLOCK / HF_SLOTS;
__global__ __launch_bounds__(HF_BLOCK) void hist_fold_kernel(const unsigned* __restrict__ part, size_t groups, int nfields, int nb3,
                                                            int64_t* __restrict__ acc) {
  __shared__ int64_t red[HF_LANES][HF_SLOTS];
  const int sx = (int)threadIdx.x % HF_SLOTS, gy = (int)threadIdx.x / HF_SLOTS;
  const int s = (int)blockIdx.x * HF_SLOTS + sx, f = (int)blockIdx.y;
  int64_t sum = 0;
  if (s < nb3)
    for (size_t g = gy; g < groups; g += HF_LANES) sum += (int64_t)part[(g * (size_t)nfields + f) * (size_t)nb3 + s];
  red[gy][sx] = sum;
  __syncthreads();
  if (gy == 0 && s < nb3) {
    int64_t t = 0;
    for (int w = 0; w < HF_LANES; ++w) t += red[w][sx];
    acc[(size_t)f * nb3 + s] += t;
  }
}

struct HistRange { double lo[6], inv[6]; };

// One component of a real field per blockIdx.y: 16 bytes per lane, the workgroup's histogram in LDS, plain stores of it into
// part[(workgroup, component, nbins + 3)].  A component need not start on 16 bytes (single precision, odd n): the elements before
// the first aligned one and after the last whole vector are taken singly by the first lanes, as absmax.hip and moments.hip do.
template <typename T>
__global__ __launch_bounds__(HS_BLOCK) void hist_kernel(const T* __restrict__ x, size_t stride, size_t n, int ncomp, const HistRange r, int nbins,
                                                       unsigned* __restrict__ part) {
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) V { T v[VEC]; };
  __shared__ unsigned hist[NB3_MAX];
  const int c = blockIdx.y, nb3 = nbins + 3;
  for (int i = threadIdx.x; i < nb3; i += HS_BLOCK) hist[i] = 0u;
  __syncthreads();
  const T* p = x + (size_t)c * stride;
  const double lo = r.lo[c], inv = r.inv[c];
  const size_t mis = ((uintptr_t)p % 16) / sizeof(T);
  size_t head = mis ? VEC - mis : 0;
  if (head > n) head = n;
  const size_t nv = (n - head) / VEC, tail0 = head + nv * VEC;
  const V* pv = reinterpret_cast<const V*>(p + head);
  const size_t gtid = (size_t)blockIdx.x * HS_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * HS_BLOCK;
  for (size_t i = gtid; i < nv; i += gsize) {
    const V q = pv[i];
#pragma unroll
    for (int k = 0; k < VEC; ++k) MFFT_LDS_COUNT(hist + hist_slot((double)q.v[k], lo, inv, nbins));
  }
  if (gtid < head) MFFT_LDS_COUNT(hist + hist_slot((double)p[gtid], lo, inv, nbins));
  if (tail0 + gtid < n) MFFT_LDS_COUNT(hist + hist_slot((double)p[tail0 + gtid], lo, inv, nbins));      // fewer than VEC <= HS_BLOCK of them
  __syncthreads();
  unsigned* dst = part + ((size_t)blockIdx.x * ncomp + c) * (size_t)nb3;
  for (int i = threadIdx.x; i < nb3; i += HS_BLOCK) dst[i] = hist[i];
}

// workgroups of a hist_kernel launch over n elements per component
unsigned hist_grid(size_t n, int prec) {
  const size_t vec = prec == MFFT_DOUBLE ? 2 : 4;
  size_t g = (n / vec + (size_t)HS_BLOCK * 8 - 1) / ((size_t)HS_BLOCK * 8);      // some eight vectors per lane
  return (unsigned)(g > 1024 ? 1024 : (g ? g : 1));
}

}  // namespace

namespace mfft {

int hist_max_bins() { return NLH_MAXBINS; }

int hist_range(double lo, double hi, int nbins, double* inv) {
  if (nbins < 1 || nbins > NLH_MAXBINS) return set_error(MFFT_ERR_INVALID, "nbins must be 1 .. %d, not %d", NLH_MAXBINS, nbins);
  if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g): lo < hi, both finite", lo, hi);
  const double v = (double)nbins / (hi - lo);
  if (!isfinite(v) || !(v > 0.0)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g) is too narrow or too wide", lo, hi);
  *inv = v;
  return 0;
}

int hist_fold(const unsigned* part, size_t groups, int nfields, int nbins, int64_t* acc, hipStream_t s) {
  if (nfields < 1 || nfields > 6 || nbins < 1 || nbins > NLH_MAXBINS) return set_error(MFFT_ERR_INTERNAL, "hist_fold: %d fields, %d bins", nfields, nbins);
  return hist_fold_slots(part, groups, nfields, nbins + 3, acc, s);
}

// the same fold for rows of any length (the joint histograms' grids, joint.hip): acc[f][s] += sum over the groups g, in fixed
// order, of part[(g * nfields + f) * nslots + s]
int hist_fold_slots(const unsigned* part, size_t groups, int nfields, int nslots, int64_t* acc, hipStream_t s) {
  if (nfields < 1 || nfields > 65535 || nslots < 1) return set_error(MFFT_ERR_INTERNAL, "hist_fold_slots: %d fields, %d slots", nfields, nslots);
  if (groups == 0) return 0;
  hipLaunchKernelGGL(hist_fold_kernel, dim3((nslots + HF_SLOTS - 1) / HF_SLOTS, nfields), dim3(HF_BLOCK), 0, s, part, groups, nfields, nslots, acc);
  MFFT_HIP(hipGetLastError());
  return 0;
}

size_t hist_part_bytes(int ngroups, int nslots, int nbins) { return (size_t)ngroups * (size_t)nslots * (size_t)(nbins + 3) * sizeof(unsigned); }

}  // namespace mfft

// acc[c][s] += counts of x[c, :], c < ncomp <= 6, on the plan's stream (acc: device int64 of the plan, rows nbins + 3 apart)
int mfft_plan_s::hist_sweep(const void* x, int ncomp, size_t n, const double* lo, const double* inv, int nbins, int64_t* acc) {
  HistRange r;
  for (int c = 0; c < 6; ++c) { r.lo[c] = c < ncomp ? lo[c] : 0.0; r.inv[c] = c < ncomp ? inv[c] : 1.0; }
  for (size_t o = 0; o < n; o += HS_CHUNK) {       // (a workgroup's share of a launch stays below 2^32 elements)
    const size_t len = std::min(HS_CHUNK, n - o);
    const unsigned grid = hist_grid(len, prec);
    MFFT_TRY(ensure(nlm, hist_part_bytes((int)grid, ncomp, nbins)));
    unsigned* part = static_cast<unsigned*>(nlm.p);
    if (prec == MFFT_DOUBLE)
      hipLaunchKernelGGL(hist_kernel<double>, dim3(grid, ncomp), dim3(HS_BLOCK), 0, stream, static_cast<const double*>(x) + o, n, len, ncomp, r, nbins, part);
    else
      hipLaunchKernelGGL(hist_kernel<float>, dim3(grid, ncomp), dim3(HS_BLOCK), 0, stream, static_cast<const float*>(x) + o, n, len, ncomp, r, nbins, part);
    MFFT_HIP(hipGetLastError());
    MFFT_TRY(hist_fold(part, grid, ncomp, nbins, acc, stream));
  }
  return 0;
}

// the plan's accumulator of a histogram call: nlhacc = 6 x (NLH_MAXBINS + 3) int64, cleared on the stream; the ranges in slot order
int mfft_plan_s::hist_begin(const double lo_slots[6], const double inv_slots[6], int nbins) {
  MFFT_TRY(ensure(nlhacc, (size_t)6 * NB3_MAX * sizeof(int64_t)));
  MFFT_HIP(hipMemsetAsync(nlhacc.p, 0, (size_t)6 * NB3_MAX * sizeof(int64_t), stream));
  for (int i = 0; i < 6; ++i) { nlcall.lo[i] = lo_slots[i]; nlcall.inv[i] = inv_slots[i]; }
  nlcall.nbins = nbins;
  return 0;
}
int mfft_plan_s::hist_end(int64_t* host, int nslots) {
  MFFT_HIP(hipMemcpyAsync(host, nlhacc.p, (size_t)nslots * (nlcall.nbins + 3) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[c * (nbins + 3) + slot] of a real device array (ncomp, n), c < ncomp.  Synchronises the plan's stream.
int mfft_ew_histogram(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* lo, const double* hi, int nbins,
                      int64_t* out_host) {
  if (!plan || !x || !out_host || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (n < 1) return set_error(MFFT_ERR_INVALID, "empty array");
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  double l6[6] = {0, 0, 0, 0, 0, 0}, i6[6] = {1, 1, 1, 1, 1, 1};
  for (int c = 0; c < ncomp; ++c) {
    MFFT_TRY(hist_range(lo[c], hi[c], nbins, &i6[c]));
    l6[c] = lo[c];
  }
  MFFT_TRY(plan->hist_begin(l6, i6, nbins));
  MFFT_TRY(plan->hist_sweep(x, ncomp, n, l6, i6, nbins, static_cast<int64_t*>(plan->nlhacc.p)));
  return plan->hist_end(out_host, ncomp);
}

}  // extern "C"
