// moments.hip -- one-point statistics on the device: per field [min, max, S1, S2, S3, S4], S_p = sum (x - c)^p.  The fold of the
// partial statistics that the fused z stage emits (nlz_moments.h NlzMoments::body) and the streaming sweep mfft_ew_moments over real
// fields (the composed route of mfft_real_moments, and the caller's own arrays), the companion of mfft_ew_absmax.
// No global atomics anywhere: waves store their partials with plain stores, one small launch adds them in a FIXED order, so the
// sums are bitwise reproducible run to run.  Powers and sums in double whatever the precision of the data.
// NaN contract: a NaN in the data is a NaN in all six statistics of its field (nan_min / nan_max keep it), Inf gives +-Inf extremes
// and NaN or Inf sums.
#include <math.h>
#include "plan_impl.h"
#include "nlz_moments.h"

using namespace mfft;

namespace {

constexpr int MF_BLOCK = 576;           // a multiple of every count of values (6, 12, 18, 36): a thread meets ONE value
constexpr int MS_BLOCK = 256;

__device__ __forceinline__ double merge_one(int stat, double m, double x) {
  return stat == 0 ? nan_min(m, x) : stat == 1 ? nan_max(m, x) : m + x;
}

__global__ void moments_clear_kernel(double* acc, int nvals) {
  const int v = (int)threadIdx.x;
  if (v < nvals) acc[v] = v % NLS_STATS == 0 ? __builtin_inf() : v % NLS_STATS == 1 ? -__builtin_inf() : 0.0;
}

// One workgroup reads the groups' slots as they lie in memory -- consecutive threads, consecutive doubles: whole slots, coalesced.
// Thread t holds value v = t % nvals and takes the groups t / nvals, + MF_BLOCK / nvals, .. in that order; the first nvals threads
// then add the MF_BLOCK / nvals rows of the workgroup in order, and the accumulator.
__global__ __launch_bounds__(MF_BLOCK) void moments_fold_kernel(const double* __restrict__ part, size_t groups, int nvals, double* acc) {
  __shared__ double red[MF_BLOCK];
  const int t = (int)threadIdx.x, stat = (t % nvals) % NLS_STATS, rows = MF_BLOCK / nvals;
  double m = stat == 0 ? __builtin_inf() : stat == 1 ? -__builtin_inf() : 0.0;
  for (size_t i = t; i < groups * (size_t)nvals; i += MF_BLOCK) m = merge_one(stat, m, part[i]);      // (MF_BLOCK % nvals == 0: i % nvals stays)
  red[t] = m;
  __syncthreads();
  if (t < nvals) {
    for (int r = 1; r < rows; ++r) m = merge_one(stat, m, red[r * nvals + t]);
    acc[t] = merge_one(stat, acc[t], m);
  }
}

// One component of a real field per blockIdx.y: 16 bytes per lane, six doubles of accumulators per lane, one wave reduction at
// the end (nlz_moments.h wave_moments_store), one plain store of six doubles per wave into part[(wave of the launch) * ncomp + component].
// A component need not start on 16 bytes (single precision, odd n): the elements before the first aligned one and after the last
// whole vector are taken singly by the first lanes, as absmax.hip does.
template <typename T>
__global__ __launch_bounds__(MS_BLOCK) void moments_kernel(const T* __restrict__ x, size_t n, int ncomp, const double* __restrict__ center,
                                                          double* __restrict__ part) {
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) V { T v[VEC]; };
  const int c = blockIdx.y;
  const T* p = x + (size_t)c * n;
  const double ctr = center[c];
  const size_t mis = ((uintptr_t)p % 16) / sizeof(T);
  size_t head = mis ? VEC - mis : 0;
  if (head > n) head = n;
  const size_t nv = (n - head) / VEC, tail0 = head + nv * VEC;
  const V* pv = reinterpret_cast<const V*>(p + head);
  const size_t gtid = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * MS_BLOCK;
  double m[NLS_STATS];
  moments_clear(m);
  for (size_t i = gtid; i < nv; i += gsize) {
    const V q = pv[i];
#pragma unroll
    for (int k = 0; k < VEC; ++k) moments_add(m, (double)q.v[k], ctr);
  }
  if (gtid < head) moments_add(m, (double)p[gtid], ctr);
  if (tail0 + gtid < n) moments_add(m, (double)p[tail0 + gtid], ctr);      // fewer than VEC <= MS_BLOCK of them
  wave_moments_store<MS_BLOCK>(m, (int)threadIdx.x, part + ((gtid >> 6) * (size_t)ncomp + c) * NLS_STATS);
}

// workgroups of a moments_kernel launch over n elements per component
unsigned moments_grid(size_t n, int prec) {
  const size_t vec = prec == MFFT_DOUBLE ? 2 : 4;
  size_t g = (n / vec + (size_t)MS_BLOCK * 8 - 1) / ((size_t)MS_BLOCK * 8);      // some eight vectors per lane
  return (unsigned)(g > 1024 ? 1024 : (g ? g : 1));
}

}  // namespace

namespace mfft {

int moments_clear(double* acc, int nvals, hipStream_t s) {
  if (nvals < 1 || nvals > 64) return set_error(MFFT_ERR_INTERNAL, "moments_clear: %d values", nvals);
  hipLaunchKernelGGL(moments_clear_kernel, dim3(1), dim3(64), 0, s, acc, nvals);
  MFFT_HIP(hipGetLastError());
  return 0;
}

int moments_fold(const double* part, size_t groups, int nvals, double* acc, hipStream_t s) {
  if (nvals < 1 || nvals % NLS_STATS != 0 || MF_BLOCK % nvals != 0) return set_error(MFFT_ERR_INTERNAL, "moments_fold: %d values", nvals);
  if (groups == 0) return 0;
  hipLaunchKernelGGL(moments_fold_kernel, dim3(1), dim3(MF_BLOCK), 0, s, part, groups, nvals, acc);
  MFFT_HIP(hipGetLastError());
  return 0;
}

}  // namespace mfft

// acc[c * 6 + k] = merge(acc[c * 6 + k], statistic k of x[c, :] about center[c]), c < ncomp <= 6, on the plan's stream (acc and
// center: device doubles of the plan)
int mfft_plan_s::moments_sweep(const void* x, int ncomp, size_t n, const double* center, double* acc) {
  const unsigned grid = moments_grid(n, prec);
  const size_t waves = (size_t)grid * (MS_BLOCK / 64);
  MFFT_TRY(ensure(nlm, waves * (size_t)ncomp * NLS_STATS * sizeof(double)));
  double* part = static_cast<double*>(nlm.p);
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(moments_kernel<double>, dim3(grid, ncomp), dim3(MS_BLOCK), 0, stream, static_cast<const double*>(x), n, ncomp, center, part);
  else
    hipLaunchKernelGGL(moments_kernel<float>, dim3(grid, ncomp), dim3(MS_BLOCK), 0, stream, static_cast<const float*>(x), n, ncomp, center, part);
  MFFT_HIP(hipGetLastError());
  return moments_fold(part, waves, ncomp * NLS_STATS, acc, stream);
}

// the plan's accumulator of a moments call: nlsacc = [36 statistics in slot order][6 centres in slot order], cleared on the stream
int mfft_plan_s::moments_begin(const double center_slots[6]) {
  MFFT_TRY(ensure(nlsacc, (NLS_SLOTS + 2 * NLS_PAIRS) * sizeof(double)));
  double* acc = static_cast<double*>(nlsacc.p);
  MFFT_TRY(moments_clear(acc, NLS_SLOTS, stream));
  for (int i = 0; i < 2 * NLS_PAIRS; ++i) nlcall.center[i] = center_slots[i];      // (a member: the copy below is asynchronous)
  MFFT_HIP(hipMemcpyAsync(acc + NLS_SLOTS, nlcall.center, sizeof nlcall.center, hipMemcpyHostToDevice, stream));
  return 0;
}
int mfft_plan_s::moments_end(double host[36]) {
  MFFT_HIP(hipMemcpyAsync(host, nlsacc.p, NLS_SLOTS * sizeof(double), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[c * 6 + {0: min, 1: max, 2..5: S1..S4}] of a real device array (ncomp, n), c < ncomp; S_p = sum (x - center[c])^p,
// center null: zeros.  Synchronises the plan's stream.
int mfft_ew_moments(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* center, double* out_host) {
  if (!plan || !x || !out_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (n < 1) return set_error(MFFT_ERR_INVALID, "empty array");
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  double c6[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; center && c < ncomp; ++c) c6[c] = center[c];
  MFFT_TRY(plan->moments_begin(c6));
  double* acc = static_cast<double*>(plan->nlsacc.p);
  MFFT_TRY(plan->moments_sweep(x, ncomp, n, acc + NLS_SLOTS, acc));
  double host[NLS_SLOTS];
  MFFT_TRY(plan->moments_end(host));
  for (int i = 0; i < ncomp * NLS_STATS; ++i) out_host[i] = host[i];
  return 0;
}

}  // extern "C"
