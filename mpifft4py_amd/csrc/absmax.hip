// absmax.hip -- max |x| reductions on the device: the fold of the partial maxima that the fused nonlinear z stage emits
// (fft_nlz.h NlzAbsMax) and the streaming sweep mfft_ew_absmax over real fields (the composed nonlinear route, and the
// caller's own arrays).  No global atomics anywhere: waves store partial maxima with plain stores, a second small launch
// folds them in a fixed order -- and a maximum does not depend on the order, so the results are bitwise reproducible.
// NaN contract: a NaN in the data is a NaN in the result (nan_max below; fmax would drop it), Inf gives Inf.
#include <math.h>
#include <vector>
#include "plan_impl.h"
#include "fft_nlz.h"

using namespace mfft;

namespace {

constexpr int FOLD_BLOCK = 192;        // a multiple of every period (1, 2, 3, 6): a thread meets ONE slot of the period
constexpr int FOLD_GRID_MAX = 256;
constexpr int AM_BLOCK = 256;

__device__ __forceinline__ double nan_max_d(double m, double x) { return (x > m || x != x) ? x : m; }

// part: (count, period) values >= 0 or NaN.  out[b * period + s] = max over the groups of workgroup b (ACC: out[s] =
// max(out[s], scale * that), one workgroup).  Values are widened to double; scale > 0.
template <typename T, bool ACC>
__global__ __launch_bounds__(FOLD_BLOCK) void absmax_fold_kernel(const T* __restrict__ part, size_t total, int period, double scale,
                                                                double* out) {
  __shared__ double red[FOLD_BLOCK];
  double m = 0.0;
  for (size_t i = (size_t)blockIdx.x * FOLD_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * FOLD_BLOCK)
    m = nan_max_d(m, (double)part[i]);           // (i mod period == threadIdx.x mod period: the strides are multiples of it)
  red[threadIdx.x] = m;
  __syncthreads();
  if ((int)threadIdx.x < period) {
    for (int t = (int)threadIdx.x + period; t < FOLD_BLOCK; t += period) m = nan_max_d(m, red[t]);
    if (ACC) out[threadIdx.x] = nan_max_d(out[threadIdx.x], m * scale);
    else out[(size_t)blockIdx.x * period + threadIdx.x] = m;
  }
}

// One component of a real field per blockIdx.y: 16 bytes per lane, the wave's maximum by shuffles, one plain store per wave
// into part[(wave of the launch) * ncomp + component].  A component need not start on 16 bytes (single precision, odd n):
// the elements before the first aligned one and after the last whole vector are taken singly by the first lanes.
template <typename T>
__global__ __launch_bounds__(AM_BLOCK) void absmax_kernel(const T* __restrict__ x, size_t n, int ncomp, T* __restrict__ part) {
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) V { T v[VEC]; };
  const int c = blockIdx.y;
  const T* p = x + (size_t)c * n;
  const size_t mis = ((uintptr_t)p % 16) / sizeof(T);
  size_t head = mis ? VEC - mis : 0;
  if (head > n) head = n;
  const size_t nv = (n - head) / VEC, tail0 = head + nv * VEC;
  const V* pv = reinterpret_cast<const V*>(p + head);
  const size_t gtid = (size_t)blockIdx.x * AM_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * AM_BLOCK;
  T m = (T)0;
  for (size_t i = gtid; i < nv; i += gsize) {
    const V q = pv[i];
#pragma unroll
    for (int k = 0; k < VEC; ++k) m = nan_max(m, abs_of(q.v[k]));
  }
  if (gtid < head) m = nan_max(m, abs_of(p[gtid]));
  if (tail0 + gtid < n) m = nan_max(m, abs_of(p[tail0 + gtid]));      // fewer than VEC <= AM_BLOCK of them
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) part[(gtid >> 6) * (size_t)ncomp + c] = m;
}

}  // namespace

namespace mfft {

size_t absmax_fold_scratch_bytes() { return (size_t)FOLD_GRID_MAX * 6 * sizeof(double); }

// acc[s] = max(acc[s], scale * max_g part[g * period + s]), s < period <= 6: two launches on `s`, `scratch` holds
// absmax_fold_scratch_bytes().  prec: the precision of `part`.
int absmax_fold(const void* part, size_t groups, int period, int prec, double scale, double* scratch, double* acc, hipStream_t s) {
  if (period < 1 || period > 6 || FOLD_BLOCK % period != 0) return set_error(MFFT_ERR_INTERNAL, "absmax_fold: period %d", period);
  const size_t total = groups * (size_t)period;
  if (total == 0) return 0;
  size_t g = (total + (size_t)FOLD_BLOCK * 8 - 1) / ((size_t)FOLD_BLOCK * 8);
  const int grid = (int)(g > (size_t)FOLD_GRID_MAX ? (size_t)FOLD_GRID_MAX : (g ? g : 1));
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL((absmax_fold_kernel<double, false>), dim3(grid), dim3(FOLD_BLOCK), 0, s, static_cast<const double*>(part), total, period, 1.0, scratch);
  else
    hipLaunchKernelGGL((absmax_fold_kernel<float, false>), dim3(grid), dim3(FOLD_BLOCK), 0, s, static_cast<const float*>(part), total, period, 1.0, scratch);
  MFFT_HIP(hipGetLastError());
  hipLaunchKernelGGL((absmax_fold_kernel<double, true>), dim3(1), dim3(FOLD_BLOCK), 0, s, scratch, (size_t)grid * period, period, scale, acc);
  MFFT_HIP(hipGetLastError());
  return 0;
}

// waves of an absmax_kernel launch over n elements per component
static unsigned absmax_grid(size_t n, int prec) {
  const size_t vec = prec == MFFT_DOUBLE ? 2 : 4;
  size_t g = (n / vec + AM_BLOCK - 1) / AM_BLOCK;
  return (unsigned)(g > 4096 ? 4096 : (g ? g : 1));
}

}  // namespace mfft

// acc[c] = max(acc[c], max |x[c, :]|), c < ncomp <= 6, on the plan's stream (acc: device, six doubles of the plan)
int mfft_plan_s::absmax_sweep(const void* x, int ncomp, size_t n, double* acc) {
  const unsigned grid = absmax_grid(n, prec);
  const size_t waves = (size_t)grid * (AM_BLOCK / 64);
  MFFT_TRY(ensure(nlm, absmax_fold_scratch_bytes() + waves * (size_t)ncomp * rs));
  double* scratch = static_cast<double*>(nlm.p);
  void* part = static_cast<char*>(nlm.p) + absmax_fold_scratch_bytes();
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(absmax_kernel<double>, dim3(grid, ncomp), dim3(AM_BLOCK), 0, stream, static_cast<const double*>(x), n, ncomp, static_cast<double*>(part));
  else
    hipLaunchKernelGGL(absmax_kernel<float>, dim3(grid, ncomp), dim3(AM_BLOCK), 0, stream, static_cast<const float*>(x), n, ncomp, static_cast<float*>(part));
  MFFT_HIP(hipGetLastError());
  return absmax_fold(part, waves, ncomp, prec, 1.0, scratch, acc, stream);
}

extern "C" {

// out_host[c] = max |x[c, :]| of a real device array (ncomp, n), c < ncomp <= 6.  Synchronises the plan's stream.
int mfft_ew_absmax(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, double* out_host) {
  if (!plan || !x || !out_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (n < 1) return set_error(MFFT_ERR_INVALID, "empty array");
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  MFFT_TRY(plan->ensure(plan->nlmacc, 12 * sizeof(double)));
  double* acc = static_cast<double*>(plan->nlmacc.p) + 6;          // (the first six belong to the nonlinear operation)
  MFFT_HIP(hipMemsetAsync(acc, 0, 6 * sizeof(double), plan->stream));
  MFFT_TRY(plan->absmax_sweep(x, ncomp, n, acc));
  double host[6];
  MFFT_HIP(hipMemcpyAsync(host, acc, sizeof host, hipMemcpyDeviceToHost, plan->stream));
  MFFT_HIP(hipStreamSynchronize(plan->stream));
  for (int c = 0; c < ncomp; ++c) out_host[c] = host[c];
  return 0;
}

}  // extern "C"
