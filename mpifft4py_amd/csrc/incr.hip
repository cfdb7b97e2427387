// incr.hip -- structure functions along z on the device: per field and separation s the sums S2, S3, S4 of the increments
// d = r(z + s) - r(z) over periodic rows (the rule: include/mpifft4py_amd.h, nlz_reduce.h incr_value, nlz_incr.h incr_add).  The fold of the
// partial sums that the fused z stage emits (nlz_incr.h NlzIncr::body), the streaming sweep mfft_ew_increments over real rows (the
// composed route of mfft_real_increments, and the caller's own arrays) and the plan's accumulator.
// No atomics anywhere: waves store their partials with plain stores, one small launch adds them in a FIXED order, so the sums are
// bitwise reproducible run to run.  Powers and sums in double whatever the precision of the data.
#include <math.h>
#include "plan_impl.h"
#include "nlz_incr.h"

using namespace mfft;

namespace {

constexpr int IF_BLOCK = 576;           // a multiple of every count of values (24, 48, 72, 144): a thread meets ONE value
constexpr int IS_BLOCK = 256;
static_assert(IF_BLOCK % NLI_SLOTS == 0, "the fold's workgroup holds whole groups of slots");

// One workgroup reads the groups' slots as they lie in memory: thread t holds value t % nvals and takes the groups t / nvals,
// + IF_BLOCK / nvals, .. in that order; the first nvals threads then add the IF_BLOCK / nvals rows of the workgroup in order, and
// the accumulator (moments.hip moments_fold_kernel, sums only).
__global__ __launch_bounds__(IF_BLOCK) void incr_fold_kernel(const double* __restrict__ part, size_t groups, int nvals, double* acc) {
  __shared__ double red[IF_BLOCK];
  const int t = (int)threadIdx.x, rows = IF_BLOCK / nvals;
  double m = 0.0;
  for (size_t i = t; i < groups * (size_t)nvals; i += IF_BLOCK) m += part[i];      // (IF_BLOCK % nvals == 0: i % nvals stays)
  red[t] = m;
  __syncthreads();
  if (t < nvals) {
    for (int r = 1; r < rows; ++r) m += red[r * nvals + t];
    acc[t] += m;
  }
}

struct SepList {
  int sep[NLI_MAXSEP];
  int nsep;
};

// One component of nrows real rows per blockIdx.y, the elements of its rows spread over the launch's threads in memory order
// (consecutive lanes, consecutive elements of a row); per element the row's value at the nsep shifted positions comes out of the
// caches.  NLI_FIELD doubles of accumulators per lane (statically indexed: the loop over the separations is unrolled and guarded),
// one wave reduction at the end, one plain store of NLI_FIELD doubles per wave into part[(wave of the launch) * ncomp + component].
template <typename T>
__global__ __launch_bounds__(IS_BLOCK) void incr_kernel(const T* __restrict__ x, int64_t nrows, int n, int64_t pitch, int ncomp, SepList L,
                                                       double* __restrict__ part) {
  const int c = blockIdx.y;
  const T* p = x + (size_t)c * (size_t)nrows * (size_t)pitch;
  const size_t total = (size_t)nrows * (size_t)n;
  const size_t gtid = (size_t)blockIdx.x * IS_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * IS_BLOCK;
  double m[NLI_FIELD];
#pragma unroll
  for (int i = 0; i < NLI_FIELD; ++i) m[i] = 0.0;
  for (size_t e = gtid; e < total; e += gsize) {
    const size_t row = e / (size_t)n;
    const int z = (int)(e - row * (size_t)n);
    const T* r = p + row * (size_t)pitch;
    const double r0 = incr_value((double)r[z], 1.0);
#pragma unroll
    for (int i = 0; i < NLI_MAXSEP; ++i)
      if (i < L.nsep) incr_add(m + i * NLI_STATS, incr_value((double)r[incr_pos(z, L.sep[i], n)], 1.0), r0);
  }
  wave_sums_store<IS_BLOCK, NLI_FIELD>(m, (int)threadIdx.x, part + ((gtid >> 6) * (size_t)ncomp + c) * NLI_FIELD);
}

// workgroups of an incr_kernel launch over `total` elements per component: some sixteen elements per lane
unsigned incr_grid(size_t total) {
  size_t g = (total + (size_t)IS_BLOCK * 16 - 1) / ((size_t)IS_BLOCK * 16);
  return (unsigned)(g > 2048 ? 2048 : (g ? g : 1));
}

}  // namespace

namespace mfft {

int incr_fold(const double* part, size_t groups, int nvals, double* acc, hipStream_t s) {
  if (nvals < NLI_FIELD || nvals % NLI_FIELD != 0 || IF_BLOCK % nvals != 0) return set_error(MFFT_ERR_INTERNAL, "incr_fold: %d values", nvals);
  if (groups == 0) return 0;
  hipLaunchKernelGGL(incr_fold_kernel, dim3(1), dim3(IF_BLOCK), 0, s, part, groups, nvals, acc);
  MFFT_HIP(hipGetLastError());
  return 0;
}

int incr_check(const int64_t* seps, int nsep, int64_t m) {
  if (!seps) return set_error(MFFT_ERR_INVALID, "null argument");
  if (nsep < 1 || nsep > NLI_MAXSEP) return set_error(MFFT_ERR_INVALID, "%d separations: one call takes 1 .. %d", nsep, NLI_MAXSEP);
  for (int i = 0; i < nsep; ++i)
    if (seps[i] < 1 || seps[i] >= m)
      return set_error(MFFT_ERR_INVALID, "separation %lld outside 1 .. %lld of a periodic row of %lld points", (long long)seps[i], (long long)(m - 1), (long long)m);
  return 0;
}

}  // namespace mfft

// acc[(c * MAXSEP + i) * 3 + k] += the sums of component c of x (ncomp x nrows rows of n elements, pitch apart), c < ncomp <= 6, at the
// plan's separations (incr_begin), on the plan's stream
int mfft_plan_s::incr_sweep(const void* x, int ncomp, int64_t nrows, int64_t n, int64_t pitch, double* acc) {
  const unsigned grid = incr_grid((size_t)nrows * (size_t)n);
  const size_t waves = (size_t)grid * (IS_BLOCK / 64);
  MFFT_TRY(ensure(nlm, waves * (size_t)ncomp * NLI_FIELD * sizeof(double)));
  double* part = static_cast<double*>(nlm.p);
  SepList L;
  for (int i = 0; i < NLI_MAXSEP; ++i) L.sep[i] = i < nlcall.nsep ? nlcall.sep[i] : 1;
  L.nsep = nlcall.nsep;
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(incr_kernel<double>, dim3(grid, ncomp), dim3(IS_BLOCK), 0, stream, static_cast<const double*>(x), nrows, (int)n, pitch, ncomp, L, part);
  else
    hipLaunchKernelGGL(incr_kernel<float>, dim3(grid, ncomp), dim3(IS_BLOCK), 0, stream, static_cast<const float*>(x), nrows, (int)n, pitch, ncomp, L, part);
  MFFT_HIP(hipGetLastError());
  return incr_fold(part, waves, ncomp * NLI_FIELD, acc, stream);
}

// the plan's accumulator of an increments call: nliacc = NLI_SLOTS doubles in slot order, zeroed on the stream; the call's
// separations (checked by the caller against the row length: incr_check)
int mfft_plan_s::incr_begin(const int64_t* seps, int nsep) {
  MFFT_TRY(ensure(nliacc, NLI_SLOTS * sizeof(double)));
  MFFT_HIP(hipMemsetAsync(nliacc.p, 0, NLI_SLOTS * sizeof(double), stream));
  for (int i = 0; i < NLI_MAXSEP; ++i) nlcall.sep[i] = i < nsep ? (int)seps[i] : 1;
  nlcall.nsep = nsep;
  return 0;
}
int mfft_plan_s::incr_end(double* host) {
  MFFT_HIP(hipMemcpyAsync(host, nliacc.p, NLI_SLOTS * sizeof(double), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[(c * nsep + i) * 3 + {0, 1, 2}] = S2, S3, S4 of component c at seps[i]: see include/mpifft4py_amd.h.  Synchronises the
// plan's stream.
int mfft_ew_increments(mfft_plan_t plan, const void* x, int ncomp, int64_t nrows, int64_t n, int64_t row_pitch, int precision,
                       const int64_t* seps, int nsep, double* out_host) {
  if (!plan || !x || !out_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (nrows < 1 || n < 2 || n >= ((int64_t)1 << 30) || row_pitch < n) return set_error(MFFT_ERR_INVALID, "bad rows: %lld of %lld elements, pitch %lld", (long long)nrows, (long long)n, (long long)row_pitch);
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  MFFT_TRY(incr_check(seps, nsep, n));
  MFFT_TRY(plan->incr_begin(seps, nsep));
  MFFT_TRY(plan->incr_sweep(x, ncomp, nrows, n, row_pitch, static_cast<double*>(plan->nliacc.p)));
  double host[NLI_SLOTS];
  MFFT_TRY(plan->incr_end(host));
  for (int c = 0; c < ncomp; ++c)
    for (int i = 0; i < nsep; ++i)
      for (int k = 0; k < NLI_STATS; ++k) out_host[(c * nsep + i) * NLI_STATS + k] = host[(c * NLI_MAXSEP + i) * NLI_STATS + k];
  return 0;
}

}  // extern "C"
