// profiles.hip -- plane-averaged profiles along z on the device: per PAIR of real fields (x, y) and per z index m the five sums
//     [ sum (x - ca), sum (y - cb), sum (x - ca)^2, sum (y - cb)^2, sum (x - ca)(y - cb) ]
// over the (x, y) plane at m (the rule: include/mpifft4py_amd.h, nlz_reduce.h incr_value, nlz_prof.h prof_add) -- the first reduction whose
// result is a vector in z.  The fold of the partial profiles that the fused z stage emits (nlz_prof.h NlzProf::body; launches:
// core.hip nlr_rows), the streaming sweep mfft_ew_profiles over two real arrays of rows (the composed route of mfft_real_profiles,
// and the caller's own arrays) and the plan's accumulator.  No atomics anywhere: every partial profile goes out by plain stores,
// one launch adds them in a FIXED order, so the sums are bitwise reproducible run to run.  Products and sums in double whatever the
// precision of the data.
#include <math.h>
#include "plan_impl.h"
#include "nlz_prof.h"

using namespace mfft;

namespace {

constexpr int PF_VALS = 32, PF_LANES = 8;      // the fold's workgroup: 32 neighbouring values x 8 lanes over the partial profiles
constexpr int PS_COLS = 64, PS_LANES = 4;      // the sweep's workgroup: 64 neighbouring z x 4 lanes over the rows of its stripe
static_assert(NLP_STATS == MFFT_PROFILE_STATS, "the public header states the kernels' number of sums");

// acc[v] += the nslots partial profiles part[g * nvals + v], g in a fixed order: lane l of a value takes g = l, l + PF_LANES, .. in
// turn, lane 0 then adds the lanes' sums in order.  Neighbouring threads read neighbouring doubles.
__global__ __launch_bounds__(PF_VALS * PF_LANES) void prof_fold_kernel(const double* __restrict__ part, size_t nslots, size_t nvals, double* acc) {
  __shared__ double red[PF_LANES][PF_VALS];
  const int tv = (int)threadIdx.x % PF_VALS, tl = (int)threadIdx.x / PF_VALS;
  const size_t v = (size_t)blockIdx.x * PF_VALS + tv;
  double m = 0.0;
  if (v < nvals)
    for (size_t g = tl; g < nslots; g += PF_LANES) m += part[g * nvals + v];
  red[tl][tv] = m;
  __syncthreads();
  if (tl == 0 && v < nvals) {
    for (int l = 1; l < PF_LANES; ++l) m += red[l][tv];
    acc[v] += m;
  }
}

struct ProfCenters { double c[2 * NLS_PAIRS]; };      // [pair][a, b]

// Component blockIdx.z of two real arrays (ncomp, nrows, n): lane (tc, tl) of stripe blockIdx.y holds column m = blockIdx.x * PS_COLS
// + tc and takes the stripe's rows tl, tl + PS_LANES, .. in turn -- neighbouring lanes, neighbouring z: coalesced loads.  Five doubles
// of accumulators per lane, plain stores into part[(stripe * PS_LANES + tl)][component][sum][m]: the layout of the fused kernel's
// partials, every slot written (a lane that met no row stores zeros).
template <typename T>
__global__ __launch_bounds__(PS_COLS * PS_LANES) void prof_kernel(const T* __restrict__ x, const T* __restrict__ y, int64_t nrows, int n, int64_t stripe_rows,
                                                                 const ProfCenters centers, int ncomp, double* __restrict__ part) {
  const int tc = (int)threadIdx.x % PS_COLS, tl = (int)threadIdx.x / PS_COLS;
  const int m = (int)blockIdx.x * PS_COLS + tc, c = (int)blockIdx.z;
  if (m >= n) return;
  const double ca = c == 0 ? centers.c[0] : c == 1 ? centers.c[2] : centers.c[4], cb = c == 0 ? centers.c[1] : c == 1 ? centers.c[3] : centers.c[5];
  const size_t comp = (size_t)c * (size_t)nrows * (size_t)n;
  const int64_t r0 = (int64_t)blockIdx.y * stripe_rows, r1 = r0 + stripe_rows < nrows ? r0 + stripe_rows : nrows;
  double acc[NLP_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + tl; r < r1; r += PS_LANES) {
    const size_t at = comp + (size_t)r * (size_t)n + (size_t)m;
    prof_add(acc, incr_value((double)x[at], 1.0) - ca, incr_value((double)y[at], 1.0) - cb);
  }
  double* dst = part + (((size_t)blockIdx.y * PS_LANES + tl) * (size_t)ncomp + c) * (size_t)(NLP_STATS * n) + m;
#pragma unroll
  for (int s = 0; s < NLP_STATS; ++s) dst[(size_t)s * n] = acc[s];
}

// stripes of a prof_kernel launch: some 32 rows per stripe at the least, some 2048 workgroups at the most
int64_t prof_stripes(int64_t nrows, int64_t n, int ncomp) {
  const int64_t colblocks = (n + PS_COLS - 1) / PS_COLS;
  int64_t most = 2048 / (colblocks * ncomp);
  most = most < 1 ? 1 : most > 256 ? 256 : most;
  const int64_t want = (nrows + 31) / 32;
  return want < 1 ? 1 : want > most ? most : want;
}

}  // namespace

namespace mfft {

int prof_fold(const double* part, size_t nslots, size_t nvals, double* acc, hipStream_t s) {
  if (nslots == 0 || nvals == 0) return 0;
  const size_t grid = (nvals + PF_VALS - 1) / PF_VALS;
  if (grid > 0x7fffffffu) return set_error(MFFT_ERR_INTERNAL, "prof_fold: %zu values", nvals);
  hipLaunchKernelGGL(prof_fold_kernel, dim3((unsigned)grid), dim3(PF_VALS * PF_LANES), 0, s, part, nslots, nvals, acc);
  MFFT_HIP(hipGetLastError());
  return 0;
}

size_t prof_part_bytes(int ngroups, int tile, int npairs, int64_t n) {
  return (size_t)ngroups * (size_t)tile * (size_t)npairs * (size_t)NLP_STATS * (size_t)n * sizeof(double);
}

int prof_check(const double* center, int nfields) {
  for (int f = 0; center && f < nfields; ++f)
    if (!isfinite(center[f])) return set_error(MFFT_ERR_INVALID, "centre %d is not finite", f);
  return 0;
}

}  // namespace mfft

// acc[(c * 5 + s) * n + m] += the sums of component c of (x, y), two real arrays (ncomp, nrows, n), c < ncomp <= 3, about the centres
// center[2 c], center[2 c + 1], on the plan's stream
int mfft_plan_s::prof_sweep(const void* x, const void* y, int ncomp, int64_t nrows, int64_t n, const double* center, double* acc) {
  const int64_t stripes = prof_stripes(nrows, n, ncomp), stripe_rows = (nrows + stripes - 1) / stripes;
  const size_t nslots = (size_t)stripes * PS_LANES, nvals = (size_t)ncomp * NLP_STATS * (size_t)n;
  MFFT_TRY(ensure(nlm, nslots * nvals * sizeof(double)));
  ProfCenters ctr;
  for (int i = 0; i < 2 * NLS_PAIRS; ++i) ctr.c[i] = i < 2 * ncomp ? center[i] : 0.0;
  double* part = static_cast<double*>(nlm.p);
  const dim3 grid((unsigned)((n + PS_COLS - 1) / PS_COLS), (unsigned)stripes, (unsigned)ncomp);
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(prof_kernel<double>, grid, dim3(PS_COLS * PS_LANES), 0, stream, static_cast<const double*>(x), static_cast<const double*>(y), nrows,
                       (int)n, stripe_rows, ctr, ncomp, part);
  else
    hipLaunchKernelGGL(prof_kernel<float>, grid, dim3(PS_COLS * PS_LANES), 0, stream, static_cast<const float*>(x), static_cast<const float*>(y), nrows,
                       (int)n, stripe_rows, ctr, ncomp, part);
  MFFT_HIP(hipGetLastError());
  return prof_fold(part, nslots, nvals, acc, stream);
}

// the plan's accumulator of a profiles call: nlpacc = npairs x 5 x n doubles, pairs in slot order, zeroed on the stream; the centres
// in slot order
int mfft_plan_s::prof_begin(const double center_slots[6], int npairs, int64_t n) {
  const size_t bytes = (size_t)npairs * NLP_STATS * (size_t)n * sizeof(double);
  MFFT_TRY(ensure(nlpacc, bytes));
  MFFT_HIP(hipMemsetAsync(nlpacc.p, 0, bytes, stream));
  for (int i = 0; i < 6; ++i) nlcall.center[i] = center_slots[i];
  return 0;
}
int mfft_plan_s::prof_end(double* host, int npairs, int64_t n) {
  MFFT_HIP(hipMemcpyAsync(host, nlpacc.p, (size_t)npairs * NLP_STATS * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[(c * 5 + s) * n + m] of the pairs (x[c, r, m], y[c, r, m]) of two real device arrays (ncomp, nrows, n): see
// include/mpifft4py_amd.h.  Synchronises the plan's stream.
int mfft_ew_profiles(mfft_plan_t plan, const void* x, const void* y, int ncomp, int64_t nrows, int64_t n, int precision, const double* center,
                     double* out_host) {
  if (!plan || !x || !y || !out_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  if (nrows < 1 || n < 1 || n >= ((int64_t)1 << 30)) return set_error(MFFT_ERR_INVALID, "bad rows: %lld of %lld elements", (long long)nrows, (long long)n);
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  MFFT_TRY(prof_check(center, 2 * ncomp));
  double c6[6] = {0, 0, 0, 0, 0, 0};              // center: a_0.., then b_0..; slots [pair][a, b]
  for (int c = 0; center && c < ncomp; ++c) { c6[2 * c] = center[c]; c6[2 * c + 1] = center[ncomp + c]; }
  MFFT_TRY(plan->prof_begin(c6, ncomp, n));
  MFFT_TRY(plan->prof_sweep(x, y, ncomp, nrows, n, c6, static_cast<double*>(plan->nlpacc.p)));
  return plan->prof_end(out_host, ncomp, n);
}

}  // extern "C"
