// joint.hip -- joint histograms on the device: per PAIR of real fields (nba + 3)(nbb + 3) int64 counts,
//     cell = sa * (nbb + 3) + sb,   sa = hist_slot(x_a, lo_a, inv_a, nba),   sb = hist_slot(x_b, lo_b, inv_b, nbb)
// (nlz_reduce.h hist_slot and nlz_joint.h joint_cell: the one rule of host, sweep, fused kernel and tests).  The plan's accumulator of the fused z
// stage that ends in a joint histogram (nlz_joint.h NlzJoint::body; launches and fold: core.hip nlr_rows), and the streaming sweep
// mfft_ew_joint_histogram over two real arrays of equal length (the composed route of mfft_real_joint_histogram, and the caller's own arrays), the companion of
// mfft_ew_histogram.  No global atomics anywhere: a workgroup counts in ONE LDS grid (unsigned), stores it with plain stores, the
// fold of hist.hip adds the workgroups' rows in a FIXED order into int64.  Counts are integers: the same bits run to run, device
// to device and for every number of ranks.
#include <math.h>
#include "plan_impl.h"
#include "nlz_joint.h"

using namespace mfft;

namespace {

constexpr int JS_BLOCK = 256;
static_assert(NLJ_MAXBINS == MFFT_JOINT_MAXBINS, "the public header states the kernels' limit");
constexpr size_t JS_CHUNK = (size_t)1 << 40;      // elements of one sweep launch: 2^40 / 1024 workgroups < 2^32 each

struct JointRange { double lo[2], inv[2]; };

// Two real arrays of n elements: 16 bytes per lane of each, the workgroup's grid in LDS, plain stores of it into part[(workgroup,
// cells)].  The arrays need not start on 16 bytes, nor on the same offset from it: the vector body runs where BOTH are aligned
// (the same misalignment), the elements before the first aligned one and after the last whole vector are taken singly by the
// first lanes, as hist.hip does; arrays of different misalignment are taken singly throughout by the host's choice of `vec`.
template <typename T>
__global__ __launch_bounds__(JS_BLOCK) void joint_kernel(const T* __restrict__ x, const T* __restrict__ y, size_t n, const JointRange r, int nba,
                                                        int nbb, int vec, unsigned* __restrict__ part) {
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) V { T v[VEC]; };
  __shared__ unsigned grid[NLJ_MAXCELLS];
  nba = nba < 1 ? 1 : nba > NLJ_MAXBINS ? NLJ_MAXBINS : nba;
  nbb = nbb < 1 ? 1 : nbb > NLJ_MAXBINS ? NLJ_MAXBINS : nbb;
  const int cells = (nba + 3) * (nbb + 3);
  for (int i = threadIdx.x; i < cells; i += JS_BLOCK) grid[i] = 0u;
  __syncthreads();
  const double loa = r.lo[0], iva = r.inv[0], lob = r.lo[1], ivb = r.inv[1];
  auto count = [&](T a, T b) {
    MFFT_LDS_COUNT(grid + joint_cell(hist_slot((double)a, loa, iva, nba), hist_slot((double)b, lob, ivb, nbb), nbb));
  };
  const size_t gtid = (size_t)blockIdx.x * JS_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * JS_BLOCK;
  if (vec) {
    const size_t mis = ((uintptr_t)x % 16) / sizeof(T);      // (the host checked: y has the same)
    size_t head = mis ? VEC - mis : 0;
    if (head > n) head = n;
    const size_t nv = (n - head) / VEC, tail0 = head + nv * VEC;
    const V* xv = reinterpret_cast<const V*>(x + head);
    const V* yv = reinterpret_cast<const V*>(y + head);
    for (size_t i = gtid; i < nv; i += gsize) {
      const V p = xv[i], q = yv[i];
#pragma unroll
      for (int k = 0; k < VEC; ++k) count(p.v[k], q.v[k]);
    }
    if (gtid < head) count(x[gtid], y[gtid]);
    if (tail0 + gtid < n) count(x[tail0 + gtid], y[tail0 + gtid]);      // fewer than VEC <= JS_BLOCK of them
  } else {
    for (size_t i = gtid; i < n; i += gsize) count(x[i], y[i]);
  }
  __syncthreads();
  unsigned* dst = part + (size_t)blockIdx.x * (size_t)cells;
  for (int i = threadIdx.x; i < cells; i += JS_BLOCK) dst[i] = grid[i];
}

// workgroups of a joint_kernel launch over n elements
unsigned joint_grid(size_t n, int prec) {
  const size_t vec = prec == MFFT_DOUBLE ? 2 : 4;
  size_t g = (n / vec + (size_t)JS_BLOCK * 8 - 1) / ((size_t)JS_BLOCK * 8);      // some eight vectors per lane
  return (unsigned)(g > 1024 ? 1024 : (g ? g : 1));
}

}  // namespace

namespace mfft {

int joint_range(double lo, double hi, int nb, double* inv) {
  if (nb < 1 || nb > NLJ_MAXBINS) return set_error(MFFT_ERR_INVALID, "a joint histogram takes 1 .. %d bins per field, not %d", NLJ_MAXBINS, nb);
  if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g): lo < hi, both finite", lo, hi);
  const double v = (double)nb / (hi - lo);
  if (!isfinite(v) || !(v > 0.0)) return set_error(MFFT_ERR_INVALID, "histogram range [%g, %g) is too narrow or too wide", lo, hi);
  *inv = v;
  return 0;
}

size_t joint_part_bytes(int ngroups, int npairs, int nba, int nbb) {
  return (size_t)ngroups * (size_t)npairs * (size_t)joint_cells(nba, nbb) * sizeof(unsigned);
}

}  // namespace mfft

// acc[cell] += counts of the pairs (x[i], y[i]), i < n, on the plan's stream (acc: device int64 of the plan, one pair's cells)
int mfft_plan_s::joint_sweep(const void* x, const void* y, size_t n, const double* lo, const double* inv, int nba, int nbb, int64_t* acc) {
  JointRange r;
  for (int c = 0; c < 2; ++c) { r.lo[c] = lo[c]; r.inv[c] = inv[c]; }
  const size_t rsz = prec == MFFT_DOUBLE ? 8 : 4;
  for (size_t o = 0; o < n; o += JS_CHUNK) {       // (a workgroup's share of a launch stays below 2^32 elements)
    const size_t len = std::min(JS_CHUNK, n - o);
    const unsigned grid = joint_grid(len, prec);
    MFFT_TRY(ensure(nlm, joint_part_bytes((int)grid, 1, nba, nbb)));
    unsigned* part = static_cast<unsigned*>(nlm.p);
    const char* px = static_cast<const char*>(x) + o * rsz;
    const char* py = static_cast<const char*>(y) + o * rsz;
    const int vec = (uintptr_t)px % 16 == (uintptr_t)py % 16 ? 1 : 0;
    if (prec == MFFT_DOUBLE)
      hipLaunchKernelGGL(joint_kernel<double>, dim3(grid), dim3(JS_BLOCK), 0, stream, reinterpret_cast<const double*>(px),
                         reinterpret_cast<const double*>(py), len, r, nba, nbb, vec, part);
    else
      hipLaunchKernelGGL(joint_kernel<float>, dim3(grid), dim3(JS_BLOCK), 0, stream, reinterpret_cast<const float*>(px),
                         reinterpret_cast<const float*>(py), len, r, nba, nbb, vec, part);
    MFFT_HIP(hipGetLastError());
    MFFT_TRY(hist_fold_slots(part, grid, 1, joint_cells(nba, nbb), acc, stream));
  }
  return 0;
}

// the plan's accumulator of a joint-histogram call: nljacc = 3 x NLJ_MAXCELLS int64, cleared on the stream; the ranges in slot order
int mfft_plan_s::joint_begin(const double lo_slots[6], const double inv_slots[6], int nba, int nbb) {
  if (nba < 1 || nba > NLJ_MAXBINS || nbb < 1 || nbb > NLJ_MAXBINS) return set_error(MFFT_ERR_INVALID, "bins outside 1 .. %d", NLJ_MAXBINS);
  MFFT_TRY(ensure(nljacc, (size_t)3 * NLJ_MAXCELLS * sizeof(int64_t)));
  MFFT_HIP(hipMemsetAsync(nljacc.p, 0, (size_t)3 * NLJ_MAXCELLS * sizeof(int64_t), stream));
  for (int i = 0; i < 6; ++i) { nlcall.lo[i] = lo_slots[i]; nlcall.inv[i] = inv_slots[i]; }
  nlcall.nba = nba;
  nlcall.nbb = nbb;
  return 0;
}
int mfft_plan_s::joint_end(int64_t* host, int npairs) {
  MFFT_HIP(hipMemcpyAsync(host, nljacc.p, (size_t)npairs * joint_cells(nlcall.nba, nlcall.nbb) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

extern "C" {

// out_host[c * cells + cell] of the pairs (x[c, i], y[c, i]) of two real device arrays (ncomp, n).  Synchronises the plan's stream.
int mfft_ew_joint_histogram(mfft_plan_t plan, const void* x, const void* y, int ncomp, size_t n, int precision, const double* lo, const double* hi,
                            int nba, int nbb, int64_t* out_host) {
  if (!plan || !x || !y || !out_host || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  if (n < 1) return set_error(MFFT_ERR_INVALID, "empty array");
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  double l6[6] = {0, 0, 0, 0, 0, 0}, i6[6] = {1, 1, 1, 1, 1, 1};
  for (int c = 0; c < ncomp; ++c) {                // lo, hi: a_0.., then b_0..; slots [pair][a, b]
    MFFT_TRY(joint_range(lo[c], hi[c], nba, &i6[2 * c]));
    MFFT_TRY(joint_range(lo[ncomp + c], hi[ncomp + c], nbb, &i6[2 * c + 1]));
    l6[2 * c] = lo[c];
    l6[2 * c + 1] = lo[ncomp + c];
  }
  MFFT_TRY(plan->joint_begin(l6, i6, nba, nbb));
  const size_t rsz = precision == MFFT_DOUBLE ? 8 : 4;
  const int cells = joint_cells(nba, nbb);
  for (int c = 0; c < ncomp; ++c)
    MFFT_TRY(plan->joint_sweep(static_cast<const char*>(x) + (size_t)c * n * rsz, static_cast<const char*>(y) + (size_t)c * n * rsz, n, l6 + 2 * c,
                               i6 + 2 * c, nba, nbb, static_cast<int64_t*>(plan->nljacc.p) + (size_t)c * cells));
  return plan->joint_end(out_host, ncomp);
}

}  // extern "C"
