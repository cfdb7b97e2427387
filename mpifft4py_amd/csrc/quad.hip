// quad.hip -- statistics of a quadratic form q = sum_f w_f r_f^2 of up to six real fields: [min, max, S1 .. S4] of q about a
// centre and, with nbins > 0, its nbins + 3 counts (nlz_reduce.h hist_slot).  The plan's accumulators of the fused z stage that
// ends in them (nlz_quad.h NlzQuad::body; launches and folds: core.hip nlr_rows), the streaming sweep mfft_ew_quadratic over real fields -- q is formed on the fly, there is
// no q array --, and the two small kernels of the composed route of mfft_real_quadratic: add one field's (w r) r into the plan's
// array of doubles, sweep that array once.  ONE evaluation rule (include/mpifft4py_amd.h; nlz_quad.h quad_term): q = 0, then per
// field in slot order q = q + (w r) r, every product and sum rounded on its own, in double.
// No global atomics: waves store their partial statistics and workgroups their LDS histograms with plain stores, the folds of
// moments.hip and hist.hip add them in a FIXED order.  Bitwise reproducible.
#include <math.h>
#include "plan_impl.h"
#include "nlz_quad.h"

using namespace mfft;

namespace {

constexpr int QS_BLOCK = 256;
constexpr int NB3_MAX = NLH_MAXBINS + 3;
constexpr size_t QS_CHUNK = (size_t)1 << 40;      // elements of one sweep launch: 2^40 / 1024 workgroups < 2^32 each

struct QuadSweep {
  double w[6];
  double center, lo, inv;
  int nbins, ncomp;
};

// Element i of the ncomp components of x (stride elements apart): SQUARE, q = sum_c (w_c x_c) x_c; otherwise x is an array of q
// itself (one component, the composed route).  VEC: 16 bytes per lane and component where every component starts on 16 bytes and
// n is whole vectors; the scalar build takes everything else.  The workgroup's histogram in LDS, its statistics in six doubles per
// lane; part of the launch: mpart[(wave of the launch) * 6], hpart[workgroup * (nbins + 3)], every slot written.
template <typename T, bool SQUARE, bool VEC>
__global__ __launch_bounds__(QS_BLOCK) void quad_sweep_kernel(const T* __restrict__ x, size_t stride, size_t n, const QuadSweep a,
                                                             double* __restrict__ mpart, unsigned* __restrict__ hpart) {
  constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
  struct alignas(V * sizeof(T)) Vt { T v[V]; };
  __shared__ unsigned hist[NB3_MAX];
  const int nb3 = a.nbins + 3;
  for (int i = threadIdx.x; i < nb3; i += QS_BLOCK) hist[i] = 0u;
  __syncthreads();
  double m[NLS_STATS];
  moments_clear(m);
  const size_t gtid = (size_t)blockIdx.x * QS_BLOCK + threadIdx.x, gsize = (size_t)gridDim.x * QS_BLOCK;
  for (size_t i = gtid; i < n / V; i += gsize) {
    double q[V];
#pragma unroll
    for (int k = 0; k < V; ++k) q[k] = 0.0;
    for (int c = 0; c < a.ncomp; ++c) {
      const Vt xv = *reinterpret_cast<const Vt*>(x + (size_t)c * stride + i * V);
      const double wc = c == 0 ? a.w[0] : c == 1 ? a.w[1] : c == 2 ? a.w[2] : c == 3 ? a.w[3] : c == 4 ? a.w[4] : a.w[5];
#pragma unroll
      for (int k = 0; k < V; ++k) q[k] = SQUARE ? quad_term(q[k], wc, (double)xv.v[k]) : (double)xv.v[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      moments_add(m, q[k], a.center);
      if (a.nbins > 0) MFFT_LDS_COUNT(hist + hist_slot(q[k], a.lo, a.inv, a.nbins));
    }
  }
  __syncthreads();
  unsigned* dst = hpart + (size_t)blockIdx.x * nb3;
  for (int i = threadIdx.x; i < nb3; i += QS_BLOCK) dst[i] = hist[i];
  wave_moments_store<QS_BLOCK>(m, (int)threadIdx.x, mpart + (gtid >> 6) * NLS_STATS);
}

// the composed route: q[i] = (first ? 0 : q[i]) + (w r[i]) r[i], the rule's step for one field
template <typename T>
__global__ __launch_bounds__(QS_BLOCK) void quad_accum_kernel(const T* __restrict__ r, double* __restrict__ q, size_t n, double w, int first) {
  const size_t gsize = (size_t)gridDim.x * QS_BLOCK;
  for (size_t i = (size_t)blockIdx.x * QS_BLOCK + threadIdx.x; i < n; i += gsize) q[i] = quad_term(first ? 0.0 : q[i], w, (double)r[i]);
}

unsigned quad_grid(size_t n) {
  size_t g = (n + (size_t)QS_BLOCK * 16 - 1) / ((size_t)QS_BLOCK * 16);      // some sixteen elements per lane
  return (unsigned)(g > 1024 ? 1024 : (g ? g : 1));
}

template <typename T, bool SQUARE>
int sweep_launch(const T* x, size_t stride, size_t n, const QuadSweep& a, unsigned grid, double* mpart, unsigned* hpart, hipStream_t s) {
  constexpr size_t V = 16 / sizeof(T);
  const bool vec = (uintptr_t)x % 16 == 0 && n % V == 0 && (a.ncomp == 1 || stride % V == 0);
  if (vec)
    hipLaunchKernelGGL((quad_sweep_kernel<T, SQUARE, true>), dim3(grid), dim3(QS_BLOCK), 0, s, x, stride, n, a, mpart, hpart);
  else
    hipLaunchKernelGGL((quad_sweep_kernel<T, SQUARE, false>), dim3(grid), dim3(QS_BLOCK), 0, s, x, stride, n, a, mpart, hpart);
  MFFT_HIP(hipGetLastError());
  return 0;
}

}  // namespace

namespace mfft {

size_t quad_mpart_bytes(int64_t waves) { return ((size_t)waves * NLS_STATS * sizeof(double) + 127) / 128 * 128; }
size_t quad_hpart_bytes(int ngroups, int nbins) { return (size_t)ngroups * (size_t)(nbins + 3) * sizeof(unsigned); }

int quad_check(const double* weights, int nfields, double lo, double hi, int nbins, double* inv) {
  if (nbins < 0 || nbins > NLH_MAXBINS) return set_error(MFFT_ERR_INVALID, "nbins must be 0 .. %d, not %d", NLH_MAXBINS, nbins);
  for (int f = 0; f < nfields; ++f)
    if (!isfinite(weights[f])) return set_error(MFFT_ERR_INVALID, "weight %d is not finite", f);
  *inv = 1.0;
  if (nbins > 0) MFFT_TRY(hist_range(lo, hi, nbins, inv));
  return 0;
}

}  // namespace mfft

// the plan's accumulators of a quadratic call: slot 0 of nlsacc (six doubles, the centre behind the statistics) and, nbins > 0, the
// first nbins + 3 counts of nlhacc, both cleared on the stream; centre and range of q are slot 0 of the call's parameters
int mfft_plan_s::quad_begin(double center, double lo, double inv, int nbins) {
  const double c6[6] = {center, 0, 0, 0, 0, 0}, l6[6] = {lo, 0, 0, 0, 0, 0}, i6[6] = {inv, 1, 1, 1, 1, 1};
  MFFT_TRY(moments_begin(c6));
  if (nbins > 0) MFFT_TRY(hist_begin(l6, i6, nbins));
  nlcall.lo[0] = lo; nlcall.inv[0] = inv; nlcall.nbins = nbins;
  return 0;
}
int mfft_plan_s::quad_end(double out6[6], int64_t* counts) {
  double nlq_host[NLS_STATS];
  MFFT_HIP(hipMemcpyAsync(nlq_host, nlsacc.p, NLS_STATS * sizeof(double), hipMemcpyDeviceToHost, stream));
  std::vector<int64_t> h((size_t)nlcall.nbins + 3);
  if (nlcall.nbins > 0) MFFT_HIP(hipMemcpyAsync(h.data(), nlhacc.p, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  for (int k = 0; k < NLS_STATS; ++k) out6[k] = nlq_host[k];      // (the outputs are written only once nothing can fail any more)
  if (nlcall.nbins > 0) memcpy(counts, h.data(), h.size() * sizeof(int64_t));
  return 0;
}

// one sweep over n elements of the ncomp components of x (stride apart), or of the plan's q array (square == false), into the
// plan's accumulators; on the plan's stream
int mfft_plan_s::quad_sweep(const void* x, bool as_double, int ncomp, size_t stride, size_t n, const double* w, bool square) {
  QuadSweep a;
  for (int c = 0; c < 6; ++c) a.w[c] = c < ncomp ? w[c] : 0.0;
  a.center = nlcall.center[0]; a.lo = nlcall.lo[0]; a.inv = nlcall.inv[0]; a.nbins = nlcall.nbins; a.ncomp = ncomp;
  double* macc = static_cast<double*>(nlsacc.p);
  int64_t* hacc = static_cast<int64_t*>(nlhacc.p);
  for (size_t o = 0; o < n; o += QS_CHUNK) {
    const size_t len = std::min(QS_CHUNK, n - o);
    const unsigned grid = quad_grid(len);
    const size_t waves = (size_t)grid * (QS_BLOCK / 64);
    MFFT_TRY(ensure(nlm, quad_mpart_bytes((int64_t)waves) + quad_hpart_bytes((int)grid, a.nbins)));
    double* mpart = static_cast<double*>(nlm.p);
    unsigned* hpart = reinterpret_cast<unsigned*>(static_cast<char*>(nlm.p) + quad_mpart_bytes((int64_t)waves));
    if (!square) MFFT_TRY((sweep_launch<double, false>(static_cast<const double*>(x) + o, stride, len, a, grid, mpart, hpart, stream)));
    else if (as_double) MFFT_TRY((sweep_launch<double, true>(static_cast<const double*>(x) + o, stride, len, a, grid, mpart, hpart, stream)));
    else MFFT_TRY((sweep_launch<float, true>(static_cast<const float*>(x) + o, stride, len, a, grid, mpart, hpart, stream)));
    MFFT_TRY(moments_fold(mpart, waves, NLS_STATS, macc, stream));
    if (a.nbins > 0) MFFT_TRY(hist_fold(hpart, grid, 1, a.nbins, hacc, stream));
  }
  return 0;
}

// q[i] = (first ? 0 : q[i]) + (w r[i]) r[i] over the plan's real work array r (plan precision) and its array of doubles q
int mfft_plan_s::quad_accum(const void* r, double* q, size_t n, double w, bool first) {
  const unsigned grid = quad_grid(n);
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(quad_accum_kernel<double>, dim3(grid), dim3(QS_BLOCK), 0, stream, static_cast<const double*>(r), q, n, w, first ? 1 : 0);
  else
    hipLaunchKernelGGL(quad_accum_kernel<float>, dim3(grid), dim3(QS_BLOCK), 0, stream, static_cast<const float*>(r), q, n, w, first ? 1 : 0);
  MFFT_HIP(hipGetLastError());
  return 0;
}

extern "C" {

// out6 = [min, max, S1 .. S4] and, nbins > 0, counts[nbins + 3] of q = sum_c (w_c x_c) x_c over a real device array (ncomp, n).
// Synchronises the plan's stream.
int mfft_ew_quadratic(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* weights, double center, double lo,
                      double hi, int nbins, double* out6, int64_t* counts) {
  if (!plan || !x || !out6 || !weights || (nbins > 0 && !counts)) return set_error(MFFT_ERR_INVALID, "null argument");
  if (ncomp < 1 || ncomp > 6 || 6 % ncomp != 0) return set_error(MFFT_ERR_INVALID, "ncomp must be 1, 2, 3 or 6, not %d", ncomp);
  if (n < 1) return set_error(MFFT_ERR_INVALID, "empty array");
  if (precision != plan->prec) return set_error(MFFT_ERR_INVALID, "precision %d is not the plan's", precision);
  if (!isfinite(center)) return set_error(MFFT_ERR_INVALID, "the centre is not finite");
  double inv = 1.0;
  MFFT_TRY(quad_check(weights, ncomp, lo, hi, nbins, &inv));
  MFFT_TRY(plan->quad_begin(center, lo, inv, nbins));
  MFFT_TRY(plan->quad_sweep(x, precision == MFFT_DOUBLE, ncomp, n, n, weights, true));
  return plan->quad_end(out6, counts);
}

}  // extern "C"
