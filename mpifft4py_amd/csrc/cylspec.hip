// cylspec.hip -- (k_perp, k_z) sums of device-resident spectra (mfft_ew_cyl_sums, mfft_cyl_row_lists): the two-dimensional
// spectra of flows with one special direction (gravity, a mean field), for fields that no host copy can hold.
//
//   R[p, q] = sum over the local modes k with shell(kx^2 + ky^2) = p and |kz| = q of  h(k) w(k) sum_c Re(conj(a_c[k]) b_c[k])
//
// (the rule of include/mpifft4py_amd.h).  nperp x npar doubles do not fit a workgroup's LDS (725 x 513 at 1024^3: 3 MB), so this is
// no histogram.  The perp bin is constant along a memory row and the z bin is the position in the row: the result is a sum of ROWS
// grouped by a key the host knows in advance.  The host sorts the rows by (perp shell, l, j) once (`rows`, `row_start`); every
// shell's list is cut into segments of at most `seg` rows; a wave takes one (segment, run of 64 * VEC z positions), keeps one sum
// per lane and element in registers, in double, and walks the segment's rows in list order, 16 bytes per lane per load from one
// contiguous stretch of the row.  hz, ikz and kz^2 belong to the lane for the whole walk, so the loop is loads and fused
// multiply-adds: no shell rule, no shuffles, no LDS.  A run narrower than a wave -- the one element behind 8 x 64 of a row of
// N/2 + 1 = 513 -- is walked 64 / tw rows at a time (tw lanes per row, a power of two) and the lanes of one z position are added
// in a fixed butterfly at the end.  The wave stores its sums once, with plain stores, to its stretch of a (segments, s2) buffer of
// the plan; a second small kernel adds the segments of a shell in list order and then the positions of equal |kz| in memory order.
// No atomics on global memory, and the same bits from run to run for a given `seg`.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "plan_impl.h"

using namespace mfft;

namespace {

constexpr int CY_BLOCK = 256;            // four waves, one item each

// shell_of of shells.hip / _mesh.Block.shell_of, in integers only (host)
int64_t perp_shell(int64_t m) {
  if (m == 0) return 0;
  int64_t s = 1;
  while ((2 * s + 1) * (2 * s + 1) <= 4 * m) s *= 2;      // 4m < (2s+1)^2 now: the shell is in [s / 2, s]
  int64_t lo = s / 2 < 1 ? 1 : s / 2, hi = s;
  while (lo < hi) {                                        // the least s with 4m < (2s+1)^2
    const int64_t mid = (lo + hi) / 2;
    if ((2 * mid + 1) * (2 * mid + 1) <= 4 * m) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename T> struct Pair;                         // two consecutive complex values of single precision: one 16-byte load
template <> struct Pair<float> { typedef float4 type; };

struct CylArgs {
  const void *a, *b;
  const int32_t* rows;                 // the local rows l * s1 + j, sorted by (perp shell, l, j)
  const uint32_t *seg_start, *row_start;      // nperp + 1 each: a shell's first segment, its first entry of `rows`
  const int32_t* ikz;
  const uint8_t* hz;
  const void *kx, *ky, *kz;            // K2 kernels only
  uint32_t s1, s2, nrows;              // rows per x plane, row length, s0 * s1
  uint32_t nperp, npar, seg, nruns, nitems;
  int tail_ltw;                        // log2 of the lanes per row of a row's last run
  size_t n;                            // elements between components
  double* part;                        // (segments, s2)
  uint32_t* flag;                      // set when a mode's |kz| is >= npar, or a row of the list is not one of the block
};

// One step of the walk: U entries of the list per lane, rpw apart (the lanes of one row share an entry), every load issued before the
// first use.
template <typename T, int VEC, int NC, bool SAME, bool K2, int U>
__device__ __forceinline__ void cyl_step(const CylArgs& g, const int32_t* __restrict__ list, uint32_t i, uint32_t rpw, uint32_t kl,
                                         const bool (&live)[VEC], const double (&kz2)[VEC], double (&acc)[VEC]) {
  const cx<T>* __restrict__ A = static_cast<const cx<T>*>(g.a);
  const cx<T>* __restrict__ B = static_cast<const cx<T>*>(g.b);
  uint32_t row[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    ok[u] = true;
    row[u] = (uint32_t)list[i + (uint32_t)u * rpw];
    if (row[u] >= g.nrows) { *g.flag = 1u; row[u] = 0; ok[u] = false; }      // reported by the host; never a load out of range
  }
  cx<T> va[U][NC][VEC], vb[U][NC][VEC];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t f0 = (size_t)row[u] * g.s2 + kl;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if constexpr (VEC == 2) {
        typedef typename Pair<T>::type P;
        const P p = *reinterpret_cast<const P*>(A + c * g.n + f0);
        va[u][c][0] = mk<T>(p.x, p.y); va[u][c][1] = mk<T>(p.z, p.w);
        if constexpr (!SAME) {
          const P q = *reinterpret_cast<const P*>(B + c * g.n + f0);
          vb[u][c][0] = mk<T>(q.x, q.y); vb[u][c][1] = mk<T>(q.z, q.w);
        }
      } else {
        va[u][c][0] = A[c * g.n + f0];
        if constexpr (!SAME) vb[u][c][0] = B[c * g.n + f0];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    double w01 = 0.0;
    if constexpr (K2) {
      const uint32_t l = row[u] / g.s1, j = row[u] - l * g.s1;
      const double K0 = (double)static_cast<const T*>(g.kx)[l], K1 = (double)static_cast<const T*>(g.ky)[j];
      w01 = K0 * K0 + K1 * K1;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double d = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const cx<T> x = va[u][c][e], y = SAME ? va[u][c][e] : vb[u][c][e];
        d += (double)x.x * (double)y.x + (double)x.y * (double)y.y;
      }
      if constexpr (K2) d *= w01 + kz2[e];
      acc[e] += (ok[u] && live[e]) ? d : 0.0;          // a choice, not a product: what lies between pitched rows may be NaN
    }
  }
}

// rows of a step in flight per lane: about eight 16-byte loads, two rows at the least
constexpr int cyl_unroll(int nc, bool same) { return nc * (same ? 1 : 2) >= 3 ? 2 : 4; }

template <typename T, int VEC, int NC, bool SAME, bool K2>
__global__ __launch_bounds__(CY_BLOCK) void cyl_kernel(const CylArgs g) {
  constexpr int U = cyl_unroll(NC, SAME);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * (CY_BLOCK / 64) + (threadIdx.x >> 6));
  if (item >= g.nitems) return;
  const uint32_t sg = item / g.nruns, run = item - sg * g.nruns;          // the runs of a segment lie in neighbouring waves
  uint32_t lo = 0, hi = g.nperp;                                           // seg_start[lo] <= sg < seg_start[hi]: the segment's shell
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (g.seg_start[mid] <= sg) lo = mid; else hi = mid;
  }
  const uint32_t first = g.row_start[lo] + (sg - g.seg_start[lo]) * g.seg, left = g.row_start[lo + 1] - first;
  const uint32_t cnt = left < g.seg ? left : g.seg;                        // >= 1: the host counted this segment
  const int32_t* __restrict__ list = g.rows + first;
  const uint32_t ltw = run + 1 == g.nruns ? (uint32_t)g.tail_ltw : 6u;
  const uint32_t rpw = 64u >> ltw, r = lane >> ltw;
  const uint32_t k = run * (64 * VEC) + (lane & ((1u << ltw) - 1u)) * VEC;  // the lane's first z position
  const uint32_t kl = k < g.s2 ? k : 0u;                                   // where it loads from (VEC 2: s2 is even, k + 1 < s2 with k)
  bool live[VEC];
  double hw[VEC], kz2[VEC], acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const uint32_t ke = k + e;
    int h = ke < g.s2 ? (int)g.hz[ke] : 0;                                 // weight 0: skipped, whatever lies there
    if (h) {
      const int32_t z = g.ikz[ke];
      if ((uint32_t)(z < 0 ? -z : z) >= g.npar) { *g.flag = 1u; h = 0; }   // reported by the host; the fold never looks at this position
    }
    live[e] = h != 0;
    hw[e] = (double)h;
    kz2[e] = 0.0;
    if constexpr (K2) { if (h) { const double K2v = (double)static_cast<const T*>(g.kz)[ke]; kz2[e] = K2v * K2v; } }
    acc[e] = 0.0;
  }
  uint32_t i = r;
  for (; i + (U - 1) * rpw < cnt; i += U * rpw) cyl_step<T, VEC, NC, SAME, K2, U>(g, list, i, rpw, kl, live, kz2, acc);
  for (; i < cnt; i += rpw) cyl_step<T, VEC, NC, SAME, K2, 1>(g, list, i, rpw, kl, live, kz2, acc);
  // a narrow run: the lanes of one z position, 64 / rpw apart, in a fixed butterfly (every lane ends with the same sum)
  for (uint32_t o = 64u >> 1; o >= (1u << ltw) && o > 0; o >>= 1) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += __shfl_xor(acc[e], (int)o, 64);
  }
  if (r == 0) {
    double* __restrict__ out = g.part + (size_t)sg * g.s2;
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (k + e < g.s2) out[k + e] = hw[e] * acc[e];
  }
}

// result[p][q] for one perp shell p and CY_BLOCK z bins q per workgroup.  A chunk of z positions k at a time: the shell's segments at k
// are added in list order (0.0 for a shell without rows) into LDS next to the bin of k (|ikz[k]|, or -1 without weight); then every
// thread adds the positions of its own bin in memory order -- a choice per position, so the order is the same whatever the layout of z.
constexpr int CY_FOLD_K = 1024;
__global__ __launch_bounds__(CY_BLOCK) void cyl_fold_kernel(const double* __restrict__ part, const uint32_t* __restrict__ seg_start,
                                                            const int32_t* __restrict__ ikz, const uint8_t* __restrict__ hz, uint32_t s2,
                                                            uint32_t npar, double* __restrict__ result) {
  __shared__ double cl[CY_FOLD_K];
  __shared__ int32_t ql[CY_FOLD_K];
  const uint32_t p = blockIdx.x, sa = seg_start[p], sb = seg_start[p + 1];
  const int32_t q = (int32_t)(blockIdx.y * CY_BLOCK + threadIdx.x);
  double t = 0.0;
  for (uint32_t k0 = 0; k0 < s2; k0 += CY_FOLD_K) {
    const uint32_t nk = s2 - k0 < (uint32_t)CY_FOLD_K ? s2 - k0 : (uint32_t)CY_FOLD_K;
    __syncthreads();                                       // the chunk before this one has been read
    for (uint32_t k = threadIdx.x; k < nk; k += CY_BLOCK) {
      double c = 0.0;
      for (uint32_t sg = sa; sg < sb; ++sg) c += part[(size_t)sg * s2 + k0 + k];
      const int32_t z = ikz[k0 + k];
      cl[k] = c;
      ql[k] = hz[k0 + k] ? (z < 0 ? -z : z) : -1;
    }
    __syncthreads();
    for (uint32_t k = 0; k < nk; ++k) t += ql[k] == q ? cl[k] : 0.0;
  }
  if ((uint32_t)q < npar) result[(size_t)p * npar + (uint32_t)q] = t;
}

typedef void (*cyl_fn)(const CylArgs);
template <typename T, int VEC, int NC>
cyl_fn pick2(bool same, bool k2) {
  if (same) return k2 ? cyl_kernel<T, VEC, NC, true, true> : cyl_kernel<T, VEC, NC, true, false>;
  return k2 ? cyl_kernel<T, VEC, NC, false, true> : cyl_kernel<T, VEC, NC, false, false>;
}
template <typename T, int VEC>
cyl_fn pick(int ncomp, bool same, bool k2) { return ncomp == 1 ? pick2<T, VEC, 1>(same, k2) : pick2<T, VEC, 3>(same, k2); }

}  // namespace

extern "C" {

int mfft_cyl_row_lists(const int32_t* ikx_host, const int32_t* iky_host, int64_t s0, int64_t s1, int nperp, int32_t* rows_out,
                       int32_t* row_start_out) {
  if (!ikx_host || !iky_host || !rows_out || !row_start_out) return set_error(MFFT_ERR_INVALID, "null argument");
  if (s0 < 1 || s1 < 1 || nperp < 1) return set_error(MFFT_ERR_INVALID, "empty block");
  if (s0 >= (1ll << 31) / s1) return set_error(MFFT_ERR_UNSUPPORTED, "block too large for mfft_cyl_row_lists");
  std::vector<int32_t> sh((size_t)(s0 * s1));
  std::vector<int64_t> count((size_t)nperp + 1, 0);
  for (int64_t l = 0; l < s0; ++l)
    for (int64_t j = 0; j < s1; ++j) {
      const int64_t mx = ikx_host[l], my = iky_host[j], s = perp_shell(mx * mx + my * my);
      if (s >= nperp) return set_error(MFFT_ERR_INVALID, "mfft_cyl_row_lists: row (%lld, %lld) lies in perp shell %lld >= nperp = %d", (long long)l, (long long)j, (long long)s, nperp);
      sh[(size_t)(l * s1 + j)] = (int32_t)s;
      ++count[(size_t)s + 1];
    }
  for (int p = 0; p < nperp; ++p) count[(size_t)p + 1] += count[(size_t)p];
  for (int p = 0; p <= nperp; ++p) row_start_out[p] = (int32_t)count[(size_t)p];
  for (int64_t row = 0; row < s0 * s1; ++row) rows_out[count[(size_t)sh[(size_t)row]]++] = (int32_t)row;      // (l, j) order inside a shell
  return 0;
}

int mfft_ew_cyl_sums(mfft_plan_t plan, const void* a, const void* b, int ncomp, const int32_t* rows_dev, const int32_t* row_start_host,
                     int nperp, const int32_t* ikz, const uint8_t* hz, const void* kx, const void* ky, const void* kz, int k2,
                     const int64_t shape[3], int npar, int seg_rows, int precision, double* result_host) {
  if (!plan || !a || !b || !rows_dev || !row_start_host || !ikz || !hz || !shape || !result_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (k2 && (!kx || !ky || !kz)) return set_error(MFFT_ERR_INVALID, "k2 without the scaled wavenumber vectors");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  if (precision != MFFT_DOUBLE && precision != MFFT_SINGLE) return set_error(MFFT_ERR_INVALID, "unknown precision %d", precision);
  if (nperp < 1 || npar < 1) return set_error(MFFT_ERR_INVALID, "nperp and npar must be at least 1, not %d and %d", nperp, npar);
  if (seg_rows < 0) return set_error(MFFT_ERR_INVALID, "seg_rows must be 0 (the default) or positive, not %d", seg_rows);
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1) return set_error(MFFT_ERR_INVALID, "empty block");
  if (shape[2] >= (1ll << 31) || shape[0] >= (1ll << 31) / shape[1]) return set_error(MFFT_ERR_UNSUPPORTED, "block too large for mfft_ew_cyl_sums");
  const int64_t nrows = shape[0] * shape[1];
  const uint32_t seg = seg_rows ? (uint32_t)seg_rows : (uint32_t)MFFT_CYL_SEG_ROWS;
  // the tables of the launch: a shell's first segment and first list entry
  std::vector<uint32_t> tab(2 * ((size_t)nperp + 1));
  uint32_t* seg_start = tab.data();
  uint32_t* row_start = tab.data() + nperp + 1;
  if (row_start_host[0] != 0) return set_error(MFFT_ERR_INVALID, "row_start[0] must be 0, not %d", row_start_host[0]);
  uint64_t nseg = 0;
  for (int p = 0; p < nperp; ++p) {
    const int64_t len = (int64_t)row_start_host[p + 1] - (int64_t)row_start_host[p];
    if (len < 0) return set_error(MFFT_ERR_INVALID, "row_start is not monotone at shell %d", p);
    seg_start[p] = (uint32_t)nseg;
    row_start[p] = (uint32_t)row_start_host[p];
    nseg += ((uint64_t)len + seg - 1) / seg;
  }
  if ((int64_t)row_start_host[nperp] != nrows)
    return set_error(MFFT_ERR_INVALID, "row_start ends at %d, the block has %lld rows", row_start_host[nperp], (long long)nrows);
  seg_start[nperp] = (uint32_t)nseg;
  row_start[nperp] = (uint32_t)nrows;

  const size_t s2 = (size_t)shape[2], n = (size_t)nrows * s2;
  const bool same = a == b;
  // 16 bytes per lane: a cx<double> each, or two cx<float> where EVERY ROW starts at a multiple of 16 bytes
  const bool pairs = precision == MFFT_SINGLE && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && s2 % 2 == 0;
  const uint32_t per = pairs ? 128u : 64u, nruns = (uint32_t)((s2 + per - 1) / per);
  const uint64_t nitems = nseg * nruns;
  if (nitems >= (1ull << 31)) return set_error(MFFT_ERR_UNSUPPORTED, "block too large for mfft_ew_cyl_sums");
  const uint32_t tail_lanes = (uint32_t)((s2 - (size_t)(nruns - 1) * per + (pairs ? 1 : 0)) / (pairs ? 2 : 1));      // 1 .. 64
  int tail_ltw = 0;
  while ((1u << tail_ltw) < tail_lanes) ++tail_ltw;
  cyl_fn fn = precision == MFFT_DOUBLE ? pick<double, 1>(ncomp, same, k2 != 0)
                                       : (pairs ? pick<float, 2>(ncomp, same, k2 != 0) : pick<float, 1>(ncomp, same, k2 != 0));

  // the plan's buffer: (segments, s2) partial rows, the (nperp, npar) result, the flag, the two tables
  hipStream_t st = plan->stream;
  const size_t npart = (size_t)nseg * s2, nres = (size_t)nperp * (size_t)npar;
  MFFT_TRY(plan->ensure(plan->shl, (npart + nres + 1) * sizeof(double) + tab.size() * sizeof(uint32_t)));
  double* part = static_cast<double*>(plan->shl.p);
  double* result = part + npart;
  uint32_t* flag = reinterpret_cast<uint32_t*>(result + nres);
  uint32_t* dtab = flag + 2;
  MFFT_HIP(hipMemsetAsync(flag, 0, sizeof(double), st));
  MFFT_HIP(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CylArgs g;
  g.a = a; g.b = b; g.rows = rows_dev; g.seg_start = dtab; g.row_start = dtab + nperp + 1; g.ikz = ikz; g.hz = hz;
  g.kx = kx; g.ky = ky; g.kz = kz;
  g.s1 = (uint32_t)shape[1]; g.s2 = (uint32_t)s2; g.nrows = (uint32_t)nrows;
  g.nperp = (uint32_t)nperp; g.npar = (uint32_t)npar; g.seg = seg; g.nruns = nruns; g.nitems = (uint32_t)nitems;
  g.tail_ltw = tail_ltw; g.n = n; g.part = part; g.flag = flag;
  hipLaunchKernelGGL(fn, dim3((unsigned)((nitems + CY_BLOCK / 64 - 1) / (CY_BLOCK / 64))), dim3(CY_BLOCK), 0, st, g);
  MFFT_HIP(hipGetLastError());
  hipLaunchKernelGGL(cyl_fold_kernel, dim3((unsigned)nperp, (unsigned)((npar + CY_BLOCK - 1) / CY_BLOCK)), dim3(CY_BLOCK), 0, st, part, g.seg_start, ikz, hz, g.s2, g.npar, result);
  MFFT_HIP(hipGetLastError());
  uint32_t f = 0;
  MFFT_HIP(hipMemcpyAsync(&f, flag, sizeof f, hipMemcpyDeviceToHost, st));
  MFFT_HIP(hipStreamSynchronize(st));
  if (f) return set_error(MFFT_ERR_INVALID, "mfft_ew_cyl_sums: a mode of the block has |kz| >= npar = %d, or a row of the list is not one of the block's %lld", npar, (long long)nrows);
  MFFT_HIP(hipMemcpyAsync(result_host, result, nres * sizeof(double), hipMemcpyDeviceToHost, st));
  MFFT_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
