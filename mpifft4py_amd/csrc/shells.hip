// shells.hip -- shell-binned sums of device-resident spectra (mfft_ew_shell_sums): the energy, transfer, enstrophy and
// variance spectra a DNS is looked at through, for fields that no host copy can hold.
//
//   S[s] = sum over the local modes k with shell(k) = s of  h(k) w(k) sum_c Re(conj(a_c[k]) b_c[k])
//
// shell(k) is the integer nearest to |k|, decided in integers: 0 for m = kx^2 + ky^2 + kz^2 = 0, else the s >= 1 with
// (2s-1)^2 <= 4m < (2s+1)^2 (a float sqrt only proposes s), so host and device can never bin a mode differently.
//
// One streaming sweep over the block as ONE flat run of elements: a wave takes 64 (fp64) or 128 (fp32) consecutive ones,
// 16 bytes per lane per load, wherever the rows end; kx^2 + ky^2 is fixed along a row, so neighbouring lanes mostly share a
// shell.  (fp32 pairs need 16-byte aligned fields and an even component size; else 8 bytes per lane.)  The components are summed in
// registers, runs of equal shell are summed inside the wave (six shuffle steps of a segmented reduction), and only the head
// of a run adds to the workgroup's LDS histogram (one ds_add_f64, no compare-and-swap loop on gfx950).  Every workgroup
// stores its histogram with plain stores to its row of a (grid, nshell) buffer of the plan and a second small kernel sums
// the rows in fixed order: no global atomics.  Products and sums are in double whatever the fields' precision.
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>
#include "plan_impl.h"

using namespace mfft;

namespace {

constexpr int SH_BLOCK = 256;            // four waves
constexpr int SH_WG_PER_CU = 4;          // upper bound of resident workgroups per CU the grid is sized for
constexpr int SH_MAX_LDS = 64 * 1024;    // bytes of histogram a workgroup can hold

__device__ __forceinline__ int shell_of(int64_t m) {
  if (m == 0) return 0;
  int64_t s = (int64_t)floorf(sqrtf((float)m) + 0.5f);
  if (s < 1) s = 1;
  while ((2 * s - 1) * (2 * s - 1) > 4 * m) --s;      // never below 1: 1 <= 4m
  while ((2 * s + 1) * (2 * s + 1) <= 4 * m) ++s;
  return (int)s;
}

template <typename T> struct Pair;                     // two consecutive complex values of single precision: one 16-byte load
template <> struct Pair<float> { typedef float4 type; };

struct ShellArgs {
  const void *a, *b;
  const int32_t *ikx, *iky, *ikz;
  const uint8_t* hz;
  const void *kx, *ky, *kz;            // null: w = 1
  uint32_t s1, s2, nchunks;            // rows per x plane, row length, wave-sized chunks of the flat block
  uint32_t dl, dj, dk;                 // (x, y, z) position of a chunk's first element advances by this from one of a wave's chunks to its next
  size_t n;                            // elements of the block = elements between components
  int nshell;
  double* part;                        // (grid, nshell)
  uint32_t* flag;                      // set when a mode's shell is >= nshell
};

// The block is ONE flat run of n elements: a wave takes 64 * VEC consecutive ones per chunk, wherever the rows end (a row
// of N/2 + 1 elements cut into chunks of its own would leave a chunk with one live lane behind every row).  The position
// (l, j, k) of a chunk's first element is wave-uniform and advances by additions; a lane steps from it to its own row.
// VEC: elements per lane (2: fp32 with 16-byte loads; chunks start at even elements, so every pair is 16-byte aligned where
// the components are, and the block's last pair is loaded element by element when n is odd)
template <typename T, int VEC, int NC, bool SAME>
__global__ __launch_bounds__(SH_BLOCK) void shell_kernel(const ShellArgs g) {
  extern __shared__ double hist[];
  for (int i = threadIdx.x; i < g.nshell; i += SH_BLOCK) hist[i] = 0.0;
  __syncthreads();
  const cx<T>* __restrict__ A = static_cast<const cx<T>*>(g.a);
  const cx<T>* __restrict__ B = static_cast<const cx<T>*>(g.b);
  const T* __restrict__ kxs = static_cast<const T*>(g.kx);
  const T* __restrict__ kys = static_cast<const T*>(g.ky);
  const T* __restrict__ kzs = static_cast<const T*>(g.kz);
  const bool k2 = g.kz != nullptr;
  const int lane = threadIdx.x & 63;
  const uint32_t nwaves = gridDim.x * (SH_BLOCK / 64);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SH_BLOCK / 64) + (threadIdx.x >> 6));
  // the first chunk's position, by division once; after that by the strides the host worked out
  const uint64_t first = (uint64_t)wave * (64 * VEC), row0 = first / g.s2;
  uint32_t wk = (uint32_t)(first - row0 * g.s2), wl = (uint32_t)(row0 / g.s1), wj = (uint32_t)(row0 - (uint64_t)wl * g.s1);
  for (uint32_t it = wave; it < g.nchunks; it += nwaves) {
    const size_t f0 = (size_t)it * (64 * VEC) + (size_t)(lane * VEC);     // the lane's first element in the flat block
    cx<T> va[NC][VEC], vb[NC][VEC];
    bool ok[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) ok[e] = f0 + e < g.n;
    if constexpr (VEC == 2) {
      if (ok[1]) {
        typedef typename Pair<T>::type P;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const P p = *reinterpret_cast<const P*>(A + c * g.n + f0);
          va[c][0] = mk<T>(p.x, p.y); va[c][1] = mk<T>(p.z, p.w);
          if constexpr (!SAME) {
            const P q = *reinterpret_cast<const P*>(B + c * g.n + f0);
            vb[c][0] = mk<T>(q.x, q.y); vb[c][1] = mk<T>(q.z, q.w);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          va[c][0] = ok[0] ? A[c * g.n + f0] : mk<T>(0, 0); va[c][1] = mk<T>(0, 0);
          if constexpr (!SAME) { vb[c][0] = ok[0] ? B[c * g.n + f0] : mk<T>(0, 0); vb[c][1] = mk<T>(0, 0); }
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        va[c][0] = ok[0] ? A[c * g.n + f0] : mk<T>(0, 0);
        if constexpr (!SAME) vb[c][0] = ok[0] ? B[c * g.n + f0] : mk<T>(0, 0);
      }
    }
    // the lane's own (l, j, k): rows of 64 * VEC elements or more are left at most once
    uint32_t l = wl, j = wj, k = wk + (uint32_t)(lane * VEC);
    while (k >= g.s2) {
      k -= g.s2;
      if (++j == g.s1) { j = 0; ++l; }
    }
    int sh[VEC];
    double val[VEC];
    int64_t m01 = 0;
    double w01 = 0.0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      sh[e] = -1;                        // no element, or weight 0: skipped, whatever lies there (NaN between pitched rows)
      val[e] = 0.0;
      if (e > 0) {                       // the lane's second element: the next one of the row, or the first of the next row
        if (++k == g.s2) { k = 0; if (++j == g.s1) { j = 0; ++l; } }
      }
      if (ok[e]) {
        if (e == 0 || k == 0) {          // (l, j) are inside the block wherever ok[e] holds
          const int64_t mx = g.ikx[l], my = g.iky[j];
          m01 = mx * mx + my * my;
          if (k2) { const double K0 = (double)kxs[l], K1 = (double)kys[j]; w01 = K0 * K0 + K1 * K1; }
        }
        const int h = (int)g.hz[k];
        if (h) {
          const int64_t mz = g.ikz[k];
          const int s = shell_of(m01 + mz * mz);
          if (s >= g.nshell) {
            *g.flag = 1u;                // reported by the host; never an LDS write out of range
          } else {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const cx<T> x = va[c][e], y = SAME ? va[c][e] : vb[c][e];
              d += (double)x.x * (double)y.x + (double)x.y * (double)y.y;
            }
            double w = (double)h;
            if (k2) { const double K2 = (double)kzs[k]; w *= w01 + K2 * K2; }
            sh[e] = s;
            val[e] = w * d;
          }
        }
      }
    }
    int s = sh[0];
    double v = val[0];
    if constexpr (VEC == 2) {            // the lane's two elements: one shell mostly; else the first one goes to LDS by itself
      if (sh[1] < 0) { /* keep the first */ }
      else if (sh[0] < 0 || sh[0] == sh[1]) { s = sh[1]; v = val[0] + val[1]; }
      else { atomicAdd(&hist[sh[0]], val[0]); s = sh[1]; v = val[1]; }
    }
    // segmented reduction over runs of equal shell: a run's head ends up with the run's sum
    const int sprev = __shfl_up(s, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || s != sprev);
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);
    const int end = above ? __builtin_ctzll(above) : 64;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_down(v, o, 64);
      if (lane + o < end) v += t;
    }
    if (((heads >> lane) & 1ull) && s >= 0) atomicAdd(&hist[s], v);
    // the wave's next chunk: nwaves * 64 * VEC elements on, as (dl, dj, dk) with dj < s1, dk < s2
    wk += g.dk;
    wj += g.dj;
    if (wk >= g.s2) { wk -= g.s2; ++wj; }
    if (wj >= g.s1) { wj -= g.s1; ++wl; }
    wl += g.dl;
  }
  __syncthreads();
  double* __restrict__ out = g.part + (size_t)blockIdx.x * g.nshell;
  for (int i = threadIdx.x; i < g.nshell; i += SH_BLOCK) out[i] = hist[i];
}

// result[s] = sum over the workgroups' histograms, in fixed order: eight interleaved partial sums per shell, then those
__global__ __launch_bounds__(SH_BLOCK) void shell_sum_kernel(const double* __restrict__ part, int ngrid, int nshell, double* __restrict__ result) {
  __shared__ double red[SH_BLOCK / 32][32];
  const int sx = threadIdx.x & 31, gy = threadIdx.x >> 5;
  const int s = blockIdx.x * 32 + sx;
  double acc = 0.0;
  if (s < nshell)
    for (int w = gy; w < ngrid; w += SH_BLOCK / 32) acc += part[(size_t)w * nshell + s];
  red[gy][sx] = acc;
  __syncthreads();
  if (gy == 0 && s < nshell) {
    double t = 0.0;
    for (int w = 0; w < SH_BLOCK / 32; ++w) t += red[w][sx];
    result[s] = t;
  }
}

typedef void (*shell_fn)(const ShellArgs);
template <typename T, int VEC>
shell_fn pick(int ncomp, bool same) {
  if (ncomp == 1) return same ? shell_kernel<T, VEC, 1, true> : shell_kernel<T, VEC, 1, false>;
  return same ? shell_kernel<T, VEC, 3, true> : shell_kernel<T, VEC, 3, false>;
}

// CUs x min(occupancy, SH_WG_PER_CU) of a kernel variant with `lds` bytes of histogram, asked of the runtime once per
// (device, variant, lds): a small mesh diagnosed every step should not pay three runtime queries per call
int resident_workgroups(shell_fn fn, size_t lds, int* cap) {
  struct Key { int dev; shell_fn fn; size_t lds; int cap; };
  static std::mutex mu;
  static std::vector<Key> known;
  int dev = 0;
  MFFT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  for (const Key& k : known)
    if (k.dev == dev && k.fn == fn && k.lds == lds) { *cap = k.cap; return 0; }
  int ncu = 0, occ = 0;
  MFFT_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  MFFT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(fn), SH_BLOCK, lds));
  if (occ < 1 || ncu < 1) return set_error(MFFT_ERR_INTERNAL, "mfft_ew_shell_sums: no resident workgroup (%d CUs, %d per CU)", ncu, occ);
  *cap = ncu * (occ < SH_WG_PER_CU ? occ : SH_WG_PER_CU);
  known.push_back(Key{dev, fn, lds, *cap});
  return 0;
}

}  // namespace

extern "C" {

int mfft_ew_shell_sums(mfft_plan_t plan, const void* a, const void* b, int ncomp, const int32_t* ikx, const int32_t* iky,
                       const int32_t* ikz, const uint8_t* hz, const void* kx, const void* ky, const void* kz, int k2,
                       const int64_t shape[3], int nshell, int precision, double* result_host) {
  if (!plan || !a || !b || !ikx || !iky || !ikz || !hz || !shape || !result_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if (k2 && (!kx || !ky || !kz)) return set_error(MFFT_ERR_INVALID, "k2 without the scaled wavenumber vectors");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  if (precision != MFFT_DOUBLE && precision != MFFT_SINGLE) return set_error(MFFT_ERR_INVALID, "unknown precision %d", precision);
  if (nshell < 1) return set_error(MFFT_ERR_INVALID, "nshell must be at least 1, not %d", nshell);
  if ((size_t)nshell * sizeof(double) > (size_t)SH_MAX_LDS)
    return set_error(MFFT_ERR_UNSUPPORTED, "%d shells: the workgroup histogram holds at most %d", nshell, SH_MAX_LDS / (int)sizeof(double));
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1) return set_error(MFFT_ERR_INVALID, "empty block");
  const size_t n = (size_t)shape[0] * (size_t)shape[1] * (size_t)shape[2];
  const bool same = a == b;
  // 16 bytes per lane: a cx<double> each, or two cx<float> where every component starts at an even element
  const bool pairs = precision == MFFT_SINGLE && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && (ncomp == 1 || n % 2 == 0);
  const int vec = pairs ? 2 : 1;
  const uint64_t per = 64 * (uint64_t)vec, nchunks = ((uint64_t)n + per - 1) / per;
  if (shape[1] >= (1ll << 31) || shape[2] >= (1ll << 31) || nchunks >= (1ull << 31)) return set_error(MFFT_ERR_UNSUPPORTED, "block too large for mfft_ew_shell_sums");
  shell_fn fn = precision == MFFT_DOUBLE ? pick<double, 1>(ncomp, same) : (pairs ? pick<float, 2>(ncomp, same) : pick<float, 1>(ncomp, same));

  hipStream_t st = plan->stream;
  const size_t lds = (size_t)nshell * sizeof(double);
  int cap = 0;
  MFFT_TRY(resident_workgroups(fn, lds, &cap));
  const uint64_t want = (nchunks + SH_BLOCK / 64 - 1) / (SH_BLOCK / 64);
  const int grid = (int)(want < (uint64_t)cap ? want : (uint64_t)cap);
  const uint64_t stride = (uint64_t)grid * (SH_BLOCK / 64) * per, drow = stride / (uint64_t)shape[2];

  // the plan's buffer: (grid, nshell) histograms, the nshell results, the flag
  MFFT_TRY(plan->ensure(plan->shl, ((size_t)grid + 1) * lds + sizeof(double)));
  double* part = static_cast<double*>(plan->shl.p);
  double* result = part + (size_t)grid * nshell;
  uint32_t* flag = reinterpret_cast<uint32_t*>(result + nshell);
  MFFT_HIP(hipMemsetAsync(flag, 0, sizeof(double), st));
  ShellArgs g;
  g.a = a; g.b = b; g.ikx = ikx; g.iky = iky; g.ikz = ikz; g.hz = hz;
  g.kx = k2 ? kx : nullptr; g.ky = k2 ? ky : nullptr; g.kz = k2 ? kz : nullptr;
  g.s1 = (uint32_t)shape[1]; g.s2 = (uint32_t)shape[2]; g.nchunks = (uint32_t)nchunks;
  g.dl = (uint32_t)(drow / (uint64_t)shape[1]); g.dj = (uint32_t)(drow % (uint64_t)shape[1]); g.dk = (uint32_t)(stride % (uint64_t)shape[2]);
  g.n = n; g.nshell = nshell; g.part = part; g.flag = flag;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(SH_BLOCK), lds, st, g);
  MFFT_HIP(hipGetLastError());
  hipLaunchKernelGGL(shell_sum_kernel, dim3((nshell + 31) / 32), dim3(SH_BLOCK), 0, st, part, grid, nshell, result);
  MFFT_HIP(hipGetLastError());
  std::vector<double> host((size_t)nshell + 1);
  MFFT_HIP(hipMemcpyAsync(host.data(), result, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  MFFT_HIP(hipStreamSynchronize(st));
  uint32_t f = 0;
  memcpy(&f, &host[nshell], sizeof f);
  if (f) return set_error(MFFT_ERR_INVALID, "mfft_ew_shell_sums: a mode of the block lies in a shell >= nshell = %d", nshell);
  memcpy(result_host, host.data(), (size_t)nshell * sizeof(double));
  return 0;
}

}  // extern "C"
