// fft_nlz.h -- the fused NONLINEAR z stage of a pseudo-spectral step (round 6).
//
// What the reference's demo does per Runge-Kutta stage (demo/spectral_dns_solver.py:53-71):
//     for i in 0..2: U[i]    = ifftn(U_hat[i])          three inverse transforms
//     for i in 0..2: curl[i] = ifftn(i K x U_hat)       three more
//     U x curl                                          in real space
//     for i in 0..2: dU[i]   = fftn((U x curl)[i])      three forward transforms
// In a slab / pencil transform the z axis is the last inverse stage and the first forward stage and it is local to a
// rank (slab.py:214-346, 349-485: irfft / rfft along axis 2), so the nine real work arrays exist only between the two
// z stages.  This kernel takes one (x, y) row of the SIX half-spectra (x and y already transformed back), produces the six
// real rows in registers, forms the cross product there and transforms the three result rows forward again: the real
// arrays -- at 1024^3 with the 3/2-rule 9 x 1536^3 x 8 B = 261 GB -- never exist, and the z stages move 9 complex rows per
// (x, y) instead of 9 complex + 27 real ones.
//
// Arithmetic.  Two real transforms ride on ONE complex transform of the full length M (no split pre- / post-pass with its
// twiddles): with A, B the Hermitian extensions of two half-spectra, the inverse DFT of Z = A + iB is a + ib; forward, the
// DFT of ra + i rb splits into Ra[k] = (Z[k] + conj Z[M-k]) / 2, Rb[k] = -i (Z[k] - conj Z[M-k]) / 2.  Per row: three
// inverse transforms (a_f + i b_f, f = 0..2) and one and a half forward ones -- r0 + i r1 of the row, and r2 of TWO
// consecutive rows together, which is why a thread group works through its rows in pairs.  4.5 transforms of length M per
// row, the minimum for nine real ones.
//
// Registers.  Thread j of a row holds positions j + k TPT (fft_core.h), the same for every field, so the cross product
// needs no exchange at all: two of the three inverse results are parked in 2 E complex registers while the third is
// computed, r2 of the first row of a pair in E more reals.  S is the COMPLEX plan of length M; `valid` (runtime) is the
// number of bins a row holds in memory (M/2 + 1, or N/2 + 1 of the un-padded mesh for the 3/2-rule: the rest reads as zero
// and is not stored -- what C2RFft / R2CFft LIMIT do).
#pragma once
#include <type_traits>
#include "fft_kernels.h"

namespace mfft {

template <typename T>
struct NlzParams {
  const cx<T>* a[3];           // half-spectra rows of the first vector field (x and y already in real space)
  const cx<T>* b[3];           // ... of the second
  cx<T>* out[3];               // half-spectra rows of (a x b); may alias a[] / b[] row for row
  const cx<T>* tw;             // inter-pass twiddles of S
  i64 in_stride, out_stride;   // complex elements between consecutive rows
  i64 nrows;
  int valid;                   // bins per OUTPUT row that are stored (and exist in memory)
  int valid_in;                // bins per INPUT row that exist (<= valid: the pruned 2/3-rule reads the kept kz only)
  T scale;                     // applied to a x b (both inverse transforms are un-normalised: 1 / M^2 gives numpy's irfft)
  const cx<T>* rt3;            // Nlz3Fft: exp(+2 pi i k / M), k = 0..L, then exp(+2 pi i 2k / M), k = 0..L   (M = 3 L)
};
// ... of the kernels that also emit max |a_f|, max |b_f| of the real rows (NlzAbsMax below).  A derived struct: a new field of
// NlzParams would be an argument of every existing kernel.
template <typename T>
struct NlmParams : NlzParams<T> {
  T* part;                     // (waves of the launch, 2 rows of a pair, [a, b], 3 fields) un-normalised maxima, every slot written
};
constexpr int NLM_SLOTS = 12;  // values per wave in NlmParams::part
// ... of the kernel that forms a x b AND sum_f a_f c_f (NlzFft::body_cross_dot below): a third field in, a fourth row out
template <typename T>
struct NlcParams : NlzParams<T> {
  const cx<T>* c[3];           // half-spectra rows of the third vector field, strides and valid_in as a[] / b[]
  cx<T>* outs;                 // half-spectra rows of sum_f a_f c_f; may alias one a[] / b[] / c[] component out[] does not take
};
// ... of the kernel that forms all NINE products a_i b_j (NlzFft::body_outer below): six rows in, nine out -- the first product with
// more rows out than in.  out[] is not used.
template <typename T>
struct NloParams : NlzParams<T> {
  cx<T>* out9[9];              // half-spectra rows of a_i b_j at 3 i + j; [0..2] may alias a[0..2], [3..5] b[0..2], row for row
};

// ... of the kernel that ends in a REDUCTION instead of a product (NlzFft::body_moments below): min, max and the sums of the first
// four powers of up to six real fields.  Pair p is a[p] + i b[p] on one complex transform, p < npairs; b[p] may be null (an odd
// field count: the partner reads as zeros and its statistics mean nothing).  out[], scale and valid are not used.
constexpr int NLS_PAIRS = 3, NLS_STATS = 6;                     // per field: min, max, S1 .. S4
constexpr int NLS_SLOTS = 2 * NLS_PAIRS * NLS_STATS;            // doubles per wave in NlsParams::part: [pair][a, b][statistic]
template <typename T>
struct NlsParams : NlzParams<T> {
  double* part;                // (waves of the launch, NLS_SLOTS) partial statistics, every slot written
  double center[2 * NLS_PAIRS];   // [pair][a, b]: S_p = sum (x - center)^p, x the normalised value
  double norm;                 // x = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};

// ... of the kernel that ends in a HISTOGRAM (NlzFft::body_hist below): counts of the values of up to six real fields in nbins
// equal bins over [lo, hi) of each field.  Pairs as in NlsParams.  Per field nbins + 3 slots: [0] below lo, [1 .. nbins] the bins,
// [nbins + 1] at or above hi, [nbins + 2] not finite (hist_slot below: the ONE rule of host, sweep, kernel and tests).
constexpr int NLH_MAXBINS = 512;                                // bins per field a workgroup's LDS histograms hold
template <typename T>
struct NlhParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, 2, nbins + 3) counts, every slot of the launch's pairs written
  double lo[2 * NLS_PAIRS];    // [pair][a, b]: the lower edge of the field's first bin
  double inv[2 * NLS_PAIRS];   // ... and nbins / (hi - lo), formed once on the host
  double norm;                 // x = norm * (the un-normalised result of the inverse transform)
  int nbins;                   // 1 .. NLH_MAXBINS
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The slot of a value.  NaN first, before any cast; the upper end compared BEFORE the cast to int (an Inf or a huge t never
// reaches it); a subtraction, then a multiplication: nothing for the compiler to contract, so host and device agree to the bit.
// The result is clamped once more: no index reaches LDS or memory on the strength of the caller's lo and inv alone.
MFFT_D int hist_slot(double x, double lo, double inv, int nbins) {
  const double t = (x - lo) * inv;
  const int s = x != x ? nbins + 2 : t < 0.0 ? 0 : t >= (double)nbins ? nbins + 1 : 1 + (int)t;
  return s < 0 ? 0 : s > nbins + 2 ? nbins + 2 : s;
}
// one count into a workgroup's LDS histogram: an atomic add whose result nobody reads (ds_add_u32); the emulator's threads are
// fibres of one host thread, a plain add there
#if defined(__HIPCC__)
#define MFFT_LDS_COUNT(p) ((void)atomicAdd((p), 1u))
#else
#define MFFT_LDS_COUNT(p) ((void)(*(p) += 1u))
#endif
// The same with runs of equal slot merged inside the wave first (NlzHist MERGE; the build that was measured against the plain add,
// profiles/real_histogram_ab.txt): neighbouring lanes hold neighbouring z positions, a smooth field puts whole runs of them into
// one slot and the LDS serialises those adds.  Every lane contributes ONE, so a run's sum is its length: the head of a run (its
// slot differs from the lane's before it) adds the distance to the next head -- one shuffle and one ballot, no reduction tree, the
// head-and-ballot scheme of shells.hip.  EVERY lane of the wave calls it (s < 0: the lane counts nothing and breaks a run).
#if defined(__HIPCC__)
MFFT_D void lds_count_runs(unsigned* hist, int s, int lane) {
  const int sprev = __shfl_up(s, 1, 64);
  const unsigned long long live = __ballot(1), heads = __ballot(lane == 0 || s != sprev);
  const unsigned long long above = heads & ~((2ull << lane) - 1ull);
  const int end = above ? __builtin_ctzll(above) : __builtin_popcountll(live);      // (a workgroup's last wave may be short)
  if (((heads >> lane) & 1ull) && s >= 0) (void)atomicAdd(hist + s, (unsigned)(end - lane));
}
#else
MFFT_D void lds_count_runs(unsigned* hist, int s, int lane) {
  if (s >= 0) hist[s] += 1u;
}
#endif

// ... of the kernel that ends in a JOINT HISTOGRAM (NlzFft::body_joint below): the two fields of a pair ride one transform, so one
// thread holds both real values of a grid point; it counts the point into ONE cell of a two-dimensional grid.  Per pair
// (nba + 3) x (nbb + 3) cells, cell = sa * (nbb + 3) + sb with sa, sb the fields' slots by hist_slot (joint_cell below: the ONE
// rule of host, sweep, kernel and tests).  Every pair has both fields: a pair without a partner is an error on the host.
constexpr int NLJ_MAXBINS = 64;                                 // bins per field: (64 + 3)^2 cells are what a workgroup's LDS holds
constexpr int NLJ_MAXCELLS = (NLJ_MAXBINS + 3) * (NLJ_MAXBINS + 3);      // 4489 cells, 17956 bytes
template <typename T>
struct NljParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, (nba + 3)(nbb + 3)) counts, every cell of the launch's pairs written
  double lo[2 * NLS_PAIRS];    // [pair][a, b]: the lower edge of the field's first bin
  double inv[2 * NLS_PAIRS];   // ... and nb / (hi - lo) of the field, formed once on the host
  double norm;                 // x = norm * (the un-normalised result of the inverse transform)
  int nba, nbb;                // 1 .. NLJ_MAXBINS each: the bins of the a fields and of the b fields
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The cell of a pair of slots.  hist_slot clamps each slot to its nb + 2; the product is clamped once more to the grid that the
// kernel reserves, so that no LDS index rests on the caller's bin counts alone.
MFFT_D int joint_cell(int sa, int sb, int nbb) {
  const int c = sa * (nbb + 3) + sb;
  return c < 0 ? 0 : c > NLJ_MAXCELLS - 1 ? NLJ_MAXCELLS - 1 : c;
}

// ... of the kernel that ends in the statistics of a QUADRATIC FORM of its fields (NlzFft::body_quad below): q = sum_f w_f r_f^2 over
// up to six real fields r_f -- enstrophy, dissipation, energy density -- reduced to [min, max, S1 .. S4] about `center` and, with
// nbins > 0, counted in nbins equal bins of [lo, hi) (hist_slot).  Pairs as in NlsParams; w in slot order, [pair][a, b].
template <typename T>
struct NlqParams : NlzParams<T> {
  double* mpart;               // (waves of the launch, NLS_STATS) partial statistics of q, every slot written
  unsigned* hpart;             // (workgroups of the launch, nbins + 3) counts of q, every slot written (zeros where nbins == 0)
  double w[2 * NLS_PAIRS];     // [pair][a, b]: the weight of the field's square; 0 where the pair has no partner
  double center;               // S_p = sum (q - center)^p
  double norm;                 // r = norm * (the un-normalised result of the inverse transform)
  double lo, inv;              // the lower edge of the first bin and nbins / (hi - lo), formed once on the host
  int nbins;                   // 0 .. NLH_MAXBINS; 0: no histogram
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The evaluation rule of q (include/mpifft4py_amd.h states it): every product and every sum rounded on its own, in double.  hipcc
// contracts a * b + c into an FMA by default, which rounds once -- the host, numpy and the emulator round twice.  HIP's __dmul_rn
// and __dadd_rn are a plain `*` and `+` in this toolchain's headers and would be contracted all the same once inlined, so the two
// operations are compiled with contraction off instead (the pragma takes the `contract` flag off the instruction itself, wherever
// it is inlined; checked in the kernels' code: v_mul_f64 and v_add_f64, no v_fma_f64 in the accumulation of q).  The emulator is
// built with -ffp-contract=off (Makefile).
MFFT_D double quad_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
MFFT_D double quad_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
// q + (w r) r: one field's term
MFFT_D double quad_term(double q, double w, double r) { return quad_add(q, quad_mul(quad_mul(w, r), r)); }

// ... of the kernel that ends in STRUCTURE FUNCTIONS (NlzFft::body_incr below): the sums of the second, third and fourth powers of
// the increments along z, d = r(z + s) - r(z), of up to six real fields for up to NLI_MAXSEP separations s -- the first two-point
// statistic.  Pairs as in NlsParams.  Per field and separation NLI_STATS sums: S2, S3, S4 (S1 is zero on a periodic row).
constexpr int NLI_MAXSEP = 8, NLI_STATS = 3;                    // separations per launch (include/mpifft4py_amd.h MFFT_INCR_MAXSEP)
constexpr int NLI_FIELD = NLI_MAXSEP * NLI_STATS;               // doubles per field: [separation][S2, S3, S4]
constexpr int NLI_SLOTS = 2 * NLS_PAIRS * NLI_FIELD;            // doubles per wave in NliParams::part: [pair][a, b][separation][sum]
template <typename T>
struct NliParams : NlzParams<T> {
  double* part;                // (waves of the launch, NLI_SLOTS) partial sums, every slot written (zeros where nothing was added)
  double norm;                 // r = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int sep[NLI_MAXSEP];         // 1 <= sep[i] <= M - 1, in grid points of the row, i < nsep; duplicates allowed
  int nsep;                    // 1 .. NLI_MAXSEP
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The rule of the increments (include/mpifft4py_amd.h states it; kernel, sweep, emulator and tests share it): the value in the
// rows' precision taken to double and normalised THERE -- one rounded product, never contracted into the difference --, the
// difference, its powers and the sums in double.
MFFT_D double incr_value(double x, double norm) { return quad_mul(x, norm); }
MFFT_D void incr_add(double* m, double r1, double r0) {      // m: the NLI_STATS sums of one field and separation
  const double d = r1 - r0, d2 = d * d;
  m[0] += d2;
  m[1] += d2 * d;
  m[2] += d2 * d2;
}
// position (pos + s) mod M of a periodic row, 0 <= pos < M, 1 <= s < M
MFFT_D int incr_pos(int pos, int s, int M) {
  const int q = pos + s;
  return q >= M ? q - M : q;
}

// ... of the kernel that ends in INCREMENT HISTOGRAMS (NlzFft::body_incr_hist below): the counts of the increments along z,
// d = r(z + s) - r(z), of up to six real fields for up to NLI_MAXSEP separations s, in nbins equal bins over a range of its own per
// field and separation.  Pairs as in NlsParams.  The ONE rule (include/mpifft4py_amd.h states it; kernel, sweep, emulator, numpy and
// tests share it): r = incr_value((double)x, norm), d = r(pos + s mod M) - r(pos) in double, slot = hist_slot(d, lo, inv, nbins).  Per
// field and separation nbins + 3 slots, as in NlhParams.
constexpr int NLK_MAXBINS = 256;                                // bins per field and separation (MFFT_INCR_HIST_MAXBINS)
constexpr int NLK_MAXCELLS = 2 * NLI_MAXSEP * (NLK_MAXBINS + 3);      // 4144 counts, 16576 bytes: a pair's histograms in LDS
static_assert(NLK_MAXCELLS <= NLJ_MAXCELLS, "the increment histograms take the joint kernels' exchange rule: they fit under its grid");
template <typename T>
struct NlkParams : NlzParams<T> {
  unsigned* part;              // (workgroups of the launch, npairs, 2, nsep, nbins + 3) counts, every slot of the launch's pairs written
  double lo[2 * NLS_PAIRS][NLI_MAXSEP];    // [pair][a, b][separation]: the lower edge of the first bin
  double inv[2 * NLS_PAIRS][NLI_MAXSEP];   // ... and nbins / (hi - lo), formed once on the host
  double norm;                 // r = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int sep[NLI_MAXSEP];         // 1 <= sep[i] <= M - 1, in grid points of the row, i < nsep; duplicates allowed
  int nsep;                    // 1 .. NLI_MAXSEP
  int nbins;                   // 1 .. NLK_MAXBINS
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The count of one increment.  hist_slot clamps the slot to nbins + 2; the cell of (field of the pair, separation, slot) is clamped
// once more to what the kernel reserves, so that no LDS index rests on the caller's nbins, nsep or separations alone.
MFFT_D int incr_hist_cell(int f, int i, int nsep, int nb3, int slot) {
  const int c = (f * nsep + i) * nb3 + slot;
  return c < 0 ? 0 : c > NLK_MAXCELLS - 1 ? NLK_MAXCELLS - 1 : c;
}
MFFT_D int incr_hist_slot(double r1, double r0, double lo, double inv, int nbins) { return hist_slot(r1 - r0, lo, inv, nbins); }

// ... of the kernel that ends in plane-averaged PROFILES along z (NlzFft::body_prof below): per pair (a_p, b_p) and per position m
// of the row NLP_STATS sums over all rows -- a row is one (x, y) point, so a sum over the rows at a fixed position is a sum over
// the plane z = m.  The first reduction whose result is a vector in z.  Every pair has both fields, as in NljParams.
constexpr int NLP_STATS = 5;                                    // per pair and position: d_a, d_b, d_a^2, d_b^2, d_a d_b (MFFT_PROFILE_STATS)
template <typename T>
struct NlpParams : NlzParams<T> {
  double* part;                // (ngroups x ROWS row slots, npairs, NLP_STATS, M) partial profiles, every slot written
  double center[2 * NLS_PAIRS];   // [pair][a, b]: d = x - center, x the normalised value
  double norm;                 // x = norm * (the un-normalised result of the inverse transform): 1 / M gives numpy's irfft
  int npairs;                  // 1 .. NLS_PAIRS
  int ngroups;                 // workgroups of the launch: the stride of the loop over the rows
};
// The rule of the profiles (include/mpifft4py_amd.h states it; kernel, sweep, emulator and tests share it): the value in the rows'
// precision taken to double and normalised THERE by one rounded product (incr_value), the centre subtracted, products and sums in
// double.  m: the NLP_STATS sums of one pair at one position; da, db: the centred values.
MFFT_D void prof_add(double* m, double da, double db) {
  m[0] += da;
  m[1] += db;
  m[2] += da * da;
  m[3] += db * db;
  m[4] += da * db;
}

// Maximum that KEEPS a NaN (fmax drops it): a blown-up field must not report a finite maximum.  m is sticky once NaN.
template <typename T> MFFT_D T nan_max(T m, T x) { return (x > m || x != x) ? x : m; }
template <typename T> MFFT_D T nan_min(T m, T x) { return (x < m || x != x) ? x : m; }
// one value into the six statistics of its field (double whatever the rows' precision): m = [min, max, S1, S2, S3, S4]
MFFT_D void moments_add(double (&m)[NLS_STATS], double x, double c) {
  m[0] = nan_min(m[0], x);
  m[1] = nan_max(m[1], x);
  const double d = x - c, d2 = d * d;
  m[2] += d;
  m[3] += d2;
  m[4] += d2 * d;
  m[5] += d2 * d2;
}
MFFT_D void moments_clear(double (&m)[NLS_STATS]) {
  m[0] = __builtin_inf();
  m[1] = -__builtin_inf();
  m[2] = m[3] = m[4] = m[5] = 0.0;
}
MFFT_D void moments_merge(double (&m)[NLS_STATS], const double (&o)[NLS_STATS]) {
  m[0] = nan_min(m[0], o[0]);
  m[1] = nan_max(m[1], o[1]);
#pragma unroll
  for (int k = 2; k < NLS_STATS; ++k) m[k] += o[k];
}
template <typename T> MFFT_D T abs_of(T x) { return x < (T)0 ? -x : x; }
// STATS kernels: a value that is not finite (x - x is 0 only for finite x) leaves the transform -- it reads as 0 -- and is kept in
// `bad` (the larger of the |x| met, NaN above Inf).  The two real fields of a pair share ONE complex transform, so left in
// it would turn the partner field's values into NaNs as well; its own field gets it back after the transform (NlzFft::stats).
template <typename T> MFFT_D void take_out_nonfinite(cx<T>& z, T& bad) {      // (the whole bin: its field is marked, whatever the other part was)
  const T s = abs_of(z.x) + abs_of(z.y);
  if ((s - s) != (T)0) {
    bad = nan_max(bad, s);
    z = mk<T>((T)0, (T)0);
  }
}
// max over the WHOLE wave of two values (>= 0 or NaN), lane 0 stores them.  Lanes past the workgroup's last thread (a
// workgroup need not be whole waves: 12 threads per row x 21 rows) are left out; lane 0 still ends with the maximum of
// the lanes that exist, because a lane l < o whose partner l + o is missing has no one behind that partner either.
template <typename T, int THREADS>
MFFT_D void wave_absmax_store(T ma, T mb, int tid, T* slot) {
  const int lane = tid & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T oa = wave_shfl(ma, lane ^ o), ob = wave_shfl(mb, lane ^ o);
    if (THREADS % 64 == 0 || (tid ^ o) < THREADS) {
      ma = nan_max(ma, oa);
      mb = nan_max(mb, ob);
    }
  }
  if (lane == 0) {
    slot[0] = ma;
    slot[3] = mb;
  }
}

// The six statistics of one field over the WHOLE wave, by a fixed butterfly (the same order of additions every run: the sums are
// bitwise reproducible); lane 0 stores them.  Missing lanes of a workgroup's last wave are left out as above.
template <int THREADS>
MFFT_D void wave_moments_store(double (&m)[NLS_STATS], int tid, double* slot) {
  const int lane = tid & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    double other[NLS_STATS];
#pragma unroll
    for (int k = 0; k < NLS_STATS; ++k) other[k] = wave_shfl(m[k], lane ^ o);
    if (THREADS % 64 == 0 || (tid ^ o) < THREADS) moments_merge(m, other);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NLS_STATS; ++k) slot[k] = m[k];
  }
}

// N plain sums over the WHOLE wave by the same fixed butterfly; lane 0 stores them.
template <int THREADS, int N>
MFFT_D void wave_sums_store(double (&m)[N], int tid, double* slot) {
  const int lane = tid & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double other = wave_shfl(m[k], lane ^ o);
      if (THREADS % 64 == 0 || (tid ^ o) < THREADS) m[k] += other;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) slot[k] = m[k];
  }
}

// WAVE: a row's threads sit inside ONE wave (TPT divides 64), so the exchanges of its transforms need no workgroup barrier at
// all: LDS operations of a wave execute in issue order, what a lane wrote is there for every lane's later read, and the only
// thing to stop is the compiler moving a read above a write (a wave barrier: no instruction).  The waves of a workgroup then
// drift apart -- one loads while another computes -- instead of meeting 60 times per pair of rows (SQ_WAIT_ANY was 55 % of
// the wave cycles with workgroup barriers, profiles/r06_nlz_pmc_counters.txt).
#if defined(__HIP_DEVICE_COMPILE__)
#define MFFT_WAVE_SYNC() __builtin_amdgcn_wave_barrier()
#else
#define MFFT_WAVE_SYNC() MFFT_BARRIER()
#endif
template <bool WAVE> MFFT_D void nlz_sync() {
  if constexpr (WAVE) MFFT_WAVE_SYNC();
  else MFFT_BARRIER();
}
template <typename T, class Slot, bool WAVE>
struct XchFullW {
  cx<T>* buf;
  Slot slot;
  template <class S, int P>
  MFFT_D void exchange(cx<T> (&v)[S::E], int j, bool pre_barrier) {
    if (pre_barrier) nlz_sync<WAVE>();
    pass_scatter<S, P>(j, [&](int pos, int reg) { buf[slot(pos)] = v[reg]; });
    nlz_sync<WAVE>();
    pass_gather<S>(j, [&](int pos, int reg) { v[reg] = buf[slot(pos)]; });
  }
};

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
struct NlzFft {
  static_assert(!WAVE || (!SPLIT && S::TPT <= 64 && 64 % S::TPT == 0), "wave-synchronous rows: whole rows inside a wave, whole-complex exchange");
  typedef typename RowXch<SPLIT, T, PadSlot<S::R(0)>>::elem XE;
  static constexpr int M = S::N;
  static constexpr int E = S::E;
  static constexpr int THREADS = S::TPT * ROWS;
  static constexpr int PD = S::R(0);       // (pad periods of 16 / 24 / 32 elements: no gain, 16 loses 50 % at 512: profiles/r06_nlz_variants.txt)
  static constexpr int PLEN = padded_len<M, PD>();
  static constexpr int TW_BYTES = (TWLDS && S::NP > 1) ? (int)(S::TW * sizeof(cx<T>)) : 0;
  static constexpr int XCH_BYTES = (int)(PLEN * ROWS * sizeof(XE));      // also the mirror exchange of the forward split
  static constexpr int LDS_BYTES = TW_BYTES + XCH_BYTES;
  typedef typename std::conditional<WAVE, XchFullW<T, PadSlot<PD>, true>, typename RowXch<SPLIT, T, PadSlot<PD>>::type>::type Xch;

  // Z = A + iB at the positions of thread j, ready for the inverse passes (swap identity)
  // (STATS: non-finite input values are taken out, bad[0] of field a, bad[1] of field b: take_out_nonfinite)
  template <bool STATS = false>
  static MFFT_D void load_pair(cx<T> (&v)[E], const cx<T>* ra, const cx<T>* rb, int j, int valid, T* bad = nullptr) {
    load_pair_rows<STATS>(v, ra, rb, j, valid, valid, bad);
  }
  // ... the two rows with bin counts of their own (0: the row reads as zeros and is not touched beyond its first element, which
  // exists)
  template <bool STATS = false>
  static MFFT_D void load_pair_rows(cx<T> (&v)[E], const cx<T>* ra, const cx<T>* rb, int j, int valid_a, int valid_b, T* bad = nullptr) {
    if constexpr (STATS) bad[0] = bad[1] = (T)0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int p = j + k * S::TPT;
      const bool mir = p > M / 2;                  // upper half: conj of bin M - p
      const int q = mir ? M - p : p;
      const bool oka = q < valid_a, okb = q < valid_b;
      // unconditional loads of a clamped position (fft_core.h keep_bits): all 2 E of them in flight together
      cx<T> xa = keep_bits(ra[oka ? q : 0], oka), xb = keep_bits(rb[okb ? q : 0], okb);
      if (q == 0 || (M % 2 == 0 && q == M / 2)) {  // imaginary parts of the k = 0 and k = M/2 bins are ignored (as c2r does)
        xa.y = (T)0;
        xb.y = (T)0;
      }
      if constexpr (STATS) {
        take_out_nonfinite(xa, bad[0]);
        take_out_nonfinite(xb, bad[1]);
      }
      if (mir) { xa.y = -xa.y; xb.y = -xb.y; }
      v[k] = mk<T>(xa.y + xb.x, xa.x - xb.y);      // swapri(A + iB)
    }
  }

  template <bool STATS = false, class TwPtr>
  static MFFT_D void inverse_pair(cx<T> (&v)[E], const cx<T>* ra, const cx<T>* rb, int j, int valid, TwPtr tw, Xch& xc, T* bad = nullptr) {
    // (Hiding j here and in forward_pair, as Nlz3Fft does, makes the address arithmetic local to each of the five transforms:
    // 216 -> 160 VGPRs for the 8-values plans -- and 5 % SLOWER, 512: 0.555 -> 0.583 ms, 1024: 0.879 -> 0.923; the 12-values plans
    // spill more, not less, 768: 1.36 -> 1.66 ms: profiles/r06_nlz_variants.txt.  Not done.)
    load_pair<STATS>(v, ra, rb, j, valid, bad);
    nlz_sync<WAVE>();
    run_passes<S, 0, T>(v, j, tw, xc);
  }

  // forward transform of v = ra + i rb and its split into the two half-spectra, bins [0, valid) stored
  template <class TwPtr>
  static MFFT_D void forward_pair(cx<T> (&v)[E], int j, TwPtr tw, Xch& xc, XE* xb, cx<T>* oa, cx<T>* ob, bool sa, bool sb,
                                  int valid) {
    nlz_sync<WAVE>();                                // the buffer is free: everybody has left the previous exchange
    run_passes<S, 0, T>(v, j, tw, xc);
    constexpr int KMAX = (M / 2) / S::TPT;         // registers beyond it hold positions > M/2 only: nothing to store
    const T half = (T)0.5;
    auto emit = [&](int p, cx<T> z, cx<T> m) {
      const cx<T> zm = conj(m);
      if (p < valid) {
        if (sa) oa[p] = scale(z + zm, half);
        if (sb) ob[p] = mul_mi(scale(z - zm, half));
      }
    };
    if constexpr (SPLIT) {
      T mx[KMAX + 1];
      if constexpr (S::NP > 1) nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k].x;
      nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k <= KMAX; ++k) {
        const int p = j + k * S::TPT;
        mx[k] = xb[padpos<PD>(p == 0 ? 0 : M - p)];
      }
      nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k].y;
      nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k <= KMAX; ++k) {
        const int p = j + k * S::TPT;
        emit(p, v[k], mk<T>(mx[k], xb[padpos<PD>(p == 0 ? 0 : M - p)]));
      }
    } else {
      if constexpr (S::NP > 1) nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k];
      nlz_sync<WAVE>();
#pragma unroll
      for (int k = 0; k <= KMAX; ++k) {
        const int p = j + k * S::TPT;
        emit(p, v[k], xb[padpos<PD>(p == 0 ? 0 : M - p)]);
      }
    }
  }

  // STATS (NlzAbsMax): max |a_f|, max |b_f| over this thread's E positions of the pair just transformed (.y = a_f, .x = b_f),
  // reduced over the wave and stored at once: the maxima themselves are not carried across the next transform.  What IS live
  // across the transform before is bad[2] (two T: four VGPRs in double), from load_pair to here -- the variant is not
  // register-neutral (profiles/nonlinear_absmax_regs.tsv).  A wave may hold several rows or a part of one: the slot is the
  // launch's wave, the fold kernel does not care which rows went into it.
  // bad[0], bad[1]: what load_pair took out of the spectra of a_f, b_f at this thread's bins (0: nothing).  It goes into that
  // field's maximum -- a NaN bin makes the whole real row NaN, an Inf bin Inf or NaN -- and, as NaNs, into this thread's values
  // of that field, so that the product rows come out NaN as the plain kernel's do (the forward transform spreads them over the
  // row); the partner field stays what it is.
  template <bool STATS, class PP>
  static MFFT_D void stats(cx<T> (&v)[E], const PP& P, int bid, int tid, int h, int f, const T* bad) {
    if constexpr (STATS) {
      T ma = bad[0], mb = bad[1];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        ma = nan_max(ma, abs_of(v[k].y));
        mb = nan_max(mb, abs_of(v[k].x));
      }
      const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
      const T pa = bad[0] * (T)0, pb = bad[1] * (T)0;        // NaN where something was taken out
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = mk<T>(bb ? pb : v[k].x, ba ? pa : v[k].y);
      constexpr int NW = (THREADS + 63) / 64;
      const i64 wave = (i64)bid * NW + tid / 64;
      wave_absmax_store<T, THREADS>(ma, mb, tid, P.part + (wave * 2 + h) * 6 + f);
    }
  }

  static MFFT_D void body(const NlzParams<T>& P, int bid, int tid, char* lds) { body_t<false>(P, bid, tid, lds); }
  template <bool STATS, class PP>
  static MFFT_D void body_t(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();          // the table is shared by the workgroup's waves: the one real barrier
    }                                              // (otherwise the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 unit = (i64)bid * ROWS + rl;         // a pair of rows
    T r2a[E];
#pragma unroll
    for (int k = 0; k < E; ++k) r2a[k] = (T)0;
    bool sa = false;
    i64 rowa = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const i64 row = 2 * unit + h;
      const bool active = row < P.nrows;           // rows past the end re-read the last row and store nothing
      const i64 lrow = active ? row : P.nrows - 1;
      const i64 io = lrow * P.in_stride;
      cx<T> pk[2][E];
      cx<T> v[E];
      T bad[2];
      inverse_pair<STATS>(v, P.a[0] + io, P.b[0] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 0, bad);
#pragma unroll
      for (int k = 0; k < E; ++k) pk[0][k] = v[k];
      inverse_pair<STATS>(v, P.a[1] + io, P.b[1] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 1, bad);
#pragma unroll
      for (int k = 0; k < E; ++k) pk[1][k] = v[k];
      inverse_pair<STATS>(v, P.a[2] + io, P.b[2] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 2, bad);
      // the results are swapped (inverse through the swap identity): .y = a_f, .x = b_f at position j + k TPT
      T r2[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const T a0 = pk[0][k].y, a1 = pk[1][k].y, a2 = v[k].y;
        const T b0 = pk[0][k].x, b1 = pk[1][k].x, b2 = v[k].x;
        v[k] = mk<T>((a1 * b2 - a2 * b1) * P.scale, (a2 * b0 - a0 * b2) * P.scale);
        r2[k] = (a0 * b1 - a1 * b0) * P.scale;
      }
      const i64 oo = row * P.out_stride;
      forward_pair(v, j, tw, xc, xb, P.out[0] + oo, P.out[1] + oo, active, active, P.valid);
      if (h == 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) r2a[k] = r2[k];
        sa = active;
        rowa = row;
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = mk<T>(r2a[k], r2[k]);
        forward_pair(v, j, tw, xc, xb, P.out[2] + rowa * P.out_stride, P.out[2] + oo, sa, active, P.valid);
      }
    }
  }

  // The same stage with the DOT product, out[0] = rfft(sum_f irfft(a_f) irfft(b_f)): the term u . grad(theta) of a transported
  // scalar.  A sum accumulates, so nothing is parked: after each inverse pair s[k] += a_f[k] b_f[k], E reals, and E more hold the
  // sum of the first row of a pair while the second is computed; the two sums then ride on ONE forward transform, as r2 does
  // above.  3.5 transforms and 7 rows of `valid` bins per (x, y) point instead of 4.5 and 9; out[1], out[2] are not read.
  // All six rows of both (x, y) points are loaded before the first store, so out[0] may alias any a[f] or b[f] row for row.
  static MFFT_D void body_dot(const NlzParams<T>& P, int bid, int tid, char* lds) { body_dot_t<false>(P, bid, tid, lds); }
  template <bool STATS, class PP>
  static MFFT_D void body_dot_t(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 unit = (i64)bid * ROWS + rl;         // a pair of rows
    T s0[E];
#pragma unroll
    for (int k = 0; k < E; ++k) s0[k] = (T)0;
    bool sa = false;
    i64 rowa = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const i64 row = 2 * unit + h;
      const bool active = row < P.nrows;           // rows past the end re-read the last row and store nothing
      const i64 lrow = active ? row : P.nrows - 1;
      const i64 io = lrow * P.in_stride;
      cx<T> v[E];
      T s[E];
      T bad[2];
      // the results are swapped (inverse through the swap identity): .y = a_f, .x = b_f at position j + k TPT
      inverse_pair<STATS>(v, P.a[0] + io, P.b[0] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 0, bad);
#pragma unroll
      for (int k = 0; k < E; ++k) s[k] = v[k].x * v[k].y;
      inverse_pair<STATS>(v, P.a[1] + io, P.b[1] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 1, bad);
#pragma unroll
      for (int k = 0; k < E; ++k) s[k] += v[k].x * v[k].y;
      inverse_pair<STATS>(v, P.a[2] + io, P.b[2] + io, j, P.valid_in, tw, xc, bad);
      stats<STATS>(v, P, bid, tid, h, 2, bad);
#pragma unroll
      for (int k = 0; k < E; ++k) s[k] += v[k].x * v[k].y;
      if (h == 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) s0[k] = s[k];
        sa = active;
        rowa = row;
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = mk<T>(s0[k] * P.scale, s[k] * P.scale);
        forward_pair(v, j, tw, xc, xb, P.out[0] + rowa * P.out_stride, P.out[0] + row * P.out_stride, sa, active, P.valid);
      }
    }
  }

  // The stage of a velocity that carries a scalar: out[f] = rfft((irfft(a) x irfft(b))_f) AND outs = rfft(sum_f irfft(a_f)
  // irfft(c_f)) -- u x omega and u . grad(theta) with irfft(a_f) computed ONCE.  Ten real rows in, four out: 6.5 complex transforms
  // of length M per row, the minimum for thirteen real ones.  The pairs are chosen so that products fall out of ONE transform:
  //     before the pair of rows   b_2[row 0] + i b_2[row 1]      (the odd tenth row: E reals of row 1 wait for their turn)
  //     per row                   a_f + i c_f, f = 0..2          s += a_f c_f at once, a_f parked (3 E reals + E)
  //                               b_0 + i b_1                    -> r_0, r_1, r_2 from the parked a and the row's b_2
  //                               forward r_0 + i r_1            -> out[0], out[1]
  //                               forward r_2 + i s              -> out[2], outs
  // Both results of every forward transform belong to the row, so nothing waits for the partner row on the forward side.  Parked
  // next to a transform's working set: 6 E reals across the fourth inverse transform (a, s, b_2 of both rows), 3 E across the first
  // forward one (r_2, s, b_2 of the partner), where the cross body parks 5 E.
  // Every load of a row, and the early b_2 load of its partner, precedes the row's first store: out[] may lie over a[] or b[], and
  // outs over any one component they leave alone.  A row past nrows reads as zeros -- it does NOT read the last row again, which
  // an in-place caller has overwritten by then -- and stores nothing.
  template <class PP>
  static MFFT_D void body_cross_dot(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 unit = (i64)bid * ROWS + rl;         // a pair of rows
    const i64 last = P.nrows - 1;
    cx<T> v[E];
    // (Seven transforms are inlined here, and hipcc keeps LDS addresses and twiddle indices of all of them live: every double-precision
    // kernel sits at 256 VGPRs with scratch, profiles/nonlinear_cross_dot_regs.tsv.  Hiding the thread index at the head of each
    // transform, as Nlz3Fft does, lowered the scratch -- and gave a WRONG cross product on the device for the 12-point plan in double
    // precision, exact in the emulator, cause not found.  Not done.)
    T b2[E], b2n[E];                               // irfft(b_2) of the row at hand and of its partner
    {
      const bool act0 = 2 * unit < P.nrows, act1 = 2 * unit + 1 < P.nrows;
      load_pair_rows(v, P.b[2] + (act0 ? 2 * unit : last) * P.in_stride, P.b[2] + (act1 ? 2 * unit + 1 : last) * P.in_stride, j,
                     act0 ? P.valid_in : 0, act1 ? P.valid_in : 0);
      nlz_sync<WAVE>();
      run_passes<S, 0, T>(v, j, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { b2[k] = v[k].y; b2n[k] = v[k].x; }      // swapped results: .y the first row, .x the second
    }
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const i64 row = 2 * unit + h;
      const bool active = row < P.nrows;
      const i64 io = (active ? row : last) * P.in_stride;
      const int vin = active ? P.valid_in : 0;
      T a0[E], a1[E], a2[E], s[E];
      inverse_pair(v, P.a[0] + io, P.c[0] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a0[k] = v[k].y; s[k] = v[k].y * v[k].x; }
      inverse_pair(v, P.a[1] + io, P.c[1] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a1[k] = v[k].y; s[k] += v[k].y * v[k].x; }
      inverse_pair(v, P.a[2] + io, P.c[2] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a2[k] = v[k].y; s[k] += v[k].y * v[k].x; }
      inverse_pair(v, P.b[0] + io, P.b[1] + io, j, vin, tw, xc);
      T r2[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const T b0 = v[k].y, b1 = v[k].x;
        v[k] = mk<T>((a1[k] * b2[k] - a2[k] * b1) * P.scale, (a2[k] * b0 - a0[k] * b2[k]) * P.scale);
        r2[k] = (a0[k] * b1 - a1[k] * b0) * P.scale;
      }
      const i64 oo = row * P.out_stride;
      forward_pair(v, j, tw, xc, xb, P.out[0] + oo, P.out[1] + oo, active, active, P.valid);
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = mk<T>(r2[k], s[k] * P.scale);
      forward_pair(v, j, tw, xc, xb, P.out[2] + oo, P.outs + oo, active, active, P.valid);
#pragma unroll
      for (int k = 0; k < E; ++k) b2[k] = b2n[k];
    }
  }

  // The stage with the OUTER product: out9[3 i + j] = rfft(irfft(a_i) irfft(b_j)), all nine -- the Elsasser products z+_i z-_j of
  // incompressible MHD, a convective term in conservative form, a stress u_i u_j (a = b).  Six real rows in, nine out: three
  // inverse transforms (a_f + i b_f) and four and a half forward ones per row, 7.5 transforms of length M, the minimum for fifteen
  // real rows.  All six real values of a position sit in the thread after the third inverse transform; the products leave in the
  // order that retires a_0 first,
  //     (a0 b0, a0 b1)   (a0 b2, a1 b0)   (a1 b1, a1 b2)   (a2 b0, a2 b1)      each pair on ONE forward transform into the row's own outputs
  //     a2 b2 of the TWO rows of a pair together on one more, as r2 / r2a of body_t.
  // Parked next to the first forward transform's working set: a0 b2, a1, a2, b0, b1, b2 and the partner row's a2 b2 -- 7 E reals,
  // where body_cross_dot parks 6 E; the later transforms park 6, 5 and 2 E.  The scale goes onto a once (3 E products instead of 9 E).
  // Every load of a row precedes its first store, and the two rows of a pair are loaded and stored one after the other: out9[0..2]
  // may lie over a[0..2] and out9[3..5] over b[0..2], row for row (the routes use exactly that); out9[6..8] are never inputs.
  // A row past nrows reads as zeros and stores nothing (body_cross_dot's rule: the last row is NOT read again).
  // (The thread index is not hidden at the head of the transforms: see body_cross_dot.)
  template <class PP>
  static MFFT_D void body_outer(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 unit = (i64)bid * ROWS + rl;         // a pair of rows
    const i64 last = P.nrows - 1;
    T w8a[E];                                      // a2 b2 of the first row of the pair
#pragma unroll
    for (int k = 0; k < E; ++k) w8a[k] = (T)0;
    bool sa = false;
    i64 rowa = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const i64 row = 2 * unit + h;
      const bool active = row < P.nrows;
      const i64 io = (active ? row : last) * P.in_stride;
      const int vin = active ? P.valid_in : 0;
      cx<T> v[E];
      T a0[E], a1[E], a2[E], b0[E], b1[E], b2[E];
      // the results are swapped (inverse through the swap identity): .y = a_f, .x = b_f at position j + k TPT
      inverse_pair(v, P.a[0] + io, P.b[0] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a0[k] = v[k].y * P.scale; b0[k] = v[k].x; }
      inverse_pair(v, P.a[1] + io, P.b[1] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a1[k] = v[k].y * P.scale; b1[k] = v[k].x; }
      inverse_pair(v, P.a[2] + io, P.b[2] + io, j, vin, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) { a2[k] = v[k].y * P.scale; b2[k] = v[k].x; }
      const i64 oo = row * P.out_stride;
      T p02[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        v[k] = mk<T>(a0[k] * b0[k], a0[k] * b1[k]);
        p02[k] = a0[k] * b2[k];
      }
      forward_pair(v, j, tw, xc, xb, P.out9[0] + oo, P.out9[1] + oo, active, active, P.valid);
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = mk<T>(p02[k], a1[k] * b0[k]);
      forward_pair(v, j, tw, xc, xb, P.out9[2] + oo, P.out9[3] + oo, active, active, P.valid);
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = mk<T>(a1[k] * b1[k], a1[k] * b2[k]);
      forward_pair(v, j, tw, xc, xb, P.out9[4] + oo, P.out9[5] + oo, active, active, P.valid);
#pragma unroll
      for (int k = 0; k < E; ++k) {
        v[k] = mk<T>(a2[k] * b0[k], a2[k] * b1[k]);
        a2[k] = a2[k] * b2[k];
      }
      forward_pair(v, j, tw, xc, xb, P.out9[6] + oo, P.out9[7] + oo, active, active, P.valid);
      if (h == 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) w8a[k] = a2[k];
        sa = active;
        rowa = row;
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = mk<T>(w8a[k], a2[k]);
        forward_pair(v, j, tw, xc, xb, P.out9[8] + rowa * P.out_stride, P.out9[8] + oo, sa, active, P.valid);
      }
    }
  }

  // The stage that ends in a REDUCTION: min, max and S_p = sum (x - c)^p, p = 1..4, of up to six real fields over all rows and all
  // M positions -- the one-point statistics of a field that never exists in real space.  ceil(nfields / 2) inverse transforms per
  // row, nothing forward, nothing stored but the partials; nothing is parked next to a transform's working set but the
  // accumulators, 2 x 6 doubles per pair.  The maxima bodies above reduce over the wave after every transform; with twelve 64-bit
  // values per pair that would be some 140 shuffles per transform, so here a workgroup strides over the pairs of rows
  // (unit += ngroups * ROWS), every thread keeps its accumulators for the whole launch, and ONE wave reduction runs at the end:
  // lane 0 of every wave stores NLS_SLOTS doubles with plain stores, a fold kernel adds the waves' slots in a fixed order.  Which
  // rows a thread meets and the order it adds them in depend on (nrows, ngroups) only: the results are bitwise reproducible.
  // Powers and sums in double in both precisions.  Non-finite inputs leave the transform on load (take_out_nonfinite) and come back
  // as NaN sums and NaN / +-Inf extremes of THEIR field; the partner of the pair stays what it is.
  // ONE transform is inlined, in a loop over the pairs that is not unrolled -- inlined transforms keep each other's LDS
  // addresses and twiddle indices live, and the 12-values plans have no registers for that --, and only the accumulation is
  // written out per pair, so that the accumulators are indexed statically: registers.  npairs is uniform over the launch, so the
  // barriers inside a transform are met by everybody or nobody.
  template <class PP>
  static MFFT_D void body_moments(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    double acc[NLS_PAIRS][2][NLS_STATS];
#pragma unroll
    for (int p = 0; p < NLS_PAIRS; ++p) {
      moments_clear(acc[p][0]);
      moments_clear(acc[p][1]);
    }
    const i64 last = P.nrows - 1;
    // the values of one pair into its accumulators (swapped results: .y = a_p, .x = b_p at position j + k TPT), and what the load
    // took out of either spectrum (Inf or NaN) into that field's
    auto add = [&](double (&m)[2][NLS_STATS], const cx<T> (&v)[E], const T (&bad)[2], double ca, double cb) {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        moments_add(m[0], (double)v[k].y * P.norm, ca);
        moments_add(m[1], (double)v[k].x * P.norm, cb);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (bad[i] != (T)0) {
          const double w = (double)bad[i], nn = w * 0.0;
          m[i][0] = nan_min(m[i][0], -w);
          m[i][1] = nan_max(m[i][1], w);
#pragma unroll
          for (int k = 2; k < NLS_STATS; ++k) m[i][k] += nn;
        }
    };
#pragma unroll 1
    for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
      const i64 unit = base + rl;                  // a pair of rows
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const i64 row = 2 * unit + h;
        const bool active = row < P.nrows;         // rows past the end re-read the last row and count nothing
        const i64 io = (active ? row : last) * P.in_stride;
#pragma unroll 1
        for (int p = 0; p < P.npairs; ++p) {
          cx<T> v[E];
          T bad[2];
          const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
          const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
          const bool hb = pb != nullptr;
          load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          if (active) {
            if (p == 0) add(acc[0], v, bad, P.center[0], P.center[1]);
            else if (p == 1) add(acc[1], v, bad, P.center[2], P.center[3]);
            else add(acc[2], v, bad, P.center[4], P.center[5]);
          }
        }
      }
    }
    constexpr int NW = (THREADS + 63) / 64;
    double* slot = P.part + ((i64)bid * NW + tid / 64) * NLS_SLOTS;
#pragma unroll
    for (int p = 0; p < NLS_PAIRS; ++p) {
      if (p < P.npairs) {
        wave_moments_store<THREADS>(acc[p][0], tid, slot + (2 * p) * NLS_STATS);
        wave_moments_store<THREADS>(acc[p][1], tid, slot + (2 * p + 1) * NLS_STATS);
      } else if ((tid & 63) == 0) {                // every slot written: the fold reads them all
#pragma unroll
        for (int k = 0; k < NLS_STATS; ++k) slot[(2 * p) * NLS_STATS + k] = slot[(2 * p + 1) * NLS_STATS + k] = acc[p][0][k];
      }
    }
  }

  // The stage that ends in a HISTOGRAM: the counts of the values of up to six real fields in nbins equal bins per field -- the PDF
  // of a field that never exists in real space.  The skeleton is body_moments': a workgroup strides over the pairs of rows, pairs of
  // fields ride on one inverse transform, ONE transform is inlined, non-finite bins leave the transform on load.  What differs is
  // where the state lives: two histograms of nbins + 3 unsigned counts in LDS behind the exchange buffers (NlzHist::LDS_BYTES), no
  // accumulator in a register.  So the loop over the PAIRS is the outer one: clear the two histograms, barrier, all rows of this
  // workgroup for this pair -- every value to its slot (hist_slot) with an LDS add --, barrier, plain stores of the two histograms
  // into the workgroup's row of P.part.  Every (row, pair) is still loaded once; the barriers sit where every thread of the
  // workgroup arrives (the bound of the row loop is the workgroup's), so the wave-synchronous builds keep their row loop free of
  // them.  A thread clears and stores the slots tid, tid + THREADS, ..: what it clears for the next pair it has stored itself.
  // Counts are integers: whatever order the adds land in, the result is the same bits.  A thread whose load took a non-finite
  // bin out of a field counts ITS values of that field in the non-finite slot (the row is NaN there); the partner stays exact.
  // A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M values per field: the host keeps that below 2^32.
  // MERGE: runs of equal slot inside the wave are merged before the add (lds_count_runs); every lane of the wave takes part, a lane
  // of a row past the end with slot -1.
  template <bool MERGE, class PP>
  static MFFT_D void body_hist(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nb3 = P.nbins + 3;
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (int p = 0; p < P.npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double loa = p == 0 ? P.lo[0] : p == 1 ? P.lo[2] : P.lo[4], lob = p == 0 ? P.lo[1] : p == 1 ? P.lo[3] : P.lo[5];
      const double iva = p == 0 ? P.inv[0] : p == 1 ? P.inv[2] : P.inv[4], ivb = p == 0 ? P.inv[1] : p == 1 ? P.inv[3] : P.inv[5];
      const bool hb = pb != nullptr;
      for (int i = tid; i < 2 * nb3; i += THREADS) hist[i] = 0u;
      MFFT_BARRIER();
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and count nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
          if constexpr (MERGE) {
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? P.nbins + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, P.nbins);
              const int sb = bb ? P.nbins + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, P.nbins);
              lds_count_runs(hist, active ? sa : -1, tid & 63);
              lds_count_runs(hist + nb3, active ? sb : -1, tid & 63);
            }
          } else if (active) {                     // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? P.nbins + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, P.nbins);
              const int sb = bb ? P.nbins + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, P.nbins);
              MFFT_LDS_COUNT(hist + sa);
              MFFT_LDS_COUNT(hist + nb3 + sb);
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * P.npairs + p) * (2 * nb3);
      for (int i = tid; i < 2 * nb3; i += THREADS) dst[i] = hist[i];
    }
  }

  // The stage that ends in a JOINT HISTOGRAM: the skeleton of body_hist, but the pairing that body_hist throws away is kept.  After
  // run_passes a thread holds .y = a_p and .x = b_p of the SAME grid point; it counts the point into one cell of the pair's grid,
  // cell = sa (nbb + 3) + sb (joint_cell), with ONE LDS add where body_hist issues two.  The grid of (nba + 3)(nbb + 3) unsigned
  // cells lies behind the exchange buffers (NlzJoint::LDS_BYTES reserves NLJ_MAXCELLS).  The loop over the pairs is outermost:
  // clear the grid, barrier, all rows of this workgroup for this pair, barrier, plain stores of the used cells into the workgroup's
  // row of P.part; the barriers sit where every thread of the workgroup arrives, so the wave-synchronous builds keep their row loop
  // free of them.  A thread clears and stores the cells tid, tid + THREADS, ..: what it clears for the next pair it has stored
  // itself.  A non-finite bin met on load marks ITS field's slot only: the partner keeps its exact slot.  Rows past the end re-read
  // the last row and count nothing.  A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M points: the host keeps
  // that below 2^32.  Every pair has both fields (the host refuses a null b).
  template <class PP>
  static MFFT_D void body_joint(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* grid = reinterpret_cast<unsigned*>(lds + LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nba = P.nba < 1 ? 1 : P.nba > NLJ_MAXBINS ? NLJ_MAXBINS : P.nba;
    const int nbb = P.nbb < 1 ? 1 : P.nbb > NLJ_MAXBINS ? NLJ_MAXBINS : P.nbb;
    const int cells = (nba + 3) * (nbb + 3);       // <= NLJ_MAXCELLS
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (int p = 0; p < P.npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double loa = p == 0 ? P.lo[0] : p == 1 ? P.lo[2] : P.lo[4], lob = p == 0 ? P.lo[1] : p == 1 ? P.lo[3] : P.lo[5];
      const double iva = p == 0 ? P.inv[0] : p == 1 ? P.inv[2] : P.inv[4], ivb = p == 0 ? P.inv[1] : p == 1 ? P.inv[3] : P.inv[5];
      for (int i = tid; i < cells; i += THREADS) grid[i] = 0u;
      MFFT_BARRIER();
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and count nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          load_pair_rows<true>(v, pa + io, pb + io, j, P.valid_in, P.valid_in, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
          if (active) {                            // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) {
              const int sa = ba ? nba + 2 : hist_slot((double)v[k].y * P.norm, loa, iva, nba);
              const int sb = bb ? nbb + 2 : hist_slot((double)v[k].x * P.norm, lob, ivb, nbb);
              MFFT_LDS_COUNT(grid + joint_cell(sa, sb, nbb));
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * P.npairs + p) * cells;
      for (int i = tid; i < cells; i += THREADS) dst[i] = grid[i];
    }
  }

  // The stage that ends in the statistics of a QUADRATIC FORM: q = sum_f w_f r_f^2 of up to six real fields at every position of
  // every row -- enstrophy density, dissipation, energy density -- reduced to [min, max, S1 .. S4] and, with nbins > 0, counted in
  // nbins equal bins: the statistics of a combination of fields none of which exists in real space.  The accumulation of body_dot
  // (a running sum in registers across the inverse transforms of a row) under the ending of body_moments and body_hist, on the
  // skeleton of body_moments: a workgroup strides over the pairs of rows, ONE transform is inlined in a loop over the pairs that is
  // not unrolled, non-finite bins leave the transform on load.  After each transform the pair's two fields go into q[E] by the one
  // rule (quad_term: q = q + (w r) r, slot order, every operation rounded on its own); after the last pair of an active row q goes
  // into ONE set of six accumulators and ONE LDS histogram of nbins + 3 counts behind the exchange buffers.  State across a
  // transform: E doubles of q and 6 accumulators, where body_moments holds 36.  A partner that is not there reads as zeros and has
  // weight 0: its term is +-0 and changes no q.  A thread whose load took a non-finite bin out of ANY field has a NaN q in that
  // row.  The histogram is cleared once before the row loop and stored once after it, the barriers where body_hist has them (the
  // first also covers the twiddles); nbins is uniform over the launch; the wave-synchronous builds keep their row loop free of
  // workgroup barriers.  Rows past the end re-read the last row and count nothing.  Plain stores of every slot of the launch's
  // mpart and hpart; the folds of moments.hip and hist.hip add them in fixed order: bitwise reproducible.
  template <class PP>
  static MFFT_D void body_quad(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const int nb3 = P.nbins + 3;
    double acc[NLS_STATS];
    moments_clear(acc);
    for (int i = tid; i < nb3; i += THREADS) hist[i] = 0u;
    MFFT_BARRIER();
    const i64 last = P.nrows - 1;
#pragma unroll 1
    for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
      const i64 unit = base + rl;                  // a pair of rows
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const i64 row = 2 * unit + h;
        const bool active = row < P.nrows;         // rows past the end re-read the last row and count nothing
        const i64 io = (active ? row : last) * P.in_stride;
        double q[E];
#pragma unroll
        for (int k = 0; k < E; ++k) q[k] = 0.0;
        bool anybad = false;
#pragma unroll 1
        for (int p = 0; p < P.npairs; ++p) {
          cx<T> v[E];
          T bad[2];
          const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
          const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
          const double wa = p == 0 ? P.w[0] : p == 1 ? P.w[2] : P.w[4], wb = p == 0 ? P.w[1] : p == 1 ? P.w[3] : P.w[5];
          const bool hb = pb != nullptr;
          load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
#pragma unroll
          for (int k = 0; k < E; ++k) {            // swapped results: .y = a_p, .x = b_p at position j + k TPT; slot 2 p, then 2 p + 1
            q[k] = quad_term(q[k], wa, quad_mul((double)v[k].y, P.norm));
            q[k] = quad_term(q[k], wb, quad_mul((double)v[k].x, P.norm));
          }
          anybad = anybad || bad[0] != (T)0 || bad[1] != (T)0;
        }
        if (active) {
#pragma unroll
          for (int k = 0; k < E; ++k) {
            const double x = anybad ? __builtin_nan("") : q[k];
            moments_add(acc, x, P.center);
            if (P.nbins > 0) MFFT_LDS_COUNT(hist + hist_slot(x, P.lo, P.inv, P.nbins));
          }
        }
      }
    }
    MFFT_BARRIER();
    unsigned* dst = P.hpart + (i64)bid * nb3;
    for (int i = tid; i < nb3; i += THREADS) dst[i] = hist[i];
    constexpr int NW = (THREADS + 63) / 64;
    wave_moments_store<THREADS>(acc, tid, P.mpart + ((i64)bid * NW + tid / 64) * NLS_STATS);
  }

  // The stage that ends in STRUCTURE FUNCTIONS: S_p(s) = sum (r(z + s) - r(z))^p, p = 2, 3, 4, over all rows and all M positions of
  // up to six real fields, for up to NLI_MAXSEP separations along z -- a two-point statistic of fields that never exist in real
  // space.  Increments along z are local to a row, and after run_passes a thread group holds the whole real row of two fields
  // (positions j + k TPT): the row goes into the row's own exchange buffer at its natural positions, and every thread reads its E
  // positions back shifted by s, once per separation.  The skeleton is body_hist's with the loop over the PAIRS outermost, so that
  // only one pair's accumulators are live: 2 fields x NLI_MAXSEP x 3 doubles in registers (statically indexed: the loop over the
  // separations is unrolled and guarded by nsep), kept over all rows of the workgroup, ONE wave reduction per pair at the end,
  // plain stores of every slot; incr_fold (incr.hip) adds the waves' slots in fixed order: bitwise reproducible, no atomics.
  // With the whole-complex exchange the buffer holds both fields of the pair at once; with the split exchange it holds ONE real
  // value per position, so the two fields take two rounds.  Synchronisation as the build requires (nlz_sync): before the store
  // everybody has left the transform's last gather and the reads of the round before; after it the row is there; the sync before
  // the next transform's passes (below, as in body_moments) keeps its scatter behind the last reads.  All of them sit where every
  // thread of the workgroup arrives -- nsep and npairs are uniform, a row past the end runs the same code and adds nothing.
  // Non-finite bins leave the transform on load; the thread that met one adds NaN to every sum of THAT field, the partner stays exact.
  template <class PP>
  static MFFT_D void body_incr(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 last = P.nrows - 1;
    const int nsep = P.nsep < NLI_MAXSEP ? P.nsep : NLI_MAXSEP;
    constexpr int NW = (THREADS + 63) / 64;
    double* slot = P.part + ((i64)bid * NW + tid / 64) * NLI_SLOTS;
    // one separation's clamped value: no index reaches LDS on the strength of the caller's list alone
    // (hidden from the optimiser inside the row loop: left alone, hipcc hoists the E LDS addresses of every separation out of the
    // loop over the rows -- 8 E registers next to 48 doubles of accumulators, 150 - 850 bytes of scratch in every kernel)
    auto sep_of = [&](int i) {
      int s = P.sep[i];
      s = s < 1 ? 1 : s > M - 1 ? M - 1 : s;
      MFFT_HIDE_RANGE(s);
      return s;
    };
#pragma unroll 1
    for (int p = 0; p < NLS_PAIRS; ++p) {
      double acc[2][NLI_FIELD];                    // [a_p, b_p][separation][S2, S3, S4]
#pragma unroll
      for (int i = 0; i < NLI_FIELD; ++i) acc[0][i] = acc[1][i] = 0.0;
      if (p < P.npairs) {                          // (uniform over the launch)
        const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
        const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
        const bool hb = pb != nullptr;
#pragma unroll 1
        for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
          const i64 unit = base + rl;              // a pair of rows
#pragma unroll 1
          for (int h = 0; h < 2; ++h) {
            const i64 row = 2 * unit + h;
            const bool active = row < P.nrows;     // rows past the end re-read the last row and add nothing
            const i64 io = (active ? row : last) * P.in_stride;
            cx<T> v[E];
            T bad[2];
            load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
            nlz_sync<WAVE>();
            run_passes<S, 0, T>(v, j, tw, xc);
            // swapped results: .y = a_p, .x = b_p at position j + k TPT
            if constexpr (SPLIT) {
#pragma unroll
              for (int f = 0; f < 2; ++f) {
                nlz_sync<WAVE>();
#pragma unroll
                for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = f == 0 ? v[k].y : v[k].x;
                nlz_sync<WAVE>();
                if (active) {
#pragma unroll
                  for (int i = 0; i < NLI_MAXSEP; ++i)
                    if (i < nsep) {
                      const int s = sep_of(i);
#pragma unroll
                      for (int k = 0; k < E; ++k) {
                        const T x1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                        incr_add(acc[f] + i * NLI_STATS, incr_value((double)x1, P.norm), incr_value((double)(f == 0 ? v[k].y : v[k].x), P.norm));
                      }
                    }
                }
              }
            } else {
              nlz_sync<WAVE>();
#pragma unroll
              for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k];
              nlz_sync<WAVE>();
              if (active) {
#pragma unroll
                for (int i = 0; i < NLI_MAXSEP; ++i)
                  if (i < nsep) {
                    const int s = sep_of(i);
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                      const cx<T> z1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                      incr_add(acc[0] + i * NLI_STATS, incr_value((double)z1.y, P.norm), incr_value((double)v[k].y, P.norm));
                      incr_add(acc[1] + i * NLI_STATS, incr_value((double)z1.x, P.norm), incr_value((double)v[k].x, P.norm));
                    }
                  }
              }
            }
            if (active) {
#pragma unroll
              for (int f = 0; f < 2; ++f)
                if (bad[f] != (T)0) {              // what the load took out of this field: all its sums are NaN
                  const double nn = (double)bad[f] * 0.0;
#pragma unroll
                  for (int i = 0; i < NLI_FIELD; ++i)
                    if (i < nsep * NLI_STATS) acc[f][i] += nn;
                }
            }
          }
        }
      }
      // every slot written, the pairs the launch does not have with zeros: the fold reads them all
      wave_sums_store<THREADS, NLI_FIELD>(acc[0], tid, slot + (2 * p) * NLI_FIELD);
      wave_sums_store<THREADS, NLI_FIELD>(acc[1], tid, slot + (2 * p + 1) * NLI_FIELD);
    }
  }

  // The stage that ends in INCREMENT HISTOGRAMS: the counts of d = r(z + s) - r(z) over all rows and all M positions of up to six
  // real fields, for up to NLI_MAXSEP separations along z, in nbins equal bins of a range per field and separation -- the PDFs of
  // the increments of fields that never exist in real space.  The skeleton is body_incr's: the loop over the PAIRS outermost, the
  // real row into the row's own exchange buffer at its natural positions, read back shifted once per separation; with the split
  // exchange the two fields of a pair take two rounds; the separation clamped and hidden from the optimiser inside the row loop;
  // the syncs where body_incr has them.  The ending is body_hist's: NO accumulator in a register -- a thread computes a slot
  // (incr_hist_slot) and issues an LDS add; the pair's 2 x nsep x (nbins + 3) unsigned counts lie behind the exchange buffers
  // (NlzIncrHist::LDS_BYTES reserves NLK_MAXCELLS), cleared once per pair, barrier, all rows of this workgroup, barrier, plain
  // stores into the workgroup's row of P.part; the barriers sit where every thread of the workgroup arrives.  nsep, nbins and every
  // cell are clamped here (incr_hist_cell): no LDS index rests on the caller's numbers alone.  A thread whose load took a non-finite
  // bin out of a field counts ITS E x nsep increments of that field in the non-finite slot; the partner stays exact.  Rows past the
  // end re-read the last row and count nothing.  A workgroup counts at most ceil(pairs of rows / ngroups) * 2 * ROWS * M
  // increments per field and separation: the host keeps that below 2^32.
  template <class PP>
  static MFFT_D void body_incr_hist(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    unsigned* hist = reinterpret_cast<unsigned*>(lds + LDS_BYTES);
    if constexpr (TWLDS && S::NP > 1) stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);      // (the first barrier below covers it)
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 last = P.nrows - 1;
    const int nsep = P.nsep < 1 ? 1 : P.nsep > NLI_MAXSEP ? NLI_MAXSEP : P.nsep;
    const int nbins = P.nbins < 1 ? 1 : P.nbins > NLK_MAXBINS ? NLK_MAXBINS : P.nbins;
    const int nb3 = nbins + 3;
    const int cells = 2 * nsep * nb3;              // <= NLK_MAXCELLS
    const int npairs = P.npairs < NLS_PAIRS ? P.npairs : NLS_PAIRS;
    // one separation's clamped value, hidden from the optimiser inside the row loop (body_incr's sep_of: left alone, hipcc hoists
    // the E LDS addresses of every separation out of the loop over the rows)
    auto sep_of = [&](int i) {
      int s = P.sep[i];
      s = s < 1 ? 1 : s > M - 1 ? M - 1 : s;
      MFFT_HIDE_RANGE(s);
      return s;
    };
#pragma unroll 1
    for (int p = 0; p < npairs; ++p) {
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const bool hb = pb != nullptr;
      // the ranges of the two fields of this pair: selects between unconditional loads at constant offsets, as above -- read where
      // they are used, under `i < nsep`, the loads of the three pairs merge into ONE load of a selected address, and the whole
      // argument block goes to scratch for it (968 bytes in every kernel)
      double plo[2][NLI_MAXSEP], piv[2][NLI_MAXSEP];
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int i = 0; i < NLI_MAXSEP; ++i) {
          plo[f][i] = p == 0 ? P.lo[f][i] : p == 1 ? P.lo[2 + f][i] : P.lo[4 + f][i];
          piv[f][i] = p == 0 ? P.inv[f][i] : p == 1 ? P.inv[2 + f][i] : P.inv[4 + f][i];
        }
      for (int c = tid; c < cells; c += THREADS) hist[c] = 0u;
      MFFT_BARRIER();
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and count nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          load_pair_rows<true>(v, pa + io, (hb ? pb : pa) + io, j, P.valid_in, hb ? P.valid_in : 0, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          const bool ba = bad[0] != (T)0, bb = bad[1] != (T)0;
          // swapped results: .y = a_p, .x = b_p at position j + k TPT
          if constexpr (SPLIT) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              nlz_sync<WAVE>();
#pragma unroll
              for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = f == 0 ? v[k].y : v[k].x;
              nlz_sync<WAVE>();
              if (active) {
                const bool bf = f == 0 ? ba : bb;
#pragma unroll
                for (int i = 0; i < NLI_MAXSEP; ++i)
                  if (i < nsep) {
                    const int s = sep_of(i);
                    const double lo = plo[f][i], iv = piv[f][i];
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                      const T x1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                      const int sl = bf ? nbins + 2
                                        : incr_hist_slot(incr_value((double)x1, P.norm), incr_value((double)(f == 0 ? v[k].y : v[k].x), P.norm), lo, iv, nbins);
                      MFFT_LDS_COUNT(hist + incr_hist_cell(f, i, nsep, nb3, sl));
                    }
                  }
              }
            }
          } else {
            nlz_sync<WAVE>();
#pragma unroll
            for (int k = 0; k < E; ++k) xb[padpos<PD>(j + k * S::TPT)] = v[k];
            nlz_sync<WAVE>();
            if (active) {
#pragma unroll
              for (int i = 0; i < NLI_MAXSEP; ++i)
                if (i < nsep) {
                  const int s = sep_of(i);
                  const double loa = plo[0][i], iva = piv[0][i], lob = plo[1][i], ivb = piv[1][i];
#pragma unroll
                  for (int k = 0; k < E; ++k) {
                    const cx<T> z1 = xb[padpos<PD>(incr_pos(j + k * S::TPT, s, M))];
                    const int sa = ba ? nbins + 2 : incr_hist_slot(incr_value((double)z1.y, P.norm), incr_value((double)v[k].y, P.norm), loa, iva, nbins);
                    const int sb = bb ? nbins + 2 : incr_hist_slot(incr_value((double)z1.x, P.norm), incr_value((double)v[k].x, P.norm), lob, ivb, nbins);
                    MFFT_LDS_COUNT(hist + incr_hist_cell(0, i, nsep, nb3, sa));
                    MFFT_LDS_COUNT(hist + incr_hist_cell(1, i, nsep, nb3, sb));
                  }
                }
            }
          }
        }
      }
      MFFT_BARRIER();
      unsigned* dst = P.part + ((i64)bid * npairs + p) * cells;
      for (int c = tid; c < cells; c += THREADS) dst[c] = hist[c];
    }
  }

  // The stage that ends in plane-averaged PROFILES along z: per pair (a_p, b_p) and per position m of the row the sums over all rows
  // of d_a, d_b, d_a^2, d_b^2, d_a d_b (prof_add) -- <theta>(z), <theta'^2>(z), <u_z theta>(z) of fields that never exist in real
  // space.  After run_passes thread (rl, j) holds both values of a pair (.y = a_p, .x = b_p) at the positions j + k TPT, k < E, and
  // it holds the SAME positions for every row it meets: a per-position sum over a thread's rows is a plane sum and needs no
  // exchange between threads at all, not even a wave reduction.  The skeleton is body_incr's with the loop over the PAIRS outermost,
  // so that only one pair's accumulators are live: E x NLP_STATS doubles in registers, statically indexed, kept over all rows of
  // the workgroup.  After the rows of a pair every thread stores its E x NLP_STATS sums with plain stores into the row slot
  // (bid ROWS + rl) of P.part, laid out [row slot][pair][sum][position]: lanes with neighbouring j write neighbouring doubles, every
  // slot of every row slot and every pair of the launch is written (zeros where nothing was added), and prof_fold (profiles.hip)
  // adds the ngroups x ROWS partial profiles in fixed order: bitwise reproducible, no atomics.  No LDS beyond the transform's own.
  // Non-finite bins leave the transform on load; the thread that met one adds NaN to ITS positions of that field's two sums and of
  // the cross sum, the partner's own two sums stay what they are.  Rows past the end re-read the last row and add nothing; npairs
  // is uniform over the launch, so the barriers inside a transform are met by everybody or nobody.  Every pair has both fields
  // (the host refuses a null b).
  template <class PP>
  static MFFT_D void body_prof(const PP& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / S::TPT;
    const int j = row_thread_index<S>(tid);
    XE* xb = reinterpret_cast<XE*>(lds + TW_BYTES) + rl * PLEN;
    if constexpr (TWLDS && S::NP > 1) {
      stage_twiddles<S, T>(ltw, P.tw, tid, THREADS);
      if constexpr (WAVE) MFFT_BARRIER();
    }
    const cx<T>* tw = (TWLDS && S::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{xb, PadSlot<PD>{}};
    const i64 last = P.nrows - 1;
    const int npairs = P.npairs < NLS_PAIRS ? P.npairs : NLS_PAIRS;
#pragma unroll 1
    for (int p = 0; p < npairs; ++p) {
      double acc[E][NLP_STATS];                    // [position j + k TPT][d_a, d_b, d_a^2, d_b^2, d_a d_b]
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int s = 0; s < NLP_STATS; ++s) acc[k][s] = 0.0;
      const cx<T>* pa = p == 0 ? P.a[0] : p == 1 ? P.a[1] : P.a[2];      // (selects, not an index into the argument block)
      const cx<T>* pb = p == 0 ? P.b[0] : p == 1 ? P.b[1] : P.b[2];
      const double ca = p == 0 ? P.center[0] : p == 1 ? P.center[2] : P.center[4];
      const double cb = p == 0 ? P.center[1] : p == 1 ? P.center[3] : P.center[5];
#pragma unroll 1
      for (i64 base = (i64)bid * ROWS; 2 * base < P.nrows; base += (i64)P.ngroups * ROWS) {      // (the bound is the workgroup's)
        const i64 unit = base + rl;                // a pair of rows
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const i64 row = 2 * unit + h;
          const bool active = row < P.nrows;       // rows past the end re-read the last row and add nothing
          const i64 io = (active ? row : last) * P.in_stride;
          cx<T> v[E];
          T bad[2];
          load_pair_rows<true>(v, pa + io, pb + io, j, P.valid_in, P.valid_in, bad);
          nlz_sync<WAVE>();
          run_passes<S, 0, T>(v, j, tw, xc);
          if (active) {                            // swapped results: .y = a_p, .x = b_p at position j + k TPT
#pragma unroll
            for (int k = 0; k < E; ++k) prof_add(acc[k], incr_value((double)v[k].y, P.norm) - ca, incr_value((double)v[k].x, P.norm) - cb);
#pragma unroll
            for (int f = 0; f < 2; ++f)
              if (bad[f] != (T)0) {                // what the load took out of this field: its own sums and the cross sum are NaN
                const double nn = (double)bad[f] * 0.0;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                  acc[k][f] += nn;
                  acc[k][2 + f] += nn;
                  acc[k][4] += nn;
                }
              }
          }
        }
      }
      // row slot bid ROWS + rl < ngroups ROWS, pair p < npairs, position j + k TPT < M: inside (ngroups ROWS, npairs, NLP_STATS, M)
      double* dst = P.part + (((i64)bid * ROWS + rl) * npairs + p) * (NLP_STATS * M) + j;
#pragma unroll
      for (int s = 0; s < NLP_STATS; ++s)
#pragma unroll
        for (int k = 0; k < E; ++k) dst[s * M + k * S::TPT] = acc[k][s];
    }
  }
};

// The product of the stage as a parameter of the kernel: NlzProd<K, NlzProduct::Dot> is K's rows, exchanges and transforms
// around the dot product.  (A wrapper, not a seventh parameter of NlzFft: that would rename every cross-product kernel's
// symbol, and scripts/kernel_regs.py --diff could no longer show that they are what they were.)
enum class NlzProduct { Cross = 0, Dot = 1, CrossDot = 2, Outer = 3 };
template <class K, NlzProduct PRODUCT = NlzProduct::Cross> struct NlzProd : K {};
template <class K> struct NlzProd<K, NlzProduct::Dot> {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_dot(p, bid, tid, lds); }
};

template <class K> struct NlzProd<K, NlzProduct::CrossDot> {      // (takes NlcParams)
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_cross_dot(p, bid, tid, lds); }
};

template <class K> struct NlzProd<K, NlzProduct::Outer> {         // (takes NloParams)
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_outer(p, bid, tid, lds); }
};

// The stage that also emits the six maxima (Build::AbsMax): K's body with STATS on and NlmParams.  A wrapper again, for the
// same reason -- and the plain bodies above forward to the same templates with STATS off, which compiles to what they were.
template <class K, NlzProduct PRODUCT = NlzProduct::Cross> struct NlzAbsMax {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // slots of NlmParams::part per workgroup
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) {
    if constexpr (PRODUCT == NlzProduct::Dot) K::template body_dot_t<true>(p, bid, tid, lds);
    else K::template body_t<true>(p, bid, tid, lds);
  }
};

// The stage that ends in the reduction (Op::Moments): K's rows, exchanges and inverse transforms around body_moments, NlsParams.
template <class K> struct NlzMoments {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLS_SLOTS doubles in NlsParams::part per workgroup
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_moments(p, bid, tid, lds); }
};

// The stage that ends in the histogram (Op::Histogram): K's rows, exchanges and inverse transforms around body_hist, NlhParams; the
// two histograms of the pair at hand lie behind K's own LDS.
template <class K, bool MERGE = false> struct NlzHist {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + 2 * (NLH_MAXBINS + 3) * 4;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::template body_hist<MERGE>(p, bid, tid, lds); }
};

// The stage that ends in the joint histogram (Op::JointHistogram): K's rows, exchanges and inverse transforms around body_joint,
// NljParams; the grid of the pair at hand lies behind K's own LDS, 17956 bytes where NlzHist takes 4120.
template <class K> struct NlzJoint {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + NLJ_MAXCELLS * 4;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_joint(p, bid, tid, lds); }
};

// The stage that ends in the statistics of a quadratic form (Op::Quadratic): K's rows, exchanges and inverse transforms around
// body_quad, NlqParams; ONE histogram lies behind K's own LDS, 2060 bytes where NlzHist takes 4120.
template <class K> struct NlzQuad {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + (NLH_MAXBINS + 3) * 4;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLS_STATS doubles in NlqParams::mpart per workgroup
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_quad(p, bid, tid, lds); }
};

// The stage that ends in structure functions (Op::Increments): K's rows, exchanges and inverse transforms around body_incr,
// NliParams; no LDS beyond K's own -- the row is read back shifted out of the row's exchange buffer.
template <class K> struct NlzIncr {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  static constexpr int WAVES = (K::THREADS + 63) / 64;       // groups of NLI_SLOTS doubles in NliParams::part per workgroup
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_incr(p, bid, tid, lds); }
};

// The stage that ends in increment histograms (Op::IncrementHistogram): K's rows, exchanges and inverse transforms around
// body_incr_hist, NlkParams; the histograms of the pair at hand lie behind K's own LDS, 16576 bytes where NlzJoint takes 17956.
template <class K> struct NlzIncrHist {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES + NLK_MAXCELLS * 4;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_incr_hist(p, bid, tid, lds); }
};

// The stage that ends in plane-averaged profiles along z (Op::Profiles): K's rows, exchanges and inverse transforms around
// body_prof, NlpParams; no LDS beyond K's own -- the sums live in registers and leave by plain stores.
template <class K> struct NlzProf {
  static constexpr int THREADS = K::THREADS, LDS_BYTES = K::LDS_BYTES;
  template <class P> static MFFT_D void body(const P& p, int bid, int tid, char* lds) { K::body_prof(p, bid, tid, lds); }
};

// ---------------------------------------------------------------------------
// The same stage for the 3/2-rule, M = 3 L with the L + 1 bins of the un-padded mesh per row (N = 2 L): PRUNED transforms.
// With n = 3 m + s the inverse transform of a spectrum that is zero outside |k| <= L falls apart into three transforms of
// length L,
//     z[3m + s] = sum_{kappa < L} e^{2 pi i kappa m / L} Y_s[kappa],   Y_s[kappa] = W^{kappa s} (Z[kappa] + w^{-s} Z[kappa - L])
// (W = e^{2 pi i / M}, w = W^L = e^{2 pi i / 3}; kappa = 0 also takes Z[L] w^s), and forward the bins 0..L are
//     Z'[k] = sum_s conj(W^{sk}) F_s[k mod L],   F_s = DFT_L of r[3m + s].
// The radix-3 pass over a spectrum that is one third zeros is never run, and -- what decides -- the three sub-transforms go
// to three thread groups of SL::TPT threads with SL::E values each: a row of 768 points is 192 threads with 4 - 8 values
// instead of 64 threads with 12, the parked fields (2 E complex + E real per thread) shrink with it and the kernel runs at
// 3 - 5 waves per SIMD where NlzFft<Spec<768, 12, ..>> sits at 256 registers with scratch (1.7 - 2.0 TB/s against 4.1 - 4.5 for the
// 8-values plans of the powers of two: profiles/r06_nlz_variants.txt).  The rows of the six fields are staged through LDS
// (every bin is read from memory once; a thread needs the bins kappa and L - kappa of both fields of a pair), the forward
// combination reads the three F_s back out of LDS.  Same arithmetic contract as NlzFft with valid = L + 1.
// (A prefetching build -- the rows of the NEXT pair of fields loaded into three more registers per thread while the passes of the
// current pair run; hipcc's workgroup barrier waits for LDS only, so the loads do stay in flight -- was exact and SLOWER: 768
// 1.39 -> 1.64 ms, 1536 1.92 -> 2.10, profiles/r06_nlz_variants.txt section 4.  Removed.)
template <class SL, typename T, int ROWS, bool TWLDS>
struct Nlz3Fft {
  static constexpr int L = SL::N, M = 3 * SL::N, E = SL::E, TPT = SL::TPT, G = 3 * SL::TPT;
  static constexpr int THREADS = G * ROWS;
  static constexpr int PD = SL::R(0);
  static constexpr int PLEN = padded_len<L, PD>();                      // >= L + 1
  static constexpr int TW_BYTES = (TWLDS && SL::NP > 1) ? (int)(SL::TW * sizeof(cx<T>)) : 0;
  static constexpr int XCH_BYTES = (int)(3 * PLEN * ROWS * sizeof(cx<T>));
  static constexpr int LDS_BYTES = TW_BYTES + XCH_BYTES;
  static constexpr int NSTAGE = (2 * (L + 1) + G - 1) / G;              // staging rounds of a pair of rows of L + 1 bins
  static constexpr int NOUT = (L + 1 + G - 1) / G;                      // output bins per thread
  typedef XchFull<T, PadSlot<PD>> Xch;

  // Y_s of this thread's positions out of the staged rows (see the header), ready for the inverse passes
  static MFFT_D void combine(cx<T> (&v)[E], int s, int j, const cx<T>* B, const cx<T>* rt) {
    const T h3 = (T)0.866025403784438646764L;
    const T wr = s == 0 ? (T)1 : (T)-0.5, wi = s == 0 ? (T)0 : (s == 1 ? -h3 : h3);      // w^{-s}: 1, conj(w), w
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int kap = j + k * TPT;
      cx<T> a = B[kap], b = B[L + 1 + kap];
      const cx<T> am = B[L - kap], bm = B[2 * L + 1 - kap];
      if (kap == 0) { a.y = (T)0; b.y = (T)0; }    // Im of the k = 0 bins is ignored (as c2r does)
      const cx<T> u = mk<T>(a.x - b.y, a.y + b.x);                      // Z[kappa]     = a + i b
      const cx<T> vm = mk<T>(am.x + bm.y, bm.x - am.y);                 // Z[kappa - L] = conj(am) + i conj(bm)
      cx<T> y = mk<T>(u.x + wr * vm.x - wi * vm.y, u.y + wr * vm.y + wi * vm.x);
      if (kap == 0) {                              // ... and Z[L] w^s = (am + i bm) conj(w^{-s})
        const cx<T> zl = mk<T>(am.x - bm.y, am.y + bm.x);
        y = mk<T>(y.x + wr * zl.x + wi * zl.y, y.y + wr * zl.y - wi * zl.x);
      }
      if (s != 0) y = y * rt[(s - 1) * (L + 1) + kap];                  // W^{kappa s}
      v[k] = swapri(y);
    }
  }
  template <class TwPtr>
  static MFFT_D void inverse_pair(cx<T> (&v)[E], const cx<T>* ra, const cx<T>* rb, int t, int s, int j, cx<T>* B,
                                  const cx<T>* rt, TwPtr tw, Xch& xc) {
    // The kernel body holds five transforms; left alone, hipcc shares every LDS address between them and keeps all of them
    // live from the first to the last (E = 8 in double precision: 256 VGPRs where ONE transform needs ~80).  Hiding the
    // thread indices at the head of each transform makes their address arithmetic local to it again.
    MFFT_HIDE_RANGE(t);
    MFFT_HIDE_RANGE(j);
    MFFT_BARRIER();                                // B is free
#pragma unroll
    for (int ii = 0; ii < NSTAGE; ++ii) {          // the L + 1 bins of both rows, each read from memory once
      const int i = t + ii * G;
      const int ic = i < 2 * (L + 1) ? i : 2 * (L + 1) - 1;
      const cx<T>* src = ic <= L ? ra + ic : rb + (ic - (L + 1));       // one unconditional load of a selected address
      const cx<T> x = *src;
      if (i < 2 * (L + 1)) B[i] = x;
    }
    MFFT_BARRIER();
    combine(v, s, j, B, rt);
    MFFT_BARRIER();                                // the staged rows are consumed: B becomes the exchange buffer
    run_passes<SL, 0, T>(v, j, tw, xc);
  }

  template <class TwPtr>
  static MFFT_D void forward_pair(cx<T> (&v)[E], int t, int s, int j, cx<T>* B, const cx<T>* rt, TwPtr tw, Xch& xc,
                                  cx<T>* oa, cx<T>* ob, bool sa, bool sb) {
    MFFT_HIDE_RANGE(t);
    MFFT_HIDE_RANGE(j);
    MFFT_BARRIER();
    run_passes<SL, 0, T>(v, j, tw, xc);
    if constexpr (SL::NP > 1) MFFT_BARRIER();      // everybody's last gather: the padded regions are dead
#pragma unroll
    for (int k = 0; k < E; ++k) B[s * L + j + k * TPT] = v[k];          // F_s, plain layout
    MFFT_BARRIER();
    const T half = (T)0.5;
#pragma unroll
    for (int ii = 0; ii < NOUT; ++ii) {
      const int k = t + ii * G;
      if (k <= L) {
        const int k1 = k == L ? 0 : k, k2 = k == 0 ? 0 : L - k;
        const cx<T> w1 = rt[k], w2 = rt[L + 1 + k];
        const cx<T> zk = B[k1] + conj(w1) * B[L + k1] + conj(w2) * B[2 * L + k1];      // Z'[k]
        const cx<T> zm = conj(B[k2] + w1 * B[L + k2] + w2 * B[2 * L + k2]);            // conj Z'[M - k]
        if (sa) oa[k] = scale(zk + zm, half);
        if (sb) ob[k] = mul_mi(scale(zk - zm, half));
      }
    }
  }

  static MFFT_D void body(const NlzParams<T>& P, int bid, int tid, char* lds) {
    cx<T>* ltw = reinterpret_cast<cx<T>*>(lds);
    const int rl = tid / G, t = tid - rl * G;
    const int s = t / TPT, j = t - s * TPT;
    cx<T>* B = reinterpret_cast<cx<T>*>(lds + TW_BYTES) + rl * 3 * PLEN;
    if constexpr (TWLDS && SL::NP > 1) stage_twiddles<SL, T>(ltw, P.tw, tid, THREADS);     // (the first barrier covers it)
    const cx<T>* tw = (TWLDS && SL::NP > 1) ? (const cx<T>*)ltw : P.tw;
    Xch xc{B + s * PLEN, PadSlot<PD>{}};
    const i64 unit = (i64)bid * ROWS + rl;         // a pair of rows
    T r2a[E];
#pragma unroll
    for (int k = 0; k < E; ++k) r2a[k] = (T)0;
    bool sa = false;
    i64 rowa = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const i64 row = 2 * unit + h;
      const bool active = row < P.nrows;
      const i64 io = (active ? row : P.nrows - 1) * P.in_stride;
      cx<T> pk[2][E];
      cx<T> v[E];
      inverse_pair(v, P.a[0] + io, P.b[0] + io, t, s, j, B, P.rt3, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) pk[0][k] = v[k];
      inverse_pair(v, P.a[1] + io, P.b[1] + io, t, s, j, B, P.rt3, tw, xc);
#pragma unroll
      for (int k = 0; k < E; ++k) pk[1][k] = v[k];
      inverse_pair(v, P.a[2] + io, P.b[2] + io, t, s, j, B, P.rt3, tw, xc);
      T r2[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {                // swapped results: .y = a_f, .x = b_f at n = 3 (j + k TPT) + s
        const T a0 = pk[0][k].y, a1 = pk[1][k].y, a2 = v[k].y;
        const T b0 = pk[0][k].x, b1 = pk[1][k].x, b2 = v[k].x;
        v[k] = mk<T>((a1 * b2 - a2 * b1) * P.scale, (a2 * b0 - a0 * b2) * P.scale);
        r2[k] = (a0 * b1 - a1 * b0) * P.scale;
      }
      const i64 oo = row * P.out_stride;
      forward_pair(v, t, s, j, B, P.rt3, tw, xc, P.out[0] + oo, P.out[1] + oo, active, active);
      if (h == 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) r2a[k] = r2[k];
        sa = active;
        rowa = row;
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = mk<T>(r2a[k], r2[k]);
        forward_pair(v, t, s, j, B, P.rt3, tw, xc, P.out[2] + rowa * P.out_stride, P.out[2] + oo, sa, active);
      }
    }
  }
};

}  // namespace mfft
