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
//
// This file holds the transform and the four PRODUCTS (cross, dot, cross-and-dot, outer), which share forward_pair and stats.  The
// endings that REDUCE instead (moments, histograms, ..) are a header each, nlz_*.h: parameters, rule and body in one place, the
// body a member of the wrapper NlzMoments<K> .. NlzProf<K> around a kernel K = NlzFft<..> of this file.
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

// Maximum that KEEPS a NaN (fmax drops it): a blown-up field must not report a finite maximum.  m is sticky once NaN.
template <typename T> MFFT_D T nan_max(T m, T x) { return (x > m || x != x) ? x : m; }
template <typename T> MFFT_D T nan_min(T m, T x) { return (x < m || x != x) ? x : m; }
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
  // the template parameters under member names: what a wrapper around this kernel reaches them by (nlz_reduce.h MFFT_NLZ_NAMES_OF)
  typedef S Plan;
  typedef T Real;
  static constexpr int NROWS = ROWS;
  static constexpr bool TW_LDS = TWLDS, SPLIT_XCH = SPLIT, WAVE_XCH = WAVE;

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
