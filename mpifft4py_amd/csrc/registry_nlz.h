// registry_nlz.h -- registration of the fused nonlinear z-stage kernels (fft_nlz.h); included by kernels_nlz_*.hip only, so
// that an edit of those kernels does not rebuild every translation unit.
#pragma once
#include "registry.h"
#include "fft_nlz.h"
#include "nlz_moments.h"
#include "nlz_hist.h"
#include "nlz_joint.h"
#include "nlz_quad.h"
#include "nlz_incr.h"
#include "nlz_incr_hist.h"
#include "nlz_prof.h"

namespace mfft {

// Round 6: the fused nonlinear z stage (fft_nlz.h NlzFft), one kernel per (length, precision).  256 threads per workgroup
// where a row has fewer; whole complex values through LDS while two workgroups (with their twiddle tables) fit a CU,
// real and imaginary parts one after the other beyond; the twiddles in LDS while the table stays under 48 KB.  The register
// cap asks for two waves per SIMD: the kernel parks 5 E real values per thread next to a transform's working set.
template <class S, typename T> constexpr int nlz_rows() { return 256 / S::TPT > 0 ? 256 / S::TPT : 1; }
template <class S, typename T> constexpr bool nlz_twlds() { return S::NP > 1 && (long long)S::TW * (int)sizeof(cx<T>) <= 49152; }
template <class S, typename T> constexpr bool nlz_split() {
  constexpr long long tw = nlz_twlds<S, T>() ? (long long)S::TW * (int)sizeof(cx<T>) : 0;
  return tw + (long long)padded_len<S::N, S::R(0)>() * nlz_rows<S, T>() * (int)sizeof(cx<T>) > 81920;
}
#ifndef MFFT_NLZ_OCC
#define MFFT_NLZ_OCC 2
#endif
// wave-synchronous build (fft_nlz.h NlzFft WAVE): rows inside one wave, no workgroup barriers in the transforms
#ifndef MFFT_NLZ_WAVE
#define MFFT_NLZ_WAVE 1
#endif
template <class S, typename T> constexpr bool nlz_wave() {
  return MFFT_NLZ_WAVE && S::TPT <= 64 && 64 % S::TPT == 0 && !nlz_split<S, T>();
}
template <class S, typename T>
void register_nlz(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;        // waves per SIMD, said directly (registry.h mfft_kern_occ)
  reg.push_back(make_entry<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>, NlzParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Plain, Build::Default, R, name));
}

// The same rows around the dot product (fft_nlz.h body_dot; Op::Dot).  It parks 2 E reals where the cross product parks 5 E, so
// the register cap was derived again: what the compiler needs under each cap (profiles/nonlinear_dot_regs.tsv, VGPRs / bytes of scratch
// per lane at 2, 3 and 4 waves per SIMD), then the candidates against each other on the device (profiles/nonlinear_dot_ab.txt,
// section 3: one process, two builds of the library, alternating windows).
//   12 values per thread (3 * 2^a, 9 * 2^a, 27 * 2^a), both precisions:  226 - 256 VGPRs at two waves WITHOUT the 8 - 500 bytes of
//     scratch of their cross-product kernels (216 / 24 / 96 / 384 in double precision keep 8 - 80 bytes) -- but ONE transform of 12
//     complex values with its twiddles already takes more than the 168 registers of three waves: 60 - 460 bytes of scratch there.
//     Two waves, as the cross product.
//   8 values (2^a), double precision:  129 - 164 VGPRs under a three-wave cap, no scratch -- and SLOWER than the two-wave build, which
//     takes 150 - 162 by itself: 512: 0.391 -> 0.534 ms, 1024: 0.655 -> 0.871, 2048: 0.730 -> 0.898, 256: 0.204 -> 0.290.  Two waves.
//   8 values, single precision:  114 - 128 VGPRs under a four-wave cap, no scratch.  Ahead from 1024 on (1024: 0.477 -> 0.412 ms,
//     2048: 0.489 -> 0.428), behind at 512 (0.213 -> 0.250), even at 256 (three waves).  Four waves at 1024 and 2048, the
//     lengths measured (4096, 512-thread workgroups, was not: two waves).
// Rows per workgroup and the twiddle placement are the cross kernels' (nlz_rows, nlz_twlds); the exchange buffers go to real /
// imaginary halves where the workgroups the cap admits, with their twiddle tables, would not fit the CU's 160 KB (nld_split:
// with two waves per SIMD that is the cross kernels' rule, so every double-precision kernel has its twin's exchange).
// MFFT_NLD_OCC = 2, 3, 4 forces one cap for every plan (0: none): the builds that were measured against each other.
#ifndef MFFT_NLD_OCC
#define MFFT_NLD_OCC -1
#endif
template <class S, typename T> constexpr int nld_occ() {
  if (MFFT_NLD_OCC >= 0) return MFFT_NLD_OCC;
  if (S::E == 8 && sizeof(T) == 4 && (S::N == 1024 || S::N == 2048)) return 4;
  return 2;
}
template <class S, typename T> constexpr int nld_rows() { return nlz_rows<S, T>(); }          // (rows and twiddle placement: the cross
template <class S, typename T> constexpr bool nld_twlds() { return nlz_twlds<S, T>(); }      // kernels' rules, not measured again)
template <class S, typename T> constexpr bool nld_split() {
  constexpr long long tw = nld_twlds<S, T>() ? (long long)S::TW * (int)sizeof(cx<T>) : 0;
  // workgroups per CU that the cap leaves registers for: a workgroup takes ceil(waves / 4) waves' registers on every SIMD
  // (registry.h, the dispatcher's rule); never fewer than two, the cross kernels' budget
  constexpr int waves = (S::TPT * nld_rows<S, T>() + 63) / 64;
  constexpr int wgs = nld_occ<S, T>() / ((waves + 3) / 4) > 2 ? nld_occ<S, T>() / ((waves + 3) / 4) : 2;
  return (tw + (long long)padded_len<S::N, S::R(0)>() * nld_rows<S, T>() * (int)sizeof(cx<T>)) * wgs > 163840;
}
template <class S, typename T> constexpr bool nld_wave() {
  return MFFT_NLZ_WAVE && S::TPT <= 64 && 64 % S::TPT == 0 && !nld_split<S, T>();
}
template <class S, typename T>
void register_nld(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nld_rows<S, T>();
  constexpr int W = nld_occ<S, T>() > 1 ? 16 + nld_occ<S, T>() : 0;
  typedef NlzProd<NlzFft<S, T, R, nld_twlds<S, T>(), nld_split<S, T>(), nld_wave<S, T>()>, NlzProduct::Dot> K;
  reg.push_back(make_entry<K, NlzParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Dot, Build::Default, R, name));
}

// Build::AbsMax: both products once more, with the six real-space maxima emitted (fft_nlz.h NlzAbsMax; kernels_nlm*.hip).  Rows,
// twiddle placement, exchange and register cap are those of the kernel it shadows (register_nlz / register_nld): the statistic
// adds two live values per thread for the length of one wave reduction, and two more (`bad`: the non-finite input met on load)
// that live across every inverse transform, plus two selects per value to put the NaNs back -- the double-precision 12-values
// plans from 192 upward hold 24 - 128 bytes more scratch than the kernel they shadow (profiles/nonlinear_absmax_regs.tsv).  One exception: the
// single-precision dot kernels of 1024 and 2048 run under a four-wave cap (nld_occ) that the plain kernel fills to the last of
// its 128 registers; with the reduction it spills 130 bytes and more per lane there, so the variant takes three waves (168: 24 bytes).
template <class S, typename T>
void register_nlm(const char* name) {
  auto& reg = kernel_registry();
  {
    constexpr int R = nlz_rows<S, T>();
    constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
    typedef NlzAbsMax<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>, NlzProduct::Cross> K;
    reg.push_back(make_entry<K, NlmParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Plain, Build::AbsMax, R, name));
  }
  {
    constexpr int R = nld_rows<S, T>();
    constexpr int O = nld_occ<S, T>() == 4 ? 3 : nld_occ<S, T>();
    constexpr int W = O > 1 ? 16 + O : 0;
    typedef NlzAbsMax<NlzFft<S, T, R, nld_twlds<S, T>(), nld_split<S, T>(), nld_wave<S, T>()>, NlzProduct::Dot> K;
    reg.push_back(make_entry<K, NlmParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Dot, Build::AbsMax, R, name));
  }
}

// Op::CrossDot: the cross product of a and b AND the dot product of a and a third field c in one pass over the rows (fft_nlz.h
// body_cross_dot, NlcParams; kernels_nlc*.hip).  Rows, twiddle placement, exchange, wave-synchronous build and the two-waves-per-SIMD
// cap are the cross kernels' (nlz_rows, nlz_twlds, nlz_split, nlz_wave, MFFT_NLZ_OCC): the body parks 6 E reals where the cross body
// parks 5 E, and inlines seven transforms where it inlines five: every double-precision kernel takes all 256 VGPRs of the cap AND
// scratch, where the 8-values twins take 166 - 244 and none (profiles/nonlinear_cross_dot_regs.tsv).  No other cap was measured.
template <class S, typename T>
void register_nlc(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzProd<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>, NlzProduct::CrossDot> K;
  reg.push_back(make_entry<K, NlcParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::CrossDot, Build::Default, R, name));
}

// Op::Outer: all nine products a_i b_j in one pass over the rows (fft_nlz.h body_outer, NloParams; kernels_nlo*.hip): six rows in,
// nine out.  Rows, twiddle placement, exchange, wave-synchronous build and the two-waves-per-SIMD cap are the cross kernels', as
// register_nlc's are: the body parks 7 E reals next to its first forward transform where body_cross_dot parks 6 E, and inlines
// eight transforms (profiles/nonlinear_outer_regs.tsv).  No other cap was measured.
template <class S, typename T>
void register_nlo(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzProd<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>, NlzProduct::Outer> K;
  reg.push_back(make_entry<K, NloParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Outer, Build::Default, R, name));
}

// Op::Moments: the stage that ends in a reduction (nlz_moments.h NlzMoments::body, NlsParams; kernels_nls*.hip).  Rows, twiddle placement,
// exchange, wave-synchronous build and the two-waves-per-SIMD cap are the cross kernels': the body inlines ONE transform where
// the cross body inlines five and parks no row, but holds 36 doubles of accumulators for the whole launch: no scratch in single
// precision, 36 - 196 bytes in the double-precision 12-values plans from 192 on (profiles/real_moments_regs.tsv).  No other cap
// was measured.
template <class S, typename T>
void register_nls(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzMoments<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NlsParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Moments, Build::Default, R, name));
}

// Op::Histogram: the stage that ends in a histogram (nlz_hist.h NlzHist::body, NlhParams; kernels_nlh*.hip).  Rows, twiddle placement,
// exchange, wave-synchronous build and the two-waves-per-SIMD cap are the cross kernels', as the moments kernels' are: the body
// inlines ONE transform and keeps its counts in LDS, 2 x (NLH_MAXBINS + 3) x 4 = 4120 bytes behind the exchange buffers
// (DESIGN.md 7 has the table of LDS bytes and resident workgroups per plan).
// MFFT_NLH_MERGE=1 builds the variant that merges runs of equal slot inside the wave before the add (nlz_hist.h lds_count_runs;
// `make nlh_variant`): measured against the plain add, profiles/real_histogram_ab.txt, and not shipped.
#ifndef MFFT_NLH_MERGE
#define MFFT_NLH_MERGE 0
#endif
template <class S, typename T>
void register_nlh(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzHist<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>, MFFT_NLH_MERGE != 0> K;
  reg.push_back(make_entry<K, NlhParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Histogram, Build::Default, R, name));
}

// Op::Quadratic: the stage that ends in the statistics of a quadratic form of its fields (nlz_quad.h NlzQuad::body, NlqParams;
// kernels_nlq*.hip).  Rows, twiddle placement, exchange, wave-synchronous build and the two-waves-per-SIMD cap are those of
// register_nls: the body inlines ONE transform, holds E doubles of running sum and 6 accumulators across it where NlzMoments::body holds
// 36, and keeps ONE histogram in LDS, (NLH_MAXBINS + 3) x 4 = 2060 bytes behind the exchange buffers (DESIGN.md 7:
// profiles/real_quadratic_regs.tsv, and the table of LDS bytes and resident workgroups).  No other cap was measured.
template <class S, typename T>
void register_nlq(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzQuad<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NlqParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Quadratic, Build::Default, R, name));
}

// Op::Increments: the stage that ends in structure functions along z (nlz_incr.h NlzIncr::body, NliParams; kernels_nli*.hip).  Rows,
// twiddle placement, exchange, wave-synchronous build and the two-waves-per-SIMD cap are those of register_nls: the body inlines ONE
// transform and holds ONE pair's accumulators across it, 2 x NLI_MAXSEP x 3 = 48 doubles where NlzMoments::body holds 36, and takes no
// LDS of its own (profiles/real_increments_regs.tsv).  No other cap was measured.
template <class S, typename T>
void register_nli(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzIncr<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NliParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Increments, Build::Default, R, name));
}

// Op::JointHistogram: the stage that ends in a joint histogram (nlz_joint.h NlzJoint::body, NljParams; kernels_nlj*.hip).  Rows, twiddle
// placement and the two-waves-per-SIMD cap are those of register_nlh: the body inlines ONE transform, computes the two slots that
// NlzHist::body computes and issues one LDS add where it issues two.  What differs is the LDS: the grid takes NLJ_MAXCELLS x 4 = 17956
// bytes behind the exchange buffers where the histograms take 4120, so the exchange has a rule of its own (nlj_split): whole complex
// values where twiddles + exchange + grid stay within the 81920 bytes that keep two workgroups on a CU, real and imaginary halves
// in turn beyond.  Every kernel whose twin has TWO resident workgroups by LDS keeps them, but for 3072 points in double precision,
// whose twin is split already (eight kernels in all hold one fewer than the twin, six of them three -> two).  The
// rule changes double precision 768, 1296, 1536, 2048, 2304, 4096 and single precision 4096; of these 768 was a wave build and
// becomes a barrier build (nlz_wave needs the whole exchange).  DESIGN.md 7 has the table and what was measured.  MFFT_NLJ_TWIN=1 builds the alternative (`make nlj_variant`): the twin's exchange and wave build,
// one resident workgroup fewer where the grid does not fit (scripts/real_joint_ab.py).  Measured on the device, z stage alone
// (profiles/real_joint_ab.txt): the rule wins by 1.4 - 1.7 x for the double-precision kernels of 768 .. 2304 points and by 1.4 x for
// 4096 in single precision, which it gives a second workgroup.  The ONE exception: 4096 points in double precision, 512 threads
// and 180 VGPRs, keeps one workgroup by REGISTERS whichever exchange it has; halving the exchange buys nothing there and
// the twin's whole exchange is 1.3 x faster: it keeps the twin's.
#ifndef MFFT_NLJ_TWIN
#define MFFT_NLJ_TWIN 0
#endif
template <class S, typename T> constexpr bool nlj_split() {
  if (MFFT_NLJ_TWIN || (sizeof(T) == 8 && S::N == 4096)) return nlz_split<S, T>();
  constexpr long long tw = nlz_twlds<S, T>() ? (long long)S::TW * (int)sizeof(cx<T>) : 0;
  return tw + (long long)padded_len<S::N, S::R(0)>() * nlz_rows<S, T>() * (int)sizeof(cx<T>) + (long long)NLJ_MAXCELLS * 4 > 81920;
}
template <class S, typename T> constexpr bool nlj_wave() {
  return MFFT_NLZ_WAVE && S::TPT <= 64 && 64 % S::TPT == 0 && !nlj_split<S, T>();
}
template <class S, typename T>
void register_nlj(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzJoint<NlzFft<S, T, R, nlz_twlds<S, T>(), nlj_split<S, T>(), nlj_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NljParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::JointHistogram, Build::Default, R, name));
}

// Op::IncrementHistogram: the stage that ends in increment histograms along z (nlz_incr_hist.h NlzIncrHist::body, NlkParams;
// kernels_nlk*.hip).  Rows, twiddle placement, the two-waves-per-SIMD cap, the exchange and the wave build are those of
// register_nlj, unchanged (nlj_split, nlj_wave): the pair's histograms take NLK_MAXCELLS x 4 = 16576 bytes behind the exchange
// buffers, under the joint grid's 17956, so whatever the joint rule keeps resident stays resident here.  The body inlines ONE
// transform and holds NO accumulators: a slot and an LDS add per increment (profiles/real_increment_histogram_regs.tsv).  No other
// rule or cap was measured.
template <class S, typename T>
void register_nlk(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzIncrHist<NlzFft<S, T, R, nlz_twlds<S, T>(), nlj_split<S, T>(), nlj_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NlkParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::IncrementHistogram, Build::Default, R, name));
}

// Op::Profiles: the stage that ends in plane-averaged profiles along z (nlz_prof.h NlzProf::body, NlpParams; kernels_nlp*.hip).  Rows,
// twiddle placement, exchange, wave-synchronous build and the two-waves-per-SIMD cap are those of register_nls: the body inlines ONE
// transform and holds ONE pair's accumulators across it, E x NLP_STATS doubles -- 40 for the 8-values plans, 60 for the 12-values
// plans, where NlzMoments::body holds 36 and NlzIncr::body 48 --, and takes no LDS of its own (profiles/real_profiles_regs.tsv).  No other
// cap was measured.
template <class S, typename T>
void register_nlp(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz_rows<S, T>();
  constexpr int W = MFFT_NLZ_OCC > 1 ? 16 + MFFT_NLZ_OCC : 0;
  typedef NlzProf<NlzFft<S, T, R, nlz_twlds<S, T>(), nlz_split<S, T>(), nlz_wave<S, T>()>> K;
  reg.push_back(make_entry<K, NlpParams<T>, S, T, W>(FAM_NLZ, S::N, 0, Op::Profiles, Build::Default, R, name));
}

// ... and its pruned 3/2-rule flavour (Nlz3Fft: Build::Nlz3, entry.n = M = 3 L): three thread groups of SL::TPT threads per row
template <class SL, typename T> constexpr int nlz3_rows() { return 256 / (3 * SL::TPT) > 0 ? 256 / (3 * SL::TPT) : 1; }
template <class SL, typename T>
void register_nlz3(const char* name) {
  auto& reg = kernel_registry();
  constexpr int R = nlz3_rows<SL, T>();
  reg.push_back(make_entry<Nlz3Fft<SL, T, R, true>, NlzParams<T>, SL, T>(FAM_NLZ, 3 * SL::N, 0, Op::Plain, Build::Nlz3, R, name));
}

}  // namespace mfft
