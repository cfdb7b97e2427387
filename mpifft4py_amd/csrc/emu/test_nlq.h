// test_nlq.h -- emulator tests of the fused z stage that ends in the statistics of a quadratic form (nlz_quad.h NlzQuad::body,
// Op::Quadratic): q = sum_f w_f r_f^2 over up to six real fields, its [min, max, S1 .. S4] and its counts in equal bins, against
// long-double transforms of the rows.  With delta the worst-case error of a row of a PAIR (test_nlh.h: 8 eps log2(M) sum_k h_k
// (|A_k| + |B_k|) / M over both fields of the transform) the pointwise bound of q is
//     dq = sum_f |w_f| (2 |r_f| delta_f + delta_f^2) + (n + 1) 2^-53 sum_f |w_f| r_f^2        (n fields: n products, n sums)
// and with d = q - c:  min and max within max dq;  |S_p - ref| <= sum p dq (|d| + dq)^(p - 1) + (cnt + 8) 2^-52 sum |d|^p;  the
// cumulative counts bracketed by those of q_ref + dq and q_ref - dq (the slot rule is monotone).  A bound, not a measurement.
#pragma once
#include "nlz_quad.h"
#include "test_nlz.h"

struct NlqCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 1, ngroups = 1, nbins = 64;
  bool negative = false, center = false;
  int bad_field = -1;
  bool inf = false;
};
// the documented rule on the host, from values already in double (include/mpifft4py_amd.h): the emulator is built without
// contraction, so this is two roundings per product pair and one per sum
static double nlq_rule(const double* r, const double* w, int n) {
  double q = 0.0;
  for (int f = 0; f < n; ++f) q = q + (w[f] * r[f]) * r[f];
  return q;
}

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nlq(const NlqCase& c) {      // broken bounds, brackets and contracts, counted; 0 is a pass
  typedef NlzQuad<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields, nbins = c.nbins;
  const int pin = valid + 2, nb3 = nbins + 3;
  const bool two = nf % 2 == 0;                      // a and b: field f of a rides with field f of b
  const int ncomp = two ? nf / 2 : nf, npairs = (nf + 1) / 2;
  NlzFixture<S, T> fx(nf, 6161 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  fx.snapshot();
  int slot_of[6];
  double w[6] = {0, 0, 0, 0, 0, 0};                  // by slot
  for (int f = 0; f < nf; ++f) {
    slot_of[f] = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
    w[slot_of[f]] = 0.75 * (f + 1);
  }
  if (c.negative) w[slot_of[1 % nf]] = -1.25;
  // the reference q, point by point, and its bound
  const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-7;
  const size_t cnt = (size_t)nrows * M;
  std::vector<long double> qref(cnt, 0.0L), dq(cnt, 0.0L), wr2(cnt, 0.0L);
  std::vector<std::vector<double>> delta(npairs, std::vector<double>(nrows, 0.0));
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) {
      const cx<T>* z = in[f].data() + (size_t)r * pin;
      long double s = 0;
      for (int q = 0; q < vin; ++q) {
        const bool self = q == 0 || (M % 2 == 0 && q == M / 2);
        s += (self ? 1 : 2) * (fabsl((long double)z[q].x) + (self ? 0 : fabsl((long double)z[q].y)));
      }
      delta[slot_of[f] / 2][r] += (double)(8 * eps * log2((double)M) * s / M);
    }
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) {
      const lreal x = nl_real_row(in[f].data() + (size_t)r * pin, vin, M);
      const long double d = delta[slot_of[f] / 2][r], aw = fabsl((long double)w[slot_of[f]]);
      for (int p = 0; p < M; ++p) {
        const size_t i = (size_t)r * M + p;
        qref[i] += (long double)w[slot_of[f]] * x[p] * x[p];
        wr2[i] += aw * x[p] * x[p];
        dq[i] += aw * (2 * fabsl(x[p]) * d + d * d);
      }
    }
  long double mn = INFINITY, mx = -INFINITY, dqmax = 0;
  for (size_t i = 0; i < cnt; ++i) {
    dq[i] += (nf + 1) * 1.1102230246251565e-16L * wr2[i];
    mn = std::min(mn, qref[i]); mx = std::max(mx, qref[i]); dqmax = std::max(dqmax, dq[i]);
  }
  // a range that leaves points on both sides: the tails are part of the contract
  const double lo = (double)(mn + 0.10L * (mx - mn)), hi = (double)(mx - 0.15L * (mx - mn));
  const double ctr = c.center ? (double)(0.5L * (mn + mx)) : 0.0;
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  if (c.bad_field >= 0) {
    in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
    fx.snapshot();
  }
  NlqParams<T> P;
  fx.params(P, valid, vin, M);
  for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; }      // the fields go where their slots are
  for (int f = 0; f < nf; ++f) (slot_of[f] % 2 ? P.b : P.a)[slot_of[f] / 2] = in[f].data();
  for (int i = 0; i < 6; ++i) P.w[i] = w[i];
  P.scale = (T)1;
  P.center = ctr; P.norm = 1.0 / (double)M; P.lo = lo; P.inv = nbins > 0 ? (double)nbins / (hi - lo) : 1.0;
  P.nbins = nbins; P.npairs = npairs; P.ngroups = grid;
  std::vector<double> mpart((size_t)grid * K::WAVES * NLS_STATS, -7.0);
  std::vector<unsigned> hpart((size_t)grid * nb3, 0xFFFFFFFFu);
  P.mpart = mpart.data(); P.hpart = hpart.data();
  emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  double bad = fx.inputs_changed() ? 1 : 0;          // the inputs are preserved
  for (double v : mpart)
    if (v == -7.0) bad += 1;                         // a slot nobody wrote
  std::vector<long long> h(nb3, 0);
  for (size_t i = 0; i < hpart.size(); ++i) {
    if (hpart[i] == 0xFFFFFFFFu) bad += 1;
    h[i % nb3] += hpart[i];                          // the fold: the workgroups' rows in order
  }
  double got[6] = {INFINITY, -INFINITY, 0, 0, 0, 0};
  for (size_t wv = 0; wv < mpart.size() / NLS_STATS; ++wv) {      // ... and the waves' slots in order
    const double* q = mpart.data() + wv * NLS_STATS;
    got[0] = (q[0] < got[0] || q[0] != q[0]) ? q[0] : got[0];
    got[1] = emu_nan_max(got[1], q[1]);
    for (int k = 2; k < 6; ++k) got[k] += q[k];
  }
  long long sum = 0;
  for (int s = 0; s < nb3; ++s) sum += h[s];
  if (nbins > 0 ? sum != (long long)cnt : sum != 0) bad += 1;      // every point is in exactly one slot; no bins, no counts
  if (c.bad_field >= 0) {                            // NaN sums, NaN min and max, counts in the non-finite slot
    for (int k = 0; k < 6; ++k)
      if (got[k] == got[k]) bad += 1;
    if (nbins > 0 && h[nbins + 2] < 1) bad += 1;
    return bad;
  }
  for (int k = 0; k < 6; ++k)
    if (got[k] != got[k]) bad += 1;
  if (fabsl(got[0] - mn) > dqmax || fabsl(got[1] - mx) > dqmax) bad += 1;
  long double sp[5] = {0, 0, 0, 0, 0}, sa[5] = {0, 0, 0, 0, 0}, se[5] = {0, 0, 0, 0, 0};
  for (size_t i = 0; i < cnt; ++i) {
    const long double d = qref[i] - (long double)ctr, ad = fabsl(d) + dq[i];
    long double dp = 1, ap = 1;                       // d^(p - 1), (|d| + dq)^(p - 1)
    for (int p = 1; p <= 4; ++p) {
      se[p] += p * dq[i] * ap;
      dp *= d; ap *= ad;
      sp[p] += dp; sa[p] += fabsl(dp);
    }
  }
  for (int p = 1; p <= 4; ++p)
    if (fabsl(got[1 + p] - sp[p]) > se[p] + ((long double)cnt + 8) * 2.220446049250313e-16L * sa[p]) bad += 1;
  if (nbins > 0) {
    if (h[nbins + 2] != 0) bad += 1;
    std::vector<long long> up(nb3, 0), dn(nb3, 0);   // histograms of q_ref + dq and q_ref - dq
    const double inv = P.inv;
    for (size_t i = 0; i < cnt; ++i) {
      up[hist_slot((double)(qref[i] + dq[i]), lo, inv, nbins)] += 1;
      dn[hist_slot((double)(qref[i] - dq[i]), lo, inv, nbins)] += 1;
    }
    long long cu = 0, cd = 0, cg = 0;
    for (int j = 0; j <= nbins + 1; ++j) {
      cu += up[j]; cd += dn[j]; cg += h[j];
      if (cg < cu || cg > cd) bad += 1;
    }
    if (h[0] < 1 || h[nbins + 1] < 1) bad += 1;      // (the range was chosen inside the extremes: both tails are met)
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nlq(int nfields, int valid, int valid_in, int nrows, int ngroups, int nbins, bool negative, bool center, int bad_kind = 0) {
  NlqCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups; c.nbins = nbins;
  c.negative = negative; c.center = center;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nlq f%d r%d n%d g%d v%d/%d b%d%s%s%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, nbins, negative ? " neg" : "",
           center ? " centre" : "", TWLDS ? " twlds" : "", SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlq<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nlq f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlq<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
}
// the rule of the module against the documented one on hand-picked values: products that are inexact, so that a contraction of
// (w r) r + q into a fused multiply-add WOULD show (an FMA keeps the low bits that the separate product rounds away)
static void test_nlq_rule() {
  const double r[3] = {1.1, 2.3, 0.7}, w[3] = {0.9, -1.7, 3.3};
  double q = 0.0, bad = 0;
  for (int f = 0; f < 3; ++f) q = quad_term(q, w[f], r[f]);
  if (q != nlq_rule(r, w, 3)) bad += 1;
  if (q != -0x1.925e353f7ced8p+2) bad += 1;          // (the contracted sum ends in ..ced7)
  // the same steps with every intermediate forced through memory: no contraction is possible here whatever the flags
  volatile double v = 0.0;
  for (int f = 0; f < 3; ++f) {
    volatile double a = w[f] * r[f];
    volatile double b = a * r[f];
    v = v + b;
  }
  if (q != v) bad += 1;
  // ... and the contracted result differs on these values, so the comparison above can tell
  double fq = 0.0;
  for (int f = 0; f < 3; ++f) fq = __builtin_fma(w[f] * r[f], r[f], fq);
  if (fq == q) bad += 1;
  report("nlq rule", 3, "double", bad, 0.5);
  printf("nlq-rule q = %a\n", q);
}
// the case matrix of test_nlh_all (test_nlh.h): bin counts of 0, 1, 64 and the maximum, a negative weight, a centre
template <class S> static void test_nlq_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlq<S, double, 2, true, false, true>(6, lim, 0, 7, 1, 64, true, false, 1);
    test_nlq<S, float, 3, false, false, true>(1, full, 0, 1, 4, 0, false, true, 2);
  }
  test_nlq<S, double, 2, true, false, false>(3, full, 0, 7, 2, NLH_MAXBINS, false, true, 2);
  test_nlq<S, double, 1, false, true, false>(2, lim, 0, 1, 1, 64, true, false, 1);
  test_nlq<S, float, 2, true, true, false>(6, full, 0, 5, 1, 64, false, false, 1);
  test_nlq<S, float, 3, false, false, false>(3, lim, 0, 2 * 6 + 3, 1, 1, true, true, 2);         // two passes of the one workgroup and a ragged rest
  test_nlq<S, float, 2, true, false, false>(2, full, 0, 1, 1, 1, false, false, 0);
  test_nlq<S, double, 1, false, true, false>(1, full, 0, 3 * 4 + 3, 2, 0, false, false, 0);      // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nlq<S, double, 2, true, false, false>(2, full, lim, 7, 1, 64, false, true, 0);
    test_nlq<S, float, 1, false, true, false>(1, full, (2 * full) / 3, 3, 1, NLH_MAXBINS, true, false, 0);
  }
}
