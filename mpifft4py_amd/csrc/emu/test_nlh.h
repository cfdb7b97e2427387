// test_nlh.h -- emulator tests of the fused z stage that ends in a histogram (nlz_hist.h NlzHist::body, Op::Histogram): the counts of up
// to six real fields in equal bins, against long-double transforms of the rows.  Counts cannot be compared with a tolerance, so
// the test brackets them: the slot rule is monotone in x, hence with |x_kernel - x_ref| <= delta every CUMULATIVE count obeys
//     C_j(x_ref + delta) <= C_j(kernel) <= C_j(x_ref - delta),   j = 0 .. nbins + 1,   C_j = points in slots 0 .. j,
// the total is exactly nrows * M and the non-finite slot is 0.  delta is a worst-case bound per row, not a measurement:
// 8 eps log2(M) sum_k h_k (|A_k| + |B_k|) / M over BOTH fields of the pair (they share the transform), h the Hermitian weights.
// In the emulator the LDS add is a plain add (the threads are fibres of one host thread).
#pragma once
#include "nlz_hist.h"
#include "test_nlz.h"

struct NlhCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 1, ngroups = 1, nbins = 64;
  int bad_field = -1;
  bool inf = false;
};
// the host's copy of the rule, in long double only where the reference is: the slots of x_ref -+ delta are formed in double, as
// the kernel forms them
static int nlh_slot(double x, double lo, double inv, int nbins) { return hist_slot(x, lo, inv, nbins); }

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE, bool MERGE = false>
static double run_nlh(const NlhCase& c) {      // broken brackets and contracts, counted; 0 is a pass
  typedef NlzHist<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>, MERGE> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields, nbins = c.nbins;
  const int pin = valid + 2, nb3 = nbins + 3;
  const bool two = nf % 2 == 0;                      // a and b: field f of a rides with field f of b
  const int ncomp = two ? nf / 2 : nf, npairs = (nf + 1) / 2;
  NlzFixture<S, T> fx(nf, 5151 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  fx.snapshot();
  // the reference rows, their extremes, and the worst-case error of a row of each PAIR
  int slot_of[6];
  for (int f = 0; f < nf; ++f) slot_of[f] = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
  std::vector<std::vector<double>> ref(nf);
  std::vector<std::vector<double>> delta(npairs, std::vector<double>(nrows, 0.0));
  const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-7;
  double lo[6] = {0, 0, 0, 0, 0, 0}, hi[6] = {1, 1, 1, 1, 1, 1};      // by slot
  for (int f = 0; f < nf; ++f) {
    double mn = INFINITY, mx = -INFINITY;
    for (int r = 0; r < nrows; ++r) {
      const cx<T>* z = in[f].data() + (size_t)r * pin;
      for (long double x : nl_real_row(z, vin, M)) { ref[f].push_back((double)x); mn = std::min(mn, (double)x); mx = std::max(mx, (double)x); }
      long double s = 0;
      for (int q = 0; q < vin; ++q) {
        const bool self = q == 0 || (M % 2 == 0 && q == M / 2);
        s += (self ? 1 : 2) * (fabsl((long double)z[q].x) + (self ? 0 : fabsl((long double)z[q].y)));
      }
      delta[slot_of[f] / 2][r] += (double)(8 * eps * log2((double)M) * s / M);
    }
    // a range that leaves points on both sides: the tails are part of the contract
    lo[slot_of[f]] = mn + 0.10 * (mx - mn);
    hi[slot_of[f]] = mx - 0.15 * (mx - mn);
  }
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  auto launch = [&](std::vector<long long>& tot) {
    NlhParams<T> P;
    fx.params(P, valid, vin, M);
    for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; }      // the fields go where their slots are
    for (int f = 0; f < nf; ++f) (slot_of[f] % 2 ? P.b : P.a)[slot_of[f] / 2] = in[f].data();
    for (int i = 0; i < 6; ++i) { P.lo[i] = lo[i]; P.inv[i] = (double)nbins / (hi[i] - lo[i]); }
    P.scale = (T)1;
    P.norm = 1.0 / (double)M; P.nbins = nbins; P.npairs = npairs; P.ngroups = grid;
    std::vector<unsigned> part((size_t)grid * npairs * 2 * nb3, 0xFFFFFFFFu);
    P.part = part.data();
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    double bad = 0;
    tot.assign((size_t)2 * npairs * nb3, 0);
    for (size_t i = 0; i < part.size(); ++i) {
      if (part[i] == 0xFFFFFFFFu) bad += 1;          // a slot nobody wrote
      tot[i % ((size_t)2 * npairs * nb3)] += part[i];      // the fold: the workgroups' rows in order
    }
    return bad;
  };
  std::vector<long long> tot, clean;
  double bad = 0;
  if (c.bad_field >= 0) {                            // the run without the bad bin first: the other fields must EQUAL it
    bad += launch(clean);
    in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
    fx.snapshot();
  }
  bad += launch(tot);
  if (fx.inputs_changed()) bad += 1;                 // the inputs are preserved
  const long long count = (long long)nrows * M;
  for (int f = 0; f < nf; ++f) {
    const long long* h = tot.data() + (size_t)slot_of[f] * nb3;
    long long sum = 0;
    for (int s = 0; s < nb3; ++s) sum += h[s];
    if (sum != count) bad += 1;                      // every point is in exactly one slot
    if (f == c.bad_field) {
      if (h[nbins + 2] < 1) bad += 1;
      continue;
    }
    if (h[nbins + 2] != 0) bad += 1;
    if (c.bad_field >= 0) {                          // a clean field next to a bad one: the counts of the clean run, exactly
      for (int s = 0; s < nb3; ++s)
        if (h[s] != clean[(size_t)slot_of[f] * nb3 + s]) bad += 1;
      continue;
    }
    std::vector<long long> up(nb3, 0), dn(nb3, 0);   // histograms of x_ref + delta and x_ref - delta
    const double l = lo[slot_of[f]], inv = (double)nbins / (hi[slot_of[f]] - l);
    for (int r = 0; r < nrows; ++r)
      for (int p = 0; p < M; ++p) {
        const double x = ref[f][(size_t)r * M + p], d = delta[slot_of[f] / 2][r];
        up[nlh_slot(x + d, l, inv, nbins)] += 1;
        dn[nlh_slot(x - d, l, inv, nbins)] += 1;
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
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE, bool MERGE = false>
static void test_nlh(int nfields, int valid, int valid_in, int nrows, int ngroups, int nbins, int bad_kind = 0) {
  NlhCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups; c.nbins = nbins;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nlh f%d r%d n%d g%d v%d/%d b%d%s%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, nbins,
           TWLDS ? " twlds" : "", SPLIT ? " split" : "", WAVE ? " wave" : "", MERGE ? " merge" : "");
  report(name, S::N, pname<T>(), run_nlh<S, T, ROWS, TWLDS, SPLIT, WAVE, MERGE>(c), 0.5);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nlh f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlh<S, T, ROWS, TWLDS, SPLIT, WAVE, MERGE>(c), 0.5);
}
// the case matrix of test_nls_all (test_nlz.h), with bin counts of 1, an odd one, 64 and the maximum
template <class S> static void test_nlh_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlh<S, double, 2, true, false, true>(6, lim, 0, 7, 1, 64, 1);
    test_nlh<S, float, 3, false, false, true>(1, full, 0, 1, 4, 7, 2);
  }
  test_nlh<S, double, 2, true, false, false>(3, full, 0, 7, 2, NLH_MAXBINS, 2);
  test_nlh<S, double, 1, false, true, false>(2, lim, 0, 1, 1, 64, 1);
  test_nlh<S, float, 2, true, true, false>(6, full, 0, 5, 1, 64, 1);
  test_nlh<S, float, 3, false, false, false>(3, lim, 0, 2 * 6 + 3, 1, 33, 2);           // two passes of the one workgroup and a ragged rest
  test_nlh<S, float, 2, true, false, false>(2, full, 0, 1, 1, 1, 0);
  test_nlh<S, double, 1, false, true, false>(1, full, 0, 3 * 4 + 3, 2, 64, 0);          // three passes of two workgroups and a ragged rest
  // the build that merges runs of equal slot first (not shipped; here the merge is a plain add, what is checked is that the
  // lanes of rows past the end count nothing): an odd row count, so the last pair of rows is half empty
  test_nlh<S, float, 2, true, false, false, true>(6, full, 0, 5, 2, 64, 1);
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nlh<S, double, 2, true, false, false>(2, full, lim, 7, 1, 64, 0);
    test_nlh<S, float, 1, false, true, false>(1, full, (2 * full) / 3, 3, 1, 64, 0);
  }
}
