// test_nlj.h -- emulator tests of the fused z stage that ends in a JOINT histogram (nlz_joint.h NlzJoint::body, Op::JointHistogram): the
// counts of the points (a_p, b_p) of one or three pairs of real fields in a grid of nba x nbb equal bins, against long-double
// transforms of the rows.  Counts cannot be compared with a tolerance, so the test brackets them in two dimensions: the cell rule
// is monotone in each argument, hence with |x_kernel - x_ref| <= delta on BOTH fields every cumulative count obeys
//     C_ij(x_ref + delta) <= C_ij(kernel) <= C_ij(x_ref - delta),   i = 0 .. nba + 1,  j = 0 .. nbb + 1,
// C_ij = points with sa <= i and sb <= j.  delta is the per-row worst-case bound of test_nlh.h over both fields of the pair.
// Both marginals EQUAL, count for count, what NlzHist of the same template parameters gives on the same inputs, ranges and bin
// counts: in the emulator the two bodies run the same arithmetic.  In the emulator the LDS add is a plain add.
#pragma once
#include "nlz_joint.h"
#include "test_nlh.h"

struct NljCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 2, ngroups = 1, nba = 64, nbb = 64;
  int bad_field = -1;
  bool inf = false;
};

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nlj(const NljCase& c) {      // broken brackets and contracts, counted; 0 is a pass
  typedef NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE> F;
  typedef NlzJoint<F> K;
  typedef NlzHist<F> KH;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields;
  const int nba = c.nba, nbb = c.nbb, na3 = nba + 3, nb3 = nbb + 3, cells = na3 * nb3;
  const int pin = valid + 2;
  const int ncomp = nf / 2, npairs = ncomp;          // field f < ncomp is a_f, field ncomp + p rides with it as b_p
  NlzFixture<S, T> fx(nf, 6161 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  fx.snapshot();
  int slot_of[6];
  for (int f = 0; f < nf; ++f) slot_of[f] = f < ncomp ? 2 * f : 2 * (f - ncomp) + 1;
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
    // a range that leaves points on both sides: the border cells are part of the contract
    lo[slot_of[f]] = mn + 0.10 * (mx - mn);
    hi[slot_of[f]] = mx - 0.15 * (mx - mn);
  }
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  auto nb_of = [&](int slot) { return slot % 2 ? nbb : nba; };
  auto launch = [&](std::vector<long long>& tot) {
    NljParams<T> P;
    fx.params(P, valid, vin, M);
    for (int p = 0; p < 3; ++p) { P.a[p] = p < npairs ? in[p].data() : nullptr; P.b[p] = p < npairs ? in[ncomp + p].data() : nullptr; }
    for (int i = 0; i < 6; ++i) { P.lo[i] = lo[i]; P.inv[i] = (double)nb_of(i) / (hi[i] - lo[i]); }
    P.scale = (T)1;
    P.norm = 1.0 / (double)M; P.nba = nba; P.nbb = nbb; P.npairs = npairs; P.ngroups = grid;
    std::vector<unsigned> part((size_t)grid * npairs * cells, 0xFFFFFFFFu);
    P.part = part.data();
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    double bad = 0;
    tot.assign((size_t)npairs * cells, 0);
    for (size_t i = 0; i < part.size(); ++i) {
      if (part[i] == 0xFFFFFFFFu) bad += 1;          // a cell nobody wrote
      tot[i % ((size_t)npairs * cells)] += part[i];  // the fold: the workgroups' rows in order
    }
    return bad;
  };
  // the histogram twin on the same inputs and ranges with `nbins` bins for every field: slot-ordered (2 npairs, nbins + 3)
  auto twin = [&](int nbins, std::vector<long long>& tot) {
    NlhParams<T> P;
    fx.params(P, valid, vin, M);
    for (int p = 0; p < 3; ++p) { P.a[p] = p < npairs ? in[p].data() : nullptr; P.b[p] = p < npairs ? in[ncomp + p].data() : nullptr; }
    for (int i = 0; i < 6; ++i) { P.lo[i] = lo[i]; P.inv[i] = (double)nbins / (hi[i] - lo[i]); }
    P.scale = (T)1;
    P.norm = 1.0 / (double)M; P.nbins = nbins; P.npairs = npairs; P.ngroups = grid;
    const size_t row = (size_t)2 * npairs * (nbins + 3);
    std::vector<unsigned> part((size_t)grid * row, 0u);
    P.part = part.data();
    emu_launch(grid, KH::THREADS, KH::LDS_BYTES, [&](int b, int t, char* lds) { KH::body(P, b, t, lds); });
    tot.assign(row, 0);
    for (size_t i = 0; i < part.size(); ++i) tot[i % row] += part[i];
  };
  // marginal of field `slot` from a pair's grid
  auto marginal = [&](const std::vector<long long>& tot, int slot) {
    const long long* g = tot.data() + (size_t)(slot / 2) * cells;
    std::vector<long long> m(slot % 2 ? nb3 : na3, 0);
    for (int i = 0; i < na3; ++i)
      for (int j = 0; j < nb3; ++j) m[slot % 2 ? j : i] += g[(size_t)i * nb3 + j];
    return m;
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
  // 3. the marginals against the histogram twin, count for count
  {
    std::vector<long long> ha, hb;
    twin(nba, ha);
    if (nbb == nba) hb = ha; else twin(nbb, hb);
    for (int f = 0; f < nf; ++f) {
      const int slot = slot_of[f];
      const std::vector<long long> m = marginal(tot, slot);
      const std::vector<long long>& h = slot % 2 ? hb : ha;
      const int n3 = nb_of(slot) + 3;
      for (int s = 0; s < n3; ++s)
        if (m[s] != h[(size_t)slot * n3 + s]) bad += 1;
    }
    if (fx.inputs_changed()) bad += 1;
  }
  const int bad_pair = c.bad_field >= 0 ? slot_of[c.bad_field] / 2 : -1;
  for (int p = 0; p < npairs; ++p) {
    const long long* g = tot.data() + (size_t)p * cells;
    long long sum = 0;
    for (int i = 0; i < cells; ++i) sum += g[i];
    if (sum != count) bad += 1;                      // 1. every point is in exactly one cell
    if (p == bad_pair) {                             // 4. the bad field's non-finite slot is met, the partner's marginal is the clean run's
      const int sbad = slot_of[c.bad_field], spart = sbad ^ 1;
      if (marginal(tot, sbad)[nb_of(sbad) + 2] < 1) bad += 1;
      if (marginal(tot, spart) != marginal(clean, spart)) bad += 1;
      if (marginal(tot, spart)[nb_of(spart) + 2] != 0) bad += 1;
      continue;
    }
    if (marginal(tot, 2 * p)[nba + 2] != 0 || marginal(tot, 2 * p + 1)[nbb + 2] != 0) bad += 1;
    if (c.bad_field >= 0) {                          // a clean pair next to a bad one: the cells of the clean run, exactly
      for (int i = 0; i < cells; ++i)
        if (g[i] != clean[(size_t)p * cells + i]) bad += 1;
      continue;
    }
    // 2. the two-dimensional brackets
    std::vector<long long> up(cells, 0), dn(cells, 0), gg(g, g + cells);
    const double la = lo[2 * p], ia = (double)nba / (hi[2 * p] - la), lb = lo[2 * p + 1], ib = (double)nbb / (hi[2 * p + 1] - lb);
    for (int r = 0; r < nrows; ++r)
      for (int q = 0; q < M; ++q) {
        const double xa = ref[p][(size_t)r * M + q], xb = ref[ncomp + p][(size_t)r * M + q], d = delta[p][r];
        up[(size_t)nlh_slot(xa + d, la, ia, nba) * nb3 + nlh_slot(xb + d, lb, ib, nbb)] += 1;
        dn[(size_t)nlh_slot(xa - d, la, ia, nba) * nb3 + nlh_slot(xb - d, lb, ib, nbb)] += 1;
      }
    auto cumulate = [&](std::vector<long long>& a) {
      for (int i = 0; i < na3; ++i)
        for (int j = 0; j < nb3; ++j)
          a[(size_t)i * nb3 + j] += (i ? a[(size_t)(i - 1) * nb3 + j] : 0) + (j ? a[(size_t)i * nb3 + j - 1] : 0) - (i && j ? a[(size_t)(i - 1) * nb3 + j - 1] : 0);
    };
    cumulate(up); cumulate(dn); cumulate(gg);
    for (int i = 0; i <= nba + 1; ++i)
      for (int j = 0; j <= nbb + 1; ++j) {
        const size_t k = (size_t)i * nb3 + j;
        if (gg[k] < up[k] || gg[k] > dn[k]) bad += 1;
      }
    // (the ranges were chosen inside the extremes: both tails of both fields are met)
    const std::vector<long long> ma = marginal(tot, 2 * p), mb = marginal(tot, 2 * p + 1);
    if (ma[0] < 1 || ma[nba + 1] < 1 || mb[0] < 1 || mb[nbb + 1] < 1) bad += 1;
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nlj(int nfields, int valid, int valid_in, int nrows, int ngroups, int nba, int nbb, int bad_kind = 0) {
  NljCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups; c.nba = nba; c.nbb = nbb;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nlj f%d r%d n%d g%d v%d/%d b%dx%d%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, nba, nbb,
           TWLDS ? " twlds" : "", SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlj<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nlj f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlj<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
}
// the case matrix of test_nlh_all, with 2 and 6 fields and the bin pairs (1, 1), (7, 33), (64, 64) and (64, 1)
template <class S> static void test_nlj_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  const int X = NLJ_MAXBINS;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlj<S, double, 2, true, false, true>(6, lim, 0, 7, 1, X, X, 1);
    test_nlj<S, float, 3, false, false, true>(2, full, 0, 1, 4, 7, 33, 2);
  }
  test_nlj<S, double, 2, true, false, false>(6, full, 0, 7, 2, X, X, 2);
  test_nlj<S, double, 1, false, true, false>(2, lim, 0, 1, 1, X, 1, 1);
  test_nlj<S, float, 2, true, true, false>(6, full, 0, 5, 1, X, X, 1);
  test_nlj<S, float, 3, false, false, false>(6, lim, 0, 2 * 6 + 3, 1, 7, 33, 2);          // two passes of the one workgroup and a ragged rest
  test_nlj<S, float, 2, true, false, false>(2, full, 0, 1, 1, 1, 1, 0);
  test_nlj<S, double, 1, false, true, false>(2, full, 0, 3 * 4 + 3, 2, X, X, 0);          // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nlj<S, double, 2, true, false, false>(2, full, lim, 7, 1, X, X, 0);
    test_nlj<S, float, 1, false, true, false>(2, full, (2 * full) / 3, 3, 1, 7, 33, 0);
  }
}
