// test_nlp.h -- emulator tests of the fused z stage that ends in plane-averaged PROFILES (nlz_prof.h NlzProf::body, Op::Profiles): per
// pair (a_p, b_p) of real fields and per position m of the row the five sums over all rows
//     [ sum d_a, sum d_b, sum d_a^2, sum d_b^2, sum d_a d_b ],   d = value - centre,
// against long-double transforms of the rows.  The bound is the moments' (test_nlz.h run_nls) applied per position: with R rows,
// |.| the 2-norm of the whole reference field and the sums on the right taken over the R values of the position,
//     sum d_a      tol sqrt(R) |a|                                        + (R + 8) 2^-52 sum |d_a|
//     sum d_a^2    2 tol sqrt(sum d_a^2) |a|                              + (R + 8) 2^-52 sum d_a^2
//     sum d_a d_b  tol (sqrt(sum d_b^2) |a| + sqrt(sum d_a^2) |b|)        + (R + 8) 2^-52 sum |d_a d_b|
// The launch has `ngroups` workgroups whatever the row count; the partial profiles are added up on the host in the order of the
// fold.  Every slot of `part` is written (poison), the inputs are preserved.
#pragma once
#include "nlz_prof.h"
#include "test_nlz.h"

struct NlpCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 2, ngroups = 1;
  int bad_field = -1;
  bool inf = false;
};
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nlp(const NlpCase& c, double tol) {      // the worst error in units of its bound, times tol; 1e30 for a broken contract
  typedef NlzProf<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields;
  const int pin = valid + 2;
  const int npairs = nf / 2;                         // field p is a_p, field npairs + p rides with it as b_p
  NlzFixture<S, T> fx(nf, 9191 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  fx.snapshot();
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  const size_t nvals = (size_t)npairs * NLP_STATS * M, nslots = (size_t)grid * ROWS;
  double center[6] = {0, 0, 0, 0, 0, 0};             // by slot: near the mean, off it, and zero
  for (int p = 0; p < npairs; ++p) { center[2 * p] = 0.5 * (p + 1) - 0.125; center[2 * p + 1] = p == 1 ? 0.0 : 0.5 * (npairs + p + 1) + 0.25; }
  const double poison = -7.0;
  auto launch = [&](std::vector<double>& part) {
    NlpParams<T> P;
    fx.params(P, valid, vin, M);
    for (int p = 0; p < 3; ++p) { P.a[p] = p < npairs ? in[p].data() : nullptr; P.b[p] = p < npairs ? in[npairs + p].data() : nullptr; }
    for (int i = 0; i < 6; ++i) P.center[i] = center[i];
    P.scale = (T)1;
    P.norm = 1.0 / (double)M; P.npairs = npairs; P.ngroups = grid;
    part.assign(nslots * nvals, poison);
    P.part = part.data();
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    double bad = 0;
    for (double v : part)
      if (v == poison) bad = 1e30;                   // a slot nobody wrote
    return bad;
  };
  std::vector<double> part, clean;
  double bad = 0;
  if (c.bad_field >= 0) {                            // the run with the bin taken out (what the transform sees) first: everybody else must EQUAL it
    in[c.bad_field][(size_t)(nrows / 2) * pin + 1] = mk<T>((T)0, (T)0);
    bad = std::max(bad, launch(clean));
    in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
    fx.snapshot();
  }
  bad = std::max(bad, launch(part));
  if (fx.inputs_changed()) bad = 1e30;               // the inputs are preserved
  // the fold: the partial profiles in order
  std::vector<double> got(nvals, 0.0);
  for (size_t g = 0; g < nslots; ++g)
    for (size_t v = 0; v < nvals; ++v) got[v] += part[g * nvals + v];
  auto stat = [&](const std::vector<double>& a, int p, int s) { return a.data() + ((size_t)p * NLP_STATS + s) * M; };
  if (c.bad_field >= 0) {
    const int bp = c.bad_field % npairs, second = c.bad_field >= npairs ? 1 : 0;
    for (size_t g = 0; g < nslots; ++g)
      for (int p = 0; p < npairs; ++p)
        for (int s = 0; s < NLP_STATS; ++s) {
          const bool touched = p == bp && (s == second || s == 2 + second || s == 4);
          const size_t at = g * nvals + ((size_t)p * NLP_STATS + s) * M;
          if (!touched && memcmp(part.data() + at, clean.data() + at, M * sizeof(double)) != 0) bad = 1e30;      // the same bytes
        }
    for (int s : {second, 2 + second, 4}) {          // the field's own sums and the cross sum: not finite
      int nans = 0;
      for (int m = 0; m < M; ++m) nans += stat(got, bp, s)[m] != stat(got, bp, s)[m];
      if (nans < 1) bad = 1e30;
    }
    for (int s : {1 - second, 3 - second})           // the partner stays finite
      for (int m = 0; m < M; ++m)
        if (!std::isfinite(stat(got, bp, s)[m])) bad = 1e30;
    return bad;
  }
  const long double eps = 2.220446049250313e-16L;
  for (int p = 0; p < npairs; ++p) {
    std::vector<lreal> ra(nrows), rb(nrows);
    long double na = 0, nb = 0;
    for (int r = 0; r < nrows; ++r) {
      ra[r] = nl_real_row(in[p].data() + (size_t)r * pin, vin, M);
      rb[r] = nl_real_row(in[npairs + p].data() + (size_t)r * pin, vin, M);
      for (long double x : ra[r]) na += x * x;
      for (long double x : rb[r]) nb += x * x;
    }
    na = sqrtl(na); nb = sqrtl(nb);
    const long double R = nrows, ca = center[2 * p], cb = center[2 * p + 1];
    for (int m = 0; m < M; ++m) {
      long double s[5] = {0, 0, 0, 0, 0}, a1 = 0, b1 = 0, ab1 = 0;
      for (int r = 0; r < nrows; ++r) {
        const long double da = ra[r][m] - ca, db = rb[r][m] - cb;
        s[0] += da; s[1] += db; s[2] += da * da; s[3] += db * db; s[4] += da * db;
        a1 += fabsl(da); b1 += fabsl(db); ab1 += fabsl(da * db);
      }
      const long double bound[5] = {tol * sqrtl(R) * na + (R + 8) * eps * a1, tol * sqrtl(R) * nb + (R + 8) * eps * b1,
                                    2 * tol * sqrtl(s[2]) * na + (R + 8) * eps * s[2], 2 * tol * sqrtl(s[3]) * nb + (R + 8) * eps * s[3],
                                    tol * (sqrtl(s[3]) * na + sqrtl(s[2]) * nb) + (R + 8) * eps * ab1};
      for (int k = 0; k < 5; ++k) {
        const double g = stat(got, p, k)[m];
        if (g != g) { bad = 1e30; continue; }
        bad = std::max(bad, (double)(fabsl(g - s[k]) / bound[k] * tol));
      }
    }
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nlp(int nfields, int valid, int valid_in, int nrows, int ngroups, int bad_kind = 0) {
  NlpCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups;
  const double tol = sizeof(T) == 8 ? 4e-14 : 2e-5;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nlp f%d r%d n%d g%d v%d/%d%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, TWLDS ? " twlds" : "",
           SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlp<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nlp f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlp<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
}
// the case matrix of test_nlj_all (test_nlj.h): 2 and 6 fields
template <class S> static void test_nlp_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlp<S, double, 2, true, false, true>(6, lim, 0, 7, 1, 1);
    test_nlp<S, float, 3, false, false, true>(2, full, 0, 1, 4, 2);
  }
  test_nlp<S, double, 2, true, false, false>(6, full, 0, 7, 2, 2);
  test_nlp<S, double, 1, false, true, false>(2, lim, 0, 1, 1, 1);
  test_nlp<S, float, 2, true, true, false>(6, full, 0, 5, 1, 1);
  test_nlp<S, float, 3, false, false, false>(6, lim, 0, 2 * 6 + 3, 1, 2);          // two passes of the one workgroup and a ragged rest
  test_nlp<S, float, 2, true, false, false>(2, full, 0, 1, 1, 0);
  test_nlp<S, double, 1, false, true, false>(2, full, 0, 3 * 4 + 3, 2, 0);         // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nlp<S, double, 2, true, false, false>(2, full, lim, 7, 1, 0);
    test_nlp<S, float, 1, false, true, false>(2, full, (2 * full) / 3, 3, 1, 0);
  }
}
