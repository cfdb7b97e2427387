// test_incr.h -- emulator tests of the fused z stage that ends in structure functions (nlz_incr.h NlzIncr::body, Op::Increments): per
// field and separation s the sums S2, S3, S4 of d = r(z + s) - r(z) over periodic rows, against long-double transforms of the
// rows.  The bound is the moments' (test_nlz.h run_nls) with the factor 2 that a difference of two values brings:
//     |S_p - ref| <= 2 tol p sqrt(sum d^(2 (p - 1)) sum x^2) + (cnt + 8) 2^-52 sum |d|^p
// The launch has `ngroups` workgroups whatever the row count; the waves' slots are added up on the host in the order of the fold.
#pragma once
#include "nlz_incr.h"
#include "test_nlz.h"

struct NliCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 1, ngroups = 1;
  int bad_field = -1;
  bool inf = false;
};
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nli(const NliCase& c, double tol) {      // the worst error in units of its bound, times tol; 1e30 for a broken contract
  typedef NlzIncr<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields;
  const int pin = valid + 2;
  const bool two = nf % 2 == 0;                      // a and b: field f of a rides with field f of b
  const int ncomp = two ? nf / 2 : nf;
  NlzFixture<S, T> fx(nf, 777 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  if (c.bad_field >= 0) in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
  fx.snapshot();
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  NliParams<T> P;
  int slot_of[6];
  fx.params(P, valid, vin, M);
  for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; }      // the fields go where their slots are
  for (int f = 0; f < nf; ++f) {
    const int slot = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
    (slot % 2 ? P.b : P.a)[slot / 2] = in[f].data();
    slot_of[f] = slot;
  }
  // 1, a multiple of the threads' stride, an odd value near the middle, n / 2, n - 1, and a duplicate
  auto clip = [&](int s) { return s < 1 ? 1 : s > M - 1 ? M - 1 : s; };
  const int seps[6] = {1, clip(S::TPT), clip((M / 2 - 1) | 1), clip(M / 2), M - 1, 1};
  const int nsep = 6;
  static_assert(NLI_MAXSEP >= 6, "the emulator's list of separations");
  for (int i = 0; i < NLI_MAXSEP; ++i) P.sep[i] = i < nsep ? seps[i] : 1;
  P.nsep = nsep;
  P.scale = (T)1;
  P.norm = 1.0 / (double)M; P.npairs = (nf + 1) / 2; P.ngroups = grid;
  std::vector<double> part((size_t)grid * K::WAVES * NLI_SLOTS, -7.0);
  P.part = part.data();
  emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  double bad = fx.inputs_changed() ? 1e30 : 0;       // the inputs are preserved
  for (double v : part)
    if (v == -7.0) bad = 1e30;                       // a slot nobody wrote
  const long double eps = 2.220446049250313e-16L;
  for (int f = 0; f < nf; ++f) {
    std::vector<lreal> rows(nrows);
    long double sx2 = 0;
    if (f != c.bad_field)
      for (int r = 0; r < nrows; ++r) {
        rows[r] = nl_real_row(in[f].data() + (size_t)r * pin, vin, M);
        for (long double x : rows[r]) sx2 += x * x;
      }
    for (int i = 0; i < nsep; ++i) {
      double got[NLI_STATS] = {0, 0, 0};
      for (size_t w = 0; w < part.size() / NLI_SLOTS; ++w) {
        const double* q = part.data() + w * NLI_SLOTS + (slot_of[f] * NLI_MAXSEP + i) * NLI_STATS;
        for (int k = 0; k < NLI_STATS; ++k) got[k] += q[k];
      }
      if (f == c.bad_field) {                        // all sums of the field are NaN
        for (int k = 0; k < NLI_STATS; ++k) if (got[k] == got[k]) bad = 1e30;
        continue;
      }
      long double sp[5] = {0, 0, 0, 0, 0}, sa[5] = {0, 0, 0, 0, 0}, s2p[5] = {0, 0, 0, 0, 0};
      for (int r = 0; r < nrows; ++r)
        for (int z = 0; z < M; ++z) {
          const long double d = rows[r][(z + seps[i]) % M] - rows[r][z];
          long double dp = 1;
          for (int p = 1; p <= 4; ++p) { s2p[p] += dp * dp; dp *= d; sp[p] += dp; sa[p] += fabsl(dp); }      // s2p[p] = sum d^(2 (p - 1))
        }
      const long double cnt = (long double)nrows * M;
      for (int p = 2; p <= 4; ++p) {
        if (got[p - 2] != got[p - 2]) { bad = 1e30; continue; }      // a clean field next to a bad one stays finite
        const long double bound = 2 * tol * p * sqrtl(s2p[p] * sx2) + (cnt + 8) * eps * sa[p];
        bad = std::max(bad, (double)(fabsl(got[p - 2] - sp[p]) / bound * tol));
      }
    }
    // the duplicate separation gives the same bits as its first occurrence
    for (size_t w = 0; w < part.size() / NLI_SLOTS; ++w) {
      const double* q = part.data() + w * NLI_SLOTS + slot_of[f] * NLI_FIELD;
      if (f != c.bad_field && memcmp(q, q + 5 * NLI_STATS, NLI_STATS * sizeof(double)) != 0) bad = 1e30;
    }
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nli(int nfields, int valid, int valid_in, int nrows, int ngroups, int bad_kind = 0) {
  NliCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups;
  const double tol = sizeof(T) == 8 ? 4e-14 : 2e-5;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nli f%d r%d n%d g%d v%d/%d%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, TWLDS ? " twlds" : "",
           SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nli<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nli f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nli<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
}
// the case matrix of test_nls_all (test_nlz.h)
template <class S> static void test_nli_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nli<S, double, 2, true, false, true>(6, lim, 0, 7, 1, 1);
    test_nli<S, float, 3, false, false, true>(1, full, 0, 1, 4, 2);
  }
  test_nli<S, double, 2, true, false, false>(3, full, 0, 7, 2, 2);
  test_nli<S, double, 1, false, true, false>(2, lim, 0, 1, 1, 1);
  test_nli<S, float, 2, true, true, false>(6, full, 0, 5, 1, 1);
  test_nli<S, float, 3, false, false, false>(3, lim, 0, 2 * 6 + 3, 1, 2);          // two passes of the one workgroup and a ragged rest
  test_nli<S, float, 2, true, false, false>(2, full, 0, 1, 1, 0);
  test_nli<S, double, 1, false, true, false>(1, full, 0, 3 * 4 + 3, 2, 0);         // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nli<S, double, 2, true, false, false>(2, full, lim, 7, 1, 0);
    test_nli<S, float, 1, false, true, false>(1, full, (2 * full) / 3, 3, 1, 0);
  }
}
