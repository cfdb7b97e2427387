// test_nlk.h -- emulator tests of the fused z stage that ends in INCREMENT HISTOGRAMS (nlz_incr_hist.h NlzIncrHist::body,
// Op::IncrementHistogram): per field and separation s the counts of d = r(z + s) - r(z) over periodic rows in nbins equal bins of a
// range of its own, against long-double transforms of the rows THROUGH THE SAME RULE (hist_slot).  Counts cannot be compared with a
// tolerance, so the test brackets them as test_nlh.h does: the slot rule is monotone in d, and with |x_kernel - x_ref| <= delta on
// both values of an increment, |d_kernel - d_ref| <= 2 delta, every cumulative count obeys
//     C_j(d_ref + 2 delta) <= C_j(kernel) <= C_j(d_ref - 2 delta),   j = 0 .. nbins + 1.
// delta is the per-row worst-case bound of test_nlh.h over both fields of the pair.  Every (field, separation) sums to the points,
// a duplicate separation with the same range gives the same counts, a field with a NaN or Inf bin meets its non-finite slot and
// leaves every other field -- the partner on its transform among them -- with the counts of the run without it.  In the emulator
// the LDS add is a plain add.
#pragma once
#include "nlz_incr_hist.h"
#include "test_nlh.h"

struct NlkCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 1, ngroups = 1, nbins = 64;
  int bad_field = -1;
  bool inf = false;
};

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nlk(const NlkCase& c) {      // broken brackets and contracts, counted; 0 is a pass
  typedef NlzIncrHist<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields, nbins = c.nbins;
  const int pin = valid + 2, nb3 = nbins + 3;
  const bool two = nf % 2 == 0;                      // a and b: field f of a rides with field f of b
  const int ncomp = two ? nf / 2 : nf, npairs = (nf + 1) / 2;
  NlzFixture<S, T> fx(nf, 4242 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  fx.snapshot();
  int slot_of[6];
  for (int f = 0; f < nf; ++f) slot_of[f] = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
  // 1, a multiple of the threads' stride, an odd value near the middle, n / 2, n - 1, a duplicate of the first, two more
  auto clip = [&](int s) { return s < 1 ? 1 : s > M - 1 ? M - 1 : s; };
  const int nsep = NLI_MAXSEP;
  static_assert(NLI_MAXSEP == 8, "the emulator's list of separations");
  const int seps[8] = {1, clip(S::TPT), clip((M / 2 - 1) | 1), clip(M / 2), M - 1, 1, clip(2), clip(3 * S::TPT + 1)};
  const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-7;
  std::vector<std::vector<lreal>> rows(nf);
  std::vector<std::vector<double>> delta(npairs, std::vector<double>(nrows, 0.0));
  double lo[6][NLI_MAXSEP], hi[6][NLI_MAXSEP];       // by slot
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < NLI_MAXSEP; ++i) { lo[s][i] = 0; hi[s][i] = 1; }
  for (int f = 0; f < nf; ++f) {
    for (int r = 0; r < nrows; ++r) {
      const cx<T>* z = in[f].data() + (size_t)r * pin;
      rows[f].push_back(nl_real_row(z, vin, M));
      long double s = 0;
      for (int q = 0; q < vin; ++q) {
        const bool self = q == 0 || (M % 2 == 0 && q == M / 2);
        s += (self ? 1 : 2) * (fabsl((long double)z[q].x) + (self ? 0 : fabsl((long double)z[q].y)));
      }
      delta[slot_of[f] / 2][r] += (double)(8 * eps * log2((double)M) * s / M);
    }
    for (int i = 0; i < nsep; ++i) {                 // a range that leaves increments on both sides; the duplicate takes its twin's
      double mn = INFINITY, mx = -INFINITY;
      for (int r = 0; r < nrows; ++r)
        for (int z = 0; z < M; ++z) {
          const double d = (double)(rows[f][r][(z + seps[i]) % M] - rows[f][r][z]);
          mn = std::min(mn, d); mx = std::max(mx, d);
        }
      if (!(mx > mn)) { mn -= 1; mx += 1; }
      lo[slot_of[f]][i] = mn + 0.10 * (mx - mn);
      hi[slot_of[f]][i] = mx - 0.15 * (mx - mn);
    }
  }
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  const size_t row = (size_t)2 * npairs * nsep * nb3;
  auto launch = [&](std::vector<long long>& tot) {
    NlkParams<T> P;
    fx.params(P, valid, vin, M);
    for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; }      // the fields go where their slots are
    for (int f = 0; f < nf; ++f) (slot_of[f] % 2 ? P.b : P.a)[slot_of[f] / 2] = in[f].data();
    for (int s = 0; s < 6; ++s)
      for (int i = 0; i < NLI_MAXSEP; ++i) { P.lo[s][i] = lo[s][i]; P.inv[s][i] = (double)nbins / (hi[s][i] - lo[s][i]); }
    for (int i = 0; i < NLI_MAXSEP; ++i) P.sep[i] = seps[i];
    P.scale = (T)1;
    P.norm = 1.0 / (double)M; P.nsep = nsep; P.nbins = nbins; P.npairs = npairs; P.ngroups = grid;
    std::vector<unsigned> part((size_t)grid * row, 0xFFFFFFFFu);
    P.part = part.data();
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    double bad = 0;
    tot.assign(row, 0);
    for (size_t i = 0; i < part.size(); ++i) {
      if (part[i] == 0xFFFFFFFFu) bad += 1;          // a slot nobody wrote
      tot[i % row] += part[i];                       // the fold: the workgroups' rows in order
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
  for (int f = 0; f < nf; ++f)
    for (int i = 0; i < nsep; ++i) {
      const int slot = slot_of[f];
      const long long* h = tot.data() + ((size_t)slot * nsep + i) * nb3;
      long long sum = 0;
      for (int j = 0; j < nb3; ++j) sum += h[j];
      if (sum != count) bad += 1;                    // every increment is in exactly one slot
      if (f == c.bad_field) {                        // the thread that met the bin counts its E increments as non-finite
        if (h[nbins + 2] < 1) bad += 1;
        continue;
      }
      if (h[nbins + 2] != 0) bad += 1;
      if (i == 5 && memcmp(h, tot.data() + (size_t)slot * nsep * nb3, nb3 * sizeof(long long)) != 0) bad += 1;      // the duplicate
      if (c.bad_field >= 0) {                        // a clean field next to a bad one: the counts of the clean run, exactly
        if (memcmp(h, clean.data() + ((size_t)slot * nsep + i) * nb3, nb3 * sizeof(long long)) != 0) bad += 1;
        continue;
      }
      std::vector<long long> up(nb3, 0), dn(nb3, 0);
      const double l = lo[slot][i], inv = (double)nbins / (hi[slot][i] - l);
      for (int r = 0; r < nrows; ++r) {
        const double d2 = 2 * delta[slot / 2][r];
        for (int z = 0; z < M; ++z) {
          const double d = (double)(rows[f][r][(z + seps[i]) % M] - rows[f][r][z]);
          up[nlh_slot(d + d2, l, inv, nbins)] += 1;
          dn[nlh_slot(d - d2, l, inv, nbins)] += 1;
        }
      }
      long long cu = 0, cd = 0, cg = 0;
      for (int j = 0; j <= nbins + 1; ++j) {
        cu += up[j]; cd += dn[j]; cg += h[j];
        if (cg < cu || cg > cd) bad += 1;
      }
      if (h[0] < 1 || h[nbins + 1] < 1) bad += 1;    // (the range was chosen inside the extremes: both tails are met)
    }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nlk(int nfields, int valid, int valid_in, int nrows, int ngroups, int nbins, int bad_kind = 0) {
  NlkCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups; c.nbins = nbins;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nlk f%d r%d n%d g%d v%d/%d b%d%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, nbins, TWLDS ? " twlds" : "",
           SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlk<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nlk f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlk<S, T, ROWS, TWLDS, SPLIT, WAVE>(c), 0.5);
}
// the case matrix of test_nli_all, with the bin counts 1, 37, 64 and NLK_MAXBINS
template <class S> static void test_nlk_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  const int X = NLK_MAXBINS;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlk<S, double, 2, true, false, true>(6, lim, 0, 7, 1, X, 1);
    test_nlk<S, float, 3, false, false, true>(1, full, 0, 1, 4, 37, 2);
  }
  test_nlk<S, double, 2, true, false, false>(3, full, 0, 7, 2, X, 2);
  test_nlk<S, double, 1, false, true, false>(2, lim, 0, 1, 1, 1, 1);
  test_nlk<S, float, 2, true, true, false>(6, full, 0, 5, 1, 64, 1);
  test_nlk<S, float, 3, false, false, false>(3, lim, 0, 2 * 6 + 3, 1, 37, 2);         // two passes of the one workgroup and a ragged rest
  test_nlk<S, float, 2, true, false, false>(2, full, 0, 1, 1, 1, 0);
  test_nlk<S, double, 1, false, true, false>(1, full, 0, 3 * 4 + 3, 2, X, 0);         // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nlk<S, double, 2, true, false, false>(2, full, lim, 7, 1, 64, 0);
    test_nlk<S, float, 1, false, true, false>(1, full, (2 * full) / 3, 3, 1, 37, 0);
  }
}
