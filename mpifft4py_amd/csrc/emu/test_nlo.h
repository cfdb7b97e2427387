// test_nlo.h -- emulator tests of the fused nonlinear z stage with the OUTER product (fft_nlz.h NlzFft::body_outer, NloParams):
// out9[3 i + j] = rfft(irfft(a_i) irfft(b_j)), nine rows out per six rows in, against long-double DFTs.  Fixture and reference
// are those of test_nlz.h.
#pragma once
#include "test_nlz.h"

// spectrum of the product of two real rows
static lvec nl_product_spectrum(const lreal& a, const lreal& b) {
  const int M = (int)a.size();
  lvec x(M);
  for (int p = 0; p < M; ++p) { x[p].x = a[p] * b[p]; x[p].y = 0; }
  return naive_dft(x, -1);
}

// inplace: results 0..2 over a_0..2 and 3..5 over b_0..2, row for row (what the routes do), 6..8 in arrays of their own; otherwise all
// nine in arrays of their own, and the six inputs must come back untouched.  poison: the buffers hold one more row than nrows (an odd
// count), full of NaNs -- the missing partner of the last row must contribute nothing and nothing is stored behind the last row.
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
static void test_nlo(int valid, bool inplace, int valid_in = 0, bool poison = false) {
  typedef NlzProd<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>, NlzProduct::Outer> K;
  const int vin = valid_in > 0 ? valid_in : valid;
  const int M = S::N;
  const int nrows = 2 * ROWS + 3;                 // an odd count: the last pair has one row
  const int pin = valid + 2, pout = inplace ? pin : valid + 1;
  const int extra = poison ? 1 : 0;
  NlzFixture<S, T> fx(6, 9009 + M + valid, nrows, pin, pout, 0, extra);
  const cx<T> nan = mk<T>(std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::quiet_NaN());
  std::vector<cx<T>> own[9];
  int over[9];
  cx<T>* res[9];
  for (int c = 0; c < 9; ++c) {
    over[c] = inplace && c < 6 ? c : -1;
    if (over[c] < 0) {
      own[c].assign((size_t)(nrows + extra) * pout, mk<T>((T)7, (T)7));
      std::fill(own[c].begin() + (size_t)nrows * pout, own[c].end(), nan);
      res[c] = own[c].data();
    } else {
      res[c] = fx.in[over[c]].data();
    }
  }
  NloParams<T> P;
  fx.params(P, valid, vin, M);
  for (int c = 0; c < 9; ++c) P.out9[c] = res[c];
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = fx.real_rows(r, vin, M);
    for (int c = 0; c < 9; ++c) {
      const cx<T>* g = res[c] + (size_t)r * pout;
      nl_accumulate(g, nl_product_spectrum(re[c / 3], re[3 + c % 3]), valid, err);
      fx.tail_kept(g, r, over[c], valid, err);
    }
  }
  for (int c = 0; c < 9; ++c)                      // ... nor behind the last row
    for (size_t i = (size_t)nrows * pout; i < (size_t)(nrows + extra) * pout; ++i)
      if (res[c][i].x == res[c][i].x || res[c][i].y == res[c][i].y) err.num += 1;
  err.num += fx.inputs_changed(over, 9);
  char name[80];
  snprintf(name, sizeof name, "nlo r%d v%d/%d%s%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "",
           inplace ? " inpl" : "", poison ? " poison" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), err.value(), sizeof(T) == 8 ? 4e-14 : 2e-5);
}
template <class S> static void test_nlo_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;     // every bin / the bins of the un-padded mesh under the 3/2-rule
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlo<S, double, 2, true, false, true>(lim, true, 0, true);
    test_nlo<S, double, 1, false, false, true>(full, true);
    test_nlo<S, float, 3, false, false, true>(full, false);
    test_nlo<S, float, 2, true, false, true>(lim, true, 0, true);
  }
  test_nlo<S, double, 2, true, false>(full, false);
  test_nlo<S, double, 1, false, true>(lim, true, 0, true);
  test_nlo<S, double, 2, true, true>(full, true);
  test_nlo<S, double, 3, false, false>(lim, false);
  test_nlo<S, float, 3, false, false>(lim, false);
  test_nlo<S, float, 2, true, true>(full, true, 0, true);
  test_nlo<S, float, 1, false, true>(lim, true);
  test_nlo<S, float, 2, true, false>(full, true);
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins in, every bin out
    test_nlo<S, double, 2, true, false>(full, true, lim);
    test_nlo<S, double, 1, false, true>(full, false, lim);
    test_nlo<S, float, 3, false, false>(full, false, (2 * full) / 3);
    test_nlo<S, float, 2, true, true>(full, true, (2 * full) / 3, true);
  }
}
