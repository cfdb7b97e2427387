// test_nlz.h -- emulator tests of the fused nonlinear z stage (fft_nlz.h): the cross product (nlz), the dot product (nld), both
// (nlc), the bodies with the real-space maxima (nlm), the bodies that end in a reduction (nls) and the 3/2-rule flavour (nlz3)
#pragma once
#include <algorithm>
#include "emu.h"
#include "fft_nlz.h"
#include "nlz_moments.h"
#include "plans.h"

// The long-double reference the tests share.
// The real row a stored half-spectrum row z stands for: its first vin bins, extended to the Hermitian spectrum of M points (the
// imaginary parts of the self-conjugate bins dropped), inverse DFT, real part / M.  nan_as_zero: a NaN real part reads as 0.
typedef std::vector<long double> lreal;
template <typename T> static lreal nl_real_row(const cx<T>* z, int vin, int M, bool nan_as_zero = false) {
  lvec X(M);
  for (int p = 0; p < M; ++p) { X[p].x = 0; X[p].y = 0; }
  for (int q = 0; q < vin; ++q) {
    long double zr = z[q].x, zi = z[q].y;
    if (nan_as_zero && zr != zr) zr = 0;
    if (q == 0 || (M % 2 == 0 && q == M / 2)) zi = 0;
    X[q].x = zr; X[q].y = zi;
    if (q != 0 && q != M - q) { X[M - q].x = zr; X[M - q].y = -zi; }
  }
  lvec x = naive_dft(X, +1);
  lreal re(M);
  for (int p = 0; p < M; ++p) re[p] = x[p].x / M;
  return re;
}
// spectra of the products of real rows: component c of a x b, and sum_f a_f b_f (a, b: three rows each)
static lvec nl_cross_spectrum(const lreal* a, const lreal* b, int c) {
  const int c1 = (c + 1) % 3, c2 = (c + 2) % 3, M = (int)a[0].size();
  lvec x(M);
  for (int p = 0; p < M; ++p) { x[p].x = a[c1][p] * b[c2][p] - a[c2][p] * b[c1][p]; x[p].y = 0; }
  return naive_dft(x, -1);
}
static lvec nl_dot_spectrum(const lreal* a, const lreal* b) {
  const int M = (int)a[0].size();
  lvec x(M);
  for (int p = 0; p < M; ++p) { x[p].x = a[0][p] * b[0][p] + a[1][p] * b[1][p] + a[2][p] * b[2][p]; x[p].y = 0; }
  return naive_dft(x, -1);
}
// a result row g against its reference X over the valid bins: num += |g - X|^2, den += |X|^2
template <typename T> static void nl_accumulate(const cx<T>* g, const lvec& X, int valid, RelL2& err) {
  for (int q = 0; q < valid; ++q) {
    const long double d = (g[q].x - X[q].x) * (g[q].x - X[q].x) + (g[q].y - X[q].y) * (g[q].y - X[q].y);
    err.num += d == d ? d : 1;                     // (a NaN must not vanish in the comparison with the tolerance)
    err.den += X[q].x * X[q].x + X[q].y * X[q].y;
  }
}
// nothing is stored beyond the valid bins of a result row g: bins [valid, pout) hold what they held -- the bins of `was`, the row
// of the input the result lies over, or (null) the 7s the tests fill their own result rows with
template <typename T> static void nl_tail_kept(const cx<T>* g, const cx<T>* was, int valid, int pout, RelL2& err) {
  for (int q = valid; q < pout; ++q) {
    const cx<T> w = was ? was[q] : mk<T>((T)7, (T)7);
    if (g[q].x != w.x || g[q].y != w.y) err.num += 1;
  }
}

// What the tests set up alike.  nf fields of nrows rows of pin bins, uniform(-amp, amp) from one seed, drawn field by field, and
// their copies keep[]; nout result arrays of nrows rows of pout bins, filled with 7s; `extra` more rows of NaNs behind both.
template <class S, typename T>
struct NlzFixture {
  int nf, nrows, pin, pout;
  std::vector<cx<T>> in[9], keep[9], out[4], tw = build_pass_twiddles<S, T>();
  NlzFixture(int nf, unsigned long long seed, int nrows, int pin, int pout, int nout, int extra = 0, double amp = 1.0)
      : nf(nf), nrows(nrows), pin(pin), pout(pout) {
    Uniform U(seed, amp);
    const cx<T> nan = mk<T>(std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::quiet_NaN());
    for (int f = 0; f < nf; ++f) {
      in[f].resize((size_t)(nrows + extra) * pin);
      U.fill(in[f]);
      std::fill(in[f].begin() + (size_t)nrows * pin, in[f].end(), nan);
    }
    for (int c = 0; c < nout; ++c) {
      out[c].assign((size_t)(nrows + extra) * pout, mk<T>((T)7, (T)7));
      std::fill(out[c].begin() + (size_t)nrows * pout, out[c].end(), nan);
    }
    snapshot();
  }
  void snapshot() { for (int f = 0; f < nf; ++f) keep[f] = in[f]; }
  // the parameters every body reads: a = fields 0 .. 2, b = fields 3 .. 5 (those there are), no results yet, scale 1 / M^2
  void params(NlzParams<T>& P, int valid, int vin, int M, const cx<T>* rt3 = nullptr) const {
    for (int f = 0; f < 3; ++f) {
      P.a[f] = f < nf ? in[f].data() : nullptr;
      P.b[f] = 3 + f < nf ? in[3 + f].data() : nullptr;
      P.out[f] = nullptr;
    }
    P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
    P.scale = (T)(1.0 / ((double)M * (double)M));
    P.rt3 = rt3;
  }
  // the real rows that row r of the fields (as they were) stands for
  std::vector<lreal> real_rows(int r, int vin, int M) const {
    std::vector<lreal> re(nf);
    for (int f = 0; f < nf; ++f) re[f] = nl_real_row(keep[f].data() + (size_t)r * pin, vin, M);
    return re;
  }
  // where result c lies: over the input field `over`, or (-1) in out[c]
  cx<T>* result(int c, int over) { return over >= 0 ? in[over].data() : out[c].data(); }
  // row r of result c holds nothing new beyond its valid bins
  void tail_kept(const cx<T>* g, int r, int over, int valid, RelL2& err) const {
    nl_tail_kept<T>(g, over >= 0 ? keep[over].data() + (size_t)r * pin : nullptr, valid, pout, err);
  }
  // the inputs that were not preserved (bytes: NaNs compare), but for those a result lies over (over[0..nres): the field, or -1)
  int inputs_changed(const int* over = nullptr, int nres = 0) const {
    int changed = 0;
    for (int f = 0; f < nf; ++f) {
      bool taken = false;
      for (int c = 0; c < nres; ++c) taken = taken || over[c] == f;
      if (!taken && memcmp(in[f].data(), keep[f].data(), keep[f].size() * sizeof(cx<T>)) != 0) ++changed;
    }
    return changed;
  }
};

// fused nonlinear z stage (fft_nlz.h): out_f = rfft((irfft(a) x irfft(b))_f), rows of `valid` bins, against long-double DFTs
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
static void test_nlz(int valid, bool inplace, int valid_in = 0) {      // valid_in: fewer input bins than stored ones (pruned 2/3-rule)
  typedef NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE> K;
  const int vin = valid_in > 0 ? valid_in : valid;
  const int M = S::N;
  const int nrows = 2 * ROWS + 3;                 // an odd count: the last pair has one row
  const int pin = valid + 2, pout = inplace ? pin : valid + 1;
  NlzFixture<S, T> fx(6, 4242 + M + valid, nrows, pin, pout, 3);
  NlzParams<T> P;
  fx.params(P, valid, vin, M);
  for (int f = 0; f < 3; ++f) P.out[f] = fx.result(f, inplace ? f : -1);
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = fx.real_rows(r, vin, M);
    for (int c = 0; c < 3; ++c) {
      const cx<T>* g = P.out[c] + (size_t)r * pout;
      nl_accumulate(g, nl_cross_spectrum(&re[0], &re[3], c), valid, err);
      if (!inplace) fx.tail_kept(g, r, -1, valid, err);
    }
  }
  char name[64];
  snprintf(name, sizeof name, "nlz r%d v%d/%d%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "", inplace ? " inpl" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), err.value(), sizeof(T) == 8 ? 4e-14 : 2e-5);
}
// ... with the dot product (NlzFft::body_dot): out = rfft(sum_f irfft(a_f) irfft(b_f)), one row out per six rows in.
// alias: 0 out of place, 1 the result over a_0, 2 over b_1 (row for row); the other five inputs must come back untouched
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
static void test_nld(int valid, int alias, int valid_in = 0) {
  typedef NlzProd<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>, NlzProduct::Dot> K;
  const int vin = valid_in > 0 ? valid_in : valid;
  const int M = S::N;
  const int nrows = 2 * ROWS + 3;                 // an odd count: the last pair has one row
  const int pin = valid + 2, pout = alias ? pin : valid + 1;
  NlzFixture<S, T> fx(6, 2424 + M + valid, nrows, pin, pout, 1);
  const int af = alias == 1 ? 0 : alias == 2 ? 4 : -1;      // the input field the result lies over
  NlzParams<T> P;
  fx.params(P, valid, vin, M);
  P.out[0] = fx.result(0, af);
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = fx.real_rows(r, vin, M);
    const cx<T>* g = P.out[0] + (size_t)r * pout;
    nl_accumulate(g, nl_dot_spectrum(&re[0], &re[3]), valid, err);
    fx.tail_kept(g, r, af, valid, err);
  }
  err.num += fx.inputs_changed(&af, 1);
  char name[72];
  snprintf(name, sizeof name, "nld r%d v%d/%d%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "",
           alias == 1 ? " over a0" : alias == 2 ? " over b1" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), err.value(), sizeof(T) == 8 ? 4e-14 : 2e-5);
}
template <class S> static void test_nld_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;     // every bin / the bins of the un-padded mesh under the 3/2-rule
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nld<S, double, 2, true, false, true>(lim, 1);
    test_nld<S, double, 1, false, false, true>(full, 2);
    test_nld<S, float, 3, false, false, true>(full, 0);
    test_nld<S, float, 2, true, false, true>(lim, 2);
  }
  test_nld<S, double, 2, true, false>(full, 0);
  test_nld<S, double, 1, false, true>(lim, 1);
  test_nld<S, double, 2, true, true>(full, 2);
  test_nld<S, double, 3, false, false>(lim, 0);
  test_nld<S, float, 3, false, false>(lim, 0);
  test_nld<S, float, 2, true, true>(full, 1);
  test_nld<S, float, 1, false, true>(lim, 2);
  test_nld<S, float, 2, true, false>(full, 2);
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins in, every bin out
    test_nld<S, double, 2, true, false>(full, 1, lim);
    test_nld<S, double, 1, false, true>(full, 0, lim);
    test_nld<S, float, 3, false, false>(full, 0, (2 * full) / 3);
    test_nld<S, float, 2, true, true>(full, 2, (2 * full) / 3);
  }
}

// ... with the cross AND the dot product (NlzFft::body_cross_dot, NlcParams): out[f] = rfft((irfft(a) x irfft(b))_f) and
// outs = rfft(sum_f irfft(a_f) irfft(c_f)), four rows out per nine rows in.  alias: 0 out of place, 1 the cross product over a and
// the scalar row over c_2, 2 the cross product over b and the scalar row over c_0 (row for row); every other input must come back
// untouched.  poison: the buffers hold one more row than nrows (an odd count), full of NaNs -- the missing partner of the last
// row must contribute nothing, whatever lies behind the last row.
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
static void test_nlc(int valid, int alias, int valid_in = 0, bool poison = false) {
  typedef NlzProd<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>, NlzProduct::CrossDot> K;
  const int vin = valid_in > 0 ? valid_in : valid;
  const int M = S::N;
  const int nrows = 2 * ROWS + 3;                 // an odd count: the last pair has one row
  const int pin = valid + 2, pout = alias ? pin : valid + 1;
  const int extra = poison ? 1 : 0;
  NlzFixture<S, T> fx(9, 4224 + M + valid, nrows, pin, pout, 4, extra);      // a, b, c
  // the input field each result lies over (-1: none)
  int over[4] = {-1, -1, -1, -1};
  if (alias == 1) { over[0] = 0; over[1] = 1; over[2] = 2; over[3] = 8; }
  if (alias == 2) { over[0] = 3; over[1] = 4; over[2] = 5; over[3] = 6; }
  NlcParams<T> P;
  fx.params(P, valid, vin, M);
  cx<T>* res[4];
  for (int c = 0; c < 4; ++c) res[c] = fx.result(c, over[c]);
  for (int f = 0; f < 3; ++f) { P.c[f] = fx.in[6 + f].data(); P.out[f] = res[f]; }
  P.outs = res[3];
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = fx.real_rows(r, vin, M);
    for (int c = 0; c < 4; ++c) {
      const cx<T>* g = res[c] + (size_t)r * pout;
      nl_accumulate(g, c < 3 ? nl_cross_spectrum(&re[0], &re[3], c) : nl_dot_spectrum(&re[0], &re[6]), valid, err);
      fx.tail_kept(g, r, over[c], valid, err);
    }
  }
  for (int c = 0; c < 4; ++c)                      // ... nor behind the last row
    for (size_t i = (size_t)nrows * pout; i < (size_t)(nrows + extra) * pout; ++i)
      if (res[c][i].x == res[c][i].x || res[c][i].y == res[c][i].y) err.num += 1;
  err.num += fx.inputs_changed(over, 4);
  char name[80];
  snprintf(name, sizeof name, "nlc r%d v%d/%d%s%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "",
           alias == 1 ? " inpl a c2" : alias == 2 ? " inpl b c0" : "", poison ? " poison" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), err.value(), sizeof(T) == 8 ? 4e-14 : 2e-5);
}
template <class S> static void test_nlc_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;     // every bin / the bins of the un-padded mesh under the 3/2-rule
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlc<S, double, 2, true, false, true>(lim, 1, 0, true);
    test_nlc<S, double, 1, false, false, true>(full, 2);
    test_nlc<S, float, 3, false, false, true>(full, 0);
    test_nlc<S, float, 2, true, false, true>(lim, 2, 0, true);
  }
  test_nlc<S, double, 2, true, false>(full, 0);
  test_nlc<S, double, 1, false, true>(lim, 1, 0, true);
  test_nlc<S, double, 2, true, true>(full, 2);
  test_nlc<S, double, 3, false, false>(lim, 0);
  test_nlc<S, float, 3, false, false>(lim, 0);
  test_nlc<S, float, 2, true, true>(full, 1, 0, true);
  test_nlc<S, float, 1, false, true>(lim, 2);
  test_nlc<S, float, 2, true, false>(full, 2);
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins in, every bin out
    test_nlc<S, double, 2, true, false>(full, 1, lim);
    test_nlc<S, double, 1, false, true>(full, 0, lim);
    test_nlc<S, float, 3, false, false>(full, 0, (2 * full) / 3);
    test_nlc<S, float, 2, true, true>(full, 2, (2 * full) / 3, true);
  }
}

// ... with the real-space maxima (fft_nlz.h NlzAbsMax, Build::AbsMax): the same rows, bit for bit, as the plain body in this
// emulator, and max |irfft(a_f)|, max |irfft(b_f)| over all rows against long-double transforms of the six rows.  A spike can
// be planted at one z position of one row of one field (over small noise), a NaN in one input bin of one field.
struct NlmCase {
  int valid = 0, valid_in = 0, nrows = 0;
  int spike_field = -1, spike_row = 0, spike_pos = 0;
  int nan_field = -1;
};
template <typename T> static T emu_nan_max(T m, T x) { return (x > m || x != x) ? x : m; }
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE, bool DOT>
static double run_nlm(const NlmCase& c) {          // the worst relative error of the six maxima; 1e30 for a broken contract
  typedef NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE> K0;
  typedef NlzProd<K0, DOT ? NlzProduct::Dot : NlzProduct::Cross> KP;
  typedef NlzAbsMax<K0, DOT ? NlzProduct::Dot : NlzProduct::Cross> KM;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows;
  const int pin = valid + 2, pout = valid + 1, nout = DOT ? 1 : 3;
  NlzFixture<S, T> fx(6, 777 + M + valid + 31 * c.spike_pos + 7 * c.spike_field, nrows, pin, pout, 3, 0, c.spike_field >= 0 ? 1e-3 : 1.0);
  std::vector<cx<T>>* const in = fx.in;
  std::vector<cx<T>>* const out0 = fx.out;
  std::vector<cx<T>> out1[3] = {out0[0], out0[1], out0[2]};      // for the body with the statistic
  if (c.spike_field >= 0) {
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int q = 0; q < vin; ++q) {
      const long double a = -two_pi * (long double)(((long long)q * c.spike_pos) % M) / M;
      cx<T>& z = in[c.spike_field][(size_t)c.spike_row * pin + q];
      z = mk<T>(z.x + (T)cosl(a), z.y + (T)sinl(a));
    }
  }
  if (c.nan_field >= 0) in[c.nan_field][(size_t)(nrows / 2) * pin + 1].x = (T)NAN;
  const int grid = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  NlmParams<T> P;
  fx.params(P, valid, vin, M);
  for (int f = 0; f < nout; ++f) P.out[f] = out0[f].data();
  P.part = nullptr;
  const NlzParams<T>& P0 = P;
  emu_launch(grid, KP::THREADS, KP::LDS_BYTES, [&](int b, int t, char* lds) { KP::body(P0, b, t, lds); });
  std::vector<T> part((size_t)grid * KM::WAVES * NLM_SLOTS, (T)-1);
  for (int f = 0; f < nout; ++f) P.out[f] = out1[f].data();
  P.part = part.data();
  emu_launch(grid, KM::THREADS, KM::LDS_BYTES, [&](int b, int t, char* lds) { KM::body(P, b, t, lds); });
  double bad = 0;
  for (int f = 0; f < nout; ++f) {                   // the statistic does not disturb the product: the same bits, NaNs where the plain body has NaNs
    if (c.nan_field < 0 && memcmp(out0[f].data(), out1[f].data(), out0[f].size() * sizeof(cx<T>)) != 0) bad = 1e30;
    for (size_t i = 0; i < out0[f].size(); ++i) {
      const T p[2] = {out0[f][i].x, out0[f][i].y}, q[2] = {out1[f][i].x, out1[f][i].y};
      for (int k = 0; k < 2; ++k)
        if ((p[k] != p[k]) != (q[k] != q[k]) || (p[k] == p[k] && memcmp(&p[k], &q[k], sizeof(T)) != 0)) bad = 1e30;
    }
  }
  T got[6] = {0, 0, 0, 0, 0, 0};
  for (size_t g = 0; g < part.size() / 6; ++g)
    for (int i = 0; i < 6; ++i) {
      if (part[g * 6 + i] < (T)0) bad = 1e30;        // a slot nobody wrote (or a negative "maximum")
      got[i] = emu_nan_max(got[i], part[g * 6 + i]);
    }
  long double want[6];
  for (int f = 0; f < 6; ++f) {
    want[f] = 0;
    for (int r = 0; r < nrows; ++r)                  // (a NaN reads as 0: the NaN field's expectation is NaN, no reference needed)
      for (long double v : nl_real_row(in[f].data() + (size_t)r * pin, vin, M, true)) want[f] = std::max(want[f], fabsl(v));
  }
  for (int f = 0; f < 6; ++f) {
    const double g = (double)got[f] / M;             // the kernel's inverse transforms are un-normalised
    // NaN: for the field that holds it ONLY.  a_f and b_f are the two halves of ONE complex transform, which is why the STATS
    // bodies take non-finite inputs out of it (fft_nlz.h take_out_nonfinite): the partner's maximum is finite and right.
    if (f == c.nan_field) { if (g == g) bad = 1e30; continue; }
    if (g != g) { bad = 1e30; continue; }
    if (c.spike_field == f && !(want[f] > 0.3L)) bad = 1e30;      // the planted extreme is the maximum of its field
    // relative to the field's OWN maximum.  One exception, the planted-extreme cases: there one field of a pair is a spike near 1
    // over noise of 1e-3, and the two share one complex transform, whose rounding errors scale with the larger of its two fields
    // (the plain kernel's rows are no better) -- the spiked field's partner, and only it, is taken relative to the pair's maximum.
    const bool partner = c.spike_field >= 0 && f != c.spike_field && f % 3 == c.spike_field % 3;
    const long double ref = partner ? std::max(want[f % 3], want[3 + f % 3]) : want[f];
    bad = std::max(bad, (double)(fabsl((long double)g - want[f]) / ref));
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE, bool DOT>
static void test_nlm(int valid, int valid_in, int nrows, bool with_nan) {
  NlmCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows;
  const double tol = sizeof(T) == 8 ? 4e-14 : 2e-5;
  char name[96];
  const int vin = valid_in > 0 ? valid_in : valid;
  snprintf(name, sizeof name, "nlm %s r%d n%d v%d/%d%s%s%s", DOT ? "dot" : "cross", ROWS, nrows, vin, valid, TWLDS ? " twlds" : "",
           SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlm<S, T, ROWS, TWLDS, SPLIT, WAVE, DOT>(c), tol);
  if (!with_nan) return;
  // a NaN in one input bin: NaN for that field, the other five as before
  c.nan_field = (S::N + ROWS + (DOT ? 1 : 0)) % 6;
  snprintf(name, sizeof name, "nlm %s r%d nan in field %d%s%s", DOT ? "dot" : "cross", ROWS, c.nan_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nlm<S, T, ROWS, TWLDS, SPLIT, WAVE, DOT>(c), tol);
}
// planted extremes: every z position for rows up to 64 points, else the positions where a lane, a register or a row would
// be left out (0, 1, TPT - 1, TPT, M/2, M - 1), in the first row and in the last row of an odd count; fields in turn
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE, bool DOT>
static void test_nlm_spikes() {
  const int M = S::N;
  std::vector<int> pos;
  if (M <= 64) for (int p = 0; p < M; ++p) pos.push_back(p);
  else pos = {0, 1, S::TPT - 1, S::TPT, M / 2, M - 1};
  double worst = 0;
  int n = 0;
  for (size_t i = 0; i < pos.size(); ++i)
    for (int last = 0; last < 2; ++last) {
      if (M > 64 && last != (int)(i % 2) && pos[i] != M - 1) continue;      // long rows: alternate, and both for the last position
      NlmCase c;
      c.valid = i % 3 == 1 ? M / 3 + 1 : M / 2 + 1;
      c.nrows = 2 * ROWS + 1;                        // odd: the last row's partner is inactive and re-reads it
      c.spike_field = (int)((i + 3 * last) % 6); c.spike_row = last ? c.nrows - 1 : 0; c.spike_pos = pos[i];
      worst = std::max(worst, run_nlm<S, T, ROWS, TWLDS, SPLIT, WAVE, DOT>(c));
      ++n;
    }
  char name[96];
  snprintf(name, sizeof name, "nlm %s r%d %d spikes%s%s%s", DOT ? "dot" : "cross", ROWS, n, TWLDS ? " twlds" : "", SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), worst, sizeof(T) == 8 ? 4e-14 : 2e-5);
}
template <class S> static void test_nlm_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nlm<S, double, 2, true, false, true, false>(lim, 0, 7, true);
    test_nlm<S, float, 3, false, false, true, true>(full, 0, 1, true);
    test_nlm_spikes<S, double, 2, true, false, true, true>();
    test_nlm_spikes<S, float, 3, false, false, true, false>();
  }
  test_nlm<S, double, 2, true, false, false, false>(full, 0, 7, false);
  test_nlm<S, double, 1, false, true, false, true>(lim, 0, 1, true);
  test_nlm<S, float, 2, true, true, false, false>(full, 0, 5, true);
  test_nlm<S, float, 3, false, false, false, true>(lim, 0, 1, false);
  test_nlm_spikes<S, double, 1, false, true, false, false>();
  test_nlm_spikes<S, float, 1, true, false, false, true>();
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins in, every bin out
    test_nlm<S, double, 2, true, false, false, true>(full, lim, 7, false);
    test_nlm<S, float, 1, false, true, false, false>(full, (2 * full) / 3, 3, false);
  }
}

// The stage that ends in a reduction (nlz_moments.h NlzMoments::body, Op::Moments): [min, max, S1 .. S4] of up to six real fields over all
// rows against long-double transforms of the rows.  The launch has `ngroups` workgroups whatever the row count, so the loop over
// the rows iterates and ends unevenly; the waves' slots are added up on the host in the order of the fold kernel.
struct NlsCase {
  int valid = 0, valid_in = 0, nrows = 0, nfields = 1, ngroups = 1;
  bool center = false;
  int bad_field = -1;
  bool inf = false;
};
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static double run_nls(const NlsCase& c, double tol) {      // the worst error in units of its bound, times tol; 1e30 for a broken contract
  typedef NlzMoments<NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE>> K;
  const int M = S::N, valid = c.valid, vin = c.valid_in > 0 ? c.valid_in : c.valid, nrows = c.nrows, nf = c.nfields;
  const int pin = valid + 2;
  const bool two = nf % 2 == 0;                      // a and b: field f of a rides with field f of b
  const int ncomp = two ? nf / 2 : nf;
  NlzFixture<S, T> fx(nf, 4242 + M + valid + 13 * nf + nrows, nrows, pin, 0, 0);
  std::vector<cx<T>>* const in = fx.in;
  for (int f = 0; f < nf; ++f)
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  if (c.bad_field >= 0) in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
  fx.snapshot();
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  NlsParams<T> P;
  int slot_of[6];
  fx.params(P, valid, vin, M);
  for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; }      // the fields go where their slots are
  for (int i = 0; i < 6; ++i) P.center[i] = 0.0;
  for (int f = 0; f < nf; ++f) {
    const int slot = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
    (slot % 2 ? P.b : P.a)[slot / 2] = in[f].data();
    P.center[slot] = c.center ? 0.5 * (f + 1) + 0.125 : 0.0;
    slot_of[f] = slot;
  }
  P.scale = (T)1;
  P.norm = 1.0 / (double)M; P.npairs = (nf + 1) / 2; P.ngroups = grid;
  std::vector<double> part((size_t)grid * K::WAVES * NLS_SLOTS, -7.0);
  P.part = part.data();
  emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  double bad = fx.inputs_changed() ? 1e30 : 0;       // the inputs are preserved
  for (double v : part)
    if (v == -7.0) bad = 1e30;                       // a slot nobody wrote
  const long double eps = 2.220446049250313e-16L;
  for (int f = 0; f < nf; ++f) {
    double got[6] = {INFINITY, -INFINITY, 0, 0, 0, 0};
    for (size_t w = 0; w < part.size() / NLS_SLOTS; ++w) {
      const double* q = part.data() + w * NLS_SLOTS + slot_of[f] * NLS_STATS;
      got[0] = (q[0] < got[0] || q[0] != q[0]) ? q[0] : got[0];
      got[1] = emu_nan_max(got[1], q[1]);
      for (int k = 2; k < 6; ++k) got[k] += q[k];
    }
    if (f == c.bad_field) {                          // NaN sums; NaN extremes, or for an Inf bin -Inf / +Inf or NaN
      for (int k = 2; k < 6; ++k) if (got[k] == got[k]) bad = 1e30;
      if (!c.inf && (got[0] == got[0] || got[1] == got[1])) bad = 1e30;
      if (c.inf && !((got[0] != got[0] || got[0] == -INFINITY) && (got[1] != got[1] || got[1] == INFINITY))) bad = 1e30;
      continue;
    }
    const long double ctr = P.center[slot_of[f]];
    long double mn = INFINITY, mx = -INFINITY, sp[5] = {0, 0, 0, 0, 0}, sa[5] = {0, 0, 0, 0, 0}, s2p[5] = {0, 0, 0, 0, 0}, sx2 = 0, amax = 0;
    for (int r = 0; r < nrows; ++r)
      for (long double x : nl_real_row(in[f].data() + (size_t)r * pin, vin, M)) {
        mn = std::min(mn, x); mx = std::max(mx, x); amax = std::max(amax, fabsl(x)); sx2 += x * x;
        const long double d = x - ctr;
        long double dp = 1;
        for (int p = 1; p <= 4; ++p) { s2p[p] += dp * dp; dp *= d; sp[p] += dp; sa[p] += fabsl(dp); }      // s2p[p] = sum d^(2 (p - 1))
      }
    const long double cnt = (long double)nrows * M;
    for (int k = 0; k < 6; ++k)
      if (got[k] != got[k]) bad = 1e30;              // a clean field next to a bad one stays finite
    bad = std::max(bad, (double)(fabsl(got[0] - mn) / amax));
    bad = std::max(bad, (double)(fabsl(got[1] - mx) / amax));
    for (int p = 1; p <= 4; ++p) {                    // the transform's relative-L2 error pushed through x -> (x - c)^p, plus a double sum in any order
      const long double bound = tol * p * sqrtl(s2p[p] * sx2) + (cnt + 8) * eps * sa[p];
      bad = std::max(bad, (double)(fabsl(got[1 + p] - sp[p]) / bound * tol));
    }
  }
  return bad;
}
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE>
static void test_nls(int nfields, int valid, int valid_in, int nrows, int ngroups, bool center, int bad_kind = 0) {
  NlsCase c;
  c.valid = valid; c.valid_in = valid_in; c.nrows = nrows; c.nfields = nfields; c.ngroups = ngroups; c.center = center;
  const double tol = sizeof(T) == 8 ? 4e-14 : 2e-5;
  const int vin = valid_in > 0 ? valid_in : valid;
  char name[128];
  snprintf(name, sizeof name, "nls f%d r%d n%d g%d v%d/%d%s%s%s%s", nfields, ROWS, nrows, ngroups, vin, valid, center ? " centre" : "",
           TWLDS ? " twlds" : "", SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nls<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
  if (!bad_kind) return;
  c.bad_field = (S::N + ROWS) % nfields;
  c.inf = bad_kind == 2;
  snprintf(name, sizeof name, "nls f%d r%d %s in field %d%s%s", nfields, ROWS, c.inf ? "inf" : "nan", c.bad_field, SPLIT ? " split" : "", WAVE ? " wave" : "");
  report(name, S::N, pname<T>(), run_nls<S, T, ROWS, TWLDS, SPLIT, WAVE>(c, tol), tol);
}
template <class S> static void test_nls_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build
    test_nls<S, double, 2, true, false, true>(6, lim, 0, 7, 1, true, 1);
    test_nls<S, float, 3, false, false, true>(1, full, 0, 1, 4, false, 2);
  }
  test_nls<S, double, 2, true, false, false>(3, full, 0, 7, 2, false, 2);
  test_nls<S, double, 1, false, true, false>(2, lim, 0, 1, 1, true, 1);
  test_nls<S, float, 2, true, true, false>(6, full, 0, 5, 1, false, 1);
  test_nls<S, float, 3, false, false, false>(3, lim, 0, 2 * 6 + 3, 1, true, 2);          // two passes of the one workgroup and a ragged rest
  test_nls<S, float, 2, true, false, false>(2, full, 0, 1, 1, false, 0);
  test_nls<S, double, 1, false, true, false>(1, full, 0, 3 * 4 + 3, 2, false, 0);         // three passes of two workgroups and a ragged rest
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins are read
    test_nls<S, double, 2, true, false, false>(2, full, lim, 7, 1, false, 0);
    test_nls<S, float, 1, false, true, false>(1, full, (2 * full) / 3, 3, 1, true, 0);
  }
}

// the pruned 3/2-rule flavour (Nlz3Fft): M = 3 L, L + 1 bins per row, three sub-transforms per row
template <class SL, typename T, int ROWS, bool TWLDS>
static void test_nlz3(bool inplace) {
  typedef Nlz3Fft<SL, T, ROWS, TWLDS> K;
  const int L = SL::N, M = 3 * L, valid = L + 1;
  const int nrows = 2 * ROWS + 3;
  const int pin = valid + 2, pout = inplace ? pin : valid + 1;
  NlzFixture<SL, T> fx(6, 777 + M, nrows, pin, pout, 3);
  auto rt = build_nlz3_twiddles<T>(L);
  NlzParams<T> P;
  fx.params(P, valid, valid, M, rt.data());
  for (int f = 0; f < 3; ++f) P.out[f] = fx.result(f, inplace ? f : -1);
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = fx.real_rows(r, valid, M);      // (L + 1 bins of 3 L points: bin 0 alone is its own conjugate)
    for (int c = 0; c < 3; ++c) {
      const cx<T>* g = P.out[c] + (size_t)r * pout;
      nl_accumulate(g, nl_cross_spectrum(&re[0], &re[3], c), valid, err);
      if (!inplace) fx.tail_kept(g, r, -1, valid, err);
    }
  }
  char name[64];
  snprintf(name, sizeof name, "nlz3 r%d%s%s", ROWS, TWLDS ? " twlds" : "", inplace ? " inpl" : "");
  report(name, M, pname<T>(), err.value(), sizeof(T) == 8 ? 4e-14 : 2e-5);
}
template <class SL> static void test_nlz3_all() {
  test_nlz3<SL, double, 2, true>(false);
  test_nlz3<SL, double, 1, false>(true);
  test_nlz3<SL, float, 3, false>(false);
  test_nlz3<SL, float, 2, true>(true);
}
template <class S> static void test_nlz_all() {
  const int M = S::N;
  const int full = M / 2 + 1, lim = M / 3 + 1;     // every bin / the bins of the un-padded mesh under the 3/2-rule
  if constexpr (S::TPT <= 64 && 64 % S::TPT == 0) {      // the wave-synchronous build (in the emulator its wave barriers are workgroup barriers)
    test_nlz<S, double, 2, true, false, true>(lim, true);
    test_nlz<S, float, 3, false, false, true>(full, false);
  }
  test_nlz<S, double, 2, true, false>(full, false);
  test_nlz<S, double, 1, false, true>(lim, true);
  test_nlz<S, float, 3, false, false>(lim, false);
  test_nlz<S, float, 2, true, true>(full, true);
  if (lim < full) {                                 // pruned 2/3-rule: the kept kz bins in, every bin out
    test_nlz<S, double, 2, true, false>(full, true, lim);
    test_nlz<S, float, 3, false, false>(full, false, (2 * full) / 3);
  }
}

// every plan of the stage:  #define EMU_CASE(N, ...) test_nld_all<Spec<N, __VA_ARGS__>>();  then  EMU_NLZ_PLANS(EMU_CASE)
#define EMU_NLZ_PLANS(X) MFFT_NLZPLANS_P2(X) MFFT_NLZPLANS_3(X) MFFT_NLZPLANS_9(X)
