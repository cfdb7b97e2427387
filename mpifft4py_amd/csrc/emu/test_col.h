// test_col.h -- emulator tests of the strided (column) kernels: ColFft with its pad / mask / band builds, the chirp-z ColFftZ
// and the three-sub-transform ColFft3 / ColFft3S
#pragma once
#include "emu.h"
#include "fft_chirpz.h"
#include "fft_col3.h"

template <class S, typename T, int COLS, bool INV, bool TWLDS, int SPLIT = 0, int VEC = 1>
static void test_col(bool two_level) {
  typedef ColFft<S, T, COLS, INV, TWLDS, SPLIT, VEC> K;
  const int N = S::N;
  const int ncols = COLS * 2 + 3;          // ragged last tile
  const int nouter = 2;
  Uniform U(1234 + N);
  // input layout [outer][row][col] with row pitch pin; output pitch pout
  const int pin = ncols + 2, pout = ncols + 5;
  const int split = two_level ? (N % 4 == 0 ? N / 4 : N) : N;
  // two-level output: row r -> (r/split)*hi + (r%split)*lo with hi = "chunk" stride
  const i64 out_lo = pout, out_hi = (i64)split * pout * nouter;   // chunks interleave the outer index
  std::vector<cx<T>> in((size_t)nouter * N * pin), out((size_t)nouter * N * pout * 2, mk<T>((T)777, (T)777));
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  ColParams<T> P;
  P.in = in.data();
  P.out = out.data();
  P.tw = tw.data();
  P.in_outer = (i64)N * pin;
  P.in_map = make_rowmap(0, pin, N, N);
  if (two_level) {
    P.out_outer = (i64)split * pout;
    P.out_map = make_rowmap(out_hi, out_lo, split, N);
  } else {
    P.out_outer = (i64)N * pout;
    P.out_map = make_rowmap(0, pout, N, N);
  }
  P.ncols = ncols;
  P.ntile_c = (ncols + COLS - 1) / COLS;
  P.nouter = nouter;
  P.remap = two_level ? 1 : 0;
  P.scale = INV ? (T)(1.0 / N) : (T)1;
  emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES,
             [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      lvec X = naive_dft(l_vec(&in[(size_t)o * N * pin + c], N, pin), INV ? +1 : -1);
      for (int r = 0; r < N; ++r)
        err.add(out[(i64)o * P.out_outer + row_off(P.out_map, r) + c], scaled(X[r], INV ? 1.0L / N : 1.0L));
    }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d %s%s%s%s", COLS, VEC, INV ? "inv" : "fwd", TWLDS ? " twlds" : "", two_level ? " 2lvl" : "", SPLIT == 2 ? " quarter" : SPLIT ? " split" : "");
  report(name, N, pname<T>(), err.value(), tol_of<T>());
}

// Wrapped input columns (ColParams::in_wrap, round 5): the same truncating forward kernel on a compact input and on one whose
// columns sit in rows of W columns at a pitch of W + 3 (W odd, so that a lane's VEC columns straddle the end of a row
// somewhere) must store the same bits.  K: any strided kernel type whose output has `nout` rows.
template <class K, typename T>
static void test_wrapped_columns(const char* what, int N, int nout, const cx<T>* tw, int cols_per_tile) {
  const int W = 5, G = 2 * cols_per_tile / W + 3, ncols = W * G, Wp = W + 3;
  const int pin_a = ncols + 1, pin_b = G * Wp + 2, pout = ncols + 2;
  Uniform U(4321 + N);
  std::vector<cx<T>> a((size_t)N * pin_a), b((size_t)N * pin_b, mk<T>((T)99, (T)99));
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < ncols; ++c) {
      const cx<T> z = U.pair<T>();
      a[(size_t)r * pin_a + c] = z;
      b[(size_t)r * pin_b + (size_t)(c / W) * Wp + c % W] = z;
    }
  std::vector<cx<T>> out_a((size_t)nout * pout, mk<T>((T)5, (T)5)), out_b = out_a;
  for (int wrapped = 0; wrapped < 2; ++wrapped) {
    ColParams<T> P;
    memset(&P, 0, sizeof P);
    P.in = wrapped ? b.data() : a.data(); P.out = wrapped ? out_b.data() : out_a.data(); P.tw = tw;
    P.in_map = make_rowmap(0, wrapped ? pin_b : pin_a, 0, N); P.out_map = make_rowmap(0, pout, 0, nout);
    P.ncols = ncols; P.ntile_c = (ncols + cols_per_tile - 1) / cols_per_tile; P.nouter = 1; P.remap = wrapped; P.fold = 1;
    P.scale = (T)0.5;
    if (wrapped) { P.in_wrap = W; P.in_wrap_gap = Wp - W; }
    emu_launch(P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int bb, int t, char* lds) { K::body(P, bb, t, lds); });
  }
  size_t bad = 0;
  for (size_t i = 0; i < out_a.size(); ++i) bad += memcmp(&out_a[i], &out_b[i], sizeof(cx<T>)) != 0;
  bool any = false;
  for (int c = 0; c < ncols; ++c) any = any || out_a[c].x != (T)5;
  report(what, N, pname<T>(), (bad == 0 && any) ? 0.0 : 1.0, tol_of<T>());
}

// 3/2-rule fusion: PAD == 1 (inverse, zero band on load) and PAD == 2 (forward, truncate on store,
// with and without the Nyquist fold) against explicit pad / truncate around a plain DFT
template <class S, typename T, int COLS, int VEC>
static void test_col_pad() {
  const int N = S::N, n = 2 * N / 3, h = n / 2;
  const int ncols = COLS + 3, nouter = 2;
  Uniform U(31 + N);
  auto tw = build_pass_twiddles<S, T>();
  {  // PAD 1, inverse: in (nouter, n, pin) -> out (nouter, N, pout)
    typedef ColFft<S, T, COLS, true, false, false, VEC, false, 1> K;
    const int pin = ncols + 1, pout = ncols + 2;
    std::vector<cx<T>> in((size_t)nouter * n * pin), out((size_t)nouter * N * pout);
    U.fill(in);
    ColParams<T> P;
    P.in = in.data(); P.out = out.data(); P.tw = tw.data();
    P.in_outer = (i64)n * pin; P.out_outer = (i64)N * pout;
    P.in_map = make_rowmap(0, pin, n, n); P.out_map = make_rowmap(0, pout, N, N);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.fold = 0;
    P.scale = (T)(1.0 / N);
    emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    RelL2 err;
    for (int o = 0; o < nouter; ++o)
      for (int c = 0; c < ncols; ++c) {
        lvec x(N);
        for (int r = 0; r < N; ++r) { x[r].x = 0; x[r].y = 0; }
        for (int r = 0; r < n; ++r) x[r < h ? r : N - n + r] = to_l(in[(size_t)o * n * pin + (size_t)r * pin + c]);
        lvec X = naive_dft(x, +1);
        for (int r = 0; r < N; ++r) {
          const cx<long double> want = {X[r].x / N, X[r].y / N};
          err.add(out[(size_t)o * N * pout + (size_t)r * pout + c], want);
        }
      }
    char name[64];
    snprintf(name, sizeof name, "col c%d v%d pad-on-load inv", COLS, VEC);
    report(name, N, pname<T>(), err.value(), tol_of<T>());
  }
  for (int fold = 0; fold < 2; ++fold) {  // PAD 2, forward: in (nouter, N, pin) -> out (nouter, n, pout)
    typedef ColFft<S, T, COLS, false, false, false, VEC, false, 2> K;
    const int pin = ncols + 1, pout = ncols + 2;
    std::vector<cx<T>> in((size_t)nouter * N * pin), out((size_t)nouter * n * pout, mk<T>((T)55, (T)55));
    U.fill(in);
    ColParams<T> P;
    P.in = in.data(); P.out = out.data(); P.tw = tw.data();
    P.in_outer = (i64)N * pin; P.out_outer = (i64)n * pout;
    P.in_map = make_rowmap(0, pin, N, N); P.out_map = make_rowmap(0, pout, n, n);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 0; P.fold = fold;
    P.scale = (T)0.5;
    emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    RelL2 err;
    for (int o = 0; o < nouter; ++o)
      for (int c = 0; c < ncols; ++c) {
        lvec X = naive_dft(l_vec(&in[(size_t)o * N * pin + c], N, pin), -1);
        lvec e(n);
        for (int r = 0; r < n; ++r) { e[r].x = 0; e[r].y = 0; }
        if (fold) {
          for (int r = 0; r <= h; ++r) e[r] = X[r];
          for (int r = 0; r < h; ++r) { e[h + r].x += X[N - h + r].x; e[h + r].y += X[N - h + r].y; }
        } else {
          for (int r = 0; r < h; ++r) e[r] = X[r];
          for (int r = h; r < n; ++r) e[r] = X[N - n + r];
        }
        for (int r = 0; r < n; ++r) err.add(out[(size_t)o * n * pout + (size_t)r * pout + c], scaled(e[r], 0.5L));
      }
    char name[64];
    snprintf(name, sizeof name, "col c%d v%d trunc-on-store%s", COLS, VEC, fold ? " fold" : "");
    report(name, N, pname<T>(), err.value(), tol_of<T>());
  }
  {
    char name[64];
    snprintf(name, sizeof name, "col c%d v%d trunc-on-store, wrapped input columns", COLS, VEC);
    test_wrapped_columns<ColFft<S, T, COLS, false, false, false, VEC, false, 2>, T>(name, N, n, tw.data(), COLS);
    snprintf(name, sizeof name, "col c%d v%d plain fwd, wrapped input columns", COLS, VEC);
    test_wrapped_columns<ColFft<S, T, COLS, false, false, false, VEC, false, 0>, T>(name, N, N, tw.data(), COLS);
  }
}

// 2/3-rule: the masked-load build (PAD == 3) against the plain inverse kernel on a pre-masked copy of the input
template <class S, typename T, int COLS, int VEC>
static void test_col_mask() {
  typedef ColFft<S, T, COLS, true, false, false, VEC, false, 3> KM;
  typedef ColFft<S, T, COLS, true, false, false, VEC> K0;
  const int N = S::N, ncols = COLS * 2 + 3, nouter = 2, pin = ncols + 1;
  Uniform U(77 + N);
  std::vector<cx<T>> in((size_t)nouter * N * pin), pre(in.size()), out1(in.size(), mk<T>((T)5, (T)5)), out0(in.size(), mk<T>((T)5, (T)5));
  std::vector<unsigned char> mask(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    in[i] = U.pair<T>();
    mask[i] = (unsigned char)((U.rng() % 3) != 0);
    pre[i] = mask[i] ? in[i] : mk<T>((T)0, (T)0);
  }
  auto tw = build_pass_twiddles<S, T>();
  ColParams<T> P;
  memset(&P, 0, sizeof P);
  P.tw = tw.data();
  P.in_outer = P.out_outer = (i64)N * pin;
  P.in_map = P.out_map = make_rowmap(0, pin, N, N);
  P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.scale = (T)(1.0 / N);
  P.in = in.data(); P.out = out1.data(); P.mask = mask.data();
  emu_launch(P.ntile_c * nouter, KM::THREADS, KM::LDS_BYTES, [&](int b, int t, char* lds) { KM::body(P, b, t, lds); });
  P.in = pre.data(); P.out = out0.data(); P.mask = nullptr;
  emu_launch(P.ntile_c * nouter, K0::THREADS, K0::LDS_BYTES, [&](int b, int t, char* lds) { K0::body(P, b, t, lds); });
  RelL2 err;
  for (int o = 0; o < nouter; ++o)
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < ncols; ++c) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        err.add(out1[i], out0[i]);
      }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d inv masked load", COLS, VEC);
  report(name, N, pname<T>(), err.value(), 1e-30);     // same arithmetic on the same values: identical
}

// pruned 2/3-rule pass (PAD == 4): removed rows read as zero, tiles without a kept column untouched, kept columns
// identical to the plain inverse kernel on an input whose removed rows were zeroed
template <class S, typename T, int COLS, int VEC>
static void test_col_band() {
  typedef ColFft<S, T, COLS, true, false, false, VEC, false, 4> KB;
  typedef ColFft<S, T, COLS, true, false, false, VEC> K0;
  const int N = S::N, ncols = COLS * 3 + 1, nouter = 2, pin = ncols + 1;
  if (N < 3) return;
  Uniform U(177 + N);
  const cx<T> sentinel = mk<T>((T)5, (T)5);
  std::vector<cx<T>> in((size_t)nouter * N * pin), pre(in.size()), out1(in.size(), sentinel), out0(in.size(), sentinel);
  const int row_lo = N / 3 > 0 ? N / 3 : 1, row_hi = (2 * N) / 3 > row_lo ? (2 * N) / 3 : row_lo;
  for (int o = 0; o < nouter; ++o)
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < pin; ++c) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        in[i] = U.pair<T>();
        pre[i] = (r >= row_lo && r < row_hi) ? mk<T>((T)0, (T)0) : in[i];
      }
  auto tw = build_pass_twiddles<S, T>();
  ColParams<T> P;
  memset(&P, 0, sizeof P);
  P.tw = tw.data();
  P.in_outer = P.out_outer = (i64)N * pin;
  P.in_map = P.out_map = make_rowmap(0, pin, N, N);
  P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.scale = (T)(1.0 / N);
  P.b_row_lo = row_lo; P.b_row_hi = row_hi; P.b_coff = 2; P.b_cper = 5; P.b_clim = 3; P.b_goff = 1; P.b_gstep = 2; P.b_glo = 3; P.b_ghi = 5;
  P.in = in.data(); P.out = out1.data();
  emu_launch(P.ntile_c * nouter, KB::THREADS, KB::LDS_BYTES, [&](int b, int t, char* lds) { KB::body(P, b, t, lds); });
  P.in = pre.data(); P.out = out0.data();
  emu_launch(P.ntile_c * nouter, K0::THREADS, K0::LDS_BYTES, [&](int b, int t, char* lds) { K0::body(P, b, t, lds); });
  RelL2 err;
  int bad = 0, skipped = 0, kept = 0;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      const int t = 2 + c, z = t % 5, y = 1 + t / 5 + o * 2;
      const bool keep = z < 3 && (y < 3 || y >= 5);
      kept += keep;
      for (int r = 0; r < N; ++r) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        const bool untouched = out1[i].x == sentinel.x && out1[i].y == sentinel.y;
        if (untouched) {
          if (keep) ++bad;               // a kept column must have been transformed
          ++skipped;
          continue;
        }
        err.add(out1[i], out0[i]);
      }
    }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d inv pruned (kept %d, skipped %d)", COLS, VEC, kept, skipped / N);
  report(name, N, pname<T>(), bad || kept == 0 ? 1.0 : (double)sqrtl(err.num / (err.den > 0 ? err.den : 1)), 1e-30);
  // complete-output mode (b_gzero = 2, the pencils' first inverse pass): EVERY column is written -- kept ones as the plain
  // kernel on the row-zeroed input, columns of a removed y or z as exact zeros (per column, also inside a lane's VEC pair)
  std::vector<cx<T>> out2(in.size(), sentinel);
  P.b_gzero = 2;
  P.in = in.data(); P.out = out2.data();
  emu_launch(P.ntile_c * nouter, KB::THREADS, KB::LDS_BYTES, [&](int b, int t, char* lds) { KB::body(P, b, t, lds); });
  err = RelL2();
  bad = 0;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      const int t = 2 + c, z = t % 5, y = 1 + t / 5 + o * 2;
      const bool keep = z < 3 && (y < 3 || y >= 5);
      for (int r = 0; r < N; ++r) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        if (out2[i].x == sentinel.x && out2[i].y == sentinel.y) { ++bad; continue; }       // nothing may stay unwritten
        const cx<T> want = keep ? out0[i] : mk<T>((T)0, (T)0);
        if (!keep && (out2[i].x != (T)0 || out2[i].y != (T)0)) ++bad;
        err.add(out2[i], want);
      }
    }
  snprintf(name, sizeof name, "col c%d v%d inv band, complete output", COLS, VEC);
  report(name, N, pname<T>(), bad ? 1.0 : (double)sqrtl(err.num / (err.den > 0 ? err.den : 1)), 1e-30);
}

template <class S, typename T, int COLS, bool INV, bool SPLIT, int VEC>
static void test_col_z(int n) {
  typedef ColFftZ<S, T, COLS, INV, SPLIT, VEC> K;
  const int ncols = COLS + 3, nouter = 2;
  Uniform U(4321 + n);
  const int pin = ncols + 2, pout = ncols + 5;
  std::vector<cx<T>> in((size_t)nouter * n * pin), out((size_t)nouter * n * pout, mk<T>((T)777, (T)777));
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(n);
  auto bh = build_chirp_filter<T>(n, S::N);
  ColParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data();
  P.in_outer = (i64)n * pin; P.out_outer = (i64)n * pout;
  P.in_map = make_rowmap(0, pin, n, n); P.out_map = make_rowmap(0, pout, n, n);
  P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.fold = 0;
  P.scale = INV ? (T)(1.0 / n) : (T)1;
  P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  RelL2 err;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      lvec X = naive_dft(l_vec(&in[(size_t)o * n * pin + c], n, pin), INV ? +1 : -1);
      for (int r = 0; r < n; ++r) err.add(out[(size_t)o * n * pout + (size_t)r * pout + c], scaled(X[r], INV ? 1.0L / n : 1.0L));
    }
  char name[64];
  snprintf(name, sizeof name, "chirpz col M=%d c%d v%d %s%s", S::N, COLS, VEC, INV ? "inv" : "fwd", SPLIT ? " split" : "");
  report(name, n, pname<T>(), err.value(), 8 * tol_of<T>());
}

// N = 3 L as three sub-transforms (fft_col3.h): plain forward / inverse (in place and out of place, two-level row maps on
// both sides, ragged last column tile), pad-on-load inverse and truncate-on-store forward with the Nyquist fold, against the
// long-double DFT of the logical data.
template <class SL, typename T, int COLS, int SPLIT, int VEC>
static void test_col3() {
  constexpr int L = SL::N, N = 3 * L;
  const int ncols = COLS + COLS / 2 + 1, nouter = 2;         // one full and one ragged tile per outer batch
  const int pitch = ncols + 3;
  Uniform U(4242 + N);
  auto tw = build_col3_twiddles<SL, T>();
  char name[96];
  for (int inv = 0; inv < 2; ++inv) {
    for (int inplace = 0; inplace < 2; ++inplace) {
      // rows through a two-level map: row r -> (r / split) * hi + (r % split) * lo
      const int split = N / 4, lo = pitch, hi = split * pitch + 5 * pitch;
      const size_t outer_stride = (size_t)4 * hi + 7;
      std::vector<cx<T>> in(outer_stride * nouter), out(outer_stride * nouter, mk<T>((T)7, (T)7));
      U.fill(in);
      std::vector<cx<T>> src = in;
      ColParams<T> P;
      memset(&P, 0, sizeof P);
      P.in = in.data(); P.out = inplace ? in.data() : out.data(); P.tw = tw.data();
      P.in_outer = (i64)outer_stride; P.out_outer = (i64)outer_stride;
      P.in_map = make_rowmap(hi, lo, split, N); P.out_map = make_rowmap(hi, lo, split, N);
      P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.scale = (T)(inv ? 1.0 / N : 1.0);
      auto run = [&](auto k) {
        typedef decltype(k) K;
        emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      };
      if (inv) run(ColFft3<SL, T, COLS, true, true, SPLIT, VEC, false, 0>{});
      else run(ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 0>{});
      const std::vector<cx<T>>& res = inplace ? in : out;
      RelL2 err;
      for (int o = 0; o < nouter; ++o)
        for (int cc = 0; cc < ncols; cc += 3) {
          auto at = [&](int r) { return o * outer_stride + (size_t)(r / split) * hi + (size_t)(r % split) * lo + cc; };
          lvec x(N);
          for (int r = 0; r < N; ++r) x[r] = to_l(src[at(r)]);
          lvec X = naive_dft(x, inv ? +1 : -1);
          for (int r = 0; r < N; ++r) err.add(res[at(r)], scaled(X[r], inv ? 1.0L / N : 1.0L));
        }
      snprintf(name, sizeof name, "col3 c%d v%d %s%s%s", COLS, VEC, inv ? "inv" : "fwd", inplace ? " in place" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), err.value(), 2 * tol_of<T>());
    }
  }
  // 3/2-rule: inverse with the zero band on input (2L physical rows), forward with the truncated output + Nyquist fold
  {
    const int n = 2 * L;
    std::vector<cx<T>> phys((size_t)n * pitch), big((size_t)N * pitch, mk<T>((T)7, (T)7)), back((size_t)n * pitch, mk<T>((T)7, (T)7));
    U.fill(phys);
    ColParams<T> P;
    memset(&P, 0, sizeof P);
    P.in = phys.data(); P.out = big.data(); P.tw = tw.data();
    P.in_map = make_rowmap(0, pitch, 0, n); P.out_map = make_rowmap(0, pitch, 0, N);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = 1; P.remap = 0; P.scale = (T)1;
    {
      typedef ColFft3<SL, T, COLS, true, true, SPLIT, VEC, false, 1> K;
      emu_launch(P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    RelL2 err;
    for (int cc = 0; cc < ncols; cc += 2) {
      lvec x(N);
      for (int r = 0; r < N; ++r) { x[r].x = 0; x[r].y = 0; }
      for (int r = 0; r < L; ++r) {
        x[r] = to_l(phys[(size_t)r * pitch + cc]);
        x[2 * L + r] = to_l(phys[(size_t)(L + r) * pitch + cc]);
      }
      lvec X = naive_dft(x, +1);
      for (int r = 0; r < N; ++r) err.add(big[(size_t)r * pitch + cc], X[r]);
    }
    snprintf(name, sizeof name, "col3 c%d v%d pad-on-load inv%s", COLS, VEC, SPLIT ? " split" : "");
    report(name, N, pname<T>(), err.value(), 2 * tol_of<T>());
    // the same with one third of a tile's transform per workgroup (ColFft3S): three times the workgroups, XCD-aware order
    // and plain order, against the kernel above (same arithmetic up to the order of the radix-3 step's sums)
    for (int remap = 0; remap < 2; ++remap) {
      std::vector<cx<T>> big2((size_t)N * pitch, mk<T>((T)7, (T)7));
      P.out = big2.data(); P.remap = remap;
      typedef ColFft3S<SL, T, COLS, true, true, SPLIT, VEC, false, 1> K;
      emu_launch(3 * P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      err = RelL2();
      for (int r = 0; r < N; ++r)
        for (int cc = 0; cc < pitch; ++cc) {     // (the differences in T, their squares in long double: not RelL2::add)
          const cx<T> g = big2[(size_t)r * pitch + cc], w0 = big[(size_t)r * pitch + cc];
          err.num += (long double)(g.x - w0.x) * (g.x - w0.x) + (long double)(g.y - w0.y) * (g.y - w0.y);
          err.den += (long double)w0.x * w0.x + (long double)w0.y * w0.y;
        }
      snprintf(name, sizeof name, "col3s c%d v%d pad-on-load inv, a third per workgroup%s%s", COLS, VEC, remap ? " remap" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), err.value(), 2 * tol_of<T>());
    }
    P.out = big.data(); P.remap = 0;
    for (int fold = 0; fold < 2; ++fold) {
      std::vector<cx<T>> full((size_t)N * pitch);
      U.fill(full);
      P.in = full.data(); P.out = back.data(); P.in_map = make_rowmap(0, pitch, 0, N); P.out_map = make_rowmap(0, pitch, 0, n);
      P.fold = fold; P.scale = (T)0.5;
      {
        typedef ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 2> K;
        emu_launch(P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      err = RelL2();
      for (int cc = 0; cc < ncols; cc += 2) {
        lvec X = naive_dft(l_vec(&full[cc], N, pitch), -1);
        for (int r = 0; r < n; ++r) {
          cx<long double> want = r < L ? X[r] : X[L + r];                  // physical row L + i = logical row 2L + i
          if (fold && r == L) { want.x += X[L].x; want.y += X[L].y; }
          err.add(back[(size_t)r * pitch + cc], scaled(want, 0.5L));
        }
      }
      snprintf(name, sizeof name, "col3 c%d v%d truncate-on-store fwd%s%s", COLS, VEC, fold ? " fold" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), err.value(), 2 * tol_of<T>());
    }
    snprintf(name, sizeof name, "col3 c%d v%d truncate-on-store fwd, wrapped input columns%s", COLS, VEC, SPLIT ? " split" : "");
    test_wrapped_columns<ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 2>, T>(name, N, n, tw.data(), COLS);
    snprintf(name, sizeof name, "col3 c%d v%d plain fwd, wrapped input columns%s", COLS, VEC, SPLIT ? " split" : "");
    test_wrapped_columns<ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 0>, T>(name, N, N, tw.data(), COLS);
  }
}
