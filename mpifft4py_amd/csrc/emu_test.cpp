// emu_test.cpp -- host-side workgroup emulator for the kernel bodies in
// fft_kernels.h (TEST INFRASTRUCTURE, built with g++, never part of the product
// library).  Each GPU thread of a workgroup is a ucontext fibre; MFFT_BARRIER()
// yields to a round-robin scheduler, so the very same body code that hipcc
// compiles for gfx950 runs here with real barrier semantics and a real shared
// "LDS" buffer.  It checks every kernel family and radix plan against an
// O(N^2) long-double DFT, so index/twiddle mistakes are found without a GPU.
//
//   make -j6 emu && for b in build/emu_test_?; do $b; done
#include <ucontext.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <functional>
#include <limits>
#include <random>
#include <vector>

#include "fft_kernels.h"
#include "fft_chirpz.h"
#include "fft_col3.h"
#include "fft_nlz.h"
#include "twiddle.h"
#include "plans.h"

namespace mfft {

struct EmuState {
  std::vector<ucontext_t> ctx;
  std::vector<char> done;
  std::vector<int> nbar;
  ucontext_t sched;
  int cur = -1;
  std::function<void(int)> fn;
};
static EmuState* g_emu = nullptr;

void emu_barrier() {
  EmuState* e = g_emu;
  e->nbar[e->cur]++;
  swapcontext(&e->ctx[e->cur], &e->sched);
}

// wave shuffle of the kernels' host build (fft_kernels.h wave_shfl): every thread parks its value, all threads meet,
// every thread reads the slot of lane `src` of its own wave, all threads meet again (the slots are reused)
static std::vector<double> g_shfl_slot;
double emu_shfl(double x, int src) {
  EmuState* e = g_emu;
  const int tid = e->cur, n = (int)e->ctx.size();
  if ((int)g_shfl_slot.size() < n) g_shfl_slot.resize(n);
  g_shfl_slot[tid] = x;
  emu_barrier();
  const int from = (tid & ~63) + src;
  if (src < 0 || src > 63) { fprintf(stderr, "EMU: shuffle from lane %d\n", src); abort(); }
  const double r = from < n ? g_shfl_slot[from] : 0.0;      // a lane beyond the workgroup: undefined on the device
  emu_barrier();
  return r;
}

static void fibre_entry() {
  EmuState* e = g_emu;
  int tid = e->cur;
  e->fn(tid);
  e->done[tid] = 1;
  swapcontext(&e->ctx[tid], &e->sched);
}

// run one workgroup of `block` threads
static void emu_run_block(int block, const std::function<void(int)>& fn) {
  static std::vector<char> stacks;
  const size_t STK = 256 * 1024;
  if (stacks.size() < STK * block) stacks.resize(STK * block);
  EmuState e;
  e.ctx.resize(block);
  e.done.assign(block, 0);
  e.nbar.assign(block, 0);
  e.fn = fn;
  g_emu = &e;
  for (int t = 0; t < block; ++t) {
    getcontext(&e.ctx[t]);
    e.ctx[t].uc_stack.ss_sp = stacks.data() + STK * t;
    e.ctx[t].uc_stack.ss_size = STK;
    e.ctx[t].uc_link = nullptr;
    makecontext(&e.ctx[t], fibre_entry, 0);
  }
  bool all_done = false;
  while (!all_done) {
    all_done = true;
    for (int t = 0; t < block; ++t) {
      if (e.done[t]) continue;
      e.cur = t;
      swapcontext(&e.sched, &e.ctx[t]);
      if (!e.done[t]) all_done = false;
    }
    // every thread must have passed the same number of barriers
    for (int t = 1; t < block; ++t)
      if (e.nbar[t] != e.nbar[0]) {
        fprintf(stderr, "EMU: divergent barrier count (thread %d: %d vs %d)\n", t, e.nbar[t], e.nbar[0]);
        abort();
      }
  }
  g_emu = nullptr;
}

template <class Body>
static void emu_launch(int grid, int block, size_t lds_bytes, Body body) {
  std::vector<char> lds(lds_bytes + 64);
  for (int b = 0; b < grid; ++b) {
    memset(lds.data(), 0xCD, lds.size());
    emu_run_block(block, [&](int tid) { body(b, tid, lds.data()); });
  }
}

}  // namespace mfft

using namespace mfft;

typedef std::vector<cx<long double>> lvec;

static lvec naive_dft_slow(const lvec& x, int sign) {
  int n = (int)x.size();
  lvec X(n);
  const long double two_pi = 6.283185307179586476925286766559L;
  for (int k = 0; k < n; ++k) {
    long double sr = 0, si = 0;
    for (int t = 0; t < n; ++t) {
      long long m = ((long long)k * t) % n;
      long double a = sign * two_pi * (long double)m / n;
      long double c = cosl(a), s = sinl(a);
      sr += x[t].x * c - x[t].y * s;
      si += x[t].x * s + x[t].y * c;
    }
    X[k].x = sr;
    X[k].y = si;
  }
  return X;
}

// O(N log N) long-double reference (recursive decimation in time over the
// smallest prime factor), validated against the O(N^2) sum in main().
static lvec naive_dft(const lvec& x, int sign) {
  int n = (int)x.size();
  int p = 0;
  for (int q : {2, 3, 5}) if (n % q == 0) { p = q; break; }
  if (n <= 5 || p == 0) return naive_dft_slow(x, sign);
  int m = n / p;
  std::vector<lvec> sub(p);
  for (int q = 0; q < p; ++q) {
    lvec s(m);
    for (int t = 0; t < m; ++t) s[t] = x[(size_t)t * p + q];
    sub[q] = naive_dft(s, sign);
  }
  lvec X(n);
  const long double two_pi = 6.283185307179586476925286766559L;
  for (int k = 0; k < n; ++k) {
    long double sr = 0, si = 0;
    for (int q = 0; q < p; ++q) {
      long long mm = ((long long)k * q) % n;
      long double a = sign * two_pi * (long double)mm / n;
      long double c = cosl(a), s = sinl(a);
      const cx<long double>& z = sub[q][k % m];
      sr += z.x * c - z.y * s;
      si += z.x * s + z.y * c;
    }
    X[k].x = sr;
    X[k].y = si;
  }
  return X;
}

static int g_fail = 0;
static void report(const char* what, int n, const char* prec, double err, double tol) {
  bool ok = err < tol && err == err;
  printf("%-28s N=%-5d %-6s rel-L2 err %.3e  %s\n", what, n, prec, err, ok ? "ok" : "FAIL");
  if (!ok) g_fail++;
}

template <typename T> static double tol_of() { return sizeof(T) == 8 ? 1e-14 : 5e-6; }
template <typename T> static const char* pname() { return sizeof(T) == 8 ? "double" : "single"; }

// ---------------------------------------------------------------------------
template <class S, typename T, int COLS, bool INV, bool TWLDS, int SPLIT = 0, int VEC = 1>
static void test_col(bool two_level) {
  typedef ColFft<S, T, COLS, INV, TWLDS, SPLIT, VEC> K;
  const int N = S::N;
  const int ncols = COLS * 2 + 3;          // ragged last tile
  const int nouter = 2;
  std::mt19937_64 rng(1234 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  // input layout [outer][row][col] with row pitch pin; output pitch pout
  const int pin = ncols + 2, pout = ncols + 5;
  const int split = two_level ? (N % 4 == 0 ? N / 4 : N) : N;
  // two-level output: row r -> (r/split)*hi + (r%split)*lo with hi = "chunk" stride
  const i64 out_lo = pout, out_hi = (i64)split * pout * nouter;   // chunks interleave the outer index
  std::vector<cx<T>> in((size_t)nouter * N * pin), out((size_t)nouter * N * pout * 2, mk<T>((T)777, (T)777));
  for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
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
  long double num = 0, den = 0;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      lvec x(N);
      for (int r = 0; r < N; ++r) {
        cx<T> z = in[(size_t)o * N * pin + (size_t)r * pin + c];
        x[r].x = z.x;
        x[r].y = z.y;
      }
      lvec X = naive_dft(x, INV ? +1 : -1);
      for (int r = 0; r < N; ++r) {
        i64 off = (i64)o * P.out_outer + row_off(P.out_map, r) + c;
        cx<T> g = out[off];
        long double ex = X[r].x * (INV ? 1.0L / N : 1.0L), ey = X[r].y * (INV ? 1.0L / N : 1.0L);
        num += (g.x - ex) * (g.x - ex) + (g.y - ey) * (g.y - ey);
        den += ex * ex + ey * ey;
      }
    }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d %s%s%s%s", COLS, VEC, INV ? "inv" : "fwd", TWLDS ? " twlds" : "", two_level ? " 2lvl" : "", SPLIT == 2 ? " quarter" : SPLIT ? " split" : "");
  report(name, N, pname<T>(), (double)sqrtl(num / den), tol_of<T>());
}

// Wrapped input columns (ColParams::in_wrap, round 5): the same truncating forward kernel on a compact input and on one whose
// columns sit in rows of W columns at a pitch of W + 3 (W odd, so that a lane's VEC columns straddle the end of a row
// somewhere) must store the same bits.  K: any strided kernel type whose output has `nout` rows.
template <class K, typename T>
static void test_wrapped_columns(const char* what, int N, int nout, const cx<T>* tw, int cols_per_tile) {
  const int W = 5, G = 2 * cols_per_tile / W + 3, ncols = W * G, Wp = W + 3;
  const int pin_a = ncols + 1, pin_b = G * Wp + 2, pout = ncols + 2;
  std::mt19937_64 rng(4321 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  std::vector<cx<T>> a((size_t)N * pin_a), b((size_t)N * pin_b, mk<T>((T)99, (T)99));
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < ncols; ++c) {
      const cx<T> z = mk<T>((T)U(rng), (T)U(rng));
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
  std::mt19937_64 rng(31 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  auto tw = build_pass_twiddles<S, T>();
  {  // PAD 1, inverse: in (nouter, n, pin) -> out (nouter, N, pout)
    typedef ColFft<S, T, COLS, true, false, false, VEC, false, 1> K;
    const int pin = ncols + 1, pout = ncols + 2;
    std::vector<cx<T>> in((size_t)nouter * n * pin), out((size_t)nouter * N * pout);
    for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
    ColParams<T> P;
    P.in = in.data(); P.out = out.data(); P.tw = tw.data();
    P.in_outer = (i64)n * pin; P.out_outer = (i64)N * pout;
    P.in_map = make_rowmap(0, pin, n, n); P.out_map = make_rowmap(0, pout, N, N);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 1; P.fold = 0;
    P.scale = (T)(1.0 / N);
    emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    long double num = 0, den = 0;
    for (int o = 0; o < nouter; ++o)
      for (int c = 0; c < ncols; ++c) {
        lvec x(N);
        for (int r = 0; r < N; ++r) { x[r].x = 0; x[r].y = 0; }
        for (int r = 0; r < h; ++r) { cx<T> z = in[(size_t)o * n * pin + (size_t)r * pin + c]; x[r].x = z.x; x[r].y = z.y; }
        for (int r = h; r < n; ++r) { cx<T> z = in[(size_t)o * n * pin + (size_t)r * pin + c]; x[N - n + r].x = z.x; x[N - n + r].y = z.y; }
        lvec X = naive_dft(x, +1);
        for (int r = 0; r < N; ++r) {
          cx<T> g = out[(size_t)o * N * pout + (size_t)r * pout + c];
          long double ex = X[r].x / N, ey = X[r].y / N;
          num += (g.x - ex) * (g.x - ex) + (g.y - ey) * (g.y - ey);
          den += ex * ex + ey * ey;
        }
      }
    char name[64];
    snprintf(name, sizeof name, "col c%d v%d pad-on-load inv", COLS, VEC);
    report(name, N, pname<T>(), (double)sqrtl(num / den), tol_of<T>());
  }
  for (int fold = 0; fold < 2; ++fold) {  // PAD 2, forward: in (nouter, N, pin) -> out (nouter, n, pout)
    typedef ColFft<S, T, COLS, false, false, false, VEC, false, 2> K;
    const int pin = ncols + 1, pout = ncols + 2;
    std::vector<cx<T>> in((size_t)nouter * N * pin), out((size_t)nouter * n * pout, mk<T>((T)55, (T)55));
    for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
    ColParams<T> P;
    P.in = in.data(); P.out = out.data(); P.tw = tw.data();
    P.in_outer = (i64)N * pin; P.out_outer = (i64)n * pout;
    P.in_map = make_rowmap(0, pin, N, N); P.out_map = make_rowmap(0, pout, n, n);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = nouter; P.remap = 0; P.fold = fold;
    P.scale = (T)0.5;
    emu_launch(P.ntile_c * nouter, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    long double num = 0, den = 0;
    for (int o = 0; o < nouter; ++o)
      for (int c = 0; c < ncols; ++c) {
        lvec x(N);
        for (int r = 0; r < N; ++r) { cx<T> z = in[(size_t)o * N * pin + (size_t)r * pin + c]; x[r].x = z.x; x[r].y = z.y; }
        lvec X = naive_dft(x, -1);
        lvec e(n);
        for (int r = 0; r < n; ++r) { e[r].x = 0; e[r].y = 0; }
        if (fold) {
          for (int r = 0; r <= h; ++r) e[r] = X[r];
          for (int r = 0; r < h; ++r) { e[h + r].x += X[N - h + r].x; e[h + r].y += X[N - h + r].y; }
        } else {
          for (int r = 0; r < h; ++r) e[r] = X[r];
          for (int r = h; r < n; ++r) e[r] = X[N - n + r];
        }
        for (int r = 0; r < n; ++r) {
          cx<T> g = out[(size_t)o * n * pout + (size_t)r * pout + c];
          long double ex = e[r].x * 0.5L, ey = e[r].y * 0.5L;
          num += (g.x - ex) * (g.x - ex) + (g.y - ey) * (g.y - ey);
          den += ex * ex + ey * ey;
        }
      }
    char name[64];
    snprintf(name, sizeof name, "col c%d v%d trunc-on-store%s", COLS, VEC, fold ? " fold" : "");
    report(name, N, pname<T>(), (double)sqrtl(num / den), tol_of<T>());
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
  std::mt19937_64 rng(77 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  std::vector<cx<T>> in((size_t)nouter * N * pin), pre(in.size()), out1(in.size(), mk<T>((T)5, (T)5)), out0(in.size(), mk<T>((T)5, (T)5));
  std::vector<unsigned char> mask(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    in[i] = mk<T>((T)U(rng), (T)U(rng));
    mask[i] = (unsigned char)((rng() % 3) != 0);
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
  long double num = 0, den = 0;
  for (int o = 0; o < nouter; ++o)
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < ncols; ++c) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        num += (out1[i].x - out0[i].x) * (out1[i].x - out0[i].x) + (out1[i].y - out0[i].y) * (out1[i].y - out0[i].y);
        den += out0[i].x * out0[i].x + out0[i].y * out0[i].y;
      }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d inv masked load", COLS, VEC);
  report(name, N, pname<T>(), (double)sqrtl(num / den), 1e-30);     // same arithmetic on the same values: identical
}

// pruned 2/3-rule pass (PAD == 4): removed rows read as zero, tiles without a kept column untouched, kept columns
// identical to the plain inverse kernel on an input whose removed rows were zeroed
template <class S, typename T, int COLS, int VEC>
static void test_col_band() {
  typedef ColFft<S, T, COLS, true, false, false, VEC, false, 4> KB;
  typedef ColFft<S, T, COLS, true, false, false, VEC> K0;
  const int N = S::N, ncols = COLS * 3 + 1, nouter = 2, pin = ncols + 1;
  if (N < 3) return;
  std::mt19937_64 rng(177 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  const cx<T> sentinel = mk<T>((T)5, (T)5);
  std::vector<cx<T>> in((size_t)nouter * N * pin), pre(in.size()), out1(in.size(), sentinel), out0(in.size(), sentinel);
  const int row_lo = N / 3 > 0 ? N / 3 : 1, row_hi = (2 * N) / 3 > row_lo ? (2 * N) / 3 : row_lo;
  for (int o = 0; o < nouter; ++o)
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < pin; ++c) {
        const size_t i = (size_t)o * N * pin + (size_t)r * pin + c;
        in[i] = mk<T>((T)U(rng), (T)U(rng));
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
  long double num = 0, den = 0;
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
        num += (out1[i].x - out0[i].x) * (out1[i].x - out0[i].x) + (out1[i].y - out0[i].y) * (out1[i].y - out0[i].y);
        den += out0[i].x * out0[i].x + out0[i].y * out0[i].y;
      }
    }
  char name[64];
  snprintf(name, sizeof name, "col c%d v%d inv pruned (kept %d, skipped %d)", COLS, VEC, kept, skipped / N);
  report(name, N, pname<T>(), bad || kept == 0 ? 1.0 : (double)sqrtl(num / (den > 0 ? den : 1)), 1e-30);
  // complete-output mode (b_gzero = 2, the pencils' first inverse pass): EVERY column is written -- kept ones as the plain
  // kernel on the row-zeroed input, columns of a removed y or z as exact zeros (per column, also inside a lane's VEC pair)
  std::vector<cx<T>> out2(in.size(), sentinel);
  P.b_gzero = 2;
  P.in = in.data(); P.out = out2.data();
  emu_launch(P.ntile_c * nouter, KB::THREADS, KB::LDS_BYTES, [&](int b, int t, char* lds) { KB::body(P, b, t, lds); });
  num = den = 0;
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
        num += (out2[i].x - want.x) * (out2[i].x - want.x) + (out2[i].y - want.y) * (out2[i].y - want.y);
        den += want.x * want.x + want.y * want.y;
      }
    }
  snprintf(name, sizeof name, "col c%d v%d inv band, complete output", COLS, VEC);
  report(name, N, pname<T>(), bad ? 1.0 : (double)sqrtl(num / (den > 0 ? den : 1)), 1e-30);
}

template <class S, bool HAS3 = (S::E % 3 == 0 && S::N >= 6)> struct PadTests {
  static void run() {}
};
template <class S> struct PadTests<S, true> {
  static void run() {
    test_col_pad<S, double, 4, 1>();
    test_col_pad<S, float, 8, 2>();
  }
};

template <class S, typename T, int ROWS, bool INV, bool TWLDS, bool SPLIT = false>
static void test_row() {
  typedef RowFft<S, T, ROWS, INV, TWLDS, false, SPLIT> K;
  const int N = S::N;
  const int nrows = ROWS * 2 + 1;
  std::mt19937_64 rng(99 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = N + 3, pout = N + 1;
  std::vector<cx<T>> in((size_t)nrows * pin), out((size_t)nrows * pout);
  for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
  auto tw = build_pass_twiddles<S, T>();
  RowParams<T> P{in.data(), out.data(), tw.data(), pin, pout, nrows, INV ? (T)(1.0 / N) : (T)1};
  emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
             [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    lvec x(N);
    for (int i = 0; i < N; ++i) { x[i].x = in[(size_t)r * pin + i].x; x[i].y = in[(size_t)r * pin + i].y; }
    lvec X = naive_dft(x, INV ? +1 : -1);
    for (int i = 0; i < N; ++i) {
      long double s = INV ? 1.0L / N : 1.0L;
      cx<T> g = out[(size_t)r * pout + i];
      num += (g.x - X[i].x * s) * (g.x - X[i].x * s) + (g.y - X[i].y * s) * (g.y - X[i].y * s);
      den += X[i].x * s * X[i].x * s + X[i].y * s * X[i].y * s;
    }
  }
  char name[64];
  snprintf(name, sizeof name, "row r%d %s%s%s", ROWS, INV ? "inv" : "fwd", TWLDS ? " twlds" : "", SPLIT ? " split" : "");
  report(name, N, pname<T>(), (double)sqrtl(num / den), tol_of<T>());
  // z-chunked side (pencil C2C): forward stores into / inverse loads out of nch equal blocks (rows_total, q)
  if (N % 4 == 0 && N >= 8) {
    const int nch = 4, q = N / nch, rows_total = nrows + 2, row0 = 1;
    const ZSplit zs = make_zsplit(q, nch, q, rows_total);
    std::vector<cx<T>> blocks((size_t)rows_total * N, mk<T>((T)3, (T)3)), out2((size_t)nrows * pout);
    typedef RowFft<S, T, ROWS, INV, TWLDS, true, SPLIT> K;
    RowParams<T> Pc{in.data(), out2.data(), tw.data(), pin, pout, nrows, INV ? (T)(1.0 / N) : (T)1, zs, row0};
    if (INV) {       // scatter the plain input rows into the blocks, transform out of them
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k < N; ++k) blocks[(size_t)(k / q) * rows_total * q + (size_t)(row0 + r) * q + k % q] = in[(size_t)r * pin + k];
      Pc.in = blocks.data();
    } else {
      Pc.out = blocks.data();
    }
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(Pc, b, t, lds); });
    long double nn = 0, dd = 0;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < N; ++k) {
        const cx<T> e = out[(size_t)r * pout + k];
        const cx<T> g = INV ? out2[(size_t)r * pout + k] : blocks[(size_t)(k / q) * rows_total * q + (size_t)(row0 + r) * q + k % q];
        nn += (g.x - e.x) * (g.x - e.x) + (g.y - e.y) * (g.y - e.y);
        dd += e.x * e.x + e.y * e.y;
      }
    snprintf(name, sizeof name, "row r%d %s z-chunked", ROWS, INV ? "inv" : "fwd");
    report(name, N, pname<T>(), (double)sqrtl(nn / dd), 1e-30 + (double)0);   // same arithmetic, other addresses: identical
  }
}

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT = false, bool MLDS = false>
static void test_real() {
  const int M = S::N, N = 2 * M;
  const int nrows = ROWS + 2;
  std::mt19937_64 rng(7 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = N + 2, pout = M + 1 + 2;
  std::vector<T> in((size_t)nrows * pin);
  std::vector<cx<T>> out((size_t)nrows * pout);
  for (auto& z : in) z = (T)U(rng);
  auto tw = build_pass_twiddles<S, T>();
  auto rtw = build_real_twiddles<T>(N);
  {
    typedef R2CFft<S, T, ROWS, TWLDS, false, false, SPLIT> K;
    RealParams<T> P{in.data(), out.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
               [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    lvec x(N);
    for (int i = 0; i < N; ++i) { x[i].x = in[(size_t)r * pin + i]; x[i].y = 0; }
    lvec X = naive_dft(x, -1);
    for (int k = 0; k <= M; ++k) {
      cx<T> g = out[(size_t)r * pout + k];
      num += (g.x - X[k].x) * (g.x - X[k].x) + (g.y - X[k].y) * (g.y - X[k].y);
      den += X[k].x * X[k].x + X[k].y * X[k].y;
    }
  }
  char name[64];
  snprintf(name, sizeof name, "r2c r%d%s%s", ROWS, TWLDS ? " twlds" : "", SPLIT ? " split" : "");
  report(name, N, pname<T>(), (double)sqrtl(num / den), tol_of<T>());
  // c2r of (the r2c result with garbage imaginary parts in bins 0 and M) must return the input
  std::vector<T> back((size_t)nrows * pin, (T)0);
  for (int r = 0; r < nrows; ++r) {
    out[(size_t)r * pout + 0].y = (T)3.5;
    out[(size_t)r * pout + M].y = (T)-2.25;
  }
  {
    typedef C2RFft<S, T, ROWS, TWLDS, false, false, SPLIT, false, MLDS> K;
    RealParams<T> P{out.data(), back.data(), tw.data(), rtw.data(), pout, pin, nrows, M + 1, (T)(1.0 / N)};
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
               [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  num = den = 0;
  for (int r = 0; r < nrows; ++r)
    for (int i = 0; i < N; ++i) {
      long double d = (long double)back[(size_t)r * pin + i] - in[(size_t)r * pin + i];
      num += d * d;
      den += (long double)in[(size_t)r * pin + i] * in[(size_t)r * pin + i];
    }
  snprintf(name, sizeof name, "c2r(r2c) r%d%s%s%s", ROWS, TWLDS ? " twlds" : "", SPLIT ? " split" : "", MLDS ? " mlds" : "");
  report(name, N, pname<T>(), (double)sqrtl(num / den), 4 * tol_of<T>());
  // 3/2-rule column handling: r2c keeps only the first `valid` bins, c2r treats the missing ones as zero
  if (M >= 4) {
    const int valid = M / 2 + 1;
    std::vector<cx<T>> part((size_t)nrows * valid, mk<T>((T)9, (T)9));
    {
      typedef R2CFft<S, T, ROWS, TWLDS, true, false, SPLIT> K;
      RealParams<T> P{in.data(), part.data(), tw.data(), rtw.data(), pin, valid, nrows, valid, (T)1};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
                 [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    long double nn = 0, dd = 0;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) {
        cx<T> g = part[(size_t)r * valid + k], e = out[(size_t)r * pout + k];
        if (k == 0) e.y = 0;        // out[] had its bin-0 imaginary part poisoned above
        nn += (g.x - e.x) * (g.x - e.x) + (g.y - e.y) * (g.y - e.y);
        dd += e.x * e.x + e.y * e.y;
      }
    snprintf(name, sizeof name, "r2c valid<M+1 r%d", ROWS);
    report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
    std::vector<T> b2((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, TWLDS, true, false, SPLIT, false, MLDS> K;
      RealParams<T> P{part.data(), b2.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
                 [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    nn = dd = 0;
    for (int r = 0; r < nrows; ++r) {
      lvec X(N);
      for (int k = 0; k < N; ++k) { X[k].x = 0; X[k].y = 0; }
      for (int k = 0; k < valid; ++k) {
        cx<T> z = part[(size_t)r * valid + k];
        X[k].x = z.x; X[k].y = (k == 0) ? 0 : z.y;
        if (k > 0) { X[N - k].x = z.x; X[N - k].y = -z.y; }
      }
      lvec x = naive_dft(X, +1);
      for (int i = 0; i < N; ++i) {
        long double e = x[i].x / N, g = b2[(size_t)r * pin + i];
        nn += (g - e) * (g - e);
        dd += e * e;
      }
    }
    snprintf(name, sizeof name, "c2r valid<M+1 r%d", ROWS);
    report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
  }
  // z-chunked complex side (fused pencil pack / unpack): the M + 1 bins of a row go to nch blocks (rows_total, len_l);
  // `drop`: the last block has no room for the Nyquist bin (the 'AlltoallN' mode), which then reads back as zero
  if (M >= 4 && M % 2 == 0) {
    for (int dp = 0; dp < 3; ++dp) {        // dp == 2: rows of the blocks further apart than their length (ZSplit pitch)
      const int drop = dp == 1;
      const int nch = 2, q = M / nch, last = q + (drop ? 0 : 1), rows_total = nrows + 3, row0 = 2;
      const int pq = dp == 2 ? q + 3 : q, plast = dp == 2 ? last + 5 : last;
      const ZSplit zs = dp == 2 ? make_zsplit(q, nch, last, rows_total, pq, plast) : make_zsplit(q, nch, last, rows_total);
      std::vector<cx<T>> blocks((size_t)rows_total * (pq * (nch - 1) + plast), mk<T>((T)7, (T)7));
      {
        typedef R2CFft<S, T, ROWS, TWLDS, false, true, SPLIT> K;
        RealParams<T> P{in.data(), blocks.data(), tw.data(), rtw.data(), pin, 0, nrows, M + 1, (T)1, zs, row0};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      long double nn = 0, dd = 0;
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k <= M - drop; ++k) {
          const int l = std::min(k / q, nch - 1), len = l == nch - 1 ? plast : pq;
          cx<T> g = blocks[(size_t)l * rows_total * pq + (size_t)(row0 + r) * len + (k - l * q)], e = out[(size_t)r * pout + k];
          if (k == 0 || k == M) e.y = 0;
          nn += (g.x - e.x) * (g.x - e.x) + (g.y - e.y) * (g.y - e.y);
          dd += e.x * e.x + e.y * e.y;
        }
      snprintf(name, sizeof name, "r2c z-chunked%s r%d", drop ? " drop" : dp == 2 ? " pitched" : "", ROWS);
      report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
      std::vector<T> b3((size_t)nrows * pin, (T)0);
      {
        typedef C2RFft<S, T, ROWS, TWLDS, false, true, SPLIT, false, MLDS> K;
        RealParams<T> P{blocks.data(), b3.data(), tw.data(), rtw.data(), 0, pin, nrows, M + 1, (T)(1.0 / N), zs, row0};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      nn = dd = 0;
      for (int r = 0; r < nrows; ++r) {
        lvec X(N);
        for (int k = 0; k < N; ++k) { X[k].x = 0; X[k].y = 0; }
        for (int k = 0; k <= M - drop; ++k) {
          const cx<T> z = out[(size_t)r * pout + k];
          X[k].x = z.x; X[k].y = (k == 0 || k == M) ? 0 : z.y;
          if (k > 0 && k < M) { X[N - k].x = z.x; X[N - k].y = -z.y; }
        }
        lvec x = naive_dft(X, +1);
        for (int i = 0; i < N; ++i) {
          long double e = x[i].x / N, g = b3[(size_t)r * pin + i];
          nn += (g - e) * (g - e);
          dd += e * e;
        }
      }
      snprintf(name, sizeof name, "c2r z-chunked%s r%d", drop ? " drop" : dp == 2 ? " pitched" : "", ROWS);
      report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
    }
  }
  // column-limited AND z-chunked (the 3/2-rule pencil transforms): only the first `valid` bins exist, split into
  // nch blocks with an uneven last one (valid = 2 * q + 1: the un-padded mesh's Nyquist column on the last rank)
  if (M >= 12 && M % 3 == 0) {
    const int valid = M / 3 * 2 / 2 * 2 + 1 <= M ? (M / 3) / 2 * 2 + 1 : 3;      // odd, about a third of the bins
    const int nch = 2, q = (valid - 1) / nch, last = q + 1, rows_total = nrows + 2, row0 = 1;
    const ZSplit zs = make_zsplit(q, nch, last, rows_total);
    std::vector<cx<T>> blocks((size_t)rows_total * (q * (nch - 1) + last), mk<T>((T)7, (T)7));
    {
      typedef R2CFft<S, T, ROWS, TWLDS, true, true, SPLIT> K;
      RealParams<T> P{in.data(), blocks.data(), tw.data(), rtw.data(), pin, 0, nrows, valid, (T)1, zs, row0};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    long double nn = 0, dd = 0;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) {
        const int l = std::min(k / q, nch - 1), len = l == nch - 1 ? last : q;
        cx<T> g = blocks[(size_t)l * rows_total * q + (size_t)(row0 + r) * len + (k - l * q)], e = out[(size_t)r * pout + k];
        if (k == 0) e.y = 0;
        nn += (g.x - e.x) * (g.x - e.x) + (g.y - e.y) * (g.y - e.y);
        dd += e.x * e.x + e.y * e.y;
      }
    snprintf(name, sizeof name, "r2c valid<M+1 z-chunked r%d", ROWS);
    report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
    std::vector<T> b4((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, TWLDS, true, true, SPLIT, false, MLDS> K;
      RealParams<T> P{blocks.data(), b4.data(), tw.data(), rtw.data(), 0, pin, nrows, valid, (T)(1.0 / N), zs, row0};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    nn = dd = 0;
    for (int r = 0; r < nrows; ++r) {
      lvec X(N);
      for (int k = 0; k < N; ++k) { X[k].x = 0; X[k].y = 0; }
      for (int k = 0; k < valid; ++k) {
        const cx<T> z = out[(size_t)r * pout + k];
        X[k].x = z.x; X[k].y = (k == 0) ? 0 : z.y;
        if (k > 0) { X[N - k].x = z.x; X[N - k].y = -z.y; }
      }
      lvec x = naive_dft(X, +1);
      for (int i = 0; i < N; ++i) {
        long double e = x[i].x / N, g = b4[(size_t)r * pin + i];
        nn += (g - e) * (g - e);
        dd += e * e;
      }
    }
    snprintf(name, sizeof name, "c2r valid<M+1 z-chunked r%d", ROWS);
    report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
  }
}

// ---------------------------------------------------------------------------
// chirp-z (Bluestein) kernels: runtime length n on the compiled plan S of length M >= 2n-1
// ---------------------------------------------------------------------------
// Pair-row kernels (R2CFft / C2RFft PAIR): the z pass of the route that splits real / complex LAST.  Forward: the x and y
// transforms of a real (n0, n1, N) field read as complex pairs go in, its half-spectrum must come out.  Inverse: an ARBITRARY
// complex (n0, n1, N/2 + 1) array goes in (not the transform of a real field: the planes kz = 0 and N/2 are not Hermitian); the
// inverse x and y transforms of what comes out, read as reals, must be numpy's irfftn of it (inverse c2c over x and y, then the
// c2r that ignores the imaginary parts of bins 0 and N/2).  Rows and planes of both sides are pitched.  yb > 0: the real side is
// blocked in y (RealPairParams::p_ymap): blocks of yb rows per x, pitched x rows inside a block, pitched blocks.
template <class S, typename T, int ROWS, bool TWLDS>
static void test_pair(int n0, int n1, int yb = 0) {
  const int M = S::N, N = 2 * M, Nf = M + 1;
  std::mt19937_64 rng(11 + N + 7 * n0 + n1);
  std::uniform_real_distribution<double> U(-1, 1);
  const int wrow = M + 1, wplane = (yb ? yb : n1) * wrow + 3, crow = Nf + 2, cplane = n1 * crow + 5;      // complex elements
  const int wblock = n0 * wplane + 5;                       // blocked: complex elements between the y blocks
  const size_t wsize = yb ? (size_t)(n1 / yb) * wblock : (size_t)n0 * wplane;
  auto woff = [&](int x, int y) { return yb ? (size_t)(y / yb) * wblock + (size_t)x * wplane + (size_t)(y % yb) * wrow
                                            : (size_t)x * wplane + (size_t)y * wrow; };
  const RowMap ymap = make_rowmap(2 * (i64)wblock, 2 * wrow, yb, n1);
  std::vector<long> wlog(wsize, -1);                        // element of W -> element of the logical (n0, n1, M) array, -1: a gap
  for (int x = 0; x < n0; ++x)
    for (int y = 0; y < n1; ++y)
      for (int k = 0; k < M; ++k) wlog[woff(x, y) + k] = ((long)x * n1 + y) * M + k;
  auto tw = build_pass_twiddles<S, T>();
  auto rtw = build_real_twiddles<T>(N);
  // the long-double transform of axis `ax` (0: x, 1: y) of an (n0, n1, len) array
  auto xy = [&](std::vector<cx<long double>>& a, int len, int ax, int sign) {
    const int n = ax == 0 ? n0 : n1;
    for (int o = 0; o < (ax == 0 ? n1 : n0); ++o)
      for (int k = 0; k < len; ++k) {
        lvec v(n);
        for (int i = 0; i < n; ++i) v[i] = a[((size_t)(ax == 0 ? i : o) * n1 + (ax == 0 ? o : i)) * len + k];
        v = naive_dft(v, sign);
        for (int i = 0; i < n; ++i) a[((size_t)(ax == 0 ? i : o) * n1 + (ax == 0 ? o : i)) * len + k] = v[i];
      }
  };
  const int slots = (n0 / 2 + 1) * n1, grid = (slots + ROWS / 2 - 1) / (ROWS / 2);
  char name[64];
  {
    std::vector<long double> u((size_t)n0 * n1 * N);
    for (auto& z : u) z = U(rng);
    std::vector<cx<long double>> w((size_t)n0 * n1 * M), ref((size_t)n0 * n1 * Nf);
    for (size_t i = 0; i < w.size(); ++i) { w[i].x = u[2 * i]; w[i].y = u[2 * i + 1]; }
    xy(w, M, 1, -1);
    xy(w, M, 0, -1);
    for (int r = 0; r < n0 * n1; ++r) {
      lvec x(N);
      for (int i = 0; i < N; ++i) { x[i].x = u[(size_t)r * N + i]; x[i].y = 0; }
      lvec X = naive_dft(x, -1);
      for (int k = 0; k < Nf; ++k) ref[(size_t)r * Nf + k] = X[k];
    }
    xy(ref, Nf, 1, -1);
    xy(ref, Nf, 0, -1);
    std::vector<cx<T>> W(wsize, mk<T>((T)9, (T)9)), fu((size_t)n0 * cplane, mk<T>((T)7, (T)7));
    for (int x = 0; x < n0; ++x)
      for (int y = 0; y < n1; ++y)
        for (int k = 0; k < M; ++k) {
          const cx<long double> z = w[((size_t)x * n1 + y) * M + k];
          W[woff(x, y) + k] = mk<T>((T)z.x, (T)z.y);
        }
    typedef R2CFft<S, T, ROWS, TWLDS, false, false, false, false, true> K;
    RealPairParams<T> P{{W.data(), fu.data(), tw.data(), rtw.data(), 2 * wrow, crow, slots, Nf, (T)1}};
    P.pn0 = n0; P.pn1 = n1; P.p_rplane = 2 * wplane; P.p_cplane = cplane; P.p_ymap = ymap;
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    long double num = 0, den = 0;
    bool gaps = true;        // nothing outside the rows is written
    for (size_t i = 0; i < fu.size(); ++i) {
      const int x = (int)(i / cplane), rem = (int)(i % cplane), y = rem / crow, k = rem % crow;
      if (y < n1 && k < Nf) {
        const cx<long double> e = ref[((size_t)x * n1 + y) * Nf + k];
        num += (fu[i].x - e.x) * (fu[i].x - e.x) + (fu[i].y - e.y) * (fu[i].y - e.y);
        den += e.x * e.x + e.y * e.y;
      } else if (fu[i].x != (T)7 || fu[i].y != (T)7) {
        gaps = false;
      }
    }
    snprintf(name, sizeof name, "r2c pair r%d %dx%d b%d%s", ROWS, n0, n1, yb, TWLDS ? " twlds" : "");
    report(name, N, pname<T>(), gaps ? (double)sqrtl(num / den) : 1.0, tol_of<T>());
  }
  {
    std::vector<cx<long double>> f((size_t)n0 * n1 * Nf);
    for (auto& z : f) { z.x = U(rng); z.y = U(rng); }
    std::vector<cx<T>> fu((size_t)n0 * cplane, mk<T>((T)7, (T)7)), W(wsize, mk<T>((T)9, (T)9));
    for (int r = 0; r < n0 * n1; ++r)
      for (int k = 0; k < Nf; ++k) {
        const cx<T> z = mk<T>((T)f[(size_t)r * Nf + k].x, (T)f[(size_t)r * Nf + k].y);
        fu[(size_t)(r / n1) * cplane + (size_t)(r % n1) * crow + k] = z;
        f[(size_t)r * Nf + k].x = z.x;
        f[(size_t)r * Nf + k].y = z.y;
      }
    // irfftn: inverse x and y, then c2r row by row
    std::vector<cx<long double>> g = f;
    xy(g, Nf, 0, +1);
    xy(g, Nf, 1, +1);
    std::vector<long double> ref((size_t)n0 * n1 * N);
    for (int r = 0; r < n0 * n1; ++r) {
      lvec X(N);
      for (int k = 0; k < Nf; ++k) X[k] = g[(size_t)r * Nf + k];
      X[0].y = 0;
      X[M].y = 0;
      for (int k = 1; k < M; ++k) { X[N - k].x = X[k].x; X[N - k].y = -X[k].y; }
      lvec x = naive_dft(X, +1);
      for (int i = 0; i < N; ++i) ref[(size_t)r * N + i] = x[i].x / ((long double)N * n0 * n1);
    }
    typedef C2RFft<S, T, ROWS, TWLDS, false, false, false, false, false, true> K;
    RealPairParams<T> P{{fu.data(), W.data(), tw.data(), rtw.data(), crow, 2 * wrow, slots, Nf, (T)(1.0 / N)}};
    P.pn0 = n0; P.pn1 = n1; P.p_rplane = 2 * wplane; P.p_cplane = cplane; P.p_ymap = ymap;
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    bool gaps = true;
    std::vector<cx<long double>> w((size_t)n0 * n1 * M);
    for (size_t i = 0; i < W.size(); ++i) {
      if (wlog[i] >= 0) { w[wlog[i]].x = W[i].x; w[wlog[i]].y = W[i].y; }
      else if (W[i].x != (T)9 || W[i].y != (T)9) gaps = false;
    }
    xy(w, M, 1, +1);
    xy(w, M, 0, +1);
    long double num = 0, den = 0;
    for (size_t i = 0; i < w.size(); ++i) {
      const long double a = w[i].x / ((long double)n0 * n1) - ref[2 * i], b = w[i].y / ((long double)n0 * n1) - ref[2 * i + 1];
      num += a * a + b * b;
      den += ref[2 * i] * ref[2 * i] + ref[2 * i + 1] * ref[2 * i + 1];
    }
    snprintf(name, sizeof name, "c2r pair r%d %dx%d b%d%s", ROWS, n0, n1, yb, TWLDS ? " twlds" : "");
    report(name, N, pname<T>(), gaps ? (double)sqrtl(num / den) : 1.0, 4 * tol_of<T>());
  }
}

template <class S, typename T, int COLS, bool INV, bool SPLIT, int VEC>
static void test_col_z(int n) {
  typedef ColFftZ<S, T, COLS, INV, SPLIT, VEC> K;
  const int ncols = COLS + 3, nouter = 2;
  std::mt19937_64 rng(4321 + n);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = ncols + 2, pout = ncols + 5;
  std::vector<cx<T>> in((size_t)nouter * n * pin), out((size_t)nouter * n * pout, mk<T>((T)777, (T)777));
  for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
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
  long double num = 0, den = 0;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c) {
      lvec x(n);
      for (int r = 0; r < n; ++r) { cx<T> z = in[(size_t)o * n * pin + (size_t)r * pin + c]; x[r].x = z.x; x[r].y = z.y; }
      lvec X = naive_dft(x, INV ? +1 : -1);
      for (int r = 0; r < n; ++r) {
        cx<T> g = out[(size_t)o * n * pout + (size_t)r * pout + c];
        long double sc = INV ? 1.0L / n : 1.0L, ex = X[r].x * sc, ey = X[r].y * sc;
        num += (g.x - ex) * (g.x - ex) + (g.y - ey) * (g.y - ey);
        den += ex * ex + ey * ey;
      }
    }
  char name[64];
  snprintf(name, sizeof name, "chirpz col M=%d c%d v%d %s%s", S::N, COLS, VEC, INV ? "inv" : "fwd", SPLIT ? " split" : "");
  report(name, n, pname<T>(), (double)sqrtl(num / den), 8 * tol_of<T>());
}

template <class S, typename T, int ROWS, bool INV>
static void test_row_z(int n) {
  typedef RowFftZ<S, T, ROWS, 0, INV> K;
  const int nrows = ROWS * 2 + 1;
  std::mt19937_64 rng(990 + n);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = n + 3, pout = n + 1;
  std::vector<cx<T>> in((size_t)nrows * pin), out((size_t)nrows * pout);
  for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(n);
  auto bh = build_chirp_filter<T>(n, S::N);
  RowParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows;
  P.scale = INV ? (T)(1.0 / n) : (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    lvec x(n);
    for (int i = 0; i < n; ++i) { x[i].x = in[(size_t)r * pin + i].x; x[i].y = in[(size_t)r * pin + i].y; }
    lvec X = naive_dft(x, INV ? +1 : -1);
    for (int i = 0; i < n; ++i) {
      long double s = INV ? 1.0L / n : 1.0L;
      cx<T> g = out[(size_t)r * pout + i];
      num += (g.x - X[i].x * s) * (g.x - X[i].x * s) + (g.y - X[i].y * s) * (g.y - X[i].y * s);
      den += X[i].x * s * X[i].x * s + X[i].y * s * X[i].y * s;
    }
  }
  char name[64];
  snprintf(name, sizeof name, "chirpz row M=%d r%d %s", S::N, ROWS, INV ? "inv" : "fwd");
  report(name, n, pname<T>(), (double)sqrtl(num / den), 8 * tol_of<T>());
}

template <class S, typename T, int ROWS>
static void test_real_z(int n) {
  const int nh = n / 2, nrows = ROWS + 2;
  std::mt19937_64 rng(70 + n);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = n + 1, pout = nh + 1 + 2;         // odd real pitch on purpose
  std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
  std::vector<cx<T>> out((size_t)nrows * pout);
  for (auto& z : in) z = (T)U(rng);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(n);
  auto bh = build_chirp_filter<T>(n, S::N);
  RealParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.rtw = nullptr; P.in_stride = pin; P.out_stride = pout;
  P.nrows = nrows; P.valid = nh + 1; P.scale = (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  {
    typedef RowFftZ<S, T, ROWS, 1, false> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    lvec x(n);
    for (int i = 0; i < n; ++i) { x[i].x = in[(size_t)r * pin + i]; x[i].y = 0; }
    lvec X = naive_dft(x, -1);
    for (int k = 0; k <= nh; ++k) {
      cx<T> g = out[(size_t)r * pout + k];
      num += (g.x - X[k].x) * (g.x - X[k].x) + (g.y - X[k].y) * (g.y - X[k].y);
      den += X[k].x * X[k].x + X[k].y * X[k].y;
    }
  }
  char name[64];
  snprintf(name, sizeof name, "chirpz r2c M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), (double)sqrtl(num / den), 8 * tol_of<T>());
  for (int r = 0; r < nrows; ++r) {                 // garbage where c2r must not look
    out[(size_t)r * pout + 0].y = (T)3.5;
    if (n % 2 == 0) out[(size_t)r * pout + nh].y = (T)-2.25;
  }
  P.in = out.data(); P.out = back.data(); P.in_stride = pout; P.out_stride = pin; P.scale = (T)(1.0 / n);
  {
    typedef RowFftZ<S, T, ROWS, 2, true> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  num = den = 0;
  for (int r = 0; r < nrows; ++r)
    for (int i = 0; i < n; ++i) {
      long double d = (long double)back[(size_t)r * pin + i] - in[(size_t)r * pin + i];
      num += d * d;
      den += (long double)in[(size_t)r * pin + i] * in[(size_t)r * pin + i];
    }
  snprintf(name, sizeof name, "chirpz c2r(r2c) M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), (double)sqrtl(num / den), 16 * tol_of<T>());
}

// half-length real chirp-z (KIND 3 / 4): even real length n = 2m, chirp-z of length m on the plan S (M >= 2m-1)
template <class S, typename T, int ROWS>
static void test_real_zh(int m) {
  const int n = 2 * m, nrows = ROWS + 2;
  std::mt19937_64 rng(170 + n);
  std::uniform_real_distribution<double> U(-1, 1);
  const int pin = n + 2, pout = m + 1 + 2;
  std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
  std::vector<cx<T>> out((size_t)nrows * pout);
  for (auto& z : in) z = (T)U(rng);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(m);
  auto bh = build_chirp_filter<T>(m, S::N);
  auto rtw = build_real_twiddles<T>(n);
  RealParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.rtw = rtw.data(); P.in_stride = pin; P.out_stride = pout;
  P.nrows = nrows; P.valid = m + 1; P.scale = (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  {
    typedef RowFftZ<S, T, ROWS, 3, false> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    lvec x(n);
    for (int i = 0; i < n; ++i) { x[i].x = in[(size_t)r * pin + i]; x[i].y = 0; }
    lvec X = naive_dft(x, -1);
    for (int k = 0; k <= m; ++k) {
      cx<T> g = out[(size_t)r * pout + k];
      num += (g.x - X[k].x) * (g.x - X[k].x) + (g.y - X[k].y) * (g.y - X[k].y);
      den += X[k].x * X[k].x + X[k].y * X[k].y;
    }
  }
  char name[64];
  snprintf(name, sizeof name, "chirpz/2 r2c M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), (double)sqrtl(num / den), 8 * tol_of<T>());
  for (int r = 0; r < nrows; ++r) {
    out[(size_t)r * pout + 0].y = (T)3.5;
    out[(size_t)r * pout + m].y = (T)-2.25;
  }
  P.in = out.data(); P.out = back.data(); P.in_stride = pout; P.out_stride = pin; P.scale = (T)(1.0 / n);
  {
    typedef RowFftZ<S, T, ROWS, 4, true> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  num = den = 0;
  for (int r = 0; r < nrows; ++r)
    for (int i = 0; i < n; ++i) {
      long double d = (long double)back[(size_t)r * pin + i] - in[(size_t)r * pin + i];
      num += d * d;
      den += (long double)in[(size_t)r * pin + i] * in[(size_t)r * pin + i];
    }
  snprintf(name, sizeof name, "chirpz/2 c2r(r2c) M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), (double)sqrtl(num / den), 16 * tol_of<T>());
}

// wave-packed c2r (fft_kernels.h C2RFft WP): plain, column-limited and z-chunked, against the input of the r2c kernels
template <class S, typename T, int WAVES, bool SPLIT>
static void test_c2r_wave_packed() {
  if constexpr (S::TPT < 64 && 64 % S::TPT != 0 && S::E % 2 == 0) {      // (register pairing: even E -- registry.h wave_packable)
    constexpr int RPW = 64 / S::TPT, ROWS = WAVES * RPW;
    const int M = S::N, N = 2 * M, nrows = 2 * ROWS + 1;       // the last workgroup is ragged, its last wave too
    std::mt19937_64 rng(99 + N);
    std::uniform_real_distribution<double> U(-1, 1);
    const int pin = N + 2, pout = M + 1 + 2;
    std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
    std::vector<cx<T>> out((size_t)nrows * pout);
    for (auto& z : in) z = (T)U(rng);
    auto tw = build_pass_twiddles<S, T>();
    auto rtw = build_real_twiddles<T>(N);
    {
      typedef R2CFft<S, T, 2, false, false, false, false> K;
      RealParams<T> P{in.data(), out.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
      emu_launch((nrows + 1) / 2, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    char name[64];
    {     // r2c, wave-packed, against the dense kernel's output (and, column-limited, its first bins)
      std::vector<cx<T>> o2((size_t)nrows * pout, mk<T>((T)7, (T)7)), o3((size_t)nrows * (M / 2 + 1), mk<T>((T)7, (T)7));
      {
        typedef R2CFft<S, T, ROWS, false, false, false, SPLIT, true> K;
        static_assert(K::THREADS == WAVES * 64, "whole waves");
        RealParams<T> P{in.data(), o2.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      {
        typedef R2CFft<S, T, ROWS, false, true, false, SPLIT, true> K;
        RealParams<T> P{in.data(), o3.data(), tw.data(), rtw.data(), pin, M / 2 + 1, nrows, M / 2 + 1, (T)1};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      long double nn = 0, dd = 0, n3 = 0;
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k <= M; ++k) {
          const cx<T> a = o2[(size_t)r * pout + k], e = out[(size_t)r * pout + k];
          nn += (long double)(a.x - e.x) * (a.x - e.x) + (long double)(a.y - e.y) * (a.y - e.y);
          dd += (long double)e.x * e.x + (long double)e.y * e.y;
          if (k <= M / 2) {
            const cx<T> c = o3[(size_t)r * (M / 2 + 1) + k];
            n3 += (long double)(c.x - e.x) * (c.x - e.x) + (long double)(c.y - e.y) * (c.y - e.y);
          }
        }
      snprintf(name, sizeof name, "r2c wave-packed w%d%s", WAVES, SPLIT ? " split" : "");
      report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
      snprintf(name, sizeof name, "r2c wave-packed valid<M+1 w%d", WAVES);
      report(name, N, pname<T>(), (double)sqrtl(n3 / dd), 4 * tol_of<T>());
    }
    for (int r = 0; r < nrows; ++r) { out[(size_t)r * pout].y = (T)3.5; out[(size_t)r * pout + M].y = (T)-2.25; }
    {
      typedef C2RFft<S, T, ROWS, false, false, false, SPLIT, true> K;
      static_assert(K::THREADS == WAVES * 64, "whole waves");
      RealParams<T> P{out.data(), back.data(), tw.data(), rtw.data(), pout, pin, nrows, M + 1, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    long double num = 0, den = 0;
    for (int r = 0; r < nrows; ++r)
      for (int i = 0; i < N; ++i) {
        long double d = (long double)back[(size_t)r * pin + i] - in[(size_t)r * pin + i];
        num += d * d;
        den += (long double)in[(size_t)r * pin + i] * in[(size_t)r * pin + i];
      }
    snprintf(name, sizeof name, "c2r wave-packed w%d%s", WAVES, SPLIT ? " split" : "");
    report(name, N, pname<T>(), (double)sqrtl(num / den), 4 * tol_of<T>());
    // column-limited: bins >= valid read as zero
    const int valid = M / 2 + 1;
    std::vector<cx<T>> part((size_t)nrows * valid);
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) part[(size_t)r * valid + k] = out[(size_t)r * pout + k];
    std::vector<T> b1((size_t)nrows * pin, (T)0), b2((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, false, true, false, SPLIT, true> K;
      RealParams<T> P{part.data(), b1.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    {
      typedef C2RFft<S, T, 2, false, true, false, false, false> K;      // the unpacked kernel as the reference
      RealParams<T> P{part.data(), b2.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + 1) / 2, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    num = den = 0;
    for (size_t i = 0; i < b1.size(); ++i) { long double d = (long double)b1[i] - b2[i]; num += d * d; den += (long double)b2[i] * b2[i]; }
    snprintf(name, sizeof name, "c2r wave-packed valid<M+1 w%d", WAVES);
    report(name, N, pname<T>(), (double)sqrtl(num / den), 4 * tol_of<T>());
  }
}

// N = 3 L as three sub-transforms (fft_col3.h): plain forward / inverse (in place and out of place, two-level row maps on
// both sides, ragged last column tile), pad-on-load inverse and truncate-on-store forward with the Nyquist fold, against the
// long-double DFT of the logical data.
template <class SL, typename T, int COLS, int SPLIT, int VEC>
static void test_col3() {
  constexpr int L = SL::N, N = 3 * L;
  const int ncols = COLS + COLS / 2 + 1, nouter = 2;         // one full and one ragged tile per outer batch
  const int pitch = ncols + 3;
  std::mt19937_64 rng(4242 + N);
  std::uniform_real_distribution<double> U(-1, 1);
  auto tw = build_col3_twiddles<SL, T>();
  char name[96];
  for (int inv = 0; inv < 2; ++inv) {
    for (int inplace = 0; inplace < 2; ++inplace) {
      // rows through a two-level map: row r -> (r / split) * hi + (r % split) * lo
      const int split = N / 4, lo = pitch, hi = split * pitch + 5 * pitch;
      const size_t outer_stride = (size_t)4 * hi + 7;
      std::vector<cx<T>> in(outer_stride * nouter), out(outer_stride * nouter, mk<T>((T)7, (T)7));
      for (auto& z : in) z = mk<T>((T)U(rng), (T)U(rng));
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
      long double num = 0, den = 0;
      for (int o = 0; o < nouter; ++o)
        for (int cc = 0; cc < ncols; cc += 3) {
          lvec x(N);
          for (int r = 0; r < N; ++r) {
            const cx<T> z = src[o * outer_stride + (size_t)(r / split) * hi + (size_t)(r % split) * lo + cc];
            x[r].x = z.x; x[r].y = z.y;
          }
          lvec X = naive_dft(x, inv ? +1 : -1);
          for (int r = 0; r < N; ++r) {
            const cx<T> g = res[o * outer_stride + (size_t)(r / split) * hi + (size_t)(r % split) * lo + cc];
            const long double s = inv ? 1.0L / N : 1.0L;
            num += (g.x - X[r].x * s) * (g.x - X[r].x * s) + (g.y - X[r].y * s) * (g.y - X[r].y * s);
            den += X[r].x * s * X[r].x * s + X[r].y * s * X[r].y * s;
          }
        }
      snprintf(name, sizeof name, "col3 c%d v%d %s%s%s", COLS, VEC, inv ? "inv" : "fwd", inplace ? " in place" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), (double)sqrtl(num / den), 2 * tol_of<T>());
    }
  }
  // 3/2-rule: inverse with the zero band on input (2L physical rows), forward with the truncated output + Nyquist fold
  {
    const int n = 2 * L;
    std::vector<cx<T>> phys((size_t)n * pitch), big((size_t)N * pitch, mk<T>((T)7, (T)7)), back((size_t)n * pitch, mk<T>((T)7, (T)7));
    for (auto& z : phys) z = mk<T>((T)U(rng), (T)U(rng));
    ColParams<T> P;
    memset(&P, 0, sizeof P);
    P.in = phys.data(); P.out = big.data(); P.tw = tw.data();
    P.in_map = make_rowmap(0, pitch, 0, n); P.out_map = make_rowmap(0, pitch, 0, N);
    P.ncols = ncols; P.ntile_c = (ncols + COLS - 1) / COLS; P.nouter = 1; P.remap = 0; P.scale = (T)1;
    {
      typedef ColFft3<SL, T, COLS, true, true, SPLIT, VEC, false, 1> K;
      emu_launch(P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    long double num = 0, den = 0;
    for (int cc = 0; cc < ncols; cc += 2) {
      lvec x(N);
      for (int r = 0; r < N; ++r) { x[r].x = 0; x[r].y = 0; }
      for (int r = 0; r < L; ++r) {
        x[r].x = phys[(size_t)r * pitch + cc].x; x[r].y = phys[(size_t)r * pitch + cc].y;
        x[2 * L + r].x = phys[(size_t)(L + r) * pitch + cc].x; x[2 * L + r].y = phys[(size_t)(L + r) * pitch + cc].y;
      }
      lvec X = naive_dft(x, +1);
      for (int r = 0; r < N; ++r) {
        const cx<T> g = big[(size_t)r * pitch + cc];
        num += (g.x - X[r].x) * (g.x - X[r].x) + (g.y - X[r].y) * (g.y - X[r].y);
        den += X[r].x * X[r].x + X[r].y * X[r].y;
      }
    }
    snprintf(name, sizeof name, "col3 c%d v%d pad-on-load inv%s", COLS, VEC, SPLIT ? " split" : "");
    report(name, N, pname<T>(), (double)sqrtl(num / den), 2 * tol_of<T>());
    // the same with one third of a tile's transform per workgroup (ColFft3S): three times the workgroups, XCD-aware order
    // and plain order, against the kernel above (same arithmetic up to the order of the radix-3 step's sums)
    for (int remap = 0; remap < 2; ++remap) {
      std::vector<cx<T>> big2((size_t)N * pitch, mk<T>((T)7, (T)7));
      P.out = big2.data(); P.remap = remap;
      typedef ColFft3S<SL, T, COLS, true, true, SPLIT, VEC, false, 1> K;
      emu_launch(3 * P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      num = den = 0;
      for (int r = 0; r < N; ++r)
        for (int cc = 0; cc < pitch; ++cc) {
          const cx<T> g = big2[(size_t)r * pitch + cc], w0 = big[(size_t)r * pitch + cc];
          num += (long double)(g.x - w0.x) * (g.x - w0.x) + (long double)(g.y - w0.y) * (g.y - w0.y);
          den += (long double)w0.x * w0.x + (long double)w0.y * w0.y;
        }
      snprintf(name, sizeof name, "col3s c%d v%d pad-on-load inv, a third per workgroup%s%s", COLS, VEC, remap ? " remap" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), (double)sqrtl(num / den), 2 * tol_of<T>());
    }
    P.out = big.data(); P.remap = 0;
    for (int fold = 0; fold < 2; ++fold) {
      std::vector<cx<T>> full((size_t)N * pitch);
      for (auto& z : full) z = mk<T>((T)U(rng), (T)U(rng));
      P.in = full.data(); P.out = back.data(); P.in_map = make_rowmap(0, pitch, 0, N); P.out_map = make_rowmap(0, pitch, 0, n);
      P.fold = fold; P.scale = (T)0.5;
      {
        typedef ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 2> K;
        emu_launch(P.ntile_c, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      num = den = 0;
      for (int cc = 0; cc < ncols; cc += 2) {
        lvec x(N);
        for (int r = 0; r < N; ++r) { x[r].x = full[(size_t)r * pitch + cc].x; x[r].y = full[(size_t)r * pitch + cc].y; }
        lvec X = naive_dft(x, -1);
        for (int r = 0; r < n; ++r) {
          cx<long double> want = r < L ? X[r] : X[L + r];                  // physical row L + i = logical row 2L + i
          if (fold && r == L) { want.x += X[L].x; want.y += X[L].y; }
          const cx<T> g = back[(size_t)r * pitch + cc];
          num += (g.x - 0.5L * want.x) * (g.x - 0.5L * want.x) + (g.y - 0.5L * want.y) * (g.y - 0.5L * want.y);
          den += 0.25L * (want.x * want.x + want.y * want.y);
        }
      }
      snprintf(name, sizeof name, "col3 c%d v%d truncate-on-store fwd%s%s", COLS, VEC, fold ? " fold" : "", SPLIT ? " split" : "");
      report(name, N, pname<T>(), (double)sqrtl(num / den), 2 * tol_of<T>());
    }
    snprintf(name, sizeof name, "col3 c%d v%d truncate-on-store fwd, wrapped input columns%s", COLS, VEC, SPLIT ? " split" : "");
    test_wrapped_columns<ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 2>, T>(name, N, n, tw.data(), COLS);
    snprintf(name, sizeof name, "col3 c%d v%d plain fwd, wrapped input columns%s", COLS, VEC, SPLIT ? " split" : "");
    test_wrapped_columns<ColFft3<SL, T, COLS, false, false, SPLIT, VEC, false, 0>, T>(name, N, N, tw.data(), COLS);
  }
}

// ---------------------------------------------------------------------------
// The long-double reference the tests of the fused nonlinear z stage (fft_nlz.h) share.
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
// row r (pitch pin) of each of nf stored fields
template <typename T> static std::vector<lreal> nl_real_rows(const std::vector<cx<T>>* keep, int nf, int r, int pin, int vin, int M) {
  std::vector<lreal> re(nf);
  for (int f = 0; f < nf; ++f) re[f] = nl_real_row(keep[f].data() + (size_t)r * pin, vin, M);
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
template <typename T> static void nl_accumulate(const cx<T>* g, const lvec& X, int valid, long double& num, long double& den) {
  for (int q = 0; q < valid; ++q) {
    const long double d = (g[q].x - X[q].x) * (g[q].x - X[q].x) + (g[q].y - X[q].y) * (g[q].y - X[q].y);
    num += d == d ? d : 1;                         // (a NaN must not vanish in the comparison with the tolerance)
    den += X[q].x * X[q].x + X[q].y * X[q].y;
  }
}
// nothing is stored beyond the valid bins of a result row g: bins [valid, pout) hold what they held -- the bins of `was`, the row
// of the input the result lies over, or (null) the 7s the tests fill their own result rows with
template <typename T> static void nl_tail_kept(const cx<T>* g, const cx<T>* was, int valid, int pout, long double& num) {
  for (int q = valid; q < pout; ++q) {
    const cx<T> w = was ? was[q] : mk<T>((T)7, (T)7);
    if (g[q].x != w.x || g[q].y != w.y) num += 1;
  }
}
// the inputs are preserved, but for those a result lies over (over[0..nres): the field, or -1)
template <typename T> static void nl_inputs_kept(const std::vector<cx<T>>* in, const std::vector<cx<T>>* keep, int nf, const int* over, int nres, long double& num) {
  for (int f = 0; f < nf; ++f) {
    bool taken = false;
    for (int c = 0; c < nres; ++c) taken = taken || over[c] == f;
    if (!taken && memcmp(in[f].data(), keep[f].data(), keep[f].size() * sizeof(cx<T>)) != 0) num += 1;
  }
}

// fused nonlinear z stage (fft_nlz.h): out_f = rfft((irfft(a) x irfft(b))_f), rows of `valid` bins, against long-double DFTs
template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT, bool WAVE = false>
static void test_nlz(int valid, bool inplace, int valid_in = 0) {      // valid_in: fewer input bins than stored ones (pruned 2/3-rule)
  typedef NlzFft<S, T, ROWS, TWLDS, SPLIT, WAVE> K;
  const int vin = valid_in > 0 ? valid_in : valid;
  const int M = S::N;
  const int nrows = 2 * ROWS + 3;                 // an odd count: the last pair has one row
  const int pin = valid + 2, pout = inplace ? pin : valid + 1;
  std::mt19937_64 rng(4242 + M + valid);
  std::uniform_real_distribution<double> U(-1, 1);
  std::vector<cx<T>> in[6], out[3];
  for (auto& f : in) {
    f.resize((size_t)nrows * pin);
    for (auto& z : f) z = mk<T>((T)U(rng), (T)U(rng));
  }
  std::vector<cx<T>> keep[6];
  for (int f = 0; f < 6; ++f) keep[f] = in[f];
  for (auto& f : out) f.assign((size_t)nrows * pout, mk<T>((T)7, (T)7));
  auto tw = build_pass_twiddles<S, T>();
  NlzParams<T> P;
  for (int f = 0; f < 3; ++f) { P.a[f] = in[f].data(); P.b[f] = in[3 + f].data(); P.out[f] = inplace ? in[f].data() : out[f].data(); }
  P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
  P.scale = (T)(1.0 / ((double)M * (double)M));
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = nl_real_rows(keep, 6, r, pin, vin, M);
    for (int c = 0; c < 3; ++c) {
      const cx<T>* g = (inplace ? in[c].data() : out[c].data()) + (size_t)r * pout;
      nl_accumulate(g, nl_cross_spectrum(&re[0], &re[3], c), valid, num, den);
      if (!inplace) nl_tail_kept<T>(g, nullptr, valid, pout, num);
    }
  }
  char name[64];
  snprintf(name, sizeof name, "nlz r%d v%d/%d%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "", inplace ? " inpl" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), (double)sqrtl(num / den), sizeof(T) == 8 ? 4e-14 : 2e-5);
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
  std::mt19937_64 rng(2424 + M + valid);
  std::uniform_real_distribution<double> U(-1, 1);
  std::vector<cx<T>> in[6], out;
  for (auto& f : in) {
    f.resize((size_t)nrows * pin);
    for (auto& z : f) z = mk<T>((T)U(rng), (T)U(rng));
  }
  std::vector<cx<T>> keep[6];
  for (int f = 0; f < 6; ++f) keep[f] = in[f];
  out.assign((size_t)nrows * pout, mk<T>((T)7, (T)7));
  const int af = alias == 1 ? 0 : alias == 2 ? 4 : -1;      // the input field the result lies over
  auto tw = build_pass_twiddles<S, T>();
  NlzParams<T> P;
  for (int f = 0; f < 3; ++f) { P.a[f] = in[f].data(); P.b[f] = in[3 + f].data(); P.out[f] = nullptr; }
  P.out[0] = af >= 0 ? in[af].data() : out.data();
  P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
  P.scale = (T)(1.0 / ((double)M * (double)M));
  P.rt3 = nullptr;
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = nl_real_rows(keep, 6, r, pin, vin, M);
    const cx<T>* g = P.out[0] + (size_t)r * pout;
    nl_accumulate(g, nl_dot_spectrum(&re[0], &re[3]), valid, num, den);
    nl_tail_kept<T>(g, af >= 0 ? keep[af].data() + (size_t)r * pin : nullptr, valid, pout, num);
  }
  nl_inputs_kept(in, keep, 6, &af, 1, num);
  char name[72];
  snprintf(name, sizeof name, "nld r%d v%d/%d%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "",
           alias == 1 ? " over a0" : alias == 2 ? " over b1" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), (double)sqrtl(num / den), sizeof(T) == 8 ? 4e-14 : 2e-5);
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
  std::mt19937_64 rng(4224 + M + valid);
  std::uniform_real_distribution<double> U(-1, 1);
  const T nan = std::numeric_limits<T>::quiet_NaN();
  std::vector<cx<T>> in[9], out[4];               // a, b, c
  for (auto& f : in) {
    f.resize((size_t)(nrows + extra) * pin);
    for (auto& z : f) z = mk<T>((T)U(rng), (T)U(rng));
    for (size_t i = (size_t)nrows * pin; i < f.size(); ++i) f[i] = mk<T>(nan, nan);
  }
  std::vector<cx<T>> keep[9];
  for (int f = 0; f < 9; ++f) keep[f] = in[f];
  for (auto& f : out) {
    f.assign((size_t)(nrows + extra) * pout, mk<T>((T)7, (T)7));
    for (size_t i = (size_t)nrows * pout; i < f.size(); ++i) f[i] = mk<T>(nan, nan);
  }
  // the input field each result lies over (-1: none)
  int over[4] = {-1, -1, -1, -1};
  if (alias == 1) { over[0] = 0; over[1] = 1; over[2] = 2; over[3] = 8; }
  if (alias == 2) { over[0] = 3; over[1] = 4; over[2] = 5; over[3] = 6; }
  auto tw = build_pass_twiddles<S, T>();
  NlcParams<T> P;
  for (int f = 0; f < 3; ++f) { P.a[f] = in[f].data(); P.b[f] = in[3 + f].data(); P.c[f] = in[6 + f].data(); }
  cx<T>* res[4];
  for (int c = 0; c < 4; ++c) res[c] = over[c] >= 0 ? in[over[c]].data() : out[c].data();
  for (int f = 0; f < 3; ++f) P.out[f] = res[f];
  P.outs = res[3];
  P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
  P.scale = (T)(1.0 / ((double)M * (double)M));
  P.rt3 = nullptr;
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = nl_real_rows(keep, 9, r, pin, vin, M);
    for (int c = 0; c < 4; ++c) {
      const cx<T>* g = res[c] + (size_t)r * pout;
      nl_accumulate(g, c < 3 ? nl_cross_spectrum(&re[0], &re[3], c) : nl_dot_spectrum(&re[0], &re[6]), valid, num, den);
      nl_tail_kept<T>(g, over[c] >= 0 ? keep[over[c]].data() + (size_t)r * pin : nullptr, valid, pout, num);
    }
  }
  for (int c = 0; c < 4; ++c)                      // ... nor behind the last row
    for (size_t i = (size_t)nrows * pout; i < (size_t)(nrows + extra) * pout; ++i)
      if (res[c][i].x == res[c][i].x || res[c][i].y == res[c][i].y) num += 1;
  nl_inputs_kept(in, keep, 9, over, 4, num);
  char name[80];
  snprintf(name, sizeof name, "nlc r%d v%d/%d%s%s%s%s%s", ROWS, vin, valid, TWLDS ? " twlds" : "", SPLIT ? " split" : "",
           alias == 1 ? " inpl a c2" : alias == 2 ? " inpl b c0" : "", poison ? " poison" : "", WAVE ? " wave" : "");
  report(name, M, pname<T>(), (double)sqrtl(num / den), sizeof(T) == 8 ? 4e-14 : 2e-5);
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
  std::mt19937_64 rng(777 + M + valid + 31 * c.spike_pos + 7 * c.spike_field);
  const double amp = c.spike_field >= 0 ? 1e-3 : 1.0;
  std::uniform_real_distribution<double> U(-amp, amp);
  std::vector<cx<T>> in[6], out0[3], out1[3];
  for (auto& f : in) {
    f.resize((size_t)nrows * pin);
    for (auto& z : f) z = mk<T>((T)U(rng), (T)U(rng));
  }
  if (c.spike_field >= 0) {
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int q = 0; q < vin; ++q) {
      const long double a = -two_pi * (long double)(((long long)q * c.spike_pos) % M) / M;
      cx<T>& z = in[c.spike_field][(size_t)c.spike_row * pin + q];
      z = mk<T>(z.x + (T)cosl(a), z.y + (T)sinl(a));
    }
  }
  if (c.nan_field >= 0) in[c.nan_field][(size_t)(nrows / 2) * pin + 1].x = (T)NAN;
  for (int f = 0; f < 3; ++f) { out0[f].assign((size_t)nrows * pout, mk<T>((T)7, (T)7)); out1[f] = out0[f]; }
  auto tw = build_pass_twiddles<S, T>();
  const int grid = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  NlmParams<T> P;
  for (int f = 0; f < 3; ++f) { P.a[f] = in[f].data(); P.b[f] = in[3 + f].data(); P.out[f] = f < nout ? out0[f].data() : nullptr; }
  P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
  P.scale = (T)(1.0 / ((double)M * (double)M));
  P.rt3 = nullptr; P.part = nullptr;
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

// The stage that ends in a reduction (fft_nlz.h body_moments, Op::Moments): [min, max, S1 .. S4] of up to six real fields over all
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
  std::mt19937_64 rng(4242 + M + valid + 13 * nf + nrows);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::vector<cx<T>> in[6];
  for (int f = 0; f < nf; ++f) {
    in[f].resize((size_t)nrows * pin);
    for (auto& z : in[f]) z = mk<T>((T)U(rng), (T)U(rng));
    for (int r = 0; r < nrows; ++r) in[f][(size_t)r * pin].x += (T)(0.5 * M * (f + 1));      // a mean of (f + 1) / 2
  }
  if (c.bad_field >= 0) in[c.bad_field][(size_t)(nrows / 2) * pin + 1].x = c.inf ? (T)INFINITY : (T)NAN;
  auto tw = build_pass_twiddles<S, T>();
  const int units = (nrows + 2 * ROWS - 1) / (2 * ROWS);
  const int grid = std::min(units, c.ngroups);
  NlsParams<T> P;
  int slot_of[6];
  for (int p = 0; p < 3; ++p) { P.a[p] = nullptr; P.b[p] = nullptr; P.out[p] = nullptr; }
  for (int i = 0; i < 6; ++i) P.center[i] = 0.0;
  for (int f = 0; f < nf; ++f) {
    const int slot = two ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
    (slot % 2 ? P.b : P.a)[slot / 2] = in[f].data();
    P.center[slot] = c.center ? 0.5 * (f + 1) + 0.125 : 0.0;
    slot_of[f] = slot;
  }
  P.tw = tw.data(); P.in_stride = pin; P.out_stride = 0; P.nrows = nrows; P.valid = valid; P.valid_in = vin;
  P.scale = (T)1; P.rt3 = nullptr;
  P.norm = 1.0 / (double)M; P.npairs = (nf + 1) / 2; P.ngroups = grid;
  std::vector<double> part((size_t)grid * K::WAVES * NLS_SLOTS, -7.0);
  P.part = part.data();
  std::vector<cx<T>> keep[6];
  for (int f = 0; f < nf; ++f) keep[f] = in[f];
  emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  double bad = 0;
  for (int f = 0; f < nf; ++f)                       // the inputs are preserved (NaNs: compare the bytes)
    if (memcmp(in[f].data(), keep[f].data(), keep[f].size() * sizeof(cx<T>)) != 0) bad = 1e30;
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
  std::mt19937_64 rng(777 + M);
  std::uniform_real_distribution<double> U(-1, 1);
  std::vector<cx<T>> in[6], out[3], keep[6];
  for (auto& f : in) {
    f.resize((size_t)nrows * pin);
    for (auto& z : f) z = mk<T>((T)U(rng), (T)U(rng));
  }
  for (int f = 0; f < 6; ++f) keep[f] = in[f];
  for (auto& f : out) f.assign((size_t)nrows * pout, mk<T>((T)7, (T)7));
  auto tw = build_pass_twiddles<SL, T>();
  auto rt = build_nlz3_twiddles<T>(L);
  NlzParams<T> P;
  for (int f = 0; f < 3; ++f) { P.a[f] = in[f].data(); P.b[f] = in[3 + f].data(); P.out[f] = inplace ? in[f].data() : out[f].data(); }
  P.tw = tw.data(); P.rt3 = rt.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows; P.valid = valid;
  P.scale = (T)(1.0 / ((double)M * (double)M));
  emu_launch((nrows + 2 * ROWS - 1) / (2 * ROWS), K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  long double num = 0, den = 0;
  for (int r = 0; r < nrows; ++r) {
    const std::vector<lreal> re = nl_real_rows(keep, 6, r, pin, valid, M);      // (L + 1 bins of 3 L points: bin 0 alone is its own conjugate)
    for (int c = 0; c < 3; ++c) {
      const cx<T>* g = (inplace ? in[c].data() : out[c].data()) + (size_t)r * pout;
      nl_accumulate(g, nl_cross_spectrum(&re[0], &re[3], c), valid, num, den);
      if (!inplace) nl_tail_kept<T>(g, nullptr, valid, pout, num);
    }
  }
  char name[64];
  snprintf(name, sizeof name, "nlz3 r%d%s%s", ROWS, TWLDS ? " twlds" : "", inplace ? " inpl" : "");
  report(name, M, pname<T>(), (double)sqrtl(num / den), sizeof(T) == 8 ? 4e-14 : 2e-5);
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

template <class S> static void test_chirpz_all() {
  const int nmax = (S::N + 1) / 2;
  for (int n : {nmax, nmax - 1, (S::N / 4) + 1, 7}) {
    if (n < 2 || 2 * n - 1 > S::N) continue;
    test_col_z<S, double, 4, false, false, 1>(n);
    test_col_z<S, double, 4, true, true, 1>(n);
    test_col_z<S, float, 8, false, false, 2>(n);
    test_col_z<S, float, 8, true, true, 2>(n);
    test_row_z<S, double, 2, false>(n);
    test_row_z<S, float, 3, true>(n);
    test_real_z<S, double, 2>(n);
    test_real_z<S, float, 3>(n);
    test_real_zh<S, double, 2>(n);
    test_real_zh<S, float, 3>(n);
  }
}

template <class S> static void test_spec_all() {
  test_col<S, double, 4, false, true>(false);
  test_col<S, double, 4, true, false>(true);
  test_col<S, float, 8, false, false>(true);
  test_col<S, float, 8, true, true>(false);
  test_col<S, double, 8, false, true, true>(true);
  test_col<S, float, 4, true, false, true>(false);
  test_col<S, float, 8, false, true, false, 2>(true);
  test_col<S, float, 8, true, false, true, 2>(false);
  test_col<S, float, 16, false, false, false, 4>(true);
  if constexpr (S::E % 2 == 0 && S::NP > 1) {        // the four-round exchange (fft_kernels.h XchQuarterV)
    test_col<S, double, 8, false, false, 2>(true);
    test_col<S, double, 4, true, true, 2>(false);
    test_col<S, float, 8, true, false, 2, 2>(true);
  }
  test_row<S, double, 2, false, true>();
  test_row<S, double, 2, true, false>();
  test_row<S, float, 3, false, false>();
  test_real<S, double, 2, true>();
  test_real<S, float, 3, false>();
  test_col_mask<S, double, 4, 1>();
  test_col_mask<S, float, 8, 2>();
  test_col_band<S, double, 4, 1>();
  test_col_band<S, float, 8, 2>();
  if constexpr (S::NP > 1 && (S::E >= 12 || S::N == 64)) {   // split re/im exchange of the contiguous-axis kernels (registry.h row_split)
    test_row<S, double, 2, false, false, true>();
    test_row<S, double, 2, true, false, true>();
    test_real<S, double, 2, false, true>();
  }
  if constexpr (S::NP > 1 && !(S::TPT <= 64 && 64 % S::TPT == 0)) {      // mirrors through LDS (C2RFft MLDS): the plans no shuffle serves
    test_real<S, double, 2, false, false, true>();
    test_real<S, float, 3, true, false, true>();
    if constexpr (S::E >= 12) test_real<S, double, 2, false, true, true>();
  }
  PadTests<S>::run();
  test_c2r_wave_packed<S, double, 1, false>();
  test_c2r_wave_packed<S, float, 2, false>();
  if constexpr (S::NP > 1 && S::E >= 12) test_c2r_wave_packed<S, double, 2, true>();
}

// The plan list is split over EMU_PART = 0..5 so that the parts compile (and run) in parallel;
// without EMU_PART everything goes into one binary.
#ifndef EMU_PART
#define EMU_PART -1
#endif
#define EMU_HAS(p) (EMU_PART < 0 || EMU_PART == (p))

int main() {
#if EMU_HAS(0)
  {  // validate the fast reference against the plain O(N^2) sum
    for (int n : {12, 40, 96, 250}) {
      lvec x(n);
      for (int i = 0; i < n; ++i) { x[i].x = sinl(1.0L + i * i); x[i].y = cosl(3.0L * i + 0.5L); }
      lvec a = naive_dft(x, -1), b = naive_dft_slow(x, -1);
      long double d = 0, r = 0;
      for (int i = 0; i < n; ++i) { d += (a[i].x - b[i].x) * (a[i].x - b[i].x) + (a[i].y - b[i].y) * (a[i].y - b[i].y); r += b[i].x * b[i].x + b[i].y * b[i].y; }
      report("reference self-check", n, "ldbl", (double)sqrtl(d / r), 1e-17);
    }
  }
#endif
  // every plan in plans.h is exercised
#define MFFT_PLAN(N, ...) test_spec_all<Spec<N, __VA_ARGS__>>();
#if EMU_HAS(0)
  MFFT_PLANS_A(MFFT_PLAN)
  test_chirpz_all<Spec<16, 16>>();
  test_chirpz_all<Spec<64, 8, 8>>();
  test_chirpz_all<Spec<96, 8, 4, 3>>();
  test_chirpz_all<Spec<512, 8, 8, 8>>();
  test_chirpz_all<Spec<160, 4, 4, 5, 2>>();
#endif
#if EMU_HAS(1)
  MFFT_PLANS_B(MFFT_PLAN) MFFT_PLANS_C(MFFT_PLAN) MFFT_COLPLANS_F32_C(MFFT_PLAN) MFFT_COLPLANS_F64_B(MFFT_PLAN)
#endif
#if EMU_HAS(2)
  MFFT_PLANS_D(MFFT_PLAN) MFFT_PLANS_E(MFFT_PLAN) MFFT_COLPLANS_F64_E(MFFT_PLAN)
  // three sub-transforms per workgroup: small stand-ins for every code path, then the shipped plans
  test_col3<Spec<16, 4, 4>, double, 4, 0, 1>();
  test_col3<Spec<16, 4, 4>, float, 8, 1, 2>();
  test_col3<Spec<32, 8, 4>, double, 2, 1, 1>();
#define MFFT_COL3(N, L, ...) test_col3<Spec<L, __VA_ARGS__>, double, 4, 0, 1>(); test_col3<Spec<L, __VA_ARGS__>, float, 4, 1, 2>();
  MFFT_COL3PLANS_E(MFFT_COL3)
#undef MFFT_COL3
#endif
#if EMU_HAS(3)
  MFFT_PLANS_F(MFFT_PLAN) MFFT_PLANS_G(MFFT_PLAN)
#endif
#if EMU_HAS(4)
  MFFT_PLANS_H(MFFT_PLAN) MFFT_PLANS_I(MFFT_PLAN) MFFT_PLANS_J(MFFT_PLAN) MFFT_COLPLANS_F64_I(MFFT_PLAN)
#endif
#if EMU_HAS(6)
  MFFT_PLANS_K(MFFT_PLAN)
#endif
#if EMU_HAS(7)
  MFFT_PLANS_L(MFFT_PLAN)
#endif
#if EMU_HAS(8)
  MFFT_PLANS_M(MFFT_PLAN)
  MFFT_COLPLANS_F64_M(MFFT_PLAN)
#endif
#if EMU_HAS(9)
  MFFT_PLANS_N(MFFT_PLAN)
  MFFT_PLANS_Q(MFFT_PLAN)      // round 5: 4608 ... 7168
#endif
#if EMU_HAS(10)
  MFFT_PLANS_O(MFFT_PLAN)
  MFFT_PLANS_R(MFFT_PLAN)      // round 5: 21 * 2^a, radix 42
#endif
#if EMU_HAS(13)
  MFFT_PLANS_S(MFFT_PLAN)      // round 6: 35 * 2^a, radix 70 (shipped in single precision)
#endif
#if EMU_HAS(14)
  MFFT_PLANS_T(MFFT_PLAN)      // round 6: 27 * 2^a, the 3/2-rule images of the 9 * 2^a meshes
#endif
#if EMU_HAS(15)
  MFFT_PLANS_U(MFFT_PLAN)      // round 6: 135 * 2^a, 1350 / 2700 / 2250, 675 / 1125
#endif
#if EMU_HAS(16)
  MFFT_PLANS_V(MFFT_PLAN)      // round 6: 81 * 2^a
#endif
#if EMU_HAS(17)
  MFFT_PLANS_W(MFFT_PLAN)      // round 6: 63 * 2^a
#endif
#if EMU_HAS(11)
  MFFT_PLANS_P(MFFT_PLAN)
  test_chirpz_all<Spec<8192, 32, 16, 16>>();
#endif
#if EMU_HAS(5)
  MFFT_FOR_EACH_ROWPLAN(MFFT_PLAN) MFFT_ROWPLANS_F64_K(MFFT_PLAN)
#endif
#if EMU_HAS(12)
#define MFFT_NLZ(N, ...) test_nlz_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZPLANS_P2(MFFT_NLZ) MFFT_NLZPLANS_3(MFFT_NLZ) MFFT_NLZPLANS_9(MFFT_NLZ)     // round 6: the fused nonlinear z stage
#undef MFFT_NLZ
#define MFFT_NLZ3(N, ...) test_nlz3_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZ3PLANS(MFFT_NLZ3)
  test_nlz3_all<Spec<256, 8, 8, 4>>();
#undef MFFT_NLZ3
#endif
#if EMU_HAS(18)      // (a binary of its own, `make emu_nld`: tests/test_cabi.py fixes the number of the emu_test_* parts)
#define MFFT_NLD(N, ...) test_nld_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZPLANS_P2(MFFT_NLD) MFFT_NLZPLANS_3(MFFT_NLD) MFFT_NLZPLANS_9(MFFT_NLD)     // the fused nonlinear z stage, dot product
#undef MFFT_NLD
#endif
#if EMU_HAS(19)      // (`make emu_nlm`, a binary of its own as well)
#define MFFT_NLM(N, ...) test_nlm_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZPLANS_P2(MFFT_NLM) MFFT_NLZPLANS_3(MFFT_NLM) MFFT_NLZPLANS_9(MFFT_NLM)     // the fused nonlinear z stage with the real-space maxima
#undef MFFT_NLM
#endif
#if EMU_HAS(20)      // (`make emu_nlc`, a binary of its own as well)
#define MFFT_NLC(N, ...) test_nlc_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZPLANS_P2(MFFT_NLC) MFFT_NLZPLANS_3(MFFT_NLC) MFFT_NLZPLANS_9(MFFT_NLC)     // the fused nonlinear z stage, cross and dot product
#undef MFFT_NLC
#endif
#if EMU_HAS(21)      // (`make emu_nls`, a binary of its own as well)
#define MFFT_NLS(N, ...) test_nls_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZPLANS_P2(MFFT_NLS) MFFT_NLZPLANS_3(MFFT_NLS) MFFT_NLZPLANS_9(MFFT_NLS)     // the fused z stage that ends in a reduction
#undef MFFT_NLS
#endif
#if EMU_HAS(1)
  // pair-row kernels (with plan group B, where the shipped 512 / 1024 plans are; tests/test_cabi.py fixes the number of parts): even and odd meshes (self-paired planes and rows), a partial last workgroup, the shipped shapes
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6);
  test_pair<Spec<32, 8, 4>, double, 4, true>(3, 5);
  test_pair<Spec<32, 8, 4>, double, 4, false>(5, 4);
  test_pair<Spec<32, 8, 4>, double, 2, true>(2, 2);
  test_pair<Spec<32, 8, 4>, double, 64, true>(9, 15);
  test_pair<Spec<32, 8, 4>, float, 8, true>(6, 3);
  test_pair<Spec<128, 16, 8>, double, 32, true>(12, 20);
  test_pair<Spec<512, 8, 8, 8>, double, 4, true>(3, 4);
  test_pair<Spec<1024, 16, 8, 8>, double, 2, false>(2, 3);
  // the real side blocked in y: partner rows in another block, ky = n1 / 2 on a block start and inside one, one row per block
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6, 3);
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6, 2);
  test_pair<Spec<32, 8, 4>, double, 64, true>(9, 15, 5);
  test_pair<Spec<32, 8, 4>, double, 4, false>(5, 4, 1);
  test_pair<Spec<128, 16, 8>, double, 32, true>(12, 20, 4);
#endif
#undef MFFT_PLAN
  printf("%s (%d failures)\n", g_fail ? "EMU TESTS FAILED" : "EMU TESTS PASSED", g_fail);
  return g_fail ? 1 : 0;
}
