// emu.h -- host-side workgroup emulator for the kernel bodies of fft_kernels.h, fft_chirpz.h, fft_col3.h, fft_nlz.h and nlz_*.h
// (TEST INFRASTRUCTURE, built with g++, never part of the product library).  Each GPU thread of a workgroup is a ucontext
// fibre; MFFT_BARRIER() yields to a round-robin scheduler, so the very same body code that hipcc compiles for gfx950 runs
// here with real barrier semantics and a real shared "LDS" buffer.  The tests (test_col.h, test_row.h, test_nlz.h) check
// every kernel family and radix plan against an O(N^2) long-double DFT, so index/twiddle mistakes are found without a GPU.
// One group_<name>.cpp per binary: it includes what it tests and defines emu_group(); main() is at the end of this file.
//
//   make -j8 emu && for g in $(make -s emu_list); do build/emu_$g; done
#pragma once
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
#include "twiddle.h"

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

// Relative L2 error of what a kernel stored against what it should have stored: sum |got - want|^2 over sum |want|^2, in long
// double and in the order of the calls.  The differences are taken in the operands' own type (T against T stays in T).
struct RelL2 {
  long double num = 0, den = 0;
  template <typename G, typename W> void add(const cx<G>& g, const cx<W>& w) {
    num += (g.x - w.x) * (g.x - w.x) + (g.y - w.y) * (g.y - w.y);
    den += w.x * w.x + w.y * w.y;
  }
  void add(long double g, long double w) { num += (g - w) * (g - w); den += w * w; }
  double value() const { return (double)sqrtl(num / den); }
};
static cx<long double> scaled(const cx<long double>& z, long double s) { return {z.x * s, z.y * s}; }
template <typename T> static cx<long double> to_l(const cx<T>& z) { return {z.x, z.y}; }

// n elements at a stride (a column; a row with stride 1) of a stored array, or n reals, as the input of the long-double reference
template <typename T> static lvec l_vec(const cx<T>* a, int n, size_t stride = 1) {
  lvec x(n);
  for (int i = 0; i < n; ++i) x[i] = to_l(a[i * stride]);
  return x;
}
template <typename T> static lvec l_real_vec(const T* a, int n) {
  lvec x(n);
  for (int i = 0; i < n; ++i) { x[i].x = a[i]; x[i].y = 0; }
  return x;
}

// uniform(-amp, amp) draws from one seed; a complex element takes two, as the arguments of one call (the reported errors
// depend on the order of the draws: fill field by field, in the order the tests always have)
struct Uniform {
  std::mt19937_64 rng;
  std::uniform_real_distribution<double> U;
  explicit Uniform(unsigned long long seed, double amp = 1.0) : rng(seed), U(-amp, amp) {}
  double operator()() { return U(rng); }
  template <typename T> cx<T> pair() { return mk<T>((T)U(rng), (T)U(rng)); }
  template <typename T> void fill(std::vector<cx<T>>& v) { for (auto& z : v) z = pair<T>(); }
  template <typename T> void fill(std::vector<T>& v) { for (auto& z : v) z = (T)U(rng); }
};

// every binary runs the cases of one group (group_<name>.cpp)
static void emu_group();
int main() {
  emu_group();
  printf("%s (%d failures)\n", g_fail ? "EMU TESTS FAILED" : "EMU TESTS PASSED", g_fail);
  return g_fail ? 1 : 0;
}
