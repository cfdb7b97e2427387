// plan_cases.h -- what the emulator runs for one radix plan: every strided and contiguous-axis kernel family on it
// (test_spec_all) and the chirp-z kernels on it (test_chirpz_all).  A group lists plans as  MFFT_PLANS_A(EMU_PLAN)
#pragma once
#include "test_col.h"
#include "test_row.h"
#include "plans.h"

#define EMU_PLAN(N, ...) test_spec_all<Spec<N, __VA_ARGS__>>();

template <class S, bool HAS3 = (S::E % 3 == 0 && S::N >= 6)> struct PadTests {
  static void run() {}
};
template <class S> struct PadTests<S, true> {
  static void run() {
    test_col_pad<S, double, 4, 1>();
    test_col_pad<S, float, 8, 2>();
  }
};

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
