// emulator group plans_a: the long-double reference against itself, plan group A, the chirp-z kernels on small plans
#include "plan_cases.h"

static void emu_group() {
  for (int n : {12, 40, 96, 250}) {      // validate the fast reference against the plain O(N^2) sum
    lvec x(n);
    for (int i = 0; i < n; ++i) { x[i].x = sinl(1.0L + i * i); x[i].y = cosl(3.0L * i + 0.5L); }
    lvec a = naive_dft(x, -1), b = naive_dft_slow(x, -1);
    RelL2 err;
    for (int i = 0; i < n; ++i) err.add(a[i], b[i]);
    report("reference self-check", n, "ldbl", err.value(), 1e-17);
  }
  MFFT_PLANS_A(EMU_PLAN)
  test_chirpz_all<Spec<16, 16>>();
  test_chirpz_all<Spec<64, 8, 8>>();
  test_chirpz_all<Spec<96, 8, 4, 3>>();
  test_chirpz_all<Spec<512, 8, 8, 8>>();
  test_chirpz_all<Spec<160, 4, 4, 5, 2>>();
}
