// emulator group plans_de_col3: plan groups D and E with their column override, and three sub-transforms per workgroup (fft_col3.h)
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_D(EMU_PLAN) MFFT_PLANS_E(EMU_PLAN) MFFT_COLPLANS_F64_E(EMU_PLAN)
  // three sub-transforms per workgroup: small stand-ins for every code path, then the shipped plans
  test_col3<Spec<16, 4, 4>, double, 4, 0, 1>();
  test_col3<Spec<16, 4, 4>, float, 8, 1, 2>();
  test_col3<Spec<32, 8, 4>, double, 2, 1, 1>();
#define EMU_COL3(N, L, ...) test_col3<Spec<L, __VA_ARGS__>, double, 4, 0, 1>(); test_col3<Spec<L, __VA_ARGS__>, float, 4, 1, 2>();
  MFFT_COL3PLANS_E(EMU_COL3)
}
