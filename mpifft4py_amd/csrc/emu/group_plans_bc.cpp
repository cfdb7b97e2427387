// emulator group plans_bc: plan groups B and C with their column overrides, and the pair-row kernels (the shipped 512 / 1024 plans are in B)
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_B(EMU_PLAN) MFFT_PLANS_C(EMU_PLAN) MFFT_COLPLANS_F32_C(EMU_PLAN) MFFT_COLPLANS_F64_B(EMU_PLAN)
  // pair-row kernels: even and odd meshes (self-paired planes and rows), a partial last workgroup, the shipped shapes
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
}
