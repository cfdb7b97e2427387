// emulator group plans_p: plan group P and the chirp-z kernels on the 8192 plan
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_P(EMU_PLAN)
  test_chirpz_all<Spec<8192, 32, 16, 16>>();
}
