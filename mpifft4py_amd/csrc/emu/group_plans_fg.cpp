// emulator group plans_fg: plan groups F and G
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_F(EMU_PLAN) MFFT_PLANS_G(EMU_PLAN)
}
