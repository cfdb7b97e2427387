// emulator group plans_l: plan group L
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_L(EMU_PLAN)
}
