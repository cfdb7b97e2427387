// emulator group plans_u: plan group U: 135 * 2^a, 1350 / 2700 / 2250, 675 / 1125
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_U(EMU_PLAN)
}
