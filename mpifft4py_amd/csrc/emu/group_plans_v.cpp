// emulator group plans_v: plan group V: 81 * 2^a
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_V(EMU_PLAN)
}
