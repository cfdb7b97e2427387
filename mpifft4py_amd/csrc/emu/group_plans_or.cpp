// emulator group plans_or: plan groups O and R (21 * 2^a, radix 42)
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_O(EMU_PLAN)
  MFFT_PLANS_R(EMU_PLAN)
}
