// emulator group plans_s: plan group S: 35 * 2^a, radix 70 (shipped in single precision)
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_S(EMU_PLAN)
}
