// emulator group plans_m: plan group M with its column override
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_M(EMU_PLAN)
  MFFT_COLPLANS_F64_M(EMU_PLAN)
}
