// emulator group plans_hij: plan groups H, I and J with the column override of I
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_H(EMU_PLAN) MFFT_PLANS_I(EMU_PLAN) MFFT_PLANS_J(EMU_PLAN) MFFT_COLPLANS_F64_I(EMU_PLAN)
}
