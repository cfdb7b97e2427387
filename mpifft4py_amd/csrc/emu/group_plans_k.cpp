// emulator group plans_k: plan group K
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_K(EMU_PLAN)
}
