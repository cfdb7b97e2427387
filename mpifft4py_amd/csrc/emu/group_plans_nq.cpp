// emulator group plans_nq: plan groups N and Q (4608 ... 7168)
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_N(EMU_PLAN)
  MFFT_PLANS_Q(EMU_PLAN)
}
