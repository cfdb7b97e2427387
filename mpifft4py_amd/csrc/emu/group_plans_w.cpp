// emulator group plans_w: plan group W: 63 * 2^a
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_W(EMU_PLAN)
}
