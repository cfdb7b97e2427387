// emulator group plans_t: plan group T: 27 * 2^a, the 3/2-rule images of the 9 * 2^a meshes
#include "plan_cases.h"

static void emu_group() {
  MFFT_PLANS_T(EMU_PLAN)
}
