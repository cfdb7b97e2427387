// emulator group rowplans: the plans of the contiguous-axis kernels alone
#include "plan_cases.h"

static void emu_group() {
  MFFT_FOR_EACH_ROWPLAN(EMU_PLAN) MFFT_ROWPLANS_F64_K(EMU_PLAN)
}
