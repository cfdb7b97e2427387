// emulator group nlm: the fused nonlinear z stage with the real-space maxima (NlzAbsMax)
#include "test_nlz.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlm_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
