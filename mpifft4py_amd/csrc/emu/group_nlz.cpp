// emulator group nlz: the fused nonlinear z stage, cross product, and its 3/2-rule flavour
#include "test_nlz.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlz_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
#define EMU_NLZ3(N, ...) test_nlz3_all<Spec<N, __VA_ARGS__>>();
  MFFT_NLZ3PLANS(EMU_NLZ3)
  test_nlz3_all<Spec<256, 8, 8, 4>>();
}
