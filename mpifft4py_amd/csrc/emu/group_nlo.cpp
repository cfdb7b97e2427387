// emulator group nlo: the fused nonlinear z stage, outer product (body_outer)
#include "test_nlo.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlo_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
