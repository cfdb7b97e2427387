// emulator group nlq: the fused z stage that ends in the statistics of a quadratic form (NlzQuad::body)
#include "test_nlq.h"

static void emu_group() {
  test_nlq_rule();
#define EMU_CASE(N, ...) test_nlq_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
