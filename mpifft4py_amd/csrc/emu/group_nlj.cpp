// emulator group nlj: the fused z stage that ends in a joint histogram (NlzJoint::body)
#include "test_nlj.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlj_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
