// emulator group nls: the fused z stage that ends in a reduction (NlzMoments::body)
#include "test_nlz.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nls_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
