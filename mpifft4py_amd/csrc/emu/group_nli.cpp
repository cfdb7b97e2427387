// emulator group nli: the fused z stage that ends in structure functions along z (NlzIncr::body)
#include "test_incr.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nli_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
