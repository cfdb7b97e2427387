// emulator group nlh: the fused z stage that ends in a histogram (NlzHist::body)
#include "test_nlh.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlh_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
