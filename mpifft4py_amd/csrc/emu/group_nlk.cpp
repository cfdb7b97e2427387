// emulator group nlk: the fused z stage that ends in increment histograms along z (NlzIncrHist::body)
#include "test_nlk.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlk_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
