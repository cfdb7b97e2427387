// emulator group nlp: the fused z stage that ends in plane-averaged profiles along z (NlzProf::body)
#include "test_nlp.h"

static void emu_group() {
#define EMU_CASE(N, ...) test_nlp_all<Spec<N, __VA_ARGS__>>();
  EMU_NLZ_PLANS(EMU_CASE)
}
