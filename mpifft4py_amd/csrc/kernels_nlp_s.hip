// gfx950 instantiations: fused nonlinear z stage that ends in plane-averaged profiles along z (nlz_prof.h NlzProf), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLP(N, ...) mfft::register_nlp<mfft::Spec<N, __VA_ARGS__>, float>("nlp n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLP) MFFT_NLZPLANS_3(MFFT_REG_NLP) });
}
