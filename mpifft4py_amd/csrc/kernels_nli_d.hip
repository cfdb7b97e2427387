// gfx950 instantiations: fused nonlinear z stage that ends in structure functions along z (nlz_incr.h NlzIncr), double precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLI(N, ...) mfft::register_nli<mfft::Spec<N, __VA_ARGS__>, double>("nli n" #N "(" #__VA_ARGS__ ")double");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLI) MFFT_NLZPLANS_3(MFFT_REG_NLI) });
}
