// gfx950 instantiations: fused nonlinear z stage that ends in the statistics of a quadratic form (nlz_quad.h NlzQuad), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLQ(N, ...) mfft::register_nlq<mfft::Spec<N, __VA_ARGS__>, float>("nlq n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLQ) MFFT_NLZPLANS_3(MFFT_REG_NLQ) });
}
