// gfx950 instantiations: fused nonlinear z stage that ends in the statistics of a quadratic form (nlz_quad.h NlzQuad), double precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLQ(N, ...) mfft::register_nlq<mfft::Spec<N, __VA_ARGS__>, double>("nlq n" #N "(" #__VA_ARGS__ ")double");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_9(MFFT_REG_NLQ) });
}
