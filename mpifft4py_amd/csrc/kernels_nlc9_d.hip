// gfx950 instantiations: fused nonlinear z stage with the cross AND the dot product (fft_nlz.h body_cross_dot), double precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLC(N, ...) mfft::register_nlc<mfft::Spec<N, __VA_ARGS__>, double>("nlc n" #N "(" #__VA_ARGS__ ")double");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_9(MFFT_REG_NLC) });
}
