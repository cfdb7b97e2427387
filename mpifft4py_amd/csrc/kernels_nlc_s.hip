// gfx950 instantiations: fused nonlinear z stage with the cross AND the dot product (fft_nlz.h body_cross_dot), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLC(N, ...) mfft::register_nlc<mfft::Spec<N, __VA_ARGS__>, float>("nlc n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLC) MFFT_NLZPLANS_3(MFFT_REG_NLC) });
}
