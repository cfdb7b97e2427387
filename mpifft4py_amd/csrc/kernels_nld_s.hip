// gfx950 instantiations: fused nonlinear z stage with the dot product (fft_nlz.h body_dot), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLD(N, ...) mfft::register_nld<mfft::Spec<N, __VA_ARGS__>, float>("nld n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLD) MFFT_NLZPLANS_3(MFFT_REG_NLD) });
}
