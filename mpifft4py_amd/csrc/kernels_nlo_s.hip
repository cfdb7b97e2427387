// gfx950 instantiations: fused nonlinear z stage with the outer product a_i b_j (fft_nlz.h body_outer), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLO(N, ...) mfft::register_nlo<mfft::Spec<N, __VA_ARGS__>, float>("nlo n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLO) MFFT_NLZPLANS_3(MFFT_REG_NLO) });
}
