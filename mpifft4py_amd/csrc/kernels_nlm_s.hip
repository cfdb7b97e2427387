// gfx950 instantiations: fused nonlinear z stage that also emits the real-space maxima (fft_nlz.h NlzAbsMax), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLM(N, ...) mfft::register_nlm<mfft::Spec<N, __VA_ARGS__>, float>("nlm n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLM) MFFT_NLZPLANS_3(MFFT_REG_NLM) });
}
