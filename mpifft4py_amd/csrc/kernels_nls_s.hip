// gfx950 instantiations: fused nonlinear z stage that ends in a reduction (nlz_moments.h NlzMoments), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLS(N, ...) mfft::register_nls<mfft::Spec<N, __VA_ARGS__>, float>("nls n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLS) MFFT_NLZPLANS_3(MFFT_REG_NLS) });
}
