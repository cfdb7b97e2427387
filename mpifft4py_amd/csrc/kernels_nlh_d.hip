// gfx950 instantiations: fused nonlinear z stage that ends in a histogram (nlz_hist.h NlzHist), double precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLH(N, ...) mfft::register_nlh<mfft::Spec<N, __VA_ARGS__>, double>("nlh n" #N "(" #__VA_ARGS__ ")double");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLH) MFFT_NLZPLANS_3(MFFT_REG_NLH) });
}
