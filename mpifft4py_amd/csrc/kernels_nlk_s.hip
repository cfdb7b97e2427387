// gfx950 instantiations: fused nonlinear z stage that ends in increment histograms along z (nlz_incr_hist.h NlzIncrHist), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLK(N, ...) mfft::register_nlk<mfft::Spec<N, __VA_ARGS__>, float>("nlk n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_P2(MFFT_REG_NLK) MFFT_NLZPLANS_3(MFFT_REG_NLK) });
}
