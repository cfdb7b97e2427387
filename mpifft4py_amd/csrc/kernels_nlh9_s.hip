// gfx950 instantiations: fused nonlinear z stage that ends in a histogram (nlz_hist.h NlzHist), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLH(N, ...) mfft::register_nlh<mfft::Spec<N, __VA_ARGS__>, float>("nlh n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_9(MFFT_REG_NLH) });
}
