// gfx950 instantiations: fused nonlinear z stage that ends in a joint histogram (nlz_joint.h NlzJoint), single precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLJ(N, ...) mfft::register_nlj<mfft::Spec<N, __VA_ARGS__>, float>("nlj n" #N "(" #__VA_ARGS__ ")float");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_9(MFFT_REG_NLJ) });
}
