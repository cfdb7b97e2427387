// gfx950 instantiations: fused nonlinear z stage that ends in a joint histogram (nlz_joint.h NlzJoint), double precision
#include "registry_nlz.h"
#include "plans.h"
namespace {
#define MFFT_REG_NLJ(N, ...) mfft::register_nlj<mfft::Spec<N, __VA_ARGS__>, double>("nlj n" #N "(" #__VA_ARGS__ ")double");
mfft::PlanRegistrar registrar([] { MFFT_NLZPLANS_9(MFFT_REG_NLJ) });
}
