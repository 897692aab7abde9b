// One instantiation of the wave-per-chain sampler (kernel 1) per object file (-DV1_RPL=1/2/4/8/16); see spec_inst.hip.
#include "denovo_mcmc_kernel.hpp"
#include "sampler_inst.hpp"

static int launch(const mchap::DenovoParams *P, unsigned gx, unsigned gy, unsigned block, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_mcmc_kernel<V1_RPL>, dim3(gx, gy), dim3(block), lds, stream, *P);
}

SAMPLER_DESCRIPTOR(mchap::V1Inst, V1_OBJ(V1_RPL), V1_RPL, mchap::sampler_init, launch)
