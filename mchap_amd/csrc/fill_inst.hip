// One ploidy of the table-completion kernel (denovo_fill_kernel.hpp) per object file (-DFILL_K=..), compiled in parallel with
// the other sampler objects; see spec_inst.hip.
#include "denovo_fill_kernel.hpp"
#include "sampler_inst.hpp"

static int launch(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_fill_kernel<FILL_K>, dim3(grid), dim3(64), lds, stream, *P);
}

SAMPLER_DESCRIPTOR(mchap::SpecInst, SAMPLER_OBJ(fill, FILL_K, 64),
                   mchap::VAR_FILL, FILL_K, 64, mchap::sampler_init, launch, nullptr, nullptr, SAMPLER_STATS)
