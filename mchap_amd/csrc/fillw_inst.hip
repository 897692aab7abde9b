// One ploidy of the table-completion kernel (denovo_fillw_kernel.hpp: workgroup per chain, wavefront per request) per object
// file (-DFILLW_K=..), compiled in parallel with the other sampler objects; see spec_inst.hip.
#include "denovo_fillw_kernel.hpp"
#include "sampler_inst.hpp"

// (lds: fillw_lds_bytes; wide != 0: genotypes of more than 64 bits, keyed by their changed words)
static int launch(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  const bool wide = (P->fill_kw & 1) != 0, deep = (P->fill_kw & 2) != 0;
  auto ks = wide ? (deep ? mchap::denovo_fillw_kernel<FILLW_K, true, true> : mchap::denovo_fillw_kernel<FILLW_K, true, false>)
                 : (deep ? mchap::denovo_fillw_kernel<FILLW_K, false, true> : mchap::denovo_fillw_kernel<FILLW_K, false, false>);
  return mchap::sampler_launch(ks, dim3(grid), dim3(mchap::FILLW_NT), lds, stream, *P);
}

SAMPLER_DESCRIPTOR(mchap::SpecInst, SAMPLER_OBJ(fillw, FILLW_K, 64),
                   mchap::VAR_FILLW, FILLW_K, 64, mchap::sampler_init, launch, nullptr, nullptr, nullptr)
