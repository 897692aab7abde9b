// One instantiation of the lanes-over-chains sampler per object file (-DSIMT_K=0/2/4/6/8); see spec_inst.hip.
#include "denovo_simt_kernel.hpp"
#include "sampler_inst.hpp"

// -DSIMT_WIDE (with -DSIMT_K=0): haplotype words of 128 bits -- the general fallback for targets wider than 64 bits of sampled
// alleles per haplotype (object simt_w.o, descriptor <0, 128>)
#ifdef SIMT_WIDE
#define SIMT_BITS 128
#define SIMT_KERNEL mchap::denovo_simt_kernel<0, mchap::u128>
#else
#define SIMT_BITS 64
#define SIMT_KERNEL mchap::denovo_simt_kernel<SIMT_K>
#endif

static int launch(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(SIMT_KERNEL, dim3(grid), dim3(64), lds, stream, *P);
}

SAMPLER_DESCRIPTOR(mchap::SpecInst, SAMPLER_OBJ(simt, SIMT_K, SIMT_BITS),
                   mchap::VAR_SIMT, SIMT_K, SIMT_BITS, mchap::sampler_init, launch, nullptr, nullptr, nullptr)
