// One instantiation of the speculative sampler per object file (-DSPEC_K=.. -DSPEC_G=..), so that the instantiations compile in
// parallel (each takes 20-60 s; in one translation unit the library took five minutes).  The host API in mchap_hip.hip reaches
// them through the object's descriptor (sampler_objects.hpp); nothing here is part of the C ABI.
#include "denovo_spec_kernel.hpp"
#include "sampler_inst.hpp"

namespace {

#ifdef SPEC_PIPE
// the phased form (kernel 5) of this instantiation: its own object file, its own copy of the constant tables; with
// -DMCHAP_SPEC_VAR=1 / 2 the "side by side" / "deep" variants (denovo_spec_kernel.hpp; "specs" / "specd" objects)
#if MCHAP_SPEC_VAR == 1
#define SPEC_KIND specs
#define SPEC_VARIANT mchap::VAR_SBS
#elif MCHAP_SPEC_VAR == 2
#define SPEC_KIND specd
#define SPEC_VARIANT mchap::VAR_DEEP
#else
#define SPEC_KIND specp
#define SPEC_VARIANT mchap::VAR_PHASED
#endif
int launch(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_spec_kernel<SPEC_K, SPEC_G, true>, dim3(grid), dim3(64), lds, stream, *P);
}
#if SPEC_G == 64
// ... with decision contexts per genotype (denovo_spec_kernel<.., CTX = true>): the launches over handed-back chains
int launch_c(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_spec_kernel<SPEC_K, SPEC_G, true, MCHAP_SPEC_VAR, false, true>, dim3(grid), dim3(64), lds, stream, *P);
}
#define SPEC_LAUNCH_C launch_c
#else
#define SPEC_LAUNCH_C nullptr
#endif
#define SPEC_LAUNCH_TW nullptr
#else
#define SPEC_KIND spec
#define SPEC_VARIANT mchap::VAR_SPEC
int launch(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_spec_kernel<SPEC_K, SPEC_G>, dim3(grid), dim3(64), lds, stream, *P);
}
#define SPEC_LAUNCH_C nullptr
#if SPEC_G == 64
// one wavefront per replica of a temperature ladder (denovo_spec_kernel<.., TW = true>): a workgroup of n_temps wavefronts per chain
int launch_tw(const mchap::SimtParams *P, unsigned grid, size_t lds, hipStream_t stream) {
  return mchap::sampler_launch(mchap::denovo_spec_kernel<SPEC_K, SPEC_G, false, MCHAP_SPEC_VAR, true>, dim3(grid), dim3(64 * P->d.n_temps), lds, stream, *P);
}
#define SPEC_LAUNCH_TW launch_tw
#else
#define SPEC_LAUNCH_TW nullptr
#endif
#endif  // SPEC_PIPE

}  // namespace

SAMPLER_DESCRIPTOR(mchap::SpecInst, SAMPLER_OBJ(SPEC_KIND, SPEC_K, SPEC_G),
                   SPEC_VARIANT, SPEC_K, SPEC_G, mchap::sampler_init, launch, SPEC_LAUNCH_C, SPEC_LAUNCH_TW, SAMPLER_STATS)
