// The coasting kernel of the phased sampler (denovo_coast_kernel.hpp) in its own object file.  The host API in
// mchap_hip.hip calls the entry point below (declared in sampler_objects.hpp); it is not part of the C ABI.
#include "denovo_coast_kernel.hpp"
#include "sampler_inst.hpp"

// wide != 0: a list of handed-back chains (few): COAST_NW_LIST wavefronts per chain, as many steps per sweep
extern "C" __attribute__((visibility("hidden"))) int mchap_coast_launch(const mchap::SimtParams *P, unsigned grid, int wide,
                                                                        hipStream_t stream) {
  const size_t lds = mchap::coast_lds_bytes(P->max_pos);
  if (wide)
    return mchap::sampler_launch(mchap::denovo_coast_kernel<mchap::COAST_NW_LIST>, dim3(grid < 1024u ? grid : 1024u),
                                 dim3(64 * mchap::COAST_NW_LIST), lds, stream, *P);
  return mchap::sampler_launch(mchap::denovo_coast_kernel<1>, dim3(grid), dim3(64), lds, stream, *P);
}
