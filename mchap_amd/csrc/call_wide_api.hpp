// Entry points of call_wide_inst.hip -- the `mchap call` sampler over many known haplotypes (call_wide_kernel.hpp), an object of its
// own so that it compiles beside call_api.hip, which calls them.  Not part of the C ABI: hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mchap {
struct CallParams;
}

#pragma GCC visibility push(hidden)
extern "C" {
int mchap_call_wide_max_haps(void);
// bytes of a unit's tables in the workspace (a multiple of 256)
int64_t mchap_call_wide_unit_bytes(int n_reads, int n_haps, int ploidy);
// chains of a unit per workgroup: as many as the LDS holds of their option arrays (`forced` >= 1: at most that many)
int mchap_call_wide_wg_chains(int n_haps, int chains, int forced);
// the setup launch (the units' tables) and the sampler; unit_tab: n_units x mchap_call_wide_unit_bytes of the workspace.  Returns
// a hipError_t.
int mchap_call_wide_launch(const mchap::CallParams *P, double *unit_tab, int wgc, hipStream_t stream);
}
#pragma GCC visibility pop
