// The `mchap call` sampler over many known haplotypes (call_wide_kernel.hpp) in its own object file.  The host API in call_api.hip
// calls the entry points below (call_wide_api.hpp); they are not part of the C ABI.  (The plain kernels of the headers this object
// shares with others -- exact_mode_kernel and exact_freq_kernel, launched by exact_api.hip, and call_coast_kernel, launched by
// call_api.hip -- are `static`: every object that includes their header compiles a copy of its own, and the copies do not clash.)
#include <hip/hip_runtime.h>

#include "../../include/mchap_hip.h"
#include "call_wide_api.hpp"
#include "call_wide_kernel.hpp"

extern "C" {

int mchap_call_wide_max_haps(void) { return mchap::CALL_WIDE_MAX_HAPS; }

// bytes of a unit's tables in the workspace (a multiple of 256)
int64_t mchap_call_wide_unit_bytes(int n_reads, int n_haps, int ploidy) {
  return (int64_t)mchap::call_wide_unit_doubles(n_reads, n_haps, ploidy) * 8;
}

// chains of a unit per workgroup: as many as the LDS holds of their option arrays (MCHAP_HIP_CALL_WIDE_CHAINS, tests: fewer)
int mchap_call_wide_wg_chains(int n_haps, int chains, int forced) {
  int wgc = chains < mchap::CALL_WG_CHAINS ? chains : mchap::CALL_WG_CHAINS;
  while (wgc > 1 && mchap::call_wide_lds_bytes(n_haps, wgc) > mchap::CALL_WIDE_LDS) wgc--;
  if (forced >= 1 && forced < wgc) wgc = forced;
  return wgc;
}

// the setup launch (the units' tables) and the sampler; unit_tab: n_units x mchap_call_wide_unit_bytes of the workspace
int mchap_call_wide_launch(const mchap::CallParams *P, double *unit_tab, int wgc, hipStream_t stream) {
  mchap::CallWideParams W;
  W.c = *P;
  W.unit_tab = unit_tab;
  W.unit_doubles = mchap::call_wide_unit_doubles(P->R, P->H, P->K);
  const size_t lds = mchap::call_wide_lds_bytes(P->H, wgc);
  if (P->H > mchap::CALL_WIDE_MAX_HAPS || lds > mchap::CALL_WIDE_LDS) return (int)hipErrorInvalidValue;
  const void *fn = P->K <= 8 ? reinterpret_cast<const void *>(mchap::call_wide_kernel<8>)
                             : reinterpret_cast<const void *>(mchap::call_wide_kernel<mchap::EXACT_KMAX>);
  // (the same bound whatever the shape: the attribute is the kernel's, and callers of different shapes on different threads would
  // otherwise lower it under each other's launches)
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mchap::CALL_WIDE_LDS);
  if (e != hipSuccess) return (int)e;
  const long long cells = (long long)P->R * P->H;
  long long nb = (cells + mchap::CALL_WIDE_SETUP_THREADS - 1) / mchap::CALL_WIDE_SETUP_THREADS;
  if (nb > 64) nb = 64;
  hipLaunchKernelGGL(mchap::call_wide_setup_kernel, dim3((unsigned)nb, (unsigned)P->n_units), dim3(mchap::CALL_WIDE_SETUP_THREADS), 0, stream, W);
  const dim3 grid((unsigned)((P->chains + wgc - 1) / wgc), (unsigned)P->n_units), block(64 * wgc);
  if (P->K <= 8) hipLaunchKernelGGL(mchap::call_wide_kernel<8>, grid, block, lds, stream, W);
  else hipLaunchKernelGGL(mchap::call_wide_kernel<mchap::EXACT_KMAX>, grid, block, lds, stream, W);
  return (int)hipGetLastError();
}

}  // extern "C"
