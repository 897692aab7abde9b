// libmchap_hip_test.so only: the keys of the call sampler's likelihood tables as the device computes them (call_mcmc_kernel.hpp),
// for the parity suite.  An object of its own, so that neither flavour of mchap_hip.hip includes the call kernels.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "call_mcmc_kernel.hpp"

using mchap::ensure_init;
using mchap::fail;

extern "C" {

/* test library only: the keys of the call sampler's likelihood tables, computed on the device.  genotypes: [n][ploidy] int32
 * alleles in any order (host); which = 0: call_key<8> (call_mcmc_kernel, ploidy <= 8), 1: call_key<16> (ploidies 9 to 15),
 * 2: call_wide_key<8>, 3: call_wide_key<16>; ranks: [n] int64 (host). */
static __global__ __launch_bounds__(256) void debug_call_keys_kernel(const int *genotypes, int n, int K, int which, long long *ranks) {
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
    int g[mchap::EXACT_KMAX];
    for (int q = 0; q < mchap::EXACT_KMAX; q++) g[q] = q < K ? genotypes[(size_t)i * K + q] : 0;
    long long r;
    if (which == 0) r = mchap::call_key<8>(g, K);
    else if (which == 1) r = mchap::call_key<mchap::EXACT_KMAX>(g, K);
    else if (which == 2) r = mchap::call_wide_key<8>(g, K);
    else r = mchap::call_wide_key<mchap::EXACT_KMAX>(g, K);
    ranks[i] = r;
  }
}
int mchap_debug_call_keys(const int32_t *genotypes, int n, int ploidy, int which, int64_t *ranks) {
  if (n <= 0) return MCHAP_OK;
  if (!genotypes || !ranks) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  if (which < 0 || which > 3 || ploidy < 1 || ploidy > ((which & 1) ? MCHAP_MAX_PLOIDY_DENOVO : 8))
    return fail(MCHAP_ERR_BAD_ARG, "key function %d at ploidy %d", which, ploidy);
  int rc = ensure_init();
  if (rc) return rc;
  int *g_dev = nullptr;
  long long *r_dev = nullptr;
  HIP_TRY(hipMalloc(&g_dev, (size_t)n * ploidy * sizeof(int)));
  hipError_t e = hipMalloc(&r_dev, (size_t)n * sizeof(long long));
  if (e == hipSuccess) e = hipMemcpy(g_dev, genotypes, (size_t)n * ploidy * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(debug_call_keys_kernel, dim3(1), dim3(256), 0, 0, g_dev, n, ploidy, which, r_dev);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(ranks, r_dev, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost);
  (void)hipFree(g_dev);
  (void)hipFree(r_dev);
  if (e != hipSuccess) return fail(MCHAP_ERR_HIP, "mchap_debug_call_keys: %s", hipGetErrorString(e));
  return MCHAP_OK;
}

}  // extern "C"
