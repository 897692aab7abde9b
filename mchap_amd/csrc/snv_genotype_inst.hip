// C ABI of the find-snvs genotype caller (snv_genotype_kernel.hpp; declared in include/mchap_hip.h).  Device pointers, a hipStream_t
// passed as void*: the caller (mchap_amd/find_snvs.py) owns every buffer.
#include <hip/hip_runtime.h>

#include <vector>

#include "host_common.hpp"
#include "snv_genotype_kernel.hpp"

extern "C" {

int mchap_snv_genotypes_device(const int32_t *depth, const int32_t *flags, const double *admf, int64_t n_rows, int n_samples,
                               const int32_t *ploidy, const double *inbreeding, int use_admf, double p_call, double p_other,
                               int32_t *gt_index, double *gpm, void *stream) {
  if (n_rows <= 0 || n_samples <= 0) return MCHAP_OK;
  if (!depth || !flags || !admf || !ploidy || !inbreeding || !gt_index || !gpm)
    return mchap::fail(MCHAP_ERR_BAD_ARG, "snv genotypes: NULL buffer");
  if (n_samples > 65535) return mchap::fail(MCHAP_ERR_LIMIT, "snv genotypes: more than 65535 samples in one launch");
  // the samples' ploidies size the lanes' tables, so they are read back first: the one wait of this call (n_samples values)
  std::vector<int32_t> k((size_t)n_samples);
  HIP_TRY(hipMemcpyAsync(k.data(), ploidy, sizeof(int32_t) * (size_t)n_samples, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  int k_max = 0;
  for (int s = 0; s < n_samples; s++) {
    if (k[s] < 1) return mchap::fail(MCHAP_ERR_BAD_ARG, "snv genotypes: ploidy %d of sample %d (must be at least 1)", (int)k[s], s);
    if (k[s] > mchap::SNV_MAX_PLOIDY)
      return mchap::fail(MCHAP_ERR_LIMIT, "snv genotypes: ploidy %d of sample %d is beyond MCHAP_MAX_PLOIDY_DENOVO (%d)", (int)k[s], s,
                         mchap::SNV_MAX_PLOIDY);
    k_max = k[s] > k_max ? k[s] : k_max;
  }
  const int rows = k_max + 1;
  int threads = 256;  // the most lanes whose tables fit the 64 KiB a workgroup may take without asking
  while (threads > 64 && mchap::snv_lds_doubles(rows, threads) * sizeof(double) > 65536) threads >>= 1;
  const size_t lds = mchap::snv_lds_doubles(rows, threads) * sizeof(double);
  const int64_t n_pairs = n_rows * (int64_t)n_samples;
  const int64_t grid = (n_pairs + threads - 1) / threads;
  if (grid > 0x7fffffff) return mchap::fail(MCHAP_ERR_LIMIT, "snv genotypes: too many (row, sample) pairs in one launch");
  hipLaunchKernelGGL(mchap::snv_genotype_kernel, dim3((unsigned)grid), dim3(threads), lds, (hipStream_t)stream, depth, flags, admf,
                     n_pairs, n_samples, ploidy, inbreeding, use_admf, p_call, p_other, rows, gt_index, gpm);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mchap::fail(MCHAP_ERR_HIP, "snv_genotype_kernel: %s", hipGetErrorString(e));
  return MCHAP_OK;
}

}  // extern "C"
