// C ABI of the find-snvs pileup kernels (pileup_kernel.hpp; declared in include/mchap_hip.h).  Device pointers, a hipStream_t
// passed as void*, enqueue and return: the caller (mchap_amd/find_snvs.py) owns every buffer.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "pileup_kernel.hpp"

namespace {

int launched(const char *what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MCHAP_OK;
  return mchap::fail(MCHAP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

unsigned grid_of(int64_t n) { return (unsigned)((n + mchap::PILEUP_THREADS - 1) / mchap::PILEUP_THREADS); }

}  // namespace

extern "C" {

int mchap_pileup_overlap_device(uint8_t *bytes, int64_t n_bytes, const int64_t *segments, const int64_t *first, int64_t n_segments,
                                int64_t n_positions, void *stream) {
  if (n_segments <= 0 || n_positions <= 0) return MCHAP_OK;
  if (!bytes || !segments || !first || n_bytes <= 0) return mchap::fail(MCHAP_ERR_BAD_ARG, "pileup overlap: NULL buffer");
  if (grid_of(n_positions) > 0x7fffffffu) return mchap::fail(MCHAP_ERR_LIMIT, "pileup overlap: too many positions");
  hipLaunchKernelGGL(mchap::pileup_overlap_kernel, dim3(grid_of(n_positions)), dim3(mchap::PILEUP_THREADS), 0, (hipStream_t)stream,
                     bytes, n_bytes, segments, first, n_segments, n_positions);
  return launched("pileup_overlap_kernel");
}

int mchap_pileup_depth_device(const uint8_t *bytes, int64_t n_bytes, const int64_t *segments, const int64_t *tile_first,
                              int n_samples, int64_t n_rows, int tile, int min_base_quality, int variant, int32_t *depth,
                              void *stream) {
  if (n_rows <= 0 || n_samples <= 0) return MCHAP_OK;
  if (!tile_first || !depth) return mchap::fail(MCHAP_ERR_BAD_ARG, "pileup depth: NULL buffer");
  if (tile < 1 || tile > mchap::PILEUP_MAX_TILE) return mchap::fail(MCHAP_ERR_BAD_ARG, "pileup depth: tile must be 1..2048");
  if (n_samples > 65535) return mchap::fail(MCHAP_ERR_LIMIT, "pileup depth: more than 65535 samples in one launch");
  const int64_t n_tiles = (n_rows + tile - 1) / tile;
  if (n_tiles > 0x7fffffff) return mchap::fail(MCHAP_ERR_LIMIT, "pileup depth: too many tiles");
  const dim3 grid((unsigned)n_tiles, (unsigned)n_samples);
  if (variant == 0)
    hipLaunchKernelGGL(mchap::pileup_depth_kernel<0>, grid, dim3(mchap::PILEUP_THREADS), 0, (hipStream_t)stream, bytes, n_bytes,
                       segments, tile_first, n_samples, n_tiles, n_rows, tile, min_base_quality, depth);
  else if (variant == 1)
    hipLaunchKernelGGL(mchap::pileup_depth_kernel<1>, grid, dim3(mchap::PILEUP_THREADS), 0, (hipStream_t)stream, bytes, n_bytes,
                       segments, tile_first, n_samples, n_tiles, n_rows, tile, min_base_quality, depth);
  else
    return mchap::fail(MCHAP_ERR_BAD_ARG, "pileup depth: variant must be 0 (LDS histogram) or 1 (global atomics)");
  return launched("pileup_depth_kernel");
}

int mchap_pileup_filter_device(const int32_t *depth, const int8_t *ref_index, int64_t n_rows, int n_samples, double maf, int64_t mad,
                               double ind_maf, int64_t ind_mad, int64_t min_ind, int32_t *flags, double *admf, void *stream) {
  if (n_rows <= 0) return MCHAP_OK;
  if (!depth || !ref_index || !flags || !admf || n_samples <= 0)
    return mchap::fail(MCHAP_ERR_BAD_ARG, "pileup filter: NULL buffer or no samples");
  if (grid_of(n_rows) > 0x7fffffffu) return mchap::fail(MCHAP_ERR_LIMIT, "pileup filter: too many rows");
  hipLaunchKernelGGL(mchap::pileup_filter_kernel, dim3(grid_of(n_rows)), dim3(mchap::PILEUP_THREADS), 0, (hipStream_t)stream, depth,
                     ref_index, n_rows, n_samples, maf, mad, ind_maf, ind_mad, min_ind, flags, admf);
  return launched("pileup_filter_kernel");
}

}  // extern "C"
