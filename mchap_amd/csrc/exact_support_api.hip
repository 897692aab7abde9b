// libmchap_hip.so -- expected read depth of every haplotype over stored likelihoods (exact_support_kernel.hpp): the evidence launches
// at the unit's own F for the normaliser, then the tiles' launch and the combine launch.  Entry points declared in
// include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_support_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

int support_nblk(long long G) { return (int)((G + mchap::EXACT_GENOS_PER_BLOCK - 1) / mchap::EXACT_GENOS_PER_BLOCK); }

// carve of the caller's workspace: the evidence pass' partials, the normalisers, the tiles' partial sums
struct SupportCarve {
  size_t ev = 0, norm = 0, part = 0, bytes = 0;
};
SupportCarve support_carve(int n_units, int n_reads, int n_haps, int ploidy, int per_read) {
  const size_t nb = (size_t)support_nblk(host_cwr(n_haps, ploidy));
  SupportCarve c;
  size_t o = 0;
  c.ev = o; o += up256((size_t)n_units * nb * 2 * 8);
  c.norm = o; o += up256((size_t)n_units * 8);
  c.part = o; o += up256((size_t)n_units * nb * (per_read ? (size_t)n_reads : 1) * (size_t)n_haps * 8);
  c.bytes = o;
  return c;
}

}  // namespace

extern "C" {

int64_t mchap_exact_support_workspace_bytes(int n_units, int n_reads, int n_haps, int ploidy, int per_read) {
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO || !cwr_fits(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_units <= 0 || n_reads < 1 || n_haps < 1) return 0;
  return (int64_t)support_carve(n_units, n_reads, n_haps, ploidy, per_read).bytes;
}

int mchap_exact_support_tile(int n_reads, int n_haps, int ploidy) {
  if (n_reads < 1 || n_haps < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  return mchap::exact_support_rows(n_reads, n_haps, ploidy);
}

int mchap_exact_allele_support_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                      const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                      const double *llks64, const double *inbreeding, const int32_t *unit_row,
                                      const double *frequencies, int stride, double *depth, double *read_post, double *log_norm,
                                      void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!reads || !haplotypes || !llks64 || !depth) return fail(MCHAP_ERR_BAD_ARG, "allele support: NULL buffer");
  if (inbreeding && (!unit_row || !frequencies)) return fail(MCHAP_ERR_BAD_ARG, "allele support: NULL buffer (a prior needs unit_row and frequencies)");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_reads < 1 || n_pos < 1 || max_allele < 1 || n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "allele support: empty shape");
  if (inbreeding && stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "allele support: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = support_nblk(G);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "allele support: %d units x %d tiles exceed one launch", n_units, nblk);
  const int rows = mchap::exact_support_rows(n_reads, n_haps, ploidy);
  if (rows == 0) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the allele support's tables: not even 64 read rows fit the LDS", n_haps);
  const SupportCarve cv = support_carve(n_units, n_reads, n_haps, ploidy, read_post != nullptr);
  if (!workspace || workspace_bytes < (int64_t)cv.bytes)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %zu needed (mchap_exact_support_workspace_bytes)",
                (long long)workspace_bytes, cv.bytes);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  double *norm = reinterpret_cast<double *>(ws + cv.norm);
  // first pass: the normaliser of every unit's posterior -- its model evidence at its own F (one grid point)
  int rc = mchap_exact_evidence_device(n_units, llks64, n_haps, ploidy, 1, inbreeding, unit_row, frequencies, stride, norm, ws + cv.ev,
                                       (int64_t)(cv.norm - cv.ev), stream_);
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactSupportParams E;
  std::memset(&E, 0, sizeof(E));
  E.reads = reads;
  E.counts = read_counts;
  E.haps = haplotypes;
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_row = unit_row;
  E.freqs = frequencies;
  E.stride = stride;
  E.R = n_reads; E.M = n_pos; E.A = max_allele; E.H = n_haps; E.K = ploidy; E.nblk = nblk;
  E.RT = rows;
  E.G = G;
  E.log_norm = norm;
  E.part = reinterpret_cast<double *>(ws + cv.part);
  E.depth = depth;
  E.read_post = read_post;
  E.log_norm_out = log_norm;
  const size_t lds = mchap::exact_support_lds(n_haps, ploidy, rows);
  auto k = ploidy <= 8 ? mchap::exact_support_kernel<8> : mchap::exact_support_kernel<mchap::EXACT_KMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::exact_support_combine_kernel, dim3(n_units), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // extern "C"
