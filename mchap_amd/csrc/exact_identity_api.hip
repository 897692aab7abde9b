// libmchap_hip.so -- sample pairs by shared-genotype evidence over stored likelihoods (exact_identity_kernel.hpp): the scaled rows
// a of every (record, sample), their register-tiled product over chunks of the genotype axis, the combine launch.  Entry points
// declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_identity_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

bool shape_ok(int n_haps, int ploidy) {
  return ploidy >= 1 && ploidy <= MCHAP_MAX_PLOIDY_DENOVO && n_haps >= 1 && cwr_fits(n_haps, ploidy);
}

// carve of the workspace: the half log prior of every record, the samples' maxima, the rows a, the chunks' partial sums
struct Carve {
  size_t hp = 0, m = 0, a = 0, part = 0, bytes = 0;
};
Carve carve(int n_records, int n_samples, long long G) {
  Carve c;
  size_t o = 0;
  const size_t R = (size_t)n_records, n = (size_t)n_samples;
  c.hp = o; o += up256(R * (size_t)G * 8);
  c.m = o; o += up256(R * n * 8);
  c.a = o; o += up256(R * n * (size_t)G * 8);
  c.part = o; o += up256(R * (size_t)mchap::identity_nchunk(G) * n * n * 8);
  c.bytes = o;
  return c;
}

}  // namespace

extern "C" {

int64_t mchap_exact_identity_workspace_bytes(int n_records, int n_samples, int n_haps, int ploidy) {
  if (!shape_ok(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_records <= 0 || n_samples <= 0) return 0;
  const long long G = host_cwr(n_haps, ploidy);
  // (every array below 2^62 bytes: what a caller cuts its records by)
  const unsigned __int128 a = (unsigned __int128)n_records * n_samples * (unsigned __int128)G * 8;
  const unsigned __int128 p = (unsigned __int128)n_records * n_samples * n_samples * (unsigned __int128)mchap::identity_nchunk(G) * 8;
  if ((a >> 61) || (p >> 61)) return -1;
  return (int64_t)carve(n_records, n_samples, G).bytes;
}

int mchap_exact_identity_device(int n_records, int n_samples, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                const double *frequencies, int stride, const double *log_norm, double error, const int32_t *reads,
                                double *lbf, int phases, void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_records <= 0 || n_samples <= 0) return MCHAP_OK;
  if (!llks64 || !log_norm || !lbf) return fail(MCHAP_ERR_BAD_ARG, "identity: NULL buffer");
  if (inbreeding && !frequencies) return fail(MCHAP_ERR_BAD_ARG, "identity: NULL buffer (a prior needs frequencies)");
  if (phases < 1 || phases > 3) return fail(MCHAP_ERR_BAD_ARG, "identity: phases = %d, not 1 (the rows a), 2 (the product) or 3 (both)", phases);
  if (!(error >= 0.0 && error <= 1.0)) return fail(MCHAP_ERR_BAD_ARG, "identity: the error lies in [0, 1]");
  if (inbreeding && !(*inbreeding >= 0.0 && *inbreeding < 1.0)) return fail(MCHAP_ERR_BAD_ARG, "identity: F must lie in [0, 1)");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_haps < 1 || (inbreeding && stride < n_haps)) return fail(MCHAP_ERR_BAD_ARG, "identity: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  if (inbreeding && mchap::exact_ev_chunk(n_haps, ploidy, 1) == 0) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the identity kernel's prior tables", n_haps);
  const int64_t need = mchap_exact_identity_workspace_bytes(n_records, n_samples, n_haps, ploidy);
  if (need < 0) return fail(MCHAP_ERR_LIMIT, "identity: %d records x %d samples exceed one call", n_records, n_samples);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_LIMIT, "workspace of %lld bytes is too small: %lld needed (mchap_exact_identity_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  const long long G = host_cwr(n_haps, ploidy);
  const Carve cv = carve(n_records, n_samples, G);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  mchap::IdentityParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk = llks64;
  E.freqs = inbreeding ? frequencies : nullptr;
  E.log_norm = log_norm;
  E.reads = reads;
  E.stride = stride; E.H = n_haps; E.K = ploidy; E.n = n_samples;
  E.has_prior = inbreeding ? 1 : 0;
  E.F = inbreeding ? *inbreeding : 0.0;
  E.error = error;
  E.G = G;
  const long long nblk = (G + mchap::EXACT_GENOS_PER_BLOCK - 1) / mchap::EXACT_GENOS_PER_BLOCK;
  if ((unsigned __int128)n_records * nblk > 0x7fffffffull)
    return fail(MCHAP_ERR_LIMIT, "identity: %d records x %lld tiles exceed one launch", n_records, nblk);
  E.nblk = (int)nblk;
  E.nt = (n_samples + mchap::IDENTITY_TILE - 1) / mchap::IDENTITY_TILE;
  E.nchunk = mchap::identity_nchunk(G);
  E.chunk_len = mchap::identity_chunk_len(G);
  const long long ntri = (long long)E.nt * (E.nt + 1) / 2;
  const long long cells = (long long)n_samples * n_samples;
  const long long ncb = (cells + mchap::EXACT_THREADS - 1) / mchap::EXACT_THREADS;
  const unsigned __int128 grid_p = (unsigned __int128)n_records * E.nchunk * (unsigned __int128)ntri;
  if (ntri > 0x7fffffffll || grid_p > 0x7fffffffull || (unsigned __int128)n_records * ncb > 0x7fffffffull ||
      (long long)n_records * E.nblk > 0x7fffffffll || (long long)n_records * n_samples > 0x7fffffffll)
    return fail(MCHAP_ERR_LIMIT, "identity: %d records x %d samples exceed one launch", n_records, n_samples);
  E.ntri = (int)ntri;
  E.ncb = (int)ncb;
  E.hp = reinterpret_cast<double *>(ws + cv.hp);
  E.m = reinterpret_cast<double *>(ws + cv.m);
  E.a = reinterpret_cast<double *>(ws + cv.a);
  E.part = reinterpret_cast<double *>(ws + cv.part);
  E.lbf = lbf;
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (inbreeding && (phases & 1)) {
    const size_t lds = mchap::identity_prior_lds(n_haps, ploidy);
    auto k = ploidy <= 8 ? mchap::identity_prior_kernel<8> : mchap::identity_prior_kernel<mchap::EXACT_KMAX>;
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_records * E.nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
    HIP_TRY(hipGetLastError());
  }
  if (phases & 1) {
    hipLaunchKernelGGL(mchap::identity_a_kernel, dim3((unsigned)((long long)n_records * n_samples)), dim3(mchap::EXACT_THREADS), 0, stream, E);
    HIP_TRY(hipGetLastError());
  }
  if (!(phases & 2)) return MCHAP_OK;
  hipLaunchKernelGGL(mchap::identity_product_kernel, dim3((unsigned)(unsigned long long)grid_p), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::identity_combine_kernel, dim3((unsigned)((long long)n_records * ncb)), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // extern "C"
