// libmchap_hip.so -- selfed parents per progeny over stored likelihoods (exact_selfing_kernel.hpp): the selfing prior of every
// candidate unit (after the gamete launch for the normaliser and the error-free gamete table), and the evidence of every progeny
// of a record under every candidate's selfing prior.  Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_selfing_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

constexpr size_t LDS_MOST = 64 * 1024;  // (no launch asks for more than the default dynamic LDS)

int tiles_of(long long n, int per) { return (int)((n + per - 1) / per); }
bool ploidy_ok(int k) { return k >= 1 && k <= MCHAP_MAX_PLOIDY_DENOVO; }
// the shapes the prior launches take: what the gamete entry takes, and the rank table in LDS
bool prior_shape_ok(int n_haps, int ploidy) {
  return ploidy_ok(ploidy) && cwr_fits(n_haps, ploidy) &&
         (n_haps < 1 || (mchap::exact_selfing_lds(n_haps, ploidy) <= LDS_MOST && mchap::exact_gamete_lds(n_haps, ploidy) <= LDS_MOST));
}

// carve of the prior call's workspace: a gamete error of 0 per unit, the normalisers, the error-free gamete tables, the
// posteriors, the gamete call's own workspace
struct PriorCarve {
  size_t zero = 0, norm = 0, gam = 0, post = 0, gws = 0, gws_bytes = 0, bytes = 0;
};
PriorCarve prior_carve(int n_units, int n_haps, int ploidy) {
  PriorCarve c;
  size_t o = 0;
  c.zero = o; o += up256((size_t)n_units * 8);
  c.norm = o; o += up256((size_t)n_units * 8);
  c.gam = o; o += up256((size_t)n_units * (size_t)host_cwr(n_haps, ploidy / 2) * 8);
  c.post = o; o += up256((size_t)n_units * (size_t)host_cwr(n_haps, ploidy) * 8);
  c.gws = o;
  c.gws_bytes = (size_t)mchap_exact_gametes_workspace_bytes(n_units, n_haps, ploidy);
  o += up256(c.gws_bytes);
  c.bytes = o;
  return c;
}

// carve of the evidence call's workspace: the progeny's maxima, the tiles' sums
struct EvidenceCarve {
  size_t lmax = 0, part = 0, bytes = 0;
};
EvidenceCarve evidence_carve(int n_records, int n_progeny, int n_cand, int ntile) {
  EvidenceCarve c;
  size_t o = 0;
  c.lmax = o; o += up256((size_t)n_records * n_progeny * 8);
  c.part = o; o += up256((size_t)n_records * n_progeny * n_cand * ntile * 8);
  c.bytes = o;
  return c;
}

}  // namespace

extern "C" {

int64_t mchap_exact_selfing_prior_workspace_bytes(int n_units, int n_haps, int ploidy) {
  if (!prior_shape_ok(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_units <= 0 || n_haps < 1 || ploidy % 2) return 0;
  const unsigned __int128 post = (unsigned __int128)n_units * (unsigned __int128)host_cwr(n_haps, ploidy) * 8;
  if (post >> 62) return -1;
  return (int64_t)prior_carve(n_units, n_haps, ploidy).bytes;
}

int mchap_exact_selfing_prior_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                     const int32_t *unit_row, const double *frequencies, int stride, const double *gamete_error,
                                     double *log_self, double *self_prior, double *log_norm, void *workspace,
                                     int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !unit_row || !frequencies || !gamete_error || !log_self) return fail(MCHAP_ERR_BAD_ARG, "selfing prior: NULL buffer");
  if (!ploidy_ok(ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (ploidy % 2) return fail(MCHAP_ERR_BAD_ARG, "selfing prior: a parent of odd ploidy %d", ploidy);
  if (n_haps < 1 || stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "selfing prior: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const size_t lds = mchap::exact_selfing_lds(n_haps, ploidy), lds_post = mchap::exact_gamete_lds(n_haps, ploidy);
  if (lds > LDS_MOST || lds_post > LDS_MOST) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the selfing kernel's rank table", n_haps);
  const int64_t need = mchap_exact_selfing_prior_workspace_bytes(n_units, n_haps, ploidy);
  if (need < 0) return fail(MCHAP_ERR_LIMIT, "selfing prior: %d units of ploidy %d over %d haplotypes exceed one call", n_units, ploidy, n_haps);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %lld needed (mchap_exact_selfing_prior_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  const int T = ploidy / 2;
  const long long G = host_cwr(n_haps, ploidy), NA = host_cwr(n_haps, T);
  const int nblk = tiles_of(G, mchap::EXACT_THREADS);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "selfing prior: %d units x %d tiles exceed one launch", n_units, nblk);
  const PriorCarve cv = prior_carve(n_units, n_haps, ploidy);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  double *zero = reinterpret_cast<double *>(ws + cv.zero);
  double *norm = reinterpret_cast<double *>(ws + cv.norm);
  double *gam = reinterpret_cast<double *>(ws + cv.gam);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // the normaliser and the ERROR-FREE gamete table of every unit: the gamete launch at a gamete error of 0 (all bits 0)
  HIP_TRY(hipMemsetAsync(zero, 0, (size_t)n_units * 8, stream));
  rc = mchap_exact_gametes_device(n_units, llks64, n_haps, ploidy, inbreeding, unit_row, frequencies, stride, zero, gam, norm, ws + cv.gws,
                                  (int64_t)cv.gws_bytes, stream_);
  if (rc) return rc;
  mchap::ExactSelfingParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_row = unit_row;
  E.freqs = frequencies;
  E.error = gamete_error;
  E.stride = stride;
  E.H = n_haps; E.K = ploidy; E.T = T; E.nblk = nblk;
  E.G = G; E.NA = NA;
  E.log_norm = norm;
  E.gam = gam;
  E.post = reinterpret_cast<double *>(ws + cv.post);
  E.log_self = log_self;
  E.self = self_prior;
  const dim3 grid((unsigned)((long long)n_units * nblk)), block(mchap::EXACT_THREADS);
  auto kp = ploidy <= 8 ? mchap::exact_selfing_post_kernel<8> : mchap::exact_selfing_post_kernel<mchap::EXACT_KMAX>;
  hipLaunchKernelGGL(kp, grid, block, lds_post, stream, E);
  HIP_TRY(hipGetLastError());
  auto k = ploidy <= 4 ? mchap::exact_selfing_prior_kernel<4>
                       : ploidy <= 8 ? mchap::exact_selfing_prior_kernel<8> : mchap::exact_selfing_prior_kernel<mchap::EXACT_KMAX>;
  hipLaunchKernelGGL(k, grid, block, lds, stream, E);
  HIP_TRY(hipGetLastError());
  if (log_norm) HIP_TRY(hipMemcpyAsync(log_norm, norm, (size_t)n_units * 8, hipMemcpyDeviceToDevice, stream));
  return MCHAP_OK;
}

int64_t mchap_exact_selfing_evidence_workspace_bytes(int n_records, int n_progeny, int n_candidates, int n_haps, int ploidy) {
  if (!ploidy_ok(ploidy) || !cwr_fits(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_records <= 0 || n_progeny <= 0 || n_candidates < 1 || n_haps < 1) return 0;
  const int ntile = tiles_of(host_cwr(n_haps, ploidy), mchap::EXACT_GENOS_PER_BLOCK);
  const unsigned __int128 part = (unsigned __int128)n_records * n_progeny * n_candidates * (unsigned __int128)ntile * 8;
  if (part >> 62) return -1;
  return (int64_t)evidence_carve(n_records, n_progeny, n_candidates, ntile).bytes;
}

int mchap_exact_selfing_evidence_device(int n_records, int n_progeny, int n_candidates, const double *self_prior, const double *llks_c,
                                        const int32_t *progeny_reads, int n_haps, int ploidy, double *log_z, void *workspace,
                                        int64_t workspace_bytes, void *stream_) {
  if (n_records <= 0 || n_progeny <= 0) return MCHAP_OK;
  if (n_candidates < 1) return fail(MCHAP_ERR_BAD_ARG, "selfing evidence: %d candidates", n_candidates);
  if (!self_prior || !llks_c || !log_z) return fail(MCHAP_ERR_BAD_ARG, "selfing evidence: NULL buffer");
  if (n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "selfing evidence: no haplotype");
  if (!ploidy_ok(ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const int64_t need = mchap_exact_selfing_evidence_workspace_bytes(n_records, n_progeny, n_candidates, n_haps, ploidy);
  if (need < 0)
    return fail(MCHAP_ERR_LIMIT, "selfing evidence: %d records x %d progeny x %d candidates exceed one call", n_records, n_progeny, n_candidates);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_LIMIT, "workspace of %lld bytes is too small: %lld needed (mchap_exact_selfing_evidence_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  const long long G = host_cwr(n_haps, ploidy);
  const int ntile = tiles_of(G, mchap::EXACT_GENOS_PER_BLOCK);
  const long long rc_n = (long long)n_records * n_progeny;
  const unsigned __int128 grid_t = (unsigned __int128)rc_n * ntile, cells = (unsigned __int128)rc_n * n_candidates;
  if (grid_t > 0x7fffffffull || cells > 0x7fffffffull)
    return fail(MCHAP_ERR_LIMIT, "selfing evidence: %d records x %d progeny x %d candidates exceed one launch", n_records, n_progeny, n_candidates);
  const EvidenceCarve cv = evidence_carve(n_records, n_progeny, n_candidates, ntile);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  mchap::SelfingEvidenceParams E;
  std::memset(&E, 0, sizeof(E));
  E.self = self_prior;
  E.llk = llks_c;
  E.reads = progeny_reads;
  E.C = n_progeny; E.n = n_candidates; E.ntile = ntile;
  E.G = G; E.cells = (long long)cells;
  E.lmax = reinterpret_cast<double *>(ws + cv.lmax);
  E.part = reinterpret_cast<double *>(ws + cv.part);
  E.log_z = log_z;
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 block(mchap::EXACT_THREADS);
  hipLaunchKernelGGL(mchap::selfing_max_kernel, dim3((unsigned)rc_n), block, 0, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::selfing_evidence_kernel, dim3((unsigned)(unsigned long long)grid_t), block, 0, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::selfing_combine_kernel, dim3((unsigned)tiles_of((long long)cells, mchap::EXACT_THREADS)), block, 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // extern "C"
