// libmchap_hip.so -- progeny calls under their parents' cross prior over stored likelihoods (exact_cross_kernel.hpp): the parents'
// gamete tables (after the evidence launches for the normaliser), the cross prior of a record, the progeny's posterior under it.
// Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_cross_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

int tiles_of(long long n, int per) { return (int)((n + per - 1) / per); }
bool ploidy_ok(int k) { return k >= 1 && k <= MCHAP_MAX_PLOIDY_DENOVO; }
bool parent_ok(int k) { return ploidy_ok(k) && k % 2 == 0; }

// carve of the gamete call's workspace: the evidence pass' partials, the normalisers
struct GameteCarve {
  size_t ev = 0, norm = 0, bytes = 0;
};
GameteCarve gamete_carve(int n_units, int n_haps, int ploidy) {
  const size_t nb = (size_t)tiles_of(host_cwr(n_haps, ploidy), mchap::EXACT_GENOS_PER_BLOCK);
  GameteCarve c;
  size_t o = 0;
  c.ev = o; o += up256((size_t)n_units * nb * 2 * 8);
  c.norm = o; o += up256((size_t)n_units * 8);
  c.bytes = o;
  return c;
}

// carve of the posterior call's workspace: the evidence pass' partials (where log_norm is asked for), the tiles' maxima and sums,
// their genotypes
struct PostCarve {
  size_t ev = 0, part = 0, part_i = 0, bytes = 0;
};
PostCarve post_carve(int n_units, int n_haps, int ploidy) {
  const size_t nb = (size_t)tiles_of(host_cwr(n_haps, ploidy), mchap::EXACT_GENOS_PER_BLOCK);
  PostCarve c;
  size_t o = 0;
  c.ev = o; o += up256((size_t)n_units * nb * 2 * 8);
  c.part = o; o += up256((size_t)n_units * nb * 2 * 8);
  c.part_i = o; o += up256((size_t)n_units * nb * 8);
  c.bytes = o;
  return c;
}

}  // namespace

extern "C" {

int64_t mchap_exact_gametes_workspace_bytes(int n_units, int n_haps, int ploidy) {
  if (!ploidy_ok(ploidy) || !cwr_fits(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_units <= 0 || n_haps < 1) return 0;
  return (int64_t)gamete_carve(n_units, n_haps, ploidy).bytes;
}

int mchap_exact_gametes_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                               const int32_t *unit_row, const double *frequencies, int stride, const double *gamete_error,
                               double *gametes, double *log_norm, void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !unit_row || !frequencies || !gamete_error || !gametes) return fail(MCHAP_ERR_BAD_ARG, "gametes: NULL buffer");
  if (!ploidy_ok(ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (ploidy % 2) return fail(MCHAP_ERR_BAD_ARG, "gametes: a parent of odd ploidy %d", ploidy);
  if (n_haps < 1 || stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "gametes: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const int T = ploidy / 2;
  const long long G = host_cwr(n_haps, ploidy), NA = host_cwr(n_haps, T), NR = host_cwr(n_haps, ploidy - T);
  const int nblk = tiles_of(NA, mchap::EXACT_THREADS);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "gametes: %d units x %d tiles exceed one launch", n_units, nblk);
  const size_t lds = mchap::exact_gamete_lds(n_haps, ploidy);
  if (lds > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the gamete kernel's prior tables", n_haps);
  const GameteCarve cv = gamete_carve(n_units, n_haps, ploidy);
  if (!workspace || workspace_bytes < (int64_t)cv.bytes)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %zu needed (mchap_exact_gametes_workspace_bytes)",
                (long long)workspace_bytes, cv.bytes);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  double *norm = reinterpret_cast<double *>(ws + cv.norm);
  // first pass: the normaliser of every parent's posterior -- its model evidence at its own F (one grid point)
  int rc = mchap_exact_evidence_device(n_units, llks64, n_haps, ploidy, 1, inbreeding, unit_row, frequencies, stride, norm, ws + cv.ev,
                                       (int64_t)(cv.norm - cv.ev), stream_);
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactGameteParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_row = unit_row;
  E.freqs = frequencies;
  E.error = gamete_error;
  E.stride = stride;
  E.H = n_haps; E.K = ploidy; E.T = T; E.nblk = nblk;
  E.G = G; E.NA = NA; E.NR = NR;
  E.log_norm = norm;
  E.gametes = gametes;
  E.log_norm_out = log_norm;
  auto k = ploidy <= 8 ? mchap::exact_gamete_kernel<8> : mchap::exact_gamete_kernel<mchap::EXACT_KMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int64_t mchap_exact_cross_prior_workspace_bytes(int n_rows, int n_haps, int ploidy_p, int ploidy_q) {
  (void)n_rows;
  if (!parent_ok(ploidy_p) || !parent_ok(ploidy_q) || !ploidy_ok(ploidy_p / 2 + ploidy_q / 2) ||
      !cwr_fits(n_haps, ploidy_p / 2 + ploidy_q / 2))
    return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  return 0;     // (every cell is written by its own lane: no partial sums)
}

int mchap_exact_cross_prior_device(int n_rows, const double *gametes_p, const double *gametes_q, int n_haps, int ploidy_p,
                                   int ploidy_q, double *log_cross, void *stream_) {
  if (n_rows <= 0) return MCHAP_OK;
  if (!gametes_p || !gametes_q || !log_cross) return fail(MCHAP_ERR_BAD_ARG, "cross prior: NULL buffer");
  if (!ploidy_ok(ploidy_p) || !ploidy_ok(ploidy_q))
    return fail(MCHAP_ERR_LIMIT, "ploidies %d and %d not in 1..%d", ploidy_p, ploidy_q, MCHAP_MAX_PLOIDY_DENOVO);
  if (ploidy_p % 2 || ploidy_q % 2) return fail(MCHAP_ERR_BAD_ARG, "cross prior: a parent of odd ploidy (%d, %d)", ploidy_p, ploidy_q);
  if (n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "cross prior: no haplotype");
  const int TP = ploidy_p / 2, TQ = ploidy_q / 2, KC = TP + TQ;
  if (!ploidy_ok(KC)) return fail(MCHAP_ERR_LIMIT, "progeny ploidy %d not in 1..%d", KC, MCHAP_MAX_PLOIDY_DENOVO);
  if (!cwr_fits(n_haps, KC)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", KC, n_haps);
  const long long GC = host_cwr(n_haps, KC);
  const int nblk = tiles_of(GC, mchap::EXACT_THREADS);
  if ((long long)n_rows * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "cross prior: %d rows x %d tiles exceed one launch", n_rows, nblk);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactCrossPriorParams E;
  std::memset(&E, 0, sizeof(E));
  E.gam_p = gametes_p;
  E.gam_q = gametes_q;
  E.H = n_haps; E.TP = TP; E.TQ = TQ; E.nblk = nblk;
  E.NAP = host_cwr(n_haps, TP); E.NAQ = host_cwr(n_haps, TQ); E.GC = GC;
  const size_t lds = mchap::exact_cross_prior_lds(E.NAP, E.NAQ);
  E.staged = lds > 0;
  E.log_x = log_cross;
  auto k = KC <= 8 ? mchap::exact_cross_prior_kernel<8> : mchap::exact_cross_prior_kernel<mchap::EXACT_KMAX>;
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_rows * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int64_t mchap_exact_cross_posterior_workspace_bytes(int n_units, int n_haps, int ploidy) {
  if (!ploidy_ok(ploidy) || !cwr_fits(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_units <= 0 || n_haps < 1) return 0;
  return (int64_t)post_carve(n_units, n_haps, ploidy).bytes;
}

int mchap_exact_cross_posterior_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *log_cross,
                                       const int32_t *unit_row, const double *inbreeding, const int32_t *freq_row,
                                       const double *frequencies, int stride, double *log_z, int64_t *mode, double *mode_prob,
                                       double *log_norm, double *posteriors, void *workspace, int64_t workspace_bytes,
                                       void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !log_cross || !unit_row || !log_z || !mode || !mode_prob) return fail(MCHAP_ERR_BAD_ARG, "cross posterior: NULL buffer");
  if (!ploidy_ok(ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "cross posterior: no haplotype");
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = tiles_of(G, mchap::EXACT_GENOS_PER_BLOCK);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "cross posterior: %d units x %d tiles exceed one launch", n_units, nblk);
  const PostCarve cv = post_carve(n_units, n_haps, ploidy);
  if (!workspace || workspace_bytes < (int64_t)cv.bytes)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %zu needed (mchap_exact_cross_posterior_workspace_bytes)",
                (long long)workspace_bytes, cv.bytes);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  int rc = ensure_init();
  if (rc) return rc;
  if (log_norm) {
    // the unit's evidence under its calling prior at its own F: what the cross evidence is compared with
    rc = mchap_exact_evidence_device(n_units, llks64, n_haps, ploidy, 1, inbreeding, freq_row, frequencies, stride, log_norm, ws + cv.ev,
                                     (int64_t)(cv.part - cv.ev), stream_);
    if (rc) return rc;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactCrossPostParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.log_x = log_cross;
  E.unit_row = unit_row;
  E.nblk = nblk;
  E.G = G;
  E.part = reinterpret_cast<double *>(ws + cv.part);
  E.part_i = reinterpret_cast<long long *>(ws + cv.part_i);
  E.log_z = log_z;
  E.mode = reinterpret_cast<long long *>(mode);
  E.mode_prob = mode_prob;
  E.post = posteriors;
  hipLaunchKernelGGL(mchap::exact_cross_post_kernel, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::exact_cross_post_combine_kernel, dim3(n_units), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // extern "C"
