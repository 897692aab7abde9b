// libmchap_hip.so -- the exact caller (exact_kernel.hpp): likelihoods, posteriors and their summaries over every genotype of the
// known haplotypes.  Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_kernel.hpp"

using mchap::cwr_fits;
using mchap::DevArena;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::HostCall;
using mchap::up256;

namespace {

size_t exact_pass1_lds(int R, int H, int K) {
  return ((size_t)R * H + R + (size_t)H * (K + 1) + (K + 1) + H + 5 * mchap::EXACT_THREADS) * 8;
}

// Rows of the LDS product table: all reads when they fit, else the passes tile the reads (exact_tile) with as many
// rows as fit beside the prior tables and the reduction scratch; 0 if not even 32 rows do
int exact_rows(int R, int H, int K) {
  if (exact_pass1_lds(R, H, K) <= 160 * 1024) return R;
  const size_t fixed = exact_pass1_lds(0, H, K) + 64;
  const size_t budget = 144 * 1024;
  if (fixed >= budget) return 0;
  const int rows = (int)((budget - fixed) / ((size_t)(H + 1) * 8)) & ~3;  // (a multiple of four: the groups of exact_llk_tiled)
  return rows >= 32 ? rows : 0;
}

int exact_check_shape(int n_reads, int n_pos, int max_allele, int n_haps, int ploidy) {
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_reads < 1 || n_pos < 1 || max_allele < 1 || n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "empty shape");
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  if (exact_rows(n_reads, n_haps, ploidy) == 0)
    return fail(MCHAP_ERR_LIMIT, "n_haps = %d: not even 32 reads of the product table fit the LDS", n_haps);
  return MCHAP_OK;
}

int exact_nblk(long long G) { return (int)((G + mchap::EXACT_GENOS_PER_BLOCK - 1) / mchap::EXACT_GENOS_PER_BLOCK); }

// carve of the caller's workspace for the streaming form
struct ExactCarve {
  size_t part_max = 0, part_idx = 0, part_llk = 0, part_lse = 0, total = 0, mode = 0, part_freq = 0, bytes = 0;
};
ExactCarve exact_carve(int n_units, int n_haps, int ploidy) {
  const long long G = host_cwr(n_haps, ploidy);
  const size_t nb = (size_t)exact_nblk(G);
  ExactCarve c;
  size_t o = 0;
  c.part_max = o; o += up256((size_t)n_units * nb * 8);
  c.part_idx = o; o += up256((size_t)n_units * nb * 8);
  c.part_llk = o; o += up256((size_t)n_units * nb * 8);
  c.part_lse = o; o += up256((size_t)n_units * nb * 8);
  c.total = o; o += up256((size_t)n_units * 8);
  c.mode = o; o += up256((size_t)n_units * ploidy * 8);
  c.part_freq = o; o += up256((size_t)n_units * nb * (2 * (size_t)n_haps + 1) * 8);
  c.bytes = o;
  return c;
}

int array_nacc(int H, int K) {
  int n = 256;
  while (n > 1 && mchap::exact_array_lds(H, K, n) > 120 * 1024) n >>= 1;
  return n;
}

int launch_exact_array(mchap::ExactArrayParams &A, int n_units, hipStream_t stream) {
  A.nacc = array_nacc(A.H, A.K);
  const size_t lds = mchap::exact_array_lds(A.H, A.K, A.nacc);
  if (lds > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the posterior array pass", A.H);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(A.K <= 8 ? mchap::exact_array_kernel<8> : mchap::exact_array_kernel<mchap::EXACT_KMAX>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // (ploidies 9 to 15: the instantiation with sixteen-entry genotype arrays -- round 5)
  if (A.K <= 8) hipLaunchKernelGGL(mchap::exact_array_kernel<8>, dim3(n_units), dim3(mchap::EXACT_ARRAY_THREADS), lds, stream, A);
  else hipLaunchKernelGGL(mchap::exact_array_kernel<mchap::EXACT_KMAX>, dim3(n_units), dim3(mchap::EXACT_ARRAY_THREADS), lds, stream, A);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // namespace

extern "C" {

int64_t mchap_exact_workspace_bytes(int n_units, int n_haps, int ploidy) {
  if (n_units <= 0 || n_haps < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  if (!cwr_fits(n_haps, ploidy)) return -1;  // (more than 2^62 genotypes: the call itself says so -- MCHAP_ERR_LIMIT)
  return (int64_t)exact_carve(n_units, n_haps, ploidy).bytes;
}

int64_t mchap_exact_workspace_bytes_cached(int n_units, int n_haps, int ploidy) {
  if (n_units <= 0 || n_haps < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  if (!cwr_fits(n_haps, ploidy)) return -1;
  return (int64_t)(exact_carve(n_units, n_haps, ploidy).bytes + up256((size_t)n_units * (size_t)host_cwr(n_haps, ploidy) * 8));
}

int mchap_exact_call_batch_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                  const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy, int has_prior,
                                  const double *inbreeding, const double *frequencies, const mchap_exact_out *out,
                                  void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!reads || !haplotypes || !out) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  int rc = exact_check_shape(n_reads, n_pos, max_allele, n_haps, ploidy);
  if (rc) return rc;
  if (has_prior && !inbreeding) return fail(MCHAP_ERR_BAD_ARG, "prior requested without inbreeding");
  rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = exact_nblk(G);
  const bool want_stream = out->mode_alleles || out->mode_llk || out->mode_prob || out->support_prob || out->freqs || out->occur;
  const bool want_second = out->support_prob || out->freqs || out->occur;
  const bool want_arr_sum = out->arr_mode_alleles || out->arr_mode_prob || out->arr_support_prob || out->arr_freqs || out->arr_counts || out->arr_occur;
  if ((out->posteriors || want_arr_sum) && !out->llks)
    return fail(MCHAP_ERR_BAD_ARG, "the posterior array is formed from the float32 likelihood array: pass `llks` too");
  if (want_arr_sum && !out->posteriors) return fail(MCHAP_ERR_BAD_ARG, "array summaries need the `posteriors` array");
  const ExactCarve cv = exact_carve(n_units, n_haps, ploidy);
  if (want_stream && (!workspace || workspace_bytes < (int64_t)cv.bytes))
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %zu needed (mchap_exact_workspace_bytes)", (long long)workspace_bytes, cv.bytes);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  mchap::ExactParams E;
  std::memset(&E, 0, sizeof(E));
  E.reads = reads;
  E.counts = read_counts;
  E.haps = haplotypes;
  E.inbreeding = has_prior ? inbreeding : nullptr;
  E.freqs = has_prior ? frequencies : nullptr;
  E.R = n_reads; E.M = n_pos; E.A = max_allele; E.H = n_haps; E.K = ploidy;
  E.G = G;
  E.ptab_scale = 1.0 / (double)ploidy;
  E.has_prior = has_prior;
  E.nblk = nblk;
  E.llk32 = out->llks;
  E.llk64 = out->llks64;
  if (want_stream) {
    E.part_max = reinterpret_cast<double *>(ws + cv.part_max);
    E.part_idx = reinterpret_cast<long long *>(ws + cv.part_idx);
    E.part_llk = reinterpret_cast<double *>(ws + cv.part_llk);
    E.part_lse = reinterpret_cast<double *>(ws + cv.part_lse);
  }
  // a workspace of mchap_exact_workspace_bytes_cached holds llk + log prior of every genotype between the two passes
  const bool cached = want_second && workspace && workspace_bytes >= (int64_t)(cv.bytes + up256((size_t)n_units * (size_t)G * 8));
  if (cached) E.ljoint = reinterpret_cast<double *>(ws + cv.bytes);
  const int rows = exact_rows(E.R, E.H, E.K);
  const bool tiled = rows < E.R;
  E.Rcap = tiled ? rows : 0;
  if (want_stream || out->llks || out->llks64) {
    const size_t lds = exact_pass1_lds(rows, E.H, E.K);
    constexpr int KX = mchap::EXACT_KMAX;
    auto k1 = E.K <= 8 ? (tiled ? mchap::exact_pass1_kernel<true, 8> : mchap::exact_pass1_kernel<false, 8>)
                       : (tiled ? mchap::exact_pass1_kernel<true, KX> : mchap::exact_pass1_kernel<false, KX>);
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k1, dim3(nblk, n_units), dim3(mchap::EXACT_THREADS), lds, stream, E);
    HIP_TRY(hipGetLastError());
  }
  if (want_stream) {
    mchap::ExactModeParams MP;
    MP.e = E;
    MP.mode_alleles = out->mode_alleles ? out->mode_alleles : reinterpret_cast<int64_t *>(ws + cv.mode);
    MP.mode_llk = out->mode_llk;
    MP.mode_prob = out->mode_prob;
    MP.total = reinterpret_cast<double *>(ws + cv.total);
    hipLaunchKernelGGL(mchap::exact_mode_kernel, dim3(n_units), dim3(64), 0, stream, MP);
    HIP_TRY(hipGetLastError());
    if (want_second) {
      // second pass over the genotypes (the reference's own structure: no per-genotype array is kept)
      const int threads = mchap::EXACT_THREADS;
      const size_t lds2 = cached ? (size_t)(2 * E.H + 1) * (threads / 64) * 8 : mchap::exact_pass2_lds(rows, E.H, E.K, threads);
      if (lds2 > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_reads x n_haps = %d x %d: the frequency pass does not fit the LDS", n_reads, n_haps);
      mchap::ExactParams E2 = E;
      E2.llk32 = nullptr;
      E2.llk64 = nullptr;
      E2.unit_total = MP.total;
      E2.unit_mode = MP.mode_alleles;
      E2.part_freq = reinterpret_cast<double *>(ws + cv.part_freq);
      constexpr int KX2 = mchap::EXACT_KMAX;
      auto k2 = E.K <= 8 ? (cached ? mchap::exact_pass2_kernel<false, true, 8> : tiled ? mchap::exact_pass2_kernel<true, false, 8> : mchap::exact_pass2_kernel<false, false, 8>)
                         : (cached ? mchap::exact_pass2_kernel<false, true, KX2> : tiled ? mchap::exact_pass2_kernel<true, false, KX2> : mchap::exact_pass2_kernel<false, false, KX2>);
      if (lds2 > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
      hipLaunchKernelGGL(k2, dim3(nblk, n_units), dim3(threads), lds2, stream, E2);
      HIP_TRY(hipGetLastError());
      mchap::ExactFreqParams FP;
      FP.part_freq = E2.part_freq;
      FP.nblk = nblk;
      FP.H = n_haps;
      FP.K = ploidy;
      FP.support_prob = out->support_prob;
      FP.freqs_out = out->freqs;
      FP.occur_out = out->occur;
      hipLaunchKernelGGL(mchap::exact_freq_kernel, dim3(n_units), dim3(64), 0, stream, FP);
      HIP_TRY(hipGetLastError());
    }
  }
  if (out->posteriors) {
    mchap::ExactArrayParams A;
    std::memset(&A, 0, sizeof(A));
    A.llk32 = out->llks;
    A.post = out->posteriors;
    A.G = G;
    A.K = ploidy;
    A.H = n_haps;
    A.has_prior = has_prior;
    A.inbreeding = inbreeding;
    A.freqs = has_prior ? frequencies : nullptr;
    A.mode_alleles = out->arr_mode_alleles;
    A.mode_prob = out->arr_mode_prob;
    A.support_prob = out->arr_support_prob;
    A.afreq = out->arr_freqs;
    A.acount = out->arr_counts;
    A.aoccur = out->arr_occur;
    rc = launch_exact_array(A, n_units, stream);
    if (rc) return rc;
  }
  return MCHAP_OK;
}

int mchap_exact_posterior_summaries_batch_device(int n_units, const double *posteriors, int64_t n_genotypes, int ploidy,
                                                 int n_alleles, int64_t *mode_alleles, double *mode_prob, double *support_prob,
                                                 double *freqs, double *counts, double *occur, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!posteriors) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_genotypes != host_cwr(n_alleles, ploidy)) return fail(MCHAP_ERR_BAD_ARG, "len(posteriors) != C(n_alleles+ploidy-1, ploidy)");
  int rc = ensure_init();
  if (rc) return rc;
  mchap::ExactArrayParams A;
  std::memset(&A, 0, sizeof(A));
  A.post_in = posteriors;
  A.G = n_genotypes;
  A.K = ploidy;
  A.H = n_alleles;
  A.mode_alleles = mode_alleles;
  A.mode_prob = mode_prob;
  A.support_prob = support_prob;
  A.afreq = freqs;
  A.acount = counts;
  A.aoccur = occur;
  return launch_exact_array(A, n_units, reinterpret_cast<hipStream_t>(stream_));
}

// ---- prior allele frequencies by EM over stored likelihoods: one iteration = the counts launch per shape group, then the update
// launch over the records ----
int64_t mchap_exact_em_workspace_bytes(int n_units, int n_haps, int ploidy) {
  if (n_units <= 0 || n_haps < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  if (!cwr_fits(n_haps, ploidy)) return -1;
  return (int64_t)up256((size_t)n_units * (size_t)exact_nblk(host_cwr(n_haps, ploidy)) * ((size_t)n_haps + 2) * 8);
}

int mchap_exact_em_counts_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                 const int32_t *unit_record, const int32_t *unit_slot, const double *frequencies, int stride,
                                 const int32_t *record_active, double *slab, void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !inbreeding || !unit_record || !unit_slot || !frequencies || !record_active || !slab)
    return fail(MCHAP_ERR_BAD_ARG, "frequency estimate: NULL buffer");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_haps < 1 || stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "frequency estimate: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = exact_nblk(G);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "frequency estimate: %d units x %d tiles exceed one launch", n_units, nblk);
  const int64_t need = mchap_exact_em_workspace_bytes(n_units, n_haps, ploidy);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %lld needed (mchap_exact_em_workspace_bytes)", (long long)workspace_bytes,
                (long long)need);
  const size_t lds = mchap::exact_em_lds(n_haps, ploidy);
  if (lds > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the frequency estimate's prior tables", n_haps);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactEmParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_record = unit_record;
  E.unit_slot = unit_slot;
  E.freqs = frequencies;
  E.active = record_active;
  E.stride = stride;
  E.H = n_haps; E.K = ploidy; E.nblk = nblk;
  E.G = G;
  E.part = reinterpret_cast<double *>(workspace);
  E.slab = slab;
  auto k = ploidy <= 8 ? mchap::exact_em_counts_kernel<8> : mchap::exact_em_counts_kernel<mchap::EXACT_KMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::exact_em_combine_kernel, dim3(n_units), dim3(64), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int mchap_exact_em_update_device(int n_records, int n_samples, const int32_t *record_haps, int stride, const double *slab,
                                 double ploidy_total, double tolerance, int max_iterations, double *frequencies,
                                 int32_t *record_iterations, int32_t *record_active, double *record_delta, void *stream_) {
  if (n_records <= 0) return MCHAP_OK;
  if (!record_haps || !slab || !frequencies || !record_iterations || !record_active) return fail(MCHAP_ERR_BAD_ARG, "frequency update: NULL buffer");
  if (n_samples < 1 || stride < 1 || !(ploidy_total > 0.0)) return fail(MCHAP_ERR_BAD_ARG, "frequency update: no samples");
  int rc = ensure_init();
  if (rc) return rc;
  mchap::ExactEmUpdateParams U;
  U.slab = slab;
  U.record_haps = record_haps;
  U.n_samples = n_samples;
  U.stride = stride;
  U.max_iterations = max_iterations;
  U.ploidy_total = ploidy_total;
  U.tolerance = tolerance;
  U.freqs = frequencies;
  U.iterations = record_iterations;
  U.active = record_active;
  U.delta = record_delta;
  hipLaunchKernelGGL(mchap::exact_em_update_kernel, dim3(n_records), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_), U);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

// ---- model evidence over stored likelihoods: the tiles' launch, then the combine launch ----
int64_t mchap_exact_evidence_workspace_bytes(int n_units, int n_haps, int ploidy, int n_grid) {
  if (n_units <= 0 || n_haps < 1 || n_grid < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  if (!cwr_fits(n_haps, ploidy)) return -1;
  return (int64_t)up256((size_t)n_units * (size_t)exact_nblk(host_cwr(n_haps, ploidy)) * (size_t)n_grid * 2 * 8);
}

int mchap_exact_evidence_chunk(int n_haps, int ploidy, int n_grid) {
  if (n_haps < 1 || n_grid < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  return mchap::exact_ev_chunk(n_haps, ploidy, n_grid);
}

int mchap_exact_evidence_device(int n_units, const double *llks64, int n_haps, int ploidy, int n_grid, const double *inbreeding,
                                const int32_t *unit_row, const double *frequencies, int stride, double *evidence, void *workspace,
                                int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !evidence) return fail(MCHAP_ERR_BAD_ARG, "model evidence: NULL buffer");
  if (inbreeding && (!unit_row || !frequencies)) return fail(MCHAP_ERR_BAD_ARG, "model evidence: NULL buffer (a prior needs unit_row and frequencies)");
  if (n_grid < 1) return fail(MCHAP_ERR_BAD_ARG, "model evidence: n_grid = %d, at least one grid point is needed", n_grid);
  if (!inbreeding && n_grid != 1) return fail(MCHAP_ERR_BAD_ARG, "model evidence: the flat prior has one grid point, not %d", n_grid);
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_haps < 1 || (inbreeding && stride < n_haps))
    return fail(MCHAP_ERR_BAD_ARG, "model evidence: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = exact_nblk(G);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "model evidence: %d units x %d tiles exceed one launch", n_units, nblk);
  const int64_t need = mchap_exact_evidence_workspace_bytes(n_units, n_haps, ploidy, n_grid);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %lld needed (mchap_exact_evidence_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  // (the flat prior builds no table: its LDS is the staging tile's)
  const int chunk = inbreeding ? mchap::exact_ev_chunk(n_haps, ploidy, n_grid) : 1;
  if (chunk == 0) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the model evidence's prior tables", n_haps);
  const size_t lds = mchap::exact_ev_lds(inbreeding ? n_haps : 0, ploidy, chunk);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactEvParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_row = unit_row;
  E.freqs = frequencies;
  E.stride = stride;
  E.H = n_haps; E.K = ploidy; E.nblk = nblk;
  E.n_grid = n_grid;
  E.chunk = chunk;
  E.G = G;
  E.part = reinterpret_cast<double *>(workspace);
  E.evidence = evidence;
  auto k = ploidy <= 8 ? mchap::exact_evidence_kernel<8> : mchap::exact_evidence_kernel<mchap::EXACT_KMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::exact_evidence_combine_kernel, dim3(n_units), dim3(64), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

// ---- SNV genotype posteriors over stored likelihoods: the evidence launches at the unit's own F for the normaliser, then the
// tiles' launch and the combine launch ----
}  // extern "C"

namespace {
// carve of the caller's workspace: the evidence pass' partials, the normalisers, the tiles' fixed-point sums
struct SnvCarve {
  size_t ev = 0, norm = 0, part = 0, bytes = 0;
};
SnvCarve snv_carve(int n_units, int n_haps, int ploidy, int n_pos, int n_snv_alleles) {
  const size_t nb = (size_t)exact_nblk(host_cwr(n_haps, ploidy));
  const size_t S = (size_t)host_cwr(n_snv_alleles, ploidy);
  SnvCarve c;
  size_t o = 0;
  c.ev = o; o += up256((size_t)n_units * nb * 2 * 8);
  c.norm = o; o += up256((size_t)n_units * 8);
  c.part = o; o += up256((size_t)n_units * nb * (size_t)n_pos * S * 8);
  c.bytes = o;
  return c;
}
bool snv_shape(int n_haps, int ploidy, int n_pos, int n_snv_alleles) {
  return n_haps >= 1 && n_pos >= 1 && n_snv_alleles >= 1 && n_snv_alleles <= mchap::SNV_MAX_ALLELES && ploidy >= 1 &&
         ploidy <= MCHAP_MAX_PLOIDY_DENOVO;
}
}  // namespace

extern "C" {

int64_t mchap_exact_snv_workspace_bytes(int n_units, int n_haps, int ploidy, int n_pos, int n_snv_alleles) {
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO || !cwr_fits(n_haps, ploidy)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_units <= 0 || !snv_shape(n_haps, ploidy, n_pos, n_snv_alleles)) return 0;
  return (int64_t)snv_carve(n_units, n_haps, ploidy, n_pos, n_snv_alleles).bytes;
}

int mchap_exact_snv_chunk(int n_haps, int ploidy, int n_pos, int n_snv_alleles) {
  if (!snv_shape(n_haps, ploidy, n_pos, n_snv_alleles)) return 0;
  return mchap::exact_snv_chunk(n_haps, ploidy, (int)host_cwr(n_snv_alleles, ploidy), n_pos);
}

int mchap_exact_snv_posteriors_device(int n_units, const double *llks64, int n_haps, int ploidy, int n_pos, int n_snv_alleles,
                                      const double *inbreeding, const int32_t *unit_row, const double *frequencies, int stride,
                                      const int8_t *hap_alleles, double *snv_post, double *log_norm, void *workspace,
                                      int64_t workspace_bytes, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!llks64 || !unit_row || !hap_alleles || !snv_post) return fail(MCHAP_ERR_BAD_ARG, "SNV posteriors: NULL buffer");
  if (inbreeding && !frequencies) return fail(MCHAP_ERR_BAD_ARG, "SNV posteriors: NULL buffer (a prior needs frequencies)");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_haps < 1 || (inbreeding && stride < n_haps))
    return fail(MCHAP_ERR_BAD_ARG, "SNV posteriors: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (n_snv_alleles < 1 || n_snv_alleles > mchap::SNV_MAX_ALLELES)
    return fail(MCHAP_ERR_BAD_ARG, "SNV posteriors: n_snv_alleles = %d not in 1..%d", n_snv_alleles, mchap::SNV_MAX_ALLELES);
  if (n_pos < 1) return fail(MCHAP_ERR_BAD_ARG, "SNV posteriors: n_pos = %d, at least one SNV is needed", n_pos);
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", ploidy, n_haps);
  const long long G = host_cwr(n_haps, ploidy);
  const int nblk = exact_nblk(G);
  const int S = (int)host_cwr(n_snv_alleles, ploidy);
  if ((long long)n_units * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "SNV posteriors: %d units x %d tiles exceed one launch", n_units, nblk);
  const long long nx = ((long long)n_pos * S + mchap::EXACT_THREADS - 1) / mchap::EXACT_THREADS;
  if ((long long)n_units * nx > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "SNV posteriors: %d units x %d SNVs exceed one launch", n_units, n_pos);
  const SnvCarve cv = snv_carve(n_units, n_haps, ploidy, n_pos, n_snv_alleles);
  if (!workspace || workspace_bytes < (int64_t)cv.bytes)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %zu needed (mchap_exact_snv_workspace_bytes)",
                (long long)workspace_bytes, cv.bytes);
  const int chunk = mchap::exact_snv_chunk(n_haps, ploidy, S, n_pos);
  if (chunk == 0) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the SNV posteriors' prior tables", n_haps);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  double *norm = reinterpret_cast<double *>(ws + cv.norm);
  // first pass: the normaliser of every unit's posterior -- its model evidence at its own F (one grid point)
  int rc = mchap_exact_evidence_device(n_units, llks64, n_haps, ploidy, 1, inbreeding, unit_row, frequencies, stride, norm, ws + cv.ev,
                                       (int64_t)(cv.norm - cv.ev), stream_);
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  mchap::ExactSnvParams E;
  std::memset(&E, 0, sizeof(E));
  E.llk64 = llks64;
  E.inbreeding = inbreeding;
  E.unit_row = unit_row;
  E.freqs = frequencies;
  E.hap_alleles = hap_alleles;
  E.stride = stride;
  E.H = n_haps; E.K = ploidy; E.M = n_pos; E.A = n_snv_alleles; E.S = S; E.nblk = nblk;
  E.chunk = chunk;
  E.G = G;
  E.log_norm = norm;
  E.part = reinterpret_cast<unsigned long long *>(ws + cv.part);
  E.snv_post = snv_post;
  E.log_norm_out = log_norm;
  const size_t lds = mchap::exact_snv_lds(n_haps, ploidy, S, chunk);
  auto k = ploidy <= 8 ? mchap::exact_snv_kernel<8> : mchap::exact_snv_kernel<mchap::EXACT_KMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)((long long)n_units * nblk)), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::exact_snv_combine_kernel, dim3((unsigned)((long long)n_units * nx)), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

// ---- host-pointer forms: one device allocation, copies in, the device entry point, copies out ----
int mchap_exact_genotype_likelihoods(const double *reads, int n_reads, int n_pos, int max_allele,
                                     const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                     float *llks_out, double *llks64_out) {
  int rc = exact_check_shape(n_reads, n_pos, max_allele, n_haps, ploidy);
  if (rc) return rc;
  const long long G = host_cwr(n_haps, ploidy);
  const size_t nr = (size_t)n_reads * n_pos * max_allele;
  DevArena M;
  rc = M.reserve(nr * 8 + (size_t)n_reads * 8 + (size_t)n_haps * n_pos + (size_t)G * 12 + 8 * 256);
  if (rc) return rc;
  HostCall hc;
  MCHAP_TRY(hc.open());
  double *d_reads = M.take<double>(nr);
  int64_t *d_counts = read_counts ? M.take<int64_t>(n_reads) : nullptr;
  int8_t *d_haps = M.take<int8_t>((size_t)n_haps * n_pos);
  float *d_l32 = llks_out ? M.take<float>(G) : nullptr;
  double *d_l64 = llks64_out ? M.take<double>(G) : nullptr;
  MCHAP_TRY(hc.up(d_reads, reads, nr * 8));
  if (read_counts) MCHAP_TRY(hc.up(d_counts, read_counts, (size_t)n_reads * 8));
  MCHAP_TRY(hc.up(d_haps, haplotypes, (size_t)n_haps * n_pos));
  mchap_exact_out out;
  std::memset(&out, 0, sizeof(out));
  out.llks = d_l32;
  out.llks64 = d_l64;
  rc = mchap_exact_call_batch_device(1, d_reads, n_reads, n_pos, max_allele, d_counts, d_haps, n_haps, ploidy, 0, nullptr, nullptr, &out,
                                     nullptr, 0, hc.stream);
  if (rc) return rc;
  if (llks_out) MCHAP_TRY(hc.down(llks_out, d_l32, (size_t)G * 4));
  if (llks64_out) MCHAP_TRY(hc.down(llks64_out, d_l64, (size_t)G * 8));
  return hc.sync();
}

int mchap_exact_genotype_posteriors(const void *llks, int is_f32, int64_t n_genotypes, int ploidy, int n_alleles,
                                    int has_prior, double inbreeding, const double *frequencies, double *post_out) {
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_genotypes != host_cwr(n_alleles, ploidy)) return fail(MCHAP_ERR_BAD_ARG, "len(log_likelihoods) != C(n_alleles+ploidy-1, ploidy)");
  int rc = ensure_init();
  if (rc) return rc;
  const size_t esz = is_f32 ? 4 : 8;
  DevArena M;
  rc = M.reserve((size_t)n_genotypes * (esz + 8) + (size_t)n_alleles * 8 + 8 + 6 * 256);
  if (rc) return rc;
  HostCall hc;
  MCHAP_TRY(hc.open());
  unsigned char *d_l = M.take<unsigned char>((size_t)n_genotypes * esz);
  double *d_out = M.take<double>(n_genotypes);
  double *d_F = M.take<double>(1);
  double *d_f = (has_prior && frequencies) ? M.take<double>(n_alleles) : nullptr;
  MCHAP_TRY(hc.up(d_l, llks, (size_t)n_genotypes * esz));
  MCHAP_TRY(hc.up(d_F, &inbreeding, 8));
  if (d_f) MCHAP_TRY(hc.up(d_f, frequencies, (size_t)n_alleles * 8));
  mchap::ExactArrayParams A;
  std::memset(&A, 0, sizeof(A));
  A.llk32 = is_f32 ? reinterpret_cast<const float *>(d_l) : nullptr;
  A.llk64 = is_f32 ? nullptr : reinterpret_cast<const double *>(d_l);
  A.post = d_out;
  A.G = n_genotypes;
  A.K = ploidy;
  A.H = n_alleles;
  A.has_prior = has_prior;
  A.inbreeding = d_F;
  A.freqs = d_f;
  rc = launch_exact_array(A, 1, hc.stream);
  if (rc) return rc;
  MCHAP_TRY(hc.down(post_out, d_out, (size_t)n_genotypes * 8));
  return hc.sync();
}

int mchap_exact_posterior_summaries(const double *posteriors, int64_t n_genotypes, int ploidy, int n_alleles,
                                    int64_t *mode_alleles, double *mode_prob, double *support_prob, double *freqs,
                                    double *counts, double *occur) {
  if (!posteriors) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  DevArena M;
  int rc = M.reserve((size_t)n_genotypes * 8 + (size_t)(ploidy + 2 + 3 * n_alleles) * 8 + 8 * 256);
  if (rc) return rc;
  HostCall hc;
  MCHAP_TRY(hc.open());
  double *d_p = M.take<double>(n_genotypes);
  int64_t *d_ma = M.take<int64_t>(ploidy);
  double *d_mp = M.take<double>(1), *d_sp = M.take<double>(1);
  double *d_fr = M.take<double>(n_alleles), *d_cn = M.take<double>(n_alleles), *d_oc = M.take<double>(n_alleles);
  MCHAP_TRY(hc.up(d_p, posteriors, (size_t)n_genotypes * 8));
  rc = mchap_exact_posterior_summaries_batch_device(1, d_p, n_genotypes, ploidy, n_alleles, d_ma, d_mp, d_sp, d_fr, d_cn, d_oc, hc.stream);
  if (rc) return rc;
  if (mode_alleles) MCHAP_TRY(hc.down(mode_alleles, d_ma, (size_t)ploidy * 8));
  if (mode_prob) MCHAP_TRY(hc.down(mode_prob, d_mp, 8));
  if (support_prob) MCHAP_TRY(hc.down(support_prob, d_sp, 8));
  if (freqs) MCHAP_TRY(hc.down(freqs, d_fr, (size_t)n_alleles * 8));
  if (counts) MCHAP_TRY(hc.down(counts, d_cn, (size_t)n_alleles * 8));
  if (occur) MCHAP_TRY(hc.down(occur, d_oc, (size_t)n_alleles * 8));
  return hc.sync();
}

int mchap_exact_posterior_mode_batch(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                     const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                     int has_prior, const double *inbreeding, const double *frequencies,
                                     int64_t *mode_alleles, double *mode_llk, double *mode_prob, double *support_prob,
                                     double *freqs, double *occur) {
  if (n_units <= 0) return MCHAP_OK;
  int rc = exact_check_shape(n_reads, n_pos, max_allele, n_haps, ploidy);
  if (rc) return rc;
  if (has_prior && !inbreeding) return fail(MCHAP_ERR_BAD_ARG, "prior requested without inbreeding");
  const size_t U = (size_t)n_units, nr = U * n_reads * n_pos * max_allele;
  // (room for llk + log prior of every genotype between the two passes while that stays under 1 GiB)
  const int64_t wsb_cached = mchap_exact_workspace_bytes_cached(n_units, n_haps, ploidy);
  const int64_t wsb = wsb_cached <= ((int64_t)1 << 30) ? wsb_cached : mchap_exact_workspace_bytes(n_units, n_haps, ploidy);
  DevArena M;
  rc = M.reserve(nr * 8 + U * n_reads * 8 + U * n_haps * n_pos + U * 8 + 3 * U * n_haps * 8 + U * ploidy * 8 + 3 * U * 8 + (size_t)wsb + 16 * 256);
  if (rc) return rc;
  HostCall hc;
  MCHAP_TRY(hc.open());
  double *d_reads = M.take<double>(nr);
  int64_t *d_counts = read_counts ? M.take<int64_t>(U * n_reads) : nullptr;
  int8_t *d_haps = M.take<int8_t>(U * n_haps * n_pos);
  double *d_F = has_prior ? M.take<double>(U) : nullptr;
  double *d_fr = (has_prior && frequencies) ? M.take<double>(U * n_haps) : nullptr;
  mchap_exact_out out;
  std::memset(&out, 0, sizeof(out));
  out.mode_alleles = M.take<int64_t>(U * ploidy);
  out.mode_llk = M.take<double>(U);
  out.mode_prob = M.take<double>(U);
  if (support_prob) out.support_prob = M.take<double>(U);
  if (freqs) out.freqs = M.take<double>(U * n_haps);
  if (occur) out.occur = M.take<double>(U * n_haps);
  unsigned char *d_ws = M.take<unsigned char>((size_t)wsb);
  MCHAP_TRY(hc.up(d_reads, reads, nr * 8));
  if (read_counts) MCHAP_TRY(hc.up(d_counts, read_counts, U * n_reads * 8));
  MCHAP_TRY(hc.up(d_haps, haplotypes, U * n_haps * n_pos));
  if (d_F) MCHAP_TRY(hc.up(d_F, inbreeding, U * 8));
  if (d_fr) MCHAP_TRY(hc.up(d_fr, frequencies, U * n_haps * 8));
  rc = mchap_exact_call_batch_device(n_units, d_reads, n_reads, n_pos, max_allele, d_counts, d_haps, n_haps, ploidy, has_prior, d_F, d_fr, &out,
                                     d_ws, wsb, hc.stream);
  if (rc) return rc;
  MCHAP_TRY(hc.down(mode_alleles, out.mode_alleles, U * ploidy * 8));
  MCHAP_TRY(hc.down(mode_llk, out.mode_llk, U * 8));
  MCHAP_TRY(hc.down(mode_prob, out.mode_prob, U * 8));
  if (support_prob) MCHAP_TRY(hc.down(support_prob, out.support_prob, U * 8));
  if (freqs) MCHAP_TRY(hc.down(freqs, out.freqs, U * n_haps * 8));
  if (occur) MCHAP_TRY(hc.down(occur, out.occur, U * n_haps * 8));
  return hc.sync();
}

}  // extern "C"
