// libmchap_hip.so -- `mchap call`: the sampler over known haplotypes (call_mcmc_kernel.hpp; over more than CALL_MAX_HAPS of them
// call_wide_kernel.hpp, which call_wide_inst.hip launches).  Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "host_common.hpp"
#include "call_mcmc_kernel.hpp"
#include "call_wide_api.hpp"

using mchap::cwr_fits;
using mchap::DevArena;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::HostCall;

extern "C" {

// more than CALL_MAX_HAPS known haplotypes, or MCHAP_HIP_CALL_WIDE=1 (measurement and tests: any number)
static bool call_use_wide(int n_haps) {
  if (n_haps > mchap::CALL_MAX_HAPS) return true;
  const char *e = std::getenv("MCHAP_HIP_CALL_WIDE");
  return e && std::atoi(e) == 1;
}
int mchap_call_mcmc_max_haps(int ploidy) {
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return 0;
  return mchap_call_wide_max_haps();
}
static long long call_cache_slots(int n_haps, int ploidy, int steps) {
  if (!cwr_fits(n_haps, ploidy)) return 64;  // (more than 2^62 genotypes: the call refuses the shape by name; nothing to size)
  const long long G = host_cwr(n_haps, ploidy);
  long long need = (long long)steps * ploidy * n_haps + (long long)ploidy * n_haps + 8;  // requests of a chain at most
  if (G < need) need = G;
  long long slots = 64;
  while (slots < 2 * need) slots <<= 1;
  return slots;
}
int64_t mchap_call_mcmc_workspace_bytes(int n_units, int n_haps, int ploidy, int steps, int chains) {
  if (n_units <= 0 || n_haps < 1 || ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO || steps < 1 || chains < 1) return 0;
  return (int64_t)n_units * chains * call_cache_slots(n_haps, ploidy, steps) * 16;
}
// bytes of the product tables kept in the workspace when they do not fit the LDS (0 when they do)
static int64_t call_ext_bytes(int n_units, int n_reads, int n_haps, int ploidy, int chains) {
  if (mchap::call_lds_bytes(n_reads, n_haps, ploidy) <= 160 * 1024) return 0;
  return (int64_t)n_units * chains * ((int64_t)n_reads * n_haps + n_reads) * 8;
}
// the chains' hand-over records between call_mcmc_kernel and call_coast_kernel (Gibbs steps at ploidies whose memo key fits: <= 8)
static int64_t call_state_bytes(int n_units, int n_haps, int ploidy, int chains) {
  if (ploidy > 8 || n_haps > mchap::CALL_MAX_HAPS) return 0;
  return (((int64_t)n_units * chains * mchap::call_state_words(n_haps) * 8) + 255) & ~(int64_t)255;
}
int64_t mchap_call_mcmc_workspace_bytes_for(int n_units, int n_reads, int n_haps, int ploidy, int steps, int chains) {
  const int64_t base = mchap_call_mcmc_workspace_bytes(n_units, n_haps, ploidy, steps, chains);
  if (base == 0 || n_reads < 1) return base;
  // (many haplotypes: the unit's tables once per unit, no hand-over records, no per-chain product tables)
  if (call_use_wide(n_haps)) return ((base + 255) & ~(int64_t)255) + (int64_t)n_units * mchap_call_wide_unit_bytes(n_reads, n_haps, ploidy);
  return ((base + 255) & ~(int64_t)255) + call_state_bytes(n_units, n_haps, ploidy, chains) + call_ext_bytes(n_units, n_reads, n_haps, ploidy, chains);
}
// rounds of (settled chains a lane each, the chains that met a new context back on their wavefront) before the last launch runs
// whatever is left to its end
constexpr int CALL_ROUNDS = 3;

int mchap_call_mcmc_batch_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                 const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy, int has_prior,
                                 const double *inbreeding, const double *frequencies, const int64_t *initial,
                                 const uint64_t *stream_ids, int steps, int chains, int step_type, uint64_t seed,
                                 int64_t *genotypes, double *llks, int32_t *status, void *workspace, int64_t workspace_bytes,
                                 void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!reads || !haplotypes || !stream_ids || !genotypes || !llks || !status) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  if (step_type != 0 && step_type != 1) return fail(MCHAP_ERR_BAD_ARG, "MCMC step type must be 0 (Gibbs) or 1 (Metropolis-Hastings)");
  if (steps < 1 || chains < 1 || chains > 65535) return fail(MCHAP_ERR_BAD_ARG, "steps and chains must be >= 1");
  if (ploidy < 1 || ploidy > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "ploidy %d not in 1..%d", ploidy, MCHAP_MAX_PLOIDY_DENOVO);
  if (n_reads < 1 || n_pos < 1 || max_allele < 1 || n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "empty shape");
  if (n_haps > mchap_call_wide_max_haps())
    return fail(MCHAP_ERR_LIMIT, "n_haps %d > %d (mchap_call_mcmc_max_haps: a chain's option arrays must fit the LDS)", n_haps, mchap_call_wide_max_haps());
  if (!cwr_fits(n_haps, ploidy)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes (the keys of the sampler's likelihood table are their ranks)", ploidy, n_haps);
  if (has_prior && !inbreeding) return fail(MCHAP_ERR_BAD_ARG, "prior requested without inbreeding");
  if (call_use_wide(n_haps)) {
    // (units are the grid's y: mchap_hip.h names the bound, application.call keeps its sub-batches within it)
    if (n_units > 65535) return fail(MCHAP_ERR_LIMIT, "more than 65535 units in one call of the sampler over many haplotypes (n_haps %d > %d, or MCHAP_HIP_CALL_WIDE)", n_haps, mchap::CALL_MAX_HAPS);
    const int64_t base = mchap_call_mcmc_workspace_bytes(n_units, n_haps, ploidy, steps, chains);
    const int64_t need = mchap_call_mcmc_workspace_bytes_for(n_units, n_reads, n_haps, ploidy, steps, chains);
    if (!workspace || workspace_bytes < need)
      return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %lld needed (mchap_call_mcmc_workspace_bytes_for)", (long long)workspace_bytes, (long long)need);
    int rc = ensure_init();
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    HIP_TRY(hipMemsetAsync(workspace, 0, (size_t)base, stream));
    HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t) * n_units, stream));
    mchap::CallParams P;
    std::memset(&P, 0, sizeof(P));
    P.reads = reads;
    P.counts = read_counts;
    P.haps = haplotypes;
    P.inbreeding = has_prior ? inbreeding : nullptr;
    P.freqs = has_prior ? frequencies : nullptr;
    P.initial = initial;
    P.stream_ids = stream_ids;
    P.R = n_reads; P.M = n_pos; P.A = max_allele; P.H = n_haps; P.K = ploidy;
    P.has_prior = has_prior;
    P.step_type = step_type;
    P.steps = steps;
    P.chains = chains;
    P.seed = seed;
    P.cache = reinterpret_cast<ulonglong2 *>(workspace);
    P.cache_slots = call_cache_slots(n_haps, ploidy, steps);
    P.genotypes = genotypes;
    P.llks = llks;
    P.status = status;
    P.n_units = n_units;
    // (MCHAP_HIP_CALL_WIDE_CHAINS, tests: fewer chains of a unit per workgroup than the LDS holds -- the traces do not depend on it)
    const char *e = std::getenv("MCHAP_HIP_CALL_WIDE_CHAINS");
    const int wgc = mchap_call_wide_wg_chains(n_haps, chains, e ? std::atoi(e) : 0);
    double *unit_tab = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + ((base + 255) & ~(int64_t)255));
    const int e2 = mchap_call_wide_launch(&P, unit_tab, wgc, stream);
    if (e2) return fail(MCHAP_ERR_HIP, "call_wide_kernel: %s", hipGetErrorString((hipError_t)e2));
    return MCHAP_OK;
  }
  const int64_t ext = call_ext_bytes(n_units, n_reads, n_haps, ploidy, chains);
  // chains of a unit per workgroup (they share the unit's tables in LDS): as many as fit, one when the table is in the workspace
  int wgc = ext ? 1 : (chains < mchap::CALL_WG_CHAINS ? chains : mchap::CALL_WG_CHAINS);
  while (wgc > 1 && mchap::call_lds_bytes(n_reads, n_haps, ploidy, wgc) > 160 * 1024) wgc--;
  const size_t lds = mchap::call_lds_bytes(ext ? 0 : n_reads, n_haps, ploidy, wgc);
  if (lds > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_haps = %d: the sampler's tables do not fit the LDS", n_haps);
  const int64_t base = mchap_call_mcmc_workspace_bytes(n_units, n_haps, ploidy, steps, chains);
  const int64_t need = mchap_call_mcmc_workspace_bytes_for(n_units, n_reads, n_haps, ploidy, steps, chains);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_BAD_ARG, "workspace of %lld bytes is too small: %lld needed (mchap_call_mcmc_workspace_bytes_for)", (long long)workspace_bytes, (long long)need);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(workspace, 0, (size_t)base, stream));
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t) * n_units, stream));
  mchap::CallParams P;
  std::memset(&P, 0, sizeof(P));
  P.reads = reads;
  P.counts = read_counts;
  P.haps = haplotypes;
  P.inbreeding = has_prior ? inbreeding : nullptr;
  P.freqs = has_prior ? frequencies : nullptr;
  P.initial = initial;
  P.stream_ids = stream_ids;
  P.R = n_reads; P.M = n_pos; P.A = max_allele; P.H = n_haps; P.K = ploidy;
  P.has_prior = has_prior;
  P.step_type = step_type;
  P.steps = steps;
  P.chains = chains;
  P.seed = seed;
  P.cache = reinterpret_cast<ulonglong2 *>(workspace);
  P.cache_slots = call_cache_slots(n_haps, ploidy, steps);
  const int64_t state_bytes = call_state_bytes(n_units, n_haps, ploidy, chains);
  unsigned char *after_cache = reinterpret_cast<unsigned char *>(workspace) + ((base + 255) & ~(int64_t)255);
  P.ptab_ext = ext ? reinterpret_cast<double *>(after_cache + state_bytes) : nullptr;
  P.genotypes = genotypes;
  P.llks = llks;
  P.status = status;
  P.n_units = n_units;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ploidy <= 8 ? mchap::call_mcmc_kernel<8> : mchap::call_mcmc_kernel<mchap::EXACT_KMAX>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((chains + wgc - 1) / wgc, n_units), block(64 * wgc);
  // Settled chains run a lane each (call_coast_kernel): Gibbs steps whose memo key fits (ploidy <= 8), a memo that fits the LDS.
  // Lanes in use per wavefront: what the LDS holds of the chains' memos, and few enough that a small batch still spreads over the
  // chip -- a chain's step is a serial program and the launch lasts as long as one wavefront's chains (MCHAP_HIP_CALL_LANES: 0
  // turns the hand-over off, else the lanes)
  const int memo_words = mchap::CALL_MEMO + mchap::call_memo_entries(n_haps) * 2 * n_haps;
  const int lds_stride = memo_words | 1;
  int lanes = 0;
  const long long n_all = (long long)n_units * chains;
  if (step_type == 0 && state_bytes > 0 && mchap::call_memo_entries(n_haps) > 0) {
    const int fit = (int)((size_t)128 * 1024 / ((size_t)mchap::CALL_COAST_WAVES * lds_stride * 8));  // chains of a wavefront the LDS holds
    // (a workgroup per compute unit -- see coast_lds below -- and fewer workgroups than the chip's 256 compute units: a launch of
    // exactly 256 was measured to run in two turns, 18.9 against 12.0 ms at the bench shape)
    const long long slots = 200 * (long long)mchap::CALL_COAST_WAVES;
    lanes = (int)((n_all + slots - 1) / slots);
    if (lanes > fit) lanes = fit;
    if (lanes > 64) lanes = 64;
    // ... and only a batch whose chains do not all have a wavefront of their own at once: a lane's step (4 us) is not much
    // shorter than a wavefront's (10 us at ploidy 4) -- the coast kernel wins by holding many chains per wavefront, and costs a
    // small batch of chains that keep moving its rounds (150 units, 6 haplotypes, 60 reads: 20 ms on wavefronts alone, 56 ms
    // with three rounds of hand-overs)
    {
      const size_t per_cu = lds > 0 ? (size_t)(160 * 1024) / lds * (size_t)wgc : 8;
      const long long resident = 256ll * (long long)(per_cu < 8 ? per_cu : 8);
      if (n_all <= resident) lanes = 0;
    }
    if (const char *e = std::getenv("MCHAP_HIP_CALL_LANES")) {
      const int v = std::atoi(e);
      if (v == 0) lanes = 0;
      else if (v >= 1 && v <= 64 && v <= fit) lanes = v;
    }
  }
  auto launch = [&](int phase, int last) {
    P.phase = phase;
    P.last = last;
    // (ploidies 9 to 15: the instantiation with sixteen-entry genotype arrays -- round 5)
    if (ploidy <= 8) hipLaunchKernelGGL(mchap::call_mcmc_kernel<8>, grid, block, lds, stream, P);
    else hipLaunchKernelGGL(mchap::call_mcmc_kernel<mchap::EXACT_KMAX>, grid, block, lds, stream, P);
  };
  if (lanes == 0) {
    P.state = nullptr;
    launch(0, 1);
    HIP_TRY(hipGetLastError());
    return MCHAP_OK;
  }
  P.state = reinterpret_cast<uint64_t *>(after_cache);
  P.state_stride = mchap::call_state_words(n_haps);
  // (at least 81 KB a workgroup: one workgroup per compute unit, a wavefront per SIMD -- one wavefront's step keeps its SIMD busy, and
  // two workgroups sharing a compute unit while others idle were measured 1.5 times slower: 24.3 against 16.6 ms at the bench shape)
  size_t coast_lds = (size_t)mchap::CALL_COAST_WAVES * lanes * lds_stride * 8;
  if (coast_lds < 81 * 1024) coast_lds = 81 * 1024;
  // (the same bound whatever the shape: the attribute is the kernel's, and callers of different shapes on different threads would
  // otherwise lower it under each other's launches)
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mchap::call_coast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const long long per_wg = (long long)mchap::CALL_COAST_WAVES * lanes;
  const dim3 cgrid((unsigned)((n_all + per_wg - 1) / per_wg));
  launch(0, 0);
  for (int r = 0; r < CALL_ROUNDS; r++) {
    hipLaunchKernelGGL(mchap::call_coast_kernel, cgrid, dim3(64 * mchap::CALL_COAST_WAVES), coast_lds, stream, P, lanes, lds_stride);
    launch(1, r + 1 == CALL_ROUNDS);
  }
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int mchap_call_mcmc_batch(int n_units, const double *reads, int n_reads, int n_pos, int max_allele, const int64_t *read_counts,
                          const int8_t *haplotypes, int n_haps, int ploidy, int has_prior, const double *inbreeding,
                          const double *frequencies, const int64_t *initial, const uint64_t *stream_ids, int steps, int chains,
                          int step_type, uint64_t seed, int64_t *genotypes, double *llks, int32_t *status) {
  if (n_units <= 0) return MCHAP_OK;
  const size_t U = (size_t)n_units, nr = U * n_reads * n_pos * max_allele;
  const int64_t wsb = mchap_call_mcmc_workspace_bytes_for(n_units, n_reads, n_haps, ploidy, steps, chains);
  const size_t ng = U * chains * steps * ploidy, nl = U * chains * steps;
  DevArena M;
  int rc = M.reserve(nr * 8 + U * n_reads * 8 + U * n_haps * n_pos + U * 8 + U * n_haps * 8 + U * ploidy * 8 + U * 8 + ng * 8 + nl * 8 + U * 4 +
                     (size_t)wsb + 16 * 256);
  if (rc) return rc;
  HostCall hc;
  MCHAP_TRY(hc.open());
  double *d_reads = M.take<double>(nr);
  int64_t *d_counts = read_counts ? M.take<int64_t>(U * n_reads) : nullptr;
  int8_t *d_haps = M.take<int8_t>(U * n_haps * n_pos);
  double *d_F = has_prior ? M.take<double>(U) : nullptr;
  double *d_fr = (has_prior && frequencies) ? M.take<double>(U * n_haps) : nullptr;
  int64_t *d_ini = initial ? M.take<int64_t>(U * ploidy) : nullptr;
  uint64_t *d_sid = M.take<uint64_t>(U);
  int64_t *d_g = M.take<int64_t>(ng);
  double *d_l = M.take<double>(nl);
  int32_t *d_st = M.take<int32_t>(U);
  unsigned char *d_ws = M.take<unsigned char>((size_t)wsb);
  if (!d_ws) return fail(MCHAP_ERR_HIP, "device arena too small");
  MCHAP_TRY(hc.up(d_reads, reads, nr * 8));
  if (read_counts) MCHAP_TRY(hc.up(d_counts, read_counts, U * n_reads * 8));
  MCHAP_TRY(hc.up(d_haps, haplotypes, U * n_haps * n_pos));
  if (d_F) MCHAP_TRY(hc.up(d_F, inbreeding, U * 8));
  if (d_fr) MCHAP_TRY(hc.up(d_fr, frequencies, U * n_haps * 8));
  if (d_ini) MCHAP_TRY(hc.up(d_ini, initial, U * ploidy * 8));
  MCHAP_TRY(hc.up(d_sid, stream_ids, U * 8));
  rc = mchap_call_mcmc_batch_device(n_units, d_reads, n_reads, n_pos, max_allele, d_counts, d_haps, n_haps, ploidy, has_prior, d_F, d_fr, d_ini,
                                    d_sid, steps, chains, step_type, seed, d_g, d_l, d_st, d_ws, wsb, hc.stream);
  if (rc) return rc;
  MCHAP_TRY(hc.down(genotypes, d_g, ng * 8));
  MCHAP_TRY(hc.down(llks, d_l, nl * 8));
  MCHAP_TRY(hc.down(status, d_st, U * 4));
  return hc.sync();
}

}  // extern "C"
