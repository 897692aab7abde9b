// (included inside extern "C" of mchap_hip.hip)
namespace {
// One launch of trace_posterior_kernel: over all units (list == null: workgroup b = unit b, a table of POST_CAP states) or over a
// list of units with a table of `cap` states (per-state outputs by list position, per-unit outputs by unit).  wph: words per
// haplotype of the traces (1: the fast samplers; 2: the general sampler's 128-bit haplotypes, ploidies up to 15)
bool post_shape_ok(int ploidy_max, int wph) {
  return (wph == 1 && ploidy_max >= 1 && ploidy_max <= MCHAP_MAX_PLOIDY) || (wph == 2 && ploidy_max >= 1 && ploidy_max <= MCHAP_MAX_PLOIDY_DENOVO);
}
int post_sw(int wph) { return wph == 1 ? MCHAP_MAX_PLOIDY : mchap::POST_SW_WIDE; }
int launch_posterior(int n_blocks, const int32_t *list, const mchap_unit *units_dev, int steps, int chains, int burn,
                     const uint64_t *trace_words, int cap, int max_states, int ploidy_max, int wph, uint64_t *post_words, int32_t *post_counts,
                     int32_t *post_n, double *mode_stats, int32_t *mode_index, uint64_t *mode_words, int32_t *mode_count, void *stream_) {
  if (!units_dev || !trace_words || !post_words || !post_counts || !post_n || !mode_stats || !mode_index)
    return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  if (burn < 0 || burn >= steps) return fail(MCHAP_ERR_BAD_ARG, "burn must be in [0, steps)");
  if (!post_shape_ok(ploidy_max, wph)) return fail(MCHAP_ERR_LIMIT, "ploidy_max %d at %d word(s) per haplotype out of range", ploidy_max, wph);
  if (max_states < 1) return fail(MCHAP_ERR_BAD_ARG, "max_states must be >= 1");
  const int kw = ploidy_max * wph, sw = post_sw(wph);
  if (cap < 1 || cap > mchap::posterior_max_cap(kw, sw))
    return fail(MCHAP_ERR_LIMIT, "a table of %d states does not fit the LDS at ploidy %d (at most %d)", cap, ploidy_max, mchap::posterior_max_cap(kw, sw));
  int rc = ensure_init();
  if (rc) return rc;
  mchap::PosteriorParams P;
  P.units = units_dev;
  P.trace = trace_words;
  P.steps = steps;
  P.chains = chains;
  P.burn = burn;
  P.max_states = max_states;
  P.ploidy_max = ploidy_max;
  P.wph = wph;
  P.cap = cap;
  P.unit_list = list;
  P.post_words = post_words;
  P.post_counts = post_counts;
  P.post_n = post_n;
  P.mode_stats = mode_stats;
  P.mode_index = mode_index;
  P.mode_words = mode_words;
  P.mode_count = mode_count;
  const size_t lds = mchap::posterior_lds_bytes(kw, cap);
  const void *fn = wph == 1 ? reinterpret_cast<const void *>(mchap::trace_posterior_kernel<MCHAP_MAX_PLOIDY>)
                            : reinterpret_cast<const void *>(mchap::trace_posterior_kernel<mchap::POST_SW_WIDE>);
  if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (wph == 1) hipLaunchKernelGGL(mchap::trace_posterior_kernel<MCHAP_MAX_PLOIDY>, dim3(n_blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream_), P);
  else hipLaunchKernelGGL(mchap::trace_posterior_kernel<mchap::POST_SW_WIDE>, dim3(n_blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream_), P);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}
int launch_incongruence(int n_blocks, const int32_t *list, const mchap_unit *units_dev, int steps, int chains, int burn,
                        const uint64_t *trace_words, int cap, int ploidy_max, int wph, double threshold, int32_t *mci, void *stream_,
                        int calling = 0) {
  if (!units_dev || !trace_words || !mci) return fail(MCHAP_ERR_BAD_ARG, "NULL buffer");
  if (burn < 0 || burn >= steps) return fail(MCHAP_ERR_BAD_ARG, "burn must be in [0, steps)");
  if (!post_shape_ok(ploidy_max, wph)) return fail(MCHAP_ERR_LIMIT, "ploidy_max %d at %d word(s) per haplotype out of range", ploidy_max, wph);
  if (chains < 1 || chains > mchap::POST_MAX_CHAINS) return fail(MCHAP_ERR_LIMIT, "chains must be in 1..%d", mchap::POST_MAX_CHAINS);
  const int kw = ploidy_max * wph, sw = post_sw(wph);
  if (cap < 1 || cap > mchap::posterior_max_cap(kw, sw))
    return fail(MCHAP_ERR_LIMIT, "a table of %d states does not fit the LDS at ploidy %d (at most %d)", cap, ploidy_max, mchap::posterior_max_cap(kw, sw));
  int rc = ensure_init();
  if (rc) return rc;
  mchap::IncongruenceParams P;
  P.units = units_dev;
  P.trace = trace_words;
  P.steps = steps;
  P.chains = chains;
  P.burn = burn;
  P.threshold = threshold;
  P.ploidy_max = ploidy_max;
  P.wph = wph;
  P.calling = calling;
  P.cap = cap;
  P.unit_list = list;
  P.mci = mci;
  const size_t lds = mchap::incongruence_lds_bytes(kw, cap, sw);
  const void *fn = wph == 1 ? reinterpret_cast<const void *>(mchap::trace_incongruence_kernel<MCHAP_MAX_PLOIDY>)
                            : reinterpret_cast<const void *>(mchap::trace_incongruence_kernel<mchap::POST_SW_WIDE>);
  if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (wph == 1) hipLaunchKernelGGL(mchap::trace_incongruence_kernel<MCHAP_MAX_PLOIDY>, dim3(n_blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream_), P);
  else hipLaunchKernelGGL(mchap::trace_incongruence_kernel<mchap::POST_SW_WIDE>, dim3(n_blocks), dim3(64), lds, reinterpret_cast<hipStream_t>(stream_), P);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}
// states of a batch launch's table: POST_CAP, or what the LDS holds of wider states
int post_batch_cap(int ploidy_max, int wph) {
  const int m = mchap::posterior_max_cap(ploidy_max * wph, post_sw(wph));
  return m < mchap::POST_CAP ? m : mchap::POST_CAP;
}
}  // namespace

int mchap_trace_posterior_batch_wph_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                           const uint64_t *trace_words, int max_states, int ploidy_max, int words_per_haplotype,
                                           uint64_t *post_words, int32_t *post_counts, int32_t *post_n,
                                           double *mode_stats, int32_t *mode_index, uint64_t *mode_words,
                                           int32_t *mode_count, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!post_shape_ok(ploidy_max, words_per_haplotype)) return fail(MCHAP_ERR_LIMIT, "ploidy_max %d at %d word(s) per haplotype out of range", ploidy_max, words_per_haplotype);
  return launch_posterior(n_units, nullptr, units_dev, steps, chains, burn, trace_words, post_batch_cap(ploidy_max, words_per_haplotype), max_states,
                          ploidy_max, words_per_haplotype, post_words, post_counts, post_n, mode_stats, mode_index, mode_words, mode_count, stream_);
}
int mchap_trace_posterior_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                       const uint64_t *trace_words, int max_states, int ploidy_max,
                                       uint64_t *post_words, int32_t *post_counts, int32_t *post_n,
                                       double *mode_stats, int32_t *mode_index, uint64_t *mode_words,
                                       int32_t *mode_count, void *stream_) {
  return mchap_trace_posterior_batch_wph_device(n_units, units_dev, steps, chains, burn, trace_words, max_states, ploidy_max, 1, post_words,
                                                post_counts, post_n, mode_stats, mode_index, mode_words, mode_count, stream_);
}
int mchap_trace_incongruence_batch_wph_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                              const uint64_t *trace_words, int ploidy_max, int words_per_haplotype, double threshold,
                                              int32_t *mci, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  if (!post_shape_ok(ploidy_max, words_per_haplotype)) return fail(MCHAP_ERR_LIMIT, "ploidy_max %d at %d word(s) per haplotype out of range", ploidy_max, words_per_haplotype);
  return launch_incongruence(n_units, nullptr, units_dev, steps, chains, burn, trace_words, post_batch_cap(ploidy_max, words_per_haplotype), ploidy_max,
                             words_per_haplotype, threshold, mci, stream_);
}
int mchap_call_incongruence_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                         const int64_t *genotypes, int ploidy_max, double threshold, int32_t *mci, void *stream_) {
  if (n_units <= 0) return MCHAP_OK;
  return launch_incongruence(n_units, nullptr, units_dev, steps, chains, burn, reinterpret_cast<const uint64_t *>(genotypes),
                             post_batch_cap(ploidy_max, 1), ploidy_max, 1, threshold, mci, stream_, 1);
}
int mchap_call_incongruence_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                          int burn, const int64_t *genotypes, int cap, int ploidy_max, double threshold, int32_t *mci,
                                          void *stream_) {
  if (n_list <= 0) return MCHAP_OK;
  if (!unit_list_dev) return fail(MCHAP_ERR_BAD_ARG, "NULL unit list");
  return launch_incongruence(n_list, unit_list_dev, units_dev, steps, chains, burn, reinterpret_cast<const uint64_t *>(genotypes), cap,
                             ploidy_max, 1, threshold, mci, stream_, 1);
}
int mchap_trace_incongruence_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                          const uint64_t *trace_words, int ploidy_max, double threshold, int32_t *mci,
                                          void *stream_) {
  return mchap_trace_incongruence_batch_wph_device(n_units, units_dev, steps, chains, burn, trace_words, ploidy_max, 1, threshold, mci, stream_);
}
int mchap_trace_posterior_max_states_wph(int ploidy_max, int words_per_haplotype) {
  if (!post_shape_ok(ploidy_max, words_per_haplotype)) return 0;
  return mchap::posterior_max_cap(ploidy_max * words_per_haplotype, post_sw(words_per_haplotype));
}
int mchap_trace_posterior_max_states(int ploidy_max) { return mchap_trace_posterior_max_states_wph(ploidy_max, 1); }
int mchap_trace_posterior_listed_wph_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                            int burn, const uint64_t *trace_words, int cap, int ploidy_max, int words_per_haplotype,
                                            uint64_t *post_words, int32_t *post_counts, int32_t *post_n, double *mode_stats,
                                            int32_t *mode_index, uint64_t *mode_words, int32_t *mode_count, void *stream_) {
  if (n_list <= 0) return MCHAP_OK;
  if (!unit_list_dev) return fail(MCHAP_ERR_BAD_ARG, "NULL unit list");
  return launch_posterior(n_list, unit_list_dev, units_dev, steps, chains, burn, trace_words, cap, cap, ploidy_max, words_per_haplotype, post_words,
                          post_counts, post_n, mode_stats, mode_index, mode_words, mode_count, stream_);
}
int mchap_trace_posterior_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                        int burn, const uint64_t *trace_words, int cap, int ploidy_max, uint64_t *post_words,
                                        int32_t *post_counts, int32_t *post_n, double *mode_stats, int32_t *mode_index,
                                        uint64_t *mode_words, int32_t *mode_count, void *stream_) {
  return mchap_trace_posterior_listed_wph_device(n_list, unit_list_dev, units_dev, steps, chains, burn, trace_words, cap, ploidy_max, 1, post_words,
                                                 post_counts, post_n, mode_stats, mode_index, mode_words, mode_count, stream_);
}
int mchap_trace_incongruence_listed_wph_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                               int burn, const uint64_t *trace_words, int cap, int ploidy_max, int words_per_haplotype,
                                               double threshold, int32_t *mci, void *stream_) {
  if (n_list <= 0) return MCHAP_OK;
  if (!unit_list_dev) return fail(MCHAP_ERR_BAD_ARG, "NULL unit list");
  return launch_incongruence(n_list, unit_list_dev, units_dev, steps, chains, burn, trace_words, cap, ploidy_max, words_per_haplotype, threshold, mci, stream_);
}
int mchap_trace_incongruence_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                           int burn, const uint64_t *trace_words, int cap, int ploidy_max, double threshold, int32_t *mci,
                                           void *stream_) {
  return mchap_trace_incongruence_listed_wph_device(n_list, unit_list_dev, units_dev, steps, chains, burn, trace_words, cap, ploidy_max, 1, threshold, mci, stream_);
}
namespace {

long long host_cwr(int n, int k) {
  if (n <= 0) return 0;
  // (the product before the division in 128 bits: it passes 2^63 for counts near 2^62, which cwr_fits admits)
  unsigned __int128 r = 1;
  for (int d = 1; d <= k; d++) r = r * (unsigned __int128)(n - 1 + d) / (unsigned __int128)d;
  return (long long)r;
}

// C(n + k - 1, k) stays below 2^62 (the genotype indices and the call sampler's cache keys are int64; ploidy 15 over 200
// haplotypes would not)
bool cwr_fits(int n, int k) {
  if (n <= 0) return true;
  unsigned __int128 r = 1;
  for (int d = 1; d <= k; d++) {
    r = r * (unsigned __int128)(n - 1 + d) / (unsigned __int128)d;
    if (r >> 62) return false;
  }
  return true;
}

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

// ---- `mchap call`: sampler over known haplotypes ----
// the path for many haplotypes (call_wide_kernel.hpp, its own object: call_wide_inst.hip)
extern "C" int mchap_call_wide_max_haps(void);
extern "C" int64_t mchap_call_wide_unit_bytes(int n_reads, int n_haps, int ploidy);
extern "C" int mchap_call_wide_wg_chains(int n_haps, int chains, int forced);
extern "C" int mchap_call_wide_launch(const mchap::CallParams *P, double *unit_tab, int wgc, hipStream_t stream);
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
