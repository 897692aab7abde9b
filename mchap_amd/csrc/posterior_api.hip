// libmchap_hip.so -- summaries of the samplers' traces (posterior_kernel.hpp): the posterior distribution of a de novo trace and
// the incongruence of a trace of either sampler.  Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "posterior_kernel.hpp"

using mchap::ensure_init;
using mchap::fail;

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

extern "C" {

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

}  // extern "C"
