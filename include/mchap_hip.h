/*
 * mchap_hip.h -- C ABI of libmchap_hip.so: MI355X (gfx950) kernels for MCHap's per-locus
 * MCMC haplotype assembler and exact genotype caller.
 *
 * The reference (PlantandFoodResearch/MCHap v0.11.1) has no FFI layer: its operator
 * boundary is Python (paths relative to /root/reference/mchap/):
 *   - DenovoMCMC.fit(reads, read_counts, initial) -> GenotypeMultiTrace   assemble/mcmc.py:24-161
 *   - calling.exact.genotype_likelihoods / genotype_posteriors /
 *     posterior_mode / posterior_allele_frequencies                      calling/exact.py:156-369
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows
 * the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions: plain pointers and sizes, caller allocates every output, the library never
 * retains a pointer.  Return value 0 on success, negative MCHAP_ERR_* otherwise (see
 * mchap_last_error()).  `*_device` entry points take DEVICE pointers and a hipStream_t
 * (passed as void*), enqueue work and return without synchronising; the plain entry points
 * take HOST pointers and are synchronous.
 */
#ifndef MCHAP_HIP_H
#define MCHAP_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCHAP_MAX_TEMPS 16
#define MCHAP_MAX_PLOIDY 8   /* the fast de novo samplers (nibble-packed labels) and the one-word forms of the device posterior summary; reference has no limit */
#define MCHAP_MAX_PLOIDY_DENOVO 15  /* ... the de novo sampler: ploidies 9 to 15 run on the general lanes-over-chains kernel (packs of
                                       sixteen nibbles; a dose of 16 does not fit one), with two trace words per haplotype */
#define MCHAP_MAX_POS 126    /* SNVs per unit.  Up to 62 SNVs and 64 bits of sampled alleles per haplotype (1 bit per biallelic, 2 per
                                tri- / tetra-allelic, 3 beyond) the fast samplers run; wider units -- up to 126 SNVs and 128 bits -- run on
                                the lanes-over-chains sampler with 128-bit haplotype words and their traces hold TWO uint64 words per
                                haplotype (mchap_denovo_trace_words_per_haplotype).  The reference has no limit. */
#define MCHAP_MAX_ALLELE 8
#define MCHAP_MAX_READS 4096 /* rows per unit after de-duplication (kernels 3 and 5; kernels 1 and 2: 1024) */

enum {
  MCHAP_OK = 0,
  MCHAP_ERR_NAN_LLK = -1,   /* ValueError("Encountered log likelihood of nan"), assemble/mcmc.py:330-331 */
  MCHAP_ERR_BAD_ARG = -2,   /* AssertionError family: shapes, temperatures (assemble/mcmc.py:134,207,220,225-226) */
  MCHAP_ERR_BREAKS = -3,    /* ValueError("breaks must be smaller then n"), assemble/structural.py:49-50 */
  MCHAP_ERR_LIMIT = -4,     /* shape exceeds what the kernels support (ploidy, packed haplotype width, LDS) */
  MCHAP_ERR_HIP = -5,       /* HIP runtime failure */
  MCHAP_ERR_NO_DEVICE = -6
};

/* per-unit status written by the sampler kernel */
enum {
  MCHAP_UNIT_OK = 0,
  MCHAP_UNIT_ALL_FIXED = 1, /* every position fixed homozygous: constant trace, llk = NaN (assemble/mcmc.py:189-199) */
  MCHAP_UNIT_NAN_LLK = 2,
  MCHAP_UNIT_BREAKS = 3,
  MCHAP_UNIT_BAD_INITIAL = 4 /* initial.shape != (ploidy, n_het_base): AssertionError, assemble/mcmc.py:207 */
};

/* Measurement / test knobs of the sampler (optional: mchap_denovo_cfg.tuning == NULL selects every default).  Results never
 * depend on them -- every setting produces the same traces (tests/test_gpu_denovo.py runs the extremes) -- only the time does.
 * A zero field means "default". */
typedef struct mchap_denovo_tuning {
  int32_t cache_slots;   /* {tag, llk} entries per chain of the likelihood cache: a power of two in 64..65536 (default: what 4 GiB
                            over the batch's chains allow, 1024..65536) */
  int32_t flags;         /* 1: no mutation memo, 2: no interval memo, 4: no coded read table, 8: no product reuse,
                            16: no LDS base-product cache, 32: skip the phased sampler's table completion (timing only: with
                            pipe_stop), 64 (libmchap_hip_test.so only): the tables completed by denovo_fill_kernel, one lane per request,
                            128: units without information (all gaps) are evaluated like any other,
                            256: never the instantiation that evaluates the requests of shallow units (<= 64 reads) side by side,
                            512: no haplotype-product rows in the workspace for deep units (> 256 reads),
                            1024: table completion inside the exporting launch, 8192: no LDS front cache of a chain's likelihoods,
                            16384: a ladder's replicas on one wavefront, 32768: no completion memo across chunks, 65536: caches
                            cleared per call instead of epoch tags, 131072: one wavefront per chain in every coasting launch,
                            262144: a round's misses behind a sub-step known to move are evaluated as well, 524288: no decision
                            contexts per genotype for the phased sampler's resumed chains, 1048576: a logarithm per read even where
                            the read weights are 0 / 1 (else one per group of four reads: the log likelihoods then differ in the last
                            bits, the traces do not)
                            (DESIGN.md section 4 names each) */
  int32_t spec_group;    /* kernel 3: lanes per chain, 16 / 32 / 64 (default: the smallest the shape allows) */
  int32_t pipe_first;    /* kernel 5: MCMC steps before the first hand-over (default ploidy * n_pos / 10, clamped to 3..32) */
  int32_t pipe_resume;   /*           steps a handed-back chain runs before it is handed over again (default 8) */
  int32_t pipe_rounds;   /*           resume rounds + 1 before the rest runs to the end in kernel 3 (default 2 + 1; 1 = none) */
  int32_t pipe_max;      /*           cap of a launch's extension while a chain of the wave is unsettled (default 64) */
  int32_t pipe_parts;    /*           wavefronts per chain completing tables when the chains are few (default 8) */
  int32_t prep_lds_limit; /* bytes of table the prepare pass copies to LDS (default 8192) */
  int32_t pipe_stop;     /* n > 0: stop after the n-th coasting launch (traces incomplete: timing / inspection of the phases) */
  int32_t reserved[6];
} mchap_denovo_tuning;

/* The fields of the DenovoMCMC dataclass (assemble/mcmc.py:24-40) that are common to a batch. */
typedef struct mchap_denovo_cfg {
  int32_t steps;                            /* steps */
  int32_t chains;                           /* chains */
  int32_t n_temps;                          /* len(temperatures) */
  int32_t n_intervals;                      /* n_intervals, 0 == None */
  double temperatures[MCHAP_MAX_TEMPS];     /* ascending, last == 1.0 (assemble/mcmc.py:224-226) */
  double fix_homozygous;                    /* fix_homozygous */
  double p_recomb;                          /* recombination_step_probability */
  double p_partial_dosage;                  /* partial_dosage_step_probability */
  double p_dosage;                          /* dosage_step_probability */
  uint64_t seed;                            /* random_seed: Philox4x32-10 key */
  const double *break_table;                /* HOST pointer, [(max_pos+1) x max_pos]: row m = Beta(alpha,beta) CDF
                                               increments over m het bases (assemble/mcmc.py:429-452) */
  int32_t max_pos;                          /* leading dimension of break_table */
  int32_t llk_cache;                        /* llk_cache_threshold >= 0: 1 = cache likelihoods per chain, 0 = recompute */
  int32_t kernel;                           /* 0 = default (5 when the batch's shape allows, else 3, else 2), 2 = lanes over
                                               chains, 3 = speculative sub-steps with a group of lanes per chain, 5 = phased:
                                               kernel 3 for a chain's first steps, then its settled stretches one lane per
                                               MCMC step (single temperature, one ploidy per launch).  Identical results
                                               whichever runs.  (1 = wavefront per chain and 4 = settle/steady pipeline are
                                               earlier designs kept for the parity suite: libmchap_hip_test.so only.) */
  int32_t cache_epoch;                      /* 1 .. 2^31 - 2: a number no other fit on memory this fit's workspace may reuse has carried
                                               (the likelihood caches of packed genotypes are tagged with it instead of being
                                               cleared: what an earlier call left in the workspace never matches).  The Python
                                               host hands out ONE process-wide sequence to every library copy it has loaded
                                               (mchap_amd/_lib.py next_cache_epoch).  0: the library's own counter -- unique among
                                               the fits of one loaded copy of the library, which is what a C caller has */
  const mchap_denovo_tuning *tuning;        /* HOST pointer or NULL */
  void *timer;                              /* mchap_timer_create() handle or NULL: the sampler launches of this call are
                                               bracketed by HIP events on the call's stream (not the prepare pass) */
} mchap_denovo_cfg;

/* One unit = one (locus x sample) call of DenovoMCMC.fit.  Offsets are in ELEMENTS of the
 * corresponding batch buffer. */
typedef struct mchap_unit {
  int64_t reads_off;     /* into reads: this unit's float64 [n_reads][n_pos][max_allele] tensor, C order */
  int64_t counts_off;    /* into read_counts, or -1 == None */
  int64_t nalleles_off;  /* into n_alleles: int8 [n_pos] */
  int64_t initial_off;   /* into initial: int8 [chains][ploidy][n_het], or -1 == None */
  int64_t trace_off;     /* into trace_words: uint64 [chains][steps][ploidy] */
  int64_t llk_off;       /* into llks: float64 [chains][steps] */
  int64_t fixed_off;     /* into fixed_alleles: int8 [n_pos] */
  int32_t n_reads;
  int32_t n_pos;
  int32_t max_allele;
  int32_t ploidy;
  double inbreeding;     /* NaN == None (flat prior) */
  uint64_t stream_id;    /* RNG stream of the unit: results do not depend on batch order or sharding */
  int32_t initial_n_het; /* last dimension of the caller's `initial` array; the unit ends with MCHAP_UNIT_BAD_INITIAL
                            (nothing sampled, `initial` not read) unless it equals the number of non-fixed positions */
  int32_t reserved;
} mchap_unit;

/* Replaces DenovoMCMC.fit (assemble/mcmc.py:103-161) for a batch of units.
 *
 * Outputs per unit:
 *   trace_words  uint64 [chains][steps][ploidy]: the cold-chain genotype of every step with its haplotypes
 *                packed over the NON-fixed positions (position 0 most significant, `bits` bits per allele,
 *                bits = 1/2/3 for max_allele <= 2/4/8) and sorted ascending -- i.e. already in the
 *                canonical order GenotypeMultiTrace.__post_init__ produces (assemble/classes.py:265-278).
 *                A batch with a unit wider than the fast samplers take (MCHAP_MAX_POS above) holds W = 2 words per haplotype,
 *                uint64 [chains][steps][ploidy][2], most significant word first (W for a batch:
 *                mchap_denovo_trace_words_per_haplotype; the caller sizes trace_words and its trace_off by it).
 *   llks         float64 [chains][steps]  (assemble/mcmc.py:418-425)
 *   fixed_alleles int8 [n_pos]: -1 for sampled positions, else the allele fixed as homozygous
 *                (assemble/mcmc.py:168-182,251-265); together with trace_words this is the full trace.
 *   status       int32 per unit, MCHAP_UNIT_*.
 * All pointers are device pointers; `units` too.  `stream` is a hipStream_t. */
int mchap_denovo_fit_batch_device(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units_dev,
                                  const mchap_unit *units_host, const double *reads, const int64_t *read_counts,
                                  const int8_t *n_alleles, const int8_t *initial, uint64_t *trace_words,
                                  double *llks, int8_t *fixed_alleles, int32_t *status, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* The same with the compact input the reference's encoders start from (encoding/integer/transcode.py:16-77,
 * io/bam.py:251-289): `calls` int8 [n_reads][n_pos] per unit (allele index, < 0 = gap; mchap_unit.reads_off counts
 * ELEMENTS of this array), `quals` int16 of the same shape or NULL, and `qual_prob[q]` = probability that a call with
 * base quality q is correct, i.e. (1 - error_rate) * (1 - 10^(-q/10)), computed by the caller exactly as the
 * reference does (qual_prob[0] = 1 - error_rate is used for every call when quals == NULL; qualities beyond the
 * table use its last entry).  The probability tensor is formed on the device by the prepare pass: the called
 * allele gets p, the others (1 - p) / 3, a gap NaN, alleles >= n_alleles[j] zero.  5x fewer input bytes than the
 * float64 tensor; same traces.  Every shipped sampler takes it (kernels 2, 3 and the phased sampler 5: they share the prepare
 * pass); kernel 1 of the parity suite does not. */
int mchap_denovo_fit_batch_calls_device(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units_dev,
                                        const mchap_unit *units_host, const int8_t *calls, const int16_t *quals,
                                        const double *qual_prob, int qual_prob_len, const int64_t *read_counts,
                                        const int8_t *n_alleles, const int8_t *initial, uint64_t *trace_words,
                                        double *llks, int8_t *fixed_alleles, int32_t *status, void *workspace,
                                        int64_t workspace_bytes, void *stream);

/* Bytes of device workspace the sampler needs: per-chain likelihood caches (the counterpart of the reference's llk
 * cache, assemble/likelihood.py:151-305; results-neutral) and, for kernel 0/2, the transposed read tensors and
 * per-unit tables written by its prepare pass. */
int64_t mchap_denovo_workspace_bytes(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units_host);

/* Same with host pointers: allocates device buffers, copies, runs, synchronises, copies back. */
int mchap_denovo_fit_batch(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units,
                           const double *reads, int64_t reads_len, const int64_t *read_counts, int64_t counts_len,
                           const int8_t *n_alleles, int64_t nalleles_len, const int8_t *initial, int64_t initial_len,
                           uint64_t *trace_words, int64_t trace_len, double *llks, int64_t llks_len,
                           int8_t *fixed_alleles, int64_t fixed_len, int32_t *status);

/* Test hook: log_likelihood (assemble/likelihood.py:17-70) of n_genotypes genotypes of one unit.
 * Host pointers. genotypes int8 [n_genotypes][ploidy][n_pos]. */
int mchap_log_likelihood_batch(const double *reads, int n_reads, int n_pos, int max_allele,
                               const int64_t *read_counts, const int8_t *genotypes, int n_genotypes, int ploidy,
                               double *llks_out);

/* Test hook: the logarithm the likelihood kernels take of their per-read terms (csrc/read_log.hpp: < 1 ulp; 0 -> -inf,
 * negative or NaN -> NaN), for n arguments.  Host pointers. */
int mchap_read_log_batch(const double *x, int64_t n, double *out);
/* Test hook: the logarithm of the product of `group` (1..4) per-read terms as ONE logarithm -- mantissas multiplied, exponents
 * summed (csrc/read_log.hpp read_log_product) -- which is what the likelihood kernels take of a lane's reads where the read weights
 * are 0 / 1: out[i] for x[i * group .. i * group + group - 1].  Host pointers. */
int mchap_read_log_product_batch(const double *x, int64_t n, int group, double *out);
/* Test hook: the 64-lane sum every likelihood goes through (csrc/denovo_kernel.hpp wave_sum: the XOR butterfly's tree, its last
 * four steps through DPP row rotations): out[w] = sum of x[64 w .. 64 w + 63].  Host pointers. */
int mchap_wave_sum_batch(const double *x, int64_t n_waves, double *out);

/* Posterior summary of a batch of traces: replaces GenotypeMultiTrace.burn(n).posterior() and the
 * mode/support statistics the assemble program reads from it (assemble/classes.py:280-325,87-128,194-205;
 * application/assemble.py:144-157).  Device pointers.
 *   post_words  uint64 [n_units][max_states][ploidy_max]  distinct genotypes, probability descending
 *   post_counts int32  [n_units][max_states]              occurrences after burn-in over all chains
 *   post_n      int32  [n_units]                          number of distinct genotypes (may exceed max_states)
 *   mode_stats  float64 [n_units][2]                      (support probability SPM, mode genotype probability GPM)
 *   mode_index  int32  [n_units]                          rank (row of post_words when < max_states) of the mode genotype
 *                                                         of the mode support
 *   mode_words  uint64 [n_units][ploidy_max] or NULL      that genotype itself, whatever its rank
 *   mode_count  int32  [n_units] or NULL                  its occurrences
 * post_n < 0: more than 512 distinct genotypes -- the table overflowed: read the sign only.  A genotype beyond the table is not
 * indexed and counts again in every batch of 64 states it reappears in, so -post_n is an upper bound of the number of distinct
 * genotypes (at least that number, at most the states of the trace), not the number.  The per-state outputs then rank the first
 * 512 distinct genotypes alone, each with all its occurrences, and the mode_* outputs are not the summary's (fall back to the listed
 * form below, or to the trace).  A table that is exactly full (512 distinct genotypes) does not overflow: post_n = 512.
 * INT32_MIN: the unit's ploidy exceeds ploidy_max. */
int mchap_trace_posterior_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                       const uint64_t *trace_words, int max_states, int ploidy_max,
                                       uint64_t *post_words, int32_t *post_counts, int32_t *post_n,
                                       double *mode_stats, int32_t *mode_index, uint64_t *mode_words,
                                       int32_t *mode_count, void *stream);

/* The same summary for the few units of a batch whose chains visited more distinct genotypes than the batch call keeps
 * (post_n < 0: shallow or empty samples whose chains wander), with a table of `cap` states per unit instead of 512 --
 * up to mchap_trace_posterior_max_states(ploidy_max), what 160 KB of LDS hold; cap >= chains * (steps - burn) can never
 * overflow.  unit_list int32 [n_list] (device): the units; post_words uint64 [n_list][cap][ploidy_max] and post_counts
 * int32 [n_list][cap] are indexed by list position, the per-unit outputs (post_n, mode_*) by unit, overwriting the batch
 * call's values.  So the program never has to download a trace (assemble/classes.py:280-325 on the host). */
int mchap_trace_posterior_max_states(int ploidy_max);
int mchap_trace_posterior_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                        int burn, const uint64_t *trace_words, int cap, int ploidy_max, uint64_t *post_words,
                                        int32_t *post_counts, int32_t *post_n, double *mode_stats, int32_t *mode_index,
                                        uint64_t *mode_words, int32_t *mode_count, void *stream);

/* `mchap call`: the sampler's traces summarised on the device (round 5).  The traces of mchap_call_mcmc_batch_device -- int64
 * genotypes [U][chains][steps][ploidy], alleles ascending -- are states of `ploidy` words, so GenotypeAllelesMultiTrace.burn(n)
 * .posterior() and PosteriorGenotypeAllelesDistribution.mode(genotype_support=True) (calling/classes.py:180-196, 303-362) are
 * mchap_trace_posterior_batch_device / _listed_device above as they stand (units: ploidy and trace_off = u * chains * steps *
 * ploidy; post_words are allele indices), ploidy <= MCHAP_MAX_PLOIDY.  The calling classes' replicate_incongruence
 * (calling/classes.py:231-263) differs from the assembler's: chains whose mode support reaches the threshold are compared by their
 * mode GENOTYPES, and the code is 2 when those genotypes together hold more distinct alleles than the ploidy.  mci int32 [n_units]:
 * 0 / 1 / 2, -1 if a chain visited more distinct genotypes than the table holds (then the listed form with a larger table). */
int mchap_call_incongruence_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                         const int64_t *genotypes, int ploidy_max, double threshold, int32_t *mci, void *stream);
int mchap_call_incongruence_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                          int burn, const int64_t *genotypes, int cap, int ploidy_max, double threshold, int32_t *mci,
                                          void *stream);

/* Exact caller: replaces calling.exact.genotype_likelihoods (calling/exact.py:266-292): llks_out float32 [G] as the
 * reference stores them and / or llks64_out float64 [G] (the unrounded values), G = C(n_haps + ploidy - 1, ploidy) genotypes in
 * VCF order; either may be NULL.  Host pointers, one unit. */
int mchap_exact_genotype_likelihoods(const double *reads, int n_reads, int n_pos, int max_allele,
                                     const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                     float *llks_out, double *llks64_out);

/* Replaces calling.exact.genotype_posteriors (calling/exact.py:295-329) on a stored likelihood array (float32 as
 * genotype_likelihoods returns it, or float64): priors in VCF order, normalisation; float64 result array whose
 * values carry float32 precision when the input is float32, as in the reference.  Host pointers. */
int mchap_exact_genotype_posteriors(const void *llks, int is_f32, int64_t n_genotypes, int ploidy, int n_alleles,
                                    int has_prior, double inbreeding, const double *frequencies, double *post_out);

/* Replicate incongruence of every unit's chains (the MCI field of `mchap assemble`): replaces
 * GenotypeMultiTrace.replicate_incongruence(threshold) (assemble/classes.py:341-376) on the traces written by
 * mchap_denovo_fit_batch_device.  mci[u] = 0 none, 1 incongruence, 2 incongruence whose union of haplotypes is larger
 * than the first qualifying chain's support (putative CNV; the reference's `len(alleles[0])`, classes.py:371-375), -1 if a chain visited more distinct genotypes than the kernel keeps (512).  Device pointers. */
int mchap_trace_incongruence_batch_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                          const uint64_t *trace_words, int ploidy_max, double threshold, int32_t *mci,
                                          void *stream);

/* ... and for a list of units with a table of `cap` states per chain (mci[u] == -1 after the batch call), as
 * mchap_trace_posterior_listed_device; mci is indexed by unit. */
int mchap_trace_incongruence_listed_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                           int burn, const uint64_t *trace_words, int cap, int ploidy_max, double threshold, int32_t *mci,
                                           void *stream);

/* The four summaries above for traces of `words_per_haplotype` 64-bit words per haplotype: 1 (the entry points above), or 2 for a
 * batch that ran on the general sampler (mchap_denovo_trace_words_per_haplotype: units of more than 64 bits per haplotype, ploidies 9
 * to MCHAP_MAX_PLOIDY_DENOVO) -- round 5, so that no shape `assemble` samples needs its traces on the host.  A state is then
 * ploidy x 2 words (a haplotype's words adjacent, genotypes sorted by haplotype as the sampler writes them) and the rows of
 * post_words / mode_words hold ploidy_max x 2 words; a batch launch keeps min(512, mchap_trace_posterior_max_states_wph) states. */
int mchap_trace_posterior_batch_wph_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                           const uint64_t *trace_words, int max_states, int ploidy_max, int words_per_haplotype,
                                           uint64_t *post_words, int32_t *post_counts, int32_t *post_n,
                                           double *mode_stats, int32_t *mode_index, uint64_t *mode_words,
                                           int32_t *mode_count, void *stream);
int mchap_trace_posterior_max_states_wph(int ploidy_max, int words_per_haplotype);
int mchap_trace_posterior_listed_wph_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                            int burn, const uint64_t *trace_words, int cap, int ploidy_max, int words_per_haplotype,
                                            uint64_t *post_words, int32_t *post_counts, int32_t *post_n, double *mode_stats,
                                            int32_t *mode_index, uint64_t *mode_words, int32_t *mode_count, void *stream);
int mchap_trace_incongruence_batch_wph_device(int n_units, const mchap_unit *units_dev, int steps, int chains, int burn,
                                              const uint64_t *trace_words, int ploidy_max, int words_per_haplotype, double threshold,
                                              int32_t *mci, void *stream);
int mchap_trace_incongruence_listed_wph_device(int n_list, const int32_t *unit_list_dev, const mchap_unit *units_dev, int steps, int chains,
                                               int burn, const uint64_t *trace_words, int cap, int ploidy_max, int words_per_haplotype,
                                               double threshold, int32_t *mci, void *stream);


/* Exact caller for a batch of units that share (n_reads, n_pos, max_allele, n_haps, ploidy), everything resident on the
 * device: what application/call_exact.py:126-179 asks of calling/exact.py per sample, for all samples of a chunk of
 * loci at once.  Every output is optional (NULL = not wanted):
 *   streaming form, float64, no per-genotype array is formed (calling.exact.posterior_mode, exact.py:156-249: a pass
 *   over the genotypes for the normaliser and the mode, a second one for the frequencies):
 *     mode_alleles int64 [U][K], mode_llk / mode_prob / support_prob float64 [U], freqs / occur float64 [U][H]
 *   array form (genotype_likelihoods 266-292: float32 store; genotype_posteriors 295-329 on that float32 array, hence
 *   float32 arithmetic, float64 result) with G = C(H + K - 1, K) genotypes in VCF order:
 *     llks float32 [U][G], llks64 float64 [U][G] (the unrounded values), posteriors float64 [U][G]
 *   and what the caller derives from the posterior array (call_exact.py:142-159; exact.py:332-407): its first maximum
 *   (arr_mode_alleles / arr_mode_prob), the summed probability of the genotypes over the mode's alleles
 *   (arr_support_prob = alternate_dosage_posteriors(...).sum()), posterior_allele_frequencies (arr_freqs, arr_counts,
 *   arr_occur [U][H]).
 * prior: has_prior == 0 -> None; else inbreeding [U] and frequencies [U][H] or NULL.  `workspace` (device,
 * mchap_exact_workspace_bytes) is only needed for the streaming outputs.  Enqueues on `stream`, no synchronisation. */
typedef struct mchap_exact_out {
  int64_t *mode_alleles;
  double *mode_llk, *mode_prob, *support_prob, *freqs, *occur;
  float *llks;
  double *llks64;
  double *posteriors;
  int64_t *arr_mode_alleles;
  double *arr_mode_prob, *arr_support_prob, *arr_freqs, *arr_counts, *arr_occur;
} mchap_exact_out;
int64_t mchap_exact_workspace_bytes(int n_units, int n_haps, int ploidy);
/* ... plus room for llk + log prior of every genotype (U * G float64): the second pass of the streaming form (support,
 * frequencies, occurrence) then reads them back instead of forming every likelihood again (calling/exact.py:156-249 makes
 * both passes from scratch to keep its memory flat; on the device 54 264 genotypes are 434 KB per unit).  Same results;
 * a workspace of either size is accepted. */
int64_t mchap_exact_workspace_bytes_cached(int n_units, int n_haps, int ploidy);
int mchap_exact_call_batch_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                  const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy, int has_prior,
                                  const double *inbreeding, const double *frequencies, const mchap_exact_out *out,
                                  void *workspace, int64_t workspace_bytes, void *stream);

/* Prior allele frequencies by EM (call-exact --estimate-prior-frequencies): one iteration of
 *   f'[h] = sum_s K_s freqs_s(f)[h] / sum_s K_s
 * over the samples s of a record, freqs_s the mean posterior allele frequency of sample s under prior (F_s, f) -- what the
 * reference writes as INFO/AFP (application/baseclass.py:282-288) and reads back as --prior-frequencies.  The likelihoods do not
 * depend on f: they are formed once (mchap_exact_call_batch_device, llks64) and stay on the device; an iteration streams them.
 * Records, not units, carry the frequencies: frequencies [records][stride], record_active [records] (0: frozen, its units are
 * skipped), and a slab [records][n_samples][stride] that takes every unit's expected allele counts K_s * freqs_s.
 *
 * The counts launch, once per iteration for each shape group (n_haps, ploidy) of the sub-block: unit u reads llks64 [u][G],
 * inbreeding [u] and the row unit_record[u] of `frequencies`, and writes row unit_slot[u] of `slab` (unit_slot = record *
 * n_samples + sample index: the groups of a record whose samples differ in ploidy fill one record's rows).  Sums in fixed order,
 * no atomics: equal inputs give equal bits.  `workspace`: mchap_exact_em_workspace_bytes (-1: more than 2^62 genotypes).
 * Enqueues on `stream`, no synchronisation. */
int64_t mchap_exact_em_workspace_bytes(int n_units, int n_haps, int ploidy);
int mchap_exact_em_counts_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                 const int32_t *unit_record, const int32_t *unit_slot, const double *frequencies, int stride,
                                 const int32_t *record_active, double *slab, void *workspace, int64_t workspace_bytes, void *stream);
/* The update launch, once per iteration after the counts launches: for every active record the slab rows summed in sample order
 * and divided by ploidy_total = sum_s K_s into its row of `frequencies` (record_haps [records]: its number of haplotypes, at most
 * stride), max |f' - f| into record_delta (or NULL), record_iterations + 1, and record_active = 0 once the maximum is below
 * `tolerance` or the counter has reached max_iterations: the host only counts the active records now and then to stop launching.
 * A NaN in the new row (a sample of the record without a finite genotype) makes the maximum NaN, and NaN is not below `tolerance`:
 * such a record runs max_iterations and keeps its NaN row, as the host's definition does.
 * Enqueues on `stream`, no synchronisation. */
int mchap_exact_em_update_device(int n_records, int n_samples, const int32_t *record_haps, int stride, const double *slab,
                                 double ploidy_total, double tolerance, int max_iterations, double *frequencies,
                                 int32_t *record_iterations, int32_t *record_active, double *record_delta, void *stream);

/* Model evidence (call-exact --model-evidence): for every unit u and grid point n
 *   evidence[u][n] = log sum_g P(g | ploidy, F_un, f_u) * P(reads_u | g),
 * the normaliser of the unit's posterior under the calling prior with inbreeding F_un = inbreeding[u][n] and the frequencies of
 * row unit_row[u] of `frequencies` [rows][stride]: the multinomial for F = 0, the Dirichlet-multinomial with alpha = f (1 - F) / F
 * for F > 0, -inf for every genotype holding an allele of frequency 0.  These priors sum to 1 over the genotypes, so the values
 * compare across grid points and across ploidies.  inbreeding = NULL: the flat genotype prior, n_grid = 1, unit_row and
 * frequencies not read, evidence = logsumexp(llk) - log(G).  A unit without a finite genotype gives -inf.
 * llks64 [U][G]: the likelihoods mchap_exact_call_batch_device leaves (llks64).  Every F must lie in [0, 1): the array is on the
 * device, so that is the caller's duty (device.ExactModelEvidence checks its host copy), as for the estimate's inbreeding.
 * The prior tables of as many grid points as keep a workgroup within 64 KB of LDS are built together
 * (mchap_exact_evidence_chunk: that number, 0 where a single table exceeds 160 KB); the grid is worked in such chunks.
 * Sums in fixed order, no atomics: equal inputs give equal bits.  `workspace`: mchap_exact_evidence_workspace_bytes (-1: more than
 * 2^62 genotypes).  A ploidy above MCHAP_MAX_PLOIDY_DENOVO (the Python layer's MAX_PLOIDY_GENERAL) is MCHAP_ERR_LIMIT.  n_grid has
 * no upper bound: a chunk may hold more grid points than a workgroup has threads.  Enqueues on `stream`, no synchronisation. */
int64_t mchap_exact_evidence_workspace_bytes(int n_units, int n_haps, int ploidy, int n_grid);
int mchap_exact_evidence_chunk(int n_haps, int ploidy, int n_grid);
int mchap_exact_evidence_device(int n_units, const double *llks64, int n_haps, int ploidy, int n_grid, const double *inbreeding,
                                const int32_t *unit_row, const double *frequencies, int stride, double *evidence, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* SNV genotype posteriors (call-exact --snv-calls): for every unit u, SNV j and SNV genotype s
 *   snv_post[u][j][s] = sum_g p_u[g] [s_j(g) = s],   p_u[g] = exp(llk_u[g] + log prior_u[g] - log_norm[u]),
 * the unit's haplotype-genotype posterior under the calling prior (as the model evidence: inbreeding[u] and row unit_row[u] of
 * `frequencies`; inbreeding = NULL: the flat genotype prior, frequencies not read) added to the SNV genotype it implies.
 * hap_alleles [rows][n_haps][n_pos]: the SNV allele 0 .. n_snv_alleles - 1 (n_snv_alleles <= 4) of every haplotype at every SNV,
 * the row of a unit again unit_row[u]; s_j(g) is the rank in VCF order of the multiset of the SNV alleles of g's haplotypes among
 * the S = C(n_snv_alleles + ploidy - 1, ploidy) SNV genotypes.  VCF order nests, so an SNV with fewer alleles fills a prefix of its
 * row and the rest is exactly 0.  log_norm [U] (may be NULL): the normaliser, the unit's model evidence at its own F.  A unit
 * without a finite genotype gives NaN everywhere (log_norm -inf).
 * Two passes: the evidence launches for log_norm, then every p[g] is added as a 64-bit integer with 62 fraction bits (LDS integer
 * atomics, tiles summed as integers): equal inputs give equal bits whatever the order of the units, and an entry is off by less
 * than G * 2^-62 from the sum of the float64 terms.  The bins of as many SNVs as keep a workgroup within 64 KB of LDS are held
 * together (mchap_exact_snv_chunk: that number, a single SNV may take up to 160 KB, 0 where not even one fits); the SNVs are
 * worked in such chunks, so n_pos has no upper bound.  `workspace`: mchap_exact_snv_workspace_bytes (-1: a ploidy outside
 * 1..MCHAP_MAX_PLOIDY_DENOVO or more than 2^62 genotypes -- the call itself is MCHAP_ERR_LIMIT).  Every F must lie in [0, 1) and
 * every SNV allele in its range: the arrays are on the device, so that is the caller's duty (device.ExactSnvPosteriors checks its
 * host copies).  Enqueues on `stream`, no synchronisation. */
int64_t mchap_exact_snv_workspace_bytes(int n_units, int n_haps, int ploidy, int n_pos, int n_snv_alleles);
int mchap_exact_snv_chunk(int n_haps, int ploidy, int n_pos, int n_snv_alleles);
int mchap_exact_snv_posteriors_device(int n_units, const double *llks64, int n_haps, int ploidy, int n_pos, int n_snv_alleles,
                                      const double *inbreeding, const int32_t *unit_row, const double *frequencies, int stride,
                                      const int8_t *hap_alleles, double *snv_post, double *log_norm, void *workspace,
                                      int64_t workspace_bytes, void *stream);

/* Expected read depth of every haplotype (call-exact --allele-depths): for every unit u, read row r and haplotype h
 *   post[u][r][h] = sum_g p_u[g] c_h(g) P[r][h] / D(r, g),   D(r, g) = sum_h c_h(g) P[r][h],   depth[u][h] = sum_r w_r post[u][r][h],
 * p_u[g] = exp(llk_u[g] + log prior_u[g] - log_norm[u]) the unit's genotype posterior under the calling prior (as the SNV
 * posteriors: inbreeding[u] and row unit_row[u] of `frequencies`; inbreeding = NULL: the flat genotype prior, unit_row and
 * frequencies not read), c_h(g) the dosage of haplotype h in genotype g, P[r][h] the product over the non-NaN cells
 * reads[r][j][haplotypes[h][j]], w_r = read_counts[u][r] (NULL: 1).  A pair (g, r) contributes only where p[g] > 0 and w_r > 0,
 * and 0 where D is 0 nevertheless; a row of weight 0 is exactly 0.  reads [U][n_reads][n_pos][max_allele], read_counts
 * [U][n_reads], haplotypes [U][n_haps][n_pos] and llks64 [U][G] are what mchap_exact_call_batch_device took and left.
 * depth [U][n_haps]; read_post [U][n_reads][n_haps] (may be NULL: the rows are then summed inside the workgroups and the
 * workspace is n_reads times smaller); log_norm [U] (may be NULL): the normaliser, the unit's model evidence at its own F.  A unit
 * without a finite genotype gives NaN everywhere (log_norm -inf).
 * Two passes: the evidence launches for log_norm, then one workgroup per (unit, tile of 4096 genotypes) walks the genotypes with
 * p > 0 with one lane per read row, every accumulator cell owned by one lane; the tiles are summed in tile order.  Equal inputs
 * give equal bits whatever the order of the units.  The read rows are worked in tiles of mchap_exact_support_tile rows (a multiple
 * of 64: as many as keep a workgroup within 64 KB of LDS, a single tile of 64 may take up to 160 KB; 0: not even that fits -- the
 * call is MCHAP_ERR_LIMIT), so n_reads has no upper bound.  `workspace`: mchap_exact_support_workspace_bytes (per_read: whether
 * read_post is asked for; -1: a ploidy outside 1..MCHAP_MAX_PLOIDY_DENOVO or more than 2^62 genotypes -- the call itself is
 * MCHAP_ERR_LIMIT).  Every F must lie in [0, 1): the arrays are on the device, so that is the caller's duty
 * (device.ExactReadSupport checks its host copy).  Enqueues on `stream`, no synchronisation. */
int64_t mchap_exact_support_workspace_bytes(int n_units, int n_reads, int n_haps, int ploidy, int per_read);
int mchap_exact_support_tile(int n_reads, int n_haps, int ploidy);
int mchap_exact_allele_support_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                      const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                      const double *llks64, const double *inbreeding, const int32_t *unit_row,
                                      const double *frequencies, int stride, double *depth, double *read_post, double *log_norm,
                                      void *workspace, int64_t workspace_bytes, void *stream);

/* Progeny calls under their parents' cross prior (call-exact --cross-calls).  Per record with n_haps haplotypes, parents P and Q of
 * even ploidies, gametes of t = ploidy / 2 haplotypes, progeny of ploidy t_P + t_Q; multisets in VCF order, like genotypes.
 *   gametes[u][a]  = (1 - e_u) (sum_{g = a + r} p_u[g] prod_h C(c_h(g), a_h)) / C(K, t) + e_u Mult(a; t, f),
 *   log_cross[r][gc] = log sum_{a in gc, |a| = t_P} gametes_p[r][a] gametes_q[r][gc - a],
 *   posterior[u][gc] = exp(llk_u[gc] + log_cross[unit_row[u]][gc] - log_z[u]).
 * p_u[g] = exp(llk_u[g] + log prior_u[g] - log_norm[u]) is the parent unit's genotype posterior under the calling prior (as the
 * SNV posteriors and the allele support: inbreeding[u] and row unit_row[u] of `frequencies`; inbreeding = NULL: the flat genotype
 * prior), c_h(g) the dosage of haplotype h in g and a_h that in a; the sum runs over the C(H + K - t - 1, K - t) complements r of a
 * in VCF order of r.  e_u = gamete_error[u] mixes in Mult, the multinomial pmf of a under f, the unit's row of `frequencies` --
 * always read, under the flat genotype prior too.  The cross sum runs over the distinct sub-multisets a of gc in VCF order of a;
 * an entry of log_cross is exactly -inf where every product is 0.  No double reduction; the two parents are independent tables.
 * gametes [U][C(H + t - 1, t)], log_norm [U] (may be NULL); a parent without a finite genotype gives NaN gametes (log_norm -inf),
 * NaN in its row of log_cross, and a NaN log_z.  gametes_p / gametes_q [rows][.] and log_cross [rows][G_c] are per record: every
 * progeny of the record shares the row.  The gamete tables of a row are staged in LDS where both fit 64 KB and read from global
 * memory otherwise: a large n_haps is slower, never refused.
 * The posterior call streams llks64 [U][G_c] + log_cross in tiles of 4096 genotypes, tiles combined in tile order: log_z [U] the
 * cross evidence, mode [U] the first maximum in VCF order (-1 where log_z is not finite: NaN, or -inf where no genotype has a
 * finite term), mode_prob [U] its probability (NaN then), posteriors [U][G_c] (may be NULL), and -- where log_norm is not NULL --
 * log_norm [U], the unit's evidence under its own calling prior (inbreeding, freq_row, frequencies, stride as
 * mchap_exact_evidence_device takes them), so that log_z - log_norm is the log Bayes factor of the cross against the population.
 * All three are gather-form: every output cell has one owning lane and a fixed summation order, no atomics; equal inputs give
 * equal bits whatever the order of the units.  `workspace`: the *_workspace_bytes of the call (the cross prior needs none; -1: a
 * ploidy outside 1..MCHAP_MAX_PLOIDY_DENOVO, an odd parent, or more than 2^62 genotypes -- the call itself is MCHAP_ERR_LIMIT, an
 * odd parent MCHAP_ERR_BAD_ARG).  Every F must lie in [0, 1) and every e in [0, 1]: the arrays are on the device, so that is the
 * caller's duty (device.ExactCross checks its host copies).  Enqueue on `stream`, no synchronisation. */
int64_t mchap_exact_gametes_workspace_bytes(int n_units, int n_haps, int ploidy);
int mchap_exact_gametes_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                               const int32_t *unit_row, const double *frequencies, int stride, const double *gamete_error,
                               double *gametes, double *log_norm, void *workspace, int64_t workspace_bytes, void *stream);
int64_t mchap_exact_cross_prior_workspace_bytes(int n_rows, int n_haps, int ploidy_p, int ploidy_q);
int mchap_exact_cross_prior_device(int n_rows, const double *gametes_p, const double *gametes_q, int n_haps, int ploidy_p,
                                   int ploidy_q, double *log_cross, void *stream);
int64_t mchap_exact_cross_posterior_workspace_bytes(int n_units, int n_haps, int ploidy);
int mchap_exact_cross_posterior_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *log_cross,
                                       const int32_t *unit_row, const double *inbreeding, const int32_t *freq_row,
                                       const double *frequencies, int stride, double *log_z, int64_t *mode, double *mode_prob,
                                       double *log_norm, double *posteriors, void *workspace, int64_t workspace_bytes,
                                       void *stream);

/* The parents and the progeny of one cross called jointly (call-exact --family-calls): the exact joint posterior of one nuclear
 * family per record.  n_records records of one shape -- n_haps haplotypes, parents P and Q of even ploidies, gametes of
 * t = ploidy / 2 haplotypes, n_progeny progeny of ploidy t_P + t_Q each; multisets in VCF order -- in one call:
 *   gamma_u(a | g) = (1 - e_u) prod_h C(c_h(g), a_h) / C(K_u, t_u) + e_u Mult(a; t_u, f),
 *   M_c[gP][gQ]    = sum_a sum_b gamma_P(a | gP) gamma_Q(b | gQ) exp(llk_c[rank(a + b)] - m_c),        m_c = max llk_c,
 *   w[gP][gQ]      = exp(lp_P[gP] + llk_P[gP] + lp_Q[gQ] + llk_Q[gQ] + sum_c (log M_c + m_c) - log_z_fam),
 *   post_p = sum_gQ w,  post_q = sum_gP w,
 *   q[c][gc]       = exp(llk_c[gc] - m_c) sum_{a in gc} (gamma_P^T (w / M_c) gamma_Q)[a][gc - a],
 *   pred_log_evidence[c] = m_c - log sum (w / M_c)     = log Z_fam - log Z_fam(without c).
 * lp_u is the log of the parent's calling prior: the flat genotype prior (inbreeding_u = NULL) or the Dirichlet-multinomial at
 * inbreeding_u[r] and row r of `frequencies` [n_records][stride]; that row is f of Mult too, always read.  gamete_error_u [n_records].
 * llks_p [R][G_P], llks_q [R][G_Q], llks_c [R][n_progeny][G_c]; progeny_reads int32 [R][n_progeny] (NULL: all 1): a progeny with
 * 0 has no reads -- its likelihoods are not read, it adds exactly nothing to the sum over c, its q is formed with w itself and its
 * pred_log_evidence is 0.  An entry of exp(llk_c - m_c) that underflows is 0; w / M_c is 0 where w is 0.  n_progeny = 0: post_p,
 * post_q are the parents' own calling posteriors.
 * Out: post_p [R][G_P], post_q [R][G_Q], their first maxima in VCF order mode_p, mode_q [R] and those probabilities; per progeny
 * q [R][n][G_c] (may be NULL), mode_c, mode_prob_c, pred_log_evidence [R][n]; log_z_fam [R].  A record whose log_z_fam is not
 * finite -- a parent or a progeny with reads that has no finite genotype, or Z_fam = 0, which needs a gamete error of 0 or a zero
 * frequency -- is null: log_z_fam NaN or -inf, every mode -1, every other output NaN; its neighbours are untouched.
 * Every stage is gather-form: one owning lane per output cell, a fixed summation order (sub-multisets in VCF order of a, then of
 * b; rows in row order), no atomics; equal inputs give equal bits whatever the place of a record in the call.  The one
 * [G_P][G_Q] array per record (the sum over c, then w) lives in `workspace`: mchap_exact_family_workspace_bytes (-1: a ploidy
 * outside 1..MCHAP_MAX_PLOIDY_DENOVO, an odd parent, 2^31 parent genotypes or more); a workspace smaller than that is
 * MCHAP_ERR_LIMIT -- nothing is allocated behind the caller's back.  A row of M_c and of w / M_c is kept in LDS where it fits 64 KB
 * and in the workspace otherwise (a second [G_P][G_Q] array); force_fallback != 0 takes the second path at any size (the workspace
 * is then the larger one).  Every F must lie in [0, 1) and every e in [0, 1]: the caller's duty (device.ExactFamily checks its host
 * copies).  Enqueue on `stream`, no synchronisation. */
int64_t mchap_exact_family_workspace_bytes(int n_records, int n_haps, int ploidy_p, int ploidy_q, int force_fallback);
int mchap_exact_family_device(int n_records, int n_progeny, const double *llks_p, const double *llks_q, const double *llks_c,
                              const int32_t *progeny_reads, int n_haps, int ploidy_p, int ploidy_q, const double *inbreeding_p,
                              const double *inbreeding_q, const double *frequencies, int stride, const double *gamete_error_p,
                              const double *gamete_error_q, double *post_p, int64_t *mode_p, double *mode_prob_p, double *post_q,
                              int64_t *mode_q, double *mode_prob_q, double *q, int64_t *mode_c, double *mode_prob_c,
                              double *pred_log_evidence, double *log_z_fam, void *workspace, int64_t workspace_bytes,
                              int force_fallback, void *stream);

/* Candidate parent pairs per progeny (call-exact --parentage): the cross evidence of every progeny of a record under every pair of
 * rows of two gamete tables, from one pass over the pairs of gametes.  n_records records of one shape -- n_haps haplotypes, n_a rows
 * of gametes of t_a haplotypes, n_b rows of gametes of t_b, n_progeny progeny of ploidy t_a + t_b each; multisets in VCF order:
 *   log_z[r][c][i][j] = m_c + log sum_a gametes_a[r][i][a] sum_b gametes_b[r][j][b] exp(llks_c[r][c][rank(a + b)] - m_c),  m_c = max llks_c[r][c].
 * The entry takes gamete SIZES, not ploidies: a row is any distribution over the gametes -- a candidate's row from
 * mchap_exact_gametes_device, or the unknown parent's Mult(a; t, f), which is what that entry returns at a gamete error of 1 and
 * which mchap_exact_parentage_population_device forms here with a small kernel of its own (the arithmetic of the gamete kernel's
 * multinomial, bit for bit; no likelihoods of a parent of ploidy 2t are needed): rows[r * row_pitch + a] = Mult(a; t, frequencies[r]),
 * so that it can be written into a row of a table.  gametes_a and gametes_b may be the same table.  For rows (i, j) from
 * mchap_exact_gametes_device at the parents' gamete errors, log_z is the log_z of mchap_exact_cross_posterior_device under the
 * cross prior of mchap_exact_cross_prior_device.
 * progeny_reads int32 [R][n_progeny] (NULL: all 1): a progeny with 0 has no reads -- its likelihoods are not read and every entry is
 * exactly 0.  A NaN row (a candidate without a finite genotype) makes its row or column of log_z NaN and nothing else; a progeny
 * with a NaN likelihood, or without a finite one, has NaN throughout; an entry whose every product is 0 is exactly -inf.
 * Gather form: one owning lane per output cell, no atomics.  One lane owns a gamete a and adds its terms over b in VCF order, one
 * after the other; the sum over a is taken by 256 lanes, lane l adding a = l, l + 256, ... in that order, then the wavefront's
 * butterfly (32, 16, 8, 4, 2, 1), then the four wavefronts in order.  Equal inputs give equal bits whatever the place of a record in
 * the call, and an entry's bits do not depend on how many other rows or progeny the call holds, on their order, or on the kernel's
 * chunks of 16 columns.  `workspace`: mchap_exact_parentage_workspace_bytes (the sums over b of every (progeny, column, gamete a));
 * -1, with the call itself MCHAP_ERR_LIMIT, for a gamete size outside 1..7, a progeny ploidy beyond MCHAP_MAX_PLOIDY_DENOVO, 2^62
 * genotypes or more, or n_haps x (t_a + t_b) rank terms beyond the LDS beside the staged rows (n_haps above about 16000 / (t_a +
 * t_b)).  A workspace smaller than asked is MCHAP_ERR_LIMIT: nothing is allocated behind the caller's back.  Any n_a, n_b >= 1.
 * Enqueue on `stream`, no synchronisation. */
int64_t mchap_exact_parentage_workspace_bytes(int n_records, int n_progeny, int n_a, int n_b, int n_haps, int t_a, int t_b);
int mchap_exact_parentage_device(int n_records, int n_progeny, int n_a, int n_b, const double *gametes_a, const double *gametes_b,
                                 const double *llks_c, const int32_t *progeny_reads, int n_haps, int t_a, int t_b, double *log_z,
                                 void *workspace, int64_t workspace_bytes, void *stream);
int mchap_exact_parentage_population_device(int n_records, const double *frequencies, int stride, int n_haps, int t, double *rows,
                                            int64_t row_pitch, void *stream);

/* Sample pairs by shared-genotype evidence (call-exact --identity): per record, for every pair (i, j) of n_samples samples of one
 * ploidy under one calling prior pi -- `inbreeding`: a HOST pointer to the one F in [0, 1) of the launch, read during the call, or
 * NULL for the flat prior; frequencies [n_records][stride], a device array, record r's row r (not read under the flat prior) --,
 * over llks64 [n_records][n_samples][G] as mchap_exact_call_batch_device leaves them and log_norm [n_records][n_samples], every
 * sample's model evidence under that prior (mchap_exact_evidence_device, one grid point):
 *   a_s[g]    = exp(llk_s[g] + log pi(g) / 2 - m_s),  m_s = max_g (llk_s[g] + log pi(g) / 2)       once per (record, sample)
 *   S_ij      = sum_g a_i[g] a_j[g]                         a sum below 1e-290 counts as 0
 *   lbf[r][i][j] = log((1 - error) r_ij + error),  log r_ij = log S_ij + (m_i - log_norm_i) + (m_j - log_norm_j)
 * the log Bayes factor of "one genotype read twice" against two independent draws from pi, error in [0, 1] the probability that the
 * genotypes are independent at this record all the same.  Both triangles are written, with equal bits, and the diagonal is NaN.
 * reads [n_records][n_samples] (or NULL: every sample has reads): the read weight of a (record, sample), 0 meaning no reads -- its
 * likelihoods are not read and its pairs are exactly 0.  A sample without a finite llk + log pi, or with a NaN, has NaN in its
 * row and column (also against a sample without reads).  S_ij = 0 gives log(error), -inf at error = 0.
 * The product is register-tiled (tiles of 64 x 64 pairs on or above the diagonal, 4 x 4 accumulators per thread) over chunks of the
 * genotype axis whose boundaries depend on G alone; a combine launch adds the chunks in order.  No atomics: equal inputs give equal
 * bits whatever the place of a record in the call and the number and order of the samples.  `workspace`:
 * mchap_exact_identity_workspace_bytes (log pi / 2 per record, the rows a, the chunks' partial sums); -1, with the call itself
 * MCHAP_ERR_LIMIT, for a ploidy beyond MCHAP_MAX_PLOIDY_DENOVO, 2^62 genotypes or more, or arrays of 2^61 bytes; with a prior the call
 * is MCHAP_ERR_LIMIT too where its tables exceed the LDS (mchap_exact_evidence_chunk = 0: the evidence launch refuses the shape as
 * well).  A workspace smaller than asked is MCHAP_ERR_LIMIT.  phases: 3 = the whole call; 1 = the launches that form log pi / 2 and
 * the rows a in the workspace, and no more; 2 = the product and combine launches over the rows a call with phases = 1 left in the
 * same workspace (same arguments) -- for a caller that times the two, or changes `error` alone.  Enqueue on `stream`, no
 * synchronisation. */
int64_t mchap_exact_identity_workspace_bytes(int n_records, int n_samples, int n_haps, int ploidy);
int mchap_exact_identity_device(int n_records, int n_samples, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                const double *frequencies, int stride, const double *log_norm, double error, const int32_t *reads,
                                double *lbf, int phases, void *workspace, int64_t workspace_bytes, void *stream);

/* Selfed parents per progeny (call-exact --parentage-selfings).  mchap_exact_selfing_prior_device: the inputs of
 * mchap_exact_gametes_device -- n_units candidate units of one shape (n_haps, even ploidy K, t = K / 2), llks64 [n_units][G],
 * inbreeding [n_units] or NULL for the flat prior, unit_row and frequencies [rows][stride], gamete_error [n_units] in [0, 1] --; out
 * log_self [n_units][G], self_prior [n_units][G] (or NULL) and log_norm [n_units] (or NULL): the genotype prior of a progeny of
 * ploidy K whose two gametes are two meioses of ONE genotype drawn from the unit's posterior p,
 *   S[gc] = sum_g p[g] sum_{a in gc, |a| = t} gamma(a | g) gamma(gc - a | g),  gamma(a | g) = (1 - e) hyp(a | g) + e Mult(a; t, f),
 * its logarithm (exactly -inf where every product is 0) and the unit's normaliser.  It is formed as
 *   ((1 - e)(1 - e)) (D[gc] / C(K, t)^2) + (e (1 - e)) E[gc] + (e e) Mult(gc; K, f)
 * with D the pairs (a, gc - a) summed over the genotypes that hold both, in VCF order of a and of the complement of their union, and E
 * the two mixed products of the error-free gamete table with Mult(.; t, f) -- never as the gamete table's product with itself plus a
 * correction.  One lane owns each cell and every sum has a fixed order: equal inputs give equal bits whatever the unit's place in
 * the batch.  A unit without a finite genotype has NaN throughout (log_norm as the gamete entry leaves it).  `workspace`:
 * mchap_exact_selfing_prior_workspace_bytes (the posteriors, the error-free gamete tables, the gamete entry's own); -1, with the call
 * itself MCHAP_ERR_LIMIT, for a ploidy beyond MCHAP_MAX_PLOIDY_DENOVO, 2^62 genotypes or more, or tables beyond 64 KB of LDS
 * (n_haps x ploidy above about 8000).
 *
 * mchap_exact_selfing_evidence_device: n_records records of one shape, n_candidates rows self_prior [n_records][n_candidates][G] (S, not
 * its logarithm), n_progeny progeny of ploidy K with llks_c [n_records][n_progeny][G]:
 *   log_z[r][c][i] = m_c + log sum_gc S[r][i][gc] exp(llks_c[r][c][gc] - m_c),  m_c = max llks_c[r][c]
 * each exp formed once per (progeny, genotype) for every candidate; per tile of 4096 genotypes a lane adds its 16 terms in order,
 * then the wavefront's butterfly, the four wavefronts in order, and the tiles in tile order.  progeny_reads [n_records][n_progeny]
 * (or NULL): 0 = no reads, the likelihoods are not read and the entries are exactly 0.  A NaN row of self_prior gives NaN in its
 * column alone; a NaN likelihood, or none that is finite, NaN throughout the progeny; a sum of 0 exactly -inf.  `workspace`:
 * mchap_exact_selfing_evidence_workspace_bytes, -1 (the call: MCHAP_ERR_LIMIT) for a refused shape; a workspace smaller than asked is
 * MCHAP_ERR_LIMIT.  Both enqueue on `stream`, no synchronisation, and allocate nothing. */
int64_t mchap_exact_selfing_prior_workspace_bytes(int n_units, int n_haps, int ploidy);
int mchap_exact_selfing_prior_device(int n_units, const double *llks64, int n_haps, int ploidy, const double *inbreeding,
                                     const int32_t *unit_row, const double *frequencies, int stride, const double *gamete_error,
                                     double *log_self, double *self_prior, double *log_norm, void *workspace,
                                     int64_t workspace_bytes, void *stream);
int64_t mchap_exact_selfing_evidence_workspace_bytes(int n_records, int n_progeny, int n_candidates, int n_haps, int ploidy);
int mchap_exact_selfing_evidence_device(int n_records, int n_progeny, int n_candidates, const double *self_prior, const double *llks_c,
                                        const int32_t *progeny_reads, int n_haps, int ploidy, double *log_z, void *workspace,
                                        int64_t workspace_bytes, void *stream);

/* Summaries of given posterior arrays [U][G] (calling.exact.posterior_allele_frequencies 332-369, the sum of
 * alternate_dosage_posteriors 372-407 for the array's mode): device pointers, any output may be NULL. */
int mchap_exact_posterior_summaries_batch_device(int n_units, const double *posteriors, int64_t n_genotypes, int ploidy,
                                                 int n_alleles, int64_t *mode_alleles, double *mode_prob, double *support_prob,
                                                 double *freqs, double *counts, double *occur, void *stream);
/* ... and for one array in host memory */
int mchap_exact_posterior_summaries(const double *posteriors, int64_t n_genotypes, int ploidy, int n_alleles,
                                    int64_t *mode_alleles, double *mode_prob, double *support_prob, double *freqs,
                                    double *counts, double *occur);

/* Exact caller, streaming form: replaces calling.exact.posterior_mode (calling/exact.py:156-249) for a batch
 * of units that share (n_reads, n_pos, max_allele, n_haps, ploidy).  Host pointers (one device allocation, copies,
 * mchap_exact_call_batch_device, copies back). */
int mchap_exact_posterior_mode_batch(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                     const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy,
                                     int has_prior, const double *inbreeding, const double *frequencies,
                                     int64_t *mode_alleles, double *mode_llk, double *mode_prob, double *support_prob,
                                     double *freqs, double *occur);

/* `mchap call`: Gibbs / Metropolis-Hastings sampler over the genotypes of known haplotypes for a batch of units that share
 * a shape: replaces CallingMCMC.fit (calling/classes.py:62-124) -> mcmc_sampler / compound_step / gibbs_options /
 * mh_options / greedy_caller (calling/mcmc.py:15-453) with the Gibbs-step priors of calling/prior.py:30-113.
 *   step_type 0 = "Gibbs", 1 = "Metropolis-Hastings"; initial int64 [U][K] or NULL (greedy_caller);
 *   stream_ids [U]: the unit's Philox stream (results do not depend on batch composition);
 *   genotypes int64 [U][chains][steps][K] (sorted alleles per step), llks float64 [U][chains][steps];
 *   status int32 [U]: 0, or MCHAP_ERR_LIMIT if a chain's table of remembered likelihoods filled up (cannot happen with a
 *   workspace of mchap_call_mcmc_workspace_bytes).
 * The workspace holds, per chain, the counterpart of the reference's llk dict (calling/likelihood.py:36-78), which never
 * forgets an entry.  Device pointers; enqueues on `stream`. */
int64_t mchap_call_mcmc_workspace_bytes(int n_units, int n_haps, int ploidy, int steps, int chains);
/* The same plus the chains' hand-over records (round 5: Gibbs steps at ploidies up to 8 -- a chain that has settled runs the
 * rest of its steps one lane of call_coast_kernel, csrc/call_mcmc_kernel.hpp; 2.2 KB a chain at 16 known haplotypes) and, when
 * n_reads x n_haps x 8 B exceeds the LDS, room for every chain's product table P[r][h] (the sampler then reads it from the
 * workspace: slower, but no limit on the read depth).  mchap_call_mcmc_batch_device needs this many bytes.  Environment
 * MCHAP_HIP_CALL_LANES (measurement): 0 = every chain on its own wavefront to the end, as before round 5; n = chains per
 * wavefront of call_coast_kernel.  The traces are the same either way. */
int64_t mchap_call_mcmc_workspace_bytes_for(int n_units, int n_reads, int n_haps, int ploidy, int steps, int chains);
/* Known haplotypes per unit.  Up to 256 the sampler above runs (call_mcmc_kernel: tables in LDS, Gibbs memo, coast hand-over).
 * Beyond, up to mchap_call_mcmc_max_haps(ploidy) -- 0 for a ploidy out of range --, call_wide_kernel
 * (csrc/call_wide_kernel.hpp) runs: the unit's product table P[r][h] and prior tables once per unit in the workspace
 * (mchap_call_mcmc_workspace_bytes_for counts them), a sub-step's options over the lanes, every lane its own likelihood in the
 * reference's order, no memo and no hand-over; the same results contract.  The bound is what the LDS holds of one chain's four
 * option arrays; more haplotypes are MCHAP_ERR_LIMIT with a message naming it.  Apart from it the genotype-count rule holds as
 * before: C(n_haps + ploidy - 1, ploidy) <= 2^62, else MCHAP_ERR_LIMIT (the table's keys are genotype ranks; 1024 haplotypes
 * pass it up to ploidy 7, 806 do at ploidy 8).  Environment (measurement and tests; the traces do not depend on them):
 * MCHAP_HIP_CALL_WIDE=1 runs call_wide_kernel whatever n_haps, MCHAP_HIP_CALL_WIDE_CHAINS=n puts at most n chains of a unit in
 * a workgroup.  On this path one call takes at most 65535 units (MCHAP_ERR_LIMIT beyond: cut the batch, as `mchap call` does).
 * Both functions above read MCHAP_HIP_CALL_WIDE too: size the workspace under the setting the call runs under. */
int mchap_call_mcmc_max_haps(int ploidy);
int mchap_call_mcmc_batch_device(int n_units, const double *reads, int n_reads, int n_pos, int max_allele,
                                 const int64_t *read_counts, const int8_t *haplotypes, int n_haps, int ploidy, int has_prior,
                                 const double *inbreeding, const double *frequencies, const int64_t *initial,
                                 const uint64_t *stream_ids, int steps, int chains, int step_type, uint64_t seed,
                                 int64_t *genotypes, double *llks, int32_t *status, void *workspace, int64_t workspace_bytes,
                                 void *stream);
/* the same with host pointers (one device allocation, copies, the device entry point, copies back) */
int mchap_call_mcmc_batch(int n_units, const double *reads, int n_reads, int n_pos, int max_allele, const int64_t *read_counts,
                          const int8_t *haplotypes, int n_haps, int ploidy, int has_prior, const double *inbreeding,
                          const double *frequencies, const int64_t *initial, const uint64_t *stream_ids, int steps, int chains,
                          int step_type, uint64_t seed, int64_t *genotypes, double *llks, int32_t *status);

/* The read tensors of a shape group of `mchap call` / `mchap call-exact` from int8 allele calls (mchap_amd/blockpath.py
 * call_unit_inputs builds the compact arrays): encoding.as_probabilistic / encode_read_distributions without base qualities, in
 * the same order.  Cell (u, r, j, a) with r < unit_rows[u] is p_call if a == call, else p_other; NaN for every a if call < 0;
 * 0.0 if a >= n_alleles[u][j] (applied last).  Rows r >= unit_rows[u] are NaN in every cell with count 0 (the programs' padding
 * of a group to its deepest unit).  The host passes p_call = 1 - error_rate and p_other = (1 - p_call) / 3 in float64; the device
 * does no arithmetic on them.  All pointers are device pointers (calls / counts may be NULL when no unit has a row); enqueues on
 * `stream`, does not synchronise.  Environment (measurement and tests; the tensor does not depend on it):
 * MCHAP_HIP_CALL_READS_WIDE=1 divides the cell index in 64 bits whatever the size (the default does below 2^32 cells in 32). */
int mchap_call_reads_from_calls_device(int n_units, const int8_t *calls, const int64_t *counts, const int64_t *unit_rows,
                                       const int64_t *unit_call_off, const int64_t *unit_count_off, const int8_t *n_alleles,
                                       int n_reads, int n_pos, int max_allele, double p_call, double p_other, double *reads,
                                       int64_t *read_counts, void *stream);

/* The same tensors with base qualities in use (--use-base-phred-scores): quals (int16, laid out like calls) holds every cell's
 * summed base quality, p_call / p_other two float64 tables of n_qual >= 1 entries the host computes as encoding.as_probabilistic
 * does: p_call[q] = prob_of_qual(q) * (1 - error_rate), p_other[q] = (1 - p_call[q]) / 3.  Cell (u, r, j, a) with r < unit_rows[u]
 * and call >= 0 is p_call[q] if a == call, else p_other[q], q the cell's quality (clamped into [0, n_qual): the host checks the
 * qualities of called cells before the upload; the quality of a gap cell is not read); everything else -- gaps, alleles a position
 * does not have, padding rows, counts, the environment variable -- as above.  The device does no arithmetic on the probabilities. */
int mchap_call_reads_from_calls_quals_device(int n_units, const int8_t *calls, const int16_t *quals, const int64_t *counts,
                                             const int64_t *unit_rows, const int64_t *unit_call_off, const int64_t *unit_count_off,
                                             const int8_t *n_alleles, int n_reads, int n_pos, int max_allele, const double *p_call,
                                             const double *p_other, int n_qual, double *reads, int64_t *read_counts, void *stream);

/* Measurement (bench.py): a timer is a pair of HIP events owned by the caller.  A fit whose cfg.timer is set records them on
 * its own stream right around its sampler launches; mchap_timer_ms waits for the second event and returns the span in
 * milliseconds (< 0: nothing recorded).  No process-wide state: fits on different threads / streams use different timers. */
int mchap_timer_create(void **timer);
double mchap_timer_ms(void *timer);
int mchap_timer_destroy(void *timer);
/* uint64 words per haplotype of this batch's trace_words: 1, or 2 when the batch holds a unit of more than 62 SNVs or more than
 * 64 bits of alleles per haplotype (a pure function of cfg and the units' shapes; < 0: the shapes are beyond the limits) */
int mchap_denovo_trace_words_per_haplotype(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units_host);
/* name of the sampler kernel(s) a fit of this batch dispatches to (a pure function of cfg and the units' shapes) */
int mchap_denovo_sampler_name(const mchap_denovo_cfg *cfg, int n_units, const mchap_unit *units_host, char *out, int out_len);

/* Host-side helpers of the programs' alignment reader (no GPU involved; the counterpart of the htslib records the reference's
 * io/bam.py:54-229 walks): the records of an INFLATED BAM payload `buf[0 .. n)` from byte `start` (just past the header, or a
 * region's first record) as columns.  mchap_bam_count: the complete records from `start` and the sum of their CIGAR operations.
 * mchap_bam_columns fills, per record: its byte offset, ref_id, pos, end (pos + reference bases its CIGAR consumes), mapq, flag,
 * byte offsets of its packed sequence and of its base qualities, the index of its RG:Z value among the `n_rg` NUL-separated
 * read-group ids `rg_ids` (-1: no such field / unknown id; the fields are walked in order as pysam's get_tag does), qname_id
 * = the index of the first record with the same query name; seg_first [n_records + 1] = first CIGAR operation of each
 * record among the flattened c_* arrays: record, operation code, length, reference / read coordinate at which it starts.
 * Returns MCHAP_OK, or MCHAP_ERR_BAD_ARG for a truncated / malformed record. */
int64_t mchap_bam_count(const uint8_t *buf, int64_t n, int64_t start, int64_t *n_cigar_ops);
int mchap_bam_columns(const uint8_t *buf, int64_t n, int64_t start, int64_t n_records, const char *rg_ids, int n_rg,
                      int64_t *offset, int32_t *ref_id, int32_t *pos, int64_t *end, int32_t *mapq, int32_t *flag,
                      int64_t *seq_off, int64_t *qual_off, int64_t *rg, int64_t *qname_id, int64_t *seg_first,
                      int64_t *c_rec, int64_t *c_op, int64_t *c_len, int64_t *c_ref0, int64_t *c_read0);

/* find-snvs pileup (reference application/find_snvs.py bam_region_depths / write_vcf_block; mchap_amd/find_snvs.py builds the
 * tables).  `bytes[0 .. n_bytes)`: the alignment records of a block, per sample one contiguous run, on the device; every offset
 * below indexes it (a sequence position as a nibble index: 2 x byte offset of the packed sequence + read offset).
 * mchap_pileup_overlap_device: htslib's mate-overlap rule on the quality bytes, in place.  segments [n_segments][4] int64 =
 *   {first mate's sequence nibble, second mate's sequence nibble, first mate's quality byte, second mate's quality byte} of a run
 *   of reference positions both mates align a base to; first [n_segments + 1] = the run's first position among n_positions.
 *   Equal bases: first q = min(q1 + q2, 200), second q = 0; else the higher (first on a tie) keeps (uint8)(0.8 q), the other 0.
 * mchap_pileup_depth_device: depth [n_rows][n_samples][4] int32 (A C G T) of the bases with quality >= min_base_quality.
 *   segments [*][4] int64 = {row, length, sequence nibble, quality byte} of an aligned run of one read, clipped to one target and
 *   one tile of `tile` (1..2048) rows; tile_first [n_samples x n_tiles + 1] = the CSR index of the segments of (sample, tile).
 *   variant 0: LDS histogram per (sample, tile), every row written; 1 (measurement): global atomics into a zeroed `depth`.
 * mchap_pileup_filter_device: per row, the reference's allele filter (maf, mad, ind_maf, ind_mad, min_ind) over `depth`;
 *   ref_index [n_rows] int8 (0-3, -1: not ACGT).  flags [n_rows]: bit 0 = a record, bits 1-4 = kept alleles, bits 8-15 = VCF
 *   order of the alleles (2 bits each, reference first), bit 16 = REFMASKED; admf [n_rows][4] float64 by allele index. */
int mchap_pileup_overlap_device(uint8_t *bytes, int64_t n_bytes, const int64_t *segments, const int64_t *first, int64_t n_segments,
                                int64_t n_positions, void *stream);
int mchap_pileup_depth_device(const uint8_t *bytes, int64_t n_bytes, const int64_t *segments, const int64_t *tile_first,
                              int n_samples, int64_t n_rows, int tile, int min_base_quality, int variant, int32_t *depth,
                              void *stream);
int mchap_pileup_filter_device(const int32_t *depth, const int8_t *ref_index, int64_t n_rows, int n_samples, double maf, int64_t mad,
                               double ind_maf, int64_t ind_mad, int64_t min_ind, int32_t *flags, double *admf, void *stream);

/* find-snvs genotype calls: per (row, sample) the posterior mode of the exact caller's model restricted to one position (reference
 * calling/exact.py posterior_mode over single-position reads), from the tensors the pileup launches leave: depth [n_rows][n_samples][4],
 * flags [n_rows] and admf [n_rows][4] as above.  A site is a row whose flag has bit 0; the record lists its reference allele and its
 * kept alternates in VCF order.  The ENUMERATED alleles are the listed ones, without the reference when the row is REFMASKED (a masked
 * reference is no candidate); m is their number, d_0 .. d_{m-1} the sample's depths on them (depth on other alleles is ignored).
 * For the sample's ploidy K (ploidy [n_samples] int32 on the device, 1..MCHAP_MAX_PLOIDY_DENOVO) the genotypes are the multisets of K
 * enumerated alleles in VCF genotype order, and
 *   llk(g)   = sum over a with d_a > 0 of d_a log((c_a p_call + (K - c_a) p_other) / K), c_a the dosage of a in g;
 *   prior(g) = flat over the genotypes when inbreeding[s] is NaN (inbreeding [n_samples] float64 on the device), else the reference's
 *              calling/prior.py log_genotype_prior(g, m, inbreeding[s], frequencies): frequencies none (use_admf = 0) or the row's
 *              admf over the enumerated alleles normalised to sum 1 (use_admf != 0; ignored for a sample whose inbreeding is NaN).
 * gt_index [n_rows][n_samples] int32: the index among the genotypes over the m enumerated alleles of the first maximum of llk + prior;
 * gpm [n_rows][n_samples] float64: its posterior probability exp(max - logsumexp) in float64.  gt_index = -1 and gpm = NaN for a row
 * that is no site, and for a NO-CALL: the sample has no depth on the enumerated alleles; frequencies are in use and an enumerated
 * allele's is 0 (AF0 of the call programs); no genotype has a likelihood above 0 (p_other = 0 and more alleles seen than K); an
 * inbreeding outside [0, 1).  Each pair is computed by one lane alone: two runs give the same bits.
 * Enqueues the launch on `stream` and does not wait for it; before that it reads the n_samples ploidies back (one wait on `stream`) to
 * size the launch and to refuse a ploidy above MCHAP_MAX_PLOIDY_DENOVO (MCHAP_ERR_LIMIT) or below 1 (MCHAP_ERR_BAD_ARG). */
int mchap_snv_genotypes_device(const int32_t *depth, const int32_t *flags, const double *admf, int64_t n_rows, int n_samples,
                               const int32_t *ploidy, const double *inbreeding, int use_admf, double p_call, double p_other,
                               int32_t *gt_index /*[n_rows][n_samples]*/, double *gpm /*[n_rows][n_samples]*/, void *stream);

/* Introspection */
const char *mchap_version(void);
const char *mchap_last_error(void);
int mchap_device_count(void);
/* bytes of LDS one block of the sampler needs for this shape, or <0 if unsupported */
int64_t mchap_denovo_lds_bytes(int n_reads, int n_pos, int max_allele, int ploidy, int chains, int n_temps);

#ifdef __cplusplus
}
#endif
#endif
