// The de novo samplers' common layer (gfx950): what two or more of the sampler kernels share -- the launch parameters
// (DenovoParams, SimtParams), the prepare pass's per-unit metadata, the hand-over record of the phased sampler, the constant
// log tables, the event counters of the profiling builds and the small device helpers on nibble packs, genotypes and staged
// draws.  No kernels: each kernel has a header of its own (denovo_mcmc_kernel.hpp, denovo_prepare_kernel.hpp,
// denovo_simt_kernel.hpp, denovo_spec_kernel.hpp, denovo_fillw_kernel.hpp, denovo_fill_kernel.hpp, denovo_lane_kernel.hpp,
// denovo_coast_kernel.hpp) that includes this one and the kernel headers it builds on.  What only one sampler uses stays with
// that sampler.  Reference citations as in denovo_mcmc_kernel.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mchap_hip.h"
#include "philox.hpp"
#include "read_log.hpp"
#include "wave_math.hpp"

namespace mchap {

constexpr uint32_t SLOT_INIT = 0xFFFFu;

// log(n), log(1/n) for small n, computed by the host's libm at library load.
static __constant__ double c_ln[260];      // per translation unit (the library is built from several)
static __constant__ double c_ln_inv[260];

struct DenovoParams {
  const mchap_unit *units;
  const double *reads;
  const int64_t *counts;
  const int8_t *n_alleles;
  const int8_t *initial;
  uint64_t *trace;
  double *llks;
  int8_t *fixed;
  int32_t *status;
  const double *break_table;  // device copy, [(max_pos+1)][max_pos]
  int max_pos;
  int steps, chains, n_temps, n_intervals;
  double temps[MCHAP_MAX_TEMPS];
  double fix_hom, p_recomb, p_partial, p_dosage;
  uint64_t seed;
  int rpad;  // 64 * RPL
  // optional per-chain likelihood cache in HBM/L2: [units*chains][cache_slots] of {tag, llk}; 0 slots = off
  uint64_t *cache;
  int cache_slots;  // power of two
  // genotypes wider than 63 bits are tagged by a hash; their full words [units*chains][cache_slots][cache_key_words]
  // are kept beside the entries and compared on every tag match, so a hit is always the genotype itself
  // (cache_key_words = the batch's largest ploidy; 0 when every unit's genotypes fit the tag)
  uint64_t *cache_keys;
  int cache_key_words;
  // compact input (kernels 2 / 3 only): int8 allele calls [R][M0] per unit instead of the float64 tensor, optional
  // int16 base qualities, and the probability of a correct call per quality (qual_prob[0] when there are none)
  const int8_t *calls;
  const int16_t *quals;
  const double *qual_prob;
  int qual_prob_len;
};

__host__ __device__ inline int align8(int x) { return (x + 7) & ~7; }

__host__ __device__ inline int snv_genotypes(int n_alleles, int ploidy) {
  // C(n + k - 1, k)
  long r = 1;
  for (int d = 1; d <= ploidy; d++) r = r * (n_alleles - 1 + d) / d;
  return (int)r;
}

__host__ __device__ inline int allele_bits(int A) { return A <= 2 ? 1 : (A <= 4 ? 2 : 3); }

// ---- small device helpers ------------------------------------------------------------------
__device__ __forceinline__ uint32_t nib(uint32_t p, int h) { return (p >> (4 * h)) & 15u; }
__device__ __forceinline__ uint32_t nib_set(uint32_t p, int h, uint32_t v) {
  return (p & ~(15u << (4 * h))) | (v << (4 * h));
}
// ... and packs of sixteen nibbles (ploidies 9 to 15: the general lanes-over-chains sampler, denovo_simt_kernel<0, u128>)
__device__ __forceinline__ uint32_t nib(uint64_t p, int h) { return (uint32_t)(p >> (4 * h)) & 15u; }
__device__ __forceinline__ uint64_t nib_set(uint64_t p, int h, uint32_t v) {
  return (p & ~(15ull << (4 * h))) | ((uint64_t)v << (4 * h));
}

// jitutils.py:77-92: searchsorted(cumsum(p), u, side="right")
__device__ __forceinline__ int choose_from(const double *p, int n, double u) {
  double c = 0.0;
  for (int i = 0; i < n; i++) {
    c += p[i];
    if (c > u) return i;
  }
  return n;
}

// first-occurrence dosage of the rows (in[h], out[h]) (jitutils.py:378-422 on label rows);
// a zero nibble marks a duplicate.
template <class P>
__device__ __forceinline__ P dosage_of_labels(P in, P out, int K, bool use_out) {
  P d = 0;
  for (int h = 0; h < K; h++) d |= (P)1 << (4 * h);
  for (int h = 0; h < K; h++) {
    if (nib(d, h) == 0) continue;
    for (int p = h + 1; p < K; p++) {
      if (nib(d, p) == 0) continue;
      if (nib(in, h) == nib(in, p) && (!use_out || nib(out, h) == nib(out, p))) {
        d += (P)1 << (4 * h);
        d &= ~((P)15 << (4 * p));
      }
    }
  }
  return d;
}

// structural.py:74-118
template <class P>
__device__ __forceinline__ int recombination_n_options(P in, P out, int K) {
  const P d = dosage_of_labels(in, out, K, true);
  int n = 0;
  for (int h0 = 0; h0 < K; h0++) {
    if (nib(d, h0) == 0) continue;
    for (int h1 = h0 + 1; h1 < K; h1++) {
      if (nib(d, h1) == 0) continue;
      if (nib(in, h0) == nib(in, h1) || nib(out, h0) == nib(out, h1)) continue;
      n++;
    }
  }
  return n;
}

// structural.py:181-237
template <class P>
__device__ __forceinline__ int dosage_n_options(P in, P out, int K) {
  const P hd = dosage_of_labels(in, out, K, true);
  const P sd = dosage_of_labels(in, out, K, false);
  int n = 0;
  for (int h0 = 0; h0 < K; h0++) {
    if (nib(hd, h0) == 0) continue;
    if (nib(sd, h0) == 1) continue;
    for (int h1 = 0; h1 < K; h1++) {
      if (nib(sd, h1) == 0) continue;
      if (nib(in, h0) == nib(in, h1)) continue;
      n++;
    }
  }
  return n;
}

// structural.py:121-178 / 240-307: option i = the `in` label pack after the move
__device__ inline int step_options(uint32_t in, uint32_t out, int K, int step_type, uint32_t *opt) {
  const uint32_t hd = dosage_of_labels(in, out, K, true);
  int n = 0;
  if (step_type == 0) {
    for (int h0 = 0; h0 < K; h0++) {
      if (nib(hd, h0) == 0) continue;
      for (int h1 = h0 + 1; h1 < K; h1++) {
        if (nib(hd, h1) == 0) continue;
        if (nib(in, h0) == nib(in, h1) || nib(out, h0) == nib(out, h1)) continue;
        uint32_t o = nib_set(in, h0, nib(in, h1));
        o = nib_set(o, h1, nib(in, h0));
        opt[n++] = o;
      }
    }
  } else {
    const uint32_t sd = dosage_of_labels(in, out, K, false);
    for (int h0 = 0; h0 < K; h0++) {
      if (nib(hd, h0) == 0) continue;
      if (nib(sd, h0) == 1) continue;
      for (int h1 = 0; h1 < K; h1++) {
        if (nib(sd, h1) == 0) continue;
        if (nib(in, h0) == nib(in, h1)) continue;
        opt[n++] = nib_set(in, h0, nib(in, h1));
      }
    }
  }
  return n;
}

// the 64-bit mix of the likelihood caches: the slot of a packed genotype, the tag of one wider than 63 bits
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// calling/prior.py:116-179 with frequencies=None, on a nibble-packed SNV genotype (snpcalling.py:55-60)
__device__ inline double snv_log_prior(uint32_t g, int K, int n_alleles, double F) {
  // allelic dosage, first-occurrence convention (calling/utils.py:7-35)
  int dose[MCHAP_MAX_PLOIDY];
  for (int i = 0; i < K; i++) dose[i] = 0;
  for (int i = 0; i < K; i++) {
    int j = 0;
    while (nib(g, i) != nib(g, j)) j++;
    dose[j] += 1;
  }
  if (F == 0.0) {
    double den = 0.0;
    for (int i = 0; i < K; i++) den += lgamma((double)dose[i] + 1.0);
    return (lgamma((double)K + 1.0) - den) - (double)K * c_ln[n_alleles];
  }
  const double alpha = (1.0 / (double)n_alleles) * ((1.0 - F) / F);
  const double sum_alphas = alpha * (double)n_alleles;
  const double left = (lgamma((double)K + 1.0) + lgamma(sum_alphas)) - lgamma((double)K + sum_alphas);
  double prod = 0.0;
  for (int i = 0; i < K; i++) {
    if (dose[i] > 0) prod += lgamma((double)dose[i] + alpha) - (lgamma((double)dose[i] + 1.0) + lgamma(alpha));
  }
  return left + prod;
}

// jitutils.py:114-146 on a nibble pack
template <class P>
__device__ inline P increment_snv_genotype(P g, int K) {
  if (K == 1) return g + 1;
  const uint32_t previous = nib(g, 0);
  for (int i = 1; i < K; i++) {
    const uint32_t allele = nib(g, i);
    if (allele == previous) continue;
    // allele > previous
    const int k = i - 1;
    g = nib_set(g, k, nib(g, k) + 1);
    for (int z = 0; z < k; z++) g = nib_set(g, z, 0);
    return g;
  }
  g = nib_set(g, K - 1, nib(g, K - 1) + 1);
  for (int z = 0; z < K - 1; z++) g = nib_set(g, z, 0);
  return g;
}

// ---- the prepare pass's workspace and the launch parameters of the samplers behind it ---------------------------
// per-unit metadata written by the prepare kernel
constexpr int META_I_MH = 0;      // number of sampled (non-fixed) positions
constexpr int META_I_STATUS = 1;  // MCHAP_UNIT_*
constexpr int META_I_NDICT = 2;   // distinct values of the unit's table (0: more than DICT_MAX, no coded table)
constexpr int META_I_FLAT = 3;    // 1: every entry of the unit's table (existing alleles) is a gap -- a sample without reads
                                  // at the locus, which the reference samples all the same (assemble/mcmc.py:132-137): the
                                  // likelihood of every genotype is then the same number
constexpr int META_I_W01 = 4;     // 1: every read weight of the unit is 0 or 1 (no counts of de-duplicated rows): the lanes take ONE
                                  // logarithm per group of up to four reads (read_log_sum, read_log.hpp); tuning flag 1048576: never
constexpr int META_I_COLS = 5;    // then [M]: column (j * A) of sampled position jj ; then [M]: n_alleles
__host__ __device__ inline int meta_i_stride(int max_pos) { return 5 + 2 * max_pos; }
// SpecLds::ndict and its like hold the dictionary size with the unit's META_I_W01 in the top bit
constexpr uint16_t ND_W01 = 0x8000u;
__host__ __device__ inline int nd_count(uint16_t x) { return (int)(x & 0x7FFFu); }
__host__ __device__ inline bool nd_w01(uint16_t x) { return (x & ND_W01) != 0; }
// Coded read table (speculative sampler): a unit's table usually holds a few dozen distinct probabilities
// (one per base quality, its error share, 1.0 for gaps), so it is also stored as uint8 codes into a per-unit
// dictionary of float64 values: lossless, 8x smaller, and what the likelihood evaluation then streams stays in L2.
constexpr int DICT_MAX = 128;  // entries kept per unit (LDS of the sampler: 1 KB per chain)
constexpr int DICT_HASH = 512;   // open-addressing slots of the prepare pass's LDS set (at most DICT_MAX = 128 are taken)
// doubles: [0] luh, [1..] prior table (2K+5), then dist [M*A]
__host__ __device__ inline int meta_f_prior(int) { return 1; }
__host__ __device__ inline int meta_f_dist(int max_ploidy) { return 1 + 2 * max_ploidy + 5; }
__host__ __device__ inline int meta_f_stride(int max_ploidy, int max_pos, int max_allele) {
  return 1 + 2 * max_ploidy + 5 + max_pos * max_allele;
}

struct SimtParams {
  DenovoParams d;
  // workspace carved by the host
  double *rt;        // [U][max_ma][rpad]
  double *cntw;      // [U][rpad]
  uint8_t *codes;    // [U][max_ma][64][cstride]: code of read lane + 64 i at byte i of the lane's group
  double *dict;      // [U][DICT_MAX]
  double *gbp;       // [U * chains][max_ploidy][rpad] haplotype products of the chains' current genotypes for read chunks >= 4, or null
  int32_t *meta_i;   // [U][meta_i_stride]
  double *meta_f;    // [U][meta_f_stride]
  int n_units;
  int max_pos, max_allele, max_ploidy;
  int max_ma;        // max over units of n_pos * max_allele
  int max_ugens_pad; // doubles reserved for the SNV posterior scratch of the prepare pass
  int prep_rows_off; // byte offset of the prepare pass's per-position row staging in its LDS
  int cstride;       // bytes per lane and row of the coded table: rpad / 64 rounded up to 1, 2 or a multiple of 4
  int flags;         // debugging: bit 0 no mutation memo, bit 1 no interval memo (MCHAP_HIP_FLAGS); bit 30 below
  // steady-state pipeline (denovo_lane_kernel.hpp): per-chain hand-over records and threshold tables
  void *lane_state;  // [U * chains] LaneState
  void *lane_memo;   // [U * chains][2][tri(max_pos)] uint32
  // phased sampler (kernel 5: denovo_spec_kernel<K, G, true> in phases + denovo_coast_kernel): hand-over records
  void *pipe_state;           // [U * chains] PipeState
  double *pipe_memo;          // [U * chains][2][tri(max_pos)] total move probabilities of the interval steps
  const int32_t *pipe_list;   // chains of this launch (nullptr: all of them, in order)
  const int32_t *pipe_count;  // their number, on the device (nullptr: all)
  int32_t *pipe_out;          // coasting kernel: the chains it hands back, appended in any order
  int32_t *pipe_out_count;
  int pipe_iters;             // compound steps per chain in this launch (<= 0: to the end)
  int pipe_iters_max;         // ... which a wave extends to while one of its chains is not settled (PIPE_EXPORT)
  int pipe_mode;              // PIPE_RESUME | PIPE_EXPORT | PIPE_FILLONLY
  int pipe_parts;             // wavefronts a short list of chains may spread the completion of one chain's tables over
  int bp_cache;               // speculative sampler with one chain per wave: base-product cache carved after its LDS
  int fill_lt, fill_kw;       // denovo_fill_kernel: lanes per tile of the read table, words kept per distinct request
  int tw_lds;                 // denovo_spec_kernel<.., TW>: bytes of one wavefront's LDS layout behind the workgroup's exchange area
  int word_bits;              // bits of a packed haplotype word of this launch's sampler: 0 / 64, or 128 (denovo_simt_kernel<0, u128>)
  uint64_t cache_epoch;       // speculative / phased sampler: this call's epoch << 33, OR-ed into every likelihood-cache tag (0: the
                              // caches were cleared for this call instead): entries of earlier calls never match, nothing is cleared
  uint64_t *ctx;              // phased sampler, resumed chains: [U * chains][ctx_n][spec_ctx_words] decision contexts per genotype
  int ctx_n;                  // (denovo_spec_kernel.hpp "decision contexts"), or null / 0
};
constexpr int PIPE_RESUME = 1;  // start from the chains' PipeState records
constexpr int PIPE_EXPORT = 2;  // at the end: complete the interval memo of the current genotype, write the records
// Completing a chain's tables is a few hundred likelihood evaluations served one after the other by its wavefront.
// When a launch holds few chains (a list of handed-back chains; a small batch of a big shape) the chip is empty
// and that latency is all there is: the exporting launch then leaves the tables as they are, and a PIPE_FILLONLY
// launch follows in which pipe_parts_eff() wavefronts per chain each complete every pipe_parts_eff()-th unknown entry
// (no steps, no records; the chain's likelihood cache is not used: the wavefronts would race on it).
constexpr int PIPE_FILLONLY = 4;
constexpr int PIPE_NOFILL = 8;  // PIPE_EXPORT without the table completion: denovo_fill_kernel (one lane per request) follows
constexpr int PIPE_FILL_SLOTS = 1024;  // wavefront slots such a launch may occupy (one per SIMD: beyond that the chip is busy anyway)
__host__ __device__ inline int pipe_parts_eff(int n_list, int parts) {
  if (parts <= 1 || n_list <= 0) return 1;
  const int pe = PIPE_FILL_SLOTS / n_list;
  return pe < 1 ? 1 : (pe > parts ? parts : pe);
}
// hand-over record of a chain between the launches of the phased sampler
struct PipeState {
  uint64_t g[8];     // haplotype words in the chain's own (unsorted) order
  double llk;
  uint64_t ctr;      // next draw of the chain's stream
  double mlo, mhi;   // mutation step: no move while every uniform is in [mlo, mhi)
  int32_t step;      // MCMC steps done (== steps: finished, or stopped by an error status)
  int32_t mvalid;
  uint64_t pad[3];
};
static_assert(sizeof(PipeState) == 128, "PipeState layout");
constexpr int SIMT_FLAG_PREP_GLOBAL = 1 << 30;  // table too large for the prepare pass's LDS copy

// ---- event counters of the profiling builds (make stats / make phases) -------------------------------------------
#if defined(MCHAP_STATS) || defined(MCHAP_PHASES)
constexpr int N_STATS = 64;  // [0..23] event counters, [24..35] phase timers of the steps, [36..47] ... of the table completion, [48..55] sub-timers of the steps
static __device__ unsigned long long g_stats[N_STATS];
#endif
#ifdef MCHAP_STATS
#define STAT_ADD(i, pred)                                                         \
  do {                                                                            \
    const int n_ = __popcll(__ballot(pred));                                      \
    if (n_ && (threadIdx.x & 63) == 0) atomicAdd(&g_stats[i], (unsigned long long)n_); \
  } while (0)
#define STAT_WAVE(i, n)                                                                     \
  do {                                                                                      \
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_stats[i], (unsigned long long)(n));           \
  } while (0)
#else
#define STAT_ADD(i, pred) \
  do {                    \
  } while (0)
#define STAT_WAVE(i, n) \
  do {                  \
  } while (0)
#endif

// ---- what the speculative sampler and the coasting kernel of the phased sampler share -----------------------------
constexpr int SPEC_DRAWS_MAX = 384;  // draws of the current stream staged in LDS per group (Philox blocks in parallel)
__host__ __device__ inline int spec_draws(int K, int Mmax) {
  int d = 2 * K * Mmax - 1;
  if (d < 3 * Mmax + 2) d = 3 * Mmax + 2;
  d = (d + 1) & ~1;
  return d < SPEC_DRAWS_MAX ? d : SPEC_DRAWS_MAX;
}

// LDS pointers carry their address space so that every access is a ds_* instruction (a pointer stored in a struct
// otherwise degrades to a generic "flat" access)
#define LDSP(T) __attribute__((address_space(3))) T *
#define GLBP(T) __attribute__((address_space(1))) T *
template <class T>
__device__ __forceinline__ LDSP(T) lds_cast(void *p) {
  return (LDSP(T))p;
}

// entries of one interval-step memo table: intervals (start, stop) with 0 <= start < stop <= Mmax, triangular
__host__ __device__ inline int spec_memo_entries(int Mmax) { return Mmax * (Mmax + 1) / 2; }
__host__ __device__ inline int spec_memo_index(int start, int stop) { return stop * (stop - 1) / 2 + start; }

// dynamic LDS of denovo_coast_kernel<NW> (denovo_coast_kernel.hpp): a chain's two memo tables, its break distribution,
// its sorted words, the wavefronts' first undecided steps
constexpr int COAST_NW_LIST = 4;  // wavefronts per chain of a coasting launch over a list of handed-back chains
__host__ __device__ inline size_t coast_lds_bytes(int Mmax) {
  return (size_t)8 * (2 * spec_memo_entries(Mmax) + Mmax) + (size_t)8 * 12;
}

// stateless Philox draws of a stream (same contract as Rng in philox.hpp)
struct Stream {
  uint32_t k0, k1, c2, c3;
};
__device__ __forceinline__ double draw_double(uint64_t w) {
  return ((double)((uint32_t)w >> 5) * 67108864.0 + (double)((uint32_t)(w >> 32) >> 6)) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ uint32_t draw_interval(uint64_t w, uint32_t max) { return __umulhi((uint32_t)w, max + 1u); }

__device__ __forceinline__ void lds_sync() {
#ifdef MCHAP_SYNC_BARRIER
  __syncthreads();
#else
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
#endif
}

}  // namespace mchap
