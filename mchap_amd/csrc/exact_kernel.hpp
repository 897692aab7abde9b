// Exact genotype caller for MI355X (gfx950): enumeration of all C(H+K-1, K) genotypes over H known
// haplotypes (reference calling/exact.py:17-369, calling/prior.py:116-179, calling/utils.py:7-35,
// jitutils.py:114-146,254-318).
//
// Per unit: the per-(read, haplotype) products P[r][h] = prod_j reads[r, j, hap[h][j]] (NaN skipped) are built
// once per workgroup in LDS, row r holding H consecutive doubles, so a wavefront whose lanes each own one
// genotype reads P[r][g_k] for a common r from one H*8-byte window: distinct haplotypes fall in distinct banks
// (H <= 32) and equal ones broadcast.  Each lane then runs the reference's own sequential sum over reads for
// its genotype; genotypes are visited in VCF order (index -> alleles by combinatorial unranking).
#pragma once
#include "read_log.hpp"
#include "wave_math.hpp"

namespace mchap {

// Ploidy bound of a kernel's genotype arrays and unrolled loops (template argument KM): 8 -- MCHAP_MAX_PLOIDY, what rounds 1-4
// took -- for ploidies up to 8, and EXACT_KMAX = 16 for ploidies 9 to 15 (round 5: the shapes the de novo sampler's general kernel
// assembles), so that the usual ploidies keep their code
constexpr int EXACT_KMAX = 16;
constexpr int EXACT_THREADS = 256;
constexpr int EXACT_GENOS_PER_BLOCK = 4096;

struct ExactParams {
  const double *reads;      // [U][R][M][A]
  const int64_t *counts;    // [U][R] or null
  const int8_t *haps;       // [U][H][M]
  const double *inbreeding; // [U] or null (no prior)
  const double *freqs;      // [U][H] or null
  int R, M, A, H, K;
  long long G;
  int has_prior;
  int nblk;
  int Rcap;                 // rows of the LDS product table (0: all R; less: the passes tile the reads, exact_tile)
  double *ptab_ext;         // product table + read weights of THIS workgroup in global memory instead of LDS, or null
  double ptab_scale;        // the table holds product * ptab_scale: 1 / ploidy for the exact caller -- the factor every term of a read's sum
                            // over a genotype's haplotypes carries (likelihood.py:60-66), applied once per table entry instead of once per
                            // (genotype, read, haplotype): the same products, a third of the arithmetic less -- 1 for the call sampler (its
                            // greedy start divides by the partial ploidies)
  // outputs / workspace
  float *llk32;             // [U][G] or null
  double *llk64;            // [U][G] or null
  double *ljoint;           // [U][G] or null (workspace for posterior_mode)
  double *part_max;         // [U][nblk] block maxima of ljoint
  long long *part_idx;      // [U][nblk] index of the block maximum (first occurrence)
  double *part_llk;         // [U][nblk] llk at the block maximum
  double *part_lse;         // [U][nblk] log-sum-exp of the block's ljoint
  // second pass of the streaming form (exact_pass2_kernel): inputs written by exact_mode_kernel, per-block partial sums out
  const double *unit_total;     // [U] log normaliser
  const int64_t *unit_mode;     // [U][K] mode alleles
  double *part_freq;            // [U][nblk][2H + 1]: allele counts, allele occurrence, mode-support probability
};

// C(n + k - 1, k), the number of genotypes of ploidy k over n alleles (jitutils.py:228-250; 0 for n == 0).
// The product r * (n - 1 + d) is formed before the division: it is d times the next partial count, at most 15 times the result, so
// the value is right while the count stays below 2^59.  The exact caller asks for cwr(n, p) with n <= H, p <= K alone (unrank_genotype,
// rank_genotype) and ENUMERATES its C(H + K - 1, K) genotypes: its workspace holds four doubles per 4096 of them and a pass
// visits each, so a count near 2^59 (2^50 bytes, years of passes) is out of its reach long before the arithmetic is.  The
// call sampler ranks single genotypes of shapes up to 2^62: its keys take call_rank (call_mcmc_kernel.hpp) above ploidy 8.
__device__ __forceinline__ long long cwr(int n, int k) {
  if (n <= 0) return 0;
  long long r = 1;
  for (int d = 1; d <= k; d++) r = r * (n - 1 + d) / d;
  return r;
}

// jitutils.py:279-318: VCF index -> ascending alleles
template <int KM>
__device__ __forceinline__ void unrank_genotype(long long index, int K, int (&g)[KM]) {
  long long remainder = index;
#pragma unroll
  for (int p = KM; p >= 1; p--) {
    if (p > K) {
      g[p - 1] = 0;
      continue;
    }
    int n = -1;
    long long nw = 0, prev = 0;
    while (nw <= remainder) {
      n += 1;
      prev = nw;
      nw = cwr(n, p);
    }
    n -= 1;
    remainder -= prev;
    g[p - 1] = n;
  }
}

// jitutils.py:253-276
__device__ inline long long rank_genotype(const int *g, int K) {
  long long idx = 0;
  for (int i = 0; i < K; i++) idx += cwr(g[i], i + 1);
  return idx;
}

// jitutils.py:114-146
__device__ inline void increment_genotype(int *g, int K) {
  if (K == 1) {
    g[0] += 1;
    return;
  }
  const int previous = g[0];
  for (int i = 1; i < K; i++) {
    if (g[i] == previous) continue;
    g[i - 1] += 1;
    for (int z = 0; z < i - 1; z++) g[z] = 0;
    return;
  }
  g[K - 1] += 1;
  for (int z = 0; z < K - 1; z++) g[z] = 0;
}

// prior tables in LDS: lgd[h][d] = lgamma(d + alpha_h) - (lgamma(d + 1) + lgamma(alpha_h)), d = 0..K
struct PriorTab {
  const double *lgd;   // [H][K+1]
  const double *lgf;   // [K+1] lgamma(d + 1)
  const double *lfreq; // [H] prior allele frequencies (F == 0 with frequencies)
  double left;         // lgamma(K+1) + lgamma(sum_alpha) - lgamma(K + sum_alpha)
  double lnH;          // log(H)
  double F;
  int has_freqs;
};

// calling/prior.py:116-179 on ascending alleles g[0..K-1]
__device__ inline double calling_log_prior(const PriorTab &t, const int *g, int K) {
  // allelic dosage in first-occurrence order (calling/utils.py:7-35); g is ascending so runs are contiguous
  if (t.F == 0.0) {
    double den = 0.0;
    int i = 0;
    double prod = 1.0;
    // dosage array holds the run length at the first copy and 0 elsewhere: lgamma(0 + 1) = 0 for the zeros
    while (i < K) {
      int j = i;
      while (j < K && g[j] == g[i]) j++;
      den += t.lgf[j - i];
      i = j;
    }
    const double ln_perms = t.lgf[K] - den;
    if (!t.has_freqs) return ln_perms - (double)K * t.lnH;
    for (int q = 0; q < K; q++) prod *= t.lfreq[g[q]];
    return ln_perms + log(prod);
  }
  double prod = 0.0;
  int i = 0;
  while (i < K) {
    int j = i;
    while (j < K && g[j] == g[i]) j++;
    prod += t.lgd[g[i] * (K + 1) + (j - i)];
    i = j;
  }
  return t.left + prod;
}

// LDS of the enumeration passes: product table, read weights, prior tables, then the caller's scratch
struct ExactLds {
  double *ptab;   // [R][H]
  double *cnt;    // [R]
  double *lgd;    // [H][K+1]
  double *lgf;    // [K+1]
  double *lfreq;  // [H]
  double *red;    // reduction scratch (the rest of the allocation)
  bool w01;       // every read weight of the unit is 1: ONE logarithm per four consecutive reads (read_log_product, round 5)
};
// Builds P[r][h], the read weights and the prior tables of `unit` (whole workgroup; ends with a barrier).
// (with P.Rcap < R only the first Rcap reads are tabulated here: exact_tile brings in the others, tile by tile)
__device__ __forceinline__ void exact_setup(const ExactParams &P, int unit, unsigned char *smem, ExactLds &E, PriorTab &pt) {
  const int M = P.M, A = P.A, H = P.H, K = P.K;
  const int R = (P.Rcap > 0 && P.Rcap < P.R) ? P.Rcap : P.R;
  if (P.ptab_ext) {  // (call sampler with a table that exceeds the LDS: slower reads, no limit)
    E.ptab = P.ptab_ext;
    E.cnt = E.ptab + (size_t)R * H;
    E.lgd = reinterpret_cast<double *>(smem);
  } else {
    E.ptab = reinterpret_cast<double *>(smem);
    E.cnt = E.ptab + (size_t)R * H;
    E.lgd = E.cnt + R;
  }
  E.lgf = E.lgd + (size_t)H * (K + 1);
  E.lfreq = E.lgf + (K + 1);
  E.red = E.lfreq + H;
  __shared__ double s_left;
  const double *reads = P.reads + (size_t)unit * P.R * M * A;
  const int8_t *haps = P.haps + (size_t)unit * H * M;
  for (int q = threadIdx.x; q < R * H; q += blockDim.x) {
    const int r = q / H, h = q % H;
    double prod = 1.0;
    for (int j = 0; j < M; j++) {
      const double v = reads[((size_t)r * M + j) * A + haps[h * M + j]];
      if (!isnan(v)) prod *= v;  // assemble/likelihood.py:54-59
    }
    E.ptab[q] = prod * P.ptab_scale;
  }
  for (int r = threadIdx.x; r < R; r += blockDim.x) E.cnt[r] = P.counts ? (double)P.counts[(size_t)unit * P.R + r] : 1.0;
  {
    // (over ALL reads of the unit, not only the first tile's: the groups of four run through the tiles)
    int weighted = 0;
    if (P.counts)
      for (int r = threadIdx.x; r < P.R; r += blockDim.x) weighted |= (P.counts[(size_t)unit * P.R + r] != 1) ? 1 : 0;
    E.w01 = __syncthreads_or(weighted) == 0;
  }
  double F = 0.0;
  const bool has_prior = P.has_prior != 0;
  const bool has_freqs = has_prior && P.freqs != nullptr;
  if (has_prior) {
    F = P.inbreeding[unit];
    const double scale = (1.0 - F) / F;
    for (int q = threadIdx.x; q < H * (K + 1); q += blockDim.x) {
      const int h = q / (K + 1), d = q % (K + 1);
      const double alpha = has_freqs ? P.freqs[(size_t)unit * H + h] * scale : (1.0 / (double)H) * scale;
      E.lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
    }
    for (int d = threadIdx.x; d <= K; d += blockDim.x) E.lgf[d] = lgamma((double)d + 1.0);
    for (int h = threadIdx.x; h < H; h += blockDim.x) E.lfreq[h] = has_freqs ? P.freqs[(size_t)unit * H + h] : 0.0;
    if (threadIdx.x == 0) {
      double sum_alpha;
      if (has_freqs) {
        sum_alpha = 0.0;
        for (int h = 0; h < H; h++) sum_alpha += P.freqs[(size_t)unit * H + h] * scale;
      } else {
        sum_alpha = ((1.0 / (double)H) * scale) * (double)H;
      }
      s_left = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
    }
  }
  __syncthreads();
  pt.lgd = E.lgd;
  pt.lgf = E.lgf;
  pt.lfreq = E.lfreq;
  pt.left = has_prior ? s_left : 0.0;
  pt.lnH = log((double)H);
  pt.F = F;
  pt.has_freqs = has_freqs ? 1 : 0;
}

// The exact kernels' product table and read weights are always in the LDS (only the call sampler's exact_setup may be
// handed a table in global memory), but the pointer in ExactLds is generic and the compiler then reads it with flat_load
// (through the vector memory path: r03 PMC, 6.4 VMEM reads per wavefront-term and no LDS instructions).  Reading through
// an LDS-qualified pointer gives ds_read_b64: same values, shorter latency, and the vector memory unit stays free.
typedef __attribute__((address_space(3))) const double lds_cdouble;
__device__ __forceinline__ lds_cdouble *lds_table(const double *p) { return (lds_cdouble *)p; }

// log likelihood of the genotype with ascending alleles g (calling/exact.py:252-263 via assemble/likelihood.py:17-70)
template <int KM>
__device__ __forceinline__ double exact_llk(const ExactLds &E, const int (&g)[KM], int R, int H, int K, double invK) {
  double llk = 0.0;
  lds_cdouble *ptab = lds_table(E.ptab), *cnt = lds_table(E.cnt);
  int r = 0;
  if (E.w01) {  // unweighted reads: the sum over four consecutive reads as the logarithm of their product
    for (; r + 4 <= R; r += 4) {
      double rp[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        lds_cdouble *row = ptab + (r + t) * H;
        rp[t] = 0.0;
#pragma unroll
        for (int k = 0; k < KM; k++)
          if (k < K) rp[t] += row[g[k]];
      }
      llk += read_log_product<4>(rp);
    }
  }
  for (; r < R; r++) {
    lds_cdouble *row = ptab + r * H;
    double rp = 0.0;
#pragma unroll
    for (int k = 0; k < KM; k++)
      if (k < K) rp += row[g[k]];
    llk += read_log(rp) * cnt[r];
  }
  return llk;
}

// NQ genotypes of one thread at once: each sum runs over the reads in order as in exact_llk (same values); the NQ
// chains of LDS reads, adds and logs are independent and hide each other's latency (two waves per SIMD is all the
// 64 KB table leaves).  MI355X, config #4: pass 1 28.0 -> 21.8 (two) -> 20.4 ms (four at a time).
template <int NQ, int KM>
__device__ __forceinline__ void exact_llkn(const ExactLds &E, const int (&g)[NQ][KM], int R, int H, int K, double invK,
                                           double (&l)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; q++) l[q] = 0.0;
  lds_cdouble *ptab = lds_table(E.ptab), *cnt = lds_table(E.cnt);
  int r = 0;
  if (E.w01) {  // (as exact_llk: groups of four consecutive reads, one logarithm each)
    for (; r + 4 <= R; r += 4) {
      double rp[NQ][4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        lds_cdouble *row = ptab + (r + t) * H;
#pragma unroll
        for (int q = 0; q < NQ; q++) rp[q][t] = 0.0;
#pragma unroll
        for (int k = 0; k < KM; k++)
          if (k < K) {
#pragma unroll
            for (int q = 0; q < NQ; q++) rp[q][t] += row[g[q][k]];
          }
      }
#pragma unroll
      for (int q = 0; q < NQ; q++) l[q] += read_log_product<4>(rp[q]);
    }
  }
  for (; r < R; r++) {
    lds_cdouble *row = ptab + r * H;
    double rp[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) rp[q] = 0.0;
#pragma unroll
    for (int k = 0; k < KM; k++)
      if (k < K) {
#pragma unroll
        for (int q = 0; q < NQ; q++) rp[q] += row[g[q][k]];
      }
    const double w = cnt[r];
#pragma unroll
    for (int q = 0; q < NQ; q++) l[q] += read_log(rp[q]) * w;
  }
}

// Reads r0 .. r0 + rn - 1 of `unit` into the product table and the weights (whole workgroup; barriers on both sides)
__device__ __forceinline__ void exact_tile(const ExactParams &P, int unit, const ExactLds &E, int r0, int rn) {
  const int M = P.M, A = P.A, H = P.H;
  const double *reads = P.reads + ((size_t)unit * P.R + r0) * M * A;
  const int8_t *haps = P.haps + (size_t)unit * H * M;
  __syncthreads();
  for (int q = threadIdx.x; q < rn * H; q += blockDim.x) {
    const int r = q / H, h = q % H;
    double prod = 1.0;
    for (int j = 0; j < M; j++) {
      const double v = reads[((size_t)r * M + j) * A + haps[h * M + j]];
      if (!isnan(v)) prod *= v;
    }
    E.ptab[q] = prod * P.ptab_scale;
  }
  for (int r = threadIdx.x; r < rn; r += blockDim.x) E.cnt[r] = P.counts ? (double)P.counts[(size_t)unit * P.R + r0 + r] : 1.0;
  __syncthreads();
}
// The log likelihoods of the thread's genotypes lo + threadIdx.x + t * blockDim.x (t < NGT) when the reads do not fit
// the LDS at once: tile by tile, every genotype's sum continued in read order -- the values of the untiled loop.
constexpr int EXACT_NGT = EXACT_GENOS_PER_BLOCK / EXACT_THREADS;
template <int KM>
__device__ __forceinline__ void exact_llk_tiled(const ExactParams &P, int unit, const ExactLds &E, long long lo, long long hi,
                                                double (&llk)[EXACT_NGT]) {
  const int H = P.H, K = P.K, cap = P.Rcap;
  const double invK = 1.0 / (double)K;
#pragma unroll
  for (int t = 0; t < EXACT_NGT; t++) llk[t] = 0.0;
  for (int r0 = 0; r0 < P.R; r0 += cap) {
    const int rn = min(cap, P.R - r0);
    if (r0 > 0) exact_tile(P, unit, E, r0, rn);  // (exact_setup brought the first tile)
#pragma unroll
    for (int t = 0; t < EXACT_NGT; t++) {
      const long long i = lo + threadIdx.x + (long long)t * EXACT_THREADS;
      if (i < hi) {
        int g[KM];
        unrank_genotype(i, K, g);
        double acc = llk[t];
        lds_cdouble *ptab = lds_table(E.ptab), *cnt = lds_table(E.cnt);
        int r = 0;
        // (the host keeps the tile a multiple of four reads, so the groups of four are those of the untiled loop)
        if (E.w01) {
          for (; r + 4 <= rn; r += 4) {
            double rp[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
              lds_cdouble *row = ptab + (r + q) * H;
              rp[q] = 0.0;
#pragma unroll
              for (int k = 0; k < KM; k++)
                if (k < K) rp[q] += row[g[k]];
            }
            acc += read_log_product<4>(rp);
          }
        }
        for (; r < rn; r++) {
          lds_cdouble *row = ptab + r * H;
          double rp = 0.0;
#pragma unroll
          for (int k = 0; k < KM; k++)
            if (k < K) rp += row[g[k]];
          acc += read_log(rp) * cnt[r];
        }
        llk[t] = acc;
      }
    }
  }
}

template <bool TILED, int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_pass1_kernel(const ExactParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.y;
  const int R = P.R, H = P.H, K = P.K;
  const bool has_prior = P.has_prior != 0;
  ExactLds E;
  PriorTab pt;
  exact_setup(P, unit, smem, E, pt);
  double *red = E.red;  // [5][EXACT_THREADS] reduction scratch

  const long long G = P.G;
  const long long lo = (long long)blockIdx.x * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double invK = 1.0 / (double)K;
  double best = -INFINITY, best_llk = -INFINITY;
  long long best_idx = 0x7fffffffffffffffll;
  double lse_m = -INFINITY, lse_s = 0.0;  // running log-sum-exp: max and scaled sum
  auto visit = [&](long long i, const int (&g)[KM], double llk) {
    const size_t o = (size_t)unit * G + i;
    if (P.llk32) P.llk32[o] = (float)llk;  // calling/exact.py:254 float32 store
    if (P.llk64) P.llk64[o] = llk;
    if (P.ljoint || P.part_max) {
      const double lpr = has_prior ? calling_log_prior(pt, g, K) : 0.0;
      const double lj = llk + lpr;
      if (P.ljoint) P.ljoint[o] = lj;
      if (lj > best) {  // calling/exact.py:51: strict, first maximum wins
        best = lj;
        best_idx = i;
        best_llk = llk;
      }
      if (lj > lse_m) {
        lse_s = lse_s * exp(lse_m - lj) + 1.0;
        lse_m = lj;
      } else if (lj > -INFINITY) {
        lse_s += exp(lj - lse_m);
      }
    }
  };
  if constexpr (TILED) {
    double tl[EXACT_NGT];
    exact_llk_tiled<KM>(P, unit, E, lo, hi, tl);
#pragma unroll
    for (int t = 0; t < EXACT_NGT; t++) {
      const long long i = lo + threadIdx.x + (long long)t * EXACT_THREADS;
      if (i < hi) {
        int g[KM];
        unrank_genotype(i, K, g);
        visit(i, g, tl[t]);
      }
    }
  } else {
    // the thread's genotypes i, i + 256, ... two at a time (visited in index order: the first maximum stays the first)
    long long i = lo + threadIdx.x;
    for (; i + 3 * (long long)blockDim.x < hi; i += 4 * (long long)blockDim.x) {
      int g4[4][KM];
      double l4[4];
#pragma unroll
      for (int q = 0; q < 4; q++) unrank_genotype(i + (long long)q * blockDim.x, K, g4[q]);
      exact_llkn<4>(E, g4, R, H, K, invK, l4);
#pragma unroll
      for (int q = 0; q < 4; q++) visit(i + (long long)q * blockDim.x, g4[q], l4[q]);
    }
    for (; i + (long long)blockDim.x < hi; i += 2 * (long long)blockDim.x) {
      int g2[2][KM];
      double l2[2];
      unrank_genotype(i, K, g2[0]);
      unrank_genotype(i + blockDim.x, K, g2[1]);
      exact_llkn<2>(E, g2, R, H, K, invK, l2);
      visit(i, g2[0], l2[0]);
      visit(i + blockDim.x, g2[1], l2[1]);
    }
    if (i < hi) {
      int g[KM];
      unrank_genotype(i, K, g);
      visit(i, g, exact_llk(E, g, R, H, K, invK));
    }
  }
  if (!P.part_max) return;
  // block reduction
  double *rb = red, *ri = red + EXACT_THREADS, *rl = red + 2 * EXACT_THREADS, *rm = red + 3 * EXACT_THREADS, *rs = red + 4 * EXACT_THREADS;
  rb[threadIdx.x] = best;
  ri[threadIdx.x] = (double)best_idx;  // indices < 2^53
  rl[threadIdx.x] = best_llk;
  rm[threadIdx.x] = lse_m;
  rs[threadIdx.x] = lse_s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = -INFINITY, bl = -INFINITY, bi = 9.0e18, m = -INFINITY, s = 0.0;
    for (int t = 0; t < (int)blockDim.x; t++) {
      if (rb[t] > b || (rb[t] == b && ri[t] < bi)) {
        b = rb[t];
        bi = ri[t];
        bl = rl[t];
      }
      if (rm[t] > -INFINITY) {
        if (rm[t] > m) {
          s = s * exp(m - rm[t]) + rs[t];
          m = rm[t];
        } else {
          s += rs[t] * exp(rm[t] - m);
        }
      }
    }
    const size_t o = (size_t)unit * P.nblk + blockIdx.x;
    P.part_max[o] = b;
    P.part_idx[o] = (long long)bi;
    P.part_llk[o] = bl;
    P.part_lse[o] = (m > -INFINITY) ? m + log(s) : -INFINITY;
  }
}

// ---- streaming form without any per-genotype array (calling/exact.py:156-249: two passes over the genotypes) ----
// After pass 1: normaliser and mode of every unit from the per-block partials.
struct ExactModeParams {
  ExactParams e;
  int64_t *mode_alleles;                  // [U][K] (output, and input of the second pass)
  double *mode_llk, *mode_prob, *total;   // [U]
};
static __global__ __launch_bounds__(64) void exact_mode_kernel(const ExactModeParams P) {
  constexpr int KM = EXACT_KMAX;
  const ExactParams &E = P.e;
  const int unit = blockIdx.x;
  if (threadIdx.x != 0) return;
  double b = -INFINITY, bl = -INFINITY, total = -INFINITY;
  long long bi = 0;
  for (int q = 0; q < E.nblk; q++) {
    const size_t o = (size_t)unit * E.nblk + q;
    if (E.part_max[o] > b) {  // blocks are in index order: strict > keeps the first maximum (calling/exact.py:51)
      b = E.part_max[o];
      bi = E.part_idx[o];
      bl = E.part_llk[o];
    }
    total = add_log_prob(total, E.part_lse[o]);
  }
  int g[KM];
  unrank_genotype(bi, E.K, g);
  for (int k = 0; k < E.K; k++) P.mode_alleles[(size_t)unit * E.K + k] = g[k];
  if (P.mode_llk) P.mode_llk[unit] = bl;
  if (P.mode_prob) P.mode_prob[unit] = exp(b - total);
  P.total[unit] = total;
}

// Second pass: every genotype's joint value again, its probability under the known normaliser added to the allele
// count / occurrence sums (calling/exact.py:108-153) and, when it consists of exactly the mode's alleles, to the
// support probability (64-105).  A wavefront takes 64 consecutive genotypes at a time; each of the 2H + 1 sums gets
// the wavefront's 64 contributions by a shuffle reduction (fixed order) and is kept per wavefront in LDS -- a
// kilobyte instead of a column per thread, so that two workgroups share a CU as in pass 1.  Wavefronts are summed
// in order, blocks in order by exact_freq_kernel: deterministic.
inline size_t exact_pass2_lds(int R, int H, int K, int threads) {
  return ((size_t)R * H + R + (size_t)H * (K + 1) + (K + 1) + H + (size_t)(2 * H + 1) * (threads / 64)) * 8;
}
// HAVE_LJ: pass 1 left llk + log prior of every genotype in P.ljoint (the caller's workspace had room for U * G
// doubles): the pass then reads them back instead of forming every likelihood a second time -- same values, same sums.
template <bool TILED, bool HAVE_LJ = false, int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_pass2_kernel(const ExactParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.y;
  const int R = P.R, H = P.H, K = P.K;
  const bool has_prior = !HAVE_LJ && P.has_prior != 0;
  ExactLds E;
  PriorTab pt;
  if constexpr (HAVE_LJ) {
    E.red = reinterpret_cast<double *>(smem);  // only the per-wavefront sums live in LDS
  } else {
    exact_setup(P, unit, smem, E, pt);
  }
  const int nt = blockDim.x, nw = nt >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int NS = 2 * H + 1;
  double *acc = E.red;  // [nw][2H + 1]
  for (int i = threadIdx.x; i < nw * NS; i += nt) acc[i] = 0.0;
  __syncthreads();
  const double total = P.unit_total[unit];
  int ms[KM], ns = 0;  // distinct alleles of the mode, ascending
  for (int k = 0; k < K; k++) {
    const int a = (int)P.unit_mode[(size_t)unit * K + k];
    if (k == 0 || a != ms[ns - 1]) ms[ns++] = a;
  }
  const long long G = P.G;
  const long long lo = (long long)blockIdx.x * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double invK = 1.0 / (double)K;
  double *mine = acc + (size_t)wave * NS;
  double tl[EXACT_NGT];
  if constexpr (HAVE_LJ) {
#pragma unroll
    for (int t = 0; t < EXACT_NGT; t++) {
      const long long i = lo + threadIdx.x + (long long)t * nt;
      tl[t] = i < hi ? P.ljoint[(size_t)unit * G + i] : 0.0;
    }
  } else if constexpr (TILED) {
    exact_llk_tiled<KM>(P, unit, E, lo, hi, tl);  // (nt == EXACT_THREADS: thread t's genotypes lo + t + 256 q)
  } else {
    // the likelihoods of the thread's genotypes, four at a time (exact_llkn), ahead of the accounting loop
#pragma unroll
    for (int tqq = 0; tqq < EXACT_NGT; tqq += 4) {
      const long long ia = lo + threadIdx.x + (long long)tqq * nt;
#pragma unroll
      for (int q = 0; q < 4; q++) tl[tqq + q] = 0.0;
      if (ia + 3 * (long long)nt < hi) {
        int g4[4][KM];
        double l4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) unrank_genotype(ia + (long long)q * nt, K, g4[q]);
        exact_llkn<4>(E, g4, R, H, K, invK, l4);
#pragma unroll
        for (int q = 0; q < 4; q++) tl[tqq + q] = l4[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (ia + (long long)q * nt < hi) {
            int ga[KM];
            unrank_genotype(ia + (long long)q * nt, K, ga);
            tl[tqq + q] = exact_llk(E, ga, R, H, K, invK);
          }
        }
      }
    }
  }
#pragma unroll
  for (int tqq = 0; tqq < EXACT_NGT; tqq++) {
    const long long i0 = lo + (long long)wave * 64 + (long long)tqq * nt;  // wave-uniform
    if (i0 >= hi) continue;
    const long long i = i0 + lane;
    int g[KM];
#pragma unroll
    for (int k = 0; k < KM; k++) g[k] = -1;
    double prob = 0.0;
    bool support = false;
    if (i < hi) {
      unrank_genotype(i, K, g);
      const double llk = tl[tqq];
      const double lpr = has_prior ? calling_log_prior(pt, g, K) : 0.0;
      prob = exp((llk + lpr) - total);
      int nd = 0;
      bool same = true;
      for (int k = 0; k < K; k++) {
        if (k == 0 || g[k] != g[k - 1]) {
          same = same && nd < ns && ms[nd] == g[k];
          nd++;
        }
      }
      support = same && nd == ns;
    }
    for (int a = 0; a < H; a++) {
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < KM; k++) cnt += (k < K && g[k] == a) ? 1 : 0;
      const double c1 = wave_sum(prob * (double)cnt);         // allele count
      const double c2 = wave_sum(cnt > 0 ? prob : 0.0);       // allele occurrence
      if (lane == 0) {
        mine[a] += c1;
        mine[H + a] += c2;
      }
    }
    const double c3 = wave_sum(support ? prob : 0.0);
    if (lane == 0) mine[2 * H] += c3;
  }
  __syncthreads();
  for (int h = threadIdx.x; h < NS; h += nt) {
    double sum = 0.0;
    for (int w = 0; w < nw; w++) sum += acc[(size_t)w * NS + h];
    P.part_freq[((size_t)unit * P.nblk + blockIdx.x) * NS + h] = sum;
  }
}
struct ExactFreqParams {
  const double *part_freq;  // [U][nblk][2H + 1]
  int nblk, H, K;
  double *support_prob;     // [U] or null
  double *freqs_out, *occur_out;  // [U][H] or null
};
static __global__ __launch_bounds__(64) void exact_freq_kernel(const ExactFreqParams P) {
  const int unit = blockIdx.x;
  for (int h = threadIdx.x; h < 2 * P.H + 1; h += blockDim.x) {
    double sum = 0.0;
    for (int q = 0; q < P.nblk; q++) sum += P.part_freq[((size_t)unit * P.nblk + q) * (2 * P.H + 1) + h];
    if (h < P.H) {
      if (P.freqs_out) P.freqs_out[(size_t)unit * P.H + h] = sum / (double)P.K;
    } else if (h < 2 * P.H) {
      if (P.occur_out) P.occur_out[(size_t)unit * P.H + (h - P.H)] = sum;
    } else if (P.support_prob) {
      P.support_prob[unit] = sum;
    }
  }
}

// ---- array form for a batch: genotype_posteriors on stored likelihoods (calling/exact.py:295-329), one workgroup per unit,
// the joint values parked in the output array itself, and what call_exact.py:126-159 / exact.py:332-407 derive from the
// posterior array: its first maximum, the probability of the mode's support, allele frequencies / counts / occurrence ----
struct ExactArrayParams {
  const float *llk32;       // [U][G] or null
  const double *llk64;      // [U][G] or null (used when llk32 is null)
  double *post;             // [U][G] out (may be null when only... never: the summaries read it)
  const double *post_in;    // [U][G] summaries of a given posterior array instead (llk32 == llk64 == null)
  long long G;
  int K, H, has_prior;
  const double *inbreeding; // [U]
  const double *freqs;      // [U][H] or null
  int64_t *mode_alleles;    // [U][K] or null
  double *mode_prob, *support_prob;       // [U] or null
  double *afreq, *acount, *aoccur;        // [U][H] or null
  int nacc;                 // threads that accumulate the allele sums (an LDS column each)
};
constexpr int EXACT_ARRAY_THREADS = 1024;
inline size_t exact_array_lds(int H, int K, int nacc) {
  return ((size_t)H * (K + 1) + (K + 1) + H + 2 * (size_t)EXACT_ARRAY_THREADS + (size_t)(2 * H + 1) * nacc) * 8;
}
template <int KM = 8>
__global__ __launch_bounds__(EXACT_ARRAY_THREADS) void exact_array_kernel(const ExactArrayParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x;
  const int K = P.K, H = P.H;
  const long long G = P.G;
  double *lgd = reinterpret_cast<double *>(smem);
  double *lgf = lgd + (size_t)H * (K + 1);
  double *lfreq = lgf + (K + 1);
  double *red = lfreq + H;                    // [2][threads]
  double *acc = red + 2 * EXACT_ARRAY_THREADS;  // [2H + 1][nacc]
  __shared__ double s_left, s_total;
  __shared__ long long s_mode;
  const int nt = blockDim.x;
  const double *post;
  if (P.post_in) {
    post = P.post_in + (size_t)unit * G;
  } else {
    // ---- genotype_posteriors ----
    const bool is_f32 = P.llk32 != nullptr;
    const bool has_freqs = P.has_prior && P.freqs;
    const double F = P.has_prior ? P.inbreeding[unit] : 0.0;
    if (P.has_prior) {
      const double scale = (1.0 - F) / F;
      for (int q = threadIdx.x; q < H * (K + 1); q += nt) {
        const int h = q / (K + 1), d = q % (K + 1);
        const double alpha = has_freqs ? P.freqs[(size_t)unit * H + h] * scale : (1.0 / (double)H) * scale;
        lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
      }
      for (int d = threadIdx.x; d <= K; d += nt) lgf[d] = lgamma((double)d + 1.0);
      for (int h = threadIdx.x; h < H; h += nt) lfreq[h] = has_freqs ? P.freqs[(size_t)unit * H + h] : 0.0;
      if (threadIdx.x == 0) {
        double sum_alpha = 0.0;
        if (has_freqs) {
          for (int h = 0; h < H; h++) sum_alpha += P.freqs[(size_t)unit * H + h] * scale;
        } else {
          sum_alpha = ((1.0 / (double)H) * scale) * (double)H;
        }
        s_left = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
      }
    }
    __syncthreads();
    PriorTab pt;
    pt.lgd = lgd;
    pt.lgf = lgf;
    pt.lfreq = lfreq;
    pt.left = P.has_prior ? s_left : 0.0;
    pt.lnH = log((double)H);
    pt.F = F;
    pt.has_freqs = has_freqs ? 1 : 0;
    double *out = P.post + (size_t)unit * G;
    double m = -INFINITY, sacc = 0.0;
    for (long long i = threadIdx.x; i < G; i += nt) {
      int g[KM];
      unrank_genotype(i, K, g);
      const double lpr = P.has_prior ? calling_log_prior(pt, g, K) : 0.0;
      double j;
      if (is_f32) j = (double)(float)((double)P.llk32[(size_t)unit * G + i] + lpr);  // stored in the array's dtype (exact.py:317)
      else j = P.llk64[(size_t)unit * G + i] + lpr;
      out[i] = j;
      if (j > m) {
        sacc = sacc * exp(m - j) + 1.0;
        m = j;
      } else if (j > -INFINITY) {
        sacc += exp(j - m);
      }
    }
    red[threadIdx.x] = m;
    red[EXACT_ARRAY_THREADS + threadIdx.x] = sacc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double mm = -INFINITY, ss = 0.0;
      for (int t = 0; t < nt; t++) {
        if (red[t] > -INFINITY) {
          if (red[t] > mm) {
            ss = ss * exp(mm - red[t]) + red[EXACT_ARRAY_THREADS + t];
            mm = red[t];
          } else {
            ss += red[EXACT_ARRAY_THREADS + t] * exp(red[t] - mm);
          }
        }
      }
      // (float64 also for float32 likelihoods: the compiled reference's log-denominator is float64 -- numba unifies
      // add_log_prob's result type -- and only the joint values are stored in float32; oracle: orc_genotype_posteriors_f32)
      s_total = mm + log(ss);
    }
    __syncthreads();
    const double total = s_total;
    for (long long i = threadIdx.x; i < G; i += nt) out[i] = exp(out[i] - total);
    __syncthreads();
    post = out;
  }
  const bool want_mode = P.mode_alleles || P.mode_prob || P.support_prob;
  const bool want_freq = P.afreq || P.acount || P.aoccur;
  if (!want_mode && !want_freq) return;
  // ---- first maximum of the posterior array (np.argmax) ----
  {
    double b = -INFINITY;
    long long bi = 0x7fffffffffffffffll;
    for (long long i = threadIdx.x; i < G; i += nt) {
      const double v = post[i];
      if (v > b) {
        b = v;
        bi = i;
      }
    }
    red[threadIdx.x] = b;
    red[EXACT_ARRAY_THREADS + threadIdx.x] = (double)bi;
    __syncthreads();
    if (threadIdx.x == 0) {
      double bb = -INFINITY, bidx = 9.0e18;
      for (int t = 0; t < nt; t++)
        if (red[t] > bb || (red[t] == bb && red[EXACT_ARRAY_THREADS + t] < bidx)) {
          bb = red[t];
          bidx = red[EXACT_ARRAY_THREADS + t];
        }
      s_mode = bidx < 9.0e18 ? (long long)bidx : 0;
      if (P.mode_prob) P.mode_prob[unit] = bb;
    }
    __syncthreads();
  }
  int mg[KM];
  unrank_genotype(s_mode, K, mg);
  if (P.mode_alleles && threadIdx.x < K) P.mode_alleles[(size_t)unit * K + threadIdx.x] = mg[threadIdx.x];
  int ms[KM], ns = 0;
  for (int k = 0; k < K; k++)
    if (k == 0 || mg[k] != mg[k - 1]) ms[ns++] = mg[k];
  // ---- sums over the genotypes: P.nacc accumulating threads (an LDS column each), summed in thread order ----
  const int na = P.nacc;
  if ((int)threadIdx.x < na) {
    for (int h = 0; h < 2 * H + 1; h++) acc[(size_t)h * na + threadIdx.x] = 0.0;
    for (long long i = threadIdx.x; i < G; i += na) {
      int g[KM];
      unrank_genotype(i, K, g);
      const double prob = post[i];
      int nd = 0;
      bool same = true;
      for (int k = 0; k < K; k++) {
        acc[(size_t)g[k] * na + threadIdx.x] += prob;
        if (k == 0 || g[k] != g[k - 1]) {
          acc[(size_t)(H + g[k]) * na + threadIdx.x] += prob;
          same = same && nd < ns && ms[nd] == g[k];
          nd++;
        }
      }
      if (same && nd == ns) acc[(size_t)(2 * H) * na + threadIdx.x] += prob;
    }
  }
  __syncthreads();
  for (int h = threadIdx.x; h < 2 * H + 1; h += nt) {
    double sum = 0.0;
    for (int t = 0; t < na; t++) sum += acc[(size_t)h * na + t];
    if (h < H) {
      if (P.afreq) P.afreq[(size_t)unit * H + h] = sum / (double)K;
      if (P.acount) P.acount[(size_t)unit * H + h] = sum;
    } else if (h < 2 * H) {
      if (P.aoccur) P.aoccur[(size_t)unit * H + (h - H)] = sum;
    } else if (P.support_prob) {
      P.support_prob[unit] = sum;
    }
  }
}

// ---- prior allele frequencies by EM over stored likelihoods (application.estimate_prior_frequencies): one iteration is
// f'[h] = sum_s K_s freqs_s(f)[h] / sum_s K_s over the samples s of a record, freqs_s the mean posterior allele frequency under
// prior (F_s, f).  The likelihoods do not depend on f: pass 1 leaves them once in llk64 [U][G], and an iteration is a stream over
// those doubles (exact_em_counts_kernel, exact_em_combine_kernel) and one small launch per record (exact_em_update_kernel). ----

// The successor of an ascending genotype in VCF order: increment_genotype (jitutils.py:114-146) with constant indices, so that the
// alleles stay in registers.
template <int KM>
__device__ __forceinline__ void next_genotype(int (&g)[KM], int K) {
  int pos = K - 1;
  bool found = false;
#pragma unroll
  for (int i = 1; i < KM; i++)
    if (!found && i < K && g[i] != g[0]) {
      pos = i - 1;
      found = true;
    }
#pragma unroll
  for (int i = 0; i < KM; i++) {
    if (i == pos) g[i] += 1;
    else if (i < pos) g[i] = 0;
  }
}

struct ExactEmParams {
  const double *llk64;         // [U][G] stored log likelihoods
  const double *inbreeding;    // [U]
  const int32_t *unit_record;  // [U] the unit's record within the sub-block
  const int32_t *unit_slot;    // [U] the unit's row in the slab: (record, sample index)
  const double *freqs;         // [records][stride] the records' current frequency rows
  const int32_t *active;       // [records] 0: the record is frozen
  int stride;                  // doubles per frequency row and per slab row (>= H)
  int H, K, nblk;
  long long G;
  double *part;                // [U][nblk][H + 2]: block maximum of llk + log prior, sum and allele counts relative to it
  double *slab;                // [slots][stride]: expected allele counts K_s * freqs_s of every (record, sample)
};
// a thread's run of consecutive genotypes, and the row pitch of the staging tile in doubles: 17 is odd, so the 32 lanes of a
// half wavefront reading element j of their rows fall on 32 distinct bank pairs (ds_read_b64: bank = (byte / 4) % 64)
constexpr int EXACT_EM_RUN = EXACT_GENOS_PER_BLOCK / EXACT_THREADS;
constexpr int EXACT_EM_PITCH = EXACT_EM_RUN + 1;
inline size_t exact_em_lds(int H, int K) {
  return ((size_t)EXACT_THREADS * EXACT_EM_PITCH + (size_t)H * (K + 1) + (K + 1) + H + (size_t)(H + 1) * (EXACT_THREADS / 64) + 8) * 8;
}
// One workgroup per (unit, tile of 4096 genotypes).  The tile is loaded with consecutive lanes on consecutive genotypes (every
// wavefront load is 512 contiguous bytes) into LDS; each thread then owns EXACT_EM_RUN consecutive genotypes: one unranking, then
// the successor step.  The sums: a wavefront's 64 contributions by the shuffle reduction of pass 2 (wave_sum, fixed order), kept
// per wavefront in LDS, wavefronts in order here, blocks in order in exact_em_combine_kernel.  No atomics.
template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_em_counts_kernel(const ExactEmParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int rec = P.unit_record[unit];
  if (P.active[rec] == 0) return;  // (whole workgroup: the record is frozen, its slab rows stay)
  const int H = P.H, K = P.K;
  constexpr int NW = EXACT_THREADS / 64;
  double *tile = reinterpret_cast<double *>(smem);       // [EXACT_THREADS][EXACT_EM_PITCH]
  double *lgd = tile + EXACT_THREADS * EXACT_EM_PITCH;  // [H][K + 1]
  double *lgf = lgd + (size_t)H * (K + 1);
  double *lfreq = lgf + (K + 1);
  double *acc = lfreq + H;                               // [NW][H + 1]
  double *red = acc + (size_t)(H + 1) * NW;              // [NW] maxima, [1] left
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double *fr = P.freqs + (size_t)rec * P.stride;
  const double F = P.inbreeding[unit];
  {
    // the prior tables of exact_setup, from the unit's F and its record's current row
    const double scale = (1.0 - F) / F;
    for (int q = threadIdx.x; q < H * (K + 1); q += EXACT_THREADS) {
      const int h = q / (K + 1), d = q % (K + 1);
      const double alpha = fr[h] * scale;
      lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
    }
    for (int d = threadIdx.x; d <= K; d += EXACT_THREADS) lgf[d] = lgamma((double)d + 1.0);
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) lfreq[h] = fr[h];
    if (threadIdx.x == 0) {
      double sum_alpha = 0.0;
      for (int h = 0; h < H; h++) sum_alpha += fr[h] * scale;
      red[NW] = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
    }
    for (int i = threadIdx.x; i < NW * (H + 1); i += EXACT_THREADS) acc[i] = 0.0;
  }
  const long long G = P.G;
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double *src = P.llk64 + (size_t)unit * G;
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    const int e = threadIdx.x + t * EXACT_THREADS;  // element of the tile: consecutive lanes, consecutive genotypes
    if (lo + e < hi) tile[(e / EXACT_EM_RUN) * EXACT_EM_PITCH + (e % EXACT_EM_RUN)] = src[lo + e];
  }
  __syncthreads();
  PriorTab pt;
  pt.lgd = lgd;
  pt.lgf = lgf;
  pt.lfreq = lfreq;
  pt.left = red[NW];
  pt.lnH = log((double)H);
  pt.F = F;
  pt.has_freqs = 1;
  // llk + log prior of the thread's run, and the block's maximum
  const long long first = lo + (long long)threadIdx.x * EXACT_EM_RUN;
  lds_cdouble *mine = lds_table(tile) + threadIdx.x * EXACT_EM_PITCH;
  double lj[EXACT_EM_RUN];
  double m = -INFINITY;
  int g[KM], g0[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) g[k] = 0;
  if (first < hi) unrank_genotype(first, K, g);
#pragma unroll
  for (int k = 0; k < KM; k++) g0[k] = g[k];
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    lj[t] = -INFINITY;
    if (first + t < hi) {
      lj[t] = mine[t] + calling_log_prior(pt, g, K);
      if (lj[t] > m) m = lj[t];
      next_genotype(g, K);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, WAVE));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int w = 1; w < NW; w++) m = fmax(m, red[w]);
  // second walk over the run: exp(lj - m) into the sum and the allele counts
  double *wacc = acc + (size_t)wave * (H + 1);
#pragma unroll
  for (int k = 0; k < KM; k++) g[k] = g0[k];
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    const long long i0 = lo + (long long)(wave * 64) * EXACT_EM_RUN + t;  // the wavefront's first genotype of this step
    if (i0 >= hi) continue;                                               // (wave-uniform)
    const bool live = first + t < hi && lj[t] > -INFINITY;
    const double p = live ? exp(lj[t] - m) : 0.0;
    const double s = wave_sum(p);
    if (lane == 0) wacc[H] += s;
    for (int a = 0; a < H; a++) {
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < KM; k++) cnt += (k < K && g[k] == a) ? 1 : 0;
      const double c = wave_sum(live ? p * (double)cnt : 0.0);
      if (lane == 0) wacc[a] += c;
    }
    if (first + t < hi) next_genotype(g, K);
  }
  __syncthreads();
  double *out = P.part + ((size_t)unit * P.nblk + blk) * (H + 2);
  for (int h = threadIdx.x; h < H + 1; h += EXACT_THREADS) {
    double sum = 0.0;
    for (int w = 0; w < NW; w++) sum += acc[(size_t)w * (H + 1) + h];
    out[h] = sum;
  }
  if (threadIdx.x == 0) out[H + 1] = m;
}
// The blocks of a unit in order: the normaliser, then the unit's expected allele counts into its slab row.
static __global__ __launch_bounds__(64) void exact_em_combine_kernel(const ExactEmParams P) {
  const int unit = blockIdx.x;
  if (P.active[P.unit_record[unit]] == 0) return;
  const int H = P.H;
  const double *part = P.part + (size_t)unit * P.nblk * (H + 2);
  double m = -INFINITY;
  for (int q = 0; q < P.nblk; q++) m = fmax(m, part[(size_t)q * (H + 2) + H + 1]);
  double total = 0.0;
  for (int q = 0; q < P.nblk; q++) {
    const double mq = part[(size_t)q * (H + 2) + H + 1];
    if (mq > -INFINITY) total += part[(size_t)q * (H + 2) + H] * exp(mq - m);
  }
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    double sum = 0.0;
    for (int q = 0; q < P.nblk; q++) {
      const double mq = part[(size_t)q * (H + 2) + H + 1];
      if (mq > -INFINITY) sum += part[(size_t)q * (H + 2) + h] * exp(mq - m);
    }
    P.slab[(size_t)P.unit_slot[unit] * P.stride + h] = sum / total;
  }
}
struct ExactEmUpdateParams {
  const double *slab;         // [records][n_samples][stride]
  const int32_t *record_haps; // [records] H of the record
  int n_samples, stride, max_iterations;
  double ploidy_total, tolerance;
  double *freqs;              // [records][stride] in / out
  int32_t *iterations;        // [records] in / out
  int32_t *active;            // [records] in / out
  double *delta;              // [records] max |f' - f| of the record's last iteration, or null
};
// the larger of two |delta|, a NaN on either side kept (fmax would drop it)
__device__ __forceinline__ double em_delta_max(double d, double e) { return (e > d || e != e) ? e : d; }
// One workgroup per record: the samples' rows in sample order, the new row, max |delta|, the iteration counter, and the freeze.
// A NaN in the new row (a sample without a finite genotype: 0 / 0) makes max |delta| NaN, and NaN does not meet the tolerance, as
// application._em_update's `max |f' - f| < eps` is False for it: such a record runs max_iterations and keeps its NaN row.
static __global__ __launch_bounds__(64) void exact_em_update_kernel(const ExactEmUpdateParams P) {
  const int rec = blockIdx.x;
  if (P.active[rec] == 0) return;
  const int H = P.record_haps[rec];
  double *fr = P.freqs + (size_t)rec * P.stride;
  const double *rows = P.slab + (size_t)rec * P.n_samples * P.stride;
  double d = 0.0;
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    double sum = 0.0;
    for (int s = 0; s < P.n_samples; s++) sum += rows[(size_t)s * P.stride + h];
    const double f = sum / P.ploidy_total;
    d = em_delta_max(d, fabs(f - fr[h]));
    fr[h] = f;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) d = em_delta_max(d, __shfl_xor(d, o, WAVE));
  if (threadIdx.x == 0) {
    const int it = P.iterations[rec] + 1;
    P.iterations[rec] = it;
    if (P.delta) P.delta[rec] = d;
    if (d < P.tolerance || it >= P.max_iterations) P.active[rec] = 0;
  }
}

// ---- model evidence over stored likelihoods (application.ModelEvidence): evidence[u][n] = log sum_g P(g | K, F_n, f) P(reads | g),
// the normaliser of the unit's posterior under prior (F_n, f), for a grid of F_n per unit.  Every prior calling_log_prior forms is
// normalised, so the values compare across F and across ploidies.  As the estimate's iteration this is a stream over llk64 [U][G]
// under a changing prior: the tile is staged once and walked once per grid point. ----
struct ExactEvParams {
  const double *llk64;       // [U][G] stored log likelihoods
  const double *inbreeding;  // [U][n_grid], or null: the flat genotype prior (n_grid = 1), evidence = logsumexp(llk) - log(G)
  const int32_t *unit_row;   // [U] the unit's row of freqs
  const double *freqs;       // [rows][stride]
  int stride;                // doubles per frequency row (>= H)
  int H, K, nblk;
  int n_grid;                // grid points of every unit
  int chunk;                 // grid points whose prior tables are in the LDS together (exact_ev_chunk)
  long long G;
  double *part;              // [U][nblk][n_grid][2]: the tile's maximum of llk + log prior, and sum exp(. - maximum)
  double *evidence;          // [U][n_grid]
};
// LDS: the staging tile of the estimate, the wavefronts' maxima and sums, `chunk` lefts, lgf, lfreq, `chunk` tables lgd [H][K + 1]
inline size_t exact_ev_lds(int H, int K, int chunk) {
  return ((size_t)EXACT_THREADS * EXACT_EM_PITCH + (size_t)chunk * H * (K + 1) + (K + 1) + H + 2 * (EXACT_THREADS / 64) + (size_t)chunk) * 8;
}
// Grid points per chunk: as many as keep the workgroup within 64 KB of LDS (two workgroups to a CU), at least one -- a single
// table may take the LDS up to 160 KB --, 0 where not even one fits.
inline int exact_ev_chunk(int H, int K, int n_grid) {
  if (exact_ev_lds(H, K, 1) > 160 * 1024) return 0;
  int c = 1;
  while (c < n_grid && exact_ev_lds(H, K, c + 1) <= 64 * 1024) c++;
  return c;
}
// One workgroup per (unit, tile of 4096 genotypes).  The tile is staged as exact_em_counts_kernel stages it, each thread unranks the
// first genotype of its run once; then, chunk by chunk of the grid, the prior tables of the chunk's points are built and every point
// walks the run with next_genotype.  Sums: a wavefront's 64 terms by wave_sum, a thread's steps in order, wavefronts in order, tiles
// in order in exact_evidence_combine_kernel.  No atomics.
template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_evidence_kernel(const ExactEvParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K, NG = P.n_grid, chunk = P.chunk;
  constexpr int NW = EXACT_THREADS / 64;
  const bool has_prior = P.inbreeding != nullptr;
  double *tile = reinterpret_cast<double *>(smem);      // [EXACT_THREADS][EXACT_EM_PITCH]
  double *redm = tile + EXACT_THREADS * EXACT_EM_PITCH;  // [NW] maxima
  double *reds = redm + NW;                              // [NW] sums
  double *left = reds + NW;                              // [chunk]
  double *lgf = left + chunk;                            // [K + 1]
  double *lfreq = lgf + (K + 1);                         // [H]       (the flat prior's launch ends here: no tables, H counted 0)
  double *lgd = lfreq + H;                               // [chunk][H][K + 1]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double *fr = has_prior ? P.freqs + (size_t)P.unit_row[unit] * P.stride : nullptr;
  const double *Fs = has_prior ? P.inbreeding + (size_t)unit * NG : nullptr;
  const long long G = P.G;
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double *src = P.llk64 + (size_t)unit * G;
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    const int e = threadIdx.x + t * EXACT_THREADS;  // element of the tile: consecutive lanes, consecutive genotypes
    if (lo + e < hi) tile[(e / EXACT_EM_RUN) * EXACT_EM_PITCH + (e % EXACT_EM_RUN)] = src[lo + e];
  }
  if (has_prior) {
    for (int d = threadIdx.x; d <= K; d += EXACT_THREADS) lgf[d] = lgamma((double)d + 1.0);
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) lfreq[h] = fr[h];
  }
  const long long first = lo + (long long)threadIdx.x * EXACT_EM_RUN;
  lds_cdouble *mine = lds_table(tile) + threadIdx.x * EXACT_EM_PITCH;
  int g[KM], g0[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) g0[k] = 0;
  if (has_prior && first < hi) unrank_genotype(first, K, g0);
  double *out = P.part + ((size_t)unit * P.nblk + blk) * NG * 2;
  for (int n0 = 0; n0 < NG; n0 += chunk) {
    const int nc = (NG - n0 < chunk) ? NG - n0 : chunk;
    __syncthreads();  // (the tables of the chunk before have been read; the first time: nothing yet)
    if (has_prior) {
      // the prior tables of exact_setup for every point of the chunk, from the unit's row
      for (int q = threadIdx.x; q < nc * H * (K + 1); q += EXACT_THREADS) {
        const int c = q / (H * (K + 1)), r = q % (H * (K + 1));
        const int h = r / (K + 1), d = r % (K + 1);
        const double F = Fs[n0 + c];
        const double alpha = fr[h] * ((1.0 - F) / F);
        lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
      }
      // (a chunk of a small shape can hold more points than the workgroup has threads: 546 at H = 2, K = 2)
      for (int c = threadIdx.x; c < nc; c += EXACT_THREADS) {
        const double F = Fs[n0 + c];
        const double scale = (1.0 - F) / F;
        double sum_alpha = 0.0;
        for (int h = 0; h < H; h++) sum_alpha += fr[h] * scale;
        left[c] = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
      }
    }
    __syncthreads();
    for (int c = 0; c < nc; c++) {
      PriorTab pt;
      pt.lgd = lgd + (size_t)c * H * (K + 1);
      pt.lgf = lgf;
      pt.lfreq = lfreq;
      pt.left = has_prior ? left[c] : 0.0;
      pt.lnH = 0.0;
      pt.F = has_prior ? Fs[n0 + c] : 0.0;
      pt.has_freqs = 1;
      // llk + log prior of the thread's run, and the tile's maximum
      double lj[EXACT_EM_RUN];
      double m = -INFINITY;
#pragma unroll
      for (int k = 0; k < KM; k++) g[k] = g0[k];
#pragma unroll
      for (int t = 0; t < EXACT_EM_RUN; t++) {
        lj[t] = -INFINITY;
        if (first + t < hi) {
          lj[t] = mine[t];
          if (has_prior) {
            lj[t] += calling_log_prior(pt, g, K);
            next_genotype(g, K);
          }
          if (lj[t] > m) m = lj[t];
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, WAVE));
      if (lane == 0) redm[wave] = m;
      __syncthreads();
      m = redm[0];
#pragma unroll
      for (int w = 1; w < NW; w++) m = fmax(m, redm[w]);
      double s = 0.0;
#pragma unroll
      for (int t = 0; t < EXACT_EM_RUN; t++) s += wave_sum(lj[t] > -INFINITY ? exp(lj[t] - m) : 0.0);
      if (lane == 0) reds[wave] = s;
      __syncthreads();
      if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int w = 0; w < NW; w++) sum += reds[w];
        out[(size_t)(n0 + c) * 2] = m;
        out[(size_t)(n0 + c) * 2 + 1] = sum;  // (a tile without a finite entry: m = -inf, every term 0)
      }
    }
  }
}
// The tiles of a unit in order, one thread per grid point: evidence = maximum + log(total relative to it), -inf where no genotype
// is finite; the flat prior takes its constant -log(G) here.
static __global__ __launch_bounds__(64) void exact_evidence_combine_kernel(const ExactEvParams P) {
  const int unit = blockIdx.x;
  const int NG = P.n_grid;
  const double *part = P.part + (size_t)unit * P.nblk * NG * 2;
  for (int n = threadIdx.x; n < NG; n += blockDim.x) {
    double m = -INFINITY;
    for (int q = 0; q < P.nblk; q++) m = fmax(m, part[((size_t)q * NG + n) * 2]);
    double ev = -INFINITY;
    if (m > -INFINITY) {
      double total = 0.0;
      for (int q = 0; q < P.nblk; q++) {
        const double mq = part[((size_t)q * NG + n) * 2];
        if (mq > -INFINITY) total += part[((size_t)q * NG + n) * 2 + 1] * exp(mq - m);
      }
      ev = m + log(total);
      if (P.inbreeding == nullptr) ev -= log((double)P.G);
    }
    P.evidence[(size_t)unit * NG + n] = ev;
  }
}

// ---- SNV genotype posteriors over stored likelihoods (application.SnvCalls): snv_post[u][j][s] = sum_g p_u[g] [s_j(g) = s], the
// unit's haplotype-genotype posterior p[g] = exp(llk[g] + log prior[g] - log_norm) added to the SNV genotype that g implies at
// SNV j.  hap_alleles[h][j] is the SNV allele (0 .. A - 1, first appearance over the haplotypes) of haplotype h at SNV j; the
// SNV genotype of g at j is the multiset of its K haplotypes' alleles, s_j(g) its rank in VCF order among the S = C(A + K - 1, K)
// genotypes over A alleles.  log_norm is the model evidence of the unit at its own F (exact_evidence_kernel, one grid point): a
// first pass.  The second pass adds every p[g] as a 64-bit fixed-point integer with SNV_FRACTION_BITS = 62 fraction bits,
// q[g] = rint(p[g] * 2^62): integer addition is associative, so the LDS integer atomics, the tiles' sums and hence the result do
// not depend on the order anything ran in -- equal inputs give equal bits.  The sum of all q stays below 2^63 (sum p = 1 up to the
// rounding of log_norm).  Quantisation: |q[g] 2^-62 - p[g]| <= 2^-63, so an entry of snv_post is off by less than G * 2^-62
// (1.2e-14 at 54 264 genotypes) plus the rounding of the final conversion to double (2^-53 relative). ----
constexpr int SNV_FRACTION_BITS = 62;
constexpr int SNV_MAX_ALLELES = 4;
struct ExactSnvParams {
  const double *llk64;        // [U][G] stored log likelihoods
  const double *inbreeding;   // [U], or null: the flat genotype prior -log(G)
  const int32_t *unit_row;    // [U] the unit's row of freqs and of hap_alleles
  const double *freqs;        // [rows][stride] (not read under the flat prior)
  const int8_t *hap_alleles;  // [rows][H][M]
  int stride;
  int H, K, M, A, S, nblk;
  int chunk;                  // SNVs whose bins are in the LDS together (exact_snv_chunk)
  long long G;
  const double *log_norm;     // [U] the first pass' result
  unsigned long long *part;   // [U][nblk][M][S] the tiles' fixed-point sums
  double *snv_post;           // [U][M][S]
  double *log_norm_out;       // [U] or null
};
// LDS: the prior tables of one F (lgd [H][K + 1], lgf, lfreq, left), the chunk's SNV alleles [H][chunk] as bytes, then ONE region
// that first is the staging tile and, once every thread holds the fixed-point posteriors of its run in registers, the bins
// [chunk][S] of 64-bit sums
inline size_t exact_snv_lds(int H, int K, int S, int chunk) {
  const size_t tile = (size_t)EXACT_THREADS * EXACT_EM_PITCH * 8, bins = (size_t)chunk * S * 8;
  return ((size_t)H * (K + 1) + (K + 1) + H + 1) * 8 + (((size_t)H * chunk + 7) & ~(size_t)7) + (bins > tile ? bins : tile);
}
// SNVs per chunk: as many as keep the workgroup within 64 KB of LDS, at least one -- a single SNV may take the LDS up to 160 KB --,
// 0 where not even one fits
inline int exact_snv_chunk(int H, int K, int S, int M) {
  if (exact_snv_lds(H, K, S, 1) > 160 * 1024) return 0;
  int c = 1;
  while (c < M && exact_snv_lds(H, K, S, c + 1) <= 64 * 1024) c++;
  return c;
}
// Rank in VCF order of the SNV genotype with c[a] copies of allele a, the four counts packed one to a byte.  The ascending
// genotype holds allele a at positions p_a .. q_a - 1 (p_a = c_0 + .. + c_{a-1}, q_a = p_a + c_a), and rank_genotype's sum of
// C(a + i, i + 1) over those positions is C(a + q_a, a) - C(a + p_a, a).
__device__ __forceinline__ int snv_rank(unsigned packed) {
  const int c0 = packed & 255, c1 = (packed >> 8) & 255, c2 = (packed >> 16) & 255, c3 = packed >> 24;
  const int p2 = c0 + c1, p3 = p2 + c2, q3 = p3 + c3;
  auto t2 = [](int n) { return (n + 2) * (n + 1) / 2; };
  auto t3 = [](int n) { return (n + 3) * (n + 2) * (n + 1) / 6; };
  return c1 + (t2(p3) - t2(p2)) + (t3(q3) - t3(p3));
}
// One workgroup per (unit, tile of 4096 genotypes).  The tile is staged as exact_evidence_kernel stages it; each thread unranks
// the first genotype of its run, walks it once with next_genotype for the fixed-point posteriors, and then once per SNV of every
// chunk: the SNV alleles of the genotype's K haplotypes counted from the staged table, the counts ranked, and the posterior added
// to that bin -- consecutive genotypes of a run that fall in the same bin are added in registers first, one atomic per change.
template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_snv_kernel(const ExactSnvParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K, M = P.M, S = P.S, chunk = P.chunk;
  const bool has_prior = P.inbreeding != nullptr;
  double *lgd = reinterpret_cast<double *>(smem);  // [H][K + 1]
  double *lgf = lgd + (size_t)H * (K + 1);         // [K + 1]
  double *lfreq = lgf + (K + 1);                   // [H]
  double *left = lfreq + H;                        // [1]
  int8_t *ha = reinterpret_cast<int8_t *>(left + 1);  // [H][chunk]
  double *tile = reinterpret_cast<double *>(ha + (((size_t)H * chunk + 7) & ~(size_t)7));  // [EXACT_THREADS][EXACT_EM_PITCH]
  unsigned long long *bins = reinterpret_cast<unsigned long long *>(tile);                 // [chunk][S], after the tile
  const int row = P.unit_row[unit];
  const double *fr = has_prior ? P.freqs + (size_t)row * P.stride : nullptr;
  const double F = has_prior ? P.inbreeding[unit] : 0.0;
  const long long G = P.G;
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double *src = P.llk64 + (size_t)unit * G;
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    const int e = threadIdx.x + t * EXACT_THREADS;  // element of the tile: consecutive lanes, consecutive genotypes
    if (lo + e < hi) tile[(e / EXACT_EM_RUN) * EXACT_EM_PITCH + (e % EXACT_EM_RUN)] = src[lo + e];
  }
  if (has_prior) {
    // the prior tables of exact_setup, from the unit's F and its row
    const double scale = (1.0 - F) / F;
    for (int q = threadIdx.x; q < H * (K + 1); q += EXACT_THREADS) {
      const int h = q / (K + 1), d = q % (K + 1);
      const double alpha = fr[h] * scale;
      lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
    }
    for (int d = threadIdx.x; d <= K; d += EXACT_THREADS) lgf[d] = lgamma((double)d + 1.0);
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) lfreq[h] = fr[h];
    if (threadIdx.x == 0) {
      double sum_alpha = 0.0;
      for (int h = 0; h < H; h++) sum_alpha += fr[h] * scale;
      left[0] = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
    }
  }
  __syncthreads();
  PriorTab pt;
  pt.lgd = lgd;
  pt.lgf = lgf;
  pt.lfreq = lfreq;
  pt.left = has_prior ? left[0] : 0.0;
  pt.lnH = 0.0;
  pt.F = F;
  pt.has_freqs = 1;
  const double norm = P.log_norm[unit];
  const double flat = has_prior ? 0.0 : -log((double)G);
  const long long first = lo + (long long)threadIdx.x * EXACT_EM_RUN;
  lds_cdouble *mine = lds_table(tile) + threadIdx.x * EXACT_EM_PITCH;
  int g[KM], g0[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) g0[k] = 0;
  if (first < hi) unrank_genotype(first, K, g0);
  // the fixed-point posteriors of the thread's run (0 past the tile's end, for a genotype of probability 0 and for a unit
  // without a finite genotype: its rows are set to NaN by exact_snv_combine_kernel)
  unsigned long long q[EXACT_EM_RUN];
#pragma unroll
  for (int k = 0; k < KM; k++) g[k] = g0[k];
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    q[t] = 0;
    if (first + t < hi) {
      const double lj = mine[t] + (has_prior ? calling_log_prior(pt, g, K) : flat);
      const double p = exp(lj - norm);
      if (p > 0.0) q[t] = (unsigned long long)rint(fmin(ldexp(p, SNV_FRACTION_BITS), 9.0e18));  // (false for NaN)
      next_genotype(g, K);
    }
  }
  unsigned long long *out = P.part + ((size_t)unit * P.nblk + blk) * (size_t)M * S;
  const int8_t *ua = P.hap_alleles + (size_t)row * H * M;
  for (int j0 = 0; j0 < M; j0 += chunk) {
    const int mc = (M - j0 < chunk) ? M - j0 : chunk;
    __syncthreads();  // (the tile has been read; later: the bins of the chunk before have been written out)
    for (int i = threadIdx.x; i < mc * S; i += EXACT_THREADS) bins[i] = 0;
    for (int i = threadIdx.x; i < H * mc; i += EXACT_THREADS) {
      const int h = i / mc, c = i % mc;
      const int a = ua[(size_t)h * M + j0 + c];
      ha[i] = (int8_t)(a < 0 ? 0 : (a >= P.A ? P.A - 1 : a));  // (a value outside the table's range cannot leave the bins)
    }
    __syncthreads();
    for (int c = 0; c < mc; c++) {
      unsigned long long *bin = bins + (size_t)c * S;
      int cur = -1;
      unsigned long long acc = 0;
#pragma unroll
      for (int k = 0; k < KM; k++) g[k] = g0[k];
#pragma unroll
      for (int t = 0; t < EXACT_EM_RUN; t++) {
        if (first + t < hi) {
          unsigned packed = 0;
#pragma unroll
          for (int k = 0; k < KM; k++)
            if (k < K) packed += 1u << (8 * ha[g[k] * mc + c]);
          const int s = snv_rank(packed);
          if (s != cur) {
            if (acc) atomicAdd(bin + cur, acc);
            cur = s;
            acc = 0;
          }
          acc += q[t];
          next_genotype(g, K);
        }
      }
      if (acc) atomicAdd(bin + cur, acc);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < mc * S; i += EXACT_THREADS) out[(size_t)j0 * S + i] = bins[i];
  }
}
// The tiles of a unit summed (integers: any order gives the same sum) and scaled back to a probability; NaN for a unit without a
// finite genotype.
static __global__ __launch_bounds__(EXACT_THREADS) void exact_snv_combine_kernel(const ExactSnvParams P) {
  const size_t MS = (size_t)P.M * P.S;
  const unsigned nx = (unsigned)((MS + EXACT_THREADS - 1) / EXACT_THREADS);  // workgroups of a unit
  const int unit = blockIdx.x / nx, bx = blockIdx.x % nx;
  const double norm = P.log_norm[unit];
  if (P.log_norm_out && bx == 0 && threadIdx.x == 0) P.log_norm_out[unit] = norm;
  const size_t i = (size_t)bx * EXACT_THREADS + threadIdx.x;
  if (i >= MS) return;
  const unsigned long long *part = P.part + (size_t)unit * P.nblk * MS;
  unsigned long long sum = 0;
  for (int b = 0; b < P.nblk; b++) sum += part[(size_t)b * MS + i];
  P.snv_post[(size_t)unit * MS + i] = (norm > -INFINITY && norm < INFINITY) ? ldexp((double)sum, -SNV_FRACTION_BITS) : NAN;
}

}  // namespace mchap
