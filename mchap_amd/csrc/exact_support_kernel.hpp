// Expected read depth of every haplotype (call-exact --allele-depths, application.AlleleDepths) for MI355X (gfx950): a second
// enumeration over (genotype x read) on top of exact_kernel.hpp's helpers, over the likelihoods the exact caller left in llk64.
//   p[g]       = exp(llk[g] + log prior[g] - log_norm)                  the calling posterior, as exact_snv_kernel forms it
//   D(r, g)    = sum_h c_h(g) P[r][h]                                   P[r][h] the product of exact_setup (a common scale cancels)
//   post[r][h] = sum_g p[g] c_h(g) P[r][h] / D(r, g)                    rows of weight 0: exactly 0
//   depth[h]   = sum_r w_r post[r][h]
// A pair (g, r) contributes only where p[g] > 0 and w_r > 0, and 0 where D(r, g) is 0 nevertheless.  log_norm is the model
// evidence of the unit at its own F (exact_evidence_kernel, one grid point): a first pass, as for the SNV posteriors.
//
// One workgroup per (unit, tile of EXACT_GENOS_PER_BLOCK genotypes).  The tile's llk is staged as exact_evidence_kernel stages it;
// every thread forms p of its run of consecutive genotypes (one unranking, then next_genotype) and puts it back in place.  The read
// rows are then worked in tiles of RT rows (mchap_exact_support_tile, a multiple of 64): P transposed [H][RT] and an accumulator
// [H][RT] in LDS.  Wavefront w owns the rows 64 c .. 64 c + 63 of the tile for c = w, w + 4, ..: one lane per row.  It walks the
// tile's genotypes in order, the genotype uniform over the wavefront: 64 staged p at a time, one ballot, and only the genotypes
// with p > 0 are visited (with deep reads nearly all are 0: a skipped group of 64 costs one LDS read and one ballot).  A visited
// genotype is the successor of the one before (next_genotype), or it is reached from the first genotype of its thread's run --
// kept packed in LDS, a byte per allele, when the run was unranked -- in at most 15 successor steps: unranking anew is K H
// 64-bit divisions and took nine tenths of the first version's time.  The K reads P[a_k][row] of a lane are
// consecutive doubles over the lanes -- conflict-free ds_read_b64 --, one divide gives p / D, and every distinct haplotype of the
// genotype gets its share added to the lane's own accumulator cell.  Every cell has one owner: no atomics, a fixed order.
// Without read_post the workgroup reduces over its rows (wave_sum's tree) and writes [H] partials; with it, [R][H] partials.  The
// tiles of a unit are combined in tile order by exact_support_combine_kernel.  Nothing depends on the unit's place in the batch.
#pragma once
#include "exact_kernel.hpp"

namespace mchap {

typedef __attribute__((address_space(3))) double lds_double;

struct ExactSupportParams {
  const double *reads;       // [U][R][M][A]
  const int64_t *counts;     // [U][R] or null (every weight 1)
  const int8_t *haps;        // [U][H][M]
  const double *llk64;       // [U][G] stored log likelihoods
  const double *inbreeding;  // [U], or null: the flat genotype prior -log(G)
  const int32_t *unit_row;   // [U] the unit's row of freqs (not read under the flat prior)
  const double *freqs;       // [rows][stride]
  int stride;
  int R, M, A, H, K, nblk;
  int RT;                    // read rows per LDS tile (a multiple of 64)
  long long G;
  const double *log_norm;    // [U] the first pass' result
  double *part;              // [U][nblk][H], or with read_post [U][nblk][R][H]
  double *depth;             // [U][H]
  double *read_post;         // [U][R][H] or null
  double *log_norm_out;      // [U] or null
};
// LDS in doubles: the staging tile (then p), the runs' first genotypes (16 bytes each), the prior tables of one F (lgd [H][K + 1],
// lgf, lfreq, left), the workgroup's depth sums [H], the tile's read weights [RT], P [H][RT], the accumulator [H][RT]
inline size_t exact_support_lds(int H, int K, int RT) {
  return ((size_t)EXACT_THREADS * EXACT_EM_PITCH + (size_t)EXACT_THREADS * 2 + (size_t)H * (K + 1) + (K + 1) + 2 * (size_t)H + 1 + (size_t)RT + 2 * (size_t)H * RT) * 8;
}
// Read rows per tile: the largest multiple of 64, no more than the reads need, that keeps the workgroup within 64 KB of LDS; a
// single tile of 64 rows may take up to 160 KB; 0 where not even that fits.
inline int exact_support_rows(int R, int H, int K) {
  const int cap = (R + 63) / 64 * 64;
  int rt = 0;
  if (H > 255) return 0;  // (a byte per allele in the packed genotypes; the tables of 64 rows end near 120 haplotypes anyway)
  while (rt + 64 <= cap && exact_support_lds(H, K, rt + 64) <= 64 * 1024) rt += 64;
  if (rt == 0 && exact_support_lds(H, K, 64) <= 160 * 1024) rt = 64;
  return rt;
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_support_kernel(const ExactSupportParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K, M = P.M, A = P.A, R = P.R, RT = P.RT;
  constexpr int NW = EXACT_THREADS / 64;
  const bool has_prior = P.inbreeding != nullptr;
  double *tile = reinterpret_cast<double *>(smem);        // [EXACT_THREADS][EXACT_EM_PITCH]: llk, then p
  unsigned *gstart = reinterpret_cast<unsigned *>(tile + EXACT_THREADS * EXACT_EM_PITCH);  // [EXACT_THREADS][4]
  double *lgd = tile + EXACT_THREADS * EXACT_EM_PITCH + EXACT_THREADS * 2;   // [H][K + 1]
  double *lgf = lgd + (size_t)H * (K + 1);                // [K + 1]
  double *lfreq = lgf + (K + 1);                          // [H]
  double *left = lfreq + H;                               // [1]
  double *dsum = left + 1;                                // [H]
  double *wgt = dsum + H;                                 // [RT]
  double *ptab = wgt + RT;                                // [H][RT]
  double *acc = ptab + (size_t)H * RT;                    // [H][RT]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double *fr = has_prior ? P.freqs + (size_t)P.unit_row[unit] * P.stride : nullptr;
  const double F = has_prior ? P.inbreeding[unit] : 0.0;
  const long long G = P.G;
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const int ntile = (int)(hi - lo);
  const double *src = P.llk64 + (size_t)unit * G;
#pragma unroll
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    const int e = threadIdx.x + t * EXACT_THREADS;  // element of the tile: consecutive lanes, consecutive genotypes
    if (e < ntile) tile[(e / EXACT_EM_RUN) * EXACT_EM_PITCH + (e % EXACT_EM_RUN)] = src[lo + e];
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
  for (int h = threadIdx.x; h < H; h += EXACT_THREADS) dsum[h] = 0.0;
  __syncthreads();
  {
    // p of the thread's run, in place of its llk (0 for a genotype of probability 0 or NaN, and for a unit without a finite
    // genotype: its outputs are set to NaN by exact_support_combine_kernel)
    PriorTab pt;
    pt.lgd = lgd;
    pt.lgf = lgf;
    pt.lfreq = lfreq;
    pt.left = has_prior ? left[0] : 0.0;
    pt.lnH = 0.0;
    pt.F = F;
    pt.has_freqs = 1;
    const double norm = P.log_norm[unit];
    const bool finite_norm = norm > -INFINITY && norm < INFINITY;
    const double flat = has_prior ? 0.0 : -log((double)G);
    const int first = threadIdx.x * EXACT_EM_RUN;
    double *mine = tile + threadIdx.x * EXACT_EM_PITCH;
    int g[KM];
#pragma unroll
    for (int k = 0; k < KM; k++) g[k] = 0;
    if (first < ntile) unrank_genotype(lo + first, K, g);
    {
      unsigned packed[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < KM; k++) packed[k >> 2] |= (unsigned)g[k] << (8 * (k & 3));
#pragma unroll
      for (int q = 0; q < 4; q++) gstart[threadIdx.x * 4 + q] = packed[q];
    }
#pragma unroll
    for (int t = 0; t < EXACT_EM_RUN; t++) {
      if (first + t < ntile) {
        const double lj = mine[t] + (has_prior ? calling_log_prior(pt, g, K) : flat);
        const double p = finite_norm ? exp(lj - norm) : 0.0;
        mine[t] = p > 0.0 ? p : 0.0;  // (NaN: 0)
        next_genotype(g, K);
      }
    }
  }
  const double *reads = P.reads + (size_t)unit * R * M * A;
  const int8_t *haps = P.haps + (size_t)unit * H * M;
  lds_cdouble *ltile = lds_table(tile), *lwgt = lds_table(wgt);
  for (int r0 = 0; r0 < R; r0 += RT) {
    const int rn = min(RT, R - r0);
    __syncthreads();  // (p is in place; later: the tile of rows before has been written out)
    for (int q = threadIdx.x; q < H * RT; q += EXACT_THREADS) {
      const int h = q / RT, r = q % RT;
      double prod = 1.0;
      if (r < rn) {
        for (int j = 0; j < M; j++) {
          const double v = reads[((size_t)(r0 + r) * M + j) * A + haps[h * M + j]];
          if (!isnan(v)) prod *= v;  // assemble/likelihood.py:54-59, as exact_setup
        }
      }
      ptab[q] = prod;
      acc[q] = 0.0;
    }
    for (int r = threadIdx.x; r < RT; r += EXACT_THREADS)
      wgt[r] = r < rn ? (P.counts ? (double)P.counts[(size_t)unit * R + r0 + r] : 1.0) : 0.0;
    __syncthreads();
    for (int c = wave; c * 64 < rn; c += NW) {
      const int row = c * 64 + lane;  // (< RT: rn <= RT and RT is a multiple of 64)
      const bool on = lwgt[row] > 0.0;
      if (!__any(on)) continue;
      lds_cdouble *prow = lds_table(ptab) + row;
      lds_double *arow = (lds_double *)acc + row;  // (LDS-qualified as lds_table's: ds_read / ds_write, not flat)
      int g[KM];
#pragma unroll
      for (int k = 0; k < KM; k++) g[k] = 0;
      int cur = -2;
      for (int base = 0; base < ntile; base += 64) {
        const int e = base + lane;
        const double pv = e < ntile ? ltile[(e / EXACT_EM_RUN) * EXACT_EM_PITCH + (e % EXACT_EM_RUN)] : 0.0;
        unsigned long long live = __ballot(pv > 0.0);
        while (live) {
          const int i = base + __builtin_ctzll(live);  // wave-uniform
          live &= live - 1;
          if (i == cur + 1) {
            next_genotype(g, K);
          } else {
            // from the first genotype of the run that holds i (wave-uniform LDS reads), at most 15 steps on
            const int run = i / EXACT_EM_RUN;
#pragma unroll
            for (int k = 0; k < KM; k++) g[k] = (int)((gstart[run * 4 + (k >> 2)] >> (8 * (k & 3))) & 255u);
            for (int s = run * EXACT_EM_RUN; s < i; s++) next_genotype(g, K);
          }
          cur = i;
          const double p = ltile[(i / EXACT_EM_RUN) * EXACT_EM_PITCH + (i % EXACT_EM_RUN)];
          double ph[KM];
          double D = 0.0;
#pragma unroll
          for (int k = 0; k < KM; k++)
            if (k < K) {
              ph[k] = prow[g[k] * RT];
              D += ph[k];
            }
          const double q = (on && D > 0.0) ? p / D : 0.0;
          // the runs of the ascending genotype: haplotype g[k] with its dosage, at the run's last copy
          int cnt = 0;
#pragma unroll
          for (int k = 0; k < KM; k++)
            if (k < K) {
              cnt++;
              const bool last = (k == K - 1) || (k + 1 < KM && g[k + 1] != g[k]);
              if (last) {
                arow[g[k] * RT] += (double)cnt * (q * ph[k]);
                cnt = 0;
              }
            }
        }
      }
    }
    __syncthreads();
    if (P.read_post) {
      double *out = P.part + (((size_t)unit * P.nblk + blk) * R + r0) * H;
      for (int q = threadIdx.x; q < rn * H; q += EXACT_THREADS) {
        const int r = q / H, h = q % H;
        out[q] = wgt[r] > 0.0 ? acc[h * RT + r] : 0.0;
      }
    } else {
      for (int h = wave; h < H; h += NW) {
        double v = 0.0;
        for (int r = lane; r < rn; r += 64) v += wgt[r] * acc[h * RT + r];
        const double s = wave_sum(v);
        if (lane == 0) dsum[h] += s;  // (haplotype h belongs to this wavefront in every tile of rows)
      }
    }
  }
  if (!P.read_post) {
    __syncthreads();
    double *out = P.part + ((size_t)unit * P.nblk + blk) * H;
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) out[h] = dsum[h];
  }
}

// The tiles of a unit in tile order.  With read_post: post[r][h] first, then depth[h] = sum_r w_r post[r][h] over the rows in
// order; without: depth[h] from the tiles' own sums.  NaN everywhere for a unit without a finite genotype.
static __global__ __launch_bounds__(EXACT_THREADS) void exact_support_combine_kernel(const ExactSupportParams P) {
  const int unit = blockIdx.x;
  const int H = P.H, R = P.R;
  const double norm = P.log_norm[unit];
  const bool finite_norm = norm > -INFINITY && norm < INFINITY;
  if (P.log_norm_out && threadIdx.x == 0) P.log_norm_out[unit] = norm;
  if (P.read_post) {
    const size_t RH = (size_t)R * H;
    const double *part = P.part + (size_t)unit * P.nblk * RH;
    double *post = P.read_post + (size_t)unit * RH;
    for (size_t i = threadIdx.x; i < RH; i += EXACT_THREADS) {
      double sum = 0.0;
      for (int b = 0; b < P.nblk; b++) sum += part[(size_t)b * RH + i];
      post[i] = finite_norm ? sum : NAN;
    }
    __syncthreads();  // (the rows this workgroup has just written)
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) {
      double sum = 0.0;
      for (int r = 0; r < R; r++) {
        const double w = P.counts ? (double)P.counts[(size_t)unit * R + r] : 1.0;
        if (w > 0.0) sum += w * post[(size_t)r * H + h];
      }
      P.depth[(size_t)unit * H + h] = finite_norm ? sum : NAN;
    }
  } else {
    const double *part = P.part + (size_t)unit * P.nblk * H;
    for (int h = threadIdx.x; h < H; h += EXACT_THREADS) {
      double sum = 0.0;
      for (int b = 0; b < P.nblk; b++) sum += part[(size_t)b * H + h];
      P.depth[(size_t)unit * H + h] = finite_norm ? sum : NAN;
    }
  }
}

}  // namespace mchap
