// Progeny calls under their parents' cross prior (call-exact --cross-calls, application.CrossCalls) for MI355X (gfx950): three
// enumerations on top of exact_kernel.hpp's helpers, over the likelihoods the exact caller left in llk64.  Per record with H
// haplotypes, parents P and Q of even ploidies K_P and K_Q, gametes of t = K / 2 haplotypes, progeny of ploidy K_c = t_P + t_Q:
//   p[g]     = exp(llk[g] + log prior[g] - log_norm)                          the parent's calling posterior, as exact_snv_kernel forms it
//   gam[a]   = (sum_{g = a + r} p[g] prod_h C(c_h(g), a_h)) / C(K, t)          over the complements r of a, in VCF order of r
//   gam'[a]  = (1 - e) gam[a] + e Mult(a; t, f)                               e the gamete error, f the record's calling frequencies
//   X[gc]    = sum_{a in gc, |a| = t_P} gam'_P[a] gam'_Q[gc - a]              over the distinct sub-multisets a, in VCF order of a
//   q[gc]    = X[gc] exp(llk_c[gc]) / Z                                       log Z the cross evidence
// log_norm is the model evidence of the unit at its own F (exact_evidence_kernel, one grid point): a first pass, as for the SNV
// posteriors and the allele support.  No double reduction, and the two parents enter as independent tables.
//
// All three kernels are gather-form: every output cell has one owning lane and a fixed summation order, no atomics, and nothing
// depends on a unit's place in the batch -- equal inputs give equal bits whatever the order of the units.
//   exact_gamete_kernel      one lane per gamete a, workgroups over (parent unit, 256 gametes).  The lane walks the
//                            C(H + K - t - 1, K - t) complements with next_genotype -- the same trip count in every lane --, merges
//                            a and r into the ascending genotype, ranks it on the way and reads p of that genotype.
//   exact_cross_prior_kernel one lane per progeny genotype, workgroups over (record row, 256 genotypes).  The lane walks the
//                            bounded compositions (a_1 .. a_m) of t_P over the dosages of gc's m distinct alleles with the highest
//                            allele most significant -- that is VCF order of a -- and ranks a and gc - a in the two gamete tables,
//                            which are staged in LDS where both fit 64 KB and read from global memory otherwise.
//   exact_cross_post_kernel  one workgroup per (progeny unit, tile of EXACT_GENOS_PER_BLOCK genotypes): the tile's first maximum of
//                            llk + log X and its sum relative to it; exact_cross_post_combine_kernel takes the tiles in tile order.
#pragma once
#include <climits>

#include "exact_kernel.hpp"

namespace mchap {

constexpr int CROSS_BIN = EXACT_KMAX + 1;  // binomials C(n, k) for n, k <= EXACT_KMAX

struct ExactGameteParams {
  const double *llk64;       // [U][G] stored log likelihoods
  const double *inbreeding;  // [U], or null: the flat genotype prior -log(G)
  const int32_t *unit_row;   // [U] the unit's row of freqs
  const double *freqs;       // [rows][stride]: read under the flat prior too (the gamete error's multinomial)
  const double *error;       // [U] gamete error e
  int stride;
  int H, K, T, nblk;         // T = K / 2; nblk tiles of EXACT_THREADS gametes
  long long G, NA, NR;       // genotypes, gametes C(H + T - 1, T), complements C(H + K - T - 1, K - T)
  const double *log_norm;    // [U] the first pass' result
  double *gametes;           // [U][NA]
  double *log_norm_out;      // [U] or null
};
// LDS in doubles: the prior tables of one F (lgd [H][K + 1], lgf, lfreq, left) and the binomials (ints, two to a double)
inline size_t exact_gamete_lds(int H, int K) {
  return ((size_t)H * (K + 1) + (K + 1) + (size_t)H + 1 + (CROSS_BIN * CROSS_BIN + 1) / 2) * 8;
}

// The LDS tables of a unit of ploidy K over H haplotypes with frequencies fr [H] (exact_gamete_lds bytes at smem): the prior tables
// of exact_setup at inbreeding F (has_prior; the flat genotype prior has none), the frequencies themselves, and the binomials
// bin[n * CROSS_BIN + k] = C(n, k).  Ends with the workgroup's barrier.
__device__ __forceinline__ void cross_setup(unsigned char *smem, int H, int K, bool has_prior, double F, const double *fr, PriorTab &pt,
                                            int *&bin) {
  double *lgd = reinterpret_cast<double *>(smem);  // [H][K + 1]
  double *lgf = lgd + (size_t)H * (K + 1);         // [K + 1]
  double *lfreq = lgf + (K + 1);                   // [H]
  double *left = lfreq + H;                        // [1]
  bin = reinterpret_cast<int *>(left + 1);         // [CROSS_BIN][CROSS_BIN]
  if (has_prior) {
    // the prior tables of exact_setup, from the unit's F and its row
    const double scale = (1.0 - F) / F;
    for (int q = threadIdx.x; q < H * (K + 1); q += EXACT_THREADS) {
      const int h = q / (K + 1), d = q % (K + 1);
      const double alpha = fr[h] * scale;
      lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
    }
    for (int d = threadIdx.x; d <= K; d += EXACT_THREADS) lgf[d] = lgamma((double)d + 1.0);
    if (threadIdx.x == 0) {
      double sum_alpha = 0.0;
      for (int h = 0; h < H; h++) sum_alpha += fr[h] * scale;
      left[0] = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
    }
  }
  for (int h = threadIdx.x; h < H; h += EXACT_THREADS) lfreq[h] = fr[h];
  for (int q = threadIdx.x; q < CROSS_BIN * CROSS_BIN; q += EXACT_THREADS) {
    const int n = q / CROSS_BIN, k = q % CROSS_BIN;
    int b = k <= n ? 1 : 0;
    for (int i = 1; i <= k && k <= n; i++) b = b * (n - k + i) / i;  // (exact at every step: a binomial times i, below 2^31)
    bin[q] = b;
  }
  __syncthreads();
  pt.lgd = lgd;
  pt.lgf = lgf;
  pt.lfreq = lfreq;
  pt.left = has_prior ? left[0] : 0.0;
  pt.lnH = 0.0;
  pt.F = F;
  pt.has_freqs = 1;
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_gamete_kernel(const ExactGameteParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K, T = P.T, KR = P.K - P.T;
  const bool has_prior = P.inbreeding != nullptr;
  const double *fr = P.freqs + (size_t)P.unit_row[unit] * P.stride;
  const double F = has_prior ? P.inbreeding[unit] : 0.0;
  PriorTab pt;
  int *bin;
  cross_setup(smem, H, K, has_prior, F, fr, pt, bin);
  const double *lfreq = pt.lfreq;
  const double norm = P.log_norm[unit];
  const bool finite_norm = norm > -INFINITY && norm < INFINITY;
  const double flat = has_prior ? 0.0 : -log((double)P.G);
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  const bool on = idx < P.NA;
  int a[KM], r[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) a[k] = r[k] = 0;
  if (on) unrank_genotype(idx, T, a);
  const double *llk = P.llk64 + (size_t)unit * P.G;
  double sum = 0.0;
  for (long long c = 0; c < P.NR; c++) {  // (the same trip count in every lane; a lane past the last gamete walks gamete 0 and writes nothing)
    // a and r merged into the ascending genotype, ranked on the way (rank_genotype's sum)
    int g[KM];
    int ia = 0, ir = 0;
    long long rank = 0;
    for (int k = 0; k < K; k++) {
      const bool take = ir >= KR || (ia < T && a[ia] <= r[ir]);
      const int v = take ? a[ia] : r[ir];
      ia += take ? 1 : 0;
      ir += take ? 0 : 1;
      g[k] = v;
      rank += cwr(v, k + 1);
    }
    // prod_h C(c_h(g), a_h) over the runs of a: the run's length x and the copies y of its haplotype in r
    int w = 1, x = 0;
    for (int i = 0; i < T; i++) {
      x++;
      if (i == T - 1 || a[i + 1] != a[i]) {
        int y = 0;
        for (int j = 0; j < KR; j++) y += r[j] == a[i] ? 1 : 0;
        w *= bin[(x + y) * CROSS_BIN + x];
        x = 0;
      }
    }
    if (on && finite_norm) {
      const double lj = llk[rank] + (has_prior ? calling_log_prior(pt, g, K) : flat);
      const double p = exp(lj - norm);
      sum += (p > 0.0 ? p : 0.0) * (double)w;  // (NaN: 0)
    }
    next_genotype(r, KR);
  }
  if (!on) return;
  // Mult(a; T, f): the multinomial coefficient from the runs of a, the frequencies multiplied in the order of a
  double coef = 1.0, pf = 1.0;
  {
    int x = 0;
    for (int i = 0; i < T; i++) {
      x++;
      pf *= lfreq[a[i]];
      if (i == T - 1 || a[i + 1] != a[i]) {
        coef *= (double)bin[(i + 1) * CROSS_BIN + x];
        x = 0;
      }
    }
  }
  const double e = P.error[unit];
  const double gam = sum / (double)bin[K * CROSS_BIN + T];
  P.gametes[(size_t)unit * P.NA + idx] = finite_norm ? (1.0 - e) * gam + e * (coef * pf) : NAN;
  if (P.log_norm_out && idx == 0) P.log_norm_out[unit] = norm;
}

struct ExactCrossPriorParams {
  const double *gam_p;  // [rows][NAP]
  const double *gam_q;  // [rows][NAQ]
  int H, TP, TQ, nblk;  // nblk tiles of EXACT_THREADS progeny genotypes
  int staged;           // the two tables of a row fit the LDS
  long long NAP, NAQ, GC;
  double *log_x;        // [rows][GC]
};
// the two gamete tables of a row in LDS, where they fit the working budget of 64 KB
inline size_t exact_cross_prior_lds(long long NAP, long long NAQ) {
  if (NAP + NAQ > (64 * 1024) / 8) return 0;
  return (size_t)(NAP + NAQ) * 8;
}

// The distinct sub-multisets a of TP alleles of the ascending multiset gc [KC], in VCF order of a: f(ra, rb, x, cn, m) with the
// ranks of a and of gc - a, and -- over the m distinct alleles of gc, ascending -- a's copies x[i] out of gc's cn[i].
template <int KM, class Fn>
__device__ __forceinline__ void for_each_submultiset(const int (&gc)[KM], int KC, int TP, Fn f) {
  // the distinct alleles of gc, ascending, and their dosages
  int al[KM], cn[KM], x[KM];
  int m = 0;
  for (int k = 0; k < KC; k++) {
    if (k == 0 || gc[k] != gc[k - 1]) {
      al[m] = gc[k];
      cn[m] = 1;
      m++;
    } else {
      cn[m - 1]++;
    }
  }
  // the first sub-multiset in VCF order: as few of the high alleles as can be
  int rem = TP;
  for (int i = 0; i < m; i++) {
    x[i] = cn[i] < rem ? cn[i] : rem;
    rem -= x[i];
  }
  for (;;) {
    long long ra = 0, rb = 0;
    int pa = 0, pb = 0;
    for (int i = 0; i < m; i++) {
      for (int d = 0; d < x[i]; d++) ra += cwr(al[i], ++pa);
      for (int d = x[i]; d < cn[i]; d++) rb += cwr(al[i], ++pb);
    }
    f(ra, rb, x, cn, m);
    // the successor: the lowest allele that can take one more copy from the alleles below it; those then as low as can be
    int s = x[0], i = 1;
    while (i < m && !(x[i] < cn[i] && s >= 1)) {
      s += x[i];
      i++;
    }
    if (i >= m) break;
    x[i]++;
    rem = s - 1;
    for (int q = 0; q < i; q++) {
      x[q] = cn[q] < rem ? cn[q] : rem;
      rem -= x[q];
    }
  }
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_cross_prior_kernel(const ExactCrossPriorParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int row = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int TP = P.TP, KC = P.TP + P.TQ;
  const double *gp = P.gam_p + (size_t)row * P.NAP, *gq = P.gam_q + (size_t)row * P.NAQ;
  if (P.staged) {
    double *tp = reinterpret_cast<double *>(smem), *tq = tp + P.NAP;
    for (int i = threadIdx.x; i < P.NAP; i += EXACT_THREADS) tp[i] = gp[i];
    for (int i = threadIdx.x; i < P.NAQ; i += EXACT_THREADS) tq[i] = gq[i];
    __syncthreads();
    gp = tp;
    gq = tq;
  }
  const long long j = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (j >= P.GC) return;
  int gc[KM];
  unrank_genotype(j, KC, gc);
  double sum = 0.0;
  for_each_submultiset<KM>(gc, KC, TP, [&](long long ra, long long rb, const int *, const int *, int) { sum += gp[ra] * gq[rb]; });
  P.log_x[(size_t)row * P.GC + j] = log(sum);  // (exactly -inf where every product is 0)
}

struct ExactCrossPostParams {
  const double *llk64;      // [U][G] the progeny units' stored log likelihoods
  const double *log_x;      // [rows][G]
  const int32_t *unit_row;  // [U] the unit's row of log_x
  int nblk;
  long long G;
  double *part;             // [U][nblk][2]: the tile's maximum of llk + log X, and sum exp(. - maximum)
  long long *part_i;        // [U][nblk]: the first genotype of the tile at that maximum
  double *log_z;            // [U]
  long long *mode;          // [U] (-1 where log Z is not finite)
  double *mode_prob;        // [U]
  double *post;             // [U][G] or null
};

static __global__ __launch_bounds__(EXACT_THREADS) void exact_cross_post_kernel(const ExactCrossPostParams P) {
  constexpr int NW = EXACT_THREADS / 64;
  constexpr int RUN = EXACT_GENOS_PER_BLOCK / EXACT_THREADS;
  __shared__ double redm[NW], reds[NW];
  __shared__ long long redi[NW];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long G = P.G;
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK;
  long long hi = lo + EXACT_GENOS_PER_BLOCK;
  if (hi > G) hi = G;
  const double *llk = P.llk64 + (size_t)unit * G;
  const double *lx = P.log_x + (size_t)P.unit_row[unit] * G;
  double lj[RUN];
  double m = -INFINITY;
  long long mi = LLONG_MAX;
#pragma unroll
  for (int t = 0; t < RUN; t++) {
    const long long gi = lo + threadIdx.x + (long long)t * EXACT_THREADS;  // consecutive lanes, consecutive genotypes
    lj[t] = -INFINITY;
    if (gi < hi) {
      lj[t] = llk[gi] + lx[gi];
      if (lj[t] > m) {  // (ascending within the thread: the first maximum stays)
        m = lj[t];
        mi = gi;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double om = __shfl_xor(m, o, WAVE);
    const long long oi = __shfl_xor(mi, o, WAVE);
    if (om > m || (om == m && oi < mi)) {
      m = om;
      mi = oi;
    }
  }
  if (lane == 0) {
    redm[wave] = m;
    redi[wave] = mi;
  }
  __syncthreads();
  m = redm[0];
  mi = redi[0];
#pragma unroll
  for (int w = 1; w < NW; w++)
    if (redm[w] > m || (redm[w] == m && redi[w] < mi)) {
      m = redm[w];
      mi = redi[w];
    }
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < RUN; t++) s += wave_sum(lj[t] == -INFINITY ? 0.0 : exp(lj[t] - m));  // (NaN stays NaN)
  if (lane == 0) reds[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int w = 0; w < NW; w++) sum += reds[w];
    P.part[((size_t)unit * P.nblk + blk) * 2] = m;
    P.part[((size_t)unit * P.nblk + blk) * 2 + 1] = sum;
    P.part_i[(size_t)unit * P.nblk + blk] = mi;
  }
}

// The tiles of a unit in tile order (every thread forms the same sums): log Z = maximum + log(total relative to it), the first
// genotype at the maximum and its probability; then, where asked for, the whole posterior.  A NaN term (a parent without a finite
// genotype) makes log Z NaN; no finite term: -inf.  Either way there is no mode (-1, NaN) and the posterior is NaN.
static __global__ __launch_bounds__(EXACT_THREADS) void exact_cross_post_combine_kernel(const ExactCrossPostParams P) {
  const int unit = blockIdx.x;
  const double *part = P.part + (size_t)unit * P.nblk * 2;
  const long long *part_i = P.part_i + (size_t)unit * P.nblk;
  double m = -INFINITY;
  long long mi = -1;
  for (int q = 0; q < P.nblk; q++)
    if (part[(size_t)q * 2] > m) {
      m = part[(size_t)q * 2];
      mi = part_i[q];
    }
  double total = 0.0;
  for (int q = 0; q < P.nblk; q++) {
    const double mq = part[(size_t)q * 2], sq = part[(size_t)q * 2 + 1];
    total += mq > -INFINITY ? sq * exp(mq - m) : sq;  // (a tile without a finite entry: 0, or NaN)
  }
  double lz = m > -INFINITY ? m + log(total) : -INFINITY;
  if (total != total) lz = NAN;
  const bool ok = lz > -INFINITY && lz < INFINITY;
  if (threadIdx.x == 0) {
    P.log_z[unit] = lz;
    P.mode[unit] = ok ? mi : -1;
    P.mode_prob[unit] = ok ? exp(m - lz) : NAN;
  }
  if (P.post) {
    const double *llk = P.llk64 + (size_t)unit * P.G;
    const double *lx = P.log_x + (size_t)P.unit_row[unit] * P.G;
    double *out = P.post + (size_t)unit * P.G;
    for (long long g = threadIdx.x; g < P.G; g += EXACT_THREADS) {
      const double lj = llk[g] + lx[g];
      out[g] = ok ? (lj == -INFINITY ? 0.0 : exp(lj - lz)) : NAN;
    }
  }
}

}  // namespace mchap
