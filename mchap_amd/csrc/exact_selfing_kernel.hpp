// Selfed parents ranked per progeny (call-exact --parentage-selfings, application.Parentage) for MI355X (gfx950): the genotype prior
// of a progeny whose two gametes come from ONE parental genotype, and the evidence of every progeny under every candidate's such
// prior, over the likelihoods the exact caller left in llk64.  Per record with H haplotypes, a candidate of even ploidy K, gametes
// of t = K / 2 haplotypes, its posterior p[g] under its calling prior (exact_gamete_kernel's), gamete error e, frequencies f:
//   hyp(a | g) = prod_h C(c_h(g), a_h) / C(K, t)
//   J[a][b]    = sum_{g = (a u b) + r} p[g] prod_h C(c_h(g), a_h) C(c_h(g), b_h)   over the complements r of the multiset union a u b
//                                                                               (dosage max(a_h, b_h)), in VCF order of r; none
//                                                                               where the union has more than K haplotypes
//   D[gc]      = sum_{a in gc, rank a <= rank (gc - a)} w J[a][gc - a]             in VCF order of a; w = 2 off the diagonal, else 1
//   E[gc]      = sum_{the same a} w (gam[a] m[gc - a] + m[a] gam[gc - a])          gam the error-free gamete table, m = Mult(.; t, f)
//   S[gc]      = ((1 - e)(1 - e)) (D[gc] / C(K, t)^2) + (e (1 - e)) E[gc] + (e e) Mult(gc; K, f)
// -- sum_g p[g] sum_a gamma(a | g) gamma(gc - a | g) with gamma = (1 - e) hyp + e m, expanded so that no term is formed for a
// genotype that cannot give the pair, and never as "the product of the gamete table with itself plus a correction".
//
// Gather form throughout: one owning lane per output cell, a fixed summation order, no atomics; nothing depends on a unit's place
// in the batch, so equal inputs give equal bits.
//   exact_selfing_post_kernel     one lane per parental genotype: p[g], NaN throughout without a finite genotype.  Materialised
//                                 once, because the prior kernel reads each p[g] many times and the prior costs an lgamma walk.
//   exact_selfing_prior_kernel    one lane per progeny genotype gc, workgroups over (unit, 256 genotypes).  The lane walks the
//                                 sub-multisets a of gc (for_each_submultiset), skips rank a > rank b, and for each pair walks the
//                                 C(H + K - |a u b| - 1, K - |a u b|) complements with next_genotype, ranking the completed genotype
//                                 from the table cw[pos][allele] in LDS without merging.  The trip counts differ between lanes (a
//                                 heterozygous gc has more pairs and wider unions): the launch is bound by its slowest lanes.
//   selfing_max_kernel            m_c per (record, progeny): NaN where a likelihood is NaN.
//   selfing_evidence_kernel       one workgroup per (record, progeny, tile of EXACT_GENOS_PER_BLOCK genotypes): exp(llk_c - m_c) once
//                                 per genotype in registers, then the candidates one after the other -- the lane's 16 terms in
//                                 order, the wave_sum tree, the four wavefronts in order.
//   selfing_combine_kernel        one lane per (record, progeny, candidate): the tiles in tile order, log_z = m_c + log(total).
#pragma once
#include "exact_cross_kernel.hpp"
#include "exact_family_kernel.hpp"

namespace mchap {

struct ExactSelfingParams {
  const double *llk64;       // [U][G] stored log likelihoods
  const double *inbreeding;  // [U], or null: the flat genotype prior -log(G)
  const int32_t *unit_row;   // [U] the unit's row of freqs
  const double *freqs;       // [rows][stride]
  const double *error;       // [U] gamete error e
  int stride;
  int H, K, T, nblk;         // T = K / 2; nblk tiles of EXACT_THREADS genotypes
  long long G, NA;           // genotypes (the parent's and the progeny's: one ploidy), gametes
  const double *log_norm;    // [U] the gamete launch's normaliser
  const double *gam;         // [U][NA] the error-free gamete table
  double *post;              // [U][G] p
  double *log_self;          // [U][G] log S
  double *self;              // [U][G] S, or null
};

// LDS of exact_selfing_prior_kernel in doubles: cw [K][H], the complements' counts nr [K + 1], factorials [K + 1], the frequencies
// [H], the binomials (ints, two to a double)
inline size_t exact_selfing_lds(int H, int K) {
  return ((size_t)H * K + 2 * (size_t)(K + 1) + (size_t)H + (CROSS_BIN * CROSS_BIN + 1) / 2) * 8;
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_selfing_post_kernel(const ExactSelfingParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K;
  const bool has_prior = P.inbreeding != nullptr;
  const double *fr = P.freqs + (size_t)P.unit_row[unit] * P.stride;
  const double F = has_prior ? P.inbreeding[unit] : 0.0;
  PriorTab pt;
  int *bin;
  cross_setup(smem, H, K, has_prior, F, fr, pt, bin);
  const double norm = P.log_norm[unit];
  const bool finite_norm = norm > -INFINITY && norm < INFINITY;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.G) return;
  int g[KM];
  unrank_genotype(idx, K, g);
  const double lj = P.llk64[(size_t)unit * P.G + idx] + (has_prior ? calling_log_prior(pt, g, K) : -log((double)P.G));
  const double p = exp(lj - norm);
  P.post[(size_t)unit * P.G + idx] = finite_norm ? (p > 0.0 ? p : 0.0) : NAN;  // (NaN likelihood: 0, as exact_gamete_kernel)
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void exact_selfing_prior_kernel(const ExactSelfingParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int unit = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K, T = P.T;
  long long *cw = reinterpret_cast<long long *>(smem);  // [K][H]: cw[pos * H + v] = C(v + pos, pos + 1), rank_genotype's term
  long long *nr = cw + (size_t)K * H;                   // [K + 1]: complements of k haplotypes
  double *fact = reinterpret_cast<double *>(nr + K + 1);  // [K + 1]
  double *f = fact + K + 1;                             // [H]
  int *bin = reinterpret_cast<int *>(f + H);            // [CROSS_BIN][CROSS_BIN]
  const double *fr = P.freqs + (size_t)P.unit_row[unit] * P.stride;
  for (int q = threadIdx.x; q < K * H; q += EXACT_THREADS) cw[q] = cwr(q % H, q / H + 1);
  for (int k = threadIdx.x; k <= K; k += EXACT_THREADS) {
    nr[k] = cwr(H, k);
    double v = 1.0;
    for (int i = 2; i <= k; i++) v *= (double)i;  // (exact: 16! < 2^53)
    fact[k] = v;
  }
  for (int h = threadIdx.x; h < H; h += EXACT_THREADS) f[h] = fr[h];
  for (int q = threadIdx.x; q < CROSS_BIN * CROSS_BIN; q += EXACT_THREADS) {
    const int n = q / CROSS_BIN, k = q % CROSS_BIN;
    int b = k <= n ? 1 : 0;
    for (int i = 1; i <= k && k <= n; i++) b = b * (n - k + i) / i;
    bin[q] = b;
  }
  __syncthreads();
  const long long j = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (j >= P.G) return;
  double *out = P.log_self + (size_t)unit * P.G + j;
  double *lin = P.self ? P.self + (size_t)unit * P.G + j : nullptr;
  const double norm = P.log_norm[unit];
  if (!(norm > -INFINITY && norm < INFINITY)) {  // a parent without a finite genotype
    *out = NAN;
    if (lin) *lin = NAN;
    return;
  }
  int gc[KM];
  unrank_genotype(j, K, gc);
  // the distinct alleles of gc, ascending, and their dosages (for_each_submultiset's own, kept here for the union)
  int al[KM], cn[KM];
#pragma unroll
  for (int i = 0; i < KM; i++) al[i] = cn[i] = 0;
  int m = 0;
#pragma unroll
  for (int k = 0; k < KM; k++) {
    if (k >= K) continue;
    const bool fresh = k == 0 || gc[k] != gc[k - 1];
    m += fresh ? 1 : 0;
#pragma unroll
    for (int i = 0; i < KM; i++)
      if (i == m - 1) {
        al[i] = gc[k];
        cn[i] = fresh ? 1 : cn[i] + 1;
      }
  }
  const double *p = P.post + (size_t)unit * P.G;
  const double *gam = P.gam + (size_t)unit * P.NA;
  double accD = 0.0, accE = 0.0;
  for_each_submultiset<KM>(gc, K, T, [&](long long ra, long long rb, const int *x, const int *, int) {
    if (ra > rb) return;  // (the pair (b, a) gives the same term)
    const double wt = ra == rb ? 1.0 : 2.0;
    // Mult(a; t, f) and Mult(b; t, f): the coefficient by exact divisions, the frequencies multiplied in the order of the gamete
    double ca = fact[T], cb = fact[T], pa = 1.0, pb = 1.0;
    int un[KM], xs[KM];
    int usum = 0;
#pragma unroll
    for (int i = 0; i < KM; i++) {
      un[i] = xs[i] = 0;
      if (i >= m) continue;
      const int xa = x[i], xb = cn[i] - xa;
      xs[i] = xa;
      ca /= fact[xa];
      cb /= fact[xb];
      for (int d = 0; d < xa; d++) pa *= f[al[i]];
      for (int d = 0; d < xb; d++) pb *= f[al[i]];
      un[i] = xa > xb ? xa : xb;
      usum += un[i];
    }
    accE += wt * (gam[ra] * (cb * pb) + (ca * pa) * gam[rb]);
    if (usum > K) return;  // no genotype holds both gametes
    const int KR = K - usum;
    int r[KM];
#pragma unroll
    for (int k = 0; k < KM; k++) r[k] = 0;
    double s = 0.0;
    const long long n_r = nr[KR];
    for (long long c = 0; c < n_r; c++) {
      // the genotype (a u b) + r ranked without merging: a copy of the union stands behind the union's copies before it and the
      // entries of r below it, an entry of r behind the entries of r before it and the union's copies up to it
      long long rank = 0, w = 1;
      int before = 0;
#pragma unroll
      for (int i = 0; i < KM; i++) {
        if (i >= m) continue;
        int lt = 0, eq = 0;
#pragma unroll
        for (int q = 0; q < KM; q++) {
          lt += (q < KR && r[q] < al[i]) ? 1 : 0;
          eq += (q < KR && r[q] == al[i]) ? 1 : 0;
        }
        for (int d = 0; d < un[i]; d++) rank += cw[(size_t)(before + d + lt) * H + al[i]];
        before += un[i];
        const int copies = un[i] + eq;
        w *= (long long)bin[copies * CROSS_BIN + xs[i]] * bin[copies * CROSS_BIN + cn[i] - xs[i]];
      }
#pragma unroll
      for (int q = 0; q < KM; q++) {
        if (q >= KR) continue;
        int le = 0;
#pragma unroll
        for (int i = 0; i < KM; i++) le += (i < m && al[i] <= r[q]) ? un[i] : 0;
        rank += cw[(size_t)(q + le) * H + r[q]];
      }
      s += p[rank] * (double)w;
      next_genotype(r, KR);
    }
    accD += wt * s;
  });
  // Mult(gc; K, f)
  double cg = fact[K], pg = 1.0;
#pragma unroll
  for (int i = 0; i < KM; i++)
    if (i < m) cg /= fact[cn[i]];
#pragma unroll
  for (int k = 0; k < KM; k++)
    if (k < K) pg *= f[gc[k]];
  const double e = P.error[unit];
  const double pairs = (double)bin[K * CROSS_BIN + T];
  const double S = ((1.0 - e) * (1.0 - e)) * (accD / (pairs * pairs)) + (e * (1.0 - e)) * accE + (e * e) * (cg * pg);
  *out = log(S);  // (exactly -inf where every product is 0)
  if (lin) *lin = S;
}

struct SelfingEvidenceParams {
  const double *self;    // [R][n][G] S of every candidate
  const double *llk;     // [R][C][G]
  const int32_t *reads;  // [R][C], or null: every progeny has reads
  int C, n, ntile;       // progeny, candidates, tiles of EXACT_GENOS_PER_BLOCK genotypes
  long long G, cells;    // cells = R * C * n
  double *lmax;          // [R][C]
  double *part;          // [R][C][n][ntile]
  double *log_z;         // [R][C][n]
};

__device__ __forceinline__ bool selfing_has_reads(const SelfingEvidenceParams &P, size_t rc) {
  return P.reads == nullptr || P.reads[rc] != 0;
}

static __global__ __launch_bounds__(EXACT_THREADS) void selfing_max_kernel(const SelfingEvidenceParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW];
  const size_t rc = blockIdx.x;
  if (!selfing_has_reads(P, rc)) return;
  const double *llk = P.llk + rc * P.G;
  double m = -INFINITY;
  bool bad = false;
  for (long long g = threadIdx.x; g < P.G; g += EXACT_THREADS) {
    const double v = llk[g];
    bad = bad || v != v;
    m = v > m ? v : m;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double om = __shfl_xor(m, o, WAVE);
    m = om > m ? om : m;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = m;
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) m = red[w] > m ? red[w] : m;
    P.lmax[rc] = any_bad ? NAN : m;
  }
}

static __global__ __launch_bounds__(EXACT_THREADS) void selfing_evidence_kernel(const SelfingEvidenceParams P) {
  constexpr int RUN = EXACT_GENOS_PER_BLOCK / EXACT_THREADS;
  __shared__ double red[EXACT_THREADS / WAVE];
  const int tile = blockIdx.x % P.ntile;
  const size_t rc = blockIdx.x / P.ntile;
  if (!selfing_has_reads(P, rc)) return;  // (the whole workgroup: its likelihoods are not read)
  const size_t rec = rc / P.C;
  const double m = P.lmax[rc];
  const long long lo = (long long)tile * EXACT_GENOS_PER_BLOCK + threadIdx.x;
  const double *llk = P.llk + rc * P.G;
  double t[RUN];
#pragma unroll
  for (int k = 0; k < RUN; k++) {
    const long long g = lo + (long long)k * EXACT_THREADS;  // consecutive lanes, consecutive genotypes
    t[k] = g < P.G ? exp(llk[g] - m) : 0.0;                 // (m_c NaN or -inf: NaN)
  }
  for (int i = 0; i < P.n; i++) {
    const double *s = P.self + (rec * P.n + i) * P.G;
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < RUN; k++) {
      const long long g = lo + (long long)k * EXACT_THREADS;
      if (g < P.G) part += s[g] * t[k];
    }
    const double z = family_block_sum(part, red);
    if (threadIdx.x == 0) P.part[(rc * P.n + i) * P.ntile + tile] = z;
  }
}

static __global__ __launch_bounds__(EXACT_THREADS) void selfing_combine_kernel(const SelfingEvidenceParams P) {
  const long long q = (long long)blockIdx.x * EXACT_THREADS + threadIdx.x;
  if (q >= P.cells) return;
  const size_t rc = (size_t)q / P.n;
  if (!selfing_has_reads(P, rc)) {
    P.log_z[q] = 0.0;
    return;
  }
  const double *part = P.part + (size_t)q * P.ntile;
  double total = 0.0;
  for (int k = 0; k < P.ntile; k++) total += part[k];
  P.log_z[q] = P.lmax[rc] + log(total);  // (exactly -inf where every product is 0)
}

}  // namespace mchap
