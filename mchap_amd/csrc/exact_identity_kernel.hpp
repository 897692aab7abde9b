// Sample pairs ranked by shared-genotype evidence (call-exact --identity, application.Identity) for MI355X (gfx950): for every record
// and every pair (i, j) of n samples of one ploidy K under one calling prior pi (one F, the record's frequencies), over the
// likelihoods the exact caller left in llk64 [R][n][G]:
//   hp[g]     = log pi(g) / 2                                      once per record (identity_prior_kernel; the flat prior: a constant)
//   m_s       = max_g (llk_s[g] + hp[g])
//   a_s[g]    = exp(llk_s[g] + hp[g] - m_s)                        once per (record, sample) (identity_a_kernel), in [0, 1]
//   S_ij      = sum_g a_i[g] a_j[g]                                 g ascending; a sum below IDENTITY_TINY counts as 0
//   lr_ij     = log S_ij + ((m_i - log_norm_i) + (m_j - log_norm_j))      log r, r = sum_g post_i post_j / pi
//   lbf_ij    = log((1 - e) exp(lr_ij) + e)                         (identity_term: e = 0 is lr itself, e = 1 is 0)
// log_norm is the model evidence of the sample at the launch's F (exact_evidence_kernel, one grid point).
//
// Gather form throughout: one owning lane per output cell, a fixed summation order, no atomics.
//   identity_prior_kernel    one workgroup per (record, tile of 4096 genotypes): the prior tables of exact_evidence_kernel in LDS,
//                            each thread unranks the first genotype of its run of 16 and walks it with next_genotype.
//   identity_a_kernel        one workgroup per (record, sample): the maximum (NaN where a term is NaN), then the row of a.  A
//                            sample without a finite term has a NaN row; a sample flagged without reads is not read, its row is 0.
//   identity_product_kernel  the register-tiled product A A^T in float64.  A workgroup of 256 threads owns a tile of 64 x 64
//                            sample pairs of one record over one chunk of the genotype axis; only tiles with ti <= tj exist.  The
//                            rows of a are staged through LDS 16 genotypes at a time, transposed ([g][sample]); a thread keeps
//                            4 x 4 accumulators, so each value it reads from LDS serves a row or a column of four of them; one
//                            v_fma_f64 per term.  It writes its chunk's partial sums to part[R][chunk][n][n] (the tile's cells).
//   identity_combine_kernel  one thread per cell (record, i, j): the chunks in chunk order, the clause, the term; the cell below
//                            the diagonal tiles reads the partial sums of its mirror image, the diagonal is NaN.
// The chunk boundaries depend on G alone (identity_nchunk, identity_chunk_len), and an accumulator takes the genotypes of its chunk
// in ascending order: equal inputs give equal bits whatever the place of a record in the launch, the number and order of the
// samples, and the tile a pair falls into; a product is commutative, so lbf[i][j] and lbf[j][i] have the same bits.
#pragma once
#include "exact_kernel.hpp"

namespace mchap {

constexpr int IDENTITY_TILE = 64;        // samples a side of a workgroup's tile
constexpr int IDENTITY_BK = 16;          // genotypes staged in LDS at a time
constexpr int IDENTITY_CHUNK = 2048;     // genotypes of a chunk, at least (the last chunks of a long axis are longer)
constexpr int IDENTITY_MAXCHUNK = 16;    // chunks of the genotype axis, at most
constexpr double IDENTITY_TINY = 1e-290; // a scaled sum below this counts as 0

inline int identity_nchunk(long long G) {
  const long long c = (G + IDENTITY_CHUNK - 1) / IDENTITY_CHUNK;
  return c > IDENTITY_MAXCHUNK ? IDENTITY_MAXCHUNK : (c < 1 ? 1 : (int)c);
}
// genotypes per chunk: a multiple of IDENTITY_BK
inline long long identity_chunk_len(long long G) {
  const long long nc = identity_nchunk(G);
  const long long len = (G + nc - 1) / nc;
  return (len + IDENTITY_BK - 1) / IDENTITY_BK * IDENTITY_BK;
}

struct IdentityParams {
  const double *llk;       // [R][n][G]
  const double *freqs;     // [R][stride], or null: the flat prior
  const double *log_norm;  // [R][n]
  const int32_t *reads;    // [R][n], or null: every sample has reads
  int stride, H, K, n;
  int has_prior;           // 0: the flat prior, hp = -log(G) / 2
  int nblk;                // tiles of EXACT_GENOS_PER_BLOCK genotypes (identity_prior_kernel)
  int nt, ntri, nchunk;    // tiles a side, tiles with ti <= tj, chunks
  int ncb;                 // workgroups of identity_combine_kernel per record
  long long G, chunk_len;
  double F, error;
  double *hp;              // [R][G]
  double *m;               // [R][n]
  double *a;               // [R][n][G]
  double *part;            // [R][nchunk][n][n]
  double *lbf;             // [R][n][n]
};

// LDS of identity_prior_kernel: lgf [K + 1], lfreq [H], lgd [H][K + 1]
inline size_t identity_prior_lds(int H, int K) { return ((size_t)H * (K + 1) + (K + 1) + H) * 8; }

__device__ __forceinline__ bool identity_has_reads(const IdentityParams &P, int rec, int s) {
  return P.reads == nullptr || P.reads[(size_t)rec * P.n + s] != 0;
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void identity_prior_kernel(const IdentityParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int H = P.H, K = P.K;
  double *lgf = reinterpret_cast<double *>(smem);  // [K + 1]
  double *lfreq = lgf + (K + 1);                   // [H]
  double *lgd = lfreq + H;                         // [H][K + 1]
  const double *fr = P.freqs + (size_t)rec * P.stride;
  const double F = P.F;
  for (int d = threadIdx.x; d <= K; d += EXACT_THREADS) lgf[d] = lgamma((double)d + 1.0);
  for (int h = threadIdx.x; h < H; h += EXACT_THREADS) lfreq[h] = fr[h];
  // the prior tables of exact_evidence_kernel
  for (int q = threadIdx.x; q < H * (K + 1); q += EXACT_THREADS) {
    const int h = q / (K + 1), d = q % (K + 1);
    const double alpha = fr[h] * ((1.0 - F) / F);
    lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
  }
  PriorTab pt;
  pt.lgd = lgd;
  pt.lgf = lgf;
  pt.lfreq = lfreq;
  pt.left = 0.0;
  if (F != 0.0) {
    const double scale = (1.0 - F) / F;
    double sum_alpha = 0.0;
    for (int h = 0; h < H; h++) sum_alpha += fr[h] * scale;
    pt.left = (lgamma((double)K + 1.0) + lgamma(sum_alpha)) - lgamma((double)K + sum_alpha);
  }
  pt.lnH = 0.0;
  pt.F = F;
  pt.has_freqs = 1;
  __syncthreads();
  const long long lo = (long long)blk * EXACT_GENOS_PER_BLOCK + (long long)threadIdx.x * EXACT_EM_RUN;
  if (lo >= P.G) return;
  int g[KM];
  unrank_genotype(lo, K, g);
  double *hp = P.hp + (size_t)rec * P.G;
#pragma unroll 1
  for (int t = 0; t < EXACT_EM_RUN; t++) {
    if (lo + t >= P.G) break;
    hp[lo + t] = 0.5 * calling_log_prior(pt, g, K);  // (-inf where a haplotype of g has frequency 0)
    next_genotype(g, K);
  }
}

static __global__ __launch_bounds__(EXACT_THREADS) void identity_a_kernel(const IdentityParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW];
  const int rec = blockIdx.x / P.n, s = blockIdx.x % P.n;
  const long long G = P.G;
  double *a = P.a + ((size_t)rec * P.n + s) * G;
  if (!identity_has_reads(P, rec, s)) {
    for (long long g = threadIdx.x; g < G; g += EXACT_THREADS) a[g] = 0.0;
    return;
  }
  const double *llk = P.llk + ((size_t)rec * P.n + s) * G;
  const double *hp = P.hp + (size_t)rec * G;
  const double flat = -0.5 * log((double)G);
  double m = -INFINITY;
  bool bad = false;
  for (long long g = threadIdx.x; g < G; g += EXACT_THREADS) {
    const double v = llk[g] + (P.has_prior ? hp[g] : flat);
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
  m = red[0];
#pragma unroll
  for (int w = 1; w < NW; w++) m = red[w] > m ? red[w] : m;
  if (any_bad) m = NAN;
  if (threadIdx.x == 0) P.m[(size_t)rec * P.n + s] = m;
  // (m NaN or -inf: a NaN row)
  for (long long g = threadIdx.x; g < G; g += EXACT_THREADS) a[g] = exp((llk[g] + (P.has_prior ? hp[g] : flat)) - m);
}

static __global__ __launch_bounds__(EXACT_THREADS) void identity_product_kernel(const IdentityParams P) {
  constexpr int T = IDENTITY_TILE, BK = IDENTITY_BK;
  __shared__ __align__(16) double As[BK * T];
  __shared__ __align__(16) double Bs[BK * T];
  int q = blockIdx.x;
  int t = q % P.ntri;
  q /= P.ntri;
  const int chunk = q % P.nchunk, rec = q / P.nchunk;
  int ti = 0;
  while (t >= P.nt - ti) {
    t -= P.nt - ti;
    ti++;
  }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const int n = P.n;
  const long long G = P.G;
  const long long g0 = (long long)chunk * P.chunk_len;
  long long g1 = g0 + P.chunk_len;
  if (g1 > G) g1 = G;
  const double *arec = P.a + (size_t)rec * n * G;
  // staging: the thread's sample of the tile and its four consecutive genotypes of the step
  const int srow = threadIdx.x & (T - 1), sk = (threadIdx.x >> 6) * 4;
  const int ia = ti * T + srow, ib = tj * T + srow;
  const double *pa = arec + (size_t)(ia < n ? ia : 0) * G;
  const double *pb = arec + (size_t)(ib < n ? ib : 0) * G;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const double *bsrc = diag ? As : Bs;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) acc[u][v] = 0.0;
  for (long long k0 = g0; k0 < g1; k0 += BK) {
    __syncthreads();  // (the step before is read to its end)
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const long long g = k0 + sk + e;
      As[(sk + e) * T + srow] = (ia < n && g < g1) ? pa[g] : 0.0;
      if (!diag) Bs[(sk + e) * T + srow] = (ib < n && g < g1) ? pb[g] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; kk++) {
      double ra[4], rb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) ra[u] = As[kk * T + ty * 4 + u];
#pragma unroll
      for (int v = 0; v < 4; v++) rb[v] = bsrc[kk * T + tx * 4 + v];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) acc[u][v] = fma(ra[u], rb[v], acc[u][v]);
    }
  }
  double *part = P.part + ((size_t)rec * P.nchunk + chunk) * n * n;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = ti * T + ty * 4 + u;
    if (i >= n) continue;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int j = tj * T + tx * 4 + v;
      if (j < n) part[(size_t)i * n + j] = acc[u][v];
    }
  }
}

// The term of a pair from its scaled sum S and c = (m_i - log_norm_i) + (m_j - log_norm_j) (application.identity_term)
__device__ __forceinline__ double identity_term(double S, double c, double e) {
  if (S < IDENTITY_TINY) S = 0.0;
  const double lr = log(S) + c;  // (-inf at S = 0)
  if (e == 0.0) return lr;
  if (e == 1.0) return 0.0;
  if (lr > 700.0) return lr + log1p(-e);
  return log((1.0 - e) * exp(lr) + e);
}

static __global__ __launch_bounds__(EXACT_THREADS) void identity_combine_kernel(const IdentityParams P) {
  const int n = P.n;
  const long long cells = (long long)n * n;
  const int rec = blockIdx.x / P.ncb;
  const long long q = (long long)(blockIdx.x % P.ncb) * EXACT_THREADS + threadIdx.x;
  if (q >= cells) return;
  const int i = (int)(q / n), j = (int)(q % n);
  double *out = P.lbf + (size_t)rec * cells + q;
  if (i == j) {
    *out = NAN;
    return;
  }
  const bool ri = identity_has_reads(P, rec, i), rj = identity_has_reads(P, rec, j);
  double ci = 0.0, cj = 0.0;
  bool bad = false;
  if (ri) {
    const double m = P.m[(size_t)rec * n + i], ln = P.log_norm[(size_t)rec * n + i];
    ci = m - ln;
    bad = bad || !(fabs(m) < INFINITY) || !(fabs(ln) < INFINITY);
  }
  if (rj) {
    const double m = P.m[(size_t)rec * n + j], ln = P.log_norm[(size_t)rec * n + j];
    cj = m - ln;
    bad = bad || !(fabs(m) < INFINITY) || !(fabs(ln) < INFINITY);
  }
  if (bad) {  // a sample without a finite genotype: the pair is not formed
    *out = NAN;
    return;
  }
  if (!ri || !rj) {  // a sample without reads: r = 1 by definition
    *out = 0.0;
    return;
  }
  // the cell of a tile with ti <= tj holds the partial sums; one below reads its mirror image's
  const bool own = i / IDENTITY_TILE <= j / IDENTITY_TILE;
  const size_t at = own ? (size_t)i * n + j : (size_t)j * n + i;
  const double *part = P.part + (size_t)rec * P.nchunk * cells + at;
  double S = 0.0;
  for (int c = 0; c < P.nchunk; c++) S += part[(size_t)c * cells];
  *out = identity_term(S, ci + cj, P.error);
}

}  // namespace mchap
