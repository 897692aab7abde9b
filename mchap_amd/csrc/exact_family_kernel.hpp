// The parents and the progeny of one cross called jointly (call-exact --family-calls, application.FamilyCalls) for MI355X (gfx950):
// the exact joint posterior of one nuclear family per record, over the likelihoods the exact caller left in llk64.  Per record with
// H haplotypes, parents P and Q of even ploidies K_P and K_Q, gametes of t = K / 2 haplotypes (NA = C(H + t - 1, t) of them), n
// progeny of ploidy K_c = t_P + t_Q; every multiset in VCF order:
//   gamma_u(a | g) = (1 - e_u) prod_h C(c_h(g), a_h) / C(K_u, t_u) + e_u Mult(a; t_u, f)      a sparse row plus a rank-one row
//   T_c[a][b]      = exp(llk_c[rank(a + b)] - m_c),  m_c = max llk_c
//   V_c[gP][b]     = sum_a gamma_P(a | gP) T_c[a][b]
//   M_c[gP][gQ]    = sum_b gamma_Q(b | gQ) V_c[gP][b]
//   S[gP][gQ]      = sum_c (log M_c + m_c)                                                 over the progeny with reads, in their order
//   w              = exp(S + lp_P + llk_P + lp_Q + llk_Q - log Z_fam),  post_P = sum_gQ w,  post_Q = sum_gP w
//   Y_c[gP][b]     = sum_gQ (w / M_c)[gP][gQ] gamma_Q(b | gQ),   R_c[a][b] = sum_gP gamma_P(a | gP) Y_c[gP][b]
//   q_c[gc]        = exp(llk_c[gc] - m_c) sum_{a in gc} R_c[a][gc - a],   pred_c = m_c - log sum (w / M_c)
// A progeny without reads adds nothing to S and takes w itself for w / M_c (pred_c = 0).  w / M_c is 0 where w is 0.  A record
// whose log Z_fam is not finite -- a parent or a progeny without a finite genotype, Z_fam = 0 -- has w = NaN, and with it every
// output (modes -1).
//
// The sparse rows do not depend on the record: family_rows_kernel lists, once per launch and parent shape, the distinct
// sub-multisets of every genotype (for_each_submultiset: at most C(K, t) of them) with their weights, and family_cols_kernel, for
// the transposed products of the back projection, the NA complements of every gamete (the merge and rank of exact_gamete_kernel).
// After that no stage ranks anything but T_c and q_c, once per cell.  Every stage is gather-form: one owning lane per output cell,
// a fixed summation order (sub-multisets in VCF order of a, complements in VCF order of r; strided partial sums, then the
// wave_sum tree, then the four wavefronts in order; row chunks in order), no atomics -- equal inputs give equal bits whatever the
// place of a record in the launch.  S, then w in its place, is the one [G_P][G_Q] array per record; M_c is formed again for the back
// projection, a row at a time: family_row_kernel owns one gP, keeps V_c[gP][.] and the row of w / M_c in LDS where they fit 64 KB
// and in global memory otherwise (`staged`; the C entry's force_fallback takes the second path at any size).
#pragma once
#include "exact_cross_kernel.hpp"

namespace mchap {

constexpr int FAMILY_LDS_BUDGET = 64 * 1024;

__device__ __forceinline__ int small_binom(int n, int k) {
  if (k < 0 || k > n) return 0;
  int b = 1;
  for (int i = 1; i <= k; i++) b = b * (n - k + i) / i;  // (exact at every step, as cross_setup's table)
  return b;
}

// a[i] for a run-time i without indexing the array by it, so that it stays in registers
template <int KM>
__device__ __forceinline__ int pick(const int (&a)[KM], int i) {
  int v = a[0];
#pragma unroll
  for (int k = 1; k < KM; k++) v = k == i ? a[k] : v;
  return v;
}

// the ascending multisets a [na] and b [nb] merged into one and ranked on the way (rank_genotype's sum, as exact_gamete_kernel)
template <int KM>
__device__ __forceinline__ long long merged_rank(const int (&a)[KM], int na, const int (&b)[KM], int nb) {
  int ia = 0, ib = 0;
  long long rank = 0;
  for (int k = 0; k < na + nb; k++) {
    const int va = pick(a, ia), vb = pick(b, ib);
    const bool take = ib >= nb || (ia < na && va <= vb);
    ia += take ? 1 : 0;
    ib += take ? 0 : 1;
    rank += cwr(take ? va : vb, k + 1);
  }
  return rank;
}

// sum over the workgroup's EXACT_THREADS lanes in every lane: the wave_sum tree, then the wavefronts in order
__device__ __forceinline__ double family_block_sum(double v, double *red) {
  constexpr int NW = EXACT_THREADS / WAVE;
  v = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; w++) s += red[w];
  __syncthreads();
  return s;
}

// ---- the tables of one parent shape (H, K): the same for every record of the launch ----
struct FamilyTables {
  int *fcnt;     // [G] distinct sub-multisets of the genotype
  int *fidx;     // [G][W] their gamete ranks, in VCF order
  double *fwt;   // [G][W] prod_h C(c_h(g), a_h) / C(K, t)
  int *bidx;     // [NA][NA] the genotype a + r of every complement r of gamete a, in VCF order of r
  double *bwt;   // [NA][NA] its weight likewise
  int K, T, W;
  long long G, NA;
};

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_rows_kernel(const FamilyTables P) {
  const long long gi = (long long)blockIdx.x * EXACT_THREADS + threadIdx.x;
  if (gi >= P.G) return;
  int g[KM];
  unrank_genotype(gi, P.K, g);
  const double all = (double)small_binom(P.K, P.T);
  int n = 0;
  for_each_submultiset<KM>(g, P.K, P.T, [&](long long ra, long long, const int *x, const int *cn, int m) {
    int w = 1;
    for (int i = 0; i < m; i++) w *= small_binom(cn[i], x[i]);
    if (n < P.W) {
      P.fidx[(size_t)gi * P.W + n] = (int)ra;
      P.fwt[(size_t)gi * P.W + n] = (double)w / all;
    }
    n++;
  });
  P.fcnt[gi] = n < P.W ? n : P.W;
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_cols_kernel(const FamilyTables P) {
  const long long idx = (long long)blockIdx.x * EXACT_THREADS + threadIdx.x;
  if (idx >= P.NA * P.NA) return;
  const int T = P.T;
  int a[KM], r[KM];
  unrank_genotype(idx / P.NA, T, a);
  unrank_genotype(idx % P.NA, T, r);  // (K - t = t: the complements are the gametes)
  const long long rank = merged_rank(a, T, r, T);
  // prod_h C(c_h(g), a_h) over the runs of a: the run's length x and the copies y of its haplotype in r
  int w = 1, x = 0;
#pragma unroll
  for (int i = 0; i < KM; i++) {
    if (i >= T) continue;
    x++;
    if (i == T - 1 || (i + 1 < KM && a[i + 1] != a[i])) {
      int y = 0;
#pragma unroll
      for (int j = 0; j < KM; j++) y += (j < T && r[j] == a[i]) ? 1 : 0;
      w *= small_binom(x + y, x);
      x = 0;
    }
  }
  P.bidx[idx] = (int)rank;
  P.bwt[idx] = (double)w / (double)small_binom(P.K, T);
}

// ---- per record: Mult(a; t, f) of every gamete, and lp + llk of every parent genotype ----
struct FamilyMultParams {
  const double *freqs;  // [R][stride]
  int stride, T, nblk;
  long long NA;
  double *mult;         // [R][NA]
};

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_mult_kernel(const FamilyMultParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.NA) return;
  const double *fr = P.freqs + (size_t)rec * P.stride;
  int a[KM];
  unrank_genotype(idx, P.T, a);
  // the multinomial coefficient from the runs of a, the frequencies multiplied in the order of a (as exact_gamete_kernel)
  double coef = 1.0, pf = 1.0;
  int x = 0;
  for (int i = 0; i < P.T; i++) {
    x++;
    pf *= fr[a[i]];
    if (i == P.T - 1 || a[i + 1] != a[i]) {
      coef *= (double)small_binom(i + 1, x);
      x = 0;
    }
  }
  P.mult[(size_t)rec * P.NA + idx] = coef * pf;
}

struct FamilyPriorParams {
  const double *llk64;       // [R][G]
  const double *inbreeding;  // [R], or null: the flat genotype prior -log(G)
  const double *freqs;       // [R][stride]
  int stride, H, K, nblk;
  long long G;
  double *joint;             // [R][G] lp + llk
};

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_prior_kernel(const FamilyPriorParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const bool has_prior = P.inbreeding != nullptr;
  PriorTab pt;
  int *bin;
  cross_setup(smem, P.H, P.K, has_prior, has_prior ? P.inbreeding[rec] : 0.0, P.freqs + (size_t)rec * P.stride, pt, bin);
  const long long gi = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (gi >= P.G) return;
  int g[KM];
  unrank_genotype(gi, P.K, g);
  const double lp = has_prior ? calling_log_prior(pt, g, P.K) : -log((double)P.G);
  P.joint[(size_t)rec * P.G + gi] = P.llk64[(size_t)rec * P.G + gi] + lp;
}

// ---- one progeny of every record (a "round"): the progeny's likelihoods are at llk + rec * llk_pitch ----
struct FamilyRoundParams {
  const double *llk;         // the round's progeny of record 0
  long long llk_pitch;       // doubles between the records' progeny of this round
  const int32_t *reads;      // the round's flag of record 0, or null: every progeny has reads
  int reads_pitch;
  int H, TP, TQ, nblk;
  long long GP, GQ, GC, NAP, NAQ;
  FamilyTables tp, tq;
  const double *mult_p, *mult_q;  // [R][NA]
  const double *err_p, *err_q;    // [R]
  double *lmax;              // [R] m_c
  double *pair;              // [R][NAP][NAQ] T_c
  double *dp;                // [R][NAQ] sum_a Mult_P(a) T_c[a][b]
  double *v;                 // [R][GP][NAQ] V_c
  double *s;                 // [R][GP][GQ] S, then w
  double *y;                 // [R][GP][NAQ] Y_c
  double *cy;                // [R][NAQ] sum_gP Y_c[gP][b]
  double *rr;                // [R][NAP][NAQ] R_c
  double *dsum;              // [R][GP] the rows' sums of w / M_c
  double *dtot;              // [R] their sum
  double *drow;              // [R][GP][GQ] w / M_c where the rows are not staged, or null
  int staged;
  const double *log_z;       // [R]
  double *q;                 // the round's q_c of record 0
  long long q_pitch;
  double *pred;              // the round's predictive log evidence of record 0
  int pred_pitch;
};

__device__ __forceinline__ bool family_has_reads(const FamilyRoundParams &P, int rec) {
  return P.reads == nullptr || P.reads[(size_t)rec * P.reads_pitch] != 0;
}

static __global__ __launch_bounds__(EXACT_THREADS) void family_max_kernel(const FamilyRoundParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW];
  const int rec = blockIdx.x;
  const double *llk = P.llk + (size_t)rec * P.llk_pitch;
  double m = -INFINITY;
  bool bad = false;
  for (long long g = threadIdx.x; g < P.GC; g += EXACT_THREADS) {
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
    P.lmax[rec] = any_bad ? NAN : m;
  }
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_pair_kernel(const FamilyRoundParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  if (!family_has_reads(P, rec)) return;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.NAP * P.NAQ) return;
  const int TP = P.TP, TQ = P.TQ;
  int a[KM], b[KM];
  unrank_genotype(idx / P.NAQ, TP, a);
  unrank_genotype(idx % P.NAQ, TQ, b);
  const long long rank = merged_rank(a, TP, b, TQ);
  const double l = P.llk[(size_t)rec * P.llk_pitch + rank];
  P.pair[(size_t)rec * P.NAP * P.NAQ + idx] = exp(l - P.lmax[rec]);  // (m_c = -inf, or a NaN likelihood: NaN)
}

// out[rec][col] = sum_row wgt[rec][row] mat[rec][row][col] (wgt null: 1): 64 columns a workgroup, its four wavefronts each a
// contiguous quarter of the rows in order, the quarters then added in order
struct FamilyColsumParams {
  const double *mat;  // [R][rows][cols]
  const double *wgt;  // [R][rows] or null
  long long rows, cols;
  int nblk;           // tiles of 64 columns
  double *out;        // [R][cols]
};

static __global__ __launch_bounds__(EXACT_THREADS) void family_colsum_kernel(const FamilyColsumParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW][WAVE];
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const long long col = (long long)blk * WAVE + lane;
  const long long chunk = (P.rows + NW - 1) / NW;
  const long long lo = wave * chunk;
  long long hi = lo + chunk;
  if (hi > P.rows) hi = P.rows;
  double sum = 0.0;
  if (col < P.cols) {
    const double *mat = P.mat + (size_t)rec * P.rows * P.cols;
    const double *wgt = P.wgt ? P.wgt + (size_t)rec * P.rows : nullptr;
    for (long long r = lo; r < hi; r++) sum += wgt ? wgt[r] * mat[(size_t)r * P.cols + col] : mat[(size_t)r * P.cols + col];
  }
  red[wave][lane] = sum;
  __syncthreads();
  if (wave == 0 && col < P.cols) {
    double total = red[0][lane];
#pragma unroll
    for (int w = 1; w < NW; w++) total += red[w][lane];
    P.out[(size_t)rec * P.cols + col] = total;
  }
}

static __global__ __launch_bounds__(EXACT_THREADS) void family_v_kernel(const FamilyRoundParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  if (!family_has_reads(P, rec)) return;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.GP * P.NAQ) return;
  const long long gp = idx / P.NAQ, b = idx % P.NAQ;
  const double *pair = P.pair + (size_t)rec * P.NAP * P.NAQ;
  const int n = P.tp.fcnt[gp];
  const int *fi = P.tp.fidx + (size_t)gp * P.tp.W;
  const double *fw = P.tp.fwt + (size_t)gp * P.tp.W;
  double own = 0.0;
  for (int k = 0; k < n; k++) own += fw[k] * pair[(size_t)fi[k] * P.NAQ + b];
  const double e = P.err_p[rec];
  P.v[(size_t)rec * P.GP * P.NAQ + idx] = (1.0 - e) * own + e * P.dp[(size_t)rec * P.NAQ + b];
}

// LDS of family_row_kernel in doubles: V_c[gP][.], and for the back projection the row of w / M_c; 0 where they do not fit
inline size_t family_row_lds(long long NAQ, long long GQ, bool back) {
  const long long n = NAQ + (back ? GQ : 0);
  return n * 8 > FAMILY_LDS_BUDGET ? 0 : (size_t)n * 8;
}

// One workgroup per (record, gP): M_c[gP][.] from V_c[gP][.].  Forward: S[gP][gQ] += log M_c + m_c.  Back: the row of w / M_c, its
// sum, and Y_c[gP][.] from it.
template <bool BACK>
__global__ __launch_bounds__(EXACT_THREADS) void family_row_kernel(const FamilyRoundParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[EXACT_THREADS / WAVE];
  const int rec = (int)(blockIdx.x / P.GP);
  const long long gp = blockIdx.x % P.GP;
  const bool reads = family_has_reads(P, rec);
  if (!BACK && !reads) return;
  const long long NAQ = P.NAQ, GQ = P.GQ;
  const double e = P.err_q[rec];
  const double *mult = P.mult_q + (size_t)rec * NAQ;
  const double *vrow = P.v + ((size_t)rec * P.GP + gp) * NAQ;
  double *srow = P.s + ((size_t)rec * P.GP + gp) * GQ;
  double *drow = BACK ? (P.staged ? reinterpret_cast<double *>(smem) + NAQ : P.drow + ((size_t)rec * P.GP + gp) * GQ) : nullptr;
  double dv = 0.0;
  if (reads) {
    if (P.staged) {
      double *stage = reinterpret_cast<double *>(smem);
      for (long long b = threadIdx.x; b < NAQ; b += EXACT_THREADS) stage[b] = vrow[b];
      __syncthreads();
      vrow = stage;
    }
    double part = 0.0;
    for (long long b = threadIdx.x; b < NAQ; b += EXACT_THREADS) part += mult[b] * vrow[b];
    dv = family_block_sum(part, red);
  }
  const double m = reads ? P.lmax[rec] : 0.0;
  double dpart = 0.0;
  for (long long gq = threadIdx.x; gq < GQ; gq += EXACT_THREADS) {
    double M = 1.0;
    if (reads) {
      const int n = P.tq.fcnt[gq];
      const int *fi = P.tq.fidx + (size_t)gq * P.tq.W;
      const double *fw = P.tq.fwt + (size_t)gq * P.tq.W;
      double own = 0.0;
      for (int k = 0; k < n; k++) own += fw[k] * vrow[fi[k]];
      M = (1.0 - e) * own + e * dv;
    }
    if (!BACK) {
      srow[gq] += log(M) + m;
    } else {
      const double w = srow[gq];
      const double d = reads ? (w == 0.0 ? 0.0 : w / M) : w;
      drow[gq] = d;
      dpart += d;
    }
  }
  if (!BACK) return;
  const double dsum = family_block_sum(dpart, red);  // (its barriers also publish drow, in LDS or -- to this workgroup -- in global memory)
  if (threadIdx.x == 0) P.dsum[(size_t)rec * P.GP + gp] = dsum;
  double *yrow = P.y + ((size_t)rec * P.GP + gp) * NAQ;
  for (long long b = threadIdx.x; b < NAQ; b += EXACT_THREADS) {
    const int *bi = P.tq.bidx + (size_t)b * NAQ;
    const double *bw = P.tq.bwt + (size_t)b * NAQ;
    double own = 0.0;
    for (long long c = 0; c < NAQ; c++) own += bw[c] * drow[bi[c]];
    yrow[b] = (1.0 - e) * own + e * mult[b] * dsum;
  }
}

static __global__ __launch_bounds__(EXACT_THREADS) void family_r_kernel(const FamilyRoundParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.NAP * P.NAQ) return;
  const long long a = idx / P.NAQ, b = idx % P.NAQ;
  const double *y = P.y + (size_t)rec * P.GP * P.NAQ;
  const int *bi = P.tp.bidx + (size_t)a * P.NAP;
  const double *bw = P.tp.bwt + (size_t)a * P.NAP;
  double own = 0.0;
  for (long long c = 0; c < P.NAP; c++) own += bw[c] * y[(size_t)bi[c] * P.NAQ + b];
  const double e = P.err_p[rec];
  P.rr[(size_t)rec * P.NAP * P.NAQ + idx] = (1.0 - e) * own + e * P.mult_p[(size_t)rec * P.NAP + a] * P.cy[(size_t)rec * P.NAQ + b];
}

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void family_q_kernel(const FamilyRoundParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const long long j = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (j >= P.GC) return;
  const bool reads = family_has_reads(P, rec);
  const double *rr = P.rr + (size_t)rec * P.NAP * P.NAQ;
  int gc[KM];
  unrank_genotype(j, P.TP + P.TQ, gc);
  double sum = 0.0;
  for_each_submultiset<KM>(gc, P.TP + P.TQ, P.TP, [&](long long ra, long long rb, const int *, const int *, int) { sum += rr[(size_t)ra * P.NAQ + rb]; });
  const double m = reads ? P.lmax[rec] : 0.0;
  const double scale = reads ? exp(P.llk[(size_t)rec * P.llk_pitch + j] - m) : 1.0;
  P.q[(size_t)rec * P.q_pitch + j] = scale * sum;
  if (j == 0) {
    const double lz = P.log_z[rec];
    const bool ok = lz > -INFINITY && lz < INFINITY;
    P.pred[(size_t)rec * P.pred_pitch] = !ok ? NAN : (reads ? m - log(P.dtot[rec]) : 0.0);
  }
}

// ---- the streaming pass over S + (lp + llk)_P + (lp + llk)_Q: a tile is one row gP ----
struct FamilyPostParams {
  const double *joint_p, *joint_q;  // [R][GP], [R][GQ]
  long long GP, GQ;
  double *s;       // [R][GP][GQ]: S in, w out
  double *part;    // [R][GP][2]: the row's maximum, and sum exp(. - maximum)
  double *log_z;   // [R]
  double *post_p;  // [R][GP]
};

static __global__ __launch_bounds__(EXACT_THREADS) void family_rowstat_kernel(const FamilyPostParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW];
  const int rec = (int)(blockIdx.x / P.GP);
  const long long gp = blockIdx.x % P.GP;
  const double *srow = P.s + ((size_t)rec * P.GP + gp) * P.GQ;
  const double *jq = P.joint_q + (size_t)rec * P.GQ;
  const double jp = P.joint_p[(size_t)rec * P.GP + gp];
  double m = -INFINITY;
  bool bad = false;
  for (long long gq = threadIdx.x; gq < P.GQ; gq += EXACT_THREADS) {
    const double l = srow[gq] + jp + jq[gq];
    bad = bad || l != l;
    m = l > m ? l : m;
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
  __syncthreads();
  double part = 0.0;
  for (long long gq = threadIdx.x; gq < P.GQ; gq += EXACT_THREADS) {
    const double l = srow[gq] + jp + jq[gq];
    part += l == -INFINITY ? 0.0 : exp(l - m);
  }
  const double sum = family_block_sum(part, red);
  if (threadIdx.x == 0) {
    P.part[((size_t)rec * P.GP + gp) * 2] = any_bad ? NAN : m;
    P.part[((size_t)rec * P.GP + gp) * 2 + 1] = any_bad ? NAN : sum;
  }
}

// the rows of a record in row order: log Z_fam = maximum + log(total relative to it); a NaN row: NaN; no finite entry: -inf
static __global__ __launch_bounds__(WAVE) void family_z_kernel(const FamilyPostParams P) {
  const int rec = blockIdx.x;
  if (threadIdx.x != 0) return;
  const double *part = P.part + (size_t)rec * P.GP * 2;
  double m = -INFINITY;
  bool bad = false;
  for (long long r = 0; r < P.GP; r++) {
    const double mr = part[r * 2];
    bad = bad || mr != mr;
    m = mr > m ? mr : m;
  }
  double total = 0.0;
  for (long long r = 0; r < P.GP; r++) {
    const double mr = part[r * 2];
    if (mr > -INFINITY) total += part[r * 2 + 1] * exp(mr - m);
  }
  P.log_z[rec] = bad ? NAN : (m > -INFINITY ? m + log(total) : -INFINITY);
}

static __global__ __launch_bounds__(EXACT_THREADS) void family_weight_kernel(const FamilyPostParams P) {
  __shared__ double red[EXACT_THREADS / WAVE];
  const int rec = (int)(blockIdx.x / P.GP);
  const long long gp = blockIdx.x % P.GP;
  double *srow = P.s + ((size_t)rec * P.GP + gp) * P.GQ;
  const double *jq = P.joint_q + (size_t)rec * P.GQ;
  const double jp = P.joint_p[(size_t)rec * P.GP + gp];
  const double lz = P.log_z[rec];
  const bool ok = lz > -INFINITY && lz < INFINITY;
  double part = 0.0;
  for (long long gq = threadIdx.x; gq < P.GQ; gq += EXACT_THREADS) {
    const double l = srow[gq] + jp + jq[gq];
    const double w = ok ? (l == -INFINITY ? 0.0 : exp(l - lz)) : NAN;
    srow[gq] = w;
    part += w;
  }
  const double sum = family_block_sum(part, red);
  if (threadIdx.x == 0) P.post_p[(size_t)rec * P.GP + gp] = sum;
}

// the first maximum of every row of p [rows][G] in VCF order and its value; a row with a NaN: -1 and NaN
struct FamilyModeParams {
  const double *p;
  long long G, pitch;        // doubles between the rows
  long long *mode;           // [rows * out_pitch]
  double *prob;
  int out_pitch;
};

static __global__ __launch_bounds__(EXACT_THREADS) void family_mode_kernel(const FamilyModeParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double redm[NW];
  __shared__ long long redi[NW];
  const int row = blockIdx.x;
  const double *p = P.p + (size_t)row * P.pitch;
  double m = -INFINITY;
  long long mi = LLONG_MAX;
  bool bad = false;
  for (long long g = threadIdx.x; g < P.G; g += EXACT_THREADS) {  // (ascending within the thread: the first maximum stays)
    const double v = p[g];
    bad = bad || v != v;
    if (v > m) {
      m = v;
      mi = g;
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
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    redm[threadIdx.x / WAVE] = m;
    redi[threadIdx.x / WAVE] = mi;
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++)
      if (redm[w] > m || (redm[w] == m && redi[w] < mi)) {
        m = redm[w];
        mi = redi[w];
      }
    const bool ok = !any_bad && mi != LLONG_MAX;
    P.mode[(size_t)row * P.out_pitch] = ok ? mi : -1;
    P.prob[(size_t)row * P.out_pitch] = ok ? m : NAN;
  }
}

}  // namespace mchap
