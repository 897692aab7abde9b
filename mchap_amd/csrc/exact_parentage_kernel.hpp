// Candidate parent pairs ranked per progeny (call-exact --parentage, application.Parentage) for MI355X (gfx950): the cross evidence
// of every progeny under every pair of two gamete tables at once, over the likelihoods the exact caller left in llk64.  Per record
// with H haplotypes, n_a gamete rows of t_a haplotypes (NA = C(H + t_a - 1, t_a) gametes each), n_b rows of t_b haplotypes, progeny c
// of ploidy K_c = t_a + t_b; every multiset in VCF order:
//   T_c[a][b]   = exp(llk_c[rank(a + b)] - m_c),  m_c = max llk_c                      never stored: formed again per column chunk
//   W_c[j][a]   = sum_b T_c[a][b] gam_b[j][b]                                           b in VCF order, one term after the other
//   Z_c[i][j]   = sum_a gam_a[i][a] W_c[j][a]                                           family_block_sum's order (below)
//   log_z[c][i][j] = m_c + log Z_c[i][j]
// The pairs (a, b) correspond one to one to the pairs (progeny genotype gc, distinct sub-multiset a of gc), so Z_c[i][j] is
// sum_gc X_ij[gc] exp(llk_c[gc] - m_c) with X_ij the cross prior of exact_cross_prior_kernel: the cross evidence of the two launches
// of --cross-calls, for every pair of rows from one pass over the pairs of gametes.  A row is any distribution over the gametes: a
// candidate's table from exact_gamete_kernel, or the population's Mult(a; t, f) -- what that kernel returns at a gamete error of 1 --,
// which parentage_mult_kernel forms (family_mult_kernel's arithmetic, written into a row of a table).
//
// Gather form throughout: one owning lane per output cell, a fixed summation order, no atomics.
//   parentage_cw_kernel   the table cw[k][n] = C(n + k, k + 1) of rank_genotype's terms, once per call: no lane divides in the loops.
//   parentage_max_kernel  m_c per (record, progeny): NaN where a likelihood is NaN.
//   parentage_w_kernel    one lane per gamete a, unranked once into registers; workgroups over (record, group of progeny, tile of
//                         256 gametes, chunk of PARENTAGE_COLS columns j).  b walks 0 .. NB - 1 with next_genotype, the same b in
//                         every lane, so gam_b[j][b] is a broadcast read of the chunk's rows, staged in LDS PARENTAGE_BTILE gametes
//                         b at a time; one rank and one exp per (a, b) serve the chunk's PARENTAGE_COLS accumulators.  Where NA is
//                         at most 128 a workgroup takes 256 / NA progeny of the record side by side.
//   parentage_z_kernel    one workgroup per (record, progeny, column j), the rows i one after the other: lane l adds the terms
//                         a = l, l + 256, l + 512, ... in that order, then the wave_sum tree, then the four wavefronts in order.
// Every sum's order depends on NA and NB alone: equal inputs give equal bits whatever the place of a record in the call, the
// number and order of the rows and of the progeny, and the width of a column chunk.  A NaN row gives NaN in its row or column of
// log_z and nowhere else (0 * NaN is NaN); a progeny with a NaN likelihood or without a finite one has m_c NaN or -inf and NaN
// throughout; Z = 0 gives exactly -inf; a progeny flagged without reads is not read and has exactly 0.
#pragma once
#include "exact_family_kernel.hpp"

namespace mchap {

constexpr int PARENTAGE_COLS = 16;     // columns j a lane accumulates at once
constexpr int PARENTAGE_BTILE = 256;   // gametes b of the chunk's rows staged in LDS at a time
constexpr int PARENTAGE_TMAX = 7;      // largest gamete size

struct ParentageParams {
  const double *gam_a;     // [R][n_a][NA]
  const double *gam_b;     // [R][n_b][NB]
  const double *llk;       // [R][C][GC]
  const int32_t *reads;    // [R][C], or null: every progeny has reads
  int H, TA, TB, C, n_a, n_b;
  int ppb;                 // progeny of a record a workgroup of parentage_w_kernel takes (NA <= 128: 256 / NA, else 1)
  int ngrp, ntile, nchunk; // groups of ppb progeny, tiles of EXACT_THREADS gametes a, chunks of PARENTAGE_COLS columns
  long long NA, NB, GC;
  long long *cw;           // [TA + TB][H]
  double *lmax;            // [R][C]
  double *w;               // [R][C][n_b][NA]
  double *log_z;           // [R][C][n_a][n_b]
};

// LDS of parentage_w_kernel: the rank table, then the staged rows
inline size_t parentage_w_lds(int H, int KC) { return ((size_t)H * KC + (size_t)PARENTAGE_COLS * PARENTAGE_BTILE) * 8; }

__device__ __forceinline__ bool parentage_has_reads(const ParentageParams &P, int rec, int c) {
  return P.reads == nullptr || P.reads[(size_t)rec * P.C + c] != 0;
}

static __global__ __launch_bounds__(EXACT_THREADS) void parentage_cw_kernel(const ParentageParams P) {
  const int q = blockIdx.x * EXACT_THREADS + threadIdx.x;
  if (q >= (P.TA + P.TB) * P.H) return;
  P.cw[q] = cwr(q % P.H, q / P.H + 1);
}

// Mult(a; t, f) of every gamete into rows + rec * pitch: the multinomial coefficient from the runs of a, the frequencies multiplied
// in the order of a (family_mult_kernel, exact_gamete_kernel)
struct ParentageMultParams {
  const double *freqs;  // [R][stride]
  int stride, T, nblk;
  long long NA, pitch;
  double *rows;
};

template <int KM = 8>
__global__ __launch_bounds__(EXACT_THREADS) void parentage_mult_kernel(const ParentageMultParams P) {
  const int rec = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
  const long long idx = (long long)blk * EXACT_THREADS + threadIdx.x;
  if (idx >= P.NA) return;
  const double *fr = P.freqs + (size_t)rec * P.stride;
  int a[KM];
  unrank_genotype(idx, P.T, a);
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
  P.rows[(size_t)rec * P.pitch + idx] = coef * pf;
}

static __global__ __launch_bounds__(EXACT_THREADS) void parentage_max_kernel(const ParentageParams P) {
  constexpr int NW = EXACT_THREADS / WAVE;
  __shared__ double red[NW];
  const int rec = blockIdx.x / P.C, c = blockIdx.x % P.C;
  if (!parentage_has_reads(P, rec, c)) return;
  const double *llk = P.llk + ((size_t)rec * P.C + c) * P.GC;
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
    P.lmax[(size_t)rec * P.C + c] = any_bad ? NAN : m;
  }
}

// The rank of the ascending multiset a [na] + b [nb] from the table, without merging: in the merged multiset a_i stands behind the
// i entries of a before it and the entries of b below it, b_j behind the j entries of b before it and the entries of a up to it --
// constant indices throughout, so that a and b stay in registers (rank_genotype's sum, the terms in another order: integers)
template <int TM>
__device__ __forceinline__ long long parentage_rank(const int (&a)[TM], int na, const int (&b)[TM], int nb, const long long *cw, int H) {
  long long rank = 0;
#pragma unroll
  for (int i = 0; i < TM; i++) {
    if (i >= na) continue;
    int at = i;
#pragma unroll
    for (int j = 0; j < TM; j++) at += (j < nb && b[j] < a[i]) ? 1 : 0;
    rank += cw[at * H + a[i]];
  }
#pragma unroll
  for (int j = 0; j < TM; j++) {
    if (j >= nb) continue;
    int at = j;
#pragma unroll
    for (int i = 0; i < TM; i++) at += (i < na && a[i] <= b[j]) ? 1 : 0;
    rank += cw[at * H + b[j]];
  }
  return rank;
}

// KM: the bound of the two gametes' arrays and of the unrolled loops over them (2, 4 or PARENTAGE_TMAX)
template <int KM>
__global__ __launch_bounds__(EXACT_THREADS) void parentage_w_kernel(const ParentageParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int H = P.H, TA = P.TA, TB = P.TB;
  long long *cw = reinterpret_cast<long long *>(smem);            // [TA + TB][H]
  double *stage = reinterpret_cast<double *>(cw + (TA + TB) * H); // [PARENTAGE_COLS][PARENTAGE_BTILE]
  int q = blockIdx.x;
  const int chunk = q % P.nchunk;
  q /= P.nchunk;
  const int tile = q % P.ntile;
  q /= P.ntile;
  const int grp = q % P.ngrp, rec = q / P.ngrp;
  for (int i = threadIdx.x; i < (TA + TB) * H; i += EXACT_THREADS) cw[i] = P.cw[i];
  // the lane's progeny and gamete
  const int cl = P.ppb > 1 ? (int)(threadIdx.x / P.NA) : 0;
  const long long ai = P.ppb > 1 ? (long long)(threadIdx.x % P.NA) : (long long)tile * EXACT_THREADS + threadIdx.x;
  const int c = grp * P.ppb + cl;
  const bool on = cl < P.ppb && c < P.C && ai < P.NA && parentage_has_reads(P, rec, c);
  const double *llk = P.llk + ((size_t)rec * P.C + (on ? c : 0)) * P.GC;
  const double m = on ? P.lmax[(size_t)rec * P.C + c] : 0.0;
  int a[KM], b[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) a[k] = 0;
  if (on) unrank_genotype(ai, TA, a);
#pragma unroll
  for (int k = 0; k < KM; k++) b[k] = 0;  // (gamete 0; the same in every lane, and next_genotype walks on across the tiles)
  const int j0 = chunk * PARENTAGE_COLS;
  const int nj = P.n_b - j0 < PARENTAGE_COLS ? P.n_b - j0 : PARENTAGE_COLS;
  double acc[PARENTAGE_COLS];
#pragma unroll
  for (int jj = 0; jj < PARENTAGE_COLS; jj++) acc[jj] = 0.0;
  const double *gb = P.gam_b + ((size_t)rec * P.n_b + j0) * P.NB;
  for (long long b0 = 0; b0 < P.NB; b0 += PARENTAGE_BTILE) {
    const int nb = P.NB - b0 < PARENTAGE_BTILE ? (int)(P.NB - b0) : PARENTAGE_BTILE;
    __syncthreads();  // (the tile before is read to its end; the first time round: the rank table is in place)
    for (int s = threadIdx.x; s < nj * nb; s += EXACT_THREADS) stage[(s / nb) * PARENTAGE_BTILE + s % nb] = gb[(size_t)(s / nb) * P.NB + b0 + s % nb];
    __syncthreads();
    for (int bi = 0; bi < nb; bi++) {
      if (on) {
        const double t = exp(llk[parentage_rank(a, TA, b, TB, cw, H)] - m);  // (m_c NaN or -inf: NaN)
#pragma unroll
        for (int jj = 0; jj < PARENTAGE_COLS; jj++)
          if (jj < nj) acc[jj] += t * stage[jj * PARENTAGE_BTILE + bi];
      }
      next_genotype(b, TB);
    }
  }
  if (!on) return;
  double *w = P.w + (((size_t)rec * P.C + c) * P.n_b + j0) * P.NA + ai;
#pragma unroll
  for (int jj = 0; jj < PARENTAGE_COLS; jj++)
    if (jj < nj) w[(size_t)jj * P.NA] = acc[jj];
}

static __global__ __launch_bounds__(EXACT_THREADS) void parentage_z_kernel(const ParentageParams P) {
  __shared__ double red[EXACT_THREADS / WAVE];
  int q = blockIdx.x;
  const int j = q % P.n_b;
  q /= P.n_b;
  const int c = q % P.C, rec = q / P.C;
  double *out = P.log_z + ((size_t)rec * P.C + c) * P.n_a * P.n_b + j;
  if (!parentage_has_reads(P, rec, c)) {
    for (int i = threadIdx.x; i < P.n_a; i += EXACT_THREADS) out[(size_t)i * P.n_b] = 0.0;
    return;
  }
  const double m = P.lmax[(size_t)rec * P.C + c];
  const double *w = P.w + (((size_t)rec * P.C + c) * P.n_b + j) * P.NA;
  const double *ga = P.gam_a + (size_t)rec * P.n_a * P.NA;
  for (int i = 0; i < P.n_a; i++) {
    double part = 0.0;
    for (long long a = threadIdx.x; a < P.NA; a += EXACT_THREADS) part += ga[(size_t)i * P.NA + a] * w[a];
    const double z = family_block_sum(part, red);
    if (threadIdx.x == 0) out[(size_t)i * P.n_b] = m + log(z);  // (exactly -inf where every product is 0)
  }
}

}  // namespace mchap
