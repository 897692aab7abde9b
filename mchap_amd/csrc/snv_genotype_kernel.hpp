// find-snvs genotype calls (mchap_amd/find_snvs.py genotypes_device; the rule: include/mchap_hip.h mchap_snv_genotypes_device): the
// exact caller's posterior mode (reference calling/exact.py posterior_mode) restricted to one position, straight from the pileup's
// depth tensor and the filter launch's flags and ADMF.
//   One lane per (row, sample) pair, pairs in row-major order: the lane's int4 of depths is one coalesced load.
//   LDS: logt[K][c] = log((c p_call + (K - c) p_other) / K) for every ploidy 1..15, filled once per workgroup; then per lane a table
//   w[j][c] (enumerated allele j at dosage c: depth x logt plus the allele's prior term), laid out [j][c][lane] so that lanes reading
//   different dosages stay on their own banks.  Every LDS access is an index into one array: no pointer into LDS is ever compared
//   or selected (docs/HISTORY A.0: a pointer to LDS offset 0 is a null pointer).
//   The genotypes of K copies over m <= 4 alleles in VCF order are three nested dosage loops (the highest allele outermost), so no
//   genotype table is needed: pass 1 keeps the maximum and the first index that reaches it, pass 2 sums exp(lp - max) in the same
//   order.  A lane works alone -- no atomics, no cross-lane sums -- so a run is reproducible bit for bit.
// Prior terms (reference calling/prior.py log_genotype_prior), without the terms that are equal for every genotype of the pair and
// cancel in the posterior: t[j][c] = sum_{i < c} log(x_j + i) - log(c!) with x_j = alpha_j = f_j (1 - F) / F for F > 0, and
// t[j][c] = c log(f_j) - log(c!) for F = 0; f_j = 1 / m without frequencies.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mchap {

constexpr int SNV_MAX_PLOIDY = 15;  // MCHAP_MAX_PLOIDY_DENOVO
constexpr int SNV_LOGT = 16 * 16;   // doubles of the shared log table: [ploidy 0..15][dosage 0..15]

// doubles of LDS one workgroup of `threads` lanes needs when the highest ploidy is rows - 1
__host__ __device__ constexpr int snv_lds_doubles(int rows, int threads) { return SNV_LOGT + 4 * rows * threads; }

__device__ __forceinline__ int snv_pick(const int4 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : a == 2 ? v.z : v.w; }

// Calls fn(lp, index) for every genotype of ploidy K over m alleles in VCF order.  w: the lane's table, w[(j * rows + c) * stride].
template <class Fn>
__device__ __forceinline__ void snv_walk(const double *w, int rows, int stride, int m, int K, Fn fn) {
  int index = 0;
  const int n3 = m > 3 ? K : 0;
  for (int c3 = 0; c3 <= n3; c3++) {
    const double w3 = w[(3 * rows + c3) * stride];
    const int r3 = K - c3, n2 = m > 2 ? r3 : 0;
    for (int c2 = 0; c2 <= n2; c2++) {
      const double w2 = w3 + w[(2 * rows + c2) * stride];
      const int r2 = r3 - c2, n1 = m > 1 ? r2 : 0;
      for (int c1 = 0; c1 <= n1; c1++) {
        const double lp = (w2 + w[(rows + c1) * stride]) + w[(r2 - c1) * stride];
        fn(lp, index);
        index++;
      }
    }
  }
}

// rows: highest ploidy of the launch + 1 (the host has checked every ploidy); blockDim.x lanes, snv_lds_doubles(rows, blockDim.x)
// doubles of dynamic LDS.  gt [n_pairs] int32: the mode's genotype index over the enumerated alleles, -1 for a row that is not a
// record and for a no-call; gpm [n_pairs] float64: the mode's posterior probability, NaN where gt is -1.
__global__ void __launch_bounds__(256) snv_genotype_kernel(const int32_t *depth, const int32_t *flags, const double *admf,
                                                           int64_t n_pairs, int n_samples, const int32_t *ploidy,
                                                           const double *inbreeding, int use_admf, double p_call, double p_other,
                                                           int rows, int32_t *gt, double *gpm) {
  extern __shared__ double snv_lds[];
  const int tid = threadIdx.x, stride = blockDim.x;
  for (int i = tid; i < SNV_LOGT; i += stride) {
    const int K = i >> 4, c = i & 15;
    snv_lds[i] = (K >= 1 && c <= K) ? log(((double)c * p_call + (double)(K - c) * p_other) / (double)K) : 0.0;
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * stride + tid;
  if (p >= n_pairs) return;
  const int64_t row = p / n_samples;
  const int s = (int)(p - row * n_samples);
  const int fl = flags[row];
  const int K = ploidy[s];
  const double F = inbreeding[s];
  const bool prior = !isnan(F);
  const bool freqs = prior && use_admf != 0;
  bool call = (fl & 1) != 0 && K >= 1 && K < rows && K <= SNV_MAX_PLOIDY && !(prior && !(F >= 0.0 && F < 1.0));

  // the enumerated alleles: the listed ones (the reference, then the kept alternates in VCF order) but for a masked reference
  const int4 v = reinterpret_cast<const int4 *>(depth)[p];
  const bool masked = ((fl >> 16) & 1) != 0;
  double d[4] = {0.0, 0.0, 0.0, 0.0}, f[4] = {0.0, 0.0, 0.0, 0.0};
  int m = 0;
  double f_sum = 0.0, d_sum = 0.0;
  if (call) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int a = (fl >> (8 + 2 * i)) & 3;
      const bool listed = i == 0 ? !masked : ((fl >> (1 + a)) & 1) != 0;
      if (!listed) continue;
      const double da = (double)snv_pick(v, a);
      const double fa = freqs ? admf[4 * row + a] : 0.0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j == m) {
          d[j] = da;
          f[j] = fa;
        }
      d_sum += da;
      f_sum += fa;
      m++;
    }
    call = m >= 1 && d_sum > 0.0;
  }
  if (call && freqs) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f[j] = f[j] / f_sum;
      if (j < m && !(f[j] > 0.0)) call = false;  // a zero (or undefined) frequency: AF0
    }
  }
  if (!call) {
    gt[p] = -1;
    gpm[p] = NAN;
    return;
  }

  // the lane's table
  const int lane_w = SNV_LOGT + tid;  // w[j][c] = snv_lds[lane_w + (j * rows + c) * stride]
  const double scale = (prior && F > 0.0) ? (1.0 - F) / F : 1.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j >= m) {
      snv_lds[lane_w + (j * rows) * stride] = 0.0;
      continue;
    }
    // x: alpha_j (F > 0), f_j (F = 0 with frequencies), 1 (F = 0 without: the term is the same for every allele)
    const double x = !prior ? 1.0 : F > 0.0 ? (freqs ? f[j] : 1.0 / (double)m) * scale : (freqs ? f[j] : 1.0);
    double t = 0.0;
    for (int c = 0; c <= K; c++) {
      if (prior && c > 0) t += log(x + (F > 0.0 ? (double)(c - 1) : 0.0)) - log((double)c);
      const double l = d[j] > 0.0 ? d[j] * snv_lds[K * 16 + c] : 0.0;  // a term with no depth is skipped (error rate 0: -inf x 0)
      snv_lds[lane_w + (j * rows + c) * stride] = l + t;
    }
  }

  const double *w = snv_lds + lane_w;
  double best = -INFINITY;
  int arg = -1;
  snv_walk(w, rows, stride, m, K, [&](double lp, int index) {
    if (lp > best) {
      best = lp;
      arg = index;
    }
  });
  if (arg < 0) {  // no genotype holds every allele seen (error rate 0 and more alleles seen than the ploidy)
    gt[p] = -1;
    gpm[p] = NAN;
    return;
  }
  double sum = 0.0;
  snv_walk(w, rows, stride, m, K, [&](double lp, int) { sum += exp(lp - best); });
  gt[p] = arg;
  gpm[p] = exp(best - (best + log(sum)));
}

}  // namespace mchap
