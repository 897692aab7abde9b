// find-snvs pileup (mchap_amd/find_snvs.py; reference application/find_snvs.py bam_region_depths + write_vcf_block): three
// launches per block of targets over the block's alignment record bytes, uploaded per sample as one contiguous run.
//   1. overlap_kernel   -- htslib's mate-overlap quality rule (tweak_overlap_quality): one lane per reference position of each
//                          overlap segment of a read pair; rewrites the device copy of both mates' quality bytes in place.  Each
//                          position belongs to exactly one pair (the host pairs records one to one), so there is no race.
//   2. depth_kernel     -- one workgroup per (sample, tile of <= PILEUP_MAX_TILE target rows): an LDS histogram (tile x 4 u32)
//                          filled from the tile's aligned segments with LDS atomics, then stored as int32 depth[row][sample][4].
//                          Variant 1 (measurement only) adds straight into a zeroed depth tensor with global atomics instead.
//   3. filter_kernel    -- one lane per row: the reference's allele filter, allele order and ADMF, bit for bit (float64, sums
//                          over samples in sample order as numpy reduces axis 1 of a (P, S, 4) array).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mchap {

constexpr int PILEUP_MAX_TILE = 2048;
constexpr int PILEUP_THREADS = 256;

// BAM 4-bit base code -> allele index (A=1 C=2 G=4 T=8); every other code (=, N, IUPAC) counts nothing
__device__ __forceinline__ int nibble_allele(unsigned nib) {
  return nib == 1u ? 0 : nib == 2u ? 1 : nib == 4u ? 2 : nib == 8u ? 3 : -1;
}

__device__ __forceinline__ unsigned base_nibble(const uint8_t *bytes, int64_t nib) {
  const unsigned b = bytes[nib >> 1];
  return (nib & 1) ? (b & 15u) : (b >> 4);
}

// ov[k] = {a_seq_nibble, b_seq_nibble, a_qual_byte, b_qual_byte}; first[k] = first position of overlap segment k among the
// n_total positions (first[n_seg] = n_total).  a is the mate met first in file order.
__global__ void __launch_bounds__(PILEUP_THREADS) pileup_overlap_kernel(uint8_t *bytes, int64_t n_bytes, const int64_t *ov,
                                                                         const int64_t *first, int64_t n_seg, int64_t n_total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_total) return;
  int64_t lo = 0, hi = n_seg - 1;  // the segment k with first[k] <= t < first[k + 1]
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (first[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int64_t i = t - first[lo];
  const int64_t *o = ov + 4 * lo;
  const int64_t an = o[0] + i, bn = o[1] + i, aq = o[2] + i, bq = o[3] + i;
  if ((an >> 1) >= n_bytes || (bn >> 1) >= n_bytes || aq >= n_bytes || bq >= n_bytes || an < 0 || bn < 0 || aq < 0 || bq < 0) return;
  const unsigned qa = bytes[aq], qb = bytes[bq];
  unsigned na, nb;
  if (base_nibble(bytes, an) == base_nibble(bytes, bn)) {
    na = qa + qb < 200u ? qa + qb : 200u;
    nb = 0;
  } else if (qa >= qb) {
    na = (unsigned)(uint8_t)(0.8 * (double)qa);
    nb = 0;
  } else {
    na = 0;
    nb = (unsigned)(uint8_t)(0.8 * (double)qb);
  }
  bytes[aq] = (uint8_t)na;
  bytes[bq] = (uint8_t)nb;
}

// seg[k] = {row, length, seq_nibble, qual_byte}: an aligned (M/=/X) run of one read, clipped to one target and one tile; the
// segments of (sample s, tile t) are seg[tile_first[s * n_tiles + t] .. tile_first[s * n_tiles + t + 1]).
template <int VARIANT>
__global__ void __launch_bounds__(PILEUP_THREADS) pileup_depth_kernel(const uint8_t *bytes, int64_t n_bytes, const int64_t *seg,
                                                                       const int64_t *tile_first, int n_samples, int64_t n_tiles,
                                                                       int64_t n_rows, int tile, int min_bq, int32_t *depth) {
  __shared__ uint32_t hist[VARIANT == 0 ? PILEUP_MAX_TILE * 4 : 1];
  const int64_t t = blockIdx.x;
  const int s = blockIdx.y;
  const int64_t row0 = t * tile;
  const int rows = (int)((n_rows - row0) < tile ? (n_rows - row0) : tile);
  if (VARIANT == 0) {
    for (int i = threadIdx.x; i < rows * 4; i += blockDim.x) hist[i] = 0;
    __syncthreads();
  }
  const int64_t k0 = tile_first[(int64_t)s * n_tiles + t], k1 = tile_first[(int64_t)s * n_tiles + t + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
  for (int64_t k = k0 + wave; k < k1; k += n_waves) {
    const int64_t *g = seg + 4 * k;
    const int64_t r = g[0] - row0, len = g[1], nib0 = g[2], q0 = g[3];
    for (int64_t i = lane; i < len; i += 64) {
      const int64_t q = q0 + i, nib = nib0 + i;
      if (r + i < 0 || r + i >= rows || q < 0 || q >= n_bytes || nib < 0 || (nib >> 1) >= n_bytes) continue;
      const int a = nibble_allele(base_nibble(bytes, nib));
      if (a < 0 || (int)bytes[q] < min_bq) continue;
      if (VARIANT == 0)
        atomicAdd(&hist[(r + i) * 4 + a], 1u);
      else
        atomicAdd(&depth[((row0 + r + i) * n_samples + s) * 4 + a], 1);
    }
  }
  if (VARIANT == 0) {
    __syncthreads();
    for (int i = threadIdx.x; i < rows; i += blockDim.x) {
      const int4 v = make_int4((int)hist[4 * i], (int)hist[4 * i + 1], (int)hist[4 * i + 2], (int)hist[4 * i + 3]);
      *reinterpret_cast<int4 *>(depth + ((row0 + i) * n_samples + s) * 4) = v;
    }
  }
}

// flags[row]: bit 0 the row is a record; bits 1-4 the kept alleles (by allele index A C G T, before the reference allele is
// forced in); bits 8-15 the VCF order of the four alleles, two bits each (reference first); bit 16 REFMASKED.
// admf[row][a]: nanmean over samples of the kept alleles' frequencies (0 for an allele that is not kept), by allele index.
__global__ void __launch_bounds__(PILEUP_THREADS) pileup_filter_kernel(const int32_t *depth, const int8_t *ref_index, int64_t n_rows,
                                                                        int n_samples, double maf, int64_t mad, double ind_maf,
                                                                        int64_t ind_mad, int64_t min_ind, int32_t *flags, double *admf) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_rows) return;
  const int ref = ref_index[p];
  const int4 *d = reinterpret_cast<const int4 *>(depth) + p * n_samples;
  double f_sum[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t d_sum[4] = {0, 0, 0, 0}, n_ind[4] = {0, 0, 0, 0};
  for (int s = 0; s < n_samples; s++) {
    const int4 v = d[s];
    const int64_t c[4] = {v.x, v.y, v.z, v.w};
    const double tot = (double)(c[0] + c[1] + c[2] + c[3]);
    for (int a = 0; a < 4; a++) {
      const double f = (double)c[a] / tot;  // NaN for a sample without depth: every comparison below is false
      f_sum[a] += f;
      d_sum[a] += c[a];
      n_ind[a] += (f >= ind_maf && c[a] >= ind_mad) ? 1 : 0;
    }
  }
  bool keep[4];
  int n_keep = 0;
  for (int a = 0; a < 4; a++) {
    keep[a] = n_ind[a] >= min_ind;
    if (maf > 0.0) keep[a] = keep[a] && (f_sum[a] / (double)n_samples >= maf);  // a plain mean: NaN with a zero-depth sample
    if (mad > 0) keep[a] = keep[a] && d_sum[a] >= mad;
    n_keep += keep[a] ? 1 : 0;
  }
  if (ref < 0 || ref > 3 || n_keep <= 1) {
    flags[p] = 0;
    return;
  }
  // ADMF = nanmean_s(where(keep, f, 0))
  double m_sum[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t m_cnt[4] = {0, 0, 0, 0};
  for (int s = 0; s < n_samples; s++) {
    const int4 v = d[s];
    const int64_t c[4] = {v.x, v.y, v.z, v.w};
    const int64_t tot = c[0] + c[1] + c[2] + c[3];
    for (int a = 0; a < 4; a++) {
      if (!keep[a]) {
        m_cnt[a] += 1;  // (a zero, not NaN)
      } else if (tot > 0) {
        m_sum[a] += (double)c[a] / (double)tot;
        m_cnt[a] += 1;
      }
    }
  }
  double m[4];
  for (int a = 0; a < 4; a++) {
    m[a] = m_sum[a] / (double)m_cnt[a];
    admf[4 * p + a] = m[a];
  }
  // argsort(m, stable) reversed: descending, ties (and NaNs, which sort last ascending) higher index first
  int desc[4];
  for (int i = 0; i < 4; i++) {
    int rank = 0;
    for (int j = 0; j < 4; j++) {
      const bool less = !isnan(m[j]) && (isnan(m[i]) || m[j] < m[i]);
      const bool tie = (m[j] == m[i]) || (isnan(m[j]) && isnan(m[i]));
      rank += (less || (tie && j < i)) ? 1 : 0;
    }
    desc[3 - rank] = i;
  }
  int order = ref, k = 1;
  for (int i = 0; i < 4; i++)
    if (desc[i] != ref) order |= desc[i] << (2 * k++);
  const int mask = (keep[0] ? 1 : 0) | (keep[1] ? 2 : 0) | (keep[2] ? 4 : 0) | (keep[3] ? 8 : 0);
  flags[p] = 1 | (mask << 1) | (order << 8) | (keep[ref] ? 0 : (1 << 16));
}

}  // namespace mchap
