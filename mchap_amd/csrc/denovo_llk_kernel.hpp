// The chain context of the wavefront-per-chain sampler (kernel 1, denovo_mcmc_kernel.hpp), its wave-private LDS layout and its
// likelihood evaluation, with the test hook that evaluates many genotypes of one unit through them (mchap_llk_batch).  Apart from
// kernel 1 itself: the one part of it the shipped library carries -- the hook, and mchap_denovo_lds_bytes, which sizes by the layout.
// Reference citations as in denovo_mcmc_kernel.hpp.
#pragma once
#include "denovo_common.hpp"

namespace mchap {

// ---- wave-private LDS scratch -------------------------------------------------------------
struct WaveLayout {
  int w, pw, llk, rngn, sub, shift, hetrow, nal, probs, llks, optin, prior, buf, total;
};

__host__ __device__ inline WaveLayout wave_layout(int K, int M, int A, int T) {
  WaveLayout L;
  int o = 0;
  L.w = o; o += 8 * T * K;
  L.pw = o; o += 8 * K;
  L.llk = o; o += 8 * T;
  L.rngn = o; o += 8 * (T + 1);
  L.probs = o; o += 8 * (K * K + 2 > A ? K * K + 2 : A);
  L.llks = o; o += 8 * (K * K + 2 > A ? K * K + 2 : A);
  L.prior = o; o += 8 * (2 * (K + 1) + 4);
  int nb = snv_genotypes(A, K);
  if (nb < M * A) nb = M * A;
  if (nb < M + 4) nb = M + 4;  // also holds the interval end points of a structural step (ints)
  L.buf = o; o += 8 * nb;
  L.optin = o; o += 4 * K * K;
  L.sub = o; o += align8(2 * K * M);
  L.hetrow = o; o += align8(2 * M);
  L.shift = o; o += align8(M);
  L.nal = o; o += align8(M);
  L.total = align8(o);
  return L;
}

// ---- per-chain context -------------------------------------------------------------------
struct Chain {
  // LDS
  const double *rl;   // staged reads [M0*A][rpad]
  uint64_t *w;        // [T][K] haplotype words per temperature
  uint64_t *pw;       // [K] proposal
  double *llk_t;      // [T]
  uint64_t *rngn;     // [T+1] draw counters
  double *probs, *llks;
  double *prior_tab;  // [0..K] lg(dose+disp) - (lg(dose+1)+lg(disp)); [K+1..2K+1] lg(dose+1); then left, lgK1, K*luh
  double *buf;
  uint32_t *optin;
  uint16_t *sub;
  uint16_t *hetrow;   // het position * A
  uint8_t *shift;
  uint8_t *nal;       // n_alleles of het positions
  // scalars
  int K, Mh, A, T, rpad, lane;
  uint32_t amask;
  int bits;
  double invK;
  double inbreeding;  // NaN == None
  double luh;
  Rng rng;
  uint64_t *cache;   // this chain's {tag, value} table or nullptr
  uint32_t cache_mask;
  int key_bits;      // bits per haplotype word actually used (Mh * bits)
  bool w01;          // every read weight of the unit is 0 or 1: one logarithm per group of four chunks (read_log_sum_chunks)
};

template <int RPL>
__device__ __forceinline__ double eval_llk(const Chain &c, const uint64_t *hw, const double (&cnt)[RPL]) {
  double acc[RPL];
#pragma unroll
  for (int i = 0; i < RPL; i++) acc[i] = 0.0;
  for (int h = 0; h < c.K; h++) {
    const uint64_t wh = hw[h];
    double prod[RPL];
#pragma unroll
    for (int i = 0; i < RPL; i++) prod[i] = 1.0;
    for (int j = 0; j < c.Mh; j++) {
      const uint32_t a = (uint32_t)(wh >> c.shift[j]) & c.amask;
      const double *row = c.rl + (size_t)(c.hetrow[j] + a) * c.rpad + c.lane;
#pragma unroll
      for (int i = 0; i < RPL; i++) prod[i] *= row[WAVE * i];
    }
#pragma unroll
    for (int i = 0; i < RPL; i++) acc[i] += prod[i] * c.invK;
  }
  return wave_sum(read_log_sum_chunks<RPL>(acc, cnt, c.w01));
}

constexpr int CHAINS_PER_BLOCK = 4;

// Test hook: log_likelihood (assemble/likelihood.py:17-70) of many genotypes of one unit; one wavefront
// per genotype, same staging and evaluation code as the sampler.
template <int RPL>
__global__ __launch_bounds__(256) void llk_batch_kernel(const double *reads, int R, int M, int A, const int64_t *counts,
                                                        const int8_t *genotypes, int n_genotypes, int K, int rpad,
                                                        double *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  double *rl = reinterpret_cast<double *>(smem);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int MA = M * A;
  for (int r = threadIdx.x; r < rpad; r += blockDim.x) {
    for (int q = 0; q < MA; q++) {
      const double v = r < R ? reads[(size_t)r * MA + q] : 1.0;
      rl[(size_t)q * rpad + r] = isnan(v) ? 1.0 : v;
    }
  }
  double cnt[RPL];
#pragma unroll
  for (int i = 0; i < RPL; i++) {
    const int r = lane + WAVE * i;
    cnt[i] = (r < R) ? (counts ? (double)counts[r] : 1.0) : 0.0;
  }
  bool w01_l = true;
#pragma unroll
  for (int i = 0; i < RPL; i++) w01_l = w01_l && (cnt[i] == 0.0 || cnt[i] == 1.0);
  unsigned char *ws = smem + (size_t)MA * rpad * sizeof(double) + (size_t)wave * (8 * K + 4 * M + 64);
  Chain c;
  c.w01 = __ballot(!w01_l) == 0ull;  // (the samplers' rule: one logarithm per group of four chunks where the weights are 0 / 1)
  c.rl = rl;
  c.pw = reinterpret_cast<uint64_t *>(ws);
  c.hetrow = reinterpret_cast<uint16_t *>(ws + 8 * K);
  c.shift = ws + 8 * K + align8(2 * M);
  c.K = K;
  c.Mh = M;
  c.A = A;
  c.rpad = rpad;
  c.lane = lane;
  c.invK = 1.0 / (double)K;
  c.bits = allele_bits(A);
  c.amask = (1u << c.bits) - 1u;
  for (int j = 0; j < M; j++) {
    c.hetrow[j] = (uint16_t)(j * A);
    c.shift[j] = (uint8_t)(c.bits * (M - 1 - j));
  }
  __syncthreads();
  const int nw = blockDim.x / WAVE;
  for (int g = blockIdx.x * nw + wave; g < n_genotypes; g += gridDim.x * nw) {
    const int8_t *gt = genotypes + (size_t)g * K * M;
    for (int h = 0; h < K; h++) {
      uint64_t x = 0;
      for (int j = 0; j < M; j++) x |= (uint64_t)(uint8_t)gt[h * M + j] << c.shift[j];
      c.pw[h] = x;
    }
    const double llk = eval_llk<RPL>(c, c.pw, cnt);
    if (lane == 0) out[g] = llk;
  }
}

}  // namespace mchap
