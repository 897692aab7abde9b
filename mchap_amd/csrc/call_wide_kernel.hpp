// `mchap call` over MANY known haplotypes (more than CALL_MAX_HAPS = 256): the sampler of call_mcmc_kernel.hpp with the
// transposed work split -- the options of a sub-step over the lanes, every lane its own likelihood -- for MI355X (gfx950).
// Reference: calling/mcmc.py:15-453, calling/classes.py:62-124, calling/likelihood.py:8-78, calling/prior.py:30-179.
//
// call_mcmc_kernel was built for few haplotypes: its product table sits in LDS (or per CHAIN in the workspace), a missed
// option is evaluated by the whole wavefront, lanes over reads, at the price of one butterfly reduction per option -- H of them
// in a chain's first sub-step --, and its Gibbs memo and coast hand-over pack alleles eight bits each.  Here:
//   * the unit's tables -- products P[r][h], read weights, prior tables -- are built ONCE PER UNIT in the workspace by
//     call_wide_setup_kernel (the arithmetic of exact_setup), row r holding H consecutive doubles: the lanes of a round read
//     consecutive haplotypes of one read (coalesced), the genotype's other alleles are one address for the whole wavefront;
//   * a sub-step's H options go over the lanes in rounds of 64: each lane forms its proposal's key (rank of the sorted alleles),
//     probes the chain's never-evicting table of remembered likelihoods, and on a miss evaluates its OWN option -- the reads one
//     after the other, the K table entries of a read added in the genotype's array order with the proposed allele in its slot:
//     the order of calling/likelihood.py:8-34, no cross-lane reduction;
//   * priors, normalisation and the categorical draw are the reference's sequential arithmetic on one lane, the Philox draws are
//     consumed exactly as in call_mcmc_kernel.  That chain of H - 1 dependent add_log_prob dominates a sub-step; parallelising it
//     would change bits;
//   * no Gibbs memo, no coast hand-over (ploidies 9 to 15 run without them on the other path too).
// A workgroup is up to CALL_WG_CHAINS wavefronts, the chains of one unit; a chain's four option arrays [H] live in LDS, which
// bounds H (call_wide_max_haps) and the chains per workgroup.  The wavefronts of a workgroup never meet at a barrier.
#pragma once
#include "call_mcmc_kernel.hpp"

namespace mchap {

// 4 arrays [H] of doubles for one chain within 160 KB of LDS, less the kernel's static part: H <= 4096 -> 128 KB
constexpr int CALL_WIDE_MAX_HAPS = 4096;
constexpr size_t CALL_WIDE_LDS = 160 * 1024 - 1024;  // dynamic LDS a workgroup may ask for

// doubles of a unit's tables in the workspace: ptab [R][H], cnt [R], lgd [H][K+1], lgf [K+1], lfreq [H], rtab [H][K],
// {left, gibbs_left} -- a multiple of 32 (256 bytes)
__host__ __device__ inline size_t call_wide_unit_doubles(int R, int H, int K) {
  const size_t n = (size_t)R * H + R + (size_t)H * (K + 1) + (K + 1) + H + (size_t)H * K + 2;
  return (n + 31) & ~(size_t)31;
}
__host__ __device__ inline size_t call_wide_lds_bytes(int H, int wg_chains) { return (size_t)wg_chains * 4 * (size_t)H * 8; }

struct CallWideParams {
  CallParams c;        // (cache, cache_slots, shapes, inputs and outputs as call_mcmc_kernel; ptab_ext, state, phase, last unused)
  double *unit_tab;    // [U][unit_doubles]
  size_t unit_doubles;
};

struct CallWideTab {
  const double *ptab, *cnt, *lgd, *lgf, *lfreq, *rtab, *scal;
};
__device__ __forceinline__ CallWideTab call_wide_tab(double *base, int R, int H, int K) {
  CallWideTab t;
  t.ptab = base;
  t.cnt = t.ptab + (size_t)R * H;
  t.lgd = t.cnt + R;
  t.lgf = t.lgd + (size_t)H * (K + 1);
  t.lfreq = t.lgf + (K + 1);
  t.rtab = t.lfreq + H;
  t.scal = t.rtab + (size_t)H * K;
  return t;
}

// The unit's tables: grid (blocks, U); P[r][h] over all blocks, the small tables by block 0.  The arithmetic of exact_setup
// (exact_kernel.hpp) and of call_mcmc_kernel's Gibbs tables, value by value.
constexpr int CALL_WIDE_SETUP_THREADS = 256;
__global__ __launch_bounds__(CALL_WIDE_SETUP_THREADS) void call_wide_setup_kernel(const CallWideParams W) {
  const CallParams &P = W.c;
  const int unit = blockIdx.y;
  const int R = P.R, M = P.M, A = P.A, H = P.H, K = P.K;
  double *base = W.unit_tab + (size_t)unit * W.unit_doubles;
  double *ptab = base, *cnt = ptab + (size_t)R * H, *lgd = cnt + R, *lgf = lgd + (size_t)H * (K + 1), *lfreq = lgf + (K + 1);
  double *rtab = lfreq + H, *scal = rtab + (size_t)H * K;
  const double *reads = P.reads + (size_t)unit * R * M * A;
  const int8_t *haps = P.haps + (size_t)unit * H * M;
  const long long n = (long long)R * H;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(q / H), h = (int)(q % H);
    double prod = 1.0;
    for (int j = 0; j < M; j++) {
      const double v = reads[((size_t)r * M + j) * A + haps[(size_t)h * M + j]];
      if (!isnan(v)) prod *= v;  // assemble/likelihood.py:54-59
    }
    ptab[q] = prod;
  }
  if (blockIdx.x != 0) return;
  const int nt = (int)blockDim.x, t = (int)threadIdx.x;
  for (int r = t; r < R; r += nt) cnt[r] = P.counts ? (double)P.counts[(size_t)unit * R + r] : 1.0;
  const bool has_prior = P.has_prior != 0;
  const bool has_freqs = has_prior && P.freqs != nullptr;
  if (!has_prior) {
    if (t == 0) scal[0] = scal[1] = 0.0;
    return;
  }
  const double F = P.inbreeding[unit];
  const double scale = (1.0 - F) / F;
  for (int q = t; q < H * (K + 1); q += nt) {
    const int h = q / (K + 1), d = q % (K + 1);
    const double alpha = has_freqs ? P.freqs[(size_t)unit * H + h] * scale : (1.0 / (double)H) * scale;
    lgd[q] = (F == 0.0 || d == 0) ? 0.0 : lgamma((double)d + alpha) - (lgamma((double)d + 1.0) + lgamma(alpha));
  }
  for (int d = t; d <= K; d += nt) lgf[d] = lgamma((double)d + 1.0);
  for (int h = t; h < H; h += nt) lfreq[h] = has_freqs ? P.freqs[(size_t)unit * H + h] : 0.0;
  if (F != 0.0) {
    for (int q = t; q < H * K; q += nt) {
      const int a = q / K, ibs = q % K;
      const double alpha = has_freqs ? P.freqs[(size_t)unit * H + a] * scale : (1.0 / (double)H) * scale;
      const double va = alpha + (double)ibs;
      rtab[q] = lgamma(1.0 + va) - lgamma(va);
    }
  }
  if (t == 0) {
    double s;
    if (has_freqs) {
      s = 0.0;
      for (int h = 0; h < H; h++) s += P.freqs[(size_t)unit * H + h] * scale;
    } else {
      s = ((1.0 / (double)H) * scale) * (double)H;
    }
    scal[0] = (F == 0.0) ? 0.0 : (lgamma((double)K + 1.0) + lgamma(s)) - lgamma((double)K + s);  // genotype prior (exact_setup)
    const double sum_alpha = (double)(K - 1) + s;                                                   // Gibbs prior (call_mcmc_kernel)
    scal[1] = (F == 0.0) ? 0.0 : lgamma(sum_alpha) - lgamma(1.0 + sum_alpha);
  }
}

// (the keys of the likelihood table: call_wide_key -> call_rank, call_mcmc_kernel.hpp)
template <int KM = 8>
__global__ __launch_bounds__(64 * CALL_WG_CHAINS) void call_wide_kernel(const CallWideParams W) {
  extern __shared__ __align__(16) unsigned char smem[];
  const CallParams &P = W.c;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nwv = (int)(blockDim.x >> 6);
  const int unit = blockIdx.y, chain = (int)blockIdx.x * nwv + wv;
  const int lane = (int)(threadIdx.x & 63);
  const int R = P.R, H = P.H, K = P.K;
  if (chain >= P.chains) return;  // (no workgroup-wide barrier anywhere below)
  const CallWideTab T = call_wide_tab(W.unit_tab + (size_t)unit * W.unit_doubles, R, H, K);
  typedef __attribute__((address_space(3))) double lds_f64;
  typedef __attribute__((address_space(3))) int lds_i32;
  lds_f64 *o_llk = (lds_f64 *)(reinterpret_cast<double *>(smem) + (size_t)wv * 4 * H);  // [H] each: this chain's
  lds_f64 *o_lpr = o_llk + H, *o_prob = o_lpr + H, *o_aux = o_prob + H;
  __shared__ double s_acc_[CALL_WG_CHAINS], s_choice_llk_[CALL_WG_CHAINS];
  __shared__ int s_g_[CALL_WG_CHAINS][KM];  // the chain's genotype (array order)
  __shared__ int s_choice_[CALL_WG_CHAINS], s_full_[CALL_WG_CHAINS];
  lds_f64 &s_acc = *(lds_f64 *)&s_acc_[wv], &s_choice_llk = *(lds_f64 *)&s_choice_llk_[wv];
  lds_i32 *s_g = (lds_i32 *)s_g_[wv];
  lds_i32 &s_choice = *(lds_i32 *)&s_choice_[wv], &s_full = *(lds_i32 *)&s_full_[wv];
  const bool has_prior = P.has_prior != 0;
  const bool has_freqs = has_prior && P.freqs != nullptr;
  const double F = has_prior ? P.inbreeding[unit] : 0.0;
  PriorTab pt;
  pt.lgd = T.lgd;
  pt.lgf = T.lgf;
  pt.lfreq = T.lfreq;
  pt.left = has_prior ? T.scal[0] : 0.0;
  pt.lnH = log((double)H);
  pt.F = F;
  pt.has_freqs = has_freqs ? 1 : 0;
  const double gibbs_left = T.scal[1];
  if (lane == 0) s_full = 0;
  call_sync();
  ulonglong2 *cache = P.cache + ((size_t)unit * P.chains + chain) * (size_t)P.cache_slots;
  const unsigned long long cmask = (unsigned long long)P.cache_slots - 1ull;

  // The lane's own likelihood of the genotype s_g[0 .. kk - 1] with allele `a` in slot `k` (k < 0: as it stands): the reads in
  // order, a read's kk table entries added in array order (calling/likelihood.py:8-34 -> assemble/likelihood.py:17-70)
  auto lane_llk = [&](int kk, int k, int a) -> double {
    const double invk = 1.0 / (double)kk;
    int go[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) go[i] = i < kk ? __builtin_amdgcn_readfirstlane((int)s_g[i]) : 0;  // (one address for the wavefront)
    double s = 0.0;
    const double *row = T.ptab;
    for (int r = 0; r < R; r++, row += H) {
      const double mine = row[a];
      double rp = 0.0;
#pragma unroll
      for (int i = 0; i < KM; i++)
        if (i < kk) rp += (i == k ? mine : row[go[i]]) * invk;
      s += read_log(rp) * T.cnt[r];
    }
    return s;
  };

  // ---- initial genotype: the caller's, or greedy_caller (calling/mcmc.py:393-453), the alleles of a position over the lanes ----
  if (P.initial) {
    if (lane < K) s_g[lane] = (int)P.initial[(size_t)unit * K + lane];
    call_sync();
  } else {
    const double scale = (1.0 - F) / F;
    double sum_alphas = 0.0;
    if (has_prior && F != 0.0) {
      if (has_freqs) {
        for (int h = 0; h < H; h++) sum_alphas += P.freqs[(size_t)unit * H + h] * scale;
      } else {
        sum_alphas = ((1.0 / (double)H) * scale) * (double)H;
      }
    }
    for (int i = 0; i < K; i++) {
      const int kk = i + 1;
      for (int a0 = 0; a0 < H; a0 += WAVE) {
        const int a = a0 + lane;
        const bool act = a < H;
        const double llk = lane_llk(kk, i, act ? a : 0);
        double lprior = 0.0;
        if (has_prior) {
          // the prior of a genotype of ploidy i + 1: its tables depend on the ploidy (left term, lgamma(ploidy + 1))
          int g[KM];
          for (int q = 0; q < i; q++) g[q] = s_g[q];
          g[i] = act ? a : 0;
          if (F == 0.0) {
            double den = 0.0;
            for (int x = 0; x < kk; x++) {
              bool first = true;
              int dose = 0;
              for (int y = 0; y < kk; y++)
                if (g[y] == g[x]) {
                  dose++;
                  if (y < x) first = false;
                }
              den += first ? lgamma((double)dose + 1.0) : 0.0;
            }
            const double ln_perms = lgamma((double)kk + 1.0) - den;
            if (!has_freqs) lprior = ln_perms - (double)kk * pt.lnH;
            else {
              double prod = 1.0;
              for (int q = 0; q < kk; q++) prod *= T.lfreq[g[q]];
              lprior = ln_perms + log(prod);
            }
          } else {
            const double left = (lgamma((double)kk + 1.0) + lgamma(sum_alphas)) - lgamma((double)kk + sum_alphas);
            double prod = 0.0;
            for (int x = 0; x < kk; x++) {
              bool first = true;
              int dose = 0;
              for (int y = 0; y < kk; y++)
                if (g[y] == g[x]) {
                  dose++;
                  if (y < x) first = false;
                }
              if (first) {
                const double alpha = has_freqs ? P.freqs[(size_t)unit * H + g[x]] * scale : (1.0 / (double)H) * scale;
                prod += lgamma((double)dose + alpha) - (lgamma((double)dose + 1.0) + lgamma(alpha));
              }
            }
            lprior = left + prod;
          }
        }
        if (act) o_llk[a] = llk + lprior;
      }
      call_sync();
      if (lane == 0) {  // the first maximum in allele order (strict >)
        double best = -INFINITY;
        int best_a = -1;
        for (int a = 0; a < H; a++) {
          const double v = o_llk[a];
          if (v > best) {
            best = v;
            best_a = a;
          }
        }
        s_g[i] = best_a;
      }
      call_sync();
    }
    if (lane == 0) {  // genotype.sort()
      for (int a = 1; a < K; a++) {
        const int v = s_g[a];
        int b = a - 1;
        while (b >= 0 && s_g[b] > v) {
          s_g[b + 1] = s_g[b];
          b--;
        }
        s_g[b + 1] = v;
      }
    }
    call_sync();
  }

  CallStream st;
  st.k0 = (uint32_t)P.seed;
  st.k1 = (uint32_t)(P.seed >> 32) ^ (uint32_t)(P.stream_ids[unit] >> 32);
  st.c2 = ((uint32_t)chain << 16) | SLOT_CALL;
  st.c3 = (uint32_t)P.stream_ids[unit];
  uint64_t ctr = 0;  // (K - 1 shuffle draws and K uniforms per step)
  int64_t *gout = P.genotypes + (((size_t)unit * P.chains + chain) * P.steps) * K;
  double *lout = P.llks + ((size_t)unit * P.chains + chain) * P.steps;

  // probe the chain's table for `key`: returns true and the value, or false and the slot to fill (null: the table is full)
  auto probe = [&](long long key, double &val, ulonglong2 *&slot) -> bool {
    unsigned long long h = (unsigned long long)key * 0x9E3779B97F4A7C15ull;
    unsigned long long i = (h >> 20) & cmask;
    for (long long tries = 0; tries < P.cache_slots; tries++) {
      ulonglong2 e = cache[i];
      if (e.x == (unsigned long long)key + 1ull) {
        val = __longlong_as_double((long long)e.y);
        return true;
      }
      if (e.x == 0ull) {
        slot = cache + i;
        return false;
      }
      i = (i + 1) & cmask;
    }
    slot = nullptr;
    return false;
  };

  // llks of the options a0 .. a0 + 63 of a sub-step at position k, into o_llk
  auto option_llks = [&](int k, int a0) {
    const int a = a0 + lane;
    const bool act = a < H;
    double val = 0.0;
    ulonglong2 *slot = nullptr;
    bool miss = false;
    long long key = -1;
    if (act) {
      int g[KM];
      for (int i = 0; i < K; i++) g[i] = s_g[i];
      g[k] = a;
      key = call_wide_key<KM>(g, K);
      miss = !probe(key, val, slot);
      if (miss && !slot) s_full = 1;
    }
    const unsigned long long missed = __ballot(miss);
    if (!missed) {
      if (act) o_llk[a] = val;
      return;
    }
    // Two missing lanes of a round whose proposals sort to the same genotype: the lower option is the one the sequential reference
    // evaluates and remembers, the other takes its value.  (The options of one sub-step differ in the allele at k alone, so their
    // sorted genotypes differ; the rule is kept for whatever proposal scheme comes later, and costs a compare per missing lane.)
    int dup_of = -1;
    for (unsigned long long todo = missed; todo; todo &= todo - 1) {
      const int src = __ffsll((long long)todo) - 1;
      const long long ks = __shfl(key, src, WAVE);
      if (miss && lane > src && dup_of < 0 && ks == key) dup_of = src;
    }
    const bool own = miss && dup_of < 0;
    if (own) val = lane_llk(K, k, a);
    const double from = __shfl(val, dup_of >= 0 ? dup_of : lane, WAVE);
    if (dup_of >= 0) val = from;
    // the lanes' new entries go into the table together: a lane claims the first empty slot of its probe sequence by compare-and-swap
    // on the key word, then stores the value (call_mcmc_kernel); nobody reads the table before the fence below.  The table never
    // forgets an entry: the first evaluated allele order's value stays (calling/likelihood.py:36-78).
    if (own && slot) {
      unsigned long long h = (unsigned long long)key * 0x9E3779B97F4A7C15ull;
      unsigned long long i = (h >> 20) & cmask;
      bool placed = false;
      for (long long tries = 0; tries < P.cache_slots && !placed; tries++) {
        const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&cache[i].x), 0ull, (unsigned long long)key + 1ull);
        if (old == 0ull) {
          cache[i].y = (unsigned long long)__double_as_longlong(val);
          placed = true;
        } else {
          i = (i + 1) & cmask;
        }
      }
      if (!placed) s_full = 1;
    }
    call_sync_global();  // (the next sub-step's probes read behind these entries)
    if (act) o_llk[a] = val;
  };

  for (int step = 0; step < P.steps; step++) {
    // np.random.shuffle(arange(ploidy)) -- every lane the same
    int order[KM];
    for (int i = 0; i < K; i++) order[i] = i;
    for (int i = K - 1; i >= 1; i--) {
      const int j = (int)call_interval(st, ctr++, (uint32_t)i);
      const int t = order[i];
      order[i] = order[j];
      order[j] = t;
    }
    for (int jj = 0; jj < K; jj++) {
      const int k = order[jj];
      const int current = s_g[k];
      double cur_llk = 0.0, cur_lprior = 0.0;
      int cur_copies = 1;
      if (P.step_type == 1) {
        // mh_options (calling/mcmc.py:15-140): likelihood and prior of the current genotype first
        int g[KM];
        for (int i = 0; i < K; i++) g[i] = s_g[i];
        cur_copies = 0;
        for (int i = 0; i < K; i++) cur_copies += g[i] == current ? 1 : 0;
        if (has_prior) cur_lprior = calling_log_prior_unsorted(pt, g, K);
        double val = 0.0;
        ulonglong2 *slot = nullptr;
        const long long key = call_wide_key<KM>(g, K);
        bool hit = false;
        if (lane == 0) {
          hit = probe(key, val, slot);
          if (!hit && !slot) s_full = 1;
        }
        hit = __shfl((int)hit, 0, WAVE) != 0;
        if (!hit) {
          val = lane_llk(K, -1, 0);  // (every lane the same sum)
          if (lane == 0 && slot) *slot = make_ulonglong2((unsigned long long)key + 1ull, (unsigned long long)__double_as_longlong(val));
          call_sync_global();
        }
        cur_llk = __shfl(val, 0, WAVE);
      }
      for (int a0 = 0; a0 < H; a0 += WAVE) option_llks(k, a0);
      // priors (and proposal ratios) of the options
      for (int a = lane; a < H; a += WAVE) {
        int g[KM];
        for (int i = 0; i < K; i++) g[i] = s_g[i];
        g[k] = a;
        int copies = 0;
        for (int i = 0; i < K; i++) copies += g[i] == a ? 1 : 0;
        if (P.step_type == 0) {
          double lp;
          if (!has_prior) lp = log((double)copies);  // log_genotype_allele_flat_prior (prior.py:30-52)
          else if (F == 0.0) lp = has_freqs ? log(T.lfreq[a]) : log(1.0 / (double)H);
          else lp = gibbs_left + T.rtab[(size_t)a * K + (copies - 1)];
          o_lpr[a] = lp;
        } else {
          if (a == current) {
            o_lpr[a] = cur_lprior;
            o_llk[a] = cur_llk;
            o_aux[a] = 0.0;
          } else {
            o_lpr[a] = has_prior ? calling_log_prior_unsorted(pt, g, K) : 0.0;
            o_aux[a] = log((double)copies / (double)cur_copies);
          }
        }
      }
      call_sync();
      if (P.step_type == 0) {
        // normalise_log_probs(llks + lpriors): sequential add_log_prob in allele order (jitutils.py:30-74) -- one lane --, then the H
        // exponentials, one lane each
        if (lane == 0) {
          double acc = o_llk[0] + o_lpr[0];
          for (int a = 1; a < H; a++) acc = add_log_prob(acc, o_llk[a] + o_lpr[a]);
          s_acc = acc;
        }
        call_sync();
        const double acc = s_acc;
        for (int a = lane; a < H; a += WAVE) o_prob[a] = exp((o_llk[a] + o_lpr[a]) - acc);
        call_sync();
      } else {
        if (lane == 0) {
          double sum = 0.0;
          for (int a = 0; a < H; a++) {
            const double r = ((o_llk[a] - cur_llk) + (o_lpr[a] - cur_lprior)) + o_aux[a];
            o_prob[a] = exp(fmin(0.0, r));
          }
          o_prob[current] = 0.0;
          for (int a = 0; a < H; a++) o_prob[a] /= (double)(H - 1);
          for (int a = 0; a < H; a++) sum += o_prob[a];
          o_prob[current] = 1.0 - sum;
        }
        call_sync();
      }
      // random_choice: searchsorted(cumsum(p), u, side="right") -- lane 0 walks the cumulative sum and stops at the choice
      if (lane == 0) {
        const double u = call_double(st, ctr);
        double cacc = 0.0;
        int ch = H;
        for (int a = 0; a < H; a++) {
          cacc += o_prob[a];
          if (cacc > u) {
            ch = a;
            break;
          }
        }
        if (ch >= H) ch = H - 1;  // u beyond the last cumulative value (probability ~1e-16)
        s_choice = ch;
        s_choice_llk = o_llk[ch];
        s_g[k] = ch;
      }
      ctr++;
      call_sync();
    }
    // genotype_alleles.sort(); the step's llk is that of the last choice
    if (lane == 0) {
      for (int a = 1; a < K; a++) {
        const int v = s_g[a];
        int b = a - 1;
        while (b >= 0 && s_g[b] > v) {
          s_g[b + 1] = s_g[b];
          b--;
        }
        s_g[b + 1] = v;
      }
      lout[step] = s_choice_llk;
    }
    call_sync();
    if (lane < K) gout[(size_t)step * K + lane] = s_g[lane];
    call_sync();
  }
  if (lane == 0 && s_full) atomicMin(&P.status[unit], MCHAP_ERR_LIMIT);
}

}  // namespace mchap
