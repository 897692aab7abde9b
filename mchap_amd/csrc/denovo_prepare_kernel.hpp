// The prepare pass of the de novo samplers behind kernel 1 (gfx950), one workgroup per unit: the homozygous fix, the read tensor
// transposed to [M0*A][RPAD] with NaN -> 1 in the workspace (and, for the speculative sampler, as uint8 codes into a per-unit
// dictionary), the initial-genotype distribution and the prior tables -- what SimtParams and the META_* constants of
// denovo_common.hpp describe.  Every sampler of the pipeline reads its output: denovo_simt_kernel, denovo_spec_kernel and what
// builds on it.  Reference citations as in denovo_mcmc_kernel.hpp.
#pragma once
#include "denovo_common.hpp"

namespace mchap {

// ---------------------------------------------------------------------------------------------------------
// prepare: grid = units, block = 64
// ---------------------------------------------------------------------------------------------------------
#ifndef MCHAP_PREP_WPE
#define MCHAP_PREP_WPE 4  // waves per SIMD the prepare pass is compiled for (it is latency-bound: one wave per unit)
#endif
template <int RPL>
__global__ __launch_bounds__(64, MCHAP_PREP_WPE) void denovo_prepare_kernel(const SimtParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const DenovoParams &D = P.d;
  const int u = blockIdx.x;
  const mchap_unit U = D.units[u];
  const int lane = threadIdx.x;
  const int R = U.n_reads, M0 = U.n_pos, A = U.max_allele, K = U.ploidy;
  const int rpad = D.rpad;
  const int MA = M0 * A;
  double *rt = P.rt + (size_t)u * P.max_ma * rpad;
  // [MA][rpad] copy for the homozygous fix: in LDS when it fits, else the global table itself (every lane only
  // re-reads the reads r = lane + 64 i it stored, so program order makes its own stores visible)
  const bool in_lds = !(P.flags & SIMT_FLAG_PREP_GLOBAL);
  double *rl = in_lds ? reinterpret_cast<double *>(smem) : rt;
  double *lp = reinterpret_cast<double *>(smem) + (in_lds ? (size_t)MA * rpad : 0);  // snv posterior scratch
  const double *gr = D.reads ? D.reads + U.reads_off : nullptr;
  const int8_t *nal0 = D.n_alleles + U.nalleles_off;
  // entry (r, q = j * A + a) of the unit's probability tensor: read from it, or formed from the allele calls as
  // encoding/integer/transcode.py:16-77 does (called allele p, the others (1 - p) / 3, NaN for a gap, then 0 for
  // alleles the position does not have)
  auto rawv = [&](int r, int q) -> double {
    if (gr) return gr[(size_t)r * MA + q];
    const int j = q / A, a = q - j * A;
    if (a >= nal0[j]) return 0.0;
    const size_t e = (size_t)U.reads_off + (size_t)r * M0 + j;
    const int call = D.calls[e];
    if (call < 0) return NAN;
    int qi = D.quals ? (int)D.quals[e] : 0;
    qi = qi < 0 ? 0 : (qi >= D.qual_prob_len ? D.qual_prob_len - 1 : qi);
    const double pc = D.qual_prob[qi];
    return a == call ? pc : (1.0 - pc) / 3.0;
  };
  double *cw = P.cntw + (size_t)u * rpad;
  int32_t *mi = P.meta_i + (size_t)u * meta_i_stride(P.max_pos);
  double *mf = P.meta_f + (size_t)u * meta_f_stride(P.max_ploidy, P.max_pos, P.max_allele);

  bool all_gaps = true;  // every factor a likelihood can read is 1.0
  for (int r = lane; r < rpad; r += WAVE) {
    // eight entries of the read's row at a time: the loads are independent and issued together (the stores that
    // follow could alias them as far as the compiler knows)
    for (int q0 = 0; q0 < MA; q0 += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = (r < R && q0 + k < MA) ? rawv(r, q0 + k) : 1.0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int q = q0 + k;
        if (q < MA) {
          const double x = isnan(v[k]) ? 1.0 : v[k];
          if (in_lds) rl[(size_t)q * rpad + r] = x;
          rt[(size_t)q * rpad + r] = x;
          if (q % A < (int)nal0[q / A]) all_gaps = all_gaps && (x == 1.0);
        }
      }
    }
  }
  {
    const bool flat = __ballot(!all_gaps) == 0ull;
    if (lane == 0) mi[META_I_FLAT] = flat ? 1 : 0;
  }
  double cnt[RPL];
#pragma unroll
  for (int i = 0; i < RPL; i++) {
    const int r = lane + WAVE * i;
    cnt[i] = (r < R) ? (U.counts_off >= 0 ? (double)D.counts[U.counts_off + r] : 1.0) : 0.0;
    cw[r] = cnt[i];
  }
  {
    bool w01 = true;
#pragma unroll
    for (int i = 0; i < RPL; i++) w01 = w01 && (cnt[i] == 0.0 || cnt[i] == 1.0);
    const bool all01 = __ballot(!w01) == 0ull;
    if (lane == 0) mi[META_I_W01] = (all01 && !(P.flags & (1 << 20))) ? 1 : 0;
  }
  __syncthreads();
  // ---- dictionary + coded table ----
  {
    unsigned long long *hkeys = reinterpret_cast<unsigned long long *>(lp + P.max_ugens_pad);  // [DICT_HASH]
    uint16_t *hcode = reinterpret_cast<uint16_t *>(hkeys + DICT_HASH);                         // [DICT_HASH]
    int *ndist = reinterpret_cast<int *>(hcode + DICT_HASH);
    const unsigned long long EMPTY = ~0ull;  // a NaN pattern: table entries are never NaN
    for (int i = lane; i < DICT_HASH; i += WAVE) hkeys[i] = EMPTY;
    if (lane == 0) *ndist = 0;
    __syncthreads();
    const int RPLT = rpad / WAVE;
    for (int q = 0; q < MA; q++) {
      // the lane's RPL values of this row: loaded together (one memory round trip per row, not one per value)
      for (int i0 = 0; i0 < RPL; i0 += 4) {
      unsigned long long keys[4];
#pragma unroll
      for (int k = 0; k < 4; k++) keys[k] = (unsigned long long)__double_as_longlong(rt[(size_t)q * rpad + lane + WAVE * min(i0 + k, RPL - 1)]);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (i0 + k >= RPL) break;
        const unsigned long long key = keys[k];
        unsigned slot = (unsigned)(mix64(key) & (DICT_HASH - 1));
        while (*(volatile int *)ndist <= DICT_MAX) {
          // plain read first: most entries repeat a value that is already in the set (same-address LDS atomics of a
          // whole wavefront serialise)
          unsigned long long old = *(volatile unsigned long long *)&hkeys[slot];
          if (old == EMPTY) {
            old = atomicCAS(&hkeys[slot], EMPTY, key);
            if (old == EMPTY) atomicAdd(ndist, 1);
          }
          if (old == EMPTY || old == key) break;
          slot = (slot + 1) & (DICT_HASH - 1);
        }
      }
      }
    }
    __syncthreads();
    const int nd = *ndist;
    uint8_t *ct = P.codes + (size_t)u * P.max_ma * WAVE * P.cstride;
    double *dict = P.dict + (size_t)u * DICT_MAX;
    if (nd <= DICT_MAX) {
      int base = 0;
      for (int s0 = 0; s0 < DICT_HASH; s0 += WAVE) {
        const unsigned long long key = hkeys[s0 + lane];
        const bool occ = key != EMPTY;
        const unsigned long long m = __ballot(occ);
        const int code = base + __popcll(m & ((1ull << lane) - 1ull));
        if (occ) {
          hcode[s0 + lane] = (uint16_t)code;
          dict[code] = __longlong_as_double((long long)key);
        }
        base += __popcll(m);
      }
      __syncthreads();
      for (int q = 0; q < MA; q++) {
        for (int i0 = 0; i0 < RPL; i0 += 4) {
          unsigned long long keys[4];
#pragma unroll
          for (int k = 0; k < 4; k++) keys[k] = (unsigned long long)__double_as_longlong(rt[(size_t)q * rpad + lane + WAVE * min(i0 + k, RPL - 1)]);
          uint32_t packed = 0;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            if (i0 + k >= RPL) break;
            const unsigned long long key = keys[k];
            unsigned slot = (unsigned)(mix64(key) & (DICT_HASH - 1));
            while (hkeys[slot] != key) slot = (slot + 1) & (DICT_HASH - 1);
            if (RPL > 2) packed |= (uint32_t)(uint8_t)hcode[slot] << (8 * k);
            else ct[((size_t)q * WAVE + lane) * P.cstride + i0 + k] = (uint8_t)hcode[slot];
          }
          // (cstride is a multiple of 4 beyond two chunks: one aligned 4-byte store instead of four byte stores;
          // bytes past the unit's chunks are padding the sampler never reads)
          if (RPL > 2) *reinterpret_cast<uint32_t *>(ct + ((size_t)q * WAVE + lane) * P.cstride + i0) = packed;
        }
      }
    }
    if (lane == 0) mi[META_I_NDICT] = nd <= DICT_MAX ? nd : 0;
  }
  const int8_t *nalleles = D.n_alleles + U.nalleles_off;
  // homozygous fix (assemble/mcmc.py:168-182, 494-541; snpcalling.py:14-70)
  int Mh = 0;
  double luh = 0.0;
  const bool pow2_ploidy = (K & (K - 1)) == 0;
  const double inv_ploidy = 1.0 / (double)K;
  // The SNV prior (snv_log_prior: calling/prior.py:116-179 with flat frequencies) needs lgamma(dose + 1) and, with
  // inbreeding, lgamma(dose + alpha_n), lgamma(alpha_n) and the normaliser for every allele count n: a few dozen
  // distinct values per unit.  Every lane used to recompute K + 1 of them per genotype (200 calls of ~400
  // instructions per unit: 60 % of this pass); now each value is formed once, one per lane.
  constexpr int KP = MCHAP_MAX_PLOIDY_DENOVO;  // (the prepare pass serves every sampler: ploidies up to 15, packs of sixteen nibbles)
  __shared__ double s_lg1[KP + 1];                              // lgamma(d + 1)
  __shared__ double s_lga[(MCHAP_MAX_ALLELE + 1) * (KP + 1)];   // lgamma(d + alpha_n), d >= 1
  __shared__ double s_lgb[MCHAP_MAX_ALLELE + 1], s_left[MCHAP_MAX_ALLELE + 1];  // lgamma(alpha_n); normaliser
  const double Fp = U.inbreeding;
  const bool with_prior = !isnan(Fp);
  if (with_prior) {
    for (int d = lane; d <= K; d += WAVE) s_lg1[d] = lgamma((double)d + 1.0);
    if (Fp != 0.0) {
      for (int e = lane; e < (A + 1) * (K + 1); e += WAVE) {
        const int n = e / (K + 1), d = e % (K + 1);
        if (n >= 1 && d >= 1) s_lga[n * (KP + 1) + d] = lgamma((double)d + (1.0 / (double)n) * ((1.0 - Fp) / Fp));
      }
      for (int n = 1 + lane; n <= A; n += WAVE) {
        const double alpha = (1.0 / (double)n) * ((1.0 - Fp) / Fp);
        const double sum_alphas = alpha * (double)n;
        s_lgb[n] = lgamma(alpha);
        s_left[n] = (lgamma((double)K + 1.0) + lgamma(sum_alphas)) - lgamma((double)K + sum_alphas);
      }
    }
    __syncthreads();
  }
  // snv_log_prior(g, K, n, F) from the tables: same arguments to the same lgamma, same order of the sums
  auto snv_prior = [&](uint64_t g, int n) -> double {
    int dose[KP];
    for (int i = 0; i < K; i++) dose[i] = 0;
    for (int i = 0; i < K; i++) {
      int j = 0;
      while (nib(g, i) != nib(g, j)) j++;
      dose[j] += 1;
    }
    if (Fp == 0.0) {
      double den = 0.0;
      for (int i = 0; i < K; i++) den += s_lg1[dose[i]];
      return (s_lg1[K] - den) - (double)K * c_ln[n];
    }
    double prod = 0.0;
    for (int i = 0; i < K; i++)
      if (dose[i] > 0) prod += s_lga[n * (KP + 1) + dose[i]] - (s_lg1[dose[i]] + s_lgb[n]);
    return s_left[n] + prod;
  };
  // without the LDS copy of the whole table, the A rows of the current position are staged in LDS (each lane its own
  // reads): the genotype loop below re-reads them K times per genotype
  double *pl = reinterpret_cast<double *>(smem + P.prep_rows_off);  // [A][rpad]
  for (int j = 0; j < M0; j++) {
    const int n = nalleles[j];
    const int u_gens = snv_genotypes(n, K);
    const double *rowp = rl + (size_t)(j * A) * rpad;
    if (!in_lds) {
      for (int a = 0; a < A; a++)
#pragma unroll
        for (int i = 0; i < RPL; i++) pl[(size_t)a * rpad + lane + WAVE * i] = rt[(size_t)(j * A + a) * rpad + lane + WAVE * i];
      rowp = pl;
    }
    uint64_t g = 0;  // the SNV genotype's alleles, one nibble each
    for (int q = 0; q < u_gens; q++) {
      double lprior = 0.0;
      if (with_prior) lprior = snv_prior(g, n);
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < RPL; i++) {
        double rp = 0.0;
        // x / K (snpcalling.py / likelihood.py:61); for K = 2, 4, 8 the product with 1 / K is the same double
        if (pow2_ploidy) {
          for (int h = 0; h < K; h++) rp += rowp[(size_t)nib(g, h) * rpad + lane + WAVE * i] * inv_ploidy;
        } else {
          for (int h = 0; h < K; h++) rp += rowp[(size_t)nib(g, h) * rpad + lane + WAVE * i] / (double)K;
        }
        s += read_log(rp) * cnt[i];
      }
      const double llk = wave_sum(s);
      lp[q] = lprior + llk;
      g = increment_snv_genotype(g, K);
    }
    double acc = lp[0];
    for (int q = 1; q < u_gens; q++) acc = add_log_prob(acc, lp[q]);
    int fixed_allele = -1;
    for (int a = 0; a < n; a++) {
      int idx = 0;
      for (int i = 0; i < K; i++) idx += (a == 0) ? 0 : snv_genotypes(a, i + 1);
      if (exp(lp[idx] - acc) >= D.fix_hom) fixed_allele = a;
    }
    if (lane == 0) D.fixed[U.fixed_off + j] = (int8_t)fixed_allele;
    if (fixed_allele < 0) {
      if (lane == 0) {
        mi[META_I_COLS + Mh] = j * A;
        mi[META_I_COLS + P.max_pos + Mh] = n;
      }
      luh += c_ln[n];  // assemble/mcmc.py:294
      Mh++;
    }
  }
  const int bits = allele_bits(A);
  int status = MCHAP_UNIT_OK;
  if (Mh == 0) status = MCHAP_UNIT_ALL_FIXED;
  else if (Mh * bits > (P.word_bits ? P.word_bits : 64)) status = MCHAP_ERR_LIMIT;
  else if (U.initial_off >= 0 && U.initial_n_het != Mh) status = MCHAP_UNIT_BAD_INITIAL;  // assemble/mcmc.py:207
  if (lane == 0) {
    mi[META_I_MH] = Mh;
    mi[META_I_STATUS] = status;
    D.status[u] = status;
    mf[0] = luh;
  }
  if (status != MCHAP_UNIT_OK) {
    if (status == MCHAP_UNIT_ALL_FIXED) {
      // assemble/mcmc.py:189-199: constant trace, NaN llks
      const size_t tb = U.trace_off, lb = U.llk_off;
      const int S = D.steps, C_ = D.chains;
      for (int i = lane; i < C_ * S * K; i += WAVE) D.trace[tb + i] = 0ull;
      for (int i = lane; i < C_ * S; i += WAVE) D.llks[lb + i] = NAN;
    }
    return;
  }
  // prior tables (assemble/prior.py:39-112), same layout as Chain::prior_tab
  if (!isnan(U.inbreeding) && lane == 0) {
    double *t = mf + meta_f_prior(0);
    const double F = U.inbreeding;
    for (int d = 0; d <= K; d++) t[K + 1 + d] = lgamma((double)d + 1.0);
    t[2 * K + 3] = lgamma((double)K + 1.0);
    t[2 * K + 4] = (double)K * luh;
    if (F != 0.0) {
      const double log_disp = log((1.0 - F) / F) - luh;
      const double disp = exp(log_disp);
      const double sum_disp = exp(log_disp + luh);
      const double lg_disp = lgamma(disp);
      t[0] = 0.0;
      for (int d = 1; d <= K; d++) t[d] = lgamma((double)d + disp) - (lgamma((double)d + 1.0) + lg_disp);
      t[2 * K + 2] = (lgamma((double)K + 1.0) + lgamma(sum_disp)) - lgamma((double)K + sum_disp);
    }
  }
  // _read_mean_dist (assemble/mcmc.py:455-491) over the sampled positions, from the raw tensor
  if (U.initial_off < 0) {
    double *dist = mf + meta_f_dist(P.max_ploidy);
    __syncthreads();
    for (int jj = 0; jj < Mh; jj++) {
      const int col = mi[META_I_COLS + jj];
      int n_nonzero = 0;
      uint32_t gapmask = 0;
      double dv[MCHAP_MAX_ALLELE];
      for (int a = 0; a < A; a++) {
        double tot = 0.0;
        int n_ok = 0, n_nz = 0;
        for (int i0 = 0; i0 < RPL; i0 += 4) {  // four of the lane's reads at a time: their loads are independent
          double v4[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int r = lane + WAVE * (i0 + k);
            v4[k] = (i0 + k < RPL && r < R) ? rawv(r, col + a) : 0.0;
          }
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int r = lane + WAVE * (i0 + k);
            if (i0 + k < RPL && r < R) {
              const double v = v4[k];
              if (!isnan(v)) {
                tot += v;
                n_ok++;
              }
              if (!(v == 0.0)) n_nz++;
            }
          }
        }
        tot = wave_sum(tot);
        n_ok = wave_sum_i(n_ok);
        n_nz = wave_sum_i(n_nz);
        if (n_ok == 0) {
          gapmask |= 1u << a;
          dv[a] = 1.0;
          n_nonzero++;
        } else {
          dv[a] = tot / (double)n_ok;
          if (n_nz > 0) n_nonzero++;
        }
      }
      for (int a = 0; a < A; a++)
        if (gapmask & (1u << a)) dv[a] = 1.0 / (double)n_nonzero;
      double s = 0.0;
      for (int a = 1; a < A; a++) s += dv[a];
      s = (A > 1) ? dv[0] + s : dv[0];
      if (lane == 0)
        for (int a = 0; a < A; a++) dist[jj * A + a] = dv[a] / s;
    }
  }
}
}  // namespace mchap
