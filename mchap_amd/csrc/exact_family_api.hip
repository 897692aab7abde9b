// libmchap_hip.so -- the parents and the progeny of one cross called jointly over stored likelihoods (exact_family_kernel.hpp): the
// tables of the two parent shapes, the accumulation of S over the progeny, the streaming pass for log Z_fam and the parents'
// marginals, the back projection for every progeny's marginal and predictive evidence.  Entry points declared in
// include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_family_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

int tiles_of(long long n, int per) { return (int)((n + per - 1) / per); }
bool ploidy_ok(int k) { return k >= 1 && k <= MCHAP_MAX_PLOIDY_DENOVO; }
bool parent_ok(int k) { return ploidy_ok(k) && k % 2 == 0; }

struct FamilyShape {
  int H = 0, KP = 0, KQ = 0, TP = 0, TQ = 0, WP = 0, WQ = 0;
  long long GP = 0, GQ = 0, GC = 0, NAP = 0, NAQ = 0;
  bool staged = false;
};

// the sub-multisets of a genotype: at most C(K, t), and no more than there are gametes
int row_width(int K, long long NA) {
  long long b = 1;
  for (int i = 1; i <= K / 2; i++) b = b * (K - K / 2 + i) / i;
  return (int)(b < NA ? b : NA);
}

// whether the shape is one the kernels take at all (the workspace apart): ploidies, genotype counts an int32 holds (the tables'
// indices), a row of blocks per launch
bool family_shape(int n_haps, int ploidy_p, int ploidy_q, int force_fallback, FamilyShape &s) {
  if (!parent_ok(ploidy_p) || !parent_ok(ploidy_q) || n_haps < 1) return false;
  s.H = n_haps; s.KP = ploidy_p; s.KQ = ploidy_q; s.TP = ploidy_p / 2; s.TQ = ploidy_q / 2;
  if (!cwr_fits(n_haps, ploidy_p) || !cwr_fits(n_haps, ploidy_q) || !cwr_fits(n_haps, s.TP + s.TQ)) return false;
  s.GP = host_cwr(n_haps, ploidy_p); s.GQ = host_cwr(n_haps, ploidy_q); s.GC = host_cwr(n_haps, s.TP + s.TQ);
  s.NAP = host_cwr(n_haps, s.TP); s.NAQ = host_cwr(n_haps, s.TQ);
  if (s.GP > 0x7fffffffll || s.GQ > 0x7fffffffll || s.GC > (1ll << 40)) return false;
  if (s.GP > (1ll << 62) / s.GQ / 8) return false;
  s.WP = row_width(ploidy_p, s.NAP); s.WQ = row_width(ploidy_q, s.NAQ);
  s.staged = !force_fallback && mchap::family_row_lds(s.NAQ, s.GQ, true) > 0;
  return true;
}

// carve of the workspace: the two parents' tables, then per record the small arrays, S, and -- where the rows of w / M_c are not
// staged -- a second [G_P][G_Q] array
struct FamilyCarve {
  size_t fcnt[2], fidx[2], fwt[2], bidx[2], bwt[2], mult[2], joint[2];
  size_t lmax, pair, dp, v, y, cy, rr, dsum, dtot, part, s, drow, bytes;
};
bool family_carve(int R, const FamilyShape &s, FamilyCarve &c) {
  const long long G[2] = {s.GP, s.GQ}, NA[2] = {s.NAP, s.NAQ};
  const int W[2] = {s.WP, s.WQ};
  // (every term below 2^62 / 8 by family_shape; their sum is checked in long double against 2^62)
  const long double total = (long double)R * ((long double)s.GP * s.GQ * 16 + (long double)(s.GP + s.NAP) * s.NAQ * 24) +
                            (long double)(s.GP * s.WP + s.GQ * s.WQ) * 12 + (long double)(s.NAP * s.NAP + s.NAQ * s.NAQ) * 12;
  if (total > 4.0e18L) return false;
  size_t o = 0;
  for (int u = 0; u < 2; u++) {
    c.fcnt[u] = o; o += up256((size_t)G[u] * 4);
    c.fidx[u] = o; o += up256((size_t)G[u] * W[u] * 4);
    c.fwt[u] = o; o += up256((size_t)G[u] * W[u] * 8);
    c.bidx[u] = o; o += up256((size_t)NA[u] * NA[u] * 4);
    c.bwt[u] = o; o += up256((size_t)NA[u] * NA[u] * 8);
    c.mult[u] = o; o += up256((size_t)R * NA[u] * 8);
    c.joint[u] = o; o += up256((size_t)R * G[u] * 8);
  }
  c.lmax = o; o += up256((size_t)R * 8);
  c.pair = o; o += up256((size_t)R * s.NAP * s.NAQ * 8);
  c.dp = o; o += up256((size_t)R * s.NAQ * 8);
  c.v = o; o += up256((size_t)R * s.GP * s.NAQ * 8);
  c.y = o; o += up256((size_t)R * s.GP * s.NAQ * 8);
  c.cy = o; o += up256((size_t)R * s.NAQ * 8);
  c.rr = o; o += up256((size_t)R * s.NAP * s.NAQ * 8);
  c.dsum = o; o += up256((size_t)R * s.GP * 8);
  c.dtot = o; o += up256((size_t)R * 8);
  c.part = o; o += up256((size_t)R * s.GP * 2 * 8);
  c.s = o; o += up256((size_t)R * s.GP * s.GQ * 8);
  c.drow = o; o += s.staged ? 0 : up256((size_t)R * s.GP * s.GQ * 8);
  c.bytes = o;
  return true;
}

template <class K, class P>
int launch(K kernel, long long blocks, int threads, size_t lds, hipStream_t stream, const P &params, const char *what) {
  if (blocks <= 0) return MCHAP_OK;
  if (blocks > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "family: %s: %lld workgroups exceed one launch", what, blocks);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, stream, params);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int colsum(int R, const double *mat, const double *wgt, long long rows, long long cols, double *out, hipStream_t stream) {
  mchap::FamilyColsumParams C;
  C.mat = mat; C.wgt = wgt; C.rows = rows; C.cols = cols; C.nblk = tiles_of(cols, mchap::WAVE); C.out = out;
  return launch(mchap::family_colsum_kernel, (long long)R * C.nblk, mchap::EXACT_THREADS, 0, stream, C, "column sums");
}

int modes(int rows, const double *p, long long G, long long pitch, int64_t *mode, double *prob, int out_pitch, hipStream_t stream) {
  mchap::FamilyModeParams M;
  M.p = p; M.G = G; M.pitch = pitch; M.mode = reinterpret_cast<long long *>(mode); M.prob = prob; M.out_pitch = out_pitch;
  return launch(mchap::family_mode_kernel, rows, mchap::EXACT_THREADS, 0, stream, M, "modes");
}

#define TRY(expr)          \
  do {                     \
    const int rc_ = (expr); \
    if (rc_) return rc_;   \
  } while (0)

}  // namespace

extern "C" {

int64_t mchap_exact_family_workspace_bytes(int n_records, int n_haps, int ploidy_p, int ploidy_q, int force_fallback) {
  FamilyShape s;
  FamilyCarve c;
  if (!family_shape(n_haps, ploidy_p, ploidy_q, force_fallback, s)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_records <= 0) return 0;
  if (!family_carve(n_records, s, c)) return -1;
  return (int64_t)c.bytes;
}

int mchap_exact_family_device(int n_records, int n_progeny, const double *llks_p, const double *llks_q, const double *llks_c,
                              const int32_t *progeny_reads, int n_haps, int ploidy_p, int ploidy_q, const double *inbreeding_p,
                              const double *inbreeding_q, const double *frequencies, int stride, const double *gamete_error_p,
                              const double *gamete_error_q, double *post_p, int64_t *mode_p, double *mode_prob_p, double *post_q,
                              int64_t *mode_q, double *mode_prob_q, double *q, int64_t *mode_c, double *mode_prob_c,
                              double *pred_log_evidence, double *log_z_fam, void *workspace, int64_t workspace_bytes,
                              int force_fallback, void *stream_) {
  if (n_records <= 0) return MCHAP_OK;
  if (n_progeny < 0) return fail(MCHAP_ERR_BAD_ARG, "family: %d progeny", n_progeny);
  if (!llks_p || !llks_q || !frequencies || !gamete_error_p || !gamete_error_q || !post_p || !mode_p || !mode_prob_p || !post_q ||
      !mode_q || !mode_prob_q || !log_z_fam)
    return fail(MCHAP_ERR_BAD_ARG, "family: NULL buffer");
  if (n_progeny > 0 && (!llks_c || !mode_c || !mode_prob_c || !pred_log_evidence))
    return fail(MCHAP_ERR_BAD_ARG, "family: NULL progeny buffer");
  if (!ploidy_ok(ploidy_p) || !ploidy_ok(ploidy_q))
    return fail(MCHAP_ERR_LIMIT, "ploidies %d and %d not in 1..%d", ploidy_p, ploidy_q, MCHAP_MAX_PLOIDY_DENOVO);
  if (ploidy_p % 2 || ploidy_q % 2) return fail(MCHAP_ERR_BAD_ARG, "family: a parent of odd ploidy (%d, %d)", ploidy_p, ploidy_q);
  if (n_haps < 1 || stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "family: rows of %d doubles for %d haplotypes", stride, n_haps);
  FamilyShape s;
  FamilyCarve cv;
  if (!family_shape(n_haps, ploidy_p, ploidy_q, force_fallback, s) || !family_carve(n_records, s, cv))
    return fail(MCHAP_ERR_LIMIT, "family: ploidies %d x %d over %d haplotypes: beyond the family kernels", ploidy_p, ploidy_q, n_haps);
  if (!workspace || workspace_bytes < (int64_t)cv.bytes)
    return fail(MCHAP_ERR_LIMIT, "family: the [G_P][G_Q] workspace needs %zu bytes, %lld are offered (mchap_exact_family_workspace_bytes)",
                cv.bytes, (long long)workspace_bytes);
  const size_t lds_prior_p = mchap::exact_gamete_lds(n_haps, ploidy_p), lds_prior_q = mchap::exact_gamete_lds(n_haps, ploidy_q);
  if (lds_prior_p > 64 * 1024 || lds_prior_q > 64 * 1024)
    return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the family kernels' prior tables", n_haps);
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  const int R = n_records, T = mchap::EXACT_THREADS;
  const bool wide = ploidy_p > 8 || ploidy_q > 8;
  auto at = [&](size_t off) { return reinterpret_cast<double *>(ws + off); };

  // the tables of the two parent shapes, Mult of every gamete, lp + llk of every parent genotype
  mchap::FamilyTables tab[2];
  const int K[2] = {ploidy_p, ploidy_q}, W[2] = {s.WP, s.WQ};
  const long long G[2] = {s.GP, s.GQ}, NA[2] = {s.NAP, s.NAQ};
  const double *llks[2] = {llks_p, llks_q}, *inb[2] = {inbreeding_p, inbreeding_q};
  for (int u = 0; u < 2; u++) {
    mchap::FamilyTables &t = tab[u];
    t.fcnt = reinterpret_cast<int *>(ws + cv.fcnt[u]);
    t.fidx = reinterpret_cast<int *>(ws + cv.fidx[u]);
    t.fwt = at(cv.fwt[u]);
    t.bidx = reinterpret_cast<int *>(ws + cv.bidx[u]);
    t.bwt = at(cv.bwt[u]);
    t.K = K[u]; t.T = K[u] / 2; t.W = W[u]; t.G = G[u]; t.NA = NA[u];
    TRY(launch(wide ? mchap::family_rows_kernel<mchap::EXACT_KMAX> : mchap::family_rows_kernel<8>, tiles_of(G[u], T), T, 0, stream, t, "rows"));
    TRY(launch(wide ? mchap::family_cols_kernel<mchap::EXACT_KMAX> : mchap::family_cols_kernel<8>, tiles_of(NA[u] * NA[u], T), T, 0, stream, t, "columns"));
    mchap::FamilyMultParams M;
    M.freqs = frequencies; M.stride = stride; M.T = K[u] / 2; M.nblk = tiles_of(NA[u], T); M.NA = NA[u]; M.mult = at(cv.mult[u]);
    TRY(launch(wide ? mchap::family_mult_kernel<mchap::EXACT_KMAX> : mchap::family_mult_kernel<8>, (long long)R * M.nblk, T, 0, stream, M, "Mult"));
    mchap::FamilyPriorParams Q;
    Q.llk64 = llks[u]; Q.inbreeding = inb[u]; Q.freqs = frequencies; Q.stride = stride; Q.H = n_haps; Q.K = K[u];
    Q.nblk = tiles_of(G[u], T); Q.G = G[u]; Q.joint = at(cv.joint[u]);
    TRY(launch(wide ? mchap::family_prior_kernel<mchap::EXACT_KMAX> : mchap::family_prior_kernel<8>, (long long)R * Q.nblk, T,
               u ? lds_prior_q : lds_prior_p, stream, Q, "priors"));
  }

  mchap::FamilyRoundParams E;
  std::memset(&E, 0, sizeof(E));
  E.H = n_haps; E.TP = s.TP; E.TQ = s.TQ;
  E.GP = s.GP; E.GQ = s.GQ; E.GC = s.GC; E.NAP = s.NAP; E.NAQ = s.NAQ;
  E.tp = tab[0]; E.tq = tab[1];
  E.mult_p = at(cv.mult[0]); E.mult_q = at(cv.mult[1]);
  E.err_p = gamete_error_p; E.err_q = gamete_error_q;
  E.lmax = at(cv.lmax); E.pair = at(cv.pair); E.dp = at(cv.dp); E.v = at(cv.v); E.s = at(cv.s); E.y = at(cv.y); E.cy = at(cv.cy);
  E.rr = at(cv.rr); E.dsum = at(cv.dsum); E.dtot = at(cv.dtot);
  E.staged = s.staged ? 1 : 0;
  E.drow = s.staged ? nullptr : at(cv.drow);
  E.log_z = log_z_fam;
  E.llk_pitch = (long long)n_progeny * s.GC;
  E.reads_pitch = n_progeny;
  E.pred_pitch = n_progeny;
  const long long pairs = s.NAP * s.NAQ;
  const size_t lds_fwd = s.staged ? mchap::family_row_lds(s.NAQ, s.GQ, false) : 0;
  const size_t lds_back = s.staged ? mchap::family_row_lds(s.NAQ, s.GQ, true) : 0;
  auto pair_kernel = wide ? mchap::family_pair_kernel<mchap::EXACT_KMAX> : mchap::family_pair_kernel<8>;
  auto q_kernel = wide ? mchap::family_q_kernel<mchap::EXACT_KMAX> : mchap::family_q_kernel<8>;

  // the forward stages of a round: m_c, T_c, its Mult_P-weighted column sums, V_c
  auto forward = [&](int c) -> int {
    E.llk = llks_c + (size_t)c * s.GC;
    E.reads = progeny_reads ? progeny_reads + c : nullptr;
    TRY(launch(mchap::family_max_kernel, R, T, 0, stream, E, "maxima"));
    E.nblk = tiles_of(pairs, T);
    TRY(launch(pair_kernel, (long long)R * E.nblk, T, 0, stream, E, "gamete pairs"));
    TRY(colsum(R, E.pair, E.mult_p, s.NAP, s.NAQ, E.dp, stream));
    E.nblk = tiles_of(s.GP * s.NAQ, T);
    TRY(launch(mchap::family_v_kernel, (long long)R * E.nblk, T, 0, stream, E, "V"));
    return MCHAP_OK;
  };

  // S over the progeny in their order
  HIP_TRY(hipMemsetAsync(E.s, 0, (size_t)R * s.GP * s.GQ * 8, stream));
  for (int c = 0; c < n_progeny; c++) {
    TRY(forward(c));
    TRY(launch(mchap::family_row_kernel<false>, (long long)R * s.GP, T, lds_fwd, stream, E, "M"));
  }

  // log Z_fam, w in the place of S, the parents' marginals and their modes
  mchap::FamilyPostParams Z;
  Z.joint_p = at(cv.joint[0]); Z.joint_q = at(cv.joint[1]);
  Z.GP = s.GP; Z.GQ = s.GQ; Z.s = E.s; Z.part = at(cv.part); Z.log_z = log_z_fam; Z.post_p = post_p;
  TRY(launch(mchap::family_rowstat_kernel, (long long)R * s.GP, T, 0, stream, Z, "row maxima"));
  TRY(launch(mchap::family_z_kernel, R, mchap::WAVE, 0, stream, Z, "log Z"));
  TRY(launch(mchap::family_weight_kernel, (long long)R * s.GP, T, 0, stream, Z, "weights"));
  TRY(colsum(R, E.s, nullptr, s.GP, s.GQ, post_q, stream));
  TRY(modes(R, post_p, s.GP, s.GP, mode_p, mode_prob_p, 1, stream));
  TRY(modes(R, post_q, s.GQ, s.GQ, mode_q, mode_prob_q, 1, stream));

  // the back projection, a progeny at a time: M_c again, w / M_c, Y_c, R_c, q_c
  // (q_c without an output array: the round's rows go to V_c's place, which the round has finished with -- G_c <= G_P NA_Q)
  for (int c = 0; c < n_progeny; c++) {
    TRY(forward(c));
    TRY(launch(mchap::family_row_kernel<true>, (long long)R * s.GP, T, lds_back, stream, E, "w / M"));
    TRY(colsum(R, E.dsum, nullptr, s.GP, 1, E.dtot, stream));
    TRY(colsum(R, E.y, nullptr, s.GP, s.NAQ, E.cy, stream));
    E.nblk = tiles_of(pairs, T);
    TRY(launch(mchap::family_r_kernel, (long long)R * E.nblk, T, 0, stream, E, "R"));
    E.q = q ? q + (size_t)c * s.GC : E.v;
    E.q_pitch = q ? (long long)n_progeny * s.GC : s.GC;
    E.pred = pred_log_evidence + c;
    E.nblk = tiles_of(s.GC, T);
    TRY(launch(q_kernel, (long long)R * E.nblk, T, 0, stream, E, "q"));
    TRY(modes(R, E.q, s.GC, E.q_pitch, mode_c + c, mode_prob_c + c, n_progeny, stream));
  }
  return MCHAP_OK;
}

}  // extern "C"
