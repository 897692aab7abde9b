// libmchap_hip.so -- candidate parent pairs per progeny over stored likelihoods (exact_parentage_kernel.hpp): the cross evidence of
// every progeny of a record under every pair of rows of two gamete tables, and the population's row of such a table.
// Entry points declared in include/mchap_hip.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_common.hpp"
#include "exact_parentage_kernel.hpp"

using mchap::cwr_fits;
using mchap::ensure_init;
using mchap::fail;
using mchap::host_cwr;
using mchap::up256;

namespace {

int tiles_of(long long n, int per) { return (int)((n + per - 1) / per); }
bool gamete_ok(int t) { return t >= 1 && t <= mchap::PARENTAGE_TMAX; }
// the shapes the launches take: gamete sizes, the progeny's ploidy and genotype count, the rank table beside the staged rows in LDS
bool shape_ok(int n_haps, int t_a, int t_b) {
  return gamete_ok(t_a) && gamete_ok(t_b) && t_a + t_b <= MCHAP_MAX_PLOIDY_DENOVO && n_haps >= 1 && cwr_fits(n_haps, t_a + t_b) &&
         mchap::parentage_w_lds(n_haps, t_a + t_b) <= 160 * 1024;
}

// carve of the workspace: the rank table, the progeny's maxima, W
struct Carve {
  size_t cw = 0, lmax = 0, w = 0, bytes = 0;
};
Carve carve(int n_records, int n_progeny, int n_b, int n_haps, int t_a, int t_b) {
  Carve c;
  size_t o = 0;
  c.cw = o; o += up256((size_t)n_haps * (t_a + t_b) * 8);
  c.lmax = o; o += up256((size_t)n_records * n_progeny * 8);
  c.w = o; o += up256((size_t)n_records * n_progeny * n_b * (size_t)host_cwr(n_haps, t_a) * 8);
  c.bytes = o;
  return c;
}

}  // namespace

extern "C" {

int64_t mchap_exact_parentage_workspace_bytes(int n_records, int n_progeny, int n_a, int n_b, int n_haps, int t_a, int t_b) {
  if (!shape_ok(n_haps, t_a, t_b)) return -1;  // (the call itself: MCHAP_ERR_LIMIT)
  if (n_records <= 0 || n_progeny <= 0 || n_a < 1 || n_b < 1) return 0;
  // (the product below 2^62: W alone is what a caller cuts its records and progeny by)
  const unsigned __int128 w = (unsigned __int128)n_records * n_progeny * n_b * (unsigned __int128)host_cwr(n_haps, t_a) * 8;
  if (w >> 62) return -1;
  return (int64_t)carve(n_records, n_progeny, n_b, n_haps, t_a, t_b).bytes;
}

int mchap_exact_parentage_device(int n_records, int n_progeny, int n_a, int n_b, const double *gametes_a, const double *gametes_b,
                                 const double *llks_c, const int32_t *progeny_reads, int n_haps, int t_a, int t_b, double *log_z,
                                 void *workspace, int64_t workspace_bytes, void *stream_) {
  if (n_records <= 0 || n_progeny <= 0) return MCHAP_OK;
  if (n_a < 1 || n_b < 1) return fail(MCHAP_ERR_BAD_ARG, "parentage: %d x %d rows", n_a, n_b);
  if (!gametes_a || !gametes_b || !llks_c || !log_z) return fail(MCHAP_ERR_BAD_ARG, "parentage: NULL buffer");
  if (n_haps < 1) return fail(MCHAP_ERR_BAD_ARG, "parentage: no haplotype");
  if (!gamete_ok(t_a) || !gamete_ok(t_b))
    return fail(MCHAP_ERR_LIMIT, "gamete sizes %d and %d not in 1..%d", t_a, t_b, mchap::PARENTAGE_TMAX);
  const int KC = t_a + t_b;
  if (KC > MCHAP_MAX_PLOIDY_DENOVO) return fail(MCHAP_ERR_LIMIT, "progeny ploidy %d not in 1..%d", KC, MCHAP_MAX_PLOIDY_DENOVO);
  if (!cwr_fits(n_haps, KC)) return fail(MCHAP_ERR_LIMIT, "ploidy %d over %d haplotypes: more than 2^62 genotypes", KC, n_haps);
  const size_t lds = mchap::parentage_w_lds(n_haps, KC);
  if (lds > 160 * 1024) return fail(MCHAP_ERR_LIMIT, "n_haps %d too large for the parentage kernel's rank table", n_haps);
  const int64_t need = mchap_exact_parentage_workspace_bytes(n_records, n_progeny, n_a, n_b, n_haps, t_a, t_b);
  if (need < 0) return fail(MCHAP_ERR_LIMIT, "parentage: %d records x %d progeny x %d columns exceed one call", n_records, n_progeny, n_b);
  if (!workspace || workspace_bytes < need)
    return fail(MCHAP_ERR_LIMIT, "workspace of %lld bytes is too small: %lld needed (mchap_exact_parentage_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
  const Carve cv = carve(n_records, n_progeny, n_b, n_haps, t_a, t_b);
  unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
  mchap::ParentageParams E;
  std::memset(&E, 0, sizeof(E));
  E.gam_a = gametes_a;
  E.gam_b = gametes_b;
  E.llk = llks_c;
  E.reads = progeny_reads;
  E.H = n_haps; E.TA = t_a; E.TB = t_b; E.C = n_progeny; E.n_a = n_a; E.n_b = n_b;
  E.NA = host_cwr(n_haps, t_a); E.NB = host_cwr(n_haps, t_b); E.GC = host_cwr(n_haps, KC);
  E.ppb = E.NA <= mchap::EXACT_THREADS / 2 ? (int)(mchap::EXACT_THREADS / E.NA) : 1;
  E.ngrp = tiles_of(n_progeny, E.ppb);
  const long long ntile = E.ppb > 1 ? 1 : (E.NA + mchap::EXACT_THREADS - 1) / mchap::EXACT_THREADS;
  E.nchunk = tiles_of(n_b, mchap::PARENTAGE_COLS);
  const unsigned __int128 grid_w = (unsigned __int128)n_records * E.ngrp * ntile * E.nchunk;
  const long long grid_z = (long long)n_records * n_progeny * n_b;
  if (grid_w > 0x7fffffffull || grid_z > 0x7fffffffll)
    return fail(MCHAP_ERR_LIMIT, "parentage: %d records x %d progeny x %d columns exceed one launch", n_records, n_progeny, n_b);
  E.ntile = (int)ntile;
  E.cw = reinterpret_cast<long long *>(ws + cv.cw);
  E.lmax = reinterpret_cast<double *>(ws + cv.lmax);
  E.w = reinterpret_cast<double *>(ws + cv.w);
  E.log_z = log_z;
  int rc = ensure_init();
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(mchap::parentage_cw_kernel, dim3(tiles_of((long long)KC * n_haps, mchap::EXACT_THREADS)), dim3(mchap::EXACT_THREADS), 0,
                     stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::parentage_max_kernel, dim3((unsigned)(n_records * n_progeny)), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  const int tm = t_a > t_b ? t_a : t_b;
  auto k = tm <= 2 ? mchap::parentage_w_kernel<2> : tm <= 4 ? mchap::parentage_w_kernel<4> : mchap::parentage_w_kernel<mchap::PARENTAGE_TMAX>;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)(unsigned long long)grid_w), dim3(mchap::EXACT_THREADS), lds, stream, E);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mchap::parentage_z_kernel, dim3((unsigned)grid_z), dim3(mchap::EXACT_THREADS), 0, stream, E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

int mchap_exact_parentage_population_device(int n_records, const double *frequencies, int stride, int n_haps, int t, double *rows,
                                            int64_t row_pitch, void *stream_) {
  if (n_records <= 0) return MCHAP_OK;
  if (!frequencies || !rows) return fail(MCHAP_ERR_BAD_ARG, "parentage population: NULL buffer");
  if (n_haps < 1 || stride < n_haps) return fail(MCHAP_ERR_BAD_ARG, "parentage population: rows of %d doubles for %d haplotypes", stride, n_haps);
  if (!gamete_ok(t)) return fail(MCHAP_ERR_LIMIT, "gamete size %d not in 1..%d", t, mchap::PARENTAGE_TMAX);
  if (!cwr_fits(n_haps, t)) return fail(MCHAP_ERR_LIMIT, "%d of %d haplotypes: more than 2^62 gametes", t, n_haps);
  const long long NA = host_cwr(n_haps, t);
  if (row_pitch < NA) return fail(MCHAP_ERR_BAD_ARG, "parentage population: a pitch of %lld doubles for %lld gametes", (long long)row_pitch, NA);
  const int nblk = tiles_of(NA, mchap::EXACT_THREADS);
  if ((long long)n_records * nblk > 0x7fffffffll) return fail(MCHAP_ERR_LIMIT, "parentage population: %d records x %d tiles exceed one launch", n_records, nblk);
  int rc = ensure_init();
  if (rc) return rc;
  mchap::ParentageMultParams E;
  std::memset(&E, 0, sizeof(E));
  E.freqs = frequencies;
  E.stride = stride; E.T = t; E.nblk = nblk;
  E.NA = NA; E.pitch = row_pitch;
  E.rows = rows;
  hipLaunchKernelGGL(mchap::parentage_mult_kernel<8>, dim3((unsigned)((long long)n_records * nblk)), dim3(mchap::EXACT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream_), E);
  HIP_TRY(hipGetLastError());
  return MCHAP_OK;
}

}  // extern "C"
