// C ABI of the read-tensor fill of `mchap call` / `mchap call-exact` (call_reads_kernel.hpp; declared in include/mchap_hip.h).
// Device pointers, a hipStream_t passed as void*, enqueue and return: the caller (mchap_amd/device.py) owns every buffer.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "host_common.hpp"
#include "call_reads_kernel.hpp"

namespace {

unsigned grid_of(int64_t n) {
  const int64_t nb = (n + mchap::CALL_READS_THREADS - 1) / mchap::CALL_READS_THREADS;
  return (unsigned)(nb < mchap::CALL_READS_MAX_BLOCKS ? nb : mchap::CALL_READS_MAX_BLOCKS);
}

// the fields both entry points fill (the probabilities, as numbers or as tables, are the entry point's own)
mchap::CallReadsParams params_of(int n_units, const int8_t *calls, const int64_t *counts, const int64_t *unit_rows,
                                 const int64_t *unit_call_off, const int64_t *unit_count_off, const int8_t *n_alleles, int n_reads,
                                 int n_pos, int max_allele, double *reads, int64_t *read_counts) {
  mchap::CallReadsParams P = {};
  P.calls = calls;
  P.counts = counts;
  P.unit_rows = unit_rows;
  P.unit_call_off = unit_call_off;
  P.unit_count_off = unit_count_off;
  P.n_alleles = n_alleles;
  P.n_units = n_units;
  P.R = n_reads;
  P.M = n_pos;
  P.A = max_allele;
  P.reads = reads;
  P.read_counts = read_counts;
  return P;
}

template <typename Index, bool QUALS>
void launch_fill(const mchap::CallReadsParams &P, int64_t cells, hipStream_t stream) {
  hipLaunchKernelGGL((mchap::call_reads_kernel<Index, QUALS>), dim3(grid_of(cells)), dim3(mchap::CALL_READS_THREADS), 0, stream, P);
}

// the fill (with or without qualities, its cell index divided in 32 or 64 bits) and the counts on `stream`
hipError_t enqueue(const mchap::CallReadsParams &P, bool quals, hipStream_t stream) {
  const int64_t rows = P.n_units * P.R;
  const int64_t cells = rows * ((int64_t)P.M * P.A);
  // (MCHAP_HIP_CALL_READS_WIDE=1 -- measurement and tests; the tensor does not depend on it -- divides in 64 bits whatever the size)
  const char *wide = getenv("MCHAP_HIP_CALL_READS_WIDE");
  const bool narrow = cells < ((int64_t)1 << 32) && !(wide && wide[0] == '1');
  if (quals)
    narrow ? launch_fill<uint32_t, true>(P, cells, stream) : launch_fill<int64_t, true>(P, cells, stream);
  else
    narrow ? launch_fill<uint32_t, false>(P, cells, stream) : launch_fill<int64_t, false>(P, cells, stream);
  hipLaunchKernelGGL(mchap::call_read_counts_kernel, dim3(grid_of(rows)), dim3(mchap::CALL_READS_THREADS), 0, stream, P);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int mchap_call_reads_from_calls_device(int n_units, const int8_t *calls, const int64_t *counts, const int64_t *unit_rows,
                                       const int64_t *unit_call_off, const int64_t *unit_count_off, const int8_t *n_alleles,
                                       int n_reads, int n_pos, int max_allele, double p_call, double p_other, double *reads,
                                       int64_t *read_counts, void *stream) {
  if (n_units <= 0) return MCHAP_OK;
  if (n_reads < 1 || n_pos < 1 || max_allele < 1)
    return mchap::fail(MCHAP_ERR_BAD_ARG, "call reads: n_reads, n_pos and max_allele must be at least 1");
  // (calls / counts may be NULL when no unit has a row: they are then never read)
  if (!unit_rows || !unit_call_off || !unit_count_off || !n_alleles || !reads || !read_counts)
    return mchap::fail(MCHAP_ERR_BAD_ARG, "call reads: NULL buffer");
  mchap::CallReadsParams P = params_of(n_units, calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, n_pos,
                                       max_allele, reads, read_counts);
  P.p_call = p_call;
  P.p_other = p_other;
  const hipError_t e = enqueue(P, false, (hipStream_t)stream);
  if (e == hipSuccess) return MCHAP_OK;
  return mchap::fail(MCHAP_ERR_HIP, "call_reads_kernel: %s", hipGetErrorString(e));
}

int mchap_call_reads_from_calls_quals_device(int n_units, const int8_t *calls, const int16_t *quals, const int64_t *counts,
                                             const int64_t *unit_rows, const int64_t *unit_call_off, const int64_t *unit_count_off,
                                             const int8_t *n_alleles, int n_reads, int n_pos, int max_allele, const double *p_call,
                                             const double *p_other, int n_qual, double *reads, int64_t *read_counts, void *stream) {
  if (n_units <= 0) return MCHAP_OK;
  if (n_reads < 1 || n_pos < 1 || max_allele < 1 || n_qual < 1)
    return mchap::fail(MCHAP_ERR_BAD_ARG, "call reads: n_reads, n_pos, max_allele and n_qual must be at least 1");
  // (calls / quals / counts may be NULL when no unit has a row: they are then never read)
  if (!unit_rows || !unit_call_off || !unit_count_off || !n_alleles || !p_call || !p_other || !reads || !read_counts ||
      (calls && !quals))
    return mchap::fail(MCHAP_ERR_BAD_ARG, "call reads: NULL buffer");
  mchap::CallReadsParams P = params_of(n_units, calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, n_pos,
                                       max_allele, reads, read_counts);
  P.quals = quals;
  P.p_call_q = p_call;
  P.p_other_q = p_other;
  P.n_qual = n_qual;
  const hipError_t e = enqueue(P, true, (hipStream_t)stream);
  if (e == hipSuccess) return MCHAP_OK;
  return mchap::fail(MCHAP_ERR_HIP, "call_reads_quals_kernel: %s", hipGetErrorString(e));
}

}  // extern "C"
