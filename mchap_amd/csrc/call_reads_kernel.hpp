// Read tensors of `mchap call` / `mchap call-exact` from int8 allele calls (mchap_call_reads_from_calls_device): what
// encoding.as_probabilistic / encode_read_distributions form on the host without base qualities, per (unit, row, position, allele)
// cell, and the [U][n_reads] counts, padded the way the programs pad a shape group (NaN rows of weight 0).
//
// Meant as a store-bound fill: one lane per output double, so a wavefront's 64 stores are 512 consecutive bytes; every lane loads
// its call byte and its n_alleles byte once (the lanes of a cell's A alleles share them: one cache line serves the wavefront);
// grid-stride over a capped grid; no LDS, no atomics, no arithmetic on the two probabilities -- the host computes them as
// as_probabilistic does and the tensor is the host's bit for bit.  A lane finds (u, r, j, a) by two integer divisions of its index:
// in 32 bits while U x Rmax x M x A is below 2^32 (the usual case), in 64 bits beyond (it passes 2^31 at the unit counts
// application.device_unit_budget allows).  NOT MEASURED: whether the stores or those divisions bound the kernel, and whether the
// grid cap (8 workgroups of 256 per CU) is the right one, has not been read off a trace yet.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mchap {

constexpr int CALL_READS_THREADS = 256;
// the grid is capped (8 workgroups per CU of 256 CUs) and strides over the rest
constexpr int CALL_READS_MAX_BLOCKS = 2048;

struct CallReadsParams {
  const int8_t *calls;            // distinct call rows, unit after unit, [rows_u][M]
  const int64_t *counts;          // their counts, unit after unit
  const int64_t *unit_rows;       // [U]
  const int64_t *unit_call_off;   // [U] first element of unit u in calls
  const int64_t *unit_count_off;  // [U] first element of unit u in counts
  const int8_t *n_alleles;        // [U][M]
  int64_t n_units;
  int R, M, A;
  double p_call, p_other;
  double *reads;                  // [U][R][M][A]
  int64_t *read_counts;           // [U][R]
};

// Index: the type a lane divides its cell index in -- uint32_t while every cell index fits 32 bits, else int64_t
template <typename Index>
__global__ __launch_bounds__(CALL_READS_THREADS) static void call_reads_kernel(const CallReadsParams P) {
  const uint32_t MA = (uint32_t)P.M * (uint32_t)P.A;
  const int64_t total = P.n_units * P.R * (int64_t)MA;
  const int64_t stride = (int64_t)gridDim.x * CALL_READS_THREADS;
  const double gap = __builtin_nan("");
  // (the loop variable stays 64-bit: i + stride may pass 2^32 on the last pass; the divisions take it as Index)
  for (int64_t i64 = (int64_t)blockIdx.x * CALL_READS_THREADS + threadIdx.x; i64 < total; i64 += stride) {
    const Index i = (Index)i64;
    const Index row = i / (Index)MA;                           // u * R + r
    const uint32_t in_row = (uint32_t)(i - row * (Index)MA);   // j * A + a
    const uint32_t j = in_row / (uint32_t)P.A;
    const int a = (int)(in_row - j * (uint32_t)P.A);
    const Index ui = row / (Index)P.R;
    const int64_t u = (int64_t)ui;
    const int64_t r = (int64_t)(row - ui * (Index)P.R);
    double v = gap;  // a padding row: NaN in every cell
    if (r < P.unit_rows[u]) {
      const int call = P.calls[P.unit_call_off[u] + r * P.M + j];
      const int n = P.n_alleles[u * P.M + j];
      v = call < 0 ? gap : (a == call ? P.p_call : P.p_other);
      if (a >= n) v = 0.0;  // (last: a gap at a biallelic position of a 3-allele tensor reads [nan, nan, 0])
    }
    P.reads[i64] = v;
  }
}

// The same tensor with base qualities in use (mchap_call_reads_from_calls_quals_device): a called cell of quality q gives its allele
// p_call[q] and every other allele p_other[q] -- two float64 tables of n_qual entries the host computed as as_probabilistic does
// (p_other[q] = (1 - p_call[q]) / 3), so here too the device does no arithmetic on probabilities and the tensor is the host's bit for
// bit.  Same shape of kernel: one lane per output double (512 consecutive bytes a wavefront), grid-stride over the same capped grid,
// the cell index divided in 32 or 64 bits.  A lane loads its call byte and its n_alleles byte; for a called cell also the int16
// quality (the lanes of a cell's A alleles share it) and ONE table entry, its index clamped into [0, n_qual) so that no input reads
// outside the tables (the host has checked the qualities before the upload).  NOT MEASURED: whether the stores, the two integer
// divisions or the table gathers (a few hundred distinct entries at most: they should stay in cache) bound this kernel.
struct CallReadsQualsParams {
  CallReadsParams base;           // (p_call / p_other of the base are not used)
  const int16_t *quals;           // laid out like base.calls
  const double *p_call;           // [n_qual]
  const double *p_other;          // [n_qual]
  int n_qual;                     // >= 1
};

template <typename Index>
__global__ __launch_bounds__(CALL_READS_THREADS) static void call_reads_quals_kernel(const CallReadsQualsParams Q) {
  const CallReadsParams &P = Q.base;
  const uint32_t MA = (uint32_t)P.M * (uint32_t)P.A;
  const int64_t total = P.n_units * P.R * (int64_t)MA;
  const int64_t stride = (int64_t)gridDim.x * CALL_READS_THREADS;
  const double gap = __builtin_nan("");
  for (int64_t i64 = (int64_t)blockIdx.x * CALL_READS_THREADS + threadIdx.x; i64 < total; i64 += stride) {
    const Index i = (Index)i64;
    const Index row = i / (Index)MA;                           // u * R + r
    const uint32_t in_row = (uint32_t)(i - row * (Index)MA);   // j * A + a
    const uint32_t j = in_row / (uint32_t)P.A;
    const int a = (int)(in_row - j * (uint32_t)P.A);
    const Index ui = row / (Index)P.R;
    const int64_t u = (int64_t)ui;
    const int64_t r = (int64_t)(row - ui * (Index)P.R);
    double v = gap;  // a padding row: NaN in every cell
    if (r < P.unit_rows[u]) {
      const int64_t e = P.unit_call_off[u] + r * P.M + j;
      const int call = P.calls[e];
      const int n = P.n_alleles[u * P.M + j];
      if (call >= 0) {
        int q = Q.quals[e];
        q = q < 0 ? 0 : (q >= Q.n_qual ? Q.n_qual - 1 : q);
        v = a == call ? Q.p_call[q] : Q.p_other[q];
      }
      if (a >= n) v = 0.0;  // (last, as in call_reads_kernel)
    }
    P.reads[i64] = v;
  }
}

// read_counts[u][r]: the row's count, 0 for a padding row -- one lane per count
__global__ __launch_bounds__(CALL_READS_THREADS) static void call_read_counts_kernel(const CallReadsParams P) {
  const int64_t total = P.n_units * P.R;
  const int64_t stride = (int64_t)gridDim.x * CALL_READS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * CALL_READS_THREADS + threadIdx.x; i < total; i += stride) {
    const int64_t u = i / P.R;
    const int64_t r = i - u * P.R;
    P.read_counts[i] = r < P.unit_rows[u] ? P.counts[P.unit_count_off[u] + r] : 0;
  }
}

}  // namespace mchap
