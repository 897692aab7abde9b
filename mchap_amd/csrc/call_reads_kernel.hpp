// Read tensors of `mchap call` / `mchap call-exact` from int8 allele calls (mchap_call_reads_from_calls_device, and with base
// qualities in use mchap_call_reads_from_calls_quals_device): what encoding.as_probabilistic / encode_read_distributions form on
// the host, per (unit, row, position, allele) cell, and the [U][n_reads] counts, padded the way the programs pad a shape group
// (NaN rows of weight 0).
//
// Meant as a store-bound fill: one lane per output double, so a wavefront's 64 stores are 512 consecutive bytes; every lane loads
// its call byte and its n_alleles byte once (the lanes of a cell's A alleles share them: one cache line serves the wavefront);
// grid-stride over a capped grid; no LDS, no atomics, no arithmetic on the probabilities -- the host computes them as
// as_probabilistic does and the tensor is the host's bit for bit.  Without qualities they are two numbers (p_call, p_other); with
// qualities a called cell of quality q gives its allele p_call_q[q] and every other allele p_other_q[q] -- two float64 tables of
// n_qual entries (p_other_q[q] = (1 - p_call_q[q]) / 3): a lane then also loads the cell's int16 quality (the lanes of a cell's A
// alleles share it) and ONE table entry, its index clamped into [0, n_qual) so that no input reads outside the tables (the host
// has checked the qualities before the upload).  A lane finds (u, r, j, a) by two integer divisions of its index: in 32 bits while
// U x Rmax x M x A is below 2^32 (the usual case), in 64 bits beyond (it passes 2^31 at the unit counts
// application.device_unit_budget allows).  NOT MEASURED: whether the stores, those divisions or the table gathers (a few hundred
// distinct entries at most: they should stay in cache) bound the kernel, and whether the grid cap (8 workgroups of 256 per CU) is
// the right one, has not been read off a trace yet.
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
  double p_call, p_other;         // without qualities
  double *reads;                  // [U][R][M][A]
  int64_t *read_counts;           // [U][R]
  // with qualities (else not read)
  const int16_t *quals;           // laid out like calls
  const double *p_call_q;         // [n_qual]
  const double *p_other_q;        // [n_qual]
  int n_qual;                     // >= 1
};

// Index: the type a lane divides its cell index in -- uint32_t while every cell index fits 32 bits, else int64_t
template <typename Index, bool QUALS>
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
      const int64_t e = P.unit_call_off[u] + r * P.M + j;
      const int call = P.calls[e];
      const int n = P.n_alleles[u * P.M + j];
      if constexpr (QUALS) {
        if (call >= 0) {
          int q = P.quals[e];
          q = q < 0 ? 0 : (q >= P.n_qual ? P.n_qual - 1 : q);
          v = a == call ? P.p_call_q[q] : P.p_other_q[q];
        }
      } else {
        v = call < 0 ? gap : (a == call ? P.p_call : P.p_other);
      }
      if (a >= n) v = 0.0;  // (last: a gap at a biallelic position of a 3-allele tensor reads [nan, nan, 0])
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
