// What the host files of the library share (mchap_hip.hip, posterior_api.hip, exact_api.hip, call_api.hip, pileup_inst.hip,
// call_reads_inst.hip, call_keys_test.hip): the error text, the once-per-device initialisation and the helpers of the host-pointer
// entry points.  Internal: everything here has hidden visibility -- libmchap_hip.so and libmchap_hip_test.so are loaded side by side
// in one process, and neither may export a helper the other could bind to.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/mchap_hip.h"

#pragma GCC visibility push(hidden)
namespace mchap {

// Both are defined once per library, in mchap_hip.hip.  fail: writes the calling thread's text behind mchap_last_error and returns
// `code`.  ensure_init: MCHAP_ERR_NO_DEVICE without a device, else the constant tables of the sampler objects, once per device.
__attribute__((format(printf, 2, 3))) int fail(int code, const char *fmt, ...);
int ensure_init();

#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return mchap::fail(MCHAP_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define MCHAP_TRY(expr)       \
  do {                        \
    const int rc_ = (expr);   \
    if (rc_) return rc_;      \
  } while (0)

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

// A host-pointer entry point works on a stream of its own (non-blocking: it neither waits for nor stalls the caller's
// other streams) and synchronises that stream only.
struct HostCall {
  hipStream_t stream = nullptr;
  int open() {
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return MCHAP_OK;
  }
  ~HostCall() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  int up(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    return MCHAP_OK;
  }
  int down(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    return MCHAP_OK;
  }
  int sync() {
    HIP_TRY(hipStreamSynchronize(stream));
    return MCHAP_OK;
  }
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// one device allocation for a host-pointer call: pieces handed out 256-byte aligned
struct DevArena {
  DevBuf buf;
  size_t cap = 0, off = 0;
  int reserve(size_t bytes) {
    cap = bytes + 4096;
    if (hipMalloc(&buf.p, cap) != hipSuccess) return fail(MCHAP_ERR_HIP, "hipMalloc of %zu bytes", cap);
    return MCHAP_OK;
  }
  template <class T>
  T *take(size_t n) {
    T *p = reinterpret_cast<T *>(reinterpret_cast<unsigned char *>(buf.p) + off);
    off += up256(n * sizeof(T));
    return off <= cap ? p : nullptr;
  }
};

// C(n + k - 1, k): the genotypes of ploidy k over n haplotypes (the exact caller's arrays, the call sampler's cache keys)
inline long long host_cwr(int n, int k) {
  if (n <= 0) return 0;
  // (the product before the division in 128 bits: it passes 2^63 for counts near 2^62, which cwr_fits admits)
  unsigned __int128 r = 1;
  for (int d = 1; d <= k; d++) r = r * (unsigned __int128)(n - 1 + d) / (unsigned __int128)d;
  return (long long)r;
}

// C(n + k - 1, k) stays below 2^62 (the genotype indices and the call sampler's cache keys are int64; ploidy 15 over 200
// haplotypes would not)
inline bool cwr_fits(int n, int k) {
  if (n <= 0) return true;
  unsigned __int128 r = 1;
  for (int d = 1; d <= k; d++) {
    r = r * (unsigned __int128)(n - 1 + d) / (unsigned __int128)d;
    if (r >> 62) return false;
  }
  return true;
}

}  // namespace mchap
#pragma GCC visibility pop
