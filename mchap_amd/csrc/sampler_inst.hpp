// What every sampler object (*_inst.hip) does besides naming its kernel: fill its own copy of the constant log tables, launch
// with a grid, a block and dynamic LDS, and -- profiling builds -- hand out its copy of the event counters.  The object then states
// only which kernel it instantiates, with which block size and extra arguments, and its descriptor (sampler_objects.hpp).
// Internal: hidden visibility, as in host_common.hpp.
#pragma once
#include "sampler_objects.hpp"

#pragma GCC visibility push(hidden)
namespace mchap {

// the two log tables into the including unit's c_ln / c_ln_inv (static __constant__: one copy per object)
static int sampler_init(const double *ln, const double *ln_inv) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(mchap::c_ln), ln, sizeof(double) * 260) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(mchap::c_ln_inv), ln_inv, sizeof(double) * 260) != hipSuccess) return 1;
  return 0;
}

// returns the hipError_t of the launch (0: launched)
template <class... Params, class... Args>
static int sampler_launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &...args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  return (int)hipGetLastError();
}

// The object's descriptor: host data (it points at host functions), so the device pass of the compile, which would emit a
// constant of the same name, does not see it
#ifdef __HIP_DEVICE_COMPILE__
#define SAMPLER_DESCRIPTOR(type, name, ...)
#else
#define SAMPLER_DESCRIPTOR(type, name, ...) extern "C" __attribute__((visibility("hidden"))) const type name = {__VA_ARGS__};
#endif

#if defined(MCHAP_STATS) || defined(MCHAP_PHASES)
// profiling builds: this object's copy of the event counters, read and optionally reset
static int sampler_stats(unsigned long long *out, int reset) {
  unsigned long long z[mchap::N_STATS] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mchap::g_stats), sizeof(z)) != hipSuccess) return 1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(mchap::g_stats), z, sizeof(z)) != hipSuccess) return 1;
  return 0;
}
#define SAMPLER_STATS mchap::sampler_stats
#else
#define SAMPLER_STATS nullptr
#endif

}  // namespace mchap
#pragma GCC visibility pop
