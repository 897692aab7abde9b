// The sampler objects of the library: every instantiation of a de novo sampler kernel is its own object file (spec_inst.hip,
// simt_inst.hip, fillw_inst.hip, fill_inst.hip, v1_inst.hip, lane_inst.hip: they compile in parallel, 20-60 s each) and exports
// ONE descriptor -- its kind, ploidy and lanes per chain, its init (the object's copy of the constant log tables) and its
// launchers.  This header is the one list of them: the instantiation files name their descriptor through it, and the de novo
// host file (mchap_hip.hip) declares every descriptor of the list and looks an object up in a table of them (find_inst).  A listed
// object that is not linked is an undefined symbol: a link-time error.  Internal: everything here has hidden visibility, as in
// host_common.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "denovo_common.hpp"

// One X(kind, K, G) per object.  (The Makefile lists the same objects -- SPEC, SPECP, SPECP_T, SIMT_OBJS, FILLW_OBJS, FILL_OBJS,
// V1_OBJS, LANE_OBJS --: a new one is added on both sides.)
// kernel 3, the speculative sampler: G lanes per chain
#define SPEC_LIST(X) X(spec, 2, 16) X(spec, 2, 32) X(spec, 2, 64) X(spec, 3, 16) X(spec, 3, 32) X(spec, 3, 64) X(spec, 4, 16) X(spec, 4, 32) \
  X(spec, 4, 64) X(spec, 5, 32) X(spec, 5, 64) X(spec, 6, 32) X(spec, 6, 64) X(spec, 7, 64) X(spec, 8, 64)
// kernel 5, the phased form: one chain per wavefront at every ploidy (the narrower groups were measured slower; they
// stay in the test library so that the parity suite keeps covering hand-over with several chains per wave) ...
#define SPECP_LIST(X) X(specp, 2, 64) X(specp, 3, 64) X(specp, 4, 64) X(specp, 5, 64) X(specp, 6, 64) X(specp, 7, 64) X(specp, 8, 64)
#define SPECP_TEST_LIST(X) X(specp, 2, 16) X(specp, 3, 16) X(specp, 4, 16) X(specp, 4, 32) X(specp, 5, 32) X(specp, 6, 32)
// ... and its variants with the side-by-side evaluation of shallow units / the deep paths compiled in (MCHAP_SPEC_VAR,
// denovo_spec_kernel.hpp)
#define SPECS_LIST(X) X(specs, 2, 64) X(specs, 3, 64) X(specs, 4, 64) X(specs, 5, 64) X(specs, 6, 64) X(specs, 7, 64) X(specs, 8, 64)
#define SPECD_LIST(X) X(specd, 2, 64) X(specd, 3, 64) X(specd, 4, 64) X(specd, 5, 64) X(specd, 6, 64) X(specd, 7, 64) X(specd, 8, 64)
// kernel 2, a lane per chain: the compile-time ploidies (0: per lane) with haplotype words of G = 64 bits, and the instantiation
// with 128-bit words (simt_inst.hip -DSIMT_WIDE): the general fallback for wide targets
#define SIMT_LIST(X) X(simt, 0, 64) X(simt, 2, 64) X(simt, 4, 64) X(simt, 6, 64) X(simt, 8, 64) X(simt, 0, 128)
// table completion of the phased sampler, one workgroup per chain and one wavefront per request (denovo_fillw_kernel.hpp): shipped
#define FILLW_LIST(X) X(fillw, 2, 64) X(fillw, 3, 64) X(fillw, 4, 64) X(fillw, 5, 64) X(fillw, 6, 64) X(fillw, 7, 64) X(fillw, 8, 64)
// ... and one lane per request (denovo_fill_kernel.hpp): test library
#define FILL_LIST(X) X(fill, 2, 64) X(fill, 3, 64) X(fill, 4, 64) X(fill, 5, 64) X(fill, 6, 64) X(fill, 7, 64) X(fill, 8, 64)
// test library: kernel 1 by reads per lane, kernel 4 (settle / steady pipeline) by ploidy
#define V1_LIST(X) X(1) X(2) X(4) X(8) X(16)
#define LANE_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

#define SAMPLER_OBJ_(kind, k, g) mchap_obj_##kind##_##k##_##g
#define SAMPLER_OBJ(kind, k, g) SAMPLER_OBJ_(kind, k, g)
#define V1_OBJ_(r) mchap_obj_v1_##r
#define V1_OBJ(r) V1_OBJ_(r)
#define LANE_OBJ_(k) mchap_obj_lane_##k
#define LANE_OBJ(k) LANE_OBJ_(k)

#pragma GCC visibility push(hidden)
namespace mchap {

typedef int (*init_fn)(const double *ln, const double *ln_inv);
typedef int (*simt_launch_fn)(const SimtParams *, unsigned grid, size_t lds, hipStream_t);
typedef int (*stats_fn)(unsigned long long *out, int reset);  // the object's copy of the event counters (profiling builds, else null)

// the speculative sampler (kernel 3), the phased form's three variants (kernel 5), the lane-per-chain sampler (kernel 2), the two
// table completions
enum Variant { VAR_SPEC, VAR_PHASED, VAR_SBS, VAR_DEEP, VAR_SIMT, VAR_FILLW, VAR_FILL };
struct SpecInst {
  int variant, K, G;         // G: lanes per chain -- but for VAR_SIMT the bits of a haplotype word, 64 or 128 (SIMT_LIST)
  init_fn init;
  simt_launch_fn launch;
  simt_launch_fn launch_c;   // with decision contexts per genotype (phased, one chain per wavefront), else null
  simt_launch_fn launch_tw;  // a wavefront per replica of a temperature ladder (speculative, one chain per wavefront), else null
  stats_fn stats;
};

// kernel 1 and the lane pipeline (test library) launch with other arguments
struct V1Inst {
  int rpl;
  init_fn init;
  int (*launch)(const DenovoParams *, unsigned gx, unsigned gy, unsigned block, size_t lds, hipStream_t);
};
struct LaneInst {
  int K;
  init_fn init;
  int (*launch)(const SimtParams *, int lsh, int mode, unsigned grid, size_t lds, hipStream_t);  // mode < 0: the steady kernel; else the settling kernel with that mode (LANE_MODE_*)
  stats_fn stats;
};

}  // namespace mchap

// the coasting kernel of the phased sampler (coast_inst.hip): one object, no tables of its own.  wide != 0: a list of handed-back
// chains (few): COAST_NW_LIST wavefronts per chain, as many steps per sweep
extern "C" int mchap_coast_launch(const mchap::SimtParams *P, unsigned grid, int wide, hipStream_t stream);
#pragma GCC visibility pop
