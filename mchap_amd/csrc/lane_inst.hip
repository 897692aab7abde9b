// One ploidy of the steady-state pipeline (denovo_lane_kernel.hpp: settling kernel + steady kernel) per object file
// (-DLANE_K=..), compiled in parallel with the other sampler objects; see spec_inst.hip.
#include "denovo_lane_kernel.hpp"
#include "sampler_inst.hpp"

// mode < 0: the steady kernel; else the settling kernel with that mode (LANE_MODE_*)
static int launch(const mchap::SimtParams *P, int lsh, int mode, unsigned grid, size_t lds, hipStream_t stream) {
  if (mode < 0) return mchap::sampler_launch(mchap::denovo_steady_kernel<LANE_K>, dim3(grid), dim3(64), lds, stream, *P, lsh);
  return mchap::sampler_launch(mchap::denovo_settle_kernel<LANE_K>, dim3(grid), dim3(64), lds, stream, *P, lsh, mode);
}

SAMPLER_DESCRIPTOR(mchap::LaneInst, LANE_OBJ(LANE_K), LANE_K, mchap::sampler_init, launch, SAMPLER_STATS)
