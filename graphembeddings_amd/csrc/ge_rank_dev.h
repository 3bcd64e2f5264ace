// ge_rank_dev.h -- what the ranking kernels (ge_rank.hip: the fp32 kernel; ge_rank_pipe.hip: the fp32 pipeline;
// ge_rank_f16.hip: the split-precision sweep) share.  Which of them runs: ge_sweep_route.h.
#pragma once
#include "ge_common.h"
#include "ge_sweep_route.h"   // kRB

#ifndef GE_PIPE_GRID_M
#define GE_PIPE_GRID_M 2   // workgroups per CU (each CU holds one at a time): equal shares, two rounds
#endif

namespace ge {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// sigmoid for the ranking epilogue: 4 VALU instructions (v_exp_f32, v_rcp_f32; ~2 ulp), used for EVERY loss the
// ranking kernels form -- candidates and true entities alike -- so comparisons are self-consistent; within 1e-6 of
// sigmoidf_dev, well inside the 1e-5 score bar.
__device__ __forceinline__ float rank_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

}  // namespace ge
