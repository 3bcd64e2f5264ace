// ge_rank_dev.h -- what the two ranking kernels (ge_rank.hip: any embedding_dim % 8 == 0; ge_rank_pipe.hip:
// the software-pipelined sweep for embedding_dim % 40, % 32 or % 24 == 0) share.
#pragma once
#include "ge_common.h"

namespace ge {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kRB = 128;          // test rows per workgroup, candidates per tile

// sigmoid for the ranking epilogue: 4 VALU instructions (v_exp_f32, v_rcp_f32; ~2 ulp), used for EVERY loss the
// ranking kernels form -- candidates and true entities alike -- so comparisons are self-consistent; within 1e-6 of
// sigmoidf_dev, well inside the 1e-5 score bar.
__device__ __forceinline__ float rank_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

}  // namespace ge
