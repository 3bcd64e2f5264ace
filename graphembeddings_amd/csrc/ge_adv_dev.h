// ge_adv_dev.h -- what the self-adversarial negative-sampling kernels share (ge_rotate_adv.hip: RotatE, ge_transx_adv.hip:
// TransE / TransH / TransD): the limit on K, the fp32 softplus and sigmoid, the softmax's scaled logit and the
// workgroup reductions of its three sums.  One workgroup of kBlock threads per row in both.
#pragma once
#include "ge_common.h"

namespace ge {

constexpr int kAdvMaxK = 1024;
constexpr int kWaves = kBlock / kWave;

// log(1 + e^x) = -log sigma(-x)
__device__ __forceinline__ float softplus_dev(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// sigma(x) in the form that never overflows
__device__ __forceinline__ float sigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// -alpha D, and 0 at alpha == 0 whatever D is (a distance that overflowed to inf keeps its uniform weight)
__device__ __forceinline__ float neg_scaled(float alpha, float D) { return alpha == 0.f ? 0.f : -alpha * D; }

// Sum / maximum over the workgroup, to every thread: an xor tree in each wave, then the four waves in order.  The
// leading barrier frees `red` of the previous reduction.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = group_sum<kWave>(v);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// lanes per team for a row of nvec VEC-wide chunks
inline int adv_lpt_for(int nvec) { return nvec <= 8 ? 8 : nvec <= 16 ? 16 : nvec <= 32 ? 32 : 64; }

}  // namespace ge
