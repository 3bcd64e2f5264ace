// ge_trans_dev.h -- what the translation models' sweeps (ge_transx_rank.hip, ge_transx_relrank.hip) share on the
// device: the distance term, the sequential dot, the preparation kernels, and the host helper that runs them.
#pragma once
#include "ge_common.h"
#include "ge_trans.h"

namespace ge {
namespace {

constexpr int kTile = 128;               // ge_known_cells' tile edge
constexpr float kNormEps = 1e-12f;

__device__ __forceinline__ float dist_acc(bool l1, float acc, float u) { return l1 ? acc + fabsf(u) : fmaf(u, u, acc); }

__device__ __forceinline__ float dot_seq(const float* __restrict__ a, const float* __restrict__ b, int n) {
  float s = 0.f;
  for (int k = 0; k < n; ++k) s = fmaf(a[k], b[k], s);
  return s;
}

// TransH: n^_r = n_r * rsqrt(max(n_r . n_r, 1e-12)), one thread per relation.
__global__ __launch_bounds__(kBlock) void trans_nhat_kernel(const float* __restrict__ normal, int64_t R, int d,
                                                            float* __restrict__ nhat) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* n = normal + r * d;
  const float inv = rsqrtf(fmaxf(dot_seq(n, n, d), kNormEps));
  for (int k = 0; k < d; ++k) nhat[r * d + k] = n[k] * inv;
}

// TransD: A_c = e_c . e_p,c, one thread per entity.  (A template, so that a source that never asks for A_c carries no
// copy of the kernel.)
template <class T>
__global__ __launch_bounds__(kBlock) void trans_transfer_dot_kernel(const T* __restrict__ ent,
                                                                    const T* __restrict__ ent2, int64_t E, int d,
                                                                    T* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) A[e] = dot_seq(ent + e * d, ent2 + e * d, d);
}

// bytes of the workspace block trans_prepare fills: n^ [R, dq] (TransH), A [E] (TransD, with_A), else none
inline size_t trans_aux_bytes(const TransModel& m, bool with_A) {
  if (m.model == kTransH) return align_up(sizeof(float) * (size_t)m.R * m.dq, 256);
  if (m.model == kTransD && with_A) return align_up(sizeof(float) * (size_t)m.E, 256);
  return 0;
}

// The preparation stage of a sweep: m's tables as the kernels read them, with TransH's n^ or (WITH_A: the entity
// sweeps; relation prediction forms e . e_p per row instead) TransD's A_c launched into aux_ws, trans_aux_bytes long.
template <bool WITH_A>
TransTables trans_prepare(const TransModel& m, void* aux_ws, hipStream_t st) {
  TransTables T{m.ent, m.rel, nullptr, nullptr, nullptr, m.E, m.R, m.dE, m.dq};
  if (m.model == kTransH) {
    hipLaunchKernelGGL(trans_nhat_kernel, dim3((unsigned)((T.R + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, m.normal,
                       T.R, T.dq, (float*)aux_ws);
    T.aux = (const float*)aux_ws;
  } else if (m.model == kTransD) {
    T.aux = m.rel_transfer;
    T.ent2 = m.ent_transfer;
    if constexpr (WITH_A) {
      hipLaunchKernelGGL(trans_transfer_dot_kernel<float>, dim3((unsigned)((T.E + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                         T.ent, T.ent2, T.E, T.dE, (float*)aux_ws);
      T.A = (const float*)aux_ws;
    }
  } else if (m.model == kTransR) {
    T.aux = m.rel_matrix;
  }
  return T;
}

}  // namespace
}  // namespace ge
