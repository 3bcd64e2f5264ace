// ge_transx_apply.h -- the apply stage of the translation family's steps, shared by ge_transx.hip (TransE / TransH /
// TransD), ge_rotate.hip (RotatE's hinge step) and ge_rotate_adv.hip (RotatE's self-adversarial step, whose per-row losses
// take the hinge terms' place): the sorted (key, slot) list summed per destination row in slot order and applied, as SGD
// (ApplyArgs) or AdaGrad (AdaArgs).
//   pass 1: one wave per window of kWin sorted positions sums each run of equal keys in slot order; a run that is a
//           whole segment (its row's every slot) is applied at once, a run cut by a window edge is stored as a partial.
//   pass 2: one wave per window that holds the head of a cut segment adds the following windows' partials in window
//           order and applies; its last block sums the hinge terms into the batch loss.
// A gradient slot is d floats wide in both planes whatever its key.  The entity tables are d wide; the relation tables
// are dr wide (dr <= d; a multiple of VEC): a relation key applies columns [0, dr) and drops the rest of its slot, which
// the gradient kernel need not have written.  TransE / TransH / TransD pass dr = d.
#pragma once
#include "ge_common.h"

namespace ge {

constexpr int kWin = 32;                  // sorted slots per wave in the apply's first pass

template <int VEC>
__device__ __forceinline__ void ld(const float* __restrict__ row, int j, float (&v)[VEC]) { load_vec<VEC>(row + j * VEC, v); }

struct ApplyArgs {
  float* ent; float* rel; float* ent2; float* rel2;
  int64_t E, R; int d; int64_t n;               // n sorted slots: 5B (hinge), (K+3)B (self-adversarial)
  const uint32_t* keys; const uint32_t* slots;
  const float* g0; const float* g1;
  float* part;                                  // [nwin][2 (first, last run)][2 (plane)][d]
  float lr;
  int dr;                                       // width of a relation row (rel, rel2 and their accumulators)
};

// chunk j of key k lies past the key's row: a relation key's columns [dr, d)
__device__ __forceinline__ bool past_row(const ApplyArgs& a, uint32_t k, int j, int vec) {
  return k >= (uint32_t)a.E && j * vec >= a.dr;
}

template <int VEC>
__device__ __forceinline__ void apply_row(const ApplyArgs& a, uint32_t k, int j, const float (&s0)[VEC], const float (&s1)[VEC]) {
  if (past_row(a, k, j, VEC)) return;
  const bool is_ent = k < (uint32_t)a.E;
  float* t0 = is_ent ? a.ent + (int64_t)k * a.d : a.rel + ((int64_t)k - a.E) * a.dr;
  float* t1 = is_ent ? (a.ent2 ? a.ent2 + (int64_t)k * a.d : nullptr) : (a.rel2 ? a.rel2 + ((int64_t)k - a.E) * a.dr : nullptr);
  float v[VEC];
  ld<VEC>(t0, j, v);
#pragma unroll
  for (int q = 0; q < VEC; ++q) v[q] -= a.lr * s0[q];
  store_vec<VEC>(t0 + j * VEC, v);
  if (t1) {
    ld<VEC>(t1, j, v);
#pragma unroll
    for (int q = 0; q < VEC; ++q) v[q] -= a.lr * s1[q];
    store_vec<VEC>(t1 + j * VEC, v);
  }
}

__device__ __forceinline__ bool has_plane1(const ApplyArgs& a, uint32_t k) {
  return k < (uint32_t)a.E ? a.ent2 != nullptr : a.rel2 != nullptr;
}

// The AdaGrad apply: ApplyArgs plus one accumulator per table (acc_ent2 / acc_rel2 null where ent2 / rel2 are).
struct AdaArgs : ApplyArgs {
  float* acc_ent; float* acc_rel; float* acc_ent2; float* acc_rel2;
};

// One row's AdaGrad update from its complete sums.  The table row and the accumulator row of both planes are requested
// before any arithmetic; then one read-modify-write per array.  Plane 1's arrays are touched only where the key has one.
template <int VEC>
__device__ __forceinline__ void apply_row(const AdaArgs& a, uint32_t k, int j, const float (&s0)[VEC], const float (&s1)[VEC]) {
  if (past_row(a, k, j, VEC)) return;
  const bool is_ent = k < (uint32_t)a.E;
  const int64_t off = (is_ent ? (int64_t)k * a.d : ((int64_t)k - a.E) * a.dr) + (int64_t)j * VEC;
  float* t0 = (is_ent ? a.ent : a.rel) + off;
  float* c0 = (is_ent ? a.acc_ent : a.acc_rel) + off;
  const bool p1 = has_plane1(a, k);
  float* t1 = p1 ? (is_ent ? a.ent2 : a.rel2) + off : nullptr;
  float* c1 = p1 ? (is_ent ? a.acc_ent2 : a.acc_rel2) + off : nullptr;
  float v0[VEC], b0[VEC], v1[VEC], b1[VEC];
  load_vec<VEC>(t0, v0); load_vec<VEC>(c0, b0);
  if (p1) { load_vec<VEC>(t1, v1); load_vec<VEC>(c1, b1); }
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    b0[q] = b0[q] + s0[q] * s0[q];
    v0[q] -= a.lr * s0[q] / sqrtf(b0[q]);
  }
  store_vec<VEC>(c0, b0); store_vec<VEC>(t0, v0);
  if (p1) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      b1[q] = b1[q] + s1[q] * s1[q];
      v1[q] -= a.lr * s1[q] / sqrtf(b1[q]);
    }
    store_vec<VEC>(c1, b1); store_vec<VEC>(t1, v1);
  }
}

// Args: ApplyArgs (SGD) or AdaArgs (AdaGrad); it selects apply_row and nothing else.
template <int VEC, class Args>
__global__ __launch_bounds__(kBlock) void transx_apply_runs_kernel(Args a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwin = (a.n + kWin - 1) / kWin;
  if (c >= nwin) return;
  const uint32_t sentinel = (uint32_t)(a.E + a.R);
  const int64_t w0 = c * kWin, w1 = min(w0 + kWin, a.n);
  const int nvec = a.d / VEC;
  for (int j = lane; j < nvec; j += kWave) {
    float s0[VEC], s1[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) s0[q] = s1[q] = 0.f;
    int64_t rs = w0;                                    // start of the current run
    for (int64_t p = w0; p < w1; ++p) {
      const uint32_t k = a.keys[p];
      if (k >= sentinel) break;                         // inactive slots sort last
      if (past_row(a, k, j, VEC)) break;                // relation keys sort after the entities': none below has column j
      const int64_t slot = a.slots[p];
      const bool p1 = has_plane1(a, k);
      float v[VEC];
      ld<VEC>(a.g0 + slot * a.d, j, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) s0[q] += v[q];
      if (p1) {
        ld<VEC>(a.g1 + slot * a.d, j, v);
#pragma unroll
        for (int q = 0; q < VEC; ++q) s1[q] += v[q];
      }
      const bool seg_end = p + 1 == a.n || a.keys[p + 1] != k;
      if (seg_end || p + 1 == w1) {
        const bool head = rs == 0 || a.keys[rs - 1] != k;
        if (head && seg_end) {
          apply_row<VEC>(a, k, j, s0, s1);
        } else {
          float* dst = a.part + ((c * 2 + (head ? 1 : 0)) * 2) * a.d;
          store_vec<VEC>(dst + j * VEC, s0);
          if (p1) store_vec<VEC>(dst + a.d + j * VEC, s1);
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) s0[q] = s1[q] = 0.f;
        rs = p + 1;
      }
    }
  }
}

// Cut segments (one per window that holds the head of a segment running past its end), then the batch loss.
template <int VEC, class Args>
__global__ __launch_bounds__(kBlock) void transx_apply_cut_kernel(Args a, const float* __restrict__ hinge,
                                                                  int64_t B, float* __restrict__ loss) {
  const int64_t nwin = (a.n + kWin - 1) / kWin;
  if (blockIdx.x == gridDim.x - 1) {                  // the loss block: fixed-order sum of the hinge terms
    __shared__ float red[kBlock];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += kBlock) s += hinge[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0];
    return;
  }
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  if (c >= nwin) return;
  const uint32_t sentinel = (uint32_t)(a.E + a.R);
  const int64_t w0 = c * kWin, q = min(w0 + kWin, a.n) - 1;
  const uint32_t k = a.keys[q];
  if (k >= sentinel || q + 1 >= a.n || a.keys[q + 1] != k) return;      // the last run ends inside this window
  if (a.keys[w0] == k && w0 > 0 && a.keys[w0 - 1] == k) return;       // ...or its head lies in an earlier window
  const bool p1 = has_plane1(a, k);
  const int nvec = a.d / VEC;
  for (int j = lane; j < nvec; j += kWave) {
    if (past_row(a, k, j, VEC)) break;                  // the partials hold nothing there
    float s0[VEC], s1[VEC], v[VEC];
    const float* src = a.part + ((c * 2 + 1) * 2) * a.d;
    ld<VEC>(src, j, s0);
    if (p1) ld<VEC>(src + a.d, j, s1);
    else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) s1[e] = 0.f;
    }
    for (int64_t cc = c + 1; cc < nwin && a.keys[cc * kWin] == k; ++cc) {
      const float* pp = a.part + ((cc * 2 + 0) * 2) * a.d;
      ld<VEC>(pp, j, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s0[e] += v[e];
      if (p1) {
        ld<VEC>(pp + a.d, j, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s1[e] += v[e];
      }
    }
    apply_row<VEC>(a, k, j, s0, s1);
  }
}

template <int VEC, class Args>
static void launch_apply(const Args& a, int grid_a, const float* hinge, int64_t B, float* loss, hipStream_t st) {
  hipLaunchKernelGGL((transx_apply_runs_kernel<VEC, Args>), dim3(grid_a), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL((transx_apply_cut_kernel<VEC, Args>), dim3(grid_a + 1), dim3(kBlock), 0, st, a, hinge, B, loss);
}

// the grid of both apply kernels (the cut kernel adds the loss block): one wave per window of n sorted slots
inline int apply_grid(int64_t n) {
  const int64_t nwin = (n + kWin - 1) / kWin;
  const int wpb = kBlock / kWave;
  return (int)((nwin + wpb - 1) / wpb);
}

inline unsigned key_bits(int64_t E, int64_t R) { return sort_key_bits(E + R); }   // the sentinel E + R

}  // namespace ge
