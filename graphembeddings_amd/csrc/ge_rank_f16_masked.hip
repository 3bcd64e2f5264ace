// ge_rank_f16_masked.hip -- per-row candidate sets on the split-precision sweep (ge_rank_1vK_masked, ge_topk_1vK_masked):
// the MASKED instantiations of rank_f16_kernel (ge_rank_f16_kern.h) for ranks, ranks with stored losses and top-k, and
// the two kernels that build a mask on the device.  A translation unit of its own: the 45 instantiations compile beside
// ge_rank_f16.hip's, and the unmasked kernels stay the code they were.
//
// The mask: uint32 [n_sets][W], W = candidate_mask_words(K) = 4 words per 128-candidate tile -- word 4 ct + wn of a row
// is exactly the 32 candidates of slice wn of tile ct, what one wave of the sweep scores per block.  Row i of a call uses
// row row_set[i] (-1: every candidate).  Semantics: include/ge_hip.h.
#include "ge_rank_f16_kern.h"

namespace ge {
namespace {

// mask[s][w] bit b <- candidate w * 32 + b exists and its class is allowed in set s (allow: [n_sets][ceil(n_class / 32)])
__global__ __launch_bounds__(256) void mask_from_classes_kernel(const int32_t* __restrict__ cand_class, int64_t K,
                                                                const uint32_t* __restrict__ allow, int32_t n_sets,
                                                                int32_t n_class, int64_t W, uint32_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_sets * W) return;
  const int64_t s = i / W, w = i - s * W;
  const int64_t aw = ((int64_t)n_class + 31) / 32;
  uint32_t word = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t c = w * 32 + b;
    if (c >= K) break;
    const int32_t cls = cand_class[c];
    if (cls >= 0 && cls < n_class && ((allow[s * aw + (cls >> 5)] >> (cls & 31)) & 1u)) word |= 1u << b;
  }
  mask[i] = word;
}

// cells [M][2] = (set, position): the bit of every pair inside [0, n_sets) x [0, K) is set; the others are ignored
__global__ __launch_bounds__(256) void mask_from_cells_kernel(const int32_t* __restrict__ cells, int64_t M, int32_t n_sets,
                                                              int64_t K, int64_t W, uint32_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int32_t s = cells[2 * i], c = cells[2 * i + 1];
  if (s < 0 || s >= n_sets || c < 0 || c >= K) return;
  atomicOr(&mask[(int64_t)s * W + (c >> 5)], 1u << (c & 31));
}

// after topk_merge_kernel: a row whose set index is out of range is a bad row, -1 / NaN in every slot (its pool was empty)
__global__ __launch_bounds__(256) void topk_bad_set_rows_kernel(const int32_t* __restrict__ row_set, int64_t B, int32_t n_sets,
                                                                int k, int32_t* __restrict__ out_id, float* __restrict__ out_loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * k) return;
  const int32_t s = row_set[i / k];
  if (s < -1 || s >= n_sets) { out_id[i] = -1; out_loss[i] = __builtin_nanf(""); }
}

}  // namespace

int64_t candidate_mask_words(int64_t K) { return K <= 0 ? 0 : planes_slices(K); }

int mask_from_classes_launch(const int32_t* cand_class, int64_t K, const uint32_t* allow, int32_t n_sets, int32_t n_class,
                             uint32_t* mask, hipStream_t st) {
  const int64_t W = candidate_mask_words(K), n = (int64_t)n_sets * W;
  if (n == 0) return 0;
  if ((n + 255) / 256 > INT32_MAX) return GE_ENOTSUP;
  hipLaunchKernelGGL(mask_from_classes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cand_class, K, allow,
                     n_sets, n_class, W, mask);
  return launch_status();
}

int mask_from_cells_launch(const int32_t* cells, int64_t M, int32_t n_sets, int64_t K, uint32_t* mask, hipStream_t st) {
  const int64_t W = candidate_mask_words(K), n = (int64_t)n_sets * W;
  if (n == 0) return 0;
  if ((M + 255) / 256 > INT32_MAX) return GE_ENOTSUP;
  const hipError_t e = hipMemsetAsync(mask, 0, (size_t)n * sizeof(uint32_t), st);
  if (e != hipSuccess) return (int)e;
  if (M == 0) return 0;
  hipLaunchKernelGGL(mask_from_cells_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, cells, M, n_sets, K, W, mask);
  return launch_status();
}

// f16_sweep_launch and topk_f16_launch with candidate sets (a.scores_only and a.sweep_flags are 0): the route's
// conditions are asserted
int masked_rank_launch(const SweepArgs& a, const SetArgs& sets, const void* planes_ws, hipStream_t st) {
  assert(route_masked_rank(a.N, a.d, a.B, a.K, a.max_norm, table_mod16(a)).kernel == SweepRoute::F16);
  return f16_sweep_run<true>(a, &sets, planes_ws, st);
}

int masked_topk_launch(const SweepArgs& a, const TopkOut& t, const SetArgs& sets, const void* planes_ws, hipStream_t st) {
  assert(route_topk(a.N, a.d, a.B, a.K, a.max_norm, table_mod16(a), t.k, true).kernel == SweepRoute::F16);
  return topk_sweep_run<true>(a, t, &sets, planes_ws, st);
}

}  // namespace ge

