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

MaskedTopkArgs masked_args(const TopkArgs& tk, const int32_t* row_set, const uint32_t* mask, int32_t n_sets) {
  MaskedTopkArgs m;
  static_cast<TopkArgs&>(m) = tk;
  m.row_set = row_set;
  m.mask = mask;
  m.n_sets = n_sets;
  return m;
}

template <int KKB>
int masked_launch_kkb(const SweepArgs& a, const MaskedTopkArgs& mk, const void* planes_ws, hipStream_t st) {
  const int64_t n_rb = (a.B + kRB - 1) / kRB, n_ct = (a.K + kRB - 1) / kRB;
  const int64_t n_tiles = n_rb * n_ct;
  const int64_t grid = std::min<int64_t>(n_tiles, GE_PIPE_GRID_M * (int64_t)cu_count());
  const int32_t* pos_of = reinterpret_cast<const int32_t*>(planes_ws);
  const _Float16* planes = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(planes_ws) + pos_bytes(a.N));
  auto go = [&](auto kern) -> int {
    if (int rc = lds_opt_in(kern)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlk), h_lds_bytes<KKB>() + kMaskLdsBytes, st, a.table, a.N, a.d, a.hr,
                       a.B, a.true_id, a.cand, a.K, a.max_norm, a.cand_is_head, a.known_off, a.known_rc, a.raw_cnt, a.skip_cnt,
                       a.true_loss, a.scores_out, (int)n_ct, n_tiles, a.spec, a.sweep_flags, pos_of, planes, mk);
    return launch_status();
  };
  if (a.scores_out) return go(rank_f16_kernel<KKB, 1, true>);
  return go(rank_f16_kernel<KKB, 0, true>);
}

// what both masked sweeps ask of the shape: the split-precision range, planes within 32-bit offsets, 32-bit tile counts
bool masked_shape_ok(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm) {
  return f16_sweep_ok(d, max_norm) && rank_planes_bytes(N, d, K) != 0 && sweep_tiles(B) <= INT32_MAX / 8;
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

// The rank sweep of f16_sweep_launch with candidate sets (a.scores_only and a.sweep_flags are 0).
int masked_rank_launch(const SweepArgs& a, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                       const void* planes_ws, hipStream_t st) {
  if (!masked_shape_ok(a.N, a.d, a.B, a.K, a.max_norm)) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(a.table) % 16 != 0) return GE_EINVAL;
  static_assert(h_lds_bytes<18>() + kMaskLdsBytes <= kLdsMax, "LDS of the largest masked instantiation");
  const MaskedTopkArgs mk = masked_args(TopkArgs{}, row_set, mask, n_sets);
  return with_planes(a.table, a.N, a.d, a.cand, a.K, a.max_norm, a.spec, planes_ws, st, [&](const void* ws) -> int {
#define GE_CALL(KKB) return masked_launch_kkb<KKB>(a, mk, ws, st)
    GE_KKB_SWITCH(a.d, GE_CALL)
#undef GE_CALL
  });
}

// topk_f16_launch with candidate sets: the same workspace, grid and merge.
int masked_topk_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand, int64_t K,
                       float max_norm, int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, int32_t k,
                       int32_t* out_id, float* out_loss, int spec, const int32_t* row_set, const uint32_t* mask,
                       int32_t n_sets, const void* planes_ws, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!masked_shape_ok(N, d, B, K, max_norm)) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(table) % 16 != 0) return GE_EINVAL;
  if (k < 1) return GE_EINVAL;
  if (k > kTopkMaxK) return GE_ENOTSUP;
  if (B == 0) return 0;
  if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < topk_ws_bytes(B, K, k)) return GE_ENOMEM;
  static_assert(topk_lds_bytes<18>() + kMaskLdsBytes <= kLdsMax, "LDS of the largest masked top-k instantiation");
  const int64_t n_rb = (B + kRB - 1) / kRB, n_ct = (K + kRB - 1) / kRB;
  const int64_t ns = topk_splits(B, K);
  if (n_rb * ns > INT32_MAX) return GE_ENOTSUP;
  TopkArgs tk;
  tk.k = k;
  tk.cap = topk_kp(k) + 128;
  tk.n_split = (int)ns;
  tk.pool = reinterpret_cast<u64*>(workspace);
  tk.part = tk.pool + B * ns * tk.cap;
  tk.out_id = out_id;
  tk.out_loss = out_loss;
  const MaskedTopkArgs mk = masked_args(tk, row_set, mask, n_sets);
  return with_planes(table, N, d, cand, K, max_norm, spec, planes_ws, st, [&](const void* ws) -> int {
    const int32_t* pos_of = reinterpret_cast<const int32_t*>(ws);
    const _Float16* planes = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(ws) + pos_bytes(N));
    auto sweep = [&]() -> int {
#define GE_CALL(KKB)                                                                                                  \
  {                                                                                                                   \
    auto kern = rank_f16_kernel<KKB, 3, true>;                                                                        \
    if (int rc = lds_opt_in(kern)) return rc;                                                                         \
    hipLaunchKernelGGL(kern, dim3((unsigned)n_rb, (unsigned)ns), dim3(kBlk), topk_lds_bytes<KKB>() + kMaskLdsBytes, st, \
                       table, N, d, hr, B, nullptr, cand, K, max_norm, cand_is_head, known_off, known_rc, nullptr,    \
                       nullptr, nullptr, nullptr, (int)n_ct, n_rb * n_ct, spec, 0, pos_of, planes, mk);               \
    return launch_status();                                                                                           \
  }
      GE_KKB_SWITCH(d, GE_CALL)
#undef GE_CALL
    };
    const int rc = sweep();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, hr, B, N, tk);
    hipLaunchKernelGGL(topk_bad_set_rows_kernel, dim3((unsigned)((B * k + 255) / 256)), dim3(256), 0, st, row_set, B, n_sets,
                       k, out_id, out_loss);
    return launch_status();
  });
}

}  // namespace ge
