// ge_rank_f16.hip -- the split-precision link-prediction sweep (holE.py:427-472, 564-575; semantics in ge_rank.hip):
// f16 MFMAs on pre-split candidate planes, eight free-running waves per workgroup (two per SIMD).  F16 of
// ge_sweep_route.h: the first choice of every rank sweep and big score sweep it can serve, the one kernel of the top-k.
//
// Why this shape (tools/probes/mfma_gap_probe.hip -> profiles/r03_mfma_gap_probe.txt; s_memtime stamps per phase and
// ablated builds, recorded in DESIGN.md section 9):
//   * with one wave per SIMD the shadow of a v_mfma_f32_32x32x16_f16 hides four or five INDEPENDENT VALU instructions
//     and next to nothing of the rank epilogue's compare -> scalar -> v_addc / v_writelane chains: cutting the epilogue
//     into the gaps of the next tile's MFMAs gained nothing (measured).  A second wave on the SIMD hides it -- if it
//     is in the OTHER phase;
//   * eight waves in one barrier domain (all in the MFMA loop, then all in the epilogue) gained 9 %; two groups of
//     four waves half a barrier cycle apart 15 %: with twelve workgroup barriers per tile the MFMA pipe still idled
//     half the time (an ablated loop with nothing but MFMAs and barriers ran at 53 % of the pipe);
//   * so nothing in the sweep is shared between waves any more.  Each wave owns a 64 x 32 block of the 128 x 128 tile:
//     its candidate operands come straight from global memory (the planes are L2-resident: every CU walks the candidate
//     tiles in the same order at the same pace) into registers in MFMA layout, three k blocks ahead; its bits go to a
//     bitmap of its own; it counts its own rows and looks up its own known cells.  No barrier between the row
//     block's set-up and its end: the two waves of a SIMD drift apart and one's epilogue runs under the other's MFMAs;
//   * splitting a candidate row into fp16 planes (norm, clip scale, 2 x cvt_pkrtz per pair) was half of the sweep's
//     VALU work and was repeated for every block of 128 test rows: it is a pre-pass (rank_planes_launch) whose output
//     -- `planes`, 1 KiB per (32 candidates, 16 columns, plane), exactly one operand fetch of one wave -- the sweep
//     only loads.
//
// x * 2^8 = hi + mid with two fp16 values (round toward zero, so mid has hi's sign) is exact to 22 bits, and
//     q . t  =  2^-16 (qh.th + qh.tm + qm.th)  +  O(2^-22) per product
// accumulated in fp32: three f16 MFMAs per 16-wide k block.  Q (pre-multiplied by the rows' clip scales) sits in LDS
// as two fp16 planes for the whole row block.  The kernel is compiled per number of k blocks (embedding_dim 56 ... 288,
// any multiple of 8); embedding_dim itself is a run-time value.
// Epilogue: raw scores against a bracket of the true candidate's raw score, bits into a row-major bitmap by
// v_writelane, the exact fp32 comparison (id tie-break) only for scores inside the bracket -- the outcome equals
// comparing the sigmoids everywhere.
#include "ge_rank_f16_kern.h"

namespace ge {
namespace {

// ---- the pre-pass: candidate planes.  Slice S = 32 candidates, k block kb = 16 columns:
//   planes[((S * kKB + kb) * 2 + plane) * 32 * 16 + row * 16 + column]   fp16
// = high halves / remainders of cand row * clip scale * 2^8 (0 behind embedding_dim; NaN for a bad id or a row behind K):
// 1 KiB per (slice, k block, plane) = one operand fetch of one wave, lane (row, half) reading its 16 bytes in place.
template <int KKB>
__global__ __launch_bounds__(256) void rank_planes_kernel(const float* __restrict__ table, int64_t N, int d,
                                                          const int32_t* __restrict__ cand, int64_t K, float max_norm,
                                                          int spec, _Float16* __restrict__ planes) {
  constexpr int kChunks = HCfg<KKB>::kChunks;
  const int srow = threadIdx.x >> 2, qt = threadIdx.x & 3;       // 64 candidates a workgroup, four threads a row
  const int64_t pos = (int64_t)blockIdx.x * 64 + srow;
  const int32_t id = pos < K ? cand[pos] : -1;
  const bool bad = id < 0 || id >= N;
  const float* row = table + (int64_t)(bad ? 0 : id) * d;
  float4 r[kChunks][2];
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int col = min(c * 32 + qt * 8, d - 8);                 // clamped into the row, zeroed below
    r[c][0] = *reinterpret_cast<const float4*>(row + col);
    r[c][1] = *reinterpret_cast<const float4*>(row + col + 4);
  }
  f2 ss2 = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const bool in = c * 32 + qt * 8 < d;                         // (embedding_dim % 8 == 0: all eight or none)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const f2 xy = in ? f2{r[c][v].x, r[c][v].y} : f2{0.f, 0.f}, zw = in ? f2{r[c][v].z, r[c][v].w} : f2{0.f, 0.f};
      ss2 = __builtin_elementwise_fma(xy, xy, ss2);
      ss2 = __builtin_elementwise_fma(zw, zw, ss2);
    }
  }
  float ss = ss2.x + ss2.y;
  ss += __shfl_xor(ss, 1, kWave);
  ss += __shfl_xor(ss, 2, kWave);
  // spectral HolE rows: |x|^2 = (2 sum - X_0^2 - X_k^2) / d; the two real bins sit at columns 0 and d/2
  if (spec) {
    const float x_dc = row[0], x_ny = row[d >> 1];
    ss = (2.f * ss - x_dc * x_dc - x_ny * x_ny) / (float)d;
  }
  float inv;
  // t * clip(t) * 2^8: |t clip| <= max_norm, or max_norm sqrt(d/2) for one bin of a spectral row -- no fp16 overflow
  // for max_norm <= 8 whatever the table holds
  const float scale = bad ? __builtin_nanf("") : clip_scale(ss, max_norm, inv) * kQScale;
  _Float16* dst = planes + (pos >> 5) * (int64_t)KKB * 2 * kOpHalves + (pos & 31) * 16 + (qt & 1) * 8;
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int kb = 2 * c + (qt >> 1);                            // this thread's eight columns: half of k block kb
    if (kb >= KKB) continue;
    const bool in = bad || c * 32 + qt * 8 < d;                  // (a bad row is NaN everywhere)
    const float x[8] = {r[c][0].x, r[c][0].y, r[c][0].z, r[c][0].w, r[c][1].x, r[c][1].y, r[c][1].z, r[c][1].w};
    h8 hi, mid;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h2 a, b;
      h_split(in ? x[2 * i] * scale : 0.f, in ? x[2 * i + 1] * scale : 0.f, a, b);
      hi[2 * i] = a.x; hi[2 * i + 1] = a.y; mid[2 * i] = b.x; mid[2 * i + 1] = b.y;
    }
    *reinterpret_cast<h8*>(dst + kb * 2 * kOpHalves) = hi;
    *reinterpret_cast<h8*>(dst + kb * 2 * kOpHalves + kOpHalves) = mid;
  }
}

template <int KKB>
int f16_launch_kkb(const SweepArgs& a, const void* planes_ws, hipStream_t st) {
  const int64_t n_rb = (a.B + kRB - 1) / kRB, n_ct = (a.K + kRB - 1) / kRB;
  assert(n_ct <= INT32_MAX / 8 && n_rb <= INT32_MAX / 8);        // route_main_road
  const int64_t n_tiles = n_rb * n_ct;
  const int64_t grid = std::min<int64_t>(n_tiles, GE_PIPE_GRID_M * (int64_t)cu_count());
  const int32_t* pos_of = reinterpret_cast<const int32_t*>(planes_ws);
  const _Float16* planes = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(planes_ws) + pos_bytes(a.N));
  auto go = [&](auto kern) -> int {
    if (int rc = lds_opt_in(kern)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlk), h_lds_bytes<KKB>(), st, a.table, a.N, a.d, a.hr, a.B, a.true_id,
                       a.cand, a.K, a.max_norm, a.cand_is_head, a.known_off, a.known_rc, a.raw_cnt, a.skip_cnt, a.true_loss,
                       a.scores_out, (int)n_ct, n_tiles, a.spec, a.sweep_flags, pos_of, planes, TopkArgs{});
    return launch_status();
  };
  if (a.scores_only) return go(rank_f16_kernel<KKB, 2>);
  if (a.scores_out) return go(rank_f16_kernel<KKB, 1>);
  return go(rank_f16_kernel<KKB, 0>);
}

}  // namespace

// ---- top-k: workgroups per row block.  With fewer than 256 row blocks (one workgroup per CU of the MI355X) the row
// blocks' candidates are cut into ranges until there are about 256 workgroups (one query against 1.2 M candidates: 256
// ranges of 37 tiles); the partial lists meet in topk_merge_kernel.  A function of (B, K) alone, so that the workspace is.
int64_t topk_splits(int64_t B, int64_t K) {
  const int64_t n_rb = (B + kRB - 1) / kRB, n_ct = (K + kRB - 1) / kRB;
  if (n_rb >= 256) return 1;
  return std::max<int64_t>(1, std::min<int64_t>(n_ct, (256 + n_rb - 1) / n_rb));
}

int64_t topk_ws_rows(int64_t n_rb, int64_t K, int32_t k) {      // bytes for n_rb full row blocks
  const int64_t ns = topk_splits(n_rb * kRB, K);
  return n_rb * kRB * ns * (topk_kp(k) + 128 + k) * (int64_t)sizeof(u64);
}

// planes_ws (rank_planes_bytes, 256-byte aligned) <- the entity -> position map, then the candidates' fp16 planes
int rank_planes_launch(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, float max_norm, int spec,
                       void* planes_ws, hipStream_t st) {
  if (!f16_sweep_ok(d, max_norm) || (K > 0 && N > 0 && rank_planes_bytes(N, d, K) == 0)) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(planes_ws) % 256 != 0 || reinterpret_cast<uintptr_t>(table) % 16 != 0) return GE_EINVAL;
  if (K <= 0 || N <= 0) return 0;
  int32_t* pos_of = reinterpret_cast<int32_t*>(planes_ws);
  _Float16* planes = reinterpret_cast<_Float16*>(reinterpret_cast<char*>(planes_ws) + pos_bytes(N));
  hipError_t e = hipMemsetAsync(pos_of, 0xff, (size_t)N * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rank_pos_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, cand, K, N, pos_of);
  const int64_t n_blocks = planes_slices(K) / 2;                // 64 candidates a workgroup (< 2^20: the planes' 2^32 bytes)
#define GE_CALL(KKB)                                                                                                   \
  hipLaunchKernelGGL(rank_planes_kernel<KKB>, dim3((unsigned)n_blocks), dim3(256), 0, st, table, N, d, cand, K, max_norm, \
                     spec, planes);                                                                                    \
  return launch_status()
  GE_KKB_SWITCH(d, GE_CALL)
#undef GE_CALL
}

// The split-precision sweep.  planes_ws: the candidates' planes from rank_planes_launch for the same (table, cand,
// max_norm, spec), or NULL.
int f16_sweep_launch(const SweepArgs& a, const void* planes_ws, hipStream_t st) {
  assert(f16_sweep_ok(a.d, a.max_norm) && rank_planes_bytes(a.N, a.d, a.K) != 0);   // route_main_road
  static_assert(h_lds_bytes<18>() <= kLdsMax, "LDS of the largest instantiation");
  return with_planes(a.table, a.N, a.d, a.cand, a.K, a.max_norm, a.spec, planes_ws, st, [&](const void* ws) -> int {
#define GE_CALL(KKB) return f16_launch_kkb<KKB>(a, ws, st)
    GE_KKB_SWITCH(a.d, GE_CALL)
#undef GE_CALL
  });
}

int topk_max_k() { return kTopkMaxK; }

// Workspace of a top-k over B rows and K candidates: the pools, [B][n_split][kp + 128] keys, and the partial lists,
// [B][n_split][k].  Taken as the largest need of any B' <= B (the ranges shrink as B grows), so that the
// size is monotone in B, K and k.
size_t topk_ws_bytes(int64_t B, int64_t K, int32_t k) {
  if (B <= 0 || K <= 0 || k < 1 || k > kTopkMaxK) return 0;
  const int64_t n_rb = (B + kRB - 1) / kRB;
  int64_t need = topk_ws_rows(n_rb, K, k);
  for (int64_t r = 1; r < std::min<int64_t>(n_rb, 256); ++r) need = std::max(need, topk_ws_rows(r, K, k));
  return (size_t)need + 256;
}

// The top-k sweep (rank_f16_kernel MODE 3, grid row blocks x candidate ranges), then the merge of the partial lists.  The same planes
// and Q staging as the rank sweep, so the losses are MODE 1's.
int topk_f16_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand, int64_t K,
                    float max_norm, int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, int32_t k,
                    int32_t* out_id, float* out_loss, int spec, const void* planes_ws, void* workspace,
                    size_t workspace_bytes, hipStream_t st) {
  if (!f16_sweep_ok(d, max_norm) || rank_planes_bytes(N, d, K) == 0) return GE_ENOTSUP;   // (incl. planes beyond 32-bit offsets)
  if (k < 1) return GE_EINVAL;
  if (k > kTopkMaxK) return GE_ENOTSUP;
  if (B == 0) return 0;
  if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < topk_ws_bytes(B, K, k)) return GE_ENOMEM;
  static_assert(topk_lds_bytes<18>() <= kLdsMax, "LDS of the largest top-k instantiation");
  const int64_t n_rb = (B + kRB - 1) / kRB, n_ct = (K + kRB - 1) / kRB;   // (n_ct < INT32_MAX / 8: the planes' 2^32 bytes)
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
  return with_planes(table, N, d, cand, K, max_norm, spec, planes_ws, st, [&](const void* ws) -> int {
    const int32_t* pos_of = reinterpret_cast<const int32_t*>(ws);
    const _Float16* planes = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(ws) + pos_bytes(N));
    auto sweep = [&]() -> int {
#define GE_CALL(KKB)                                                                                                  \
  {                                                                                                                   \
    auto kern = rank_f16_kernel<KKB, 3>;                                                                              \
    if (int rc = lds_opt_in(kern)) return rc;                                                                         \
    hipLaunchKernelGGL(kern, dim3((unsigned)n_rb, (unsigned)ns), dim3(kBlk), topk_lds_bytes<KKB>(), st, table, N, d, hr, B,   \
                       nullptr, cand, K, max_norm, cand_is_head, known_off, known_rc, nullptr, nullptr, nullptr,      \
                       nullptr, (int)n_ct, n_rb * n_ct, spec, 0, pos_of, planes, tk);                                 \
    return launch_status();                                                                                           \
  }
      GE_KKB_SWITCH(d, GE_CALL)
#undef GE_CALL
    };
    const int rc = sweep();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, hr, B, N, tk);
    return launch_status();
  });
}

}  // namespace ge
