// ge_sweep_route.h -- which kernel serves a ComplEx / HolE 1-vs-K candidate sweep, and the size formulas that decision
// rests on: route_rank (ge_rank_1vK_planes, ge_rank_1vK_vs_loss), route_score (ge_complex_score_1vK), route_masked_rank
// (ge_rank_1vK_masked) and route_topk (ge_topk_1vK_planes, ge_topk_1vK_masked), with the top-k workspace (topk_splits,
// topk_ws_bytes) and its grid limit (topk_grid_ok).  The ONE place that decides: ge_rank.hip, ge_rank_pipe.hip,
// ge_rank_f16.hip, ge_rank_f16_masked.hip and ge_1vk.hip switch on the route, or assert it, and launch; none refuses a
// shape for another to catch.  Host only, plain C++17: tested without a GPU (tests/sweep_route_dump.cpp).
// The route as a table: DESIGN.md section 4.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ge_hip.h"

namespace ge {

constexpr int kRB = 128;                   // test rows per workgroup, candidates per tile
constexpr size_t kLdsMax = 160 * 1024;     // LDS of a CU
constexpr int kRankMaxDim = 288;           // the split-precision sweep's Q planes fill the LDS at 18 k blocks
constexpr int kRankMaxDimF32 = 232;        // the fp32 kernels: Q (128 x (d+1) floats) + two candidate chunks must fit the LDS

// ---- the split-precision sweep (ge_rank_f16.hip): embedding_dim % 8 == 0 in 56 ... 288 (k blocks 4 ... 18),
// max_norm <= 8 (|q sa (1/d)| <= 2 max_norm^2, |t clip| <= max_norm sqrt(d/2): x 2^8 inside fp16)
constexpr bool f16_dim_ok(int d) { return d % 8 == 0 && d >= 56 && d <= kRankMaxDim; }
constexpr bool f16_sweep_ok(int d, float max_norm) { return f16_dim_ok(d) && max_norm <= 8.f; }

// its candidate planes (layout: ge_f16_dev.h, ge_rank_f16.hip)
constexpr int kSL = 32;                    // candidates per slice of `planes` = one wave's columns
constexpr int kOpHalves = kSL * 16;        // one operand fetch of one wave in `planes`: [32 candidates][16 columns], 1 KiB
constexpr int64_t planes_slices(int64_t K) { return 4 * ((K + kRB - 1) / kRB); }   // whole 128-candidate tiles
constexpr int64_t pos_bytes(int64_t N) { return (N * (int64_t)sizeof(int32_t) + 255) / 256 * 256; }

// bytes of the planes workspace of a K-candidate sweep over an N-row table: the entity -> position map, then the fp16
// planes.  0: no split-precision sweep for this shape -- the dim, or planes of 2^32 bytes and more (the sweep addresses
// them with 32-bit byte offsets: about 5.1 M candidates at d = 200).
constexpr int64_t rank_planes_bytes(int64_t N, int32_t d, int64_t K) {
  if (!f16_dim_ok(d) || N <= 0 || K <= 0) return 0;
  const int64_t plane_bytes = planes_slices(K) * ((d + 15) / 16) * 2 * kOpHalves * 2 /* fp16 */;
  return plane_bytes >= ((int64_t)1 << 32) ? 0 : pos_bytes(N) + plane_bytes;
}

// ---- the fp32 pipeline (ge_rank_pipe.hip), candidate chunk width CW
constexpr int pipe_ldb(int cw) { return cw + 1; }   // odd LDS row stride
template <int CW>
constexpr size_t pipe_lds_bytes(int d) {           // PipeLds: A, Bs, sA / sB / eT | lohi | bm | skip, tI
  return sizeof(float) * ((size_t)kRB * (d + 1) + 2 * kRB * pipe_ldb(CW) + 3 * kRB) + 2 * sizeof(float) * kRB +
         sizeof(unsigned) * kRB * 4 + sizeof(int) * 2 * kRB;
}

// ---- score_1vK_fullk_kernel: two 64-row operands over the whole (4-padded) k range
constexpr int fullk_kp(int d) { return (d / 2 + 3) & ~3; }
constexpr size_t fullk_lds(int d) { return sizeof(float) * (size_t)(2 * 64 * (2 * fullk_kp(d) + 1) + 128); }

// ---- the route
struct SweepRoute {
  enum Kernel { None, F16, Pipe40, Pipe32, Pipe24, RankF32, ScoreTileF16, ScoreTile, ScoreFullK, ScoreBasic };
  int kernel;   // None: nothing to launch, the entry returns `status`
  int status;   // 0 or GE_E*
};

constexpr int pipe_cw(int kernel) { return kernel == SweepRoute::Pipe40 ? 40 : kernel == SweepRoute::Pipe32 ? 32 : 24; }
constexpr int64_t sweep_tiles(int64_t n) { return (n + kRB - 1) / kRB; }
constexpr bool sweep_is_big(int64_t B, int64_t K) { return sweep_tiles(B) * sweep_tiles(K) >= 512; }

// The main road of ranks and big score sweeps: F16, else Pipe<CW>, else None.  Tile counts: the kernels' 32-bit tile
// arithmetic (for F16's candidate tiles the planes limit implies it: 2^32 bytes / 8 KiB a tile and k block < 2^19 tiles).
inline int route_main_road(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm) {
  const int64_t n_rb = sweep_tiles(B), n_ct = sweep_tiles(K);
  if (f16_sweep_ok(d, max_norm) && rank_planes_bytes(N, d, K) != 0 && n_rb <= INT32_MAX / 8) return SweepRoute::F16;
  const bool tiles_ok = n_rb <= INT32_MAX / 2 && n_ct <= INT32_MAX / 2;
  // the first chunk width that divides d decides: when its LDS does not fit, no narrower one is tried
  if (d % 40 == 0) return tiles_ok && pipe_lds_bytes<40>(d) <= kLdsMax ? SweepRoute::Pipe40 : SweepRoute::None;
  if (d % 32 == 0) return tiles_ok && pipe_lds_bytes<32>(d) <= kLdsMax ? SweepRoute::Pipe32 : SweepRoute::None;
  if (d % 24 == 0) return tiles_ok && pipe_lds_bytes<24>(d) <= kLdsMax ? SweepRoute::Pipe24 : SweepRoute::None;
  return SweepRoute::None;
}

inline SweepRoute route_rank(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm, int table_addr_mod_16) {
  if (d <= 0 || (d & 1)) return {SweepRoute::None, GE_EINVAL};
  if (d % 8 != 0 || d > kRankMaxDim) return {SweepRoute::None, GE_ENOTSUP};   // 16-byte candidate loads, 8-float tail
  if (table_addr_mod_16 != 0) return {SweepRoute::None, GE_EINVAL};
  if (B == 0 || K == 0) return {SweepRoute::None, 0};
  if (const int kernel = route_main_road(N, d, B, K, max_norm)) return {kernel, 0};
  if (d <= kRankMaxDimF32 && sweep_tiles(B) <= 65535) return {SweepRoute::RankF32, 0};   // grid.y = row blocks
  return {SweepRoute::None, GE_ENOTSUP};
}

inline SweepRoute route_score(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm, int table_addr_mod_16) {
  if (d <= 0 || (d & 1)) return {SweepRoute::None, GE_EINVAL};
  if (B == 0 || K == 0) return {SweepRoute::None, 0};
  const bool big = sweep_is_big(B, K), aligned = table_addr_mod_16 == 0;
  if (big && aligned)
    if (const int kernel = route_main_road(N, d, B, K, max_norm)) return {kernel, 0};
  const int bm = big ? 128 : 64;                       // the tile kernels' grid: (candidate tiles, row tiles)
  if ((B + bm - 1) / bm > 65535 || (K + bm - 1) / bm > INT32_MAX) return {SweepRoute::None, GE_ENOTSUP};
  if (!big) {
    if (aligned && f16_sweep_ok(d, max_norm) && d <= 224) return {SweepRoute::ScoreTileF16, 0};
    if (aligned && d % 8 == 0 && d <= 256) return {SweepRoute::ScoreTile, 0};
    if (fullk_lds(d) <= 150 * 1024) return {SweepRoute::ScoreFullK, 0};
  }
  return {SweepRoute::ScoreBasic, 0};
}

// ---- the top-k sweep and the candidate-set (masked) forms: F16 is their one kernel, so no other road.
// In order: the split-precision range, addressable planes and -- masked -- 32-bit row-block arithmetic, GE_ENOTSUP; then
// -- masked -- the table's 16-byte alignment, GE_EINVAL.  The unmasked top-k asks neither of the last two.
inline int f16_only_status(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm, int table_addr_mod_16, bool masked) {
  if (!f16_sweep_ok(d, max_norm) || rank_planes_bytes(N, d, K) == 0) return GE_ENOTSUP;
  if (masked && sweep_tiles(B) > INT32_MAX / 8) return GE_ENOTSUP;
  return masked && table_addr_mod_16 != 0 ? GE_EINVAL : 0;
}

// (ge_rank_1vK_masked returns for B == 0 or K == 0 before it asks)
inline SweepRoute route_masked_rank(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm, int table_addr_mod_16) {
  if (const int rc = f16_only_status(N, d, B, K, max_norm, table_addr_mod_16, true)) return {SweepRoute::None, rc};
  if (B == 0) return {SweepRoute::None, 0};
  return {SweepRoute::F16, 0};
}

constexpr int kTopkMaxK = 128;             // the longest list of the top-k sweeps, ComplEx / HolE and translation alike
// a top-k pool past kp entries is cut back to k after a tile (>= 32 appends apart)
constexpr int topk_kp(int k) { return (k + 95) / 64 * 64; }   // k + 32 rounded up: 64 for k <= 32, 192 for k = 128

inline SweepRoute route_topk(int64_t N, int32_t d, int64_t B, int64_t K, float max_norm, int table_addr_mod_16, int32_t k,
                             bool masked) {
  if (const int rc = f16_only_status(N, d, B, K, max_norm, table_addr_mod_16, masked)) return {SweepRoute::None, rc};
  if (k < 1) return {SweepRoute::None, GE_EINVAL};
  if (k > kTopkMaxK) return {SweepRoute::None, GE_ENOTSUP};
  if (B == 0) return {SweepRoute::None, 0};
  return {SweepRoute::F16, 0};
}

// Top-k: workgroups per row block.  With fewer than 256 row blocks (one workgroup per CU of the MI355X) the row
// blocks' candidates are cut into ranges until there are about 256 workgroups (one query against 1.2 M candidates: 256
// ranges of 37 tiles); the partial lists meet in topk_merge_kernel.  A function of (B, K) alone, so that the workspace is.
// B > 0.
constexpr int64_t topk_splits(int64_t B, int64_t K) {
  const int64_t n_rb = sweep_tiles(B), n_ct = sweep_tiles(K);
  if (n_rb >= 256) return 1;
  const int64_t want = (256 + n_rb - 1) / n_rb, ns = n_ct < want ? n_ct : want;
  return ns < 1 ? 1 : ns;
}

constexpr int64_t topk_ws_rows(int64_t n_rb, int64_t K, int32_t k) {      // bytes for n_rb full row blocks
  return n_rb * kRB * topk_splits(n_rb * kRB, K) * (topk_kp(k) + 128 + k) * (int64_t)sizeof(uint64_t);
}

// Workspace of a top-k over B rows and K candidates: the pools, [B][n_split][kp + 128] keys, and the partial lists,
// [B][n_split][k].  Taken as the largest need of any B' <= B (the ranges shrink as B grows), so that the
// size is monotone in B, K and k.
constexpr size_t topk_ws_bytes(int64_t B, int64_t K, int32_t k) {
  if (B <= 0 || K <= 0 || k < 1 || k > kTopkMaxK) return 0;
  const int64_t n_rb = sweep_tiles(B);
  int64_t need = topk_ws_rows(n_rb, K, k);
  for (int64_t r = 1; r < n_rb && r < 256; ++r) {
    const int64_t rows = topk_ws_rows(r, K, k);
    if (rows > need) need = rows;
  }
  return (size_t)need + 256;
}

// the top-k's grid, row blocks x candidate ranges.  The launcher asks it behind the workspace's pointer and size, so a
// call too large for the grid answers GE_ENOMEM first when its workspace is short.
constexpr bool topk_grid_ok(int64_t B, int64_t K) { return sweep_tiles(B) * topk_splits(B, K) <= INT32_MAX; }

}  // namespace ge
