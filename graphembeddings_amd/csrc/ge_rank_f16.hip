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

}  // namespace

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

// The F16 of route_rank / route_score, and of route_topk without candidate sets: the route's conditions are asserted
int f16_sweep_launch(const SweepArgs& a, const void* planes_ws, hipStream_t st) {
  assert(f16_sweep_ok(a.d, a.max_norm) && rank_planes_bytes(a.N, a.d, a.K) != 0);   // route_main_road
  return f16_sweep_run<false>(a, nullptr, planes_ws, st);
}

int topk_f16_launch(const SweepArgs& a, const TopkOut& t, const void* planes_ws, hipStream_t st) {
  assert(route_topk(a.N, a.d, a.B, a.K, a.max_norm, 0, t.k, false).kernel == SweepRoute::F16);
  return topk_sweep_run<false>(a, t, nullptr, planes_ws, st);
}

}  // namespace ge
