// ge_softmax.hip -- 1-vs-all softmax training of ComplEx (the "1vsAll" objective of Lacroix et al. 2018 in place of the
// hinge of holE.py:231): multiclass log-loss of the true candidate over ALL candidates, on the candidate GEMM of
// ge_1vk.hip (score_1vK_kernel) in exact fp32 (v_mfma_f32_32x32x2_f32).  No [B, K] array exists at any point: scores
// are recomputed tile by tile, flash-attention style.  No float atomics: every sum has one fixed order.
//
//   s_ij = Q'_i . C'_j        Q'_i = clip(fixed_i) o clip(rel_i) in score_1vK_kernel's staging form, C'_j = clip(cand_j)
//   z_ij = -scale * s_ij      (lower score = more plausible, as every evaluator ranks)
//   loss_i = logsumexp_j z_ij - z_i,true,      w_ij = dL/ds_ij = -scale * (softmax_j(z_ij) - [cand_j == true_i])
//
//   softmax_prepare_kernel   one wave per query / candidate: Q' [B, d], C' [K, d] (clipped, dense) and the match keys
//                            (true id of a valid row, candidate id of a valid candidate, -1 otherwise);
//   softmax_sweep_kernel     a fixed tile of 64 X rows against a range of 64-row Y tiles.  Per Y tile: S = X . Y^T (Y whole
//                            in LDS; X whole too up to d = 256, beyond that in 32-column chunks per Y tile), then
//       LSE    X = queries: running (max, sum) and z_true per row, one partial per (row, range);
//       GRAD   w -> LDS, G_X += W . Y (second GEMM, accumulators in registers): X = candidates over all queries gives
//              dL/dC'_j (straight into the candidates' gradient slots), X = queries over a candidate range dL/dQ'_i
//              (one partial per range);
//   softmax_merge_kernel     partials in range order, in double -> lse_i as the pair (max, log sum), loss_i, validity;
//   softmax_finish_kernel    one wave per slot: the clip derivative (alpha g + beta x, row_coef of ge_complex_dev.h) on
//                            the candidate rows; dL/dQ' (partials summed in range order) split into the fixed row's and
//                            the relation's gradients (two complex products, two clips); IndexedSlices written.
//
// The scalar x . g the clip's beta needs is a dot product in the finish kernel, not a second sum in the sweep.
#include "ge_common.h"
#include "ge_launch.h"

namespace ge {

using sm_f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kSmTile = 64;          // X and Y rows of a tile
constexpr int kSmChunk = 32;         // X columns staged at a time
constexpr int kSmLdx = kSmChunk + 1; // LDS row strides are odd: the 32 rows a half-wave reads fall in 32 banks
constexpr int kSmLdw = kSmTile + 1;
constexpr int kSmMaxSplit = 8;       // candidate ranges of the query-side sweeps
constexpr int kSmXresMaxDim = 256;   // up to here X and Y tiles fit whole in LDS together (149 KB with the W tile)

static inline int sm_col_blocks(int d) { return (d + 31) / 32; }
static inline int sm_ldy(int d) { return 32 * sm_col_blocks(d) + 1; }
static inline int64_t sm_tiles(int64_t n) { return (n + kSmTile - 1) / kSmTile; }
// candidate ranges: enough workgroups for the device at a small B, never more than kSmMaxSplit or than tiles
static inline int sm_split(int64_t B, int64_t K) {
  const int64_t tb = sm_tiles(B), tk = sm_tiles(K);
  int64_t s = 512 / tb;
  if (s < 1) s = 1;
  if (s > kSmMaxSplit) s = kSmMaxSplit;
  if (s > tk) s = tk;
  return (int)s;
}

SoftmaxWs softmax_ws(void* base, int64_t B, int64_t K, int32_t d) {
  SoftmaxWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  w.qp = ws_at<float>(base, take(sizeof(float) * (size_t)B * d));
  w.cp = ws_at<float>(base, take(sizeof(float) * (size_t)K * d));
  w.qkey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)B));
  w.ckey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)K));
  w.lse = ws_at<float>(base, take(sizeof(float) * 2 * (size_t)B));
  w.part = ws_at<float4>(base, take(sizeof(float4) * (size_t)B * kSmMaxSplit));
  w.gq = ws_at<float>(base, take(sizeof(float) * (size_t)B * d * kSmMaxSplit));
  w.bytes = off;
  return w;
}

// ------------------------------------------------------------------ prepare
__device__ __forceinline__ float sm_wave_sum(float v) { return group_sum<kWave>(v); }

__global__ __launch_bounds__(kBlock) void softmax_prepare_kernel(
    const float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ hr, int64_t B,
    const int32_t* __restrict__ true_id, const int32_t* __restrict__ cand, int64_t K, float max_norm, int cand_is_head,
    float* __restrict__ qp, float* __restrict__ cp, int32_t* __restrict__ qkey, int32_t* __restrict__ ckey) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  for (int64_t u = wave; u < B + K; u += nwaves) {      // (wave-uniform)
    if (u < B) {
      const int32_t f = hr[2 * u], r = hr[2 * u + 1], tr = true_id[u];
      const bool ok = f >= 0 && f < N && r >= 0 && r < N && tr >= 0 && tr < N;
      float* dst = qp + u * d;
      if (!ok) {
        for (int c = lane; c < d; c += kWave) dst[c] = 0.f;
        if (lane == 0) qkey[u] = -1;
        continue;
      }
      const float* fr = table + (int64_t)f * d;
      const float* rr = table + (int64_t)r * d;
      float ssf = 0.f, ssr = 0.f;
      for (int c = lane; c < d; c += kWave) { ssf += fr[c] * fr[c]; ssr += rr[c] * rr[c]; }
      float i0, i1;
      const float scf = clip_scale(sm_wave_sum(ssf), max_norm, i0), scr = clip_scale(sm_wave_sum(ssr), max_norm, i1);
      for (int c = lane; c < k; c += kWave) {
        const float a = fr[c] * scf, b = fr[k + c] * scf, e = rr[c] * scr, g = rr[k + c] * scr;
        if (!cand_is_head) { dst[c] = a * e - b * g; dst[k + c] = a * g + b * e; }     // q = h * r
        else               { dst[c] = e * a + g * b; dst[k + c] = e * b - g * a; }     // [Re(r conj t) | -Im(r conj t)]
      }
      if (lane == 0) qkey[u] = tr;
    } else {
      const int64_t j = u - B;
      const int32_t c_id = cand[j];
      const bool ok = c_id >= 0 && c_id < N;
      float* dst = cp + j * d;
      if (!ok) {
        for (int c = lane; c < d; c += kWave) dst[c] = 0.f;
        if (lane == 0) ckey[j] = -1;
        continue;
      }
      const float* cr = table + (int64_t)c_id * d;
      float ss = 0.f;
      for (int c = lane; c < d; c += kWave) ss += cr[c] * cr[c];
      float i0;
      const float sc = clip_scale(sm_wave_sum(ss), max_norm, i0);
      for (int c = lane; c < d; c += kWave) dst[c] = cr[c] * sc;
      if (lane == 0) ckey[j] = c_id;
    }
  }
}

// ------------------------------------------------------------------ sweep
// z = -scale * s as ONE rounded product in every sweep: the gradient sweeps subtract lse_i from the same bits the LSE
// sweep summed (contracted into an fma with the subtraction, z would differ from them by up to half an ulp of |z| --
// 1e-4 at |z| = 2000 --, which the exp turns into a relative error of p, and K = 1 would not give p = 1 exactly)
// (The empty asm makes the product a value of its own: no pragma or intrinsic to rely on.)
__device__ __forceinline__ float sm_logit(float scale, float s) {
  float z = -scale * s;
  asm volatile("" : "+v"(z));
  return z;
}

// MODE 0: LSE (X = queries).  MODE 1: GRAD.  XQ: X rows are the queries (Y the candidates), else the other way round.
// MAXCB: 32-column blocks of G a wave owns (row block w & 1, column blocks (w >> 1) + 2 n).
// Grid: x = X tiles, y = Y ranges of tiles_per_range tiles.  out: MODE 0 the partials [range][NX] (float4), MODE 1
// G [range][NX][d].
template <int MODE, bool XQ, int MAXCB>
__global__ __launch_bounds__(kBlock) void softmax_sweep_kernel(
    const float* __restrict__ xp, const int32_t* __restrict__ xkey, int64_t NX, const float* __restrict__ yp,
    const int32_t* __restrict__ ykey, int64_t NY, int d, float scale, const float* __restrict__ lse,
    int tiles_per_range, int xres, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ncb = (d + 31) >> 5, ldy = 32 * ncb + 1;
  float* Ys = smem;                                  // [64][ldy], columns [d, ldy) stay zero
  float* Xs = Ys + kSmTile * ldy;                    // xres: the X tile whole, [64][ldy]; else one chunk, [64][33]
  float* Ws = Xs + kSmTile * (xres ? ldy : kSmLdx);  // [64][65]
  int32_t* xk = reinterpret_cast<int32_t*>(Ws + kSmTile * kSmLdw);   // [64]
  int32_t* yk = xk + kSmTile;                        // [64]
  float* qm = reinterpret_cast<float*>(yk + kSmTile);                // [64] (max, log sum) of the tile's queries, X or Y side
  float* qs = qm + kSmTile;                          // [64]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w >> 1, wn = w & 1, li = lane & 31, lh = lane >> 5;
  const int64_t x0 = (int64_t)blockIdx.x * kSmTile;
  const int64_t ty0 = (int64_t)blockIdx.y * tiles_per_range;
  const int64_t ny_tiles = (NY + kSmTile - 1) / kSmTile;
  const int64_t ty1 = ty0 + tiles_per_range < ny_tiles ? ty0 + tiles_per_range : ny_tiles;
  const int d4 = d >> 2;
  const float ninf = -__builtin_inff();

  for (int i = t; i < kSmTile * (ldy - d); i += kBlock) Ys[(i / (ldy - d)) * ldy + d + i % (ldy - d)] = 0.f;
  if (t < kSmTile) {
    const int64_t x = x0 + t;
    xk[t] = x < NX ? xkey[x] : -1;
    if (MODE == 1 && XQ) { qm[t] = x < NX ? lse[x] : 0.f; qs[t] = x < NX ? lse[NX + x] : 0.f; }
  }

  if (xres) {                                        // the X tile once, as the Y tiles are staged
    for (int i = t; i < kSmTile * d4; i += kBlock) {
      const int row = i / d4, c4 = i - row * d4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (x0 + row < NX) v = *reinterpret_cast<const float4*>(xp + (x0 + row) * d + 4 * c4);
      float* dst = Xs + row * ldy + 4 * c4;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
  }
  sm_f32x16 g[MAXCB];
  if (MODE == 1) {
#pragma unroll
    for (int n = 0; n < MAXCB; ++n)
#pragma unroll
      for (int q = 0; q < 16; ++q) g[n][q] = 0.f;
  }
  // LSE: thread t owns row t >> 2 with its three neighbours (16 columns of a tile each)
  float run_m = ninf, run_s = 0.f, run_zt = 0.f, run_found = 0.f;

  for (int64_t ty = ty0; ty < ty1; ++ty) {
    const int64_t y0 = ty * kSmTile;
    __syncthreads();                                   // the previous tile's readers of Ys / Ws / yk are done
    for (int i = t; i < kSmTile * d4; i += kBlock) {
      const int row = i / d4, c4 = i - row * d4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y0 + row < NY) v = *reinterpret_cast<const float4*>(yp + (y0 + row) * d + 4 * c4);
      float* dst = Ys + row * ldy + 4 * c4;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    if (t < kSmTile) {
      const int64_t y = y0 + t;
      yk[t] = y < NY ? ykey[y] : -1;
      if (MODE == 1 && !XQ) { qm[t] = y < NY ? lse[y] : 0.f; qs[t] = y < NY ? lse[NY + y] : 0.f; }
    }
    // four independent chains over k (k mod 8 in {0,1}, {2,3}, {4,5}, {6,7}; d % 8 == 0), added pairwise at the end:
    // a quarter of the sequential chain's length per sum, and four MFMAs in flight instead of one dependent chain
    sm_f32x16 ac4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) ac4[c][q] = 0.f;
    if (xres) {                                      // (block-uniform) the same k order as the chunks: the same bits
      __syncthreads();
      const float* ap = Xs + (wm * 32 + li) * ldy + lh;
      const float* bp = Ys + (wn * 32 + li) * ldy + lh;
#pragma unroll 4
      for (int kk = 0; kk < d; kk += 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ac4[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 2 * c], bp[kk + 2 * c], ac4[c], 0, 0, 0);
      }
    } else {
    for (int kc = 0; kc < d; kc += kSmChunk) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {                    // 64 rows x 8 float4 = 512: two per thread
        const int i = t + kBlock * p, row = i >> 3, c = kc + 4 * (i & 7);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x0 + row < NX && c < d) v = *reinterpret_cast<const float4*>(xp + (x0 + row) * d + c);
        float* dst = Xs + row * kSmLdx + 4 * (i & 7);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      }
      __syncthreads();
      const int kn = d - kc < kSmChunk ? d - kc : kSmChunk;      // even: d % 8 == 0
      const float* ap = Xs + (wm * 32 + li) * kSmLdx + lh;
      const float* bp = Ys + (wn * 32 + li) * ldy + kc + lh;
      for (int kk = 0; kk < kn; kk += 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ac4[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 2 * c], bp[kk + 2 * c], ac4[c], 0, 0, 0);
      }
      __syncthreads();
    }
    }
    sm_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = (ac4[0][q] + ac4[1][q]) + (ac4[2][q] + ac4[3][q]);
    // S tile in C layout: column (Y) wn * 32 + li, rows (X) wm * 32 + (q & 3) + 8 (q >> 2) + 4 lh
    const int yl = wn * 32 + li;
    const int ykey_l = yk[yl];
    if (MODE == 0) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int xl = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
        Ws[xl * kSmLdw + yl] = ykey_l >= 0 ? sm_logit(scale, acc[q]) : ninf;
      }
      __syncthreads();
      const int row = t >> 2, part = t & 3;
      const int key = xk[row];
      float z[16];
      float m = ninf, zt = 0.f, found = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        z[j] = Ws[row * kSmLdw + 16 * part + j];
        m = fmaxf(m, z[j]);
        if (key >= 0 && yk[16 * part + j] == key) { zt = z[j]; found = 1.f; }
      }
      m = fmaxf(m, __shfl_xor(m, 1, kWave));
      m = fmaxf(m, __shfl_xor(m, 2, kWave));
      float s = 0.f;
      if (m > ninf) {
#pragma unroll
        for (int j = 0; j < 16; ++j) s += expf(z[j] - m);        // exp(-inf) = 0: an empty slot
      }
      s += __shfl_xor(s, 1, kWave); s += __shfl_xor(s, 2, kWave);
      zt += __shfl_xor(zt, 1, kWave); zt += __shfl_xor(zt, 2, kWave);
      found += __shfl_xor(found, 1, kWave); found += __shfl_xor(found, 2, kWave);
      if (m > ninf) {
        const float nm = fmaxf(run_m, m);
        run_s = run_s * expf(run_m - nm) + s * expf(m - nm);      // (run_m = -inf: run_s = 0 times exp(-inf) = 0)
        run_m = nm;
      }
      if (found > 0.f) { run_zt = zt; run_found = 1.f; }
    } else {
      const float m_y = XQ ? 0.f : qm[yl], s_y = XQ ? 0.f : qs[yl];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int xl = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
        const int xkey_l = xk[xl];
        float wv = 0.f;
        if (xkey_l >= 0 && ykey_l >= 0) {
          const float p = expf((sm_logit(scale, acc[q]) - (XQ ? qm[xl] : m_y)) - (XQ ? qs[xl] : s_y));
          wv = -scale * (p - (xkey_l == ykey_l ? 1.f : 0.f));
        }
        Ws[xl * kSmLdw + yl] = wv;
      }
      __syncthreads();
      // G[x][c] += sum_y W[x][y] Y[y][c]
      const float* ap = Ws + ((w & 1) * 32 + li) * kSmLdw + lh;
      const float* bp = Ys + lh * ldy + li;
      for (int kk = 0; kk < kSmTile; kk += 2) {
        const float a = ap[kk];
#pragma unroll
        for (int n = 0; n < MAXCB; ++n) {
          const int cb = (w >> 1) + 2 * n;
          if (cb < ncb) g[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[kk * ldy + 32 * cb], g[n], 0, 0, 0);
        }
      }
    }
  }

  if (MODE == 0) {
    const int row = t >> 2;
    if ((t & 3) == 0 && x0 + row < NX)
      reinterpret_cast<float4*>(out)[(int64_t)blockIdx.y * NX + x0 + row] = make_float4(run_m, run_s, run_zt, run_found);
  } else {
    float* dst = out + (int64_t)blockIdx.y * NX * d;
#pragma unroll
    for (int n = 0; n < MAXCB; ++n) {
      const int cb = (w >> 1) + 2 * n;
      const int c = 32 * cb + li;
      if (cb >= ncb || c >= d) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t x = x0 + (w & 1) * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
        if (x < NX) dst[x * d + c] = g[n][q];
      }
    }
  }
}

// ------------------------------------------------------------------ merge
__global__ __launch_bounds__(kBlock) void softmax_merge_kernel(
    const float4* __restrict__ part, int n_ranges, int64_t B, int32_t* __restrict__ qkey, float* __restrict__ lse,
    float* __restrict__ loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float ninf = -__builtin_inff();
  // one thread a row and at most eight partials: the merge, the logarithm and the loss's last sum are taken in double and
  // rounded once, so the loss carries the sweep's fp32 errors only
  float m = ninf, zt = 0.f;
  double s = 0.0;
  bool found = false;
  for (int r = 0; r < n_ranges; ++r) {
    const float4 p = part[(int64_t)r * B + i];
    if (p.x > ninf) {
      const float nm = fmaxf(m, p.x);
      s = (m > ninf ? s * exp((double)m - (double)nm) : 0.0) + (double)p.y * exp((double)p.x - (double)nm);
      m = nm;
    }
    if (p.w > 0.f) { zt = p.z; found = true; }
  }
  const bool ok = qkey[i] >= 0 && found;
  // lse_i stays the pair (m, log s): z - m is exact for the logits that matter (within a factor 2 of m) and neither
  // p = exp((z - m) - log s) nor the loss carries the rounding of m + log s at the magnitude of m
  const double ls = log(s);
  lse[i] = ok ? m : 0.f;
  lse[B + i] = ok ? (float)ls : 0.f;
  loss[i] = ok ? (float)(((double)m - (double)zt) + ls) : __builtin_nanf("");
  if (!ok) qkey[i] = -1;                               // an invalid row contributes to no gradient
}

// ------------------------------------------------------------------ finish
// -lr * (the gradient through the clip of row x, given g = dL/d clip(x)): alpha g + beta x of row_coef
// (ge_complex_dev.h), with x . g taken here; ss = |x|^2.
__device__ __forceinline__ void sm_clip_back(float ss, float xg, float max_norm, float& alpha, float& beta) {
  float inv;
  clip_scale(ss, max_norm, inv);
  const bool active = inv <= 1.0f / max_norm;
  alpha = active ? max_norm * inv : 1.f;
  beta = active ? -max_norm * xg * inv * inv * inv : 0.f;
}

__global__ __launch_bounds__(kBlock) void softmax_finish_kernel(
    const float* __restrict__ table, int d, const int32_t* __restrict__ hr, int64_t B, int64_t K, float max_norm, float lr,
    int cand_is_head, const int32_t* __restrict__ qkey, const int32_t* __restrict__ ckey, const float* __restrict__ gq,
    int n_ranges, int32_t* __restrict__ grad_idx, float* __restrict__ grad_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  const float neg_lr = -lr;
  for (int64_t u = wave; u < K + B; u += nwaves) {      // (wave-uniform)
    if (u < K) {
      // candidate slot u: grad_val[u] holds dL/dC'_u
      float* gv = grad_val + u * d;
      const int32_t id = ckey[u];
      if (lane == 0) grad_idx[u] = id;
      if (id < 0) {
        for (int c = lane; c < d; c += kWave) gv[c] = 0.f;
        continue;
      }
      const float* x = table + (int64_t)id * d;
      float ss = 0.f, xg = 0.f;
      for (int c = lane; c < d; c += kWave) { ss += x[c] * x[c]; xg += x[c] * gv[c]; }
      float alpha, beta;
      sm_clip_back(sm_wave_sum(ss), sm_wave_sum(xg), max_norm, alpha, beta);
      for (int c = lane; c < d; c += kWave) {
        const float gr = alpha * gv[c] + beta * x[c];
        gv[c] = neg_lr * gr;
      }
    } else {
      const int64_t i = u - K;
      float* gf = grad_val + (K + 2 * i) * d;
      float* gr = gf + d;
      const bool ok = qkey[i] >= 0;
      if (lane == 0) { grad_idx[K + 2 * i] = ok ? hr[2 * i] : -1; grad_idx[K + 2 * i + 1] = ok ? hr[2 * i + 1] : -1; }
      if (!ok) {
        for (int c = lane; c < 2 * d; c += kWave) gf[c] = 0.f;
        continue;
      }
      const float* f = table + (int64_t)hr[2 * i] * d;
      const float* r = table + (int64_t)hr[2 * i + 1] * d;
      float ssf = 0.f, ssr = 0.f;
      for (int c = lane; c < d; c += kWave) { ssf += f[c] * f[c]; ssr += r[c] * r[c]; }
      ssf = sm_wave_sum(ssf); ssr = sm_wave_sum(ssr);
      float i0, i1;
      const float scf = clip_scale(ssf, max_norm, i0), scr = clip_scale(ssr, max_norm, i1);
      // pass 1: the gradients wrt the CLIPPED rows into the output rows, and the two dot products
      float fg = 0.f, rg = 0.f;
      for (int c = lane; c < k; c += kWave) {
        float Gre = 0.f, Gim = 0.f;
        for (int s = 0; s < n_ranges; ++s) {
          const float* gp = gq + ((int64_t)s * B + i) * d;
          Gre += gp[c]; Gim += gp[k + c];
        }
        const float a = f[c] * scf, b = f[k + c] * scf, e = r[c] * scr, h = r[k + c] * scr;
        float fa, fb, ra, rb;
        if (!cand_is_head) {     // Q' = (a + ib)(e + ih)
          fa = Gre * e + Gim * h; fb = Gim * e - Gre * h;
          ra = Gre * a + Gim * b; rb = Gim * a - Gre * b;
        } else {                 // Q' = [e a + h b | e b - h a], (a, b) the fixed tail
          fa = Gre * e - Gim * h; fb = Gre * h + Gim * e;
          ra = Gre * a + Gim * b; rb = Gre * b - Gim * a;
        }
        gf[c] = fa; gf[k + c] = fb; gr[c] = ra; gr[k + c] = rb;
        fg += f[c] * fa + f[k + c] * fb;
        rg += r[c] * ra + r[k + c] * rb;
      }
      float af, bf, ar, br;
      sm_clip_back(ssf, sm_wave_sum(fg), max_norm, af, bf);
      sm_clip_back(ssr, sm_wave_sum(rg), max_norm, ar, br);
      // pass 2: each lane rereads the columns it wrote
      for (int c = lane; c < k; c += kWave) {
        const float v0 = af * gf[c] + bf * f[c], v1 = af * gf[k + c] + bf * f[k + c];
        const float v2 = ar * gr[c] + br * r[c], v3 = ar * gr[k + c] + br * r[k + c];
        gf[c] = neg_lr * v0; gf[k + c] = neg_lr * v1; gr[c] = neg_lr * v2; gr[k + c] = neg_lr * v3;
      }
    }
  }
}

// ------------------------------------------------------------------ host
size_t softmax_ws_bytes(int64_t B, int64_t K, int32_t d) { return softmax_ws(nullptr, B, K, d).bytes; }

template <int MODE, bool XQ>
static int sm_sweep(const float* xp, const int32_t* xkey, int64_t NX, const float* yp, const int32_t* ykey, int64_t NY, int d,
                    float scale, const float* lse, int n_ranges, float* out, hipStream_t st) {
  const int64_t ty = sm_tiles(NY);
  const int tpr = (int)((ty + n_ranges - 1) / n_ranges);
  const int xres = d <= kSmXresMaxDim;
  const size_t lds = sizeof(float) * ((size_t)kSmTile * sm_ldy(d) + kSmTile * (xres ? sm_ldy(d) : kSmLdx) + kSmTile * kSmLdw +
                                      4 * kSmTile);
  const dim3 grid((unsigned)sm_tiles(NX), (unsigned)n_ranges);
  auto go = [&](auto kern) -> int {
    if (int rc = lds_opt_in(kern)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, xp, xkey, NX, yp, ykey, NY, d, scale, lse, tpr, xres, out);
    return launch_status();
  };
  if constexpr (MODE == 0) return go(softmax_sweep_kernel<MODE, XQ, 1>);
  else switch ((sm_col_blocks(d) + 1) / 2) {
    case 1: return go(softmax_sweep_kernel<MODE, XQ, 1>);
    case 2: return go(softmax_sweep_kernel<MODE, XQ, 2>);
    case 3: return go(softmax_sweep_kernel<MODE, XQ, 3>);
    case 4: return go(softmax_sweep_kernel<MODE, XQ, 4>);
    default: return go(softmax_sweep_kernel<MODE, XQ, 5>);
  }
}

int softmax_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                   const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head, float* loss,
                   int32_t* grad_idx, float* grad_val, void* workspace, hipStream_t st) {
  assert(d % 8 == 0 && d >= 8 && d <= kRankMaxDim);
  const SoftmaxWs w = softmax_ws(workspace, B, K, d);
  hipLaunchKernelGGL(softmax_prepare_kernel, dim3(grid_for(B + K, kBlock / kWave)), dim3(kBlock), 0, st, table, N, d, hr, B,
                     true_id, cand, K, max_norm, cand_is_head, w.qp, w.cp, w.qkey, w.ckey);
  if (int rc = launch_status()) return rc;
  const int ns = sm_split(B, K);
  if (int rc = sm_sweep<0, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, nullptr, ns, reinterpret_cast<float*>(w.part), st))
    return rc;
  hipLaunchKernelGGL(softmax_merge_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, w.part, ns, B,
                     w.qkey, w.lse, loss);
  if (int rc = launch_status()) return rc;
  if (!grad_idx) return 0;
  // dL/dC' over all queries, straight into the candidates' slots; dL/dQ' per candidate range
  if (int rc = sm_sweep<1, false>(w.cp, w.ckey, K, w.qp, w.qkey, B, d, scale, w.lse, 1, grad_val, st)) return rc;
  if (int rc = sm_sweep<1, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, w.lse, ns, w.gq, st)) return rc;
  hipLaunchKernelGGL(softmax_finish_kernel, dim3(grid_for(B + K, kBlock / kWave)), dim3(kBlock), 0, st, table, d, hr, B, K,
                     max_norm, lr, cand_is_head, w.qkey, w.ckey, w.gq, ns, grad_idx, grad_val);
  return launch_status();
}

}  // namespace ge
