// ge_softmax_kern.h -- the sweep kernel of the softmax objectives and what its launchers share: one template, instantiated
// by ge_softmax.hip (1-vs-all: the true entity is one of the candidates), by ge_softmax_sampled.hip (SAMPLED: the true
// entity has a logit of its own and every candidate slot that holds it is left out of the row's softmax) and by
// ge_softmax_masked.hip (MASKED: 1-vs-all over the candidate positions the row's set admits), each in a translation unit
// of its own so that none's instantiations depend on another's being there.
#pragma once
#include "ge_common.h"
#include "ge_launch.h"
#include "ge_softmax_route.h"   // kSm*, sm_tiles, sm_split, sm_maxcb, sm_plan: the launch arithmetic, host only

namespace ge {

using sm_f32x16 = __attribute__((ext_vector_type(16))) float;

// What a MASKED sweep takes beside the operands (all null / zero otherwise): set [queries] the rows' set ids, mask
// [n_sets][W] in the format of ge_candidate_mask_words (W a multiple of 4: both words of a 64-candidate tile are in
// bounds), live [query tiles][live_words] one bit per (query tile, candidate tile), bit ct & 31 of word ct >> 5: a pair
// whose bit is clear is skipped.
struct SmMaskArgs { const int32_t* set; const uint32_t* mask; const uint32_t* live; int64_t W; int32_t n_sets; int32_t live_words; };
// (sm_live_words(K), the words per query tile of the live bitmap: ge_softmax_route.h)

__device__ __forceinline__ float sm_wave_sum(float v) { return group_sum<kWave>(v); }

// z = -scale * s as ONE rounded product in every sweep: the gradient sweeps subtract lse_i from the same bits the LSE
// sweep summed (contracted into an fma with the subtraction, z would differ from them by up to half an ulp of |z| --
// 1e-4 at |z| = 2000 --, which the exp turns into a relative error of p, and K = 1 would not give p = 1 exactly)
// (The empty asm makes the product a value of its own: no pragma or intrinsic to rely on.)
__device__ __forceinline__ float sm_logit(float scale, float s) {
  float z = -scale * s;
  asm volatile("" : "+v"(z));
  return z;
}

// -lr * (the gradient through the clip of row x, given g = dL/d clip(x)): alpha g + beta x of row_coef
// (ge_complex_dev.h), with x . g taken by the caller; ss = |x|^2.
__device__ __forceinline__ void sm_clip_back(float ss, float xg, float max_norm, float& alpha, float& beta) {
  float inv;
  clip_scale(ss, max_norm, inv);
  const bool active = inv <= 1.0f / max_norm;
  alpha = active ? max_norm * inv : 1.f;
  beta = active ? -max_norm * xg * inv * inv * inv : 0.f;
}

// MODE 0: LSE (X = queries).  MODE 1: GRAD.  XQ: X rows are the queries (Y the candidates), else the other way round.
// MAXCB: 32-column blocks of G a wave owns (row block w & 1, column blocks (w >> 1) + 2 n).
// SAMPLED: a pair whose keys match is no term of the softmax (LSE: its logit is -inf and no z_true is recorded -- the
// partial's third word is the Y row of the maximum instead, as int bits; GRAD: w = 0); the true entity's own term is the
// merge and finish kernels' business.
// MASKED (never with SAMPLED): row i's softmax runs over the candidate POSITIONS its set admits (set id -1: all).  The two
// mask words of every query row of the tile for the current candidate tile are staged in LDS; LSE: an inadmissible logit
// is -inf before the maximum, the sum and the key match (an inadmissible true candidate is never `found`); GRAD: w = 0.
// A (query tile, candidate tile) pair whose live bit is clear is skipped before the first barrier: block-uniform, and it
// would have contributed -inf logits / +0 products only.
// Grid: x = X tiles, y = Y ranges of tiles_per_range tiles.  out: MODE 0 the partials [range][NX] (float4), MODE 1
// G [range][NX][d].
template <int MODE, bool XQ, int MAXCB, bool SAMPLED, bool MASKED>
__global__ __launch_bounds__(kBlock) void softmax_sweep_kernel(
    const float* __restrict__ xp, const int32_t* __restrict__ xkey, int64_t NX, const float* __restrict__ yp,
    const int32_t* __restrict__ ykey, int64_t NY, int d, float scale, const float* __restrict__ lse,
    int tiles_per_range, int xres, float* __restrict__ out, SmMaskArgs mk) {
  static_assert(!(MASKED && SAMPLED), "the sampled objective has no candidate sets");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ncb = (d + 31) >> 5, ldy = 32 * ncb + 1;
  float* Ys = smem;                                  // [64][ldy], columns [d, ldy) stay zero
  float* Xs = Ys + kSmTile * ldy;                    // xres: the X tile whole, [64][ldy]; else one chunk, [64][33]
  float* Ws = Xs + kSmTile * (xres ? ldy : kSmLdx);  // [64][65]
  int32_t* xk = reinterpret_cast<int32_t*>(Ws + kSmTile * kSmLdw);   // [64]
  int32_t* yk = xk + kSmTile;                        // [64]
  float* qm = reinterpret_cast<float*>(yk + kSmTile);                // [64] (max, log sum) of the tile's queries, X or Y side
  float* qs = qm + kSmTile;                          // [64]
  int32_t* qset = reinterpret_cast<int32_t*>(qs + kSmTile);          // MASKED: [64] set ids of the X queries (XQ)
  uint32_t* mw = reinterpret_cast<uint32_t*>(qset + kSmTile);        // MASKED: [64][2] a query's words of the candidate tile
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
    if constexpr (MASKED && XQ) {                      // an id outside [0, n_sets) never indexes the mask (its row's key is -1)
      const int32_t sid = x < NX ? mk.set[x] : -1;
      qset[t] = sid >= 0 && sid < mk.n_sets ? sid : -1;
    }
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
  int run_arg = -1;                                    // SAMPLED: the candidate the running maximum belongs to

  for (int64_t ty = ty0; ty < ty1; ++ty) {
    const int64_t y0 = ty * kSmTile;
    if constexpr (MASKED) {                            // (block-uniform: one word, the same for every thread)
      const int64_t qt = XQ ? (int64_t)blockIdx.x : ty, ct = XQ ? ty : (int64_t)blockIdx.x;
      const uint32_t lw = __builtin_amdgcn_readfirstlane(mk.live[qt * mk.live_words + (ct >> 5)]);
      if (!((lw >> (ct & 31)) & 1u)) continue;
    }
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
    if constexpr (MASKED) {
      if (t < 2 * kSmTile) {                           // query t >> 1, word t & 1 of the candidate tile's two
        int32_t sid;
        if constexpr (XQ) sid = qset[t >> 1];          // (written before the barrier above)
        else {
          const int64_t y = y0 + (t >> 1);
          sid = y < NY ? mk.set[y] : -1;
          if (sid >= mk.n_sets) sid = -1;
        }
        const int64_t ct = XQ ? ty : (int64_t)blockIdx.x;
        mw[t] = sid >= 0 ? mk.mask[(int64_t)sid * mk.W + 2 * ct + (t & 1)] : 0xffffffffu;
      }
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
      uint32_t adm = 0xffffu;                          // MASKED: the row's bits of its 16 columns
      if constexpr (MASKED) adm = mw[2 * row + (part >> 1)] >> (16 * (part & 1));
      float z[16];
      float m = ninf, zt = 0.f, found = 0.f;
      int arg = -1;                                    // SAMPLED: the column of the maximum, the lowest of equal ones
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        z[j] = Ws[row * kSmLdw + 16 * part + j];
        if constexpr (MASKED) { if (!((adm >> j) & 1u)) z[j] = ninf; }
        if (SAMPLED) {
          if (key >= 0 && yk[16 * part + j] == key) z[j] = ninf;   // accidental hit: no term of this row's sum
          if (z[j] > m) { m = z[j]; arg = 16 * part + j; }
        } else {
          m = fmaxf(m, z[j]);
          bool hit = key >= 0 && yk[16 * part + j] == key;
          if constexpr (MASKED) hit = hit && ((adm >> j) & 1u);      // an inadmissible true candidate is never found
          if (hit) { zt = z[j]; found = 1.f; }
        }
      }
      if (SAMPLED) {
#pragma unroll
        for (int x = 1; x <= 2; x <<= 1) {
          const float om = __shfl_xor(m, x, kWave);
          const int oa = __shfl_xor(arg, x, kWave);
          if (om > m || (om == m && oa >= 0 && oa < arg)) { m = om; arg = oa; }
        }
      } else {
        m = fmaxf(m, __shfl_xor(m, 1, kWave));
        m = fmaxf(m, __shfl_xor(m, 2, kWave));
      }
      float s = 0.f;
      if (m > ninf) {
#pragma unroll
        for (int j = 0; j < 16; ++j) s += expf(z[j] - m);        // exp(-inf) = 0: an empty slot
      }
      s += __shfl_xor(s, 1, kWave); s += __shfl_xor(s, 2, kWave);
      if (!SAMPLED) {
        zt += __shfl_xor(zt, 1, kWave); zt += __shfl_xor(zt, 2, kWave);
        found += __shfl_xor(found, 1, kWave); found += __shfl_xor(found, 2, kWave);
      }
      if (m > ninf) {
        if (SAMPLED && m > run_m) run_arg = (int)y0 + arg;
        const float nm = fmaxf(run_m, m);
        if constexpr (MASKED) {
          // the two products rounded each on its own and then added, which is the code the unmasked instantiation has
          // (there the compiler pairs them in one packed multiply; here it would contract one into an fma, and with more
          // than one tile a range the sum would differ from the unmasked call's in its last bit)
          float pa = run_s * expf(run_m - nm), pb = s * expf(m - nm);
          asm volatile("" : "+v"(pa), "+v"(pb));
          run_s = pa + pb;
        } else
        run_s = run_s * expf(run_m - nm) + s * expf(m - nm);      // (run_m = -inf: run_s = 0 times exp(-inf) = 0)
        run_m = nm;
      }
      if (!SAMPLED && found > 0.f) { run_zt = zt; run_found = 1.f; }
    } else {
      const float m_y = XQ ? 0.f : qm[yl], s_y = XQ ? 0.f : qs[yl];
      uint32_t adm_y = 0xffffffffu;                    // MASKED, Y = queries: query yl's word of X rows wm * 32 ...
      if constexpr (MASKED && !XQ) adm_y = mw[2 * yl + wm];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int xl = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
        const int xkey_l = xk[xl];
        float wv = 0.f;
        bool adm = true;
        if constexpr (MASKED) adm = XQ ? (mw[2 * xl + wn] >> li) & 1u : (adm_y >> (xl & 31)) & 1u;
        if (xkey_l >= 0 && ykey_l >= 0 && !(SAMPLED && xkey_l == ykey_l) && adm) {
          const float p = expf((sm_logit(scale, acc[q]) - (XQ ? qm[xl] : m_y)) - (XQ ? qs[xl] : s_y));
          wv = -scale * (p - (!SAMPLED && xkey_l == ykey_l ? 1.f : 0.f));
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
      reinterpret_cast<float4*>(out)[(int64_t)blockIdx.y * NX + x0 + row] = make_float4(run_m, run_s, SAMPLED ? __int_as_float(run_arg) : run_zt, run_found);
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

// One sweep of NX fixed rows against NY in n_ranges ranges of Y tiles (a range past the last tile writes zeros / an
// empty partial).
template <int MODE, bool XQ, bool SAMPLED, bool MASKED = false>
static int sm_sweep(const float* xp, const int32_t* xkey, int64_t NX, const float* yp, const int32_t* ykey, int64_t NY, int d,
                    float scale, const float* lse, int n_ranges, float* out, hipStream_t st, const SmMaskArgs& mk = SmMaskArgs{}) {
  const SmPlan pl = sm_plan(NY, n_ranges, d, MASKED);
  const int tpr = pl.tiles_per_range, xres = pl.xres;
  const size_t lds = pl.lds_bytes;
  const dim3 grid((unsigned)sm_tiles(NX), (unsigned)n_ranges);
  auto go = [&](auto kern) -> int {
    if (int rc = lds_opt_in(kern)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, xp, xkey, NX, yp, ykey, NY, d, scale, lse, tpr, xres, out, mk);
    return launch_status();
  };
  if constexpr (MODE == 0) return go(softmax_sweep_kernel<MODE, XQ, 1, SAMPLED, MASKED>);
  else switch (sm_maxcb(d)) {
    case 1: return go(softmax_sweep_kernel<MODE, XQ, 1, SAMPLED, MASKED>);
    case 2: return go(softmax_sweep_kernel<MODE, XQ, 2, SAMPLED, MASKED>);
    case 3: return go(softmax_sweep_kernel<MODE, XQ, 3, SAMPLED, MASKED>);
    case 4: return go(softmax_sweep_kernel<MODE, XQ, 4, SAMPLED, MASKED>);
    default: return go(softmax_sweep_kernel<MODE, XQ, 5, SAMPLED, MASKED>);
  }
}

}  // namespace ge
