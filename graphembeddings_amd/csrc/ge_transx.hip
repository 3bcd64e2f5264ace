// ge_transx.hip -- the translation models of transE.py / transH.py / transD.py on gfx950: batch scoring,
// the margin-hinge SGD step (TF1 GradientDescentOptimizer on tf.reduce_sum(tf.maximum(pos - neg + margin, 0)))
// and the multi-step native loop that draws its own batches (init.cpp getBatch, 224-246).
//
// Tables: ent [E,d] and rel [R,d] (separate, not holE.py's shared table), plus ent2 [E,d] / rel2 [R,d]:
//   TransE: ent2 = rel2 = NULL.   TransH: rel2 = normal_vector.   TransD: ent2 = ent_transfer, rel2 = rel_transfer.
// Distance D = sum_k |h_p + r - t_p| (L1) or sum_k (h_p + r - t_p)^2 (L2, no square root) with the projection
//   TransE: e;   TransH: e - (e.n^) n^,  n^ = n * rsqrt(max(n.n, 1e-12));   TransD: e + (e.e_p) r_p.
//
// Step layout (all stream-ordered, no host synchronisation):
//   1. grad kernel: one group of LPT lanes per pair.  Writes D+/D- hinge terms and, for an active pair
//      (D+ - D- + margin >= 0, MaximumGrad ties to x), one gradient row per slot: slots 4i..4i+3 = pos h, pos t,
//      neg h, neg t (keys = entity ids) and slot 4B+i = the pair's relation row (pos_r == neg_r; key E + r).
//      ent2/rel2 gradients go to a second plane with the same slot numbers.  Inactive pairs get the
//      sentinel key E + R and write no rows.
//   2. stable radix sort of (key, slot) with rocPRIM: slots of one destination row become adjacent, in slot order.
//   3. apply, pass 1: one wave per window of kWin sorted positions sums each run of equal keys in slot order;
//      a run that is a whole segment (its row's every slot) is applied at once (row -= lr * sum), a run cut by a
//      window edge is stored as a partial.  A hot row of L slots thus costs L / kWin waves, not one wave of L.
//   4. apply, pass 2: one wave per window that holds the head of a cut segment adds the following windows'
//      partials in window order and applies; its last block sums the hinge terms into the batch loss.
// Every sum runs in a fixed order, so a step is bitwise reproducible.
//
// AdaGrad (TF1 AdagradOptimizer in place of the SGD line): the same four stages.  The apply hands every row its
// complete sum in one apply_row call, which is what AdaGrad's s * s needs, so the two apply kernels are instantiated a
// second time on AdaArgs (the tables' accumulators beside them) and only apply_row differs:
//   acc[row] += s * s,  row -= lr * s / sqrt(acc[row])      (the updated accumulator, no epsilon).
#include <cstring>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>

#include "ge_common.h"
#include "ge_bernoulli_dev.h"
#include "ge_launch.h"
#include "ge_transx_apply.h"   // stages 3 and 4: the apply kernels, shared with ge_rotate.hip

namespace ge {

constexpr int kTxMaxDim = 1024;
constexpr float kNormEps = 1e-12f;        // tf.nn.l2_normalize epsilon

template <bool L1>
__device__ __forceinline__ float dist_term(float u) { return L1 ? fabsf(u) : u * u; }
// d|u|/du = sign(u) with sign(0) = 0;  d(u^2)/du = 2u
template <bool L1>
__device__ __forceinline__ float dist_grad(float u) { return L1 ? (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f)) : 2.f * u; }

// The projection scalars of one triple: TransH a = e.n (raw n; scaled by inv later), TransD a = e.e_p.
struct Proj { float ah, at, nn; };

template <int MODEL, int VEC, int LPT>
__device__ __forceinline__ Proj proj_dots(const float* eh, const float* et, const float* eh2, const float* et2,
                                          const float* r2, int nvec, int lane) {
  Proj p{0.f, 0.f, 0.f};
  if constexpr (MODEL == kTransE) return p;
  for (int j = lane; j < nvec; j += LPT) {
    float h[VEC], t[VEC];
    ld<VEC>(eh, j, h); ld<VEC>(et, j, t);
    if constexpr (MODEL == kTransH) {
      float n[VEC]; ld<VEC>(r2, j, n);
#pragma unroll
      for (int q = 0; q < VEC; ++q) { p.ah += h[q] * n[q]; p.at += t[q] * n[q]; p.nn += n[q] * n[q]; }
    } else {
      float hp[VEC], tp[VEC]; ld<VEC>(eh2, j, hp); ld<VEC>(et2, j, tp);
#pragma unroll
      for (int q = 0; q < VEC; ++q) { p.ah += h[q] * hp[q]; p.at += t[q] * tp[q]; }
    }
  }
  p.ah = group_sum<LPT>(p.ah); p.at = group_sum<LPT>(p.at);
  if constexpr (MODEL == kTransH) p.nn = group_sum<LPT>(p.nn);
  return p;
}

// u_q = proj(h)_q + r_q - proj(t)_q for one VEC chunk.  TransH: s = inv (n^ = n * s), ah/at already e.n^.
template <int MODEL, int VEC>
__device__ __forceinline__ void residual(const float* eh, const float* et, const float* rr, const float* r2,
                                         int j, const Proj& p, float inv, float (&u)[VEC], float (&x)[VEC]) {
  float h[VEC], t[VEC], r[VEC];
  ld<VEC>(eh, j, h); ld<VEC>(et, j, t); ld<VEC>(rr, j, r);
  if constexpr (MODEL == kTransE) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) { u[q] = h[q] + r[q] - t[q]; x[q] = 0.f; }
  } else {
    ld<VEC>(r2, j, x);                                   // TransH: n, TransD: r_p
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      if constexpr (MODEL == kTransH) {
        x[q] *= inv;                                     // n^
        u[q] = (h[q] - p.ah * x[q]) + r[q] - (t[q] - p.at * x[q]);
      } else {
        u[q] = (h[q] + p.ah * x[q]) + r[q] - (t[q] + p.at * x[q]);
      }
    }
  }
}

template <int MODEL>
__device__ __forceinline__ float norm_inv(Proj& p) {
  if constexpr (MODEL != kTransH) return 1.f;
  const float inv = rsqrtf(fmaxf(p.nn, kNormEps));
  p.ah *= inv; p.at *= inv;
  return inv;
}

__device__ __forceinline__ bool id_ok(int32_t x, int64_t n) { return x >= 0 && x < n; }

// ------------------------------------------------------------------------------------------- score
template <int MODEL, bool L1, int VEC, int LPT>
__global__ __launch_bounds__(kBlock) void transx_score_kernel(
    const float* __restrict__ ent, const float* __restrict__ rel, const float* __restrict__ ent2,
    const float* __restrict__ rel2, int64_t E, int64_t R, int d, const int32_t* __restrict__ tri, int64_t B,
    float* __restrict__ out) {
  constexpr int G = kWave / LPT;                        // triples per wave
  const int lane = threadIdx.x & (LPT - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int nvec = d / VEC;
  for (int64_t w0 = wave * G; w0 < B; w0 += nwaves * G) {     // uniform per wave: group_sum needs every lane
    const int64_t i = w0 + (threadIdx.x & (kWave - 1)) / LPT;
    int32_t h = 0, t = 0, r = 0;
    bool ok = false;
    if (i < B) {
      h = tri[3 * i]; t = tri[3 * i + 1]; r = tri[3 * i + 2];
      ok = id_ok(h, E) && id_ok(t, E) && id_ok(r, R);
    }
    if (!ok) h = t = r = 0;
    const float* eh = ent + (int64_t)h * d; const float* et = ent + (int64_t)t * d;
    const float* rr = rel + (int64_t)r * d;
    const float* eh2 = ent2 ? ent2 + (int64_t)h * d : nullptr; const float* et2 = ent2 ? ent2 + (int64_t)t * d : nullptr;
    const float* r2 = rel2 ? rel2 + (int64_t)r * d : nullptr;
    Proj p = proj_dots<MODEL, VEC, LPT>(eh, et, eh2, et2, r2, nvec, lane);
    const float inv = norm_inv<MODEL>(p);
    float D = 0.f;
    for (int j = lane; j < nvec; j += LPT) {
      float u[VEC], x[VEC];
      residual<MODEL, VEC>(eh, et, rr, r2, j, p, inv, u, x);
#pragma unroll
      for (int q = 0; q < VEC; ++q) D += dist_term<L1>(u[q]);
    }
    D = group_sum<LPT>(D);
    if (i < B && lane == 0) out[i] = ok ? D : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------- gradient
template <int VEC>
__device__ __forceinline__ void st(float* __restrict__ plane, int64_t slot, int d, int j, const float (&v)[VEC]) {
  store_vec<VEC>(plane + slot * d + j * VEC, v);
}

template <int MODEL, bool L1, int VEC, int LPT>
__global__ __launch_bounds__(kBlock) void transx_grad_kernel(
    const float* __restrict__ ent, const float* __restrict__ rel, const float* __restrict__ ent2,
    const float* __restrict__ rel2, int64_t E, int64_t R, int d, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ neg, int64_t B, float margin, float* __restrict__ hinge,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ slots, float* __restrict__ g0, float* __restrict__ g1) {
  constexpr int G = kWave / LPT;
  const int lane = threadIdx.x & (LPT - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int nvec = d / VEC;
  const uint32_t sentinel = (uint32_t)(E + R);
  for (int64_t w0 = wave * G; w0 < B; w0 += nwaves * G) {
    const int64_t i = w0 + (threadIdx.x & (kWave - 1)) / LPT;
    int32_t h = 0, t = 0, r = 0, nh = 0, nt = 0;
    bool ok = false;
    if (i < B) {
      h = pos[3 * i]; t = pos[3 * i + 1]; r = pos[3 * i + 2];
      nh = neg[3 * i]; nt = neg[3 * i + 1];
      ok = id_ok(h, E) && id_ok(t, E) && id_ok(r, R) && id_ok(nh, E) && id_ok(nt, E) && neg[3 * i + 2] == r;
    }
    if (!ok) h = t = r = nh = nt = 0;
    const float* eh = ent + (int64_t)h * d; const float* et = ent + (int64_t)t * d;
    const float* fh = ent + (int64_t)nh * d; const float* ft = ent + (int64_t)nt * d;
    const float* rr = rel + (int64_t)r * d;
    const float* eh2 = nullptr; const float* et2 = nullptr; const float* fh2 = nullptr; const float* ft2 = nullptr;
    if constexpr (MODEL == kTransD) {
      eh2 = ent2 + (int64_t)h * d; et2 = ent2 + (int64_t)t * d; fh2 = ent2 + (int64_t)nh * d; ft2 = ent2 + (int64_t)nt * d;
    }
    const float* r2 = MODEL == kTransE ? nullptr : rel2 + (int64_t)r * d;
    Proj pp = proj_dots<MODEL, VEC, LPT>(eh, et, eh2, et2, r2, nvec, lane);
    Proj pn = proj_dots<MODEL, VEC, LPT>(fh, ft, fh2, ft2, r2, nvec, lane);
    const float inv = norm_inv<MODEL>(pp);
    norm_inv<MODEL>(pn);
    // pass 2: distances and c = f(u).x (x = n^ for TransH, r_p for TransD)
    float Dp = 0.f, Dn = 0.f, cp = 0.f, cn = 0.f;
    for (int j = lane; j < nvec; j += LPT) {
      float up[VEC], un[VEC], x[VEC];
      residual<MODEL, VEC>(eh, et, rr, r2, j, pp, inv, up, x);
      residual<MODEL, VEC>(fh, ft, rr, r2, j, pn, inv, un, x);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        Dp += dist_term<L1>(up[q]); Dn += dist_term<L1>(un[q]);
        if constexpr (MODEL != kTransE) { cp += dist_grad<L1>(up[q]) * x[q]; cn += dist_grad<L1>(un[q]) * x[q]; }
      }
    }
    Dp = group_sum<LPT>(Dp); Dn = group_sum<LPT>(Dn);
    if constexpr (MODEL != kTransE) { cp = group_sum<LPT>(cp); cn = group_sum<LPT>(cn); }
    const float z = Dp - Dn + margin;
    const bool active = ok && z >= 0.f;
    if (i < B && lane == 0) {
      hinge[i] = active ? z : 0.f;
      const uint32_t ks[5] = {(uint32_t)h, (uint32_t)t, (uint32_t)nh, (uint32_t)nt, (uint32_t)(E + r)};
#pragma unroll
      for (int s = 0; s < 4; ++s) { keys[4 * i + s] = active ? ks[s] : sentinel; slots[4 * i + s] = (uint32_t)(4 * i + s); }
      keys[4 * B + i] = active ? ks[4] : sentinel; slots[4 * B + i] = (uint32_t)(4 * B + i);
    }
    if (!active) continue;                            // group-uniform: no shuffles below
    // pass 3: gradient rows.  g+ = f(u+), g- = -f(u-).
    const float dap = pp.ah - pp.at, dan = pn.ah - pn.at;
    // TransH: d/dn^ summed over the pair, then through l2_normalize (the max branch only when n.n >= eps):
    //   g_n = inv * g_n^ - [n.n >= eps] inv^2 (g_n^.n^) n,  g_n^.n^ = -2 c+ (a+ - b+) + 2 c- (a- - b-)
    const float gnn = 2.f * (cn * dan - cp * dap);
    const float kclamp = (MODEL == kTransH && pp.nn >= kNormEps) ? inv * inv * gnn : 0.f;
    for (int j = lane; j < nvec; j += LPT) {
      float up[VEC], un[VEC], x[VEC];
      residual<MODEL, VEC>(eh, et, rr, r2, j, pp, inv, up, x);
      residual<MODEL, VEC>(fh, ft, rr, r2, j, pn, inv, un, x);
      float gh[VEC], gt[VEC], gfh[VEC], gft[VEC], gr[VEC];
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const float fp = dist_grad<L1>(up[q]), fn = dist_grad<L1>(un[q]);
        gr[q] = fp - fn;
        if constexpr (MODEL == kTransE) {
          gh[q] = fp; gt[q] = -fp; gfh[q] = -fn; gft[q] = fn;
        } else if constexpr (MODEL == kTransH) {
          gh[q] = fp - cp * x[q]; gt[q] = -gh[q];
          gft[q] = fn - cn * x[q]; gfh[q] = -gft[q];
        } else {
          gh[q] = gt[q] = gfh[q] = gft[q] = 0.f;                               // transfer rows loaded below
        }
      }
      if constexpr (MODEL == kTransD) {
        float hp[VEC], tp[VEC], fhp[VEC], ftp[VEC], hh[VEC], tt[VEC], fhh[VEC], ftt[VEC];
        ld<VEC>(eh2, j, hp); ld<VEC>(et2, j, tp); ld<VEC>(fh2, j, fhp); ld<VEC>(ft2, j, ftp);
        ld<VEC>(eh, j, hh); ld<VEC>(et, j, tt); ld<VEC>(fh, j, fhh); ld<VEC>(ft, j, ftt);
        float r2g[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float fp = dist_grad<L1>(up[q]), fn = dist_grad<L1>(un[q]);
          gh[q] = fp + cp * hp[q];
          gt[q] = -(fp + cp * tp[q]);
          gfh[q] = -(fn + cn * fhp[q]);
          gft[q] = fn + cn * ftp[q];
          r2g[q] = dap * fp - dan * fn;
          hp[q] = cp * hh[q]; tt[q] = -cp * tt[q]; fhh[q] = -cn * fhh[q]; ftt[q] = cn * ftt[q];
        }
        st<VEC>(g1, 4 * i + 0, d, j, hp); st<VEC>(g1, 4 * i + 1, d, j, tt);
        st<VEC>(g1, 4 * i + 2, d, j, fhh); st<VEC>(g1, 4 * i + 3, d, j, ftt);
        st<VEC>(g1, 4 * B + i, d, j, r2g);
      }
      if constexpr (MODEL == kTransH) {
        float hh[VEC], tt[VEC], fhh[VEC], ftt[VEC], n[VEC], gn[VEC];
        ld<VEC>(eh, j, hh); ld<VEC>(et, j, tt); ld<VEC>(fh, j, fhh); ld<VEC>(ft, j, ftt); ld<VEC>(r2, j, n);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float fp = dist_grad<L1>(up[q]), fn = dist_grad<L1>(un[q]);
          // g_n^ = -c+ (h - t) - (a+ - b+) f+  +  c- (h' - t') + (a- - b-) f-
          const float gnh = -cp * (hh[q] - tt[q]) - dap * fp + cn * (fhh[q] - ftt[q]) + dan * fn;
          gn[q] = inv * gnh - kclamp * n[q];
        }
        st<VEC>(g1, 4 * B + i, d, j, gn);
      }
      st<VEC>(g0, 4 * i + 0, d, j, gh); st<VEC>(g0, 4 * i + 1, d, j, gt);
      st<VEC>(g0, 4 * i + 2, d, j, gfh); st<VEC>(g0, 4 * i + 3, d, j, gft);
      st<VEC>(g0, 4 * B + i, d, j, gr);
    }
  }
}

// ------------------------------------------------------------------------------------------- draw (loop)
// Positive i of step `step`: a uniform row of the triple list, with replacement (getBatch, init.cpp:229);
// then the Bernoulli corruption of the same (seed, step, row).
__global__ __launch_bounds__(kBlock) void transx_draw_kernel(
    const int32_t* __restrict__ triples, int64_t T, int64_t B, const int64_t* __restrict__ bh_key,
    const int32_t* __restrict__ bh_ent, const int64_t* __restrict__ bt_key, const int32_t* __restrict__ bt_ent,
    int64_t n_known, const uint32_t* __restrict__ tail_threshold, int32_t n_rel, int32_t n_ent, uint64_t seed,
    uint64_t step, int32_t* __restrict__ pos, int32_t* __restrict__ neg) {
  const uint32_t slo = (uint32_t)step, shi = (uint32_t)(step >> 32);
  const uint32_t klo = (uint32_t)seed, khi = (uint32_t)(seed >> 32);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = philox_w0(slo, shi, (uint32_t)i, (uint32_t)((uint64_t)i >> 32), klo ^ GE_TAG_TXDRAW, khi);
    const int64_t row = (int64_t)(((uint64_t)w * (uint64_t)T) >> 32);
    int32_t t[3] = {triples[3 * row], triples[3 * row + 1], triples[3 * row + 2]};
    pos[3 * i] = t[0]; pos[3 * i + 1] = t[1]; pos[3 * i + 2] = t[2];
    bernoulli_corrupt_row(t, i, bh_key, bh_ent, bt_key, bt_ent, n_known, tail_threshold, n_rel, 0, n_ent, seed, step);
    neg[3 * i] = t[0]; neg[3 * i + 1] = t[1]; neg[3 * i + 2] = t[2];
  }
}

// ------------------------------------------------------------------------------------------- host side
static inline int lpt_for(int nvec) { return nvec <= 8 ? 8 : nvec <= 16 ? 16 : nvec <= 32 ? 32 : 64; }

struct TxWs {
  uint32_t *keys_in, *keys_out, *slots_in, *slots_out;
  float *hinge, *g0, *g1, *part;
  int32_t *pos, *neg;
  void* sort_tmp; size_t sort_bytes;
  size_t total;
};

static int ws_layout(int64_t E, int64_t R, int32_t d, int64_t B, void* base, TxWs& w) {
  const int64_t n = 5 * B, nwin = (n + kWin - 1) / kWin;
  size_t sort_bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, key_bits(E, R));
  if (e != hipSuccess) return (int)e;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += align_up(bytes, 256); return q; };
  w.keys_in = (uint32_t*)take(n * 4); w.keys_out = (uint32_t*)take(n * 4);
  w.slots_in = (uint32_t*)take(n * 4); w.slots_out = (uint32_t*)take(n * 4);
  w.hinge = (float*)take(B * 4);
  w.g0 = (float*)take((size_t)n * d * 4); w.g1 = (float*)take((size_t)n * d * 4);
  w.part = (float*)take((size_t)nwin * 4 * d * 4);
  w.pos = (int32_t*)take(B * 12); w.neg = (int32_t*)take(B * 12);
  w.sort_bytes = sort_bytes ? sort_bytes : 4;
  w.sort_tmp = take(w.sort_bytes);
  w.total = off;
  return 0;
}

size_t transx_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B) {
  TxWs w;
  if (ws_layout(E, R, d, B, nullptr, w) != 0) return 0;
  return w.total;
}

int transx_max_dim() { return kTxMaxDim; }

template <int MODEL, bool L1, int VEC>
static void launch_score_v(int lpt, int grid, hipStream_t st, const float* ent, const float* rel, const float* ent2,
                           const float* rel2, int64_t E, int64_t R, int d, const int32_t* tri, int64_t B, float* out) {
#define GE_TX_SCORE(L) hipLaunchKernelGGL((transx_score_kernel<MODEL, L1, VEC, L>), dim3(grid), dim3(kBlock), 0, st, \
                                          ent, rel, ent2, rel2, E, R, d, tri, B, out)
  switch (lpt) { case 8: GE_TX_SCORE(8); break; case 16: GE_TX_SCORE(16); break; case 32: GE_TX_SCORE(32); break; default: GE_TX_SCORE(64); }
#undef GE_TX_SCORE
}

template <int MODEL, bool L1, int VEC>
static void launch_grad_v(int lpt, int grid, hipStream_t st, const float* ent, const float* rel, const float* ent2,
                          const float* rel2, int64_t E, int64_t R, int d, const int32_t* pos, const int32_t* neg,
                          int64_t B, float margin, const TxWs& w) {
#define GE_TX_GRAD(L) hipLaunchKernelGGL((transx_grad_kernel<MODEL, L1, VEC, L>), dim3(grid), dim3(kBlock), 0, st, \
                                         ent, rel, ent2, rel2, E, R, d, pos, neg, B, margin, w.hinge, w.keys_in,   \
                                         w.slots_in, w.g0, w.g1)
  switch (lpt) { case 8: GE_TX_GRAD(8); break; case 16: GE_TX_GRAD(16); break; case 32: GE_TX_GRAD(32); break; default: GE_TX_GRAD(64); }
#undef GE_TX_GRAD
}

template <bool SCORE, int VEC, typename... A>
static void dispatch_mn(int model, int l1, A... args) {
  auto go = [&](auto m, auto l) {
    if constexpr (SCORE) launch_score_v<decltype(m)::value, decltype(l)::value, VEC>(args...);
    else launch_grad_v<decltype(m)::value, decltype(l)::value, VEC>(args...);
  };
  using T = std::true_type; using F = std::false_type;
  using IE = std::integral_constant<int, kTransE>; using IH = std::integral_constant<int, kTransH>;
  using ID = std::integral_constant<int, kTransD>;
  if (model == kTransE) { if (l1) go(IE{}, T{}); else go(IE{}, F{}); }
  else if (model == kTransH) { if (l1) go(IH{}, T{}); else go(IH{}, F{}); }
  else { if (l1) go(ID{}, T{}); else go(ID{}, F{}); }
}

// ent2 / rel2 as the kernels take them, from the model's named tables
static void extra_tables(int model, const float* normal, const float* ent_transfer, const float* rel_transfer,
                         const float*& ent2, const float*& rel2) {
  ent2 = model == kTransD ? ent_transfer : nullptr;
  rel2 = model == kTransH ? normal : model == kTransD ? rel_transfer : nullptr;
}

int transx_score_launch(const TransModel& m, const int32_t* tri, int64_t B, float* out, hipStream_t st) {
  if (B == 0) return 0;
  const float *ent2, *rel2;
  extra_tables(m.model, m.normal, m.ent_transfer, m.rel_transfer, ent2, rel2);
  const int d = m.dE;
  const bool v4 = d % 4 == 0 && aligned16({m.ent, m.rel, ent2, rel2});
  const int nvec = v4 ? d / 4 : d, lpt = lpt_for(nvec);
  const int grid = grid_for((B + kWave / lpt - 1) / (kWave / lpt), kBlock / kWave);
  if (v4) dispatch_mn<true, 4>(m.model, m.l1, lpt, grid, st, m.ent, m.rel, ent2, rel2, m.E, m.R, d, tri, B, out);
  else dispatch_mn<true, 1>(m.model, m.l1, lpt, grid, st, m.ent, m.rel, ent2, rel2, m.E, m.R, d, tri, B, out);
  return launch_status();
}

// The accumulators of an AdaGrad step as the kernels take them (ent2 / rel2's order); all null: plain SGD.
struct TxAcc { float *ent = nullptr, *rel = nullptr, *ent2 = nullptr, *rel2 = nullptr; };

// One step on caller-given (or drawn) pos/neg; loss = one float.  acc.ent set: the AdaGrad apply.
static int step_core(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* ent2, float* rel2,
                     int32_t d, const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss,
                     TxWs& w, hipStream_t st, const TxAcc& acc = TxAcc{}) {
  const bool v4 = d % 4 == 0 && aligned16({ent, rel, ent2, rel2, w.g0, w.g1, w.part, acc.ent, acc.rel, acc.ent2, acc.rel2});
  const int nvec = v4 ? d / 4 : d, lpt = lpt_for(nvec);
  const int grid = grid_for((B + kWave / lpt - 1) / (kWave / lpt), kBlock / kWave);
  if (v4) dispatch_mn<false, 4>(model, l1, lpt, grid, st, ent, rel, ent2, rel2, E, R, (int)d, pos, neg, B, margin, w);
  else dispatch_mn<false, 1>(model, l1, lpt, grid, st, ent, rel, ent2, rel2, E, R, (int)d, pos, neg, B, margin, w);
  int rc = launch_status();
  if (rc) return rc;
  const int64_t n = 5 * B;
  size_t sb = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)n,
                                           0u, key_bits(E, R), st);
  if (e != hipSuccess) return (int)e;
  const ApplyArgs a{ent, rel, ent2, rel2, E, R, (int)d, n, w.keys_out, w.slots_out, w.g0, w.g1, w.part, lr, (int)d};
  const int grid_a = apply_grid(n);
  if (acc.ent) {
    AdaArgs g;
    static_cast<ApplyArgs&>(g) = a;
    g.acc_ent = acc.ent; g.acc_rel = acc.rel; g.acc_ent2 = ent2 ? acc.ent2 : nullptr; g.acc_rel2 = rel2 ? acc.rel2 : nullptr;
    if (v4) launch_apply<4>(g, grid_a, w.hinge, B, loss, st);
    else launch_apply<1>(g, grid_a, w.hinge, B, loss, st);
  } else {
    if (v4) launch_apply<4>(a, grid_a, w.hinge, B, loss, st);
    else launch_apply<1>(a, grid_a, w.hinge, B, loss, st);
  }
  return launch_status();
}

int transx_hinge_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                          float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* neg,
                          int64_t B, float margin, float lr, float* loss, void* workspace, size_t workspace_bytes,
                          hipStream_t st) {
  TxWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const float *e2, *r2;
  extra_tables(model, normal, ent_transfer, rel_transfer, e2, r2);
  return step_core(model, l1, ent, E, rel, R, (float*)e2, (float*)r2, d, pos, neg, B, margin, lr, loss, w, st);
}

int transx_draw_launch(const SamplerArgs& s, int64_t B, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg,
                       hipStream_t st) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(transx_draw_kernel, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, st, s.triples, s.T, B, s.bh_key,
                     s.bh_ent, s.bt_key, s.bt_ent, s.n_known, s.tail_threshold, s.n_rel, s.n_ent, seed, step, pos, neg);
  return launch_status();
}

int transx_train_steps_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                           float* ent_transfer, float* rel_transfer, int32_t d, const SamplerArgs& sa, uint64_t seed,
                           uint64_t first_step, int64_t n_steps, int64_t B, float margin, float lr, float* losses,
                           void* workspace, size_t workspace_bytes, hipStream_t st) {
  TxWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const float *e2, *r2;
  extra_tables(model, normal, ent_transfer, rel_transfer, e2, r2);
  return draw_then_step(sa, B, seed, first_step, n_steps, w.pos, w.neg, st, [&](int64_t s) {
    return step_core(model, l1, ent, E, rel, R, (float*)e2, (float*)r2, d, w.pos, w.neg, B, margin, lr, losses + s, w, st);
  });
}

// the accumulators of the model's tables in the kernels' order (extra_tables)
static TxAcc extra_accs(const TransAccs& c, int model) {
  TxAcc a;
  a.ent = c.ent; a.rel = c.rel;
  a.ent2 = model == kTransD ? c.ent_transfer : nullptr;
  a.rel2 = model == kTransH ? c.normal : model == kTransD ? c.rel_transfer : nullptr;
  return a;
}

int transx_adagrad_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                            float* ent_transfer, float* rel_transfer, const TransAccs& accs, int32_t d,
                            const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss,
                            void* workspace, size_t workspace_bytes, hipStream_t st) {
  TxWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const float *e2, *r2;
  extra_tables(model, normal, ent_transfer, rel_transfer, e2, r2);
  return step_core(model, l1, ent, E, rel, R, (float*)e2, (float*)r2, d, pos, neg, B, margin, lr, loss, w, st,
                   extra_accs(accs, model));
}

int transx_train_steps_adagrad_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                                   float* ent_transfer, float* rel_transfer, const TransAccs& accs, int32_t d,
                                   const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B,
                                   float margin, float lr, float* losses, void* workspace, size_t workspace_bytes,
                                   hipStream_t st) {
  TxWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const float *e2, *r2;
  extra_tables(model, normal, ent_transfer, rel_transfer, e2, r2);
  const TxAcc acc = extra_accs(accs, model);
  return draw_then_step(sa, B, seed, first_step, n_steps, w.pos, w.neg, st, [&](int64_t s) {
    return step_core(model, l1, ent, E, rel, R, (float*)e2, (float*)r2, d, w.pos, w.neg, B, margin, lr, losses + s, w, st, acc);
  });
}

}  // namespace ge
