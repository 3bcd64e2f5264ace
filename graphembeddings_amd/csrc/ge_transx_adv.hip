// ge_transx_adv.hip -- the self-adversarial negative-sampling loss (Sun et al., ICLR 2019, eq. 5-6) for TransE / TransH /
// TransD on gfx950: the per-row loss, the step (SGD and AdaGrad) and the native loop.  The batch, the loss, the slot
// layout, the draw and the apply stage are ge_rotate_adv.hip's; the distance and its projections are ge_transx.hip's.
//
// Row i: a positive (h, t, r), side[i] (0: the tail is replaced, 1: the head) and K replacing entities neg_ent[i, :].
//   u = proj(h) + r - proj(t),  D = sum |u| (L1) or sum u^2,  f = dD/du (sign(0) = 0)
//   TransE proj(e) = e;  TransH proj(e) = e - (e.n^) n^, n^ = n rsqrt(max(n.n, 1e-12));  TransD proj(e) = e + (e.e_p) r_p
//   p_ij   = softmax_j(-alpha D-_ij) over the row's live slots (ids in [0, E)), a constant for the gradient
//   loss_i = softplus(D+_i - gamma) + sum_j p_ij softplus(gamma - D-_ij),   loss = sum_i loss_i
//   a+_i = sigma(D+_i - gamma),   a-_ij = -p_ij sigma(gamma - D-_ij).
//
// One workgroup per row.  The fixed entity (h when tails are replaced, t when heads are) is projected ONCE per row:
// F = proj(h) + r, or F = proj(t) - r, kept in registers with x = n^ (TransH) or r_p (TransD).  Every other entity m of
// the row -- the positive's moving entity and the K replacements -- has u = +-(F - proj(m)): one row read for TransE, and
// for TransH / TransD the dot b = m.n^ / m.m_p before the residual and c = f.x before the gradient rows.
//   teams   a wave is cut into G = 64 / LPT groups of LPT lanes (LPT = 8, 16, 32, 64 by the number of chunks of a row), a
//           workgroup has NT = 4 G teams; team q takes negatives j = q, q + NT, q + 2 NT, ... in that order
//   pass 1  D+ and the K distances (and the K dots b) into LDS
//   softmax ge_rotate_adv.hip's: thread x takes j = x, x + 256, ...; the coefficient a_ij replaces D-_ij in LDS
//   pass 2  each team re-reads its negatives, writes the moving rows of each live one (both planes for TransD) and keeps
//           in registers what the fixed entity, the relation and plane 1 need:
//             T = sum a f,  C = sum a c,  V1 = sum a c m (TransH),  V2 = sum a b f (TransH, TransD)
//           summed in this order: a team's negatives in index order; the teams of a wave by an xor tree (lane masks LPT,
//           2 LPT, ..., 32); the four waves in order through LDS, ((w0 + w1) + w2) + w3; the positive's term last.  Then
//           wave 0 writes the positive's moving rows, the fixed rows and the relation rows (its team 0 stores):
//             TransE  fixed = +-T, r = T
//             TransH  fixed = +-(T - C n^), r = T, n^: +-(V1 - C f - (f.n^) T + V2), through l2_normalize ONCE (linear)
//             TransD  fixed = +-(T + C f_p), f_p: +-C f, r = T, r_p: +-((f.f_p) T - V2)
// Gradient slots (d floats each, in plane 0 and plane 1): (K+2) i + 0, + 1 = the positive's head and tail,
// (K+2) i + 2 + j = negative j's replacing entity, (K+2) B + i = the relation; n = (K+3) B slots.  Plane 1 carries
// ent_transfer on entity slots (TransD) and normal_vector / rel_transfer on the relation slot.  Keys = entity ids, E + r
// for the relation, the sentinel E + R for an empty slot and for every slot of an invalid row.  Then rocPRIM's stable radix
// sort of (key, slot) and the family's two apply kernels (ge_transx_apply.h), exactly as the hinge step.  No float atomics.
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>

#include "ge_adv_dev.h"
#include "ge_common.h"
#include "ge_launch.h"
#include "ge_transx_apply.h"

namespace ge {
namespace {

constexpr int kTxAdvMaxDim = 1024;        // transx_max_dim()
constexpr float kNormEps = 1e-12f;        // tf.nn.l2_normalize epsilon

__device__ __forceinline__ bool id_ok(int32_t x, int64_t n) { return x >= 0 && x < n; }

template <bool L1>
__device__ __forceinline__ float dist_term(float u) { return L1 ? fabsf(u) : u * u; }
template <bool L1>
__device__ __forceinline__ float dist_grad(float u) { return L1 ? (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f)) : 2.f * u; }

struct TxAdvArgs {
  const float* ent; const float* rel; const float* ent2; const float* rel2; int64_t E, R; int d;
  const int32_t* pos; const int32_t* side; const int32_t* neg_ent; int64_t B; int K;
  float margin, alpha;
  float* loss_rows; uint32_t* keys; uint32_t* slots; float* g0; float* g1;
};

// u = +-(F - proj(m)) of one chunk: + where tails are replaced (sd = false), - where heads are
template <int MODEL, int VEC>
__device__ __forceinline__ void resid(const float (&F)[VEC], const float (&X)[VEC], const float (&m)[VEC], float b, bool sd,
                                      float (&u)[VEC]) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const float pm = MODEL == kTransE ? m[q] : MODEL == kTransH ? m[q] - b * X[q] : m[q] + b * X[q];
    const float w = F[q] - pm;
    u[q] = sd ? -w : w;
  }
}

// b of an entity row: e.n^ (TransH), e.e_p (TransD), 0 (TransE).  Every lane of the wave calls it.
template <int MODEL, int VEC, int LPT, int MAXC>
__device__ __forceinline__ float proj_dot(const float* __restrict__ e, const float* __restrict__ e2,
                                          const float (&X)[MAXC][VEC], int nvec, int lane) {
  if constexpr (MODEL == kTransE) return 0.f;
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < MAXC; ++it) {
    const int jv = lane + it * LPT;
    if (jv < nvec) {
      float m[VEC];
      ld<VEC>(e, jv, m);
      if constexpr (MODEL == kTransH) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) s += m[q] * X[it][q];
      } else {
        float mp[VEC];
        ld<VEC>(e2, jv, mp);
#pragma unroll
        for (int q = 0; q < VEC; ++q) s += m[q] * mp[q];
      }
    }
  }
  return group_sum<LPT>(s);
}

// D of a moving entity row with dot b.  Every lane of the wave calls it.
template <int MODEL, bool L1, int VEC, int LPT, int MAXC>
__device__ __forceinline__ float moving_dist(const float* __restrict__ e, const float (&F)[MAXC][VEC],
                                             const float (&X)[MAXC][VEC], float b, bool sd, int nvec, int lane) {
  float D = 0.f;
#pragma unroll
  for (int it = 0; it < MAXC; ++it) {
    const int jv = lane + it * LPT;
    if (jv < nvec) {
      float m[VEC], u[VEC];
      ld<VEC>(e, jv, m);
      resid<MODEL, VEC>(F[it], X[it], m, b, sd, u);
#pragma unroll
      for (int q = 0; q < VEC; ++q) D += dist_term<L1>(u[q]);
    }
  }
  return group_sum<LPT>(D);
}

// One moving entity with coefficient a = dloss/dD and dot b: its gradient rows to o0 (and o1, TransD) where `write`, and
// its terms added to T, C, V1, V2.  Every lane of the wave calls it (the shuffle of c comes before the `live` test); a
// slot that is not live reads a valid row and adds nothing.
template <int MODEL, bool L1, int VEC, int LPT, int MAXC>
__device__ __forceinline__ void moving_grad(const float* __restrict__ e, const float* __restrict__ e2,
                                            const float (&F)[MAXC][VEC], const float (&X)[MAXC][VEC], float a, float b,
                                            bool sd, bool live, bool write, float* __restrict__ o0, float* __restrict__ o1,
                                            int nvec, int lane, float (&T)[MAXC][VEC], float& C, float (&V1)[MAXC][VEC],
                                            float (&V2)[MAXC][VEC]) {
  float m[MAXC][VEC], f[MAXC][VEC], mp[MODEL == kTransD ? MAXC : 1][VEC];
  float c = 0.f;
#pragma unroll
  for (int it = 0; it < MAXC; ++it) {
    const int jv = lane + it * LPT;
    if (jv < nvec) {
      float u[VEC];
      ld<VEC>(e, jv, m[it]);
      if constexpr (MODEL == kTransD) ld<VEC>(e2, jv, mp[it]);
      resid<MODEL, VEC>(F[it], X[it], m[it], b, sd, u);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        f[it][q] = dist_grad<L1>(u[q]);
        if constexpr (MODEL != kTransE) c += f[it][q] * X[it][q];
      }
    }
  }
  if constexpr (MODEL != kTransE) c = group_sum<LPT>(c);
  if (live) {
    const float ac = a * c, ab = a * b;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
      const int jv = lane + it * LPT;
      if (jv < nvec) {
        float r0[VEC], r1[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float g = a * f[it][q];
          T[it][q] += g;
          float w = g;
          if constexpr (MODEL == kTransH) {
            w = g - ac * X[it][q];
            V1[it][q] += ac * m[it][q];
            V2[it][q] += ab * f[it][q];
          } else if constexpr (MODEL == kTransD) {
            w = g + ac * mp[it][q];
            const float w1 = ac * m[it][q];
            r1[q] = sd ? w1 : -w1;
            V2[it][q] += ab * f[it][q];
          }
          r0[q] = sd ? w : -w;
        }
        if (write) {
          store_vec<VEC>(o0 + jv * VEC, r0);
          if constexpr (MODEL == kTransD) store_vec<VEC>(o1 + jv * VEC, r1);
        }
      }
    }
    C += ac;
  }
}

// The teams of a wave by an xor tree, then wave w's sum to row[w] (its team 0 stores).
template <int VEC, int LPT, int MAXC>
__device__ __forceinline__ void teams_to_lds(float (&V)[MAXC][VEC], float* __restrict__ row, int nvec, int lane, int grp) {
#pragma unroll
  for (int it = 0; it < MAXC; ++it) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
#pragma unroll
      for (int m = LPT; m < kWave; m <<= 1) V[it][q] += __shfl_xor(V[it][q], m, kWave);
    }
    const int jv = lane + it * LPT;
    if (grp == 0 && jv < nvec) store_vec<VEC>(row + jv * VEC, V[it]);
  }
}

// the four waves' rows in order
template <int VEC, int LPT, int MAXC>
__device__ __forceinline__ void waves_sum(const float (*sT)[kTxAdvMaxDim], float (&V)[MAXC][VEC], int nvec, int lane) {
#pragma unroll
  for (int it = 0; it < MAXC; ++it) {
    const int jv = lane + it * LPT;
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      const int x = jv * VEC + q;
      V[it][q] = jv < nvec ? ((sT[0][x] + sT[1][x]) + sT[2][x]) + sT[3][x] : 0.f;
    }
  }
}

// GRAD = false: the loss rows alone (NaN for an invalid row); keys, slots, g0 and g1 are not touched.
template <int MODEL, bool L1, int VEC, int LPT, bool GRAD>
__global__ __launch_bounds__(kBlock) void transx_adv_kernel(const TxAdvArgs a) {
  constexpr int G = kWave / LPT, NT = kWaves * G;
  constexpr int MAXC = LPT < kWave ? 1 : kTxAdvMaxDim / VEC / kWave;
  constexpr int MAXJ = kAdvMaxK / kBlock;               // negatives per thread in the softmax
  __shared__ float sD[kAdvMaxK];                         // D-_ij, then a_ij
  __shared__ float sB[MODEL == kTransE ? 1 : kAdvMaxK];  // b_ij
  __shared__ alignas(16) float sT[GRAD ? kWaves : 1][GRAD ? kTxAdvMaxDim : 1];   // each wave's T, then V1, then V2
  __shared__ float sC[kWaves];
  __shared__ float red[kWaves];
  const float* __restrict__ ent = a.ent; const float* __restrict__ rel = a.rel;
  const float* __restrict__ ent2 = a.ent2; const float* __restrict__ rel2 = a.rel2;
  const int64_t E = a.E, R = a.R, B = a.B;
  const int d = a.d, K = a.K;
  const float margin = a.margin, alpha = a.alpha;
  const int tid = threadIdx.x, wave = tid / kWave;
  const int lane = tid & (LPT - 1), grp = (tid & (kWave - 1)) / LPT, team = wave * G + grp;
  const int nvec = d / VEC;
  const uint32_t sentinel = (uint32_t)(E + R);
  const int64_t S = (int64_t)K + 2;                      // entity slots per row
  for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
    __syncthreads();                                     // the previous row's LDS is free
    const int32_t h = a.pos[3 * i], t = a.pos[3 * i + 1], r = a.pos[3 * i + 2];
    const int32_t sdv = a.side[i];
    const bool ok = id_ok(h, E) && id_ok(t, E) && id_ok(r, R) && (sdv == 0 || sdv == 1);
    const int32_t* __restrict__ ni = a.neg_ent + i * (int64_t)K;
    if (!ok) {                                           // workgroup-uniform
      if (tid == 0) a.loss_rows[i] = GRAD ? 0.f : __builtin_nanf("");
      if constexpr (GRAD) {
        for (int s = tid; s < K + 2; s += kBlock) { a.keys[S * i + s] = sentinel; a.slots[S * i + s] = (uint32_t)(S * i + s); }
        if (tid == 0) { a.keys[S * B + i] = sentinel; a.slots[S * B + i] = (uint32_t)(S * B + i); }
      }
      continue;
    }
    const bool sd = sdv != 0;
    const int32_t fixed = sd ? t : h, moving = sd ? h : t;
    const float* ef = ent + (int64_t)fixed * d; const float* em = ent + (int64_t)moving * d;
    const float* ef2 = nullptr; const float* em2 = nullptr; const float* r2 = nullptr;
    if constexpr (MODEL == kTransD) { ef2 = ent2 + (int64_t)fixed * d; em2 = ent2 + (int64_t)moving * d; }
    if constexpr (MODEL != kTransE) r2 = rel2 + (int64_t)r * d;
    const float* rr = rel + (int64_t)r * d;
    // x, the fixed side F and D+: every team holds them for itself
    float X[MAXC][VEC], F[MAXC][VEC];
    float nn = 0.f, inv = 1.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) X[it][q] = 0.f;
      const int jv = lane + it * LPT;
      if (MODEL != kTransE && jv < nvec) {
        ld<VEC>(r2, jv, X[it]);
#pragma unroll
        for (int q = 0; q < VEC; ++q) nn += X[it][q] * X[it][q];
      }
    }
    if constexpr (MODEL == kTransH) {
      nn = group_sum<LPT>(nn);
      inv = rsqrtf(fmaxf(nn, kNormEps));
#pragma unroll
      for (int it = 0; it < MAXC; ++it)
#pragma unroll
        for (int q = 0; q < VEC; ++q) X[it][q] *= inv;      // n^
    }
    const float bf = proj_dot<MODEL, VEC, LPT, MAXC>(ef, ef2, X, nvec, lane);
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
      const int jv = lane + it * LPT;
#pragma unroll
      for (int q = 0; q < VEC; ++q) F[it][q] = 0.f;
      if (jv < nvec) {
        float e[VEC], rv[VEC];
        ld<VEC>(ef, jv, e); ld<VEC>(rr, jv, rv);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float pf = MODEL == kTransE ? e[q] : MODEL == kTransH ? e[q] - bf * X[it][q] : e[q] + bf * X[it][q];
          F[it][q] = sd ? pf - rv[q] : pf + rv[q];
        }
      }
    }
    const float bp = proj_dot<MODEL, VEC, LPT, MAXC>(em, em2, X, nvec, lane);
    const float Dp = moving_dist<MODEL, L1, VEC, LPT, MAXC>(em, F, X, bp, sd, nvec, lane);
    // pass 1: the K distances
    for (int jb = 0; jb < K; jb += NT) {                 // workgroup-uniform trip count: group_sum needs every lane
      const int j = jb + team;
      const int32_t c = j < K ? ni[j] : -1;
      const bool live = id_ok(c, E);
      const float* ec = ent + (int64_t)(live ? c : 0) * d;
      const float* ec2 = nullptr;
      if constexpr (MODEL == kTransD) ec2 = ent2 + (int64_t)(live ? c : 0) * d;
      const float b = proj_dot<MODEL, VEC, LPT, MAXC>(ec, ec2, X, nvec, lane);
      const float Dn = moving_dist<MODEL, L1, VEC, LPT, MAXC>(ec, F, X, b, sd, nvec, lane);
      if (j < K && lane == 0) {
        sD[j] = live ? Dn : 0.f;
        if constexpr (MODEL != kTransE) sB[j] = live ? b : 0.f;
      }
    }
    __syncthreads();
    // the softmax over the live slots, the loss and the coefficients
    float Dl[MAXJ], ex[MAXJ];
    bool lv[MAXJ];
    float mx = -__builtin_inff();
#pragma unroll
    for (int m = 0; m < MAXJ; ++m) {
      const int j = tid + m * kBlock;
      lv[m] = j < K && id_ok(ni[j], E);
      Dl[m] = lv[m] ? sD[j] : 0.f;
      if (lv[m]) mx = fmaxf(mx, neg_scaled(alpha, Dl[m]));
    }
    mx = block_max(mx, red);
    float se = 0.f, sl = 0.f;
#pragma unroll
    for (int m = 0; m < MAXJ; ++m) {
      ex[m] = lv[m] ? expf(neg_scaled(alpha, Dl[m]) - mx) : 0.f;
      if (lv[m]) { se += ex[m]; sl += ex[m] * softplus_dev(margin - Dl[m]); }
    }
    se = block_sum(se, red);
    sl = block_sum(sl, red);
    if (tid == 0) a.loss_rows[i] = softplus_dev(Dp - margin) + (se > 0.f ? sl / se : 0.f);
    if constexpr (GRAD) {
#pragma unroll
      for (int m = 0; m < MAXJ; ++m) {
        const int j = tid + m * kBlock;
        if (j < K) sD[j] = lv[m] ? -(ex[m] / se) * sigmoid_stable(margin - Dl[m]) : 0.f;
      }
      // keys and slots of the row: the positive's head and tail, the K replacements, the relation
      for (int s = tid; s < K + 2; s += kBlock) {
        uint32_t key = s == 0 ? (uint32_t)h : (uint32_t)t;
        if (s >= 2) { const int32_t c = ni[s - 2]; key = id_ok(c, E) ? (uint32_t)c : sentinel; }
        a.keys[S * i + s] = key; a.slots[S * i + s] = (uint32_t)(S * i + s);
      }
      if (tid == 0) { a.keys[S * B + i] = (uint32_t)(E + r); a.slots[S * B + i] = (uint32_t)(S * B + i); }
      __syncthreads();
      // pass 2: the moving rows of each live negative; T, C, V1, V2 stay in registers
      float T[MAXC][VEC], V1[MAXC][VEC], V2[MAXC][VEC];
      float C = 0.f;
#pragma unroll
      for (int it = 0; it < MAXC; ++it)
#pragma unroll
        for (int q = 0; q < VEC; ++q) T[it][q] = V1[it][q] = V2[it][q] = 0.f;
      for (int jb = 0; jb < K; jb += NT) {               // workgroup-uniform trip count, as pass 1
        const int j = jb + team;
        const int32_t c = j < K ? ni[j] : -1;
        const bool live = id_ok(c, E);
        const float* ec = ent + (int64_t)(live ? c : 0) * d;
        const float* ec2 = nullptr;
        if constexpr (MODEL == kTransD) ec2 = ent2 + (int64_t)(live ? c : 0) * d;
        const float aj = live ? sD[j] : 0.f;
        float b = 0.f;
        if constexpr (MODEL != kTransE) b = live ? sB[j] : 0.f;
        const int64_t row = (S * i + 2 + (live ? j : 0)) * (int64_t)d;
        float* o1 = nullptr;
        if constexpr (MODEL == kTransD) o1 = a.g1 + row;
        moving_grad<MODEL, L1, VEC, LPT, MAXC>(ec, ec2, F, X, aj, b, sd, live, true, a.g0 + row, o1, nvec, lane, T, C, V1, V2);
      }
      // the teams of a wave by an xor tree, the waves in order through LDS, one vector after the other
#pragma unroll
      for (int m = LPT; m < kWave; m <<= 1) C += __shfl_xor(C, m, kWave);
      if ((tid & (kWave - 1)) == 0) sC[wave] = C;
      teams_to_lds<VEC, LPT, MAXC>(T, sT[wave], nvec, lane, grp);
      __syncthreads();
      waves_sum<VEC, LPT, MAXC>(sT, T, nvec, lane);
      C = ((sC[0] + sC[1]) + sC[2]) + sC[3];
      if constexpr (MODEL == kTransH) {
        __syncthreads();
        teams_to_lds<VEC, LPT, MAXC>(V1, sT[wave], nvec, lane, grp);
        __syncthreads();
        waves_sum<VEC, LPT, MAXC>(sT, V1, nvec, lane);
      }
      if constexpr (MODEL != kTransE) {
        __syncthreads();
        teams_to_lds<VEC, LPT, MAXC>(V2, sT[wave], nvec, lane, grp);
        __syncthreads();
        waves_sum<VEC, LPT, MAXC>(sT, V2, nvec, lane);
      }
      if (wave == 0) {                                   // wave-uniform: its teams all compute, team 0 stores
        const bool wr = grp == 0;
        const float ap = sigmoid_stable(Dp - margin);
        const int64_t rowf = (S * i + (sd ? 1 : 0)) * (int64_t)d, rowm = (S * i + (sd ? 0 : 1)) * (int64_t)d;
        const int64_t rowr = (S * B + i) * (int64_t)d;
        float* om1 = nullptr;
        if constexpr (MODEL == kTransD) om1 = a.g1 + rowm;
        // the positive's term last, and its moving rows
        moving_grad<MODEL, L1, VEC, LPT, MAXC>(em, em2, F, X, ap, bp, sd, true, wr, a.g0 + rowm, om1, nvec, lane, T, C, V1, V2);
        float dnh[MODEL == kTransH ? MAXC : 1][VEC];
        float dot = 0.f;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
          const int jv = lane + it * LPT;
          if (jv < nvec) {
            float gf[VEC], gr[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) gr[q] = T[it][q];
            if constexpr (MODEL == kTransE) {
#pragma unroll
              for (int q = 0; q < VEC; ++q) gf[q] = sd ? -T[it][q] : T[it][q];
            } else if constexpr (MODEL == kTransH) {
              float e[VEC];
              ld<VEC>(ef, jv, e);
#pragma unroll
              for (int q = 0; q < VEC; ++q) {
                const float w = T[it][q] - C * X[it][q];
                gf[q] = sd ? -w : w;
                const float v = ((V1[it][q] - C * e[q]) - bf * T[it][q]) + V2[it][q];
                dnh[it][q] = sd ? -v : v;
                dot += dnh[it][q] * X[it][q];
              }
            } else {
              float e[VEC], ep[VEC], gf1[VEC], gr1[VEC];
              ld<VEC>(ef, jv, e); ld<VEC>(ef2, jv, ep);
#pragma unroll
              for (int q = 0; q < VEC; ++q) {
                const float w = T[it][q] + C * ep[q], w1 = C * e[q], v = bf * T[it][q] - V2[it][q];
                gf[q] = sd ? -w : w;
                gf1[q] = sd ? -w1 : w1;
                gr1[q] = sd ? -v : v;
              }
              if (wr) { store_vec<VEC>(a.g1 + rowf + jv * VEC, gf1); store_vec<VEC>(a.g1 + rowr + jv * VEC, gr1); }
            }
            if (wr) { store_vec<VEC>(a.g0 + rowf + jv * VEC, gf); store_vec<VEC>(a.g0 + rowr + jv * VEC, gr); }
          }
        }
        if constexpr (MODEL == kTransH) {
          // through l2_normalize once: dn = inv dn^ - [n.n >= eps] inv^3 (dn^.n) n, with dn^.n^ = inv (dn^.n)
          dot = group_sum<LPT>(dot);
          const float kclamp = nn >= kNormEps ? inv * inv * dot : 0.f;
#pragma unroll
          for (int it = 0; it < MAXC; ++it) {
            const int jv = lane + it * LPT;
            if (jv < nvec) {
              float n[VEC], gn[VEC];
              ld<VEC>(r2, jv, n);
#pragma unroll
              for (int q = 0; q < VEC; ++q) gn[q] = inv * dnh[it][q] - kclamp * n[q];
              if (wr) store_vec<VEC>(a.g1 + rowr + jv * VEC, gn);
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- host side
// The step's workspace: sort keys and slots (in, out) [(K+3)B] each | loss rows [B] | gradient plane 0 [(K+3)B, d] |
// plane 1 [(K+3)B, d] (TransH, TransD) | the apply's partials [windows][4][d] | the loop's pos [B,3], side [B],
// neg_ent [B,K] | rocPRIM's scratch; each padded to 256 B.
struct TxAdvWs {
  uint32_t *keys_in, *keys_out, *slots_in, *slots_out;
  float *loss_rows, *g0, *g1, *part;
  int32_t *pos, *side, *neg_ent;
  void* sort_tmp; size_t sort_bytes;
  size_t total;
};

int ws_layout(int model, int64_t E, int64_t R, int32_t d, int64_t B, int32_t K, void* base, TxAdvWs& w) {
  const int64_t n = ((int64_t)K + 3) * B, nwin = (n + kWin - 1) / kWin;
  size_t sort_bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, key_bits(E, R));
  if (e != hipSuccess) return (int)e;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += align_up(bytes, 256); return q; };
  w.keys_in = (uint32_t*)take(n * 4); w.keys_out = (uint32_t*)take(n * 4);
  w.slots_in = (uint32_t*)take(n * 4); w.slots_out = (uint32_t*)take(n * 4);
  w.loss_rows = (float*)take(B * 4);
  w.g0 = (float*)take((size_t)n * d * 4);
  w.g1 = model == kTransE ? nullptr : (float*)take((size_t)n * d * 4);
  w.part = (float*)take((size_t)nwin * 4 * d * 4);
  w.pos = (int32_t*)take(B * 12); w.side = (int32_t*)take(B * 4); w.neg_ent = (int32_t*)take((size_t)B * K * 4);
  w.sort_bytes = sort_bytes ? sort_bytes : 4;
  w.sort_tmp = take(w.sort_bytes);
  w.total = off;
  return 0;
}

template <int MODEL, bool L1, int VEC, bool GRAD>
void launch_adv_v(int lpt, int grid, hipStream_t st, const TxAdvArgs& a) {
#define GE_TX_ADV(L) hipLaunchKernelGGL((transx_adv_kernel<MODEL, L1, VEC, L, GRAD>), dim3(grid), dim3(kBlock), 0, st, a)
  switch (lpt) { case 8: GE_TX_ADV(8); break; case 16: GE_TX_ADV(16); break; case 32: GE_TX_ADV(32); break; default: GE_TX_ADV(64); }
#undef GE_TX_ADV
}

// v4: the float4 path (d % 4 == 0 and every buffer the kernels vector-load 16-byte aligned)
template <bool GRAD>
int launch_adv(int model, int l1, bool v4, hipStream_t st, const TxAdvArgs& a) {
  const int nvec = v4 ? a.d / 4 : a.d, lpt = adv_lpt_for(nvec);
  const int grid = grid_for(a.B, 1);
  auto go = [&](auto m, auto l) {
    if (v4) launch_adv_v<decltype(m)::value, decltype(l)::value, 4, GRAD>(lpt, grid, st, a);
    else launch_adv_v<decltype(m)::value, decltype(l)::value, 1, GRAD>(lpt, grid, st, a);
  };
  using T = std::true_type; using F = std::false_type;
  using IE = std::integral_constant<int, kTransE>; using IH = std::integral_constant<int, kTransH>;
  using ID = std::integral_constant<int, kTransD>;
  if (model == kTransE) { if (l1) go(IE{}, T{}); else go(IE{}, F{}); }
  else if (model == kTransH) { if (l1) go(IH{}, T{}); else go(IH{}, F{}); }
  else { if (l1) go(ID{}, T{}); else go(ID{}, F{}); }
  return launch_status();
}

// ent2 / rel2 and their accumulators as the kernels take them (ge_transx.hip's extra_tables / extra_accs)
struct TxTabs { float *ent, *rel, *ent2, *rel2; int64_t E, R; int32_t d; float *acc_ent, *acc_rel, *acc_ent2, *acc_rel2; };

TxTabs tabs_of(int model, float* ent, int64_t E, float* rel, int64_t R, float* normal, float* ent_transfer,
               float* rel_transfer, const TransAccs* c, int32_t d) {
  TxTabs t{ent, rel, model == kTransD ? ent_transfer : nullptr,
           model == kTransH ? normal : model == kTransD ? rel_transfer : nullptr, E, R, d, nullptr, nullptr, nullptr, nullptr};
  if (c) {
    t.acc_ent = c->ent; t.acc_rel = c->rel;
    t.acc_ent2 = model == kTransD ? c->ent_transfer : nullptr;
    t.acc_rel2 = model == kTransH ? c->normal : model == kTransD ? c->rel_transfer : nullptr;
  }
  return t;
}

// One step on caller-given (or drawn) rows; loss = one float.  t.acc_ent set: the AdaGrad apply.
int step_core(int model, int l1, const TxTabs& t, const int32_t* pos, const int32_t* side, const int32_t* neg_ent,
              int64_t B, int32_t K, float margin, float alpha, float lr, float* loss, TxAdvWs& w, hipStream_t st) {
  const int d = t.d;
  const bool v4 = d % 4 == 0 && aligned16({t.ent, t.rel, t.ent2, t.rel2, w.g0, w.g1, w.part, t.acc_ent, t.acc_rel,
                                            t.acc_ent2, t.acc_rel2});
  const TxAdvArgs g{t.ent, t.rel, t.ent2, t.rel2, t.E, t.R, d, pos, side, neg_ent, B, (int)K, margin, alpha,
                    w.loss_rows, w.keys_in, w.slots_in, w.g0, w.g1};
  int rc = launch_adv<true>(model, l1, v4, st, g);
  if (rc) return rc;
  const int64_t n = ((int64_t)K + 3) * B;
  size_t sb = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)n,
                                           0u, key_bits(t.E, t.R), st);
  if (e != hipSuccess) return (int)e;
  const ApplyArgs a{t.ent, t.rel, t.ent2, t.rel2, t.E, t.R, d, n, w.keys_out, w.slots_out, w.g0, w.g1, w.part, lr, d};
  const int grid_a = apply_grid(n);
  if (t.acc_ent) {
    AdaArgs ada;
    static_cast<ApplyArgs&>(ada) = a;
    ada.acc_ent = t.acc_ent; ada.acc_rel = t.acc_rel; ada.acc_ent2 = t.acc_ent2; ada.acc_rel2 = t.acc_rel2;
    if (v4) launch_apply<4>(ada, grid_a, w.loss_rows, B, loss, st);
    else launch_apply<1>(ada, grid_a, w.loss_rows, B, loss, st);
  } else {
    if (v4) launch_apply<4>(a, grid_a, w.loss_rows, B, loss, st);
    else launch_apply<1>(a, grid_a, w.loss_rows, B, loss, st);
  }
  return launch_status();
}

}  // namespace

int transx_adv_max_negatives() { return kAdvMaxK; }

size_t transx_adv_ws_bytes(int model, int64_t E, int64_t R, int32_t d, int64_t B, int32_t K) {
  TxAdvWs w;
  if (ws_layout(model, E, R, d, B, K, nullptr, w) != 0) return 0;
  return w.total;
}

int transx_adv_loss_launch(const TransModel& m, const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B,
                           int32_t K, float margin, float alpha, float* out, hipStream_t st) {
  if (B == 0) return 0;
  const TxTabs t = tabs_of(m.model, (float*)m.ent, m.E, (float*)m.rel, m.R, (float*)m.normal, (float*)m.ent_transfer,
                           (float*)m.rel_transfer, nullptr, m.dE);
  const bool v4 = t.d % 4 == 0 && aligned16({t.ent, t.rel, t.ent2, t.rel2});
  const TxAdvArgs g{t.ent, t.rel, t.ent2, t.rel2, t.E, t.R, t.d, pos, side, neg_ent, B, (int)K, margin, alpha, out,
                    nullptr, nullptr, nullptr, nullptr};
  return launch_adv<false>(m.model, m.l1, v4, st, g);
}

int transx_adv_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal, float* ent_transfer,
                        float* rel_transfer, const TransAccs* accs, int32_t d, const int32_t* pos, const int32_t* side,
                        const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr, float* loss,
                        void* workspace, size_t workspace_bytes, hipStream_t st) {
  TxAdvWs w;
  int rc = ws_layout(model, E, R, d, B, K, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const TxTabs t = tabs_of(model, ent, E, rel, R, normal, ent_transfer, rel_transfer, accs, d);
  return step_core(model, l1, t, pos, side, neg_ent, B, K, margin, alpha, lr, loss, w, st);
}

int transx_adv_train_steps_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                               float* ent_transfer, float* rel_transfer, const TransAccs* accs, int32_t d,
                               const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B,
                               int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                               size_t workspace_bytes, hipStream_t st) {
  TxAdvWs w;
  int rc = ws_layout(model, E, R, d, B, K, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  const TxTabs t = tabs_of(model, ent, E, rel, R, normal, ent_transfer, rel_transfer, accs, d);
  for (int64_t s = 0; s < n_steps; ++s) {                // the draw is the model-independent one of ge_rotate_adv.hip
    rc = rotate_adv_draw_launch(sa, B, K, seed, first_step + (uint64_t)s, w.pos, w.side, w.neg_ent, st);
    if (rc) return rc;
    rc = step_core(model, l1, t, w.pos, w.side, w.neg_ent, B, K, margin, alpha, lr, losses + s, w, st);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace ge
