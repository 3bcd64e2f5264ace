// ge_rotate_adv.hip -- RotatE's self-adversarial negative-sampling loss (Sun et al., ICLR 2019, eq. 5-6) on gfx950: the
// per-row loss, the step (SGD and AdaGrad), the draw of K filtered negatives per positive and the native loop.
//
// Row i: a positive (h, t, r), side[i] (0: the tail is replaced, 1: the head) and K replacing entities neg_ent[i, :].
// With D of ge_rotate.hip, gamma = margin, alpha = the adversarial temperature:
//   p_ij   = softmax_j(-alpha D-_ij) over the row's live slots (ids in [0, E)), a constant for the gradient
//   loss_i = softplus(D+_i - gamma) + sum_j p_ij softplus(gamma - D-_ij),   loss = sum_i loss_i
//   dloss/dD+_i = sigma(D+_i - gamma),   dloss/dD-_ij = -p_ij sigma(gamma - D-_ij).
// fp32 with the accurate expf / log1pf; the softmax is max-subtracted and every sum runs in a fixed order.
//
// One workgroup per row.  The fixed entity f (h when tails are replaced, t when heads are) is rotated ONCE per row and
// coordinate: F = h e^{i theta}, or F = t e^{-i theta} (|c e^{i theta} - t| = |c - t e^{-i theta}|, the rank sweep's
// identity), kept in registers with (cos, sin).  Every other entity m of the row -- the positive's moving entity and
// the K replacements -- then costs one row read and no trigonometry: u = F - m, D = sum |u| (or |u|^2), g = dD/du,
// dD/dm = -g and dD/dF = g on both sides.
//   teams   a wave is cut into G = 64 / LPT groups of LPT lanes (LPT = 8, 16, 32, 64 by the number of chunks of a row), a
//           workgroup has NT = 4 G teams; team q takes negatives j = q, q + NT, q + 2 NT, ... in that order
//   pass 1  D+ and the K distances into LDS
//   softmax the 256 threads over j (thread x takes j = x, x + 256, ...): max, then sum and the loss, each reduced by an
//           xor tree per wave and the four waves in order; the coefficient a_ij = dloss/dD-_ij replaces D-_ij in LDS
//   pass 2  each team re-reads its negatives, writes the gradient row -a g of each live one and accumulates sum_j a g for
//           the fixed entity in registers; the groups of a wave are combined by an xor tree, the waves in order through
//           LDS; team 0 adds the positive's term, rotates back once (dF/df and dF/dtheta) and writes the three remaining
//           rows.
// Gradient slots (d floats each): (K+2) i + 0, + 1 = the positive's head and tail, (K+2) i + 2 + j = negative j's
// replacing entity, (K+2) B + i = the relation (its first k floats); n = (K+3) B slots.  Keys = entity ids, E + r for the
// relation, the sentinel E + R for an empty slot and for every slot of an invalid row.  Then rocPRIM's stable radix sort
// of (key, slot) and the family's two apply kernels (ge_transx_apply.h) with relation rows k wide, exactly as
// ge_rotate.hip's hinge step.  No float atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include "ge_adv_dev.h"      // softplus, sigmoid, the softmax's reductions: shared with ge_transx_adv.hip
#include "ge_common.h"
#include "ge_bernoulli_dev.h"
#include "ge_launch.h"
#include "ge_rotate_dev.h"
#include "ge_transx_apply.h"

namespace ge {
namespace {

__device__ __forceinline__ bool id_ok(int32_t x, int64_t n) { return x >= 0 && x < n; }

// GRAD = false: the loss rows alone (NaN for an invalid row); keys, slots and g0 are not touched.
template <bool L1, int VEC, int LPT, bool GRAD>
__global__ __launch_bounds__(kBlock) void rotate_adv_kernel(
    const float* __restrict__ ent, const float* __restrict__ rel, int64_t E, int64_t R, int d,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ side, const int32_t* __restrict__ neg_ent, int64_t B,
    int K, float margin, float alpha, float* __restrict__ loss_rows, uint32_t* __restrict__ keys,
    uint32_t* __restrict__ slots, float* __restrict__ g0) {
  constexpr int G = kWave / LPT, NT = kWaves * G;
  constexpr int MAXC = LPT < kWave ? 1 : kRotMaxDim / 2 / VEC / kWave;
  constexpr int MAXJ = kAdvMaxK / kBlock;              // negatives per thread in the softmax
  __shared__ float sD[kAdvMaxK];                        // D-_ij, then a_ij
  __shared__ alignas(16) float sT[GRAD ? kWaves : 1][GRAD ? kRotMaxDim : 1];   // each wave's sum_j a g, [Re (k) | Im (k)]; float4 stores
  __shared__ float red[kWaves];
  const int tid = threadIdx.x, wave = tid / kWave;
  const int lane = tid & (LPT - 1), grp = (tid & (kWave - 1)) / LPT, team = wave * G + grp;
  const int k = d / 2, nvec = k / VEC;
  const uint32_t sentinel = (uint32_t)(E + R);
  const int64_t S = (int64_t)K + 2;                     // entity slots per row
  for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
    __syncthreads();                                    // the previous row's LDS is free
    int32_t h = pos[3 * i], t = pos[3 * i + 1], r = pos[3 * i + 2];
    const int32_t sd = side[i];
    const bool ok = id_ok(h, E) && id_ok(t, E) && id_ok(r, R) && (sd == 0 || sd == 1);
    const int32_t* ni = neg_ent + i * (int64_t)K;
    if (!ok) {                                          // workgroup-uniform
      if (tid == 0) loss_rows[i] = GRAD ? 0.f : __builtin_nanf("");
      if constexpr (GRAD) {
        for (int s = tid; s < K + 2; s += kBlock) { keys[S * i + s] = sentinel; slots[S * i + s] = (uint32_t)(S * i + s); }
        if (tid == 0) { keys[S * B + i] = sentinel; slots[S * B + i] = (uint32_t)(S * B + i); }
      }
      continue;
    }
    const int32_t fixed = sd ? t : h, moving = sd ? h : t;
    const float* ef = ent + (int64_t)fixed * d; const float* em = ent + (int64_t)moving * d;
    const float* th = rel + (int64_t)r * k;
    // the rotation (e^{i theta}, or e^{-i theta} when heads are replaced), F and D+: every group holds them for itself
    float cs[MAXC][VEC], sn[MAXC][VEC], Fre[MAXC][VEC], Fim[MAXC][VEC];
    float Dp = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
      const int j = lane + it * LPT;
      if (j < nvec) {
        float are[VEC], aim[VEC], bre[VEC], bim[VEC], p[VEC];
        ld<VEC>(th, j, p);
        ld<VEC>(ef, j, are); ld<VEC>(ef + k, j, aim); ld<VEC>(em, j, bre); ld<VEC>(em + k, j, bim);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          sincosf(p[q], &sn[it][q], &cs[it][q]);
          if (sd) sn[it][q] = -sn[it][q];
          const Coord x = coord(are[q], aim[q], bre[q], bim[q], cs[it][q], sn[it][q]);
          Fre[it][q] = x.wre; Fim[it][q] = x.wim;
          Dp += dist_term<L1>(x);
        }
      }
    }
    Dp = group_sum<LPT>(Dp);
    // pass 1: the K distances
    for (int jb = 0; jb < K; jb += NT) {                // workgroup-uniform trip count: group_sum needs every lane
      const int j = jb + team;
      const int32_t c = j < K ? ni[j] : -1;
      const bool live = id_ok(c, E);
      const float* ec = ent + (int64_t)(live ? c : 0) * d;
      float Dn = 0.f;
#pragma unroll
      for (int it = 0; it < MAXC; ++it) {
        const int jv = lane + it * LPT;
        if (jv < nvec) {
          float cre[VEC], cim[VEC];
          ld<VEC>(ec, jv, cre); ld<VEC>(ec + k, jv, cim);
#pragma unroll
          for (int q = 0; q < VEC; ++q) Dn += dist_term<L1>(coord_rotated(Fre[it][q], Fim[it][q], cre[q], cim[q]));
        }
      }
      Dn = group_sum<LPT>(Dn);
      if (j < K && lane == 0) sD[j] = live ? Dn : 0.f;
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
    if (tid == 0) loss_rows[i] = softplus_dev(Dp - margin) + (se > 0.f ? sl / se : 0.f);
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
        keys[S * i + s] = key; slots[S * i + s] = (uint32_t)(S * i + s);
      }
      if (tid == 0) { keys[S * B + i] = (uint32_t)(E + r); slots[S * B + i] = (uint32_t)(S * B + i); }
      __syncthreads();
      // pass 2: one gradient row per live negative; T = sum_j a g stays in registers
      float Tre[MAXC][VEC], Tim[MAXC][VEC];
#pragma unroll
      for (int it = 0; it < MAXC; ++it)
#pragma unroll
        for (int q = 0; q < VEC; ++q) Tre[it][q] = Tim[it][q] = 0.f;
      for (int jb = 0; jb < K; jb += NT) {
        const int j = jb + team;
        const int32_t c = j < K ? ni[j] : -1;
        if (!id_ok(c, E)) continue;                     // group-uniform: no shuffles in this loop
        const float a = sD[j];
        const float* ec = ent + (int64_t)c * d;
        float* gc = g0 + (S * i + 2 + j) * (int64_t)d;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
          const int jv = lane + it * LPT;
          if (jv < nvec) {
            float cre[VEC], cim[VEC], ore[VEC], oim[VEC];
            ld<VEC>(ec, jv, cre); ld<VEC>(ec + k, jv, cim);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
              float gre, gim;
              dist_grad<L1>(coord_rotated(Fre[it][q], Fim[it][q], cre[q], cim[q]), gre, gim);
              Tre[it][q] += a * gre; Tim[it][q] += a * gim;
              ore[q] = -(a * gre); oim[q] = -(a * gim);
            }
            store_vec<VEC>(gc + jv * VEC, ore); store_vec<VEC>(gc + k + jv * VEC, oim);
          }
        }
      }
      // the groups of a wave by an xor tree, the waves through LDS in order
#pragma unroll
      for (int it = 0; it < MAXC; ++it) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
#pragma unroll
          for (int m = LPT; m < kWave; m <<= 1) {
            Tre[it][q] += __shfl_xor(Tre[it][q], m, kWave);
            Tim[it][q] += __shfl_xor(Tim[it][q], m, kWave);
          }
        }
        const int jv = lane + it * LPT;
        if (grp == 0 && jv < nvec) { store_vec<VEC>(&sT[wave][jv * VEC], Tre[it]); store_vec<VEC>(&sT[wave][k + jv * VEC], Tim[it]); }
      }
      __syncthreads();
      if (team == 0) {
        // the positive's term, then the rotation undone once: df = T conj(rotation), dtheta = Im T Re F - Re T Im F
        // (of -theta when heads are replaced, hence the sign)
        const float ap = sigmoid_stable(Dp - margin);
        float* gf = g0 + (S * i + (sd ? 1 : 0)) * (int64_t)d; float* gm = g0 + (S * i + (sd ? 0 : 1)) * (int64_t)d;
        float* gr = g0 + (S * B + i) * (int64_t)d;      // its first k floats
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
          const int jv = lane + it * LPT;
          if (jv < nvec) {
            float bre[VEC], bim[VEC], fre[VEC], fim[VEC], mre[VEC], mim[VEC], gth[VEC];
            ld<VEC>(em, jv, bre); ld<VEC>(em + k, jv, bim);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
              const int x = jv * VEC + q;
              const float tre = ((sT[0][x] + sT[1][x]) + sT[2][x]) + sT[3][x];
              const float tim = ((sT[0][k + x] + sT[1][k + x]) + sT[2][k + x]) + sT[3][k + x];
              float gre, gim;
              dist_grad<L1>(coord_rotated(Fre[it][q], Fim[it][q], bre[q], bim[q]), gre, gim);
              const float Tr = tre + ap * gre, Ti = tim + ap * gim;
              const float c = cs[it][q], s = sn[it][q];
              mre[q] = -(ap * gre); mim[q] = -(ap * gim);
              fre[q] = Tr * c + Ti * s; fim[q] = Ti * c - Tr * s;
              const float dth = Ti * Fre[it][q] - Tr * Fim[it][q];
              gth[q] = sd ? -dth : dth;
            }
            store_vec<VEC>(gf + jv * VEC, fre); store_vec<VEC>(gf + k + jv * VEC, fim);
            store_vec<VEC>(gm + jv * VEC, mre); store_vec<VEC>(gm + k + jv * VEC, mim);
            store_vec<VEC>(gr + jv * VEC, gth);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- draw (loop)
// The draw reads no table: ge_transx_adv.hip's loops call rotate_adv_draw_launch for TransE / TransH / TransD as well.
#define GE_TAG_ADVPICK 0x61647670u

// One thread per (row i, negative j).  The positive and the side are ge_transx_draw_batch's of (seed, step, i): the same
// Philox words.  Negative j: the entity the word at row index i K + j under the tag above draws among those that are not
// known completions of (fixed entity, r) -- bernoulli_corrupt_row's pick with ent_lo = 0; -1 when none is free.  A
// relation outside [0, n_rel) gives side 0 and -1s.  Every thread of a row repeats the row's two words and the two
// bisections of known_run: the kernel's time is one thread's chain of dependent loads (about 40 of them through the
// triple list and the sorted keys), which sharing them among a row's threads does not shorten -- one thread per 8
// negatives measured 22.3 against 19.6 to 20.1 us at B 4,096, K 64 -- so the simple form stays.
__global__ __launch_bounds__(kBlock) void rotate_adv_draw_kernel(
    const int32_t* __restrict__ triples, int64_t T, int64_t B, int K, const int64_t* __restrict__ bh_key,
    const int32_t* __restrict__ bh_ent, const int64_t* __restrict__ bt_key, const int32_t* __restrict__ bt_ent,
    int64_t n_known, const uint32_t* __restrict__ tail_threshold, int32_t n_rel, int32_t n_ent, uint64_t seed,
    uint64_t step, int32_t* __restrict__ pos, int32_t* __restrict__ side, int32_t* __restrict__ neg_ent) {
  const uint32_t slo = (uint32_t)step, shi = (uint32_t)(step >> 32);
  const uint32_t klo = (uint32_t)seed, khi = (uint32_t)(seed >> 32);
  const int64_t total = B * K;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = x / K;
    const int j = (int)(x - i * K);
    const uint32_t ilo = (uint32_t)i, ihi = (uint32_t)((uint64_t)i >> 32);
    const uint32_t w = philox_w0(slo, shi, ilo, ihi, klo ^ GE_TAG_TXDRAW, khi);
    const int64_t row = (int64_t)(((uint64_t)w * (uint64_t)T) >> 32);
    const int32_t h = triples[3 * row], t = triples[3 * row + 1], r = triples[3 * row + 2];
    int32_t sd = 0, repl = -1;
    if (r >= 0 && r < n_rel) {
      const bool tail_side = philox_w0(slo, shi, ilo, ihi, klo ^ GE_TAG_BSIDE, khi) < tail_threshold[r];
      sd = tail_side ? 0 : 1;
      const KnownRun run = known_run(tail_side, tail_side ? h : t, r, bh_key, bh_ent, bt_key, bt_ent, n_known, n_rel);
      const uint32_t w_pick = philox_w0(slo, shi, (uint32_t)x, (uint32_t)((uint64_t)x >> 32), klo ^ GE_TAG_ADVPICK, khi);
      repl = pick_free_entity(run, w_pick, 0, n_ent);
    }
    if (j == 0) { pos[3 * i] = h; pos[3 * i + 1] = t; pos[3 * i + 2] = r; side[i] = sd; }
    neg_ent[x] = repl;
  }
}

// ------------------------------------------------------------------------------------------- host side
// The step's workspace: sort keys and slots (in, out) [(K+3)B] each | loss rows [B] | gradient rows [(K+3)B, d] | the
// apply's partials [windows][4][d] | the loop's pos [B,3], side [B], neg_ent [B,K] | rocPRIM's scratch; each padded to
// 256 B.
struct AdvWs {
  uint32_t *keys_in, *keys_out, *slots_in, *slots_out;
  float *loss_rows, *g0, *part;
  int32_t *pos, *side, *neg_ent;
  void* sort_tmp; size_t sort_bytes;
  size_t total;
};

int ws_layout(int64_t E, int64_t R, int32_t d, int64_t B, int32_t K, void* base, AdvWs& w) {
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
  w.part = (float*)take((size_t)nwin * 4 * d * 4);
  w.pos = (int32_t*)take(B * 12); w.side = (int32_t*)take(B * 4); w.neg_ent = (int32_t*)take((size_t)B * K * 4);
  w.sort_bytes = sort_bytes ? sort_bytes : 4;
  w.sort_tmp = take(w.sort_bytes);
  w.total = off;
  return 0;
}

struct AdvArgs {
  const float* ent; const float* rel; int64_t E, R; int d;
  const int32_t* pos; const int32_t* side; const int32_t* neg_ent; int64_t B; int K;
  float margin, alpha;
  float* loss_rows; uint32_t* keys; uint32_t* slots; float* g0;
};

template <bool L1, int VEC, bool GRAD>
void launch_adv_v(int lpt, int grid, hipStream_t st, const AdvArgs& a) {
#define GE_ROT_ADV(L) hipLaunchKernelGGL((rotate_adv_kernel<L1, VEC, L, GRAD>), dim3(grid), dim3(kBlock), 0, st, a.ent, \
                                         a.rel, a.E, a.R, a.d, a.pos, a.side, a.neg_ent, a.B, a.K, a.margin, a.alpha,  \
                                         a.loss_rows, a.keys, a.slots, a.g0)
  switch (lpt) { case 8: GE_ROT_ADV(8); break; case 16: GE_ROT_ADV(16); break; case 32: GE_ROT_ADV(32); break; default: GE_ROT_ADV(64); }
#undef GE_ROT_ADV
}

// v4: the float4 path (d % 8 == 0 and every buffer the kernels vector-load 16-byte aligned)
template <bool GRAD>
int launch_adv(int l1, bool v4, hipStream_t st, const AdvArgs& a) {
  const int nvec = v4 ? a.d / 8 : a.d / 2, lpt = adv_lpt_for(nvec);
  const int grid = grid_for(a.B, 1);
  if (v4) {
    if (l1) launch_adv_v<true, 4, GRAD>(lpt, grid, st, a);
    else launch_adv_v<false, 4, GRAD>(lpt, grid, st, a);
  } else {
    if (l1) launch_adv_v<true, 1, GRAD>(lpt, grid, st, a);
    else launch_adv_v<false, 1, GRAD>(lpt, grid, st, a);
  }
  return launch_status();
}

// One step on caller-given (or drawn) rows; loss = one float.  acc_ent set: the AdaGrad apply.
int step_core(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
              const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K, float margin,
              float alpha, float lr, float* loss, AdvWs& w, hipStream_t st) {
  const int k = d / 2;
  const bool v4 = d % 8 == 0 && aligned16({ent, rel, w.g0, w.part, acc_ent, acc_rel});
  const AdvArgs g{ent, rel, E, R, (int)d, pos, side, neg_ent, B, (int)K, margin, alpha, w.loss_rows, w.keys_in, w.slots_in, w.g0};
  int rc = launch_adv<true>(l1, v4, st, g);
  if (rc) return rc;
  const int64_t n = ((int64_t)K + 3) * B;
  size_t sb = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)n,
                                           0u, key_bits(E, R), st);
  if (e != hipSuccess) return (int)e;
  // one plane: no ent2 / rel2, and a relation row k wide
  const ApplyArgs a{ent, rel, nullptr, nullptr, E, R, (int)d, n, w.keys_out, w.slots_out, w.g0, nullptr, w.part, lr, k};
  const int grid_a = apply_grid(n);
  if (acc_ent) {
    AdaArgs ada;
    static_cast<ApplyArgs&>(ada) = a;
    ada.acc_ent = acc_ent; ada.acc_rel = acc_rel; ada.acc_ent2 = nullptr; ada.acc_rel2 = nullptr;
    if (v4) launch_apply<4>(ada, grid_a, w.loss_rows, B, loss, st);
    else launch_apply<1>(ada, grid_a, w.loss_rows, B, loss, st);
  } else {
    if (v4) launch_apply<4>(a, grid_a, w.loss_rows, B, loss, st);
    else launch_apply<1>(a, grid_a, w.loss_rows, B, loss, st);
  }
  return launch_status();
}

}  // namespace

int rotate_adv_max_negatives() { return kAdvMaxK; }

size_t rotate_adv_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B, int32_t K) {
  AdvWs w;
  if (ws_layout(E, R, d, B, K, nullptr, w) != 0) return 0;
  return w.total;
}

int rotate_adv_loss_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d,
                           const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                           float margin, float alpha, float* out, hipStream_t st) {
  if (B == 0) return 0;
  const bool v4 = d % 8 == 0 && aligned16({ent, rel});
  const AdvArgs g{ent, rel, E, R, (int)d, pos, side, neg_ent, B, (int)K, margin, alpha, out, nullptr, nullptr, nullptr};
  return launch_adv<false>(l1, v4, st, g);
}

int rotate_adv_step_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
                        const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                        float margin, float alpha, float lr, float* loss, void* workspace, size_t workspace_bytes,
                        hipStream_t st) {
  AdvWs w;
  int rc = ws_layout(E, R, d, B, K, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  return step_core(l1, ent, E, rel, R, acc_ent, acc_rel, d, pos, side, neg_ent, B, K, margin, alpha, lr, loss, w, st);
}

int rotate_adv_draw_launch(const SamplerArgs& s, int64_t B, int32_t K, uint64_t seed, uint64_t step, int32_t* pos,
                           int32_t* side, int32_t* neg_ent, hipStream_t st) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(rotate_adv_draw_kernel, dim3(grid_for(B * K, kBlock)), dim3(kBlock), 0, st, s.triples, s.T, B, (int)K,
                     s.bh_key, s.bh_ent, s.bt_key, s.bt_ent, s.n_known, s.tail_threshold, s.n_rel, s.n_ent, seed, step,
                     pos, side, neg_ent);
  return launch_status();
}

int rotate_adv_train_steps_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel,
                               int32_t d, const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps,
                               int64_t B, int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                               size_t workspace_bytes, hipStream_t st) {
  AdvWs w;
  int rc = ws_layout(E, R, d, B, K, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  for (int64_t s = 0; s < n_steps; ++s) {               // draw_then_step's pattern with this loss's draw
    rc = rotate_adv_draw_launch(sa, B, K, seed, first_step + (uint64_t)s, w.pos, w.side, w.neg_ent, st);
    if (rc) return rc;
    rc = step_core(l1, ent, E, rel, R, acc_ent, acc_rel, d, w.pos, w.side, w.neg_ent, B, K, margin, alpha, lr,
                   losses + s, w, st);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace ge
