// ge_rotate.hip -- RotatE (Sun et al., ICLR 2019) on gfx950: the translation model in the complex plane, t ~ h o r with
// |r_j| = 1.  Batch scoring, the margin-hinge step (SGD and AdaGrad), the native loop that draws its own batches, and
// the link-prediction rank sweep over every entity.
//
// Tables: ent [E,d] fp32, d even, k = d / 2, a row [Re (k) | Im (k)] (the ComplEx table's split); rel [R,k] holds
// PHASES theta in radians, unconstrained: never wrapped, never normalised.  The rotation is (c, s) = (cosf, sinf)(theta)
// from the accurate sincosf (its error does not grow with |theta|; the fast intrinsic's does, and phases drift).
// With u_j = h_j e^{i theta_j} - t_j and m_j = sqrtf(Re u_j^2 + Im u_j^2):
//   D = sum_j m_j (l1, the paper's norm)   or   D = sum_j m_j^2 (no square root, as the family's L2).
// Gradients (g_j = u_j / m_j, 0 where m_j == 0: the family's sign(0) = 0; g_j = 2 u_j for the squared norm):
//   dD/dh_j = g_j conj(e^{i theta_j}),  dD/dt_j = -g_j,  dD/dtheta_j = Re g_j (-Im w_j) + Im g_j Re w_j,  w_j = h_j e^{i theta_j}.
//
// The step is the family's (ge_transx.hip): loss = sum_i max(D(pos_i) - D(neg_i) + margin, 0), a pair active iff that
// argument is >= 0; the gradient kernel writes the hinge terms, the keys and five gradient rows per active pair in the
// slot scheme 4i..4i+3 = pos h, pos t, neg h, neg t (keys = entity ids), 4B+i = the relation (key E + r), inactive or
// invalid pairs the sentinel E + R; rocPRIM's stable radix sort of (key, slot); then the family's two apply kernels
// (ge_transx_apply.h), told that a relation row is k wide: a relation slot's gradient is its first k floats, and columns
// k..d-1 of that slot are neither written nor read.  No float atomics: every sum runs in a fixed order.
//
// Ranks: a row kernel stores q once per row -- q = h o e^{i theta} on the tail side, q = t o e^{-i theta} on the head
// side (|c e^{i theta} - t| = |c - t e^{-i theta}|) -- and the sweep, the true distance and the filter pass all evaluate
//   a = q_re,j - c_re,j;  b = q_im,j - c_im,j;  m2 = fmaf(b, b, a * a);  part += l1 ? sqrtf(m2) : m2     for j in order
// on that stored q (rot_term: every operation explicit, so contraction cannot differ between them), a partial sum per
// block of kRotSumBlock coordinates, the partial sums added in block order: at k = 512 one serial fp32 sum lies ten
// times further from the exact one than a pairwise sum does.  The target never ranks before itself and the filter
// counts exactly the cells the sweep counted.
#include <rocprim/device/device_radix_sort.hpp>

#include "ge_common.h"
#include "ge_launch.h"
#include "ge_rotate_dev.h"     // Coord, coord, dist_term, dist_grad, kRotMaxDim
#include "ge_transx_apply.h"

namespace ge {
namespace {

constexpr int kRows = 16;                 // rows per sweep workgroup
constexpr int kKnownTile = 128;           // ge_known_cells' tile edge
constexpr int kRotSumBlock = 32;          // coordinates per partial sum of a rank distance (a multiple of 4)

__device__ __forceinline__ bool id_ok(int32_t x, int64_t n) { return x >= 0 && x < n; }

// ------------------------------------------------------------------------------------------- score
// One group of LPT lanes per triple; a lane takes chunks of VEC complex coordinates.
template <bool L1, int VEC, int LPT>
__global__ __launch_bounds__(kBlock) void rotate_score_kernel(const float* __restrict__ ent, const float* __restrict__ rel,
                                                              int64_t E, int64_t R, int d,
                                                              const int32_t* __restrict__ tri, int64_t B,
                                                              float* __restrict__ out) {
  constexpr int G = kWave / LPT;                        // triples per wave
  const int lane = threadIdx.x & (LPT - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int k = d / 2, nvec = k / VEC;
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
    const float* th = rel + (int64_t)r * k;
    float D = 0.f;
    for (int j = lane; j < nvec; j += LPT) {
      float hre[VEC], him[VEC], tre[VEC], tim[VEC], p[VEC];
      ld<VEC>(eh, j, hre); ld<VEC>(eh + k, j, him); ld<VEC>(et, j, tre); ld<VEC>(et + k, j, tim); ld<VEC>(th, j, p);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        float s, c;
        sincosf(p[q], &s, &c);
        D += dist_term<L1>(coord(hre[q], him[q], tre[q], tim[q], c, s));
      }
    }
    D = group_sum<LPT>(D);
    if (i < B && lane == 0) out[i] = ok ? D : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------- gradient
// One group of LPT lanes per pair.  A pair's positive and negative share r, hence (c, s): the rotation of each of the
// lane's coordinates is computed once, in the distance pass, and kept in registers for the gradient pass (a lane holds
// at most MAXC chunks: nvec <= LPT below 64 lanes, k <= 512 at 64).
template <bool L1, int VEC, int LPT>
__global__ __launch_bounds__(kBlock) void rotate_grad_kernel(
    const float* __restrict__ ent, const float* __restrict__ rel, int64_t E, int64_t R, int d,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int64_t B, float margin, float* __restrict__ hinge,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ slots, float* __restrict__ g0) {
  constexpr int G = kWave / LPT;
  constexpr int MAXC = LPT < kWave ? 1 : kRotMaxDim / 2 / VEC / kWave;
  const int lane = threadIdx.x & (LPT - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int k = d / 2, nvec = k / VEC;
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
    const float* th = rel + (int64_t)r * k;
    // pass 1: the rotations and both distances
    float cs[MAXC][VEC], sn[MAXC][VEC];
    float Dp = 0.f, Dn = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
      const int j = lane + it * LPT;
      if (j < nvec) {
        float are[VEC], aim[VEC], bre[VEC], bim[VEC], p[VEC];
        ld<VEC>(th, j, p);
#pragma unroll
        for (int q = 0; q < VEC; ++q) sincosf(p[q], &sn[it][q], &cs[it][q]);
        ld<VEC>(eh, j, are); ld<VEC>(eh + k, j, aim); ld<VEC>(et, j, bre); ld<VEC>(et + k, j, bim);
#pragma unroll
        for (int q = 0; q < VEC; ++q) Dp += dist_term<L1>(coord(are[q], aim[q], bre[q], bim[q], cs[it][q], sn[it][q]));
        ld<VEC>(fh, j, are); ld<VEC>(fh + k, j, aim); ld<VEC>(ft, j, bre); ld<VEC>(ft + k, j, bim);
#pragma unroll
        for (int q = 0; q < VEC; ++q) Dn += dist_term<L1>(coord(are[q], aim[q], bre[q], bim[q], cs[it][q], sn[it][q]));
      }
    }
    Dp = group_sum<LPT>(Dp); Dn = group_sum<LPT>(Dn);
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
    // pass 2: the five gradient rows.  The positive's rows carry +dD+, the negative's -dD-; the relation's both.
    float* gph = g0 + (4 * i + 0) * (int64_t)d; float* gpt = g0 + (4 * i + 1) * (int64_t)d;
    float* gnh = g0 + (4 * i + 2) * (int64_t)d; float* gnt = g0 + (4 * i + 3) * (int64_t)d;
    float* gr = g0 + (4 * B + i) * (int64_t)d;        // its first k floats
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
      const int j = lane + it * LPT;
      if (j < nvec) {
        float are[VEC], aim[VEC], bre[VEC], bim[VEC];
        float hre[VEC], him[VEC], tre[VEC], tim[VEC], gth[VEC];
        ld<VEC>(eh, j, are); ld<VEC>(eh + k, j, aim); ld<VEC>(et, j, bre); ld<VEC>(et + k, j, bim);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float c = cs[it][q], s = sn[it][q];
          const Coord x = coord(are[q], aim[q], bre[q], bim[q], c, s);
          float gre, gim;
          dist_grad<L1>(x, gre, gim);
          hre[q] = gre * c + gim * s; him[q] = gim * c - gre * s;
          tre[q] = -gre; tim[q] = -gim;
          gth[q] = gim * x.wre - gre * x.wim;
        }
        store_vec<VEC>(gph + j * VEC, hre); store_vec<VEC>(gph + k + j * VEC, him);
        store_vec<VEC>(gpt + j * VEC, tre); store_vec<VEC>(gpt + k + j * VEC, tim);
        ld<VEC>(fh, j, are); ld<VEC>(fh + k, j, aim); ld<VEC>(ft, j, bre); ld<VEC>(ft + k, j, bim);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float c = cs[it][q], s = sn[it][q];
          const Coord x = coord(are[q], aim[q], bre[q], bim[q], c, s);
          float gre, gim;
          dist_grad<L1>(x, gre, gim);
          hre[q] = -(gre * c + gim * s); him[q] = -(gim * c - gre * s);
          tre[q] = gre; tim[q] = gim;
          gth[q] -= gim * x.wre - gre * x.wim;
        }
        store_vec<VEC>(gnh + j * VEC, hre); store_vec<VEC>(gnh + k + j * VEC, him);
        store_vec<VEC>(gnt + j * VEC, tre); store_vec<VEC>(gnt + k + j * VEC, tim);
        store_vec<VEC>(gr + j * VEC, gth);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- ranks
// The one arithmetic of a rank distance: coordinate (cre, cim) of a candidate against (qre, qim) of the row's stored q.
__device__ __forceinline__ float rot_term(bool l1, float acc, float qre, float qim, float cre, float cim) {
  const float a = qre - cre, b = qim - cim;
  const float m2 = fmaf(b, b, __fmul_rn(a, a));
  return __fadd_rn(acc, l1 ? sqrtf(m2) : m2);
}

// D of candidate row c (entity row [Re | Im]) for the stored query q: the sweep's sequence, one lane.  (At
// k <= kRotSumBlock the one partial sum is added to 0: the distance is the serial sum.)
template <bool L1>
__device__ __forceinline__ float rot_dist(const float* __restrict__ q, const float* __restrict__ c, int k) {
  float acc = 0.f;
  for (int j0 = 0; j0 < k; j0 += kRotSumBlock) {
    const int j1 = j0 + kRotSumBlock < k ? j0 + kRotSumBlock : k;
    float part = 0.f;
    for (int j = j0; j < j1; ++j) part = rot_term(L1, part, q[j], q[k + j], c[j], c[k + j]);
    acc = __fadd_rn(acc, part);
  }
  return acc;
}

// One thread per row: ids checked, q written, the target, D_true, and the counters' initial values: 0, or -1 for a row
// with an id out of range, whose NaN D_true keeps sweep and filter from counting.
template <bool L1>
__global__ __launch_bounds__(kBlock) void rotate_rank_row_kernel(const float* __restrict__ ent,
                                                                 const float* __restrict__ rel, int64_t E, int64_t R,
                                                                 int d, const int32_t* __restrict__ tri, int64_t B,
                                                                 int head, float* __restrict__ q,
                                                                 int32_t* __restrict__ tid, float* __restrict__ true_dist,
                                                                 int32_t* __restrict__ n_before,
                                                                 int32_t* __restrict__ n_known) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
  const bool ok = id_ok(h, E) && id_ok(t, E) && id_ok(r, R);
  if (!ok) h = t = r = 0;
  const int k = d / 2;
  const int32_t fixed = head ? t : h, target = head ? h : t;
  const float* f = ent + (int64_t)fixed * d;
  const float* th = rel + (int64_t)r * k;
  float* qi = q + i * d;
  for (int j = 0; j < k; ++j) {
    float s, c;
    sincosf(th[j], &s, &c);
    if (head) s = -s;                                   // e^{-i theta}
    qi[j] = f[j] * c - f[k + j] * s;
    qi[k + j] = f[j] * s + f[k + j] * c;
  }
  tid[i] = target;
  true_dist[i] = ok ? rot_dist<L1>(qi, ent + (int64_t)target * d, k) : __builtin_nanf("");
  n_before[i] = ok ? 0 : -1;
  n_known[i] = ok ? 0 : -1;
}

// The sweep.  blockIdx.x: rows [x * kRows, +kRows); candidate blocks of 256 (one lane each) strided by gridDim.y; the
// query values are uniform (scalar loads).  Per row: ballot + popcount of the before-test, summed over the workgroup's
// four waves in LDS, one integer atomic per row and workgroup.  VEC: coordinates per entity load (4 needs k % 4 == 0 and
// a 16-byte aligned ent).
template <bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void rotate_rank_sweep_kernel(const float* __restrict__ ent, int64_t E, int d,
                                                                   const float* __restrict__ q,
                                                                   const int32_t* __restrict__ tid,
                                                                   const float* __restrict__ true_dist, int64_t B,
                                                                   int32_t* __restrict__ n_before,
                                                                   float* __restrict__ scores) {
  __shared__ int32_t wave_cnt[kBlock / kWave][kRows];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nrows = (int)(B - row0 < kRows ? B - row0 : kRows);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int k = d / 2;
  int32_t tt[kRows], cnt[kRows];
  float dt[kRows];
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const bool in = j < nrows;
    tt[j] = in ? tid[row0 + j] : 0;
    dt[j] = in ? true_dist[row0 + j] : 0.f;
    cnt[j] = 0;
  }
  for (int64_t cb = blockIdx.y; cb * kBlock < E; cb += gridDim.y) {
    const int64_t c = cb * kBlock + threadIdx.x;
    const bool valid = c < E;
    const float* e = ent + (valid ? c : E - 1) * d;     // a padding lane reads a real row; its result is dropped
    float acc[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) acc[j] = 0.f;
    for (int x0 = 0; x0 < k; x0 += kRotSumBlock) {      // rot_dist's sequence: a partial sum per block of coordinates
      const int x1 = x0 + kRotSumBlock < k ? x0 + kRotSumBlock : k;
      float part[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) part[j] = 0.f;
      for (int x = x0; x < x1; x += VEC) {
        float cre[VEC], cim[VEC];
        load_vec<VEC>(e + x, cre); load_vec<VEC>(e + k + x, cim);
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
          if (j < nrows) {
            const float* qj = q + (row0 + j) * d + x;
#pragma unroll
            for (int v = 0; v < VEC; ++v) part[j] = rot_term(L1, part[j], qj[v], qj[k + v], cre[v], cim[v]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) acc[j] = __fadd_rn(acc[j], part[j]);
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (j < nrows) {
        const bool before = valid && (acc[j] < dt[j] || (acc[j] == dt[j] && c < tt[j]));
        cnt[j] += __popcll(__ballot(before));
        if (scores && valid) scores[(row0 + j) * E + c] = acc[j];
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kRows; ++j) wave_cnt[w][j] = cnt[j];
  }
  __syncthreads();
  if ((int)threadIdx.x < nrows) {
    int32_t tot = 0;
#pragma unroll
    for (int x = 0; x < kBlock / kWave; ++x) tot += wave_cnt[x][threadIdx.x];
    if (tot) atomicAdd(&n_before[row0 + threadIdx.x], tot);
  }
}

// One thread per known cell (grid-stride over known_off[n_tiles] entries; the cell's tile by binary search): D
// recomputed on the row's stored q, integer atomic when it ranks before.
template <bool L1>
__global__ __launch_bounds__(kBlock) void rotate_rank_filter_kernel(const float* __restrict__ ent, int64_t E, int d,
                                                                    const float* __restrict__ q,
                                                                    const int32_t* __restrict__ tid,
                                                                    const float* __restrict__ true_dist, int64_t B,
                                                                    const int32_t* __restrict__ off,
                                                                    const uint16_t* __restrict__ rc, int64_t n_tiles,
                                                                    int32_t* __restrict__ n_known) {
  const int64_t total = off[n_tiles];
  const int64_t n_ct = (E + kKnownTile - 1) / kKnownTile;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n_tiles;                       // the last tile with off[tile] <= x
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= x) lo = mid; else hi = mid;
    }
    const int cell = rc[x];
    const int64_t row = (lo / n_ct) * kKnownTile + (cell >> 7), col = (lo % n_ct) * kKnownTile + (cell & 127);
    if (row >= B || col >= E) continue;
    const float dt = true_dist[row];
    const float D = rot_dist<L1>(q + row * d, ent + col * d, d / 2);
    if (D < dt || (D == dt && col < tid[row])) atomicAdd(&n_known[row], 1);
  }
}

// ------------------------------------------------------------------------------------------- host side
inline int lpt_for(int nvec) { return nvec <= 8 ? 8 : nvec <= 16 ? 16 : nvec <= 32 ? 32 : 64; }

// The step's workspace: sort keys and slots (in, out) [5B] each | hinge [B] | gradient rows [5B, d] | the apply's
// partials [windows][4][d] | the loop's pos, neg [B,3] | rocPRIM's scratch; each padded to 256 B.
struct RotWs {
  uint32_t *keys_in, *keys_out, *slots_in, *slots_out;
  float *hinge, *g0, *part;
  int32_t *pos, *neg;
  void* sort_tmp; size_t sort_bytes;
  size_t total;
};

int ws_layout(int64_t E, int64_t R, int32_t d, int64_t B, void* base, RotWs& w) {
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
  w.g0 = (float*)take((size_t)n * d * 4);
  w.part = (float*)take((size_t)nwin * 4 * d * 4);
  w.pos = (int32_t*)take(B * 12); w.neg = (int32_t*)take(B * 12);
  w.sort_bytes = sort_bytes ? sort_bytes : 4;
  w.sort_tmp = take(w.sort_bytes);
  w.total = off;
  return 0;
}

template <bool L1, int VEC>
void launch_score_v(int lpt, int grid, hipStream_t st, const float* ent, const float* rel, int64_t E, int64_t R, int d,
                    const int32_t* tri, int64_t B, float* out) {
#define GE_ROT_SCORE(L) hipLaunchKernelGGL((rotate_score_kernel<L1, VEC, L>), dim3(grid), dim3(kBlock), 0, st, ent, rel, \
                                           E, R, d, tri, B, out)
  switch (lpt) { case 8: GE_ROT_SCORE(8); break; case 16: GE_ROT_SCORE(16); break; case 32: GE_ROT_SCORE(32); break; default: GE_ROT_SCORE(64); }
#undef GE_ROT_SCORE
}

template <bool L1, int VEC>
void launch_grad_v(int lpt, int grid, hipStream_t st, const float* ent, const float* rel, int64_t E, int64_t R, int d,
                   const int32_t* pos, const int32_t* neg, int64_t B, float margin, const RotWs& w) {
#define GE_ROT_GRAD(L) hipLaunchKernelGGL((rotate_grad_kernel<L1, VEC, L>), dim3(grid), dim3(kBlock), 0, st, ent, rel, E, \
                                          R, d, pos, neg, B, margin, w.hinge, w.keys_in, w.slots_in, w.g0)
  switch (lpt) { case 8: GE_ROT_GRAD(8); break; case 16: GE_ROT_GRAD(16); break; case 32: GE_ROT_GRAD(32); break; default: GE_ROT_GRAD(64); }
#undef GE_ROT_GRAD
}

// One step on caller-given (or drawn) pos / neg; loss = one float.  acc_ent set: the AdaGrad apply.
int step_core(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
              const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss, RotWs& w,
              hipStream_t st) {
  const int k = d / 2;
  const bool v4 = d % 8 == 0 && aligned16({ent, rel, w.g0, w.part, acc_ent, acc_rel});
  const int nvec = v4 ? k / 4 : k, lpt = lpt_for(nvec);
  const int grid = grid_for((B + kWave / lpt - 1) / (kWave / lpt), kBlock / kWave);
  if (v4) {
    if (l1) launch_grad_v<true, 4>(lpt, grid, st, ent, rel, E, R, (int)d, pos, neg, B, margin, w);
    else launch_grad_v<false, 4>(lpt, grid, st, ent, rel, E, R, (int)d, pos, neg, B, margin, w);
  } else {
    if (l1) launch_grad_v<true, 1>(lpt, grid, st, ent, rel, E, R, (int)d, pos, neg, B, margin, w);
    else launch_grad_v<false, 1>(lpt, grid, st, ent, rel, E, R, (int)d, pos, neg, B, margin, w);
  }
  int rc = launch_status();
  if (rc) return rc;
  const int64_t n = 5 * B;
  size_t sb = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)n,
                                           0u, key_bits(E, R), st);
  if (e != hipSuccess) return (int)e;
  // one plane: no ent2 / rel2, and a relation row k wide
  const ApplyArgs a{ent, rel, nullptr, nullptr, E, R, (int)d, n, w.keys_out, w.slots_out, w.g0, nullptr, w.part, lr, k};
  const int grid_a = apply_grid(n);
  if (acc_ent) {
    AdaArgs g;
    static_cast<ApplyArgs&>(g) = a;
    g.acc_ent = acc_ent; g.acc_rel = acc_rel; g.acc_ent2 = nullptr; g.acc_rel2 = nullptr;
    if (v4) launch_apply<4>(g, grid_a, w.hinge, B, loss, st);
    else launch_apply<1>(g, grid_a, w.hinge, B, loss, st);
  } else {
    if (v4) launch_apply<4>(a, grid_a, w.hinge, B, loss, st);
    else launch_apply<1>(a, grid_a, w.hinge, B, loss, st);
  }
  return launch_status();
}

// The rank workspace: q [B, d] | the target ids [B], each padded to 256 B.
struct RankWs { size_t q, tid, end; };

RankWs rank_ws(int32_t d, int64_t B) {
  RankWs P;
  P.q = 0;
  P.tid = P.q + align_up(sizeof(float) * (size_t)B * d, 256);
  P.end = P.tid + align_up(sizeof(int32_t) * (size_t)B, 256);
  return P;
}

// The sweep's grid, the family's rule: 16-row chunks x about two waves of resident workgroups over the grid, at most
// one per candidate block.
dim3 rank_grid(int64_t B, int64_t E) {
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (E + kBlock - 1) / kBlock;
  int64_t gy = (2 * kMaxBlocks + n_chunks - 1) / n_chunks;
  gy = gy < 1 ? 1 : (gy > n_cb ? n_cb : gy);
  return dim3((unsigned)n_chunks, (unsigned)gy);
}

template <bool L1>
int run_rank(const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const int32_t* tri, int64_t B,
             int head, const RankOut& o, void* ws, hipStream_t st) {
  const RankWs P = rank_ws(d, B);
  float* q = (float*)((char*)ws + P.q);
  int32_t* tid = (int32_t*)((char*)ws + P.tid);
  hipLaunchKernelGGL((rotate_rank_row_kernel<L1>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ent,
                     rel, E, R, (int)d, tri, B, head, q, tid, o.true_dist, o.n_before, o.n_known_before);
  if (d % 8 == 0 && aligned16({ent}))
    hipLaunchKernelGGL((rotate_rank_sweep_kernel<L1, 4>), rank_grid(B, E), dim3(kBlock), 0, st, ent, E, (int)d, q, tid,
                       o.true_dist, B, o.n_before, o.scores_out);
  else
    hipLaunchKernelGGL((rotate_rank_sweep_kernel<L1, 1>), rank_grid(B, E), dim3(kBlock), 0, st, ent, E, (int)d, q, tid,
                       o.true_dist, B, o.n_before, o.scores_out);
  if (o.known_off && o.known_rc) {
    const int64_t n_tiles = ((B + kKnownTile - 1) / kKnownTile) * ((E + kKnownTile - 1) / kKnownTile);
    hipLaunchKernelGGL((rotate_rank_filter_kernel<L1>), dim3(1024), dim3(kBlock), 0, st, ent, E, (int)d, q, tid,
                       o.true_dist, B, o.known_off, o.known_rc, n_tiles, o.n_known_before);
  }
  return launch_status();
}

}  // namespace

int rotate_max_dim() { return kRotMaxDim; }

size_t rotate_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B) {
  RotWs w;
  if (ws_layout(E, R, d, B, nullptr, w) != 0) return 0;
  return w.total;
}

int rotate_score_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const int32_t* tri,
                        int64_t B, float* out, hipStream_t st) {
  if (B == 0) return 0;
  const bool v4 = d % 8 == 0 && aligned16({ent, rel});
  const int nvec = v4 ? d / 8 : d / 2, lpt = lpt_for(nvec);
  const int grid = grid_for((B + kWave / lpt - 1) / (kWave / lpt), kBlock / kWave);
  if (v4) {
    if (l1) launch_score_v<true, 4>(lpt, grid, st, ent, rel, E, R, (int)d, tri, B, out);
    else launch_score_v<false, 4>(lpt, grid, st, ent, rel, E, R, (int)d, tri, B, out);
  } else {
    if (l1) launch_score_v<true, 1>(lpt, grid, st, ent, rel, E, R, (int)d, tri, B, out);
    else launch_score_v<false, 1>(lpt, grid, st, ent, rel, E, R, (int)d, tri, B, out);
  }
  return launch_status();
}

int rotate_step_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
                    const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss,
                    void* workspace, size_t workspace_bytes, hipStream_t st) {
  RotWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  return step_core(l1, ent, E, rel, R, acc_ent, acc_rel, d, pos, neg, B, margin, lr, loss, w, st);
}

int rotate_train_steps_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel,
                           int32_t d, const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps,
                           int64_t B, float margin, float lr, float* losses, void* workspace, size_t workspace_bytes,
                           hipStream_t st) {
  RotWs w;
  int rc = ws_layout(E, R, d, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  return draw_then_step(sa, B, seed, first_step, n_steps, w.pos, w.neg, st, [&](int64_t s) {
    return step_core(l1, ent, E, rel, R, acc_ent, acc_rel, d, w.pos, w.neg, B, margin, lr, losses + s, w, st);
  });
}

size_t rotate_rank_ws_bytes(int32_t d, int64_t B) { return rank_ws(d, B).end; }

int rotate_rank_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const int32_t* tri,
                       int64_t B, int cand_is_head, const RankOut& o, void* workspace, size_t workspace_bytes,
                       hipStream_t st) {
  if (workspace_bytes < rotate_rank_ws_bytes(d, B)) return GE_ENOMEM;
  const int head = cand_is_head ? 1 : 0;
  return l1 ? run_rank<true>(ent, E, rel, R, d, tri, B, head, o, workspace, st)
            : run_rank<false>(ent, E, rel, R, d, tri, B, head, o, workspace, st);
}

}  // namespace ge
