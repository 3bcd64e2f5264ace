// ge_transx_rank_kern.h -- what the translation models' entity sweeps share between ge_transx_rank.hip (ranks and
// top-k over every entity) and ge_transx_rank_masked.hip (the same with per-relation candidate sets): the projection
// and distance device code, the one distance loop GE_SWEEP_DISTS, the top-k merge kernel and the workspace layouts.
// The masked sweeps live in a translation unit of their own so that the unmasked kernels stay the code they were.
#pragma once
#include "ge_common.h"
#include "ge_launch.h"
#include "ge_topk_dev.h"
#include "ge_trans_dev.h"

#include <algorithm>

namespace ge {
namespace {

constexpr int kRows = 16;                // rows per sweep workgroup

// The projection scalar of entity e under relation r: TransH a = e . n^_r, TransD A_e, else 0.
template <int MODEL>
__device__ __forceinline__ float proj_scalar(const TransTables& T, int64_t e, int64_t r) {
  if constexpr (MODEL == kTransH) return dot_seq(T.ent + e * T.dE, T.aux + r * T.dq, T.dq);
  else if constexpr (MODEL == kTransD) return T.A[e];
  else return 0.f;
}

// Component k of entity e's projection under relation r (a: proj_scalar(e, r)).
template <int MODEL>
__device__ __forceinline__ float proj_elem(const TransTables& T, int64_t e, int64_t r, float a, int k) {
  const float x = MODEL == kTransR ? 0.f : T.ent[e * T.dE + k];
  if constexpr (MODEL == kTransH) return fmaf(-a, T.aux[r * T.dq + k], x);
  else if constexpr (MODEL == kTransD) return fmaf(a, T.aux[r * T.dq + k], x);
  else if constexpr (MODEL == kTransR) {
    const float* m = T.aux + r * (int64_t)T.dq * T.dE + (int64_t)k * T.dE;
    const float* v = T.ent + e * T.dE;
    float p = 0.f;
    for (int j = 0; j < T.dE; ++j) p = fmaf(m[j], v[j], p);
    return p;
  } else return x;
}

// D of candidate c for the row whose query is q (relation r): the sweep's sequence, one lane.
template <int MODEL, bool L1>
__device__ __forceinline__ float dist_one(const TransTables& T, const float* __restrict__ q, int64_t c, int64_t r) {
  const float a = proj_scalar<MODEL>(T, c, r);
  float acc = 0.f;
  for (int k = 0; k < T.dq; ++k) acc = dist_acc(L1, acc, q[k] - proj_elem<MODEL>(T, c, r, a, k));
  return acc;
}


// The distances of one lane's candidate cc (a real row: a padding lane passes E - 1) to the rows [row0, row0 + nrows)
// of a sweep workgroup: declares and fills float acc[kRows], acc[j] for row j.  The rank sweep and the top-k sweep
// share this one distance loop.  It is a macro, not a function, so that the rank sweep's code stays what it was
// (hipcc -O3 schedules and allocates a forceinline function or a lambda epilogue differently: the listings differ).
// Names it reads from the kernel: MODEL, L1, VEC, T, q, rel_of, row0, nrows, cc, dE, dq.  Consecutive rows of one
// relation form a segment that shares the lane's projection scalar.  VEC: entity components per load (4 needs
// dE % 4 == 0, dq % 4 == 0 and a 16-byte aligned ent).
#define GE_SWEEP_DISTS \
  const float* e = T.ent + cc * dE;                                                                \
  float acc[kRows];                                                                                \
  _Pragma("unroll")                                                                                \
  for (int j = 0; j < kRows; ++j) acc[j] = 0.f;                                                    \
  for (int s = 0; s < nrows;) {                                                                    \
    const int64_t r = rel_of[row0 + s];                                                            \
    int s1 = s + 1;                                                                                \
    if constexpr (MODEL != kTransE)                                                                \
      while (s1 < nrows && rel_of[row0 + s1] == r) ++s1;                                           \
    else                                                                                           \
      s1 = nrows;                                                                                  \
    const float a = proj_scalar<MODEL>(T, cc, r);                                                  \
    for (int k = 0; k < dq; k += VEC) {                                                            \
      float p[VEC];                                                                                \
      if constexpr (MODEL == kTransR) {                                                            \
        const float* m = T.aux + r * (int64_t)dq * dE + (int64_t)k * dE;                           \
        _Pragma("unroll")                                                                          \
        for (int v = 0; v < VEC; ++v) p[v] = 0.f;                                                  \
        for (int jj = 0; jj < dE; jj += VEC) {                                                     \
          float x[VEC];                                                                            \
          load_vec<VEC>(e + jj, x);                                                                \
          _Pragma("unroll")                                                                        \
          for (int v = 0; v < VEC; ++v)                                                            \
            _Pragma("unroll")                                                                      \
            for (int z = 0; z < VEC; ++z) p[v] = fmaf(m[(int64_t)v * dE + jj + z], x[z], p[v]);    \
        }                                                                                          \
      } else {                                                                                     \
        load_vec<VEC>(e + k, p);                                                                   \
        if constexpr (MODEL == kTransH) {                                                          \
          _Pragma("unroll")                                                                        \
          for (int v = 0; v < VEC; ++v) p[v] = fmaf(-a, T.aux[r * dq + k + v], p[v]);              \
        } else if constexpr (MODEL == kTransD) {                                                   \
          _Pragma("unroll")                                                                        \
          for (int v = 0; v < VEC; ++v) p[v] = fmaf(a, T.aux[r * dq + k + v], p[v]);               \
        }                                                                                          \
      }                                                                                            \
      _Pragma("unroll")                                                                            \
      for (int j = 0; j < kRows; ++j) {                                                            \
        if (j >= s && j < s1) {                                                                    \
          const float* qj = q + (row0 + j) * dq + k;                                               \
          _Pragma("unroll")                                                                        \
          for (int v = 0; v < VEC; ++v) acc[j] = dist_acc(L1, acc[j], qj[v] - p[v]);               \
        }                                                                                          \
      }                                                                                            \
    }                                                                                              \
    s = s1;                                                                                        \
  }

// ---- top-k (ge_transx_topk / ge_transr_topk): per query row (fixed f, relation r) the first k candidates c in
// ascending (D_c, c), D_c the rank sweep's own value (GE_SWEEP_DISTS), known cells skipped.  D is a sum of |u| or u^2
// from +0, never negative or -0.0, so topk_key's integer order is that order.
constexpr int kTopkMaxK = 128;
constexpr int kTopkLanes = 7;            // pool entries per lane: cap = kp + 256 <= 448 (a candidate block adds <= 256)
constexpr int kMergeFan = 16;            // partial lists per merge wave

struct TopkWs {
  int k, kp, cap;       // kp = topk_kp(k): a pool past kp keys is cut back to k; cap = kp + 256
  u64* pool;            // [B][n_split][cap]
  u64* part;            // [B][n_split][k]: each (row chunk, candidate range)'s k best, sorted, kNoKey-padded
  int32_t* bad;         // [B]: an id out of range, or a NaN distance of a candidate that is not known
};

// One wave per (row, group of up to kMergeFan partial lists): the group's lists -- each sorted, kNoKey-padded -- into
// one (out), or, in the last round (out_id set, one group per row), into the row's ids and distances: -1 / NaN for a
// flagged row, padding -1 / +inf.  Only keys below the running k-th best are taken (a prefix of each list); the pool
// collects them and is cut back to k whenever the next list might not fit (cap >= 2 k).
__global__ __launch_bounds__(kBlock) void topk_merge_kernel(const u64* __restrict__ in, int n_in, u64* __restrict__ out,
                                                            int64_t B, TopkWs W, int32_t* __restrict__ out_id,
                                                            float* __restrict__ out_dist) {
  const int lane = threadIdx.x & (kWave - 1);
  const int n_out = (n_in + kMergeFan - 1) / kMergeFan, k = W.k;
  const int64_t wv = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (wv >= B * n_out) return;
  const int64_t row = wv / n_out;
  const int g0 = (int)(wv % n_out) * kMergeFan, ng = min(kMergeFan, n_in - g0);
  const u64* L0 = in + (row * n_in + g0) * (int64_t)k;
  if (out_id && W.bad[row]) {
    for (int i = lane; i < k; i += kWave) { out_id[row * k + i] = -1; out_dist[row * k + i] = __builtin_nanf(""); }
    return;
  }
  if (ng == 1) {
    for (int i = lane; i < k; i += kWave) {
      const u64 key = L0[i];
      if (out_id) {
        out_id[row * k + i] = key == kNoKey ? -1 : (int32_t)(unsigned)key;
        out_dist[row * k + i] = key == kNoKey ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
      } else {
        out[wv * k + i] = key;
      }
    }
    return;
  }
  u64* pool = W.pool + wv * (int64_t)W.cap;
  int n = 0;
  u64 kth = kNoKey;
  for (int s = 0; s < ng; ++s) {
    const u64* L = L0 + s * (int64_t)k;
    const u64 a = lane < k ? L[lane] : kNoKey, b = lane + 64 < k ? L[lane + 64] : kNoKey;
    const int na = __popcll(__ballot(a < kth)), nb = __popcll(__ballot(b < kth));
    if (na + nb == 0) continue;
    if (n + na + nb > W.cap) {                           // (after the cut n = k, and k + na + nb <= 2 k <= cap)
      kth = topk_shrink<kTopkLanes>(pool, n, k, lane);
      n = k;
      __threadfence_block();
    }
    if (lane < na) pool[n + lane] = a;                   // (a list is sorted: the taken keys are its prefix)
    if (lane < nb) pool[n + na + lane] = b;
    n += na + nb;
    __threadfence_block();
  }
  if (out_id) topk_emit<kTopkLanes>(pool, n, k, lane, out_id + row * k, out_dist + row * k, nullptr);
  else topk_emit<kTopkLanes>(pool, n, k, lane, nullptr, nullptr, out + wv * k);
}

// float4 entity loads: both widths multiples of 4 and ent 16-byte aligned
bool rank_vec4(const float* ent, int32_t d_ent, int32_t d_q) {
  return d_ent % 4 == 0 && d_q % 4 == 0 && ((uintptr_t)ent & 15) == 0;
}

// What the rank and the top-k workspaces begin with: q [B, dq] | rel_of [B] | one int32 per row (rank: the target id;
// top-k: the row's flag) | n^ [R, d] (TransH) or A [E] (TransD).  Offsets; end: the first byte after.
struct SweepPrefix {
  size_t q, rel_of, row, aux, end;
};

SweepPrefix sweep_prefix(const TransModel& m, int64_t B) {
  SweepPrefix P;
  P.q = 0;
  P.rel_of = P.q + align_up(sizeof(float) * (size_t)B * m.dq, 256);
  P.row = P.rel_of + align_up(sizeof(int32_t) * (size_t)B, 256);
  P.aux = P.row + align_up(sizeof(int32_t) * (size_t)B, 256);
  P.end = P.aux + trans_aux_bytes(m, true);
  return P;
}

// ---- the top-k's host side
// candidate ranges per 16-row chunk: about one round of resident workgroups (kMaxBlocks) over the grid, at most one
// range per candidate block.  A function of (B, E) alone, so that the workspace is.
int64_t topk_ranges(int64_t B, int64_t E) {
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (E + kBlock - 1) / kBlock;
  int64_t ns = (kMaxBlocks + n_chunks - 1) / n_chunks;
  return ns < 1 ? 1 : (ns > n_cb ? n_cb : ns);
}

// workspace: the sweeps' prefix (its row array: bad [B]) | pools [B][ns][cap] | partial lists [B][ns][k] | the first
// merge round's lists [B][ceil(ns / kMergeFan)][k]
struct TopkLayout {
  SweepPrefix P;
  size_t pool, part, part2, total;
};

TopkLayout topk_layout(const TransModel& m, int64_t B, int k) {
  const int64_t ns = topk_ranges(B, m.E), cap = topk_kp(k) + kBlock;
  TopkLayout L;
  L.P = sweep_prefix(m, B);
  L.pool = L.P.end;
  L.part = L.pool + align_up(sizeof(u64) * (size_t)(B * ns * cap), 256);
  L.part2 = L.part + align_up(sizeof(u64) * (size_t)(B * ns * k), 256);
  L.total = L.part2 + align_up(sizeof(u64) * (size_t)(B * ((ns + kMergeFan - 1) / kMergeFan) * k), 256);
  return L;
}

// the largest layout of any B' <= B (the ranges shrink as B grows), so that the size is monotone in B, E and k
size_t topk_ws_bytes(const TransModel& m, int64_t B, int32_t k) {
  if (B <= 0 || m.E <= 0 || k < 1 || k > kTopkMaxK) return 0;
  const int64_t n_chunks = (B + kRows - 1) / kRows;
  size_t need = topk_layout(m, B, k).total;
  for (int64_t ch = 1; ch < n_chunks && ch <= kMaxBlocks; ++ch)
    need = std::max(need, topk_layout(m, ch * kRows, k).total);
  return need;
}

}  // namespace
}  // namespace ge
