// ge_transx_rank_kern.h -- what the translation models' entity sweeps share between ge_transx_rank.hip (ranks and
// top-k over every entity) and ge_transx_rank_masked.hip (the same with per-relation candidate sets): everything but
// the loops of the four sweep kernels.  Device: the projection and distance code, the set test, the row and filter
// kernels (instantiated with a SetArgs they check the row's set), the sweeps' shared texts as macros (GE_SWEEP_DISTS,
// GE_RANK_COMMIT, GE_TOPK_*) and the top-k merge kernel.  Host: the workspace layouts and their carving, the grid
// rules, the launches of the row and filter kernels and the merge rounds.
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

// ---- candidate sets (SetArgs, ge_launch.h): a row's set index is -1 (unrestricted), in [0, n_sets), or bad
constexpr int kSetFree = -1;             // a sanitised set index: unrestricted
constexpr int kSetBad = -2;              //                        index out of range: the row admits nothing

__device__ __forceinline__ bool set_ok(int32_t s, int32_t n_sets) { return s >= -1 && s < n_sets; }

// The word of set s (in [0, n_sets)) that holds entity c's bit (c < E), and that bit of it.
__device__ __forceinline__ uint32_t mask_word(const SetArgs& S, int32_t s, int64_t c) {
  return S.mask[(int64_t)s * S.mw + (c >> 5)];
}
__device__ __forceinline__ unsigned mask_bit(uint32_t word, int64_t c) { return (word >> (c & 31)) & 1u; }

// The row and filter kernels end in a pack SETS: empty, or one SetArgs, whose sets they then check.

// One thread per row: q, the sanitised relation and target, D_true, and the counters' initial values: 0, or -1 for a
// bad row (an id out of range; with sets: or a bad set index), whose NaN D_true keeps sweep and filter from counting.
template <int MODEL, bool L1, class... SETS>
__global__ __launch_bounds__(kBlock) void rank_row_kernel(TransTables T, const int32_t* __restrict__ tri, int64_t B,
                                                          int head, float* __restrict__ q, int32_t* __restrict__ rel_of,
                                                          int32_t* __restrict__ tid, float* __restrict__ true_dist,
                                                          int32_t* __restrict__ n_before, int32_t* __restrict__ n_known,
                                                          SETS... sets) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
  bool ok = h >= 0 && h < T.E && t >= 0 && t < T.E && r >= 0 && r < T.R;
  if (!ok) h = t = r = 0;
  if constexpr (sizeof...(SETS) != 0) ok = ok && set_ok((sets, ...).row_set[i], (sets, ...).n_sets);
  const int32_t fixed = head ? t : h, target = head ? h : t;
  float* qi = q + i * T.dq;
  const float a = proj_scalar<MODEL>(T, fixed, r);
  for (int k = 0; k < T.dq; ++k) {
    const float p = proj_elem<MODEL>(T, fixed, r, a, k), rk = T.rel[(int64_t)r * T.dq + k];
    qi[k] = head ? p - rk : p + rk;
  }
  rel_of[i] = r;
  tid[i] = target;
  true_dist[i] = ok ? dist_one<MODEL, L1>(T, qi, target, r) : __builtin_nanf("");
  n_before[i] = ok ? 0 : -1;
  n_known[i] = ok ? 0 : -1;
}

// One thread per known cell (grid-stride over known_off[n_tiles] entries; the cell's tile by binary search): recompute
// D with the row's operands, integer atomic when it ranks before.  With sets: a cell whose column the row's set does
// not admit is skipped.
template <int MODEL, bool L1, class... SETS>
__global__ __launch_bounds__(kBlock) void rank_filter_kernel(TransTables T, const float* __restrict__ q,
                                                             const int32_t* __restrict__ rel_of,
                                                             const int32_t* __restrict__ tid,
                                                             const float* __restrict__ true_dist, int64_t B,
                                                             const int32_t* __restrict__ off,
                                                             const uint16_t* __restrict__ rc, int64_t n_tiles,
                                                             int32_t* __restrict__ n_known, SETS... sets) {
  const int64_t total = off[n_tiles];
  const int64_t n_ct = (T.E + kTile - 1) / kTile;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n_tiles;                       // the last tile with off[tile] <= x
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= x) lo = mid; else hi = mid;
    }
    const int cell = rc[x];
    const int64_t row = (lo / n_ct) * kTile + (cell >> 7), col = (lo % n_ct) * kTile + (cell & 127);
    if (row >= B || col >= T.E) continue;
    if constexpr (sizeof...(SETS) != 0) {
      const SetArgs& S = (sets, ...);
      const int32_t s = S.row_set[row];
      if (!set_ok(s, S.n_sets)) continue;               // a bad row: its counters stay -1
      if (s >= 0 && !mask_bit(mask_word(S, s, col), col)) continue;
    }
    const float dt = true_dist[row];
    const float D = dist_one<MODEL, L1>(T, q + row * T.dq, col, rel_of[row]);
    if (D < dt || (D == dt && col < tid[row])) atomicAdd(&n_known[row], 1);
  }
}

// The end of a rank sweep: the four waves' counts cnt[kRows] summed in LDS (wave_cnt[kBlock / kWave][kRows]), one
// integer atomic per row and workgroup.  A macro for GE_SWEEP_DISTS' reason.  Reads the kernel's wave_cnt, cnt,
// n_before, row0, nrows, lane, w.
#define GE_RANK_COMMIT \
  if (lane == 0) {                                                                                 \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < kRows; ++j) wave_cnt[w][j] = cnt[j];                                       \
  }                                                                                                \
  __syncthreads();                                                                                 \
  if (threadIdx.x < nrows) {                                                                       \
    int32_t tot = 0;                                                                               \
    _Pragma("unroll")                                                                              \
    for (int x = 0; x < kBlock / kWave; ++x) tot += wave_cnt[x][threadIdx.x];                      \
    if (tot) atomicAdd(&n_before[row0 + threadIdx.x], tot);                                        \
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
// (k <= kTopkMaxK: ge_sweep_route.h)
constexpr int kTopkLanes = 7;            // pool entries per lane: cap = kp + 256 <= 448 (a candidate block adds <= 256)
constexpr int kMergeFan = 16;            // partial lists per merge wave

struct TopkWs {
  int k, kp, cap;       // kp = topk_kp(k): a pool past kp keys is cut back to k; cap = kp + 256
  u64* pool;            // [B][n_split][cap]
  u64* part;            // [B][n_split][k]: each (row chunk, candidate range)'s k best, sorted, kNoKey-padded
  int32_t* bad;         // [B]: an id out of range, or a NaN distance of a candidate that is not known
};

// One thread per query row: q (as rank_row_kernel forms it), the sanitised relation and the row's flag (an id out of
// range; with sets: or a bad set index).
template <int MODEL, class... SETS>
__global__ __launch_bounds__(kBlock) void topk_row_kernel(TransTables T, const int32_t* __restrict__ qr, int64_t B,
                                                          int head, float* __restrict__ q, int32_t* __restrict__ rel_of,
                                                          int32_t* __restrict__ bad, SETS... sets) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t f = qr[2 * i], r = qr[2 * i + 1];
  bool ok = f >= 0 && f < T.E && r >= 0 && r < T.R;
  if (!ok) f = r = 0;
  if constexpr (sizeof...(SETS) != 0) ok = ok && set_ok((sets, ...).row_set[i], (sets, ...).n_sets);
  float* qi = q + i * T.dq;
  const float a = proj_scalar<MODEL>(T, f, r);
  for (int k = 0; k < T.dq; ++k) {
    const float p = proj_elem<MODEL>(T, f, r, a, k), rk = T.rel[(int64_t)r * T.dq + k];
    qi[k] = head ? p - rk : p + rk;
  }
  rel_of[i] = r;
  bad[i] = ok ? 0 : 1;
}

// The texts of a top-k sweep around its distance loop, macros for GE_SWEEP_DISTS' reason.  A workgroup keeps, per row,
// a pool of keys in the workspace (row j's at pool0 + j * pstride), and in LDS the pool's fill[kRows], the row's k-th
// best key kth[kRows] (kNoKey until a cut-back) and the known bitmap bm[kRows][kBlock / 32].  They read those and the
// kernel's known_off, known_rc, cb, n_ct, rtile, rsub, acc, c, W, row0, nrows, ns, nan_rows, lane, w.

// bm = the known cells of the workgroup's rows x the 256 candidates of source block cb, from ge_known_cells' lists of
// the (at most two) 128 x 128 tiles the block covers.  The whole workgroup runs it (two barriers).
#define GE_TOPK_KNOWN_BITMAP \
  if (threadIdx.x < kRows * kBlock / 32) (&bm[0][0])[threadIdx.x] = 0u;                            \
  __syncthreads();                                                                                 \
  for (int h = 0; h < 2 && 2 * cb + h < n_ct; ++h) {                                               \
    const int64_t tile = rtile * n_ct + 2 * cb + h;                                                \
    const int32_t x1 = known_off[tile + 1];                                                        \
    for (int32_t x = known_off[tile] + threadIdx.x; x < x1; x += kBlock) {                         \
      const int cell = known_rc[x], rl = (cell >> 7) - rsub, cl = (cell & 127) + kTile * h;        \
      if (rl >= 0 && rl < kRows) atomicOr(&bm[rl][cl >> 5], 1u << (cl & 31));                      \
    }                                                                                              \
  }                                                                                                \
  __syncthreads();

// bm's bit of row j and this lane's candidate of the source block
__device__ __forceinline__ bool known_bit(const uint32_t (&bm)[kRows][kBlock / 32], int j) {
  return (bm[j][threadIdx.x >> 5] >> (threadIdx.x & 31)) & 1u;
}

// The lane offers its candidate c to row j (ON: c is a real candidate that row j admits and does not know).  A NaN
// flags the row; a key below the row's k-th best goes to the pool: ballot + prefix count, one LDS atomic per wave and
// row.  (The index stays below cap: <= kp keys before a block or batch, <= 256 in it.)
#define GE_TOPK_OFFER(ON) \
  const float D = acc[j];                                                                          \
  if (__ballot((ON) && D != D)) nan_rows |= 1u << j;                                               \
  const u64 key = topk_key(D, (int32_t)c);                                                         \
  const bool take = (ON) && D < __builtin_inff() && key < kth[j];                                  \
  const u64 m = __ballot(take);                                                                    \
  if (m) {                                                                                         \
    int base = 0;                                                                                  \
    if (lane == 0) base = atomicAdd(&fill[j], __popcll(m));                                        \
    base = __shfl(base, 0);                                                                        \
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); \
    if (take) pool0[j * pstride + base + below] = key;                                             \
  }

// After a block's or a batch's offers are in (a barrier): the pools past kp keys are cut back to k; wave w cuts rows
// 4 w ... 4 w + 3.
#define GE_TOPK_CUT \
  for (int jj = 0; jj < kRows / 4; ++jj) {                                                         \
    const int rl = w * (kRows / 4) + jj;                                                           \
    const int n = __builtin_amdgcn_readfirstlane(fill[rl]);                                        \
    if (n > W.kp) {                                                                                \
      const u64 t = topk_shrink<kTopkLanes>(pool0 + rl * pstride, n, W.k, lane);                   \
      if (lane == 0) {                                                                             \
        fill[rl] = W.k;                                                                            \
        kth[rl] = t;                                                                               \
      }                                                                                            \
    }                                                                                              \
  }

// The end of a top-k sweep (after a barrier): the NaN rows flagged, and each row's list of this candidate range
// (blockIdx.y of ns), sorted and padded, to W.part.
#define GE_TOPK_FINISH \
  if (lane == 0 && nan_rows) {                                                                     \
    for (int j = 0; j < nrows; ++j)                                                                \
      if ((nan_rows >> j) & 1u) W.bad[row0 + j] = 1;                                               \
  }                                                                                                \
  for (int jj = 0; jj < kRows / 4; ++jj) {                                                         \
    const int rl = w * (kRows / 4) + jj;                                                           \
    if (rl >= nrows) break;                                                                        \
    const int n = __builtin_amdgcn_readfirstlane(fill[rl]);                                        \
    topk_emit<kTopkLanes>(pool0 + rl * pstride, n, W.k, lane, nullptr, nullptr,                    \
                          W.part + ((row0 + rl) * ns + blockIdx.y) * W.k);                         \
  }

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

// The prefix's arrays in a workspace.
struct SweepWs {
  float* q; int32_t* rel_of; int32_t* row; void* aux;
};

SweepWs sweep_carve(const SweepPrefix& P, void* ws) {
  char* p = (char*)ws;
  return {(float*)(p + P.q), (int32_t*)(p + P.rel_of), (int32_t*)(p + P.row), p + P.aux};
}

// The rank sweep's grid: 16-row chunks x about two waves of resident workgroups (kMaxBlocks) over the grid, at most
// one per candidate block:  gridDim.y = ceil(2 * kMaxBlocks / n_chunks) clamped to [1, ceil(E / 256)].
dim3 rank_grid(int64_t B, int64_t E) {
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (E + kBlock - 1) / kBlock;
  int64_t gy = (2 * kMaxBlocks + n_chunks - 1) / n_chunks;
  gy = gy < 1 ? 1 : (gy > n_cb ? n_cb : gy);
  return dim3((unsigned)n_chunks, (unsigned)gy);
}

// The row kernel's launch (w: the carved workspace) and, when known lists are given, the filter pass's; S: none, or
// the call's SetArgs.
template <int MODEL, bool L1, class... SETS>
void rank_row_launch(const TransTables& T, const int32_t* tri, int64_t B, int head, const SweepWs& w, const RankOut& o,
                     hipStream_t st, const SETS&... S) {
  hipLaunchKernelGGL((rank_row_kernel<MODEL, L1, SETS...>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, st, T, tri, B, head, w.q, w.rel_of, w.row, o.true_dist, o.n_before, o.n_known_before, S...);
}

template <int MODEL, bool L1, class... SETS>
void rank_filter_launch(const TransTables& T, int64_t B, const SweepWs& w, const RankOut& o, hipStream_t st,
                        const SETS&... S) {
  if (!o.known_off || !o.known_rc) return;
  const int64_t n_tiles = ((B + kTile - 1) / kTile) * ((T.E + kTile - 1) / kTile);
  hipLaunchKernelGGL((rank_filter_kernel<MODEL, L1, SETS...>), dim3(1024), dim3(kBlock), 0, st, T, w.q, w.rel_of, w.row,
                     o.true_dist, B, o.known_off, o.known_rc, n_tiles, o.n_known_before, S...);
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

// A top-k call's workspace carved: the prefix, the kernels' TopkWs (bad = the prefix's row array), the second list
// buffer, and ns = topk_ranges(B, E), the sweep's gridDim.y.
struct TopkCall {
  SweepWs s; TopkWs W; u64* part2; int64_t ns;
};

TopkCall topk_carve(const TransModel& m, int64_t B, int k, void* ws) {
  const TopkLayout L = topk_layout(m, B, k);
  char* p = (char*)ws;
  TopkCall c;
  c.s = sweep_carve(L.P, ws);
  c.W = {k, topk_kp(k), topk_kp(k) + kBlock, (u64*)(p + L.pool), (u64*)(p + L.part), c.s.row};
  c.part2 = (u64*)(p + L.part2);
  c.ns = topk_ranges(B, m.E);
  return c;
}

// The top-k row kernel's launch; S: none, or the call's SetArgs.
template <int MODEL, class... SETS>
void topk_row_launch(const TransTables& T, const int32_t* qr, int64_t B, int head, const TopkCall& c, hipStream_t st,
                     const SETS&... S) {
  hipLaunchKernelGGL((topk_row_kernel<MODEL, SETS...>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, T, qr, B, head, c.s.q, c.s.rel_of, c.W.bad, S...);
}

// The top-k sweep's grid: 16-row chunks x candidate ranges.
dim3 topk_grid(int64_t B, const TopkCall& c) { return dim3((unsigned)((B + kRows - 1) / kRows), (unsigned)c.ns); }

// Merge rounds over the c.ns sorted lists per row that the sweep left in W.part: groups of kMergeFan lists, until one
// group per row is left; that round writes ids / distances.  A round reads one of W.part / part2 and writes the other.
void topk_merge_rounds(const TopkCall& c, int64_t B, int32_t* out_id, float* out_dist, hipStream_t st) {
  u64* lists[2] = {c.W.part, c.part2};
  int cur = 0;
  for (int64_t n = c.ns;;) {
    const int64_t n_out = (n + kMergeFan - 1) / kMergeFan, waves = B * n_out;
    const dim3 mg((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
    const bool last = n_out == 1;
    hipLaunchKernelGGL(topk_merge_kernel, mg, dim3(kBlock), 0, st, lists[cur], (int)n, last ? nullptr : lists[cur ^ 1],
                       B, c.W, last ? out_id : nullptr, last ? out_dist : nullptr);
    if (last) break;
    cur ^= 1;
    n = n_out;
  }
}

}  // namespace
}  // namespace ge
