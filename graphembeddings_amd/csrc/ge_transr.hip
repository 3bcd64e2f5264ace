// ge_transr.hip -- transR.py on gfx950: batch scoring, one step of tf.train.AdamOptimizer on the margin-hinge
// loss tf.reduce_sum(tf.maximum(pos - neg + margin, 0)), and the multi-step native loop.
//
// Tables, row-major fp32: ent [E,dE], rel [R,dR], rel_matrix [R,dR*dE] (row r read as [dR][dE] is M_r).
// u = M_r (h - t) + r: ONE mat-vec per triple on the difference (equal to M_r h - M_r t in exact arithmetic);
// D = sum_k |u_k| (L1) or sum_k u_k^2.  A pair's negative keeps its relation, so M_r is the same on both sides.
//
// Step layout (all stream-ordered, no host synchronisation):
//   1. prep: relation key of every pair (R for a pair with a bad id or neg_r != pos_r), row maps cleared.
//   2. stable radix sort of (relation key, pair): the pairs of one relation become a segment, in pair order.
//   3. plan (one workgroup): each segment is cut into chunks of at most kChunk pairs, numbered in sorted order;
//      relation r owns chunks [rfirst[r], rfirst[r] + rcount[r]).  A hot relation is spread over many chunks.
//   4. chunk kernel, one workgroup per chunk (relation r, n pairs): X = the 2n columns h - t (pos, neg) in LDS,
//      U = M_r X + r, distances, the mask, G = the 2n columns +g+ / -g- (zero for an inactive pair), then
//        entity rows  V = M_r^T G  -> gent[2i + side]  (slots 4i..4i+3 = pos h (+V), pos t (-V), neg h, neg t),
//        the chunk's partial dM_r = G X^T and drel_r = sum of G's columns -> part[chunk].
//      M_r is read once for the forward pass and once for the backward pass of each chunk.
//   5. stable radix sort of the 4B entity slots by entity (inactive / invalid slots take the sentinel E),
//      then estart/eend = each entity's run of sorted slots.
//   6. Adam: one dense pass over (x, m, v) of all three tables.  A row's gradient is the in-order sum of its
//      entity slots, or of its relation's chunk partials; 0 for an untouched row, which still decays.  The last
//      block sums the hinge terms into the loss in pair order.
// Every sum runs in a fixed order and nothing uses float atomics, so a step is bitwise reproducible.
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

#include "ge_common.h"
#include "ge_launch.h"

namespace ge {

constexpr int kTrMaxDim = 256;
constexpr int kChunk = 16;                 // pairs per chunk: at most 32 columns
constexpr int kPlanBlock = 1024;
constexpr int kAdamMaxBlocks = 4096;       // per table

template <bool L1>
__device__ __forceinline__ float tr_term(float u) { return L1 ? fabsf(u) : u * u; }
// d|u|/du = sign(u) with sign(0) = 0;  d(u^2)/du = 2u
template <bool L1>
__device__ __forceinline__ float tr_grad(float u) { return L1 ? (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f)) : 2.f * u; }

__device__ __forceinline__ bool tr_id_ok(int32_t x, int64_t n) { return x >= 0 && x < n; }

// ------------------------------------------------------------------------------------------- score
// One wave per triple: lane k owns rows k, k+64, ... of M_r.
template <bool L1>
__global__ __launch_bounds__(kBlock) void transr_score_kernel(
    const float* __restrict__ ent, const float* __restrict__ rel, const float* __restrict__ mat, int64_t E, int64_t R,
    int dE, int dR, const int32_t* __restrict__ tri, int64_t B, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t i = wave; i < B; i += nwaves) {
    int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
    const bool ok = tr_id_ok(h, E) && tr_id_ok(t, E) && tr_id_ok(r, R);
    if (!ok) h = t = r = 0;
    const float* eh = ent + (int64_t)h * dE;
    const float* et = ent + (int64_t)t * dE;
    const float* M = mat + (int64_t)r * dR * dE;
    float D = 0.f;
    for (int k = lane; k < dR; k += kWave) {
      const float* Mk = M + (int64_t)k * dE;
      float acc = 0.f;
      for (int j = 0; j < dE; ++j) acc += Mk[j] * (eh[j] - et[j]);
      D += tr_term<L1>(acc + rel[(int64_t)r * dR + k]);
    }
    D = group_sum<kWave>(D);
    if (lane == 0) out[i] = ok ? D : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------- step: prep, plan
__global__ __launch_bounds__(kBlock) void transr_prep_kernel(
    const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int64_t B, int64_t E, int64_t R,
    uint32_t* __restrict__ rkeys, uint32_t* __restrict__ rpairs, float* __restrict__ hinge,
    uint32_t* __restrict__ ekeys, uint32_t* __restrict__ eslots, int32_t* __restrict__ estart,
    int32_t* __restrict__ eend, int32_t* __restrict__ rcount) {
  const int64_t n = max(B, max(E, R));
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
    if (x < B) {
      const int32_t r = pos[3 * x + 2];
      const bool ok = tr_id_ok(pos[3 * x], E) && tr_id_ok(pos[3 * x + 1], E) && tr_id_ok(r, R) &&
                      tr_id_ok(neg[3 * x], E) && tr_id_ok(neg[3 * x + 1], E) && neg[3 * x + 2] == r;
      rkeys[x] = ok ? (uint32_t)r : (uint32_t)R;
      rpairs[x] = (uint32_t)x;
      if (!ok) {                                   // valid pairs get these from their chunk
        hinge[x] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) { ekeys[4 * x + s] = (uint32_t)E; eslots[4 * x + s] = (uint32_t)(4 * x + s); }
      }
    }
    if (x < E) estart[x] = eend[x] = 0;
    if (x < R) rcount[x] = 0;
  }
}

// One workgroup: chunk c of the sorted pairs = (chunk_pos[c], chunk_n[c], chunk_rel[c]), c < *nchunks.
__global__ __launch_bounds__(kPlanBlock) void transr_plan_kernel(
    const uint32_t* __restrict__ skey, int64_t B, int64_t R, int32_t* __restrict__ chunk_pos,
    int32_t* __restrict__ chunk_n, int32_t* __restrict__ chunk_rel, int32_t* __restrict__ nchunks,
    int32_t* __restrict__ rfirst, int32_t* __restrict__ rcount) {
  __shared__ int sc[kPlanBlock];
  __shared__ int base;
  const int tid = threadIdx.x;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int64_t p0 = 0; p0 < B; p0 += kPlanBlock) {
    const int64_t p = p0 + tid;
    int cnt = 0, len = 0;
    uint32_t k = 0;
    if (p < B) {
      k = skey[p];
      if (k < (uint32_t)R && (p == 0 || skey[p - 1] != k)) {     // the head of k's segment
        int64_t lo = p + 1, hi = B;                              // upper bound of k in [p, B)
        while (lo < hi) {
          const int64_t mid = (lo + hi) / 2;
          if (skey[mid] <= k) lo = mid + 1; else hi = mid;
        }
        len = (int)(lo - p);
        cnt = (len + kChunk - 1) / kChunk;
      }
    }
    sc[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < kPlanBlock; o <<= 1) {                   // inclusive scan
      const int v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    const int first = base + sc[tid] - cnt;
    for (int q = 0; q < cnt; ++q) {
      chunk_pos[first + q] = (int)p + q * kChunk;
      chunk_n[first + q] = min(kChunk, len - q * kChunk);
      chunk_rel[first + q] = (int)k;
    }
    if (cnt) { rfirst[k] = first; rcount[k] = cnt; }
    __syncthreads();
    if (tid == kPlanBlock - 1) base += sc[tid];
    __syncthreads();
  }
  if (tid == 0) *nchunks = base;
}

// ------------------------------------------------------------------------------------------- step: chunks
struct ChunkArgs {
  const float* ent; const float* rel; const float* mat;
  int64_t E, R; int dE, dR;
  const int32_t* pos; const int32_t* neg; float margin;
  const uint32_t* spair;                                     // pair ids in relation order
  const int32_t* chunk_pos; const int32_t* chunk_n; const int32_t* chunk_rel; const int32_t* nchunks;
  float* hinge; uint32_t* ekeys; uint32_t* eslots;
  float* gent;                                               // [2B][dE]: row 2i + side = M_r^T G[:, 2q + side]
  float* part; int64_t pstride;                              // [chunk][dR*dE (dM) | dR (drel)]
};

// NC = 2n rounded up to a power of two: the columns the register accumulators carry.
template <bool L1, int VEC, int NC>
__device__ __forceinline__ void chunk_body(const ChunkArgs& a, int c, int n, int p0, int r, float* lds) {
  __shared__ int32_t ids[kChunk][5];                         // pair, h, t, neg h, neg t
  __shared__ float Ds[2 * kChunk];
  __shared__ int act[kChunk];
  const int dE = a.dE, dR = a.dR, tid = threadIdx.x;
  float* Xs = lds;                                           // [NC][dE]
  float* Us = lds + NC * dE;                                 // [NC][dR]: U, then G
  if (tid < kChunk && tid < n) {
    const int32_t i = (int32_t)a.spair[p0 + tid];
    ids[tid][0] = i;
    ids[tid][1] = a.pos[3 * (int64_t)i]; ids[tid][2] = a.pos[3 * (int64_t)i + 1];
    ids[tid][3] = a.neg[3 * (int64_t)i]; ids[tid][4] = a.neg[3 * (int64_t)i + 1];
  }
  __syncthreads();
  for (int idx = tid; idx < NC * dE; idx += kBlock) {
    const int col = idx / dE, j = idx - col * dE, q = col >> 1;
    float x = 0.f;
    if (q < n) {
      const int32_t h = ids[q][1 + 2 * (col & 1)], t = ids[q][2 + 2 * (col & 1)];
      x = a.ent[(int64_t)h * dE + j] - a.ent[(int64_t)t * dE + j];
    }
    Xs[idx] = x;
  }
  __syncthreads();
  const float* M = a.mat + (int64_t)r * dR * dE;
  // forward: U[cc][k] = sum_j M[k][j] X[cc][j] (j ascending) + rel[r][k]
  for (int k = tid; k < dR; k += kBlock) {
    float acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = 0.f;
    const float* Mk = M + (int64_t)k * dE;
    for (int j = 0; j < dE; j += VEC) {
      float m[VEC];
      load_vec<VEC>(Mk + j, m);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) acc[cc] += m[e] * Xs[cc * dE + j + e];
    }
    const float rk = a.rel[(int64_t)r * dR + k];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) Us[cc * dR + k] = acc[cc] + rk;
  }
  __syncthreads();
  const int wave = tid / kWave, lane = tid & (kWave - 1);
  for (int cc = wave; cc < NC; cc += kBlock / kWave) {
    float s = 0.f;
    for (int k = lane; k < dR; k += kWave) s += tr_term<L1>(Us[cc * dR + k]);
    s = group_sum<kWave>(s);
    if (lane == 0) Ds[cc] = s;
  }
  __syncthreads();
  if (tid < kChunk) {
    int on = 0;
    if (tid < n) {
      const int64_t i = ids[tid][0];
      const float z = Ds[2 * tid] - Ds[2 * tid + 1] + a.margin;
      on = z >= 0.f;                                         // MaximumGrad: a tie is active
      a.hinge[i] = on ? z : 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a.ekeys[4 * i + s] = on ? (uint32_t)ids[tid][1 + s] : (uint32_t)a.E;
        a.eslots[4 * i + s] = (uint32_t)(4 * i + s);
      }
    }
    act[tid] = on;
  }
  __syncthreads();
  for (int idx = tid; idx < NC * dR; idx += kBlock) {         // G: +g+ (pos column), -g- (neg column)
    const int cc = idx / dR;
    const float f = tr_grad<L1>(Us[idx]);
    Us[idx] = act[cc >> 1] ? ((cc & 1) ? -f : f) : 0.f;
  }
  __syncthreads();
  // entity rows: V[cc][j] = sum_k M[k][j] G[cc][k] (k ascending)
  for (int j = tid; j < dE; j += kBlock) {
    float acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = 0.f;
    for (int k = 0; k < dR; ++k) {
      const float m = M[(int64_t)k * dE + j];
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) acc[cc] += m * Us[cc * dR + k];
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
      if (cc < 2 * n) a.gent[(2 * (int64_t)ids[cc >> 1][0] + (cc & 1)) * dE + j] = acc[cc];
  }
  // the chunk's partials: dM[k][j] = sum_cc G[cc][k] X[cc][j], drel[k] = sum_cc G[cc][k] (cc ascending)
  float* P = a.part + (int64_t)c * a.pstride;
  const int nm = dR * dE;
  for (int idx = tid; idx < nm; idx += kBlock) {
    const int k = idx / dE, j = idx - k * dE;
    float acc = 0.f;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc += Us[cc * dR + k] * Xs[cc * dE + j];
    P[idx] = acc;
  }
  for (int k = tid; k < dR; k += kBlock) {
    float s = 0.f;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) s += Us[cc * dR + k];
    P[nm + k] = s;
  }
}

template <bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void transr_chunk_kernel(ChunkArgs a) {
  extern __shared__ float lds[];
  const int c = blockIdx.x;
  if (c >= *a.nchunks) return;
  const int n = a.chunk_n[c], p0 = a.chunk_pos[c], r = a.chunk_rel[c];
  const int nc = 2 * n;
  if (nc <= 2) chunk_body<L1, VEC, 2>(a, c, n, p0, r, lds);
  else if (nc <= 4) chunk_body<L1, VEC, 4>(a, c, n, p0, r, lds);
  else if (nc <= 8) chunk_body<L1, VEC, 8>(a, c, n, p0, r, lds);
  else if (nc <= 16) chunk_body<L1, VEC, 16>(a, c, n, p0, r, lds);
  else chunk_body<L1, VEC, 2 * kChunk>(a, c, n, p0, r, lds);
}

// ------------------------------------------------------------------------------------------- step: entity map
__global__ __launch_bounds__(kBlock) void transr_emap_kernel(const uint32_t* __restrict__ skey, int64_t n, int64_t E,
                                                            int32_t* __restrict__ estart, int32_t* __restrict__ eend) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = skey[p];
    if (k >= (uint32_t)E) continue;                          // the sentinel sorts last
    if (p == 0 || skey[p - 1] != k) estart[k] = (int32_t)p;
    if (p + 1 == n || skey[p + 1] != k) eend[k] = (int32_t)(p + 1);
  }
}

// ------------------------------------------------------------------------------------------- step: Adam
struct AdamArgs {
  float* x[3];                                               // ent, rel, rel_matrix
  int64_t rows[3]; int cols[3]; int64_t off[3];              // off = the table's offset in m and v
  int nblk[3];
  float* m; float* v;
  const int32_t* estart; const int32_t* eend; const uint32_t* eslot; const float* gent;
  const int32_t* rfirst; const int32_t* rcount; const float* part; int64_t pstride; int64_t drel_off;
  float lr_t, b1, b2, eps;
  const float* hinge; int64_t B; float* loss;
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void transr_adam_kernel(AdamArgs a) {
  int b = blockIdx.x;
  if (b == (int)gridDim.x - 1) {                             // the loss block: fixed-order sum of the hinge terms
    __shared__ float red[kBlock];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < a.B; i += kBlock) s += a.hinge[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) *a.loss = red[0];
    return;
  }
  int tbl = 0;
  while (tbl < 2 && b >= a.nblk[tbl]) { b -= a.nblk[tbl]; ++tbl; }
  const int cols = a.cols[tbl];
  const int64_t units = a.rows[tbl] * cols / VEC;
  float* X = a.x[tbl];
  float* Mm = a.m + a.off[tbl];
  float* Vv = a.v + a.off[tbl];
  const float c1 = 1.f - a.b1, c2 = 1.f - a.b2;
  const int dE = tbl == 0 ? cols : 0;
  for (int64_t u = (int64_t)b * kBlock + threadIdx.x; u < units; u += (int64_t)a.nblk[tbl] * kBlock) {
    const int64_t e0 = u * VEC, row = e0 / cols;
    const int col = (int)(e0 - row * cols);
    float g[VEC], w[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) g[q] = 0.f;
    if (tbl == 0) {                                          // entity slots, in sorted (= slot) order
      const int32_t s1 = a.eend[row];
      for (int32_t p = a.estart[row]; p < s1; ++p) {
        const uint32_t s = a.eslot[p];
        load_vec<VEC>(a.gent + (int64_t)(s >> 1) * dE + col, w);
#pragma unroll
        for (int q = 0; q < VEC; ++q) g[q] = (s & 1) ? g[q] - w[q] : g[q] + w[q];
      }
    } else {                                                 // the relation's chunk partials, in chunk order
      const int32_t nc = a.rcount[row];
      const float* src = a.part + (tbl == 1 ? a.drel_off : 0) + col;
      for (int32_t q0 = 0; q0 < nc; ++q0) {
        load_vec<VEC>(src + (int64_t)(a.rfirst[row] + q0) * a.pstride, w);
#pragma unroll
        for (int q = 0; q < VEC; ++q) g[q] += w[q];
      }
    }
    float xv[VEC], mv[VEC], vv[VEC];
    load_vec<VEC>(X + e0, xv); load_vec<VEC>(Mm + e0, mv); load_vec<VEC>(Vv + e0, vv);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      mv[q] = a.b1 * mv[q] + c1 * g[q];
      vv[q] = a.b2 * vv[q] + c2 * (g[q] * g[q]);
      xv[q] -= (a.lr_t * mv[q]) / (sqrtf(vv[q]) + a.eps);
    }
    store_vec<VEC>(X + e0, xv); store_vec<VEC>(Mm + e0, mv); store_vec<VEC>(Vv + e0, vv);
  }
}

// ------------------------------------------------------------------------------------------- host side
static inline int64_t max_chunks(int64_t R, int64_t B) { return (B + kChunk - 1) / kChunk + (R < B ? R : B); }

struct TrWs {
  uint32_t *rkeys_in, *rkeys_out, *rpairs_in, *rpairs_out;
  uint32_t *ekeys_in, *ekeys_out, *eslots_in, *eslots_out;
  float *hinge, *gent, *part;
  int32_t *chunk_pos, *chunk_n, *chunk_rel, *nchunks, *estart, *eend, *rfirst, *rcount;
  int32_t *pos, *neg;
  void* sort_tmp; size_t sort_bytes;
  int64_t pstride, nchunk_max;
  size_t total;
};

static int tr_ws_layout(int64_t E, int64_t R, int32_t dE, int32_t dR, int64_t B, void* base, TrWs& w) {
  size_t sb_r = 0, sb_e = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sb_r, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (size_t)B, 0u, sort_key_bits(R));
  if (e != hipSuccess) return (int)e;
  e = rocprim::radix_sort_pairs(nullptr, sb_e, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                (uint32_t*)nullptr, (size_t)(4 * B), 0u, sort_key_bits(E));
  if (e != hipSuccess) return (int)e;
  w.pstride = (int64_t)dR * dE + dR;
  w.nchunk_max = max_chunks(R, B);
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += align_up(bytes, 256); return q; };
  w.rkeys_in = (uint32_t*)take(B * 4); w.rkeys_out = (uint32_t*)take(B * 4);
  w.rpairs_in = (uint32_t*)take(B * 4); w.rpairs_out = (uint32_t*)take(B * 4);
  w.ekeys_in = (uint32_t*)take(16 * B); w.ekeys_out = (uint32_t*)take(16 * B);
  w.eslots_in = (uint32_t*)take(16 * B); w.eslots_out = (uint32_t*)take(16 * B);
  w.hinge = (float*)take(B * 4);
  w.gent = (float*)take((size_t)2 * B * dE * 4);
  w.part = (float*)take((size_t)w.nchunk_max * w.pstride * 4);
  w.chunk_pos = (int32_t*)take(w.nchunk_max * 4); w.chunk_n = (int32_t*)take(w.nchunk_max * 4);
  w.chunk_rel = (int32_t*)take(w.nchunk_max * 4); w.nchunks = (int32_t*)take(4);
  w.estart = (int32_t*)take(E * 4); w.eend = (int32_t*)take(E * 4);
  w.rfirst = (int32_t*)take(R * 4); w.rcount = (int32_t*)take(R * 4);
  w.pos = (int32_t*)take(B * 12); w.neg = (int32_t*)take(B * 12);
  w.sort_bytes = sb_r > sb_e ? sb_r : sb_e;
  if (w.sort_bytes == 0) w.sort_bytes = 4;
  w.sort_tmp = take(w.sort_bytes);
  w.total = off;
  return 0;
}

size_t transr_ws_bytes(int64_t E, int64_t R, int32_t dE, int32_t dR, int64_t B) {
  TrWs w;
  if (tr_ws_layout(E, R, dE, dR, B, nullptr, w) != 0) return 0;
  return w.total;
}

int transr_max_dim() { return kTrMaxDim; }

int transr_score_launch(const TransModel& m, const int32_t* tri, int64_t B, float* out, hipStream_t st) {
  if (B == 0) return 0;
  const int grid = grid_for(B, kBlock / kWave);
  if (m.l1) hipLaunchKernelGGL(transr_score_kernel<true>, dim3(grid), dim3(kBlock), 0, st, m.ent, m.rel, m.rel_matrix, m.E, m.R, m.dE, m.dq, tri, B, out);
  else hipLaunchKernelGGL(transr_score_kernel<false>, dim3(grid), dim3(kBlock), 0, st, m.ent, m.rel, m.rel_matrix, m.E, m.R, m.dE, m.dq, tri, B, out);
  return launch_status();
}

// lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), the powers taken from t in double (not a running fp32 product).
static float adam_lr_t(float lr, float b1, float b2, int64_t t) {
  const double p1 = std::pow((double)b1, (double)t), p2 = std::pow((double)b2, (double)t);
  return (float)((double)lr * std::sqrt(1.0 - p2) / (1.0 - p1));
}

template <bool L1, int VEC>
static int launch_chunks(const ChunkArgs& ca, int64_t grid, size_t lds, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(transr_chunk_kernel<L1, VEC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((transr_chunk_kernel<L1, VEC>), dim3((unsigned)grid), dim3(kBlock), lds, st, ca);
  return launch_status();
}

static int tr_step_core(int l1, float* ent, int64_t E, float* rel, float* mat, int64_t R, int32_t dE, int32_t dR,
                        float* m, float* v, const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr,
                        float b1, float b2, float eps, int64_t t, float* loss, TrWs& w, hipStream_t st) {
  const int64_t nmax = B > E ? (B > R ? B : R) : (E > R ? E : R);
  hipLaunchKernelGGL(transr_prep_kernel, dim3(grid_for(nmax, kBlock)), dim3(kBlock), 0, st, pos, neg, B, E, R,
                     w.rkeys_in, w.rpairs_in, w.hinge, w.ekeys_in, w.eslots_in, w.estart, w.eend, w.rcount);
  int rc = launch_status();
  if (rc) return rc;
  size_t sb = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.rkeys_in, w.rkeys_out, w.rpairs_in, w.rpairs_out,
                                           (size_t)B, 0u, sort_key_bits(R), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(transr_plan_kernel, dim3(1), dim3(kPlanBlock), 0, st, w.rkeys_out, B, R, w.chunk_pos, w.chunk_n,
                     w.chunk_rel, w.nchunks, w.rfirst, w.rcount);
  if ((rc = launch_status())) return rc;
  const bool v4 = dE % 4 == 0 && dR % 4 == 0 && aligned16({ent, rel, mat, m, v, w.gent, w.part});
  ChunkArgs ca{ent, rel, mat, E, R, (int)dE, (int)dR, pos, neg, margin, w.rpairs_out, w.chunk_pos, w.chunk_n,
               w.chunk_rel, w.nchunks, w.hinge, w.ekeys_in, w.eslots_in, w.gent, w.part, w.pstride};
  const size_t lds = (size_t)2 * kChunk * (dE + dR) * sizeof(float);
  if (l1) rc = v4 ? launch_chunks<true, 4>(ca, w.nchunk_max, lds, st) : launch_chunks<true, 1>(ca, w.nchunk_max, lds, st);
  else rc = v4 ? launch_chunks<false, 4>(ca, w.nchunk_max, lds, st) : launch_chunks<false, 1>(ca, w.nchunk_max, lds, st);
  if (rc) return rc;
  sb = w.sort_bytes;
  e = rocprim::radix_sort_pairs(w.sort_tmp, sb, w.ekeys_in, w.ekeys_out, w.eslots_in, w.eslots_out, (size_t)(4 * B),
                                0u, sort_key_bits(E), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(transr_emap_kernel, dim3(grid_for(4 * B, kBlock)), dim3(kBlock), 0, st, w.ekeys_out, 4 * B, E,
                     w.estart, w.eend);
  if ((rc = launch_status())) return rc;
  const int vec = v4 ? 4 : 1;
  AdamArgs aa{};
  aa.x[0] = ent; aa.x[1] = rel; aa.x[2] = mat;
  aa.rows[0] = E; aa.rows[1] = R; aa.rows[2] = R;
  aa.cols[0] = dE; aa.cols[1] = dR; aa.cols[2] = dR * dE;
  aa.off[0] = 0; aa.off[1] = E * dE; aa.off[2] = E * dE + R * dR;
  int grid = 1;                                              // + the loss block
  for (int q = 0; q < 3; ++q) {
    const int64_t units = aa.rows[q] * aa.cols[q] / vec;
    int64_t nb = (units + kBlock - 1) / kBlock;
    aa.nblk[q] = (int)(nb < 1 ? 1 : nb > kAdamMaxBlocks ? kAdamMaxBlocks : nb);
    grid += aa.nblk[q];
  }
  aa.m = m; aa.v = v;
  aa.estart = w.estart; aa.eend = w.eend; aa.eslot = w.eslots_out; aa.gent = w.gent;
  aa.rfirst = w.rfirst; aa.rcount = w.rcount; aa.part = w.part; aa.pstride = w.pstride; aa.drel_off = (int64_t)dR * dE;
  aa.lr_t = adam_lr_t(lr, b1, b2, t); aa.b1 = b1; aa.b2 = b2; aa.eps = eps;
  aa.hinge = w.hinge; aa.B = B; aa.loss = loss;
  if (v4) hipLaunchKernelGGL(transr_adam_kernel<4>, dim3(grid), dim3(kBlock), 0, st, aa);
  else hipLaunchKernelGGL(transr_adam_kernel<1>, dim3(grid), dim3(kBlock), 0, st, aa);
  return launch_status();
}

int transr_adam_step_run(int l1, float* ent, int64_t E, float* rel, float* rel_matrix, int64_t R, int32_t dE,
                         int32_t dR, float* m, float* v, const int32_t* pos, const int32_t* neg, int64_t B,
                         float margin, float lr, float b1, float b2, float eps, int64_t t, float* loss,
                         void* workspace, size_t workspace_bytes, hipStream_t st) {
  TrWs w;
  int rc = tr_ws_layout(E, R, dE, dR, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  return tr_step_core(l1, ent, E, rel, rel_matrix, R, dE, dR, m, v, pos, neg, B, margin, lr, b1, b2, eps, t, loss, w,
                      st);
}

int transr_train_steps_run(int l1, float* ent, int64_t E, float* rel, float* rel_matrix, int64_t R, int32_t dE,
                           int32_t dR, float* m, float* v, const SamplerArgs& sa, uint64_t seed, uint64_t first_step,
                           int64_t n_steps, int64_t B, float margin, float lr, float b1, float b2, float eps,
                           int64_t first_t, float* losses, void* workspace, size_t workspace_bytes, hipStream_t st) {
  TrWs w;
  int rc = tr_ws_layout(E, R, dE, dR, B, workspace, w);
  if (rc) return rc;
  if (workspace_bytes < w.total) return GE_ENOMEM;
  return draw_then_step(sa, B, seed, first_step, n_steps, w.pos, w.neg, st, [&](int64_t s) {
    return tr_step_core(l1, ent, E, rel, rel_matrix, R, dE, dR, m, v, w.pos, w.neg, B, margin, lr, b1, b2, eps,
                        first_t + s, losses + s, w, st);
  });
}

}  // namespace ge
