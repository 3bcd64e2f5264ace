// ge_transx_relrank.hip -- relation prediction (h, ?, t) of the translation models (TransE / TransH / TransD / TransR):
// for row i = (h, t, r) every relation c in [0, R) is a candidate with D_c = D(h, t, c); rows are ordered ascending by
// (D, relation id), n_before = #{c : D_c < D_r, or D_c == D_r and c < r}, n_known_before counts those c the caller
// lists as known (ge_known_cells' 128 x 128 tile lists, candidate position = relation id), true_dist = D_r.
//
// The arithmetic.  The row's difference is taken once and the projection applied to it:
//   w = e_h - e_t                                       one rounding per component
//   TransE  u_k = w_k + r_c,k
//   TransH  a = n^_c . w;  u_k = fmaf(-a, n^_c,k, w_k) + r_c,k      n^ = n * rsqrt(max(n . n, 1e-12))
//   TransD  s = e_h . p_h - e_t . p_t (once per row);  u_k = fmaf(s, rp_c,k, w_k) + r_c,k
//   TransR  u_k = (M_c w)_k + r_c,k
//   D = sum_k |u_k| or sum_k u_k^2, k in order; every dot and sum is a sequential fmaf chain in index order.
// Every D is computed once, by the distance kernel, and stored; the counts, the true distance and the filter all read
// the stored values, so the target never ranks before itself and the filter counts exactly the cells the count saw.
//
// Launches per chunk of rows (stream-ordered, no host synchronisation, nothing allocated):
//   row     one thread per row: ids checked, w (and TransD's s) written to the workspace, relation id or -1
//   dist    TransE/H/D: a workgroup takes a tile of rows x relations, every lane a 4 x 4 block of (row, relation) cells;
//           the rows' w and the relation-side rows (rel, n^, rel_transfer) are staged in LDS in panels of k.  The tile
//           is 64 x 64, or 512 rows x 8 relations when that wastes fewer relation slots (R = 18: 24 slots, not 64).
//           TransR: a workgroup takes one relation and 64 rows; the same 4 x 4 blocks over (row, k) form M_c w for 64 k
//           at a time from LDS panels of M_c and w, the dim_e-long chain sequential; the 64 terms of each row go
//           through LDS to one lane per row, which adds them in k order.
//   count   one wave per row: D_r from the stored row, ballot + popcount of the before-test over the row's R values
//   known   one thread per known cell of the chunk's row tiles: the same stored values, an integer atomic per hit
#include "ge_common.h"
#include "ge_launch.h"
#include "ge_trans_dev.h"

namespace ge {
namespace {

constexpr int kPad = 4;                  // floats of padding per LDS panel row
constexpr int64_t kChunkCells = (int64_t)1 << 22;   // stored distances per chunk, about
constexpr int64_t kChunkMin = 1024, kChunkMax = 65536;

// One thread per row of the chunk: w = e_h - e_t, TransD's s, the row's relation (-1: an id out of range; w = 0).
template <int MODEL>
__global__ __launch_bounds__(kBlock) void relrank_row_kernel(const float* __restrict__ ent,
                                                             const float* __restrict__ ent2, int64_t E, int64_t R,
                                                             int dE, const int32_t* __restrict__ tri, int64_t n,
                                                             float* __restrict__ w, float* __restrict__ s,
                                                             int32_t* __restrict__ rel_of) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
  const bool ok = h >= 0 && h < E && t >= 0 && t < E && r >= 0 && r < R;
  float* wi = w + i * dE;
  rel_of[i] = ok ? r : -1;
  if (!ok) {
    for (int k = 0; k < dE; ++k) wi[k] = 0.f;
    if constexpr (MODEL == kTransD) s[i] = 0.f;
    return;
  }
  const float* eh = ent + (int64_t)h * dE;
  const float* et = ent + (int64_t)t * dE;
  for (int k = 0; k < dE; ++k) wi[k] = eh[k] - et[k];
  if constexpr (MODEL == kTransD) s[i] = dot_seq(eh, ent2 + (int64_t)h * dE, dE) - dot_seq(et, ent2 + (int64_t)t * dE, dE);
}

// Rows [row0, row0 + NR) x components [k0, k0 + KP) of a row-major table (leading dimension ld, n_rows rows, d
// components) into an LDS panel [NR][KP + kPad]; cells outside the table are 0.  VEC = 4: ld % 4 == 0, src 16-byte
// aligned (k0 and KP are multiples of 4, so a float4 lies wholly inside or outside).
template <int NR, int KP, int VEC>
__device__ __forceinline__ void stage_panel(float* __restrict__ lds, const float* __restrict__ src, int64_t row0,
                                            int64_t n_rows, int ld, int d, int k0) {
  constexpr int per_row = KP / VEC;
  for (int x = threadIdx.x; x < NR * per_row; x += kBlock) {
    const int rl = x / per_row, kk = (x % per_row) * VEC;
    float v[VEC];
#pragma unroll
    for (int z = 0; z < VEC; ++z) v[z] = 0.f;
    if (row0 + rl < n_rows && k0 + kk < d) load_vec<VEC>(src + (row0 + rl) * ld + k0 + kk, v);
    float* dst = lds + rl * (KP + kPad) + kk;
#pragma unroll
    for (int z = 0; z < VEC; ++z) dst[z] = v[z];
  }
}

__device__ __forceinline__ void lds_load4(const float* __restrict__ p, float (&r)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
}

// TransE / TransH / TransD distances of a tile of rows x relations.  LC lanes along the relations: the tile is
// TR = 1024 / LC rows x 4 LC relations, lane (lr, lc) holds rows lr + i TR / 4 x relations lc + j LC, i, j in 0 .. 3
// (interleaved, so that a wave's LDS reads spread over the banks and its stores of one row are consecutive).
// blockIdx.x: relation tile; blockIdx.y: row tile.  aux: n^ (TransH) or rel_transfer (TransD).  D: [n, R] of the chunk.
template <int MODEL, bool L1, int VEC, int LC>
__global__ __launch_bounds__(kBlock) void relrank_dist_kernel(const float* __restrict__ w, const float* __restrict__ s,
                                                              const int32_t* __restrict__ rel_of, int64_t n,
                                                              const float* __restrict__ rel,
                                                              const float* __restrict__ aux, int64_t R, int d,
                                                              float* __restrict__ D) {
  constexpr int TR = 4 * kBlock / LC, TC = 4 * LC, KP = LC >= 16 ? 32 : 16, LD = KP + kPad;
  constexpr bool kAux = MODEL != kTransE;
  __shared__ __attribute__((aligned(16))) float w_s[TR * LD];
  __shared__ __attribute__((aligned(16))) float r_s[TC * LD];
  __shared__ __attribute__((aligned(16))) float a_s[kAux ? TC * LD : 4];
  const int lr = threadIdx.x / LC, lc = threadIdx.x % LC;
  const int64_t row0 = (int64_t)blockIdx.y * TR, c0 = (int64_t)blockIdx.x * TC;
  float acc[4][4], a[4][4], sv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + lr + i * (TR / 4);
    sv[i] = (MODEL == kTransD && row < n) ? s[row] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = a[i][j] = 0.f;
  }
  // TransH: pass 0 forms a = n^ . w over every k, pass 1 the distance; the others have pass 1 alone
  for (int pass = (MODEL == kTransH ? 0 : 1); pass < 2; ++pass) {
    for (int k0 = 0; k0 < d; k0 += KP) {
      __syncthreads();
      stage_panel<TR, KP, VEC>(w_s, w, row0, n, d, d, k0);
      if (pass == 1) stage_panel<TC, KP, VEC>(r_s, rel, c0, R, d, d, k0);
      if constexpr (kAux) stage_panel<TC, KP, VEC>(a_s, aux, c0, R, d, d, k0);
      __syncthreads();
      const int kn = d - k0 < KP ? d - k0 : KP;
      for (int kk = 0; kk < kn; kk += 4) {
        float wv[4][4], rv[4][4], av[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_load4(w_s + (lr + i * (TR / 4)) * LD + kk, wv[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (pass == 1) lds_load4(r_s + (lc + j * LC) * LD + kk, rv[j]);
          if constexpr (kAux) lds_load4(a_s + (lc + j * LC) * LD + kk, av[j]);
        }
        if (MODEL == kTransH && pass == 0) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) a[i][j] = fmaf(av[j][v], wv[i][v], a[i][j]);
        } else {
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float p = wv[i][v];
                if constexpr (MODEL == kTransH) p = fmaf(-a[i][j], av[j][v], p);
                if constexpr (MODEL == kTransD) p = fmaf(sv[i], av[j][v], p);
                acc[i][j] = dist_acc(L1, acc[i][j], p + rv[j][v]);
              }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + lr + i * (TR / 4);
    if (row >= n) continue;
    const bool bad = rel_of[row] < 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = c0 + lc + j * LC;
      if (c < R) D[row * R + c] = bad ? __builtin_nanf("") : acc[i][j];
    }
  }
}

// TransR distances of relation blockIdx.x to rows [64 blockIdx.y, +64).  Lane (lr, lk) of 16 x 16 holds rows
// lr + 16 i x components lk + 16 j (i, j in 0 .. 3) of the current 64 components k of M_c w.
template <bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void relrank_transr_kernel(const float* __restrict__ w,
                                                                const int32_t* __restrict__ rel_of, int64_t n,
                                                                const float* __restrict__ rel,
                                                                const float* __restrict__ mat, int64_t R, int dE, int dR,
                                                                float* __restrict__ D) {
  constexpr int TR = 64, TK = 64, KP = 32, LD = KP + kPad, LU = TK + 1;
  __shared__ __attribute__((aligned(16))) float w_s[TR * LD];
  __shared__ __attribute__((aligned(16))) float m_s[TK * LD];
  __shared__ float u_s[TR * LU];
  const int lr = threadIdx.x >> 4, lk = threadIdx.x & 15;
  const int64_t c = blockIdx.x, row0 = (int64_t)blockIdx.y * TR;
  const float* M = mat + c * (int64_t)dR * dE;
  const float* rc = rel + c * dR;
  float acc = 0.f;                                       // lanes 0 .. 63: the distance of row row0 + lane
  for (int q0 = 0; q0 < dR; q0 += TK) {
    float p[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) p[i][j] = 0.f;
    for (int j0 = 0; j0 < dE; j0 += KP) {
      __syncthreads();
      stage_panel<TR, KP, VEC>(w_s, w, row0, n, dE, dE, j0);
      stage_panel<TK, KP, VEC>(m_s, M, q0, dR, dE, dE, j0);
      __syncthreads();
      const int jn = dE - j0 < KP ? dE - j0 : KP;
      for (int jj = 0; jj < jn; jj += 4) {
        float wv[4][4], mv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_load4(w_s + (lr + 16 * i) * LD + jj, wv[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_load4(m_s + (lk + 16 * j) * LD + jj, mv[j]);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) p[i][j] = fmaf(mv[j][v], wv[i][v], p[i][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = q0 + lk + 16 * j;
      const float rk = k < dR ? rc[k] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) u_s[(lr + 16 * i) * LU + lk + 16 * j] = p[i][j] + rk;
    }
    __syncthreads();
    if (threadIdx.x < TR) {
      const int kn = dR - q0 < TK ? dR - q0 : TK;
      for (int k = 0; k < kn; ++k) acc = dist_acc(L1, acc, u_s[threadIdx.x * LU + k]);
    }
  }
  const int64_t row = row0 + threadIdx.x;
  if (threadIdx.x < TR && row < n) D[row * R + c] = rel_of[row] < 0 ? __builtin_nanf("") : acc;
}

// One wave per row of the chunk: the counters and the true distance from the row's stored distances.
__global__ __launch_bounds__(kBlock) void relrank_count_kernel(const float* __restrict__ D,
                                                               const int32_t* __restrict__ rel_of, int64_t n, int64_t R,
                                                               int32_t* __restrict__ n_before,
                                                               int32_t* __restrict__ n_known,
                                                               float* __restrict__ true_dist) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int32_t r = rel_of[row];
  if (r < 0) {
    if (lane == 0) {
      n_before[row] = -1;
      n_known[row] = -1;
      true_dist[row] = __builtin_nanf("");
    }
    return;
  }
  const float* Dr = D + row * R;
  const float dt = Dr[r];
  int32_t cnt = 0;
  for (int64_t c0 = 0; c0 < R; c0 += kWave) {
    const int64_t c = c0 + lane;
    const float Dc = c < R ? Dr[c] : 0.f;
    const bool before = c < R && (Dc < dt || (Dc == dt && c < r));
    cnt += __popcll(__ballot(before));
  }
  if (lane == 0) {
    n_before[row] = cnt;
    n_known[row] = 0;
    true_dist[row] = dt;
  }
}

// One thread per known cell of the row tiles [rt0, rt1) (grid-stride; the cell's tile by binary search).  row_base:
// the call's row of the chunk's first row; D, rel_of and n_known are the chunk's.
__global__ __launch_bounds__(kBlock) void relrank_known_kernel(const float* __restrict__ D,
                                                               const int32_t* __restrict__ rel_of, int64_t row_base,
                                                               int64_t n, int64_t R, const int32_t* __restrict__ off,
                                                               const uint16_t* __restrict__ rc, int64_t tile0,
                                                               int64_t tile1, int32_t* __restrict__ n_known) {
  const int64_t n_ct = (R + kTile - 1) / kTile;
  const int64_t x0 = off[tile0], x1 = off[tile1];
  for (int64_t x = x0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < x1; x += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = tile0, hi = tile1;                     // the last tile with off[tile] <= x
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= x) lo = mid; else hi = mid;
    }
    const int cell = rc[x];
    const int64_t row = (lo / n_ct) * kTile + (cell >> 7) - row_base, col = (lo % n_ct) * kTile + (cell & 127);
    if (row < 0 || row >= n || col >= R) continue;
    const int32_t r = rel_of[row];
    if (r < 0) continue;
    const float dt = D[row * R + r], Dc = D[row * R + col];
    if (Dc < dt || (Dc == dt && col < r)) atomicAdd(&n_known[row], 1);
  }
}

// rows per chunk: a power of two (a multiple of the known lists' tile edge), about kChunkCells stored distances
int64_t chunk_rows(int64_t R) {
  int64_t c = kChunkMax;
  while (c > kChunkMin && c * R > kChunkCells) c >>= 1;
  return c;
}

// workspace: w [rows, dE] | s [rows] | rel_of [rows] | D [rows, R] | n^ [R, d] (TransH); rows = min(B, chunk_rows(R))
struct Layout {
  size_t w, s, rel_of, D, nhat, total;
  int64_t rows;
};

Layout layout(const TransModel& m, int64_t B) {
  Layout L;
  L.rows = B < chunk_rows(m.R) ? B : chunk_rows(m.R);
  L.w = 0;
  L.s = L.w + align_up(sizeof(float) * (size_t)L.rows * m.dE, 256);
  L.rel_of = L.s + align_up(sizeof(float) * (size_t)L.rows, 256);
  L.D = L.rel_of + align_up(sizeof(int32_t) * (size_t)L.rows, 256);
  L.nhat = L.D + align_up(sizeof(float) * (size_t)L.rows * (size_t)m.R, 256);
  L.total = L.nhat + trans_aux_bytes(m, false);
  return L;
}

template <int MODEL, bool L1, int VEC>
void launch_dist(const TransTables& T, const float* w, const float* s, const int32_t* rel_of, int64_t n, float* D,
                 hipStream_t st) {
  if constexpr (MODEL == kTransR) {
    const dim3 grid((unsigned)T.R, (unsigned)((n + 63) / 64));
    hipLaunchKernelGGL((relrank_transr_kernel<L1, VEC>), grid, dim3(kBlock), 0, st, w, rel_of, n, T.rel, T.aux, T.R,
                       T.dE, T.dq, D);
  } else {
    // the tile that wastes fewer relation slots; 64 x 64 when they tie
    const int64_t wide = (T.R + 63) / 64 * 64, narrow = (T.R + 7) / 8 * 8;
    if (wide <= narrow) {
      const dim3 grid((unsigned)(wide / 64), (unsigned)((n + 63) / 64));
      hipLaunchKernelGGL((relrank_dist_kernel<MODEL, L1, VEC, 16>), grid, dim3(kBlock), 0, st, w, s, rel_of, n, T.rel,
                         T.aux, T.R, T.dq, D);
    } else {
      const dim3 grid((unsigned)(narrow / 8), (unsigned)((n + 511) / 512));
      hipLaunchKernelGGL((relrank_dist_kernel<MODEL, L1, VEC, 2>), grid, dim3(kBlock), 0, st, w, s, rel_of, n, T.rel,
                         T.aux, T.R, T.dq, D);
    }
  }
}

template <int MODEL, bool L1>
int run(const TransModel& m, const int32_t* tri, int64_t B, const RankOut& o, void* ws, hipStream_t st) {
  const Layout L = layout(m, B);
  char* p = (char*)ws;
  float* w = (float*)(p + L.w);
  float* s = (float*)(p + L.s);
  int32_t* rel_of = (int32_t*)(p + L.rel_of);
  const TransTables T = trans_prepare<false>(m, p + L.nhat, st);
  // float4 staging: every staged table 16-byte aligned with a leading dimension % 4 == 0 (w and n^ lie in the workspace)
  const bool vec4 = T.dE % 4 == 0 && T.dq % 4 == 0 && aligned16({T.rel, T.aux});
  const int64_t n_ct = (T.R + kTile - 1) / kTile;
  for (int64_t r0 = 0; r0 < B; r0 += L.rows) {
    const int64_t n = B - r0 < L.rows ? B - r0 : L.rows;
    float* D = o.scores_out ? o.scores_out + r0 * T.R : (float*)(p + L.D);
    hipLaunchKernelGGL((relrank_row_kernel<MODEL>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       T.ent, T.ent2, T.E, T.R, T.dE, tri + 3 * r0, n, w, s, rel_of);
    if (vec4) launch_dist<MODEL, L1, 4>(T, w, s, rel_of, n, D, st);
    else launch_dist<MODEL, L1, 1>(T, w, s, rel_of, n, D, st);
    hipLaunchKernelGGL(relrank_count_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kBlock), 0, st, D, rel_of, n, T.R,
                       o.n_before + r0, o.n_known_before + r0, o.true_dist + r0);
    if (o.known_off && o.known_rc) {
      // (chunks are multiples of the tile edge: a chunk's row tiles are its own)
      const int64_t rt0 = r0 / kTile, rt1 = (r0 + n + kTile - 1) / kTile;
      hipLaunchKernelGGL(relrank_known_kernel, dim3(512), dim3(kBlock), 0, st, D, rel_of, r0, n, T.R, o.known_off,
                         o.known_rc, rt0 * n_ct, rt1 * n_ct, o.n_known_before + r0);
    }
  }
  return launch_status();
}

}  // namespace

size_t trans_relrank_ws_bytes(const TransModel& m, int64_t B) { return layout(m, B).total; }

int trans_relrank_launch(const TransModel& m, const int32_t* tri, int64_t B, const RankOut& o, void* workspace,
                         size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < layout(m, B).total) return GE_ENOMEM;
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run<decltype(model)::value, decltype(l1)::value>(m, tri, B, o, workspace, st);
  });
}

}  // namespace ge
