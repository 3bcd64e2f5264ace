// ge_transx_rank.hip -- link-prediction ranks of the translation models (TransE / TransH / TransD / TransR) over
// every entity, counted in the distance sweep: no [B, E] matrix.  For test row i = (h, t, r) the candidates c in
// [0, E) replace the tail (D_c = D(h, c, r)) or the head (D_c = D(c, t, r)); rows are ordered ascending by
// (D, entity id), n_before = #{c : D_c < D_true, or D_c == D_true and c < true}, and n_known_before counts those c
// that the caller lists as known (ge_known_cells' 128 x 128 tile lists, candidate position = entity id).
//
// Every distance is  D = sum_k term(q_k - P_c,k)  over k = 0 .. dq-1 in order, term = |u| or fmaf(u, u, acc):
//   q   the row's query: proj(h) + r on the tail side, proj(t) - r on the head side (one vector per row)
//   P_c the candidate's projection under the row's relation:
//       TransE e_c;  TransH fmaf(-a_c, n^_k, e_c,k) with a_c = e_c . n^ (sequential fmaf dot);
//       TransD fmaf(A_c, r_p,k, e_c,k) with A_c = e_c . e_p,c;  TransR (M_r e_c)_k, a sequential fmaf chain over dim_e.
// The sweep, the true distance and the filter pass all evaluate exactly this sequence with the same operands (every
// multiply-add is an explicit fmaf, so contraction cannot differ between them), so the target never ranks before
// itself and the filter counts exactly the known cells the sweep counted.  A row's arithmetic does not depend on the
// rows that share its call: the sweep only groups rows to reuse a relation's projection scalar.
//
// Launches (stream-ordered, no host synchronisation):
//   prep   (TransH) n^ per relation;  (TransD) A_c per entity
//   row    one thread per row: ids checked, q written to the workspace, D_true, counters set to 0 (-1 for a bad id)
//   sweep  256 candidates per workgroup (one lane each) x kRows consecutive rows; the query values are uniform
//          (scalar loads).  Per row: ballot + popcount of the before-test, summed over the workgroup's four waves in
//          LDS, one integer atomic per row and workgroup.
//   filter one thread per known cell: recompute D with the row's operands, integer atomic when it ranks before.
#include "ge_common.h"
#include "ge_launch.h"

namespace ge {
namespace {

constexpr int kTransE = GE_TRANSX_TRANSE, kTransH = GE_TRANSX_TRANSH, kTransD = GE_TRANSX_TRANSD;
constexpr int kTransR = 3;               // this file's own code for TransR (not an ABI value)
constexpr int kRows = 16;                // rows per sweep workgroup
constexpr int kTile = 128;               // ge_known_cells' tile edge
constexpr float kNormEps = 1e-12f;

// the tables of one call
struct RankTables {
  const float* ent;     // [E, dE]
  const float* rel;     // [R, dq]
  const float* aux;     // TransH: n^ [R, d] (workspace);  TransD: rel_transfer [R, d];  TransR: rel_matrix [R, dq*dE]
  const float* ent2;    // TransD: ent_transfer [E, d]
  const float* A;       // TransD: A_c = e_c . e_p,c [E] (workspace)
  int64_t E, R;
  int dE, dq;           // entity width; width of q and of the distance (d for TransX, dim_r for TransR)
};

__device__ __forceinline__ float dist_acc(bool l1, float acc, float u) { return l1 ? acc + fabsf(u) : fmaf(u, u, acc); }

__device__ __forceinline__ float dot_seq(const float* __restrict__ a, const float* __restrict__ b, int n) {
  float s = 0.f;
  for (int k = 0; k < n; ++k) s = fmaf(a[k], b[k], s);
  return s;
}

// The projection scalar of entity e under relation r: TransH a = e . n^_r, TransD A_e, else 0.
template <int MODEL>
__device__ __forceinline__ float proj_scalar(const RankTables& T, int64_t e, int64_t r) {
  if constexpr (MODEL == kTransH) return dot_seq(T.ent + e * T.dE, T.aux + r * T.dq, T.dq);
  else if constexpr (MODEL == kTransD) return T.A[e];
  else return 0.f;
}

// Component k of entity e's projection under relation r (a: proj_scalar(e, r)).
template <int MODEL>
__device__ __forceinline__ float proj_elem(const RankTables& T, int64_t e, int64_t r, float a, int k) {
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
__device__ __forceinline__ float dist_one(const RankTables& T, const float* __restrict__ q, int64_t c, int64_t r) {
  const float a = proj_scalar<MODEL>(T, c, r);
  float acc = 0.f;
  for (int k = 0; k < T.dq; ++k) acc = dist_acc(L1, acc, q[k] - proj_elem<MODEL>(T, c, r, a, k));
  return acc;
}

// TransH: n^_r = n_r * rsqrt(max(n_r . n_r, 1e-12)), one thread per relation.
__global__ __launch_bounds__(kBlock) void rank_nhat_kernel(const float* __restrict__ normal, int64_t R, int d,
                                                           float* __restrict__ nhat) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* n = normal + r * d;
  const float inv = rsqrtf(fmaxf(dot_seq(n, n, d), kNormEps));
  for (int k = 0; k < d; ++k) nhat[r * d + k] = n[k] * inv;
}

// TransD: A_c = e_c . e_p,c, one thread per entity.
__global__ __launch_bounds__(kBlock) void rank_transfer_dot_kernel(const float* __restrict__ ent,
                                                                   const float* __restrict__ ent2, int64_t E, int d,
                                                                   float* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) A[e] = dot_seq(ent + e * d, ent2 + e * d, d);
}

// One thread per row: q, the sanitised relation and target, D_true, and the counters' initial values.
template <int MODEL, bool L1>
__global__ __launch_bounds__(kBlock) void rank_row_kernel(RankTables T, const int32_t* __restrict__ tri, int64_t B,
                                                          int head, float* __restrict__ q, int32_t* __restrict__ rel_of,
                                                          int32_t* __restrict__ tid, float* __restrict__ true_dist,
                                                          int32_t* __restrict__ n_before, int32_t* __restrict__ n_known) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
  const bool ok = h >= 0 && h < T.E && t >= 0 && t < T.E && r >= 0 && r < T.R;
  if (!ok) h = t = r = 0;
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

// The sweep.  blockIdx.x: rows [x * kRows, +kRows); candidate blocks of 256 strided by gridDim.y.  Consecutive rows of
// one relation form a segment that shares the lane's projection scalar.  VEC: entity components per load (4 needs
// dE % 4 == 0, dq % 4 == 0 and a 16-byte aligned ent).
template <int MODEL, bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void rank_sweep_kernel(RankTables T, const float* __restrict__ q,
                                                            const int32_t* __restrict__ rel_of,
                                                            const int32_t* __restrict__ tid,
                                                            const float* __restrict__ true_dist, int64_t B,
                                                            int32_t* __restrict__ n_before, float* __restrict__ scores) {
  __shared__ int32_t wave_cnt[kBlock / kWave][kRows];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nrows = (int)(B - row0 < kRows ? B - row0 : kRows);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  int32_t tt[kRows], cnt[kRows];
  float dt[kRows];
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const bool in = j < nrows;
    tt[j] = in ? tid[row0 + j] : 0;
    dt[j] = in ? true_dist[row0 + j] : 0.f;
    cnt[j] = 0;
  }
  const int dE = T.dE, dq = T.dq;
  for (int64_t cb = blockIdx.y; cb * kBlock < T.E; cb += gridDim.y) {
    const int64_t c = cb * kBlock + threadIdx.x;
    const bool valid = c < T.E;
    const int64_t cc = valid ? c : T.E - 1;            // a padding lane reads a real row; its result is dropped
    const float* e = T.ent + cc * dE;
    float acc[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) acc[j] = 0.f;
    for (int s = 0; s < nrows;) {                       // segments of equal relation (uniform)
      const int64_t r = rel_of[row0 + s];
      int s1 = s + 1;
      if constexpr (MODEL != kTransE)
        while (s1 < nrows && rel_of[row0 + s1] == r) ++s1;
      else
        s1 = nrows;
      const float a = proj_scalar<MODEL>(T, cc, r);
      for (int k = 0; k < dq; k += VEC) {
        float p[VEC];
        if constexpr (MODEL == kTransR) {
          const float* m = T.aux + r * (int64_t)dq * dE + (int64_t)k * dE;
#pragma unroll
          for (int v = 0; v < VEC; ++v) p[v] = 0.f;
          for (int jj = 0; jj < dE; jj += VEC) {
            float x[VEC];
            load_vec<VEC>(e + jj, x);
#pragma unroll
            for (int v = 0; v < VEC; ++v)
#pragma unroll
              for (int z = 0; z < VEC; ++z) p[v] = fmaf(m[(int64_t)v * dE + jj + z], x[z], p[v]);
          }
        } else {
          load_vec<VEC>(e + k, p);
          if constexpr (MODEL == kTransH) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) p[v] = fmaf(-a, T.aux[r * dq + k + v], p[v]);
          } else if constexpr (MODEL == kTransD) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) p[v] = fmaf(a, T.aux[r * dq + k + v], p[v]);
          }
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
          if (j >= s && j < s1) {
            const float* qj = q + (row0 + j) * dq + k;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[j] = dist_acc(L1, acc[j], qj[v] - p[v]);
          }
        }
      }
      s = s1;
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (j < nrows) {
        const bool before = valid && (acc[j] < dt[j] || (acc[j] == dt[j] && c < tt[j]));
        cnt[j] += __popcll(__ballot(before));
        if (scores && valid) scores[(row0 + j) * T.E + c] = acc[j];
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kRows; ++j) wave_cnt[w][j] = cnt[j];
  }
  __syncthreads();
  if (threadIdx.x < nrows) {
    int32_t tot = 0;
#pragma unroll
    for (int x = 0; x < kBlock / kWave; ++x) tot += wave_cnt[x][threadIdx.x];
    if (tot) atomicAdd(&n_before[row0 + threadIdx.x], tot);
  }
}

// One thread per known cell (grid-stride over known_off[n_tiles] entries; the cell's tile by binary search).
template <int MODEL, bool L1>
__global__ __launch_bounds__(kBlock) void rank_filter_kernel(RankTables T, const float* __restrict__ q,
                                                             const int32_t* __restrict__ rel_of,
                                                             const int32_t* __restrict__ tid,
                                                             const float* __restrict__ true_dist, int64_t B,
                                                             const int32_t* __restrict__ off,
                                                             const uint16_t* __restrict__ rc, int64_t n_tiles,
                                                             int32_t* __restrict__ n_known) {
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
    const float dt = true_dist[row];
    const float D = dist_one<MODEL, L1>(T, q + row * T.dq, col, rel_of[row]);
    if (D < dt || (D == dt && col < tid[row])) atomicAdd(&n_known[row], 1);
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: q [B, dq] | rel_of [B] | tid [B] | n^ [R, d] (TransH) or A [E] (TransD)
size_t ws_bytes(int model, int64_t E, int64_t R, int dq, int64_t B) {
  size_t n = align256(sizeof(float) * (size_t)B * dq) + 2 * align256(sizeof(int32_t) * (size_t)B);
  if (model == kTransH) n += align256(sizeof(float) * (size_t)R * dq);
  if (model == kTransD) n += align256(sizeof(float) * (size_t)E);
  return n;
}

template <int MODEL, bool L1>
int run(RankTables T, const float* normal, const int32_t* tri, int64_t B, int head, const int32_t* known_off,
        const uint16_t* known_rc, int32_t* n_before, int32_t* n_known, float* true_dist, float* scores, void* ws,
        hipStream_t st) {
  char* p = (char*)ws;
  float* q = (float*)p;  p += align256(sizeof(float) * (size_t)B * T.dq);
  int32_t* rel_of = (int32_t*)p;  p += align256(sizeof(int32_t) * (size_t)B);
  int32_t* tid = (int32_t*)p;  p += align256(sizeof(int32_t) * (size_t)B);
  if constexpr (MODEL == kTransH) {
    float* nhat = (float*)p;
    hipLaunchKernelGGL(rank_nhat_kernel, dim3((unsigned)((T.R + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, normal,
                       T.R, T.dq, nhat);
    T.aux = nhat;
  }
  if constexpr (MODEL == kTransD) {
    float* A = (float*)p;
    hipLaunchKernelGGL(rank_transfer_dot_kernel, dim3((unsigned)((T.E + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       T.ent, T.ent2, T.E, T.dE, A);
    T.A = A;
  }
  hipLaunchKernelGGL((rank_row_kernel<MODEL, L1>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, T,
                     tri, B, head, q, rel_of, tid, true_dist, n_before, n_known);
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (T.E + kBlock - 1) / kBlock;
  int64_t gy = (2 * kMaxBlocks + n_chunks - 1) / n_chunks;   // about two waves of resident workgroups
  gy = gy < 1 ? 1 : (gy > n_cb ? n_cb : gy);
  const dim3 grid((unsigned)n_chunks, (unsigned)gy);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 4>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid, true_dist, B,
                       n_before, scores);
  else
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 1>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid, true_dist, B,
                       n_before, scores);
  if (known_off && known_rc) {
    const int64_t n_tiles = ((B + kTile - 1) / kTile) * ((T.E + kTile - 1) / kTile);
    hipLaunchKernelGGL((rank_filter_kernel<MODEL, L1>), dim3(1024), dim3(kBlock), 0, st, T, q, rel_of, tid, true_dist,
                       B, known_off, known_rc, n_tiles, n_known);
  }
  return launch_status();
}

template <int MODEL>
int run_l(int l1, RankTables T, const float* normal, const int32_t* tri, int64_t B, int head, const int32_t* known_off,
          const uint16_t* known_rc, int32_t* n_before, int32_t* n_known, float* true_dist, float* scores, void* ws,
          hipStream_t st) {
  return l1 ? run<MODEL, true>(T, normal, tri, B, head, known_off, known_rc, n_before, n_known, true_dist, scores, ws, st)
            : run<MODEL, false>(T, normal, tri, B, head, known_off, known_rc, n_before, n_known, true_dist, scores, ws, st);
}

}  // namespace

bool rank_vec4(const float* ent, int32_t d_ent, int32_t d_q) {
  return d_ent % 4 == 0 && d_q % 4 == 0 && ((uintptr_t)ent & 15) == 0;
}

size_t transx_rank_ws_bytes(int model, int64_t E, int64_t R, int32_t d, int64_t B) { return ws_bytes(model, E, R, d, B); }

size_t transr_rank_ws_bytes(int64_t E, int64_t R, int32_t dR, int64_t B) { return ws_bytes(kTransR, E, R, dR, B); }

int transx_rank_launch(int model, int l1, const float* ent, int64_t E, const float* rel, int64_t R, const float* normal,
                       const float* ent_transfer, const float* rel_transfer, int32_t d, const int32_t* tri, int64_t B,
                       int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before,
                       int32_t* n_known_before, float* true_dist, float* scores_out, void* workspace,
                       size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < ws_bytes(model, E, R, d, B)) return GE_ENOMEM;
  RankTables T{ent, rel, nullptr, nullptr, nullptr, E, R, d, d};
  const int head = cand_is_head ? 1 : 0;
  switch (model) {
    case kTransE:
      return run_l<kTransE>(l1, T, nullptr, tri, B, head, known_off, known_rc, n_before, n_known_before, true_dist,
                            scores_out, workspace, st);
    case kTransH:
      return run_l<kTransH>(l1, T, normal, tri, B, head, known_off, known_rc, n_before, n_known_before, true_dist,
                            scores_out, workspace, st);
    default:
      T.aux = rel_transfer;
      T.ent2 = ent_transfer;
      return run_l<kTransD>(l1, T, nullptr, tri, B, head, known_off, known_rc, n_before, n_known_before, true_dist,
                            scores_out, workspace, st);
  }
}

int transr_rank_launch(int l1, const float* ent, int64_t E, const float* rel, const float* rel_matrix, int64_t R,
                       int32_t dE, int32_t dR, const int32_t* tri, int64_t B, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_dist,
                       float* scores_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < ws_bytes(kTransR, E, R, dR, B)) return GE_ENOMEM;
  RankTables T{ent, rel, rel_matrix, nullptr, nullptr, E, R, dE, dR};
  return run_l<kTransR>(l1, T, nullptr, tri, B, cand_is_head ? 1 : 0, known_off, known_rc, n_before, n_known_before,
                        true_dist, scores_out, workspace, st);
}

}  // namespace ge
