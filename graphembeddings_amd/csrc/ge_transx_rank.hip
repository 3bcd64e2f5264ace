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
// Top-k (ge_transx_topk / ge_transr_topk): the same prep, a row kernel for (fixed, relation)
// queries, topk_sweep_kernel (the rank sweep's grid and distance loop, GE_SWEEP_DISTS; per row a pool of keys cut back
// to k as the bound tightens) and rounds of topk_merge_kernel over the candidate ranges' sorted lists.
// The device code shared with the candidate-set sweeps (ge_transx_rank_masked.hip) is in ge_transx_rank_kern.h.
#include "ge_transx_rank_kern.h"

namespace ge {
namespace {

// One thread per row: q, the sanitised relation and target, D_true, and the counters' initial values.
template <int MODEL, bool L1>
__global__ __launch_bounds__(kBlock) void rank_row_kernel(TransTables T, const int32_t* __restrict__ tri, int64_t B,
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

// The rank sweep.  blockIdx.x: rows [x * kRows, +kRows); candidate blocks of 256 strided by gridDim.y.
template <int MODEL, bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void rank_sweep_kernel(TransTables T, const float* __restrict__ q,
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
    GE_SWEEP_DISTS
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
__global__ __launch_bounds__(kBlock) void rank_filter_kernel(TransTables T, const float* __restrict__ q,
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

// One thread per query row: q (as rank_row_kernel forms it), the sanitised relation and the row's flag.
template <int MODEL>
__global__ __launch_bounds__(kBlock) void topk_row_kernel(TransTables T, const int32_t* __restrict__ qr, int64_t B,
                                                          int head, float* __restrict__ q, int32_t* __restrict__ rel_of,
                                                          int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t f = qr[2 * i], r = qr[2 * i + 1];
  const bool ok = f >= 0 && f < T.E && r >= 0 && r < T.R;
  if (!ok) f = r = 0;
  float* qi = q + i * T.dq;
  const float a = proj_scalar<MODEL>(T, f, r);
  for (int k = 0; k < T.dq; ++k) {
    const float p = proj_elem<MODEL>(T, f, r, a, k), rk = T.rel[(int64_t)r * T.dq + k];
    qi[k] = head ? p - rk : p + rk;
  }
  rel_of[i] = r;
  bad[i] = ok ? 0 : 1;
}

// The top-k sweep: the rank sweep's grid and distance loop.  Per row of the workgroup a pool of keys in the workspace,
// its fill and its k-th best key in LDS.  A lane appends its candidate when the key beats the row's k-th best and the
// cell is not known (ballot + prefix count, one LDS atomic per wave and row); after each block of 256 candidates the
// pools past kp keys are cut back to k (one wave per row).  Known cells: a bitmap of the block's rows x candidates,
// built from ge_known_cells' lists of the (at most two) 128 x 128 tiles the block covers.
template <int MODEL, bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void topk_sweep_kernel(TransTables T, const float* __restrict__ q,
                                                            const int32_t* __restrict__ rel_of, int64_t B,
                                                            const int32_t* __restrict__ known_off,
                                                            const uint16_t* __restrict__ known_rc, TopkWs W) {
  __shared__ u64 kth[kRows];
  __shared__ int fill[kRows];
  __shared__ uint32_t bm[kRows][kBlock / 32];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nrows = (int)(B - row0 < kRows ? B - row0 : kRows);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int64_t ns = gridDim.y, pstride = ns * W.cap;
  u64* const pool0 = W.pool + (row0 * ns + blockIdx.y) * W.cap;          // row j's pool: pool0 + j * pstride
  const int64_t n_ct = (T.E + kTile - 1) / kTile, rtile = row0 / kTile;
  const int rsub = (int)(row0 % kTile);
  if (threadIdx.x < kRows) {
    kth[threadIdx.x] = kNoKey;
    fill[threadIdx.x] = 0;
  }
  unsigned nan_rows = 0;                                 // bit j: a NaN distance in row j (wave-uniform)
  const int dE = T.dE, dq = T.dq;
  __syncthreads();
  for (int64_t cb = blockIdx.y; cb * kBlock < T.E; cb += gridDim.y) {
    const int64_t c = cb * kBlock + threadIdx.x;
    const bool valid = c < T.E;
    const int64_t cc = valid ? c : T.E - 1;            // a padding lane reads a real row; its result is dropped
    if (known_off) {
      if (threadIdx.x < kRows * kBlock / 32) (&bm[0][0])[threadIdx.x] = 0u;
      __syncthreads();
      for (int h = 0; h < 2 && 2 * cb + h < n_ct; ++h) {
        const int64_t tile = rtile * n_ct + 2 * cb + h;
        const int32_t x1 = known_off[tile + 1];
        for (int32_t x = known_off[tile] + threadIdx.x; x < x1; x += kBlock) {
          const int cell = known_rc[x], rl = (cell >> 7) - rsub, cl = (cell & 127) + kTile * h;
          if (rl >= 0 && rl < kRows) atomicOr(&bm[rl][cl >> 5], 1u << (cl & 31));
        }
      }
      __syncthreads();
    }
    GE_SWEEP_DISTS
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (j < nrows) {
        const bool known = known_off && ((bm[j][threadIdx.x >> 5] >> (threadIdx.x & 31)) & 1u);
        const float D = acc[j];
        if (__ballot(valid && !known && D != D)) nan_rows |= 1u << j;
        const u64 key = topk_key(D, (int32_t)c);
        const bool take = valid && !known && D < __builtin_inff() && key < kth[j];
        const u64 m = __ballot(take);
        if (m) {
          int base = 0;
          if (lane == 0) base = atomicAdd(&fill[j], __popcll(m));
          base = __shfl(base, 0);
          const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (take) pool0[j * pstride + base + below] = key;          // < cap: <= kp before the block, <= 256 in it
        }
      }
    }
    __syncthreads();                                     // the block's appends are in
    for (int jj = 0; jj < kRows / 4; ++jj) {             // wave w cuts rows 4 w ... 4 w + 3
      const int rl = w * (kRows / 4) + jj;
      const int n = __builtin_amdgcn_readfirstlane(fill[rl]);
      if (n > W.kp) {
        const u64 t = topk_shrink<kTopkLanes>(pool0 + rl * pstride, n, W.k, lane);
        if (lane == 0) {
          fill[rl] = W.k;
          kth[rl] = t;
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0 && nan_rows) {
    for (int j = 0; j < nrows; ++j)
      if ((nan_rows >> j) & 1u) W.bad[row0 + j] = 1;
  }
  for (int jj = 0; jj < kRows / 4; ++jj) {               // each row's list of this candidate range, sorted and padded
    const int rl = w * (kRows / 4) + jj;
    if (rl >= nrows) break;
    const int n = __builtin_amdgcn_readfirstlane(fill[rl]);
    topk_emit<kTopkLanes>(pool0 + rl * pstride, n, W.k, lane, nullptr, nullptr,
                          W.part + ((row0 + rl) * ns + blockIdx.y) * W.k);
  }
}

template <int MODEL, bool L1>
int run(const TransModel& m, const int32_t* tri, int64_t B, int head, const RankOut& o, void* ws, hipStream_t st) {
  const SweepPrefix P = sweep_prefix(m, B);
  char* p = (char*)ws;
  float* q = (float*)(p + P.q);
  int32_t* rel_of = (int32_t*)(p + P.rel_of);
  int32_t* tid = (int32_t*)(p + P.row);
  const TransTables T = trans_prepare<true>(m, p + P.aux, st);
  hipLaunchKernelGGL((rank_row_kernel<MODEL, L1>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, T,
                     tri, B, head, q, rel_of, tid, o.true_dist, o.n_before, o.n_known_before);
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (T.E + kBlock - 1) / kBlock;
  int64_t gy = (2 * kMaxBlocks + n_chunks - 1) / n_chunks;   // about two waves of resident workgroups
  gy = gy < 1 ? 1 : (gy > n_cb ? n_cb : gy);
  const dim3 grid((unsigned)n_chunks, (unsigned)gy);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 4>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid, o.true_dist, B,
                       o.n_before, o.scores_out);
  else
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 1>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid, o.true_dist, B,
                       o.n_before, o.scores_out);
  if (o.known_off && o.known_rc) {
    const int64_t n_tiles = ((B + kTile - 1) / kTile) * ((T.E + kTile - 1) / kTile);
    hipLaunchKernelGGL((rank_filter_kernel<MODEL, L1>), dim3(1024), dim3(kBlock), 0, st, T, q, rel_of, tid,
                       o.true_dist, B, o.known_off, o.known_rc, n_tiles, o.n_known_before);
  }
  return launch_status();
}

template <int MODEL, bool L1>
int run_topk(const TransModel& m, const int32_t* qr, int64_t B, int head, const int32_t* known_off,
             const uint16_t* known_rc, int k, int32_t* out_id, float* out_dist, void* ws, hipStream_t st) {
  const TopkLayout L = topk_layout(m, B, k);
  char* p = (char*)ws;
  float* q = (float*)(p + L.P.q);
  int32_t* rel_of = (int32_t*)(p + L.P.rel_of);
  TopkWs W;
  W.k = k;
  W.kp = topk_kp(k);
  W.cap = W.kp + kBlock;
  W.bad = (int32_t*)(p + L.P.row);
  W.pool = (u64*)(p + L.pool);
  W.part = (u64*)(p + L.part);
  u64* part2 = (u64*)(p + L.part2);
  const TransTables T = trans_prepare<true>(m, p + L.P.aux, st);
  hipLaunchKernelGGL((topk_row_kernel<MODEL>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, T, qr,
                     B, head, q, rel_of, W.bad);
  const int64_t n_chunks = (B + kRows - 1) / kRows, ns = topk_ranges(B, T.E);
  const dim3 grid((unsigned)n_chunks, (unsigned)ns);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((topk_sweep_kernel<MODEL, L1, 4>), grid, dim3(kBlock), 0, st, T, q, rel_of, B, known_off,
                       known_rc, W);
  else
    hipLaunchKernelGGL((topk_sweep_kernel<MODEL, L1, 1>), grid, dim3(kBlock), 0, st, T, q, rel_of, B, known_off,
                       known_rc, W);
  // merge rounds: groups of kMergeFan lists, until one group per row is left; that round writes ids / distances
  u64* lists[2] = {W.part, part2};                      // a round reads one and writes the other
  int cur = 0;
  for (int64_t n = ns;;) {
    const int64_t n_out = (n + kMergeFan - 1) / kMergeFan, waves = B * n_out;
    const dim3 mg((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
    const bool last = n_out == 1;
    hipLaunchKernelGGL(topk_merge_kernel, mg, dim3(kBlock), 0, st, lists[cur], (int)n, last ? nullptr : lists[cur ^ 1],
                       B, W, last ? out_id : nullptr, last ? out_dist : nullptr);
    if (last) break;
    cur ^= 1;
    n = n_out;
  }
  return launch_status();
}

}  // namespace

size_t trans_rank_ws_bytes(const TransModel& m, int64_t B) { return sweep_prefix(m, B).end; }

int trans_rank_launch(const TransModel& m, const int32_t* tri, int64_t B, int cand_is_head, const RankOut& o,
                      void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < trans_rank_ws_bytes(m, B)) return GE_ENOMEM;
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run<decltype(model)::value, decltype(l1)::value>(m, tri, B, cand_is_head ? 1 : 0, o, workspace, st);
  });
}

int transx_topk_max_k() { return kTopkMaxK; }

size_t trans_topk_ws_bytes(const TransModel& m, int64_t B, int32_t k) { return topk_ws_bytes(m, B, k); }

int trans_topk_launch(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head,
                      const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist,
                      void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < topk_ws_bytes(m, B, k)) return GE_ENOMEM;
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run_topk<decltype(model)::value, decltype(l1)::value>(m, queries, B, cand_is_head ? 1 : 0, known_off,
                                                                 known_rc, k, out_id, out_dist, workspace, st);
  });
}

}  // namespace ge
