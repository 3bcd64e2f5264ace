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
// This file holds the two unmasked sweep kernels and their launchers.  The row, filter and merge kernels, the distance
// loop, the workspace layouts, the grid rules, the row / filter launches and the merge rounds are shared with the
// candidate-set sweeps (ge_transx_rank_masked.hip) and live in ge_transx_rank_kern.h.
#include "ge_transx_rank_kern.h"

namespace ge {
namespace {

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
  GE_RANK_COMMIT
}

// The top-k sweep: the rank sweep's grid and distance loop.  Per row of the workgroup a pool of keys in the workspace,
// its fill and its k-th best key in LDS.  A lane appends its candidate when the key beats the row's k-th best and the
// cell is not known (ballot + prefix count, one LDS atomic per wave and row); after each block of 256 candidates the
// pools past kp keys are cut back to k (one wave per row).  Known cells: a bitmap of the block's rows x candidates,
// built from ge_known_cells' lists of the (at most two) 128 x 128 tiles the block covers.  The bitmap, the offer, the
// cut-back and the end are the GE_TOPK_* texts of ge_transx_rank_kern.h, shared with the masked sweep.
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
      GE_TOPK_KNOWN_BITMAP
    }
    GE_SWEEP_DISTS
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (j < nrows) {
        const bool known = known_off && known_bit(bm, j);
        GE_TOPK_OFFER(valid && !known)
      }
    }
    __syncthreads();                                     // the block's appends are in
    GE_TOPK_CUT
    __syncthreads();
  }
  GE_TOPK_FINISH
}

template <int MODEL, bool L1>
int run(const TransModel& m, const int32_t* tri, int64_t B, int head, const RankOut& o, void* ws, hipStream_t st) {
  const SweepWs w = sweep_carve(sweep_prefix(m, B), ws);
  const TransTables T = trans_prepare<true>(m, w.aux, st);
  rank_row_launch<MODEL, L1>(T, tri, B, head, w, o, st);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 4>), rank_grid(B, T.E), dim3(kBlock), 0, st, T, w.q, w.rel_of,
                       w.row, o.true_dist, B, o.n_before, o.scores_out);
  else
    hipLaunchKernelGGL((rank_sweep_kernel<MODEL, L1, 1>), rank_grid(B, T.E), dim3(kBlock), 0, st, T, w.q, w.rel_of,
                       w.row, o.true_dist, B, o.n_before, o.scores_out);
  rank_filter_launch<MODEL, L1>(T, B, w, o, st);
  return launch_status();
}

template <int MODEL, bool L1>
int run_topk(const TransModel& m, const int32_t* qr, int64_t B, int head, const int32_t* known_off,
             const uint16_t* known_rc, int k, int32_t* out_id, float* out_dist, void* ws, hipStream_t st) {
  const TopkCall c = topk_carve(m, B, k, ws);
  const TransTables T = trans_prepare<true>(m, c.s.aux, st);
  topk_row_launch<MODEL>(T, qr, B, head, c, st);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((topk_sweep_kernel<MODEL, L1, 4>), topk_grid(B, c), dim3(kBlock), 0, st, T, c.s.q, c.s.rel_of, B,
                       known_off, known_rc, c.W);
  else
    hipLaunchKernelGGL((topk_sweep_kernel<MODEL, L1, 1>), topk_grid(B, c), dim3(kBlock), 0, st, T, c.s.q, c.s.rel_of, B,
                       known_off, known_rc, c.W);
  topk_merge_rounds(c, B, out_id, out_dist, st);
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
