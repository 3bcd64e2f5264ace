// ge_transx_rank_masked.hip -- per-relation candidate sets on the translation models' entity sweeps (ge_transx_rank_masked,
// ge_transr_rank_masked, ge_transx_topk_masked, ge_transr_topk_masked).  The candidates are the
// entities [0, E), candidate position = entity id.
//   mask     uint32 [n_sets][mw], mw = candidate_mask_words(E): bit c & 31 of word c >> 5 of row s = entity c is
//            admissible in set s; bits at positions >= E are never read
//   row_set  int32 [B]: -1 = the row is unrestricted; any other value outside [0, n_sets) makes the row a bad row (what
//            an id out of range gives)
// Every distance is the unmasked sweep's own (GE_SWEEP_DISTS of ge_transx_rank_kern.h, one arithmetic per row), so a
// masked result is a function of what ge_transx_rank stores in scores_out.
//
// The sweeps compute a distance only for candidates that some row of the workgroup admits: a stream compaction in front
// of the distance loop.  A workgroup owns kRows consecutive rows and the 256-candidate source blocks blockIdx.y,
// blockIdx.y + gridDim.y, ...  Per source block lane c forms the 16-bit word "row j admits c" (top-k: "and c is no known
// cell of row j"); lanes with a non-zero word append (c, word) to a queue in LDS (ballot, mbcnt prefix, one LDS atomic
// per wave).  Whenever the queue holds 256 entries or more the workgroup takes its last 256 as a batch: cc = the lane's
// queue entry, GE_SWEEP_DISTS, and the unmasked epilogue with the lane's row bit ANDed into the before-test (ranks) or
// into take (top-k).  After the last source block one partial batch is flushed; its idle lanes read entity E - 1 with
// row bits 0.  Fewer than 256 entries carry over and a block adds at most 256: the queue holds at most 511.
// Which entries share a batch depends on the order the waves append in; no result does: the counts are sums over the
// admissible candidates, and the top-k pools only ever drop keys that k smaller keys of the same row exclude.
//
// This file holds the queue, the two masked sweep kernels and their launchers.  The row and filter kernels (here with
// the sets), the set test, the sweeps' shared texts (GE_SWEEP_DISTS, GE_RANK_COMMIT, GE_TOPK_*), the merge rounds, the
// workspace carving and the grid rules (rank_grid, topk_ranges: those of the unmasked sweeps; the workspace layouts
// depend on the top-k's) are in ge_transx_rank_kern.h.
#include "ge_transx_rank_kern.h"

namespace ge {
namespace {

constexpr int kQueue = 2 * kBlock;       // queue entries: < 256 carried over + <= 256 of one source block

// The queue and the chunk's sets in LDS.
struct SweepQueue {
  int32_t id[kQueue];
  uint16_t bits[kQueue];
  int32_t set_of[kRows];                 // set index, kSetFree or kSetBad (rows past nrows: kSetBad)
  int n;
};

__device__ __forceinline__ void queue_init(SweepQueue& Q, const SetArgs& S, int64_t row0, int nrows) {
  if (threadIdx.x < kRows) {
    int32_t s = kSetBad;
    if ((int)threadIdx.x < nrows) {
      s = S.row_set[row0 + threadIdx.x];
      if (!set_ok(s, S.n_sets)) s = kSetBad;
    }
    Q.set_of[threadIdx.x] = s;
  }
  if (threadIdx.x == 0) Q.n = 0;
}

// Bit j: row j of the chunk admits entity c (c < E: the caller drops the other lanes, so that no word past a mask row's
// end -- the last source block reaches past word mw - 1 whenever ceil(E / 128) is odd -- is ever read).  Consecutive rows
// of one set share the load; the 32 lanes of a word read one address.
__device__ __forceinline__ unsigned admit_bits(const SweepQueue& Q, const SetArgs& S, int64_t c, int nrows) {
  unsigned bits = 0;
  int32_t prev = kSetBad;
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    if (j < nrows) {
      const int32_t s = Q.set_of[j];
      if (s == kSetFree) {
        bits |= 1u << j;
      } else if (s >= 0) {
        if (s != prev) word = mask_word(S, s, c);
        prev = s;
        bits |= mask_bit(word, c) << j;
      }
    }
  }
  return bits;
}

// Lanes with bits != 0 append (c, bits): one LDS atomic per wave.  (Q.n < kBlock before a source block, so every index
// written is below kQueue.)
__device__ __forceinline__ void queue_append(SweepQueue& Q, int64_t c, unsigned bits, int lane) {
  const u64 m = __ballot(bits != 0);
  if (m) {
    int base = 0;
    if (lane == 0) base = atomicAdd(&Q.n, __popcll(m));
    base = __shfl(base, 0);
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (bits) {
      Q.id[base + below] = (int32_t)c;
      Q.bits[base + below] = (uint16_t)bits;
    }
  }
}

// The masked rank sweep: rank_sweep_kernel's grid, distance loop and count, over the queue's batches.
template <int MODEL, bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void rank_sweep_masked_kernel(TransTables T, const float* __restrict__ q,
                                                                   const int32_t* __restrict__ rel_of,
                                                                   const int32_t* __restrict__ tid,
                                                                   const float* __restrict__ true_dist, int64_t B,
                                                                   int32_t* __restrict__ n_before, SetArgs S) {
  __shared__ int32_t wave_cnt[kBlock / kWave][kRows];
  __shared__ SweepQueue Q;
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
  queue_init(Q, S, row0, nrows);
  const int dE = T.dE, dq = T.dq;
  __syncthreads();
  for (int64_t cb = blockIdx.y;; cb += gridDim.y) {
    const bool more = cb * kBlock < T.E;                 // false: the pass that flushes what the queue still holds
    if (more) {
      const int64_t c = cb * kBlock + threadIdx.x;
      queue_append(Q, c, c < T.E ? admit_bits(Q, S, c, nrows) : 0u, lane);
    }
    __syncthreads();                                     // the block's appends are in
    const int n = Q.n;
    if (n >= kBlock || (!more && n > 0)) {               // (uniform)
      const int take = n < kBlock ? n : kBlock;
      const bool valid = (int)threadIdx.x < take;
      const int64_t c = valid ? Q.id[n - take + threadIdx.x] : T.E - 1;   // an idle lane reads a real row, bits 0
      const unsigned bits = valid ? Q.bits[n - take + threadIdx.x] : 0u;
      const int64_t cc = c;
      __syncthreads();                                   // every lane has read n and its entry
      if (threadIdx.x == 0) Q.n = n - take;
      GE_SWEEP_DISTS
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (j < nrows) {
          const bool before = ((bits >> j) & 1u) && (acc[j] < dt[j] || (acc[j] == dt[j] && c < tt[j]));
          cnt[j] += __popcll(__ballot(before));
        }
      }
    }
    if (!more) break;
    __syncthreads();                                     // Q.n as the batch left it, before the next block appends
  }
  GE_RANK_COMMIT
}

// The masked top-k sweep: topk_sweep_kernel's grid, pools and cut-back, over the queue's batches.  A lane's row bit says
// "admissible and not known": the known bitmap of a source block is applied where the bits are formed, so a batch needs
// none.  A batch adds at most 256 keys to a row's pool -- the bound of the unmasked sweep's source block -- and the
// cut-back to k follows each batch, so a pool never exceeds cap = kp + 256.
template <int MODEL, bool L1, int VEC>
__global__ __launch_bounds__(kBlock) void topk_sweep_masked_kernel(TransTables T, const float* __restrict__ q,
                                                                   const int32_t* __restrict__ rel_of, int64_t B,
                                                                   const int32_t* __restrict__ known_off,
                                                                   const uint16_t* __restrict__ known_rc, TopkWs W,
                                                                   SetArgs S) {
  __shared__ u64 kth[kRows];
  __shared__ int fill[kRows];
  __shared__ uint32_t bm[kRows][kBlock / 32];
  __shared__ SweepQueue Q;
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
  queue_init(Q, S, row0, nrows);
  unsigned nan_rows = 0;                                 // bit j: a NaN distance in row j (wave-uniform)
  const int dE = T.dE, dq = T.dq;
  __syncthreads();
  for (int64_t cb = blockIdx.y;; cb += gridDim.y) {
    const bool more = cb * kBlock < T.E;                 // false: the pass that flushes what the queue still holds
    if (more) {
      const int64_t c = cb * kBlock + threadIdx.x;
      if (known_off) {
        GE_TOPK_KNOWN_BITMAP
      }
      unsigned bits = c < T.E ? admit_bits(Q, S, c, nrows) : 0u;
      if (known_off) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) bits &= ~((unsigned)known_bit(bm, j) << j);
      }
      queue_append(Q, c, bits, lane);
    }
    __syncthreads();                                     // the block's appends are in (and bm has been read)
    const int n = Q.n;
    if (n >= kBlock || (!more && n > 0)) {               // (uniform)
      const int take_n = n < kBlock ? n : kBlock;
      const bool valid = (int)threadIdx.x < take_n;
      const int64_t c = valid ? Q.id[n - take_n + threadIdx.x] : T.E - 1;   // an idle lane reads a real row, bits 0
      const unsigned bits = valid ? Q.bits[n - take_n + threadIdx.x] : 0u;
      const int64_t cc = c;
      __syncthreads();                                   // every lane has read n and its entry
      if (threadIdx.x == 0) Q.n = n - take_n;
      GE_SWEEP_DISTS
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (j < nrows) {
          GE_TOPK_OFFER((bits >> j) & 1u)                // bit j: admissible in row j's set and not known
        }
      }
      __syncthreads();                                   // the batch's appends are in
      GE_TOPK_CUT
    }
    if (!more) break;
    __syncthreads();                                     // Q.n, fill and kth as the batch left them
  }
  __syncthreads();
  GE_TOPK_FINISH
}

template <int MODEL, bool L1>
int run_masked(const TransModel& m, const int32_t* tri, int64_t B, int head, const RankOut& o, const SetArgs& S, void* ws,
               hipStream_t st) {
  const SweepWs w = sweep_carve(sweep_prefix(m, B), ws);
  const TransTables T = trans_prepare<true>(m, w.aux, st);
  rank_row_launch<MODEL, L1>(T, tri, B, head, w, o, st, S);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((rank_sweep_masked_kernel<MODEL, L1, 4>), rank_grid(B, T.E), dim3(kBlock), 0, st, T, w.q,
                       w.rel_of, w.row, o.true_dist, B, o.n_before, S);
  else
    hipLaunchKernelGGL((rank_sweep_masked_kernel<MODEL, L1, 1>), rank_grid(B, T.E), dim3(kBlock), 0, st, T, w.q,
                       w.rel_of, w.row, o.true_dist, B, o.n_before, S);
  rank_filter_launch<MODEL, L1>(T, B, w, o, st, S);
  return launch_status();
}

template <int MODEL, bool L1>
int run_topk_masked(const TransModel& m, const int32_t* qr, int64_t B, int head, const int32_t* known_off,
                    const uint16_t* known_rc, int k, int32_t* out_id, float* out_dist, const SetArgs& S, void* ws,
                    hipStream_t st) {
  const TopkCall c = topk_carve(m, B, k, ws);
  const TransTables T = trans_prepare<true>(m, c.s.aux, st);
  topk_row_launch<MODEL>(T, qr, B, head, c, st, S);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((topk_sweep_masked_kernel<MODEL, L1, 4>), topk_grid(B, c), dim3(kBlock), 0, st, T, c.s.q,
                       c.s.rel_of, B, known_off, known_rc, c.W, S);
  else
    hipLaunchKernelGGL((topk_sweep_masked_kernel<MODEL, L1, 1>), topk_grid(B, c), dim3(kBlock), 0, st, T, c.s.q,
                       c.s.rel_of, B, known_off, known_rc, c.W, S);
  topk_merge_rounds(c, B, out_id, out_dist, st);
  return launch_status();
}

}  // namespace

int trans_rank_masked_launch(const TransModel& m, const int32_t* tri, int64_t B, int cand_is_head, const RankOut& o,
                             const SetArgs& sets, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < sweep_prefix(m, B).end) return GE_ENOMEM;
  const SetArgs S{sets.row_set, sets.mask, sets.n_sets, candidate_mask_words(m.E)};
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run_masked<decltype(model)::value, decltype(l1)::value>(m, tri, B, cand_is_head ? 1 : 0, o, S, workspace, st);
  });
}

int trans_topk_masked_launch(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head,
                             const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id,
                             float* out_dist, const SetArgs& sets, void* workspace, size_t workspace_bytes,
                             hipStream_t st) {
  if (workspace_bytes < topk_ws_bytes(m, B, k)) return GE_ENOMEM;
  const SetArgs S{sets.row_set, sets.mask, sets.n_sets, candidate_mask_words(m.E)};
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run_topk_masked<decltype(model)::value, decltype(l1)::value>(m, queries, B, cand_is_head ? 1 : 0, known_off,
                                                                        known_rc, k, out_id, out_dist, S, workspace, st);
  });
}

}  // namespace ge
