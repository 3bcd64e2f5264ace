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
// Grid rule (unchanged from the unmasked sweeps; the workspace layouts depend on the top-k's):
//   ranks  gridDim.y = ceil(2 * kMaxBlocks / n_chunks) clamped to [1, ceil(E / 256)], n_chunks = ceil(B / kRows)
//   top-k  gridDim.y = topk_ranges(B, E) = ceil(kMaxBlocks / n_chunks) clamped the same way: a function of (B, E) alone
#include "ge_transx_rank_kern.h"

namespace ge {
namespace {

constexpr int kQueue = 2 * kBlock;       // queue entries: < 256 carried over + <= 256 of one source block
constexpr int kSetFree = -1;             // a row's set in LDS: unrestricted
constexpr int kSetBad = -2;              //                     index out of range: the row admits nothing

struct SetArgs {
  const int32_t* row_set;                // [B]
  const uint32_t* mask;                  // [n_sets][mw]
  int32_t n_sets;
  int64_t mw;                            // words per mask row
};

__device__ __forceinline__ bool set_ok(int32_t s, int32_t n_sets) { return s >= -1 && s < n_sets; }

// rank_row_kernel of ge_transx_rank.hip with the set index checked: a bad index is a bad row (NaN, counters -1).
template <int MODEL, bool L1>
__global__ __launch_bounds__(kBlock) void rank_row_masked_kernel(TransTables T, const int32_t* __restrict__ tri,
                                                                 int64_t B, int head, const int32_t* __restrict__ row_set,
                                                                 int32_t n_sets, float* __restrict__ q,
                                                                 int32_t* __restrict__ rel_of, int32_t* __restrict__ tid,
                                                                 float* __restrict__ true_dist,
                                                                 int32_t* __restrict__ n_before,
                                                                 int32_t* __restrict__ n_known) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int32_t h = tri[3 * i], t = tri[3 * i + 1], r = tri[3 * i + 2];
  const bool ids_ok = h >= 0 && h < T.E && t >= 0 && t < T.E && r >= 0 && r < T.R;
  if (!ids_ok) h = t = r = 0;
  const bool ok = ids_ok && set_ok(row_set[i], n_sets);
  const int32_t fixed = head ? t : h, target = head ? h : t;
  float* qi = q + i * T.dq;
  const float a = proj_scalar<MODEL>(T, fixed, r);
  for (int k = 0; k < T.dq; ++k) {
    const float p = proj_elem<MODEL>(T, fixed, r, a, k), rk = T.rel[(int64_t)r * T.dq + k];
    qi[k] = head ? p - rk : p + rk;
  }
  rel_of[i] = r;
  tid[i] = target;
  true_dist[i] = ok ? dist_one<MODEL, L1>(T, qi, target, r) : __builtin_nanf("");   // NaN: the sweep never counts
  n_before[i] = ok ? 0 : -1;
  n_known[i] = ok ? 0 : -1;
}

// topk_row_kernel of ge_transx_rank.hip with the set index checked: a bad index flags the row.
template <int MODEL>
__global__ __launch_bounds__(kBlock) void topk_row_masked_kernel(TransTables T, const int32_t* __restrict__ qr, int64_t B,
                                                                 int head, const int32_t* __restrict__ row_set,
                                                                 int32_t n_sets, float* __restrict__ q,
                                                                 int32_t* __restrict__ rel_of, int32_t* __restrict__ bad) {
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
  bad[i] = ok && set_ok(row_set[i], n_sets) ? 0 : 1;
}

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
        if (s != prev) word = S.mask[(int64_t)s * S.mw + (c >> 5)];
        prev = s;
        bits |= ((word >> (c & 31)) & 1u) << j;
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

// rank_filter_kernel of ge_transx_rank.hip; a cell whose column the row's set does not admit is skipped.
template <int MODEL, bool L1>
__global__ __launch_bounds__(kBlock) void rank_filter_masked_kernel(TransTables T, const float* __restrict__ q,
                                                                    const int32_t* __restrict__ rel_of,
                                                                    const int32_t* __restrict__ tid,
                                                                    const float* __restrict__ true_dist, int64_t B,
                                                                    const int32_t* __restrict__ off,
                                                                    const uint16_t* __restrict__ rc, int64_t n_tiles,
                                                                    int32_t* __restrict__ n_known, SetArgs S) {
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
    const int32_t s = S.row_set[row];
    if (!set_ok(s, S.n_sets)) continue;                 // a bad row: its counters stay -1
    if (s >= 0 && !((S.mask[(int64_t)s * S.mw + (col >> 5)] >> (col & 31)) & 1u)) continue;
    const float dt = true_dist[row];
    const float D = dist_one<MODEL, L1>(T, q + row * T.dq, col, rel_of[row]);
    if (D < dt || (D == dt && col < tid[row])) atomicAdd(&n_known[row], 1);
  }
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
      unsigned bits = c < T.E ? admit_bits(Q, S, c, nrows) : 0u;
      if (known_off) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) bits &= ~(((bm[j][threadIdx.x >> 5] >> (threadIdx.x & 31)) & 1u) << j);
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
          const bool on = (bits >> j) & 1u;              // admissible in row j's set and not known
          const float D = acc[j];
          if (__ballot(on && D != D)) nan_rows |= 1u << j;
          const u64 key = topk_key(D, (int32_t)c);
          const bool take = on && D < __builtin_inff() && key < kth[j];
          const u64 m = __ballot(take);
          if (m) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&fill[j], __popcll(m));
            base = __shfl(base, 0);
            const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (take) pool0[j * pstride + base + below] = key;        // < cap: <= kp before the batch, <= 256 in it
          }
        }
      }
      __syncthreads();                                   // the batch's appends are in
      for (int jj = 0; jj < kRows / 4; ++jj) {           // wave w cuts rows 4 w ... 4 w + 3
        const int rl = w * (kRows / 4) + jj;
        const int nf = __builtin_amdgcn_readfirstlane(fill[rl]);
        if (nf > W.kp) {
          const u64 t = topk_shrink<kTopkLanes>(pool0 + rl * pstride, nf, W.k, lane);
          if (lane == 0) {
            fill[rl] = W.k;
            kth[rl] = t;
          }
        }
      }
    }
    if (!more) break;
    __syncthreads();                                     // Q.n, fill and kth as the batch left them
  }
  __syncthreads();
  if (lane == 0 && nan_rows) {
    for (int j = 0; j < nrows; ++j)
      if ((nan_rows >> j) & 1u) W.bad[row0 + j] = 1;
  }
  for (int jj = 0; jj < kRows / 4; ++jj) {               // each row's list of this candidate range, sorted and padded
    const int rl = w * (kRows / 4) + jj;
    if (rl >= nrows) break;
    const int nf = __builtin_amdgcn_readfirstlane(fill[rl]);
    topk_emit<kTopkLanes>(pool0 + rl * pstride, nf, W.k, lane, nullptr, nullptr,
                          W.part + ((row0 + rl) * ns + blockIdx.y) * W.k);
  }
}

template <int MODEL, bool L1>
int run_masked(const TransModel& m, const int32_t* tri, int64_t B, int head, const RankOut& o, const SetArgs& S, void* ws,
               hipStream_t st) {
  const SweepPrefix P = sweep_prefix(m, B);
  char* p = (char*)ws;
  float* q = (float*)(p + P.q);
  int32_t* rel_of = (int32_t*)(p + P.rel_of);
  int32_t* tid = (int32_t*)(p + P.row);
  const TransTables T = trans_prepare<true>(m, p + P.aux, st);
  hipLaunchKernelGGL((rank_row_masked_kernel<MODEL, L1>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, T, tri, B, head, S.row_set, S.n_sets, q, rel_of, tid, o.true_dist, o.n_before, o.n_known_before);
  const int64_t n_chunks = (B + kRows - 1) / kRows, n_cb = (T.E + kBlock - 1) / kBlock;
  int64_t gy = (2 * kMaxBlocks + n_chunks - 1) / n_chunks;   // the unmasked sweep's rule: about two waves of workgroups
  gy = gy < 1 ? 1 : (gy > n_cb ? n_cb : gy);
  const dim3 grid((unsigned)n_chunks, (unsigned)gy);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((rank_sweep_masked_kernel<MODEL, L1, 4>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid,
                       o.true_dist, B, o.n_before, S);
  else
    hipLaunchKernelGGL((rank_sweep_masked_kernel<MODEL, L1, 1>), grid, dim3(kBlock), 0, st, T, q, rel_of, tid,
                       o.true_dist, B, o.n_before, S);
  if (o.known_off && o.known_rc) {
    const int64_t n_tiles = ((B + kTile - 1) / kTile) * ((T.E + kTile - 1) / kTile);
    hipLaunchKernelGGL((rank_filter_masked_kernel<MODEL, L1>), dim3(1024), dim3(kBlock), 0, st, T, q, rel_of, tid,
                       o.true_dist, B, o.known_off, o.known_rc, n_tiles, o.n_known_before, S);
  }
  return launch_status();
}

template <int MODEL, bool L1>
int run_topk_masked(const TransModel& m, const int32_t* qr, int64_t B, int head, const int32_t* known_off,
                    const uint16_t* known_rc, int k, int32_t* out_id, float* out_dist, const SetArgs& S, void* ws,
                    hipStream_t st) {
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
  hipLaunchKernelGGL((topk_row_masked_kernel<MODEL>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, T,
                     qr, B, head, S.row_set, S.n_sets, q, rel_of, W.bad);
  const int64_t n_chunks = (B + kRows - 1) / kRows, ns = topk_ranges(B, T.E);
  const dim3 grid((unsigned)n_chunks, (unsigned)ns);
  if (rank_vec4(T.ent, T.dE, T.dq))
    hipLaunchKernelGGL((topk_sweep_masked_kernel<MODEL, L1, 4>), grid, dim3(kBlock), 0, st, T, q, rel_of, B, known_off,
                       known_rc, W, S);
  else
    hipLaunchKernelGGL((topk_sweep_masked_kernel<MODEL, L1, 1>), grid, dim3(kBlock), 0, st, T, q, rel_of, B, known_off,
                       known_rc, W, S);
  // merge rounds, as the unmasked top-k runs them
  u64* lists[2] = {W.part, part2};
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

int trans_rank_masked_launch(const TransModel& m, const int32_t* tri, int64_t B, int cand_is_head, const RankOut& o,
                             const int32_t* row_set, const uint32_t* mask, int32_t n_sets, void* workspace,
                             size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < sweep_prefix(m, B).end) return GE_ENOMEM;
  const SetArgs S{row_set, mask, n_sets, candidate_mask_words(m.E)};
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run_masked<decltype(model)::value, decltype(l1)::value>(m, tri, B, cand_is_head ? 1 : 0, o, S, workspace, st);
  });
}

int trans_topk_masked_launch(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head,
                             const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id,
                             float* out_dist, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                             void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (workspace_bytes < topk_ws_bytes(m, B, k)) return GE_ENOMEM;
  const SetArgs S{row_set, mask, n_sets, candidate_mask_words(m.E)};
  return dispatch_trans(m, [&](auto model, auto l1) {
    return run_topk_masked<decltype(model)::value, decltype(l1)::value>(m, queries, B, cand_is_head ? 1 : 0, known_off,
                                                                        known_rc, k, out_id, out_dist, S, workspace, st);
  });
}

}  // namespace ge
