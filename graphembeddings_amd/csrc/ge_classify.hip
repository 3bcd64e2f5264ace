// ge_classify.hip -- triple classification: per-segment decision thresholds fitted from labelled scores, and the decision.
// A segment is one relation.  Every model scores "lower is more plausible", so the rule is  score <= thr[segment].
//
// Fit.  The input is ordered by (segment, score ascending, NaN last).  With  G(i) = #positives - #negatives  among the
// elements [0, i] of the WHOLE input (elements of a segment outside [0, n_seg) count as nothing), the cut after element
// i of a segment that starts at a has  correct = n_neg + G(i) - G(a - 1):  the best cut of a segment is the first
// admissible i with the largest G(i), and it beats "accept nothing" iff G(i) > G(a - 1).  So one plain prefix count over
// the input serves every segment, however long, and no workgroup ever walks a segment:
//   count    one workgroup per tile of kFitTile elements: its positives and negatives
//   scan     exclusive prefix sum over the tiles (one workgroup; 2^20 tiles at the largest M)
//   cuts     one workgroup per tile: the prefix counts of its elements; the first element of a segment stores the
//            segment's start and base counts, the last one its end counts, and every admissible cut goes into the
//            segment's 64-bit key (G biased | ~index) by an integer atomicMax -- one per wave where a wave holds one
//            segment, so the relation that owns most of the input costs M / 512 atomics, not M
//   finish   one thread per segment: decode the key, copy thr_lo / thr_hi from the scores, the counts
// All counting is in int32 (M < 2^31); no float is added or compared across workgroups, and the maximum of a set of
// integers does not depend on the order it is taken in: the result is the same for every grid and every run.
// Unsorted input gives other numbers, never another address: every index read comes from an element that wrote it.
#include "ge_common.h"
#include "ge_launch.h"

#include <math.h>

namespace ge {
namespace {

constexpr int kPerThread = 8;
constexpr int kFitTile = kBlock * kPerThread;           // 2048 elements a workgroup (tests read it as classify.FIT_TILE)
static_assert(kFitTile == GE_THRESHOLD_FIT_TILE, "include/ge_hip.h states the tile");

// the per-segment and per-tile arrays of the workspace, each 256-byte aligned
struct FitWs {
  unsigned long long* key;   // [n_seg] best admissible cut: (G + 2^31) << 32 | ~index; 0 = none
  int32_t* start1;           // [n_seg] index of the segment's first element + 1; 0 = empty
  int32_t* base_pos;         // [n_seg] positives / negatives before the segment's first element
  int32_t* base_neg;
  int32_t* end_pos;          // [n_seg] positives / negatives up to the segment's last element
  int32_t* end_neg;
  int32_t* tile_pos;         // [n_tiles] positives / negatives of a tile, then of all tiles before it
  int32_t* tile_neg;
  size_t seg_bytes, total;
};

inline int64_t fit_tiles(int64_t M) { return (M + kFitTile - 1) / kFitTile; }

inline FitWs fit_layout(void* base, int64_t M, int32_t n_seg) {
  FitWs w;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p + off; off += align_up(bytes, 256); return q; };
  w.key = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)n_seg);
  w.start1 = (int32_t*)take(4 * (size_t)n_seg);
  w.base_pos = (int32_t*)take(4 * (size_t)n_seg);
  w.base_neg = (int32_t*)take(4 * (size_t)n_seg);
  w.end_pos = (int32_t*)take(4 * (size_t)n_seg);
  w.end_neg = (int32_t*)take(4 * (size_t)n_seg);
  w.seg_bytes = off;
  w.tile_pos = (int32_t*)take(4 * (size_t)fit_tiles(M));
  w.tile_neg = (int32_t*)take(4 * (size_t)fit_tiles(M));
  w.total = off;
  return w;
}

__device__ __forceinline__ unsigned long long pack_cut(int32_t g, int64_t i) {
  return ((unsigned long long)((uint32_t)g + 0x80000000u) << 32) | (uint32_t)~(uint32_t)i;
}

__device__ __forceinline__ int32_t wave_incl_scan(int32_t v, int lane) {
#pragma unroll
  for (int s = 1; s < kWave; s <<= 1) {
    const int32_t up = __shfl_up(v, s, kWave);
    if (lane >= s) v += up;
  }
  return v;
}

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// tile_pos[b] / tile_neg[b] = the labelled elements of tile b whose segment is in range
__global__ __launch_bounds__(kBlock) void fit_count_kernel(const int32_t* __restrict__ seg, const uint8_t* __restrict__ label,
                                                           int64_t M, int32_t n_seg, int32_t* __restrict__ tile_pos,
                                                           int32_t* __restrict__ tile_neg) {
  __shared__ int32_t wp[kBlock / kWave], wn[kBlock / kWave];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kFitTile + (int64_t)t * kPerThread;
  int32_t cp = 0, cn = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t i = i0 + j;
    if (i < M) {
      const int32_t s = seg[i];
      if (s >= 0 && s < n_seg) { const int l = label[i] != 0; cp += l; cn += 1 - l; }
    }
  }
  cp = wave_sum(cp);
  cn = wave_sum(cn);
  if ((t & 63) == 0) { wp[t >> 6] = cp; wn[t >> 6] = cn; }
  __syncthreads();
  if (t == 0) {
    int32_t a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) { a += wp[k]; b += wn[k]; }
    tile_pos[blockIdx.x] = a;
    tile_neg[blockIdx.x] = b;
  }
}

// in place: a[b] <- sum of a[0 .. b - 1], for both arrays; one workgroup, 4096 counters a round (ge_known.hip's scan)
__global__ __launch_bounds__(1024) void fit_scan_kernel(int32_t* __restrict__ a0, int32_t* __restrict__ a1, int64_t n) {
  __shared__ int32_t wave_tot[2][16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int32_t carry[2] = {0, 0};
  for (int64_t base = 0; base < n; base += 4096) {
    const int64_t i0 = base + 4 * t;
    int32_t v[2][4], mine[2], incl[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int32_t* a = c ? a1 : a0;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = i0 + j < n ? a[i0 + j] : 0;
      mine[c] = v[c][0] + v[c][1] + v[c][2] + v[c][3];
      incl[c] = wave_incl_scan(mine[c], lane);
      if (lane == 63) wave_tot[c][w] = incl[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int32_t* a = c ? a1 : a0;
      int32_t before = carry[c], all = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) { const int32_t x = wave_tot[c][k]; if (k < w) before += x; all += x; }
      int32_t run = before + incl[c] - mine[c];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) { a[i0 + j] = run; run += v[c][j]; }
      carry[c] += all;
    }
    __syncthreads();
  }
}

// One workgroup per tile, kPerThread consecutive elements a thread.  tile_pos / tile_neg: the counts before the tile.
__global__ __launch_bounds__(kBlock) void fit_cuts_kernel(const float* __restrict__ score, const int32_t* __restrict__ seg,
                                                          const uint8_t* __restrict__ label, int64_t M, int32_t n_seg,
                                                          const int32_t* __restrict__ tile_pos,
                                                          const int32_t* __restrict__ tile_neg,
                                                          unsigned long long* __restrict__ key, int32_t* __restrict__ start1,
                                                          int32_t* __restrict__ base_pos, int32_t* __restrict__ base_neg,
                                                          int32_t* __restrict__ end_pos, int32_t* __restrict__ end_neg) {
  __shared__ int32_t wp[kBlock / kWave], wn[kBlock / kWave];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kFitTile + (int64_t)t * kPerThread;
  // element j of this thread, j = -1 (the one before) ... kPerThread (the one after); a segment of -1 is no segment
  int32_t sg[kPerThread + 2];
  float sc[kPerThread + 1];
  int lb[kPerThread];
  sg[0] = (i0 > 0 && i0 - 1 < M) ? seg[i0 - 1] : -1;
#pragma unroll
  for (int j = 0; j <= kPerThread; ++j) {
    const int64_t i = i0 + j;
    const bool in = i < M;
    int32_t s = in ? seg[i] : -1;
    if (s < 0 || s >= n_seg) s = -1;
    sg[j + 1] = s;
    sc[j] = in ? score[i] : 0.f;
    if (j < kPerThread) lb[j] = (in && s >= 0) ? (label[i] != 0) : 0;
  }
  if (sg[0] < 0 || sg[0] >= n_seg) sg[0] = -1;

  int32_t cp = 0, cn = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (sg[j + 1] >= 0) { cp += lb[j]; cn += 1 - lb[j]; }
  const int32_t ip = wave_incl_scan(cp, lane), in_ = wave_incl_scan(cn, lane);
  if (lane == 63) { wp[w] = ip; wn[w] = in_; }
  __syncthreads();
  int32_t P = tile_pos[blockIdx.x] + ip - cp, N = tile_neg[blockIdx.x] + in_ - cn;
#pragma unroll
  for (int k = 0; k < kBlock / kWave; ++k)
    if (k < w) { P += wp[k]; N += wn[k]; }

  // the running best cut of the segment this thread is in; flushed when the segment changes
  int32_t run_seg = -1;
  unsigned long long run_key = 0;
  bool one_seg = true;                                  // all kPerThread elements in range and of one segment
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int32_t s = sg[j + 1];
    if (s < 0) { one_seg = false; continue; }
    const int64_t i = i0 + j;
    if (sg[j] != s) { start1[s] = (int32_t)(i + 1); base_pos[s] = P; base_neg[s] = N; }
    P += lb[j];
    N += 1 - lb[j];
    const bool last = sg[j + 2] != s;
    if (last) { end_pos[s] = P; end_neg[s] = N; }
    if (s != run_seg) {
      if (run_key) atomicMax(&key[run_seg], run_key);
      if (run_seg >= 0) one_seg = false;
      run_seg = s;
      run_key = 0;
    }
    const float x = sc[j], y = sc[j + 1];
    if (!isnan(x) && (last || isnan(y) || x < y)) {
      const unsigned long long k = pack_cut(P - N, i);
      if (k > run_key) run_key = k;
    }
  }
  // a wave that lies inside one segment sends one atomic
  const int32_t s0 = __builtin_amdgcn_readfirstlane(run_seg);
  if (__all(one_seg && run_seg == s0)) {
    uint32_t hi = (uint32_t)(run_key >> 32), lo = (uint32_t)run_key;
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const uint32_t ohi = __shfl_xor(hi, m, kWave), olo = __shfl_xor(lo, m, kWave);
      if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
    }
    const unsigned long long k = ((unsigned long long)hi << 32) | lo;
    if (lane == 0 && k) atomicMax(&key[s0], k);
  } else if (run_key) {
    atomicMax(&key[run_seg], run_key);
  }
}

__global__ __launch_bounds__(kBlock) void fit_finish_kernel(const float* __restrict__ score, const int32_t* __restrict__ seg,
                                                            int64_t M, int32_t n_seg,
                                                            const unsigned long long* __restrict__ key,
                                                            const int32_t* __restrict__ start1,
                                                            const int32_t* __restrict__ base_pos,
                                                            const int32_t* __restrict__ base_neg,
                                                            const int32_t* __restrict__ end_pos,
                                                            const int32_t* __restrict__ end_neg, float* __restrict__ thr_lo,
                                                            float* __restrict__ thr_hi, int32_t* __restrict__ best_correct,
                                                            int32_t* __restrict__ n_pos, int32_t* __restrict__ n_neg) {
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n_seg; s += (int64_t)gridDim.x * kBlock) {
    const int32_t st = start1[s];
    float lo = -INFINITY, hi = INFINITY;
    int32_t bc = 0, np = 0, nn = 0;
    if (st > 0) {
      np = end_pos[s] - base_pos[s];
      nn = end_neg[s] - base_neg[s];
      const int32_t base = base_pos[s] - base_neg[s];
      const unsigned long long k = key[s];
      const int32_t g = (int32_t)((uint32_t)(k >> 32) - 0x80000000u);
      bc = nn;
      if (k != 0 && g > base) {                         // the cut after element i
        const int64_t i = (int64_t)(uint32_t)~(uint32_t)k;
        lo = score[i];
        if (i + 1 < M && seg[i + 1] == (int32_t)s) { const float y = score[i + 1]; if (!isnan(y)) hi = y; }
        bc = nn + (g - base);
      } else {                                          // accept nothing: thr_hi is the segment's smallest score
        const float y = score[(int64_t)st - 1];
        if (!isnan(y)) hi = y;
      }
    }
    thr_lo[s] = lo;
    thr_hi[s] = hi;
    best_correct[s] = bc;
    n_pos[s] = np;
    n_neg[s] = nn;
  }
}

// pred[i] = score[i] <= thr[seg[i]]; confusion[seg][tp, fp, tn, fn] by integer atomics, one set per wave where the wave
// holds one segment, else one per element.  This kernel serves calls without a confusion table and those with more
// than kHistMax counters; classify_hist_kernel serves the rest.
__global__ __launch_bounds__(kBlock) void classify_kernel(const float* __restrict__ score, const int32_t* __restrict__ seg,
                                                          const uint8_t* __restrict__ label, int64_t M, int32_t n_seg,
                                                          const float* __restrict__ thr, uint8_t* __restrict__ pred,
                                                          int32_t* __restrict__ confusion) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t rounds = (M + stride - 1) / stride;     // every lane makes every round: the wave votes below
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t i = r * stride + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t s = -1;
    bool p = false;
    if (i < M) {
      s = seg[i];
      if (s < 0 || s >= n_seg) s = -1;
      if (s >= 0) p = score[i] <= thr[s];               // false for a NaN on either side
      pred[i] = p ? 1 : 0;
    }
    if (confusion == nullptr) continue;
    const bool l = s >= 0 && label[i] != 0;
    const int cls = p ? (l ? 0 : 1) : (l ? 3 : 2);      // tp, fp, tn, fn
    const int32_t s0 = __builtin_amdgcn_readfirstlane(s);
    if (__all(s == s0)) {
      if (s0 < 0) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int n = __popcll(__ballot(cls == c));
        if (lane == 0 && n) atomicAdd(&confusion[(int64_t)s0 * 4 + c], n);
      }
    } else if (s >= 0) {
      atomicAdd(&confusion[(int64_t)s * 4 + cls], 1);
    }
  }
}

constexpr int kHistMax = 8192;          // confusion counters a workgroup holds in LDS (32 KB): n_seg <= 2048
constexpr int kHistPerThread = 32;      // elements a thread takes per chunk, four of them in flight

// The same decision with the confusion table counted in LDS first: one global atomic per workgroup and non-zero
// counter, where a relation that holds half of an unordered input would otherwise take half of all the atomics on its
// four counters.  A workgroup takes chunks of kBlock * kHistPerThread consecutive elements.
__global__ __launch_bounds__(kBlock) void classify_hist_kernel(const float* __restrict__ score,
                                                               const int32_t* __restrict__ seg,
                                                               const uint8_t* __restrict__ label, int64_t M, int32_t n_seg,
                                                               const float* __restrict__ thr, uint8_t* __restrict__ pred,
                                                               int32_t* __restrict__ confusion) {
  extern __shared__ int32_t hist[];     // [4 * n_seg]
  const int n_cnt = 4 * n_seg;
  for (int c = threadIdx.x; c < n_cnt; c += kBlock) hist[c] = 0;
  __syncthreads();
  constexpr int64_t kChunk = (int64_t)kBlock * kHistPerThread;
  for (int64_t base = (int64_t)blockIdx.x * kChunk; base < M; base += (int64_t)gridDim.x * kChunk) {
    for (int r = 0; r < kHistPerThread && base + (int64_t)r * kBlock < M; r += 4) {
      int32_t s[4];
      float x[4];
      int l[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t i = base + (int64_t)(r + k) * kBlock + threadIdx.x;
        const bool in = i < M;
        s[k] = in ? seg[i] : -1;
        x[k] = in ? score[i] : 0.f;
        l[k] = in ? label[i] != 0 : 0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t i = base + (int64_t)(r + k) * kBlock + threadIdx.x;
        if (i >= M) continue;
        const bool ok = s[k] >= 0 && s[k] < n_seg;
        const bool p = ok && x[k] <= thr[s[k]];         // false for a NaN on either side
        pred[i] = p ? 1 : 0;
        if (ok) atomicAdd(&hist[s[k] * 4 + (p ? (l[k] ? 0 : 1) : (l[k] ? 3 : 2))], 1);
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < n_cnt; c += kBlock) {
    const int32_t v = hist[c];
    if (v) atomicAdd(&confusion[c], v);
  }
}

}  // namespace

size_t threshold_fit_ws_bytes(int64_t M, int32_t n_seg) {
  if (M < 1 || M > INT32_MAX || n_seg < 1) return 0;
  return fit_layout(nullptr, M, n_seg).total;
}

int threshold_fit_launch(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                         float* thr_lo, float* thr_hi, int32_t* best_correct, int32_t* n_pos, int32_t* n_neg,
                         void* workspace, hipStream_t st) {
  const FitWs w = fit_layout(workspace, M, n_seg);
  const int64_t tiles = fit_tiles(M);
  hipError_t e = hipMemsetAsync(workspace, 0, w.seg_bytes, st);   // keys, starts, base and end counts: 0 = empty
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fit_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, seg, label, M, n_seg, w.tile_pos,
                     w.tile_neg);
  hipLaunchKernelGGL(fit_scan_kernel, dim3(1), dim3(1024), 0, st, w.tile_pos, w.tile_neg, tiles);
  hipLaunchKernelGGL(fit_cuts_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, score, seg, label, M, n_seg, w.tile_pos,
                     w.tile_neg, w.key, w.start1, w.base_pos, w.base_neg, w.end_pos, w.end_neg);
  hipLaunchKernelGGL(fit_finish_kernel, dim3(grid_for(n_seg, kBlock)), dim3(kBlock), 0, st, score, seg, M, n_seg, w.key,
                     w.start1, w.base_pos, w.base_neg, w.end_pos, w.end_neg, thr_lo, thr_hi, best_correct, n_pos, n_neg);
  return launch_status();
}

int threshold_classify_launch(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                              const float* thr, uint8_t* pred, int32_t* confusion, hipStream_t st) {
  if (confusion) {
    hipError_t e = hipMemsetAsync(confusion, 0, sizeof(int32_t) * 4 * (size_t)n_seg, st);
    if (e != hipSuccess) return (int)e;
  }
  if (M > 0 && confusion && n_seg <= kHistMax / 4) {
    const int64_t chunks = (M + kBlock * kHistPerThread - 1) / (kBlock * kHistPerThread);
    hipLaunchKernelGGL(classify_hist_kernel, dim3((unsigned)(chunks < 1024 ? chunks : 1024)), dim3(kBlock),
                       sizeof(int32_t) * 4 * (size_t)n_seg, st, score, seg, label, M, n_seg, thr, pred, confusion);
  } else if (M > 0) {
    hipLaunchKernelGGL(classify_kernel, dim3(grid_for(M, kBlock)), dim3(kBlock), 0, st, score, seg, label, M, n_seg, thr,
                       pred, confusion);
  }
  return launch_status();
}

}  // namespace ge
