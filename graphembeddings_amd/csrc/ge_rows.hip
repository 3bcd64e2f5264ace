// ge_rows.hip -- row scatter-add (the ScatterSub of holE.py:296), row gather, and the type-safe
// corruption sampler (holE.py:97-140 fused with the host resample of holE.py:343-347).
#include "ge_common.h"
#include "ge_bernoulli_dev.h"
#include "ge_launch.h"

namespace ge {

// table[idx[i]] += val[i]  -- one wavefront per row, one dword per lane per atomic instruction,
// 256 contiguous bytes per wave-instruction (the shape the memory-side float atomics run at full
// rate for).  Duplicated indices all land (ScatterSub semantics, graph.pbtxt:47850-48001).
__global__ __launch_bounds__(kBlock) void scatter_add_rows_kernel(
    float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ idx,
    const float* __restrict__ val, int64_t R) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < R; r += nwaves) {
    const int32_t id = idx[r];
    if (id < 0 || id >= N) continue;
    float* dst = table + (int64_t)id * d;
    const float* src = val + r * d;
    for (int c = lane; c < d; c += kWave) atomic_add_f32(dst + c, src[c]);
  }
}

// out[i] = table[idx[i]]  (zeros for idx < 0) -- one wavefront per row.
template <int VEC>
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(
    const float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ idx, int64_t R,
    float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nvec = d / VEC;
  for (int64_t r = wave; r < R; r += nwaves) {
    const int32_t id = idx[r];
    const bool ok = id >= 0 && id < N;
    const float* src = table + (int64_t)(ok ? id : 0) * d;
    float* dst = out + r * d;
    for (int j = lane; j < nvec; j += kWave) {
      float v[VEC];
      if (ok) load_vec<VEC>(src + j * VEC, v);
      else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] = 0.f;
      }
      store_vec<VEC>(dst + j * VEC, v);
    }
  }
}

__global__ __launch_bounds__(kBlock) void corrupt_batch_kernel(
    const int32_t* __restrict__ pos, int64_t B, const int32_t* __restrict__ id_to_type, int64_t N,
    const int64_t* __restrict__ type_offsets, int32_t n_types, const int32_t* __restrict__ type_ids,
    uint64_t seed, uint64_t step, int32_t padded_size, int32_t mode, int32_t* __restrict__ neg) {
  const bool batch_heads = (mode == GE_CORRUPT_BATCH_COIN) ? batch_coin_heads(seed, step) : false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t t[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    int col;
    const int32_t repl = corrupt_one(t, i, batch_heads, id_to_type, N, type_offsets, n_types, type_ids,
                                     seed, step, padded_size, mode, col);
    t[col] = repl;
    neg[3 * i] = t[0]; neg[3 * i + 1] = t[1]; neg[3 * i + 2] = t[2];
  }
}

// ---------------------------------------------------------------- Bernoulli filtered sampler
// GPU form of the reference's native sampler init.so (init.cpp:159-246): the side to corrupt is
// chosen per triple with P(tail) = hpt/(hpt+tph) of its relation (init.cpp:226-228) and the
// replacement is drawn uniformly among the entities that do NOT complete a known triple, by mapping
// tmp in [0, E - cnt) past the sorted known entities of the (fixed entity, relation) key with a
// binary search (init.cpp:177-188).  One thread per triple, per-row Philox draws instead of the
// reference's single global LCG (init.cpp:145-150); the two init.cpp defects (sizeof(pointer) memset,
// `j < rig` loop bound) live in the host-side statistics and are fixed there.
__global__ __launch_bounds__(kBlock) void bernoulli_corrupt_kernel(
    const int32_t* __restrict__ pos, int64_t B, const int64_t* __restrict__ bh_key,
    const int32_t* __restrict__ bh_ent, const int64_t* __restrict__ bt_key,
    const int32_t* __restrict__ bt_ent, int64_t n_known, const uint32_t* __restrict__ tail_threshold,
    int32_t n_rel, int32_t ent_lo, int32_t n_ent, uint64_t seed, uint64_t step, int32_t* __restrict__ neg) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t t[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    bernoulli_corrupt_row(t, i, bh_key, bh_ent, bt_key, bt_ent, n_known, tail_threshold, n_rel, ent_lo, n_ent,
                          seed, step);
    neg[3 * i] = t[0]; neg[3 * i + 1] = t[1]; neg[3 * i + 2] = t[2];
  }
}

int bernoulli_corrupt_launch(const int32_t* pos, int64_t B, const SamplerArgs& s, int32_t ent_lo, uint64_t seed,
                             uint64_t step, int32_t* neg, hipStream_t st) {
  if (s.n_known < 0 || s.n_rel <= 0 || s.n_ent <= 0) return GE_EINVAL;
  if (B == 0) return 0;
  const int grid = grid_for(B, kBlock);
  hipLaunchKernelGGL(bernoulli_corrupt_kernel, dim3(grid), dim3(kBlock), 0, st, pos, B, s.bh_key, s.bh_ent, s.bt_key,
                     s.bt_ent, s.n_known, s.tail_threshold, s.n_rel, ent_lo, s.n_ent, seed, step, neg);
  return launch_status();
}

int scatter_add_rows_launch(float* table, int64_t N, int32_t d, const int32_t* idx, const float* val,
                            int64_t R, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (d <= 0) return GE_EINVAL;
  if (R == 0) return 0;
  const int grid = grid_for(R, kBlock / kWave);
  hipExtLaunchKernelGGL(scatter_add_rows_kernel, dim3(grid), dim3(kBlock), 0, st, ev_start, ev_stop, 0, table, N, d, idx, val, R);
  return launch_status();
}

int gather_rows_launch(const float* table, int64_t N, int32_t d, const int32_t* idx, int64_t R,
                       float* out, hipStream_t st) {
  if (d <= 0) return GE_EINVAL;
  if (R == 0) return 0;
  const int grid = grid_for(R, kBlock / kWave);
  const uintptr_t a = reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out);
  if (d % 4 == 0 && a % 16 == 0)
    hipLaunchKernelGGL(gather_rows_kernel<4>, dim3(grid), dim3(kBlock), 0, st, table, N, d, idx, R, out);
  else if (d % 2 == 0 && a % 8 == 0)
    hipLaunchKernelGGL(gather_rows_kernel<2>, dim3(grid), dim3(kBlock), 0, st, table, N, d, idx, R, out);
  else
    hipLaunchKernelGGL(gather_rows_kernel<1>, dim3(grid), dim3(kBlock), 0, st, table, N, d, idx, R, out);
  return launch_status();
}

int corrupt_batch_launch(const int32_t* pos, int64_t B, const TypeSampler& ts, uint64_t step, int32_t* neg, hipStream_t st) {
  if (!sampler_ranges_ok(ts)) return GE_EINVAL;
  if (B == 0) return 0;
  const int grid = grid_for(B, kBlock);
  hipLaunchKernelGGL(corrupt_batch_kernel, dim3(grid), dim3(kBlock), 0, st, pos, B, ts.id_to_type, ts.N,
                     ts.type_offsets, ts.n_types, ts.type_ids, ts.seed, step, ts.padded_size, ts.mode, neg);
  return launch_status();
}

// ---------------------------------------------------------------- validation tick (holE.py:299-304, 351-360)
#define GE_TAG_VSEL 0x7673656Cu

// a batch of validation triples drawn uniformly with replacement (the reference takes them from a shuffle queue
// over the validation split, holE.py:300): out[i] = valid[philox(seed, counter, i) % V]
__global__ __launch_bounds__(kBlock) void select_rows_kernel(const int32_t* __restrict__ valid, int64_t V, int64_t B,
                                                             uint64_t seed, uint64_t counter, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B) return;
  const uint32_t w0 = philox_w0((uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)i, (uint32_t)(i >> 32),
                                (uint32_t)seed ^ GE_TAG_VSEL, (uint32_t)(seed >> 32));
  const uint32_t w1 = philox_w0((uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)i, (uint32_t)(i >> 32) ^ 0x80000000u,
                                (uint32_t)seed ^ GE_TAG_VSEL, (uint32_t)(seed >> 32));
  const uint64_t r = (((uint64_t)w1 << 32) | w0) % (uint64_t)V;
  out[3 * i] = valid[3 * r];
  out[3 * i + 1] = valid[3 * r + 1];
  out[3 * i + 2] = valid[3 * r + 2];
}

// one workgroup: mean of the loss vector (fixed summation order: bitwise reproducible) -> *mean_out; the pocket
// bookkeeping of holE.py:357-360 on the device: improved = mean < *best, *best = min, *flag = improved
__global__ __launch_bounds__(1024) void mean_pocket_kernel(const float* __restrict__ loss, int64_t B,
                                                           float* __restrict__ mean_out, float* __restrict__ best,
                                                           int32_t* __restrict__ flag) {
  __shared__ double part[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 1024) s += (double)loss[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, kWave);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    const float mean = (float)(t / (double)B);
    *mean_out = mean;
    const bool improved = mean < *best;     // a NaN loss never improves
    if (improved) *best = mean;
    *flag = improved ? 1 : 0;
  }
}

// one workgroup: the summary of holE.py:475-490 from the counts of a rank sweep, and the pocket bookkeeping on the
// filtered MRR (higher is better).  Row i counts iff its true_loss is not NaN (the sweeps' bad rows: counts 0, true_loss
// NaN -- they must not score as rank 1) and 0 <= n_known_before[i] <= n_before[i].  Every sum has one fixed order
// (thread-strided, xor shuffles, the 16 wave partials in turn): two calls agree bitwise.  The rank sums and the hit
// counts are integers, added as 64-bit integers and converted once; each output is one double division rounded to float.
// n = 0: 0.0 / 0.0 = NaN in entries 0-6.
__global__ __launch_bounds__(1024) void rank_metrics_kernel(const int32_t* __restrict__ n_before,
                                                            const int32_t* __restrict__ n_known_before,
                                                            const float* __restrict__ true_loss, int64_t M,
                                                            float* __restrict__ metrics_out, float* __restrict__ best,
                                                            int32_t* __restrict__ improved) {
  __shared__ double part_d[2][16];
  __shared__ long long part_i[6][16];
  double inv_fil = 0.0, inv_raw = 0.0;
  long long v[6] = {0, 0, 0, 0, 0, 0};      // sum of filtered ranks, of raw ranks, hits at 1 / 3 / 10, counted rows
  for (int64_t i = threadIdx.x; i < M; i += 1024) {
    const int32_t nb = n_before[i], nk = n_known_before[i];
    if (nk < 0 || nk > nb) continue;
    if (true_loss) {
      const float tl = true_loss[i];
      if (tl != tl) continue;
    }
    const long long raw = 1ll + nb, fil = raw - nk;
    inv_fil += 1.0 / (double)fil;
    inv_raw += 1.0 / (double)raw;
    v[0] += fil;
    v[1] += raw;
    v[2] += fil <= 1;
    v[3] += fil <= 3;
    v[4] += fil <= 10;
    v[5] += 1;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    inv_fil += __shfl_xor(inv_fil, m, kWave);
    inv_raw += __shfl_xor(inv_raw, m, kWave);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] += __shfl_xor(v[j], m, kWave);
  }
  if ((threadIdx.x & 63) == 0) {
    part_d[0][threadIdx.x >> 6] = inv_fil;
    part_d[1][threadIdx.x >> 6] = inv_raw;
    for (int j = 0; j < 6; ++j) part_i[j][threadIdx.x >> 6] = v[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sf = 0.0, sr = 0.0;
    long long t[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 16; ++w) {
      sf += part_d[0][w];
      sr += part_d[1][w];
      for (int j = 0; j < 6; ++j) t[j] += part_i[j][w];
    }
    const double n = (double)t[5];
    const float mrr = (float)(sf / n);
    metrics_out[0] = mrr;
    metrics_out[1] = (float)(sr / n);
    metrics_out[2] = (float)((double)t[0] / n);
    metrics_out[3] = (float)((double)t[1] / n);
    metrics_out[4] = (float)((100.0 * (double)t[2]) / n);
    metrics_out[5] = (float)((100.0 * (double)t[3]) / n);
    metrics_out[6] = (float)((100.0 * (double)t[4]) / n);
    metrics_out[7] = (float)n;
    bool better = false;
    if (best) {
      better = mrr > *best;                 // a NaN never improves, an equal value keeps the first best
      if (better) *best = mrr;
    }
    if (improved) *improved = better ? 1 : 0;
  }
}

// pocket <- table iff *flag (the flag is read on the device: no host decision, no synchronisation)
__global__ __launch_bounds__(kBlock) void copy_if_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                         int64_t n4, const float* __restrict__ src_tail,
                                                         float* __restrict__ dst_tail, int n_tail,
                                                         const int32_t* __restrict__ flag) {
  if (*flag == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) dst[i] = src[i];
  if (blockIdx.x == 0 && (int)threadIdx.x < n_tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}

// ge_copy_if: every segment's dst <- src iff *flag, all segments in one launch.  Workgroup b moves chunk b of
// kCopyIfChunk words; chunk_start[s] is the first chunk of segment s (ascending: the launcher drops empty segments), so
// the segment of b is the number of starts at or below it.  b, the starts and the table entries are wave-uniform: the
// lookup reads the by-value table with scalar loads.  A chunk begins a multiple of 32 KiB into its segment, so it is
// 16-byte aligned iff the segment is.
__global__ __launch_bounds__(kBlock) void copy_if_segments_kernel(const int32_t* __restrict__ flag, CopyIfSegments t) {
  if (*flag == 0) return;
  const int64_t b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 1; k < GE_COPY_IF_MAX_SEGMENTS; ++k) s += (k < t.n_seg && b >= t.chunk_start[k]) ? 1 : 0;
  const int64_t off = (b - t.chunk_start[s]) * kCopyIfChunk;
  const uint32_t* src = t.src[s] + off;
  uint32_t* dst = t.dst[s] + off;
  const int n = (int)std::min<int64_t>(t.count[s] - off, kCopyIfChunk);
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0) {
    const int n4 = n / 4;
    const uint4* src4 = reinterpret_cast<const uint4*>(src);
    uint4* dst4 = reinterpret_cast<uint4*>(dst);
    if (n == kCopyIfChunk) {                            // a whole chunk: its 8 loads a lane in flight together
      uint4 v[kCopyIfChunk / 4 / kBlock];
#pragma unroll
      for (int j = 0; j < kCopyIfChunk / 4 / kBlock; ++j) v[j] = src4[j * kBlock + threadIdx.x];
#pragma unroll
      for (int j = 0; j < kCopyIfChunk / 4 / kBlock; ++j) dst4[j * kBlock + threadIdx.x] = v[j];
      return;
    }
    for (int i = threadIdx.x; i < n4; i += kBlock) dst4[i] = src4[i];
    const int i = 4 * n4 + (int)threadIdx.x;            // the count % 4 words after the last whole 16 bytes
    if (i < n) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
  }
}

int copy_if_segments_launch(const int32_t* flag, int32_t n_seg, const float* const* src, float* const* dst,
                            const int64_t* count, hipStream_t st) {
  CopyIfSegments t{};
  int64_t chunks = 0;
  for (int32_t s = 0; s < n_seg; ++s) {
    if (count[s] == 0) continue;
    t.src[t.n_seg] = reinterpret_cast<const uint32_t*>(src[s]);
    t.dst[t.n_seg] = reinterpret_cast<uint32_t*>(dst[s]);
    t.count[t.n_seg] = count[s];
    t.chunk_start[t.n_seg++] = chunks;
    chunks += (count[s] + kCopyIfChunk - 1) / kCopyIfChunk;
  }
  if (chunks == 0) return 0;
  if (chunks > INT32_MAX) return GE_ENOTSUP;
  hipLaunchKernelGGL(copy_if_segments_kernel, dim3((unsigned)chunks), dim3(kBlock), 0, st, flag, t);
  return launch_status();
}

int select_rows_launch(const int32_t* valid, int64_t V, int64_t B, uint64_t seed, uint64_t counter, int32_t* out,
                       hipStream_t st) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(select_rows_kernel, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, st, valid, V, B, seed, counter, out);
  return launch_status();
}

int mean_pocket_launch(const float* loss, int64_t B, float* mean_out, float* best, int32_t* flag, hipStream_t st) {
  hipLaunchKernelGGL(mean_pocket_kernel, dim3(1), dim3(1024), 0, st, loss, B, mean_out, best, flag);
  return launch_status();
}

int rank_metrics_launch(const int32_t* n_before, const int32_t* n_known_before, const float* true_loss, int64_t M,
                        float* metrics_out, float* best, int32_t* improved, hipStream_t st) {
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(1), dim3(1024), 0, st, n_before, n_known_before, true_loss, M, metrics_out,
                     best, improved);
  return launch_status();
}

// what copy_if_launch takes: 16-byte aligned buffers, or no more floats than its tail path copies
bool copy_if_ok(const float* src, const float* dst, int64_t n) {
  const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  return vec || n <= kBlock;
}

int copy_if_launch(const float* src, float* dst, int64_t n, const int32_t* flag, hipStream_t st) {
  if (n == 0) return 0;
  const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  const int64_t rest = n - 4 * n4;
  if (rest > kBlock) {   // unaligned buffers: plain float copy through the tail path is not enough; fall back to scalars
    return GE_EINVAL;
  }
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n4 + kBlock - 1) / kBlock, 256 * 8));
  hipLaunchKernelGGL(copy_if_kernel, dim3(grid), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(src),
                     reinterpret_cast<float4*>(dst), n4, src + 4 * n4, dst + 4 * n4, (int)rest, flag);
  return launch_status();
}

}  // namespace ge
