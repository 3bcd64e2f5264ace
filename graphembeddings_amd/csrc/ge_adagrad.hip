// ge_adagrad.hip -- AdaGrad on the IndexedSlices of holE.py:296: TF1's AdagradOptimizer(lr, initial_accumulator_value)
// in place of GradientDescentOptimizer, duplicates summed first (_apply_sparse_duplicate_indices).
//
//   s           = the sum of every gradient row of the step that names the table row
//   accum[row] += s * s
//   table[row] -= lr * s / sqrt(accum[row])        (the updated accumulator, no epsilon)
//
// AdaGrad squares the SUM, so a row needs its complete sum before anything is written: the prepared step record
// (ge_prep.h) lists every distinct row once with all its gradient slots, and the two kernels below walk it the way the
// GE_STEP_DETERMINISTIC update of ge_train.hip does -- copies of that code, which itself stays as it is:
//
//   adagrad_items_kernel     one wavefront per work item sums the item's live slots in slot order; a single-item row is
//                            updated on the spot (table row and accumulator row requested together with the gradient
//                            rows), an item of a row split over several items parks its partial sum over the gradient
//                            row of its first slot;
//   adagrad_hot_rows_kernel  every split row: the parked partials in item order, then the one read-modify-write.
//
// The gradient rows hold MINUS the gradient (ge_hinge_grad at lr = 1), so the table row takes + lr * s / sqrt(accum).
// No float atomics anywhere: every sum has one fixed order, the results are bitwise reproducible.
// adagrad_rows_kernel is the same update for any IndexedSlices with a sort permutation (ge_adagrad_rows).
#include "ge_prep.h"
#include "ge_launch.h"

namespace ge {

// the update of one element; returns the new table value, a is the accumulator in and out
__device__ __forceinline__ float adagrad_elem(float t, float& a, float s, float lr) {
  a = a + s * s;
  return t + lr * s / sqrtf(a);
}

// Lane l holds VW consecutive columns of each of NJ lane rounds (d = 200: 50 lanes x 16 bytes, one request a row).
// Rows in flight per wave beside the table and accumulator rows: 32 row registers' worth.
template <int VW, int NJ>
__global__ __launch_bounds__(kBlock) void adagrad_items_kernel(
    float* __restrict__ table, float* __restrict__ accum, int d, const int32_t* __restrict__ sub0, int64_t sub_stride,
    int off_items, int off_islots, const int32_t* __restrict__ grad_idx, float* grad_val, float lr) {
  constexpr int NR = VW * NJ;
  constexpr int RG0 = 32 / NR;
  constexpr int RG = RG0 > 8 ? 8 : (RG0 < 2 ? 2 : RG0);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const int nwaves = (int)(((int64_t)gridDim.x * blockDim.x) >> 6);
  const int32_t* subrec = sub0 + (int64_t)blockIdx.y * sub_stride;
  const int32_t* items = subrec + off_items;
  const int32_t* islots = subrec + off_islots;
  const int n_items = subrec[0];
  int col[NJ];
  bool ok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) { col[j] = VW * (lane + kWave * j); ok[j] = col[j] < d; if (!ok[j]) col[j] = 0; }
  for (int w = wave; w < n_items; w += nwaves) {
    const int row = items[2 * w], cm = items[2 * w + 1];
    int slot_v = (lane < kItemCap) ? islots[w * kItemCap + lane] : -1;
    const int cnt = cm & 0x3FFFFFFF;
    const bool multi = (cm >> 30) & 1;
    // both rows of a single-item row are requested now, under the liveness flags and the gradient rows
    float* trow = table + (int64_t)row * d;
    float* arow = accum + (int64_t)row * d;
    float base[NJ][VW], acc2[NJ][VW];
    if (!multi) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) { load_vec<VW>(trow + col[j], base[j]); load_vec<VW>(arow + col[j], acc2[j]); }
    }
    const bool act_v = slot_v >= 0 && grad_idx[slot_v] >= 0;   // pair was hinge-active
    if (slot_v < 0) slot_v = 0;
    const uint32_t cap = cnt < kItemCap ? (1u << cnt) - 1u : (1u << kItemCap) - 1u;   // listed slots only
    uint32_t m = (uint32_t)__ballot(act_v) & cap;
    if (m == 0u && !multi) continue;                  // wave-uniform: no live slot, neither array is touched
    float sum[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) sum[r] = 0.f;
    // live rows in dense groups of RG, added in ascending slot order; a register that got no row holds +0
    while (m) {
      float v[RG][NR];
#pragma unroll
      for (int q = 0; q < RG; ++q) {
        if (m) {
          const int b = __builtin_ctz(m);
          m &= m - 1u;
          const float* src = grad_val + (int64_t)__builtin_amdgcn_readlane(slot_v, b) * d;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            float wv[VW];
            load_vec<VW>(src + col[j], wv);
#pragma unroll
            for (int e = 0; e < VW; ++e) v[q][j * VW + e] = wv[e];
          }
        } else {
#pragma unroll
          for (int r = 0; r < NR; ++r) v[q][r] = 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < RG; ++q)
#pragma unroll
        for (int r = 0; r < NR; ++r) sum[r] += v[q][r];
    }
    if (multi) {
      // a row of more than 16 slots: this item's sum (zeros included) waits for adagrad_hot_rows_kernel
      float* parked = grad_val + (int64_t)__builtin_amdgcn_readlane(slot_v, 0) * d;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!ok[j]) continue;
        float o_[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) o_[e] = sum[j * VW + e];
        store_vec<VW>(parked + col[j], o_);
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      float t_[VW], a_[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        a_[e] = acc2[j][e];
        t_[e] = adagrad_elem(base[j][e], a_[e], sum[j * VW + e], lr);
      }
      store_vec<VW>(arow + col[j], a_);
      store_vec<VW>(trow + col[j], t_);
    }
  }
}

// Every row that is split over several items (its items are consecutive in the sorted item lists, possibly across a
// tile boundary) is reduced by ONE workgroup in a fixed order: a row of fewer than 64 items by one wave (the parked
// partials in item order), a longer one by the eight waves of the workgroup (wave j: items j, j + 8, ... in that order;
// the wave sums added in wave order).  Workgroup (b, t) looks at items [64 b, 64 b + 64) of tile t for HEADS (a multi
// item whose predecessor belongs to another row) and reduces the rows that start there.  A row whose sum is zero in
// every column (no live slot in any item) is left alone.
constexpr int kAdaHotBlock = 512;
template <int NJ>
__global__ __launch_bounds__(kAdaHotBlock) void adagrad_hot_rows_kernel(
    float* __restrict__ table, float* __restrict__ accum, int d, const int32_t* __restrict__ sub0, int64_t sub_stride,
    int off_items, int off_islots, int n_sub, const float* __restrict__ grad_val, float lr) {
  constexpr int kScan = kWave;
  constexpr int kWv = kAdaHotBlock / kWave;
  __shared__ int heads[kScan];
  __shared__ int n_heads;
  __shared__ float part[kWv - 1][NJ * kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6, tile = blockIdx.y;
  auto sub_of = [&](int tl) { return sub0 + (int64_t)tl * sub_stride; };
  const int32_t* subrec = sub_of(tile);
  const int n_items = subrec[0];
  // the item at flattened position k0 + r of the row that starts at item k0 of this tile: (belongs to the row?, first slot)
  auto item_at = [&](int k0, int r, int row, int& first_slot) -> bool {
    int idx = k0 + r, tl = tile;
    const int32_t* sr = subrec;
    int ni = n_items;
    while (idx >= ni) {
      idx -= ni; ++tl;
      if (tl >= n_sub) return false;
      sr = sub_of(tl); ni = sr[0];
    }
    first_slot = sr[off_islots + idx * kItemCap];
    return sr[off_items + 2 * idx] == row;             // the row's items are consecutive: valid r form a prefix
  };
  // n parked rows (first slots in lanes 0 .. n-1 of `fs`) added to acc in lane order
  constexpr int kInFlight = NJ <= 4 ? 16 : 8;
  auto add_rows = [&](int fs, int n, float (&acc)[NJ]) {
    for (int o = 0; o < n; o += kInFlight) {
      float v[kInFlight][NJ];
#pragma unroll
      for (int q = 0; q < kInFlight; ++q)
        if (o + q < n) {
          const float* src = grad_val + (int64_t)__shfl(fs, o + q, kWave) * d;
#pragma unroll
          for (int j = 0; j < NJ; ++j) { const int c = lane + kWave * j; v[q][j] = src[c < d ? c : 0]; }
        }
#pragma unroll
      for (int q = 0; q < kInFlight; ++q)
        if (o + q < n) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] += v[q][j];
        }
    }
  };
  // the one read-modify-write of a row, by one wave
  auto update = [&](int row, const float (&s)[NJ]) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) any = any || s[j] != 0.f;
    if (__ballot(any) == 0ull) return;                 // wave-uniform
    float* trow = table + (int64_t)row * d;
    float* arow = accum + (int64_t)row * d;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + kWave * j;
      if (c < d) {
        float a = arow[c];
        const float tv = adagrad_elem(trow[c], a, s[j], lr);
        arow[c] = a;
        trow[c] = tv;
      }
    }
  };
  for (int win = blockIdx.x; win * kScan < n_items; win += gridDim.x) {    // (block-uniform trip count)
    if (t == 0) n_heads = 0;
    __syncthreads();
    const int k = win * kScan + t;
    if (t < kScan && k < n_items) {
      const int32_t* items = subrec + off_items;
      const int row = items[2 * k], cm = items[2 * k + 1];
      if ((cm >> 30) & 1) {
        int prev_row = -1;
        if (k > 0) prev_row = items[2 * (k - 1)];
        else if (tile > 0) { const int32_t* ps = sub_of(tile - 1); const int pn = ps[0]; if (pn > 0) prev_row = ps[off_items + 2 * (pn - 1)]; }
        if (prev_row != row) heads[atomicAdd(&n_heads, 1)] = k;   // (any order: every head is reduced independently)
      }
    }
    __syncthreads();
    const int nh = n_heads;
    // (1) rows of fewer than 64 items (nearly all): one WAVE a row, the window's heads spread over the waves
    for (int h = wv; h < nh; h += kWv) {
      const int k0 = heads[h];
      const int row = (subrec + off_items)[2 * k0];
      int fs = 0;
      const bool mine = item_at(k0, lane, row, fs);
      const int n = __popcll(__ballot(mine));
      if (n == kWave) continue;                          // a long row: step (2)
      float acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
      add_rows(fs, n, acc);
      update(row, acc);
      if (lane == 0) heads[h] = -1;                       // done
    }
    __syncthreads();
    // (2) rows of 64 items and more: the whole workgroup, wave j taking items j, j + 8, ...
    for (int h = 0; h < nh; ++h) {
      const int k0 = heads[h];
      if (k0 < 0) continue;                              // (block-uniform: heads[] is read after the barrier)
      const int row = (subrec + off_items)[2 * k0];
      float acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
      for (int r0 = wv; ; r0 += kWv * kWave) {
        int fs = 0;
        const bool mine = item_at(k0, r0 + kWv * lane, row, fs);
        const int n = __popcll(__ballot(mine));
        add_rows(fs, n, acc);
        if (n < kWave) break;                            // wave-uniform
      }
      if (wv > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) part[wv - 1][j * kWave + lane] = acc[j];
      }
      __syncthreads();
      if (wv == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int w2 = 0; w2 < kWv - 1; ++w2) acc[j] += part[w2][j * kWave + lane];
        update(row, acc);
      }
      __syncthreads();
    }
    __syncthreads();
  }
}

int adagrad_items_launch(float* table, float* accum, int d, const TileGeom& G, const int32_t* step_rec, const int32_t* gidx,
                         float* gval, float lr, hipStream_t st) {
  const int nj = (d + kWave - 1) / kWave;
  if (d <= 0 || nj > 16) return GE_ENOTSUP;
  const int vw = (d % 4 == 0 && aligned16({table, accum, gval})) ? 4
               : (d % 2 == 0 && (((uintptr_t)table | (uintptr_t)accum | (uintptr_t)gval) & 7) == 0) ? 2 : 1;
  const int njr = (d / vw + kWave - 1) / kWave;
  // one wave per key of a one-tile step, per 8 keys of a tile of a larger one (apply_items_launch has the measurements)
  const dim3 g((unsigned)(G.n_sub > 1 ? grid_for((G.P + 7) / 8, kBlock / kWave) : grid_for(G.P, kBlock / kWave)), (unsigned)G.n_sub);
  const int32_t* sub0 = step_rec + G.off_sub;
#define LI(VW, NJ) hipLaunchKernelGGL((adagrad_items_kernel<VW, NJ>), g, dim3(kBlock), 0, st, table, accum, d, sub0, G.sub_stride, G.off_items, G.off_islots, gidx, gval, lr)
  if (vw == 4) { if (njr <= 1) LI(4, 1); else if (njr <= 2) LI(4, 2); else LI(4, 4); }
  else if (vw == 2) { if (njr <= 1) LI(2, 1); else if (njr <= 2) LI(2, 2); else if (njr <= 4) LI(2, 4); else LI(2, 8); }
  else { if (njr <= 1) LI(1, 1); else if (njr <= 2) LI(1, 2); else if (njr <= 4) LI(1, 4); else if (njr <= 8) LI(1, 8); else LI(1, 16); }
#undef LI
  int rc = launch_status();
  if (rc) return rc;
  const dim3 gh((unsigned)((G.P + kWave - 1) / kWave), (unsigned)G.n_sub);   // one 64-item window a workgroup
#define LH(NJ) hipLaunchKernelGGL((adagrad_hot_rows_kernel<NJ>), gh, dim3(kAdaHotBlock), 0, st, table, accum, d, sub0, G.sub_stride, G.off_items, G.off_islots, G.n_sub, gval, lr)
  if (nj <= 1) LH(1); else if (nj <= 2) LH(2); else if (nj <= 4) LH(4); else if (nj <= 8) LH(8); else LH(16);
#undef LH
  return launch_status();
}

// ------------------------------------------------------------------ any IndexedSlices (ge_adagrad_rows)
// perm is the stable argsort of (idx[i] < 0 ? N : idx[i]): a row's occurrences are consecutive in perm order.  One wave
// per position: the wave at the FIRST occurrence of a row walks the run (64 positions looked up at a time, the rows
// added one after the other in perm order, 256 columns a pass) and does the row's read-modify-write.  A run may be all
// R positions.  Positions whose perm entry lies outside [0, R), or whose id is negative or >= N, belong to no run and
// are never dereferenced.
__device__ __forceinline__ int64_t adagrad_key(const int32_t* __restrict__ idx, const int32_t* __restrict__ perm, int64_t R,
                                               int64_t N, int64_t p, int64_t& i) {
  if (p < 0 || p >= R) return -1;
  i = perm[p];
  if (i < 0 || i >= R) return -1;
  const int64_t id = idx[i];
  return (id < 0 || id >= N) ? -1 : id;
}

__global__ __launch_bounds__(kBlock) void adagrad_rows_kernel(
    float* __restrict__ table, float* __restrict__ accum, int64_t N, int d, const int32_t* __restrict__ idx,
    const float* __restrict__ val, const int32_t* __restrict__ perm, int64_t R, float lr) {
  constexpr int NC = 4;                                  // lane rounds of a column pass
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p = wave; p < R; p += nwaves) {
    int64_t i0 = 0, ip = 0;
    const int64_t id = adagrad_key(idx, perm, R, N, p, i0);
    if (id < 0 || adagrad_key(idx, perm, R, N, p - 1, ip) == id) continue;   // wave-uniform: not the head of a run
    float* trow = table + id * d;
    float* arow = accum + id * d;
    for (int c0 = 0; c0 < d; c0 += NC * kWave) {
      float s[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) s[j] = 0.f;
      for (int64_t q0 = p; ; q0 += kWave) {
        int64_t iq = 0;
        const bool mine = adagrad_key(idx, perm, R, N, q0 + lane, iq) == id;
        const unsigned long long bal = __ballot(mine);
        const int n = bal == ~0ull ? kWave : __builtin_ctzll(~bal);           // the run's members form a prefix
        const int src_i = (int)iq;
        for (int o = 0; o < n; ++o) {
          const float* src = val + (int64_t)__shfl(src_i, o, kWave) * d;
#pragma unroll
          for (int j = 0; j < NC; ++j) { const int c = c0 + lane + kWave * j; if (c < d) s[j] += src[c]; }
        }
        if (n < kWave) break;                            // wave-uniform
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = c0 + lane + kWave * j;
        if (c < d) {
          float a = arow[c];
          const float tv = adagrad_elem(trow[c], a, s[j], lr);
          arow[c] = a;
          trow[c] = tv;
        }
      }
    }
  }
}

int adagrad_rows_launch(float* table, float* accum, int64_t N, int32_t d, const int32_t* idx, const float* val,
                        const int32_t* perm, int64_t R, float lr, hipStream_t st) {
  if (d <= 0) return GE_EINVAL;
  if (R == 0) return 0;
  hipLaunchKernelGGL(adagrad_rows_kernel, dim3(grid_for(R, kBlock / kWave)), dim3(kBlock), 0, st, table, accum, N, d, idx,
                     val, perm, R, lr);
  return launch_status();
}

}  // namespace ge
