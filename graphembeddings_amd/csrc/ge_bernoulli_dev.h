// ge_bernoulli_dev.h -- one row of the filtered Bernoulli sampler (init.cpp:159-246), shared by
// bernoulli_corrupt_kernel (ge_rows.hip), the TransX training loop's draw kernel (ge_transx.hip) and the K-negative draw
// of RotatE's self-adversarial loop (ge_rotate_adv.hip), which takes the pick alone.
#pragma once
#include "ge_common.h"

namespace ge {

__device__ __forceinline__ int64_t lower_bound64(const int64_t* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ int64_t upper_bound64(const int64_t* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}

#define GE_TAG_BSIDE 0x62736964u
#define GE_TAG_BPICK 0x62706963u
#define GE_TAG_TXDRAW 0x74786472u      // the native loops' pick of a positive row (ge_transx.hip, ge_rotate_adv.hip)

// The known completions of (fixed entity, relation) on one side: a sorted run [first, first + cnt) of `ent`.
struct KnownRun { const int32_t* ent; int64_t first, cnt; };

__device__ __forceinline__ KnownRun known_run(bool tail_side, int32_t fixed, int32_t r,
                                              const int64_t* __restrict__ bh_key, const int32_t* __restrict__ bh_ent,
                                              const int64_t* __restrict__ bt_key, const int32_t* __restrict__ bt_ent,
                                              int64_t n_known, int32_t n_rel) {
  const int64_t* key_arr = tail_side ? bh_key : bt_key;
  const int64_t key = (int64_t)fixed * n_rel + r;
  const int64_t first = lower_bound64(key_arr, n_known, key);
  const int64_t last = upper_bound64(key_arr, n_known, key) - 1;
  return KnownRun{tail_side ? bh_ent : bt_ent, first, last >= first ? last - first + 1 : 0};
}

// The entity the 32-bit word w_pick draws among those in [ent_lo, ent_lo + n_ent) that are NOT in the run; -1 when the
// run leaves none free.
__device__ __forceinline__ int32_t pick_free_entity(const KnownRun& k, uint32_t w_pick, int32_t ent_lo, int32_t n_ent) {
  const int64_t first = k.first, cnt = k.cnt, last = first + cnt - 1;
  const int64_t free_n = (int64_t)n_ent - cnt;
  if (free_n <= 0) return -1;
  // the draw-th entity that is NOT a known completion (init.cpp:159-190: skip the known ones by bisection on
  // "free entities below the p-th known one" = ent[p] - ent_lo - (p - first))
  const int64_t draw = (int64_t)(((uint64_t)w_pick * (uint64_t)free_n) >> 32);
  auto free_below = [&](int64_t p) { return (int64_t)k.ent[p] - ent_lo - (p - first); };
  int64_t j;
  if (cnt == 0 || draw < free_below(first)) j = draw;
  else if (draw >= free_below(last)) j = draw + cnt;
  else {
    int64_t below = first, above = last + 1;        // free_below(below) <= draw < free_below(above)
    while (below + 1 < above) {
      const int64_t probe = (below + above) >> 1;
      if (free_below(probe) <= draw) below = probe; else above = probe;
    }
    j = draw + (below - first + 1);
  }
  return ent_lo + (int32_t)j;
}

// Corrupts t (h, t, r) in place as row i of step `step`: a relation outside [0, n_rel) gives (-1,-1,-1),
// a (fixed entity, relation) key with no free entity gives -1 in the corrupted column.
__device__ __forceinline__ void bernoulli_corrupt_row(
    int32_t (&t)[3], int64_t i, const int64_t* __restrict__ bh_key, const int32_t* __restrict__ bh_ent,
    const int64_t* __restrict__ bt_key, const int32_t* __restrict__ bt_ent, int64_t n_known,
    const uint32_t* __restrict__ tail_threshold, int32_t n_rel, int32_t ent_lo, int32_t n_ent, uint64_t seed,
    uint64_t step) {
  const uint32_t slo = (uint32_t)step, shi = (uint32_t)(step >> 32);
  const uint32_t klo = (uint32_t)seed, khi = (uint32_t)(seed >> 32);
  const int32_t r = t[2];
  if (r < 0 || r >= n_rel) { t[0] = -1; t[1] = -1; t[2] = -1; return; }
  const uint32_t ilo = (uint32_t)i, ihi = (uint32_t)((uint64_t)i >> 32);
  const uint32_t w_side = philox_w0(slo, shi, ilo, ihi, klo ^ GE_TAG_BSIDE, khi);
  const uint32_t w_pick = philox_w0(slo, shi, ilo, ihi, klo ^ GE_TAG_BPICK, khi);
  const bool tail_side = w_side < tail_threshold[r];
  const KnownRun run = known_run(tail_side, tail_side ? t[0] : t[1], r, bh_key, bh_ent, bt_key, bt_ent, n_known, n_rel);
  t[tail_side ? 1 : 0] = pick_free_entity(run, w_pick, ent_lo, n_ent);
}

}  // namespace ge
