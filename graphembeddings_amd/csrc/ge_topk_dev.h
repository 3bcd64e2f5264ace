// ge_topk_dev.h -- what the two top-k sweeps (ge_rank_f16.hip MODE 3: ComplEx / HolE; ge_transx_rank.hip: the
// translation models) share: candidate keys, and the one-wave rank / cut / emit / merge of a pool of keys.
// NL: pool entries per lane, so a pool holds at most NL * 64 keys.
#pragma once
#include "ge_common.h"
#include "ge_sweep_route.h"

namespace ge {

typedef unsigned long long u64;
constexpr u64 kNoKey = ~0ull;           // (also the padding of a partial list)

// A candidate's key: (value bits, entity id) as one unsigned 64-bit number.  For values that are never negative, -0.0
// or NaN the integer order of the keys is the order ascending by (value, id); distinct candidates have distinct keys.
__device__ __forceinline__ u64 topk_key(float e, int32_t id) { return ((u64)__float_as_uint(e) << 32) | (unsigned)id; }

// (topk_kp(k), the pool size past which a pool is cut back to k: ge_sweep_route.h, where the workspace size needs it)

__device__ __forceinline__ u64 readlane64(u64 x, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)x, l);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
  return ((u64)hi << 32) | lo;
}

// One wave: the first n (<= NL * 64) keys of `pool`, entry m * 64 + lane in key[m], and each one's rank among them (the
// number of smaller keys; kNoKey beyond n).  Every key is compared with every other: n^2 / 64 compares per lane, no
// scratch, no LDS.
template <int NL>
__device__ __forceinline__ void topk_rank(const u64* pool, int n, int lane, u64 (&key)[NL], int (&rank)[NL]) {
#pragma unroll
  for (int m = 0; m < NL; ++m) {
    const int i = m * 64 + lane;
    key[m] = i < n ? pool[i] : kNoKey;
    rank[m] = 0;
  }
#pragma unroll
  for (int m2 = 0; m2 < NL; ++m2) {
    const int lim = min(64, n - m2 * 64);
    for (int l = 0; l < lim; ++l) {
      const u64 kj = readlane64(key[m2], l);
#pragma unroll
      for (int m = 0; m < NL; ++m) rank[m] += kj < key[m] ? 1 : 0;
    }
  }
}

// One wave: keep the k best of a pool of n > k keys in its first k entries; returns the k-th best key (all lanes)
template <int NL>
__device__ __forceinline__ u64 topk_shrink(u64* pool, int n, int k, int lane) {
  u64 key[NL];
  int rank[NL];
  topk_rank<NL>(pool, n, lane, key, rank);
  u64 kth = kNoKey;
#pragma unroll
  for (int m = 0; m < NL; ++m) {
    if (key[m] != kNoKey && rank[m] < k) pool[rank[m]] = key[m];
    if (key[m] != kNoKey && rank[m] == k - 1) kth = key[m];
  }
  const u64 has = __ballot(kth != kNoKey);
  return has ? readlane64(kth, __ffsll((long long)has) - 1) : kNoKey;
}

// One wave: the final list of a row -- the k best of n keys of `pool` into ids / values (or keys), padded
template <int NL>
__device__ __forceinline__ void topk_emit(const u64* pool, int n, int k, int lane, int32_t* out_id, float* out_loss,
                                          u64* out_key) {
  u64 key[NL];
  int rank[NL];
  topk_rank<NL>(pool, n, lane, key, rank);
#pragma unroll
  for (int m = 0; m < NL; ++m) {
    if (key[m] != kNoKey && rank[m] < k) {
      if (out_key) out_key[rank[m]] = key[m];
      else { out_id[rank[m]] = (int32_t)(unsigned)key[m]; out_loss[rank[m]] = __uint_as_float((unsigned)(key[m] >> 32)); }
    }
  }
  for (int i = min(n, k) + lane; i < k; i += 64) {       // fewer eligible candidates than k
    if (out_key) out_key[i] = kNoKey;
    else { out_id[i] = -1; out_loss[i] = __builtin_inff(); }
  }
}

}  // namespace ge
