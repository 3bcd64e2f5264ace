// ge_neighbors.hip -- nearest-neighbour entity search (the k-nearest-neighbour use of the embeddings, README.md:23-29):
// for query rows q of a table and a list of candidate rows c, the first k candidates in ascending (D, row id) by
//     cosine     D = max(0, 1 - cos)
//     euclidean  D = sqrt(max(0, |q|^2 + |c|^2 - 2 |q| |c| cos))
// with cos = u_q . u_c, u_x = x / |x| (0 for a zero row), on the split-precision sweep of ge_rank_f16.hip (ge_f16_dev.h):
//   * a pre-pass writes every candidate's unit row * 2^8 as fp16 high halves and remainders in the planes' layout, zero
//     padded to whole 16-column k blocks (at least four: any embedding_dim 1 ... 288), and its fp32 norm;
//   * the sweep stages the query rows * 1 / |q| * 2^8 in LDS the same way and runs the same MFMA loop: acc = 2^16 cos.
//     The stored mode writes every distance; the top-k mode keeps per row a pool of (D, id) keys (ge_topk_dev.h) in the
//     caller's workspace, its k-th best key and a bound on the pre-clamp value of that key in LDS, cuts full pools back
//     to k after a tile, and a merge kernel joins the candidate ranges' sorted lists.
// Both modes form every distance with nb_pre / nb_finish from the same acc: the top-k lists are the stored distances'
// first k by (D, id), bit for bit.  No scratch, no float atomics, no allocation.
#include <algorithm>

#include "ge_f16_dev.h"
#include "ge_launch.h"
#include "ge_topk_dev.h"

namespace ge {
namespace {

constexpr int kNbMaxK = 128;
constexpr int kNbMaxDim = 288;
constexpr int kNbLane = 5;              // pool entries per lane: cap = topk_kp(k) + 128 <= 320
constexpr float kCosScale = 1.0f / (kQScale * kQScale);   // acc -> cos

inline int nb_kkb(int32_t d) { return std::max(4, (d + 15) / 16); }
inline int64_t nb_norm_bytes(int64_t K) { return ((K + kRB - 1) / kRB * kRB * (int64_t)sizeof(float) + 255) / 256 * 256; }

struct NbArgs {
  int k;              // 1 ... kNbMaxK
  int exclude_self;   // skip the candidate whose row is the query's
  u64* pool;          // [n_rb * kRB][n_split][cap]
  u64* part;          // [n_rb * kRB][n_split][k] each range's k best, sorted, kNoKey-padded
  int32_t* nan_flag;  // [B][n_split] the range met a NaN distance at an eligible candidate
  int32_t* out_id;    // [B][k]
  float* out_dist;    // [B][k]
};

// |x| of a table row, four threads a row (qt = 0 ... 3 sum the columns = qt mod 4): the pre-pass and the query staging
// call this same code, so a row has one norm whether it is a query or a candidate
__device__ __forceinline__ float nb_row_norm(const float* row, int d, int qt) {
  float ss = 0.f;
#pragma unroll 1
  for (int j = qt; j < d; j += 4) ss = __builtin_fmaf(row[j], row[j], ss);
  ss += __shfl_xor(ss, 1, kWave);
  ss += __shfl_xor(ss, 2, kWave);
  return __builtin_sqrtf(ss);
}

// the plane scale of a row of norm n: 2^8 / n, 0 for a zero row (a NaN or infinite row: NaN planes)
__device__ __forceinline__ float nb_scale(float n) { return n == 0.f ? 0.f : kQScale / n; }

// one row's 16 * KKB columns (zero behind d) * sc as high halves / remainders; thread qt writes column pairs 2 qt + 8 i.
// dst(c, hi, mid) stores the pair at column c.
template <int KKB, typename F>
__device__ __forceinline__ void nb_split_row(const float* row, int d, float sc, bool zero, int qt, F&& dst) {
#pragma unroll 1
  for (int c = 2 * qt; c < 16 * KKB; c += 8) {
    const float x0 = (!zero && c < d) ? row[c] * sc : 0.f, x1 = (!zero && c + 1 < d) ? row[c + 1] * sc : 0.f;
    h2 hi, mid;
    h_split(x0, x1, hi, mid);
    dst(c, hi, mid);
  }
}

// The distance of one cell, from c = acc * 2^-16 (NaN for a bad query row of the stored mode): nb_pre is the value
// before the clamp, nb_finish the distance.  Fixed fp32 expressions (no contraction): every mode forms the same bits.
__device__ __forceinline__ float nb_pre(int metric, float c, float nq, float nc) {
#pragma clang fp contract(off)
  return metric == GE_METRIC_COSINE ? 1.0f - c : (nq * nq + nc * nc) - ((2.0f * nq) * nc) * c;
}
__device__ __forceinline__ float nb_finish(int metric, float p) {
  const float z = p > 0.f ? p : (p == p ? 0.f : p);          // max(0, p): never -0, NaN kept
  return metric == GE_METRIC_COSINE ? z : __builtin_sqrtf(z);
}
// A cell whose pre-clamp value lies above the bound of a k-th best distance e has a distance > e.  Cosine: D <= e
// exactly when 1 - c <= e.  Euclidean: sqrt is correctly rounded, so D <= e needs p <= e^2 (1 + 2^-22); the bound
// e^2 (1 + 2^-20), rounded twice, stays above that (and is +inf where e^2 overflows).
__device__ __forceinline__ float nb_bound(int metric, float e) {
#pragma clang fp contract(off)
  return metric == GE_METRIC_COSINE ? e : (e * e) * (1.0f + 0x1p-20f);
}

// ---- the pre-pass: 64 candidates a workgroup, four threads a row.  norms[pos] = |cand row| (0 behind K, NaN for an id
// outside [0, N)); planes as rank_planes_kernel lays them out: planes[((S * KKB + kb) * 2 + plane) * 512 + row * 16 + col]
template <int KKB>
__global__ __launch_bounds__(256) void nb_planes_kernel(const float* __restrict__ table, int64_t N, int d,
                                                        const int32_t* __restrict__ cand, int64_t K,
                                                        float* __restrict__ norms, _Float16* __restrict__ planes) {
  const int srow = threadIdx.x >> 2, qt = threadIdx.x & 3;
  const int64_t pos = (int64_t)blockIdx.x * 64 + srow;
  const int32_t id = pos < K ? cand[pos] : 0;
  const bool bad = id < 0 || id >= N;
  const float* row = table + (int64_t)(bad ? 0 : id) * d;
  const float n = nb_row_norm(row, d, qt);
  const float sc = bad ? __builtin_nanf("") : nb_scale(n);
  if (qt == 0) norms[pos] = pos >= K ? 0.f : bad ? __builtin_nanf("") : n;
  _Float16* dst = planes + (pos >> 5) * (int64_t)KKB * 2 * kOpHalves + (pos & 31) * 16;
  // (a bad id: NaN everywhere, so its distances are NaN; behind K: zeros, never eligible)
  const float* src = bad ? nullptr : row;
#pragma unroll 1
  for (int c = 2 * qt; c < 16 * KKB; c += 8) {
    float x0 = 0.f, x1 = 0.f;
    if (bad && pos < K) x0 = x1 = __builtin_nanf("");
    else if (pos < K) { x0 = c < d ? src[c] * sc : 0.f; x1 = c + 1 < d ? src[c + 1] * sc : 0.f; }
    h2 hi, mid;
    h_split(x0, x1, hi, mid);
    _Float16* p = dst + (c >> 4) * 2 * kOpHalves + (c & 15);
    *reinterpret_cast<h2*>(p) = hi;
    *reinterpret_cast<h2*>(p + kOpHalves) = mid;
  }
}

// per row of the block behind the Q planes: norm, cos scale, id, bound, pool fill, NaN flag, k-th best key
template <int KKB>
constexpr size_t nb_lds_bytes() {
  return sizeof(_Float16) * ((size_t)2 * kRB * HCfg<KKB>::kSA) + (3 * sizeof(float) + 3 * sizeof(int) + sizeof(u64)) * kRB;
}

// The sweep.  Grid (row block, candidate range): workgroup (rb, s) takes query rows rb * 128 ... + 127 against the
// 128-candidate tiles [n_ct s / n_split, n_ct (s + 1) / n_split).  Wave (wm, wn) owns rows wm * 64 ... + 63 and slice
// wn of every tile.  TOPK = false: dist_out[B][K] <- every distance.  TOPK: the range's k best per row into a.part.
template <int KKB, bool TOPK>
__global__ __launch_bounds__(kBlk) void nb_sweep_kernel(const float* __restrict__ table, int64_t N, int d,
                                                        const int32_t* __restrict__ queries, int64_t B,
                                                        const int32_t* __restrict__ cand, int64_t K,
                                                        const float* __restrict__ norms,
                                                        const _Float16* __restrict__ planes, int n_ct, int metric,
                                                        float* __restrict__ dist_out, NbArgs a) {
  constexpr int kSA = HCfg<KKB>::kSA;
  constexpr int64_t kSliceHalves = (int64_t)KKB * 2 * kOpHalves;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), wm = w >> 2, wn = w & 3;
  const int li = lane & 31, lh = lane >> 5, qt = t & 3;
  const int n_sl = 4 * n_ct;
  HLds lds{};
  lds.Ah = reinterpret_cast<_Float16*>(smem);
  lds.Am = lds.Ah + kRB * kSA;
  float* s_qn = reinterpret_cast<float*>(lds.Am + kRB * kSA);    // |q|
  float* s_qs = s_qn + kRB;                                       // 2^-16 (a bad row: NaN; read by the stored mode)
  float* s_thr = s_qs + kRB;                                      // bound of the k-th best distance (-inf: bad row)
  int* s_qid = reinterpret_cast<int*>(s_thr + kRB);               // query id (-1: bad row or beyond B)
  int* s_cnt = s_qid + kRB;                                       // pool fill
  int* s_nan = s_cnt + kRB;                                       // an eligible candidate's distance was NaN
  u64* s_kth = reinterpret_cast<u64*>(s_nan + kRB);               // (8-byte aligned: kSA is even, 6 x 128 words before)

  const int64_t m0 = (int64_t)blockIdx.x * kRB;
  const int s = (int)blockIdx.y, ns = (int)gridDim.y;
  const int ct0 = (int)((int64_t)n_ct * s / ns), ct1 = (int)((int64_t)n_ct * (s + 1) / ns);
  const int cap = topk_kp(a.k) + 128;

  // ---- Q = query row / |q| * 2^8, split into two fp16 planes (four threads a row)
  {
    const int qrow = t >> 2;
    const int64_t r = m0 + qrow;
    const int32_t qid = r < B ? queries[r] : -1;
    const bool bad = qid < 0 || qid >= N;
    const float* row = table + (int64_t)(bad ? 0 : qid) * d;
    const float nq = nb_row_norm(row, d, qt);
    _Float16* ah = lds.Ah + qrow * kSA;
    _Float16* am = lds.Am + qrow * kSA;
    nb_split_row<KKB>(row, d, nb_scale(nq), bad, qt, [&](int c, h2 hi, h2 mid) {
      *reinterpret_cast<h2*>(ah + c) = hi;
      *reinterpret_cast<h2*>(am + c) = mid;
    });
    if (qt == 0) {
      s_qn[qrow] = bad ? 0.f : nq;
      s_qs[qrow] = bad ? __builtin_nanf("") : kCosScale;
      s_qid[qrow] = bad ? -1 : qid;
      s_thr[qrow] = bad ? -__builtin_inff() : __builtin_inff();
      s_cnt[qrow] = 0;
      s_nan[qrow] = 0;
      s_kth[qrow] = kNoKey;
    }
  }
  __syncthreads();

  auto slice_src = [&](int sl) -> unsigned {                      // byte offset of this lane's 16 bytes of slice sl's k block 0
    return (unsigned)min(sl, n_sl - 1) * (unsigned)(kSliceHalves * 2) + (unsigned)(li * 32 + lh * 16);
  };
  const int pstride = ns * cap;
  u64* const pbase = a.pool + (m0 * ns + s) * (int64_t)cap;      // row rl's pool: pbase + rl * pstride
  f32x16 acc[2];
  HB Bq[kAhead + 1];
  unsigned cur = slice_src(4 * ct0 + wn);
#pragma unroll
  for (int j = 0; j < kAhead; ++j) h_loadB(Bq[j], planes, cur, j);
  for (int ct = ct0; ct < ct1; ++ct) {
    const unsigned nxt = slice_src(4 * (ct + 1) + wn);
    h_mfma_loop<KKB>(lds, planes, cur, nxt, Bq, acc, wm, li, lh);  // leaves the next block's leading operands in Bq
    cur = nxt;
    // C layout of the 32x32 f32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int64_t col = (int64_t)(4 * ct + wn) * kSL + li;        // this lane's candidate
    const float nc = norms[col];                                  // (norms cover whole tiles)
    // this lane's rows: rb0 + tm * 32 + (q & 3) + 8 (q >> 2), every per-row array read at rb0 plus a constant
    const int rb0 = wm * 64 + 4 * lh;
    if constexpr (!TOPK) {
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int r = tm * 32 + (q & 3) + 8 * (q >> 2);
          const int64_t row = m0 + rb0 + r;
          const float v = nb_finish(metric, nb_pre(metric, acc[tm][q] * s_qs[rb0 + r], s_qn[rb0 + r], nc));
          if (row < B && col < K) dist_out[row * K + col] = v;
        }
    } else {
      // Per cell one test against the row's bound (NaN passes it); the few cells that pass take the exact distance and,
      // when eligible and their key beats the k-th best, are appended to the row's pool.  After the tile, pools past kp
      // entries are cut back to their k best and the bound tightens.
      __syncthreads();                                            // the cuts after the previous tile are done
      const int32_t cid = col < K ? cand[col] : -1;
      // (c = acc * 2^-16, s_qs of a good row; a bad row has zero Q planes and a bound of -inf, so only a NaN candidate
      // passes, and it is not eligible)
      const float* qn_l = s_qn + rb0;
      const float* thr_l = s_thr + rb0;
      const int* qid_l = s_qid + rb0;
      int* cnt_l = s_cnt + rb0;
      int* nan_l = s_nan + rb0;
      const u64* kth_l = s_kth + rb0;
      u64* pool_l = pbase + rb0 * pstride;
      auto epilogue = [&](auto mc) {                              // the metric as a constant: one lean copy each
        constexpr int M = decltype(mc)::value;
        static_for<0, 2>([&](auto tc) {                           // one 32-row half at a time (registers)
          constexpr int tm = decltype(tc)::value;
          unsigned I = 0;                                         // bit 15 - q: the cell passed the bound
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int r = tm * 32 + (q & 3) + 8 * (q >> 2);
            const float p = nb_pre(M, acc[tm][q] * kCosScale, M ? qn_l[r] : 0.f, nc);
            I = (I << 1) | (p > thr_l[r] ? 0u : 1u);
          }
          if (I && col < K) {
            static_for<0, 4>([&](auto gc) {                       // 4 cells per outer test (most groups are empty)
              constexpr int g4 = decltype(gc)::value;
              if (I & (0xf000u >> (4 * g4))) {
                static_for<0, 4>([&](auto kc) {
                  constexpr int q = 4 * g4 + decltype(kc)::value;
                  if (I & (0x8000u >> q)) {
                    constexpr int r = tm * 32 + (q & 3) + 8 * (q >> 2);
                    const int32_t qid = qid_l[r];
                    if (qid >= 0 && !(a.exclude_self && cid == qid)) {
                      const float D = nb_finish(M, nb_pre(M, acc[tm][q] * kCosScale, M ? qn_l[r] : 0.f, nc));
                      if (D != D) {
                        nan_l[r] = 1;
                      } else {
                        const u64 key = topk_key(D, cid);
                        if (key < kth_l[r]) {
                          const int slot = atomicAdd(&cnt_l[r], 1);  // < cap: <= kp before the tile, <= 128 cells a tile
                          pool_l[r * pstride + slot] = key;
                        }
                      }
                    }
                  }
                });
              }
            });
          }
        });
      };
      if (metric == GE_METRIC_COSINE) epilogue(std::integral_constant<int, GE_METRIC_COSINE>{});
      else epilogue(std::integral_constant<int, GE_METRIC_EUCLIDEAN>{});
      __syncthreads();                                            // the tile's appends are in
      for (int j = 0; j < kRB / 8; ++j) {                         // wave w cuts rows 16 w ... 16 w + 15
        const int rl = w * (kRB / 8) + j;
        const int n = __builtin_amdgcn_readfirstlane(s_cnt[rl]);
        if (n > topk_kp(a.k)) {
          const u64 kth = topk_shrink<kNbLane>(pbase + rl * pstride, n, a.k, lane);
          if (lane == 0) {
            s_cnt[rl] = a.k;
            s_kth[rl] = kth;
            s_thr[rl] = nb_bound(metric, __uint_as_float((unsigned)(kth >> 32)));
          }
        }
      }
    }
  }
  if constexpr (TOPK) {
    __syncthreads();
    // the range's list of each row, sorted and kNoKey-padded, and its NaN flag, for nb_merge_kernel
    for (int j = 0; j < kRB / 8; ++j) {
      const int rl = w * (kRB / 8) + j;
      const int64_t row = m0 + rl;
      if (row >= B) break;
      const int n = __builtin_amdgcn_readfirstlane(s_cnt[rl]);
      topk_emit<kNbLane>(pbase + rl * pstride, n, a.k, lane, nullptr, nullptr, a.part + (row * ns + s) * (int64_t)a.k);
      if (lane == 0) a.nan_flag[row * ns + s] = s_nan[rl];
    }
  }
}

// Per row (one wave): -1 / NaN for a query id outside [0, N) or a NaN distance in any range; otherwise the n_split
// sorted lists into the final k ids and distances.  Only keys below the running k-th best are taken (a prefix of each
// list); the row's first pool collects them and is cut back to k whenever the next list might not fit.
__global__ __launch_bounds__(256) void nb_merge_kernel(const int32_t* __restrict__ queries, int64_t B, int64_t N, int ns,
                                                       NbArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int k = a.k, cap = topk_kp(k) + 128;
  int32_t* oid = a.out_id + row * k;
  float* od = a.out_dist + row * k;
  const int32_t qid = queries[row];
  int bad = qid < 0 || qid >= N;
  for (int s = lane; s < ns; s += 64) bad |= a.nan_flag[row * ns + s];
  if (__ballot(bad != 0)) {
    for (int i = lane; i < k; i += 64) { oid[i] = -1; od[i] = __builtin_nanf(""); }
    return;
  }
  u64* pool = a.pool + row * ns * (int64_t)cap;
  int n = 0;
  u64 kth = kNoKey;
  for (int s = 0; s < ns; ++s) {
    const u64* L = a.part + (row * ns + s) * (int64_t)k;
    const u64 x = lane < k ? L[lane] : kNoKey, y = lane + 64 < k ? L[lane + 64] : kNoKey;
    const int nx = __popcll(__ballot(x < kth)) + __popcll(__ballot(y < kth));
    if (nx == 0) continue;
    if (n + nx > cap) {                                           // (after the cut n = k, and k + nx <= 2 k <= cap)
      kth = topk_shrink<kNbLane>(pool, n, k, lane);
      n = k;
      __threadfence_block();
    }
    if (lane < nx) pool[n + lane] = x;
    if (lane + 64 < nx) pool[n + 64 + lane] = y;
    n += nx;
    __threadfence_block();
  }
  topk_emit<kNbLane>(pool, n, k, lane, oid, od, nullptr);
}

inline bool nb_planes_fit(int64_t K, int32_t d) {                  // (the sweep's 32-bit byte offsets into the planes)
  return planes_slices(K) * nb_kkb(d) * 2 * kOpHalves * (int64_t)sizeof(_Float16) < ((int64_t)1 << 32);
}

template <int KKB, bool TOPK>
int nb_sweep(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B, const int32_t* cand, int64_t K,
             int metric, const void* planes_ws, float* dist_out, const NbArgs& a, int64_t ns, hipStream_t st) {
  static_assert(nb_lds_bytes<18>() <= 160 * 1024, "LDS of the largest instantiation");
  const int64_t n_rb = (B + kRB - 1) / kRB, n_ct = (K + kRB - 1) / kRB;
  const float* norms = reinterpret_cast<const float*>(planes_ws);
  const _Float16* planes = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(planes_ws) + nb_norm_bytes(K));
  auto kern = nb_sweep_kernel<KKB, TOPK>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)n_rb, (unsigned)ns), dim3(kBlk), nb_lds_bytes<KKB>(), st, table, N, d, queries,
                     B, cand, K, norms, planes, (int)n_ct, metric, dist_out, a);
  return launch_status();
}

// Candidate ranges per row block: the largest count that keeps the grid within one workgroup per CU of the MI355X
// (256; one 512-thread workgroup fits a CU).  ceil(256 / n_rb), the ComplEx / HolE top-k's count (topk_splits), leaves
// a second, partly filled round of workgroups: at FB15k all-pairs (117 row blocks) 351 workgroups in two rounds against
// 234 in one.  Never more than topk_splits, so topk_ws_bytes covers the pools and lists.
int64_t nb_splits(int64_t B, int64_t K) {
  const int64_t n_rb = (B + kRB - 1) / kRB, n_ct = (K + kRB - 1) / kRB;
  return std::max<int64_t>(1, std::min<int64_t>(n_ct, 256 / n_rb));
}

// the shared checks of the two sweeps (the C ABI has checked pointers and sizes)
int nb_sweep_ok(int32_t d, int64_t B, int64_t K, int metric, const void* planes_ws) {
  if (metric != GE_METRIC_COSINE && metric != GE_METRIC_EUCLIDEAN) return GE_EINVAL;
  if (d > kNbMaxDim || !nb_planes_fit(K, d)) return GE_ENOTSUP;
  if (!planes_ws || reinterpret_cast<uintptr_t>(planes_ws) % 256 != 0) return GE_EINVAL;
  const int64_t n_rb = (B + kRB - 1) / kRB;
  if (n_rb > INT32_MAX / 8 || (K + kRB - 1) / kRB > INT32_MAX / 8) return GE_ENOTSUP;
  return 0;
}

}  // namespace

int neighbor_max_k() { return kNbMaxK; }
int neighbor_max_dim() { return kNbMaxDim; }

// norms [whole tiles] (256-byte padded) | planes [planes_slices(K)][KKB][2][512] fp16; 0 outside the supported range
int64_t neighbor_planes_bytes(int64_t K, int32_t d) {
  if (K <= 0 || d < 1 || d > kNbMaxDim || !nb_planes_fit(K, d)) return 0;
  return nb_norm_bytes(K) + planes_slices(K) * nb_kkb(d) * 2 * kOpHalves * (int64_t)sizeof(_Float16);
}

int neighbor_planes_launch(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, void* planes_ws,
                           hipStream_t st) {
  if (d > kNbMaxDim || !nb_planes_fit(K, d)) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(planes_ws) % 256 != 0) return GE_EINVAL;
  float* norms = reinterpret_cast<float*>(planes_ws);
  _Float16* planes = reinterpret_cast<_Float16*>(reinterpret_cast<char*>(planes_ws) + nb_norm_bytes(K));
  const int64_t n_blocks = planes_slices(K) / 2;                  // 64 candidates a workgroup: every slice written
  if (n_blocks > INT32_MAX) return GE_ENOTSUP;
#define GE_CALL(KKB)                                                                                                   \
  hipLaunchKernelGGL(nb_planes_kernel<KKB>, dim3((unsigned)n_blocks), dim3(256), 0, st, table, N, d, cand, K, norms,    \
                     planes);                                                                                          \
  return launch_status()
  GE_KKB_SWITCH(16 * nb_kkb(d), GE_CALL)
#undef GE_CALL
}

// Workspace of a top-k over B queries and K candidates: the pools and partial lists within topk_ws_bytes (sized for
// topk_splits >= nb_splits ranges), then the NaN flags, [B][n_split] <= 128 (n_rb + 256) words.  Monotone in B, K, k.
size_t neighbor_ws_bytes(int64_t B, int64_t K, int32_t k) {
  if (B <= 0 || K <= 0 || k < 1 || k > kNbMaxK) return 0;
  const size_t lists = topk_ws_bytes(B, K, k);
  if (lists == 0) return 0;
  const int64_t n_rb = (B + kRB - 1) / kRB;
  return lists + (size_t)(n_rb + 256) * kRB * sizeof(int32_t);
}

int neighbor_dists_launch(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B,
                          const int32_t* cand, int64_t K, int metric, const void* planes_ws, float* out, hipStream_t st) {
  if (int rc = nb_sweep_ok(d, B, K, metric, planes_ws)) return rc;
  if (B == 0) return 0;
  const int64_t ns = nb_splits(B, K);
  NbArgs a{};
  a.k = 1;
#define GE_CALL(KKB) return nb_sweep<KKB, false>(table, N, d, queries, B, cand, K, metric, planes_ws, out, a, ns, st)
  GE_KKB_SWITCH(16 * nb_kkb(d), GE_CALL)
#undef GE_CALL
}

int neighbor_topk_launch(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B,
                         const int32_t* cand, int64_t K, int32_t k, int metric, int exclude_self, const void* planes_ws,
                         int32_t* out_id, float* out_dist, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (k < 1) return GE_EINVAL;
  if (k > kNbMaxK) return GE_ENOTSUP;
  if (int rc = nb_sweep_ok(d, B, K, metric, planes_ws)) return rc;
  if (B == 0) return 0;
  if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < neighbor_ws_bytes(B, K, k)) return GE_ENOMEM;
  const int64_t n_rb = (B + kRB - 1) / kRB, ns = nb_splits(B, K);
  const int64_t rows = n_rb * kRB, cap = topk_kp(k) + 128;
  NbArgs a;
  a.k = k;
  a.exclude_self = exclude_self ? 1 : 0;
  a.pool = reinterpret_cast<u64*>(workspace);
  a.part = a.pool + rows * ns * cap;
  a.nan_flag = reinterpret_cast<int32_t*>(a.part + rows * ns * k);   // (<= topk_ws_bytes - 256 bytes in)
  a.out_id = out_id;
  a.out_dist = out_dist;
  auto run = [&]() -> int {
#define GE_CALL(KKB) return nb_sweep<KKB, true>(table, N, d, queries, B, cand, K, metric, planes_ws, nullptr, a, ns, st)
    GE_KKB_SWITCH(16 * nb_kkb(d), GE_CALL)
#undef GE_CALL
  };
  int rc = run();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(nb_merge_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, queries, B, N, (int)ns, a);
  return launch_status();
}

}  // namespace ge
