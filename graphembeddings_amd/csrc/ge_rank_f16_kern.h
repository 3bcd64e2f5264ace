// ge_rank_f16_kern.h -- the kernel template of the split-precision sweep (ge_rank_f16.hip: why it has this shape) and
// the host side of its two sweeps, one body each for the plain and the candidate-set form (f16_sweep_run,
// topk_sweep_run): LDS sizes, the top-k arguments and merge, the planes helper.  Included by ge_rank_f16.hip (the
// unmasked instantiations) and ge_rank_f16_masked.hip (the MASKED ones: per-row candidate sets), so that the two sets of
// instantiations compile side by side.
#pragma once
#include <algorithm>
#include <type_traits>

#include "ge_f16_dev.h"
#include "ge_launch.h"
#include "ge_topk_dev.h"

namespace ge {
namespace {

// (kBlk, the planes' layout, HLds and the MFMA loop: ge_f16_dev.h)
template <int KKB>
constexpr size_t h_lds_bytes() {
  return sizeof(_Float16) * ((size_t)2 * kRB * HCfg<KKB>::kSA) + sizeof(float) * 2 * kRB + sizeof(float2) * kRB +
         sizeof(unsigned) * 8 * 64 + sizeof(int) * (4 * kRB + 4);
}

// ---- top-k (MODE 3, ge_topk_1vK): keys, pools, thresholds (keys, rank / cut / emit: ge_topk_dev.h; kTopkMaxK and the
// workspace: ge_sweep_route.h)
// Losses are sigmoids in [0, 1] (never NaN for a candidate that survives), so the integer order of topk_key's keys is the
// reference heap's pop order (ascending loss, ties by id).

// per row of the block behind HLds: the current k-th best key, the pool's fill and the raw-score bound of that key
template <int KKB>
constexpr size_t topk_lds_bytes() { return h_lds_bytes<KKB>() + (sizeof(u64) + sizeof(int) + sizeof(float)) * kRB; }

// (the sweep reads k, pool and part only -- n_split is gridDim.y, kp and cap follow from k: every kernel argument it
// keeps live costs scalar registers the staging then spills)
struct TopkArgs {
  int k;              // 1 ... kTopkMaxK
  int cap;            // pool entries per (row, split): topk_kp(k) + 128 <= 320 (one tile adds at most 128 to a row)
  int n_split;        // workgroups per row block (gridDim.y), each over its own range of candidate tiles
  u64* pool;          // [B][n_split][cap]
  u64* part;          // [B][n_split][k] partial lists: each segment's k best, sorted, kNoKey-padded
  int32_t* out_id;    // [B][k]
  float* out_loss;    // [B][k]
};

// Per-row candidate sets (ge_rank_1vK_masked, ge_topk_1vK_masked).  The MASKED instantiations take them behind the top-k
// arguments; the unmasked ones take TopkArgs itself -- the kernel arguments, and with them the scalar registers, they
// always had.
struct MaskedTopkArgs : TopkArgs {
  const int32_t* row_set;   // [B] the set of each row; -1: unrestricted, anything else outside [0, n_sets): a bad row
  const uint32_t* mask;     // [n_sets][4 n_ct] bit c & 31 of word c >> 5: the candidate at position c is admissible
  int n_sets;
};
template <bool MASKED>
using SweepTk = std::conditional_t<MASKED, MaskedTopkArgs, TopkArgs>;
constexpr size_t kMaskLdsBytes = sizeof(int) * kRB;            // MASKED: the row block's set indices, behind everything else

constexpr int kTopkLane = 5;            // pool entries per lane in a merge: cap = kp + 128 <= 320

// the raw-score bound of a k-th best loss e: a candidate whose raw score lies above it has a loss > e (the bracket of
// rank_f16_kernel's vs-loss mode, one-sided; infinite near saturation)
__device__ __forceinline__ float topk_bound(float e) {
  const float sa = 1.0f / (kQScale * kQScale);
  const float ec = fminf(fmaxf(e, 1e-30f), 0.99999994f);
  const float xs = logf(ec / (1.0f - ec));
  const float gs = e * (1.0f - e);
  const float wx = !(gs >= 1e-5f) ? __builtin_inff() : 1e-6f / gs + 4e-7f * fabsf(xs);
  return xs / sa + wx / sa;
}

// v_writelane_b32 with a constant lane: lane `LANE` of m = the wave-uniform v (v must not come straight out of a
// VALU compare: see bracket_item)
template <int LANE>
__device__ __forceinline__ void set_lane(int& m, unsigned v) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(m) : "s"(v), "n"(LANE));
}

// One score of the bracket epilogue, as ONE instruction sequence (the compiler's hazard recognizer does not look
// inside inline asm: on gfx950 a VALU read of an SGPR that a VALU wrote needs two instructions in between, which the
// order below provides -- the v_writelane read vcc two instructions after the compare that wrote it):
//   inside = (x <= hi) & ~(x < lo) shifted into the per-lane bitmap I; the wave mask of x < lo into lanes R32 / R32 + 4 of M
template <int R32>
__device__ __forceinline__ void bracket_item(float x, float2 br, int& M, unsigned& I) {
  unsigned long long tmp;
  asm("v_cmp_le_f32_e64 %2, %3, %5\n\t"
      "v_cmp_lt_f32_e32 vcc, %3, %4\n\t"
      "s_andn2_b64 %2, %2, vcc\n\t"
      "v_addc_co_u32_e64 %1, %2, %1, %1, %2\n\t"
      "v_writelane_b32 %0, vcc_lo, %6\n\t"
      "v_writelane_b32 %0, vcc_hi, %7"
      : "+v"(M), "+v"(I), "=&s"(tmp)
      : "v"(x), "v"(br.x), "v"(br.y), "n"(R32), "n"(R32 + 4)
      : "vcc");
}

// MODE 0: ranks.  1: ranks, every loss computed exactly and stored too (tests).  2: no ranking at all -- the sweep
// writes scores_out[B,K] (raw score, or its sigmoid when `sweep_flags` & 1): ge_complex_score_1vK on this pipeline.
// 3: top-k (ge_topk_1vK, `tk`): the k first pops of the reference's heap per row, from the losses MODE 1 stores.
// MASKED (MODE 0, 1, 3): row i counts / returns only the candidates whose bit is set in row tk.row_set[i] of tk.mask.  The
// losses are untouched: the mask is ANDed into the "pops before" bitmap (ranks) or ORed, inverted, into the bitmap of
// known cells (top-k).  Everything it adds sits behind `if constexpr (MASKED)`.
template <int KKB, int MODE, bool MASKED = false>
__global__ __launch_bounds__(kBlk) void rank_f16_kernel(
    const float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ hr, int64_t B,
    const int32_t* __restrict__ true_id, const int32_t* __restrict__ cand, int64_t K, float max_norm,
    int cand_is_head, const int32_t* __restrict__ known_off, const uint16_t* __restrict__ known_rc,
    int32_t* __restrict__ raw_cnt, int32_t* __restrict__ skip_cnt, float* true_loss,
    float* __restrict__ scores_out, int n_ct, int64_t n_tiles, int spec, int sweep_flags,
    const int32_t* __restrict__ pos_of, const _Float16* __restrict__ planes, SweepTk<MASKED> tk) {
  static_assert(!MASKED || MODE != 2, "the score sweep takes no candidate sets");
  constexpr bool SCORES = MODE == 1;
  constexpr int kSA = HCfg<KKB>::kSA;
  constexpr int64_t kSliceHalves = (int64_t)KKB * 2 * kOpHalves;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 2, wn = w & 3;
  const int li = lane & 31, lh = lane >> 5;
  const int qt = t & 3;
  const int n_sl = 4 * n_ct;                                     // slices in `planes` (rows behind K: NaN)
  HLds lds;
  lds.Ah = reinterpret_cast<_Float16*>(smem);
  lds.Am = lds.Ah + kRB * kSA;
  lds.sA = reinterpret_cast<float*>(lds.Am + kRB * kSA);
  lds.eT = lds.sA + kRB;
  lds.lohi = reinterpret_cast<float2*>(lds.eT + kRB);             // an even number of floats in: 8-byte aligned
  lds.bm = reinterpret_cast<unsigned*>(lds.lohi + kRB) + w * 64;
  lds.skip = reinterpret_cast<int*>(reinterpret_cast<unsigned*>(lds.lohi + kRB) + 8 * 64);
  lds.extra = lds.skip + kRB;
  lds.tI = lds.extra + kRB;
  lds.tP = lds.tI + kRB;
  lds.next = lds.tP + kRB;
  // MODE 3 only: behind HLds (topk_lds_bytes)
  u64* tk_kth = reinterpret_cast<u64*>(lds.next + 4);           // (HLds ends on a multiple of 8 bytes)
  int* tk_cnt = reinterpret_cast<int*>(tk_kth + kRB);
  float* tk_hi = reinterpret_cast<float*>(tk_cnt + kRB);
  // MASKED only: behind all of the above
  [[maybe_unused]] int* const mset = MODE == 3 ? reinterpret_cast<int*>(tk_hi + kRB) : lds.next + 4;
  const int k = d >> 1;

  // This workgroup's share of the (row block, 128-candidate tile) list, row-block major -- walked so that every
  // workgroup of the chip starts at candidate tile 0 and sweeps upwards at the same pace: the share's FIRST row block
  // (entered at some tile ct_a > 0) is taken last.  The CUs of an XCD then read the same tiles of `planes` within a
  // few tiles of each other and the XCD's 4 MiB L2 serves all but the first of them; walked in list order the 32 CUs
  // sat at 32 different places of the candidate ring, the planes (13 MB) streamed through every L2 and 80 % of the
  // reads missed it (TCC_HIT / TCC_MISS: 20 % -> 93 % hits).
  // (MODE 3: workgroup = (row block, candidate range): n_split equal ranges of the row block's tiles, one each)
  const int tk_s = MODE == 3 ? (int)blockIdx.y : 0;
  const int64_t tk_rb = MODE == 3 ? (int64_t)blockIdx.x : 0;
  const int tk_ns = MODE == 3 ? (int)gridDim.y : 1;            // (MODE 3: n_split, kp and cap from the grid and k)
  const int tk_kp = topk_kp(tk.k), tk_cap = tk_kp + 128;
  const int64_t share0 = MODE == 3 ? tk_rb * n_ct + (int64_t)n_ct * tk_s / tk_ns : n_tiles * blockIdx.x / gridDim.x;
  const int64_t share1 = MODE == 3 ? tk_rb * n_ct + (int64_t)n_ct * (tk_s + 1) / tk_ns
                                   : n_tiles * (blockIdx.x + 1) / gridDim.x;
  const int64_t first_end = min(share1, (share0 / n_ct + 1) * n_ct);
  for (int pass = 0; pass < 2; ++pass) {
  int64_t idx = pass ? share0 : first_end;
  const int64_t idx_end = pass ? first_end : share1;
  while (idx < idx_end) {
    const int rb = (int)(idx / n_ct);
    const int ct0 = (int)(idx - (int64_t)rb * n_ct);
    const int ct1 = (int)min((int64_t)n_ct, ct0 + (idx_end - idx));
    const int64_t m0 = (int64_t)rb * kRB;
    idx += ct1 - ct0;
    __syncthreads();                                             // the previous row block's LDS is done with

    // ---- Q = fixed o relation for the block's 128 rows (four threads a row), scaled by the rows' clip scales and
    // 2^8, split into two fp16 planes
    {
      const int qrow = t >> 2;
      const int64_t r = m0 + qrow;
      int32_t fid = -1, rid = -1;
      if (r < B) { fid = hr[2 * r]; rid = hr[2 * r + 1]; }
      bool bad = fid < 0 || fid >= N || rid < 0 || rid >= N;
      [[maybe_unused]] int32_t sid = -1;
      if constexpr (MASKED) {
        if (r < B) sid = tk.row_set[r];
        bad = bad || sid < -1 || sid >= tk.n_sets;
      }
      const float* frow = table + (int64_t)(bad ? 0 : fid) * d;
      const float* rrow = table + (int64_t)(bad ? 0 : rid) * d;
      // Two compact loops (not unrolled: straight-line code that runs once per row block is fetched cold -- about 300
      // cycles per 64 bytes of instructions, measured on the unrolled form of this staging and on a second copy of the
      // MFMA loop), each requesting the next iteration's four float4 before this iteration's arithmetic.
      const int nj = k >> 2;
      auto ld4 = [&](const float* row, int j) -> float4 { return *reinterpret_cast<const float4*>(row + 4 * min(j, nj - 1)); };
      float ssf = 0.f, ssr = 0.f;
      // spectral HolE (ge_complex_dev.h): Hermitian weight 2 on every bin but element 0, which packs the two REAL
      // bins X_0 | X_k; norms and score carry the Parseval factor 1/d
      {
        float4 nfre = ld4(frow, qt), nfim = ld4(frow + k, qt), nrre = ld4(rrow, qt), nrim = ld4(rrow + k, qt);
#pragma unroll 1
        for (int j = qt; j < nj; j += 4) {                       // pass 1: the two clip norms
          const float4 fre = nfre, fim = nfim, rre = nrre, rim = nrim;
          nfre = ld4(frow, j + 4); nfim = ld4(frow + k, j + 4); nrre = ld4(rrow, j + 4); nrim = ld4(rrow + k, j + 4);
          const float w0 = (spec && j != 0) ? 2.f : 1.f, w1 = spec ? 2.f : 1.f;   // element 0 of the row / the others
          ssf += w0 * (fre.x * fre.x + fim.x * fim.x) + w1 * (fre.y * fre.y + fre.z * fre.z + fre.w * fre.w + fim.y * fim.y + fim.z * fim.z + fim.w * fim.w);
          ssr += w0 * (rre.x * rre.x + rim.x * rim.x) + w1 * (rre.y * rre.y + rre.z * rre.z + rre.w * rre.w + rim.y * rim.y + rim.z * rim.z + rim.w * rim.w);
        }
      }
      ssf += __shfl_xor(ssf, 1, kWave); ssf += __shfl_xor(ssf, 2, kWave);
      ssr += __shfl_xor(ssr, 1, kWave); ssr += __shfl_xor(ssr, 2, kWave);
      float i0, i1;
      const float inv_d = spec ? 1.0f / (float)d : 1.0f;
      // The planes hold q * (clip scales) * (1/d for a spectral table) * 2^8.  ComplEx: |q sa| <= 2 max_norm^2.  A spectral
      // row's clip bounds its Parseval-weighted norm, so ONE bin may reach max_norm sqrt(d/2) and a Hermitian-weighted
      // product d max_norm^2: the 1/d of the correlation theorem is folded in BEFORE the split (|q sa / d| <= max_norm^2),
      // which keeps every plane entry below 2^8 * 64 for max_norm <= 8 whatever the table holds.
      const float sa = clip_scale(ssf * inv_d, max_norm, i0) * clip_scale(ssr * inv_d, max_norm, i1) * inv_d * kQScale;
      _Float16* ah = lds.Ah + qrow * kSA;
      _Float16* am = lds.Am + qrow * kSA;
      {
        float4 nfre = ld4(frow, qt), nfim = ld4(frow + k, qt), nrre = ld4(rrow, qt), nrim = ld4(rrow + k, qt);
#pragma unroll 1
        for (int j = qt; j < nj; j += 4) {                       // pass 2: q * sa * 2^8 -> high halves and remainders
          const float4 fre = nfre, fim = nfim, rre = nrre, rim = nrim;
          nfre = ld4(frow, j + 4); nfim = ld4(frow + k, j + 4); nrre = ld4(rrow, j + 4); nrim = ld4(rrow + k, j + 4);
          const float fr[4] = {fre.x, fre.y, fre.z, fre.w}, fi[4] = {fim.x, fim.y, fim.z, fim.w};
          const float rr[4] = {rre.x, rre.y, rre.z, rre.w}, ri[4] = {rim.x, rim.y, rim.z, rim.w};
          float qre[4], qim[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool packed = spec && j == 0 && i == 0;
            if (packed) {          // two independent real dimensions: products of the re slots and of the im slots
              qre[i] = fr[i] * rr[i];
              qim[i] = fi[i] * ri[i];
            } else if (!cand_is_head) {   // q = h * r ; score = Re(q conj t)
              qre[i] = fr[i] * rr[i] - fi[i] * ri[i];
              qim[i] = fr[i] * ri[i] + fi[i] * rr[i];
            } else {               // Re(h r conj t) with h the candidate: Q = [Re(r conj t) | -Im(r conj t)]
              qre[i] = rr[i] * fr[i] + ri[i] * fi[i];
              qim[i] = -(ri[i] * fr[i] - rr[i] * fi[i]);
            }
            if (spec && !packed) { qre[i] *= 2.f; qim[i] *= 2.f; }   // Hermitian weight
          }
          h4 rh, rm, ih, im;
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            h2 a, b;
            h_split(qre[i] * sa, qre[i + 1] * sa, a, b);
            rh[i] = a.x; rh[i + 1] = a.y; rm[i] = b.x; rm[i + 1] = b.y;
            h_split(qim[i] * sa, qim[i + 1] * sa, a, b);
            ih[i] = a.x; ih[i + 1] = a.y; im[i] = b.x; im[i + 1] = b.y;
          }
          *reinterpret_cast<h4*>(ah + 4 * j) = rh; *reinterpret_cast<h4*>(am + 4 * j) = rm;          // (row stride, k: multiples of 4)
          *reinterpret_cast<h4*>(ah + k + 4 * j) = ih; *reinterpret_cast<h4*>(am + k + 4 * j) = im;
        }
      }
      if (qt == 0) {
        for (int c = d; c < 16 * KKB; ++c) { ah[c] = (_Float16)0.f; am[c] = (_Float16)0.f; }       // k padding
        lds.sA[qrow] = (bad || r >= B) ? __builtin_nanf("") : 1.0f / (kQScale * kQScale);
        lds.skip[qrow] = 0;
        lds.extra[qrow] = 0;
        const int32_t tid = (MODE < 2 && r < B) ? true_id[r] : -1;
        lds.tI[qrow] = tid;
        // (sweep_flags & 2, ranking against GIVEN losses: the "true candidate" pass still runs -- the loop below has one
        // copy of the MFMA code -- on candidate 0's planes, and its result is replaced by the given loss)
        lds.tP[qrow] = (sweep_flags & 2) ? (r < B ? 0 : -1) : (tid >= 0 && tid < N) ? pos_of[tid] : -1;
        if constexpr (MASKED) mset[qrow] = bad ? -1 : sid;      // (a bad row sets no bit anyway)
      }
      if constexpr (MODE == 3) {
        tk_kth[qrow] = kNoKey;                                   // (no list yet: every candidate of a good row survives)
        tk_cnt[qrow] = 0;
        tk_hi[qrow] = (bad || r >= B) ? __builtin_nanf("") : __builtin_inff();
      }
      if (t < 4) lds.next[t] = 2;                                // (blocks 0 and 1 of a slice go to its two waves up front)
    }
    __syncthreads();

    // this wave's slices of `planes`: 32 candidates each, slice 4 ct + wn of the share's 128-candidate tiles
    auto slice_src = [&](int s) -> unsigned {                     // byte offset of this lane's 16 bytes of slice s's k block 0 (clamped)
      return (unsigned)min(s, n_sl - 1) * (unsigned)(kSliceHalves * 2) + (unsigned)(li * 32 + lh * 16);
    };
    auto known_of = [&](int ct, int32_t& k0, int32_t& k1) {
      k0 = k1 = 0;
      if (known_off && ct < ct1) {
        const int64_t tile = (int64_t)rb * n_ct + ct;
        k0 = known_off[tile]; k1 = known_off[tile + 1];
      }
    };
    f32x16 acc[2];
    HB Bq[kAhead + 1];
    // The sweep's blocks of candidate slice wn -- (tile, row half) = (ct0 + (i >> 1), i & 1), i < 2 (ct1 - ct0) -- are handed
    // out from a counter to the two waves that own the slice (w = wn and wn + 4: the two waves of one SIMD).  With a fixed
    // row half each, the older wave of the SIMD won every issue arbitration, finished 14 tiles early and waited 11 % of
    // the kernel at the closing barrier while its partner ran alone, MFMA loop and epilogue back to back (measured;
    // alternating s_setprio did not change it).  A wave holds two blocks: the one it computes and the one it prefetches
    // (the first is block wm, so a row block with a single tile still keeps both waves busy).
    const int n_items = 2 * (ct1 - ct0);
    auto take = [&]() -> int {
      int v = 0;
      if (lane == 0) v = atomicAdd(&lds.next[wn], 1);
      return __builtin_amdgcn_readfirstlane(v);
    };
    // (MODE 3: no counter -- wave (wm, wn) takes row half wm of slice wn of every tile, so it alone appends to and merges
    // nothing but its own cells, and all waves pass the same number of barriers)
    int item = wm, item_next = MODE == 3 ? wm + 2 : take();
    const int s0 = 4 * (ct0 + (item >> 1)) + wn;
    // ---- the first pass of the loop below (ranks): the true candidates -- a tile whose candidate rows are the block's 128
    // true entities (this wave: 32 of them, gathered by position), through the SAME copy of the MFMA loop as the sweep's
    // blocks (a second copy, fetched cold once per row block, took six tiles' time)
    bool diag = MODE < 2;
    unsigned cur = slice_src(s0);
    if constexpr (MODE < 2) {
      const int pos = lds.tP[wn * 32 + li];
      const int pc = pos < 0 ? 0 : pos;
      cur = (unsigned)(pc >> 5) * (unsigned)(kSliceHalves * 2) + (unsigned)((pc & 31) * 32 + lh * 16);
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) h_loadB(Bq[j], planes, cur, j);
    int raw_reg[2][2] = {{0, 0}, {0, 0}};                         // lane r < 32: bits counted for row half*64 + tm*32 + r

    // ---- the sweep: behind the true-candidate pass no barrier until the row block is done
    int32_t kn0 = 0, kn1 = 0, kn0_next, kn1_next;
    known_of(ct0 + (item >> 1), kn0_next, kn1_next);
    while (diag || item < n_items) {
      const int ct = ct0 + (item >> 1), wmi = diag ? wm : (item & 1);
      const int64_t col = (int64_t)(4 * ct + wn) * kSL + li;     // this lane's candidate
      const unsigned nxt = slice_src(4 * (ct0 + ((diag ? item : item_next) >> 1)) + wn);
      if (!diag) {
        // (the next block's known-cell range is requested BEFORE the MFMA loop: it is a scalar load, and the wait in front
        // of the epilogue -- for the brackets -- waits for everything on that counter)
        kn0 = kn0_next; kn1 = kn1_next;
        known_of(ct0 + (item_next >> 1), kn0_next, kn1_next);
      }
      // MASKED: the mask words of this wave's 64 rows for its slice, one per lane (row wmi * 64 + lane), requested before
      // the MFMA loop like the known-cell range above; all ones for an unrestricted row
      [[maybe_unused]] unsigned mw = ~0u;
      if constexpr (MASKED) {
        if (!diag) {
          const int sid = mset[wmi * 64 + lane];
          if (sid >= 0) mw = tk.mask[(int64_t)sid * n_sl + 4 * ct + wn];
        }
      }
      if constexpr (MODE == 3) {
        // (top-k) this wave's known cells of the block -> its own bitmap, before the MFMA loop: nothing of the epilogue
        // is live yet
        if (known_off) {
          lds.bm[lane] = 0u;
          for (int32_t e = kn0 + lane; e < kn1; e += kWave) {
            const unsigned rc = known_rc[e];
            const int rl = rc >> 7, cl = rc & 127;
            if ((rl >> 6) == wmi && (cl >> 5) == wn) atomicOr(&lds.bm[rl & 63], 1u << (cl & 31));
          }
        }
      }
      h_mfma_loop<KKB>(lds, planes, cur, nxt, Bq, acc, wmi, li, lh);     // leaves the next block's leading operands in Bq
      cur = nxt;
      if (diag) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int rl = wm * 64 + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
            if (rl == wn * 32 + li) lds.eT[rl] = acc[tm][q];      // raw score, row scale still to come
          }
        __syncthreads();
        if (t < kRB) {
          // Bracket of the true candidate's raw score.  With g = e (1 - e) the sigmoid's slope at the true score and
          // w = 1e-6 / g <= 0.1, the slope anywhere inside [xs - w, xs + w] is >= g exp(-w) (the sigmoid is concave on one
          // side: a first-order bound alone is not enough), so a candidate whose scaled score lies outside has a loss that
          // differs by >= 0.9e-6, three times what the roundings of x * sA and of the 4-instruction sigmoid
          // (< 1.5e-7 each side) can move: outside the bracket the order of the losses is the order of the raw scores.
          // Near saturation (g < 1e-5, |score| > 11.5) no finite bracket gives that margin: it is infinite there and
          // every candidate of the row takes the exact comparison.  A true entity that is not among the candidates has
          // no rank: NaN bracket, NaN loss, no bit is ever set.
          float xp = lds.tP[t] < 0 ? __builtin_nanf("") : lds.eT[t];
          const float sa = lds.sA[t];
          float xs = xp * sa, e = rank_sigmoid(xs);
          if ((sweep_flags & 2) && lds.tP[t] >= 0) {
            // ranking against a GIVEN loss (ge_rank_1vK_vs_loss: the candidate it belongs to need not be in this list):
            // the bracket is centred on its logit -- rounded, but by orders of magnitude less than the bracket's
            // 1e-6 in loss units -- and the exact comparison inside the bracket is against the given value itself
            e = true_loss[m0 + t];
            const float ec = fminf(fmaxf(e, 1e-30f), 0.99999994f);
            xs = (e == e) ? logf(ec / (1.0f - ec)) : e;
            xp = xs / sa;
          }
          const float gs = e * (1.0f - e);
          const float wx = !(gs >= 1e-5f) ? __builtin_inff() : 1e-6f / gs + 4e-7f * fabsf(xs);
          const float wq = wx / sa;
          lds.lohi[t] = make_float2(xp - wq, xp + wq);
          lds.eT[t] = e;
          if (true_loss && !(sweep_flags & 2) && ct0 == 0 && m0 + t < B) true_loss[m0 + t] = e;
        }
        __syncthreads();
        diag = false;
        continue;
      }
      item = item_next;
      item_next = MODE == 3 ? item + 2 : take();
      // the brackets of this lane's 32 rows, requested together (read score by score -- a wait on the LDS queue in front
      // of every compare sequence -- the epilogue took 200 cycles per score; held in registers across the MFMA loop
      // they are spilled)
      float2 br[2][16];
      if constexpr (MODE == 0) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int q = 0; q < 16; ++q) br[tm][q] = lds.lohi[wmi * 64 + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh];
      }
      // epilogue: C layout of the 32x32 f32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).  A candidate
      // beyond K or with a bad id has NaN planes, a row beyond B a NaN bracket: no bit is set.
      if constexpr (MODE == 3) {
        // Top-k epilogue.  Per row: a pool of candidate keys in global memory (tk.pool), its fill, the k-th best key so
        // far and that key's raw-score bound (LDS).  A score above the bound cannot enter the list (one compare); the
        // few below it take the exact loss of MODE 1 -- rank_sigmoid(acc * 2^-16), bit for bit -- and, when their key beats
        // the k-th best and they are no known-true cell, are appended.  After the tile, pools past kp entries are cut
        // back to their k best and the bound tightens.
        if constexpr (MASKED) {                                  // inadmissible candidates are skipped as known cells are
          unsigned skip = ~mw;
          if (known_off) skip |= lds.bm[lane];
          lds.bm[lane] = skip;
        }
        __syncthreads();                                         // the merges after the previous tile are done
        u64* const pbase = tk.pool + (m0 * tk_ns + tk_s) * (int64_t)tk_cap;   // row rl's pool: pbase + rl * pstride
        const int pstride = tk_ns * tk_cap;
        static_for<0, 2>([&](auto tc) {                          // one 32-row half at a time (registers)
          constexpr int tm = decltype(tc)::value;
          float hv[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) hv[q] = tk_hi[wmi * 64 + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh];
          unsigned I = 0;                                        // bit 15 - q: the score passed the bound
#pragma unroll
          for (int q = 0; q < 16; ++q) I = (I << 1) | (acc[tm][q] <= hv[q] ? 1u : 0u);
          if (I) {
            const int32_t cid = col < K ? cand[col] : -1;        // (beyond K: NaN planes, never below a bound)
            static_for<0, 4>([&](auto gc) {                      // 4 scores per outer test (most groups are empty)
              constexpr int g4 = decltype(gc)::value;
              if (I & (0xf000u >> (4 * g4))) {
                static_for<0, 4>([&](auto kc) {
                  constexpr int q = 4 * g4 + decltype(kc)::value, R32 = (q & 3) + 8 * (q >> 2);
                  if (I & (0x8000u >> q)) {
                    const int rl = wmi * 64 + tm * 32 + R32 + 4 * lh;
                    if ((!MASKED && !known_off) || !((lds.bm[rl & 63] >> li) & 1u)) {
                      const u64 key = topk_key(rank_sigmoid(acc[tm][q] * (1.0f / (kQScale * kQScale))), cid);
                      if (key < tk_kth[rl]) {
                        const int slot = atomicAdd(&tk_cnt[rl], 1);  // < cap: <= kp before the tile, <= 128 cells per tile
                        pbase[rl * pstride + slot] = key;
                      }
                    }
                  }
                });
              }
            });
          }
        });
        __syncthreads();                                         // the tile's appends are in
        for (int j = 0; j < kRB / 8; ++j) {                      // wave w merges rows 16 w ... 16 w + 15
          const int rl = w * (kRB / 8) + j;
          const int n = __builtin_amdgcn_readfirstlane(tk_cnt[rl]);
          if (n > tk_kp) {
            const u64 kth = topk_shrink<kTopkLane>(pbase + rl * pstride, n, tk.k, lane);
            if (lane == 0) {
              tk_cnt[rl] = tk.k;
              tk_kth[rl] = kth;
              tk_hi[rl] = topk_bound(__uint_as_float((unsigned)(kth >> 32)));
            }
          }
        }
        continue;
      }
      if constexpr (MODE == 2) {                                 // scores only: 32 consecutive floats of a row per half-wave
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int rl = wmi * 64 + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
            const int64_t row = m0 + rl;
            float v = acc[tm][q] * lds.sA[rl];
            if (sweep_flags & 1) v = rank_sigmoid(v);            // 4 VALU, within 3e-7 of expf's
            if (row < B && col < K) scores_out[row * K + col] = v;
          }
        continue;
      }
      int32_t c0 = -1;
      if constexpr (SCORES) c0 = col < K ? cand[col] : -1;
      (void)c0;
      // MASKED: lane r < 32 of M holds row tm * 32 + r of the wave's block, whose mask word lane tm * 32 + r loaded
      [[maybe_unused]] const unsigned mw_hi = MASKED ? (unsigned)__shfl((int)mw, (lane + 32) & 63, kWave) : 0u;
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) {
        int M = 0;                                               // lane r: the 32 column bits of row r of the 32 x 32 block
        unsigned* mrow = lds.bm + tm * 32;
        if constexpr (SCORES) {                                  // tests: every loss exactly, and stored
          static_for<0, 16>([&](auto qc) {
            constexpr int q = decltype(qc)::value, R32 = (q & 3) + 8 * (q >> 2);
            const int rl = wmi * 64 + tm * 32 + R32 + 4 * lh;
            const float et = lds.eT[rl];
            const float e0 = rank_sigmoid(acc[tm][q] * lds.sA[rl]);
            const unsigned long long mk = __ballot(e0 < et) | __ballot(e0 == et && c0 < lds.tI[rl]);
            if (m0 + rl < B && col < K) scores_out[(m0 + rl) * K + col] = e0;
            set_lane<R32>(M, (unsigned)mk);                      // (mk comes out of a scalar OR: no VALU -> VALU SGPR hazard)
            set_lane<R32 + 4>(M, (unsigned)(mk >> 32));
          });
          if constexpr (MASKED) M &= (int)(tm ? mw_hi : mw);
          raw_reg[0][tm] += wmi ? 0 : __popc((unsigned)M);
          raw_reg[1][tm] += wmi ? __popc((unsigned)M) : 0;
          if (lane < 32) mrow[lane] = (unsigned)M;
        } else {
          // Per score: "x < lo" (the bit, as a wave mask -> two v_writelane) and "x <= hi"; the scores inside the bracket
          // (le and not lt: one scalar and-not) are shifted into a per-lane bitmap (one v_addc): bracket_item.  Longer
          // scalar chains on compare results (compare / select / or per score) stall the wave: measured.
          unsigned I = 0;                                        // per-lane bitmap of "inside the bracket"
          static_for<0, 16>([&](auto qc) {
            constexpr int q = decltype(qc)::value, R32 = (q & 3) + 8 * (q >> 2);
            bracket_item<R32>(acc[tm][q], br[tm][q], M, I);      // (the planes carry the clip scale)
          });
          if constexpr (MASKED) M &= (int)(tm ? mw_hi : mw);
          raw_reg[0][tm] += wmi ? 0 : __popc((unsigned)M);       // (lanes 32 .. 63 of M stay 0; no dynamic register index)
          raw_reg[1][tm] += wmi ? __popc((unsigned)M) : 0;
          if (lane < 32) mrow[lane] = (unsigned)M;
          if (I) {                                               // lanes owning a score inside a bracket: the exact
            static_for<0, 4>([&](auto gc) {                      // comparison, bit set in LDS; 4 scores per outer test
              constexpr int g4 = decltype(gc)::value;
              if (I & (0xf000u >> (4 * g4))) {
                static_for<0, 4>([&](auto kc) {
                  constexpr int q = 4 * g4 + decltype(kc)::value, R32 = (q & 3) + 8 * (q >> 2);
                  if (I & (0x8000u >> q)) {
                    const int rl = wmi * 64 + tm * 32 + R32 + 4 * lh;
                    // (a score inside a bracket belongs to a row WITH a bracket: its sA is the constant, not NaN -- no LDS read)
                    const float e = rank_sigmoid(acc[tm][q] * (1.0f / (kQScale * kQScale))), et = lds.eT[rl];
                    bool before = e < et;
                    if (e == et) before = (col < K ? cand[col] : -1) < lds.tI[rl];   // equal losses pop in id order
                    if constexpr (MASKED) {                      // the candidate's own bit (the word another lane holds)
                      const int sid = mset[rl];
                      if (before && sid >= 0) before = (tk.mask[(int64_t)sid * n_sl + 4 * ct + wn] >> li) & 1u;
                    }
                    if (before) { atomicOr(mrow + R32 + 4 * lh, 1u << li); atomicAdd(&lds.extra[rl], 1); }
                  }
                });
              }
            });
          }
        }
      }
      // this wave's bitmap is complete (its own LDS writes, in order): known cells of its 64 x 32 block that rank before
      // the target are tallied (every wave scans the tile's few cells and keeps its own)
      if (known_off) {
        for (int32_t e = kn0 + lane; e < kn1; e += kWave) {
          const unsigned rc = known_rc[e];
          const int rl = rc >> 7, cl = rc & 127;
          if ((rl >> 6) == wmi && (cl >> 5) == wn && ((lds.bm[rl & 63] >> (cl & 31)) & 1u)) atomicAdd(&lds.skip[rl], 1);
        }
      }
    }
    __syncthreads();
    if constexpr (MODE == 3) {
      // the segment's list of each row, sorted and kNoKey-padded, for topk_merge_kernel
      for (int j = 0; j < kRB / 8; ++j) {
        const int rl = w * (kRB / 8) + j;
        const int64_t row = m0 + rl;
        if (row >= B) break;
        const int n = __builtin_amdgcn_readfirstlane(tk_cnt[rl]);
        // (rows with an id out of range have an empty pool; topk_merge_kernel gives them -1 / NaN)
        topk_emit<kTopkLane>(tk.pool + (row * tk_ns + tk_s) * (int64_t)tk_cap, n, tk.k, lane, nullptr, nullptr,
                  tk.part + (row * tk_ns + tk_s) * (int64_t)tk.k);
      }
    }
    if constexpr (MODE < 2) {
      if (lane < 32) {
#pragma unroll
        for (int hm = 0; hm < 2; ++hm)
#pragma unroll
          for (int tm = 0; tm < 2; ++tm) {
            const int64_t row = m0 + hm * 64 + tm * 32 + lane;
            if (row < B && raw_reg[hm][tm]) atomicAdd(&raw_cnt[row], raw_reg[hm][tm]);
          }
      }
      if (t < kRB && m0 + t < B) {
        if (lds.extra[t]) atomicAdd(&raw_cnt[m0 + t], lds.extra[t]);
        if (lds.skip[t]) atomicAdd(&skip_cnt[m0 + t], lds.skip[t]);
      }
    }
  }
  }
}

// (two plain kernels, defined here in this order: they are emitted in front of every template instantiation, and the code
// object of ge_rank_f16.hip keeps the layout it had when the sweep kernel lived in that file)
// pos_of[entity] = its position in `cand` (-1, from the memset before: none)
__global__ void rank_pos_kernel(const int32_t* __restrict__ cand, int64_t K, int64_t N, int32_t* __restrict__ pos_of) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K) {
    const int32_t id = cand[i];
    if (id >= 0 && id < N) pos_of[id] = (int32_t)i;
  }
}

// The second step of a top-k: per row (one wave), the n_split partial lists -- each sorted, kNoKey-padded -- into the
// final k ids and losses (one list: a copy).  Only keys below the running k-th best are taken (a prefix of each list);
// the row's first pool collects them and is cut back to k whenever the next list might not fit.
__global__ __launch_bounds__(256) void topk_merge_kernel(const int32_t* __restrict__ hr, int64_t B, int64_t N, TopkArgs tk) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int k = tk.k;
  int32_t* oid = tk.out_id + row * k;
  float* ol = tk.out_loss + row * k;
  const int32_t fid = hr[2 * row], rid = hr[2 * row + 1];
  if (fid < 0 || fid >= N || rid < 0 || rid >= N) {
    for (int i = lane; i < k; i += 64) { oid[i] = -1; ol[i] = __builtin_nanf(""); }
    return;
  }
  if (tk.n_split == 1) {
    const u64* L = tk.part + row * (int64_t)k;
    for (int i = lane; i < k; i += 64) {
      const u64 key = L[i];
      oid[i] = key == kNoKey ? -1 : (int32_t)(unsigned)key;
      ol[i] = key == kNoKey ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
    }
    return;
  }
  u64* pool = tk.pool + row * tk.n_split * (int64_t)tk.cap;
  int n = 0;
  u64 kth = kNoKey;
  for (int s = 0; s < tk.n_split; ++s) {
    const u64* L = tk.part + (row * tk.n_split + s) * (int64_t)k;
    const u64 a = lane < k ? L[lane] : kNoKey, b = lane + 64 < k ? L[lane + 64] : kNoKey;
    const int ns = __popcll(__ballot(a < kth)) + __popcll(__ballot(b < kth));
    if (ns == 0) continue;
    if (n + ns > tk.cap) {                                   // (after the cut n = k, and k + ns <= 2 k <= cap)
      kth = topk_shrink<kTopkLane>(pool, n, k, lane);
      n = k;
      __threadfence_block();
    }
    if (lane < ns) pool[n + lane] = a;
    if (lane + 64 < ns) pool[n + 64 + lane] = b;
    n += ns;
    __threadfence_block();
  }
  topk_emit<kTopkLane>(pool, n, k, lane, oid, ol, nullptr);
}

// run(planes_ws) on the caller's planes, or -- planes_ws NULL -- on planes built here in a stream-ordered allocation that
// is freed on every path (one more pass over the K candidate rows)
template <class Run>
int with_planes(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, float max_norm, int spec,
                const void* planes_ws, hipStream_t st, Run run) {
  void* own = nullptr;
  if (!planes_ws) {
    hipError_t e = hipMallocAsync(&own, (size_t)rank_planes_bytes(N, d, K), st);
    if (e != hipSuccess) return (int)e;
    const int rc = rank_planes_launch(table, N, d, cand, K, max_norm, spec, own, st);
    if (rc != 0) { (void)hipFreeAsync(own, st); return rc; }
    planes_ws = own;
  }
  int rc = run(planes_ws);
  if (own) {
    const hipError_t e = hipFreeAsync(own, st);
    if (rc == 0 && e != hipSuccess) rc = (int)e;
  }
  return rc;
}

// ---- the host side of both sweeps, plain (MASKED false: ge_rank_f16.hip, sets null) and with candidate sets (true:
// ge_rank_f16_masked.hip).  Each unit instantiates its own form alone.
template <bool MASKED>
constexpr size_t kSetsLds = MASKED ? kMaskLdsBytes : 0;

template <bool MASKED>
SweepTk<MASKED> sweep_tk(const TopkArgs& tk, const SetArgs* sets) {
  SweepTk<MASKED> m;
  static_cast<TopkArgs&>(m) = tk;
  if constexpr (MASKED) {
    m.row_set = sets->row_set;
    m.mask = sets->mask;
    m.n_sets = sets->n_sets;
  }
  return m;
}

struct PlanesWs { const int32_t* pos_of; const _Float16* planes; };
inline PlanesWs planes_at(const void* planes_ws, int64_t N) {
  return {reinterpret_cast<const int32_t*>(planes_ws),
          reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(planes_ws) + pos_bytes(N))};
}

template <bool MASKED, int KKB>
int f16_launch_kkb(const SweepArgs& a, const SetArgs* sets, const void* planes_ws, hipStream_t st) {
  const int64_t n_rb = (a.B + kRB - 1) / kRB, n_ct = (a.K + kRB - 1) / kRB;
  assert(n_ct <= INT32_MAX / 8 && n_rb <= INT32_MAX / 8);        // route_main_road, f16_only_status
  const int64_t n_tiles = n_rb * n_ct;
  const int64_t grid = std::min<int64_t>(n_tiles, GE_PIPE_GRID_M * (int64_t)cu_count());
  const PlanesWs p = planes_at(planes_ws, a.N);
  const SweepTk<MASKED> tk = sweep_tk<MASKED>(TopkArgs{}, sets);
  auto go = [&](auto kern) -> int {
    if (int rc = lds_opt_in(kern)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlk), h_lds_bytes<KKB>() + kSetsLds<MASKED>, st, a.table, a.N, a.d,
                       a.hr, a.B, a.true_id, a.cand, a.K, a.max_norm, a.cand_is_head, a.known_off, a.known_rc, a.raw_cnt,
                       a.skip_cnt, a.true_loss, a.scores_out, (int)n_ct, n_tiles, a.spec, a.sweep_flags, p.pos_of, p.planes,
                       tk);
    return launch_status();
  };
  if constexpr (!MASKED) {                                       // (the score sweep takes no candidate sets)
    if (a.scores_only) return go(rank_f16_kernel<KKB, 2, MASKED>);
  }
  if (a.scores_out) return go(rank_f16_kernel<KKB, 1, MASKED>);
  return go(rank_f16_kernel<KKB, 0, MASKED>);
}

// The rank (or score) sweep.  planes_ws: the candidates' planes from rank_planes_launch for the same (table, cand,
// max_norm, spec), or NULL.
template <bool MASKED>
int f16_sweep_run(const SweepArgs& a, const SetArgs* sets, const void* planes_ws, hipStream_t st) {
  static_assert(h_lds_bytes<18>() + kSetsLds<MASKED> <= kLdsMax, "LDS of the largest instantiation");
  return with_planes(a.table, a.N, a.d, a.cand, a.K, a.max_norm, a.spec, planes_ws, st, [&](const void* ws) -> int {
#define GE_CALL(KKB) return f16_launch_kkb<MASKED, KKB>(a, sets, ws, st)
    GE_KKB_SWITCH(a.d, GE_CALL)
#undef GE_CALL
  });
}

// after topk_merge_kernel in a MASKED top-k: ge_rank_f16_masked.hip
__global__ void topk_bad_set_rows_kernel(const int32_t* __restrict__ row_set, int64_t B, int32_t n_sets, int k,
                                         int32_t* __restrict__ out_id, float* __restrict__ out_loss);

// The top-k sweep (rank_f16_kernel MODE 3, grid row blocks x candidate ranges), then the merge of the partial lists.
// The same planes and Q staging as the rank sweep, so the losses are MODE 1's.  Behind route_topk; the workspace and the
// grid are checked here, in this order.
template <bool MASKED>
int topk_sweep_run(const SweepArgs& a, const TopkOut& t, const SetArgs* sets, const void* planes_ws, hipStream_t st) {
  if (!t.workspace || reinterpret_cast<uintptr_t>(t.workspace) % 256 != 0) return GE_EINVAL;
  if (t.workspace_bytes < topk_ws_bytes(a.B, a.K, t.k)) return GE_ENOMEM;
  if (!topk_grid_ok(a.B, a.K)) return GE_ENOTSUP;
  static_assert(topk_lds_bytes<18>() + kSetsLds<MASKED> <= kLdsMax, "LDS of the largest top-k instantiation");
  const int64_t n_rb = (a.B + kRB - 1) / kRB, n_ct = (a.K + kRB - 1) / kRB;   // (n_ct < INT32_MAX / 8: the planes' 2^32 bytes)
  const int64_t ns = topk_splits(a.B, a.K);
  TopkArgs tk;
  tk.k = t.k;
  tk.cap = topk_kp(t.k) + 128;
  tk.n_split = (int)ns;
  tk.pool = reinterpret_cast<u64*>(t.workspace);
  tk.part = tk.pool + a.B * ns * tk.cap;
  tk.out_id = t.out_id;
  tk.out_loss = t.out_loss;
  const SweepTk<MASKED> stk = sweep_tk<MASKED>(tk, sets);
  return with_planes(a.table, a.N, a.d, a.cand, a.K, a.max_norm, a.spec, planes_ws, st, [&](const void* ws) -> int {
    const PlanesWs p = planes_at(ws, a.N);
    auto sweep = [&]() -> int {
#define GE_CALL(KKB)                                                                                                  \
  {                                                                                                                   \
    auto kern = rank_f16_kernel<KKB, 3, MASKED>;                                                                      \
    if (int rc = lds_opt_in(kern)) return rc;                                                                         \
    hipLaunchKernelGGL(kern, dim3((unsigned)n_rb, (unsigned)ns), dim3(kBlk), topk_lds_bytes<KKB>() + kSetsLds<MASKED>, st, \
                       a.table, a.N, a.d, a.hr, a.B, nullptr, a.cand, a.K, a.max_norm, a.cand_is_head, a.known_off,    \
                       a.known_rc, nullptr, nullptr, nullptr, nullptr, (int)n_ct, n_rb * n_ct, a.spec, 0, p.pos_of,    \
                       p.planes, stk);                                                                                \
    return launch_status();                                                                                           \
  }
      GE_KKB_SWITCH(a.d, GE_CALL)
#undef GE_CALL
    };
    const int rc = sweep();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a.hr, a.B, a.N, tk);
    if constexpr (MASKED) {   // a row whose set index is out of range is a bad row
      hipLaunchKernelGGL(topk_bad_set_rows_kernel, dim3((unsigned)((a.B * t.k + 255) / 256)), dim3(256), 0, st, sets->row_set,
                         a.B, sets->n_sets, t.k, t.out_id, t.out_loss);
    }
    return launch_status();
  });
}

}  // namespace
}  // namespace ge
