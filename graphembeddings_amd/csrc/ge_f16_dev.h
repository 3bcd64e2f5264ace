// ge_f16_dev.h -- what the split-precision sweeps (ge_rank_f16.hip: ranks, scores and top-k of ComplEx / HolE;
// ge_neighbors.hip: nearest-neighbour search) share: the candidate planes' layout, the Q operands in LDS and the MFMA
// loop of one wave's 64 x 32 block.  Included by those two files only; everything but the macro is internal to each.
#pragma once
#include <type_traits>

#include "ge_rank_dev.h"

namespace ge {
namespace {

constexpr int kBlk = 512;               // eight waves: wm = w >> 2 (64 rows), wn = w & 3 (32 candidates of the 128-wide tile)
// (kSL, kOpHalves, planes_slices -- the planes' sizes: ge_sweep_route.h)

template <int I0, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < N) {
    f(std::integral_constant<int, I0>{});
    static_for<I0 + 1, N>(f);
  }
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

template <int KKB>
struct HCfg {
  static constexpr int kKB = KKB;                   // k blocks of 16 (the last zero padded behind embedding_dim)
  static constexpr int kChunks = (KKB + 1) / 2;     // 32-column pieces of a row (the pre-pass's unit)
  static constexpr int kSA = 16 * KKB + 8;          // halves per Q row (+16 bytes: ds_read_b128 of 32 rows hits 32 bank groups)
  static_assert(KKB >= 4 && KKB <= 18, "embedding_dim 56 ... 288 (LDS: the Q planes, 152 KB at 18 k blocks)");
};
constexpr float kQScale = 256.f;        // both operands: |q|, |t * clip| <= max_norm^2 resp. max_norm sqrt(d/2)
constexpr int kAhead = 3;               // k blocks between a candidate operand's request and its first MFMA

struct HLds {
  _Float16* Ah;    // [kRB][kSA] high halves of Q * 2^8 ...
  _Float16* Am;    //   ... and the remainders (Q * 2^8 = Ah + Am to 22 bits)
  float* sA;       // [kRB] 2^-16 (NaN: bad id / beyond B)
  float* eT;       // [kRB] loss of the true candidate
  float2* lohi;    // [kRB] raw-score bracket of the true candidate
  unsigned* bm;    // this wave's [64] rows x 32 `pops before` bits of its current block
  int* skip;       // [kRB] known-true candidates ranked before the target
  int* extra;      // [kRB] candidates inside the bracket that the exact comparison put before the target
  int* tI;         // [kRB] entity id of the true candidate (-1 beyond B)
  int* tP;         // [kRB] its position among the candidates (-1: not a candidate)
  int* next;       // [4] per candidate slice wn: the next (tile, row half) block of the sweep not yet taken by a wave
};

struct HA { h8 ah[2], am[2]; };          // the Q operands of one k block of this wave's 64 rows
struct HB { h8 bh, bm; };                // the candidate operands of one k block of this wave's 32 columns

__device__ __forceinline__ void h_split(float x0, float x1, h2& hi, h2& mid) {
  typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
  const fp16x2 h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
  hi = __builtin_bit_cast(h2, h);
  const fp16x2 m = __builtin_amdgcn_cvt_pkrtz(x0 - (float)hi.x, x1 - (float)hi.y);
  mid = __builtin_bit_cast(h2, m);
}

// the candidate operands of k block kb; off = byte offset in `planes` of this lane's 16 bytes of the slice's k block 0, high
// plane -- a wave-uniform base and a 32-bit lane offset: the loads take the scalar-base form and the stride over the k
// blocks costs one 32-bit add per load, not a 64-bit add with its carry chain
__device__ __forceinline__ void h_loadB(HB& b, const _Float16* __restrict__ planes, unsigned off, int kb) {
  const char* base = reinterpret_cast<const char*>(planes);
  b.bh = *reinterpret_cast<const h8*>(base + (off + (unsigned)(kb * 2 * kOpHalves * 2)));
  b.bm = *reinterpret_cast<const h8*>(base + (off + (unsigned)((kb * 2 + 1) * kOpHalves * 2)));
}

// piece i (0..3) of the Q operands of k block `kb`, in the order the MFMAs of that k block first need them: ah0 ah1 am0 am1
template <int KKB>
__device__ __forceinline__ void h_opsA(HA& o, const HLds& lds, int wm, int li, int lh, int kb, int i) {
  constexpr int kSA = HCfg<KKB>::kSA;
  const int tm = i & 1, mid = i >> 1;
  const _Float16* ap = (mid ? lds.Am : lds.Ah) + (wm * 64 + tm * 32 + li) * kSA + kb * 16 + lh * 8;
  if (mid) o.am[tm] = *reinterpret_cast<const h8*>(ap); else o.ah[tm] = *reinterpret_cast<const h8*>(ap);
}

// The MFMA loop of one 64 x 32 block.  B[0 .. kAhead - 1] hold the candidate operands of k blocks 0 .. kAhead - 1 of the
// slice `cur` on entry and of the slice `nxt` on exit (a ring of kAhead + 1 register sets; a k block's operands are
// requested kAhead k blocks -- 18 MFMAs -- before its first MFMA, across the block boundary too).  No barrier.
template <int KKB>
__device__ __forceinline__ void h_mfma_loop(const HLds& lds, const _Float16* __restrict__ planes, unsigned cur, unsigned nxt,
                                            HB (&B)[kAhead + 1], f32x16 (&acc)[2], int wm, int li, int lh) {
  constexpr int kKB = KKB, kR = kAhead + 1;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[a][q] = 0.f;
  HA ops[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) h_opsA<KKB>(ops[0], lds, wm, li, lh, 0, i);
  static_for<0, kKB>([&](auto kbc) {
    constexpr int kb = decltype(kbc)::value;
    HA& ca = ops[kb & 1];
    HA& na = ops[(kb + 1) & 1];
    HB& cb = B[kb % kR];
    static_for<0, 6>([&](auto pc) {
      constexpr int p = decltype(pc)::value, ty = p >> 1, tm = p & 1;   // consecutive MFMAs hit different accumulators
      const h8 a = ty == 2 ? ca.am[tm] : ca.ah[tm];
      const h8 b = ty == 1 ? cb.bm : cb.bh;
      acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[tm], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (p < 4) {
        if constexpr (kb + 1 < kKB) h_opsA<KKB>(na, lds, wm, li, lh, kb + 1, p);
      } else if constexpr (p == 4) {                              // the ring slot of k block kb - 1 is free: k block kb + kAhead
        constexpr int kn = kb + kAhead;
        if constexpr (kn < kKB) h_loadB(B[kn % kR], planes, cur, kn);
        else h_loadB(B[kn % kR], planes, nxt, kn - kKB);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  });
  // the next block's k blocks 0 .. kAhead - 1 sit in ring slots (kKB + j) % kR: move them to slots j (register renaming
  // at the loop's back edge; a few v_mov at most)
  HB t[kAhead];
#pragma unroll
  for (int j = 0; j < kAhead; ++j) t[j] = B[(kKB + j) % kR];
#pragma unroll
  for (int j = 0; j < kAhead; ++j) B[j] = t[j];
}

}  // namespace
}  // namespace ge

// one instantiation per number of 16-column k blocks (4 ... 18) of a run-time embedding_dim
#define GE_KKB_SWITCH(d, CALL)                                                                        \
  switch (((d) + 15) / 16) {                                                                          \
    case 4: CALL(4); case 5: CALL(5); case 6: CALL(6); case 7: CALL(7); case 8: CALL(8);              \
    case 9: CALL(9); case 10: CALL(10); case 11: CALL(11); case 12: CALL(12); case 13: CALL(13);      \
    case 14: CALL(14); case 15: CALL(15); case 16: CALL(16); case 17: CALL(17); case 18: CALL(18);    \
    default: return GE_ENOTSUP;                                                                       \
  }
