// ge_softmax_route.h -- the launch arithmetic of the softmax objectives' sweeps (ge_softmax_kern.h and its four
// translation units): tile and range counts, which gradient instantiation a width takes, whether the X tile stays in LDS,
// the dynamic-LDS request, the live bitmap's words and the sampled objective's rows of candidate-side partials.  Host
// only, plain C++17, nothing from HIP: tested without a GPU (tests/softmax_route_dump.cpp).
// The coverage map of the widths and shapes the GPU tests run: DESIGN.md section 22.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ge {

constexpr int kSmTile = 64;          // X and Y rows of a tile
constexpr int kSmChunk = 32;         // X columns staged at a time
constexpr int kSmLdx = kSmChunk + 1; // LDS row strides are odd: the 32 rows a half-wave reads fall in 32 banks
constexpr int kSmLdw = kSmTile + 1;
constexpr int kSmMaxSplit = 8;       // Y ranges of a split sweep
constexpr int kSmXresMaxDim = 256;   // up to here X and Y tiles fit whole in LDS together (149 KB with the W tile)
constexpr int kSmMaxColBlocks = 5;   // the largest MAXCB instantiated: 9 column blocks (d <= 288), two waves a block row

static inline int sm_col_blocks(int d) { return (d + 31) / 32; }
static inline int sm_ldy(int d) { return 32 * sm_col_blocks(d) + 1; }
static inline int64_t sm_tiles(int64_t n) { return (n + kSmTile - 1) / kSmTile; }
// Y ranges of a sweep of NX fixed rows against NY: enough workgroups for the device at a small NX, never more than
// kSmMaxSplit or than Y tiles
static inline int sm_split(int64_t NX, int64_t NY) {
  const int64_t tx = sm_tiles(NX), ty = sm_tiles(NY);
  int64_t s = 512 / tx;
  if (s < 1) s = 1;
  if (s > kSmMaxSplit) s = kSmMaxSplit;
  if (s > ty) s = ty;
  return (int)s;
}

// words per query tile of the live bitmap: even, so that a wave's 64-bit ballot is two whole words
static inline int64_t sm_live_words(int64_t K) { return 2 * ((sm_tiles(K) + 63) / 64); }

// rows of dL/dC' partials of the sampled objective: split * K for every split softmax_sampled_launch can choose
// (sm_split(K, B) is at most min(8, tiles(B)) and at most max(1, 512 / tiles(K))), in a form that never shrinks as B or K
// grow
static inline size_t sm_gc_rows(int64_t B, int64_t K) {
  const int64_t tb = sm_tiles(B), tk = sm_tiles(K);
  const int64_t by_b = (tb < kSmMaxSplit ? tb : kSmMaxSplit) * K;
  const int64_t by_k = (int64_t)kSmTile * (tk > 512 ? tk : 512);
  return (size_t)(by_b < by_k ? by_b : by_k);
}

// MAXCB of a gradient sweep: the 32-column blocks of G one wave owns, half the width's blocks rounded up
static inline int sm_maxcb(int d) {
  const int n = (sm_col_blocks(d) + 1) / 2;
  return n < kSmMaxColBlocks ? n : kSmMaxColBlocks;
}

// What sm_sweep launches with: the Y tiles of a range (grid.y = n_ranges), whether the X tile is resident, the dynamic LDS
struct SmPlan { int tiles_per_range; int xres; size_t lds_bytes; };
static inline SmPlan sm_plan(int64_t NY, int n_ranges, int d, bool masked) {
  const int64_t ty = sm_tiles(NY);
  const int tpr = (int)((ty + n_ranges - 1) / n_ranges);
  const int xres = d <= kSmXresMaxDim;
  const size_t lds = sizeof(float) * ((size_t)kSmTile * sm_ldy(d) + kSmTile * (xres ? sm_ldy(d) : kSmLdx) + kSmTile * kSmLdw +
                                      4 * kSmTile + (masked ? 3 * kSmTile : 0));
  return SmPlan{tpr, xres, lds};
}

}  // namespace ge
