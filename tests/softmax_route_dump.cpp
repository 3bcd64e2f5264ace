// softmax_route_dump.cpp -- the launch arithmetic of csrc/ge_softmax_route.h as text, for
// tests/test_softmax_sweep_cases_host.py (host only; no GPU, no HIP).  stdin: one shape per line, `d B K`; stdout, one line:
//   col_blocks ldy maxcb | xres lds_bytes lds_bytes(MASKED) | tiles(B) tiles(K) live_words(K) |
//   ns = split(B, K), tiles_per_range of K in ns ranges | nq = split(K, B), tiles_per_range of B in nq ranges | gc_rows(B, K)
// (without the bars).
#include <stdio.h>

#include "ge_softmax_route.h"

int main() {
  int d;
  long long B, K;
  while (scanf("%d %lld %lld", &d, &B, &K) == 3) {
    const int ns = ge::sm_split(B, K), nq = ge::sm_split(K, B);
    const ge::SmPlan pk = ge::sm_plan(K, ns, d, false), pm = ge::sm_plan(K, ns, d, true), pb = ge::sm_plan(B, nq, d, false);
    printf("%d %d %d %d %zu %zu %lld %lld %lld %d %d %d %d %zu\n", ge::sm_col_blocks(d), ge::sm_ldy(d), ge::sm_maxcb(d), pk.xres,
           pk.lds_bytes, pm.lds_bytes, (long long)ge::sm_tiles(B), (long long)ge::sm_tiles(K), (long long)ge::sm_live_words(K), ns,
           pk.tiles_per_range, nq, pb.tiles_per_range, ge::sm_gc_rows(B, K));
  }
  return 0;
}
