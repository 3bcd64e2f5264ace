// sweep_route_dump.cpp -- the routes of csrc/ge_sweep_route.h as text, for tests/test_sweep_route_host.py (host only; no
// GPU, no HIP).  stdin: one shape per line, `entry N d B K max_norm table_addr_mod_16 k` with entry one of rank, score,
// topk, masked_rank, masked_topk (k is read by the top-k entries alone); stdout: `kernel status`.  Entry ws, same line:
// `topk_splits(B, K) topk_ws_bytes(B, K, k) topk_grid_ok(B, K)`.
#include <stdio.h>
#include <string.h>

#include "ge_sweep_route.h"

int main() {
  char entry[16];
  long long N, B, K;
  int d, mod16, k;
  float max_norm;
  while (scanf("%15s %lld %d %lld %lld %f %d %d", entry, &N, &d, &B, &K, &max_norm, &mod16, &k) == 8) {
    if (strcmp(entry, "ws") == 0) {
      printf("%lld %zu %d\n", (long long)ge::topk_splits(B, K), ge::topk_ws_bytes(B, K, k), (int)ge::topk_grid_ok(B, K));
      continue;
    }
    const ge::SweepRoute r = strcmp(entry, "rank") == 0          ? ge::route_rank(N, d, B, K, max_norm, mod16)
                             : strcmp(entry, "score") == 0       ? ge::route_score(N, d, B, K, max_norm, mod16)
                             : strcmp(entry, "masked_rank") == 0 ? ge::route_masked_rank(N, d, B, K, max_norm, mod16)
                                 : ge::route_topk(N, d, B, K, max_norm, mod16, k, strcmp(entry, "masked_topk") == 0);
    printf("%d %d\n", r.kernel, r.status);
  }
  return 0;
}
