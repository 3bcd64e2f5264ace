// sweep_route_dump.cpp -- the routes of csrc/ge_sweep_route.h as text, for tests/test_sweep_route_host.py (host only; no
// GPU, no HIP).  stdin: one shape per line, `rank|score N d B K max_norm table_addr_mod_16`; stdout: `kernel status`.
#include <stdio.h>
#include <string.h>

#include "ge_sweep_route.h"

int main() {
  char entry[16];
  long long N, B, K;
  int d, mod16;
  float max_norm;
  while (scanf("%15s %lld %d %lld %lld %f %d", entry, &N, &d, &B, &K, &max_norm, &mod16) == 7) {
    const ge::SweepRoute r = strcmp(entry, "rank") == 0 ? ge::route_rank(N, d, B, K, max_norm, mod16)
                                                        : ge::route_score(N, d, B, K, max_norm, mod16);
    printf("%d %d\n", r.kernel, r.status);
  }
  return 0;
}
