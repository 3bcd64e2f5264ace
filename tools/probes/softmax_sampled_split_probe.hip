// softmax_sampled_split_probe.hip -- the candidate-side gradient sweep of the sampled softmax (softmax_sweep_kernel<1, false,
// MAXCB, true> of csrc/ge_softmax_kern.h) with ONE query range and with the split softmax_sampled_launch chooses, on
// random operands at (B, K, d) = (4096, K, 200): ms per launch between device events.  The library has no switch for this;
// the probe launches the kernel template itself.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -I graphembeddings_amd/csrc tools/probes/softmax_sampled_split_probe.hip \
//         -o tools/probes/softmax_sampled_split_probe  &&  tools/probes/softmax_sampled_split_probe [K ...]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ge_softmax_kern.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int64_t B = 4096;
  const int d = 200;
  std::vector<int64_t> Ks;
  for (int i = 1; i < argc; ++i) Ks.push_back(atoll(argv[i]));
  if (Ks.empty()) Ks = {256, 1024, 4096};
  for (int64_t K : Ks) {
    if (K < 1 || K > 65536) { printf("K out of range\n"); return 1; }
    std::vector<float> q((size_t)B * d), c((size_t)K * d), lse(2 * B);
    std::vector<int32_t> qk(B), ck(K);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f - 0.5f; };
    for (auto& v : q) v = rnd() * 0.14f;                 // |row| about 0.57: rows as after the clip
    for (auto& v : c) v = rnd() * 0.14f;
    for (int64_t i = 0; i < B; ++i) { qk[i] = 1000 + (int32_t)i; lse[i] = 6.f; lse[B + i] = 7.f; }
    for (int64_t j = 0; j < K; ++j) ck[j] = 1000 + (int32_t)(j * 3);      // some accidental hits
    float *dq, *dc, *dl, *dout;
    int32_t *dqk, *dck;
    const int split = ge::sm_split(K, B);
    CK(hipMalloc(&dq, q.size() * 4)); CK(hipMalloc(&dc, c.size() * 4)); CK(hipMalloc(&dl, lse.size() * 4));
    CK(hipMalloc(&dqk, B * 4)); CK(hipMalloc(&dck, K * 4)); CK(hipMalloc(&dout, (size_t)split * K * d * 4));
    CK(hipMemcpy(dq, q.data(), q.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dc, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, lse.data(), lse.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dqk, qk.data(), B * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dck, ck.data(), K * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int round = 0; round < 3; ++round)
      for (int ranges : {1, split}) {
        auto go = [&]() { return ge::sm_sweep<1, false, true>(dc, dck, K, dq, dqk, B, d, 20.f, dl, ranges, dout, nullptr); };
        for (int i = 0; i < 3; ++i) if (int rc = go()) { printf("launch: %d\n", rc); return 1; }
        const int calls = 30;
        CK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < calls; ++i) if (int rc = go()) { printf("launch: %d\n", rc); return 1; }
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("{\"B\": %lld, \"K\": %lld, \"d\": %d, \"query_ranges\": %d, \"workgroups\": %lld, \"round\": %d, \"ms_per_sweep\": %.4f}\n",
               (long long)B, (long long)K, d, ranges, (long long)(ge::sm_tiles(K) * ranges), round, ms / calls);
      }
    CK(hipFree(dq)); CK(hipFree(dc)); CK(hipFree(dl)); CK(hipFree(dqk)); CK(hipFree(dck)); CK(hipFree(dout));
  }
  return 0;
}
