// softmax_masked_skip_probe.hip -- the three MASKED sweeps of the type-constrained softmax (softmax_sweep_kernel<.., false,
// true> of csrc/ge_softmax_kern.h) with the live-tile bitmap the library computes and with a bitmap of all ones, on random
// operands at (B, K, d) = (4096, K, 200) with S block sets (set s admits the candidates [s K / S, (s + 1) K / S), rows in
// set order): the outputs of the two launches compared bit for bit, and ms per launch between device events.  The library
// has no switch for this; the probe launches the kernel template itself and builds the bitmap on the host, by the rule of
// softmax_live_kernel.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -I graphembeddings_amd/csrc tools/probes/softmax_masked_skip_probe.hip \
//         -o tools/probes/softmax_masked_skip_probe  &&  tools/probes/softmax_masked_skip_probe [K [S]]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ge_softmax_kern.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <class T>
static int up(T** dst, const std::vector<T>& v) {
  CK(hipMalloc(dst, v.size() * sizeof(T)));
  CK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t B = 4096;
  const int d = 200;
  const int64_t K = argc > 1 ? atoll(argv[1]) : 14951;
  const int S = argc > 2 ? atoi(argv[2]) : 16;
  if (K < 1 || K > 65536 || S < 1 || S > 4096) { printf("K or S out of range\n"); return 1; }
  const int64_t W = 4 * ((K + 127) / 128), TB = ge::sm_tiles(B), TK = ge::sm_tiles(K);
  const int LW = (int)ge::sm_live_words(K);
  std::vector<float> q((size_t)B * d), c((size_t)K * d), lse(2 * B);
  std::vector<int32_t> qk(B), ck(K), set(B);
  std::vector<uint32_t> mask((size_t)S * W, 0u), live((size_t)TB * LW, 0u), ones((size_t)TB * LW, 0xffffffffu);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f - 0.5f; };
  for (auto& v : q) v = rnd() * 0.14f;                   // |row| about 0.57: rows as after the clip
  for (auto& v : c) v = rnd() * 0.14f;
  for (int64_t j = 0; j < K; ++j) ck[j] = 1000 + (int32_t)j;
  for (int t = 0; t < S; ++t)
    for (int64_t j = t * K / S; j < (t + 1) * K / S; ++j) mask[(size_t)t * W + (j >> 5)] |= 1u << (j & 31);
  for (int64_t i = 0; i < B; ++i) {
    set[i] = (int32_t)(i * S / B);
    qk[i] = ck[set[i] * K / S];                          // the true candidate: the first of the row's set
    lse[i] = 6.f; lse[B + i] = 7.f;
    for (int64_t ct = 0; ct < TK; ++ct) {                // softmax_live_kernel's rule
      const int64_t left = K - ct * 64;
      const unsigned long long in_k = left >= 64 ? ~0ull : (1ull << left) - 1ull;
      const unsigned long long bits = (unsigned long long)mask[(size_t)set[i] * W + 2 * ct] |
                                      ((unsigned long long)mask[(size_t)set[i] * W + 2 * ct + 1] << 32);
      if (bits & in_k) live[(size_t)(i / 64) * LW + (ct >> 5)] |= 1u << (ct & 31);
    }
  }
  int64_t n_live = 0;
  for (int64_t qt = 0; qt < TB; ++qt)
    for (int64_t ct = 0; ct < TK; ++ct) n_live += (live[(size_t)qt * LW + (ct >> 5)] >> (ct & 31)) & 1u;
  float *dq, *dc, *dl, *dout[2];
  int32_t *dqk, *dck, *dset;
  uint32_t *dmask, *dlive[2];
  if (up(&dq, q) || up(&dc, c) || up(&dl, lse) || up(&dqk, qk) || up(&dck, ck) || up(&dset, set) || up(&dmask, mask) ||
      up(&dlive[0], live) || up(&dlive[1], ones))
    return 1;
  const int ns = ge::sm_split(B, K);
  const size_t out_bytes = sizeof(float) * (size_t)(ns * B > K ? ns * B : K) * d;
  CK(hipMalloc(&dout[0], out_bytes)); CK(hipMalloc(&dout[1], out_bytes));
  std::vector<char> h0(out_bytes), h1(out_bytes);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char* names[3] = {"lse", "grad_candidates", "grad_queries"};
  for (int sweep = 0; sweep < 3; ++sweep) {
    size_t used = 0;
    auto go = [&](int which) {
      const ge::SmMaskArgs mk{dset, dmask, dlive[which], W, S, LW};
      float* out = dout[which];
      if (sweep == 0) { used = sizeof(float) * 4 * (size_t)ns * B; return ge::sm_sweep<0, true, false, true>(dq, dqk, B, dc, dck, K, d, 20.f, nullptr, ns, out, nullptr, mk); }
      if (sweep == 1) { used = sizeof(float) * (size_t)K * d; return ge::sm_sweep<1, false, false, true>(dc, dck, K, dq, dqk, B, d, 20.f, dl, 1, out, nullptr, mk); }
      used = sizeof(float) * (size_t)ns * B * d;
      return ge::sm_sweep<1, true, false, true>(dq, dqk, B, dc, dck, K, d, 20.f, dl, ns, out, nullptr, mk);
    };
    float ms[2] = {0.f, 0.f};
    for (int which = 0; which < 2; ++which) {
      CK(hipMemset(dout[which], 0xff, out_bytes));
      for (int i = 0; i < 3; ++i) if (int rc = go(which)) { printf("launch: %d\n", rc); return 1; }
      const int calls = 20;
      CK(hipEventRecord(e0, nullptr));
      for (int i = 0; i < calls; ++i) if (int rc = go(which)) { printf("launch: %d\n", rc); return 1; }
      CK(hipEventRecord(e1, nullptr));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms[which], e0, e1));
      ms[which] /= calls;
    }
    CK(hipMemcpy(h0.data(), dout[0], used, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h1.data(), dout[1], used, hipMemcpyDeviceToHost));
    printf("{\"B\": %lld, \"K\": %lld, \"d\": %d, \"sets\": %d, \"sweep\": \"%s\", \"live_pairs\": %lld, \"pairs\": %lld, "
           "\"ms_skip\": %.4f, \"ms_no_skip\": %.4f, \"bits_equal\": %s}\n",
           (long long)B, (long long)K, d, S, names[sweep], (long long)n_live, (long long)(TB * TK), ms[0], ms[1],
           memcmp(h0.data(), h1.data(), used) == 0 ? "true" : "false");
  }
  return 0;
}
