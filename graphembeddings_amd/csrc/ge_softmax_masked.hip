// ge_softmax_masked.hip -- type-constrained 1-vs-all softmax training of ComplEx: the objective of ge_softmax.hip with
// row i's softmax taken over the candidate POSITIONS its set admits (the mask format of ge_rank_f16_masked.hip:
// mask [n_sets][W], W = candidate_mask_words(K), row_set[i] = -1: unrestricted).
//
//   loss_i = logsumexp_{j admissible for i} z_ij - z_i,true,      w_ij = 0 exactly for an inadmissible pair
//
//   softmax_prepare_kernel<true>      ge_softmax.hip's, which also gives a row with a bad set id the key -1;
//   softmax_live_kernel               one bit per (query tile, candidate tile): some row of the tile with a valid key
//                                     admits some position < K of the candidate tile;
//   softmax_sweep_kernel<.., MASKED>  the MASKED instantiations of ge_softmax_kern.h: the three sweeps of ge_softmax.hip,
//                                     each skipping the pairs whose bit is clear -- on sets that follow the order of the
//                                     candidates, the sweeps cost what the admissible sets cost, not what the table costs;
//   softmax_merge_kernel, softmax_finish_kernel   ge_softmax.hip's: a row whose true candidate is inadmissible was never
//                                     `found` and is invalid as a row whose true id is no candidate is.
//
// A skipped pair would have contributed -inf logits to the LSE (ignored by its m > -inf guard) and +0 products to the
// gradient accumulators: skipping changes no bit (tools/probes/softmax_masked_skip_probe.hip launches both).  No float
// atomics: every sum has one fixed order.
#include "ge_softmax_kern.h"

namespace ge {

SoftmaxMaskedWs softmax_masked_ws(void* base, int64_t B, int64_t K, int32_t d) {
  SoftmaxMaskedWs w;
  w.base = softmax_ws(base, B, K, d);
  w.live = ws_at<uint32_t>(base, w.base.bytes);
  w.bytes = w.base.bytes + align_up(sizeof(uint32_t) * (size_t)sm_tiles(B) * (size_t)sm_live_words(K), 256);
  return w;
}

size_t softmax_masked_ws_bytes(int64_t B, int64_t K, int32_t d) { return softmax_masked_ws(nullptr, B, K, d).bytes; }

// One wave per (query tile, 64 candidate tiles): lane l owns candidate tile 64 blockIdx.x + l and walks the tile's 64 rows
// (the set id is wave-uniform; the lanes' word pairs of a row are consecutive).  The ballot is the two words of the bitmap.
__global__ __launch_bounds__(kWave) void softmax_live_kernel(
    const int32_t* __restrict__ qkey, const int32_t* __restrict__ row_set, int64_t B, int64_t K,
    const uint32_t* __restrict__ mask, int64_t W, int32_t n_sets, int live_words, uint32_t* __restrict__ live) {
  const int lane = threadIdx.x;
  const int64_t qt = blockIdx.y, ct = (int64_t)blockIdx.x * kWave + lane;
  const int64_t left = K - ct * kSmTile;               // positions of the tile below K
  unsigned long long in_k = 0ull;
  if (left >= kSmTile) in_k = ~0ull;
  else if (left > 0) in_k = (1ull << left) - 1ull;
  bool any = false;
  for (int r = 0; r < kSmTile; ++r) {
    const int64_t i = qt * kSmTile + r;
    if (i >= B) break;
    if (qkey[i] < 0) continue;                         // (wave-uniform) a bad set id is a key of -1 already
    const int32_t sid = row_set[i];
    unsigned long long bits = ~0ull;
    if (sid >= 0 && sid < n_sets && in_k) {
      const uint32_t* mp = mask + (int64_t)sid * W + 2 * ct;      // (the mask is 4-byte aligned, no more)
      bits = (unsigned long long)mp[0] | ((unsigned long long)mp[1] << 32);
    }
    any = any || (bits & in_k) != 0ull;
  }
  const unsigned long long b = __ballot(any);
  if (lane == 0) {
    uint32_t* dst = live + qt * live_words + 2 * (int64_t)blockIdx.x;
    dst[0] = (uint32_t)b;
    dst[1] = (uint32_t)(b >> 32);
  }
}

int softmax_masked_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                          const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head,
                          float* loss, int32_t* grad_idx, float* grad_val, void* workspace, const SetArgs& sets,
                          hipStream_t st) {
  assert(d % 8 == 0 && d >= 8 && d <= kRankMaxDim);
  const SoftmaxMaskedWs mws = softmax_masked_ws(workspace, B, K, d);
  const SoftmaxWs& w = mws.base;
  if (int rc = softmax_prepare_launch(table, N, d, hr, B, true_id, cand, K, max_norm, cand_is_head, sets.row_set, sets.n_sets,
                                      w, st))
    return rc;
  const int lw = (int)sm_live_words(K);
  const SmMaskArgs mk{sets.row_set, sets.mask, mws.live, candidate_mask_words(K), sets.n_sets, lw};
  hipLaunchKernelGGL(softmax_live_kernel, dim3((unsigned)(lw / 2), (unsigned)sm_tiles(B)), dim3(kWave), 0, st, w.qkey,
                     sets.row_set, B, K, sets.mask, mk.W, sets.n_sets, lw, mws.live);
  if (int rc = launch_status()) return rc;
  const int ns = sm_split(B, K);
  if (int rc = sm_sweep<0, true, false, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, nullptr, ns,
                                              reinterpret_cast<float*>(w.part), st, mk))
    return rc;
  if (int rc = softmax_merge_launch(w, ns, B, loss, st)) return rc;
  if (!grad_idx) return 0;
  // the two gradient sweeps of softmax_launch; the queries' set ids are the Y side's in the first, the X side's in the second
  if (int rc = sm_sweep<1, false, false, true>(w.cp, w.ckey, K, w.qp, w.qkey, B, d, scale, w.lse, 1, grad_val, st, mk)) return rc;
  if (int rc = sm_sweep<1, true, false, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, w.lse, ns, w.gq, st, mk)) return rc;
  return softmax_finish_launch(table, d, hr, B, K, max_norm, lr, cand_is_head, w, ns, grad_idx, grad_val, st);
}

}  // namespace ge
