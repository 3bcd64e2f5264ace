// ge_softmax_labels.hip -- multi-label ("KvsAll") softmax training of ComplEx: the objective of ge_softmax.hip with one row
// per distinct QUERY (fixed, relation) and all its known answers as labels, the target uniform over them.  Row i's labels
// are the candidate POSITIONS label_pos[label_off[i] .. label_off[i + 1]), n_i of them (a position named twice counts twice).
//
//   loss_i = logsumexp_j z_ij - (1 / n_i) sum_l z_i,l,      w_ij = dL/ds_ij = -scale * (softmax_j(z_ij) - y_ij / n_i)
//
// The dense part -scale * p_ij is what ge_softmax.hip's sweeps compute for a query whose key matches no candidate's, so the
// sweeps run as they are (through their launchers: this file instantiates none).  The sparse part is new:
//
//   softmax_prepare_kernel     ge_softmax.hip's, with a true id of 0 for every row: it leaves key 0 on a row whose fixed and
//                              relation ids are in the table, -1 otherwise;
//   softmax_labels_kernel      one wave per query: the offsets and every label checked (a row with none, with offsets that
//                              decrease or leave [0, L], with a position outside [0, K) or on an empty slot is invalid);
//                              each label's logit sm_logit(scale, Q'_i . C'_l) with the dot product taken as the sweeps take
//                              it (32 labels a pass on the MFMA, the sweeps' k order), so it has the sweeps' bits;
//                              their mean in double; (scale / n_i) sum_l C'_l in label order as one more dL/dQ' partial; the
//                              key kSmNoMatch on a valid row, -1 on an invalid one -- before any gradient sweep.  Then one
//                              thread per label entry: the row it belongs to, by a binary search in label_off;
//   softmax_labels_merge_kernel   softmax_merge_kernel's arithmetic with the label mean in z_true's place;
//   softmax_finish_kernel      ge_softmax.hip's over the sweep's partials and the label term: candidate and query slots;
//   softmax_label_slots_kernel    one wave per label entry x of row i: slot K + 2B + x = -lr * the clip derivative of the
//                              label's candidate row applied to (scale / n_i) Q'_i.  The clip derivative is linear in g, so
//                              the label term of a candidate's gradient is a slice of its own and the step's sort + sum adds
//                              it to the dense slot in a fixed order: no transposed list, no scatter, no float atomics.
#include "ge_softmax_kern.h"

namespace ge {

// a key no candidate can have (candidate keys are ids below N <= INT32_MAX, or -1) and that counts as valid (>= 0)
constexpr int32_t kSmNoMatch = INT32_MAX;
constexpr int kSmLabelCols = (kRankMaxDim + kWave - 1) / kWave;      // columns a lane owns of a row

SoftmaxLabelsWs softmax_labels_ws(void* base, int64_t B, int64_t K, int32_t d, int64_t L) {
  SoftmaxLabelsWs w;
  w.base = softmax_ws(base, B, K, d);
  size_t off = w.base.bytes;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  // d % 8 == 0: the eight partials end on a multiple of 256 bytes, the ninth follows them without a gap
  w.lsum = ws_at<float>(base, take(sizeof(float) * (size_t)B * d));
  w.mean = ws_at<double>(base, take(sizeof(double) * (size_t)B));
  w.row_of = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)L));
  w.bytes = off;
  return w;
}

size_t softmax_labels_ws_bytes(int64_t B, int64_t K, int32_t d, int64_t L) { return softmax_labels_ws(nullptr, B, K, d, L).bytes; }

__global__ __launch_bounds__(kBlock) void softmax_labels_kernel(
    const float* __restrict__ qp, const float* __restrict__ cp, const int32_t* __restrict__ ckey, int d, int64_t B, int64_t K,
    const int32_t* __restrict__ label_off, const int32_t* __restrict__ label_pos, int64_t L, float scale,
    int32_t* __restrict__ qkey, float* __restrict__ lsum, double* __restrict__ mean, int32_t* __restrict__ row_of) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid >> 6; i < B; i += nthreads >> 6) {          // (wave-uniform)
    const int64_t lo = label_off[i], hi = label_off[i + 1];
    bool ok = qkey[i] >= 0 && lo >= 0 && hi > lo && hi <= L;
    const float* q = qp + i * d;
    float acc[kSmLabelCols];
#pragma unroll
    for (int n = 0; n < kSmLabelCols; ++n) acc[n] = 0.f;
    double zsum = 0.0;
    // 32 labels a pass: lane li (both halves) owns label x0 + li.  Its logit is the sweep's OWN arithmetic -- the same MFMA,
    // the same four chains over k, the same pairwise sum and the same sm_logit -- on an A operand whose 32 rows are all
    // Q'_i, so z_i,l has the bits the LSE sweep summed: at K = 1 the loss is exactly 0, and a row's loss carries one error
    // of its logits, not the difference of two
    const int li = lane & 31, lh = lane >> 5;
    for (int64_t x0 = lo; ok && x0 < hi; x0 += 32) {
      const int cnt = hi - x0 < 32 ? (int)(hi - x0) : 32;
      const int32_t p = li < cnt ? label_pos[x0 + li] : 0;
      const bool in_k = p >= 0 && p < K;
      if (__any(li < cnt && (!in_k || ckey[in_k ? p : 0] < 0))) { ok = false; break; }
      const float* ap = q + lh;
      const float* bp = cp + (int64_t)p * d + lh;
      sm_f32x16 ac4[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) ac4[c][e] = 0.f;
      for (int kk = 0; kk < d; kk += 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          ac4[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 2 * c], li < cnt ? bp[kk + 2 * c] : 0.f, ac4[c], 0, 0, 0);
      }
      // (C layout: this lane holds column li of rows 4 lh ...: every row is the query, element 0 will do)
      const float z = sm_logit(scale, (ac4[0][0] + ac4[1][0]) + (ac4[2][0] + ac4[3][0]));
      for (int j = 0; j < cnt; ++j) {                    // in label order
        zsum += (double)__shfl(z, j, kWave);
        const float* c = cp + (int64_t)__shfl(p, j, kWave) * d;
#pragma unroll
        for (int n = 0; n < kSmLabelCols; ++n) {
          const int col = lane + kWave * n;
          if (col < d) acc[n] += c[col];
        }
      }
    }
    const float coef = ok ? scale / (float)(hi - lo) : 0.f;
#pragma unroll
    for (int n = 0; n < kSmLabelCols; ++n) {
      const int col = lane + kWave * n;
      if (col < d) lsum[i * d + col] = ok ? coef * acc[n] : 0.f;
    }
    if (lane == 0) {
      mean[i] = ok ? zsum / (double)(hi - lo) : 0.0;
      qkey[i] = ok ? kSmNoMatch : -1;                      // an invalid row contributes to no gradient
    }
  }
  // the row of every label entry: the last row whose offset is <= x, if x is inside it (offsets that are not sorted give
  // some row or none, the same one every time; whether the row is valid is its key's business)
  for (int64_t x = tid; x < L; x += nthreads) {
    int64_t a = 0, b = B;
    while (b - a > 1) {
      const int64_t mid = (a + b) >> 1;
      if (label_off[mid] <= x) a = mid; else b = mid;
    }
    row_of[x] = label_off[a] <= x && x < label_off[a + 1] ? (int32_t)a : -1;
  }
}

// softmax_merge_kernel (ge_softmax.hip) with the mean of the label logits for z_true; validity is the key's, decided by
// softmax_labels_kernel (a valid row has a label on a live candidate, so its sum is positive)
__global__ __launch_bounds__(kBlock) void softmax_labels_merge_kernel(
    const float4* __restrict__ part, int n_ranges, int64_t B, const int32_t* __restrict__ qkey, const double* __restrict__ mean,
    float* __restrict__ lse, float* __restrict__ loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float ninf = -__builtin_inff();
  float m = ninf;
  double s = 0.0;
  for (int r = 0; r < n_ranges; ++r) {
    const float4 p = part[(int64_t)r * B + i];
    if (p.x > ninf) {
      const float nm = fmaxf(m, p.x);
      s = (m > ninf ? s * exp((double)m - (double)nm) : 0.0) + (double)p.y * exp((double)p.x - (double)nm);
      m = nm;
    }
  }
  const bool ok = qkey[i] >= 0;
  const double ls = log(s);
  lse[i] = ok ? m : 0.f;
  lse[B + i] = ok ? (float)ls : 0.f;
  loss[i] = ok ? (float)(((double)m - mean[i]) + ls) : __builtin_nanf("");
}

__global__ __launch_bounds__(kBlock) void softmax_label_slots_kernel(
    const float* __restrict__ table, int d, int64_t B, int64_t K, int64_t L, float max_norm, float scale, float lr,
    const float* __restrict__ qp, const int32_t* __restrict__ qkey, const int32_t* __restrict__ ckey,
    const int32_t* __restrict__ label_off, const int32_t* __restrict__ label_pos, const int32_t* __restrict__ row_of,
    int32_t* __restrict__ grad_idx, float* __restrict__ grad_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float neg_lr = -lr;
  for (int64_t x = wave; x < L; x += nwaves) {             // (wave-uniform)
    float* gv = grad_val + (K + 2 * B + x) * d;
    const int32_t i = row_of[x];
    const bool ok = i >= 0 && qkey[i] >= 0;               // a valid row: every label of it is a live candidate's position
    const int32_t id = ok ? ckey[label_pos[x]] : -1;
    if (lane == 0) grad_idx[K + 2 * B + x] = id;
    if (!ok) {
      for (int c = lane; c < d; c += kWave) gv[c] = 0.f;
      continue;
    }
    const float coef = scale / (float)(label_off[i + 1] - label_off[i]);
    const float* q = qp + (int64_t)i * d;
    const float* xr = table + (int64_t)id * d;
    float ss = 0.f, xg = 0.f;
    for (int c = lane; c < d; c += kWave) { ss += xr[c] * xr[c]; xg += xr[c] * (coef * q[c]); }
    float alpha, beta;
    sm_clip_back(sm_wave_sum(ss), sm_wave_sum(xg), max_norm, alpha, beta);
    for (int c = lane; c < d; c += kWave) {
      const float gr = alpha * (coef * q[c]) + beta * xr[c];
      gv[c] = neg_lr * gr;
    }
  }
}

int softmax_labels_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                          const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                          float lr, int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                          hipStream_t st) {
  assert(d % 8 == 0 && d >= 8 && d <= kRankMaxDim && N <= INT32_MAX);
  const SoftmaxLabelsWs lw = softmax_labels_ws(workspace, B, K, d, L);
  const SoftmaxWs& w = lw.base;
  assert(lw.lsum == w.gq + (size_t)kSmMaxSplit * B * d);
  // the prepare kernel's true ids: B zeros, in the words the merge kernel fills later
  int32_t* zeros = reinterpret_cast<int32_t*>(w.lse);
  if (hipError_t e = hipMemsetAsync(zeros, 0, sizeof(int32_t) * (size_t)B, st)) return (int)e;
  if (int rc = softmax_prepare_launch(table, N, d, hr, B, zeros, cand, K, max_norm, cand_is_head, nullptr, 0, w, st)) return rc;
  // the label term is the partial after the sweep's ns (lw.lsum is the room for it when ns is kSmMaxSplit)
  const int ns = sm_split(B, K);
  hipLaunchKernelGGL(softmax_labels_kernel, dim3(grid_for(B, kBlock / kWave)), dim3(kBlock), 0, st, w.qp, w.cp, w.ckey, d, B, K,
                     label_off, label_pos, L, scale, w.qkey, w.gq + (size_t)ns * B * d, lw.mean, lw.row_of);
  if (int rc = launch_status()) return rc;
  if (int rc = softmax_lse_launch(w, B, K, d, scale, ns, st)) return rc;
  hipLaunchKernelGGL(softmax_labels_merge_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, w.part, ns,
                     B, w.qkey, lw.mean, w.lse, loss);
  if (int rc = launch_status()) return rc;
  if (!grad_idx) return 0;
  if (int rc = softmax_grad_sweeps_launch(w, B, K, d, scale, ns, grad_val, st)) return rc;
  if (int rc = softmax_finish_launch(table, d, hr, B, K, max_norm, lr, cand_is_head, w, ns + 1, grad_idx, grad_val, st)) return rc;
  if (L == 0) return 0;
  hipLaunchKernelGGL(softmax_label_slots_kernel, dim3(grid_for(L, kBlock / kWave)), dim3(kBlock), 0, st, table, d, B, K, L,
                     max_norm, scale, lr, w.qp, w.qkey, w.ckey, label_off, label_pos, lw.row_of, grad_idx, grad_val);
  return launch_status();
}

}  // namespace ge
