// ge_softmax.hip -- 1-vs-all softmax training of ComplEx (the "1vsAll" objective of Lacroix et al. 2018 in place of the
// hinge of holE.py:231): multiclass log-loss of the true candidate over ALL candidates, on the candidate GEMM of
// ge_1vk.hip (score_1vK_kernel) in exact fp32 (v_mfma_f32_32x32x2_f32).  No [B, K] array exists at any point: scores
// are recomputed tile by tile, flash-attention style.  No float atomics: every sum has one fixed order.
//
//   s_ij = Q'_i . C'_j        Q'_i = clip(fixed_i) o clip(rel_i) in score_1vK_kernel's staging form, C'_j = clip(cand_j)
//   z_ij = -scale * s_ij      (lower score = more plausible, as every evaluator ranks)
//   loss_i = logsumexp_j z_ij - z_i,true,      w_ij = dL/ds_ij = -scale * (softmax_j(z_ij) - [cand_j == true_i])
//
//   softmax_prepare_kernel   one wave per query / candidate: Q' [B, d], C' [K, d] (clipped, dense) and the match keys
//                            (true id of a valid row, candidate id of a valid candidate, -1 otherwise);
//   softmax_sweep_kernel     a fixed tile of 64 X rows against a range of 64-row Y tiles.  Per Y tile: S = X . Y^T (Y whole
//                            in LDS; X whole too up to d = 256, beyond that in 32-column chunks per Y tile), then
//       LSE    X = queries: running (max, sum) and z_true per row, one partial per (row, range);
//       GRAD   w -> LDS, G_X += W . Y (second GEMM, accumulators in registers): X = candidates over all queries gives
//              dL/dC'_j (straight into the candidates' gradient slots), X = queries over a candidate range dL/dQ'_i
//              (one partial per range);
//   softmax_merge_kernel     partials in range order, in double -> lse_i as the pair (max, log sum), loss_i, validity;
//   softmax_finish_kernel    one wave per slot: the clip derivative (alpha g + beta x, row_coef of ge_complex_dev.h) on
//                            the candidate rows; dL/dQ' (partials summed in range order) split into the fixed row's and
//                            the relation's gradients (two complex products, two clips); IndexedSlices written.
//
// The scalar x . g the clip's beta needs is a dot product in the finish kernel, not a second sum in the sweep.
// The sweep template, its constants and the helpers the sampled form (ge_softmax_sampled.hip) shares are in ge_softmax_kern.h.
// The masked form (ge_softmax_masked.hip) runs this file's prepare, merge and finish kernels through their launchers; the
// multi-label form (ge_softmax_labels.hip) runs its prepare, its three sweeps and its finish kernel through theirs.
#include "ge_softmax_kern.h"

namespace ge {

SoftmaxWs softmax_ws(void* base, int64_t B, int64_t K, int32_t d) {
  SoftmaxWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  w.qp = ws_at<float>(base, take(sizeof(float) * (size_t)B * d));
  w.cp = ws_at<float>(base, take(sizeof(float) * (size_t)K * d));
  w.qkey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)B));
  w.ckey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)K));
  w.lse = ws_at<float>(base, take(sizeof(float) * 2 * (size_t)B));
  w.part = ws_at<float4>(base, take(sizeof(float4) * (size_t)B * kSmMaxSplit));
  w.gq = ws_at<float>(base, take(sizeof(float) * (size_t)B * d * kSmMaxSplit));
  w.bytes = off;
  return w;
}

// ------------------------------------------------------------------ prepare
// SETS (the masked form, ge_softmax_masked.hip): a row whose set id is neither -1 nor in [0, n_sets) is invalid too.
template <bool SETS>
__global__ __launch_bounds__(kBlock) void softmax_prepare_kernel(
    const float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ hr, int64_t B,
    const int32_t* __restrict__ true_id, const int32_t* __restrict__ cand, int64_t K, float max_norm, int cand_is_head,
    float* __restrict__ qp, float* __restrict__ cp, int32_t* __restrict__ qkey, int32_t* __restrict__ ckey,
    const int32_t* __restrict__ row_set, int32_t n_sets) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  for (int64_t u = wave; u < B + K; u += nwaves) {      // (wave-uniform)
    if (u < B) {
      const int32_t f = hr[2 * u], r = hr[2 * u + 1], tr = true_id[u];
      bool ok = f >= 0 && f < N && r >= 0 && r < N && tr >= 0 && tr < N;
      if constexpr (SETS) { const int32_t sid = row_set[u]; ok = ok && sid >= -1 && sid < n_sets; }
      float* dst = qp + u * d;
      if (!ok) {
        for (int c = lane; c < d; c += kWave) dst[c] = 0.f;
        if (lane == 0) qkey[u] = -1;
        continue;
      }
      const float* fr = table + (int64_t)f * d;
      const float* rr = table + (int64_t)r * d;
      float ssf = 0.f, ssr = 0.f;
      for (int c = lane; c < d; c += kWave) { ssf += fr[c] * fr[c]; ssr += rr[c] * rr[c]; }
      float i0, i1;
      const float scf = clip_scale(sm_wave_sum(ssf), max_norm, i0), scr = clip_scale(sm_wave_sum(ssr), max_norm, i1);
      for (int c = lane; c < k; c += kWave) {
        const float a = fr[c] * scf, b = fr[k + c] * scf, e = rr[c] * scr, g = rr[k + c] * scr;
        if (!cand_is_head) { dst[c] = a * e - b * g; dst[k + c] = a * g + b * e; }     // q = h * r
        else               { dst[c] = e * a + g * b; dst[k + c] = e * b - g * a; }     // [Re(r conj t) | -Im(r conj t)]
      }
      if (lane == 0) qkey[u] = tr;
    } else {
      const int64_t j = u - B;
      const int32_t c_id = cand[j];
      const bool ok = c_id >= 0 && c_id < N;
      float* dst = cp + j * d;
      if (!ok) {
        for (int c = lane; c < d; c += kWave) dst[c] = 0.f;
        if (lane == 0) ckey[j] = -1;
        continue;
      }
      const float* cr = table + (int64_t)c_id * d;
      float ss = 0.f;
      for (int c = lane; c < d; c += kWave) ss += cr[c] * cr[c];
      float i0;
      const float sc = clip_scale(sm_wave_sum(ss), max_norm, i0);
      for (int c = lane; c < d; c += kWave) dst[c] = cr[c] * sc;
      if (lane == 0) ckey[j] = c_id;
    }
  }
}

// ------------------------------------------------------------------ merge
__global__ __launch_bounds__(kBlock) void softmax_merge_kernel(
    const float4* __restrict__ part, int n_ranges, int64_t B, int32_t* __restrict__ qkey, float* __restrict__ lse,
    float* __restrict__ loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float ninf = -__builtin_inff();
  // one thread a row and at most eight partials: the merge, the logarithm and the loss's last sum are taken in double and
  // rounded once, so the loss carries the sweep's fp32 errors only
  float m = ninf, zt = 0.f;
  double s = 0.0;
  bool found = false;
  for (int r = 0; r < n_ranges; ++r) {
    const float4 p = part[(int64_t)r * B + i];
    if (p.x > ninf) {
      const float nm = fmaxf(m, p.x);
      s = (m > ninf ? s * exp((double)m - (double)nm) : 0.0) + (double)p.y * exp((double)p.x - (double)nm);
      m = nm;
    }
    if (p.w > 0.f) { zt = p.z; found = true; }
  }
  const bool ok = qkey[i] >= 0 && found;
  // lse_i stays the pair (m, log s): z - m is exact for the logits that matter (within a factor 2 of m) and neither
  // p = exp((z - m) - log s) nor the loss carries the rounding of m + log s at the magnitude of m
  const double ls = log(s);
  lse[i] = ok ? m : 0.f;
  lse[B + i] = ok ? (float)ls : 0.f;
  loss[i] = ok ? (float)(((double)m - (double)zt) + ls) : __builtin_nanf("");
  if (!ok) qkey[i] = -1;                               // an invalid row contributes to no gradient
}

// ------------------------------------------------------------------ finish
__global__ __launch_bounds__(kBlock) void softmax_finish_kernel(
    const float* __restrict__ table, int d, const int32_t* __restrict__ hr, int64_t B, int64_t K, float max_norm, float lr,
    int cand_is_head, const int32_t* __restrict__ qkey, const int32_t* __restrict__ ckey, const float* __restrict__ gq,
    int n_ranges, int32_t* __restrict__ grad_idx, float* __restrict__ grad_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  const float neg_lr = -lr;
  for (int64_t u = wave; u < K + B; u += nwaves) {      // (wave-uniform)
    if (u < K) {
      // candidate slot u: grad_val[u] holds dL/dC'_u
      float* gv = grad_val + u * d;
      const int32_t id = ckey[u];
      if (lane == 0) grad_idx[u] = id;
      if (id < 0) {
        for (int c = lane; c < d; c += kWave) gv[c] = 0.f;
        continue;
      }
      const float* x = table + (int64_t)id * d;
      float ss = 0.f, xg = 0.f;
      for (int c = lane; c < d; c += kWave) { ss += x[c] * x[c]; xg += x[c] * gv[c]; }
      float alpha, beta;
      sm_clip_back(sm_wave_sum(ss), sm_wave_sum(xg), max_norm, alpha, beta);
      for (int c = lane; c < d; c += kWave) {
        const float gr = alpha * gv[c] + beta * x[c];
        gv[c] = neg_lr * gr;
      }
    } else {
      const int64_t i = u - K;
      float* gf = grad_val + (K + 2 * i) * d;
      float* gr = gf + d;
      const bool ok = qkey[i] >= 0;
      if (lane == 0) { grad_idx[K + 2 * i] = ok ? hr[2 * i] : -1; grad_idx[K + 2 * i + 1] = ok ? hr[2 * i + 1] : -1; }
      if (!ok) {
        for (int c = lane; c < 2 * d; c += kWave) gf[c] = 0.f;
        continue;
      }
      const float* f = table + (int64_t)hr[2 * i] * d;
      const float* r = table + (int64_t)hr[2 * i + 1] * d;
      float ssf = 0.f, ssr = 0.f;
      for (int c = lane; c < d; c += kWave) { ssf += f[c] * f[c]; ssr += r[c] * r[c]; }
      ssf = sm_wave_sum(ssf); ssr = sm_wave_sum(ssr);
      float i0, i1;
      const float scf = clip_scale(ssf, max_norm, i0), scr = clip_scale(ssr, max_norm, i1);
      // pass 1: the gradients wrt the CLIPPED rows into the output rows, and the two dot products
      float fg = 0.f, rg = 0.f;
      for (int c = lane; c < k; c += kWave) {
        float Gre = 0.f, Gim = 0.f;
        for (int s = 0; s < n_ranges; ++s) {
          const float* gp = gq + ((int64_t)s * B + i) * d;
          Gre += gp[c]; Gim += gp[k + c];
        }
        const float a = f[c] * scf, b = f[k + c] * scf, e = r[c] * scr, h = r[k + c] * scr;
        float fa, fb, ra, rb;
        if (!cand_is_head) {     // Q' = (a + ib)(e + ih)
          fa = Gre * e + Gim * h; fb = Gim * e - Gre * h;
          ra = Gre * a + Gim * b; rb = Gim * a - Gre * b;
        } else {                 // Q' = [e a + h b | e b - h a], (a, b) the fixed tail
          fa = Gre * e - Gim * h; fb = Gre * h + Gim * e;
          ra = Gre * a + Gim * b; rb = Gre * b - Gim * a;
        }
        gf[c] = fa; gf[k + c] = fb; gr[c] = ra; gr[k + c] = rb;
        fg += f[c] * fa + f[k + c] * fb;
        rg += r[c] * ra + r[k + c] * rb;
      }
      float af, bf, ar, br;
      sm_clip_back(ssf, sm_wave_sum(fg), max_norm, af, bf);
      sm_clip_back(ssr, sm_wave_sum(rg), max_norm, ar, br);
      // pass 2: each lane rereads the columns it wrote
      for (int c = lane; c < k; c += kWave) {
        const float v0 = af * gf[c] + bf * f[c], v1 = af * gf[k + c] + bf * f[k + c];
        const float v2 = ar * gr[c] + br * r[c], v3 = ar * gr[k + c] + br * r[k + c];
        gf[c] = neg_lr * v0; gf[k + c] = neg_lr * v1; gr[c] = neg_lr * v2; gr[k + c] = neg_lr * v3;
      }
    }
  }
}

// ------------------------------------------------------------------ host
size_t softmax_ws_bytes(int64_t B, int64_t K, int32_t d) { return softmax_ws(nullptr, B, K, d).bytes; }

int softmax_prepare_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, int cand_is_head, const int32_t* row_set,
                           int32_t n_sets, const SoftmaxWs& w, hipStream_t st) {
  const dim3 grid(grid_for(B + K, kBlock / kWave));
  if (row_set)
    hipLaunchKernelGGL(softmax_prepare_kernel<true>, grid, dim3(kBlock), 0, st, table, N, d, hr, B, true_id, cand, K, max_norm,
                       cand_is_head, w.qp, w.cp, w.qkey, w.ckey, row_set, n_sets);
  else
    hipLaunchKernelGGL(softmax_prepare_kernel<false>, grid, dim3(kBlock), 0, st, table, N, d, hr, B, true_id, cand, K, max_norm,
                       cand_is_head, w.qp, w.cp, w.qkey, w.ckey, row_set, n_sets);
  return launch_status();
}

int softmax_merge_launch(const SoftmaxWs& w, int n_ranges, int64_t B, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(softmax_merge_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, w.part, n_ranges,
                     B, w.qkey, w.lse, loss);
  return launch_status();
}

int softmax_finish_launch(const float* table, int32_t d, const int32_t* hr, int64_t B, int64_t K, float max_norm, float lr,
                          int cand_is_head, const SoftmaxWs& w, int n_ranges, int32_t* grad_idx, float* grad_val,
                          hipStream_t st) {
  hipLaunchKernelGGL(softmax_finish_kernel, dim3(grid_for(B + K, kBlock / kWave)), dim3(kBlock), 0, st, table, d, hr, B, K,
                     max_norm, lr, cand_is_head, w.qkey, w.ckey, w.gq, n_ranges, grad_idx, grad_val);
  return launch_status();
}

int softmax_lse_launch(const SoftmaxWs& w, int64_t B, int64_t K, int32_t d, float scale, int n_ranges, hipStream_t st) {
  return sm_sweep<0, true, false>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, nullptr, n_ranges, reinterpret_cast<float*>(w.part), st);
}

int softmax_grad_sweeps_launch(const SoftmaxWs& w, int64_t B, int64_t K, int32_t d, float scale, int n_ranges, float* grad_val,
                               hipStream_t st) {
  // dL/dC' over all queries, straight into the candidates' slots; dL/dQ' per candidate range
  if (int rc = sm_sweep<1, false, false>(w.cp, w.ckey, K, w.qp, w.qkey, B, d, scale, w.lse, 1, grad_val, st)) return rc;
  return sm_sweep<1, true, false>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, w.lse, n_ranges, w.gq, st);
}

int softmax_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                   const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head, float* loss,
                   int32_t* grad_idx, float* grad_val, void* workspace, hipStream_t st) {
  assert(d % 8 == 0 && d >= 8 && d <= kRankMaxDim);
  const SoftmaxWs w = softmax_ws(workspace, B, K, d);
  if (int rc = softmax_prepare_launch(table, N, d, hr, B, true_id, cand, K, max_norm, cand_is_head, nullptr, 0, w, st)) return rc;
  const int ns = sm_split(B, K);
  if (int rc = softmax_lse_launch(w, B, K, d, scale, ns, st)) return rc;
  if (int rc = softmax_merge_launch(w, ns, B, loss, st)) return rc;
  if (!grad_idx) return 0;
  if (int rc = softmax_grad_sweeps_launch(w, B, K, d, scale, ns, grad_val, st)) return rc;
  return softmax_finish_launch(table, d, hr, B, K, max_norm, lr, cand_is_head, w, ns, grad_idx, grad_val, st);
}

}  // namespace ge
