// ge_softmax_sampled.hip -- sampled softmax training of ComplEx with shared negatives: the objective of ge_softmax.hip
// over K candidates that need not hold the true entity, so that the work follows K and not the table.
//
//   z_i,true = -scale * (Q'_i . T'_i)        T'_i = clip(true_i): the true entity's own logit, counted once
//   loss_i = log(exp(z_i,true) + sum_{j: cand_j valid, cand_j != true_i} exp(z_ij)) - z_i,true
//   w_ij = -scale * p_ij (0 where cand_j == true_i: accidental hits are removed),  w_i,true = -scale * (p_i,true - 1)
//
//   softmax_sampled_prepare_kernel   softmax_prepare_kernel's Q', C' and keys, and T' [B, d] and z_i,true (the dot product
//                                    summed in double and rounded once, then sm_logit's one rounded product);
//   softmax_sweep_kernel<.., true>   the SAMPLED instantiations of ge_softmax_kern.h.  The candidate-side gradient sweep is
//                                    split over query ranges as the query-side ones are over candidate ranges: at K = 1024
//                                    it would otherwise be 16 workgroups;
//   softmax_sampled_merge_kernel     the partials in range order and then the true logit, one more term of the double merge;
//                                    the loss with its two dominant logits (the true one, the largest candidate's) from
//                                    the table in double;
//   softmax_sampled_finish_kernel    candidates: their partials summed in range order, then the clip derivative; queries:
//                                    dL/dQ'_i = sum of partials + w_i,true T'_i, split as in softmax_finish_kernel; the third
//                                    slot of a row: the clip derivative of the true row on w_i,true Q'_i.
//
// No float atomics: every sum has one fixed order.
#include "ge_softmax_kern.h"

namespace ge {

// (sm_gc_rows(B, K), the rows of dL/dC' partials for every split softmax_sampled_launch can choose: ge_softmax_route.h)
SoftmaxSampledWs softmax_sampled_ws(void* base, int64_t B, int64_t K, int32_t d) {
  SoftmaxSampledWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  w.qp = ws_at<float>(base, take(sizeof(float) * (size_t)B * d));
  w.cp = ws_at<float>(base, take(sizeof(float) * (size_t)K * d));
  w.tp = ws_at<float>(base, take(sizeof(float) * (size_t)B * d));
  w.qkey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)B));
  w.ckey = ws_at<int32_t>(base, take(sizeof(int32_t) * (size_t)K));
  w.zt = ws_at<float>(base, take(sizeof(float) * (size_t)B));
  w.lse = ws_at<float>(base, take(sizeof(float) * 2 * (size_t)B));
  w.part = ws_at<float4>(base, take(sizeof(float4) * (size_t)B * kSmMaxSplit));
  w.gq = ws_at<float>(base, take(sizeof(float) * (size_t)B * d * kSmMaxSplit));
  w.gc = ws_at<float>(base, take(sizeof(float) * sm_gc_rows(B, K) * d));
  w.bytes = off;
  return w;
}

size_t softmax_sampled_ws_bytes(int64_t B, int64_t K, int32_t d) { return softmax_sampled_ws(nullptr, B, K, d).bytes; }

// ------------------------------------------------------------------ prepare
__device__ __forceinline__ double sm_wave_sum_f64(double v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

__global__ __launch_bounds__(kBlock) void softmax_sampled_prepare_kernel(
    const float* __restrict__ table, int64_t N, int d, const int32_t* __restrict__ hr, int64_t B,
    const int32_t* __restrict__ true_id, const int32_t* __restrict__ cand, int64_t K, float max_norm, float scale,
    int cand_is_head, float* __restrict__ qp, float* __restrict__ cp, float* __restrict__ tp, int32_t* __restrict__ qkey,
    int32_t* __restrict__ ckey, float* __restrict__ zt) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  for (int64_t u = wave; u < B + K; u += nwaves) {      // (wave-uniform)
    if (u < B) {
      const int32_t f = hr[2 * u], r = hr[2 * u + 1], tr = true_id[u];
      const bool ok = f >= 0 && f < N && r >= 0 && r < N && tr >= 0 && tr < N;
      float* dst = qp + u * d;
      float* dt = tp + u * d;
      if (!ok) {
        for (int c = lane; c < d; c += kWave) { dst[c] = 0.f; dt[c] = 0.f; }
        if (lane == 0) { qkey[u] = -1; zt[u] = 0.f; }
        continue;
      }
      const float* fr = table + (int64_t)f * d;
      const float* rr = table + (int64_t)r * d;
      const float* xr = table + (int64_t)tr * d;
      float ssf = 0.f, ssr = 0.f, sst = 0.f;
      for (int c = lane; c < d; c += kWave) { ssf += fr[c] * fr[c]; ssr += rr[c] * rr[c]; sst += xr[c] * xr[c]; }
      float i0, i1, i2;
      const float scf = clip_scale(sm_wave_sum(ssf), max_norm, i0), scr = clip_scale(sm_wave_sum(ssr), max_norm, i1);
      const float sct = clip_scale(sm_wave_sum(sst), max_norm, i2);
      double dot = 0.0;
      for (int c = lane; c < k; c += kWave) {
        const float a = fr[c] * scf, b = fr[k + c] * scf, e = rr[c] * scr, g = rr[k + c] * scr;
        float q0, q1;
        if (!cand_is_head) { q0 = a * e - b * g; q1 = a * g + b * e; }     // q = h * r
        else               { q0 = e * a + g * b; q1 = e * b - g * a; }     // [Re(r conj t) | -Im(r conj t)]
        const float t0 = xr[c] * sct, t1 = xr[k + c] * sct;
        dst[c] = q0; dst[k + c] = q1; dt[c] = t0; dt[k + c] = t1;
        dot += (double)q0 * (double)t0 + (double)q1 * (double)t1;
      }
      dot = sm_wave_sum_f64(dot);
      if (lane == 0) { qkey[u] = tr; zt[u] = sm_logit(scale, (float)dot); }
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
// The gradient sweeps need (m, log sum) of the fp32 logits they recompute, and get it: softmax_merge_kernel's merge in
// double, with the true logit as the last term.  It is always there for a valid row, so the sum is never empty, and a row
// whose slots are all empty or left out gives m = z_true, s = 1, loss = 0 exactly.
// The LOSS is log sum - z_true, which unlike the 1-vs-all loss can be large (a candidate far above the true entity): then
// it is the difference of two logits, and what fp32 does to the larger one -- the clip scales and products that make Q'
// and C', the score GEMM's sum, the product with scale -- is an error of the size of the loss's own spacing.  So the loss
// takes its two dominant terms from the table in double: the true logit and the logit of the candidate the sweep named
// as the row's maximum.  One thread a row, five rows of d: nothing next to the sweeps.  Every other term keeps its fp32
// logit, relative to the fp32 maximum.
__device__ __forceinline__ double sm_clip_f64(const float* x, int d, float max_norm) {
  double ss = 0.0;
  for (int c = 0; c < d; ++c) ss += (double)x[c] * (double)x[c];
  const double n = sqrt(ss);
  return n > (double)max_norm ? (double)max_norm / n : 1.0;
}

__global__ __launch_bounds__(kBlock) void softmax_sampled_merge_kernel(
    const float4* __restrict__ part, int n_ranges, int64_t B, const float* __restrict__ table, int d,
    const int32_t* __restrict__ hr, const int32_t* __restrict__ true_id, float max_norm, float scale, int cand_is_head,
    const int32_t* __restrict__ qkey, const int32_t* __restrict__ ckey, const float* __restrict__ zt,
    float* __restrict__ lse, float* __restrict__ loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float ninf = -__builtin_inff();
  float m = ninf;
  double s = 0.0;
  int arg = -1;
  for (int r = 0; r < n_ranges; ++r) {
    const float4 p = part[(int64_t)r * B + i];
    if (p.x > ninf) {
      if (p.x > m) arg = __float_as_int(p.z);
      const float nm = fmaxf(m, p.x);
      s = (m > ninf ? s * exp((double)m - (double)nm) : 0.0) + (double)p.y * exp((double)p.x - (double)nm);
      m = nm;
    }
  }
  const bool ok = qkey[i] >= 0;
  double l = 0.0;                                      // no candidate term: log(exp(z_true)) - z_true
  if (ok && arg >= 0) {
    const int k = d >> 1;
    const float* f = table + (int64_t)hr[2 * i] * d;
    const float* r = table + (int64_t)hr[2 * i + 1] * d;
    const float* x = table + (int64_t)true_id[i] * d;
    const float* c = table + (int64_t)ckey[arg] * d;   // (a maximum above -inf is a valid candidate's)
    const double sf = sm_clip_f64(f, d, max_norm), sr = sm_clip_f64(r, d, max_norm);
    const double sx = sm_clip_f64(x, d, max_norm), sc = sm_clip_f64(c, d, max_norm);
    double dx = 0.0, dc = 0.0;
    for (int j = 0; j < k; ++j) {
      const double a = f[j] * sf, b = f[k + j] * sf, e = r[j] * sr, g = r[k + j] * sr;
      const double q0 = !cand_is_head ? a * e - b * g : e * a + g * b;
      const double q1 = !cand_is_head ? a * g + b * e : e * b - g * a;
      dx += q0 * (double)x[j] + q1 * (double)x[k + j];
      dc += q0 * (double)c[j] + q1 * (double)c[k + j];
    }
    const double zd = -(double)scale * (dx * sx), zm = -(double)scale * (dc * sc);
    const double top = zm > zd ? zm : zd;
    const double gap = zm > zd ? zm - zd : zd - zm;    // (|zm - zd| as ONE value: contracted into the products that
    const double rest = s > 1.0 ? s - 1.0 : 0.0;       //  make zd, `top - zd` is their rounding error, not zero)
    // rest: the candidates' sum without its largest term, relative to m.  The larger of the two logits is the term 1 of
    // log1p: the loss is never below zero, and a tiny one keeps its digits
    l = (zm > zd ? gap : 0.0) + log1p(rest * exp((double)m - top) + exp(-gap));
  }
  const float z = zt[i];
  {
    const float nm = fmaxf(m, z);
    s = (m > ninf ? s * exp((double)m - (double)nm) : 0.0) + exp((double)z - (double)nm);
    m = nm;
  }
  lse[i] = ok ? m : 0.f;
  lse[B + i] = ok ? (float)log(s) : 0.f;
  loss[i] = ok ? (float)l : __builtin_nanf("");
}

// ------------------------------------------------------------------ finish
// Slots: [0, K) the candidates, K + 3 i the fixed row, K + 3 i + 1 the relation, K + 3 i + 2 the true entity of row i.
__global__ __launch_bounds__(kBlock) void softmax_sampled_finish_kernel(
    const float* __restrict__ table, int d, const int32_t* __restrict__ hr, const int32_t* __restrict__ true_id, int64_t B,
    int64_t K, float max_norm, float scale, float lr, int cand_is_head, const int32_t* __restrict__ qkey,
    const int32_t* __restrict__ ckey, const float* __restrict__ qp, const float* __restrict__ tp,
    const float* __restrict__ zt, const float* __restrict__ lse, const float* __restrict__ gq, int n_ranges,
    const float* __restrict__ gc, int n_qranges, int32_t* __restrict__ grad_idx, float* __restrict__ grad_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int k = d >> 1;
  const float neg_lr = -lr;
  for (int64_t u = wave; u < K + B; u += nwaves) {      // (wave-uniform)
    if (u < K) {
      float* gv = grad_val + u * d;
      const int32_t id = ckey[u];
      if (lane == 0) grad_idx[u] = id;
      if (id < 0) {
        for (int c = lane; c < d; c += kWave) gv[c] = 0.f;
        continue;
      }
      const float* x = table + (int64_t)id * d;
      float ss = 0.f, xg = 0.f;
      for (int c = lane; c < d; c += kWave) {
        float g = 0.f;
        for (int s = 0; s < n_qranges; ++s) g += gc[((int64_t)s * K + u) * d + c];      // range order
        gv[c] = g;
        ss += x[c] * x[c]; xg += x[c] * g;
      }
      float alpha, beta;
      sm_clip_back(sm_wave_sum(ss), sm_wave_sum(xg), max_norm, alpha, beta);
      for (int c = lane; c < d; c += kWave) {           // each lane rereads the columns it wrote
        const float gr = alpha * gv[c] + beta * x[c];
        gv[c] = neg_lr * gr;
      }
    } else {
      const int64_t i = u - K;
      float* gf = grad_val + (K + 3 * i) * d;
      float* gr = gf + d;
      float* gt = gr + d;
      const bool ok = qkey[i] >= 0;
      if (lane == 0) {
        grad_idx[K + 3 * i] = ok ? hr[2 * i] : -1;
        grad_idx[K + 3 * i + 1] = ok ? hr[2 * i + 1] : -1;
        grad_idx[K + 3 * i + 2] = ok ? true_id[i] : -1;
      }
      if (!ok) {
        for (int c = lane; c < 3 * d; c += kWave) gf[c] = 0.f;
        continue;
      }
      const float* f = table + (int64_t)hr[2 * i] * d;
      const float* r = table + (int64_t)hr[2 * i + 1] * d;
      const float* x = table + (int64_t)true_id[i] * d;
      const float* q = qp + i * d;
      const float* tc = tp + i * d;
      // w_i,true = -scale (p_i,true - 1), p from the same (m, log sum) pair the sweeps subtract
      const float wt = -scale * (expf((zt[i] - lse[i]) - lse[B + i]) - 1.f);
      float ssf = 0.f, ssr = 0.f, sst = 0.f, tg = 0.f;
      for (int c = lane; c < d; c += kWave) {
        const float g = wt * q[c];
        gt[c] = g;
        ssf += f[c] * f[c]; ssr += r[c] * r[c]; sst += x[c] * x[c]; tg += x[c] * g;
      }
      ssf = sm_wave_sum(ssf); ssr = sm_wave_sum(ssr); sst = sm_wave_sum(sst);
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
        Gre += wt * tc[c]; Gim += wt * tc[k + c];
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
      float af, bf, ar, br, at, bt;
      sm_clip_back(ssf, sm_wave_sum(fg), max_norm, af, bf);
      sm_clip_back(ssr, sm_wave_sum(rg), max_norm, ar, br);
      sm_clip_back(sst, sm_wave_sum(tg), max_norm, at, bt);
      // pass 2: each lane rereads the columns it wrote
      for (int c = lane; c < k; c += kWave) {
        const float v0 = af * gf[c] + bf * f[c], v1 = af * gf[k + c] + bf * f[k + c];
        const float v2 = ar * gr[c] + br * r[c], v3 = ar * gr[k + c] + br * r[k + c];
        gf[c] = neg_lr * v0; gf[k + c] = neg_lr * v1; gr[c] = neg_lr * v2; gr[k + c] = neg_lr * v3;
      }
      for (int c = lane; c < d; c += kWave) {
        const float v = at * gt[c] + bt * x[c];
        gt[c] = neg_lr * v;
      }
    }
  }
}

// ------------------------------------------------------------------ host
int softmax_sampled_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head,
                           float* loss, int32_t* grad_idx, float* grad_val, void* workspace, hipStream_t st) {
  assert(d % 8 == 0 && d >= 8 && d <= kRankMaxDim);
  const SoftmaxSampledWs w = softmax_sampled_ws(workspace, B, K, d);
  hipLaunchKernelGGL(softmax_sampled_prepare_kernel, dim3(grid_for(B + K, kBlock / kWave)), dim3(kBlock), 0, st, table, N, d,
                     hr, B, true_id, cand, K, max_norm, scale, cand_is_head, w.qp, w.cp, w.tp, w.qkey, w.ckey, w.zt);
  if (int rc = launch_status()) return rc;
  const int ns = sm_split(B, K);
  if (int rc = sm_sweep<0, true, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, nullptr, ns, reinterpret_cast<float*>(w.part),
                                       st))
    return rc;
  hipLaunchKernelGGL(softmax_sampled_merge_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, w.part, ns,
                     B, table, d, hr, true_id, max_norm, scale, cand_is_head, w.qkey, w.ckey, w.zt, w.lse, loss);
  if (int rc = launch_status()) return rc;
  if (!grad_idx) return 0;
  // dL/dC' per query range (the mirror image of the candidate ranges), dL/dQ' per candidate range
  const int nq = sm_split(K, B);
  assert((size_t)nq * (size_t)K <= sm_gc_rows(B, K));
  if (int rc = sm_sweep<1, false, true>(w.cp, w.ckey, K, w.qp, w.qkey, B, d, scale, w.lse, nq, w.gc, st)) return rc;
  if (int rc = sm_sweep<1, true, true>(w.qp, w.qkey, B, w.cp, w.ckey, K, d, scale, w.lse, ns, w.gq, st)) return rc;
  hipLaunchKernelGGL(softmax_sampled_finish_kernel, dim3(grid_for(B + K, kBlock / kWave)), dim3(kBlock), 0, st, table, d, hr,
                     true_id, B, K, max_norm, scale, lr, cand_is_head, w.qkey, w.ckey, w.qp, w.tp, w.zt, w.lse, w.gq, ns, w.gc,
                     nq, grad_idx, grad_val);
  return launch_status();
}

}  // namespace ge
