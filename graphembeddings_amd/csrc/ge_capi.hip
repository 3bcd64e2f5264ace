// ge_capi.hip -- the extern "C" boundary declared in include/ge_hip.h.
// Argument checks happen here, on the host, before any launch: a kernel that faults can take
// the whole node down, so shapes, alignment and workspace sizes are validated up front.
#include <cmath>

#include "ge_common.h"
#include "ge_launch.h"

using namespace ge;

static inline bool ok_table(const void* t, int64_t N, int32_t d) { return t != nullptr && N > 0 && d > 0; }
static inline bool max_norm_ok(float m) { return m > 0.f; }

extern "C" {

int ge_version(void) { return GE_VERSION; }

int ge_max_dim(void) { return complex_max_dim(); }

int ge_complex_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                     float max_norm, int apply_sigmoid, float* out, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (B > 0 && (!triples || !out)) return GE_EINVAL;
  return complex_score_launch(table, N, d, triples, B, max_norm, apply_sigmoid, out, (hipStream_t)stream);
}

int ge_complex_score_strided(const float* table, int64_t N, int32_t d, int64_t ld, const int32_t* triples, int64_t B,
                             float max_norm, int apply_sigmoid, float* out, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || ld < d) return GE_EINVAL;
  if (B > 0 && (!triples || !out)) return GE_EINVAL;
  return complex_score_launch(table, N, d, triples, B, max_norm, apply_sigmoid, out, (hipStream_t)stream, 0, 0.f, 0.f, nullptr, ld);
}

int ge_complex_logloss(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B, float label,
                       float l2, float max_norm, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (B == 0) return 0;
  if (!triples || !out || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < 256) return GE_ENOMEM;
  float* sumsq = reinterpret_cast<float*>(workspace);
  int rc = table_sumsq_launch(table, N * (int64_t)d, sumsq, (hipStream_t)stream);
  if (rc) return rc;
  return complex_score_launch(table, N, d, triples, B, max_norm, 2, out, (hipStream_t)stream, 0, label, l2, sumsq);
}

int ge_hole_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                  float max_norm, int apply_sigmoid, float* out, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (B > 0 && (!triples || !out)) return GE_EINVAL;
  return hole_score_launch(table, N, d, triples, B, max_norm, apply_sigmoid, out, (hipStream_t)stream);
}

int ge_hole_to_spectral(float* table, int64_t N, int32_t d, void* stream) {
  if (!ok_table(table, N, d)) return GE_EINVAL;
  return hole_spectral_launch(table, N, d, 0, (hipStream_t)stream);
}

int ge_hole_from_spectral(float* table, int64_t N, int32_t d, void* stream) {
  if (!ok_table(table, N, d)) return GE_EINVAL;
  return hole_spectral_launch(table, N, d, 1, (hipStream_t)stream);
}

int ge_hole_spectral_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                           float max_norm, int apply_sigmoid, float* out, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (B > 0 && (!triples || !out)) return GE_EINVAL;
  return complex_score_launch(table, N, d, triples, B, max_norm, apply_sigmoid, out, (hipStream_t)stream, 1);
}

int ge_hinge_loss(const float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                  int64_t B, float margin, float max_norm, int model, float* loss, float* sig_out,
                  void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || model < 0 || model > 2) return GE_EINVAL;
  if (B > 0 && (!pos || !neg || !loss)) return GE_EINVAL;
  if (model != GE_MODEL_HOLE)
    return complex_hinge_loss_launch(table, N, d, pos, neg, B, margin, max_norm, loss, sig_out, (hipStream_t)stream,
                                     model == GE_MODEL_HOLE_SPECTRAL);
  return hole_hinge_loss_launch(table, N, d, pos, neg, B, margin, max_norm, loss, sig_out, (hipStream_t)stream);
}

// The type tables of a sampler, checked and ts filled.  check_ranges: mode, padded_size and n_types too.  The entry
// points do NOT agree on that and are kept as they were (aligning them changes what callers see): the three loops
// (ge_train_steps -- behind its workspace size, sampler_ranges_ok there --, ge_train_steps_logloss,
// ge_train_prepare_steps) refuse a value out of range themselves; ge_corrupt_batch and the two validation ticks pass it
// on to corrupt_batch_launch, which refuses it -- for a tick that is behind its workspace checks and its first launch.
static int type_sampler(TypeSampler& ts, const int32_t* id_to_type, int64_t N, const int64_t* type_offsets, int32_t n_types,
                        const int32_t* type_ids, uint64_t seed, int32_t padded_size, int32_t mode, bool check_ranges) {
  ts = TypeSampler{id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode};
  if (!id_to_type || !type_offsets || !type_ids) return GE_EINVAL;
  return check_ranges && !sampler_ranges_ok(ts) ? GE_EINVAL : 0;
}

// validation tick workspace, K = 0 (hinge) or the negative ratio: (K > 0: sumsq 256 B) | pos [B,3] | neg [B,3] |
// loss [(1+K)B] | flag
struct TickWs { float* sumsq; int32_t* pos; int32_t* neg; float* loss; int32_t* flag; size_t bytes; };
static TickWs tick_ws(void* base, int64_t B, int64_t K) {
  const size_t lead = K > 0 ? 256 : 0, b = (size_t)B;
  return TickWs{ws_at<float>(base, 0), ws_at<int32_t>(base, lead), ws_at<int32_t>(base, lead + 12 * b),
                ws_at<float>(base, lead + 24 * b), ws_at<int32_t>(base, lead + 24 * b + 4 * (size_t)(1 + K) * b),
                (b * (3 + 3 + 1 + (size_t)K) * 4 + 16 + 255) / 256 * 256 + lead};
}
size_t ge_validation_workspace_bytes(int64_t B) { return B <= 0 ? 0 : tick_ws(nullptr, B, 0).bytes; }
size_t ge_validation_logloss_workspace_bytes(int64_t B, int32_t negative_ratio) {
  return (B <= 0 || negative_ratio < 1) ? 0 : tick_ws(nullptr, B, negative_ratio).bytes;
}
// first half of both ticks, behind the entry point's own shape and table checks: the remaining pointers, the workspace
// carved and its size tested, the batch drawn into w.pos
static int tick_head(TickWs& w, const int32_t* valid, int64_t V, int64_t B, int64_t K, uint64_t seed, uint64_t counter,
                     void* workspace, size_t workspace_bytes, const float* mean_out, const float* best, hipStream_t st) {
  if (!valid || !workspace || !mean_out || !best) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  w = tick_ws(workspace, B, K);
  if (workspace_bytes < w.bytes) return GE_ENOMEM;
  return select_rows_launch(valid, V, B, seed, counter, w.pos, st);
}
// second half: the mean of the M losses into the history, the pocket kept iff it is the best so far
static int tick_tail(const TickWs& w, int64_t M, const float* table, int64_t N, int32_t d, float* mean_out, float* best,
                     float* pocket, hipStream_t st) {
  const int rc = mean_pocket_launch(w.loss, M, mean_out, best, w.flag, st);
  if (rc || !pocket) return rc;
  return copy_if_launch(table, pocket, N * (int64_t)d, w.flag, st);
}

int ge_validation_tick(const float* table, int64_t N, int32_t d, const int32_t* valid, int64_t V, int64_t B,
                       const int32_t* id_to_type, const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids,
                       uint64_t seed, uint64_t counter, int32_t padded_size, int32_t mode, float margin, float max_norm,
                       int model, void* workspace, size_t workspace_bytes, float* mean_out, float* best, float* pocket,
                       void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TypeSampler ts;
  TickWs w;
  if (B <= 0 || V <= 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || model < 0 || model > 2) return GE_EINVAL;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, false)) return GE_EINVAL;
  int rc = tick_head(w, valid, V, B, 0, seed, counter, workspace, workspace_bytes, mean_out, best, st);
  if (rc) return rc;
  rc = corrupt_batch_launch(w.pos, B, ts, counter, w.neg, st);
  if (rc) return rc;
  rc = ge_hinge_loss(table, N, d, w.pos, w.neg, B, margin, max_norm, model, w.loss, nullptr, stream);
  if (rc) return rc;
  return tick_tail(w, B, table, N, d, mean_out, best, pocket, st);
}

// the same tick for the --log_loss objective (holE.py:194-196, 206-220 on a validation batch): positives with
// label +1, K corrupted batches with label -1, every loss plus l2 * l2_loss(table)
int ge_validation_tick_logloss(const float* table, int64_t N, int32_t d, const int32_t* valid, int64_t V, int64_t B,
                               const int32_t* id_to_type, const int64_t* type_offsets, int32_t n_types,
                               const int32_t* type_ids, uint64_t seed, uint64_t counter, int32_t padded_size, int32_t mode,
                               int32_t negative_ratio, float l2, float max_norm, void* workspace, size_t workspace_bytes,
                               float* mean_out, float* best, float* pocket, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t K = negative_ratio;
  TypeSampler ts;
  TickWs w;
  if (B <= 0 || V <= 0 || negative_ratio < 1 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, false)) return GE_EINVAL;
  int rc = tick_head(w, valid, V, B, K, seed, counter, workspace, workspace_bytes, mean_out, best, st);
  if (rc) return rc;
  rc = table_sumsq_launch(table, N * (int64_t)d, w.sumsq, st);
  if (rc) return rc;
  rc = complex_score_launch(table, N, d, w.pos, B, max_norm, 2, w.loss, st, 0, 1.0f, l2, w.sumsq);
  if (rc) return rc;
  for (int64_t k = 0; k < K; ++k) {
    rc = corrupt_batch_launch(w.pos, B, ts, counter * (uint64_t)K + (uint64_t)k, w.neg, st);
    if (rc) return rc;
    rc = complex_score_launch(table, N, d, w.neg, B, max_norm, 2, w.loss + (1 + k) * B, st, 0, -1.0f, l2, w.sumsq);
    if (rc) return rc;
  }
  return tick_tail(w, (1 + K) * B, table, N, d, mean_out, best, pocket, st);
}

int ge_hinge_grad(const float* rows, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                  int64_t B, float margin, float lr, float max_norm, int model, float* loss,
                  int32_t* grad_idx, float* grad_val, void* stream) {
  if (B < 0 || !ok_table(rows, N, d) || !max_norm_ok(max_norm) || model < 0 || model > 2) return GE_EINVAL;
  if (B > 0 && (!pos || !neg || !loss || !grad_idx || !grad_val)) return GE_EINVAL;
  if (model != GE_MODEL_HOLE)
    return complex_hinge_grad_launch(rows, N, d, pos, neg, B, margin, lr, max_norm, loss, grad_idx, grad_val, (hipStream_t)stream,
                                     nullptr, nullptr, nullptr, nullptr, model == GE_MODEL_HOLE_SPECTRAL);
  return hole_hinge_grad_launch(rows, N, d, pos, neg, B, margin, lr, max_norm, loss, grad_idx, grad_val, (hipStream_t)stream);
}

int ge_scatter_add_rows(float* table, int64_t N, int32_t d, const int32_t* idx, const float* val,
                        int64_t R, void* stream) {
  if (R < 0 || !ok_table(table, N, d)) return GE_EINVAL;
  if (R > 0 && (!idx || !val)) return GE_EINVAL;
  return scatter_add_rows_launch(table, N, d, idx, val, R, (hipStream_t)stream);
}

// [a, a + n floats) and [b, b + n floats) share a byte
static inline bool rows_overlap(const float* a, const float* b, int64_t N, int32_t d) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  const uintptr_t n = (uintptr_t)N * (uintptr_t)d * sizeof(float);
  return x < y + n && y < x + n;
}

int ge_adagrad_rows(float* table, float* accum, int64_t N, int32_t d, const int32_t* idx, const float* val,
                    const int32_t* perm, int64_t R, float lr, void* stream) {
  if (R < 0 || !ok_table(table, N, d) || !accum) return GE_EINVAL;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(accum)) % 4 != 0) return GE_EINVAL;
  if (rows_overlap(table, accum, N, d)) return GE_EINVAL;
  if (R == 0) return 0;
  if (!idx || !val || !perm) return GE_EINVAL;
  return adagrad_rows_launch(table, accum, N, d, idx, val, perm, R, lr, (hipStream_t)stream);
}

static inline bool softmax_dim_ok(int32_t d) { return d >= 8 && d <= kRankMaxDim && d % 8 == 0; }

size_t ge_softmax_workspace_bytes(int64_t B, int64_t K, int32_t d) {
  if (B < 1 || K < 1 || !softmax_dim_ok(d)) return 0;
  return softmax_ws_bytes(B, K, d);
}

// the one check of the six softmax entry points; grad: the gradient outputs are asked for; sampled: ge_softmax_sampled_*;
// sets: ge_softmax_masked_* (its pointers and n_sets join the GE_EINVAL groups, its size function is the one checked)
static int softmax_call(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                        const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model, int cand_is_head,
                        float* loss, bool grad, int32_t* grad_idx, float* grad_val, void* workspace, size_t workspace_bytes,
                        void* stream, bool sampled = false, const SetArgs* sets = nullptr) {
  if (B < 1 || K < 1 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || !(scale > 0.f) || !std::isfinite(scale))
    return GE_EINVAL;
  if (!hr || !true_id || !cand || !loss || !workspace || (grad && (!grad_idx || !grad_val))) return GE_EINVAL;
  if (sets && (!sets->row_set || !sets->mask || sets->n_sets < 1)) return GE_EINVAL;
  if (model != GE_MODEL_COMPLEX || !softmax_dim_ok(d)) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(table) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (grad && reinterpret_cast<uintptr_t>(grad_val) % 4 != 0) return GE_EINVAL;
  if (sets && reinterpret_cast<uintptr_t>(sets->mask) % 4 != 0) return GE_EINVAL;
  if (sets) {
    if (workspace_bytes < softmax_masked_ws_bytes(B, K, d)) return GE_ENOMEM;
    return softmax_masked_launch(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, cand_is_head, loss,
                                 grad ? grad_idx : nullptr, grad_val, workspace, *sets, (hipStream_t)stream);
  }
  if (workspace_bytes < (sampled ? softmax_sampled_ws_bytes(B, K, d) : softmax_ws_bytes(B, K, d))) return GE_ENOMEM;
  if (sampled)
    return softmax_sampled_launch(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, cand_is_head, loss,
                                  grad ? grad_idx : nullptr, grad_val, workspace, (hipStream_t)stream);
  return softmax_launch(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, cand_is_head, loss,
                        grad ? grad_idx : nullptr, grad_val, workspace, (hipStream_t)stream);
}

int ge_softmax_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                    const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                    float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, 0.f, model, cand_is_head, loss, false, nullptr,
                      nullptr, workspace, workspace_bytes, stream);
}

int ge_softmax_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                    const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model, int cand_is_head,
                    float* loss, int32_t* grad_idx, float* grad_val, void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, model, cand_is_head, loss, true, grad_idx,
                      grad_val, workspace, workspace_bytes, stream);
}

size_t ge_softmax_sampled_workspace_bytes(int64_t B, int64_t K, int32_t d) {
  if (B < 1 || K < 1 || !softmax_dim_ok(d)) return 0;
  return softmax_sampled_ws_bytes(B, K, d);
}

int ge_softmax_sampled_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                            const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                            float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, 0.f, model, cand_is_head, loss, false, nullptr,
                      nullptr, workspace, workspace_bytes, stream, true);
}

int ge_softmax_sampled_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                            const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model,
                            int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, model, cand_is_head, loss, true, grad_idx,
                      grad_val, workspace, workspace_bytes, stream, true);
}

size_t ge_softmax_masked_workspace_bytes(int64_t B, int64_t K, int32_t d) {
  if (B < 1 || K < 1 || !softmax_dim_ok(d)) return 0;
  return softmax_masked_ws_bytes(B, K, d);
}

int ge_softmax_masked_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                           float* loss, void* workspace, size_t workspace_bytes, const int32_t* row_set,
                           const uint32_t* mask, int32_t n_sets, void* stream) {
  const SetArgs sets{row_set, mask, n_sets, 0};
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, 0.f, model, cand_is_head, loss, false, nullptr,
                      nullptr, workspace, workspace_bytes, stream, false, &sets);
}

int ge_softmax_masked_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model,
                           int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                           size_t workspace_bytes, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                           void* stream) {
  const SetArgs sets{row_set, mask, n_sets, 0};
  return softmax_call(table, N, d, hr, B, true_id, cand, K, max_norm, scale, lr, model, cand_is_head, loss, true, grad_idx,
                      grad_val, workspace, workspace_bytes, stream, false, &sets);
}

size_t ge_softmax_labels_workspace_bytes(int64_t B, int64_t K, int32_t d, int64_t L) {
  if (B < 1 || K < 1 || L < 0 || !softmax_dim_ok(d)) return 0;
  return softmax_labels_ws_bytes(B, K, d, L);
}

// softmax_call's checks, in its order, with the labels' arguments in their groups
static int softmax_labels_call(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                               const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                               float lr, int model, int cand_is_head, float* loss, bool grad, int32_t* grad_idx, float* grad_val,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || K < 1 || L < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || !(scale > 0.f) || !std::isfinite(scale))
    return GE_EINVAL;
  if (!hr || !label_off || !label_pos || !cand || !loss || !workspace || (grad && (!grad_idx || !grad_val))) return GE_EINVAL;
  if (model != GE_MODEL_COMPLEX || !softmax_dim_ok(d) || N > INT32_MAX) return GE_ENOTSUP;
  if (reinterpret_cast<uintptr_t>(table) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (grad && reinterpret_cast<uintptr_t>(grad_val) % 4 != 0) return GE_EINVAL;
  if (workspace_bytes < softmax_labels_ws_bytes(B, K, d, L)) return GE_ENOMEM;
  return softmax_labels_launch(table, N, d, hr, B, label_off, label_pos, L, cand, K, max_norm, scale, lr, cand_is_head, loss,
                               grad ? grad_idx : nullptr, grad_val, workspace, (hipStream_t)stream);
}

int ge_softmax_labels_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                           const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                           int model, int cand_is_head, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_labels_call(table, N, d, hr, B, label_off, label_pos, L, cand, K, max_norm, scale, 0.f, model, cand_is_head,
                             loss, false, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int ge_softmax_labels_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                           const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                           float lr, int model, int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val,
                           void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_labels_call(table, N, d, hr, B, label_off, label_pos, L, cand, K, max_norm, scale, lr, model, cand_is_head,
                             loss, true, grad_idx, grad_val, workspace, workspace_bytes, stream);
}

int ge_gather_rows(const float* table, int64_t N, int32_t d, const int32_t* idx, int64_t R, float* out,
                   void* stream) {
  if (R < 0 || !ok_table(table, N, d)) return GE_EINVAL;
  if (R > 0 && (!idx || !out)) return GE_EINVAL;
  return gather_rows_launch(table, N, d, idx, R, out, (hipStream_t)stream);
}

size_t ge_hinge_step_workspace_bytes(int64_t B, int32_t d) {
  if (B <= 0 || d <= 0) return 0;
  return hinge_ws(nullptr, B, d).bytes;
}

size_t ge_train_workspace_bytes(int64_t B, int32_t d) {
  if (B <= 0 || d <= 0) return 0;
  return train_ws_bytes(B, d);
}

static int hinge_step(float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg, int64_t B,
                      float margin, float lr, float max_norm, int model, float* loss, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (B < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (B == 0) return 0;
  if (!pos || !neg || !loss || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  const HingeWs w = hinge_ws(workspace, B, d);
  if (workspace_bytes < w.bytes) return GE_ENOMEM;
  int rc = ge_hinge_grad(table, N, d, pos, neg, B, margin, lr, max_norm, model, loss, w.gidx, w.gval, stream);
  if (rc != 0) return rc;
  return scatter_add_rows_launch(table, N, d, w.gidx, w.gval, 6 * B, (hipStream_t)stream);
}

int ge_complex_hinge_step(float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                          int64_t B, float margin, float lr, float max_norm, float* loss, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return hinge_step(table, N, d, pos, neg, B, margin, lr, max_norm, 0, loss, workspace, workspace_bytes, stream);
}

int ge_hole_hinge_step(float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                       int64_t B, float margin, float lr, float max_norm, float* loss, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return hinge_step(table, N, d, pos, neg, B, margin, lr, max_norm, 1, loss, workspace, workspace_bytes, stream);
}

int ge_corrupt_batch(const int32_t* pos, int64_t B, const int32_t* id_to_type, int64_t N,
                     const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids, uint64_t seed,
                     uint64_t step, int32_t padded_size, int32_t mode, int32_t* neg, void* stream) {
  TypeSampler ts;
  if (B < 0 || N <= 0 || type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, false))
    return GE_EINVAL;
  if (B > 0 && (!pos || !neg)) return GE_EINVAL;
  return corrupt_batch_launch(pos, B, ts, step, neg, (hipStream_t)stream);
}

int ge_bernoulli_corrupt_batch(const int32_t* pos, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                               const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                               const uint32_t* tail_threshold, int32_t n_rel, int32_t ent_lo, int32_t n_ent,
                               uint64_t seed, uint64_t step, int32_t* neg, void* stream) {
  if (B < 0 || !tail_threshold) return GE_EINVAL;
  if (n_known > 0 && (!bh_key || !bh_ent || !bt_key || !bt_ent)) return GE_EINVAL;
  if (B > 0 && (!pos || !neg)) return GE_EINVAL;
  const SamplerArgs s{nullptr, 0, bh_key, bh_ent, bt_key, bt_ent, n_known, tail_threshold, n_rel, n_ent};
  return bernoulli_corrupt_launch(pos, B, s, ent_lo, seed, step, neg, (hipStream_t)stream);
}

// ---------------------------------------------------------------- translation models: the descriptor (ge_trans.h)
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static inline bool sweep_batch_ok(int64_t B) { return B > 0 && B <= ((int64_t)1 << 28); }
// TransE / TransH / TransD: shapes and the model's tables checked, m filled.  Every table the model has is present,
// every table given 4-byte aligned, ids fit the sort's 32-bit keys.
static int transx_model(TransModel& m, int model, int l1, const float* ent, int64_t E, const float* rel, int64_t R,
                        const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d) {
  if (model < GE_TRANSX_TRANSE || model > GE_TRANSX_TRANSD) return GE_EINVAL;
  if (!ent || !rel || E <= 0 || R <= 0 || E + R >= ((int64_t)1 << 31)) return GE_EINVAL;
  if (d <= 0) return GE_EINVAL;
  if (d > transx_max_dim()) return GE_ENOTSUP;
  if (model == GE_TRANSX_TRANSH && !normal) return GE_EINVAL;
  if (model == GE_TRANSX_TRANSD && (!ent_transfer || !rel_transfer)) return GE_EINVAL;
  for (const void* p : {ent, rel, normal, ent_transfer, rel_transfer})
    if (p && !aligned4(p)) return GE_EINVAL;
  m = TransModel{model, l1, ent, rel, normal, ent_transfer, rel_transfer, nullptr, E, R, d, d};
  return 0;
}
// TransR: tables present and 4-byte aligned, dimensions in range, entity and relation ids fit the sorts' 32-bit keys
static int transr_model(TransModel& m, int l1, const float* ent, int64_t E, const float* rel, const float* rel_matrix,
                        int64_t R, int32_t dE, int32_t dR) {
  if (!ent || !rel || !rel_matrix || E <= 0 || R <= 0 || E >= ((int64_t)1 << 31) || R >= ((int64_t)1 << 31))
    return GE_EINVAL;
  if (dE <= 0 || dR <= 0) return GE_EINVAL;
  if (dE > transr_max_dim() || dR > transr_max_dim()) return GE_ENOTSUP;
  for (const void* p : {ent, rel, rel_matrix})
    if (!aligned4(p)) return GE_EINVAL;
  m = TransModel{kTransR, l1, ent, rel, nullptr, nullptr, nullptr, rel_matrix, E, R, dE, dR};
  return 0;
}
// The shape test of the six sweep size functions: m filled with the shape alone (model kTransR, which only the
// ge_transr_* sizes pass: dE x dq, else an ABI model code and dE = dq = d).  id_limits: the tables' limit on the counts (TransX n_ent + n_rel < 2^31, TransR each < 2^31).  Only the
// relation-rank sizes apply it; the rank and top-k sizes never did and answer for counts their entry points refuse.
// Kept as it was: aligning them changes what callers see.
static bool sweep_shape(TransModel& m, bool tr, int model, int64_t E, int64_t R, int32_t dE, int32_t dq, int64_t B,
                        bool id_limits) {
  const int dmax = tr ? transr_max_dim() : transx_max_dim();
  if (!tr && (model < GE_TRANSX_TRANSE || model > GE_TRANSX_TRANSD)) return false;
  if (E <= 0 || R <= 0 || dE <= 0 || dq <= 0 || dE > dmax || dq > dmax || !sweep_batch_ok(B)) return false;
  if (id_limits && (tr ? E >= ((int64_t)1 << 31) || R >= ((int64_t)1 << 31) : E + R >= ((int64_t)1 << 31))) return false;
  m = TransModel{model, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, E, R, dE, dq};
  return true;
}

// ---------------------------------------------------------------- TransE / TransH / TransD
static inline bool transx_batch_ok(int64_t B) { return B > 0 && B <= ((int64_t)1 << 31) / 5 - 1; }
// the triples and Bernoulli tables a draw reads, checked and s filled: T rows fit its 32-bit row pick, the four arrays
// are there when n_known > 0
static inline bool sampler_ok(SamplerArgs& s, const int32_t* triples, int64_t T, const uint32_t* tail_threshold,
                              int64_t n_known, const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key,
                              const int32_t* bt_ent, int32_t n_rel, int32_t n_ent) {
  s = SamplerArgs{triples, T, bh_key, bh_ent, bt_key, bt_ent, n_known, tail_threshold, n_rel, n_ent};
  return triples && T > 0 && T <= ((int64_t)1 << 32) && tail_threshold && n_known >= 0 &&
         (n_known == 0 || (bh_key && bh_ent && bt_key && bt_ent));
}

int ge_transx_max_dim(void) { return transx_max_dim(); }

int ge_transx_score(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                    const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                    const int32_t* triples, int64_t B, float* out, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (B < 0) return GE_EINVAL;
  if (B > 0 && (!triples || !out || !aligned4(triples) || !aligned4(out))) return GE_EINVAL;
  return transx_score_launch(m, triples, B, out, (hipStream_t)stream);
}

size_t ge_transx_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B) {
  if (n_ent <= 0 || n_rel <= 0 || d <= 0 || d > transx_max_dim() || !transx_batch_ok(B)) return 0;
  return transx_ws_bytes(n_ent, n_rel, d, B);
}

int ge_transx_hinge_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                         float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* neg,
                         int64_t B, float margin, float lr, float* loss, void* workspace, size_t workspace_bytes,
                         void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (!transx_batch_ok(B) || !pos || !neg || !loss || !workspace) return GE_EINVAL;
  if (!aligned4(pos) || !aligned4(neg) || !aligned4(loss) || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  return transx_hinge_step_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d, pos, neg, B,
                               margin, lr, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_transx_draw_batch(const int32_t* triples, int64_t T, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                         const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold,
                         int32_t n_rel, int32_t n_ent, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg,
                         void* stream) {
  SamplerArgs s;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, n_rel, n_ent)) return GE_EINVAL;
  if (B < 0 || n_rel <= 0 || n_ent <= 0 || (B > 0 && (!pos || !neg))) return GE_EINVAL;
  return transx_draw_launch(s, B, seed, step, pos, neg, (hipStream_t)stream);
}

int ge_transx_train_steps(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                          float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* triples, int64_t T,
                          const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                          int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                          int64_t n_steps, int64_t B, float margin, float lr, float* losses, void* workspace,
                          size_t workspace_bytes, void* stream) {
  TransModel m;
  SamplerArgs s;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (!transx_batch_ok(B) || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return transx_train_steps_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d, s, seed,
                                first_step, n_steps, B, margin, lr, losses, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

// The accumulators of an AdaGrad step, after transx_model: every table the model has brings its accumulator, 4-byte
// aligned, whose [rows * d] floats share no byte with a table of the model or with another accumulator.  An accumulator
// of a table the model does not have is dropped (as its table is ignored).
static int transx_accs(TransAccs& c, const TransModel& m, float* acc_ent, float* acc_rel, float* acc_normal,
                       float* acc_ent_transfer, float* acc_rel_transfer) {
  struct Span { const float* p; int64_t rows; };
  const Span tabs[5] = {{m.ent, m.E}, {m.rel, m.R}, {m.model == kTransH ? m.normal : nullptr, m.R},
                        {m.model == kTransD ? m.ent_transfer : nullptr, m.E}, {m.model == kTransD ? m.rel_transfer : nullptr, m.R}};
  const float* given[5] = {acc_ent, acc_rel, acc_normal, acc_ent_transfer, acc_rel_transfer};
  Span accs[5];
  for (int i = 0; i < 5; ++i) accs[i] = Span{tabs[i].p ? given[i] : nullptr, tabs[i].rows};
  for (int i = 0; i < 5; ++i)
    if (tabs[i].p && !accs[i].p) return GE_EINVAL;
  for (int i = 0; i < 5; ++i)
    if (accs[i].p && !aligned4(accs[i].p)) return GE_EINVAL;
  auto overlap = [&](const Span& a, const Span& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    const uintptr_t nx = (uintptr_t)a.rows * (uintptr_t)m.dE * sizeof(float), ny = (uintptr_t)b.rows * (uintptr_t)m.dE * sizeof(float);
    return x < y + ny && y < x + nx;
  };
  for (int i = 0; i < 5; ++i) {
    if (!accs[i].p) continue;
    for (int k = 0; k < 5; ++k) {
      if (tabs[k].p && overlap(accs[i], tabs[k])) return GE_EINVAL;
      if (k > i && accs[k].p && overlap(accs[i], accs[k])) return GE_EINVAL;
    }
  }
  c = TransAccs{(float*)accs[0].p, (float*)accs[1].p, (float*)accs[2].p, (float*)accs[3].p, (float*)accs[4].p};
  return 0;
}

int ge_transx_adagrad_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                           float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel, float* acc_normal,
                           float* acc_ent_transfer, float* acc_rel_transfer, int32_t d, const int32_t* pos,
                           const int32_t* neg, int64_t B, float margin, float lr, float* loss, void* workspace,
                           size_t workspace_bytes, void* stream) {
  TransModel m;
  TransAccs c;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = transx_accs(c, m, acc_ent, acc_rel, acc_normal, acc_ent_transfer, acc_rel_transfer)) return rc;
  if (!transx_batch_ok(B) || !pos || !neg || !loss || !workspace) return GE_EINVAL;
  if (!aligned4(pos) || !aligned4(neg) || !aligned4(loss) || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  return transx_adagrad_step_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, c, d, pos, neg,
                                 B, margin, lr, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_transx_train_steps_adagrad(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                                  float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel,
                                  float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer, int32_t d,
                                  const int32_t* triples, int64_t T, const int64_t* bh_key, const int32_t* bh_ent,
                                  const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                                  const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                                  int64_t B, float margin, float lr, float* losses, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  TransModel m;
  TransAccs c;
  SamplerArgs s;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = transx_accs(c, m, acc_ent, acc_rel, acc_normal, acc_ent_transfer, acc_rel_transfer)) return rc;
  if (!transx_batch_ok(B) || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return transx_train_steps_adagrad_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, c, d, s,
                                        seed, first_step, n_steps, B, margin, lr, losses, workspace, workspace_bytes,
                                        (hipStream_t)stream);
}

// ---------------------------------------------------------------- RotatE
// The shape and the two tables checked, in transx_model's order: present, sizes >= 1, ids fit the sort's 32-bit keys
// (GE_EINVAL); d even and at most rotate_max_dim() (GE_ENOTSUP); 4-byte aligned (GE_EINVAL).
static int rotate_model(const float* ent, int64_t E, const float* rel, int64_t R, int32_t d) {
  if (!ent || !rel || E <= 0 || R <= 0 || E + R >= ((int64_t)1 << 31)) return GE_EINVAL;
  if (d <= 0) return GE_EINVAL;
  if (d % 2 || d > rotate_max_dim()) return GE_ENOTSUP;
  if (!aligned4(ent) || !aligned4(rel)) return GE_EINVAL;
  return 0;
}
// The two accumulators of an AdaGrad step, after rotate_model: present, 4-byte aligned, and their [E, d] and [R, d / 2]
// floats share no byte with a table or with each other.
static int rotate_accs(const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const float* acc_ent,
                       const float* acc_rel) {
  if (!acc_ent || !acc_rel || !aligned4(acc_ent) || !aligned4(acc_rel)) return GE_EINVAL;
  struct Span { uintptr_t p, n; };
  const uintptr_t ne = (uintptr_t)E * (uintptr_t)d * sizeof(float), nr = (uintptr_t)R * (uintptr_t)(d / 2) * sizeof(float);
  const Span tabs[2] = {{(uintptr_t)ent, ne}, {(uintptr_t)rel, nr}}, accs[2] = {{(uintptr_t)acc_ent, ne}, {(uintptr_t)acc_rel, nr}};
  auto overlap = [](const Span& a, const Span& b) { return a.p < b.p + b.n && b.p < a.p + a.n; };
  for (const Span& a : accs)
    for (const Span& t : tabs)
      if (overlap(a, t)) return GE_EINVAL;
  return overlap(accs[0], accs[1]) ? GE_EINVAL : 0;
}
static int rotate_step_args_ok(int64_t B, const int32_t* pos, const int32_t* neg, const float* loss, const void* workspace) {
  if (!transx_batch_ok(B) || !pos || !neg || !loss || !workspace) return GE_EINVAL;
  if (!aligned4(pos) || !aligned4(neg) || !aligned4(loss) || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  return 0;
}

int ge_rotate_max_dim(void) { return rotate_max_dim(); }

int ge_rotate_score(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                    const int32_t* triples, int64_t B, float* out, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (B < 0) return GE_EINVAL;
  if (B > 0 && (!triples || !out || !aligned4(triples) || !aligned4(out))) return GE_EINVAL;
  return rotate_score_launch(l1, ent, n_ent, rel, n_rel, d, triples, B, out, (hipStream_t)stream);
}

size_t ge_rotate_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B) {
  if (n_ent <= 0 || n_rel <= 0 || d <= 0 || d % 2 || d > rotate_max_dim() || !transx_batch_ok(B)) return 0;
  return rotate_ws_bytes(n_ent, n_rel, d, B);
}

int ge_rotate_hinge_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* pos,
                         const int32_t* neg, int64_t B, float margin, float lr, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_step_args_ok(B, pos, neg, loss, workspace)) return rc;
  return rotate_step_run(l1, ent, n_ent, rel, n_rel, nullptr, nullptr, d, pos, neg, B, margin, lr, loss, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_adagrad_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent, float* acc_rel,
                           int32_t d, const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr,
                           float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_accs(ent, n_ent, rel, n_rel, d, acc_ent, acc_rel)) return rc;
  if (int rc = rotate_step_args_ok(B, pos, neg, loss, workspace)) return rc;
  return rotate_step_run(l1, ent, n_ent, rel, n_rel, acc_ent, acc_rel, d, pos, neg, B, margin, lr, loss, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_train_steps(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* triples,
                          int64_t T, const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key,
                          const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold, uint64_t seed,
                          uint64_t first_step, int64_t n_steps, int64_t B, float margin, float lr, float* losses,
                          void* workspace, size_t workspace_bytes, void* stream) {
  SamplerArgs s;
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (!transx_batch_ok(B) || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return rotate_train_steps_run(l1, ent, n_ent, rel, n_rel, nullptr, nullptr, d, s, seed, first_step, n_steps, B, margin,
                                lr, losses, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_train_steps_adagrad(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                                  float* acc_rel, int32_t d, const int32_t* triples, int64_t T, const int64_t* bh_key,
                                  const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                                  const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                                  int64_t B, float margin, float lr, float* losses, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  SamplerArgs s;
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_accs(ent, n_ent, rel, n_rel, d, acc_ent, acc_rel)) return rc;
  if (!transx_batch_ok(B) || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return rotate_train_steps_run(l1, ent, n_ent, rel, n_rel, acc_ent, acc_rel, d, s, seed, first_step, n_steps, B, margin,
                                lr, losses, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------- RotatE, the self-adversarial loss
// What this loss adds to a step's or a loop's refusals, after the tables (and accumulators) and in front of the batch,
// the output and the workspace checks, in this order: K < 1 (GE_EINVAL), K > the maximum (GE_ENOTSUP), (K + 3) B >= 2^31
// (GE_EINVAL), then -- where the call takes them (rows = true) -- a null side or neg_ent (GE_EINVAL), a margin or alpha
// that is not finite, alpha < 0 (GE_EINVAL).
static inline bool adv_count_ok(int64_t B, int32_t K) { return B <= (((int64_t)1 << 31) - 1) / ((int64_t)K + 3); }
static int rotate_adv_args(int32_t K, int64_t B, bool rows, const int32_t* side, const int32_t* neg_ent, float margin,
                           float alpha) {
  if (K < 1) return GE_EINVAL;
  if (K > rotate_adv_max_negatives()) return GE_ENOTSUP;
  if (!adv_count_ok(B, K)) return GE_EINVAL;
  if (rows && (!side || !neg_ent)) return GE_EINVAL;
  if (!std::isfinite(margin) || !std::isfinite(alpha) || alpha < 0.f) return GE_EINVAL;
  return 0;
}
static int rotate_adv_step_args_ok(int64_t B, const int32_t* pos, const int32_t* side, const int32_t* neg_ent,
                                   const float* loss, const void* workspace) {
  if (B <= 0 || !pos || !loss || !workspace) return GE_EINVAL;
  if (!aligned4(pos) || !aligned4(side) || !aligned4(neg_ent) || !aligned4(loss) || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  return 0;
}

int ge_rotate_adv_max_negatives(void) { return rotate_adv_max_negatives(); }

size_t ge_rotate_adv_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t K) {
  if (n_ent <= 0 || n_rel <= 0 || d <= 0 || d % 2 || d > rotate_max_dim() || B <= 0) return 0;
  if (K < 1 || K > rotate_adv_max_negatives() || !adv_count_ok(B, K)) return 0;
  return rotate_adv_ws_bytes(n_ent, n_rel, d, B, K);
}

int ge_rotate_adv_loss(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                       const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                       float margin, float alpha, float* out, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_adv_args(K, B, B > 0, side, neg_ent, margin, alpha)) return rc;
  if (B < 0) return GE_EINVAL;
  if (B > 0 && (!pos || !out || !aligned4(pos) || !aligned4(side) || !aligned4(neg_ent) || !aligned4(out))) return GE_EINVAL;
  return rotate_adv_loss_launch(l1, ent, n_ent, rel, n_rel, d, pos, side, neg_ent, B, K, margin, alpha, out,
                                (hipStream_t)stream);
}

int ge_rotate_adv_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* pos,
                       const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha,
                       float lr, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_adv_args(K, B, true, side, neg_ent, margin, alpha)) return rc;
  if (int rc = rotate_adv_step_args_ok(B, pos, side, neg_ent, loss, workspace)) return rc;
  return rotate_adv_step_run(l1, ent, n_ent, rel, n_rel, nullptr, nullptr, d, pos, side, neg_ent, B, K, margin, alpha, lr,
                             loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_adv_adagrad_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                               float* acc_rel, int32_t d, const int32_t* pos, const int32_t* side,
                               const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr,
                               float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_accs(ent, n_ent, rel, n_rel, d, acc_ent, acc_rel)) return rc;
  if (int rc = rotate_adv_args(K, B, true, side, neg_ent, margin, alpha)) return rc;
  if (int rc = rotate_adv_step_args_ok(B, pos, side, neg_ent, loss, workspace)) return rc;
  return rotate_adv_step_run(l1, ent, n_ent, rel, n_rel, acc_ent, acc_rel, d, pos, side, neg_ent, B, K, margin, alpha, lr,
                             loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_adv_draw_batch(const int32_t* triples, int64_t T, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                             const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                             const uint32_t* tail_threshold, int32_t n_rel, int32_t n_ent, uint64_t seed, uint64_t step,
                             int32_t K, int32_t* pos, int32_t* side, int32_t* neg_ent, void* stream) {
  SamplerArgs s;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, n_rel, n_ent)) return GE_EINVAL;
  if (B < 0 || n_rel <= 0 || n_ent <= 0) return GE_EINVAL;
  if (K < 1) return GE_EINVAL;
  if (K > rotate_adv_max_negatives()) return GE_ENOTSUP;
  if (!adv_count_ok(B, K) || (B > 0 && (!pos || !side || !neg_ent))) return GE_EINVAL;
  return rotate_adv_draw_launch(s, B, K, seed, step, pos, side, neg_ent, (hipStream_t)stream);
}

int ge_rotate_adv_train_steps(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d,
                              const int32_t* triples, int64_t T, const int64_t* bh_key, const int32_t* bh_ent,
                              const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                              const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                              int64_t B, int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                              size_t workspace_bytes, void* stream) {
  SamplerArgs s;
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_adv_args(K, B, false, nullptr, nullptr, margin, alpha)) return rc;
  if (B <= 0 || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return rotate_adv_train_steps_run(l1, ent, n_ent, rel, n_rel, nullptr, nullptr, d, s, seed, first_step, n_steps, B, K,
                                    margin, alpha, lr, losses, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_rotate_adv_train_steps_adagrad(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                                      float* acc_rel, int32_t d, const int32_t* triples, int64_t T,
                                      const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key,
                                      const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold,
                                      uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B, int32_t K,
                                      float margin, float alpha, float lr, float* losses, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  SamplerArgs s;
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  if (int rc = rotate_accs(ent, n_ent, rel, n_rel, d, acc_ent, acc_rel)) return rc;
  if (int rc = rotate_adv_args(K, B, false, nullptr, nullptr, margin, alpha)) return rc;
  if (B <= 0 || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return rotate_adv_train_steps_run(l1, ent, n_ent, rel, n_rel, acc_ent, acc_rel, d, s, seed, first_step, n_steps, B, K,
                                    margin, alpha, lr, losses, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------- TransE / TransH / TransD, the self-adversarial loss
// rotate_adv_args' checks and order between the model (and accumulators) and the batch; the draw is RotatE's.
size_t ge_transx_adv_step_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t K) {
  if (model < GE_TRANSX_TRANSE || model > GE_TRANSX_TRANSD) return 0;
  if (n_ent <= 0 || n_rel <= 0 || d <= 0 || d > transx_max_dim() || B <= 0) return 0;
  if (K < 1 || K > transx_adv_max_negatives() || !adv_count_ok(B, K)) return 0;
  return transx_adv_ws_bytes(model, n_ent, n_rel, d, B, K);
}

int ge_transx_adv_max_negatives(void) { return transx_adv_max_negatives(); }

int ge_transx_adv_loss(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                       const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                       const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                       float margin, float alpha, float* out, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = rotate_adv_args(K, B, B > 0, side, neg_ent, margin, alpha)) return rc;
  if (B < 0) return GE_EINVAL;
  if (B > 0 && (!pos || !out || !aligned4(pos) || !aligned4(side) || !aligned4(neg_ent) || !aligned4(out))) return GE_EINVAL;
  return transx_adv_loss_launch(m, pos, side, neg_ent, B, K, margin, alpha, out, (hipStream_t)stream);
}

int ge_transx_adv_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                       float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* side,
                       const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr, float* loss,
                       void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = rotate_adv_args(K, B, true, side, neg_ent, margin, alpha)) return rc;
  if (int rc = rotate_adv_step_args_ok(B, pos, side, neg_ent, loss, workspace)) return rc;
  return transx_adv_step_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, nullptr, d, pos, side,
                             neg_ent, B, K, margin, alpha, lr, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_transx_adv_adagrad_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                               float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel,
                               float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer, int32_t d,
                               const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                               float margin, float alpha, float lr, float* loss, void* workspace, size_t workspace_bytes,
                               void* stream) {
  TransModel m;
  TransAccs c;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = transx_accs(c, m, acc_ent, acc_rel, acc_normal, acc_ent_transfer, acc_rel_transfer)) return rc;
  if (int rc = rotate_adv_args(K, B, true, side, neg_ent, margin, alpha)) return rc;
  if (int rc = rotate_adv_step_args_ok(B, pos, side, neg_ent, loss, workspace)) return rc;
  return transx_adv_step_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, &c, d, pos, side,
                             neg_ent, B, K, margin, alpha, lr, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_transx_adv_train_steps(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                              float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* triples, int64_t T,
                              const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                              int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                              int64_t n_steps, int64_t B, int32_t K, float margin, float alpha, float lr, float* losses,
                              void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  SamplerArgs s;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = rotate_adv_args(K, B, false, nullptr, nullptr, margin, alpha)) return rc;
  if (B <= 0 || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return transx_adv_train_steps_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, nullptr, d, s,
                                    seed, first_step, n_steps, B, K, margin, alpha, lr, losses, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}

int ge_transx_adv_train_steps_adagrad(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel,
                                      float* normal, float* ent_transfer, float* rel_transfer, float* acc_ent,
                                      float* acc_rel, float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer,
                                      int32_t d, const int32_t* triples, int64_t T, const int64_t* bh_key,
                                      const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                                      int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                                      int64_t n_steps, int64_t B, int32_t K, float margin, float alpha, float lr,
                                      float* losses, void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  TransAccs c;
  SamplerArgs s;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  if (int rc = transx_accs(c, m, acc_ent, acc_rel, acc_normal, acc_ent_transfer, acc_rel_transfer)) return rc;
  if (int rc = rotate_adv_args(K, B, false, nullptr, nullptr, margin, alpha)) return rc;
  if (B <= 0 || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return transx_adv_train_steps_run(model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, &c, d, s, seed,
                                    first_step, n_steps, B, K, margin, alpha, lr, losses, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}

// ---------------------------------------------------------------- TransR
// 4B entity slots and every sorted position fit an int32
static inline bool transr_batch_ok(int64_t B) { return sweep_batch_ok(B); }
static inline bool adam_ok(float b1, float b2, float eps, int64_t t, const void* m, const void* v) {
  return b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f && eps >= 0.f && t >= 1 && m && v && aligned4(m) && aligned4(v);
}

int ge_transr_max_dim(void) { return transr_max_dim(); }

int ge_transr_score(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                    int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B, float* out, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  if (B < 0) return GE_EINVAL;
  if (B > 0 && (!triples || !out || !aligned4(triples) || !aligned4(out))) return GE_EINVAL;
  return transr_score_launch(m, triples, B, out, (hipStream_t)stream);
}

size_t ge_transr_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B) {
  if (n_ent <= 0 || n_rel <= 0 || n_ent >= ((int64_t)1 << 31) || n_rel >= ((int64_t)1 << 31)) return 0;
  if (dim_e <= 0 || dim_r <= 0 || dim_e > transr_max_dim() || dim_r > transr_max_dim() || !transr_batch_ok(B)) return 0;
  return transr_ws_bytes(n_ent, n_rel, dim_e, dim_r, B);
}

int ge_transr_adam_step(int l1, float* ent, int64_t n_ent, float* rel, float* rel_matrix, int64_t n_rel, int32_t dim_e,
                        int32_t dim_r, float* m, float* v, const int32_t* pos, const int32_t* neg, int64_t B,
                        float margin, float lr, float b1, float b2, float eps, int64_t t, float* loss, void* workspace,
                        size_t workspace_bytes, void* stream) {
  TransModel tm;
  if (int rc = transr_model(tm, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  if (!transr_batch_ok(B) || !pos || !neg || !loss || !workspace || !adam_ok(b1, b2, eps, t, m, v)) return GE_EINVAL;
  if (!aligned4(pos) || !aligned4(neg) || !aligned4(loss) || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  return transr_adam_step_run(l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r, m, v, pos, neg, B, margin, lr, b1,
                              b2, eps, t, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ge_transr_train_steps(int l1, float* ent, int64_t n_ent, float* rel, float* rel_matrix, int64_t n_rel,
                          int32_t dim_e, int32_t dim_r, float* m, float* v, const int32_t* triples, int64_t T,
                          const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                          int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                          int64_t n_steps, int64_t B, float margin, float lr, float b1, float b2, float eps,
                          int64_t first_t, float* losses, void* workspace, size_t workspace_bytes, void* stream) {
  TransModel tm;
  SamplerArgs s;
  if (int rc = transr_model(tm, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  if (!transr_batch_ok(B) || n_steps < 0 || !losses || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (!adam_ok(b1, b2, eps, first_t, m, v)) return GE_EINVAL;
  if (!sampler_ok(s, triples, T, tail_threshold, n_known, bh_key, bh_ent, bt_key, bt_ent, (int32_t)n_rel, (int32_t)n_ent))
    return GE_EINVAL;
  return transr_train_steps_run(l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r, m, v, s, seed, first_step, n_steps,
                                B, margin, lr, b1, b2, eps, first_t, losses, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

// ---------------------------------------------------------------- translation-model sweeps: entity ranks, relation
// ranks, top-k.  Each has one body behind its TransX and its TransR entry point; the order inside is the tables (the
// entry point's transx_model / transr_model), the candidate sets where the entry point has them, the outputs, B == 0
// (returns 0), then the launcher's GE_ENOMEM.
// B rows of int32 counters, q rows of the workspace and the sweep's row-chunk grid all fit; the outputs are 4-byte
// aligned; the known lists come as a pair
static int rank_outputs_ok(int64_t B, const int32_t* triples, const RankOut& o, const void* workspace) {
  if (B < 0 || B > ((int64_t)1 << 28)) return GE_EINVAL;
  if ((o.known_off == nullptr) != (o.known_rc == nullptr)) return GE_EINVAL;
  if (B == 0) return 0;
  if (!triples || !o.n_before || !o.n_known_before || !o.true_dist || !workspace || ((uintptr_t)workspace & 255))
    return GE_EINVAL;
  for (const void* p : {(const void*)triples, (const void*)o.known_off, (const void*)o.n_before,
                        (const void*)o.n_known_before, (const void*)o.true_dist, (const void*)o.scores_out})
    if (p && !aligned4(p)) return GE_EINVAL;
  return 0;
}
// the top-k's outputs: B in range, k in [1, max_k], every buffer present and aligned; the known lists come as a pair
static int topk_outputs_ok(int64_t B, const int32_t* queries, const int32_t* known_off, const uint16_t* known_rc,
                           int32_t k, const int32_t* out_id, const float* out_dist, const void* workspace) {
  if (B < 0 || B > ((int64_t)1 << 28) || k < 1 || k > transx_topk_max_k()) return GE_EINVAL;
  if ((known_off == nullptr) != (known_rc == nullptr)) return GE_EINVAL;
  if (B == 0) return 0;
  if (!queries || !out_id || !out_dist || !workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  for (const void* p : {(const void*)queries, (const void*)known_off, (const void*)out_id, (const void*)out_dist})
    if (p && !aligned4(p)) return GE_EINVAL;
  return 0;
}

// the candidate sets of a masked entry point
static int sets_ok(const SetArgs& s) {
  return s.row_set && s.mask && s.n_sets >= 1 && aligned4(s.row_set) && aligned4(s.mask) ? 0 : GE_EINVAL;
}

static int trans_rank(const TransModel& m, const int32_t* triples, int64_t B, int cand_is_head, const RankOut& o,
                      void* workspace, size_t workspace_bytes, void* stream, const SetArgs* sets = nullptr) {
  if (sets)
    if (int rc = sets_ok(*sets)) return rc;
  if (int rc = rank_outputs_ok(B, triples, o, workspace)) return rc;
  if (B == 0) return 0;
  if (sets)
    return trans_rank_masked_launch(m, triples, B, cand_is_head, o, *sets, workspace, workspace_bytes,
                                    (hipStream_t)stream);
  return trans_rank_launch(m, triples, B, cand_is_head, o, workspace, workspace_bytes, (hipStream_t)stream);
}
static int trans_relation_rank(const TransModel& m, const int32_t* triples, int64_t B, const RankOut& o, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (int rc = rank_outputs_ok(B, triples, o, workspace)) return rc;
  if (B == 0) return 0;
  return trans_relrank_launch(m, triples, B, o, workspace, workspace_bytes, (hipStream_t)stream);
}
static int trans_topk(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head, const int32_t* known_off,
                      const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist, void* workspace,
                      size_t workspace_bytes, void* stream, const SetArgs* sets = nullptr) {
  if (sets)
    if (int rc = sets_ok(*sets)) return rc;
  if (int rc = topk_outputs_ok(B, queries, known_off, known_rc, k, out_id, out_dist, workspace)) return rc;
  if (B == 0) return 0;
  if (sets)
    return trans_topk_masked_launch(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, *sets,
                                    workspace, workspace_bytes, (hipStream_t)stream);
  return trans_topk_launch(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

size_t ge_transx_rank_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B) {
  TransModel m;
  return sweep_shape(m, false, model, n_ent, n_rel, d, d, B, false) ? trans_rank_ws_bytes(m, B) : 0;
}

int ge_transx_rank(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                   const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                   const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_dist,
                   float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  return trans_rank(m, triples, B, cand_is_head, {known_off, known_rc, n_before, n_known_before, true_dist, scores_out},
                    workspace, workspace_bytes, stream);
}

// RotatE's ranks over every entity (ge_rotate.hip): the tables, the outputs, B == 0 (returns 0), the launcher's GE_ENOMEM
size_t ge_rotate_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B) {
  if (n_ent <= 0 || n_rel <= 0 || d <= 0 || d % 2 || d > rotate_max_dim() || !sweep_batch_ok(B)) return 0;
  return rotate_rank_ws_bytes(d, B);
}

int ge_rotate_rank(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                   const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_dist,
                   float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = rotate_model(ent, n_ent, rel, n_rel, d)) return rc;
  const RankOut o{known_off, known_rc, n_before, n_known_before, true_dist, scores_out};
  if (int rc = rank_outputs_ok(B, triples, o, workspace)) return rc;
  if (B == 0) return 0;
  return rotate_rank_launch(l1, ent, n_ent, rel, n_rel, d, triples, B, cand_is_head, o, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

size_t ge_transr_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B) {
  TransModel m;
  return sweep_shape(m, true, kTransR, n_ent, n_rel, dim_e, dim_r, B, false) ? trans_rank_ws_bytes(m, B) : 0;
}

int ge_transr_rank(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                   int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B, int cand_is_head,
                   const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before,
                   float* true_dist, float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  return trans_rank(m, triples, B, cand_is_head, {known_off, known_rc, n_before, n_known_before, true_dist, scores_out},
                    workspace, workspace_bytes, stream);
}

size_t ge_transx_relation_rank_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B) {
  TransModel m;
  return sweep_shape(m, false, model, n_ent, n_rel, d, d, B, true) ? trans_relrank_ws_bytes(m, B) : 0;
}

int ge_transx_relation_rank(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                            const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                            const int32_t* triples, int64_t B, const int32_t* known_off, const uint16_t* known_rc,
                            int32_t* n_before, int32_t* n_known_before, float* true_dist, float* scores_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  return trans_relation_rank(m, triples, B, {known_off, known_rc, n_before, n_known_before, true_dist, scores_out},
                             workspace, workspace_bytes, stream);
}

size_t ge_transr_relation_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B) {
  TransModel m;
  return sweep_shape(m, true, kTransR, n_ent, n_rel, dim_e, dim_r, B, true) ? trans_relrank_ws_bytes(m, B) : 0;
}

int ge_transr_relation_rank(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                            int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B,
                            const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before,
                            int32_t* n_known_before, float* true_dist, float* scores_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  return trans_relation_rank(m, triples, B, {known_off, known_rc, n_before, n_known_before, true_dist, scores_out},
                             workspace, workspace_bytes, stream);
}

int ge_transx_topk_max_k(void) { return transx_topk_max_k(); }

size_t ge_transx_topk_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t k) {
  TransModel m;
  return sweep_shape(m, false, model, n_ent, n_rel, d, d, B, false) ? trans_topk_ws_bytes(m, B, k) : 0;
}

int ge_transx_topk(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                   const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                   const int32_t* queries, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist, void* workspace,
                   size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  return trans_topk(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, workspace, workspace_bytes,
                    stream);
}

size_t ge_transr_topk_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B, int32_t k) {
  TransModel m;
  return sweep_shape(m, true, kTransR, n_ent, n_rel, dim_e, dim_r, B, false) ? trans_topk_ws_bytes(m, B, k) : 0;
}

int ge_transr_topk(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                   int32_t dim_e, int32_t dim_r, const int32_t* queries, int64_t B, int cand_is_head,
                   const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist,
                   void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  return trans_topk(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, workspace, workspace_bytes,
                    stream);
}

// The same sweeps with per-relation candidate sets (ge_transx_rank_masked.hip): trans_rank / trans_topk with the sets.
int ge_transx_rank_masked(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                          const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                          const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                          const uint16_t* known_rc, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                          int32_t* n_before, int32_t* n_known_before, float* true_dist, void* workspace,
                          size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  const SetArgs sets{row_set, mask, n_sets, 0};
  return trans_rank(m, triples, B, cand_is_head, {known_off, known_rc, n_before, n_known_before, true_dist, nullptr},
                    workspace, workspace_bytes, stream, &sets);
}

int ge_transr_rank_masked(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                          int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B,
                          int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, const int32_t* row_set,
                          const uint32_t* mask, int32_t n_sets, int32_t* n_before, int32_t* n_known_before,
                          float* true_dist, void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  const SetArgs sets{row_set, mask, n_sets, 0};
  return trans_rank(m, triples, B, cand_is_head, {known_off, known_rc, n_before, n_known_before, true_dist, nullptr},
                    workspace, workspace_bytes, stream, &sets);
}

int ge_transx_topk_masked(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                          const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                          const int32_t* queries, int64_t B, int cand_is_head, const int32_t* known_off,
                          const uint16_t* known_rc, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                          int32_t k, int32_t* out_id, float* out_dist, void* workspace, size_t workspace_bytes,
                          void* stream) {
  TransModel m;
  if (int rc = transx_model(m, model, l1, ent, n_ent, rel, n_rel, normal, ent_transfer, rel_transfer, d)) return rc;
  const SetArgs sets{row_set, mask, n_sets, 0};
  return trans_topk(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, workspace, workspace_bytes,
                    stream, &sets);
}

int ge_transr_topk_masked(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                          int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* queries, int64_t B,
                          int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, const int32_t* row_set,
                          const uint32_t* mask, int32_t n_sets, int32_t k, int32_t* out_id, float* out_dist,
                          void* workspace, size_t workspace_bytes, void* stream) {
  TransModel m;
  if (int rc = transr_model(m, l1, ent, n_ent, rel, rel_matrix, n_rel, dim_e, dim_r)) return rc;
  const SetArgs sets{row_set, mask, n_sets, 0};
  return trans_topk(m, queries, B, cand_is_head, known_off, known_rc, k, out_id, out_dist, workspace, workspace_bytes,
                    stream, &sets);
}

static inline int neighbor_args_ok(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B,
                                   const int32_t* cand, int64_t K, int metric, const void* planes) {
  if (!ok_table(table, N, d) || B < 0 || B > ((int64_t)1 << 28) || K <= 0 || K > INT32_MAX) return GE_EINVAL;
  if (metric != GE_METRIC_COSINE && metric != GE_METRIC_EUCLIDEAN) return GE_EINVAL;
  if (d > neighbor_max_dim()) return GE_ENOTSUP;
  if (!cand || !planes || ((uintptr_t)planes & 255) || !aligned4(table) || !aligned4(cand)) return GE_EINVAL;
  if (B > 0 && (!queries || !aligned4(queries))) return GE_EINVAL;
  return 0;
}

int ge_neighbor_max_k(void) { return neighbor_max_k(); }
int ge_neighbor_max_dim(void) { return neighbor_max_dim(); }
int64_t ge_neighbor_planes_bytes(int64_t K, int32_t d) { return neighbor_planes_bytes(K, d); }

int ge_neighbor_planes(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, void* planes,
                       void* stream) {
  if (!ok_table(table, N, d) || K <= 0 || K > INT32_MAX || !cand || !planes) return GE_EINVAL;
  if (d > neighbor_max_dim()) return GE_ENOTSUP;
  if (((uintptr_t)planes & 255) || !aligned4(table) || !aligned4(cand)) return GE_EINVAL;
  if (neighbor_planes_bytes(K, d) == 0) return GE_ENOTSUP;
  return neighbor_planes_launch(table, N, d, cand, K, planes, (hipStream_t)stream);
}

size_t ge_neighbor_workspace_bytes(int64_t B, int64_t K, int32_t k) {
  if (B <= 0 || B > ((int64_t)1 << 28) || K <= 0 || K > INT32_MAX) return 0;
  return neighbor_ws_bytes(B, K, k);
}

int ge_neighbor_dists(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B, const int32_t* cand,
                      int64_t K, int metric, const void* planes, float* out, void* stream) {
  if (int rc = neighbor_args_ok(table, N, d, queries, B, cand, K, metric, planes)) return rc;
  if (B == 0) return 0;
  if (!out || !aligned4(out)) return GE_EINVAL;
  return neighbor_dists_launch(table, N, d, queries, B, cand, K, metric, planes, out, (hipStream_t)stream);
}

int ge_neighbor_topk(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B, const int32_t* cand,
                     int64_t K, int32_t k, int metric, int exclude_self, const void* planes, int32_t* out_id,
                     float* out_dist, void* workspace, size_t workspace_bytes, void* stream) {
  if (k < 1) return GE_EINVAL;
  if (int rc = neighbor_args_ok(table, N, d, queries, B, cand, K, metric, planes)) return rc;
  if (k > neighbor_max_k()) return GE_ENOTSUP;
  if (B == 0) return 0;
  if (!out_id || !out_dist || !aligned4(out_id) || !aligned4(out_dist)) return GE_EINVAL;
  if (!workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (workspace_bytes < neighbor_ws_bytes(B, K, k)) return GE_ENOMEM;
  return neighbor_topk_launch(table, N, d, queries, B, cand, K, k, metric, exclude_self, planes, out_id, out_dist,
                              workspace, workspace_bytes, (hipStream_t)stream);
}

size_t ge_threshold_fit_workspace_bytes(int64_t M, int32_t n_seg) { return threshold_fit_ws_bytes(M, n_seg); }

int ge_threshold_fit(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                     float* thr_lo, float* thr_hi, int32_t* best_correct, int32_t* n_pos, int32_t* n_neg,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (M < 1 || M > INT32_MAX || n_seg < 1 || !score || !seg || !label) return GE_EINVAL;
  if (!thr_lo || !thr_hi || !best_correct || !n_pos || !n_neg) return GE_EINVAL;
  for (const void* p : {(const void*)score, (const void*)seg, (const void*)thr_lo, (const void*)thr_hi,
                        (const void*)best_correct, (const void*)n_pos, (const void*)n_neg})
    if (!aligned4(p)) return GE_EINVAL;
  if (!workspace || ((uintptr_t)workspace & 255)) return GE_EINVAL;
  if (workspace_bytes < threshold_fit_ws_bytes(M, n_seg)) return GE_ENOMEM;
  return threshold_fit_launch(score, seg, label, M, n_seg, thr_lo, thr_hi, best_correct, n_pos, n_neg, workspace,
                              (hipStream_t)stream);
}

int ge_threshold_classify(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                          const float* thr, uint8_t* pred, int32_t* confusion, void* stream) {
  if (M < 0 || M > INT32_MAX || n_seg < 1 || !thr || !aligned4(thr)) return GE_EINVAL;
  if (confusion && (!label || !aligned4(confusion))) return GE_EINVAL;
  if (M > 0 && (!score || !seg || !pred || !aligned4(score) || !aligned4(seg))) return GE_EINVAL;
  return threshold_classify_launch(score, seg, label, M, n_seg, thr, pred, confusion, (hipStream_t)stream);
}

int ge_complex_score_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B,
                         const int32_t* cand, int64_t K, float max_norm, int apply_sigmoid, int cand_is_head,
                         float* out, void* stream) {
  if (B < 0 || K < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || (d & 1)) return GE_EINVAL;
  if (B > 0 && K > 0 && (!hr || !cand || !out)) return GE_EINVAL;
  return complex_score_1vK_launch(table, N, d, hr, B, cand, K, max_norm, apply_sigmoid, cand_is_head, out,
                                  (hipStream_t)stream);
}

// the sweeps of ge_sweep_route.h serve ComplEx and HolE on a spectral table; 0, or the code for any other model
static inline int sweep_model_ok(int model) {
  if (model == GE_MODEL_COMPLEX || model == GE_MODEL_HOLE_SPECTRAL) return 0;
  return model == GE_MODEL_HOLE || model == GE_MODEL_HOLE_DIRECT ? GE_ENOTSUP : GE_EINVAL;
}

// the rank sweeps add into their two counters
static inline int zero_counts(int32_t* n_before, int32_t* n_known_before, int64_t B, hipStream_t st) {
  hipError_t e = hipMemsetAsync(n_before, 0, sizeof(int32_t) * (size_t)B, st);
  if (e == hipSuccess) e = hipMemsetAsync(n_known_before, 0, sizeof(int32_t) * (size_t)B, st);
  return e == hipSuccess ? 0 : (int)e;
}

int ge_rank_max_dim(void) { return kRankMaxDim; }

int64_t ge_rank_planes_bytes(int64_t N, int32_t d, int64_t K) { return rank_planes_bytes(N, d, K); }

int ge_rank_planes(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, float max_norm, int model,
                   void* planes, void* stream) {
  if (K < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm) || !planes) return GE_EINVAL;
  if (int rc = sweep_model_ok(model)) return rc;
  if (K > 0 && !cand) return GE_EINVAL;
  return rank_planes_launch(table, N, d, cand, K, max_norm, model == GE_MODEL_HOLE_SPECTRAL, planes, (hipStream_t)stream);
}

// The ONE check of what the rank and top-k sweeps, plain and with candidate sets, take: `a` as the entry point packed
// it (the checker fills a.spec from the model), topk / sets null where the call has none.  Codes and order are what
// each entry point answered when it had a copy of its own (tests/test_sweep_refusals_host.py).  The forms differ, and
// stay different -- aligning them would change what callers see:
//   * ranks refuse K < 0; top-k refuses K < 1, and k < 1, in the first line;
//   * candidate sets are checked second, ahead of the model, and ask for the split-precision range (GE_ENOTSUP) ahead
//     of the planes -- and so ahead of B == 0, where the plain forms leave the range to the route;
//   * sweep_rank: ge_rank_1vK_vs_loss and ge_rank_1vK_masked return 0 for K == 0 once the counts are zeroed;
//     ge_rank_1vK_planes leaves K == 0 to route_rank, which first refuses an odd or unsupported embedding_dim;
//   * behind the shape's GE_ENOTSUP the routes of the candidate-set forms refuse a table that is not 16-byte aligned and
//     more than INT32_MAX / 8 row blocks; route_topk without sets asks neither, so a misaligned table with the caller's
//     own planes is not refused there.
static int sweep_args(SweepArgs& a, int model, const void* planes, const TopkOut* topk, const SetArgs* sets) {
  if (a.B < 0 || a.K < (topk ? 1 : 0) || (topk && topk->k < 1) || !ok_table(a.table, a.N, a.d) || !max_norm_ok(a.max_norm))
    return GE_EINVAL;
  if (sets && (!sets->row_set || !sets->mask || sets->n_sets < 1 || !aligned4(sets->row_set) || !aligned4(sets->mask)))
    return GE_EINVAL;
  if (int rc = sweep_model_ok(model)) return rc;
  a.spec = model == GE_MODEL_HOLE_SPECTRAL;
  if (a.B > 0) {
    if (!a.hr || (a.K > 0 && !a.cand)) return GE_EINVAL;
    if (topk ? !topk->out_id || !topk->out_loss : !a.true_id || !a.raw_cnt || !a.skip_cnt) return GE_EINVAL;
    if ((a.sweep_flags & 2) && !a.true_loss) return GE_EINVAL;   // (ranks against stored losses read them)
  }
  if ((a.known_off == nullptr) != (a.known_rc == nullptr)) return GE_EINVAL;
  if (sets && !f16_sweep_ok(a.d, a.max_norm)) return GE_ENOTSUP;
  if (planes && (rank_planes_bytes(a.N, a.d, a.K) == 0 || reinterpret_cast<uintptr_t>(planes) % 256 != 0)) return GE_EINVAL;
  return 0;
}

// a checked rank sweep: the counters zeroed, then the route's kernel
static int sweep_rank(const SweepArgs& a, bool k0_returns, const void* planes, const SetArgs* sets, void* stream) {
  if (a.B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = zero_counts(a.raw_cnt, a.skip_cnt, a.B, st)) return rc;
  if (k0_returns && a.K == 0) return 0;
  if (!sets) return complex_rank_1vK_launch(a, planes, st);
  const SweepRoute r = route_masked_rank(a.N, a.d, a.B, a.K, a.max_norm, table_mod16(a));
  return r.kernel == SweepRoute::None ? r.status : masked_rank_launch(a, *sets, planes, st);
}

// a checked top-k sweep
static int sweep_topk(const SweepArgs& a, const TopkOut& t, const void* planes, const SetArgs* sets, void* stream) {
  const SweepRoute r = route_topk(a.N, a.d, a.B, a.K, a.max_norm, table_mod16(a), t.k, sets != nullptr);
  if (r.kernel == SweepRoute::None) return r.status;
  return sets ? masked_topk_launch(a, t, *sets, planes, (hipStream_t)stream) : topk_f16_launch(a, t, planes, (hipStream_t)stream);
}

int ge_rank_1vK_planes(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                       const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                       float* scores_out, const void* planes, void* stream) {
  SweepArgs a{table, N, d, hr, B, true_id, cand, K, max_norm, cand_is_head, known_off, known_rc, n_before, n_known_before,
              true_loss, scores_out, /*spec=*/0, /*scores_only=*/0, /*sweep_flags=*/0};
  if (int rc = sweep_args(a, model, planes, nullptr, nullptr)) return rc;
  return sweep_rank(a, /*k0_returns=*/false, planes, nullptr, stream);
}

int ge_rank_1vK_vs_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* ref_id,
                        const float* ref_loss, const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head,
                        const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before,
                        const void* planes, void* stream) {
  // (the launchers take the losses through their true_loss argument, which sweep_flags & 2 only reads)
  SweepArgs a{table, N, d, hr, B, ref_id, cand, K, max_norm, cand_is_head, known_off, known_rc, n_before, n_known_before,
              const_cast<float*>(ref_loss), nullptr, /*spec=*/0, /*scores_only=*/0, /*sweep_flags=*/2};
  if (int rc = sweep_args(a, model, planes, nullptr, nullptr)) return rc;
  return sweep_rank(a, /*k0_returns=*/true, planes, nullptr, stream);
}

int ge_topk_max_k(void) { return kTopkMaxK; }

size_t ge_topk_workspace_bytes(int64_t B, int64_t K, int32_t k) { return topk_ws_bytes(B, K, k); }

int ge_topk_1vK_planes(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand,
                       int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_loss, const void* planes,
                       void* workspace, size_t workspace_bytes, void* stream) {
  SweepArgs a{table, N, d, hr, B, nullptr, cand, K, max_norm, cand_is_head, known_off, known_rc};
  const TopkOut t{k, out_id, out_loss, workspace, workspace_bytes};
  if (int rc = sweep_args(a, model, planes, &t, nullptr)) return rc;
  return sweep_topk(a, t, planes, nullptr, stream);
}

int64_t ge_candidate_mask_words(int64_t K) { return candidate_mask_words(K); }

int ge_candidate_mask_from_classes(const int32_t* cand_class, int64_t K, const uint32_t* allow, int32_t n_sets,
                                   int32_t n_class, uint32_t* mask, void* stream) {
  if (K < 1 || K > INT32_MAX || n_sets < 1 || n_class < 1 || !cand_class || !allow || !mask) return GE_EINVAL;
  if (!aligned4(cand_class) || !aligned4(allow) || !aligned4(mask)) return GE_EINVAL;
  return mask_from_classes_launch(cand_class, K, allow, n_sets, n_class, mask, (hipStream_t)stream);
}

int ge_candidate_mask_from_cells(const int32_t* cells, int64_t M, int32_t n_sets, int64_t K, uint32_t* mask, void* stream) {
  if (K < 1 || K > INT32_MAX || n_sets < 1 || M < 0 || !mask || (M > 0 && !cells)) return GE_EINVAL;
  if (!aligned4(cells) || !aligned4(mask)) return GE_EINVAL;
  return mask_from_cells_launch(cells, M, n_sets, K, mask, (hipStream_t)stream);
}

int ge_rank_1vK_masked(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                       const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                       float* scores_out, const void* planes, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                       void* stream) {
  SweepArgs a{table, N, d, hr, B, true_id, cand, K, max_norm, cand_is_head, known_off, known_rc, n_before, n_known_before,
              true_loss, scores_out, /*spec=*/0, /*scores_only=*/0, /*sweep_flags=*/0};
  const SetArgs sets{row_set, mask, n_sets, 0};
  if (int rc = sweep_args(a, model, planes, nullptr, &sets)) return rc;
  return sweep_rank(a, /*k0_returns=*/true, planes, &sets, stream);
}

int ge_topk_1vK_masked(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand,
                       int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_loss, const void* planes,
                       void* workspace, size_t workspace_bytes, const int32_t* row_set, const uint32_t* mask,
                       int32_t n_sets, void* stream) {
  SweepArgs a{table, N, d, hr, B, nullptr, cand, K, max_norm, cand_is_head, known_off, known_rc};
  const TopkOut t{k, out_id, out_loss, workspace, workspace_bytes};
  const SetArgs sets{row_set, mask, n_sets, 0};
  if (int rc = sweep_args(a, model, planes, &t, &sets)) return rc;
  return sweep_topk(a, t, planes, &sets, stream);
}

int ge_rank_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                float* scores_out, void* stream) {
  return ge_rank_1vK_planes(table, N, d, hr, B, true_id, cand, K, max_norm, model, cand_is_head, known_off, known_rc,
                            n_before, n_known_before, true_loss, scores_out, nullptr, stream);
}

int ge_known_cells(int pass, const int64_t* known_key, const int64_t* known_ent, int64_t M, const int64_t* fixed,
                   const int64_t* rel, int64_t B, const int64_t* pos_of, int64_t n_rows, int64_t n_cand, int32_t* tile_scratch,
                   int32_t* known_off, uint16_t* known_rc, void* stream) {
  if (pass < 0 || pass > 1 || M < 0 || B < 0 || n_rows <= 0 || n_cand <= 0 || !tile_scratch || !known_off) return GE_EINVAL;
  if (M > 0 && (!known_key || !known_ent)) return GE_EINVAL;
  if (B > 0 && (!fixed || !rel || !pos_of)) return GE_EINVAL;
  if (pass == 1 && !known_rc) return GE_EINVAL;
  return known_cells_launch(pass, known_key, known_ent, M, fixed, rel, B, pos_of, n_rows, n_cand, tile_scratch, known_off,
                            known_rc, (hipStream_t)stream);
}

// ---------------------------------------------------------------- rank metrics and the rank validation tick
constexpr int64_t kRankMetricsMaxRows = (int64_t)1 << 24;   // the counted rows stay exact in metrics_out[7]

int ge_rank_metrics(const int32_t* n_before, const int32_t* n_known_before, const float* true_loss, int64_t M,
                    float* metrics_out, float* best, int32_t* improved, void* stream) {
  if (!n_before || !n_known_before || !metrics_out || M < 1) return GE_EINVAL;
  if (M > kRankMetricsMaxRows) return GE_ENOTSUP;
  return rank_metrics_launch(n_before, n_known_before, true_loss, M, metrics_out, best, improved, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the gated copy of several buffers
constexpr int64_t kCopyIfMaxCount = (int64_t)1 << 44;       // words of one segment: byte ranges stay far from wrapping

int ge_copy_if_chunk(void) { return kCopyIfChunk; }

int ge_copy_if(const int32_t* flag, int32_t n_seg, const float* const* src, float* const* dst, const int64_t* count,
               void* stream) {
  if (!flag || !src || !dst || !count || n_seg < 1 || n_seg > GE_COPY_IF_MAX_SEGMENTS) return GE_EINVAL;
  uintptr_t s0[GE_COPY_IF_MAX_SEGMENTS], d0[GE_COPY_IF_MAX_SEGMENTS], bytes[GE_COPY_IF_MAX_SEGMENTS];
  bool too_long = false;
  for (int32_t s = 0; s < n_seg; ++s) {
    if (count[s] < 0) return GE_EINVAL;
    s0[s] = reinterpret_cast<uintptr_t>(src[s]);
    d0[s] = reinterpret_cast<uintptr_t>(dst[s]);
    if (count[s] > 0 && (!s0[s] || !d0[s] || s0[s] % 4 != 0 || d0[s] % 4 != 0)) return GE_EINVAL;
    too_long = too_long || count[s] > kCopyIfMaxCount;
    bytes[s] = 4 * (uintptr_t)std::min(count[s], kCopyIfMaxCount);
  }
  // a dst range against every other dst range and every src range: any order of the segments gives the same result
  auto overlap = [](uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a < b + nb && b < a + na; };
  for (int32_t s = 0; s < n_seg; ++s) {
    if (count[s] == 0) continue;
    for (int32_t u = 0; u < n_seg; ++u) {
      if (count[u] == 0) continue;
      if (u != s && overlap(d0[s], bytes[s], d0[u], bytes[u])) return GE_EINVAL;
      if (overlap(d0[s], bytes[s], s0[u], bytes[u])) return GE_EINVAL;
    }
  }
  if (too_long) return GE_ENOTSUP;
  return copy_if_segments_launch(flag, n_seg, src, dst, count, (hipStream_t)stream);
}

// the tick's workspace: n_before [2V] | n_known_before [2V] | true_loss [2V] | flag -- the tail side's V rows first, so
// that the three vectors are what ge_rank_metrics takes for M = 2V
struct RankTickWs { int32_t* raw; int32_t* skip; float* true_loss; int32_t* flag; size_t bytes; };
static RankTickWs rank_tick_ws(void* base, int64_t V) {
  const size_t m = 2 * (size_t)V;
  return RankTickWs{ws_at<int32_t>(base, 0), ws_at<int32_t>(base, 4 * m), ws_at<float>(base, 8 * m),
                    ws_at<int32_t>(base, 12 * m), (12 * m + 16 + 255) / 256 * 256};
}
size_t ge_rank_tick_workspace_bytes(int64_t V) { return V < 1 ? 0 : rank_tick_ws(nullptr, V).bytes; }

// Every check of both sides comes before the first launch: the tick's own, then sweep_args for the tail rows and the
// head rows (the codes and the order of ge_rank_1vK_planes / ge_rank_1vK_masked), then what their routes and
// copy_if_launch would refuse behind a launch, then the workspace's size.
int ge_rank_validation_tick(const float* table, int64_t N, int32_t d, const int32_t* hr, const int32_t* true_id, int64_t V,
                            const int32_t* cand, int64_t K, float max_norm, int model, const int32_t* known_off_tail,
                            const uint16_t* known_rc_tail, const int32_t* known_off_head, const uint16_t* known_rc_head,
                            void* planes, const int32_t* row_set, const uint32_t* mask_tail, const uint32_t* mask_head,
                            int32_t n_sets, const float* accumulator, float* metrics_out, float* best, float* pocket,
                            float* pocket_accumulator, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (V < 1 || K < 1 || !metrics_out || !best || !workspace) return GE_EINVAL;
  const bool masked = row_set || mask_tail || mask_head;
  if (masked && (!row_set || !mask_tail || !mask_head)) return GE_EINVAL;
  if (!masked && n_sets != 0) return GE_EINVAL;
  if (pocket_accumulator && !accumulator) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (2 * V > kRankMetricsMaxRows) return GE_ENOTSUP;
  const RankTickWs w = rank_tick_ws(workspace, V);
  SweepArgs tail{table, N, d, hr, V, true_id, cand, K, max_norm, /*cand_is_head=*/0, known_off_tail, known_rc_tail, w.raw,
                 w.skip, w.true_loss, nullptr, /*spec=*/0, /*scores_only=*/0, /*sweep_flags=*/0};
  SweepArgs head{table, N, d, hr ? hr + 2 * V : nullptr, V, true_id ? true_id + V : nullptr, cand, K, max_norm,
                 /*cand_is_head=*/1, known_off_head, known_rc_head, w.raw + V, w.skip + V, w.true_loss + V, nullptr,
                 /*spec=*/0, /*scores_only=*/0, /*sweep_flags=*/0};
  const SetArgs sets_tail{row_set, mask_tail, n_sets, 0}, sets_head{row_set ? row_set + V : nullptr, mask_head, n_sets, 0};
  if (int rc = sweep_args(tail, model, planes, nullptr, masked ? &sets_tail : nullptr)) return rc;
  if (int rc = sweep_args(head, model, planes, nullptr, masked ? &sets_head : nullptr)) return rc;
  const SweepRoute r = masked ? route_masked_rank(N, d, V, K, max_norm, table_mod16(tail))
                              : route_rank(N, d, V, K, max_norm, table_mod16(tail));
  if (r.kernel == SweepRoute::None) return r.status ? r.status : GE_EINVAL;
  const bool f16 = r.kernel == SweepRoute::F16;
  if (f16 && !planes) return GE_EINVAL;     // (no allocation in a tick: the split-precision sweep runs on the caller's planes)
  const int64_t n = N * (int64_t)d;
  if (pocket && !copy_if_ok(table, pocket, n)) return GE_EINVAL;
  if (pocket_accumulator && !copy_if_ok(accumulator, pocket_accumulator, n)) return GE_EINVAL;
  if (workspace_bytes < w.bytes) return GE_ENOMEM;

  if (f16)
    if (int rc = rank_planes_launch(table, N, d, cand, K, max_norm, tail.spec, planes, st)) return rc;
  const void* pl = f16 ? planes : nullptr;
  if (int rc = sweep_rank(tail, /*k0_returns=*/true, pl, masked ? &sets_tail : nullptr, stream)) return rc;
  if (int rc = sweep_rank(head, /*k0_returns=*/true, pl, masked ? &sets_head : nullptr, stream)) return rc;
  if (int rc = rank_metrics_launch(w.raw, w.skip, w.true_loss, 2 * V, metrics_out, best, w.flag, st)) return rc;
  if (pocket)
    if (int rc = copy_if_launch(table, pocket, n, w.flag, st)) return rc;
  if (pocket_accumulator)
    if (int rc = copy_if_launch(accumulator, pocket_accumulator, n, w.flag, st)) return rc;
  return 0;
}

int ge_complex_rank_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                        const int32_t* cand, int64_t K, float max_norm, int cand_is_head, const int32_t* known_off,
                        const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                        float* scores_out, void* stream) {
  return ge_rank_1vK(table, N, d, hr, B, true_id, cand, K, max_norm, GE_MODEL_COMPLEX, cand_is_head, known_off, known_rc,
                     n_before, n_known_before, true_loss, scores_out, stream);
}

int ge_train_steps(float* table, int64_t N, int32_t d, const int32_t* triples, int64_t T, int64_t first_row,
                   int64_t B, int64_t n_steps, const int32_t* id_to_type, const int64_t* type_offsets,
                   int32_t n_types, const int32_t* type_ids, uint64_t seed, uint64_t global_step0,
                   int32_t padded_size, int32_t mode, float margin, float lr0, float decay_steps,
                   float decay_rate, float max_norm, int model, float* loss, int keep_all_losses,
                   int32_t* neg_ws, void* workspace, size_t workspace_bytes, void** ev_pairs, int ev_kernel,
                   void* pipeline, void* stream) {
  if (B <= 0 || n_steps < 0 || T < B || first_row < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm))
    return GE_EINVAL;
  TypeSampler ts;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, false)) return GE_EINVAL;
  if (!triples || !loss || !neg_ws || !workspace) return GE_EINVAL;
  if ((model & ~GE_STEP_DETERMINISTIC) < 0 || (model & ~GE_STEP_DETERMINISTIC) > 3) return GE_EINVAL;
  if ((model & ~GE_STEP_DETERMINISTIC) == GE_MODEL_HOLE_SPECTRAL && (d & 1)) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < ge_hinge_step_workspace_bytes(B, d)) return GE_ENOMEM;
  if (ev_pairs && (ev_kernel < 0 || ev_kernel > 2)) return GE_EINVAL;
  if (!sampler_ranges_ok(ts)) return GE_EINVAL;
  return train_steps_run(table, d, StepSeq{triples, T, first_row, B, global_step0}, n_steps, ts, margin,
                         StepHyper{lr0, decay_steps, decay_rate, max_norm}, model, loss, keep_all_losses, neg_ws, workspace,
                         workspace_bytes, ev_pairs, ev_kernel, pipeline, (hipStream_t)stream);
}

size_t ge_train_adagrad_workspace_bytes(int64_t B, int32_t d) { return ge_train_workspace_bytes(B, d); }

int ge_train_steps_adagrad(float* table, float* accum, int64_t N, int32_t d, const int32_t* triples, int64_t T,
                           int64_t first_row, int64_t B, int64_t n_steps, const int32_t* id_to_type,
                           const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids, uint64_t seed,
                           uint64_t global_step0, int32_t padded_size, int32_t mode, float margin, float lr0,
                           float decay_steps, float decay_rate, float max_norm, int model, float* loss,
                           int keep_all_losses, int32_t* neg_ws, void* workspace, size_t workspace_bytes, void* pipeline,
                           void* stream) {
  if (B <= 0 || n_steps < 0 || T < B || first_row < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (!accum || rows_overlap(table, accum, N, d)) return GE_EINVAL;
  TypeSampler ts;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, true)) return GE_EINVAL;
  if (!triples || !loss || !neg_ws || !workspace) return GE_EINVAL;
  if (model < 0 || model > 3) return GE_EINVAL;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(accum)) % 4 != 0) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  return train_adagrad_run(table, accum, d, StepSeq{triples, T, first_row, B, global_step0}, n_steps, ts, margin,
                           StepHyper{lr0, decay_steps, decay_rate, max_norm}, model, loss, keep_all_losses, neg_ws,
                           workspace, workspace_bytes, pipeline, (hipStream_t)stream);
}

size_t ge_train_logloss_workspace_bytes(int64_t B, int32_t negative_ratio, int32_t d) {
  if (B <= 0 || negative_ratio <= 0 || d <= 0) return 0;
  return train_logloss_ws_bytes(B, negative_ratio, d);
}

int ge_train_steps_logloss(float* table, int64_t N, int32_t d, const int32_t* triples, int64_t T, int64_t first_row,
                           int64_t B, int64_t n_steps, const int32_t* id_to_type, const int64_t* type_offsets,
                           int32_t n_types, const int32_t* type_ids, uint64_t seed, uint64_t global_step0,
                           int32_t padded_size, int32_t mode, int32_t negative_ratio, float l2, float lr0,
                           float decay_steps, float decay_rate, float max_norm, float* loss, int keep_all_losses,
                           int32_t* neg_ws, void* workspace, size_t workspace_bytes, void* pipeline, void* stream) {
  if (B <= 0 || n_steps < 0 || T < B || first_row < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (negative_ratio <= 0 || negative_ratio > 1024 || (d & 1)) return GE_EINVAL;
  TypeSampler ts;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, true)) return GE_EINVAL;
  if (!triples || !loss || !neg_ws || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if ((int64_t)(1 + negative_ratio) * B > ((int64_t)1 << 24)) return GE_ENOTSUP;
  return train_logloss_run(table, d, StepSeq{triples, T, first_row, B, global_step0}, n_steps, ts, negative_ratio, l2,
                           StepHyper{lr0, decay_steps, decay_rate, max_norm}, loss, keep_all_losses, neg_ws, workspace,
                           workspace_bytes, pipeline, (hipStream_t)stream);
}

int ge_train_pipeline_create(void** pipeline) { return pipeline ? pipeline_create(pipeline) : GE_EINVAL; }
int ge_train_pipeline_reset(void* pipeline) { return pipeline_reset(pipeline); }
int ge_train_pipeline_destroy(void* pipeline) { return pipeline_destroy(pipeline); }

int64_t ge_train_max_chunk_steps(int64_t B, int64_t negs) { return (B <= 0 || negs < 0) ? 0 : train_chunk_steps(B, negs); }

int ge_train_prepared_layout(int64_t B, int64_t* out8) {
  if (B <= 0 || !out8) return GE_EINVAL;
  train_prepared_layout(B, out8);
  return 0;
}

size_t ge_train_prepare_bytes(int64_t B, int64_t n_steps) { return (B <= 0 || n_steps <= 0) ? 0 : train_prepare_bytes(B, n_steps); }

int ge_train_prepare_steps(const int32_t* triples, int64_t T, int64_t first_row, int64_t B, int64_t n_steps,
                           const int32_t* id_to_type, int64_t N, const int64_t* type_offsets, int32_t n_types,
                           const int32_t* type_ids, uint64_t seed, uint64_t global_step0, int32_t padded_size,
                           int32_t mode, int direct, int32_t* out, size_t out_bytes, void* stream) {
  if (B <= 0 || n_steps < 0 || T < B || first_row < 0 || N <= 0) return GE_EINVAL;
  TypeSampler ts;
  if (type_sampler(ts, id_to_type, N, type_offsets, n_types, type_ids, seed, padded_size, mode, true)) return GE_EINVAL;
  if (!triples || !out) return GE_EINVAL;
  if (out_bytes < train_prepare_bytes(B, n_steps)) return GE_ENOMEM;
  return train_prepare_run(StepSeq{triples, T, first_row, B, global_step0}, n_steps, ts, direct, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the row-sharded step (csrc/ge_shard.hip)
static inline bool shard_ok(int64_t N, int32_t G, int32_t rank) { return N > 0 && G >= 1 && G <= 64 && rank >= 0 && rank < G && N + 2 * ((N + G - 1) / G) < ((int64_t)1 << 31); }

size_t ge_shard_plan_workspace_bytes(int64_t B, int64_t S) { return (B <= 0 || S <= 0) ? 0 : shard_plan_scratch_bytes(B, S); }

int ge_shard_plan(const int32_t* pos, const int32_t* neg, int64_t S, int64_t B, int64_t N, int32_t G, int32_t rank,
                  int32_t* records, int32_t* pos_src, int32_t* neg_src, int32_t* req_row, int32_t* counts,
                  void* workspace, size_t workspace_bytes, int32_t peer_mapped, void* stream) {
  if (S < 0 || B <= 0 || B > ((int64_t)1 << 24) || !shard_ok(N, G, rank)) return GE_EINVAL;
  if (peer_mapped && (G > 8 || ((N + G - 1) / G) * (G + 1) >= ((int64_t)1 << 30))) return GE_EINVAL;
  if (S == 0) return 0;
  if (!pos || !neg || !records || !pos_src || !neg_src || !req_row || !counts || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < shard_plan_scratch_bytes(B, S)) return GE_ENOMEM;
  return shard_plan_launch(pos, neg, S, B, N, G, rank, records, pos_src, neg_src, req_row, counts, workspace, peer_mapped, (hipStream_t)stream);
}

int ge_shard_grad(float* shard, int64_t rows_local, int32_t d, const float* staged, int64_t n_staged, const int32_t* pos_src,
                  const int32_t* neg_src, const int32_t* record, int64_t B, int64_t N, int32_t G, float margin, float lr,
                  float max_norm, int model, float* loss, int32_t* grad_idx, float* grad_val, float* gsum,
                  const float* const* peer_shards, void* stream) {
  if (B < 0 || !ok_table(shard, rows_local, d) || !max_norm_ok(max_norm) || !shard_ok(N, G, 0)) return GE_EINVAL;
  if (peer_shards && (staged || G > 8)) return GE_EINVAL;
  if (model != GE_MODEL_COMPLEX && model != GE_MODEL_HOLE_SPECTRAL) return GE_ENOTSUP;   // hole: keep the shard spectral
  if (B == 0) return 0;
  const int64_t R = (N + G - 1) / G;
  if (rows_local > R || n_staged < 0 || (n_staged > 0 && ((!staged && !peer_shards) || !gsum))) return GE_EINVAL;
  if (!pos_src || !neg_src || !record || !loss || !grad_idx || !grad_val) return GE_EINVAL;
  return shard_grad_launch(shard, d, staged, pos_src, neg_src, record, (int32_t)R, B, margin, lr, max_norm,
                           model == GE_MODEL_HOLE_SPECTRAL, loss, grad_idx, grad_val, gsum, peer_shards, G, (hipStream_t)stream,
                           nullptr, nullptr);
}

int ge_shard_apply(float* shard, int64_t rows_local, int32_t d, const int32_t* record, int64_t B, int64_t N, int32_t G,
                   const int32_t* grad_idx, const float* grad_val, float* gsum, void* stream) {
  if (B < 0 || !ok_table(shard, rows_local, d) || !shard_ok(N, G, 0)) return GE_EINVAL;
  if (B == 0) return 0;
  if (!record || !grad_idx || !grad_val) return GE_EINVAL;
  return shard_apply_launch(shard, d, record, B, grad_idx, grad_val, (int32_t)((N + G - 1) / G), gsum, (hipStream_t)stream,
                            nullptr, nullptr);
}

int64_t ge_shard_owner_record_words(int64_t cap) { return shard_owner_record_words(cap); }
size_t ge_shard_owner_workspace_bytes(int64_t cap, int64_t S) { return (cap <= 0 || S <= 0) ? 0 : shard_owner_scratch_bytes(cap, S); }

int ge_shard_owner_plan(const int32_t* req_all, const int64_t* req_start, int64_t S, int64_t cap, int64_t rows_local,
                        int32_t* records, void* workspace, size_t workspace_bytes, void* stream) {
  if (S < 0 || cap < 0 || rows_local <= 0 || rows_local >= ((int64_t)1 << 31) || cap >= ((int64_t)1 << 30)) return GE_EINVAL;
  if (S == 0 || cap == 0) return 0;
  if (!req_all || !req_start || !records || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  if (workspace_bytes < shard_owner_scratch_bytes(cap, S)) return GE_ENOMEM;
  return shard_owner_plan_launch(req_all, req_start, S, cap, (int32_t)rows_local, records, workspace, (hipStream_t)stream);
}

int ge_shard_owner_apply(float* shard, int64_t rows_local, int32_t d, const int32_t* record, int64_t cap, const float* recv,
                         void* stream) {
  if (cap < 0 || !ok_table(shard, rows_local, d)) return GE_EINVAL;
  if (cap == 0) return 0;
  if (!record || !recv) return GE_EINVAL;
  return shard_owner_apply_launch(shard, d, record, cap, recv, (hipStream_t)stream);
}

size_t ge_logloss_step_workspace_bytes(int64_t M, int32_t d) {
  if (M <= 0 || d <= 0) return 0;
  return logloss_ws(nullptr, M, d).bytes;
}

int ge_complex_logloss_step(float* table, int64_t N, int32_t d, const int32_t* triples, const float* labels,
                            int64_t M, float lr, float l2, float max_norm, float* loss, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (M < 0 || !ok_table(table, N, d) || !max_norm_ok(max_norm)) return GE_EINVAL;
  if (M == 0) return 0;
  if (!triples || !labels || !loss || !workspace) return GE_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return GE_EINVAL;
  const LoglossWs w = logloss_ws(workspace, M, d);
  if (workspace_bytes < w.bytes) return GE_ENOMEM;
  hipStream_t st = (hipStream_t)stream;
  int rc = table_sumsq_launch(table, N * (int64_t)d, w.sumsq, st);               // l2_loss of the OLD table
  if (rc) return rc;
  rc = complex_logloss_grad_launch(table, N, d, triples, labels, M, lr, max_norm, l2, w.sumsq, loss, w.gidx, w.gval, st);
  if (rc) return rc;
  // new = old - lr * (sparse + M * l2 * old) = old * (1 - lr*M*l2) + (-lr * sparse)
  if (l2 != 0.f) {
    rc = table_scale_launch(table, N * (int64_t)d, 1.0f - lr * (float)M * l2, st);
    if (rc) return rc;
  }
  return scatter_add_rows_launch(table, N, d, w.gidx, w.gval, 3 * M, st);
}

int ge_event_create(void** ev) {
  if (!ev) return GE_EINVAL;
  hipEvent_t e;
  hipError_t rc = hipEventCreate(&e);
  if (rc != hipSuccess) return (int)rc;
  *ev = (void*)e;
  return 0;
}
int ge_event_destroy(void* ev) { return ev ? (int)hipEventDestroy((hipEvent_t)ev) : GE_EINVAL; }
int ge_event_record(void* ev, void* stream) { return ev ? (int)hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) : GE_EINVAL; }
int ge_event_synchronize(void* ev) { return ev ? (int)hipEventSynchronize((hipEvent_t)ev) : GE_EINVAL; }
int ge_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return GE_EINVAL;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}

}  // extern "C"
