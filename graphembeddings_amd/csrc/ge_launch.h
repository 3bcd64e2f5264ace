// ge_launch.h -- the host entry points one source of libge_hip.so defines and another calls: the one declaration of
// each, included by the defining source too, so the compiler checks every definition against it.  Default arguments
// live here and nowhere else.  Launchers return 0 or an error code (hipError_t, GE_E*);
// the launchers behind a route (ge_sweep_route.h) assert the route's conditions instead -- on purpose in the shipped
// library too (no NDEBUG): a launcher and the router out of step would otherwise launch on a shape the kernel cannot take.
#pragma once
#include <assert.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ge_step_id.h"       // TypeSampler, StepSeq
#include "ge_sweep_route.h"   // rank_planes_bytes, kRankMaxDim
#include "ge_trans.h"         // TransModel

namespace ge {

struct TileGeom;
struct ShardOut;

// ge_complex.hip: ComplEx scoring, hinge and log-loss steps, the row-sharded grad step, table reductions
int complex_max_dim();
// the kernels below take this embedding_dim on a table at this address (the vector width follows its alignment); where
// they do not, their launchers answer GE_ENOTSUP (GE_EINVAL for an odd or non-positive d)
bool complex_shape_ok(int32_t d, const void* table);
int complex_score_launch(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B, float max_norm,
                         int apply_sigmoid, float* out, hipStream_t st, int spectral = 0, float label = 0.f, float l2 = 0.f,
                         const float* table_sumsq = nullptr, int64_t ld = 0);
int complex_hinge_loss_launch(const float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg, int64_t B,
                              float margin, float max_norm, float* loss, float* sig_out, hipStream_t st, int spectral = 0);
int complex_hinge_grad_launch(const float* rows, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg, int64_t B,
                              float margin, float lr, float max_norm, float* loss, int32_t* grad_idx, float* grad_val,
                              hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                              const int32_t* slot_item = nullptr, float* table_rw = nullptr, int spectral = 0,
                              const int32_t* order = nullptr);
int complex_logloss_grad_launch(const float* rows, int64_t N, int32_t d, const int32_t* triples, const float* labels,
                                int64_t M, float lr, float max_norm, float l2, const float* table_sumsq, float* loss,
                                int32_t* grad_idx, float* grad_val, hipStream_t st, const int32_t* negs = nullptr,
                                int64_t B = 0, float row_scale = 1.f, float neg_lr_eff = 0.f, hipEvent_t ev_start = nullptr,
                                hipEvent_t ev_stop = nullptr);
int shard_hinge_grad_launch(float* shard, int32_t d, const float* staged, const int32_t* pos_src, const int32_t* neg_src,
                            const int32_t* slot_item, int32_t R, int64_t B, float margin, float lr, float max_norm,
                            float* loss, int32_t* grad_idx, float* grad_val, float* gsum, int spectral, hipStream_t st,
                            hipEvent_t ev_start, hipEvent_t ev_stop, const int32_t* order, const float* const* peers,
                            int n_peers);
int table_sumsq_launch(const float* table, int64_t n, float* out, hipStream_t st);
int table_scale_launch(float* table, int64_t n, float factor, hipStream_t st);

// ge_hole.hip: HolE scoring and hinge steps
int hole_max_dim();           // widest embedding_dim of the direct-correlation kernels (GE_ENOTSUP beyond)
int hole_score_launch(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B, float max_norm,
                      int apply_sigmoid, float* out, hipStream_t st);
int hole_hinge_loss_launch(const float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg, int64_t B,
                           float margin, float max_norm, float* loss, float* sig_out, hipStream_t st);
int hole_hinge_grad_launch(const float* rows, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg, int64_t B,
                           float margin, float lr, float max_norm, float* loss, int32_t* grad_idx, float* grad_val,
                           hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// ge_spectral.hip: row-wise real DFT of a HolE table, in place
int hole_spectral_launch(float* table, int64_t N, int32_t d, int inverse, hipStream_t st);

// ge_rows.hip: row gather / scatter-add, samplers, pocket bookkeeping
int scatter_add_rows_launch(float* table, int64_t N, int32_t d, const int32_t* idx, const float* val, int64_t R,
                            hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
int gather_rows_launch(const float* table, int64_t N, int32_t d, const int32_t* idx, int64_t R, float* out, hipStream_t st);
int corrupt_batch_launch(const int32_t* pos, int64_t B, const TypeSampler& ts, uint64_t step, int32_t* neg, hipStream_t st);
// What a Bernoulli draw reads: the triple list it picks positives from (transx_draw_launch alone) and the known
// (entity, relation) keys with their entities, sorted, for the corruption.
struct SamplerArgs {
  const int32_t* triples; int64_t T; const int64_t* bh_key; const int32_t* bh_ent; const int64_t* bt_key;
  const int32_t* bt_ent; int64_t n_known; const uint32_t* tail_threshold; int32_t n_rel, n_ent;
};
int bernoulli_corrupt_launch(const int32_t* pos, int64_t B, const SamplerArgs& s, int32_t ent_lo, uint64_t seed,
                             uint64_t step, int32_t* neg, hipStream_t st);
int select_rows_launch(const int32_t* valid, int64_t V, int64_t B, uint64_t seed, uint64_t counter, int32_t* out,
                       hipStream_t st);
int mean_pocket_launch(const float* loss, int64_t B, float* mean_out, float* best, int32_t* flag, hipStream_t st);
int copy_if_launch(const float* src, float* dst, int64_t n, const int32_t* flag, hipStream_t st);
bool copy_if_ok(const float* src, const float* dst, int64_t n);   // false: copy_if_launch would refuse these buffers
// ge_copy_if: the segments as the kernel takes them, by value.  Non-empty segments only, chunk_start ascending from 0.
constexpr int kCopyIfChunk = 8192;   // 32-bit words one workgroup moves: 8 x 16 bytes a lane (ge_copy_if_chunk())
struct CopyIfSegments {
  const uint32_t* src[GE_COPY_IF_MAX_SEGMENTS]; uint32_t* dst[GE_COPY_IF_MAX_SEGMENTS];
  int64_t count[GE_COPY_IF_MAX_SEGMENTS], chunk_start[GE_COPY_IF_MAX_SEGMENTS]; int32_t n_seg;
};
// the host arrays as ge_copy_if checked them (n_seg in [1, 16], counts >= 0); one launch, none when every count is 0
int copy_if_segments_launch(const int32_t* flag, int32_t n_seg, const float* const* src, float* const* dst,
                            const int64_t* count, hipStream_t st);
// the summary of a rank sweep's counts (metrics_out [8]) and the pocket decision on its filtered MRR: one workgroup
int rank_metrics_launch(const int32_t* n_before, const int32_t* n_known_before, const float* true_loss, int64_t M,
                        float* metrics_out, float* best, int32_t* improved, hipStream_t st);

// ge_1vk.hip: 1-vs-K candidate scoring
int complex_score_1vK_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand,
                             int64_t K, float max_norm, int apply_sigmoid, int cand_is_head, float* out, hipStream_t st);

// What the sweep kernels behind the routes of ge_sweep_route.h take.  spec: the table is a spectral HolE table.
// scores_only: no ranking, scores_out [B,K] = score (its sigmoid with sweep_flags & 1): ge_complex_score_1vK.
// Ranks: scores_out may be null; sweep_flags & 2: true_loss is an INPUT, the loss every candidate of row i is ranked
// against, and true_id the tie-break id (ge_rank_1vK_vs_loss).  Top-k: the rank outputs are unused, see TopkOut.
struct SweepArgs {
  const float* table; int64_t N; int32_t d; const int32_t* hr; int64_t B; const int32_t* true_id; const int32_t* cand;
  int64_t K; float max_norm; int cand_is_head; const int32_t* known_off; const uint16_t* known_rc; int32_t* raw_cnt;
  int32_t* skip_cnt; float* true_loss; float* scores_out; int spec, scores_only, sweep_flags;
};
inline int table_mod16(const SweepArgs& a) { return (int)(reinterpret_cast<uintptr_t>(a.table) % 16); }   // (for the routes)
// what a top-k sweep takes beside them: k <= kTopkMaxK, out_id / out_loss [B][k], a workspace of topk_ws_bytes(B, K, k)
struct TopkOut { int32_t k; int32_t* out_id; float* out_loss; void* workspace; size_t workspace_bytes; };
// The candidate sets of a call (include/ge_hip.h): mask [n_sets][candidate_mask_words(candidates)], row_set [B].  The C
// ABI fills the first three; mw, the words per mask row, is the translation launchers'.
struct SetArgs {
  const int32_t* row_set; const uint32_t* mask; int32_t n_sets;
  int64_t mw;
};

// ge_rank.hip: link-prediction ranks -- the switch on route_rank (ge_sweep_route.h) and the fp32 kernel
int complex_rank_1vK_launch(const SweepArgs& a, const void* planes_ws, hipStream_t st);

// ge_rank_pipe.hip: Pipe<cw> of the route, cw in 40, 32, 24 dividing embedding_dim
int pipe_sweep_launch(int cw, const SweepArgs& a, hipStream_t st);

// ge_rank_f16.hip: the F16 of the route, ranks or scores.
// planes_ws: the candidates' fp16 planes + entity -> position map (rank_planes_launch into rank_planes_bytes bytes,
// 256-byte aligned) for the same (table, cand, max_norm, spec); NULL: built inside, in a stream-ordered allocation.
int rank_planes_launch(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, float max_norm, int spec,
                       void* planes_ws, hipStream_t st);
int f16_sweep_launch(const SweepArgs& a, const void* planes_ws, hipStream_t st);
// the top-k sweep on the same planes, behind route_topk: the workspace's pointer and size (GE_EINVAL, GE_ENOMEM) and
// topk_grid_ok (GE_ENOTSUP) are the launcher's own
int topk_f16_launch(const SweepArgs& a, const TopkOut& t, const void* planes_ws, hipStream_t st);

// ge_rank_f16_masked.hip: the same two sweeps with per-row candidate sets, behind route_masked_rank and route_topk, and
// the mask builders
int64_t candidate_mask_words(int64_t K);
int mask_from_classes_launch(const int32_t* cand_class, int64_t K, const uint32_t* allow, int32_t n_sets, int32_t n_class,
                             uint32_t* mask, hipStream_t st);
int mask_from_cells_launch(const int32_t* cells, int64_t M, int32_t n_sets, int64_t K, uint32_t* mask, hipStream_t st);
int masked_rank_launch(const SweepArgs& a, const SetArgs& sets, const void* planes_ws, hipStream_t st);
int masked_topk_launch(const SweepArgs& a, const TopkOut& t, const SetArgs& sets, const void* planes_ws, hipStream_t st);

// ge_neighbors.hip: nearest-neighbour search (cosine / Euclidean) on the split-precision sweep; embedding_dim 1 ... 288
int neighbor_max_k();
int neighbor_max_dim();
int64_t neighbor_planes_bytes(int64_t K, int32_t d);
int neighbor_planes_launch(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, void* planes_ws,
                           hipStream_t st);
size_t neighbor_ws_bytes(int64_t B, int64_t K, int32_t k);
int neighbor_dists_launch(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B,
                          const int32_t* cand, int64_t K, int metric, const void* planes_ws, float* out, hipStream_t st);
int neighbor_topk_launch(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B,
                         const int32_t* cand, int64_t K, int32_t k, int metric, int exclude_self, const void* planes_ws,
                         int32_t* out_id, float* out_dist, void* workspace, size_t workspace_bytes, hipStream_t st);

// ge_known.hip: the known-true cells of a ranking sweep as per-tile lists
int known_cells_launch(int pass, const int64_t* key, const int64_t* ent, int64_t M, const int64_t* fixed, const int64_t* rel,
                       int64_t B, const int64_t* pos_of, int64_t n_rows, int64_t n_cand, int32_t* tile_cnt, int32_t* off,
                       uint16_t* rc, hipStream_t st);

// ge_prep_big.hip: the multi-workgroup radix sort and the prepare stage of steps of more than one tile
size_t sort_scratch_bytes(int64_t n, int64_t n_sub, int64_t P);
unsigned long long* sort_scratch_keys(void* scratch);
int sort_tiles_launch(void* scratch, int64_t n, int64_t n_sub, int64_t P, int64_t n_rows, hipStream_t st,
                      const unsigned* limit, const unsigned long long** sorted);
int items_launch(const unsigned long long* sorted, int64_t n, const TileGeom& G, int direct, int32_t* out, const ShardOut* so,
                 hipStream_t st);
int relation_order_launch(const int32_t* triples, int64_t T, int64_t first_row, int64_t B, int64_t s0, int64_t n, int64_t N,
                          int32_t* out, int64_t stride, int64_t off_order, void* scratch, hipStream_t st);
size_t prep_big_scratch_bytes(int64_t B, int64_t negs, int64_t n);
int prepare_big_launch(const StepSeq& q, int64_t s0, int64_t n, const TypeSampler& ts, int direct, int32_t* out,
                       void* scratch, hipStream_t st, int negs);

// ge_train.hip: the native training loops, their prepare stage and pipeline handle, the row-sorted update
int apply_items_launch(float* table, int d, const TileGeom& G, const int32_t* step_rec, const int32_t* gidx,
                       const float* gval, int split, float* out2, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop,
                       int det);
// A workspace is carved in ONE place: a function that takes the base address and the shape and returns the pointers
// and the total size.  The size function calls it on a null base, the user on its workspace.
template <class T>
inline T* ws_at(void* base, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off); }
// the hinge step: gidx 6B int32, padded to 256 B | gval 6B x d fp32
struct HingeWs { int32_t* gidx; float* gval; size_t bytes; };
HingeWs hinge_ws(void* base, int64_t B, int32_t d);
// the log-loss step of M triples: sumsq 256 B | gidx 3M int32, padded to 256 B | gval 3M x d fp32
struct LoglossWs { float* sumsq; int32_t* gidx; float* gval; size_t bytes; };
LoglossWs logloss_ws(void* base, int64_t M, int32_t d);
// learning rate (tf.train.inverse_time_decay, no staircase; decay_steps <= 0: constant) and the clip of a loop
struct StepHyper {
  float lr0, decay_steps, decay_rate, max_norm;
  float lr_at(uint64_t gs) const { return decay_steps > 0.f ? lr0 / (1.0f + decay_rate * ((float)gs / decay_steps)) : lr0; }
};
size_t train_ws_bytes(int64_t B, int32_t d);
int train_steps_run(float* table, int32_t d, const StepSeq& q, int64_t n_steps, const TypeSampler& ts, float margin,
                    const StepHyper& hp, int model, float* loss, int keep_all_losses, int32_t* neg_ws, void* workspace,
                    size_t workspace_bytes, void** ev_pairs, int ev_kernel, void* pipe_handle, hipStream_t st);
size_t train_logloss_ws_bytes(int64_t B, int32_t negs, int32_t d);
int train_logloss_run(float* table, int32_t d, const StepSeq& q, int64_t n_steps, const TypeSampler& ts, int32_t negs,
                      float l2, const StepHyper& hp, float* loss, int keep_all_losses, int32_t* neg_ws, void* workspace,
                      size_t workspace_bytes, void* pipe_handle, hipStream_t st);
size_t train_prepare_bytes(int64_t B, int64_t n_steps);
int train_prepare_run(const StepSeq& q, int64_t n_steps, const TypeSampler& ts, int direct, int32_t* out, hipStream_t st);
void train_prepared_layout(int64_t B, int64_t* out);
int64_t train_chunk_steps(int64_t B, int64_t negs);   // steps per prepare launch of the native loops (negs = 0: hinge, AdaGrad)
// the AdaGrad loop (holE.py:296 with AdagradOptimizer): the prepared path only, its workspace is train_ws_bytes'
int train_adagrad_run(float* table, float* accum, int32_t d, const StepSeq& q, int64_t n_steps, const TypeSampler& ts,
                      float margin, const StepHyper& hp, int model, float* loss, int keep_all_losses, int32_t* neg_ws,
                      void* workspace, size_t workspace_bytes, void* pipe_handle, hipStream_t st);
int pipeline_create(void** out);
int pipeline_reset(void* h);
int pipeline_destroy(void* h);

// ge_adagrad.hip: the AdaGrad update of a prepared step record (items kernel + ordered pass over the split rows; gval
// holds minus the gradient and is written: split rows park their partial sums there) and of any sorted IndexedSlices
int adagrad_items_launch(float* table, float* accum, int d, const TileGeom& G, const int32_t* step_rec, const int32_t* gidx,
                         float* gval, float lr, hipStream_t st);
int adagrad_rows_launch(float* table, float* accum, int64_t N, int32_t d, const int32_t* idx, const float* val,
                        const int32_t* perm, int64_t R, float lr, hipStream_t st);

// ge_softmax.hip: 1-vs-all softmax loss and gradients of ComplEx (d % 8 == 0 in 8 ... kRankMaxDim, table 16-byte aligned:
// asserted).  The workspace: Q' [B,d] | C' [K,d] | query keys [B] | candidate keys [K] | (max, log sum) [2][B] | (max, sum, z_true,
// found) partials [8][B] | dL/dQ' partials [8][B,d], each padded to 256 B.  grad_idx == null: the loss alone.
struct SoftmaxWs { float* qp; float* cp; int32_t* qkey; int32_t* ckey; float* lse; float4* part; float* gq; size_t bytes; };
SoftmaxWs softmax_ws(void* base, int64_t B, int64_t K, int32_t d);
size_t softmax_ws_bytes(int64_t B, int64_t K, int32_t d);
int softmax_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                   const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head, float* loss,
                   int32_t* grad_idx, float* grad_val, void* workspace, hipStream_t st);
// its prepare (row_set non-null: a row whose set id is neither -1 nor in [0, n_sets) gets key -1 too), merge and finish
// stages on a carved workspace, for the masked form
int softmax_prepare_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, int cand_is_head, const int32_t* row_set,
                           int32_t n_sets, const SoftmaxWs& w, hipStream_t st);
int softmax_merge_launch(const SoftmaxWs& w, int n_ranges, int64_t B, float* loss, hipStream_t st);
int softmax_finish_launch(const float* table, int32_t d, const int32_t* hr, int64_t B, int64_t K, float max_norm, float lr,
                          int cand_is_head, const SoftmaxWs& w, int n_ranges, int32_t* grad_idx, float* grad_val,
                          hipStream_t st);
// its three sweeps: the LSE sweep into w.part, and the two gradient sweeps (dL/dC' into grad_val's first K rows, dL/dQ'
// into w.gq's first n_ranges partials) -- the instantiations softmax_launch runs, for ge_softmax_labels.hip
int softmax_lse_launch(const SoftmaxWs& w, int64_t B, int64_t K, int32_t d, float scale, int n_ranges, hipStream_t st);
int softmax_grad_sweeps_launch(const SoftmaxWs& w, int64_t B, int64_t K, int32_t d, float scale, int n_ranges, float* grad_val,
                               hipStream_t st);

// ge_softmax_labels.hip: multi-label (K-vs-all) softmax: row i is a query whose labels are the candidate positions
// label_pos[label_off[i] .. label_off[i + 1]), the target uniform over them; gradients in K + 2B + L slots.  The workspace:
// SoftmaxWs' parts with a ninth dL/dQ' partial [B,d] (the label term) | label means [B] double | row of entry [L] int32.
struct SoftmaxLabelsWs { SoftmaxWs base; float* lsum; double* mean; int32_t* row_of; size_t bytes; };
SoftmaxLabelsWs softmax_labels_ws(void* base, int64_t B, int64_t K, int32_t d, int64_t L);
size_t softmax_labels_ws_bytes(int64_t B, int64_t K, int32_t d, int64_t L);
int softmax_labels_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                          const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                          float lr, int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                          hipStream_t st);

// ge_softmax_masked.hip: ge_softmax.hip's objective with per-row candidate sets (SetArgs; mw is not read).  The workspace:
// SoftmaxWs' parts | the live-tile bitmap [query tiles][sm_live_words(K)] uint32, padded to 256 B.
struct SoftmaxMaskedWs { SoftmaxWs base; uint32_t* live; size_t bytes; };
SoftmaxMaskedWs softmax_masked_ws(void* base, int64_t B, int64_t K, int32_t d);
size_t softmax_masked_ws_bytes(int64_t B, int64_t K, int32_t d);
int softmax_masked_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                          const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head,
                          float* loss, int32_t* grad_idx, float* grad_val, void* workspace, const SetArgs& sets,
                          hipStream_t st);

// ge_softmax_sampled.hip: the same objective over candidates that need not hold the true entity (its logit is the row's
// own; slots that hold it are left out), gradients in K + 3B slots.  The workspace: Q' [B,d] | C' [K,d] | T' [B,d] (the
// clipped true rows) | query keys [B] | candidate keys [K] | z_true [B] | (max, log sum) [2][B] | (max, sum, row of the max, -) partials
// [8][B] | dL/dQ' partials [8][B,d] | dL/dC' partials [ranges][K,d] (sized for every number of query ranges the launch
// can choose), each padded to 256 B.  grad_idx == null: the loss alone.
struct SoftmaxSampledWs {
  float* qp; float* cp; float* tp; int32_t* qkey; int32_t* ckey; float* zt; float* lse; float4* part; float* gq; float* gc;
  size_t bytes;
};
SoftmaxSampledWs softmax_sampled_ws(void* base, int64_t B, int64_t K, int32_t d);
size_t softmax_sampled_ws_bytes(int64_t B, int64_t K, int32_t d);
int softmax_sampled_launch(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int cand_is_head,
                           float* loss, int32_t* grad_idx, float* grad_val, void* workspace, hipStream_t st);

// ge_shard.hip: the row-sharded step's requester and owner planners
size_t shard_plan_scratch_bytes(int64_t B, int64_t S);
int shard_plan_launch(const int32_t* pos, const int32_t* neg, int64_t S, int64_t B, int64_t N, int32_t G, int32_t rank,
                      int32_t* records, int32_t* pos_src, int32_t* neg_src, int32_t* req_row, int32_t* counts,
                      void* scratch, int peer, hipStream_t st);
int shard_grad_launch(float* shard, int32_t d, const float* staged, const int32_t* pos_src, const int32_t* neg_src,
                      const int32_t* record, int32_t R, int64_t B, float margin, float lr, float max_norm, int spectral,
                      float* loss, int32_t* gidx, float* gval, float* gsum, const float* const* peers, int n_peers,
                      hipStream_t st, hipEvent_t e0, hipEvent_t e1);
int shard_apply_launch(float* shard, int32_t d, const int32_t* record, int64_t B, const int32_t* gidx, const float* gval,
                       int32_t R, float* gsum, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
int64_t shard_owner_record_words(int64_t cap);
size_t shard_owner_scratch_bytes(int64_t cap, int64_t S);
int shard_owner_plan_launch(const int32_t* req_all, const int64_t* req_start, int64_t S, int64_t cap, int32_t rows_local,
                            int32_t* records, void* scratch, hipStream_t st);
int shard_owner_apply_launch(float* shard, int32_t d, const int32_t* record, int64_t cap, const float* recv, hipStream_t st);

// ge_transx.hip: TransE / TransH / TransD scoring, hinge steps, sampler and native loop
int transx_max_dim();
size_t transx_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B);
int transx_score_launch(const TransModel& m, const int32_t* tri, int64_t B, float* out, hipStream_t st);
int transx_hinge_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                          float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* neg,
                          int64_t B, float margin, float lr, float* loss, void* workspace, size_t workspace_bytes,
                          hipStream_t st);
int transx_draw_launch(const SamplerArgs& s, int64_t B, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg,
                       hipStream_t st);
// The native loop of transx_train_steps_run and transr_train_steps_run: for s in [0, n_steps), draw step
// first_step + s's batch into pos / neg, then run step(s) on it; stops at the first nonzero code.
template <class Step>
int draw_then_step(const SamplerArgs& sa, int64_t B, uint64_t seed, uint64_t first_step, int64_t n_steps, int32_t* pos,
                   int32_t* neg, hipStream_t st, Step step) {
  for (int64_t s = 0; s < n_steps; ++s) {
    int rc = transx_draw_launch(sa, B, seed, first_step + (uint64_t)s, pos, neg, st);
    if (rc || (rc = step(s))) return rc;
  }
  return 0;
}
int transx_train_steps_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                           float* ent_transfer, float* rel_transfer, int32_t d, const SamplerArgs& sa, uint64_t seed,
                           uint64_t first_step, int64_t n_steps, int64_t B, float margin, float lr, float* losses,
                           void* workspace, size_t workspace_bytes, hipStream_t st);
// The same step and loop with AdaGrad (acc += s * s, row -= lr * s / sqrt(acc) on each row's summed gradient): one
// accumulator per table under the table's name, those of tables the model does not have ignored.  The workspace is
// transx_ws_bytes' for both optimizers.
struct TransAccs { float *ent, *rel, *normal, *ent_transfer, *rel_transfer; };
int transx_adagrad_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                            float* ent_transfer, float* rel_transfer, const TransAccs& accs, int32_t d,
                            const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss,
                            void* workspace, size_t workspace_bytes, hipStream_t st);
int transx_train_steps_adagrad_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                                   float* ent_transfer, float* rel_transfer, const TransAccs& accs, int32_t d,
                                   const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B,
                                   float margin, float lr, float* losses, void* workspace, size_t workspace_bytes,
                                   hipStream_t st);

// ge_transr.hip: TransR scoring, Adam steps and native loop
int transr_max_dim();
size_t transr_ws_bytes(int64_t E, int64_t R, int32_t dE, int32_t dR, int64_t B);
int transr_score_launch(const TransModel& m, const int32_t* tri, int64_t B, float* out, hipStream_t st);
int transr_adam_step_run(int l1, float* ent, int64_t E, float* rel, float* rel_matrix, int64_t R, int32_t dE,
                         int32_t dR, float* m, float* v, const int32_t* pos, const int32_t* neg, int64_t B,
                         float margin, float lr, float b1, float b2, float eps, int64_t t, float* loss,
                         void* workspace, size_t workspace_bytes, hipStream_t st);
int transr_train_steps_run(int l1, float* ent, int64_t E, float* rel, float* rel_matrix, int64_t R, int32_t dE,
                           int32_t dR, float* m, float* v, const SamplerArgs& sa, uint64_t seed, uint64_t first_step,
                           int64_t n_steps, int64_t B, float margin, float lr, float b1, float b2, float eps,
                           int64_t first_t, float* losses, void* workspace, size_t workspace_bytes, hipStream_t st);

// The outputs of a rank sweep (entities or relations); known_off / known_rc: ge_known_cells' lists, or both null.
struct RankOut {
  const int32_t* known_off; const uint16_t* known_rc; int32_t* n_before; int32_t* n_known_before; float* true_dist;
  float* scores_out;
};

// ge_transx_rank.hip: link-prediction ranks of TransE / TransH / TransD / TransR over every entity.  The size
// functions read m's shape alone.
size_t trans_rank_ws_bytes(const TransModel& m, int64_t B);
int trans_rank_launch(const TransModel& m, const int32_t* tri, int64_t B, int cand_is_head, const RankOut& o,
                      void* workspace, size_t workspace_bytes, hipStream_t st);
// top-k prediction of the same models on the rank sweep's distances: k <= transx_topk_max_k()
int transx_topk_max_k();
size_t trans_topk_ws_bytes(const TransModel& m, int64_t B, int32_t k);
int trans_topk_launch(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head,
                      const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist,
                      void* workspace, size_t workspace_bytes, hipStream_t st);
// ge_transx_rank_masked.hip: the same two sweeps with per-row candidate sets (SetArgs) over the entities; the workspaces
// of the unmasked forms; o.scores_out unused
int trans_rank_masked_launch(const TransModel& m, const int32_t* tri, int64_t B, int cand_is_head, const RankOut& o,
                             const SetArgs& sets, void* workspace, size_t workspace_bytes, hipStream_t st);
int trans_topk_masked_launch(const TransModel& m, const int32_t* queries, int64_t B, int cand_is_head,
                             const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id,
                             float* out_dist, const SetArgs& sets, void* workspace, size_t workspace_bytes,
                             hipStream_t st);

// ge_transx_relrank.hip: relation prediction (h, ?, t) of TransE / TransH / TransD / TransR over every relation
size_t trans_relrank_ws_bytes(const TransModel& m, int64_t B);
int trans_relrank_launch(const TransModel& m, const int32_t* tri, int64_t B, const RankOut& o, void* workspace,
                         size_t workspace_bytes, hipStream_t st);

// ge_rotate.hip: RotatE (ent [E,d] as [Re | Im], rel [R,d/2] phases; d even, at most rotate_max_dim()): scoring, the
// hinge step and native loop (acc_ent / acc_rel both null: SGD; both set: AdaGrad), ranks over every entity.  One
// workspace size serves both optimizers and the loops.
int rotate_max_dim();
size_t rotate_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B);
int rotate_score_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const int32_t* tri,
                        int64_t B, float* out, hipStream_t st);
int rotate_step_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
                    const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr, float* loss,
                    void* workspace, size_t workspace_bytes, hipStream_t st);
int rotate_train_steps_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel,
                           int32_t d, const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps,
                           int64_t B, float margin, float lr, float* losses, void* workspace, size_t workspace_bytes,
                           hipStream_t st);
size_t rotate_rank_ws_bytes(int32_t d, int64_t B);
int rotate_rank_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d, const int32_t* tri,
                       int64_t B, int cand_is_head, const RankOut& o, void* workspace, size_t workspace_bytes,
                       hipStream_t st);

// ge_rotate_adv.hip: RotatE's self-adversarial negative-sampling loss on the same tables: B positives pos [B,3] with K
// replacing entities each (neg_ent [B,K], side [B]: 0 replaces the tail, 1 the head).  Per-row losses, the step (acc_ent /
// acc_rel both null: SGD; both set: AdaGrad), the draw of a step's (pos, side, neg_ent) and the native loop, which keeps
// them in the workspace.  One workspace size serves both optimizers and the loops.
int rotate_adv_max_negatives();
size_t rotate_adv_ws_bytes(int64_t E, int64_t R, int32_t d, int64_t B, int32_t K);
int rotate_adv_loss_launch(int l1, const float* ent, int64_t E, const float* rel, int64_t R, int32_t d,
                           const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                           float margin, float alpha, float* out, hipStream_t st);
int rotate_adv_step_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel, int32_t d,
                        const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                        float margin, float alpha, float lr, float* loss, void* workspace, size_t workspace_bytes,
                        hipStream_t st);
// (the draw reads no table: ge_transx_adv.hip's loops call it for TransE / TransH / TransD as well)
int rotate_adv_draw_launch(const SamplerArgs& s, int64_t B, int32_t K, uint64_t seed, uint64_t step, int32_t* pos,
                           int32_t* side, int32_t* neg_ent, hipStream_t st);
int rotate_adv_train_steps_run(int l1, float* ent, int64_t E, float* rel, int64_t R, float* acc_ent, float* acc_rel,
                               int32_t d, const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps,
                               int64_t B, int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                               size_t workspace_bytes, hipStream_t st);

// ge_transx_adv.hip: the same loss for TransE / TransH / TransD on ge_transx.hip's tables and distance: per-row losses, the
// step and the native loop (accs null: SGD; set: AdaGrad, the accumulators under their tables' names), with
// ge_rotate_adv.hip's batch, slots and draw.  The workspace depends on the model: TransE has no second gradient plane.
int transx_adv_max_negatives();
size_t transx_adv_ws_bytes(int model, int64_t E, int64_t R, int32_t d, int64_t B, int32_t K);
int transx_adv_loss_launch(const TransModel& m, const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B,
                           int32_t K, float margin, float alpha, float* out, hipStream_t st);
int transx_adv_step_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal, float* ent_transfer,
                        float* rel_transfer, const TransAccs* accs, int32_t d, const int32_t* pos, const int32_t* side,
                        const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr, float* loss,
                        void* workspace, size_t workspace_bytes, hipStream_t st);
int transx_adv_train_steps_run(int model, int l1, float* ent, int64_t E, float* rel, int64_t R, float* normal,
                               float* ent_transfer, float* rel_transfer, const TransAccs* accs, int32_t d,
                               const SamplerArgs& sa, uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B,
                               int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                               size_t workspace_bytes, hipStream_t st);

// ge_classify.hip: triple classification -- per-segment thresholds fitted from sorted labelled scores, the decision
size_t threshold_fit_ws_bytes(int64_t M, int32_t n_seg);
int threshold_fit_launch(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                         float* thr_lo, float* thr_hi, int32_t* best_correct, int32_t* n_pos, int32_t* n_neg,
                         void* workspace, hipStream_t st);
int threshold_classify_launch(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                              const float* thr, uint8_t* pred, int32_t* confusion, hipStream_t st);

}  // namespace ge
