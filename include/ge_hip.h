/* ge_hip.h -- flat C ABI of libge_hip.so, the MI355X (gfx950) drop-in for the hot path of
 * greysun/GraphEmbeddings' holE.py (gather -> max-norm clip -> ComplEx / HolE score -> sigmoid ->
 * pairwise hinge -> gradient of the SUM -> sparse SGD scatter), plus the type-safe corruption
 * sampler and the 1-vs-K candidate scorer.
 *
 * The holE.py path has no FFI of its own (it is in-process TensorFlow); the calling convention
 * below is the one the reference uses for its only native library, init.so
 * (init.cpp:47-48,129-142,223-224 loaded by transE.py:9-10, buffers passed as raw addresses
 * transE.py:95-112): C linkage, caller-owned caller-sized flat buffers, int32 ids.  Differences
 * that make it usable from a GPU training loop: every entry point returns an int status
 * (0 = ok, <0 = -errno style argument error, >0 = hipError_t), takes the hipStream_t it must
 * enqueue on (as void*), never synchronises, allocates no device memory of its own -- with ONE exception,
 * stated where it applies: ge_rank_1vK / ge_complex_rank_1vK / ge_rank_1vK_vs_loss / ge_topk_1vK_planes without a `planes` buffer and
 * ge_complex_score_1vK on large sweeps build the candidates' fp16 planes in a stream-ordered allocation
 * (hipMallocAsync / hipFreeAsync on `stream`, nothing outlives the call; pass ge_rank_planes' buffer to avoid it) --
 * and keeps no global state (the only state is inside the explicit ge_train_pipeline handle, see ge_train_steps).
 *
 * All pointers except where noted are DEVICE pointers (e.g. torch.Tensor.data_ptr()).
 * `table` is the single shared entity+relation table of holE.py:263-264: row-major fp32 [N, d],
 * first d/2 floats of a row = real parts, last d/2 = imaginary parts (holE.py:164-166).
 * Triples are int32 [B,3] in the reference's column order (head, tail, relation)
 * (holE.py:76-81, 181-185).  A triple with an id outside [0,N) yields NaN / is skipped.
 */
#ifndef GE_HIP_H
#define GE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GE_VERSION 449 /* 0.4.4.9: + ge_copy_if (a copy of up to 16 buffers gated by a device flag: the pocket of the translation models' validation ticks) */

/* argument errors (negative, -errno style) */
#define GE_EINVAL (-22)  /* bad dimension / null pointer / misaligned buffer */
#define GE_ENOTSUP (-95) /* dimension outside the compiled kernel range */
#define GE_ENOMEM (-12)  /* workspace too small */

/* ge_corrupt_batch modes */
#define GE_CORRUPT_BATCH_COIN 0 /* reference: one heads/tails coin per batch (holE.py:137-140) */
#define GE_CORRUPT_ROW_COIN 1   /* one coin per row (extension) */
#define GE_CORRUPT_HEADS 2      /* holE.py:97-114 */
#define GE_CORRUPT_TAILS 3      /* holE.py:117-133 */

/* model codes (ge_hinge_loss, ge_hinge_grad, ge_train_steps) */
#define GE_MODEL_COMPLEX 0       /* holE.py:191-192 */
#define GE_MODEL_HOLE 1          /* README.md:42 on a real-valued table */
#define GE_MODEL_HOLE_SPECTRAL 2 /* the same model on a table transformed by ge_hole_to_spectral */
#define GE_MODEL_HOLE_DIRECT 3   /* ge_train_steps only: force the direct-correlation kernels */
/* ge_train_steps only, OR-ed into `model` (prepared path): rows with more than 16 gradient slots in a step -- split over
 * several work items, whose partial sums otherwise meet by float atomics in scheduler order -- are reduced in a FIXED
 * order (one more launch per step), so that every row of the table is bitwise reproducible run to run whatever the ids'
 * distribution.  Off by default: it costs a launch per step (measured: DESIGN.md section 5). */
#define GE_STEP_DETERMINISTIC 0x100

/* ge_neighbor_dists / ge_neighbor_topk metrics */
#define GE_METRIC_COSINE 0    /* D = max(0, 1 - cos) */
#define GE_METRIC_EUCLIDEAN 1 /* D = sqrt(max(0, |q|^2 + |c|^2 - 2 |q| |c| cos)) */

int ge_version(void);

/* Largest embedding_dim the compiled kernels accept (score path / train path). */
int ge_max_dim(void);

/* --- evaluate_triples (holE.py:179-202), ComplEx: out[i] = sigma(sum_k Re(h_k r_k conj(t_k)))
 * with rows clipped to max_norm as tf.nn.embedding_lookup(max_norm=1) does (holE.py:162).
 * apply_sigmoid=0 returns the raw score.  d must be even.  out: [B] fp32. */
int ge_complex_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                     float max_norm, int apply_sigmoid, float* out, void* stream);
/* The same on a table whose rows are `ld` >= d floats apart (row i at table + i * ld; the reference's table is dense,
 * ld = d).  Exists to measure padded row layouts (800-byte rows straddle 64-byte sectors; profiles/r03_padded_rows.txt).
 * Any ld >= d is taken: a pitch that is no multiple of 4 (or 2) floats is read with narrower loads (GE_ENOTSUP above
 * d = 256, where the narrow kernels end). */
int ge_complex_score_strided(const float* table, int64_t N, int32_t d, int64_t ld, const int32_t* triples, int64_t B,
                             float max_norm, int apply_sigmoid, float* out, void* stream);

/* --- evaluate_triples(triple_batch, embeddings, label) in --log_loss mode (holE.py:194-196), forward only:
 * out[i] = log(1 + exp(-label * score_i)) + l2 * sum(table^2) / 2 (tf.nn.l2_loss of the WHOLE table).
 * workspace: >= 256 bytes of device scratch (the table's sum of squares), 256-byte aligned (else GE_EINVAL). */
int ge_complex_logloss(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B, float label,
                       float l2, float max_norm, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* --- HolE score of README.md:42: sigma(sum_k r_k [h (star) t]_k), circular correlation over the
 * full d real values of the clipped rows.  Same layout as ge_complex_score. */
int ge_hole_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                  float max_norm, int apply_sigmoid, float* out, void* stream);

/* --- HolE in the frequency domain.  ge_hole_to_spectral replaces every row x (d reals, d even, k = d/2)
 * IN PLACE by its half spectrum X_f = sum_n x_n exp(-2 pi i f n / d), packed into the same d floats as
 * [Re X_0 .. Re X_{k-1} | Re X_k, Im X_1 .. Im X_{k-1}] (X_0 and the Nyquist bin X_k are real);
 * ge_hole_from_spectral is the inverse.  On a spectral table the HolE score of README.md:42 is
 * (1/d) sum_f w_f Re(H_f R_f conj(T_f)), w_0 = w_k = 1, else 2 -- the ComplEx-shaped trilinear form --
 * and |x|^2 = (1/d) sum_f w_f |X_f|^2, so scoring, the max-norm clip and the SGD step run without any
 * transform (model GE_MODEL_HOLE_SPECTRAL).  ge_hole_spectral_score = ge_hole_score on such a table. */
int ge_hole_to_spectral(float* table, int64_t N, int32_t d, void* stream);
int ge_hole_from_spectral(float* table, int64_t N, int32_t d, void* stream);
int ge_hole_spectral_score(const float* table, int64_t N, int32_t d, const int32_t* triples, int64_t B,
                           float max_norm, int apply_sigmoid, float* out, void* stream);

/* --- evaluate_batch forward only (holE.py:222-234): loss[i] = max(E(pos_i) - E(neg_i) + margin, 0).
 * model: GE_MODEL_COMPLEX, GE_MODEL_HOLE or GE_MODEL_HOLE_SPECTRAL.  sig_out (nullable) receives E(pos) in
 * [0,B) and E(neg) in [B,2B). */
int ge_hinge_loss(const float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                  int64_t B, float margin, float max_norm, int model, float* loss, float* sig_out,
                  void* stream);

/* --- one validation tick of the training loop (holE.py:299-304, 351-360), enqueued without any host decision:
 * a batch of B triples drawn uniformly (with replacement, Philox keyed by (seed, counter)) from the device-resident
 * validation split valid [V,3]; type-safe negatives (ge_corrupt_batch with step = counter); the hinge of
 * ge_hinge_loss; its mean -> *mean_out (device); and the reference's "pocket": if the mean is below *best (device
 * scalar, start it at 2.0 as holE.py:336 does) then *best = mean and, when pocket is not NULL, pocket <- table.
 * The host reads the means whenever it likes (e.g. once per epoch) and knows from them which tick the pocket
 * holds.  workspace: >= ge_validation_workspace_bytes(B) (else GE_ENOMEM), 256-byte aligned (else GE_EINVAL). */
size_t ge_validation_workspace_bytes(int64_t B);
int ge_validation_tick(const float* table, int64_t N, int32_t d, const int32_t* valid, int64_t V, int64_t B,
                       const int32_t* id_to_type, const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids,
                       uint64_t seed, uint64_t counter, int32_t padded_size, int32_t mode, float margin, float max_norm,
                       int model, void* workspace, size_t workspace_bytes, float* mean_out, float* best, float* pocket,
                       void* stream);
/* The same tick for --log_loss (holE.py:194-196, 206-220 evaluated on a validation batch): the batch with label +1,
 * negative_ratio corrupted batches (ge_corrupt_batch with step = counter * negative_ratio + k) with label -1, every
 * loss = log(1 + exp(-y s)) + l2 * sum(table^2) / 2; mean over the (1 + negative_ratio) * B values, pocket and
 * workspace rules as above (ge_validation_logloss_workspace_bytes(B, negative_ratio) bytes). */
size_t ge_validation_logloss_workspace_bytes(int64_t B, int32_t negative_ratio);
int ge_validation_tick_logloss(const float* table, int64_t N, int32_t d, const int32_t* valid, int64_t V, int64_t B,
                               const int32_t* id_to_type, const int64_t* type_offsets, int32_t n_types,
                               const int32_t* type_ids, uint64_t seed, uint64_t counter, int32_t padded_size, int32_t mode,
                               int32_t negative_ratio, float l2, float max_norm, void* workspace, size_t workspace_bytes,
                               float* mean_out, float* best, float* pocket, void* stream);

/* --- one SGD step of holE.py:296 on the hinge of holE.py:231: forward of both sides, gradient of
 * SUM_i loss_i through sigmoid, score and the clip, then table[row] -= lr * grad for every
 * occurrence (ScatterSub semantics, duplicates accumulate; holE-20170724/graph.pbtxt:47850-48001).
 * Every gradient is evaluated against the table as it was before the call.  In place on `table`.
 * workspace: device scratch of at least ge_hinge_step_workspace_bytes(B, d) bytes, 256-B aligned.
 * loss: [B] fp32.  Rows that pos and neg share (relation, and the uncorrupted entity) are read
 * and updated once with the summed gradient. */
size_t ge_hinge_step_workspace_bytes(int64_t B, int32_t d);
int ge_complex_hinge_step(float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                          int64_t B, float margin, float lr, float max_norm, float* loss,
                          void* workspace, size_t workspace_bytes, void* stream);
int ge_hole_hinge_step(float* table, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                       int64_t B, float margin, float lr, float max_norm, float* loss,
                       void* workspace, size_t workspace_bytes, void* stream);

/* --- the --log_loss branch (holE.py:194-196, 206-220 + minimize, holE.py:296), ComplEx: `triples`
 * [M,3] is the concatenation of the B positives and negative_ratio corrupted batches, `labels` [M]
 * fp32 +1 / -1 (holE.py:209, 215).  loss[i] = log(1 + exp(-y_i s_i)) + l2 * sum(table^2)/2
 * (tf.nn.l2_loss of the WHOLE table, holE.py:196).  minimize() differentiates the SUM of the loss
 * vector, so the dense term counts once per row: table <- table*(1 - lr*M*l2) - lr * sparse grads.
 * workspace >= ge_logloss_step_workspace_bytes(M, d), 256-B aligned. */
size_t ge_logloss_step_workspace_bytes(int64_t M, int32_t d);
int ge_complex_logloss_step(float* table, int64_t N, int32_t d, const int32_t* triples, const float* labels,
                            int64_t M, float lr, float l2, float max_norm, float* loss, void* workspace,
                            size_t workspace_bytes, void* stream);

/* --- the two halves of the step, exposed for the row-sharded multi-GPU path (rows are fetched
 * from / gradients routed to their owner GPU between the halves).
 * ge_hinge_grad: `rows` is any [N,d] row store (the table itself, or a staging buffer of fetched
 * rows with pos/neg re-indexed into it).  Emits IndexedSlices: grad_idx [6B] int32 (row index in
 * `rows`, or -1 for an empty slot) and grad_val [6B,d] fp32 already multiplied by -lr, slot order
 * per pair: h+, t+, r+, h-, t-, r-.  model: GE_MODEL_COMPLEX, GE_MODEL_HOLE or GE_MODEL_HOLE_SPECTRAL
 * (then `rows` holds spectral rows and the emitted gradient rows are spectral too).
 * ge_scatter_add_rows: table[idx[i]] += val[i] for idx[i] >= 0, float atomics.
 * ge_gather_rows: out[i] = table[idx[i]] (zeros for idx[i] < 0). */
int ge_hinge_grad(const float* rows, int64_t N, int32_t d, const int32_t* pos, const int32_t* neg,
                  int64_t B, float margin, float lr, float max_norm, int model, float* loss,
                  int32_t* grad_idx, float* grad_val, void* stream);
int ge_scatter_add_rows(float* table, int64_t N, int32_t d, const int32_t* idx, const float* val,
                        int64_t R, void* stream);
int ge_gather_rows(const float* table, int64_t N, int32_t d, const int32_t* idx, int64_t R,
                   float* out, void* stream);

/* --- the optimizer half for AdaGrad: TF1's AdagradOptimizer(lr, initial_accumulator_value) in place of the
 * GradientDescentOptimizer of holE.py:296, on any IndexedSlices -- the counterpart of ge_scatter_add_rows.  `val` holds
 * MINUS the gradient (what ge_hinge_grad emits at lr = 1).  For every table row named by an idx[i] in [0, N):
 *   s = sum of its val rows (duplicates are summed first, in `perm` order),
 *   accum[row] += s * s,   table[row] += lr * s / sqrt(accum[row])   (the updated accumulator, no epsilon).
 * accum: the caller's [N,d] fp32 accumulator (filled with initial_accumulator_value before the first step), not
 * overlapping `table`.  perm [R] int32: the STABLE argsort of (idx[i] < 0 ? N : idx[i]) -- a row's occurrences are
 * consecutive in that order; an entry outside [0, R) and an id >= N are skipped and never dereferenced.  idx[i] < 0 is
 * skipped; rows not named are not touched in either array.  No float atomics: bitwise reproducible.  R = 0 returns 0. */
int ge_adagrad_rows(float* table, float* accum, int64_t N, int32_t d, const int32_t* idx, const float* val,
                    const int32_t* perm, int64_t R, float lr, void* stream);

/* --- 1-vs-all softmax training of ComplEx: the multiclass log-loss over all candidates ("1vsAll", Lacroix et al. 2018)
 * in place of the hinge of holE.py:231, on the candidate sweep of ge_complex_score_1vK (holE.py:564-569) -- extends
 * ge_hinge_loss / ge_hinge_grad to an objective the reference does not have.  hr [B,2] (fixed entity, relation),
 * true_id [B], cand [K] (distinct ids), loss [B] as for ge_rank_1vK.  With s_ij the un-squashed score of
 * ge_complex_score_1vK (rows clipped to max_norm on lookup) and z_ij = -scale * s_ij (lower score = more plausible):
 *   loss_i = logsumexp_j(z_ij) - z_i,true     (running maximum subtracted; no [B,K] array is ever formed)
 * A row whose fixed, relation or true id lies outside [0,N), or whose true id is not among the candidates, is invalid:
 * loss = NaN, no contribution to any gradient.  A candidate id outside [0,N) is left out of every softmax.
 * ge_softmax_grad is the counterpart of ge_hinge_grad: IndexedSlices of R = K + 2B slots, grad_idx [R] int32 and
 * grad_val [R,d] fp32 = -lr * the gradient of SUM_i loss_i taken through the three clips, against the table as it is:
 *   slot j < K: cand[j] (-1 for an id outside [0,N)); slot K + 2i: fixed_i; slot K + 2i + 1: rel_i (both -1 for an
 *   invalid row); an empty slot's row is zeros.  At lr = 1 the slices are what ge_adagrad_rows takes, scaled by lr what
 *   ge_scatter_add_rows takes.  Exact-fp32 MFMA, no float atomics: two identical calls give identical bits.
 * model: GE_MODEL_COMPLEX only (any other code GE_ENOTSUP).  embedding_dim % 8 == 0 in 8 ... ge_rank_max_dim(), else
 * GE_ENOTSUP; table 16-byte aligned.  GE_EINVAL: a null pointer; N, B, K or d < 1; scale <= 0 or not finite;
 * max_norm <= 0; a table off 16 bytes; a workspace off 256 bytes.  GE_ENOMEM: workspace_bytes below
 * ge_softmax_workspace_bytes(B, K, d) (monotone in each argument, a multiple of 256, 0 for sizes the calls refuse).
 * Nothing is allocated and the host never waits. */
size_t ge_softmax_workspace_bytes(int64_t B, int64_t K, int32_t d);
int ge_softmax_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                    const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                    float* loss, void* workspace, size_t workspace_bytes, void* stream);
int ge_softmax_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                    const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model, int cand_is_head,
                    float* loss, int32_t* grad_idx, float* grad_val, void* workspace, size_t workspace_bytes, void* stream);

/* --- sampled softmax with shared negatives: the objective above over K candidates that need NOT hold the true entity,
 * so that a step's work follows K and not the table.  Arguments, clips, s, z, cand_is_head and model as for
 * ge_softmax_loss / ge_softmax_grad.  cand [K] may hold any ids: duplicates are allowed and each slot is a term of its
 * own; an id outside [0,N) is an empty slot.  A row is valid iff its fixed, relation and true ids all lie in [0,N).  The
 * true entity counts once, through a logit of its own, z_i,true = -scale * (Q'_i . clip(true_i)), and every slot with
 * cand[j] == true_id[i] is left out of row i's softmax (accidental-hit removal):
 *   loss_i = log(exp(z_i,true) + SUM_{j: cand_j in [0,N), cand_j != true_i} exp(z_ij)) - z_i,true   (>= 0; NaN if invalid)
 * A row whose slots are all empty or left out has loss exactly 0 and exact zero gradient rows.
 * ge_softmax_sampled_grad emits IndexedSlices of R = K + 3B slots, grad_idx [R] int32 and grad_val [R,d] fp32 = -lr * the
 * gradient of SUM_i loss_i through all four clips, against the table as it is:
 *   slot j < K: cand[j] (-1 and a zero row for an empty slot); slot K + 3i: fixed_i; K + 3i + 1: rel_i; K + 3i + 2:
 *   true_i (all three -1 with zero rows for an invalid row).  At lr = 1 the slices are what ge_adagrad_rows takes.
 * No float atomics: two identical calls give identical bits.  Refusals as for ge_softmax_loss / ge_softmax_grad, in the
 * same order, against ge_softmax_sampled_workspace_bytes(B, K, d) (monotone in each argument, a multiple of 256, 0 for
 * sizes the calls refuse).  Nothing is allocated and the host never waits. */
size_t ge_softmax_sampled_workspace_bytes(int64_t B, int64_t K, int32_t d);
int ge_softmax_sampled_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                            const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                            float* loss, void* workspace, size_t workspace_bytes, void* stream);
int ge_softmax_sampled_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                            const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model,
                            int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                            size_t workspace_bytes, void* stream);

/* --- type-constrained 1-vs-all softmax: ge_softmax_loss / ge_softmax_grad with each row's softmax taken over the
 * candidates its set admits -- the training counterpart of the candidate sets of ge_rank_1vK_masked.  Everything is as
 * for ge_softmax_loss / ge_softmax_grad (clips, s, z, cand_is_head, model, validity, the R = K + 2B slots, grad_val = -lr *
 * the gradient of SUM_i loss_i, no float atomics, two identical calls give identical bits) except:
 *   row_set [B] int32, mask uint32 [n_sets][W], W = ge_candidate_mask_words(K): the sets in the format described at
 *   ge_candidate_mask_words -- a bit is addressed by candidate POSITION, bits at positions >= K are ignored,
 *   row_set[i] = -1 means unrestricted.
 *   loss_i = logsumexp_{j admissible for row i} z_ij - z_i,true;  w_ij = 0 exactly for an inadmissible pair.
 * A row is valid iff it is valid for ge_softmax_loss AND row_set[i] is -1 or in [0, n_sets) AND the position of its true
 * candidate is admissible; any other row (a row with an empty set among them) is invalid as there: loss = NaN, grad_idx
 * -1, zero rows, no contribution anywhere.  Candidate slot j keeps grad_idx[j] = cand[j] for an id in the table; a
 * candidate that no valid row admits gets an exact zero row (ge_adagrad_rows then leaves its table and accumulator bits
 * as they are).  With every bit set, or every row_set = -1, loss, grad_idx and grad_val equal ge_softmax_loss /
 * ge_softmax_grad's bit for bit.  A (64-row, 64-candidate) tile pair that no valid row admits is not computed: on sets
 * that follow the order of cand, the work follows the sets' sizes.  Non-finite table rows: unspecified, as there.
 * Refusals as for ge_softmax_loss / ge_softmax_grad, in the same order: a null row_set or mask and n_sets < 1 with the
 * null pointers, a mask off 4 bytes with the other alignments; GE_ENOMEM against ge_softmax_masked_workspace_bytes(B, K,
 * d) (ge_softmax_workspace_bytes' parts plus one bit per tile pair; monotone in each argument, a multiple of 256, 0 for
 * sizes the calls refuse).  Nothing is allocated and the host never waits. */
size_t ge_softmax_masked_workspace_bytes(int64_t B, int64_t K, int32_t d);
int ge_softmax_masked_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, int model, int cand_is_head,
                           float* loss, void* workspace, size_t workspace_bytes, const int32_t* row_set,
                           const uint32_t* mask, int32_t n_sets, void* stream);
int ge_softmax_masked_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                           const int32_t* cand, int64_t K, float max_norm, float scale, float lr, int model,
                           int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val, void* workspace,
                           size_t workspace_bytes, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                           void* stream);

/* --- multi-label (K-vs-all) softmax: one row per distinct QUERY (fixed, relation) with ALL its known answers as labels and
 * a target uniform over them, where ge_softmax_loss has one row per triple and one true candidate.  Clips, s, z, Q', C',
 * cand_is_head, model and empty candidate slots as for ge_softmax_loss / ge_softmax_grad.  Row i's labels are the candidate
 * POSITIONS label_pos[label_off[i] .. label_off[i + 1]) (label_off [B + 1], label_pos [L], int32, on the device), n_i of
 * them; a position named twice counts as two labels.
 *   loss_i = logsumexp_j z_ij - (1 / n_i) SUM_{l in labels_i} z_i,l
 *   dL/ds_ij = -scale * (softmax_j(z_ij) - y_ij / n_i),   y_ij = the number of labels of row i at position j
 * A row is valid iff its fixed and relation ids lie in [0,N), 0 <= label_off[i] < label_off[i + 1] <= L, and every label
 * is a position in [0,K) whose candidate id lies in [0,N); any other row has loss = NaN and contributes to no gradient.
 * Offsets that decrease or point past L invalidate rows and are never followed out of bounds.
 * ge_softmax_labels_grad emits IndexedSlices of R = K + 2B + L slots, grad_val [R,d] = -lr * the gradient of SUM_i loss_i
 * through the clips, against the table as it is:
 *   slot j < K: cand[j], the dense part (the softmax term) of the candidate's gradient; slot K + 2i: fixed_i;
 *   K + 2i + 1: rel_i, both with the label term included (-1 and zero rows for an invalid row);
 *   slot K + 2B + x: the candidate id of label entry x, with the label term of that candidate's gradient from the row the
 *   entry belongs to: the clip derivative of the candidate row applied to (scale / n_i) Q'_i, which is linear in its
 *   argument, so the slices of one table row sum to its gradient (-1 and a zero row for an entry of an invalid row or of
 *   none).  At lr = 1 the slices are what ge_adagrad_rows takes.  No [B,K] array, no float atomics: two identical calls
 *   give identical bits.
 * Refusals as for ge_softmax_loss / ge_softmax_grad, in the same order: a null label_off or label_pos and L < 0 with the
 * null pointers (L = 0 is taken: every row is then invalid); N > INT32_MAX with GE_ENOTSUP; GE_ENOMEM against
 * ge_softmax_labels_workspace_bytes(B, K, d, L) (ge_softmax_workspace_bytes' parts plus the label-sum rows [B,d], the label
 * means [B] and a row-of-entry array [L]; monotone in each argument, a multiple of 256, 0 for sizes the calls refuse).
 * Nothing is allocated and the host never waits. */
size_t ge_softmax_labels_workspace_bytes(int64_t B, int64_t K, int32_t d, int64_t L);
int ge_softmax_labels_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                           const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                           int model, int cand_is_head, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int ge_softmax_labels_grad(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* label_off,
                           const int32_t* label_pos, int64_t L, const int32_t* cand, int64_t K, float max_norm, float scale,
                           float lr, int model, int cand_is_head, float* loss, int32_t* grad_idx, float* grad_val,
                           void* workspace, size_t workspace_bytes, void* stream);

/* --- corrupt_batch (holE.py:152-153 -> 136-140 -> 97-133) fused with the per-batch host
 * resample of holE.py:343-347.  id_to_type [N] int32 type code per table row (-1 = unknown, the
 * reference's '?' default -> corrupted id -1, holE.py:39); type lists as CSR type_offsets
 * [n_types+1] int64 / type_ids int32.  Row i's replaced entity is drawn as the reference does:
 * uniform slot in [0,padded_size) of a per-batch with-replacement subsample of its type's list
 * (padded_size = 0: uniform over the whole list).  Randomness is a counter-based Philox4x32-10
 * stream keyed by (seed, step, row/type) -- no state, bitwise reproducible (oracle/hole_oracle.py
 * states the stream).  neg: [B,3] int32. */
int ge_corrupt_batch(const int32_t* pos, int64_t B, const int32_t* id_to_type, int64_t N,
                     const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids,
                     uint64_t seed, uint64_t step, int32_t padded_size, int32_t mode, int32_t* neg,
                     void* stream);

/* --- Bernoulli filtered corruption: GPU form of the reference's native TransX sampler init.so
 * (getBatch / corrupt_head / corrupt_tail, init.cpp:159-246; tph/hpt statistics init.cpp:107-127).
 * Known triples are given as two sorted indexes: bh_* sorted by (head, relation, tail) with
 * bh_key = head*n_rel + relation and bh_ent = tail; bt_* sorted by (tail, relation, head) likewise.
 * tail_threshold[r] = floor(2^32 * hpt_r / (hpt_r + tph_r)): a row corrupts its TAIL iff a uniform
 * 32-bit word is below it, else its head (init.cpp:226-228).  The replacement is uniform over the
 * entities [ent_lo, ent_lo+n_ent) that do not complete a known triple (filtered, init.cpp:177-188).
 * Unlike init.so (void returns, one global LCG, not thread-safe) this is stateless: per-row
 * Philox4x32-10 draws keyed by (seed, step, row); oracle/transx_oracle.py states the stream and is
 * itself pinned against the compiled init.cpp. */
int ge_bernoulli_corrupt_batch(const int32_t* pos, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                               const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                               const uint32_t* tail_threshold, int32_t n_rel, int32_t ent_lo,
                               int32_t n_ent, uint64_t seed, uint64_t step, int32_t* neg, void* stream);

/* --- TransE / TransH / TransD (transE.py, transH.py, transD.py).  Separate tables, row-major fp32:
 * ent [n_ent,d] and rel [n_rel,d]; TransH adds normal [n_rel,d] (normal_vector); TransD adds ent_transfer
 * [n_ent,d] and rel_transfer [n_rel,d].  A table the model does not have is passed as NULL (and ignored).
 * Entity ids are rows of ent, [0, n_ent); relation ids rows of rel.  Triples are int32 [B,3] (h, t, r).
 *   D = sum_k |h_p + r - t_p| (l1 != 0) or sum_k (h_p + r - t_p)^2 (l1 = 0), with the projection
 *   TransE e;  TransH e - (e.n^) n^, n^ = n * rsqrt(max(n.n, 1e-12));  TransD e + (e.e_p) r_p.
 * 1 <= d <= ge_transx_max_dim() (1024); d % 4 == 0 with 16-byte aligned tables takes the vectorised path. */
#define GE_TRANSX_TRANSE 0
#define GE_TRANSX_TRANSH 1
#define GE_TRANSX_TRANSD 2
int ge_transx_max_dim(void);
/* out[i] = D of triple i ([B] fp32); NaN for a triple with an id out of range. */
int ge_transx_score(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                    const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                    const int32_t* triples, int64_t B, float* out, void* stream);
/* Workspace of one hinge step / of ge_transx_train_steps for B pairs (the same size serves both). */
size_t ge_transx_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B);
/* One SGD step of loss = sum_i max(D(pos_i) - D(neg_i) + margin, 0) (a sum, not a mean) on every table of the
 * model: gradients on the pre-step tables with TF's rules (a pair is active iff D+ - D- + margin >= 0,
 * d|x|/dx = sign(x) with sign(0) = 0, the l2_normalize clamp differentiated on the branch max() takes),
 * duplicate rows summed in slot order, then row -= lr * sum.  neg_i must keep pos_i's relation; a pair with
 * an id out of range or neg_r != pos_r is skipped.  *loss (device, one float) = the batch loss before the step.
 * Bitwise reproducible: no float atomics. */
int ge_transx_hinge_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                         float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* neg,
                         int64_t B, float margin, float lr, float* loss, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The batch draw of the native loop (init.cpp getBatch, 224-246): pos_i = triples[(w * T) >> 32] with w a
 * Philox4x32-10 word keyed by (seed, step, i), then neg_i = the Bernoulli corruption of pos_i
 * (ge_bernoulli_corrupt_batch with ent_lo = 0, n_ent entities, the same seed and step). */
int ge_transx_draw_batch(const int32_t* triples, int64_t T, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                         const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold,
                         int32_t n_rel, int32_t n_ent, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg,
                         void* stream);
/* n_steps steps in one call: step s draws its batch as ge_transx_draw_batch(.., seed, first_step + s, ..) and runs
 * ge_transx_hinge_step on it; losses[s] (device) = its batch loss.  No host synchronisation inside. */
int ge_transx_train_steps(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                          float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* triples, int64_t T,
                          const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                          int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                          int64_t n_steps, int64_t B, float margin, float lr, float* losses, void* workspace,
                          size_t workspace_bytes, void* stream);
/* ge_transx_hinge_step with TF1's AdagradOptimizer(lr, initial_accumulator_value).minimize(loss) in place of the
 * GradientDescentOptimizer of transE.py:76 / transH.py:91 / transD.py:94, on the IndexedSlices of every table's lookups.
 * Each table X of the model has an accumulator acc_X of X's shape (fp32, filled by the caller with
 * initial_accumulator_value > 0 before the first step).  For every row that an ACTIVE pair names, in every table:
 *   s = the sum of its gradient rows (the gradient, not minus it; duplicates summed first, in the order
 *       ge_transx_hinge_step sums them),
 *   acc_X[row] += s * s,   X[row] -= lr * s / sqrtf(acc_X[row])   (the updated accumulator, no epsilon: the element
 *   rule of ge_adagrad_rows).
 * A row no active pair names is not touched in either array.  The loss, the activity rule, sign(0) = 0, the TransH clamp
 * branch and the skipping of invalid pairs are ge_transx_hinge_step's.  No float atomics: two calls from one state give
 * the same bits in tables, accumulators and loss.
 * Refused before any launch, in this order: whatever ge_transx_hinge_step refuses about the model and its tables;
 * GE_EINVAL for a missing accumulator of a table the model has, then for an accumulator that is not 4-byte aligned, then
 * for an accumulator whose [rows * d] floats share a byte with a table of the model or with another accumulator; then
 * everything else ge_transx_hinge_step refuses; GE_ENOMEM below ge_transx_step_workspace_bytes(n_ent, n_rel, d, B), which
 * serves both optimizers.  An accumulator of a table the model does not have is ignored, as its table is.  d % 4 == 0
 * takes the vectorised path when the accumulators are 16-byte aligned too. */
int ge_transx_adagrad_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                           float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel, float* acc_normal,
                           float* acc_ent_transfer, float* acc_rel_transfer, int32_t d, const int32_t* pos,
                           const int32_t* neg, int64_t B, float margin, float lr, float* loss, void* workspace,
                           size_t workspace_bytes, void* stream);
/* ge_transx_train_steps with that step: step s draws its batch as ge_transx_draw_batch(.., seed, first_step + s, ..)
 * (the SGD loop's draw) and runs ge_transx_adagrad_step on it; losses[s] (device) = its batch loss.  Refusals: those of
 * ge_transx_adagrad_step about the accumulators, in its order, then those of ge_transx_train_steps (the sampler checks
 * included), then GE_ENOMEM.  n_steps = 0 returns 0 after the checks.  No host synchronisation inside. */
int ge_transx_train_steps_adagrad(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                                  float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel,
                                  float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer, int32_t d,
                                  const int32_t* triples, int64_t T, const int64_t* bh_key, const int32_t* bh_ent,
                                  const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                                  const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                                  int64_t B, float margin, float lr, float* losses, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* --- RotatE (Sun et al., ICLR 2019): the translation model in the complex plane, t ~ h o r with |r_j| = 1.
 * Row-major fp32 tables: ent [n_ent,d], d even, k = d / 2, a row [Re (k) | Im (k)] (the ComplEx table's split);
 * rel [n_rel,k] holds PHASES theta in radians, unconstrained: never wrapped, never normalised.  The rotation is
 * (c, s) = (cosf theta, sinf theta) from the accurate sincosf.  With u_j = h_j e^{i theta_j} - t_j (complex) and
 * m_j = sqrtf(Re u_j^2 + Im u_j^2):
 *   D = sum_j m_j (l1 != 0, the paper's norm)  or  D = sum_j m_j^2 (l1 = 0, no square root).
 * Gradients: dD/du_j = g_j = u_j / m_j (0 where m_j == 0; 2 u_j for the squared norm), dD/dh_j = g_j conj(e^{i theta_j}),
 * dD/dt_j = -g_j, dD/dtheta_j = Re g_j (-Im w_j) + Im g_j Re w_j with w_j = h_j e^{i theta_j}.
 * Triples are int32 [B,3] (h, t, r).  The arguments follow the ge_transx_* entry points without `model`, with
 * (ent, n_ent, rel, n_rel, d) in place of the five tables and (acc_ent, acc_rel) as the AdaGrad accumulators
 * (acc_rel is [n_rel,k]).  Refused before any launch, in this order: GE_EINVAL for a null table, n_ent or n_rel < 1,
 * n_ent + n_rel >= 2^31 or d < 1; GE_ENOTSUP for an odd d or d > ge_rotate_max_dim() (1024); GE_EINVAL for a table
 * that is not 4-byte aligned; (AdaGrad) GE_EINVAL for an accumulator that is missing, not 4-byte aligned, or shares a
 * byte with a table or the other accumulator; then whatever the ge_transx_* counterpart refuses about its other
 * arguments; GE_ENOMEM below the size function, which answers 0 for a refused shape.  d % 8 == 0 with 16-byte aligned
 * buffers takes the vectorised path, every other even d the scalar one.
 * Not provided for this model: top-k prediction, candidate sets, relation prediction, multi-GPU. */
int ge_rotate_max_dim(void);
/* out[i] = D of triple i ([B] fp32); NaN for a triple with an id out of range. */
int ge_rotate_score(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                    const int32_t* triples, int64_t B, float* out, void* stream);
/* Workspace of one step (either optimizer) / of either native loop for B pairs: one size serves all four. */
size_t ge_rotate_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B);
/* ge_transx_hinge_step's step on the two tables: loss = sum_i max(D(pos_i) - D(neg_i) + margin, 0), a pair active iff
 * that argument is >= 0, gradients on the pre-step tables, duplicates summed in slot order (4i..4i+3 = pos h, pos t,
 * neg h, neg t; 4B+i = the relation), row -= lr * sum.  neg_i must keep pos_i's relation; a pair with an id out of
 * range or another relation is skipped.  *loss (device, one float) = the batch loss before the step.  No float atomics:
 * two calls from one state give the same bits. */
int ge_rotate_hinge_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* pos,
                         const int32_t* neg, int64_t B, float margin, float lr, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same step with ge_transx_adagrad_step's update: per row an active pair names, s = its summed gradient,
 * acc[row] += s * s, row -= lr * s / sqrtf(acc[row]), on ent and on rel.  A row no active pair names is untouched in
 * either array. */
int ge_rotate_adagrad_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent, float* acc_rel,
                           int32_t d, const int32_t* pos, const int32_t* neg, int64_t B, float margin, float lr,
                           float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* n_steps steps in one call: step s draws its batch as ge_transx_draw_batch(.., seed, first_step + s, ..) and runs
 * ge_rotate_hinge_step (ge_rotate_adagrad_step) on it; losses[s] (device) = its batch loss.  n_steps = 0 returns 0 after
 * the checks.  No host synchronisation inside. */
int ge_rotate_train_steps(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* triples,
                          int64_t T, const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key,
                          const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold, uint64_t seed,
                          uint64_t first_step, int64_t n_steps, int64_t B, float margin, float lr, float* losses,
                          void* workspace, size_t workspace_bytes, void* stream);
int ge_rotate_train_steps_adagrad(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                                  float* acc_rel, int32_t d, const int32_t* triples, int64_t T, const int64_t* bh_key,
                                  const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                                  const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                                  int64_t B, float margin, float lr, float* losses, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Link-prediction ranks over every entity, ge_transx_rank's contract: candidates c in [0, n_ent) replace the tail
 * (cand_is_head = 0) or the head; ascending (D, entity id); n_before, n_known_before (known_off / known_rc:
 * ge_known_cells' lists, or both NULL), true_dist, optional scores_out [B, n_ent]; -1 / -1 / NaN for a row with an id out
 * of range.  A row kernel stores q = h o e^{i theta} (tail side) or t o e^{-i theta} (head side) once; the sweep, the
 * true distance and the filter pass evaluate one arithmetic on it, so the target never ranks before itself and the
 * filter counts exactly the cells the sweep counted. */
size_t ge_rotate_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B);
int ge_rotate_rank(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                   const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_dist,
                   float* scores_out, void* workspace, size_t workspace_bytes, void* stream);

/* --- RotatE, the self-adversarial negative-sampling loss (Sun et al., ICLR 2019, eq. 5-6) on the same tables.
 * A batch has B positives pos [B,3] (h, t, r) with K negatives each; row i's negatives all replace the same side:
 * side [B] int32 (0: the tail is replaced, 1: the head), neg_ent [B,K] int32 the replacing entity ids; negative j of row i
 * is (h, neg_ent[i,j], r) or (neg_ent[i,j], t, r).  D = ge_rotate_score's distance in either norm, gamma = margin,
 * alpha = adversarial_temperature >= 0:
 *   p_ij   = softmax_j(-alpha D-_ij) over row i's live slots, a constant for the gradient (not differentiated)
 *   loss_i = softplus(D+_i - gamma) + sum_j p_ij softplus(gamma - D-_ij)       softplus(x) = log(1 + e^x) = -log sigma(-x)
 *   loss   = sum_i loss_i
 *   dloss/dD+_i = sigma(D+_i - gamma)        dloss/dD-_ij = -p_ij sigma(gamma - D-_ij)
 * The batch loss is a sum, as in every step of this family; the paper's (mean + mean) / 2 is this divided by 2B, a factor
 * on lr.  alpha = 0 gives p = 1 / n_i, the paper's uniform baseline.
 * Live slots and invalid rows: a slot whose id is outside [0, n_ent) is empty -- left out of the softmax, no gradient, its
 * sort key the sentinel n_ent + n_rel; a row whose slots are all empty keeps its positive term alone; a slot that holds
 * the true entity is an ordinary negative.  A row is invalid if a positive id is out of range or side is outside {0, 1}:
 * it contributes 0 and names no row (ge_rotate_adv_loss writes NaN for it).  There are no inactive pairs: every valid row
 * names its rows.
 * Arithmetic: fp32 with the accurate expf / log1pf; softplus(x) = fmaxf(x, 0) + log1pf(expf(-fabsf(x))); sigma in the
 * form that never overflows; the softmax max-subtracted (at alpha = 0 the exponent is 0 whatever D is); every sum in a
 * fixed order.  On the head side the distances are evaluated as |h' - t e^{-i theta}| (the rank sweep's identity), on
 * the tail side as |h e^{i theta} - t'|.
 * The update is ge_rotate_hinge_step's / ge_rotate_adagrad_step's: gradients on the pre-step tables, duplicates summed in
 * slot order by the same sort-and-apply stage, relation rows k = d / 2 wide.  Gradient slots of row i: (K+2) i + 0 and
 * + 1 the positive's head and tail, (K+2) i + 2 + j negative j's replacing entity, (K+2) B + i the relation;
 * n = (K+3) B slots in all.  The fixed entity of row i (h on the tail side, t on the head side) and its relation are the
 * same table rows in the positive and in all K negatives: the negatives' contributions are added into the positive's slot
 * for that entity and into the relation's slot in a fixed order (groups of j = q mod NT ascending, then a fixed tree),
 * not written as K more rows.  No float atomics: two calls from one state give the same bits in the tables, the
 * accumulators and the loss.
 * Refused before any launch, in this order: what ge_rotate_hinge_step (ge_rotate_adagrad_step) refuses about the shape,
 * the tables and the accumulators; GE_EINVAL for K < 1; GE_ENOTSUP for K > ge_rotate_adv_max_negatives() (1024);
 * GE_EINVAL for (K + 3) B >= 2^31; GE_EINVAL for a null side or neg_ent (steps and ge_rotate_adv_loss with B > 0);
 * GE_EINVAL for a margin or alpha that is not finite, then for alpha < 0; then GE_EINVAL for B < 1 (ge_rotate_adv_loss:
 * B < 0; its B = 0 returns 0), a null or misaligned pos / side / neg_ent / loss(es) / workspace, n_steps < 0 and a bad
 * sampler, as the hinge counterpart; GE_ENOMEM below the size function. */
int ge_rotate_adv_max_negatives(void);
/* Workspace of one step (either optimizer) / of either native loop: one size serves all four; 0 for a refused shape
 * (the tables' sizes, d, B < 1, K outside [1, max], (K + 3) B >= 2^31). */
size_t ge_rotate_adv_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t K);
/* out[i] = loss_i ([B] fp32); NaN for an invalid row. */
int ge_rotate_adv_loss(int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel, int32_t d,
                       const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                       float margin, float alpha, float* out, void* stream);
/* One SGD step (row -= lr * sum) / one AdaGrad step (acc += s * s, row -= lr * s / sqrtf(acc)) on the loss above; *loss
 * (device, one float) = the batch loss before the step. */
int ge_rotate_adv_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d, const int32_t* pos,
                       const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha,
                       float lr, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int ge_rotate_adv_adagrad_step(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                               float* acc_rel, int32_t d, const int32_t* pos, const int32_t* side,
                               const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr,
                               float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* The batch of (seed, step): pos and the replaced side are ge_transx_draw_batch's of the same (seed, step) -- the same
 * Philox words -- and neg_ent[i,j] is the entity that the word at row index i K + j under the tag 'advp' draws among
 * those that are not known completions of (fixed entity, r): ge_bernoulli_corrupt_batch's pick with ent_lo = 0.  Picks
 * may repeat.  A key with no free entity gives -1 in all K slots.  Refused: what ge_transx_draw_batch refuses, then K as
 * above, then null outputs with B > 0.  The draw reads no table: it is also the draw of ge_transx_adv_train_steps*. */
int ge_rotate_adv_draw_batch(const int32_t* triples, int64_t T, int64_t B, const int64_t* bh_key, const int32_t* bh_ent,
                             const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                             const uint32_t* tail_threshold, int32_t n_rel, int32_t n_ent, uint64_t seed, uint64_t step,
                             int32_t K, int32_t* pos, int32_t* side, int32_t* neg_ent, void* stream);
/* n_steps steps in one call: step s draws ge_rotate_adv_draw_batch(.., seed, first_step + s, K, ..) into the workspace and
 * runs ge_rotate_adv_step (ge_rotate_adv_adagrad_step) on it; losses[s] (device) = its batch loss.  n_steps = 0 returns 0
 * after the checks.  No host synchronisation inside. */
int ge_rotate_adv_train_steps(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, int32_t d,
                              const int32_t* triples, int64_t T, const int64_t* bh_key, const int32_t* bh_ent,
                              const int64_t* bt_key, const int32_t* bt_ent, int64_t n_known,
                              const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step, int64_t n_steps,
                              int64_t B, int32_t K, float margin, float alpha, float lr, float* losses, void* workspace,
                              size_t workspace_bytes, void* stream);
int ge_rotate_adv_train_steps_adagrad(int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* acc_ent,
                                      float* acc_rel, int32_t d, const int32_t* triples, int64_t T,
                                      const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key,
                                      const int32_t* bt_ent, int64_t n_known, const uint32_t* tail_threshold,
                                      uint64_t seed, uint64_t first_step, int64_t n_steps, int64_t B, int32_t K,
                                      float margin, float alpha, float lr, float* losses, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* --- TransE / TransH / TransD, the self-adversarial negative-sampling loss: ge_rotate_adv_*'s loss on ge_transx_*'s
 * tables.  The tables, the distance D, the projections and TransH's clamp are ge_transx_score's (model, l1, the five
 * tables, d); the batch (pos [B,3], side [B], neg_ent [B,K]), gamma = margin, alpha, p_ij, loss_i, the two coefficients,
 * live slots, invalid rows, the fp32 forms of softplus / sigma / the softmax, the (K+3) B gradient slots and the draw are
 * ge_rotate_adv_*'s above, word for word.
 * Gradients: a triple with coefficient a (sigma(D+ - gamma), or -p_ij sigma(gamma - D-_ij)) contributes a times the
 * hinge step's gradient of D: sign(0) = 0 for L1, TransH's l2_normalize differentiated on the branch max takes (ties to
 * n.n).  Plane 0 of a slot carries the ent / rel gradient, plane 1 ent_transfer on entity slots (TransD) and
 * normal_vector / rel_transfer on the relation slot.  The fixed entity and the relation of row i are the same table rows
 * in the positive and all K negatives: their K + 1 contributions are summed into the positive's slot for that entity and
 * into the relation slot, in both planes, in a fixed order (a team's negatives j = q, q + NT, ... ascending, a fixed tree
 * over the teams, the positive's term last); through TransH's normalisation that sum goes once.  The update is
 * ge_transx_hinge_step's / ge_transx_adagrad_step's sort-and-apply stage.  No float atomics: two calls from one state
 * give the same bits in every table, accumulator and loss.
 * Refused before any launch, in this order: what ge_transx_hinge_step (ge_transx_adagrad_step) refuses about the model,
 * its tables and accumulators; GE_EINVAL for K < 1; GE_ENOTSUP for K > ge_transx_adv_max_negatives() (1024); GE_EINVAL for
 * (K + 3) B >= 2^31; GE_EINVAL for a null side or neg_ent (steps and ge_transx_adv_loss with B > 0); GE_EINVAL for a
 * margin or alpha that is not finite, then for alpha < 0; then GE_EINVAL for B < 1 (ge_transx_adv_loss: B < 0; its B = 0
 * returns 0), a null or misaligned pos / side / neg_ent / loss(es) / workspace, n_steps < 0 and a bad sampler, as the
 * hinge counterpart; GE_ENOMEM below the size function. */
int ge_transx_adv_max_negatives(void);
/* Workspace of one step (either optimizer) / of either native loop of `model`: TransE has one gradient plane, TransH and
 * TransD two.  Monotone in B, K and d, a multiple of 256; 0 for a refused shape (the model code, the tables' sizes, d,
 * B < 1, K outside [1, max], (K + 3) B >= 2^31). */
size_t ge_transx_adv_step_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t K);
/* out[i] = loss_i ([B] fp32); NaN for an invalid row. */
int ge_transx_adv_loss(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                       const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                       const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                       float margin, float alpha, float* out, void* stream);
/* One SGD step (row -= lr * sum) / one AdaGrad step (acc += s * s, row -= lr * s / sqrtf(acc)) on the loss above; *loss
 * (device, one float) = the batch loss before the step. */
int ge_transx_adv_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                       float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* pos, const int32_t* side,
                       const int32_t* neg_ent, int64_t B, int32_t K, float margin, float alpha, float lr, float* loss,
                       void* workspace, size_t workspace_bytes, void* stream);
int ge_transx_adv_adagrad_step(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                               float* ent_transfer, float* rel_transfer, float* acc_ent, float* acc_rel,
                               float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer, int32_t d,
                               const int32_t* pos, const int32_t* side, const int32_t* neg_ent, int64_t B, int32_t K,
                               float margin, float alpha, float lr, float* loss, void* workspace, size_t workspace_bytes,
                               void* stream);
/* n_steps steps in one call: step s draws ge_rotate_adv_draw_batch(.., seed, first_step + s, K, ..) -- the draw reads no
 * table, so both families share it -- into the workspace and runs ge_transx_adv_step (ge_transx_adv_adagrad_step) on it;
 * losses[s] (device) = its batch loss.  n_steps = 0 returns 0 after the checks.  No host synchronisation, no allocation. */
int ge_transx_adv_train_steps(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel, float* normal,
                              float* ent_transfer, float* rel_transfer, int32_t d, const int32_t* triples, int64_t T,
                              const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                              int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                              int64_t n_steps, int64_t B, int32_t K, float margin, float alpha, float lr, float* losses,
                              void* workspace, size_t workspace_bytes, void* stream);
int ge_transx_adv_train_steps_adagrad(int model, int l1, float* ent, int64_t n_ent, float* rel, int64_t n_rel,
                                      float* normal, float* ent_transfer, float* rel_transfer, float* acc_ent,
                                      float* acc_rel, float* acc_normal, float* acc_ent_transfer, float* acc_rel_transfer,
                                      int32_t d, const int32_t* triples, int64_t T, const int64_t* bh_key,
                                      const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                                      int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                                      int64_t n_steps, int64_t B, int32_t K, float margin, float alpha, float lr,
                                      float* losses, void* workspace, size_t workspace_bytes, void* stream);

/* --- TransR (transR.py).  Row-major fp32 tables: ent [n_ent,dim_e], rel [n_rel,dim_r] and rel_matrix
 * [n_rel, dim_r*dim_e], whose row r read as [dim_r][dim_e] is M_r.  Triples are int32 [B,3] (h, t, r).
 *   u = M_r (h - t) + r (one mat-vec on the difference), D = sum_k |u_k| (l1 != 0) or sum_k u_k^2 (l1 = 0).
 * 1 <= dim_e, dim_r <= ge_transr_max_dim() (256); dim_e and dim_r % 4 == 0 with 16-byte aligned buffers takes the
 * vectorised path.  Adam state: m and v are two flat fp32 buffers of n_ent*dim_e + n_rel*dim_r + n_rel*dim_r*dim_e
 * floats each, laid out [ent | rel | rel_matrix] in the tables' own row-major order; zero them before step t = 1. */
int ge_transr_max_dim(void);
/* out[i] = D of triple i ([B] fp32); NaN for a triple with an id out of range. */
int ge_transr_score(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                    int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B, float* out, void* stream);
/* Workspace of one Adam step / of ge_transr_train_steps for B pairs (the same size serves both). */
size_t ge_transr_step_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B);
/* One step of tf.train.AdamOptimizer (transR.py:88) on loss = sum_i max(D(pos_i) - D(neg_i) + margin, 0), t >= 1
 * the 1-based step.  Gradients on the pre-step tables with TF's rules (a pair is active iff D+ - D- + margin >= 0;
 * d|x|/dx = sign(x) with sign(0) = 0); neg_i must keep pos_i's relation, a pair with an id out of range or
 * neg_r != pos_r is skipped.  Duplicate rows are summed first (TF 1.x deduplicates IndexedSlices before its sparse
 * Adam), so v receives (1-b2) (sum g)^2.  Then on EVERY element of the three tables, g = 0 where the batch did not
 * touch the row:  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  x -= lr_t m / (sqrt(v) + eps),  with
 * lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) computed in double from t (not a running fp32 product of b1 and b2).
 * Needs 0 <= b1 < 1, 0 <= b2 < 1, eps >= 0.  *loss (device, one float) = the batch loss before the step.
 * Bitwise reproducible: no float atomics. */
int ge_transr_adam_step(int l1, float* ent, int64_t n_ent, float* rel, float* rel_matrix, int64_t n_rel, int32_t dim_e,
                        int32_t dim_r, float* m, float* v, const int32_t* pos, const int32_t* neg, int64_t B,
                        float margin, float lr, float b1, float b2, float eps, int64_t t, float* loss, void* workspace,
                        size_t workspace_bytes, void* stream);
/* n_steps Adam steps in one call: step s draws its batch as ge_transx_draw_batch(.., seed, first_step + s, ..) and
 * runs ge_transr_adam_step on it with t = first_t + s; losses[s] (device) = its batch loss.  No host
 * synchronisation inside. */
int ge_transr_train_steps(int l1, float* ent, int64_t n_ent, float* rel, float* rel_matrix, int64_t n_rel,
                          int32_t dim_e, int32_t dim_r, float* m, float* v, const int32_t* triples, int64_t T,
                          const int64_t* bh_key, const int32_t* bh_ent, const int64_t* bt_key, const int32_t* bt_ent,
                          int64_t n_known, const uint32_t* tail_threshold, uint64_t seed, uint64_t first_step,
                          int64_t n_steps, int64_t B, float margin, float lr, float b1, float b2, float eps,
                          int64_t first_t, float* losses, void* workspace, size_t workspace_bytes, void* stream);

/* --- link-prediction ranks of the translation models over EVERY entity, counted in the distance sweep (no [B, n_ent]
 * matrix).  Row i = (h, t, r) of triples [B,3]: the candidates c in [0, n_ent) replace the tail (cand_is_head = 0,
 * D_c = D(h, c, r)) or the head (D_c = D(c, t, r)), D as ge_transx_score / ge_transr_score state it, computed as
 * sum_k term(q_k - P_c,k) with q = proj(h) + r (tail side) or proj(t) - r (head side) and P_c = proj(c):
 *     n_before[i]       = #{c : D_c < D_true, or D_c == D_true and c < true}   (ascending (D, id); raw rank = 1 + it)
 *     n_known_before[i] = how many of those c are listed in known_off / known_rc  (filtered rank = raw - it)
 *     true_dist[i]      = D_true, computed by the same arithmetic as every D_c of the row (and of the filter pass)
 * The known cells are ge_known_cells' lists for these rows with pos_of = the identity (candidate position = entity
 * id); known_off = known_rc = NULL ranks unfiltered (n_known_before = 0).  A row with an id out of range gets
 * n_before = n_known_before = -1 and true_dist NaN.  scores_out (nullable, tests) [B, n_ent] receives every D_c.
 * A row's counts do not depend on the other rows of the call; rows grouped by relation share projection work.
 * Integer counts only: two identical calls agree bitwise.  No host synchronisation inside; no CPU path. */
size_t ge_transx_rank_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B);
int ge_transx_rank(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                   const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                   const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_dist,
                   float* scores_out, void* workspace, size_t workspace_bytes, void* stream);
size_t ge_transr_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B);
int ge_transr_rank(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                   int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B, int cand_is_head,
                   const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before,
                   float* true_dist, float* scores_out, void* workspace, size_t workspace_bytes, void* stream);

/* --- relation prediction (h, ?, t) of the translation models: ranks of a triple's relation among EVERY relation.
 * Row i = (h, t, r) of triples [B,3]: every c in [0, n_rel) is a candidate with D_c = D(h, t, c).  The arithmetic is
 * fixed: the row's difference is taken once, w = e_h - e_t (one rounding per component), and the projection applied to
 * it:  TransE u_k = w_k + r_c,k;  TransH a = n^_c . w, u_k = fmaf(-a, n^_c,k, w_k) + r_c,k (n^ normalised with the
 * 1e-12 clamp, as ge_transx_score does);  TransD s = e_h . p_h - e_t . p_t (once per row), u_k = fmaf(s, rp_c,k, w_k)
 * + r_c,k;  TransR u_k = (M_c w)_k + r_c,k;  D = sum_k |u_k| or sum_k u_k^2, k in order, every dot and sum a
 * sequential fmaf chain in index order.  This equals ge_transx_score / ge_transr_score of (h, t, c) up to rounding.
 *     n_before[i]       = #{c : D_c < D_r, or D_c == D_r and c < r}   (ascending (D, relation id); raw rank = 1 + it)
 *     n_known_before[i] = how many of those c are listed in known_off / known_rc   (filtered rank = raw - it)
 *     true_dist[i]      = D_r
 *     scores_out        nullable, [B, n_rel]: every D_c (NaN in a row with an id out of range)
 * Every D_c is computed once and stored (in the workspace, or in scores_out when given); the counts, true_dist and the
 * filter read the stored values.  known_off / known_rc: ge_known_cells' tile lists for these rows with pos_of = the
 * identity over [0, n_rel) and n_cand = n_rel (fixed = h, rel = t against an index keyed h * n_rows + t that holds the
 * relations); NULL ranks unfiltered.  A row with an id out of range gets n_before = n_known_before = -1, true_dist
 * NaN.  A row's result does not depend on the other rows of the call; two identical calls agree bitwise.
 * Dims: 1 <= d <= ge_transx_max_dim(); TransR dims up to ge_transr_max_dim().  The caller passes `workspace`
 * (256-byte aligned) of *_relation_rank_workspace_bytes bytes (0 for bad sizes; GE_ENOMEM when smaller): a fixed chunk
 * of rows is processed at a time.  No host synchronisation inside; nothing allocated; no CPU path. */
size_t ge_transx_relation_rank_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B);
int ge_transx_relation_rank(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                            const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                            const int32_t* triples, int64_t B, const int32_t* known_off, const uint16_t* known_rc,
                            int32_t* n_before, int32_t* n_known_before, float* true_dist, float* scores_out,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t ge_transr_relation_rank_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B);
int ge_transr_relation_rank(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                            int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B,
                            const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before,
                            int32_t* n_known_before, float* true_dist, float* scores_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* --- triple classification: is (h, r, t) true?  All six models score "lower is more plausible" (the distance D of
 * ge_transx_score / ge_transr_score, E = sigmoid(score) of ge_complex_score / ge_hole_score), so one rule serves them:
 * a triple is predicted true iff  score <= thr[segment]  (a segment is a relation; a NaN score is never accepted).
 *
 * ge_threshold_fit fits thr from labelled scores.  score / seg / label [M] (label 0 or 1) are ORDERED by (seg ascending,
 * score ascending, NaN last); an element whose seg is outside [0, n_seg) is ignored.  Per segment of m elements, m_v of
 * them not NaN:  a cut p accepts the first p;  p is admissible iff p == 0, or 1 <= p <= m_v and (p == m_v or
 * score[p-1] < score[p])  -- equal scores are never separated, NaNs are rejected at every cut;
 * correct(p) = #positives in [0,p) + #negatives in [p,m);  the fit takes the admissible p with the largest correct(p),
 * the smallest such p on a tie.  Outputs, each [n_seg]:
 *     thr_lo = score[p-1] (-inf for p = 0)     thr_hi = score[p] (+inf for p = m_v)
 *     best_correct = correct(p)                n_pos, n_neg = the segment's positives / negatives
 * An empty segment gives -inf, +inf, 0, 0, 0.  Every output is an integer or a copy of an input float or an infinity.
 * Any threshold in [thr_lo, thr_hi) reproduces the cut.  1 <= M <= 2^31 - 1, n_seg >= 1, segments of any length: the
 * work is spread over workgroups of GE_THRESHOLD_FIT_TILE consecutive elements whatever the segment lengths are; the
 * counting is in integers (integer atomics only), so the result does not depend on the grid and two identical calls
 * agree bitwise.  Input that is not ordered gives other numbers but no access outside the buffers.
 * workspace: ge_threshold_fit_workspace_bytes(M, n_seg) bytes (0 for sizes out of range; monotone in both arguments;
 * GE_ENOMEM when smaller), 256-byte aligned (else GE_EINVAL).
 *
 * ge_threshold_classify decides, in any order of the input:  pred[i] = score[i] <= thr[seg[i]]  (uint8 0 / 1; 0 for a
 * NaN score or threshold and for a seg outside [0, n_seg)).  thr [n_seg].  label and confusion are nullable; with both,
 * confusion [n_seg, 4] = (tp, fp, tn, fn) per segment over the elements whose seg is in range, zeroed by the call and
 * accumulated with integer atomics (confusion without label is GE_EINVAL).  M >= 0.
 * Both: no host synchronisation inside; nothing allocated; no CPU path. */
#define GE_THRESHOLD_FIT_TILE 2048
size_t ge_threshold_fit_workspace_bytes(int64_t M, int32_t n_seg);
int ge_threshold_fit(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                     float* thr_lo, float* thr_hi, int32_t* best_correct, int32_t* n_pos, int32_t* n_neg,
                     void* workspace, size_t workspace_bytes, void* stream);
int ge_threshold_classify(const float* score, const int32_t* seg, const uint8_t* label, int64_t M, int32_t n_seg,
                          const float* thr, uint8_t* pred, int32_t* confusion, void* stream);

/* --- top-k tail / head prediction of the translation models over EVERY entity, selected inside the rank sweep (no
 * [B, n_ent] matrix).  Query row i = queries[2i], queries[2i+1] = (fixed f, relation r); every entity c is a candidate:
 * D_c = D(f, c, r) (cand_is_head = 0) or D(c, f, r), the SAME value ge_transx_rank / ge_transr_rank compute for that
 * cell (one distance loop: bit-equal to what their scores_out stores for a row with the same (fixed, relation)).
 *     out_id[i*k + j], out_dist[i*k + j]   the j-th candidate in ascending (D, entity id)
 * Filtered (known_off / known_rc as ge_transx_rank takes them, pos_of = the identity): known cells are skipped, so with
 * the same known set the filtered rank of the j-th candidate is j + 1.  Padding: id -1, distance +inf (fewer eligible
 * candidates than k; +inf distances count as padding).  A row with an id out of range, or with a NaN distance at a
 * candidate that is not known, gets id -1, distance NaN in every slot.  A row's result does not depend on the other rows
 * of the call; two identical calls agree bitwise.  1 <= k <= ge_transx_topk_max_k() (128), else GE_EINVAL.
 * Memory: the caller passes `workspace` (256-byte aligned) of the *_topk_workspace_bytes bytes (GE_ENOMEM when
 * smaller; 0 for k outside [1, max_k] or bad sizes): per row a pool of candidate keys and the partial lists of the
 * candidate ranges.  No host synchronisation inside; nothing allocated. */
int ge_transx_topk_max_k(void);
size_t ge_transx_topk_workspace_bytes(int model, int64_t n_ent, int64_t n_rel, int32_t d, int64_t B, int32_t k);
int ge_transx_topk(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                   const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                   const int32_t* queries, int64_t B, int cand_is_head, const int32_t* known_off,
                   const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t ge_transr_topk_workspace_bytes(int64_t n_ent, int64_t n_rel, int32_t dim_e, int32_t dim_r, int64_t B, int32_t k);
int ge_transr_topk(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix, int64_t n_rel,
                   int32_t dim_e, int32_t dim_r, const int32_t* queries, int64_t B, int cand_is_head,
                   const int32_t* known_off, const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_dist,
                   void* workspace, size_t workspace_bytes, void* stream);

/* --- nearest-neighbour entity search: for query rows q = table[queries[i]] and the K candidate rows cand (distinct, in
 * [0, N)) of a float32 table [N, d] used as stored, the candidates in ascending (D, row id) with
 *     u_x = x / |x| (0 for a zero row),  cos = u_q . u_c
 *     GE_METRIC_COSINE     D = max(0, 1 - cos)
 *     GE_METRIC_EUCLIDEAN  D = sqrt(max(0, |q|^2 + |c|^2 - 2 |q| |c| cos))
 * D is never negative and never -0.  cos is formed by f16 MFMAs on 22-bit operands (unit rows * 2^8 as fp16 high
 * halves and remainders) accumulated in fp32; every distance is one fixed fp32 expression of it, the same in both calls.
 *   ge_neighbor_planes_bytes  bytes of the candidates' planes + norms (0: d outside 1 ... ge_neighbor_max_dim() (288)
 *                             or more candidates than the sweep addresses)
 *   ge_neighbor_planes        fills them (256-byte aligned); valid until the table or cand change
 *   ge_neighbor_dists         out[i*K + c] = D of query i and candidate cand[c], every cell (NaN for a query id outside
 *                             [0, N)): tests, and k > ge_neighbor_max_k()
 *   ge_neighbor_topk          out_id[i*k + j], out_dist[i*k + j]: the j-th candidate of query i, no [B, K] matrix.
 *                             exclude_self: the candidate equal to the query's row is skipped.  Padding -1 / +inf; a
 *                             query id outside [0, N), or a NaN D at an eligible candidate, gives -1 / NaN in every
 *                             slot.  The lists are the first k of ge_neighbor_dists' values by (D, id), bit for bit.
 * 1 <= k <= ge_neighbor_max_k() (128); d > 288 or k > 128: GE_ENOTSUP.  Bad sizes, metric, null or misaligned
 * pointers: GE_EINVAL.  Workspace (256-byte aligned) below ge_neighbor_workspace_bytes(B, K, k), which is monotone in
 * every argument: GE_ENOMEM.  No host synchronisation, nothing allocated; two identical calls agree bitwise. */
int ge_neighbor_max_k(void);
int ge_neighbor_max_dim(void);
int64_t ge_neighbor_planes_bytes(int64_t K, int32_t d);
int ge_neighbor_planes(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, void* planes,
                       void* stream);
size_t ge_neighbor_workspace_bytes(int64_t B, int64_t K, int32_t k);
int ge_neighbor_dists(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B, const int32_t* cand,
                      int64_t K, int metric, const void* planes, float* out, void* stream);
int ge_neighbor_topk(const float* table, int64_t N, int32_t d, const int32_t* queries, int64_t B, const int32_t* cand,
                     int64_t K, int32_t k, int metric, int exclude_self, const void* planes, int32_t* out_id,
                     float* out_dist, void* workspace, size_t workspace_bytes, void* stream);


/* --- 1-vs-K candidate scoring (the inference loop of holE.py:564-569: fixed (head, relation)
 * against many tails; also K shared negatives per positive).  hr: [B,2] int32 (fixed entity,
 * relation); cand: [K] int32 candidate entity rows; cand_is_head = 0 scores (fixed, cand_j, rel),
 * 1 scores (cand_j, fixed, rel).  out: [B,K] fp32 row-major.  Runs as an MFMA GEMM
 * S = Q . T^T with Q = clip(fixed) o clip(rel) (complex product) and T the clipped candidates: fp32 MFMA, or --
 * d % 8 == 0 in 56 ... 224 (small sweeps) / 56 ... 288 (large ones) and max_norm <= 8 -- three f16 MFMAs on operands
 * split into fp16 high halves and remainders (22 bits), fp32 accumulation; scores within 1e-7 of fp64 either way. */
int ge_complex_score_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B,
                         const int32_t* cand, int64_t K, float max_norm, int apply_sigmoid,
                         int cand_is_head, float* out, void* stream);

/* --- link-prediction ranks straight out of the candidate sweep (holE.py:427-472 applied to the sweep of
 * holE.py:564-575): for test row i = (fixed entity, relation) = hr[i] with true candidate entity true_id[i]
 * (which must be in `cand`), over the K candidates,
 *     n_before[i]       = #{c : (E_ic, id_c) < (E_i,true, true_id[i])}   -- ascending loss, ties by entity id,
 *                         the pop order of the reference's heap; raw rank = 1 + n_before
 *     n_known_before[i] = how many of those are known-true candidates; filtered rank = raw - n_known_before.
 * The known-true candidates are given per (block of 128 test rows, tile of 128 candidates): known_off
 * [ceil(B/128) * ceil(K/128) + 1] int32 offsets into known_rc, whose entries are (row % 128) << 7 | (column % 128)
 * (both NULL: no filtering).  No [B,K] score matrix is written: the counting is the epilogue of the fp32-MFMA
 * GEMM (E = sigmoid(score) as in ge_complex_score_1vK).  true_loss (nullable) [B] receives E_i,true;
 * scores_out (nullable) [B,K] receives every loss -- for tests.  d must be a multiple of 8 and <= ge_rank_max_dim() (288; above 232 only with max_norm <= 8)
 * (the block's Q operand lives in LDS for the whole sweep), table 16-byte aligned; otherwise GE_ENOTSUP and the
 * caller falls back to ge_complex_score_1vK.
 * Arithmetic: fp32 MFMA with fp32 accumulation; for every d % 8 == 0 in 56 ... 288 and max_norm <= 8 the operands are split
 * into fp16 high halves and remainders (22 bits each, after the clip scales, so no fp16 overflow for any table) and
 * multiplied by three f16 MFMAs with fp32 accumulation -- losses within 1e-7 of the fp64 restatement either way
 * (ge_complex_score_1vK takes the same route for large sweeps at those dims). */
int ge_rank_max_dim(void);
int ge_complex_rank_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                        const int32_t* cand, int64_t K, float max_norm, int cand_is_head, const int32_t* known_off,
                        const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                        float* scores_out, void* stream);
/* The same sweep for `model` GE_MODEL_COMPLEX or GE_MODEL_HOLE_SPECTRAL (the README.md:42 HolE score on a table
 * held in the frequency domain, ge_hole_to_spectral: the ComplEx-shaped trilinear form with Hermitian weights, so
 * the candidate operand is still the row exactly as stored).  A real-valued HolE table (GE_MODEL_HOLE /
 * GE_MODEL_HOLE_DIRECT) is GE_ENOTSUP: transform a copy first. */
int ge_rank_1vK(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                float* scores_out, void* stream);

/* The split-precision sweep (embedding_dim % 8 == 0 in 56 ... 288, max_norm <= 8) reads the candidates as pre-split fp16
 * planes (high halves and remainders of row * clip scale * 2^8, laid out per 64-candidate tile) plus an entity ->
 * candidate-position map.  ge_rank_1vK builds them on every call (one pass over the K candidate rows, in a
 * stream-ordered allocation); a caller that ranks many batches against the same (table, cand, max_norm, model) --
 * holE.py:564-575 sweeps all entities for every test triple, tails and heads -- builds them once:
 *   ge_rank_planes_bytes   bytes of the buffer (0: this embedding_dim has no such sweep -- pass planes = NULL)
 *   ge_rank_planes         fills it (256-byte aligned); valid until the table, cand or max_norm change.  The buffer is
 *                          opaque; the padding of its last tile and between its parts is UNDEFINED (never written,
 *                          and never read into a result)
 *   ge_rank_1vK_planes     ge_rank_1vK with the buffer (NULL: as ge_rank_1vK).  cand_is_head does not enter the planes.
 * The contract says true_id[i] is in `cand`; where it is not, the split-precision sweep reports no rank (n_before =
 * n_known_before = 0, true_loss NaN) while the fp32 kernels rank the entity against the candidates all the same. */
int64_t ge_rank_planes_bytes(int64_t N, int32_t d, int64_t K);
int ge_rank_planes(const float* table, int64_t N, int32_t d, const int32_t* cand, int64_t K, float max_norm, int model,
                   void* planes, void* stream);
int ge_rank_1vK_planes(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                       const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                       float* scores_out, const void* planes, void* stream);

/* The same sweep against GIVEN losses: n_before[i] = #{ j : E_ij < ref_loss[i], or E_ij == ref_loss[i] and cand[j] <
 * ref_id[i] }, n_known_before[i] = how many of those are listed in the known cells -- i.e. the position the reference's
 * heap (holE.py:427-472) would give a triple of loss ref_loss[i] and tail id ref_id[i] among THESE candidates, whether or
 * not it is one of them.  Two uses: (1) a candidate list sharded over several devices -- each sweeps its own candidates
 * against the true triple's loss (computed once, by whoever holds the true candidate: ge_rank_1vK_planes' true_loss) and
 * the counts ADD across shards (exactly: equal table rows give bit-equal losses on every device); (2) the reference's
 * `is_confident = min_loss < infer_threshold` gate (holE.py:436-438): min_loss < t  <=>  n_before(ref_loss = t, ref_id
 * = INT32_MIN) > 0.  ref_id need not be a table row.  planes: as ge_rank_1vK_planes (NULL: built per call).
 * embedding_dim % 8 == 0 up to ge_rank_max_dim() (above 232 only with the planes' conditions), else GE_ENOTSUP. */
int ge_rank_1vK_vs_loss(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* ref_id,
                        const float* ref_loss, const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head,
                        const int32_t* known_off, const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before,
                        const void* planes, void* stream);

/* --- top-k prediction straight out of the split-precision sweep: for query row i = hr[i] = (fixed entity, relation) over
 * the K candidates `cand` (distinct entity rows; cand_is_head = 0: the candidate is the tail, 1: the head), the first k
 * pops of the reference's heap (holE.py:427-469): ascending (E_ic, cand_c) with E = sigmoid(score), ties by entity id
 * (the tuple order of holE.py:434, as ge_rank_1vK ranks).
 *     out_id[i*k + j], out_loss[i*k + j]   the j-th pop: its entity id and its loss
 * Filtered (known_off / known_rc exactly as ge_rank_1vK takes them): known-true candidates are skipped -- the first k
 * filtered pops.  The losses, and so the order, are bit-equal to the ones ge_rank_1vK_planes stores in scores_out for the
 * same cells (the same MFMA loop over the same planes, then rank_sigmoid(acc * 2^-16)): the ranks of the returned
 * candidates agree with ge_rank_1vK's by construction.
 * A row with fewer than k eligible candidates is padded with id -1, loss +inf; a row whose fixed entity or relation is
 * outside [0, N) gets id -1, loss NaN in every slot.
 * Scope: GE_MODEL_COMPLEX and GE_MODEL_HOLE_SPECTRAL (a real-valued HolE table is GE_ENOTSUP: transform a copy), the
 * split-precision range (embedding_dim % 8 == 0 in 56 ... 288, max_norm <= 8), 1 <= k <= ge_topk_max_k() (128);
 * otherwise GE_ENOTSUP.  k < 1, K < 1 or a null pointer: GE_EINVAL.
 * Memory: no [B,K] matrix; the caller passes `workspace` (256-byte aligned) of ge_topk_workspace_bytes(B, K, k) bytes
 * (GE_ENOMEM when smaller) -- per row a pool of candidate keys, and partial lists when few rows leave the GPU idle and
 * the candidates are cut into ranges.  `planes`: ge_rank_planes' buffer for (table, cand, max_norm, model), or NULL --
 * then built per call in a stream-ordered allocation, as ge_rank_1vK_planes does. */
int ge_topk_max_k(void);
size_t ge_topk_workspace_bytes(int64_t B, int64_t K, int32_t k);
int ge_topk_1vK_planes(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand,
                       int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_loss, const void* planes,
                       void* workspace, size_t workspace_bytes, void* stream);

/* --- per-relation candidate sets on the two sweeps above (the type-constrained protocol; holE.py:493-499, 535-541 give
 * each group of relations its own tail candidates).  A sweep over cand[K] takes
 *     mask     uint32 [n_sets][W], W = ge_candidate_mask_words(K) = 4 * ceil(K / 128) (0 for K <= 0): bit c & 31 of word
 *              c >> 5 of row s is set iff the candidate at POSITION c of `cand` is admissible in set s; bits at positions
 *              >= K are ignored
 *     row_set  int32 [B]: row i uses set row_set[i]; -1: unrestricted.  Any other value outside [0, n_sets) makes the row
 *              a bad row, with exactly what a fixed id out of range gives (ranks: counts 0, true_loss and stored losses
 *              NaN; top-k: id -1, loss NaN in every slot).
 * ge_rank_1vK_masked: n_before[i] counts the ADMISSIBLE candidates whose (E, id) is below the true candidate's,
 * n_known_before[i] those of them that are known cells; true_loss and scores_out are unchanged.  The true candidate
 * need not be admissible: its rank is the position it would take among the admissible ones (as ge_rank_1vK_vs_loss).
 * ge_topk_1vK_masked: the first k pops that are admissible and not known; fewer than k of them, or an empty set: id -1,
 * loss +inf padding.  workspace: ge_topk_workspace_bytes(B, K, k).
 * The losses are the unmasked sweep's, bit for bit: every masked result is a function of what ge_rank_1vK_planes stores
 * in scores_out, and with every bit set, or row_set = -1, the outputs equal the unmasked entry points' bitwise.
 * Scope: the split-precision range only (embedding_dim % 8 == 0 in 56 ... 288, max_norm <= 8, GE_MODEL_COMPLEX or
 * GE_MODEL_HOLE_SPECTRAL), else GE_ENOTSUP -- the fp32 kernels take no mask.  A null mask or row_set, or n_sets < 1:
 * GE_EINVAL.  No host synchronisation, no allocation beyond the planes' stream-ordered one when planes is NULL.
 * Mask builders (all device pointers):
 *   ge_candidate_mask_from_classes  mask[s] <- the candidates c with allow[s] bit cand_class[c] set; cand_class int32 [K]
 *                                   (a class outside [0, n_class): never admissible), allow uint32 [n_sets][ceil(n_class/32)]
 *   ge_candidate_mask_from_cells    mask <- 0, then the bit of every (set, position) pair of cells int32 [M][2]; pairs
 *                                   outside [0, n_sets) x [0, K) are ignored */
int64_t ge_candidate_mask_words(int64_t K);
int ge_candidate_mask_from_classes(const int32_t* cand_class, int64_t K, const uint32_t* allow, int32_t n_sets,
                                   int32_t n_class, uint32_t* mask, void* stream);
int ge_candidate_mask_from_cells(const int32_t* cells, int64_t M, int32_t n_sets, int64_t K, uint32_t* mask, void* stream);
int ge_rank_1vK_masked(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* true_id,
                       const int32_t* cand, int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t* n_before, int32_t* n_known_before, float* true_loss,
                       float* scores_out, const void* planes, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                       void* stream);
int ge_topk_1vK_masked(const float* table, int64_t N, int32_t d, const int32_t* hr, int64_t B, const int32_t* cand,
                       int64_t K, float max_norm, int model, int cand_is_head, const int32_t* known_off,
                       const uint16_t* known_rc, int32_t k, int32_t* out_id, float* out_loss, const void* planes,
                       void* workspace, size_t workspace_bytes, const int32_t* row_set, const uint32_t* mask,
                       int32_t n_sets, void* stream);

/* --- the summary of holE.py:475-490 from a rank sweep's counts, and a pocket decision on it, on the device.
 * Row i of the M rows COUNTS iff true_loss is NULL or true_loss[i] is not NaN (the sweeps report a bad row as counts 0
 * with true_loss NaN: it must not score as rank 1) and 0 <= n_known_before[i] <= n_before[i].  For a counted row raw =
 * 1 + n_before, fil = raw - n_known_before; with n the number of counted rows, metrics_out [8] receives
 *     [0] filtered MRR = mean 1 / fil    [1] raw MRR    [2] mean fil    [3] mean raw
 *     [4] [5] [6] 100 * #{fil <= 1 / 3 / 10} / n        [7] n
 * n = 0: entries 0-6 are NaN, entry 7 is 0.  Arithmetic: one workgroup; the reciprocal sums in double in one fixed
 * order (two calls agree bitwise, no atomics), the rank sums and hit counts as 64-bit integers; each output is one
 * double division rounded once to float ((100.0 * count) / n, sum / n).
 * Pocket: improved = metrics_out[0] > *best (a NaN never improves, an equal value does not: the first best is kept, as
 * ge_validation_tick keeps it); if improved, *best = metrics_out[0]; *improved (nullable) = 1 or 0.  best NULL: no
 * decision, *improved = 0.
 * GE_EINVAL: n_before, n_known_before or metrics_out NULL, M < 1.  GE_ENOTSUP: M > 2^24 (n stays exact in entry 7). */
int ge_rank_metrics(const int32_t* n_before, const int32_t* n_known_before, const float* true_loss, int64_t M,
                    float* metrics_out, float* best, int32_t* improved, void* stream);

/* --- a copy gated by a device flag, for a pocket of several buffers (the tables and optimiser state of a translation
 * model): iff *flag != 0 when the kernel runs, dst[s][0 .. count[s]) <- src[s] for every segment s, as 32-bit words
 * (NaN payloads survive); iff *flag == 0, no byte of any dst is written.  flag: a device int32, e.g. ge_rank_metrics'
 * `improved`.  src, dst and count are HOST arrays of n_seg entries, read during the call and handed to the kernel by
 * value: the caller may free them on return.  One launch for all segments, enqueued on `stream`; no synchronisation, no
 * allocation.  count[s] == 0 is allowed and skipped (its pointers are not looked at); every count 0: nothing is
 * launched, 0 is returned.
 * Any 4-byte alignment is served: a segment whose src and dst are both 16-byte aligned moves 16 bytes a lane, any
 * other moves dwords; the count % 4 tail is covered by both.  Each workgroup moves ge_copy_if_chunk() = 8192 words of
 * one segment (the last chunk of a segment is shorter) and reads *flag first.
 * Refusals, all before the launch.  GE_EINVAL: flag, src, dst or count NULL; n_seg outside [1,
 * GE_COPY_IF_MAX_SEGMENTS]; a negative count; with count[s] > 0, src[s] or dst[s] NULL or not 4-byte aligned, or
 * dst[s]'s range overlapping another segment's dst range or any segment's src range (its own included; checked on the
 * host, so the result never depends on the order of the segments).  GE_ENOTSUP: a count above 2^44, or more than
 * 2^31 - 1 chunks in all. */
#define GE_COPY_IF_MAX_SEGMENTS 16
int ge_copy_if_chunk(void);
int ge_copy_if(const int32_t* flag, int32_t n_seg, const float* const* src, float* const* dst, const int64_t* count,
               void* stream);

/* --- one validation tick on the evaluation's own metric, enqueued on `stream` without a host decision, a
 * synchronisation or an allocation: `planes` rebuilt from the table as it is now (ge_rank_planes), the V tail-side rows
 * ranked (cand_is_head = 0), the V head-side rows ranked (cand_is_head = 1), ge_rank_metrics over the 2V rows into
 * metrics_out [8] and *best (device scalar, start it at 0), and -- iff this tick improved on *best -- pocket <- table
 * and pocket_accumulator <- accumulator (each nullable; otherwise neither is touched).
 *     hr [2V,2]       V rows (head, relation), then V rows (tail, relation);  true_id [2V]: their tails, then their heads
 *     known_*_tail / known_*_head   ge_known_cells' lists of each side's V rows, as ge_rank_1vK takes them for B = V
 *                     (both of a side NULL: unfiltered)
 *     planes          ge_rank_planes_bytes(N, d, K) bytes, 256-byte aligned, overwritten by every call; NULL iff that
 *                     size is 0 (the fp32 kernels then rank, and take no candidate sets)
 *     row_set [2V], mask_tail, mask_head, n_sets   per-relation candidate sets as ge_rank_1vK_masked takes them, one
 *                     mask per side; all NULL / 0: unmasked.  Every row is ranked against its set whether or not its
 *                     true entity is admissible.
 *     workspace       ge_rank_tick_workspace_bytes(V) bytes (the counts and true losses of the 2V rows and the flag;
 *                     a multiple of 256, monotone, 0 for V < 1), 256-byte aligned
 * The counts are ge_rank_1vK_planes' (ge_rank_1vK_masked's with masks), bit for bit; bad rows do not count.
 * Refusals, all before the first launch, in this order: GE_EINVAL for V < 1, K < 1, metrics_out, best or workspace NULL;
 * masks without row_set, row_set without both masks, n_sets != 0 without them; pocket_accumulator without accumulator;
 * a workspace off 256 bytes.  GE_ENOTSUP for 2V > 2^24.  Then everything ge_rank_1vK_planes / ge_rank_1vK_masked refuse,
 * with their codes (the masked form outside embedding_dim 56 ... 288 included); GE_EINVAL for planes NULL where the
 * split-precision sweep runs, and for a pocket that is not 16-byte aligned; GE_ENOMEM for a workspace below the size. */
size_t ge_rank_tick_workspace_bytes(int64_t V);
int ge_rank_validation_tick(const float* table, int64_t N, int32_t d, const int32_t* hr, const int32_t* true_id, int64_t V,
                            const int32_t* cand, int64_t K, float max_norm, int model, const int32_t* known_off_tail,
                            const uint16_t* known_rc_tail, const int32_t* known_off_head, const uint16_t* known_rc_head,
                            void* planes, const int32_t* row_set, const uint32_t* mask_tail, const uint32_t* mask_head,
                            int32_t n_sets, const float* accumulator, float* metrics_out, float* best, float* pocket,
                            float* pocket_accumulator, void* workspace, size_t workspace_bytes, void* stream);

/* --- per-relation candidate sets on the translation models' sweeps over every entity (ge_transx_rank / ge_transr_rank,
 * ge_transx_topk / ge_transr_topk): the same type-constrained protocol (holE.py:493-499, 533-541), with candidate
 * position = entity id.  Each entry point has its unmasked counterpart's arguments with (row_set, mask, n_sets) after the
 * known-cell pointers; the rank forms have no scores_out.
 *     mask     uint32 [n_sets][W], W = ge_candidate_mask_words(n_ent): bit c & 31 of word c >> 5 of row s is set iff
 *              entity c is admissible in set s; bits at positions >= n_ent are ignored (what the mask builders above
 *              produce for cand = 0 .. n_ent - 1)
 *     row_set  int32 [B]: row i uses set row_set[i]; -1: unrestricted.  Any other value outside [0, n_sets) makes the row
 *              a bad row, with exactly what an id out of range gives (ranks: n_before = n_known_before = -1, true_dist
 *              NaN; top-k: id -1, distance NaN in every slot).
 * ge_transx_rank_masked / ge_transr_rank_masked: n_before[i] counts the ADMISSIBLE entities c with (D_c, c) below
 * (D_true, true), n_known_before[i] those of them that are known cells; true_dist is unchanged.  The true entity need
 * not be admissible: its rank is the place it would take among the admissible ones.
 * ge_transx_topk_masked / ge_transr_topk_masked: the first k entities in ascending (D, c) that are admissible and not
 * known; fewer than k of them, or an empty set: id -1, distance +inf padding.  A NaN distance flags the row (-1 / NaN)
 * only at an entity that is admissible and not known.
 * Every distance is the unmasked sweep's own, bit for bit: every masked result is a function of what ge_transx_rank /
 * ge_transr_rank store in scores_out, and with every bit set, or row_set = -1 everywhere, the outputs equal the unmasked
 * entry points' bitwise.  The sweep computes a distance only for entities that some row of a 16-row chunk admits.
 * workspace: ge_transx_rank_workspace_bytes / ge_transx_topk_workspace_bytes (ge_transr_* for TransR) of the same shape;
 * a shortfall is GE_ENOMEM, a workspace not 256-byte aligned GE_EINVAL.  A null mask or row_set, or n_sets < 1:
 * GE_EINVAL.  No host synchronisation, no allocation, no CPU path. */
int ge_transx_rank_masked(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                          const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                          const int32_t* triples, int64_t B, int cand_is_head, const int32_t* known_off,
                          const uint16_t* known_rc, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                          int32_t* n_before, int32_t* n_known_before, float* true_dist, void* workspace,
                          size_t workspace_bytes, void* stream);
int ge_transr_rank_masked(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                          int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* triples, int64_t B,
                          int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, const int32_t* row_set,
                          const uint32_t* mask, int32_t n_sets, int32_t* n_before, int32_t* n_known_before,
                          float* true_dist, void* workspace, size_t workspace_bytes, void* stream);
int ge_transx_topk_masked(int model, int l1, const float* ent, int64_t n_ent, const float* rel, int64_t n_rel,
                          const float* normal, const float* ent_transfer, const float* rel_transfer, int32_t d,
                          const int32_t* queries, int64_t B, int cand_is_head, const int32_t* known_off,
                          const uint16_t* known_rc, const int32_t* row_set, const uint32_t* mask, int32_t n_sets,
                          int32_t k, int32_t* out_id, float* out_dist, void* workspace, size_t workspace_bytes,
                          void* stream);
int ge_transr_topk_masked(int l1, const float* ent, int64_t n_ent, const float* rel, const float* rel_matrix,
                          int64_t n_rel, int32_t dim_e, int32_t dim_r, const int32_t* queries, int64_t B,
                          int cand_is_head, const int32_t* known_off, const uint16_t* known_rc, const int32_t* row_set,
                          const uint32_t* mask, int32_t n_sets, int32_t k, int32_t* out_id, float* out_dist,
                          void* workspace, size_t workspace_bytes, void* stream);

/* --- the known_off / known_rc lists of ge_rank_1vK from a sorted index of the known-true triples (the filter of
 * holE.py:454-463, built by the reference as a dict of sets, holE.py:413-422).  known_key [M] ascending = fixed entity *
 * n_rows + relation of every distinct known (fixed, other, relation); known_ent [M] = the other entity; fixed / rel [B] =
 * the test rows; pos_of [n_rows] = position of an entity in the candidate list (-1: not a candidate).  Two passes:
 *   pass 0  known_off [tiles + 1] <- offsets of every (128 rows x 128 candidates) tile's cells; known_off[tiles] = total
 *   pass 1  known_rc [total] <- the cells, (row % 128) << 7 | (column % 128), in no particular order inside a tile
 * tile_scratch: int32 [tiles], the same buffer in both passes.  All ids are int64 (the evaluator's dtype). */
int ge_known_cells(int pass, const int64_t* known_key, const int64_t* known_ent, int64_t M, const int64_t* fixed,
                   const int64_t* rel, int64_t B, const int64_t* pos_of, int64_t n_rows, int64_t n_cand, int32_t* tile_scratch,
                   int32_t* known_off, uint16_t* known_rc, void* stream);

/* --- the inner training loop of holE.py:340-362 (minus validation), enqueued natively: for
 * s in [0, n_steps): batch = triples[(first_row + s*B) .. +B) (rows of a device-resident, already
 * shuffled [T,3] int32 array, wrapping to row 0 when the next batch would run past T -- the
 * reference's shuffle queue never yields a short batch, holE.py:283); negatives from
 * ge_corrupt_batch with step = global_step0 + s; lr_s = lr0 / (1 + decay_rate * (global_step0+s) /
 * decay_steps) (tf.train.inverse_time_decay, holE.py:292-294; decay_steps <= 0 keeps lr0); then one
 * ge_*_hinge_step.  No host synchronisation.
 *
 * workspace >= ge_train_workspace_bytes(B, d) enables the PREPARED path: the negatives and a
 * row-sorted index of the step's gradient slots are built ahead of time, for a chunk of steps per
 * launch (one workgroup per step and per sub-batch of 4096 pairs: sampler + stable LDS radix sort by
 * row), into two chunk buffers inside the workspace.  The update then touches every distinct row
 * once, with plain read-modify-writes at any B (float atomics only for rows with > 16 gradient slots in a
 * step; for B > 4096 the sort runs across workgroups, csrc/ge_prep_big.hip).  The workspace also holds a
 * ring of gradient-row regions, one per step in turn.  With only ge_hinge_step_workspace_bytes the
 * loop falls back to sampler + float-atomic scatter per step.
 *
 * pipeline (nullable): a handle from ge_train_pipeline_create, bound to the device that was current
 * at creation.  It owns a non-blocking side stream and four events on which the prepare launch for
 * the NEXT chunk of steps runs while `stream` executes the current one -- across calls too: when a
 * call continues exactly where the previous call with the same handle stopped (same arrays, sizes,
 * seed, mode, workspace; global_step0 and first_row advanced by the steps already run) its records
 * are already built and nothing but the two per-step kernels is on the critical path.  Any other
 * call restarts the sequence (its first prepare launch, ~120 us at B = 4096, is then exposed).  While a handle
 * is live the caller must not modify `triples`, the type tables or the workspace between calls
 * without ge_train_pipeline_reset; the streams are ordered by events only, the host never blocks,
 * and before returning every call makes `stream` wait for the look-ahead launch, so work enqueued
 * on `stream` afterwards (e.g. a stream-ordered free of the workspace) is ordered after it.  One
 * handle must not be used from two host threads at once.  pipeline = NULL: the prepare launches go
 * to `stream` itself and the library keeps no state whatsoever.
 *
 * neg_ws: device [B,3] int32 scratch (holds the last step's negatives on return).  loss: device
 * [n_steps*B] when keep_all_losses, else [B] (last step).  model: GE_MODEL_COMPLEX; GE_MODEL_HOLE (real
 * table; for even d the call transforms it to the frequency domain on entry, runs the spectral steps
 * and transforms back on exit -- two O(N d^2) passes per call, so prefer long calls or keep the table
 * spectral); GE_MODEL_HOLE_SPECTRAL (table already spectral, no transforms); GE_MODEL_HOLE_DIRECT
 * (direct-correlation kernels on the real table, O(d^2) per triple).
 * The width is decided before anything is launched.  The ComplEx-shaped kernels (models 0 and 2, and model 1's
 * spectral steps) take an even d whose d / 2 complex elements fit 128 lane vectors of the widest width (4, 2 or 1
 * elements) that divides d / 2 and that the table's alignment allows (16, 8, 4 bytes): every d = 0 (mod 8) up to
 * ge_max_dim() on a 16-byte boundary, but d = 4 (mod 8) only up to 512 and d = 2 (mod 4) only up to 256, less on a
 * table off the boundary.  Elsewhere models 0 and 2 are GE_ENOTSUP; GE_MODEL_HOLE then runs the direct-correlation
 * kernels on the real table (as it does for odd d) up to d = 512 and is GE_ENOTSUP beyond.  A refused call has launched
 * nothing and changed nothing; a call that fails later hands a GE_MODEL_HOLE table back real-valued.  The log-loss and
 * AdaGrad loops below decide the same way.
 * ev_pairs (nullable, HOST array of 2*n_steps events from ge_event_create): the events ride on the
 * dispatch of kernel `ev_kernel` of every step (1 = gather+score+hinge+grad, 2 = row update; 0 =
 * the per-step sampler of the fallback path) and report that kernel's own begin/end -- the hook
 * bench.py uses to time one kernel; NULL entries skip a step.
 * ge_train_workspace_bytes (and ge_train_logloss_workspace_bytes) never shrink as B grows: a workspace sized for the
 * largest batch serves every smaller one on the prepared path.  ge_train_logloss_workspace_bytes is NOT monotone in
 * negative_ratio: the steps prepared per chunk and the gradient ring shrink as (1 + negative_ratio) * B grows, so a
 * larger ratio can need fewer bytes (B = 1024, d = 8: ratio 31 needs more than ratio 32).  Size the workspace for the
 * ratio the loop is called with; a call with another ratio than it was sized for may be GE_ENOMEM.
 * ge_train_max_chunk_steps(B, negative_ratio; 0 = the hinge and AdaGrad loops): the steps one prepare launch holds, i.e.
 * where the chunk boundaries of a sequence lie (step s of a sequence is in chunk s / that number).  128 steps while
 * (1 + negative_ratio) * B <= 4096, where a launch is one workgroup per step and lasts the same for 32 steps or 128 but
 * slows the steps it runs beside, so fewer and longer launches cost less; 31 and falling beyond, never rising with B;
 * 0 for B <= 0 or a negative ratio.  The two chunk buffers dominate the workspace of small steps: B = 4096, d = 200
 * needs 419 MB (ge_train_workspace_bytes), 302 MB of it records (1.18 MB each, about 0.3 MB of which is ever touched;
 * 32-step chunks took 75 MB), the rest the gradient ring. */
size_t ge_train_workspace_bytes(int64_t B, int32_t d);
int64_t ge_train_max_chunk_steps(int64_t B, int64_t negative_ratio);
int ge_train_pipeline_create(void** pipeline);
int ge_train_pipeline_reset(void* pipeline);
int ge_train_pipeline_destroy(void* pipeline); /* waits for the side stream, then frees */
int ge_train_steps(float* table, int64_t N, int32_t d, const int32_t* triples, int64_t T,
                   int64_t first_row, int64_t B, int64_t n_steps, const int32_t* id_to_type,
                   const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids,
                   uint64_t seed, uint64_t global_step0, int32_t padded_size, int32_t mode,
                   float margin, float lr0, float decay_steps, float decay_rate, float max_norm,
                   int model, float* loss, int keep_all_losses, int32_t* neg_ws, void* workspace,
                   size_t workspace_bytes, void** ev_pairs, int ev_kernel, void* pipeline, void* stream);

/* --- the same loop for the --log_loss objective (holE.py:194-196, 206-220, minimised as holE.py:296), ComplEx:
 * per step the M = (1 + negative_ratio) * B triples are the positives (label +1) followed by negative_ratio
 * corrupted batches (label -1; the k-th is ge_corrupt_batch with step = (global_step0 + s) * negative_ratio + k),
 * loss_i = log(1 + exp(-y_i s_i)) + l2 * sum(table^2) / 2, and table <- table * (1 - lr M l2) - lr * sparse gradient.
 * Negatives and the row-sorted slot index (slot = 3 * triple + {h, t, r}) are prepared ahead as in
 * ge_train_steps; the dense decay is carried as one scalar between steps (rows are read scaled, the sparse
 * update is divided by the new scale) and the table is materialised once, before the call returns -- instead of
 * two passes over the whole table per step; sum(table^2) is formed only for the steps whose loss is kept.
 * loss: [n_steps * M] with keep_all_losses, else [M] (last step), in the reference's concat order.
 * neg_ws: [negative_ratio, B, 3] int32 (last step's negatives on return).  workspace >=
 * ge_train_logloss_workspace_bytes(B, negative_ratio, d), 256-B aligned.  pipeline: as for ge_train_steps
 * (a handle used for the hinge loop restarts when it meets this one and vice versa). */
size_t ge_train_logloss_workspace_bytes(int64_t B, int32_t negative_ratio, int32_t d);
int ge_train_steps_logloss(float* table, int64_t N, int32_t d, const int32_t* triples, int64_t T, int64_t first_row,
                           int64_t B, int64_t n_steps, const int32_t* id_to_type, const int64_t* type_offsets,
                           int32_t n_types, const int32_t* type_ids, uint64_t seed, uint64_t global_step0,
                           int32_t padded_size, int32_t mode, int32_t negative_ratio, float l2, float lr0,
                           float decay_steps, float decay_rate, float max_norm, float* loss, int keep_all_losses,
                           int32_t* neg_ws, void* workspace, size_t workspace_bytes, void* pipeline, void* stream);

/* --- the hinge loop of ge_train_steps with AdagradOptimizer(lr_s, initial_accumulator_value) in place of the plain SGD
 * of holE.py:296 (semantics: ge_adagrad_rows; s is the snapshot gradient of the step, taken through the clip; lr_s the
 * same inverse_time_decay value).  accum: [N,d] fp32, caller-owned, 4-byte aligned, not overlapping `table`.  The
 * prepared path only: workspace >= ge_train_adagrad_workspace_bytes(B, d) (never shrinks as B grows), 256-B aligned,
 * GE_ENOMEM below.  Per step: the gradient kernel at lr = 1, then two update kernels that give every distinct row its
 * complete sum in a fixed order and one read-modify-write of both arrays -- no float atomics, bitwise reproducible.  A
 * row that no hinge-active pair names is not touched in either array.  model: GE_MODEL_COMPLEX; GE_MODEL_HOLE and
 * GE_MODEL_HOLE_DIRECT (both: direct-correlation kernels on the real table, which is never transformed -- AdaGrad is
 * elementwise and not linear, so it does not commute with the DFT); GE_MODEL_HOLE_SPECTRAL is GE_ENOTSUP.  loss, neg_ws,
 * pipeline: as for ge_train_steps (a handle used for another loop restarts when it meets this one). */
size_t ge_train_adagrad_workspace_bytes(int64_t B, int32_t d);
int ge_train_steps_adagrad(float* table, float* accum, int64_t N, int32_t d, const int32_t* triples, int64_t T,
                           int64_t first_row, int64_t B, int64_t n_steps, const int32_t* id_to_type,
                           const int64_t* type_offsets, int32_t n_types, const int32_t* type_ids, uint64_t seed,
                           uint64_t global_step0, int32_t padded_size, int32_t mode, float margin, float lr0,
                           float decay_steps, float decay_rate, float max_norm, int model, float* loss,
                           int keep_all_losses, int32_t* neg_ws, void* workspace, size_t workspace_bytes, void* pipeline,
                           void* stream);

/* The prepare launch on its own: the records of n_steps consecutive steps, as ge_train_steps builds
 * them, into `out` (ge_train_prepare_bytes(B, n_steps) bytes: n_steps * layout[0] int32 words of records,
 * then -- for B > 4096 -- the key arrays of the multi-workgroup sort).  ge_train_prepared_layout fills out8 =
 * {words per step record, tiles per step, pairs per tile S, offset of slot_item[6B],
 * offset of tile 0, words per tile, offset of items inside a tile, offset of islots}.
 * A step record is  neg[3B] | slot_item[6B] | tiles { n_items, pad | items[4S][2] = {table row,
 * count | multi << 30} | islots[4S][16] = the IndexedSlices slots (6*pair + k) an item sums, -1 padded }.
 * The step's (row, slot) keys are sorted as one sequence of tiles * 4S positions; tile t lists the items that
 * start in positions [t*4S, (t+1)*4S).
 * direct = 1: a row with exactly one gradient slot in the step is not queued as an
 * item; its slot is tagged -2 in slot_item and the pair that produces it updates the table row. */
size_t ge_train_prepare_bytes(int64_t B, int64_t n_steps);
int ge_train_prepared_layout(int64_t B, int64_t* out8);
int ge_train_prepare_steps(const int32_t* triples, int64_t T, int64_t first_row, int64_t B, int64_t n_steps,
                           const int32_t* id_to_type, int64_t N, const int64_t* type_offsets, int32_t n_types,
                           const int32_t* type_ids, uint64_t seed, uint64_t global_step0, int32_t padded_size,
                           int32_t mode, int direct, int32_t* out, size_t out_bytes, void* stream);

/* --- the row-sharded training step (holE.py:287-296 on a table mod-sharded over G processes: owner = id % G,
 * local row = id / G, R = ceil(N / G); the reference itself is single-device).  The host
 * (graphembeddings_amd/sharded.py) moves rows and gradient sums with torch.distributed all-to-alls; these entry
 * points are everything else.  All buffers device, caller-owned; nothing synchronises.
 *
 * ge_shard_plan -- requester side, for S steps of B pairs at once (pos, neg [S,B,3] GLOBAL ids; neg differs from
 *   pos in at most one of head / tail, as ge_corrupt_batch produces; other pairs count as invalid):
 *   records [S, ge_train_prepared_layout(B)[0]]: the step's work items in the native loop's record format, over
 *     this rank's rows (read and updated in place) and, behind them, the other owners' rows in staging order
 *     (an item row R + u = row u of the gradient-sum buffer); slot_item tags: -2 sole slot of an own row, -3 - u
 *     sole slot of staged row u (the producing pair stores the row straight into the gradient-sum buffer);
 *   pos_src [S,B,3], neg_src [S,B]: where each pair reads its rows (own row, or R + u; neg_src = source << 1 |
 *     column of the corrupted entity, -1 when it has no row of its own; pos_src -1 = invalid pair);
 *   req_row [S,4*Bt] (Bt = B rounded up to the record's tile size: layout[1] * layout[2]): entry u = staged row u's
 *     index in its owner's shard, grouped by owner; counts [S,G]: rows requested from each owner.
 *   peer_mapped = 1 (experiment, G <= 8): pos_src / neg_src name another owner's row by R * (1 + owner) + local row
 *     instead of R + u -- for ge_shard_grad with peer_shards (HOST array of the G shards' device addresses, mapped
 *     into this process; entry `rank` unused), which reads those rows in place and takes no staging buffer.
 *   workspace: ge_shard_plan_workspace_bytes(B, S) bytes (GE_ENOMEM when smaller), 256-byte aligned (else GE_EINVAL). */
size_t ge_shard_plan_workspace_bytes(int64_t B, int64_t S);
int ge_shard_plan(const int32_t* pos, const int32_t* neg, int64_t S, int64_t B, int64_t N, int32_t G, int32_t rank,
                  int32_t* records, int32_t* pos_src, int32_t* neg_src, int32_t* req_row, int32_t* counts,
                  void* workspace, size_t workspace_bytes, int32_t peer_mapped, void* stream);
/* One step's fused gather -> clip -> score -> sigmoid -> hinge -> gradient rows on two row stores: the shard
 * (rows < R, in place; sole-slot rows are updated here) and `staged` [n_staged,d], the rows fetched from the
 * other owners.  gsum [n_staged,d] receives the gradient rows tagged -3 - u.  model: GE_MODEL_COMPLEX or
 * GE_MODEL_HOLE_SPECTRAL.  loss [B], grad_idx [6B], grad_val [6B,d] as for ge_hinge_grad. */
int ge_shard_grad(float* shard, int64_t rows_local, int32_t d, const float* staged, int64_t n_staged, const int32_t* pos_src,
                  const int32_t* neg_src, const int32_t* record, int64_t B, int64_t N, int32_t G, float margin, float lr,
                  float max_norm, int model, float* loss, int32_t* grad_idx, float* grad_val, float* gsum,
                  const float* const* peer_shards, void* stream);
/* The step's work items: own rows get ONE read-modify-write each, staged rows their sum in gsum (which must be
 * zero beforehand: rows with more than 16 slots combine atomically). */
int ge_shard_apply(float* shard, int64_t rows_local, int32_t d, const int32_t* record, int64_t B, int64_t N, int32_t G,
                   const int32_t* grad_idx, const float* grad_val, float* gsum, void* stream);
/* Owner side: req_all = the chunk's received request lists (rows of this shard) in (step, peer) order, step s =
 * [req_start[s], req_start[s+1]) (req_start: DEVICE int64 [S+1]); cap >= the longest per-step list.  records
 * [S, ge_shard_owner_record_words(cap)]: work items that add row j of the step's receive buffer to shard row
 * req[j] -- one read-modify-write per distinct row, fixed order.  workspace: ge_shard_owner_workspace_bytes(cap, S)
 * bytes (GE_ENOMEM when smaller), 256-byte aligned (else GE_EINVAL). */
int64_t ge_shard_owner_record_words(int64_t cap);
size_t ge_shard_owner_workspace_bytes(int64_t cap, int64_t S);
int ge_shard_owner_plan(const int32_t* req_all, const int64_t* req_start, int64_t S, int64_t cap, int64_t rows_local,
                        int32_t* records, void* workspace, size_t workspace_bytes, void* stream);
int ge_shard_owner_apply(float* shard, int64_t rows_local, int32_t d, const int32_t* record, int64_t cap, const float* recv,
                         void* stream);

/* --- thin wrappers over hipEvent_t so a ctypes host can time kernels on the launch stream. */
int ge_event_create(void** ev);
int ge_event_destroy(void* ev);
int ge_event_record(void* ev, void* stream);
int ge_event_synchronize(void* ev);
int ge_event_elapsed_ms(void* start, void* stop, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* GE_HIP_H */
