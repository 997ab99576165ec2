/*
 * kelpie_hip.h -- C ABI of the MI355X-native Kelpie relevance engine.
 *
 * The reference has no FFI: its relevance engine is the Python class API of
 * src/relevance_engines/post_training_engine.py.  This library replaces the
 * arithmetic below that API (KelpieModel construction, the Kelpie optimizers'
 * post-training loop and get_triple_results' all-entity filtered rank); the
 * Python package kelpie_amd binds it with ctypes and re-exposes the
 * reference's class interface (NecessaryPostTrainingEngine, ...).  Each entry
 * point names the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative KP_E* code otherwise;
 *     kp_last_error(ctx) describes the last failure (thread-local when ctx is
 *     NULL, e.g. for a failed kp_ctx_create);
 *   - all pointers are HOST pointers owned by the caller; the context copies
 *     what it needs to device memory and owns that copy;
 *   - calls are synchronous at return; a context is not re-entrant (one host
 *     thread per context);
 *   - entity ids: frozen entities are [0, n_ent); the kelpie ("mimic") entity
 *     of a slot has id n_ent, like KelpieDataset.kelpie_entity
 *     (src/data/kelpie_dataset.py:20-25);
 *   - relation ids: [0, n_rel2) with n_rel2 = 2|R|; inverse of p is p+|R|
 *     (src/data/dataset.py:319-331).
 */
#ifndef KELPIE_HIP_H
#define KELPIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KP_OK 0
#define KP_EINVAL (-22)
#define KP_ENOMEM (-12)
#define KP_EDEVICE (-5)
#define KP_ENOTSUP (-95)
/* kp_rng_transe_calls_async only: no walker thread could start, so the walk ran inline
 * on the caller's thread; torch_state then holds the advanced stream (not an error) */
#define KP_INLINE 1

/* model families (src/link_prediction/__init__.py:5-9, MODEL_REGISTRY) */
#define KP_MODEL_TRANSE 0
#define KP_MODEL_COMPLEX 1
#define KP_MODEL_CONVE 2
/* DistMult (src/link_prediction/models/distmult.py:38-68; the reference leaves it out of its
 * registry): plain [d] float rows, score (lhs * rel) . rhs, maximizer, post-trained by the
 * ComplEx optimizer (multiclass_nll_optimizer.py:57-164).  Rows of at most 400 floats;
 * kp_posttrain_rank (and kp_posttrain_rank_f64), kp_all_scores, kp_convertible and kp_predict_tails serve it,
 * kp_train_epoch, kp_dp_relevance and kp_criage_relevance do not. */
#define KP_MODEL_DISTMULT 3

/* optimizers (multiclass_nll_optimizer.py:41-48; Kelpie TransE / ConvE use Adam) */
#define KP_OPT_ADAGRAD 0
#define KP_OPT_ADAM 1
#define KP_OPT_SGD 2

typedef struct kp_ctx kp_ctx;

/* Frozen model tables.  Replaces the E/R clones every KelpieModel makes per
 * candidate (transe.py:86-87, complex.py:146-147, conve.py:206-207): the
 * tables are uploaded ONCE per context and shared by every slot. */
typedef struct {
  int32_t model;      /* KP_MODEL_* */
  int32_t n_ent;      /* |E| */
  int32_t n_rel2;     /* 2|R| */
  int32_t dim;        /* row width: TransE/ConvE/DistMult d, ComplEx 2d ([Re | Im], complex.py:24-25) */
  const float* entity;   /* [n_ent][dim] */
  const float* relation; /* [n_rel2][dim] */
  /* ConvE frozen layers (conve.py:40-52, frozen copies at :214-237); NULL otherwise */
  const float* conv_w;   /* [32][3][3] (Conv2d(1,32,3) weight) */
  const float* conv_b;   /* [32] */
  const float* fc_w;     /* [dim][hidden], hidden = 32*38*(dim/20-2) */
  const float* fc_b;     /* [dim] */
  const float* bn_alpha; /* [1 + 32 + dim]: eval-mode BN1|BN2|BN3 scale  w/sqrt(var+eps) */
  const float* bn_beta;  /* [1 + 32 + dim]: eval-mode BN1|BN2|BN3 shift  b - mean*scale  */
  /* TransE score norm p (TransEHyperParams.norm, transe.py:12-15,46; tune.py:19 searches
   * {1, 2}): 2 = L2, 1 = L1, 0 = the default 2; must be 0 for the other models */
  int32_t norm_p;
} kp_model_desc;

/* Post-training hyper-parameters (the *_explanation.json "training" block,
 * validated by the optimizers' HyperParams classes). */
typedef struct {
  int32_t optimizer;     /* KP_OPT_*; TransE and ConvE: KP_OPT_ADAM */
  int32_t epochs;
  int32_t batch_size;
  float lr;              /* ConvE: 1e-3 (KelpieBCEOptimizer ignores hp lr, bce_optimizer.py:165) */
  float beta1, beta2;    /* Adam betas */
  float eps;             /* Adagrad 1e-10, Adam 1e-8 */
  float reg_weight;      /* ComplEx / DistMult N3 (N2) weight / TransE L2 weight */
  float margin;          /* TransE */
  int32_t neg_ratio;     /* TransE negative_triples_ratio */
  float label_smoothing; /* ConvE */
  float hidden_dropout;  /* ConvE hidden dropout rate (masks are inputs) */
  float input_dropout;   /* ConvE input dropout rate (conve.py:142) */
  float fmap_dropout;    /* ConvE feature-map Dropout2d rate (conve.py:147) */
  int32_t reg_kind;      /* ComplEx regulariser (multiclass_nll_optimizer.py:45-48): KP_REG_N3 | KP_REG_N2 */
} kp_hp;

enum { KP_REG_N3 = 0, KP_REG_N2 = 1 }; /* regularizers.py:37-46 (N3), :25-35 (N2) */

/* One batch of post-training slots.  A slot is one KelpieModel post-training
 * (PostTrainingEngine.post_train, post_training_engine.py:64-76) followed by
 * get_triple_results (:101-125).  Base and post-trained models are both just
 * slots.
 *
 *   x0          [n_slots][dim]   initial kelpie row (after the model's init:
 *                                ComplEx init*init_scale, TransE xavier, ConvE raw)
 *   row_off     [n_slots+1]      CSR offsets into rows
 *   rows        [total][3]       training rows of each slot: the kelpie triples
 *                                followed by their inverses, in reference order
 *                                (optimizer.train's vstack(triples, inverse))
 *   rng_off     [n_slots+1]      CSR offsets (in int32 words) into rng
 *   rng         [...]            per-slot random draws, generated on the host in
 *                                reference order (RNG-as-input):
 *       ComplEx: epochs x R permutation (torch.randperm, multiclass_nll_optimizer.py:148)
 *       TransE:  epochs x [R row order | R negative entities | R head_or_tail]
 *                (pairwise_ranking_optimizer.py:166-181; only rows [0,R) are stepped)
 *       ConvE:   per step: ceil(b*dim/32) words of hidden-dropout keep bits
 *   pred        [n_slots][3]     kelpie-form triple to rank (s = n_ent)
 *   filt_off    [n_slots+1]      CSR offsets into filt
 *   filt        [...]            entities filtered out of the rank (to_filter[(s,p)]
 *                                of the slot's KelpieDataset after the edit)
 * outputs:
 *   out_x       [n_slots][dim]   final kelpie rows (may be NULL)
 *   out_score   [n_slots]        target score  (all_scores[o])
 *   out_rank    [n_slots]        filtered rank (minimizer: <=, o restored before
 *                                counting; maximizer: >=, o excluded if filtered)
 */
typedef struct {
  int32_t n_slots;
  const float* x0;
  const int32_t* row_off;
  const int32_t* rows;
  const int64_t* rng_off;
  const int32_t* rng;
  const int32_t* pred;
  const int32_t* filt_off;
  const int32_t* filt;
  float* out_x;
  float* out_score;
  int64_t* out_rank;
} kp_batch;

/* Create a context on HIP device `device` and upload the frozen tables. */
int kp_ctx_create(int device, const kp_model_desc* model, kp_ctx** out);
int kp_ctx_destroy(kp_ctx* ctx);
const char* kp_last_error(const kp_ctx* ctx);

/* Page-locked host memory (hipHostMalloc) for the buffers the caller fills and a
 * context uploads every batch: the deferred-draw arenas of kelpie_amd.rng, which
 * kp_posttrain_rank then reads by DMA with no staging copy (the reference has no
 * counterpart: its draws never leave the host).  KP_EDEVICE without a usable GPU. */
int kp_host_alloc(size_t bytes, void** out);
int kp_host_free(void* p);

/* Post-train every slot of the batch and rank its target triple.
 * Replaces, per slot: KelpieX(...) construction, Kelpie*Optimizer.train
 * (pairwise_ranking_optimizer.py:160-203, multiclass_nll_optimizer.py:138-164,
 * bce_optimizer.py:161-208) and PostTrainingEngine.get_triple_results
 * (post_training_engine.py:101-125). */
int kp_posttrain_rank(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch);

/* kp_posttrain_rank, plus what each slot's post-trained row would predict instead: the k
 * best tails of (kelpie, p, .) among the columns 0 .. n_ent (column n_ent = the kelpie
 * entity), taken from the values the rank compares (the reference keeps only the target's
 * score and rank of get_triple_results' masked row, post_training_engine.py:101-125).
 *   masking     as the rank: every filtered column is left out, the target o too when it is
 *               filtered (ComplEx, ConvE, DistMult); TransE restores its filtered o; the
 *               kelpie column takes part unless filtered
 *   order       better value first (TransE: the smaller distance), equal values by column
 *               id; ConvE orders on its fp64 logits (two saturated sigmoids, a tie for the
 *               rank, stay in logit order)
 *   out_ids     [n_slots][k] column ids, -1 past the last unmasked column
 *   out_scores  [n_slots][k] the columns' scores, converted as out_score is; 0 past the end
 * If o is unmasked and out_rank <= k, o is among the first out_rank ids of its slot.
 * out_x, out_score and out_rank are bit for bit those of kp_posttrain_rank.
 * k in [1, 32]; k == 0 with NULL outputs is kp_posttrain_rank.  KP_EINVAL (after the batch
 * check, before any device work) for k < 0, k > 32 or k > 0 with a NULL output;
 * KP_ENOTSUP for k > 0 when the context ranks in fp32 (KP_TE_RANK=f32, KP_CV_RANK=f32). */
int kp_posttrain_rank_topk(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                           float* out_scores);

/* Probes: further kelpie-form triples (kelpie, p, o) ranked against the post-trained row of
 * a slot, each as get_triple_results (post_training_engine.py:101-125) ranks it on that
 * slot's post-trained model -- scored, masked, counted and converted exactly as the slot's
 * own target is.  Slot s owns the probes [probe_off[s], probe_off[s+1]).
 *   probe_off   [n_slots+1]  CSR offsets into probes; probe_off[0] = 0, probe_off[n_slots] = n
 *   probes      [n][2]       (p, o): p in [0, n_rel2), o in [0, n_ent] (n_ent = the kelpie entity)
 *   filt_off    [n+1]        CSR offsets into filt, one list per probe
 *   filt        [...]        to_filter[(kelpie, p)] of the owning slot's edited KelpieDataset
 * outputs:
 *   out_score   [n]          the probe's score, converted as kp_batch.out_score is
 *   out_rank    [n]          its filtered rank */
typedef struct {
  int32_t n;
  const int32_t* probe_off;
  const int32_t* probes;
  const int32_t* filt_off;
  const int32_t* filt;
  float* out_score;
  int64_t* out_rank;
} kp_probes;

/* kp_posttrain_rank_topk, plus the probes' scores and ranks (get_triple_results,
 * post_training_engine.py:101-125, called on the slot's post-trained model for other
 * triples than the explained prediction).  A probe equal to its slot's own (p, o) with the
 * slot's own filter returns the slot's out_score bit for bit and its out_rank.  out_x,
 * out_score, out_rank and the top-k lists are bit for bit those without probes.
 * probes == NULL or probes->n == 0 is kp_posttrain_rank_topk.  KP_EINVAL (after the batch
 * check, before any upload) for malformed probes; KP_ENOTSUP with probes when the context
 * ranks in fp32 (KP_TE_RANK=f32, KP_CV_RANK=f32).  The probe rows run in chunks whose fp64
 * query rows and filter bitmaps stay within 64 MiB (KP_PROBE_CHUNK=n, a diagnostic, forces
 * n rows per chunk). */
int kp_posttrain_rank_probes(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                             float* out_scores, const kp_probes* probes);

/* ---- Post-training trace: the optimizer's loss of every step of every slot ----
 * Step j of slot s is the j-th step_on_batch call of that post-training in the reference
 * (multiclass_nll_optimizer.py:147-164, pairwise_ranking_optimizer.py:165-203,
 * bce_optimizer.py:167-208); its trace value is the `l` that call returns: the loss at the
 * kelpie row BEFORE the step's update, on the step's minibatch of B rows, with the step's
 * own dropout masks.
 *   ComplEx / DistMult  CrossEntropyLoss(mean) of the batch's rows against all n_ent + 1
 *       columns, the kelpie column included, plus the regulariser's value:
 *       N3 (regularizers.py:37-46)  w (sum |lhs|^3 + sum |rel|^3 + sum |rhs|^3) / B,
 *       N2 (regularizers.py:25-35)  w (sum_rows ||lhs||^3 + ||rel||^3 + ||rhs||^3) / B,
 *       |.| the model's factor modulus (ComplEx sqrt(re^2 + im^2), complex.py:80-84;
 *       DistMult |x_i|, distmult.py:66), ||.|| the 2-norm of a row's moduli.  The frozen
 *       rows' factors count in the value (they are constant in the gradient, not in l).
 *   TransE  mean(max(0, f+ - f- + margin)) + lambda (L2(pos) + L2(neg)) / 2,
 *       L2 = (mean lhs^2 + mean rel^2 + mean rhs^2) / 3 over the rows actually stepped
 *       (regularizers.py:15-22, pairwise_ranking_optimizer.py:183-203).
 *   ConvE   BCELoss (mean over B x (n_ent + 1), every log clamped at -100 as torch does) of
 *       the train-mode forward -- batch norms in eval mode, the three dropouts with the
 *       masks the step draws -- against the targets (1 - ls) y + 1 / (n_ent + 1)
 *       (bce_optimizer.py:190-208).
 * Steps per slot: ComplEx / DistMult / TransE epochs * ceil(R / batch_size), R the slot's
 * rows including the inverses; ConvE epochs * ceil(P / batch_size), P the slot's distinct
 * (head, relation) pairs (er_vocab).  A slot without rows has zero steps.
 * A value is accumulated in fp64 in a fixed order and rounded to fp32 once, at the store: a
 * trace is bitwise the same on a rerun with a fresh context. */

/* out_steps[s] = the steps of slot s by the rule above: pure host work, no context.  hp:
 * epochs and batch_size are read.  KP_EINVAL (kp_last_error(NULL) names the rule) for an
 * unknown model, batch_size <= 0, epochs < 0, a row_off that does not start at 0 or
 * decreases, or a missing array. */
int kp_trace_steps(int32_t model, const kp_hp* hp, int32_t n_slots, const int32_t* row_off, const int32_t* rows,
                   int32_t* out_steps);

/*   trace_off   [n_slots+1]            CSR offsets into out_loss: the prefix sums of kp_trace_steps
 *   out_loss    [trace_off[n_slots]]   slot s's losses at [trace_off[s], trace_off[s+1]), step order */
typedef struct {
  const int32_t* trace_off;
  float* out_loss;
} kp_trace;

/* kp_posttrain_rank_probes, plus the trace of every slot.  out_x, out_score, out_rank, the
 * top-k lists and the probes' results are bit for bit those without the trace.  trace == NULL
 * is kp_posttrain_rank_probes.  KP_EINVAL (after the batch and probe checks, before any
 * upload) for a trace_off that disagrees with kp_trace_steps or a NULL out_loss with steps
 * to write.  The trace does not depend on the rank: the fp32 rank switches do not refuse it.
 * Every model family.  ConvE scores each row of a step against all columns for it, in chunks
 * of rows whose logits stay within 64 MiB (KP_TRACE_CHUNK=n, a diagnostic, forces n rows). */
int kp_posttrain_rank_trace(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                            float* out_scores, const kp_probes* probes, const kp_trace* trace);

/* ---- Epoch marks: score and rank of every post-training after chosen epochs ----
 * A call carries one strictly increasing list of epochs 0 <= e_0 < ... < e_{n-1} <= hp->epochs,
 * 1 <= n <= 16.  Mark j of slot s is what kp_posttrain_rank returns for that slot on the same
 * batch with hp->epochs = e_j: the kelpie row after e_j epochs, scored, masked, counted and
 * converted exactly as the slot's own target (get_triple_results, post_training_engine.py:
 * 101-125, on the model under training).  Every family's draws are laid out epoch-major or
 * step-major, so the shorter run reads a prefix of the same draws.  Hence mark 0 is the result
 * of x0, mark hp->epochs is the slot's own out_score and out_x row bit for bit and its
 * out_rank, a slot without rows has x0's result at every mark, and ConvE marks are ranked on
 * the eval-mode forward as the final row is.
 * It is NOT the reference started with epochs = e_j from the same seed: that run draws fewer
 * numbers per post-training, so every post-training after the first starts elsewhere in the
 * random stream.
 *   epochs      [n]                strictly increasing, in [0, hp->epochs]
 *   out_score   [n_slots][n]       the marks' target scores, converted as kp_batch.out_score
 *   out_rank    [n_slots][n]       their filtered ranks
 *   out_x       [n_slots][n][dim]  the kelpie rows at the marks (may be NULL) */
typedef struct {
  int32_t n;
  const int32_t* epochs;
  float* out_score;
  int64_t* out_rank;
  float* out_x;
} kp_marks;

/* kp_posttrain_rank_trace, plus the marks of every slot.  out_x, out_score, out_rank, the
 * top-k lists, the probes' results and the trace are bit for bit those without marks; the
 * lists and the probes stay on the final row.  marks == NULL is kp_posttrain_rank_trace.
 * KP_EINVAL (after the batch, probe and trace checks, before any upload) for malformed marks;
 * KP_ENOTSUP with marks when the context ranks in fp32 (KP_TE_RANK=f32, KP_CV_RANK=f32).
 * The rows are captured by the step kernels themselves (no launch is added to the step path)
 * and ranked after the slots, in chunks of whole 16-row groups whose fp64 query rows and
 * filter bitmaps stay within 64 MiB (KP_MARKS_CHUNK=n, a diagnostic, forces n rows). */
int kp_posttrain_rank_marks(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                            float* out_scores, const kp_probes* probes, const kp_trace* trace,
                            const kp_marks* marks);

/* ---- Rank margins: how far every rank row's rank is from changing ----
 * A rank row is anything the fp64 rank ranks: a slot's target, a probe, a mark.  For a rank row
 * with target column o, c_e is the value the count compares for column e (columns 0 .. n_ent,
 * column n_ent = the kelpie entity) and c_t the target's.  Masking is exactly the rank's, the
 * filtered-target rules of each family included, and `own` is what the rank counts for the
 * target column itself (0 or 1).  The compared value and the score units per family:
 *   ComplEx / DistMult   the fp64 score          the same
 *   ConvE                the fp64 logit          the same
 *   TransE L2            the squared distance    sqrt(c)
 *   TransE L1            the L1 distance         the same
 * Tolerance: a call carries one tol, finite, 0 <= tol <= 1.  Per row delta = tol * max(1, |v_t|)
 * with v_t = c_t in score units.
 * Thresholds, in compared units, once per row in fp64:
 *   maximizers  thr_lo = c_t + delta           thr_hi = c_t - delta
 *   L1          thr_lo = c_t - delta           thr_hi = c_t + delta
 *   L2          thr_lo = max(v_t - delta, 0)^2 thr_hi = (v_t + delta)^2
 *   tol == 0    both are c_t itself, not a recomputation of it.
 * (L2: a threshold that the rounding of the root and the square would carry across c_t, which
 * takes a delta below one ulp of v_t, is c_t.)
 * Band:
 *   rank_lo = own + #{e != o unmasked: c_e at least as good as thr_lo}
 *   rank_hi = own + #{e != o unmasked: c_e at least as good as thr_hi}
 * "as good as" is >= for maximizers and <= for minimizers.  ConvE keeps the saturation rule on
 * both thresholds: with a saturated target (float32 sigmoid 1.0) a saturated column counts in
 * both.  Hence rank_lo <= out_rank <= rank_hi always, and at tol == 0 all three are equal: the
 * predicate is the rank's own.
 * Ties: the number of other unmasked columns with c_e == c_t exactly.
 * Nearest competitors: id_better is, among the unmasked columns other than o strictly better
 * than the target, the one closest to it in compared order, the lower column id on equal
 * values; gap_better = |v_e - v_t| in score units, fp64 (>= 0; it may be 0 after the L2 square
 * root).  id_worse / gap_worse are the same on the other side.  Without such a column the id
 * is -1 and the gap +inf.  The kelpie column takes part unless it is masked.
 * Determinism: a margin is a pure function of the row's inputs.  The counts are integer sums of
 * per-workgroup partial counts, the nearest competitors minima of (value key, column) pairs;
 * no floating-point atomics; a rerun on a fresh context gives the same bits.
 *
 * One set of outputs per kind of rank row; a NULL pointer = not wanted (rank_lo and rank_hi go
 * together). */
typedef struct {
  int64_t *rank_lo, *rank_hi, *ties;
  double *gap_better, *gap_worse;
  int32_t *id_better, *id_worse;
} kp_margin_out;
typedef struct {
  double tol;
  kp_margin_out slots;  /* [n_slots] */
  kp_margin_out probes; /* [probes->n] */
  kp_margin_out marks;  /* [n_slots][marks->n] */
} kp_margins;

/* kp_posttrain_rank_marks, plus the margins of every rank row.  Every other output of the call
 * (out_x, out_score, out_rank, the lists, the probes, the trace, the marks) is bit for bit what
 * it is without margins: the margins come from one more fp64 pass over the entity table per
 * rank row, after the row's own count.  margins == NULL is kp_posttrain_rank_marks.
 * KP_EINVAL (after the marks check, before any upload) for a tol that is NaN, negative or above
 * 1, for probe or mark outputs wanted without probes or marks, or for an output set with only
 * one of rank_lo / rank_hi; KP_ENOTSUP when the context ranks in fp32 (KP_TE_RANK=f32,
 * KP_CV_RANK=f32).  Not offered on kp_posttrain_rank_f64. */
int kp_posttrain_rank_margins(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                              float* out_scores, const kp_probes* probes, const kp_trace* trace,
                              const kp_marks* marks, const kp_margins* margins);

/* ---- Attributions: every post-training's score change split over its training rows ----
 * For the bilinear families (ComplEx, DistMult) the target score is linear in the kelpie row,
 * s(x) = <c, x> with c = grad_x score(kelpie, p, o), and every Adagrad or SGD step is a
 * diagonal matrix applied to a sum of per-row gradients, so s(x_T) - s(x_0) splits exactly
 * into one number per training row plus the regulariser's share.  This is the only definition.
 *
 * Per slot, x_t is the kelpie row before step t and B_t the step's minibatch of b_t rows (the
 * rows of kp_batch.rows: the kelpie triples followed by their inverses).  All columns
 * 0 .. n_ent count, the kelpie column included.
 *
 * Row gradient gamma_i(x) = grad_x [lse_i(x) - s_{i,target}(x)], everything but x frozen:
 *   row (K, r, t), t frozen:  J_r^T (<E> - E_t) + p_k q,   q = x o r,
 *                             <E> = sum_e p_e E_e + p_k x,  p_k the kelpie column's softmax weight
 *   row (K, r, K):            J_r^T (<E> - x) + (p_k - 1) q
 *   row (h, r, K), h frozen:  (p_k - 1) q_pair
 * Regulariser gradient rho_i(x) = occ_i * 3 w |x| o x (N3) or occ_i * 3 w ||f|| x (N2), occ_i in
 * {1, 2} the number of times the kelpie occurs in the row; |.| and ||.|| are the family's moduli
 * (the complex modulus of a (re, im) pair for ComplEx, |x_i| for DistMult).
 *
 * Step: g_t = (1 / b_t) sum_{i in B_t} (gamma_i + rho_i) and x_{t+1} - x_t = -D_t o g_t, with
 * D_t = lr (SGD) or lr / (sqrt(s_t) + eps) (Adagrad, s_t the state after this step's
 * accumulation), in the step's own fp32 arithmetic.
 *
 * Attributions, accumulated in fp64 in a fixed order with one writer per row:
 *   fit_i = sum_{t: i in B_t} -(1 / b_t) <c o D_t, gamma_i(x_t)>
 *   reg_i = sum_{t: i in B_t} -(1 / b_t) <c o D_t, rho_i(x_t)>
 * delta = <c, x_T - x_0> in fp64 from the fp32 rows; sum_i (fit_i + reg_i) = delta up to the
 * fp32 rounding of the updates, and s(x_0) = out_score - delta.  Rows that are never stepped
 * (epochs = 0) keep 0; a slot without rows writes nothing to out_fit / out_reg.  Duplicate rows
 * of a slot get equal values only when they share every minibatch (R <= batch_size). */
typedef struct {
  double* out_fit;   /* [row_off[n_slots]] */
  double* out_reg;   /* [row_off[n_slots]] */
  double* out_delta; /* [n_slots] */
} kp_attrib;

/* kp_posttrain_rank_margins, plus the attributions.  Every other output of the call (out_x,
 * out_score, out_rank, the lists, the probes, the trace, the marks, the margins) is bit for bit
 * what it is without attributions.  attrib == NULL is kp_posttrain_rank_margins.  Refusals,
 * after the margins check and before any upload, the first rule broken: KP_EINVAL for a NULL
 * out_fit, out_reg or out_delta with rows to write; KP_ENOTSUP for a context that is not ComplEx
 * or DistMult (TransE's and ConvE's scores are not linear in the row), for
 * hp->optimizer == KP_OPT_ADAM (its momentum would need one vector per training row), and for
 * a slot whose pred tail is the kelpie entity (its score is quadratic in x).  Keyed draws are
 * served.  Not offered on kp_posttrain_rank_f64. */
int kp_posttrain_rank_attrib(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, int32_t k, int32_t* out_ids,
                             float* out_scores, const kp_probes* probes, const kp_trace* trace,
                             const kp_marks* marks, const kp_margins* margins, const kp_attrib* attrib);

/* ---- fp64: post-train and rank in double precision on the device (ComplEx, DistMult) ----
 * The fp64 result of a slot is what the reference returns when every tensor of the run is a
 * float64 one (the `fp64` variant of tools/conditioning.py):
 *   - the frozen tables are the fp32 tables upcast (exact);
 *   - the kelpie init is drawn in fp32, upcast, and multiplied by init_scale in fp64: x0 below;
 *   - every hyper-parameter is the Python double (0.01, not (float)0.01);
 *   - the row, the query, the logits, the softmax, the gradient, the N3 / N2 term, the
 *     optimizer state and the update are all fp64, in torch's op order;
 *   - the draws are those of the fp32 run (kp_batch.rng_off / rng), so the generators end
 *     in the same state in either precision;
 *   - the score and the rank come from the fp64 row.
 * Nothing is rounded to fp32 anywhere between x0 and the outputs.  The device sums its
 * contractions in its own fixed order (an fp64 MFMA attention over the frozen entities whose
 * key ranges merge by log-sum-exp in range order), so it agrees with the reference's fp64
 * run to fp64 rounding, not bit for bit; a rerun on a fresh context is bitwise equal.
 *   x0          [n_slots][dim]   the initial kelpie rows in fp64 (kp_batch.x0 is ignored)
 *   lr .. reg_weight             take precedence over kp_hp's floats; the integers of kp_hp
 *                                (optimizer, epochs, batch_size, reg_kind) are read from it
 *   out_x       [n_slots][dim]   the final kelpie rows (may be NULL)
 *   out_score   [n_slots]        the fp64 target score itself */
typedef struct {
  const double* x0;
  double lr, beta1, beta2, eps, reg_weight;
  double* out_x;
  double* out_score;
} kp_f64;

/* kp_posttrain_rank in fp64 by the definition above.  batch->out_rank is the rank output;
 * batch->x0, batch->out_x and batch->out_score are not read or written and may be NULL.
 * Refusals, in this order: the batch check (KP_EINVAL); a NULL r, r->x0 or r->out_score
 * (KP_EINVAL); a context that is not ComplEx / DistMult (KP_ENOTSUP, before any upload).
 * The fp32 rank switches do not apply to these families.  Top-k lists, probes, the trace
 * and the marks are not offered on this entry point.  The call uses workspaces of its own:
 * a context that has served it returns bitwise the fp32 results of a fresh one afterwards. */
int kp_posttrain_rank_f64(kp_ctx* ctx, const kp_hp* hp, const kp_batch* batch, const kp_f64* r);

/* ---- Keyed draws: order-independent post-training randomness, generated on the device ----
 * The reference draws each post-training's kelpie init, epoch shuffles and negatives from
 * process-global generators in call order; kp_batch.x0 / rng_off / rng carry those draws and
 * that stays the default.  Keyed draws are a second, opt-in source: every slot's numbers are
 * a pure function of two 64-bit keys, generated by a counter-based generator on the device
 * into the buffers the step kernels read.  No generator state exists; a rerun gives the same
 * bits.  TransE, ComplEx and DistMult (ConvE's mask layout is not keyed yet).
 *
 * Generator: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds).  Known answers (counter | key | output), the Random123 vectors:
 *   00000000 x4 | 00000000 x2 | 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ffffffff x4 | ffffffff x2 | 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   243f6a88 85a308d3 13198a2e 03707344 | a4093822 299f31d0 | d16cfe09 94fdcceb 5001e420 24126ea1
 *
 * Keys: a slot carries init_key and slot_key.  The library takes whatever keys the caller
 * passes.  kelpie_amd (kelpie_amd/keyed.py) derives both as the first 8 bytes, little-endian,
 * of blake2b(digest_size = 8) over
 *   init_key: "kelpie-keyed/init\0" | seed int64 | s, p, o int32
 *   slot_key: "kelpie-keyed/slot\0" | seed int64 | s, p, o int32 | role uint8 (0 base, 1 edited)
 *             | mode uint8 (0 necessary, 1 sufficient) | count uint32 | the rule's triples
 *             SORTED, each h, r, t int32
 * every integer little-endian, (s, p, o) the prediction the slot ranks in the dataset's ids
 * (for a conversion entity: after replace_entity_in_triple).  A prediction's base slot and
 * all of its edited slots share init_key, hence x0: common random numbers.
 *
 * Words: word w of stream s, epoch e, under key k is lane w % 4 of
 *   Philox(counter = (w / 4, e, s, 0), key = (lo32(k), hi32(k))).
 * Streams:
 *   0  x0, under init_key, epoch 0.  ComplEx / DistMult: element i =
 *      float(word_i >> 8) * 2^-24, then * x0_scale in float32 (kelpie_init's one multiply).
 *      TransE: element i takes words 2 i, 2 i + 1: u1 = (w + 1) * 2^-32, u2 = w' * 2^-32,
 *      value (x0_scale * sqrt(-2 ln u1)) * cos(2 pi u2) in float64, rounded once to float32
 *      (x0_scale: the xavier std, float(sqrt(2 / (d + 1)))).
 *   1  the permutation of epoch e, under slot_key: row i gets key word i; the permutation is
 *      the stable ascending argsort of the key words (ties by row index).
 *   2  TransE negative entity of (epoch, row): (uint64(word) * neg_bound) >> 32.
 *   3  TransE head-or-tail of (epoch, row): word >> 31 (1 corrupts the head).
 * Layout: exactly kp_batch.rng's.  ComplEx / DistMult: epochs x R permutations for a slot with
 * R > batch_size, no words otherwise.  TransE: epochs x [R row order | R negatives | R
 * head_or_tail], each epoch's row order its own permutation.
 *   init_key    [n_slots]
 *   slot_key    [n_slots]
 *   x0_scale    ComplEx / DistMult: init_scale; TransE: the normal's std
 *   neg_bound   TransE: the bound of the negatives (n_ent + 1 as the reference draws), in
 *               [1, 2^31]; not read otherwise */
typedef struct {
  int32_t n_slots;
  const uint64_t* init_key;
  const uint64_t* slot_key;
  float x0_scale;
  int64_t neg_bound;
} kp_keyed;

/* Arm the context: the next kp_posttrain_rank, _topk, _probes, _trace or _marks call on it
 * whose batch has x0, rng_off and rng all NULL generates its draws from these keys (copied
 * here; the caller's arrays are not read later) and disarms.  A call that brings its buffers
 * leaves the context armed; any failing call disarms.  The armed call checks the request after
 * the batch check and before any device work (KP_EINVAL: n_slots differs from the batch's,
 * missing keys, neg_bound out of range, a word count beyond int64).  Its results are bit for
 * bit those of the same batch fed with kp_keyed_draws' arrays.  kp_posttrain_rank_f64 on an
 * armed context answers KP_ENOTSUP and disarms; so does arming a ConvE context.  keyed == NULL
 * disarms.  Unarmed, a NULL buffer is the KP_EINVAL it always was. */
int kp_ctx_arm_keyed(kp_ctx* ctx, const kp_keyed* keyed);

/* The per-slot word counts of the layout above, out_words [n_slots]: pure host work, no
 * context.  hp: epochs and batch_size are read.  They are what the reference protocol's draws
 * occupy for the same slot.  KP_ENOTSUP for ConvE, KP_EINVAL (kp_last_error(NULL)) otherwise. */
int kp_keyed_rng_words(int32_t model, const kp_hp* hp, int32_t n_slots, const int32_t* row_off, int64_t* out_words);

/* Generate the draws of n_slots slots on the device and download them: out_x0 [n_slots][dim]
 * (may be NULL), out_rng_off [n_slots + 1] the prefix sums of kp_keyed_rng_words, out_rng
 * [out_rng_off[n_slots]] (cap: its capacity in words; KP_EINVAL when too small).  These are
 * kp_batch's x0 / rng_off / rng of the armed call.  For tests and for callers that want the
 * numbers.  The armed call downloads none of them, but for ComplEx / DistMult the permutations
 * of its multi-step slots (R > batch_size): those families plan their steps on the host. */
int kp_keyed_draws(kp_ctx* ctx, const kp_hp* hp, int32_t n_slots, const int32_t* row_off, const kp_keyed* keyed,
                   float* out_x0, int64_t* out_rng_off, int32_t* out_rng, int64_t cap);

/* Model.all_scores (model.py:19; transe.py:48-65, complex.py:88-112,
 * conve.py:133-158) for n (head, relation) pairs over the frozen entities:
 * out[n][n_ent].  The RelevanceEngine.select_entities_to_convert sweep
 * (engine.py:94-101) is built on it. */
int kp_all_scores(kp_ctx* ctx, int32_t n, const int32_t* heads, const int32_t* rels, float* out);

/* Filtered-rank sweep of engine.py:89-120 for n candidate heads e with
 * relation p and object o: keep[i] = 1 iff o is not the model's top-1 for
 * (e,p,.) once to_filter[(e,p)] is masked to +-1e6.  filt CSR as in kp_batch. */
int kp_convertible(kp_ctx* ctx, int32_t n, const int32_t* heads, int32_t rel, int32_t obj,
                   const int32_t* filt_off, const int32_t* filt, uint8_t* keep);

/* Model.predict_tails (src/link_prediction/models/model.py:42-68; ConvE:
 * conve.py:160-184) for n frozen triples (h, r, t), r in [0, n_rel2) (inverse
 * relations give head prediction, model.py:30-31): out_score[i] = score of t,
 * out_rank[i] = filtered rank of t among all entities with to_filter[(h, r)]
 * (CSR as in kp_batch) masked to +-1e6 and t restored, counting <= (TransE) or
 * >= (ComplEx) the target; ConvE ranks by a descending sort with filtered
 * entries at 0.0, i.e. 1 + #(scores > target).  The Evaluator's MRR / Hits@k
 * (link_prediction/evaluation.py:16-48) are computed from these ranks. */
int kp_predict_tails(kp_ctx* ctx, int32_t n, const int32_t* triples, const int32_t* filt_off, const int32_t* filt,
                     float* out_score, int64_t* out_rank);

/* One training epoch of the context's OWN tables, for the retraining of
 * verify_explanations.py:141-143 / :230-232 (RNG-as-input: the host draws what the
 * optimizer draws).  The optimizer state persists across calls and restarts at
 * epoch == 0.
 *  ComplEx: MultiClassNLLOptimizer.epoch (src/link_prediction/optimization/
 *    multiclass_nll_optimizer.py:101-135; ComplEx.forward complex.py:58-86, N3
 *    regularizers.py): triples [n][3] are train()'s stack of the training triples and
 *    their inverses (:66-67), aux [n] this epoch's torch.randperm(n) (:102); batches of
 *    min(hp->batch_size, n) start every hp->batch_size rows (:112-118); Adagrad / Adam /
 *    SGD (hp->optimizer).
 *  TransE: PairwiseRankingOptimizer.epoch (pairwise_ranking_optimizer.py:102-157;
 *    TransE.forward transe.py:67-75, L2 regularizers.py): triples [n][3] are this
 *    epoch's positive rows in order (the stack after its in-place np.random.shuffle),
 *    aux [n][3] the matching corrupted rows (the first n of the epoch's ratio * n
 *    torch.randint draws); MarginRankingLoss(hp->margin), L2 (hp->reg_weight), Adam.
 * ConvE contexts: KP_EINVAL. */
int kp_train_epoch(kp_ctx* ctx, const kp_hp* hp, int32_t n, const int32_t* triples, const int32_t* aux,
                   int32_t epoch);

/* Copy the context's tables to the host: entity [n_ent][dim], relation [n_rel2][dim]
 * (the trained model's state_dict tensors). */
int kp_read_tables(kp_ctx* ctx, float* entity, float* relation);

/* ConvE full-model training (BCEOptimizer.train, bce_optimizer.py:45-150, on ConvE.forward
 * in train mode, conve.py:133-158), for verification's retraining
 * (verify_explanations.py:141-143): the context's tables, conv and FC layers are the
 * starting point and are trained in place; kp_conve_train_begin adds the three batch
 * norms' affine parameters and running statistics (1 + 32 + dim values each: BN1, BN2,
 * BN3) and resets Adam's state.  One kp_conve_train_step = one optimizer step on a batch
 * of B (head, relation) pairs: tails of pair b = tails[tail_off[b] .. tail_off[b+1])
 * (the er_vocab targets); in_noise [B][40 h], fm_noise [B][32], hid_noise [B][dim]: the
 * dropouts' multipliers (0 or 1 / (1 - p), drawn by the caller from the torch generator
 * in the forward's order; null = no dropout); lr = the epoch's learning rate
 * (ExponentialLR); bn_train = 0 runs the batch norms in eval mode (a one-pair batch).
 * Adam with torch's defaults on every parameter.  kp_conve_train_read copies the trained
 * layers back (the tables: kp_read_tables).  The context's eval-mode batch norm is not
 * updated: build a new context from the trained parameters to score with them. */
int kp_conve_train_begin(kp_ctx* ctx, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                         const float* bn_var);
int kp_conve_train_step(kp_ctx* ctx, int32_t B, const int32_t* pairs, const int32_t* tail_off, const int32_t* tails,
                        const float* in_noise, const float* fm_noise, const float* hid_noise, float lr,
                        float label_smoothing, int32_t bn_train);
int kp_conve_train_read(kp_ctx* ctx, float* conv_w, float* conv_b, float* fc_w, float* fc_b, float* bn_weight,
                        float* bn_bias, float* bn_mean, float* bn_var);

/* Data-poisoning relevance, ComplEx (src/relevance_engines/data_poisoning_engine.py:
 * DPEngine.get_gradient :21-49, NecessaryDPEngine.compute_relevance :52-94,
 * SufficientDPEngine.compute_individual_relevance :97-137; the other models have no
 * score_embeddings and raise in the reference).  items[n][7] = (pred s, p, o,
 * perspective entity e, triple h, r, t).  Per item: g = d score(s, p, o) / d emb(e)
 * (the lhs when e == s, else the rhs), e' = emb(e) + step_sign * (epsilon * g), the
 * triple's score with e' in its head when h == e (else in its tail), and
 * out[i] = rel_sign * (score - lambd * perturbed score). */
int kp_dp_relevance(kp_ctx* ctx, int32_t n, const int32_t* items, float epsilon, float lambd, int32_t step_sign,
                    int32_t rel_sign, float* out);

/* CRIAGE score variation (src/relevance_engines/criage_engine.py: compute_hessian
 * :74-104, estimate_score_variation :107-134 / :158-177), ComplEx and ConvE.
 * items[n][5] = (z_pred s, p, z_triple s, p, entity slot); z = criage_first_step
 * (complex.py:131, conve.py:102-124).  Entity slot k is ent_ids[k] with tail
 * triples (h, r) = tails[tails_off[k] .. tails_off[k+1]) in training order.
 * out[i] = z_pred . ((1 - sig) z_triple A^{-1}), A = H_e + sig (1 - sig) z^T z,
 * sig = sigmoid(e . z_triple), in float64 (the necessary engine negates it);
 * status[i] = 1 when A is exactly singular (numpy.linalg.inv raises). */
int kp_criage_relevance(kp_ctx* ctx, int32_t n, const int32_t* items, int32_t n_ents, const int32_t* ent_ids,
                        const int32_t* tails_off, const int32_t* tails, double* out, int32_t* status);

/* Advance a torch CPU generator state (the 5056-byte torch.get_rng_state()
 * blob) by n 32-bit mt19937 outputs, in place.  Used by the host RNG protocol
 * to replay the draws of reset_parameters() that each KelpieConvE
 * construction makes (conve.py:46-52 via :202) without materialising them. */
int kp_mt19937_discard(uint8_t* state, size_t state_len, uint64_t n);

/* Batches of deferred draws (the host RNG protocol, kelpie_amd/rng.py): every task queued
 * by kp_rng_transe_enqueue / kp_rng_transe_calls_async / kp_rng_conve_masks_enqueue is
 * tagged with the batch open at the time (tasks queued by a task inherit its tag).
 * kp_rng_batch_close closes the open batch and returns its id; kp_rng_batch_wait(id)
 * returns once every task of the batches <= id is done, while later batches' tasks may
 * still be queued or running -- so the thread that packs batch k waits for batch k's
 * draws while the scheduling thread already queues batch k + 1's (kp_rng_wait waits
 * for everything). */
int kp_rng_batch_close(int64_t* id);
int kp_rng_batch_wait(int64_t id);

/* torch.empty(n).normal_(mean, std) on the CPU generator for float32, n >= 16
 * (ATen normal_fill / normal_fill_AVX2, aten/src/ATen/native/cpu/DistributionTemplates.h),
 * bit for bit, advancing the state blob like torch.  cap = 1 for torch's AVX2 / AVX512 CPU
 * kernels (torch.backends.cpu.get_cpu_capability()), 0 for its scalar default kernel.
 * Replaces the xavier_normal_ of KelpieTransE (src/link_prediction/models/transe.py:93-95). */
int kp_rng_normal(uint8_t* state, size_t state_len, int64_t n, float mean, float std, int32_t cap, float* out);

/* Keep-mask of torch.empty(n).bernoulli_(p) on the CPU generator (ATen draws
 * one random64 = (hi << 32) | lo per element; keep iff u53 * 2^-53 < p), written
 * as packed bits (bit i of word i/32) and advancing the state blob in place.
 * Replaces the per-step hidden-dropout mask draw of KelpieConvE training
 * (conve.py:151 via model.py:114-125, Dropout stays in train mode). */
int kp_rng_bernoulli_bits(uint8_t* state, size_t state_len, uint64_t n, double p, uint32_t* out_bits);

/* One TransE post-training's draws (pairwise_ranking_optimizer.py:166-172) for
 * `epochs` epochs over R rows, from the two process-global generators the
 * reference uses: per epoch np.random.shuffle of the rows (numpy's legacy
 * MT19937 state: key[624] and *pos, from np.random.get_state()), then
 * torch.randint(n_entities, ratio*R) and torch.randint(2, ratio*R) on the torch
 * CPU generator.  Writes per epoch [row order (R) | entity (R) | head_or_tail (R)]
 * (only the first R of the ratio*R draws are stepped) and advances both states. */
int kp_rng_transe_epochs(uint8_t* torch_state, size_t torch_len, uint32_t* np_key, int32_t* np_pos, int32_t R,
                         int32_t epochs, int32_t ratio, int64_t n_entities, int32_t* out);

/* Deferred form of kp_rng_transe_epochs for a batch of slots scheduled in order:
 * snapshots the torch state, advances it past the slot's randints at once, and
 * queues the draws.  One worker thread runs the queued numpy shuffles in queue
 * order on the live numpy state at np_key / np_pos (which nobody else may touch
 * until kp_rng_wait returns); a small pool (KP_RNG_THREADS, default 4) fills the
 * randints from each snapshot.  `out` must stay valid until kp_rng_wait.
 * Same draws, same final states as calling kp_rng_transe_epochs per slot. */
int kp_rng_transe_enqueue(uint8_t* torch_state, size_t torch_len, uint32_t* np_key, int32_t* np_pos, int32_t R,
                          int32_t epochs, int32_t ratio, int64_t n_entities, int32_t* out);

/* The torch / numpy draws of n TransE compute_relevance calls, in the reference's order
 * (post_training_engine.py:46-62 with transe.py:93-95 and
 * pairwise_ranking_optimizer.py:166-181), in one library call.  Per call i:
 * torch.rand(1, D) (its values are overwritten, only the state advances), xavier_normal_
 * of the base kelpie row -> x_base[i] (kp_rng_normal, std = xavier_std), the base
 * post-training's epoch draws if R_base[i] >= 0, xavier_normal_ of the post-trained row
 * -> x_pt[i], and its epoch draws if R_pt[i] >= 0 (R = -1: the call schedules no such
 * post-training).  The epoch draws (as kp_rng_transe_epochs, deferred as
 * kp_rng_transe_enqueue: complete after kp_rng_wait) go to `out` back to back in that
 * order.  want (NULL = all): per call, bit 0 = the base post-training's draws are
 * wanted, bit 1 = the post-trained one's; an unwanted post-training (one that another
 * rank runs, kelpie_amd/distributed.py) only advances both generators and takes no
 * space in `out`.  d >= 16; x_base / x_pt are [n][d]. */
int kp_rng_transe_calls(uint8_t* torch_state, size_t torch_len, uint32_t* np_key, int32_t* np_pos, int32_t cap,
                        int32_t D, int32_t d, float xavier_std, int32_t n, const int32_t* R_base,
                        const int32_t* R_pt, const uint8_t* want, int32_t epochs, int32_t ratio,
                        int64_t n_entities, float* x_base, float* x_pt, int32_t* out);

/* kp_rng_transe_calls with the torch-stream walk on the library's walker thread: returns
 * at once; x_base, x_pt and out are complete after kp_rng_wait().  The walk starts from
 * torch_state unless an earlier asynchronous walk still carries the stream (it then
 * continues that one and torch_state is not read); kp_rng_torch_take hands the stream
 * back.  Lets the scheduling thread queue calls while the generator is advanced past
 * their draws (the randint outputs alone are ~22 M words per TransE batch).  Returns
 * KP_OK when queued, KP_INLINE when it walked inline (then nothing is carried). */
int kp_rng_transe_calls_async(const uint8_t* torch_state, size_t torch_len, uint32_t* np_key, int32_t* np_pos,
                              int32_t normal_cap, int32_t D, int32_t d, float xavier_std, int32_t n,
                              const int32_t* R_base, const int32_t* R_pt, const uint8_t* want, int32_t epochs,
                              int32_t ratio, int64_t n_entities, float* x_base, float* x_pt, int32_t* out);

/* Wait for every asynchronous walk; if one carries the torch stream, store it into
 * torch_state (*taken = 1) and release it, else *taken = 0 and torch_state is untouched. */
int kp_rng_torch_take(uint8_t* torch_state, size_t torch_len, int32_t* taken);

/* Block until every slot queued by kp_rng_transe_enqueue is written. */
int kp_rng_wait(void);

/* ConvE dropout keep bits for n_steps steps of rows_per_step[i] pairs.  Per step, the
 * forward's draws in order (conve.py:142,147,151): for each segment j < n_seg,
 * torch.empty(rows, seg_elems[j]).bernoulli_(seg_keep[j]) -- the input dropout over the
 * 40 x (d/20) image, the feature-map Dropout2d over 32 channels, the hidden dropout over
 * d -- each segment starting on a fresh 32-bit word.  A segment with keep == 0 (rate 1:
 * ATen draws nothing and returns zeros) gets zero words and consumes nothing.  Advances
 * the torch state. */
int kp_rng_conve_masks(uint8_t* torch_state, size_t torch_len, int32_t n_steps, const int32_t* rows_per_step,
                       int32_t n_seg, const int32_t* seg_elems, const double* seg_keep, uint32_t* out_words);

/* Deferred form of kp_rng_conve_masks (see kp_rng_transe_enqueue): advances the
 * torch state now, fills `out_words` on the worker pool; complete after kp_rng_wait. */
int kp_rng_conve_masks_enqueue(uint8_t* torch_state, size_t torch_len, int32_t n_steps, const int32_t* rows_per_step,
                               int32_t n_seg, const int32_t* seg_elems, const double* seg_keep,
                               uint32_t* out_words);

/* Device time of the last kp_posttrain_rank (HIP events on the context's
 * stream): the whole call, the summed durations of its dominant kernel's
 * launches, their count, and the work units those launches processed
 * (ComplEx: query rows x frozen entities; TransE: slot-epochs; ConvE:
 * encoder rows x frozen entities).  bench.py derives the roofline from it. */
int kp_last_timing(const kp_ctx* ctx, double* device_seconds, double* hot_kernel_seconds,
                   int64_t* hot_kernel_launches, double* hot_work_units);

/* How many batches have their device work in flight at once, this context's next
 * kp_posttrain_rank among them (n >= 1; 1, the default, is a batch that has the device
 * to itself).  The reference has no counterpart: PostTrainingEngine runs one post-training
 * at a time (post_training_engine.py:64-76).  A hint for the attention kernel's work
 * partition only (ComplEx: with n >= 2 a query tile is cut into fewer key ranges, since
 * other batches' workgroups fill what a launch leaves idle); results agree to rounding
 * for every n.  The caller sets it before each kp_posttrain_rank whose neighbours it
 * knows, and back to 1 afterwards. */
int kp_ctx_set_inflight(kp_ctx* ctx, int n);

/* The attention plan of the last kp_posttrain_rank's largest launch (ComplEx / ConvE;
 * zeros otherwise): out[0] = the in-flight hint it was planned with, out[1] = key ranges
 * per query tile (0: stream-K), out[2] = partial slots per query, out[3] = workgroups,
 * out[4] = the launch's queries. */
int kp_last_attn_plan(const kp_ctx* ctx, int32_t out[5]);

/* [start, end] (seconds, on a time base shared by every context of the device) of
 * each dominant-kernel launch of the last kp_posttrain_rank: *n = the launch count,
 * the first min(cap, *n) pairs are written to out[2 i], out[2 i + 1].  With batches
 * in flight on several contexts the launches can overlap; bench.py merges the
 * intervals to the time the device spent in the kernel. */
int kp_hot_intervals(const kp_ctx* ctx, int64_t cap, double* out, int64_t* n);

/* ---- candidate prefilters, host C++ ----------------
 * The undirected multigraph of TopologyPreFilter / WeightedTopologyPreFilter
 * (topology_prefilter.py:12-14, weighted_topology_prefilter.py:16-18): one
 * edge per training triple (h, t) over entities [0, n_ent); neighbour order is
 * networkx's insertion order.  Errors: kp_graph_last_error() (thread-local). */
typedef struct kp_graph kp_graph;
int kp_graph_create(int32_t n_ent, int64_t n_triples, const int32_t* triples, kp_graph** out);
void kp_graph_destroy(kp_graph* g);
const char* kp_graph_last_error(void);

/* Hop distance from each source to every entity, dist[i * n_ent + v]; -1 when
 * unreachable (nx.NetworkXNoPath -> 1e6 at topology_prefilter.py:36-37).  One
 * search from a prediction's object serves all of its candidates
 * (topology_prefilter.py:29-34 searches once per candidate; distances are symmetric). */
int kp_graph_bfs(const kp_graph* g, int32_t n_src, const int32_t* src, int32_t* dist);

/* Entity classes (CSR: class ids of entity v at cls[cls_off[v] .. cls_off[v+1]))
 * for the edge cost 1 - jaccard_similarity(classes(u), classes(v))
 * (weighted_topology_prefilter.py:40-44, utils/utils.py:11-14), float64. */
int kp_graph_set_classes(kp_graph* g, const int64_t* cls_off, const int32_t* cls);

/* nx.shortest_path_length(G, src[i], dst[i], weight=semantic_score) for each i
 * (weighted_topology_prefilter.py:46-56), replaying networkx's Dijkstra
 * (neighbour order, (distance, push counter) heap) so sums match bit for bit;
 * +inf when there is no path. */
int kp_graph_dijkstra_pairs(const kp_graph* g, int32_t n, const int32_t* src, const int32_t* dst, double* out);

/* ---- slot assembly of a post-training batch, host C++ ----
 * Replaces the per-call KelpieDataset work of the reference
 * (src/data/kelpie_dataset.py:13-158: the deep-copied kelpie dataset, its
 * remove_training_triples / add_training_triples edits and the to_filter lists
 * get_triple_results reads, post_training_engine.py:101-125) for a whole batch of
 * calls: one view per subject, one library call per run of calls, rows and filters
 * packed straight into kp_batch's arrays (csrc/kp_sched.cpp).
 *
 * kp_view_create: base[n][3] = the subject's training triples with the original entity
 * replaced by `kelpie` (the caller's order: Dataset.entity_to_training_triples),
 * extra[m][3] = its validation and test triples (they only enter the filters);
 * n_rel = |R| (inverse relation = p + n_rel). */
typedef struct kp_view kp_view;
typedef struct kp_sched_batch kp_sched_batch;
int kp_view_create(int32_t kelpie, int32_t n_rel, int32_t original, const int32_t* base, int32_t n,
                   const int32_t* extra, int32_t m, kp_view** out);
void kp_view_destroy(kp_view* v);
int kp_sched_batch_create(kp_sched_batch** out);
void kp_sched_batch_destroy(kp_sched_batch* b);

/* n calls: call c ranks (kelpie, rel[c], ·) after editing views[c] with the candidate
 * triples cands[cand_off[c] .. cand_off[c+1]) (original ids); flags[c]: bit 0 the call
 * needs its base post-training, bit 1 this process runs that base slot, bit 2 it runs the
 * edited (pt) slot, bit 3 sufficient mode (an addition; else a removal).  Per call and
 * slot (base, pt): slot_idx[2c + j] (-1: not run here), n_rows[2c + j] (rows incl.
 * inverses), n_filt[2c + j] (filter length).  The edits are checked in the reference's
 * order; at the first failing call fail = {call, code, triple}: code 1 a triple without
 * the entity (AssertionError), 2 not a kelpie training triple (KeyError), 3 a removal the
 * filter multiset cannot take (list.remove ValueError); that call's base slot is added,
 * nothing after it.  Otherwise fail[0] = -1.  The views must outlive the batch. */
int kp_sched_add_calls(kp_sched_batch* b, int32_t n, kp_view* const* views, const int32_t* rel, const uint8_t* flags,
                       const int32_t* cand_off, const int32_t* cands, int32_t* slot_idx, int32_t* n_rows,
                       int32_t* n_filt, int32_t* fail);

/* Rows (kelpie rows then their inverses, the optimizers' order) and rank filters of the
 * batch slots idx[0 .. n), back to back, into rows[rows_cap] / filt[filt_cap] (int32). */
int kp_sched_pack(const kp_sched_batch* b, int32_t n, const int32_t* idx, int32_t* rows, int64_t rows_cap,
                  int32_t* filt, int64_t filt_cap);

/* out[...] = the n int32 arrays (address ptrs[i], counts[i] values) back to back (the
 * slots' draws gathered into one upload buffer without holding the caller's lock). */
int kp_gather_i32(int32_t n, const uint64_t* ptrs, const int64_t* counts, int32_t* out, int64_t cap);

/* Library version string. */
const char* kp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KELPIE_HIP_H */
