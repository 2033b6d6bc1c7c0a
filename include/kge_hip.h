/*
 * kge_hip.h — C-ABI of the MI355X (gfx950) knowledge-graph-embedding hot path.
 *
 * Drop-in boundary for the scoring / self-adversarial-loss / filtered-ranking
 * path of kahrabian/KnowledgeGraphEmbedding.  The reference has no FFI: its
 * boundary is the Python methods of `KGEModel` (codes/model.py).  Each entry
 * point below names the reference interface it replaces (file:line); the
 * Python host mirror in knowledgegraphembedding_amd/ binds these through
 * ctypes (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (hipMalloc / torch CUDA tensors),
 *     row-major and contiguous.  Embeddings are fp32, indices int64 — the
 *     reference's own dtypes (model.py:45,52; dataloader.py:63-65).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Nothing here allocates, frees or synchronises: every call is meant to
 *     be graph-capturable (what is pinned: "Graph capture" below).  Scratch comes from a caller-owned workspace whose
 *     size the matching *_workspace_bytes() query returns.  The workspace
 *     must be 256-byte aligned (what hipMalloc gives): its sub-buffers sit at
 *     256-byte offsets from its base and are read 16 bytes at a time.  A
 *     call is meant to touch no byte beyond that size and to initialise
 *     whatever it reads, so the workspace needs no clearing
 *     (tests/test_arena_gpu.py, and tests/test_ship_stages_gpu.py for
 *     kge_ship_step, run the entries on
 *     a poisoned workspace of exactly the queried size; the end of the
 *     training layout is not written at its shapes, so there the exact size
 *     is exercised but a short one would not be noticed).
 *   - Graph capture (tests/test_graph_gpu.py).  A call captured on `stream`
 *     reads every DEVICE pointer's contents at replay: tables, ids, filter
 *     lists, weights and optimizer state may be overwritten in place between
 *     replays.  Every by-value argument and every descriptor's contents are
 *     those of the capture: kge_adam_desc / kge_adagrad_desc scalars
 *     (step_size and bias_correction2_sqrt: a captured Adam step replays with
 *     the bias corrections of the step it was captured at), kge_adam_step's
 *     and kge_adagrad_step's scalars, kge_sample_negatives' key, the ranking
 *     `flags` / path, kge_topk's k and parts, phase ranges, sizes.  Environment
 *     switches (KGE_RANK_SIDE, KGE_CSR_SERIAL, ...) are read at capture.  The
 *     stage timers (kge_stage_timer) must be off.  A first call may be
 *     captured cold: the side stream and its events are created inside the
 *     capture if need be (pinned for kge_rank_filtered_ex under
 *     KGE_RANK_SIDE=1 and kge_topk with k = 128 in a fresh process).
 *     Pinned against eager calls, bit for bit, on two input sets and repeated
 *     replays: kge_score, kge_rank_filtered_ex (every path, KGE_RANK_SIDE=1,
 *     KGE_RANK_REUSE_TABLE after a call of the same graph),
 *     kge_rank_filtered_both, kge_topk, kge_rank_candidates,
 *     kge_rank_relations, kge_sample_negatives, kge_adam_step,
 *     kge_adagrad_step.  These zero their counters and bitmaps with a kernel:
 *     a captured hipMemsetAsync replayed a stale fill pattern.
 *     NOT pinned: kge_score_backward, the kge_train_* family and
 *     kge_ship_step.  Their occurrence CSR still zeroes its bucket counts with
 *     hipMemsetAsync, and one captured factor-exchange program ended in a GPU
 *     memory fault whose cause was not established; treat their capture as
 *     unsupported.  Their multi-call protocols would in any case have to be
 *     captured whole, because the side stream forks in one call and joins in
 *     another: KGE_PHASE_ROWS forks, KGE_PHASE_ENTITY / KGE_PHASE_FINALIZE
 *     join; KGE_SHIP_ROWS forks, KGE_SHIP_CHAIN joins.  (kge_train_csr and
 *     kge_train_csr_range run on the caller's stream alone.)  A fork or join
 *     edge the runtime refuses is returned as KGE_ERR_HIP_BASE + hipError_t by
 *     the ranking and by kge_ship_step; the kge_train_* phases do not check
 *     theirs yet.  pRotatE's three-call ranking form has a host sin between
 *     its calls and cannot be one graph.
 *   - Large entity tables (tests/test_big_table_gpu.py).  Pinned on tables of
 *     2.16e9, 4.32e9 and 8.60e9 bytes (past 2^31 bytes, 2^32 bytes and 2^31
 *     floats), with ids on either side of each line: the ranking, top-k,
 *     gather, training and optimizer entries.  Ranking paths by table size:
 *     the split-bf16 MFMA tile (path 1) while its split operands stay under
 *     0x7FFFFFF0 bytes (a table of about 2 GiB), the fp32 MFMA tile (path 4)
 *     up to 0xFFFFFF00 table bytes, the register tile and the wave scan
 *     (paths 2 and 3) at any size; a path the table does not admit is
 *     KGE_ERR_ARG, and path 0 falls through them in that order.  NOT pinned:
 *     pRotatE ranking, tables of 2^32 elements (16 GiB) and more,
 *     kge_ship_step and the kge_train_step_from_rows* family on such tables.
 *   - Return value: 0 on success, a KGE_ERR_* code for argument errors
 *     (checked on the host before anything is launched), or a hipError_t
 *     (offset by KGE_ERR_HIP_BASE) if a launch fails.
 *   - Index range errors (reference: index_select raises, model.py:86-146)
 *     cannot be checked on the host without a sync; kernels clamp nothing,
 *     skip the offending row, and set *err_flag (a device int32) to
 *     KGE_DEVERR_INDEX.  The host mirror reads the flag at its next sync
 *     point and raises IndexError.
 */
#ifndef KGE_HIP_H
#define KGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Model ids: model.py:151-157 (the model_func plug-in registry). */
enum kge_model_id {
    KGE_TRANSE = 0,   /* model.py:166-173 */
    KGE_DISTMULT = 1, /* model.py:175-182 */
    KGE_COMPLEX = 2,  /* model.py:184-199 */
    KGE_ROTATE = 3,   /* model.py:201-229 */
    KGE_PROTATE = 4   /* model.py:231-249 */
};

/* Modes: model.py:83 'single', :104 'head-batch', :126 'tail-batch'. */
enum kge_mode_id { KGE_SINGLE = 0, KGE_HEAD_BATCH = 1, KGE_TAIL_BATCH = 2 };

enum kge_status {
    KGE_OK = 0,
    KGE_ERR_MODEL = 1,      /* ValueError('model %s not supported'), model.py:64,162 */
    KGE_ERR_MODE = 2,       /* ValueError('mode %s not supported'), model.py:149 */
    KGE_ERR_SHAPE = 3,      /* entity/relation dims inconsistent with the model (model.py:66-70) */
    KGE_ERR_ARG = 4,        /* null pointer / negative size */
    KGE_ERR_WORKSPACE = 5,  /* workspace smaller than *_workspace_bytes() */
    KGE_ERR_DIM = 6,        /* a size outside a kernel's range (negatives per row, queries per call, LDS) */
    KGE_ERR_ABI = 7,        /* kge_model_desc.struct_size != sizeof(kge_model_desc) of this library */
    KGE_ERR_HIP_BASE = 1000 /* + hipError_t */
};

/* Device-side error bits written to *err_flag. */
#define KGE_DEVERR_INDEX 1
#define KGE_DEVERR_SAMPLER 2 /* a row's true list left no room within max_draws draws */
#define KGE_DEVERR_ARG 4     /* kge_rank_sin_args / finish_sin: item_off or the list stage does not match */

/*
 * The parameters of one KGEModel (model.py:22-70).
 *   phase_divisor   = float(embedding_range.item() / 3.14159265358979323846)  model.py:202,209
 *   phase_divisor_p = float(embedding_range.item() / 3.14159262358979323846)  model.py:232,236-238
 *                     (the reference's pi typo is part of the contract)
 *   modulus         = device pointer to the pRotatE [1,1] modulus (model.py:59-60), else NULL
 *   relation_trig   = RotatE only, nullable: device [nrelation, 2, relation_dim] fp32 table of
 *                     (cos θ | sin θ) of every relation phase θ = relation / phase_divisor, as
 *                     the caller's reference evaluates them (model.py:209-212: the reference's
 *                     ATen CPU cos / sin).  The filtered ranking (kge_rank_filtered*) then builds
 *                     its queries' rotation from these values, so its ranks are the reference's
 *                     bit for bit; NULL = correctly rounded cos / sin on the device.  Training
 *                     and kge_score do not read it (scores are held to 1e-4, not to bits).
 *                     "The reference" is its CPU run: with --cuda its test_step evaluates
 *                     cos / sin and sum(dim=2) with ATen's GPU kernels, whose bits are not
 *                     reproduced here (parity against that configuration is unpinned).
 *
 * Alignment.  Every table is a contiguous array of 4-byte aligned floats.  When the row span
 * (entity_dim; its half for RotatE / ComplEx) is a multiple of 4 and entity_embedding and
 * relation_embedding are both 16-byte aligned, the kernels read rows in 16-byte slots; any
 * other table runs the same kernels with single-float slots.  With 16-byte slots the
 * gradient passes also write grad_entity / grad_relation, and stream a fused optimizer's
 * param / exp_avg / exp_avg_sq of the entity and relation tables (kge_adam_desc; likewise
 * kge_adagrad_desc's param / state_sum, but for a row-wise [nentity] state), 16 bytes
 * at a time: kge_score_backward, kge_train_step* and kge_ship_step return KGE_ERR_ARG,
 * before any launch, if one of those buffers is not 16-byte aligned (as kge_adam_step does
 * for its four arrays); relation_trig must then be 16-byte aligned too (kge_rank_filtered*).
 * With single-float slots none of these needs more than float alignment.  An entity table
 * that is not 16-byte aligned is ranked by the wave scan (path 3) only.
 */
typedef struct kge_model_desc {
    int32_t model;
    int32_t entity_dim;   /* floats per entity row   (model.py:42) */
    int32_t relation_dim; /* floats per relation row (model.py:43) */
    int32_t struct_size;  /* = sizeof(kge_model_desc) as the caller compiled it (else KGE_ERR_ABI) */
    int64_t nentity;
    int64_t nrelation;
    float gamma;          /* model.py:32-35 */
    float phase_divisor;
    float phase_divisor_p;
    float reserved_f;
    const float *entity_embedding;   /* [nentity, entity_dim] */
    const float *relation_embedding; /* [nrelation, relation_dim] */
    const float *modulus;            /* [1] or NULL */
    const float *relation_trig;      /* RotatE [nrelation, 2, relation_dim] or NULL (ranking only) */
} kge_model_desc;

/* Library identity: "knowledgegraphembedding_amd <KGE_ABI_VERSION> gfx950".  The
 * version changes with every change of a struct, a signature or a call
 * protocol in this header (0.3: pRotatE's three-call item counts; 0.4:
 * kge_rank_filtered_both, the ranking timer counting directions; 0.5: the
 * one-step-ahead training CSR entry point of an earlier 0.4 build removed);
 * loaders refuse a library whose version differs from the header they bind. */
#define KGE_ABI_VERSION "0.5"
const char *kge_version(void);
const char *kge_status_string(int status);

/*
 * Scores of a batch — replaces KGEModel.forward(sample, mode) (model.py:72-164)
 * together with the score plug-ins (model.py:166-249).
 *   mode == KGE_SINGLE:      pos[batch,3] triples, neg ignored, nneg must be 1 → out[batch,1]
 *   mode == KGE_HEAD_BATCH:  sample = (tail_part=pos[batch,3], head_part=neg[batch,nneg])
 *   mode == KGE_TAIL_BATCH:  sample = (head_part=pos[batch,3], tail_part=neg[batch,nneg])
 *   out: [batch, nneg] fp32.
 */
int kge_score(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
              int64_t batch, int64_t nneg, float *out, int32_t *err_flag, void *stream);

/*
 * Gradient of sum(grad_scores * score) w.r.t. the tables — replaces the autograd
 * of KGEModel.forward (IndexSelectBackward = dense zero-fill + index_add_, then
 * the plug-in's elementwise backward).
 *   grad_entity [nentity, entity_dim], grad_relation [nrelation, relation_dim] are
 *   OVERWRITTEN densely (rows no sample touches become 0); grad_modulus [1] is
 *   overwritten when non-NULL (pRotatE).
 */
size_t kge_backward_workspace_bytes(const kge_model_desc *m, int32_t mode, int64_t batch, int64_t nneg);
int kge_score_backward(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                       int64_t batch, int64_t nneg, const float *grad_scores, float *grad_entity,
                       float *grad_relation, float *grad_modulus, void *workspace, size_t workspace_bytes,
                       int32_t *err_flag, void *stream);

/*
 * Fused negative scoring + self-adversarial logsigmoid loss + backward —
 * replaces KGEModel.train_step (model.py:252-301) from the forward calls up to
 * and including loss.backward(); the optimizer step stays separate (kge_adam_step).
 *   mode:            KGE_HEAD_BATCH or KGE_TAIL_BATCH (dataloader.py:171-177 alternates them)
 *   pos [batch,3], neg [batch,nneg], subsampling_weight [batch]
 *   weight_sum:      device scalar Σw over the GLOBAL batch (data-parallel ranks all-reduce it);
 *                    NULL = computed from subsampling_weight of this call.
 *   uni_weight:      args.uni_weight (model.py:281-286)
 *   uni_batch:       the global batch size used for the uni_weight means (0 = batch)
 *   adversarial:     args.negative_adversarial_sampling; temperature = args.adversarial_temperature
 *   regularization:  args.regularization (model.py:290-296); 0 disables
 *   losses_out [5]:  {positive_sample_loss, negative_sample_loss, loss, regularization,
 *                     error flag} (device fp32; the reference's log dict, model.py:305-310,
 *                    plus a copy of *err_flag so one read-back serves both)
 *   grad_* overwritten densely, as in kge_score_backward.
 */
size_t kge_train_workspace_bytes(const kge_model_desc *m, int64_t batch, int64_t nneg);
int kge_train_step_grads(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                         int64_t batch, int64_t nneg, const float *subsampling_weight,
                         const float *weight_sum, int32_t uni_weight, int64_t uni_batch,
                         int32_t adversarial, float adversarial_temperature, float regularization,
                         float *grad_entity, float *grad_relation, float *grad_modulus,
                         float *losses_out, void *workspace, size_t workspace_bytes,
                         int32_t *err_flag, void *stream);

/* Phases of kge_train_step_grads, for callers that overlap the entity-gradient
 * reduction with the entity pass (data parallel, distributed.py): ROWS runs
 * the q build, the fused scoring/loss row pass, the epilogue, the occurrence
 * CSR and the relation pass; ENTITY runs the entity-major pass over rows
 * [entity_begin, entity_end) only (call it once per chunk, in any order, until
 * every row is covered); FINALIZE joins the relation pass and writes the
 * losses (and the pRotatE modulus gradient).  Same stream, same workspace,
 * same arguments in every phase; ALL = one kge_train_step_grads call.
 * [entity_begin, entity_end) is read by ENTITY (the rows of its chunk) and
 * by FINALIZE, which sums the regulariser's entity terms over it: pass
 * [0, nentity) to FINALIZE (a narrower range leaves the other rows out of
 * losses_out[2] and [3]).  ROWS ignores the range; any valid one will do. */
#define KGE_PHASE_ROWS 1
#define KGE_PHASE_ENTITY 2
#define KGE_PHASE_FINALIZE 4
#define KGE_PHASE_ALL 7
int kge_train_step_grads_phased(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                                int64_t batch, int64_t nneg, const float *subsampling_weight,
                                const float *weight_sum, int32_t uni_weight, int64_t uni_batch,
                                int32_t adversarial, float adversarial_temperature, float regularization,
                                float *grad_entity, float *grad_relation, float *grad_modulus, float *losses_out,
                                void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream,
                                int32_t phases, int64_t entity_begin, int64_t entity_end);

/*
 * kge_train_step_grads + the optimizer step, fused — replaces model.py:268-303
 * (forward, loss, loss.backward() AND optimizer.step()) for a torch.optim.Adam
 * optimizer (run.py:266-269).  The dense Adam update of every entity /
 * relation row (zero-gradient rows included, as torch's dense Adam does) is
 * applied in the gradient passes while each gradient row is in registers, so
 * gradients are never re-read from HBM.  The parameter pointers must be the
 * model's own tables (m->entity_embedding etc.; they are updated in place).
 * Per-tensor step_size = lr / (1 - beta1^t) and bias_correction2_sqrt =
 * sqrt(1 - beta2^t), computed in double by the caller (torch's formula).
 * write_grad != 0 also stores the dense gradients into grad_* (as
 * loss.backward() leaves them in .grad); 0 skips those writes.
 */
typedef struct kge_adam_tensor {
    float *param;
    float *exp_avg;
    float *exp_avg_sq;
    float step_size;
    float bias_correction2_sqrt;
} kge_adam_tensor;

typedef struct kge_adam_desc {
    kge_adam_tensor entity;
    kge_adam_tensor relation;
    kge_adam_tensor modulus; /* pRotatE only (param NULL otherwise) */
    float beta1, beta2, eps;
    int32_t write_grad;
} kge_adam_desc;

int kge_train_step(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                   int64_t batch, int64_t nneg, const float *subsampling_weight, const float *weight_sum,
                   int32_t uni_weight, int64_t uni_batch, int32_t adversarial, float adversarial_temperature,
                   float regularization, const kge_adam_desc *adam, float *grad_entity, float *grad_relation,
                   float *grad_modulus, float *losses_out, void *workspace, size_t workspace_bytes,
                   int32_t *err_flag, void *stream);

/*
 * LAZY entity Adam: kge_train_step with one difference, for the ENTITY table
 * only — the update covers the rows the batch touches, so a step's optimizer
 * traffic follows the batch (at most batch·nneg + 2·batch rows), not the table.
 *   Touched: a row with at least one in-range occurrence in the batch — a
 *     positive head, a positive tail or a negative — whether or not its
 *     gradient is zero.
 *   A touched row gets exactly kge_train_step's update: the same gradient bits
 *     (same occurrence order, same arithmetic) and the same per-element Adam,
 *     with adam->entity.step_size / bias_correction2_sqrt from the optimizer's
 *     GLOBAL step count (the caller's, as for kge_train_step; no per-row count).
 *   An untouched row's param, exp_avg and exp_avg_sq are neither read nor
 *     written (a dense step would decay its moments and move it by them).
 *   The relation table and the pRotatE modulus keep the dense Adam.
 * This is "lazy Adam" with this library's per-element update (eps added to
 * sqrt(exp_avg_sq) / bias_correction2_sqrt); it is NOT torch.optim.SparseAdam's
 * formula.  From zero moments one lazy step equals one dense step bit for bit
 * (an untouched row's dense update is p + (-step_size)·(0 / eps)).
 *   grad_entity is neither read nor written and may be NULL: no dense entity
 *     gradient exists.  grad_relation follows adam->write_grad as in kge_train_step.
 *   Single process, whole step: no phases, no entity range, no exchange stage.
 * Host checks, in kge_train_step's fixed order with the lazy step's own behind
 * the optimizer descriptor's: adam == NULL (KGE_ERR_ARG); the model; the mode;
 * grad_relation / losses_out; pos / neg / err_flag / batch / nneg; the adam
 * descriptor (an entity or relation tensor missing or not the model's own:
 * KGE_ERR_ARG); regularization != 0 (KGE_ERR_ARG: the L3 gradient is dense);
 * rows over 2048 floats per (half-)row (KGE_ERR_DIM); 16-byte alignment of the
 * streamed buffers; subsampling_weight; pRotatE's grad_modulus; the workspace
 * (KGE_ERR_WORKSPACE); nneg > 8192 (KGE_ERR_DIM).
 * Workspace: kge_train_lazy_workspace_bytes — kge_train_workspace_bytes plus the
 * touched-row list and its compaction's scratch.  The list (int32 ids,
 * ascending) and its length are built on the device behind the occurrence CSR,
 * O(nentity) integer work at 8 bytes per entity and nothing proportional to
 * nentity × entity_dim; no allocation, no synchronisation.
 */
size_t kge_train_lazy_workspace_bytes(const kge_model_desc *m, int64_t batch, int64_t nneg);
int kge_train_step_lazy(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                        int64_t batch, int64_t nneg, const float *subsampling_weight, const float *weight_sum,
                        int32_t uni_weight, int64_t uni_batch, int32_t adversarial, float adversarial_temperature,
                        float regularization, const kge_adam_desc *adam, float *grad_entity, float *grad_relation,
                        float *grad_modulus, float *losses_out, void *workspace, size_t workspace_bytes,
                        int32_t *err_flag, void *stream);

/*
 * Fused lazy ADAGRAD: kge_train_step_lazy with Adagrad in the place of Adam.
 * The rule, per element in IEEE fp32, one rounding per operation, no
 * contraction (lr and eps are the caller's doubles rounded to fp32):
 *   element-wise (entity_rowwise = 0; always the relation table and the
 *   pRotatE modulus), state_sum shaped like the parameter:
 *       s'  = s + g*g
 *       std = sqrtf(s') + eps
 *       p'  = p + (-lr) * (g / std)
 *   row-wise (entity_rowwise = 1, entity table only), state_sum [nentity]:
 *       G'   = G + (sum_k g_k*g_k) / (float)entity_dim
 *       std  = sqrtf(G') + eps
 *       p_k' = p_k + (-lr) * (g_k / std)
 *     the row sum in a fixed order: each of the 64 lanes adds the squares of
 *     its own elements in ascending slot order (a complex row's re element
 *     before the im element of the same dimension), then the wave's fixed tree
 *     (the order of the regulariser's per-row partial sum).
 * This is torch.optim.Adagrad's formula with lr_decay = 0, weight_decay = 0 and
 * initial_accumulator_value = 0 (no other setting is served); its CPU kernel
 * rounds g*g + s once, so its state can differ from this rule's by an ulp.
 * eps must be > 0: with eps = 0 an untouched all-zero row would be NaN under
 * the dense rule and untouched under this one.
 * A zero gradient changes nothing under the rule (s + 0, p + (-lr)*(0/std)),
 * so updating only the touched rows IS the dense update:
 *   A touched row gets the rule from the same gradient bits as kge_train_step
 *     (same occurrence order, same arithmetic).
 *   An untouched row's param and state are neither read nor written.
 *   The result equals applying the rule to every row of the dense gradient,
 *     bit for bit, at every step (no staleness, unlike the lazy Adam).
 * Everything else is kge_train_step_lazy's: a whole single-process step;
 * grad_entity neither read nor written (may be NULL); the touched-row list built
 * behind the occurrence CSR; no allocation, no synchronisation, capturable.
 * The row-wise kind runs the row-per-wave entity pass whatever the row length
 * (the sliced pass never holds a whole row).
 * Host checks, in this order: opt == NULL (KGE_ERR_ARG); the model; the mode;
 * grad_relation / losses_out; pos / neg / err_flag / batch / nneg; the
 * descriptor — struct_size (KGE_ERR_ABI), then, each KGE_ERR_ARG: an entity or
 * relation param / state_sum missing, a param that is not the model's own table
 * (pRotatE: a modulus.param that is not the model's or has no state_sum;
 * modulus.param NULL leaves the modulus alone), eps not > 0 (NaN included), lr
 * negative or not finite, entity_rowwise outside {0, 1}; regularization != 0
 * (KGE_ERR_ARG); rows over 2048 floats per (half-)row (KGE_ERR_DIM); with
 * 16-byte slots, 16-byte alignment of grad_relation and of the streamed param /
 * state_sum arrays (the row-wise [nentity] state needs float alignment only);
 * subsampling_weight; pRotatE's grad_modulus; the workspace
 * (KGE_ERR_WORKSPACE); nneg > 8192 (KGE_ERR_DIM).
 * Workspace: kge_train_adagrad_workspace_bytes = kge_train_lazy_workspace_bytes.
 */
typedef struct kge_adagrad_tensor {
    float *param;
    float *state_sum;
} kge_adagrad_tensor;

typedef struct kge_adagrad_desc {
    kge_adagrad_tensor entity;
    kge_adagrad_tensor relation;
    kge_adagrad_tensor modulus; /* pRotatE only (param NULL otherwise) */
    float lr, eps;
    int32_t entity_rowwise;     /* 0: entity.state_sum [nentity, entity_dim]; 1: [nentity] */
    int32_t write_grad;         /* grad_relation / grad_modulus, as kge_adam_desc.write_grad */
    int32_t struct_size;        /* = sizeof(kge_adagrad_desc) as the caller compiled it (else KGE_ERR_ABI) */
} kge_adagrad_desc;

size_t kge_train_adagrad_workspace_bytes(const kge_model_desc *m, int64_t batch, int64_t nneg);
int kge_train_step_adagrad(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                           int64_t batch, int64_t nneg, const float *subsampling_weight, const float *weight_sum,
                           int32_t uni_weight, int64_t uni_batch, int32_t adversarial,
                           float adversarial_temperature, float regularization, const kge_adagrad_desc *opt,
                           float *grad_entity, float *grad_relation, float *grad_modulus, float *losses_out,
                           void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * Data-parallel FACTOR EXCHANGE (distributed.py, exchange "factors"): instead
 * of all-reducing the dense [E, entity_dim] gradient, the ranks all-gather the
 * row pass's per-row factors — dL/ds [B, nneg], dL/dq [B, entity_dim] and the
 * row statistics [B, 4] — and every rank runs the rest of the step for the
 * GLOBAL batch itself.  On point-to-point xGMI with few ranks this moves
 * ~9 MB per rank instead of ~2·(N-1)/N · 120 MB (RotatE FB15k).
 *
 * kge_train_rows_slice: the negative-row pass (q build + k_row, no epilogue)
 * for `nrows` rows; pos/neg/subsampling_weight point at the slice's own rows,
 * weight_sum at the GLOBAL Σw (kge_weight_sum over all weights: the same
 * fixed order as a single process's in-kernel sum), uni_batch = global batch.
 * Writes g_out [nrows, nneg], dq_out [nrows, entity_dim] and columns 1-2 of
 * stats_out [nrows, 4] (pass the slice's place in the gathered buffers).
 * Workspace: kge_train_workspace_bytes(m, nrows, nneg).
 *
 * kge_train_step_from_rows: the rest of a kge_train_step (adam != NULL) or
 * kge_train_step_grads (adam == NULL) for the global batch from the gathered
 * buffers: q rebuilt, positive scores and chain rule, occurrence CSR, entity-
 * major and relation passes, losses.  Bit-identical to the single-process call
 * on the whole batch.  Workspace: kge_train_workspace_bytes(m, batch, nneg).
 */
int kge_train_rows_slice(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                         int64_t nrows, int64_t nneg, const float *subsampling_weight, const float *weight_sum,
                         int32_t uni_weight, int64_t uni_batch, int32_t adversarial, float adversarial_temperature,
                         float *g_out, float *dq_out, float *stats_out, void *workspace, size_t workspace_bytes,
                         int32_t *err_flag, void *stream);
int kge_train_step_from_rows(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                             int64_t batch, int64_t nneg, const float *subsampling_weight, const float *weight_sum,
                             int32_t uni_weight, int64_t uni_batch, float regularization, const float *g_in,
                             const float *dq_in, float *stats_inout, const kge_adam_desc *adam,
                             float *grad_entity, float *grad_relation, float *grad_modulus, float *losses_out,
                             void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * The same split with the occurrence CSR built ahead: kge_train_csr builds
 * the CSR of the (gathered) batch into the workspace on `stream` — it needs
 * only the ids, so a rank runs it while the factors are still on the wire —
 * and kge_train_step_from_rows_csr is kge_train_step_from_rows reading that
 * CSR instead of building it (same workspace, same batch).  Bit-identical.
 */
int kge_train_csr(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg, int64_t batch,
                  int64_t nneg, void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * kge_train_csr for an owner of the entity rows [entity_begin, entity_end):
 * only those entities' buckets are filled (the others stay empty; the
 * relation buckets are all built) — what kge_train_step_from_rows_phased /
 * _range with csr_ready read for that range, at 1/N of the fill and ordering
 * work of the whole batch's CSR.
 */
int kge_train_csr_range(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                        int64_t batch, int64_t nneg, int64_t entity_begin, int64_t entity_end, void *workspace,
                        size_t workspace_bytes, int32_t *err_flag, void *stream);
int kge_train_step_from_rows_csr(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                                 int64_t batch, int64_t nneg, const float *subsampling_weight,
                                 const float *weight_sum, int32_t uni_weight, int64_t uni_batch,
                                 float regularization, const float *g_in, const float *dq_in, float *stats_inout,
                                 const kge_adam_desc *adam, float *grad_entity, float *grad_relation,
                                 float *grad_modulus, float *losses_out, void *workspace, size_t workspace_bytes,
                                 int32_t *err_flag, void *stream);

/*
 * OWNER-COMPUTES step (partition.py, exchange "factors"): the rest of the step
 * from the gathered factors, with the entity-major pass — gradient, fused Adam
 * and regulariser — restricted to the caller's own rows [entity_begin,
 * entity_end) of the global batch's occurrences; the relation pass, the
 * positive epilogue and the losses cover the whole batch (identical on every
 * rank).  adam->entity.exp_avg / exp_avg_sq may point `entity_begin` rows
 * before the caller's shard-sized moment buffers (only owned rows are
 * touched).  reg_relations = 0 leaves the relation rows out of the
 * regularisation loss (another rank counts them); losses_out[3] then holds
 * this rank's part.  csr_ready: the CSR was built by kge_train_csr.
 */
int kge_train_step_from_rows_range(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                                   int64_t batch, int64_t nneg, const float *subsampling_weight,
                                   const float *weight_sum, int32_t uni_weight, int64_t uni_batch,
                                   float regularization, const float *g_in, const float *dq_in, float *stats_inout,
                                   const kge_adam_desc *adam, float *grad_entity, float *grad_relation,
                                   float *grad_modulus, float *losses_out, void *workspace, size_t workspace_bytes,
                                   int32_t *err_flag, void *stream, int64_t entity_begin, int64_t entity_end,
                                   int32_t csr_ready, int32_t reg_relations);

/*
 * kge_train_step_from_rows_range in phases (KGE_PHASE_ROWS: q rebuilt, the
 * positive epilogue, the relation pass; KGE_PHASE_ENTITY: the entity-major
 * pass + fused Adam of the rows [entity_begin, entity_end); KGE_PHASE_FINALIZE:
 * the losses, with the regulariser over [entity_begin, entity_end)), the same
 * arguments in every call.  An owner runs ROWS once, ENTITY once per chunk of
 * its rows — the all-gather of each finished chunk overlapping the next
 * chunk's pass — and FINALIZE over its whole range: bit-identical to one
 * kge_train_step_from_rows_range call.
 */
int kge_train_step_from_rows_phased(const kge_model_desc *m, int32_t mode, const int64_t *pos, const int64_t *neg,
                                    int64_t batch, int64_t nneg, const float *subsampling_weight,
                                    const float *weight_sum, int32_t uni_weight, int64_t uni_batch,
                                    float regularization, const float *g_in, const float *dq_in, float *stats_inout,
                                    const kge_adam_desc *adam, float *grad_entity, float *grad_relation,
                                    float *grad_modulus, float *losses_out, void *workspace, size_t workspace_bytes,
                                    int32_t *err_flag, void *stream, int32_t phases, int64_t entity_begin,
                                    int64_t entity_end, int32_t csr_ready, int32_t reg_relations);

/*
 * Query shipping: the training step of model.py:252-312 with the entity table
 * split into row shards, one per rank (no rank holds another's rows — the
 * reference's single table, model.py:45-53, never exists as a whole).  The
 * ranks exchange the global batch's ids and q vectors, not rows; every row-
 * side term is computed by the owner of the row.  The model descriptor's
 * entity_embedding points own_begin rows before this rank's shard and its
 * nentity is the GLOBAL entity count; the Adam entity pointers (and
 * grad_entity) are offset the same way.  Stages, each a call with the same
 * arguments, with the host's collectives between them:
 *   KGE_SHIP_Q      q_i (and head-batch the positive's h∘r) from the owner
 *                   of its row, zero elsewhere         → all-reduce(SUM) q[, qp]
 *   KGE_SHIP_ROWS   the owned negatives of every row: partial softmax state,
 *                   V relative to this shard's max (and the occurrence CSR,
 *                   on a side stream)                  → all-gather part → parts
 *   KGE_SHIP_MERGE  the rows' softmax over the shards (shard order), this
 *                   shard's dL/dq share and dL/ds; the positive triple on the
 *                   owner of t                         → all-reduce(SUM) dq | pstats [| pq]
 *   KGE_SHIP_CHAIN  chain rule on the owners of h / t; this shard's part of the
 *                   relation gradient (regulariser on rank 0) into
 *                   grad_relation                      → all-reduce(SUM) grad_relation,
 *                   relation Adam by the caller
 *   KGE_SHIP_ENTITY entity-major pass + fused Adam over [own_begin, own_end),
 *                   losses (regulariser partial of the owned rows; of the
 *                   relations on rank 0 only), pRotatE modulus grad + Adam
 * Same maths as one process on the global batch; the cross-shard sums run in
 * another order, so results agree to fp32 rounding, not bit for bit.
 *
 * Workspace: kge_train_workspace_bytes(m, ship->batch, ship->nneg) — the GLOBAL
 * batch, the same size on every rank; no rank offset enters it.  Same workspace
 * in every stage of a step (ROWS builds the occurrence CSR that CHAIN and
 * ENTITY read).  The per-row buffers of kge_ship_desc are the caller's, because
 * they cross the ranks between the stages; with B = batch, n = nneg, Le =
 * entity_dim, Lr = relation_dim, in floats, exactly:
 *   q, qp [B, Le]; part [B, 4]; parts [world, B, 4]; scores, g [B, n];
 *   dq, pq [B, Le]; pstats [B, 4]; ent_contrib [2B, Le]; rel_contrib [B, Lr];
 *   row_stats [B, 4].
 * qp and pq are touched head-batch only (they may be NULL tail-batch).  The
 * buffers that cross the ranks (q, qp, part, dq, pq, pstats) are written for
 * every row of the batch, owned or not (zeros where this shard has no share),
 * so the sums need no clearing; g and scores are written only where this
 * shard owns the negative, ent_contrib only in rows it owns.  With regularization,
 * losses_out[3] and the regulariser's part of losses_out[2] are this rank's
 * share: the caller sums losses_out[3] over the ranks.
 * (tests/test_ship_stages_gpu.py runs the stages on buffers of exactly these
 * sizes, every rank's table, gradient and moments inside a full-size poisoned
 * allocation: no row outside [own_begin, own_end) is read or written.)
 */
#define KGE_SHIP_Q 1
#define KGE_SHIP_ROWS 2
#define KGE_SHIP_MERGE 3
#define KGE_SHIP_CHAIN 4
#define KGE_SHIP_ENTITY 5
typedef struct kge_ship_desc {
  int32_t world, rank;
  int64_t own_begin, own_end;       /* entity rows this rank owns (global ids) */
  const int64_t *pos, *neg;         /* [B,3], [B,n] the global batch (all ranks' rows, rank order) */
  int64_t batch, nneg;              /* B (global), n */
  const float *subsampling_weight;  /* [B] */
  const float *weight_sum;          /* global Σw (device scalar; unused with uni_weight) */
  int32_t uni_weight, adversarial;
  int64_t uni_batch;
  float adversarial_temperature, regularization;
  float *q, *qp;                    /* [B, Le] each; qp: head-batch only */
  float *part;                      /* [B, 4] */
  const float *parts;               /* [world, B, 4] */
  float *scores, *g;                /* [B, n] each */
  float *dq, *pq, *pstats;          /* [B, Le], [B, Le] (head-batch), [B, 4] */
  float *ent_contrib, *rel_contrib; /* [2B, Le], [B, Lr] */
  float *row_stats;                 /* [B, 4] */
} kge_ship_desc;
int kge_ship_step(const kge_model_desc *m, int32_t mode, const kge_ship_desc *ship, int32_t stage,
                  const kge_adam_desc *adam, float *grad_entity, float *grad_relation, float *grad_modulus,
                  float *losses_out, void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);


/*
 * Σ subsampling_weight into *out (device scalar) — the denominator of
 * model.py:285-286; exposed so data-parallel ranks can all-reduce it.
 */
int kge_weight_sum(const float *w, int64_t n, float *out, void *stream);

/*
 * One dense Adam update — replaces torch.optim.Adam.step() as the reference
 * uses it (run.py:266-269, model.py:303; betas/eps defaults, no weight decay,
 * no amsgrad).  step_size = lr / (1 - beta1^t) and bias_correction2_sqrt =
 * sqrt(1 - beta2^t) are computed by the caller in double, as torch does.
 */
int kge_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t numel,
                  float beta1, float beta2, float eps, float step_size, float bias_correction2_sqrt,
                  void *stream);

/*
 * One dense element-wise Adagrad update (the rule of kge_train_step_adagrad)
 * over numel elements, like kge_adam_step: every array 16-byte aligned.
 * KGE_ERR_ARG, in this order: a NULL array or numel < 0; eps not > 0 (NaN
 * included), lr negative or not finite; (numel == 0 returns KGE_OK here;) an
 * array that is not 16-byte aligned.
 */
int kge_adagrad_step(float *param, const float *grad, float *state_sum, int64_t numel, float lr, float eps,
                     void *stream);

/*
 * Filtered link-prediction ranks — replaces the per-batch body of
 * KGEModel.test_step (model.py:383-418) with TestDataset's filter semantics
 * (dataloader.py:134-154).
 *   queries [nq,3] (h,r,t); mode KGE_HEAD_BATCH ranks the head, KGE_TAIL_BATCH the tail.
 *   filter CSR: for query q the ids filt_ids[filt_off[q] .. filt_off[q+1]) are the
 *   candidates (other than the true one) that form a true triple in
 *   all_true_triples; the reference gives them bias -1 and the true id
 *   (dataloader.py:138-144), so they never outrank the positive.
 *   ranks_out [nq] int64: 1 + #{unfiltered e != true : score_e > score_true}.
 *   ties_out  [nq] int32 (nullable): #{unfiltered e != true : score_e == score_true}
 *   (the reference's argsort is not stable; a tie may land either side).
 * "score" is the reference's own fp32 score: a fast fp32 pass counts every
 * candidate whose score clears the true one's by more than a rounding bound
 * and lists the rest, which are re-scored in the reference's operation order
 * (the ATen elementwise ops and its sum(dim=2) / norm(p=1) reduction order) —
 * bit-exact to the reference for TransE, DistMult and ComplEx, and for RotatE
 * when m->relation_trig holds the reference's cos / sin of the relation phases
 * (without it: correctly rounded values, which differ from the reference's
 * CPU vector library in the last bit on a few percent of arguments).
 * pRotatE's sin acts on per-candidate phase sums, so it cannot be tabulated:
 * correctly rounded in this one-call form (ranks equal the reference's up to
 * that last bit); bit-exact with the three-call form below
 * (KGE_RANK_STAGE_LIST, kge_rank_sin_args, kge_rank_finish_sin).
 */
size_t kge_rank_workspace_bytes(const kge_model_desc *m, int64_t nq);
int kge_rank_filtered(const kge_model_desc *m, int32_t mode, const int64_t *queries, int64_t nq,
                      const int64_t *filt_off, const int64_t *filt_ids, int64_t *ranks_out,
                      int32_t *ties_out, void *workspace, size_t workspace_bytes, int32_t *err_flag,
                      void *stream);
/*
 * The same with the fast pass chosen (path: 0 auto, 1 split-bf16 MFMA tile —
 * DistMult / ComplEx, 4 fp32 MFMA tile — DistMult / ComplEx with float4-aligned
 * rows, 2 register tile — reduction length % 4 == 0, 3 wave scan; paths 1, 2
 * and 4 need a 16-byte aligned entity table; KGE_ERR_ARG
 * if the rows do not suit the requested path) and
 * listed_out [nq] int32 (nullable): near-ties re-scored per query (above the
 * 1024-per-query list capacity the query is rescanned exactly).  Every path
 * returns the same ranks and ties.  path | KGE_RANK_REUSE_TABLE: the caller
 * asserts that the entity table's CONTENTS are unchanged since the last
 * ranking call on this workspace (the other direction or another query block
 * of one evaluation, any nq).  The table statistics and split operands that
 * call left at the start of the workspace are reused only where a tag written
 * beside them (on the device, stream-ordered) shows they were written for the
 * same table pointer and shape — a call on another table, or one whose path
 * wrote no split operands, makes this call recompute them.
 */
#define KGE_RANK_REUSE_TABLE 0x100
/* path | KGE_RANK_STAGE_LIST (pRotatE only, listed_out required, ranks_out
 * unused): stop after the fast pass — listed_out holds each query's near-tie
 * count and the lists stay in the workspace for kge_rank_sin_args /
 * kge_rank_finish_sin below. */
#define KGE_RANK_STAGE_LIST 0x200
/* path | KGE_RANK_FILTER_TABLE: filt_off / filt_ids are the whole filter
 * index instead of per-query lists: filt_off [E·R + 1] int64 start offsets,
 * by key h·R + r (tail-batch) or r·E + t (head-batch), into filt_ids — every
 * true triple's tail (tail-batch) or head (head-batch), sorted by key.  The
 * device looks each query's list up itself (no per-query CSR on the host);
 * the same ranks and ties. */
#define KGE_RANK_FILTER_TABLE 0x400
#define KGE_RANK_LIST_CAP 1024 /* listed near-ties per query; above it the query is rescanned in full */
int kge_rank_filtered_ex(const kge_model_desc *m, int32_t mode, const int64_t *queries, int64_t nq,
                         const int64_t *filt_off, const int64_t *filt_ids, int64_t *ranks_out,
                         int32_t *ties_out, int32_t *listed_out, int32_t path, void *workspace,
                         size_t workspace_bytes, int32_t *err_flag, void *stream);
/*
 * Both directions of one evaluation in one pass (model.py:349-418 ranks every
 * test triple as a head-batch query, then as a tail-batch query): the same
 * ranks and ties as kge_rank_filtered_ex(KGE_HEAD_BATCH, ...) followed by
 * kge_rank_filtered_ex(KGE_TAIL_BATCH, ...) on the same queries, written to
 *   ranks_out / ties_out / listed_out [2·nq]: the head-batch direction's nq,
 *   then the tail-batch direction's;
 * filt_off_head / filt_ids_head and filt_off_tail / filt_ids_tail: each
 * direction's filter (per-query lists, or with KGE_RANK_FILTER_TABLE each
 * direction's whole filter index).  The workspace holds 2·nq queries
 * (kge_rank_workspace_bytes(m, 2·nq)).  The mode-independent stages — the
 * table's statistics and split operands, the split of every q, the MFMA
 * counting tile and the emission — run once over all 2·nq queries; the
 * mode-dependent ones (q, filter bitmap, windows, refinement) once per
 * direction.  Not with KGE_RANK_STAGE_LIST (pRotatE's three-call form is per
 * direction): KGE_ERR_ARG.
 */
int kge_rank_filtered_both(const kge_model_desc *m, const int64_t *queries, int64_t nq,
                           const int64_t *filt_off_head, const int64_t *filt_ids_head,
                           const int64_t *filt_off_tail, const int64_t *filt_ids_tail, int64_t *ranks_out,
                           int32_t *ties_out, int32_t *listed_out, int32_t path, void *workspace,
                           size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * Top-k link prediction — "given (h, r), which tails score highest?" (the
 * reference has no such method: its users call KGEModel.forward with every
 * entity as a negative, model.py:72-164, and torch.topk the [nq, E] scores).
 *   queries [nq,3] (h,r,t); KGE_TAIL_BATCH predicts tails from (h, r),
 *   KGE_HEAD_BATCH heads from (r, t).  The predicted column is never read and
 *   never range-checked (callers may pass -1).  An out-of-range id in one of
 *   the other two columns sets KGE_DEVERR_INDEX and fills that query's outputs
 *   with id -1 and score NaN; the other queries proceed.
 *   filt_off / filt_ids: the candidates to exclude, in the two forms of
 *   kge_rank_filtered_ex — per-query lists, or with path | KGE_RANK_FILTER_TABLE
 *   the whole filter index; filt_off == NULL: no filter.  There is no "true
 *   id": nothing is excluded beyond the lists.
 *   ids_out [nq,k] int64, scores_out [nq,k] fp32: each query's k best
 *   unexcluded candidates ordered by (score descending, id ascending) — a total
 *   order, so the result is deterministic and does not depend on `parts`, on
 *   the launch geometry or on which other queries share the call.  If fewer
 *   than k candidates remain, the tail is padded with id -1 and score -inf.  A
 *   candidate whose score is NaN (or -inf, which the padding means) is never
 *   selected.
 * "score" is the fast pass's own fp32 score — the per-element arithmetic of the
 * ranking's fast pass, with device cos / sin for RotatE (relation_trig is not
 * read).  UNLIKE the ranks of kge_rank_filtered*, which are the reference's bit
 * for bit, these scores agree with the reference to the score tolerance
 * (1e-4 * max(|s|, 1), as kge_score), so candidates whose reference scores lie
 * closer than that may come out in the other order.
 *   path low bits: 0 auto, 2 register tile, 3 wave scan, with the eligibility
 *   rules of kge_rank_filtered_ex (2 for rows the tile cannot take:
 *   KGE_ERR_ARG).  The MFMA paths 1 and 4 have no top-k form: KGE_ERR_ARG.
 *   The two paths may differ in the last bits of a score; each alone is
 *   deterministic.  Rows over 2048 floats per (half-)row: KGE_ERR_DIM.
 *   parts: the number of candidate ranges the table is cut into (at most 64,
 *   and at most one per 64 candidates); 0 = chosen so that the grid fills the
 *   device when nq is small.  Each (query block, part) produces a partial
 *   list; a merge kernel reduces them.
 * Host checks, in this order: the model (as every entry), mode, then null
 * queries / ids_out / scores_out / err_flag, nq < 0, parts < 0 or a bad path
 * (KGE_ERR_ARG); nq == 0 returns KGE_OK; k < 1 or k > KGE_TOPK_MAX_K and
 * nq > 65535 (KGE_ERR_DIM); the path's fit; the workspace (KGE_ERR_WORKSPACE).
 * The workspace holds the q vectors, the bitmap, pRotatE's phase tables and the
 * [nq, parts, k] partial lists — never an [nq, E] score matrix.
 */
#define KGE_TOPK_MAX_K 128
size_t kge_topk_workspace_bytes(const kge_model_desc *m, int64_t nq, int32_t k, int32_t parts);
int kge_topk(const kge_model_desc *m, int32_t mode, const int64_t *queries, int64_t nq,
             const int64_t *filt_off, const int64_t *filt_ids, int32_t k, int64_t *ids_out,
             float *scores_out, int32_t path, int32_t parts, void *workspace, size_t workspace_bytes,
             int32_t *err_flag, void *stream);

/*
 * Ranks against PER-QUERY CANDIDATE LISTS — the OGB link-prediction protocol
 * (each test triple ranked against its own fixed list of heads or tails) and
 * sampled validation (the reference has neither: its users call
 * KGEModel.forward with the candidates as negatives, model.py:72-164, and
 * compare the [nq, ncand] scores themselves).
 *   queries [nq,3] (h,r,t); KGE_HEAD_BATCH ranks h among candidate heads,
 *   KGE_TAIL_BATCH t among candidate tails.
 *   cand [nq, ncand] int64, row-major: query q's candidates.  A negative id is
 *   padding and is skipped (ragged lists are padded with -1).
 *   ranks_out [nq] int64: 1 + #{j : cand[q,j] >= 0, score(cand[q,j]) > score(true)}.
 *   ties_out  [nq] int32 (nullable): the same count with ==.
 *   Nothing else is excluded: there is no filter, and a candidate equal to the
 *   true id, or a duplicate, counts like any other (a copy of the true id is a
 *   tie) — what comparing forward's scores gives, and what OGB's evaluator
 *   combines as 1 + gt + ties / 2.
 * "score" is the reference's fp32 score on the contract of kge_rank_filtered:
 * the true entity and every candidate are scored in the mode's reference
 * operation order (no fast pass) — bit-exact for TransE, DistMult and ComplEx,
 * for RotatE when m->relation_trig holds the reference's cos / sin (NULL:
 * correctly rounded on the device), and pRotatE with the correctly rounded
 * device sin as in the one-call form of kge_rank_filtered (there is no
 * three-call form here).
 *   A query with h, r or t out of range sets KGE_DEVERR_INDEX and gets rank 0
 *   and ties 0; a candidate id >= nentity sets KGE_DEVERR_INDEX and is skipped,
 *   the rest of its query proceeds.
 *   Rows of any width and alignment: 16-byte slots or single floats by the
 *   alignment rule above (relation_trig needs float alignment only); rows too
 *   wide to stage in LDS are read in place.  Queries go on grid.x: one call
 *   takes any nq and ncand whose (query, candidate chunk) count stays below
 *   2^31 — the 65,535-query ceiling of the other ranking calls does not apply.
 *   The counts are integer sums over the chunks: deterministic, and independent
 *   of the launch geometry.
 * Host checks, in this order: the model (as every entry); the mode (KGE_SINGLE:
 * KGE_ERR_MODE); null queries / cand / ranks_out / err_flag, nq < 0 or
 * ncand < 1 (KGE_ERR_ARG); nq == 0 returns KGE_OK; more work items than
 * grid.x holds (KGE_ERR_DIM); the workspace (KGE_ERR_WORKSPACE).
 * The workspace holds two int32 counters per query (and the queries' q vectors
 * when rows are read in place) — never an [nq, ncand] score matrix.
 */
size_t kge_rank_candidates_workspace_bytes(const kge_model_desc *m, int64_t nq, int64_t ncand);
int kge_rank_candidates(const kge_model_desc *m, int32_t mode, const int64_t *queries, int64_t nq,
                        const int64_t *cand, int64_t ncand, int64_t *ranks_out, int32_t *ties_out,
                        void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * RELATION PREDICTION — "which relation holds between h and t?": every query
 * (h, r, t) of queries [nq,3] is scored with every relation r' in
 * [0, nrelation), and its own r is ranked among them (the reference has no such
 * call: its users flatten nq × R triples through KGEModel.forward(mode='single')).
 * "score" is the reference's fp32 score of the triple (h, r', t) in 'single'
 * mode — (h + r') − t, (h * r') * t, the non-head-batch branch of
 * model.py:166-249, reduced by ATen's sum(dim=2) / norm(p=1) — on the contract
 * of kge_rank_candidates: bit-exact for TransE, DistMult and ComplEx, for RotatE
 * when m->relation_trig holds the reference's cos / sin (NULL: correctly rounded
 * on the device, evaluated once per relation into a table in the workspace),
 * and pRotatE with the correctly rounded device sin — its sin acts on the
 * phase sum (h + r') − t, so no table can carry it and it is evaluated per
 * (query, relation, element); there is no three-call form here.
 *   filt_off [nq + 1] / filt_ids: per-query lists of relation ids to exclude —
 *   the other relations r' with (h, r', t) a known true triple; both NULL: no
 *   filter.  Listing the true r, an id twice or an id outside [0, nrelation)
 *   is harmless and no error.
 *   ranks_out [nq] int64: 1 + #{r' != r, r' not excluded : score(r') > score(r)}.
 *   ties_out  [nq] int32 (nullable): the same count with ==.  The true relation
 *   is never counted against itself (as kge_rank_filtered, unlike
 *   kge_rank_candidates).
 *   scores_out [nq, nrelation] float (nullable): the score of every relation,
 *   excluded ones included — the only [nq, nrelation] object of the call, and
 *   the caller's; the workspace never holds one.
 *   r == -1 means "no true relation" (prediction): rank 0, ties 0, the scores
 *   are written, no error.  Any other r outside [0, nrelation), or an h or t
 *   outside [0, nentity), sets KGE_DEVERR_INDEX and gives that query rank 0,
 *   ties 0 and a NaN row of scores_out; the other queries proceed.
 *   Rows of any width and alignment: 16-byte slots or single floats by the
 *   alignment rule above (RotatE: of the entity table and the trig table);
 *   rows too wide to stage h, t and one relation row in LDS are read in place.
 *   The counts are integer sums over chunks of the relation range:
 *   deterministic, and independent of the launch geometry.  Queries go on
 *   grid.x: the 65,535-query ceiling of the other ranking calls does not apply.
 * Host checks, in this order: the model (as every entry); null queries /
 * ranks_out / err_flag (KGE_ERR_ARG); nq < 0 (KGE_ERR_ARG); filt_off and
 * filt_ids not both NULL or both set (KGE_ERR_ARG); nq == 0 returns KGE_OK;
 * more (query, relation chunk) work items than grid.x holds (KGE_ERR_DIM); the
 * workspace (KGE_ERR_WORKSPACE).  There is no mode argument.
 * The workspace holds two int32 counters per query, and RotatE's
 * [nrelation, 2, relation_dim] table when relation_trig is NULL.
 */
size_t kge_rank_relations_workspace_bytes(const kge_model_desc *m, int64_t nq);
int kge_rank_relations(const kge_model_desc *m, const int64_t *queries, int64_t nq,
                       const int64_t *filt_off, const int64_t *filt_ids,
                       int64_t *ranks_out, int32_t *ties_out, float *scores_out,
                       void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * SHARDED FILTERED RANKING — the filtered ranks of kge_rank_filtered over an
 * entity table that is split into row shards, one per rank, evaluated in place:
 * no rank ever holds another's rows (the evaluation half of "Query shipping"
 * above).  The conventions are kge_ship_step's: m->entity_embedding points
 * own_begin rows BEFORE this rank's shard, m->nentity is the GLOBAL count, and
 * only rows [own_begin, own_end) are read.  A rank is a count of candidates
 * whose reference-order fp32 score beats the true one's, so the shards' counts
 * sum to the single-process rank bit for bit.  One entry, three stages, each a
 * call with the same arguments, with the host's collectives between them:
 *   KGE_RSHARD_ROWS   fixed_rows[q] = the row of the query's fixed side (t
 *                     head-batch, h tail-batch) where this rank owns it, all-zero
 *                     bits elsewhere         → all-reduce(SUM) fixed_rows viewed
 *                     as int32 (adding zero integers keeps every bit, −0.0 too).
 *                     A fixed-side id outside [0, nentity) sets KGE_DEVERR_INDEX
 *                     and leaves zeros.
 *   KGE_RSHARD_TRUE   reads the reduced fixed_rows; s_true[q] = the reference-
 *                     order score of the true triple (the bits kge_rank_candidates
 *                     gives the true entity) where this rank owns the ranked
 *                     entity (h head-batch, t tail-batch), zero bits elsewhere
 *                     and for a query with an id out of range
 *                                            → all-reduce(SUM) s_true as int32.
 *   KGE_RSHARD_COUNT  reads the reduced fixed_rows and s_true;
 *                     counts[0][q] = #{e in [own_begin, own_end), e != true id,
 *                     e not in the query's filter list : score(e) > s_true[q]},
 *                     counts[1][q] the same with ==  → all-reduce(SUM) counts
 *                     (int64); rank = 1 + counts[0], ties = counts[1].
 *                     A query with h, r or t out of range gets 0 / 0 and sets
 *                     KGE_DEVERR_INDEX; the other queries proceed.  Filter-list
 *                     ids outside the shard (or outside the table) are simply
 *                     not this shard's: no error.
 * "score" is the reference's fp32 score on the contract of kge_rank_candidates:
 * every owned row is scored in the mode's reference operation order (no fast
 * pass) — bit-exact for TransE, DistMult and ComplEx, for RotatE when
 * m->relation_trig holds the reference's cos / sin (NULL: correctly rounded on
 * the device), and pRotatE with the correctly rounded device sin (there is no
 * three-call form here).
 *   flags: 0 = filt_off [nq + 1] / filt_ids are per-query lists;
 *   KGE_RANK_FILTER_TABLE = they are the whole filter index, as
 *   kge_rank_filtered_ex.  Lists may be empty, repeat ids and list the true id.
 *   own_begin == own_end is a valid empty shard: ROWS and TRUE write zeros,
 *   COUNT writes zero counts.
 *   Rows of any width and alignment: 16-byte slots or single floats by the
 *   alignment rule above (of the shard's first row and the relation table;
 *   fixed_rows, s_true and relation_trig need float alignment only); rows too
 *   wide to stage in LDS are read in place.  Queries go on grid.x: the
 *   65,535-query ceiling of kge_rank_filtered* does not apply, and there is no
 *   [nq, E/32] bitmap — each workgroup builds the exclusion bits of its own
 *   chunk of at most 1024 rows in LDS.  The counts are integer sums over the
 *   chunks: deterministic, and independent of the launch geometry
 *   (KGE_RANK_SHARD_CHUNK, diagnostic: rows per chunk; KGE_RANK_SHARD_QPW,
 *   diagnostic: 2 or 4 queries share every staged row of a workgroup).
 *   Nothing allocates or synchronises; counts is zeroed by a kernel.  Every
 *   stage writes its output for every query, so no buffer needs clearing.
 * Host checks, in this order: the model (as every entry); the mode (KGE_SINGLE:
 * KGE_ERR_MODE); a NULL descriptor (KGE_ERR_ARG), then its struct_size
 * (KGE_ERR_ABI); then KGE_ERR_ARG for a stage that is not one of the three,
 * own_begin > own_end or a range outside [0, nentity], flags other than 0 or
 * KGE_RANK_FILTER_TABLE, null queries / err_flag or nq < 0, and a NULL buffer
 * of the stage (ROWS: fixed_rows; TRUE: fixed_rows, s_true; COUNT: fixed_rows,
 * s_true, counts, filt_off, filt_ids); nq == 0 returns KGE_OK; more queries
 * (COUNT: (chunk, query) work items) than grid.x holds (KGE_ERR_DIM); the
 * workspace (KGE_ERR_WORKSPACE).
 * The workspace holds the queries' q vectors when rows are read in place, and
 * nothing otherwise (a 256-byte minimum); any stage may use any workspace.
 * NOT pinned for this entry: graph capture, and tables past 2 GiB (row offsets
 * are 64-bit, but no test runs it there).
 */
#define KGE_RSHARD_ROWS  1
#define KGE_RSHARD_TRUE  2
#define KGE_RSHARD_COUNT 3
typedef struct kge_rank_shard_desc {
  int32_t struct_size;          /* = sizeof(kge_rank_shard_desc) (else KGE_ERR_ABI) */
  int32_t flags;                /* 0 or KGE_RANK_FILTER_TABLE */
  int64_t own_begin, own_end;   /* global ids; own_begin == own_end is a valid empty shard */
  float *fixed_rows;            /* [nq, entity_dim]: row of h (tail-batch) / t (head-batch) */
  float *s_true;                /* [nq]: reference-order score of the true triple */
  const int64_t *filt_off, *filt_ids; /* as kge_rank_filtered_ex, both forms */
  int64_t *counts;              /* [2, nq]: row 0 strictly greater, row 1 equal */
} kge_rank_shard_desc;
size_t kge_rank_shard_workspace_bytes(const kge_model_desc *m, int64_t nq);
int kge_rank_shard(const kge_model_desc *m, int32_t mode, const kge_rank_shard_desc *sh, int32_t stage,
                   const int64_t *queries, int64_t nq, void *workspace, size_t workspace_bytes,
                   int32_t *err_flag, void *stream);

/*
 * SHARDED FILTERED RANKING, THE FAST COUNTING PASS — a drop-in for the call
 * kge_rank_shard(..., KGE_RSHARD_COUNT, ...): the same descriptor and
 * conventions (the entity pointer own_begin rows before the shard, nentity the
 * global count, only rows [own_begin, own_end) read, fixed_rows and s_true the
 * reduced outputs of the ROWS and TRUE stages), and sh->counts [2, nq] bit for
 * bit what KGE_RSHARD_COUNT writes for the same arguments — a query with an id
 * out of range (0 / 0 and KGE_DEVERR_INDEX), an empty shard, filter ids outside
 * the shard or the table (no error), lists that repeat ids or list the true id,
 * both filter forms, a true id owned by another rank.  A rank is an integer
 * count: the fast pass of kge_rank_filtered_ex runs on a shard-local view (rows
 * = own_end - own_begin, local id = global id - own_begin), counts every owned
 * candidate whose fast score clears the query's near-tie window around s_true,
 * and scores the others in the reference's order against the given s_true[q].
 * s_true is already the reference-order score, so the window has to cover the
 * candidate's own fast-pass error only; it uses the SHARD's table statistics.
 * The true row is never read (its owner may be another rank); neither is the
 * table row of the fixed side: q comes from fixed_rows[q] and the relation row
 * (RotatE: m->relation_trig as in the other ranking entries).
 *   listed_out [nq] int32, nullable: the owned candidates of query q that were
 *   scored in the reference's order; 0 on path 3; above KGE_RANK_LIST_CAP the
 *   query was rescanned exactly over the own rows (so is a query whose s_true
 *   is infinite: no window catches a score of the same infinity).  The table's
 *   rows are assumed finite, as by kge_rank_filtered_ex's fast paths: a fast
 *   score that is NaN where the reference's is infinite is not listed.
 *   sh->flags = path | optional KGE_RANK_FILTER_TABLE.  Paths:
 *     0  auto: 1 where it fits, else 2 where it fits, else 3.
 *     1  split-bf16 MFMA tile: DistMult and ComplEx, the shard's first row
 *        16-byte aligned, the split operands within 32-bit buffer offsets.
 *     2  register tile: TransE, DistMult, ComplEx and RotatE with reduction
 *        length % 4 == 0 and the shard's first row 16-byte aligned (the
 *        shard's alignment decides, not the table's, as in kge_topk_shard).
 *     3  exact: KGE_RSHARD_COUNT's own kernel, for every shape that stage
 *        serves.
 *   An explicit path the shard's rows do not admit is KGE_ERR_ARG; so is path 4
 *   (the fp32 MFMA tile is not offered here) and any path above 4.  pRotatE
 *   resolves to path 3 — its window rests on the score-interval argument of the
 *   one-table pipeline, which has no given-s_true form yet — and an explicit 1 or
 *   2 for pRotatE is KGE_ERR_ARG.  Rows over 2048 floats per (half-)row, and a
 *   RotatE relation_trig that is not 16-byte aligned while fixed_rows and the
 *   relation table are, resolve to 3 likewise.
 *   kge_rank_shard_fast_path: the path a call with these arguments takes (1, 2
 *   or 3), or minus the status it is refused with.  fixed_rows must be set: its
 *   alignment picks the q kernel's slots.
 *   The call runs on the caller's stream only, allocates and synchronises
 *   nothing, and every buffer it reads is initialised by a kernel.  The shard's
 *   statistics and split operands are recomputed every call
 *   (KGE_RANK_REUSE_TABLE is not offered).  Deterministic: the counts are
 *   integers, whatever order the list was filled in.
 * Host checks, in this order: the model; the mode; a NULL descriptor
 * (KGE_ERR_ARG), then its struct_size (KGE_ERR_ABI); then KGE_ERR_ARG for
 * own_begin > own_end or a range outside [0, nentity], flags with bits other
 * than 7 | KGE_RANK_FILTER_TABLE or a path above 4, null queries / err_flag or
 * nq < 0, and a NULL fixed_rows, s_true, counts, filt_off or filt_ids;
 * nq == 0 returns KGE_OK; a resolved path 3 continues with KGE_RSHARD_COUNT's
 * checks (its grid rule, its workspace); nq > 65535 on a resolved path 1 or 2
 * (KGE_ERR_DIM: the bitmap and tile launches put queries on grid.y); the path's
 * fit (KGE_ERR_ARG); the workspace (KGE_ERR_WORKSPACE).
 * The workspace (kge_rank_shard_fast_workspace_bytes; 0 for arguments the call
 * refuses) holds the fast and reference q vectors, the counters,
 * nq x KGE_RANK_LIST_CAP list entries, the shard's bitmap [nq, ceil(rows/32)],
 * the statistics and, on path 1, the split operands of the own rows and of q.
 * It grows with the shard, never with the table, and holds no [nq, rows] score
 * matrix; on path 3 it is kge_rank_shard_workspace_bytes.
 * NOT pinned for this entry: graph capture, and tables past 2 GiB.
 */
size_t kge_rank_shard_fast_workspace_bytes(const kge_model_desc *m, const kge_rank_shard_desc *sh, int64_t nq);
int kge_rank_shard_fast_path(const kge_model_desc *m, const kge_rank_shard_desc *sh);
int kge_rank_shard_fast(const kge_model_desc *m, int32_t mode, const kge_rank_shard_desc *sh,
                        const int64_t *queries, int64_t nq, int32_t *listed_out,
                        void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * SHARDED RANKING AGAINST CANDIDATE LISTS — kge_rank_candidates over an entity
 * table that is split into row shards, one per rank, evaluated in place: no
 * rank ever holds another's rows.  The conventions are kge_rank_shard's:
 * m->entity_embedding points own_begin rows BEFORE this rank's shard,
 * m->nentity is the GLOBAL count, and only rows [own_begin, own_end) are read.
 * Every rank passes the same queries and the same lists.  Per block of queries:
 *   1. kge_rank_shard(KGE_RSHARD_ROWS)  → all-reduce(SUM) fixed_rows as int32;
 *   2. kge_rank_shard(KGE_RSHARD_TRUE)  → all-reduce(SUM) s_true as int32;
 *   3. this call                        → all-reduce(SUM) counts (int64);
 *      rank = 1 + counts[0], ties = counts[1].
 * (Stages 1 and 2 take a kge_rank_shard_desc; this call its own descriptor.)
 *   counts[0][q] = #{j : own_begin <= cand[q,j] < own_end,
 *                        score(cand[q,j]) > s_true[q]},
 *   counts[1][q] the same with ==.
 * "score" is the score of kge_rank_candidates: the mode's reference operation
 * order, no fast pass, the same per-model exactness (RotatE reads
 * m->relation_trig; pRotatE uses the correctly rounded device sin).  A rank is
 * an integer count, so summed over a partition's shards the counts equal
 * kge_rank_candidates' (rank − 1, ties) on the whole table, bit for bit.
 *   Nothing is excluded: an owned copy of the true id is a tie, duplicates count
 *   each time.  A negative id is padding.  An id >= nentity sets
 *   KGE_DEVERR_INDEX and is skipped (every rank sees every list, so every rank
 *   flags it); an id inside the table but outside the shard is simply not this
 *   shard's.  A query with h, r or t out of range gets 0 / 0 and sets
 *   KGE_DEVERR_INDEX, on an empty shard too; the other queries proceed.
 *   own_begin == own_end is a valid empty shard: zero counts.
 *   Rows of any width and alignment: 16-byte slots or single floats by the
 *   alignment rule above (of the shard's first row and the relation table;
 *   fixed_rows, s_true and relation_trig need float alignment only); rows too
 *   wide to stage in LDS are read in place.  Queries go on grid.x: one call
 *   takes any nq and ncand whose (query, list chunk) count stays below 2^31.
 *   Each workgroup compacts the owned ids of its chunk of at most 1024 list
 *   places and scores those alone, so a shard's work is its share of the
 *   lists.  The counts are integer sums over the chunks: deterministic, and
 *   independent of the launch geometry (KGE_RANK_CAND_SHARD_CHUNK, diagnostic:
 *   list places per chunk).  Nothing allocates or synchronises; counts is
 *   zeroed by a kernel and every place of it is written.
 * Host checks, in this order: the model (as every entry); the mode (KGE_SINGLE:
 * KGE_ERR_MODE); a NULL descriptor (KGE_ERR_ARG), then its struct_size
 * (KGE_ERR_ABI); then KGE_ERR_ARG for own_begin > own_end or a range outside
 * [0, nentity], flags other than 0, null queries / cand / err_flag /
 * fixed_rows / s_true / counts, nq < 0 or ncand < 1; nq == 0 returns KGE_OK;
 * more (query, chunk) work items than grid.x holds (KGE_ERR_DIM); the workspace
 * (KGE_ERR_WORKSPACE).
 * The workspace holds the queries' q vectors when rows are read in place, and
 * nothing otherwise (a 256-byte minimum) — never an [nq, ncand] object.
 * NOT pinned for this entry: graph capture, and tables past 2 GiB (row offsets
 * are 64-bit, but no test runs it there).
 */
typedef struct kge_rank_cand_shard_desc {
  int32_t struct_size;          /* = sizeof(kge_rank_cand_shard_desc) (else KGE_ERR_ABI) */
  int32_t flags;                /* must be 0 */
  int64_t own_begin, own_end;   /* global ids; own_begin == own_end is a valid empty shard */
  const float *fixed_rows;      /* [nq, entity_dim], reduced output of KGE_RSHARD_ROWS */
  const float *s_true;          /* [nq], reduced output of KGE_RSHARD_TRUE */
  int64_t *counts;              /* [2, nq]: row 0 strictly greater, row 1 equal */
} kge_rank_cand_shard_desc;
size_t kge_rank_candidates_shard_workspace_bytes(const kge_model_desc *m, int64_t nq, int64_t ncand);
int kge_rank_candidates_shard(const kge_model_desc *m, int32_t mode, const kge_rank_cand_shard_desc *sh,
                              const int64_t *queries, int64_t nq, const int64_t *cand, int64_t ncand,
                              void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * SHARDED TOP-K LINK PREDICTION — kge_topk over an entity table that is split
 * into row shards, one per rank, predicted in place: no rank ever holds
 * another's rows.  The conventions are kge_rank_shard's: m->entity_embedding
 * points own_begin rows BEFORE this rank's shard, m->nentity is the GLOBAL
 * count, and only rows [own_begin, own_end) are read.  The order (score
 * descending, id ascending) is total and a pair's score does not depend on the
 * launch geometry, so the merged result equals kge_topk's on the whole table
 * with the same path, ids and score bits.  One entry, two stages, with the
 * host's collectives around them, per block of queries:
 *   1. kge_rank_shard(KGE_RSHARD_ROWS)   → all-reduce(SUM) fixed_rows as int32
 *      (its kernel reads the fixed side only: the predicted column may be -1);
 *   2. KGE_TSHARD_LIST    reads the reduced fixed_rows; list_scores / list_ids
 *      [nq, k] = the k best unexcluded rows of [own_begin, own_end) per query,
 *      sorted by (score descending, id ascending), with GLOBAL ids.  Unused
 *      places — fewer than k candidates in the shard, an empty shard, a bad
 *      query — hold score -inf and id INT32_MAX: the padding loses to every
 *      candidate in the merge, whichever rank it comes from.
 *                          → all-gather both into [world, nq, k], rank-major;
 *   3. KGE_TSHARD_MERGE   reduces the `world` lists of every query in the same
 *      order into ids_out / scores_out [nq, k] as kge_topk writes them: padding
 *      becomes id -1 / score -inf, a bad query id -1 / score NaN.  Badness is
 *      recomputed from `queries`, so it is the same on every rank.
 * LIST builds q from fixed_rows[q] and the relation row with kge_topk's own
 * arithmetic (device cos / sin; the same row bits give the same q bits), the
 * exclusion bitmap over the shard's own rows only (nq × ceil(own_n / 32) words,
 * bit = id - own_begin), and scans the shard with kge_topk's kernels on a
 * shard-local view; the shard's parts are reduced with own_begin added.
 *   queries [nq,3], mode, k: as kge_topk.  A fixed-side id or relation out of
 *   range sets KGE_DEVERR_INDEX; that query's list is all padding, the others
 *   proceed.  The predicted column is never read and never range-checked.
 *   flags: the path's low bits (0 auto, 2 register tile, 3 wave scan), with
 *   kge_topk's eligibility rules applied to the SHARD'S FIRST ROW (its
 *   alignment decides, not the table's), | KGE_RANK_FILTER_TABLE.
 *   filt_off / filt_ids: both forms of kge_topk; both NULL: no filter.  A
 *   filter id inside [0, nentity) but outside the shard is not this shard's: no
 *   bit, no error.  One outside [0, nentity) sets KGE_DEVERR_INDEX.
 *   parts: as kge_topk, cutting THIS shard's rows.
 *   own_begin == own_end is a valid empty shard: all-padding lists, no scan.
 *   fixed_rows needs float alignment only.  Nothing allocates or synchronises;
 *   the bitmap is zeroed by a kernel.  Both stages write every output place.
 * Host checks, in this order: the model (as every entry); the mode (KGE_SINGLE:
 * KGE_ERR_MODE); a NULL descriptor (KGE_ERR_ARG), then its struct_size
 * (KGE_ERR_ABI); then KGE_ERR_ARG for a stage that is neither of the two,
 * own_begin > own_end or a range outside [0, nentity], flags with other bits or
 * a path that is not 0, 2 or 3, parts < 0, null queries / err_flag, a NULL
 * buffer of the stage (LIST: fixed_rows, list_scores, list_ids; MERGE:
 * lists_scores, lists_ids, ids_out, scores_out), filt_off without filt_ids,
 * and nq < 0; nq == 0 returns KGE_OK; then KGE_ERR_DIM for k < 1 or
 * k > KGE_TOPK_MAX_K, nq > 65535 (LIST), world outside 1..64 (MERGE) and rows
 * over 2048 floats per (half-)row; the path's fit (LIST, path 2 for rows the
 * tile cannot take: KGE_ERR_ARG); the workspace (KGE_ERR_WORKSPACE).
 * LIST's workspace holds the q vectors, the shard's bitmap, pRotatE's phase
 * tables over the own rows and the [nq, parts, k] partial lists: it grows with
 * the shard, not with the table.  MERGE needs the 256-byte minimum.
 * NOT pinned for this entry: graph capture, and tables past 2 GiB (row offsets
 * are 64-bit, but no test runs it there).
 */
#define KGE_TSHARD_LIST  1
#define KGE_TSHARD_MERGE 2
typedef struct kge_topk_shard_desc {
  int32_t struct_size;          /* = sizeof(kge_topk_shard_desc) (else KGE_ERR_ABI) */
  int32_t flags;                /* path low bits (0 auto, 2 tile, 3 scan) | KGE_RANK_FILTER_TABLE */
  int32_t k, parts;             /* as kge_topk; parts cuts THIS shard's rows */
  int32_t world, reserved;      /* MERGE: lists to merge, 1..64 */
  int64_t own_begin, own_end;   /* global ids; own_begin == own_end is a valid empty shard */
  const float *fixed_rows;      /* [nq, entity_dim], reduced output of KGE_RSHARD_ROWS */
  const int64_t *filt_off, *filt_ids; /* both forms of kge_topk; both NULL: no filter */
  float *list_scores; int32_t *list_ids;               /* LIST out  [nq, k] */
  const float *lists_scores; const int32_t *lists_ids; /* MERGE in  [world, nq, k], rank-major */
  int64_t *ids_out; float *scores_out;                 /* MERGE out [nq, k] */
} kge_topk_shard_desc;
size_t kge_topk_shard_workspace_bytes(const kge_model_desc *m, const kge_topk_shard_desc *sh, int32_t stage,
                                      int64_t nq);
int kge_topk_shard(const kge_model_desc *m, int32_t mode, const kge_topk_shard_desc *sh, int32_t stage,
                   const int64_t *queries, int64_t nq, void *workspace, size_t workspace_bytes,
                   int32_t *err_flag, void *stream);

/*
 * pRotatE ranks bit-exact to the reference — whose sin (model.py:245) is its
 * CPU vector library's (ATen → MKL VML here), which no device instruction
 * sequence reproduces — in three calls on one stream and workspace:
 *   1. kge_rank_filtered_ex(..., path | KGE_RANK_STAGE_LIST, listed_out): fast
 *      pass, windows widened by the library's ≤ 1 ulp, near-tie lists; then
 *      every listed candidate's score as an interval under ANY sin within one
 *      ulp of the exact value, in the reference's operation order (each later
 *      operation is monotone), and the candidates whose interval clears the
 *      true score's are decided on the device.  listed_out[q] = the candidates
 *      left for the library sin (0: the query is fully ranked; > KGE_RANK_LIST_CAP:
 *      a degenerate window with more undecided candidates than a list, ranked on
 *      the device with correctly rounded sin instead).
 *   2. the caller sets item_off [nq + 1] (device int64, exclusive scan) to
 *      n_items(q) = 1 + listed_out[q] for 1 ≤ listed_out[q] ≤ KGE_RANK_LIST_CAP,
 *      else 0; kge_rank_sin_args writes args_out [item_off[nq], entity_dim]: per
 *      item (0 = the true entity, then the listed candidates) the K phase sums
 *      θh + (θr − θt) (head-batch) or (θh + θr) − θt (tail-batch) the reference
 *      takes the sin of (model.py:236-245; IEEE divisions and adds,
 *      host-independent).
 *   3. the caller evaluates sin_values = sin(args) with the reference's own
 *      library call (torch.sin on the host CPU) and kge_rank_finish_sin
 *      re-scores every item from those values in the reference's order
 *      (abs, ATen sum(dim=2), × modulus, γ −) and writes ranks / ties / listed
 *      as kge_rank_filtered_ex does.
 * Steps 2-3 may be repeated over disjoint subsets of the queries (a query
 * outside the subset gets 0 items) to bound the caller's buffers; ranks are
 * final once every query with items has been delivered once.  A query whose
 * non-empty item range does not hold exactly 1 + listed_out[q] items, a second
 * delivery of a query, or a call whose mode / nq / entity table differ from the
 * list stage's (or after another ranking call used the workspace) sets
 * KGE_DEVERR_ARG.
 */
/*
 * Self-test of the bound the pRotatE list stage's interval screen relies on:
 * writes to max_dist_out (device int32, zeroed by the caller) the largest
 * distance, in representable floats, between the device's sinf and the
 * correctly rounded sin over every float x with |x| <= range (where the double
 * sin lies next to a float midpoint, against both floats it may round to).
 * The screen assumes at most 1 for |x| <= 16 and 2 for |x| <= 65536
 * (kge_rank_ref.h SIN_FAST_*); tests/test_rank_parity_gpu.py checks both on
 * each GPU.
 */
int kge_selftest_sin(float range, int32_t *max_dist_out, void *stream);

int kge_rank_sin_args(const kge_model_desc *m, int32_t mode, int64_t nq, const int64_t *item_off, float *args_out,
                      void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);
int kge_rank_finish_sin(const kge_model_desc *m, int32_t mode, int64_t nq, const int64_t *item_off,
                        const float *sin_values, int64_t *ranks_out, int32_t *ties_out, int32_t *listed_out,
                        void *workspace, size_t workspace_bytes, int32_t *err_flag, void *stream);

/*
 * Live stage timing for benchmarks (no reference counterpart): when enabled,
 * kge_train_step_grads records a hipEvent on its stream before and after each
 * stage of the caller's stream — 0 q build, 1 fused negative scoring +
 * self-adversarial loss (the gather loop), 2 positive score + chain rule,
 * 3 wait for the occurrence CSR (built on an internal side stream in parallel
 * with stages 0-2), 4 entity-major gradient pass (+ fused Adam), 5 wait for the
 * relation pass (side stream, parallel with 4) + loss finalisation.
 *   command 1: enable and reset, timing one call in every n_out (n_out <= 0:
 *              every call) — sampling keeps the event records' own cost
 *              (~4 % of a step when every call is timed) out of the throughput;
 *   command 0: disable and reset;
 *   command 2: synchronise the recorded events and write the summed
 *              milliseconds per stage to stage_ms_out[0..5] and the number of
 *              timed calls to stage_ms_out[6] (n_out >= 7);
 *   command 3: the same per timed call: stage_ms_out[7c .. 7c+5] the call's
 *              stage times, stage_ms_out[7c+6] its start (ms after the first
 *              timed call's start); n_out >= 7 × timed calls.
 *   command 4: enable and reset the RANKING timer: every kge_rank_filtered* call
 *              (and pRotatE's three-call form, list → finish) records events
 *              at its start, around its fast counting pass and after its ranks
 *              are written (every finish call of the three-call form marks
 *              "ranks written"; the last one before the next call counts)
 *              (command 0 disables it too);
 *   command 5: synchronise them and write the summed milliseconds of its
 *              KGE_RANK_TIMER_STAGES stages — 0 query / filter / table
 *              preparation and windows, 1 the fast counting pass (MFMA tile,
 *              register tile or wave scan), 2 near-tie refinement and rank
 *              emission (pRotatE's three-call form: including the caller's
 *              host sin between the calls) — then the number of DIRECTIONS
 *              ranked (a kge_rank_filtered_both call counts 2) (n_out >= 4).
 * Not graph-capturable while enabled.
 */
#define KGE_TIMER_STAGES 6
#define KGE_RANK_TIMER_STAGES 3
int kge_stage_timer(int32_t command, float *stage_ms_out, int32_t n_out);

/*
 * Device negative sampler: one training batch as TrainDataset.__getitem__ +
 * collate_fn build it (dataloader.py:34-66, sampling loop :44-61), for the
 * triples `batch[0..batch_size)` (ids into `triples`).
 *   pos_out[i] = triples[batch[i]], w_out[i] = weights[batch[i]]
 *     (weights = sqrt(1 / (count(h,r) + count(t,-r-1))), dataloader.py:40-42)
 *   neg_out[i, :] = the first negative_sample_size draws of row i's uniform
 *     stream over [0, nentity) that are NOT in the row's true list — the true
 *     heads of (r, t) for head-batch, the true tails of (h, r) for tail-batch
 *     (dataloader.py:47-56): true_ids[true_off[t] .. + true_len[t]), sorted.
 * Row i's stream is a splitmix64 sequence keyed by (key, i); the caller
 * advances `key` every batch.  The reference draws with numpy's global
 * MT19937, so parity is distributional and bit-exact against
 * the restatement of this generator in oracle/kge_oracle.py.
 * A row still short after max_draws draws sets KGE_DEVERR_SAMPLER (the
 * reference would loop forever) and is zero-padded.
 */
int kge_sample_negatives(const int64_t *triples, int64_t ntriples, const int64_t *batch, int64_t batch_size,
                         int64_t nentity, int64_t negative_sample_size, const int64_t *true_off,
                         const int32_t *true_len, const int64_t *true_ids, const float *weights, uint64_t key,
                         int64_t max_draws, int64_t *pos_out, int64_t *neg_out, float *w_out, int32_t *err_flag,
                         void *stream);

#ifdef __cplusplus
}
#endif

#endif /* KGE_HIP_H */
