/* dr4sr_hip.h — C ABI of the MI355X (gfx950) hot path for DR4SR's target-model training loop.
 *
 * The reference (USTC-StarTeam/DR4SR) has no FFI of its own: the path is pure PyTorch.  The
 * boundary a maintainer would bind is therefore "what the reference asks torch to do" on
 *   model/basemodel.py:177-214  (training_epoch / training_step: neg-sampling, encoder forward,
 *                                tied-embedding scorer, BCE, backward, Adam)
 *   model/sasrec.py:39-75       (SASRecQueryEncoder.forward; its batch['input_weight'] scale: dr4sr_sasrec_inputs,
 *                                dr4sr_sasrec_encode_w / _encode_w_bwd — seq_emb is not bound)
 *   model/loss_func.py:9-38     (BinaryCrossEntropyLoss)
 *   model/basemodel.py:354-365  (topk: full-item scorer)
 * Every entry point below names the reference lines it replaces.  INTEGRATION.md shows the
 * ctypes stub that binds them from the reference's Python.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless said otherwise
 *   - fp32 activations/parameters, int64 ids (as the reference stores them), row-major, contiguous
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no host sync,
 *     no allocation) so calls may be captured into a hipGraph
 *   - return value: 0 = ok, negative = argument error (DR4SR_E_*; transport: DR4SR_E_RCCL_BASE - ncclResult_t), positive = hipError_t
 *   - nothing is retained across calls except what the caller passes in (plan + workspace)
 */
#ifndef DR4SR_HIP_H
#define DR4SR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR4SR_ABI_VERSION 10

#define DR4SR_E_ARG      (-1)   /* null pointer / bad size                                   */
#define DR4SR_E_SHAPE    (-2)   /* unsupported D / H / F / L combination     */
#define DR4SR_E_WS       (-3)   /* workspace too small                                       */
#define DR4SR_E_RCCL_BASE (-100) /* transport (ABI 8): an RCCL error r is returned as DR4SR_E_RCCL_BASE - r (ncclResult_t, r >= 1) */

/* dropout sites (RNG stream ids); per-layer sites are  kind + 4*layer */
#define DR4SR_SITE_EMB   0      /* sasrec.py:66   dropout(seq_embs + position_embs)          */
#define DR4SR_SITE_ATTN  1      /* torch MHA      dropout on attention probabilities         */
#define DR4SR_SITE_PROJ  2      /* torch TEL      dropout1 after out_proj                    */
#define DR4SR_SITE_ACT   3      /* torch TEL      dropout after the activation               */
#define DR4SR_SITE_FFN   4      /* torch TEL      dropout2 after linear2                     */

/* plan->optimizer (ABI 6): basemodel.py:79-98's `optimizer` choices, each with torch's defaults as the reference constructs them */
#define DR4SR_OPT_ADAM    0     /* torch.optim.Adam(lr, weight_decay); also what an unknown name falls back to (weight_decay 0)   */
#define DR4SR_OPT_SGD     1     /* torch.optim.SGD(lr, weight_decay): no momentum                                                */
#define DR4SR_OPT_ADAGRAD 2     /* torch.optim.Adagrad(lr, weight_decay): adam_v = state_sum, adam_eps = 1e-10                    */
#define DR4SR_OPT_RMSPROP 3     /* torch.optim.RMSprop(lr, weight_decay): adam_v = square_avg, beta2 = alpha 0.99, adam_eps 1e-8  */

#define DR4SR_POOL_NONE   0
#define DR4SR_POOL_ORIGIN 1     /* module/layers.py:41-50  zero rows >= seqlen  -> [B,L,D]   */
#define DR4SR_POOL_LAST   2     /* module/layers.py:69-73  row seqlen-1         -> [B,D]     */
#define DR4SR_POOL_MEAN   3     /* module/functional.py:50-55  mean of rows < seqlen -> [B,D] (CL4SRec views)   */

/* slots of the int32 `state` buffer (device), DR4SR_STATE_WORDS words, owned by the caller */
#define DR4SR_STATE_STEP     0  /* optimizer step counter t (incremented by dr4sr_adam_step) */
#define DR4SR_STATE_T        1  /* number of packed (valid) tokens of the current batch      */
#define DR4SR_STATE_NVALID   2  /* number of loss positions (target != 0)                    */
#define DR4SR_STATE_RNGSTEP  3  /* RNG step (incremented by every fwd_bwd)                   */
#define DR4SR_STATE_WORDS    16

/* Flat parameter layout (fp32), identical for params / grads / adam_m / adam_v:
 *   E[N,D] | P[L,D] | per layer: in_w[3D,D] in_b[3D] out_w[D,D] out_b[D] w1[F,D] b1[F] w2[D,F] b2[D]
 *                                 ln1_w[D] ln1_b[D] ln2_w[D] ln2_b[D]
 * (names: item_embedding.weight, query_encoder.position_emb.weight,
 *  query_encoder.transformer_layer.layers.{i}.{self_attn.in_proj_weight, ...} — SURVEY.md §8a)
 * The grads buffer has DR4SR_GRAD_TAIL extra floats after n_params:
 *   grads[n_params+0] = number of loss positions (as float), grads[n_params+1] = loss SUM,
 *   grads[n_params+2] = poison word (non-zero: a producer of this gradient failed on the device; the optimizer skips the step).
 * Gradients are accumulated UN-normalised (d loss_sum); dr4sr_adam_step divides by
 * grads[n_params+0], so that under data parallelism ONE sum-all-reduce of the whole buffer yields
 * the reference's global-batch normalisation (loss_func.py:18-19, :29-30). */
#define DR4SR_GRAD_TAIL 4

typedef struct dr4sr_sasrec_plan {
    int32_t abi_version;            /* must be DR4SR_ABI_VERSION                                */
    /* ---- model dims (configs/basemodel.yaml, configs/sasrec.yaml) ---- */
    int32_t B, L, D, H, F, n_layer, n_items;
    float   ln_eps;                 /* layer_norm_eps                                            */
    float   p_drop;                 /* dropout_rate (0 => no RNG work at all)                    */
    uint64_t seed;                  /* Philox key                                                */
    /* ---- parameters ---- */
    float*  params;                 /* [n_params]                                                */
    float*  grads;                  /* [n_params + DR4SR_GRAD_TAIL]                              */
    float*  adam_m;                 /* [n_params]                                                */
    float*  adam_v;                 /* [n_params]                                                */
    int64_t n_params;
    /* ---- batch: rows `rows[0..B)` of device-resident dataset tensors (data/dataset.py:79-91).
     *      rows == NULL means rows 0..B-1, i.e. the three pointers ARE the batch tensors. ---- */
    const int64_t* in_item_id;      /* [U,L]  batch['in_item_id']                                */
    const int64_t* item_id;         /* [U,L]  batch['item_id'] (targets), may be NULL for encode */
    const int64_t* seqlen;          /* [U]    batch['seqlen']                                    */
    const int64_t* rows;            /* [B] or NULL                                               */
    int64_t* neg_item;              /* [B,L]  batch['neg_item'] (K = 1)                          */
    int32_t  sample_neg;            /* 1: draw negatives in-kernel (basemodel.py:50-61) and WRITE
                                          them to neg_item; 0: READ neg_item                     */
    /* ---- scratch ---- */
    void*    workspace;             /* >= dr4sr_sasrec_workspace_bytes(plan) bytes               */
    int64_t  workspace_bytes;
    int32_t* state;                 /* [DR4SR_STATE_WORDS] device words, zero-initialised once   */
    /* ---- optimizer (basemodel.py:79-98: torch.optim.Adam) ---- */
    float lr, beta1, beta2, adam_eps, weight_decay;
    /* ---- a1 fused batch selection (optional; replaces a separate dr4sr_select_rows launch): when perm != NULL the first
     *      kernel of dr4sr_sasrec_fwd_bwd/_train_step/_encode(training) FILLS rows[i] = perm[(c*perm_stride + perm_offset + i)
     *      mod n_perm], i < B, with c = *perm_counter, then sets *perm_counter = c + 1.  `rows` must then be writable. ---- */
    const int64_t* perm;            /* [n_perm] one epoch's permutation of dataset rows, or NULL  */
    int64_t  n_perm;
    int64_t  perm_stride;           /* global batch size                                          */
    int64_t  perm_offset;           /* this rank's offset inside the global batch                 */
    int32_t* perm_counter;          /* device int32: batch index within the epoch                 */
    /* ---- optional per-step loss log: dr4sr_adam_step / _train_step write loss_log[slot] = loss_sum / n_valid of the step with
     *      slot = *perm_counter - 1 when perm != NULL (the batch index just consumed), else slot = 0.  NULL = off. ---- */
    float*   loss_log;
    /* ---- regime hint (ABI 4): the host's estimate of the VALID tokens of a batch of B rows (B * mean(min(seqlen, L)) of the
     *      dataset).  The launchers pick their forms from it — token-tile kernels: 16-row tiles + atomics for the table gradient up to
     *      ~7 k packed tokens, 32-row tiles + scatter / owner jobs above; attention: one workgroup per sequence up to ~14 k tokens,
     *      length-class lists above — because the real count lives on the device.  0 = unknown: the capacity B * L decides (boundary
     *      16 384 for both), as before ABI 4.  (Boundaries quoted for d = 64; they scale with 64 / d.)  A wrong hint costs speed, never
     *      correctness. ---- */
    int32_t  expected_tokens;
    int32_t  optimizer;             /* DR4SR_OPT_* (ABI 6; 0 = Adam)                                                              */
} dr4sr_sasrec_plan;

/* -------------------------------------------------------------------------------------------- */
int  dr4sr_abi_version(void);
int  dr4sr_sasrec_plan_sizeof(void);   /* sizeof(dr4sr_sasrec_plan) as compiled: lets a binding verify its struct mirror */
/* Fills offsets[0]=E, [1]=P, [2+12*i+j] = j-th tensor of layer i (order above); returns n_params. */
int64_t dr4sr_sasrec_param_layout(int32_t n_items, int32_t L, int32_t D, int32_t F, int32_t n_layer,
                                  int64_t* offsets /* [2+12*n_layer] or NULL */);
/* Bytes of scratch a plan of this shape needs (plan->workspace may be NULL here), or a negative DR4SR_E_* code: DR4SR_E_SHAPE for an
 * encoder shape without kernels — L > 64; (D, F) outside {(64,128), (64,256), (128,128)}; head_dim other than 32 / 64; a head count != 2
 * whose one-wave-per-head attention would not fit 160 KB of LDS — so an unsupported configuration is refused when the engine is built. */
int64_t dr4sr_sasrec_workspace_bytes(const dr4sr_sasrec_plan* plan);
/* Byte offsets, from plan->workspace, of buffers of `layer` inside that scratch (plan->workspace itself may be NULL): the layout depends
 * on the plan's B and on the switches in force (deterministic mode), so whoever prefills or reads a buffer back — the tests — asks for it.
 * out[DR4SR_WS_OFF_COUNT]: attn_keep [T][H][2] words | u1 [T][D] | st1 [T][2] | a [T][F] | u2 [T][D] | st2 [T][2] floats |
 * row_keep [T][16] half-words | Adam's bias-correction record (2 slots x 8 words, not per layer), with T = B * L. */
#define DR4SR_WS_OFF_ATTN_KEEP 0
#define DR4SR_WS_OFF_U1        1
#define DR4SR_WS_OFF_ST1       2
#define DR4SR_WS_OFF_A         3
#define DR4SR_WS_OFF_U2        4
#define DR4SR_WS_OFF_ST2       5
#define DR4SR_WS_OFF_ROW_KEEP  6
#define DR4SR_WS_OFF_BC_REC    7
#define DR4SR_WS_OFF_COUNT     8
int dr4sr_sasrec_workspace_offsets(const dr4sr_sasrec_plan* plan, int32_t layer, int64_t* out);
/* launch forms a step of this plan takes (see expected_tokens): bit 0 = at-scale token-tile kernels (32-row tiles, scatter / owner jobs),
 * bit 1 = the at-scale attention regime of short-sequence plans (length-class lists, or — bit 4 — the wave-per-tile launches that
 * replace them: csrc/attn_wave.hip), bit 2 = the attention runs inside the 16-token tile launches (the latency forms: no attention
 * launches; csrc/attn_tile.h), bit 3 = the opt-in window launches (csrc/attn_tile_sa.hip), bit 5 = bit 4 with the forward folded into the
 * wave-tile forward launches (bits 3 and 5: experiments build only, both measured slower), bit 6 = the deterministic latency form
 * (DR4SR_DETERMINISTIC on a plan of the latency regime: the latency launches of bit 2 with the attention's shared dK | dV rows, the table
 * gradient and the weight-gradient splits summed in a fixed order); < 0: DR4SR_E_* */
int dr4sr_sasrec_at_scale(const dr4sr_sasrec_plan* plan);

/* Deterministic mode (the reference's run-to-run determinism request, utils/utils.py:13-20).  Environment switch DR4SR_DETERMINISTIC=1, read
 * when a plan's workspace is carved (like every switch: cached per call site until the hooks header's reload entry point is called): every reduction of the training
 * steps dr4sr_sasrec_fwd_bwd[_weighted / _phase] / _train_step[s], dr4sr_fmlp_fwd_bwd / _train_step, dr4sr_gru4rec_fwd_bwd / _train_step[s] and
 * of the autograd-path backwards (dr4sr_*_encode_bwd) and of the dense scorer backward (dr4sr_score_bce_bwd / _bpr_bwd) runs in a fixed order — no fp32 atomics — so two runs from one state are bit-identical.
 * The mode needs partial-sum buffers: the *_workspace_bytes entry points answer for the mode that is set when it is called, and a workspace sized without
 * the mode is refused with DR4SR_E_WS once the mode is on.  It is combined with neither DR4SR_WGRAD_F32 (DR4SR_E_SHAPE) nor, for ordered
 * results, DR4SR_DE_ATOMIC. */

/* One reference training step minus the optimizer:  basemodel.py:193-198
 *   (_neg_sampling) -> training_step (sasrec.py:39-75 encoder, basemodel.py:204-214 scorer,
 *   loss_func.py:9-38 BCE) -> loss.backward().
 * Leaves un-normalised gradients + {n_valid, loss_sum} in plan->grads (zeroed first). */
int dr4sr_sasrec_fwd_bwd(const dr4sr_sasrec_plan* plan, void* stream);

/* optimizer.step() (basemodel.py:199) on the flat buffers: dense torch.optim.Adam semantics,
 * g = grads[i] / grads[n_params] (+ weight_decay * p).  Increments state[STEP]. */
int dr4sr_adam_step(const dr4sr_sasrec_plan* plan, void* stream);

/* fwd_bwd + adam in one call (single-GPU fast path). */
int dr4sr_sasrec_train_step(const dr4sr_sasrec_plan* plan, void* stream);

/* n_steps iterations of the loop body of BaseModel.training_epoch (basemodel.py:193-199) in one call: with plan->perm set,
 * consecutive batches of the epoch permutation (perm_counter advances n_steps times), each with fresh dropout masks and
 * negatives.  Same results as n_steps calls of dr4sr_sasrec_train_step; the optimizer launch of every step but the last
 * also prepares the step that follows (batch selection, sequence offsets, zeroed gradients), so the call enqueues one prep
 * kernel instead of n_steps.  After the call plan->grads holds the last step's gradients. */
int dr4sr_sasrec_train_steps(const dr4sr_sasrec_plan* plan, int32_t n_steps, void* stream);

/* The same fusion for a data-parallel loop, where the all-reduce of plan->grads sits between the two halves of a step:
 *   dr4sr_sasrec_fwd_bwd(plan)                                    first step (runs its own prep)
 *   all-reduce ; dr4sr_adam_step_prepare_next(plan)               optimizer + prep of the next batch (selection, offsets, zeroed grads)
 *   dr4sr_sasrec_fwd_bwd_prepared(plan) ; all-reduce ; dr4sr_adam_step_prepare_next(plan) ; ...
 * Finish with dr4sr_adam_step to leave no batch prepared (harmless if not: the next dr4sr_sasrec_fwd_bwd prepares again, but a
 * plan->perm counter has then advanced once more). */
int dr4sr_sasrec_fwd_bwd_prepared(const dr4sr_sasrec_plan* plan, void* stream);
int dr4sr_adam_step_prepare_next(const dr4sr_sasrec_plan* plan, void* stream);

/* ABI 7 — the data-parallel step with the gradient in TWO buckets that become final at different times ("optionally
 * 2 buckets ... overlapped with backward"; the reference has no distributed path, /root/reference/utils/callbacks.py:130 is its TODO).
 *   dr4sr_sasrec_grad_buckets(plan, bounds)  -> number of buckets a step of this plan produces, 1 or 2; bounds[0..2] (floats into
 *       plan->grads): bucket 0 = [bounds[0], bounds[1]), bucket 1 = [bounds[1], bounds[2]).  Two buckets exist where the item-table
 *       gradient is a set of jobs of the last backward launch (the at-scale launch forms, dr4sr_sasrec_at_scale bit 0): bucket 0 = the
 *       item table E and the position table P, [0, offsets[2]) — 92 % of a toys-sized replica's bytes; bucket 1 = the encoder layers and
 *       the {n_valid, loss_sum, poison, -} tail.  One bucket otherwise (latency forms: every producer is one launch), bounds[1] = bounds[2].
 *   dr4sr_sasrec_fwd_bwd_phase(plan, prepared, 1, stream)   everything up to and including the launch that makes bucket 0 final
 *       (prepared = 0: runs its own prep like dr4sr_sasrec_fwd_bwd; != 0: on a batch prepared by dr4sr_adam_step_prepare_next);
 *   dr4sr_sasrec_fwd_bwd_phase(plan, prepared, 2, stream)   the remaining weight-gradient launch (nothing when there is one bucket).
 * Caller:  phase 1 ; all-reduce(bucket 0) on a side stream ; phase 2 ; all-reduce(bucket 1) ; join ; dr4sr_adam_step[_prepare_next].
 * Phase 1 + phase 2 leave exactly what dr4sr_sasrec_fwd_bwd[_prepared] leaves (same kernels, same jobs, cut into two launches). */
int dr4sr_sasrec_grad_buckets(const dr4sr_sasrec_plan* plan, int64_t* bounds /* [3] or NULL */);
int dr4sr_sasrec_fwd_bwd_phase(const dr4sr_sasrec_plan* plan, int32_t prepared, int32_t phase, void* stream);

/* ABI 8 — the data-parallel TRANSPORT: RCCL collectives enqueued on the caller's HIP stream (csrc/comm.hip; library links librccl).
 * SURVEY.md section 8(b) names `allreduce_flat(buf)` (RCCL) among the native entry points and 8(e) `ncclAllReduce(sum, fp32)` over the
 * flat gradient buffer {E | P | encoder layers | n_valid, loss_sum, poison, -}; the reference has no distributed path
 * (/root/reference/utils/callbacks.py:130 is its TODO), so these replace no reference line — they are what a maintainer adding DP to
 * model/basemodel.py:193-199 (between `loss.backward()` and `optimizer.step()`) would call.  One communicator per process and GPU:
 *   rank 0:      dr4sr_comm_unique_id(id)        (HOST buffer of DR4SR_COMM_ID_BYTES) ; carry `id` to every rank by any host means
 *   every rank:  dr4sr_comm_init_rank(id, rank, world, device, &comm)                   (collective; hipSetDevice(device) inside)
 *   per step:    dr4sr_sasrec_fwd_bwd(plan, s) ; dr4sr_allreduce_f32(comm, plan->grads, plan->n_params + 4, s) ; dr4sr_adam_step(plan, s)
 * A collective is an enqueue on `stream`, ordered like a kernel launch: no host thread, no host sync, capturable into a hipGraph with the
 * kernels around it.  Two-bucket step (dr4sr_sasrec_fwd_bwd_phase): dr4sr_allreduce_f32_async puts the collective on the communicator's
 * own side stream BEHIND everything already enqueued on `stream`, which does not wait for it — phase 2's launch runs beside the table
 * bucket's all-reduce (inside a capture: a parallel branch of the graph); dr4sr_comm_join(comm, stream) makes `stream` wait for every
 * collective started that way.  Every rank must enter the same collectives in the same order with the same sizes.
 * Errors: DR4SR_E_ARG, a hipError_t (> 0), or DR4SR_E_RCCL_BASE - ncclResult_t; dr4sr_comm_error_string(rc) names any of them.
 * dr4sr_comm_destroy synchronises the side stream and frees the communicator (collective with RCCL: call on every rank). */
#define DR4SR_COMM_ID_BYTES 128
#define DR4SR_RED_SUM 0
#define DR4SR_RED_MAX 1
#define DR4SR_RED_MIN 2
typedef struct dr4sr_comm dr4sr_comm;
int dr4sr_comm_unique_id(void* id_out /* host, DR4SR_COMM_ID_BYTES */);
int dr4sr_comm_init_rank(const void* id /* host */, int32_t rank, int32_t world, int32_t device, dr4sr_comm** out);
int dr4sr_comm_destroy(dr4sr_comm* comm);
int dr4sr_comm_rank(const dr4sr_comm* comm);
int dr4sr_comm_world(const dr4sr_comm* comm);
int dr4sr_comm_async_error(dr4sr_comm* comm);                 /* 0, or the communicator's asynchronous RCCL error as a return code */
const char* dr4sr_comm_error_string(int rc);
int dr4sr_allreduce_f32(dr4sr_comm* comm, float* buf, int64_t n, void* stream);            /* in place, sum */
int dr4sr_allreduce_f64(dr4sr_comm* comm, double* buf, int64_t n, int32_t op /* DR4SR_RED_* */, void* stream);
int dr4sr_allreduce_f32_async(dr4sr_comm* comm, float* buf, int64_t n, void* stream);      /* on the side stream, after `stream`'s work so far */
int dr4sr_comm_join(dr4sr_comm* comm, void* stream);                                       /* `stream` waits for the async collectives */
int dr4sr_allgather_bytes(dr4sr_comm* comm, const void* send, void* recv /* world * bytes */, int64_t bytes, void* stream);
int dr4sr_broadcast_bytes(dr4sr_comm* comm, void* buf, int64_t bytes, int32_t root, void* stream);

/* SASRecQueryEncoder.forward + SeqPoolingLayer (sasrec.py:39-75, layers.py:41-50/:69-73).
 * training != 0 applies dropout (RNG step = state[RNGSTEP]) and keeps activations in the
 * workspace for dr4sr_sasrec_encode_bwd.  out: [B,L,D] (NONE/ORIGIN; NONE leaves rows >= seqlen
 * ZERO as well — they are never computed) or [B,D] (LAST, MEAN). */
int dr4sr_sasrec_encode(const dr4sr_sasrec_plan* plan, int32_t training, int32_t pooling,
                        float* out, void* stream);
/* autograd of the above (same `training` / `pooling` as the forward call it differentiates, no
 * other encode call in between): d_out has the shape of `out`; parameter gradients are ACCUMULATED
 * into plan->grads (exactly d_out-weighted, no normalisation). */
int dr4sr_sasrec_encode_bwd(const dr4sr_sasrec_plan* plan, int32_t training, int32_t pooling,
                            const float* d_out, void* stream);

/* The encoder's optional inputs (sasrec.py:61-64: `batch['input_weight'] * (seq_embs + position_embs)` when the batch carries a weight).
 * Additive to ABI 10: the plan struct is untouched.
 *   input_weight: one scale per position, x = dropout(input_weight[b,pos] * (E[id] + P[pos])) — the scale sits BEFORE the embedding-stage
 *     dropout, as in the reference; everything behind the encoder's input is unchanged.  Indexed by the BATCH SLOT b of the plan, not
 *     through plan->rows (it belongs to the batch, not to the dataset).  Values at pos >= seqlen[b] are never read.
 *   d_input_weight (backward only): d_input_weight[b,pos] = sum_c g[b,pos,c] * (E[id] + P[pos])[c] with g the gradient that reaches the
 *     dropout's input.  WRITTEN, not accumulated (a second backward on one forward stores the same values), for pos < seqlen[b] only:
 *     the caller zero-fills the buffer, the reference's gradient is 0 at the other positions for every pooling of this library.
 *     The item / position table gradients pick the factor input_weight[b,pos] up.
 * in == NULL or in->input_weight == NULL is dr4sr_sasrec_encode / _encode_bwd: the same launches, the same bits (those two ARE these calls
 * with in = NULL).  d_input_weight without input_weight: DR4SR_E_ARG.  The backward takes the input_weight of the forward it differentiates.
 * The fused training steps (dr4sr_sasrec_fwd_bwd, _train_step(s), _weighted) take their rows from dataset tensors and stay unweighted;
 * seq_emb (an encoder input without item ids) is not on this path. */
typedef struct dr4sr_sasrec_inputs {
    const float* input_weight;    /* [B,L] fp32 by BATCH SLOT b (not through plan->rows), or NULL */
    float*       d_input_weight;  /* [B,L] or NULL; backward only; written, zero-filled by the caller */
} dr4sr_sasrec_inputs;
int dr4sr_sasrec_encode_w(const dr4sr_sasrec_plan* plan, const dr4sr_sasrec_inputs* in, int32_t training, int32_t pooling,
                          float* out, void* stream);
int dr4sr_sasrec_encode_w_bwd(const dr4sr_sasrec_plan* plan, const dr4sr_sasrec_inputs* in, int32_t training, int32_t pooling,
                              const float* d_out, void* stream);

/* a1: device-side batch selection replacing DataLoader(shuffle=True) + per-sample __getitem__ +
 * default_collate (data/dataset.py:105-108, :149-164).  rows_out[i] = perm[(c*stride + offset + i)
 * mod n_perm] for i < B where c = *counter (device int32), then *counter = c + 1.  With
 * stride = global batch and offset = rank*B every rank walks its own slice of one permutation. */
int dr4sr_select_rows(const int64_t* perm, int64_t n_perm, int64_t* rows_out, int32_t B,
                      int64_t stride, int64_t offset, int32_t* counter, void* stream);

/* K1: item_encoder(idx) + position_emb(arange(L))  (sasrec.py:43-46, :64) for ALL B*L positions,
 * bit-exact with torch (gather + one IEEE add).  out [B,L,D]. */
int dr4sr_embed_gather_posadd(const float* E, const float* P, const int64_t* idx, float* out,
                              int64_t B, int32_t L, int32_t D, int32_t n_items, void* stream);

/* K4: tied-embedding scorer + BCE on a DENSE query (basemodel.py:204-214, loss_func.py:9-38).
 * query [B,L,D]; target, neg [B,L] int64.  Outputs (any may be NULL): pos/neg score [B,L] (pos is
 * -inf where target==0), loss_pos [B,L] = per-position (-logsigmoid(pos)+softplus(neg)) or 0 at
 * pads (UN-normalised), stats[0] = n_valid, stats[1] = loss sum (floats, accumulated: zero them). */
int dr4sr_score_bce_fwd(const float* query, const float* E, const int64_t* target,
                        const int64_t* neg, float* pos_score, float* neg_score, float* loss_pos,
                        float* stats, int64_t B, int32_t L, int32_t D, void* stream);
/* backward of the above with per-position upstream weight w[B,L] (NULL => 1) times *scale
 * (device float, NULL => 1):  d_query [B,L,D] written, dE [N,D] accumulated (atomics). */
int dr4sr_score_bce_bwd(const float* query, const float* E, const int64_t* target,
                        const int64_t* neg, const float* w, const float* scale, float* d_query,
                        float* dE, int64_t B, int32_t L, int32_t D, void* stream);

/* a8: the same two entry points for BPRLoss (loss_func.py:40-48; selected by loss_fn: 'bpr', basemodel.py:103-104): per position
 * -logsigmoid(pos - neg) (K = 1: softmax(ones) = 1), same masks, same outputs, same normalisation contract (stats / upstream w). */
int dr4sr_score_bpr_fwd(const float* query, const float* E, const int64_t* target,
                        const int64_t* neg, float* pos_score, float* neg_score, float* loss_pos,
                        float* stats, int64_t B, int32_t L, int32_t D, void* stream);
int dr4sr_score_bpr_bwd(const float* query, const float* E, const int64_t* target,
                        const int64_t* neg, const float* w, const float* scale, float* d_query,
                        float* dE, int64_t B, int32_t L, int32_t D, void* stream);
/* The loss modules called on SCORE tensors (model/loss_func.py used outside training_step): pos [n] (-inf marks a padded position),
 * neg [n,K].  kind 0: BinaryCrossEntropyLoss.forward masked branch (:12-31) -logsigmoid(pos) + sum_k softplus(neg_k)/K;
 * kind 1: BPRLoss.forward (:44-49) -sum_k logsigmoid(pos - neg_k)/K.  loss_pos [n] per position UN-normalised (0 at padded
 * positions, NULL ok); stats[0] += #valid, stats[1] += loss sum.  Backward: upstream g[n] (NULL = 1) times *scale (NULL = 1). */
int dr4sr_loss_from_scores_fwd(const float* pos, const float* neg, int64_t n, int32_t K, int32_t kind, float* loss_pos,
                               float* stats, void* stream);
int dr4sr_loss_from_scores_bwd(const float* pos, const float* neg, int64_t n, int32_t K, int32_t kind, const float* g,
                               const float* scale, float* d_pos, float* d_neg, void* stream);

/* K0: _neg_sampling (basemodel.py:50-61): uniform on 1..n_items-1 with replacement, never PAD.
 * out [n] int64.  Stream (seed, step) is the one dr4sr_sasrec_fwd_bwd uses for sample_neg=1. */
int dr4sr_neg_sample(int64_t* out, int64_t n, int32_t n_items, uint64_t seed, uint32_t step,
                     void* stream);
/* the same with the step read from a device word at run time (graph replays) */
int dr4sr_neg_sample_dev(int64_t* out, int64_t n, int32_t n_items, uint64_t seed, const int32_t* step_dev, void* stream);

/* BaseModel.topk (basemodel.py:354-365) for the single-domain case: scores = q @ E[:n_items]^T,
 * column 0 (PAD) and every id in hist[b,:] set to -inf, top-k (k <= 128) by score, ties -> lower id.
 * q [B,D], hist [B,Lh] int64, out_score [B,k] fp32, out_item [B,k] int64. */
/* *bad_count += number of ids outside [0, n_items) among idx[0..n) (device int32, zeroed by the caller).  The gather kernels CLAMP
 * such ids (a launch cannot raise); torch's nn.Embedding — the reference's gather, model/sasrec.py:43 — raises "index out of range in
 * self": a caller that wants that behaviour checks its id tensors with this (dr4sr_amd: once per dataset tensor, and per call of the
 * dense dispatcher op). */
int dr4sr_check_ids(const int64_t* idx, int64_t n, int32_t n_items, int32_t* bad_count, void* stream);

int dr4sr_full_score_topk(const float* q, const float* E, const int64_t* hist, float* out_score,
                          int64_t* out_item, int64_t B, int32_t D, int32_t n_items, int32_t Lh,
                          int32_t k, void* stream);
/* the same through a [B, round_up(n_items, 64)] fp32 score workspace (dr4sr_full_score_topk_workspace_bytes): the scores come from
 * one MFMA GEMM instead of B passes over the table and the top-k from a radix select — identical results, ~15x faster at the
 * reference's eval shape (2048 x 11925, k = 100); no limit on n_items (rows that do not fit LDS are selected from the workspace, whose
 * history columns are then overwritten with -inf). */
int64_t dr4sr_full_score_topk_workspace_bytes(int64_t B, int32_t n_items);
int dr4sr_full_score_topk_ws(const float* q, const float* E, const int64_t* hist, float* out_score, int64_t* out_item, int64_t B,
                             int32_t D, int32_t n_items, int32_t Lh, int32_t k, float* workspace, int64_t workspace_bytes,
                             void* stream);

/* the multi-domain form of basemodel.py:354-365: item_blocked [n_items] bytes, 1 = the item is NOT in domain_item_mapping[eval_domain]
 * (its score becomes -inf exactly like the reference's domain_mask, :358-360); NULL = single domain (only PAD is blocked). */
int dr4sr_full_score_topk_masked_ws(const float* q, const float* E, const int64_t* hist, const uint8_t* item_blocked,
                                    float* out_score, int64_t* out_item, int64_t B, int32_t D, int32_t n_items, int32_t Lh,
                                    int32_t k, float* workspace, int64_t workspace_bytes, void* stream);

/* ---- additive to ABI 10: evaluation by TARGET RANK (csrc/rank.hip).  With one target per row every rank metric at every cutoff is a
 * function of one integer: rank_out[b] = the number of VALID items that precede target[b] in the order (score descending, id
 * ascending), counted from 0.  Validity is dr4sr_full_score_topk_masked_ws's, word for word: 1 <= j < n_items, item_blocked[j] == 0
 * (NULL: nothing blocked), j not among the row's Lh history words (a word counts only if, as an int64, it lies in [0, n_items);
 * duplicates count once; hist may be NULL with Lh = 0).  A target that is itself not valid (PAD, out of range, blocked, in the row's own
 * history) gives DR4SR_RANK_NONE.  The scores, the target's included, come from the MFMA loop of the top-k's score GEMM, so for any
 * finite q / E "rank < k" holds exactly when the top-k call returns the target at position rank.  q [B, D], E [n_items, D], D = 64 or
 * 128 (else DR4SR_E_SHAPE); B < 0, n_items < 2, Lh < 0 or a null pointer: DR4SR_E_ARG; a null or too small workspace
 * (dr4sr_target_rank_workspace_bytes): DR4SR_E_WS; B = 0 is a no-op.  Two launches on the caller's stream, no host synchronisation, no
 * allocation, capturable; integer atomics only: two calls on the same inputs are bitwise equal. */
#define DR4SR_RANK_NONE 2147483647   /* INT32_MAX */
int64_t dr4sr_target_rank_workspace_bytes(int64_t B);
int dr4sr_target_rank(const float* q, const float* E, const int64_t* target, const int64_t* hist, const uint8_t* item_blocked,
                      int32_t* rank_out, int64_t B, int32_t D, int32_t n_items, int32_t Lh, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* One launch of one workgroup ADDS a batch to acc (device, fp64, [1 + 7 * n_cut], zeroed by the caller once per epoch): acc[0] += B, and
 * per cutoff c (cutoffs: HOST array, n_cut in [1, 8], passed by value) the sums over the rows of ndcg, recall, precision, map, mrr, hit,
 * f1 in that order — the reference's evaluation/__init__.py formulas for one target per row in IEEE fp64, with h = [rank < c] and
 * count = [label > 0]: ndcg = label <= eps ? 0 : h / log2(rank + 2); recall = h / count; precision = h / c;
 * map = h (1 / (rank + 1)) / min(count, c); mrr = h ? 1 / (rank + 1) : 0; hit = h; f1 = 2 h / (count + c).  A row with label <= 0 gives
 * what those formulas give, NaN included.  The order of the additions is fixed, and calls are ordered by the stream, so an epoch's
 * accumulator is bitwise reproducible.  Every cutoff must lie in [1, topk] (the reference's map breaks above it): else DR4SR_E_ARG. */
int dr4sr_rank_metrics_accumulate(const int32_t* rank, const float* label, int64_t B, const int32_t* cutoffs, int32_t n_cut,
                                  int32_t topk, double* acc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FMLP (model/fmlp.py:18-39, module/layers.py:740-807): embedding + position -> LayerNorm -> dropout ->
 * n_layer x { spectral FilterLayer (rfft * complex weight -> irfft, 'ortho') -> dropout -> +x -> LayerNorm ;
 * Intermediate (64 -> 256 GELU -> 64, dropout, +x, LayerNorm) } -> x[:, -1].  Rows are LEFT-padded prefixes with a SCALAR
 * target (dataset/dataset_transform.ipynb), all B*L positions are computed (the filter mixes every position).
 * The reference hard-codes L = 50, D = 64, hidden 256, dropout 0.5 (fmlp.py:11-13, layers.py:743-744,:762); the kernels
 * require D = 64, F = 256, L <= 50... any L <= 50 even.
 * Flat parameter layout: E[N,D] | P[L,D] | ln_w[D] ln_b[D] | per layer: complex_weight[L/2+1, D, 2] | filt_ln_w filt_ln_b |
 *   dense_1.w[F,D] dense_1.b[F] dense_2.w[D,F] dense_2.b[D] | inter_ln_w inter_ln_b      (+ DR4SR_GRAD_TAIL on grads) */
typedef struct dr4sr_fmlp_plan {
    int32_t abi_version;
    int32_t B, L, D, F, n_layer, n_items;
    float   ln_eps, p_drop;
    uint64_t seed;
    float*  params; float* grads; float* adam_m; float* adam_v;
    int64_t n_params;
    const int64_t* in_item_id;      /* [U,L] left-padded prefixes                                  */
    const int64_t* item_id;         /* [U]   scalar targets (may be NULL for encode)               */
    const int64_t* rows;            /* [B] or NULL                                                  */
    int64_t* neg_item;              /* [B]   one negative per row                                   */
    int32_t  sample_neg;
    void*    workspace; int64_t workspace_bytes;
    int32_t* state;                 /* [DR4SR_STATE_WORDS]                                          */
    float lr, beta1, beta2, adam_eps, weight_decay;
    int32_t optimizer;              /* DR4SR_OPT_* (ABI 6)                                          */
    /* ---- fused batch selection + per-step loss log (ABI 6; dr4sr_sasrec_plan's contract): perm != NULL -> the step's first kernel FILLS
     *      rows[i] = perm[(c * perm_stride + perm_offset + i) mod n_perm], c = *perm_counter, and bumps the counter;
     *      dr4sr_fmlp_train_step / _adam_step write loss_log[c] = loss_sum / n_valid ---- */
    const int64_t* perm; int64_t n_perm; int64_t perm_stride; int64_t perm_offset; int32_t* perm_counter;
    float* loss_log;
} dr4sr_fmlp_plan;

int     dr4sr_fmlp_plan_sizeof(void);
/* offsets[0]=E [1]=P [2]=ln_w [3]=ln_b, [4+9*i+j] = j-th tensor of layer i in the order above; returns n_params */
int64_t dr4sr_fmlp_param_layout(int32_t n_items, int32_t L, int32_t D, int32_t F, int32_t n_layer, int64_t* offsets);
/* bytes, or DR4SR_E_SHAPE unless D = 64, F = 256, L even and <= 50 */
int64_t dr4sr_fmlp_workspace_bytes(const dr4sr_fmlp_plan* plan);
/* basemodel.py:193-198 for model = FMLP: negatives, forward, scorer + BCE (1-D targets), backward; un-normalised grads */
int dr4sr_fmlp_fwd_bwd(const dr4sr_fmlp_plan* plan, void* stream);
/* fwd_bwd + dense Adam */
int dr4sr_fmlp_train_step(const dr4sr_fmlp_plan* plan, void* stream);
/* the optimizer half on the plan's buffers (plan->optimizer, loss_log): data parallel = fwd_bwd, all-reduce of plan->grads, this */
int dr4sr_fmlp_adam_step(const dr4sr_fmlp_plan* plan, void* stream);
/* FMLP.forward -> out [B,D] (= encoder output at the last position); training != 0 applies dropout */
int dr4sr_fmlp_encode(const dr4sr_fmlp_plan* plan, int32_t training, float* out, void* stream);
/* autograd of dr4sr_fmlp_encode: d_out [B,D]; parameter gradients ACCUMULATE into plan->grads */
int dr4sr_fmlp_encode_bwd(const dr4sr_fmlp_plan* plan, int32_t training, const float* d_out, void* stream);
/* torch.optim.Adam on arbitrary flat buffers (grads[n] = normaliser, as dr4sr_adam_step); state[STEP] is bumped */
int dr4sr_adam_flat(float* params, const float* grads, float* adam_m, float* adam_v, int64_t n, int32_t* state,
                    float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* the same for any DR4SR_OPT_* (basemodel.py:79-98) */
int dr4sr_optimizer_flat(int32_t optimizer, float* params, const float* grads, float* adam_m, float* adam_v, int64_t n, int32_t* state,
                         float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GRU4Rec (model/gru4rec.py:12-34; module/layers.py:117-136 = torch.nn.GRU(bias=False, batch_first, n_layer) + Linear(H->D)):
 * x = dropout(E[idx]) -> GRU -> Linear -> 'origin'/'last' pooling -> scorer + BCE as SASRec.  D in {64, 128}, H in {128, 256},
 * n_layer <= 4, L <= 64.  Only rows < seqlen are computed (post-padded rows; the recurrence is causal).
 * Flat parameter layout: E[N,D] | per layer: weight_ih_l[3H,in] weight_hh_l[3H,H] | out_w[D,H] out_b[D]
 *   (names: item_embedding.weight == query_encoder.0.1.weight, query_encoder.0.3.gru.weight_{ih,hh}_l{l},
 *    query_encoder.1.{weight,bias}; gates ordered r|z|n as torch).  Optimizer: dr4sr_adam_flat (weight_decay 1e-4 in
 *   configs/gru4rec.yaml is torch.optim.Adam's L2 form). */
typedef struct dr4sr_gru4rec_plan {
    int32_t abi_version;
    int32_t B, L, D, H, n_layer, n_items;
    float   p_drop;                 /* dropout on the item embeddings (configs/gru4rec.yaml: 0.2) */
    uint64_t seed;
    float*  params; float* grads; float* adam_m; float* adam_v;
    int64_t n_params;
    const int64_t* in_item_id;      /* [U,L] */
    const int64_t* item_id;         /* [U,L] targets (may be NULL for encode) */
    const int64_t* seqlen;          /* [U]   */
    const int64_t* rows;            /* [B] or NULL */
    int64_t* neg_item;              /* [B,L] */
    int32_t  sample_neg;
    void*    workspace; int64_t workspace_bytes;
    int32_t* state;
    float lr, beta1, beta2, adam_eps, weight_decay;
    int32_t optimizer;              /* DR4SR_OPT_* (ABI 6) */
    /* ---- fused batch selection + per-step loss log (ABI 6; same contract as dr4sr_sasrec_plan's perm / loss_log fields): when
     *      perm != NULL the step's first kernel FILLS rows[i] = perm[(c * perm_stride + perm_offset + i) mod n_perm] with
     *      c = *perm_counter and bumps the counter; dr4sr_gru4rec_train_step / _adam_step write loss_log[c] = loss_sum / n_valid ---- */
    const int64_t* perm; int64_t n_perm; int64_t perm_stride; int64_t perm_offset; int32_t* perm_counter;
    float* loss_log;
} dr4sr_gru4rec_plan;

int     dr4sr_gru4rec_plan_sizeof(void);
/* offsets[0]=E, [1+2l]=weight_ih_l, [2+2l]=weight_hh_l, [1+2n]=out_w, [2+2n]=out_b; returns n_params */
int64_t dr4sr_gru4rec_param_layout(int32_t n_items, int32_t D, int32_t H, int32_t n_layer, int64_t* offsets);
/* The workspace must be ZERO-initialised once by the caller (hipMemset at allocation): for small batches (8*ceil(B/16) <= 192
 * workgroups) the recurrences run cooperatively over 8 CUs per 16 sequences and keep their exchange granules and a launch counter
 * there (csrc/gru_coop.hip); `DR4SR_GRU_NOCOOP=1` forces the single-workgroup recurrence.  The waits of that exchange are bounded:
 * a wait that runs out never hangs the GPU but sets a sticky error flag — the int32 word 2 of the workspace (words 0, 1: launch
 * counter, finish ticket) — and leaves garbage; the caller should read that word whenever it synchronises anyway (per epoch) and
 * treat non-zero as a failed run. */
/* bytes, or DR4SR_E_SHAPE unless D in {64, 128}, H in {128, 256}, L <= 64 */
int64_t dr4sr_gru4rec_workspace_bytes(const dr4sr_gru4rec_plan* plan);
/* the optimizer half of dr4sr_gru4rec_train_step on the plan's buffers (plan->optimizer, loss_log): data parallel = fwd_bwd,
 * all-reduce of plan->grads, this */
int dr4sr_gru4rec_adam_step(const dr4sr_gru4rec_plan* plan, void* stream);
/* n consecutive training steps, one prep launch: every optimizer launch but the last prepares the following step (see
 * dr4sr_sasrec_train_steps) */
int dr4sr_gru4rec_train_steps(const dr4sr_gru4rec_plan* plan, int32_t n_steps, void* stream);
/* 1 when a batch of B sequences takes the cooperative multi-CU recurrence on the CURRENT device (its 8*ceil(B/16) workgroups must be
 * co-resident: the budget is 3/4 of the device's compute units, at most 192, and 0 under DR4SR_GRU_NOCOOP), 0 for the
 * single-workgroup recurrence.  A timeout of the cooperative exchange also POISONS the step: the gradient tail word grads[n_params+2]
 * becomes non-zero and dr4sr_adam_flat / dr4sr_gru4rec_train_step then leave parameters, moments and the step counter untouched
 * (under data parallelism the all-reduced tail poisons every replica alike). */
int dr4sr_gru4rec_uses_cooperative(int32_t B, int32_t H);
/* 1 when a two-layer plan runs BOTH layers' recurrences in one launch, the second layer one time step behind the first (layer
 * wavefront, csrc/gru_coop.hip: n_layer == 2, H == 256, batches the 16-slice cooperative form takes; 0 under DR4SR_GRU_NOWAVE) */
int dr4sr_gru4rec_uses_wavefront(int32_t B, int32_t H, int32_t n_layer, int32_t L);
int dr4sr_gru4rec_fwd_bwd(const dr4sr_gru4rec_plan* plan, void* stream);       /* basemodel.py:193-198, un-normalised grads */
int dr4sr_gru4rec_train_step(const dr4sr_gru4rec_plan* plan, void* stream);    /* + dense Adam */
int dr4sr_gru4rec_encode(const dr4sr_gru4rec_plan* plan, int32_t training, int32_t pooling, float* out, void* stream);
int dr4sr_gru4rec_encode_bwd(const dr4sr_gru4rec_plan* plan, int32_t training, int32_t pooling, const float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DR4SR+ MetaModel (model/metamodel.py:19-197, utils/utils.py:134-252).
 *
 * The meta module is nn.Sequential(Linear(D,D), ReLU, Linear(D,2)) (metamodel.py:52-57); phi is its flat parameter vector
 * W1[D,D] | b1[D] | W2[2,D] | b2[2] (dr4sr_meta_param_count floats: 4 290 at D = 64, 16 770 at D = 128; any other D is
 * DR4SR_E_SHAPE).  D = 128 goes through dr4sr_meta_select_fwd_d / _bwd_d (same arguments, same semantics).
 *
 * dr4sr_meta_select_fwd — MetaModel.selection + the two masks of training_step (metamodel.py:169-185):
 *   weight[p] = softmax((meta_module(query[p]) + gumbel[p]) / tau)[0];  1 where user_id[p / L] == 0;  0 where target[p] == 0.
 *   n = B*L positions (L = 1 for scalar-target models).  gumbel [n,2] explicit noise, or NULL: drawn in-kernel from Philox
 *   (seed, step) as -log(-log(u)) like F.gumbel_softmax; step_dev != NULL: the step is *step_dev (a device word such as the plan's
 *   state[RNGSTEP], so that a captured graph draws fresh noise on every replay).  tau = clip(tau, tau_min) is passed by the caller.
 *   gate_in  [n][D/64] (NULL = off): a FROZEN ReLU pattern used instead of (pre > 0) — D/64 uint64 words per position, position-major;
 *            bit l of word h = hidden unit 64 h + l active (D = 64: one word per position);
 *   gate_out [n][D/64] (NULL = off): the pattern this call used, same layout.
 * dr4sr_meta_select_bwd — backward of the above for upstream d_weight[n] (times *scale if scale != NULL):
 *   d_query [n,D] is ACCUMULATED (+=; NULL = skip), d_phi ACCUMULATED, deterministically (per-block partials in `workspace`,
 *   dr4sr_meta_select_workspace_floats_d(n, D) floats, summed in a fixed order: two calls on the same inputs are bitwise equal).
 *   dr4sr_meta_select_workspace_floats(n) is the D = 64 size. */
int64_t dr4sr_meta_param_count(int32_t D);
int64_t dr4sr_meta_select_workspace_floats(int64_t n);
int64_t dr4sr_meta_select_workspace_floats_d(int64_t n, int32_t D);
/* D = 64 or 128 (dr4sr_meta_select_fwd / _bwd below keep meaning D = 64 alone and answer DR4SR_E_SHAPE to any other width, as they
 * always have; at D = 64 the _d forms ARE those calls, bit for bit): */
int dr4sr_meta_select_fwd_d(const float* query, const float* phi, const float* gumbel, uint64_t seed, uint32_t step,
                            const int32_t* step_dev, float tau,
                            const int64_t* user_id, const int64_t* target, int64_t B, int32_t L, int32_t D,
                            const uint64_t* gate_in, uint64_t* gate_out, float* weight, void* stream);
int dr4sr_meta_select_bwd_d(const float* query, const float* phi, const float* gumbel, uint64_t seed, uint32_t step,
                            const int32_t* step_dev, float tau,
                            const int64_t* user_id, const int64_t* target, int64_t B, int32_t L, int32_t D,
                            const uint64_t* gate_in, const float* d_weight, const float* scale, float* d_query, float* d_phi,
                            float* workspace, void* stream);
int dr4sr_meta_select_fwd(const float* query, const float* phi, const float* gumbel, uint64_t seed, uint32_t step,
                          const int32_t* step_dev, float tau,
                          const int64_t* user_id, const int64_t* target, int64_t B, int32_t L, int32_t D,
                          const uint64_t* gate_in, uint64_t* gate_out, float* weight, void* stream);
int dr4sr_meta_select_bwd(const float* query, const float* phi, const float* gumbel, uint64_t seed, uint32_t step,
                          const int32_t* step_dev, float tau,
                          const int64_t* user_id, const int64_t* target, int64_t B, int32_t L, int32_t D,
                          const uint64_t* gate_in, const float* d_weight, const float* scale, float* d_query, float* d_phi,
                          float* workspace, void* stream);

/* MetaModel's weighted loss fused into the SASRec training step (the fast path of dr4sr_amd/model/metamodel.py): the per-token
 * scorer computes weight_t = selection(z_t; phi) itself (same masks, noise keyed by (plan->seed, state[RNGSTEP], b*L+pos) exactly
 * like dr4sr_meta_select_fwd with step_dev = &state[RNGSTEP]) and back-propagates sum_t weight_t loss_t including
 * loss_t * d weight_t / d z_t.  grads tail = {n_valid, sum_t weight_t loss_t}.  d phi is NOT produced (the inner step never uses it;
 * the hyper-gradient takes it from dr4sr_meta_select_bwd).  gate_in / gate_out / weight_out are indexed by PACKED token
 * (workspace order: sequence by sequence, valid positions only), [B*L] words are enough.  D = 64 only. */
typedef struct dr4sr_meta_weighting {
    const float*   phi;             /* flat meta parameters (dr4sr_meta_param_count floats)                      */
    const float*   gumbel;          /* [B,L,2] explicit noise or NULL (Philox)                                   */
    const int64_t* user_id;         /* [U] addressed like the other dataset tensors (through plan->rows), or NULL */
    const uint64_t* gate_in;        /* frozen ReLU pattern per packed token, or NULL                             */
    uint64_t*      gate_out;        /* pattern used, per packed token, or NULL                                   */
    float*         weight_out;      /* weight per packed token, or NULL                                          */
    float          tau;             /* clip(tau, tau_min)                                                        */
} dr4sr_meta_weighting;
int dr4sr_sasrec_fwd_bwd_weighted(const dr4sr_sasrec_plan* plan, const dr4sr_meta_weighting* mw, void* stream);
/* the same on a batch already prepared by dr4sr_adam_step_prepare_next (k-step graphs of the MetaModel inner loop) */
int dr4sr_sasrec_fwd_bwd_weighted_prepared(const dr4sr_sasrec_plan* plan, const dr4sr_meta_weighting* mw, void* stream);

/* Hypergrad.grad (utils/utils.py:145-205) from FIRST-ORDER gradients: with G(W) = dL_train/dW (this library's backward),
 *     H v            = [G(W + e v) - G(W - e v)] / 2e                      (Neumann terms; scaled by hpo_lr, :196-203)
 *     d/dphi (G . p) = [dL_train/dphi(W + e p) - dL_train/dphi(W - e p)] / 2e   (:170-175)
 * evaluated with identical dropout masks / negatives / Gumbel noise and the meta module's ReLU pattern frozen at W (autograd's
 * second derivative of ReLU is 0).  All scalars stay on the device.
 *   step_size: *out_e = rel_step * sqrt(sum_{dir!=0} theta^2 / sum dir^2)
 *   shift    : out = x + sign * (*e) * dir
 *   neumann  : v -= lr * (gp / *np - gm / *nm) / (2 * *e) ;  pacc += v          (gp, gm un-normalised, np/nm their n_valid)
 *   diff     : out = coef * (fp / *np - fm / *nm) / (2 * *e)
 *   diff4    : out = coef * (4 D(e) - D(2e)) / 3 with D(h) = (f(+h)/n - f(-h)/n) / 2h from the probes at +-e (fp1, fm1) and +-2e
 *              (fp2, fm2), nv4 = their four n_valid words {+e, -e, +2e, -2e}: Richardson extrapolation, truncation error O(e^4).
 *              The mixed term is the whole hyper-gradient up to O(hpo_lr); at TRAINED weights (the reference's shipped checkpoint)
 *              its plain central difference sits at 1.0e-3 of the reference's double-backward, the extrapolated one at 1e-5.
 *   scale_by : out = x / *den */
int dr4sr_fd_step_size(const float* theta, const float* dir, int64_t n, float rel_step, float* out_e, void* stream);
/* the same with a caller-owned reduction scratch (dr4sr_fd_step_size_scratch_floats() floats, zeroed once): re-entrant, which the
 * form above — it reduces through a module-level scratch — is not */
int64_t dr4sr_fd_step_size_scratch_floats(void);
int dr4sr_fd_step_size_ws(const float* theta, const float* dir, int64_t n, float rel_step, float* out_e, float* scratch, void* stream);
int dr4sr_fd_shift(float* out, const float* x, const float* dir, const float* e, float sign, int64_t n, void* stream);
int dr4sr_fd_neumann(float* v, float* pacc, const float* gp, const float* gm, const float* np, const float* nm, const float* e,
                     float lr, int64_t n, void* stream);
int dr4sr_fd_diff(float* out, const float* fp, const float* fm, const float* np, const float* nm, const float* e, float coef,
                  int64_t n, void* stream);
int dr4sr_fd_diff4(float* out, const float* fp1, const float* fm1, const float* fp2, const float* fm2, const float* nv4,
                   const float* e, float coef, int64_t n, void* stream);
int dr4sr_scale_by(float* out, const float* x, const float* den, int64_t n, void* stream);

/* MetaOptimizer.step tail (utils/utils.py:240-247) for the reference's default meta optimizer (metamodel.py:68-69):
 * clip_grad_norm_(max_norm; <= 0 disables) then torch.optim.SGD(lr, momentum, weight_decay) on phi[n].
 * step_count (device int32) selects the first-step momentum initialisation and is incremented; out_norm (NULL ok) = |grad|. */
int dr4sr_meta_sgd_step(float* phi, const float* grad, float* momentum_buf, int32_t n, float lr, float momentum,
                        float weight_decay, float max_norm, int32_t* step_count, float* out_norm, void* stream);
/* ABI 7 — the same tail for the reference's other `meta_optimizer` choices (metamodel.py:59-81): optimizer = DR4SR_OPT_ADAM
 * ('adam': torch.optim.Adam(lr), weight_decay 0; any unknown name: Adam(lr, weight_decay = meta_weight_decay)), DR4SR_OPT_ADAGRAD
 * (Adagrad(lr): eps 1e-10, state_v = state_sum), DR4SR_OPT_RMSPROP (RMSprop(lr): beta2 = alpha 0.99, eps 1e-8, state_v = square_avg);
 * state_m / state_v [n] zero-initialised by the caller; step_count = steps taken so far (bias corrections use step_count + 1).
 * `tau` sits in the reference's parameter list but never receives a gradient (it is not in aux_params, metamodel.py:142), so torch
 * skips it: nothing to step.  'sparse_adam' raises in the reference's first step (dense gradients) — the binding raises the same error. */
int dr4sr_meta_opt_step(int32_t optimizer, float* phi, const float* grad, float* state_m, float* state_v, int32_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, float max_norm, int32_t* step_count,
                        float* out_norm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CL4SRec (model/cl4srec.py, module/data_augmentation.py:20-95,:305-350,:577-619): two augmented views of every sequence are
 * encoded by the SAME SASRec encoder (dr4sr_sasrec_encode with DR4SR_POOL_MEAN, one workspace per view), InfoNCE between the views.
 *
 * dr4sr_cl_augment — Item_Crop (mode 0: contiguous max(1, int(tau n)) items, left-aligned, out_len = that), Item_Mask (mode 1:
 *   int(gamma n) distinct positions -> mask_id), Item_Reorder (mode 2: a contiguous int(beta n) segment shuffled), Item_Random
 *   (mode 3: one of the three, drawn once per call).  seq/out [B,L] int64 (L <= 64), seqlen/out_len [B].  Philox (seed, step):
 *   same distributions as the reference's torch/numpy/random draws, not the same streams.
 * dr4sr_infonce_fwd — InfoNCELoss('inner_product', 'batch_both'): logits[i] = [x_i.x_j^T | x_i.x_i^T, diagonal -inf] / temperature,
 *   cross-entropy with label i.  valid[B] (uint8, NULL = all): rows with 0 are removed from rows and columns (the reference drops
 *   sequences of length 1, data_augmentation.py:613-615).  Outputs lse[B], loss_row[B] (0 at invalid rows), stats[0] += #valid rows,
 *   stats[1] += sum loss_row  (reduce=True loss = stats[1] / stats[0]; reduce=False = loss_row / #valid).
 * dr4sr_infonce_bwd — d(sum loss_row) * (*scale) accumulated into dxi, dxj [B,D]. */
int dr4sr_cl_augment(const int64_t* seq, const int64_t* seqlen, int64_t* out, int64_t* out_len, int32_t B, int32_t L, int32_t mode,
                     double tau, double gamma, double beta, int64_t mask_id, uint64_t seed, uint32_t step, void* stream);
/* the same with step = *step_dev + step_offset read at run time (graph replays of a training step) */
int dr4sr_cl_augment_dev(const int64_t* seq, const int64_t* seqlen, int64_t* out, int64_t* out_len, int32_t B, int32_t L, int32_t mode,
                         double tau, double gamma, double beta, int64_t mask_id, uint64_t seed, const int32_t* step_dev,
                         uint32_t step_offset, void* stream);
/* two views in one launch: what two consecutive dr4sr_cl_augment_dev calls (step_offset, step_offset + 1) produce */
int dr4sr_cl_augment2_dev(const int64_t* seq, const int64_t* seqlen, int64_t* out_i, int64_t* len_i, int64_t* out_j, int64_t* len_j,
                          int32_t B, int32_t L, int32_t mode, double tau, double gamma, double beta, int64_t mask_id, uint64_t seed,
                          const int32_t* step_dev, uint32_t step_offset, void* stream);
/* both views of the batch rows[0..B) of dataset tensors seq [U,L] / seqlen [U] (the batch a captured step selected on the device:
 * dr4sr_sasrec_plan.perm): the draws of dr4sr_cl_augment2_dev on the gathered rows */
int dr4sr_cl_augment2_rows_dev(const int64_t* seq, const int64_t* seqlen, const int64_t* rows, int64_t* out_i, int64_t* len_i,
                               int64_t* out_j, int64_t* len_j, int32_t B, int32_t L, int32_t mode, double tau, double gamma, double beta,
                               int64_t mask_id, uint64_t seed, const int32_t* step_dev, uint32_t step_offset, void* stream);
/* round 4: dr4sr_cl_prepare_rows that also advances the augmentation's device call counter by step_add (module/data_augmentation.py
 * end_step()), and dr4sr_infonce_bwd with the step's scalars computed inside: backward scale = cl_weight * tail[0] / stats[0], and with
 * fold_tail != 0 the contrastive term's share of the reported loss folded into tail[1] (what dr4sr_cl_scalars_dp in front of it gives) —
 * two launches less per CL4SRec step (model/cl4srec.py:_cl_term) */
int dr4sr_cl_prepare_rows_step(const int64_t* seqlen, const int64_t* rows, int32_t B, uint8_t* valid, float* stats, float* zero,
                               int64_t nzero, int32_t* step_dev, int32_t step_add, void* stream);
int dr4sr_infonce_bwd_scaled(const float* xi, const float* xj, const uint8_t* valid, int32_t B, int32_t D, float temperature,
                             const float* lse, float* tail, const float* stats, float cl_weight, int32_t fold_tail,
                             float* dxi, float* dxj, void* stream);
/* glue of a CL4SRec step composed without autograd (model/cl4srec.py:49-73 = BCE + cl_weight * InfoNCE):
 *   dr4sr_cl_prepare: valid[b] = seqlen[b] != 1 (data_augmentation.py:613-615), stats[0..1] = 0, zero[0..nzero) = 0;
 *   dr4sr_cl_scalars: with {n_valid, loss_sum} of the main pass in `tail` and InfoNCE's {rows, loss_sum} in `stats`:
 *     *scale_out = cl_weight * n_valid / rows (the InfoNCE backward scale under an optimizer that divides by n_valid),
 *     *loss_out = loss_sum / n_valid + cl_weight * stats[1] / rows;  either output may be NULL. */
int dr4sr_cl_prepare(const int64_t* seqlen, int32_t B, uint8_t* valid, float* stats, float* zero, int64_t nzero, void* stream);
int dr4sr_cl_prepare_rows(const int64_t* seqlen, const int64_t* rows, int32_t B, uint8_t* valid, float* stats, float* zero, int64_t nzero,
                          void* stream);      /* valid[b] = seqlen[rows[b]] != 1 */
int dr4sr_cl_scalars(const float* tail, const float* stats, float cl_weight, float* scale_out, float* loss_out, void* stream);
/* the same when n_valid is spread over n_parts words nv_parts[r * stride] (data parallel: every rank's count, all-gathered next to its
 * pooled views — InfoNCE's negatives are the GLOBAL batch; a single part = the local tail itself):
 *   *scale_out = cl_weight * sum_r nv_parts[r * stride] / rows;
 *   tail_local[1] += cl_weight * stats[1] / rows * tail_local[0]   (the contrastive term's share of the reported loss, so that the
 *   all-reduced tail[1] / tail[0] = BCE mean + cl_weight * InfoNCE mean).  Either output may be NULL. */
int dr4sr_cl_scalars_dp(const float* nv_parts, int32_t n_parts, int64_t stride, const float* stats, float cl_weight, float* scale_out,
                        float* tail_local, void* stream);
int dr4sr_infonce_fwd(const float* xi, const float* xj, const uint8_t* valid, int32_t B, int32_t D, float temperature, float* lse,
                      float* loss_row, float* stats, void* stream);
int dr4sr_infonce_bwd(const float* xi, const float* xj, const uint8_t* valid, int32_t B, int32_t D, float temperature,
                      const float* lse, const float* scale, float* dxi, float* dxj, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 9 — dataset regeneration (stage 3 of DR4SR, the reference's 3.Hybrid_inference.py): greedy decode of every training sequence
 * under each condition of the pre-trained regenerator (csrc/regen.hip).  The model is nn.Transformer(d_model 64, nhead 2, 2 encoder +
 * 2 decoder post-norm layers, FFN 256, erf-GELU, layer_norm_eps) with the final encoder / decoder norms, in eval mode:
 *   encode  : x = E[src] + P[0:Ls] -> 2 bidirectional layers (key padding beyond src_len) -> encoder.norm -> condition_linear[0] + ReLU;
 *             memory_k = features k*64:(k+1)*64 of condition_linear[2]; both decoder layers' cross-attention K | V of memory_k
 *   decode  : ys = [SOS]; per step i < max_len - 1: causal self-attention (per-layer K/V cache), cross-attention over memory_k, FFN,
 *             decoder.norm; logits = h @ E^T over ALL n_rows rows (PAD row 0 included); steps i <= 1 may pick only ids of src not in ys,
 *             steps i >= 2 any id not in ys; argmax (ties -> lowest id); stop after EOS = n_rows - 1 or max_len - 1 generated tokens.
 * Supported shape (anything else: DR4SR_E_SHAPE): D = 64, H = 2, F = 256, n_layer = 2 (encoder and decoder), K <= 5, 50 position rows,
 * 2 <= max_len <= 25, source rows of at most 50 ids.
 * Flat parameter layout (fp32; state-dict names of the reference's Generator):
 *   [0] E[n_rows,D] item_embedding.weight (= item_embedding_decoder.weight)   [1] P[50,D] position_embedding.weight
 *   per encoder layer i, [2+12*i+j]: transformer.encoder.layers.{i}.
 *        self_attn.in_proj_weight[3D,D] self_attn.in_proj_bias[3D] self_attn.out_proj.weight[D,D] self_attn.out_proj.bias[D]
 *        linear1.weight[F,D] linear1.bias[F] linear2.weight[D,F] linear2.bias[D] norm1.weight norm1.bias norm2.weight norm2.bias
 *   [26] transformer.encoder.norm.weight  [27] transformer.encoder.norm.bias
 *   per decoder layer i, [28+18*i+j]: transformer.decoder.layers.{i}.
 *        self_attn.{in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias}
 *        multihead_attn.{in_proj_weight[3D,D], in_proj_bias[3D], out_proj.weight, out_proj.bias}
 *        linear1.weight linear1.bias linear2.weight linear2.bias norm1.weight norm1.bias norm2.weight norm2.bias norm3.weight norm3.bias
 *   [64] transformer.decoder.norm.weight  [65] transformer.decoder.norm.bias
 *   [66] condition_linear.0.weight[K*D,D]  [67] condition_linear.0.bias[K*D]  [68] condition_linear.2.weight[K*D,K*D]
 *   [69] condition_linear.2.bias[K*D]                                      (condition_encoder.* is not used at inference) */
#define DR4SR_REGEN_TENSORS 70
typedef struct dr4sr_regen_plan {
    int32_t abi_version;            /* must be DR4SR_ABI_VERSION                                                               */
    int32_t n_rows;                 /* table rows N + 2 (SOS = N, EOS = N + 1; N counts PAD)                                  */
    int32_t K;                      /* conditions (condition_linear.2.weight is [64K, 64K])                                    */
    int32_t max_len;                /* the reference's max_len (25): at most max_len - 1 generated tokens                     */
    int32_t D, H, F, n_layer;       /* 64, 2, 256, 2                                                                          */
    float   ln_eps;                 /* layer_norm_eps (1e-12)                                                                  */
    const float* params;            /* [n_params] in the layout above                                                         */
    int64_t n_params;
} dr4sr_regen_plan;
int dr4sr_regen_plan_sizeof(void);
/* fills offsets[0..DR4SR_REGEN_TENSORS) (may be NULL) for the supported shape; returns n_params, or DR4SR_E_ARG for n_rows < 3 / K < 1 */
int64_t dr4sr_regen_param_layout(int32_t n_rows, int32_t K, int64_t* offsets);
/* bytes of scratch for a call over n_seq source rows and n_cond conditions (R = n_seq * n_cond decode rows: about 77 KB per row),
 * or DR4SR_E_SHAPE / DR4SR_E_ARG */
int64_t dr4sr_regen_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_seq, int32_t n_cond);
/* src [n_seq, Lsrc] int64 ids (row s holds src_len[s] ids: [SOS] + items + [EOS]; the rest is ignored), src_len [n_seq] int64.
 * Lsrc > 50 (the reference's position table) -> DR4SR_E_SHAPE.  Ids are clamped to [0, n_rows) and src_len to [1, Lsrc] on the device.
 * dr4sr_regen_encode fills the workspace with the cross-attention K | V of conditions cond0 .. cond0 + n_cond - 1 (cond0 + n_cond <= K);
 * dr4sr_regen_decode then enqueues all max_len - 1 steps for the R = n_cond * n_seq rows, condition-major (row c * n_seq + s decodes
 * source s under condition cond0 + c), and writes tokens [R, max_len] int64 (tokens[r, 0] = SOS; entries at or past len[r] are 0) and
 * len [R] int32 (the number of valid entries of tokens[r], SOS included).  Both calls take the same src / src_len / n_seq / n_cond /
 * workspace; the results do not depend on n_seq (a row decodes bit-identically alone or in any batch). */
int dr4sr_regen_encode(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_seq, int32_t Lsrc,
                       int32_t cond0, int32_t n_cond, void* workspace, int64_t workspace_bytes, void* stream);
int dr4sr_regen_decode(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, int64_t n_seq, int32_t Lsrc,
                       int32_t cond0, int32_t n_cond, void* workspace, int64_t workspace_bytes, int64_t* tokens, int32_t* len,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 10 — the regenerator's pre-training pairs (stage 1 of DR4SR, the second half of the reference's 1.Build_pretraining_dataset.py,
 * lines 70-93: `shuffle(patterns_value)` per sequence, then is_sublist over the list until ten patterns matched), csrc/pairs.hip.
 *   match(i, j) : pattern j is a subsequence of sequence i — not necessarily contiguous, repeated ids respected: the greedy left-most
 *                 scan of is_sublist (:70-77).  A pattern longer than the sequence does not match.
 *   n_match[i]  : the number m_i of matching patterns (all of them, not capped at 10).
 *   chosen[i,:] : the min(10, m_i) matching patterns with the smallest (key, j), ascending, -1 padded, where
 *                 key(i, j) = word x of philox4x32_10(counter = (seq_index0 + i, pat_index0 + j, 0x50414952, 0), key = (low, high 32 bits
 *                 of seed)) — a uniformly random subset in uniformly random order (what "shuffle, take the first ten hits" draws, :79-93),
 *                 a pure function of (seed, seq_index0 + i, pat_index0 + j): the same for any n_chunks, for any split of the sequences
 *                 over calls (pass the first row's index in the file as seq_index0), and whatever else is in the batch.  The values
 *                 written are pat_index0 + j.
 * seqs [n_seq, Lmax] int32 ids with seq_len [n_seq] int32 valid ids per row (clamped to [0, Lmax] on the device; the rest of a row is
 * ignored); patterns in ragged form: pat_ids [n_ids] int32 and pat_off [n_pat + 1] int64, pattern j = pat_ids[pat_off[j] : pat_off[j+1]].
 * n_chunks: how many workgroups share the pattern list per tile of 32 sequences (1..64; 0 = chosen from the sizes).
 * Checked on the host before anything is launched: null pointers, negative or >= 2^31 sizes and indices, n_chunks outside 0..64
 * (DR4SR_E_ARG); Lmax > 64 (DR4SR_E_SHAPE); a null or too small workspace (DR4SR_E_WS).  NOT checked on the host: the contents of
 * pat_off.  On the device a pattern whose offsets are not 0 <= pat_off[j] < pat_off[j+1] <= n_ids (non-monotonic offsets, an empty
 * pattern) or that has more than 64 ids matches nothing, so nothing is read out of bounds; ids are compared as given, whatever their
 * range.  Everything is enqueued on `stream`; there is no host synchronisation. */
int64_t dr4sr_pairs_workspace_bytes(int64_t n_seq, int64_t n_pat, int32_t n_chunks);
int dr4sr_pairs_match(const int32_t* seqs, const int32_t* seq_len, int64_t n_seq, int32_t Lmax, const int32_t* pat_ids,
                      const int64_t* pat_off, int64_t n_pat, int64_t n_ids, uint64_t seed, int64_t seq_index0, int64_t pat_index0,
                      int32_t n_chunks, void* workspace, int64_t workspace_bytes, int32_t* n_match, int32_t* chosen, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pattern mining for the regenerator (stage 1 of DR4SR, the first half of the reference's 1.Build_pretraining_dataset.py, lines 24-27:
 * Seq2Pat(sequences, max_span = alpha).get_patterns(min_frequency = beta)), csrc/mine.hip.  Additive to ABI 10.  The rule:
 *   pattern     : a tuple of k ids, 2 <= k <= alpha.
 *   occurrence  : positions p_0 < ... < p_{k-1} of one sequence that hold the tuple's ids, with p_{k-1} - p_0 <= alpha - 1 (all items
 *                 inside a window of alpha consecutive positions; csrc/mine.hip mine_reach is the one place of that bound).
 *   frequency   : the number of sequences with at least one occurrence.
 *   result      : every pattern with frequency >= beta, as rows of out_ids [cap, alpha] int32 (zero padded) and out_freq [cap] int32, in
 *                 NO particular order (the set of rows is a pure function of the input, their order is not; the caller sorts).
 * Sequences in ragged form: ids [n_ids] int32, every id >= 1, and seq_off [n_seq + 1] int64, sequence i = ids[seq_off[i] : seq_off[i+1]].
 * n_out [1] int32 receives the number of patterns found even when it exceeds cap (rows past cap are not written: call again with a
 * larger cap).  status [4] int64: [0] != 0 if the table filled up (the outputs are then meaningless), [1] the table's taken slots = the
 * number of distinct tuples seen, [2] the sum over them of the distance from their home slot, [3] 0.
 * The table: table_slots = 0 sizes it from n_ids * (2^(alpha-1) - 1), the number of (position, offset set) pairs, which no input can
 * exceed, so it never fills up; an explicit power of two up to 2^30 is used as given (probing is bounded by the table's size, so a table
 * that is too small ends the call quickly with status[0] set).  Workspace: 12 bytes per slot.
 * Checked on the host before anything is launched: null pointers, negative or >= 2^31 sizes, beta < 1, cap < 0, table_slots not 0 or a
 * power of two up to 2^30, n_ids * 2^(alpha-1) > 2^38 (DR4SR_E_ARG); alpha outside 2..10 (DR4SR_E_SHAPE); a null or too small
 * workspace (DR4SR_E_WS).  NOT checked on the host: the contents of seq_off and ids.  On the device a position that does not lie inside
 * 0 <= seq_off[i] <= position < seq_off[i+1] <= n_ids of the sequence a binary search finds for it starts no candidate, so nothing is
 * read out of bounds; an id <= 0 is compared as given and can merge two patterns.  A sequence of n ids costs O(n) reads per candidate
 * (the earlier-start test), which is why dr4sr_amd/mine.py refuses more than 4 096.  Three launches on `stream`, no host synchronisation. */
int64_t dr4sr_mine_workspace_bytes(int64_t n_ids, int64_t n_seq, int32_t alpha, int64_t table_slots);
int dr4sr_mine_patterns(const int32_t* ids, const int64_t* seq_off, int64_t n_ids, int64_t n_seq, int32_t alpha, int32_t beta,
                        int64_t table_slots, void* workspace, int64_t workspace_bytes, int32_t* out_ids, int32_t* out_freq, int64_t cap,
                        int32_t* n_out, int64_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Teacher-forced scoring of the regenerator (the forward and loss of DR4SR stage 2, the reference's 2.Pretrain_regenerator.py
 * Generator.forward + CrossEntropyLoss(ignore_index = 0) in eval mode: dropout off), csrc/regen_score.hip.  Additive to ABI 10.
 * A pair is (sequence s, pattern t); src row = [SOS] + s + [EOS], tgt row = [SOS] + t + [EOS], both padded with 0 to the widths of the
 * whole pairs file: src [n_pair, Ls], tgt [n_pair, T + 1] (tgt_in = columns 0..T-1, tgt_out = columns 1..T), src_len / tgt_len [n_pair]
 * int64 = len(s) + 2 / len(t) + 2.  Unlike the decode entry points, the PAD entries of a src row are read: they are masked as attention
 * keys and PAD 0 is one of the ids the softmax runs over when the row is padded (the reference's condition_mask).
 *   source    : E[src] + P[0:Ls] -> 2 encoder layers, causal (causal_source != 0: what stage 2 trains with) or bidirectional (what stage
 *               3 decodes with), keys with id 0 masked -> encoder.norm -> condition_linear -> memory[Ls, K, 64]
 *   condition : condition_encoder = 2 causal encoder layers over E[tgt_in] + P[0:T] (no final norm) -> sum of the first min(tgt_len, T)
 *               outputs divided by tgt_len (a row that fills the width has lost its EOS column and still divides by tgt_len) ->
 *               Linear 64 -> 64, ReLU, Linear 64 -> K: cond_logits [n_pair, K]
 *   score     : memory_cond = sum_k w[k] memory[:, k] for a weight vector w[K] (one-hot: the slice stage 3 decodes with; training feeds
 *               gumbel_softmax(cond_logits)) -> 2 decoder layers over E[tgt_in] + P[0:T] (causal, keys with id 0 masked; cross-attention
 *               over memory_cond, keys with src id 0 masked) -> decoder.norm -> logits h . E[id] over the DISTINCT ids of the padded src
 *               row only -> nll[t] = logsumexp - logit[tgt_out[t]]; 0 where tgt_out[t] = 0; +inf where tgt_out[t] is not in the src row.
 * w [n_w, n_pair, K] fp32, nll [n_w, n_pair, T] fp32 (every entry is written).  The source side runs once per pair for all n_w weight
 * vectors.  A pair's values do not depend on n_pair, n_w, its index or the other pairs (bit-identical alone or batched); no atomics.
 * Parameters: the DR4SR_REGEN_TENSORS tensors of the decode layout at the same indices and offsets, then
 *   per condition-encoder layer i, [70+12*i+j]: condition_encoder.encoder.layers.{i}. with the 12 tensors of an encoder layer above
 *   [94] condition_encoder.condition_layer.0.weight[D,D]  [95] .0.bias[D]  [96] .2.weight[K,D]  [97] .2.bias[K]
 * (all zero for a model saved without them: only the condition call reads them).  The plan is a dr4sr_regen_plan whose params / n_params
 * are THIS layout's buffer and size (max_len is not used); a buffer of the 70-tensor layout is refused with DR4SR_E_ARG.
 * Checked on the host before anything is launched: the plan (as for decode), null pointers, n_pair < 0 or >= 2^24, n_w < 1,
 * n_pair * n_w * T >= 2^30, Ls < 1, T < 1 (DR4SR_E_ARG); Ls > 50 or T > 50, the position table (DR4SR_E_SHAPE); a null or too small
 * workspace (DR4SR_E_WS).  Ids are clamped to [0, n_rows) and the lengths to their widths on the device.  Everything is enqueued on
 * `stream` (capturable); the workspace needs no initialisation and may be reused by any later call. */
#define DR4SR_REGEN_SCORE_TENSORS 98
/* fills offsets[0..DR4SR_REGEN_SCORE_TENSORS) (may be NULL); returns n_params, or DR4SR_E_ARG for n_rows < 3 / K < 1 */
int64_t dr4sr_regen_score_param_layout(int32_t n_rows, int32_t K, int64_t* offsets);
/* bytes of scratch: 4 (n_pair + 1) rounded up to 256, plus n_pair * K * 2 * Ls * 128 floats (the cross-attention K | V of every
 * condition, both decoder layers: 256 KB per pair at Ls = 50, K = 5); the same for every n_w.  The condition call needs the first term
 * only: the size for Ls = 1 is always enough for it. */
int64_t dr4sr_regen_score_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t Ls, int32_t T, int32_t n_w);
int dr4sr_regen_score_condition(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                void* workspace, int64_t workspace_bytes, float* cond_logits, void* stream);
int dr4sr_regen_score(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt, const int64_t* tgt_len,
                      int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w, int32_t causal_source, void* workspace,
                      int64_t workspace_bytes, float* nll, void* stream);

/* Gradients of teacher-forced scoring (csrc/regen_score_bwd.hip), additive to ABI 10.  Common to both calls: self-contained (each runs
 * the forward it needs), only enqueues on `stream` (capturable, no memset nodes), no floating-point atomics (the same call on the same
 * inputs gives the same bits); `grad` is a flat buffer in the 98-tensor score layout, accumulate = 0 overwrites every element of it,
 * accumulate = 1 adds; the workspace needs no initialisation.  Return codes and argument checks as dr4sr_regen_score. */

/* The vector-Jacobian product of dr4sr_regen_score: dnll [n_w, n_pair, T] (ignored where the target is PAD or outside its source: such a
 * token contributes nothing) -> grad (transformer.*, condition_linear.* and the two tables; the table takes its three terms: source
 * lookups, target lookups and the restricted logits, PAD row 0 through the logits of a padded source row) and dw [n_w, n_pair, K], the
 * gradient with respect to the condition weights.  nll_or_null, when given, receives the forward's NLLs [n_w, n_pair, T].  The workspace
 * is large (about 20 KB per decoder token slot and 26 KB per source position: ~2 MB per pair at Ls = 50, n_w = 1): callers chunk, the
 * Python wrapper at 256 pairs. */
int64_t dr4sr_regen_score_bwd_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t Ls, int32_t T, int32_t n_w);
int dr4sr_regen_score_bwd(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt, const int64_t* tgt_len,
                          int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w, int32_t causal_source, const float* dnll,
                          void* workspace, int64_t workspace_bytes, float* grad, float* dw, float* nll_or_null, int32_t accumulate,
                          void* stream);

/* The vector-Jacobian product of dr4sr_regen_score_condition: dlogits [n_pair, K] -> grad (condition_encoder.*, the item table and the
 * position table receive values).  Workspace: about 16 KB per token slot, 64 slots per tile of 65 - T live tokens, sized for
 * n_pair * T tokens. */
int64_t dr4sr_regen_score_condition_bwd_workspace_bytes(const dr4sr_regen_plan* plan, int64_t n_pair, int32_t T);
int dr4sr_regen_score_condition_bwd(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                    const float* dlogits, void* workspace, int64_t workspace_bytes, float* grad, int32_t accumulate,
                                    void* stream);

/* ---- additive to ABI 10: TRAIN MODE of the four teacher-forced calls (nn.Transformer's dropout, model.train() of
 * 2.Pretrain_regenerator.py:270-292).  Each *_train form is its eval form plus (p, seed, step, pair0) in front of the stream: the keep
 * factor 0 or 1 / (1 - p) at the reference's 30 sites, regenerated from (seed, step, site, element index) wherever it is consumed
 * (csrc/common.h's 16-bit Philox decisions; p = 0.5 is exact), never stored.  Row i of a call takes the masks of GLOBAL pair pair0 + i, so
 * a chunked run equals the unchunked one; the n_w weight vectors of a pair share their masks; the condition encoder's and the decoder's
 * calls of one (seed, step) share the tgt_emb mask, as the reference drops tgt_emb once.  p == 0 dispatches to the eval kernels (the
 * same bits as the eval entry point); p outside [0, 1) or pair0 outside [0, 2^40) is DR4SR_E_ARG.  Workspaces: the eval queries.
 * Sites (what the mask hook of include/dr4sr_hip_hooks.h takes as `site`): DR4SR_REGEN_SITE(stack, layer, kind) with stack 0 source encoder,
 * 1 condition encoder, 2 decoder; an encoder layer's kinds are 0 attention probabilities, 1 attention output, 2 FFN hidden, 3 FFN output, a
 * decoder layer's 0 self probabilities, 1 self output, 2 cross probabilities, 3 cross output, 4 FFN hidden, 5 FFN output.  Element index
 * (64-bit): hidden sites (pair 64 + position) 64 + column; FFN hidden (pair 64 + position) 256 + column; probabilities
 * ((pair 2 + head) 64 + query position) 64 + key position.  DESIGN.md has the table; dr4sr_amd/regen_dropout.py is the host mirror. */
#define DR4SR_REGEN_SITE_BASE 0x52470000u
#define DR4SR_REGEN_SITE(stack, layer, kind) (DR4SR_REGEN_SITE_BASE + (stack) * 32 + (layer) * 8 + (kind))
#define DR4SR_REGEN_SITE_SRC_EMB (DR4SR_REGEN_SITE_BASE + 96)
#define DR4SR_REGEN_SITE_TGT_EMB (DR4SR_REGEN_SITE_BASE + 97)
int dr4sr_regen_score_train(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                            const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                            int32_t causal_source, void* workspace, int64_t workspace_bytes, float* nll, float p, uint64_t seed,
                            uint32_t step, int64_t pair0, void* stream);
int dr4sr_regen_score_condition_train(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                      void* workspace, int64_t workspace_bytes, float* cond_logits, float p, uint64_t seed, uint32_t step,
                                      int64_t pair0, void* stream);
int dr4sr_regen_score_bwd_train(const dr4sr_regen_plan* plan, const int64_t* src, const int64_t* src_len, const int64_t* tgt,
                                const int64_t* tgt_len, int64_t n_pair, int32_t Ls, int32_t T, const float* w, int32_t n_w,
                                int32_t causal_source, const float* dnll, void* workspace, int64_t workspace_bytes, float* grad, float* dw,
                                float* nll_or_null, int32_t accumulate, float p, uint64_t seed, uint32_t step, int64_t pair0, void* stream);
int dr4sr_regen_score_condition_bwd_train(const dr4sr_regen_plan* plan, const int64_t* tgt, const int64_t* tgt_len, int64_t n_pair, int32_t T,
                                          const float* dlogits, void* workspace, int64_t workspace_bytes, float* grad, int32_t accumulate,
                                          float p, uint64_t seed, uint32_t step, int64_t pair0, void* stream);

/* ---- additive to ABI 10: the condition head of the pre-training step (csrc/regen_head.hip; 2.Pretrain_regenerator.py:270-292): what lies
 * between dr4sr_regen_score_condition's logits and dr4sr_regen_score_bwd's weights, and back.  Plain fp32, one thread per pair, no
 * atomics, only enqueues on `stream`; a pair's values depend on its GLOBAL index pair0 + i alone (a chunked batch gives the bits of the
 * whole).  DR4SR_E_ARG: a null pointer, n_pair outside [1, 2^24), K outside [1, 8], T outside [1, 50], tau <= 0, n_tok < 1,
 * n_batch < n_pair, pair0 outside [0, 2^40), slot < 0.
 * forward: w [n_pair, K] = softmax((cond_logits + g) / tau), ent [n_pair] = -(w log(w + 1e-12)).sum(-1), dnll [1, n_pair, T] = 1 / n_tok
 * (n_tok: the live target tokens of the whole BATCH, known to the host from the lengths).  g = noise [n_pair, K] when given (recorded
 * samples), else Gumbel(0, 1) from the project's Philox convention: element e = (pair0 + i) * 8 + k is word e & 3 of the call with counter
 * (e >> 2 low, e >> 2 high, DR4SR_REGEN_SITE_GUMBEL, step) under the key `seed`; u = ((r >> 8) + 0.5) 2^-24 in fp32, held below 1 (the
 * largest 24-bit value rounds up to 1 in fp32), g = -log(-log(u)) with both logs in double, rounded to fp32.  noise_out, when given,
 * receives the g that were used [n_pair, K].  dr4sr_amd/regen_dropout.py gumbel_noise is the host mirror.
 * backward: dw [1, n_pair, K] (the gradient of the cross entropy with respect to w, as dr4sr_regen_score_bwd returns it for the dnll
 * above), the forward's w and ent -> dlogits [n_pair, K], the gradient of CE + entropy_weight * (sum of ent over the batch / n_batch):
 * (diag(w) - w w^T) / tau applied to dw + (entropy_weight / n_batch) (-log(w + 1e-12) - w / (w + 1e-12)).  The same launch adds the
 * call's share of the step's log: loss_log[slot] += sum(nll [1, n_pair, T]) / n_tok and ent_log[slot] += sum(ent) / n_batch, each summed
 * in a fixed order by one wave (either log may be NULL; nll only then).  The caller zeroes the slot once per step. */
#define DR4SR_REGEN_SITE_GUMBEL (DR4SR_REGEN_SITE_BASE + 98)
int dr4sr_regen_head_fwd(const float* cond_logits, const float* noise_or_null, int64_t n_pair, int32_t K, int32_t T, float tau,
                         int64_t n_tok, uint64_t seed, uint32_t step, int64_t pair0, float* w, float* ent, float* dnll,
                         float* noise_out_or_null, void* stream);
int dr4sr_regen_head_bwd(const float* dw, const float* w, const float* ent, const float* nll, int64_t n_pair, int32_t K, int32_t T,
                         float tau, float entropy_weight, int64_t n_batch, int64_t n_tok, float* dlogits, float* loss_log_or_null,
                         float* ent_log_or_null, int64_t slot, void* stream);

/* ---- additive to ABI 10: graph propagation of the item table for the GNN target model (csrc/gnn.hip; the reference's model/gnn.py:43-50)
 *   out (+)= (in + A in + A^2 in + ... + A^n_hop in) / (n_hop + 1)
 * A [n_items, n_items] is CSR in fp32: row_ptr [n_items + 1] int64, col [nnz] int32 with every row's columns ascending, val [nnz].  in and
 * out are [n_items, D] fp32, D = 64 or 128 (anything else: DR4SR_E_SHAPE), and must not be the same buffer; in is only read.  accumulate = 0
 * overwrites out, 1 adds onto it.  n_hop = 0 copies (adds) bit-exactly and needs no workspace.  For a symmetric A (what
 * dr4sr_amd/model/gnn.py build_graph builds and asserts) the call is its own adjoint: forward in = E, out = G, accumulate 0; backward
 * in = dG, out = dE, accumulate 1.
 * One gather launch per hop (plus one single-workgroup launch per call that derives the chunk list of the long rows from row_ptr on the
 * device), all on `stream`, capturable; no float atomics and every sum in a fixed order: the same inputs give the same bits.  A row with
 * more than dr4sr_gnn_split_rows() edges is cut into chunks of that many edges, summed by separate waves and added in chunk order.
 * The workspace (dr4sr_gnn_workspace_bytes for the graph's nnz) holds the tables of A^k in, the running sum and the chunks' partial sums;
 * nothing in it survives a call.  DR4SR_E_ARG: a null pointer, in == out, n_items < 1, nnz < 0, n_hop outside [0, 64], accumulate not
 * 0 / 1; DR4SR_E_WS: a null or too small workspace with n_hop > 0.  NOT checked on the host: the contents of row_ptr / col (column ids are
 * clamped to [0, n_items) on the device). */
int32_t dr4sr_gnn_split_rows(void);
int64_t dr4sr_gnn_workspace_bytes(int32_t n_items, int32_t D, int64_t nnz);
int dr4sr_gnn_propagate(const int64_t* row_ptr, const int32_t* col, const float* val, int32_t n_items, int32_t D, int32_t n_hop,
                        const float* in, float* out, int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- additive to ABI 10: the stateless encoder-layer op and sequence pooling on dense tensors (csrc/layer_op.hip; what
 * torch.ops.dr4sr_hip.sasrec_layer / seq_pool / dropout run).  No plan, no workspace that survives a call, no device state words.
 *
 * The layer is ONE post-norm torch.nn.TransformerEncoderLayer as the reference configures it (model/sasrec.py:21-30): packed in_proj,
 * score scale 1 / sqrt(head_dim), exact-erf GELU, LayerNorm eps from the caller; x, y, dy, dx are [B, L, D] fp32, contiguous.  The mask is
 * general: key_pad is [B, L] uint8 (non-zero: the key is padded) or NULL for no padded key, and causal != 0 adds triu(1) (query i admits
 * keys j <= i).  A QUERY POSITION WITH NO ADMISSIBLE KEY GETS A ZERO ATTENTION CONTEXT (torch yields NaN there; the reference never reads
 * such a position): its output row is LayerNorm of the remaining terms, and the result and every gradient stay finite.
 * Supported shapes (anything else: DR4SR_E_SHAPE, before any launch): L <= 64 and (D, F, head_dim) in (64, 128 | 256, 32), (128, 128, 64),
 * head_dim = D / H.  DR4SR_E_ARG: a null pointer (key_pad and, in the forward, saved may be NULL), B < 0, p_drop outside [0, 1), eps < 0,
 * layer outside [0, 1024].  B = 0 launches nothing (the backward zero-fills dw); the activation pointers may then be null.
 *
 * Dropout: the four sites DR4SR_SITE_ATTN / PROJ / ACT / FFN + 4 * layer of the library's Philox stream keyed by (seed, step, site); the
 * decision of an element is that of element e of the hooks header's dr4sr_dropout_mask for the same (p, seed, step, site), with
 *     PROJ, FFN:  e = (b * L + pos) * D + c          ACT:  e = (b * L + pos) * F + c          ATTN:  e = ((b * H + h) * L + i) * L + j
 * (i the query, j the key).  p_drop == 0 does no RNG work.
 *
 * saved (forward: written when non-NULL; backward: read) is opaque, dr4sr_sasrec_layer_saved_floats floats: NULL for inference.  The
 * backward takes the inputs of the forward it differentiates; dx and the 12 tensors of dw are WRITTEN, not accumulated.  It uses no float
 * atomics: every workgroup sums the sequences it owns in index order into its slot of ws (dr4sr_sasrec_layer_workspace_bytes), a second
 * launch adds the slots in index order — two calls give the same bits.  A null or too small ws: DR4SR_E_WS.
 * Launches on `stream` only (capturable), no allocation, no host synchronisation. */
typedef struct dr4sr_layer_weights {       /* the layer tensors in the flat layout's order */
    const float *in_proj_weight, *in_proj_bias, *out_proj_weight, *out_proj_bias, *linear1_weight, *linear1_bias, *linear2_weight,
        *linear2_bias, *norm1_weight, *norm1_bias, *norm2_weight, *norm2_bias;
} dr4sr_layer_weights;
typedef struct dr4sr_layer_grads {
    float *in_proj_weight, *in_proj_bias, *out_proj_weight, *out_proj_bias, *linear1_weight, *linear1_bias, *linear2_weight, *linear2_bias,
        *norm1_weight, *norm1_bias, *norm2_weight, *norm2_bias;
} dr4sr_layer_grads;
/* floats / bytes, or a negative DR4SR_E_* code */
int64_t dr4sr_sasrec_layer_saved_floats(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F);
int64_t dr4sr_sasrec_layer_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F);
int dr4sr_sasrec_layer_fwd(const float* x, const uint8_t* key_pad, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                           int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer, float* y,
                           float* saved, void* stream);
int dr4sr_sasrec_layer_bwd(const float* x, const uint8_t* key_pad, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                           int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer,
                           const float* saved, const float* dy, float* dx, const dr4sr_layer_grads* dw, void* ws, int64_t ws_bytes,
                           void* stream);
/* Pooling of x [B, L, D] by seqlen [B] int64 (clamped to [0, L]): DR4SR_POOL_ORIGIN zeroes the rows at pos >= seqlen -> [B, L, D]
 * (module/layers.py:41-50); DR4SR_POOL_LAST is row seqlen - 1 -> [B, D] (layers.py:69-73); DR4SR_POOL_MEAN the mean of the rows below
 * seqlen -> [B, D] (module/functional.py:50-55).  A row with seqlen 0 pools to zeros.  The backward WRITES dx [B, L, D] from dout in the
 * forward's output shape.  Any other pooling value, a null pointer, B < 0, L < 1, D < 1: DR4SR_E_ARG. */
int dr4sr_seq_pool_fwd(const float* x, const int64_t* seqlen, int32_t pooling, int64_t B, int32_t L, int32_t D, float* out, void* stream);
int dr4sr_seq_pool_bwd(const float* dout, const int64_t* seqlen, int32_t pooling, int64_t B, int32_t L, int32_t D, float* dx, void* stream);
/* out[e] = x[e] * keep(e) / (1 - p) with the keep decision of element e of stream (seed, step, site), n a multiple of 4 (the embedding
 * dropout, DR4SR_SITE_EMB, of a model written on the ops; its own backward with dy for x).  out may be x.  p_drop == 0 copies. */
int dr4sr_dropout_apply(const float* x, int64_t n, float p_drop, uint64_t seed, uint32_t step, uint32_t site, float* out, void* stream);
/* Backward of dr4sr_embed_gather_posadd for a model written on the ops: dE [n_items, D] and dP [n_pos, D] are WRITTEN — dE[idx] += dx over
 * the tokens (PAD id 0 and ids outside the table pass nothing: row 0 is exactly 0), dP[pos] = the sum of dx[b, pos] over b in index order
 * (rows at and behind L are 0).  The table scatter adds with float atomics: dE is reproducible to rounding, not to the bit.  D a multiple
 * of 4 (else DR4SR_E_SHAPE); a null pointer, B < 0 or above 2^24, L < 1, n_items < 1, n_pos < L: DR4SR_E_ARG. */
int dr4sr_embed_gather_posadd_bwd(const float* dx, const int64_t* idx, int64_t B, int32_t L, int32_t D, int32_t n_items, int32_t n_pos,
                                  float* dE, float* dP, void* stream);

/* ---- additive to ABI 10: the stateless FMLP layer op and the LayerNorm op on dense tensors (csrc/fmlp_op.hip; what
 * torch.ops.dr4sr_hip.fmlp_layer / layer_norm run).  No plan, no workspace that survives a call, no device state words.
 *
 * The layer is ONE FMLP `Layer` of the reference (module/layers.py:781-791) on x [B, L, D] fp32, contiguous:
 *     f  = irfft(rfft(x, dim=1, 'ortho') * view_as_complex(complex_weight), n=L, dim=1, 'ortho')
 *     xf = LayerNorm_f(drop_FILT(f) + x)
 *     y  = LayerNorm_i(drop_FFN(dense_2(gelu_erf(dense_1(xf)))) + xf)          (no dropout behind the GELU, as in the reference)
 * complex_weight is [1, L/2 + 1, D, 2] (re | im innermost), the LayerNorm tensors [D], dense_1 [F, D] | [F], dense_2 [D, F] | [D]; LayerNorm
 * eps from the caller.  The filter is computed as the per-feature circular convolution it equals (csrc/fmlp.hip): the imaginary parts
 * of the DC and Nyquist bins contribute nothing and receive a zero gradient, as in torch.
 * Supported shapes (anything else: DR4SR_E_SHAPE, before any launch): D = 64, F = 256, L even, 2 <= L <= 64.  DR4SR_E_ARG: a null
 * pointer (in the forward, saved may be NULL), B < 0, p_drop outside [0, 1), eps < 0, layer outside [0, 1024].  A null or too small
 * workspace (dr4sr_fmlp_layer_workspace_bytes with backward = 0 for the forward, 1 for the backward): DR4SR_E_WS; nothing in it survives a
 * call.  B = 0 launches nothing (the backward zero-fills dw); the activation pointers and the workspace may then be null.
 *
 * Dropout: the two sites 1 + 2 * layer (behind the filter) and 2 + 2 * layer (behind dense_2) of the library's Philox stream keyed by
 * (seed, step, site) — the numbering of the FMLP engine, site 0 being its embedding dropout; the decision of an element is that of
 * element e = (b * L + pos) * D + c of the hooks header's dr4sr_dropout_mask for the same (p, seed, step, site), which is what the engine
 * draws on a plan without `rows`.  p_drop == 0 does no RNG work.
 *
 * saved (forward: written when non-NULL; backward: read) is opaque, dr4sr_fmlp_layer_saved_floats floats (both LayerNorm inputs and the
 * FFN pre-activation): NULL for inference.  The backward takes the inputs of the forward it differentiates; dx and the 9 tensors of dw
 * are WRITTEN, not accumulated.  It uses no float atomics: every workgroup sums the sequences it owns in index order into its slot of
 * ws, a second launch adds the slots in index order and folds the filter-kernel gradient back to d complex_weight — two calls give the
 * same bits.  Launches on `stream` only (capturable), no allocation, no host synchronisation. */
typedef struct dr4sr_fmlp_layer_weights {  /* the layer tensors in the flat layout's order (dr4sr_fmlp_param_layout) */
    const float *complex_weight, *filter_ln_weight, *filter_ln_bias, *dense_1_weight, *dense_1_bias, *dense_2_weight, *dense_2_bias,
        *inter_ln_weight, *inter_ln_bias;
} dr4sr_fmlp_layer_weights;
typedef struct dr4sr_fmlp_layer_grads {
    float *complex_weight, *filter_ln_weight, *filter_ln_bias, *dense_1_weight, *dense_1_bias, *dense_2_weight, *dense_2_bias,
        *inter_ln_weight, *inter_ln_bias;
} dr4sr_fmlp_layer_grads;
/* floats / bytes, or a negative DR4SR_E_* code */
int64_t dr4sr_fmlp_layer_saved_floats(int64_t B, int32_t L, int32_t D, int32_t F);
int64_t dr4sr_fmlp_layer_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t F, int32_t backward);
int dr4sr_fmlp_layer_fwd(const float* x, const dr4sr_fmlp_layer_weights* w, int64_t B, int32_t L, int32_t D, int32_t F, float eps,
                         float p_drop, uint64_t seed, uint32_t step, int32_t layer, float* y, float* saved, void* ws, int64_t ws_bytes,
                         void* stream);
int dr4sr_fmlp_layer_bwd(const float* x, const dr4sr_fmlp_layer_weights* w, int64_t B, int32_t L, int32_t D, int32_t F, float eps,
                         float p_drop, uint64_t seed, uint32_t step, int32_t layer, const float* saved, const float* dy, float* dx,
                         const dr4sr_fmlp_layer_grads* dw, void* ws, int64_t ws_bytes, void* stream);
/* torch.nn.LayerNorm over the last dimension of x [n_rows, D] (FMLP's embedding LayerNorm, model/fmlp.py:25): biased variance, eps from
 * the caller, D a multiple of 4 up to 1024 (else DR4SR_E_SHAPE).  The backward recomputes the statistics from x and WRITES dx, dw and db
 * (slots of ws summed in index order: two calls give the same bits).  A null pointer, n_rows < 0, eps < 0: DR4SR_E_ARG; a null or too
 * small ws (dr4sr_layer_norm_workspace_bytes): DR4SR_E_WS.  n_rows = 0 launches nothing (the backward zero-fills dw and db). */
int64_t dr4sr_layer_norm_workspace_bytes(int64_t n_rows, int32_t D);
int dr4sr_layer_norm_fwd(const float* x, const float* weight, const float* bias, int64_t n_rows, int32_t D, float eps, float* y,
                         void* stream);
int dr4sr_layer_norm_bwd(const float* x, const float* weight, int64_t n_rows, int32_t D, float eps, const float* dy, float* dx, float* dw,
                         float* db, void* ws, int64_t ws_bytes, void* stream);

/* ---- additive to ABI 10: the stateless GRU layer op on dense tensors (csrc/gru_op.hip; what torch.ops.dr4sr_hip.gru_layer runs).  No
 * plan, no workspace that survives a call, no device state words, no communication between workgroups inside a launch.
 *
 * ONE layer of torch.nn.GRU(bias=False, batch_first=True) (module/layers.py:117-136) on x [B, L, I] fp32, contiguous, h_0 = 0;
 * w_ih [3H, I] and w_hh [3H, H] hold the gates in torch's order r | z | n:
 *     gi = x_t w_ih^T ;  gh = h_{t-1} w_hh^T
 *     r = sigmoid(gi_r + gh_r) ;  z = sigmoid(gi_z + gh_z) ;  n = tanh(gi_n + r * gh_n) ;  h_t = (1 - z) * n + z * h_{t-1}
 * y [B, L, H] holds every h_t.  fp32 MFMA throughout.
 * Supported shapes (anything else: DR4SR_E_SHAPE, from the size entry points and from the calls, before any launch): I = 64, 128 or 256,
 * H = 128 or 256, 1 <= L <= 1024.  DR4SR_E_ARG: a null pointer (seqlen may be NULL, and in the forward saved), B < 0 or above 2^24.  A
 * null or too small workspace (dr4sr_gru_layer_workspace_bytes with backward = 0 for the forward, 1 for the backward): DR4SR_E_WS;
 * nothing in it survives a call.  B = 0 launches nothing (the backward zero-fills dw_ih and dw_hh); the activation pointers and the
 * workspace may then be null.  Index arithmetic is 64-bit.
 *
 * seqlen: NULL computes all L steps of every sequence, as the reference does (it feeds the pads).  With seqlen [B] (int64, on the
 * device) every value is clamped to [0, L] and the steps at and behind seqlen[b] are skipped: y and dx are exactly 0 there, x and dy
 * there are never read (they may hold anything).  Both agree wherever only positions in front of seqlen[b] are read downstream (the
 * recurrence is causal; 'origin' and 'last' pooling read nothing else).  A sequence of length 0 is legal and gives zeros.
 *
 * saved (forward: written when non-NULL; backward: read) is opaque, dr4sr_gru_layer_saved_floats floats (r, z, n and gh_n per token;
 * h_{t-1} is y shifted by one step): NULL for inference.  The backward takes the inputs and the y of the forward it differentiates; dx,
 * dw_ih and dw_hh are WRITTEN, not accumulated.  It uses no float atomics: every workgroup of the weight-gradient launch sums the
 * 64-token tiles of its token split in index order into its own slot of ws, a last launch adds the slots in index order — two calls
 * give the same bits.  Launches on `stream` only (capturable), no allocation, no host synchronisation. */
/* floats / bytes, or a negative DR4SR_E_* code */
int64_t dr4sr_gru_layer_saved_floats(int64_t B, int32_t L, int32_t I, int32_t H);
int64_t dr4sr_gru_layer_workspace_bytes(int64_t B, int32_t L, int32_t I, int32_t H, int32_t backward);
int dr4sr_gru_layer_fwd(const float* x, const float* w_ih, const float* w_hh, const int64_t* seqlen, int64_t B, int32_t L, int32_t I,
                        int32_t H, float* y, float* saved, void* ws, int64_t ws_bytes, void* stream);
int dr4sr_gru_layer_bwd(const float* x, const float* w_ih, const float* w_hh, const int64_t* seqlen, int64_t B, int32_t L, int32_t I,
                        int32_t H, const float* y, const float* saved, const float* dy, float* dx, float* dw_ih, float* dw_hh, void* ws,
                        int64_t ws_bytes, void* stream);

/* ---- additive to ABI 10: the encoder-layer op with sequence lengths, short sequences sharing a 64-row tile (csrc/layer_packed.hip; what
 * torch.ops.dr4sr_hip.sasrec_layer_packed runs).  No plan that survives a call, no device state words, no host synchronisation.
 *
 * The layer, the supported shapes, the dropout sites and elements and the refusals are those of dr4sr_sasrec_layer_fwd / _bwd above; x, y,
 * dy, dx are the same dense [B, L, D] fp32 tensors.  Instead of a key-padding mask the call takes seqlen [B] (int64, on the device; NULL:
 * DR4SR_E_ARG): sequence b has n_b = clamp(seqlen[b], 0, L) valid positions 0 .. n_b - 1 (the rows are post-padded) and its keys at
 * pos >= n_b are padded; causal != 0 adds triu(1).  y and dx are EXACTLY 0 at pos >= n_b; x and dy there are never read (they may hold
 * anything).  At pos < n_b the result is that of the dense op with key_pad = (pos >= n_b) up to the summation order of the weight
 * gradients, and the dropout decisions are the dense op's: an element's index uses the token's own (b, pos), so a sequence draws the same
 * masks packed, dense, alone or in a batch.
 *
 * Work: a small launch on `stream` assigns the sequences to 64-row tiles, in chunks of C consecutive sequences planned independently
 * (C: the probe dr4sr_sasrec_layer_packed_chunk, include/dr4sr_hip_probes.h).  A chunk starts a tile; a sequence with n_b = 0 takes no
 * rows; a sequence that does not fit behind the rows already in the tile starts the next one; no sequence straddles a tile.  One
 * workgroup computes one tile at a time, attention being
 * block-diagonal over the tile's sequences.  The grid depends on B alone; the tile count stays on the device.
 *
 * saved is opaque, dr4sr_sasrec_layer_packed_saved_floats floats (never more than dr4sr_sasrec_layer_saved_floats of the shape); nothing
 * is written into it for pos >= n_b; NULL for inference.  ws: dr4sr_sasrec_layer_packed_workspace_bytes (backward = 0 for the forward,
 * 1 for the backward), else DR4SR_E_WS; nothing in it survives a call, the backward plans again from seqlen.  dx and the 12 tensors of dw
 * are WRITTEN, not accumulated, without float atomics: a workgroup sums the tiles it owns (blockIdx.x, + gridDim.x, ...) in that order into
 * its slot of ws, a last launch adds the min(tiles, slots) written slots in index order — two calls give the same bits.  B = 0 launches
 * nothing and every n_b = 0 gives y = 0, dx = 0; in both cases the backward zero-fills dw. */
int64_t dr4sr_sasrec_layer_packed_saved_floats(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F);
int64_t dr4sr_sasrec_layer_packed_workspace_bytes(int64_t B, int32_t L, int32_t D, int32_t H, int32_t F, int32_t backward);
int dr4sr_sasrec_layer_packed_fwd(const float* x, const int64_t* seqlen, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                                  int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer,
                                  float* y, float* saved, void* ws, int64_t ws_bytes, void* stream);
int dr4sr_sasrec_layer_packed_bwd(const float* x, const int64_t* seqlen, int32_t causal, const dr4sr_layer_weights* w, int64_t B, int32_t L,
                                  int32_t D, int32_t H, int32_t F, float eps, float p_drop, uint64_t seed, uint32_t step, int32_t layer,
                                  const float* saved, const float* dy, float* dx, const dr4sr_layer_grads* dw, void* ws, int64_t ws_bytes,
                                  void* stream);

/* Test / measurement hooks (dr4sr_dropout_mask, dr4sr_*_launch_kernel) are NOT part of this product surface: they are declared in
 * include/dr4sr_hip_hooks.h, and nothing under dr4sr_amd/ calls them. */

#ifdef __cplusplus
}
#endif
#endif /* DR4SR_HIP_H */
