/*
 * eegnet_abi.h -- C-ABI of libeegnet_hip.so, the MI355X (gfx950) EEGNet train/infer step.
 *
 * Drop-in boundary for the reference's hot path (PraKesEy/EEGNetReplication):
 *   EEGNet.forward            src/eegnet_repl/model.py:91-99   -> eegnet_forward_train / eegnet_forward_eval
 *   loss.backward() + hooks   src/eegnet_repl/model.py:44,84,147 -> eegnet_backward
 *   optimizer.step() (Adam)   src/eegnet_repl/train.py:94-101, model.py:148 -> eegnet_adam_step
 *   one hot-loop iteration    src/eegnet_repl/model.py:136-148 -> eegnet_train_step
 *   saliency / x.grad in .eval() (plain autograd on the nn.Module) -> eegnet_input_grad_eval
 *   the hot loop with bn.eval() on the three BatchNorm2d (fine-tuning) -> eegnet_frozen_step
 *   that fine-tuning loop for many models at once (per-subject fine-tuning, k folds each) -> eegnet_frozen_step_folds
 *   the per-epoch validation loop src/eegnet_repl/model.py:151-172, many folds at once -> eegnet_eval_folds
 *   raw_exponential_moving_standardize  src/eegnet_repl/dataset.py:45-70 -> eegnet_ems
 *   raw.filter(4., 38., fir_design='firwin')  src/eegnet_repl/dataset.py:113-125 -> eegnet_fir
 *   mne.Epochs(tmin=0.5, tmax=2.5) + model.eval()  src/eegnet_repl/dataset.py:223-224 -> eegnet_forward_eval_windows_at
 *   raw.resample(128, npad="auto")  src/eegnet_repl/dataset.py:114 -> eegnet_resample (the polyphase method, not
 *                                                                       the FFT method that call defaults to)
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor) unless noted.  The library never
 *     allocates or frees; the caller owns params, buffers and the workspace (eegnet_workspace_bytes).
 *   - All work is enqueued on `stream`; no host synchronisation happens inside, so every call can be
 *     captured in a hipGraph.
 *   - Return 0 on success, a negative EEGNET_E* code otherwise; eegnet_last_error() (thread-local)
 *     describes the failure.  The Python side raises RuntimeError with that text.
 *   - `params` is ONE flat fp32 buffer in nn.Module.named_parameters() order:
 *       temporal.0.weight[F1,1,1,K1]  temporal.1.weight[F1]  temporal.1.bias[F1]
 *       spatial.weight[F2,1,C,1]      aggregation.0.weight[F2] aggregation.0.bias[F2]
 *       block_2.0.weight[F2,1,1,16]   block_2.1.weight[F2,F2,1,1]
 *       block_2.2.weight[F2]          block_2.2.bias[F2]
 *       classifier.weight[4,F2*(T/32)] classifier.bias[4]          (F2 = F1*D)
 *     (1,716 floats for EEGNet-8,2 at C=22, T=256).  `grads` has the same layout.
 *   - `bn_buffers` is one flat fp32 buffer: running_mean/running_var of temporal.1 [F1,F1],
 *     aggregation.0 [F2,F2], block_2.2 [F2,F2].  The three num_batches_tracked counters are an
 *     optional separate int64[3] device buffer (the last argument of eegnet_forward_train and
 *     eegnet_train_step; NULL = not tracked), incremented in-kernel once per train-mode forward.
 *   - x is [B,C,T] fp32 row-major; labels int64 [B] in [0,4); logits fp32 [B,4].
 *   - Dropout keep-masks: uint8 [B,F2,T/4] and [B,F2,T/128] (1 = keep), nullable.  NULL means the
 *     on-device counter-based generator keyed by (seed, offset): the same (seed, offset) always
 *     produces the same masks, and forward and backward see the same ones.
 */
#ifndef EEGNET_ABI_H
#define EEGNET_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eegnet_dims {
    int B;          /* trials in the batch                                  */
    int C;          /* EEG channels          (model.py:13 `C`)              */
    int T;          /* samples per trial     (model.py:13 `T`)              */
    int F1;         /* temporal filters      (model.py:13, default 8)       */
    int D;          /* depth multiplier      (model.py:13, default 2)       */
    int K1;         /* temporal kernel length (model.py:26: 32; 64 also supported, except for
                       training with F1*D > 16: eegnet_forward_train, _backward and _train_step
                       return EEGNET_EINVAL for those dims, the eval forward takes them)  */
    float p_drop;   /* dropout p             (model.py:13, 50, 74)          */
    float bn_eps;   /* BatchNorm2d eps (1e-5)                               */
    float bn_momentum; /* BatchNorm2d momentum (0.1)                        */
    int x_pitch;    /* floats between consecutive channel rows of x (0: T, x is [B][C][T]); a
                       larger pitch (eegnet_x_pitch) lets the training kernels load the rows of
                       x in 16-byte units; samples [T, x_pitch) of a row are never read     */
} eegnet_dims;

enum {
    EEGNET_OK = 0,
    EEGNET_EINVAL = -1,   /* unsupported or inconsistent dims / null pointer */
    EEGNET_ELAUNCH = -2,  /* a kernel launch failed                          */
};

enum { EEGNET_TRAIN = 1, EEGNET_EVAL = 0 };

/* eegnet_backward flags */
enum {
    EEGNET_NO_CLAMP = 1,      /* leave model.py:44/84 clamps to eegnet_clamp_grads (after an all-reduce) */
    EEGNET_KEY_FROM_STEP = 2  /* eegnet_train_step: dropout key = mix(seed, offset + *step), read on the
                                 device, so a captured hipGraph draws fresh masks on every replay */
    /* 4 (round 5's opt-in one-launch persistent step) is retired: eegnet_train_step rejects any other
       bit with EEGNET_EINVAL */
};

/* Number of fp32 elements of the flat parameter buffer for these dims. */
int eegnet_param_count(const eegnet_dims* dims, int64_t* out);

/* Bytes of scratch the train-mode calls need (forward -> backward state lives here).  The workspace
 * must be zero-filled once before its first use (hipMemset / torch.zeros); the library keeps its
 * reduction tickets re-armed from then on. */
int eegnet_workspace_bytes(const eegnet_dims* dims, size_t* out);

/* Train-mode forward (BN batch statistics, dropout, running-stat momentum update).
 * Replaces model.py:141 `preds = model(signals)` in train mode.  Leaves what backward needs in `ws`.
 * num_batches_tracked (nullable): the three BatchNorm2d counters as one int64[3] device buffer,
 * incremented in-kernel. */
int eegnet_forward_train(const eegnet_dims* dims, const float* params, float* bn_buffers,
                         const float* x, const uint8_t* mask2, const uint8_t* mask3,
                         uint64_t seed, uint64_t offset, float* logits, void* ws, void* stream,
                         int64_t* num_batches_tracked);

/* Backward of the last eegnet_forward_train on the same `ws` (same x, params, masks, seed/offset).
 * Gradient source: `dlogits` [B,4] if non-NULL (autograd), else mean cross-entropy against `labels`
 * (train.py:103), in which case the scalar loss is written to `loss` (device fp32, nullable).
 * `grads` receives all 12 parameter gradients with the clamps of model.py:44 (+-1) and model.py:84
 * (+-0.25) applied, unless flags has EEGNET_NO_CLAMP. */
int eegnet_backward(const eegnet_dims* dims, const float* params, const float* x,
                    const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                    const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads, float* loss,
                    void* ws, void* stream, int flags);

/* The gradient hooks of model.py:44 (spatial.weight, +-1) and model.py:84 (classifier.weight,
 * +-0.25) on a flat grad buffer -- for data-parallel runs, after the gradient all-reduce. */
int eegnet_clamp_grads(const eegnet_dims* dims, float* grads, void* stream);

/* Eval-mode forward (running statistics, no dropout): one fused kernel.  model.py:161/220, ui.py:35. */
int eegnet_forward_eval(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                        const float* x, float* logits, void* stream);

/* Seed of eegnet_input_grad_eval: the per-trial gradient g[4] with respect to the logits. */
enum { EEGNET_SEED_DLOGITS = 0,  /* g = dlogits[b]                                   */
       EEGNET_SEED_LOGIT   = 1,  /* g = onehot(targets[b]); targets NULL: the trial's */
                                 /*     own argmax (lowest index on a tie)            */
       EEGNET_SEED_CE      = 2 };/* g = softmax(logits[b]) - onehot(targets[b])       */
                                 /*     (per-trial CE, reduction "sum")               */

/* Eval-mode input gradient (saliency): dx[b] = d(g[b] . logits[b]) / dx[b] with running statistics and
 * no dropout, so every trial is independent.  One fused kernel runs the forward of eegnet_forward_eval
 * and its transposed chain per trial without leaving the CU; the logits it computes on the way are
 * written to `logits` [B,4] when non-NULL.  dlogits [B,4] is read for EEGNET_SEED_DLOGITS only; targets
 * int64 [B] is required for EEGNET_SEED_CE and optional for EEGNET_SEED_LOGIT.  dx is [B,C,T] fp32
 * (any 4-byte alignment; no byte outside it is written); x is 16-byte aligned when T % 4 == 0, and
 * x_pitch must be 0 or T.  F1*D <= 16 only
 * (wide dims return EEGNET_EINVAL); gradients of train-mode BatchNorm are not provided.  The
 * validation needs no GPU. */
int eegnet_input_grad_eval(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                           const float* x, int seed_kind, const float* dlogits,
                           const int64_t* targets, float* dx, float* logits, void* stream);

/* Frozen-BatchNorm fine-tuning: train mode with the three BatchNorm layers frozen, as bn.eval() on a
 * stock module -- running statistics used and never written (bn_buffers is const, there is no
 * num_batches_tracked argument), dropout applied as in the train path (masks or the (seed, offset)
 * generator).  Every trial is then independent: one fused kernel runs forward, loss, backward and all
 * 12 parameter gradients of a trial on one CU and leaves one partial row per workgroup in `ws`; a small
 * second kernel sums the rows in workgroup order (fp64), clamps and writes `grads` / `loss`.  No
 * atomics: the same inputs give the same bits.  F1*D <= 16 only, x_pitch 0 or T, x 16-byte aligned when
 * T % 4 == 0; the shapes eegnet_input_grad_eval takes.  The validation needs no GPU.
 *
 * eegnet_frozen_workspace_bytes: bytes of `ws` (the partial rows; zero-fill it once, as the other
 * workspaces).
 * eegnet_forward_frozen: the logits alone (the autograd forward).
 * eegnet_frozen_step: exactly one of dlogits [B,4] (autograd) and labels (mean cross-entropy; the loss
 * goes to `loss`, device fp32, nullable).  adam_state == NULL stops after the gradients; otherwise the
 * Adam kernel of eegnet_adam_step is enqueued behind the reduction on the same stream (adam_state, step
 * as for eegnet_train_step).  flags: EEGNET_NO_CLAMP, EEGNET_KEY_FROM_STEP (needs step); any other bit
 * is EEGNET_EINVAL.  logits is nullable.  No host synchronisation: capturable in a hipGraph. */
int eegnet_frozen_workspace_bytes(const eegnet_dims* dims, size_t* out);
int eegnet_forward_frozen(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                          const float* x, const uint8_t* mask2, const uint8_t* mask3, uint64_t seed,
                          uint64_t offset, float* logits, void* stream);
int eegnet_frozen_step(const eegnet_dims* dims, float* params, const float* bn_buffers, const float* x,
                       const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                       const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads,
                       float* adam_state, int32_t* step, float lr, float beta1, float beta2, float eps,
                       float* loss, float* logits, void* ws, void* stream, int flags);

/* Partial fine-tuning: the frozen-BatchNorm step that trains a suffix of the layers.  train_from names the
 * first trainable module in network order; every module before it is frozen.  The flat parameter layout is
 * in network order, so the trainable set is the suffix [off, param_count) of params / grads and of both
 * halves of adam_state, with off = eegnet_trainable_offset(dims, train_from):
 *   EEGNET_TRAIN_ALL               nothing frozen                                        off = 0
 *   EEGNET_TRAIN_FROM_AGGREGATION  temporal.0, temporal.1, spatial frozen                aggregation.0.weight
 *   EEGNET_TRAIN_FROM_BLOCK2       ... and aggregation.0 (gamma2, beta2)                 block_2.0.weight
 *   EEGNET_TRAIN_FROM_CLASSIFIER   ... and block_2.0, block_2.1, block_2.2               classifier.weight
 * (a cut at `spatial` is not offered: it still needs the whole block-1 backward but the temporal lag
 * correlation.)  The backward of a trial stops where the trainable layers stop, so a later cut is cheaper.
 *
 * eegnet_frozen_step_from / eegnet_frozen_step_folds_from take the arguments of eegnet_frozen_step /
 * eegnet_frozen_step_folds (same flags, same pointer checks, same workspace) and train_from:
 *   - train_from = EEGNET_TRAIN_ALL is the existing call, bit for bit (the same kernels);
 *   - otherwise grads[0 : off), params[0 : off) and both Adam moments of the prefix are never written;
 *   - grads[off :), loss and logits are bit-identical to the full step on the same inputs; Adam runs on the
 *     suffix alone and the step counter advances as in the full step;
 *   - the content of ws before the call does not matter (as for the full step);
 *   - a train_from outside 0..3 is EEGNET_EINVAL, wide dims (F1*D > 16) are rejected as by
 *     eegnet_frozen_step.  All validation works without a GPU; capturable in a hipGraph.
 * For the fold call train_from is shared by every fold. */
enum { EEGNET_TRAIN_ALL = 0, EEGNET_TRAIN_FROM_AGGREGATION = 1,
       EEGNET_TRAIN_FROM_BLOCK2 = 2, EEGNET_TRAIN_FROM_CLASSIFIER = 3 };
int eegnet_trainable_offset(const eegnet_dims* dims, int train_from, int64_t* out);
int eegnet_frozen_step_from(const eegnet_dims* dims, float* params, const float* bn_buffers, const float* x,
                            const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                            const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads,
                            float* adam_state, int32_t* step, float lr, float beta1, float beta2, float eps,
                            float* loss, float* logits, void* ws, void* stream, int flags, int train_from);

/* bf16 batched eval-mode forward (BASELINE cfg5, EEGNet-16,4 at 64ch x 512):
 * the same function as eegnet_forward_eval (model.py:91-99 in .eval(), called at model.py:161/220,
 * ui.py:35) on bf16 input x [B,C,T] (16-byte aligned when T % 8 == 0), bf16 MFMA operands and fp32
 * accumulation; params / bn_buffers / logits as for eegnet_forward_eval (fp32).  Covers every
 * supported (C, T, F1, D) whose trial fits one workgroup's LDS, including the F2 > 16 shapes the
 * fp32 path runs through the wide kernels. */
int eegnet_forward_eval_bf16(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                             const uint16_t* x, float* logits, void* stream);

/* torch.optim.Adam step (weight_decay 0, amsgrad off) over n elements; `step` is a device int32
 * that is incremented in-kernel (graph-capturable).  torch/optim/adam.py:457,476,531-547. */
int eegnet_adam_step(int64_t n, float* params, const float* grads, float* exp_avg,
                     float* exp_avg_sq, int32_t* step, float lr, float beta1, float beta2,
                     float eps, void* stream);

/* One fused hot-loop iteration (model.py:141-148): forward_train + CE + backward + clamps + Adam.
 * adam_state = [exp_avg | exp_avg_sq] (2 * param_count floats); step as in eegnet_adam_step.
 * adam_state == NULL stops after the gradients (data-parallel callers all-reduce them, then call
 * eegnet_clamp_grads and eegnet_adam_step); flags as for eegnet_backward, plus EEGNET_KEY_FROM_STEP
 * (needs step; the mask key then follows the device step, for hipGraph capture).  logits is nullable. */
int eegnet_train_step(const eegnet_dims* dims, float* params, float* bn_buffers, const float* x,
                      const int64_t* labels, uint64_t seed, uint64_t offset, float* grads,
                      float* adam_state, int32_t* step, float lr, float beta1, float beta2,
                      float eps, float* loss, float* logits, void* ws, void* stream, int flags,
                      int64_t* num_batches_tracked);

/* One stage of a data-parallel train step with synchronised BatchNorm (SURVEY 8(e)2's SyncBN option;
 * the reference has no multi-device path -- this is the single-device semantics of model.py:141-148
 * over the global batch, split at the five batch-global reductions so a caller can all-reduce each).
 * stage 2k (k = 0..4: passes A..E) launches pass k and leaves its fp64 sums in the workspace
 * (eegnet_stage_sums says where) instead of finalizing; stage 2k + 1 runs pass k's finalize on those
 * sums once the caller has summed them over the ranks (all_reduce SUM).  norm_batch = the global batch:
 * BatchNorm statistics, running statistics and the CE mean are normalised by it, so the gradients,
 * clamps (model.py:44/84, on the global gradient) and the fused Adam of stage 9 come out the same on
 * every rank and no separate gradient all-reduce is needed.  Other arguments as for eegnet_train_step
 * (adam_state NULL: gradients only).  F1*D <= 16 only. */
int eegnet_train_stage(const eegnet_dims* dims, int stage, int64_t norm_batch, float* params,
                       float* bn_buffers, const float* x, const int64_t* labels, uint64_t seed,
                       uint64_t offset, float* grads, float* adam_state, int32_t* step, float lr,
                       float beta1, float beta2, float eps, float* loss, void* ws, void* stream,
                       int flags, int64_t* num_batches_tracked);

/* Where stage 2k leaves pass k's sums in a workspace of eegnet_workspace_bytes(dims): byte offset and
 * number of fp64 values (the buffer a synchronised-BatchNorm caller all-reduces). */
int eegnet_stage_sums(const eegnet_dims* dims, int pass, size_t* offset_bytes, int* count);

/* One model (fold) of a fold-indexed train step: everything eegnet_train_step takes per model.
 * Every pointer is a device pointer; an array of these lives in DEVICE memory. */
typedef struct eegnet_fold {
    float* params;                  /* flat parameters (named_parameters order)                   */
    float* bn_buffers;              /* rm1 rv1 rm2 rv2 rm3 rv3                                    */
    int64_t* num_batches_tracked;   /* int64[3] or NULL                                           */
    const float* x;                 /* this fold's epoch data [N, C, T], rows already shuffled    */
    const int64_t* labels;          /* [N]                                                        */
    float* grads;                   /* flat gradients (written)                                   */
    float* adam_state;              /* [exp_avg | exp_avg_sq]                                     */
    int32_t* step;                  /* Adam step counter (device int32)                           */
    float* losses;                  /* per-batch loss slots (NULL: not written)                   */
    void* ws;                       /* workspace of eegnet_workspace_bytes(dims), zeroed once     */
    const int64_t* perm;            /* epoch permutation: batch row r is x / labels row perm[r]   */
                                    /* (NULL: row r itself, i.e. x already shuffled)              */
    uint64_t seed;                  /* dropout key seed: key = mix(seed, offset + *step)          */
    const float* xstat;             /* NULL, or eegnet_x_stats(x) of this fold's x: its rows' BN1  */
                                    /* lag sums, read instead of recomputed every epoch (ABI 5:   */
                                    /* appended after seed, so the round-3 fields keep offsets)   */
} eegnet_fold;

/* The hot-loop iteration of eegnet_train_step (forward + CE + backward + clamps + Adam) for
 * `nfolds` independent models in ONE launch per pass: the fold index is the grid's y dimension,
 * each fold keeps its own parameters, BN buffers, Adam state, workspace and reductions.  Replaces
 * the per-fold loops of train.py:50-140 (within-subject, 36 runs) and train.py:182-290
 * (cross-subject, 90 runs) at batch 64 (train.py:87,229), where one model's step cannot fill the
 * GPU.  All folds train on batch [row0, row0 + dims.B) of their own x / labels -- rows
 * perm[row0 ...] of x / labels when the fold has a perm (the epoch's shuffle without a gather of
 * the trials) -- and the loss goes to losses[slot].  Dropout keys follow each fold's device step (EEGNET_KEY_FROM_STEP semantics with
 * `offset`), so a captured graph draws fresh masks on every replay.  F1*D <= 16 only. */
int eegnet_train_step_folds(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds, int64_t row0,
                            int64_t slot, uint64_t offset, float lr, float beta1, float beta2, float eps,
                            void* stream);

/* eegnet_frozen_step (forward with running statistics and dropout, mean CE, backward, all 12 gradients
 * with both clamps, Adam) for `nfolds` independent models in four launches, whatever nfolds: the fold
 * index is the grid's y dimension.  `folds` is a DEVICE array of eegnet_fold, the record of
 * eegnet_train_step_folds unchanged.  Per fold: params (updated by Adam), bn_buffers (read, never
 * written), x [N, C, T] contiguous (x_pitch 0 or T; 16-byte aligned when T % 4 == 0 -- the host never
 * reads the table, so this is not checked), labels, perm (batch row r is row perm[row0 + r] of x /
 * labels; NULL: row row0 + r), grads (written), adam_state and step (adam_state == NULL: the fold stops
 * after its gradients and its step is not advanced), losses (the mean CE goes to losses[slot]; NULL: not
 * written), ws (eegnet_frozen_workspace_bytes(dims) bytes of its own) and seed.  num_batches_tracked and
 * xstat are ignored and never dereferenced.  The dropout key of a fold is mix(seed, offset + *step), read
 * on the device (EEGNET_KEY_FROM_STEP semantics: a captured graph draws fresh masks at every replay);
 * dims->p_drop is shared.  flags: 0 or EEGNET_NO_CLAMP; any other bit is EEGNET_EINVAL.
 * The per-fold grid is eegnet_frozen_step's for the same dims -- a function of dims->B alone, never of
 * nfolds -- so every output of a fold is bit-identical to eegnet_frozen_step with EEGNET_KEY_FROM_STEP,
 * the same (seed, offset) and the batch's rows gathered, on that fold alone, wherever it stands in the
 * table.  No atomics, no host synchronisation: capturable in a hipGraph.  1 <= nfolds <= 65535, row0 and
 * slot >= 0, F1*D <= 16 only; the validation needs no GPU. */
int eegnet_frozen_step_folds(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds,
                             int64_t row0, int64_t slot, uint64_t offset,
                             float lr, float beta1, float beta2, float eps,
                             int flags, void* stream);
/* eegnet_frozen_step_folds training the suffix train_from of every fold (see eegnet_frozen_step_from):
 * per fold bit-identical to eegnet_frozen_step_from with the same train_from on that fold alone. */
int eegnet_frozen_step_folds_from(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds,
                                  int64_t row0, int64_t slot, uint64_t offset,
                                  float lr, float beta1, float beta2, float eps,
                                  int flags, void* stream, int train_from);

/* One model (fold) of a fold-indexed validation call.  Every pointer is a device pointer; an array of
 * these lives in DEVICE memory.  Nothing in it is written except through logits, ce, pred, loss and
 * correct. */
typedef struct eegnet_eval_fold {
    const float* params;       /* flat parameters                                  */
    const float* bn_buffers;   /* rm1 rv1 rm2 rv2 rm3 rv3 (read only)              */
    const float* x;            /* [n, C, T] contiguous; folds may share one        */
    const int64_t* labels;     /* [n] in [0,4); NULL: logits / pred only           */
    int64_t n;                 /* trials of this fold (0: nothing read, loss 0, correct 0) */
    float* logits;             /* [n,4] or NULL                                    */
    float* ce;                 /* [n] per-trial CE; required when labels != NULL   */
    int32_t* pred;             /* [n] argmax; required when labels != NULL         */
    double* loss;              /* loss[slot] (needs labels) or NULL                */
    int64_t* correct;          /* correct[slot] (needs labels) or NULL             */
} eegnet_eval_fold;

/* Validation of `nfolds` independent models, each on its own held-out set, as model.py:151-172 computes
 * it after every epoch: the eval-mode forward of eegnet_forward_eval per trial (the same per-trial code:
 * a fold's logits are bit-identical to that call on the fold alone), the trial's cross-entropy
 * ce[i] = logsumexp(logits[i]) - logits[i][labels[i]] and its prediction pred[i] (argmax, the lowest
 * index on a tie) in one launch over every fold's trials; then, one workgroup per fold,
 *     loss[slot]    = (1/nb) sum_j mean_{i in batch j} ce[i],  nb = ceil(n / batch)
 *                     (batches of `batch` consecutive trials, the last one short; fp64, index order:
 *                     running_val_loss / len(val_loader))
 *     correct[slot] = #{i : pred[i] == labels[i]}.
 * `folds` is a DEVICE array the host never reads; max_n, 0 <= max_n <= 2^31, must be the largest n in it
 * (it sizes the grid: trials at or beyond max_n would not be evaluated).  dims->B is ignored.
 * batch >= 1; batch >= n makes the loss a plain mean.  Each output is written only when its pointer is non-NULL (ce, loss and correct
 * also need labels; a fold with n = 0 reads none of its pointers and reports loss 0, correct 0 with or
 * without them).  No atomics: the same inputs give the same bits.  F1*D <= 16 only, x_pitch 0 or T, x
 * 16-byte aligned when T % 4 == 0; the shapes eegnet_train_step_folds takes.  No host synchronisation:
 * capturable in a hipGraph.  The validation needs no GPU. */
int eegnet_eval_folds(const eegnet_dims* dims, int nfolds, const eegnet_eval_fold* folds,
                      int64_t max_n, int batch, int64_t slot, void* stream);

/* Sliding-window inference over continuous recordings, read in place (pseudo-online decoding, cropped
 * evaluation).  `rec` holds n_rec recordings of dims->C channel rows: row (r, c) starts at
 * rec + (r*C + c)*pitch and has n_samples valid floats, pitch >= n_samples (a time slice of a larger
 * buffer is passed in place); rec may have any 4-byte alignment, and no byte outside
 * [row start, row start + n_samples) of a row is read.  Window w of recording r is samples
 * [w*hop, w*hop + T) of each of its rows, w < W = (n_samples - T)/hop + 1 (eegnet_window_count; host only).
 *   logits [n_rec, W, 4]  required: logits[r, w] is bit-identical to eegnet_forward_eval on that window
 *                         copied out as one [1, C, T] trial
 *   probs  [n_rec, 4]     nullable, fp32: mean_w softmax(logits[r, w]), the softmax and the sum in fp64 in
 *                         window-index order with a fixed reduction shape
 *   pred   [n_rec]        nullable: the argmax of that fp64 mean, the lowest index on a tie (it does not
 *                         need probs)
 * One launch over all n_rec*W windows, and one more (a workgroup per recording) when probs or pred is
 * asked for.  No atomics: the same inputs give the same bits.  dims->B is ignored; x_pitch must be 0 or
 * T; hop >= 1, n_rec >= 1, n_samples >= T; n_rec*W must be a batch eegnet_forward_eval takes for these
 * dims; F1*D <= 16 only.  No host synchronisation and no allocation: capturable in a hipGraph.  The
 * validation needs no GPU. */
int eegnet_window_count(const eegnet_dims* dims, int64_t n_samples, int64_t hop, int64_t* out);
int eegnet_forward_eval_windows(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                                const float* rec, int64_t n_rec, int64_t n_samples, int64_t pitch,
                                int64_t hop, float* logits, float* probs, int32_t* pred, void* stream);

/* Cue epoching in place: the eval forward of n_windows windows whose origins come from a table instead of
 * w*hop.  `rec`, n_rec, n_samples and pitch are eegnet_forward_eval_windows's.  starts, int64 [n_windows], and
 * rec_index, int32 [n_windows] (nullable: every window is of recording 0), are DEVICE arrays the host never
 * reads: window w is samples [starts[w], starts[w] + T) of recording rec_index[w], and logits[w] (fp32
 * [n_windows, 4]) is bit-identical to eegnet_forward_eval on that window copied out as one [1, C, T] trial.
 * The kernel clamps a start into [0, n_samples - T] and a recording index into [0, n_rec): no table makes it
 * read outside the recordings (an out-of-range entry gives the logits of the clamped window; callers that
 * want an error check the table on the host, as the Python side does for host tables).  The load width is
 * chosen per window on the device; the bits do not depend on it.  dims->B is ignored; x_pitch must be 0 or T;
 * n_rec >= 1, n_samples >= T, 1 <= n_windows, and n_windows must be a batch eegnet_forward_eval takes;
 * F1*D <= 16 only.  One launch, no atomics, no allocation, no host synchronisation: capturable in a hipGraph.
 * The validation needs no GPU. */
int eegnet_forward_eval_windows_at(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                                   const float* rec, int64_t n_rec, int64_t n_samples, int64_t pitch,
                                   const int64_t* starts, const int32_t* rec_index, int64_t n_windows,
                                   float* logits, void* stream);

/* Fine-tuning on cue epochs read in place: eegnet_frozen_step_from on windows of continuous recordings that
 * a table places, without copying them out.  `rec`, n_rec, n_samples, pitch, starts and rec_index are
 * eegnet_forward_eval_windows_at's, the table having n_table entries; dims->B is the batch, the windows of
 * this step.  Batch row b is table entry e = sel ? clamp(sel[b], 0, n_table - 1) : b (sel: int64 [B], DEVICE,
 * nullable; B <= n_table without it): its x is samples [starts[e], starts[e] + T) of recording rec_index[e],
 * both clamped into the recordings as in eegnet_forward_eval_windows_at, and its mean-CE label is labels[e]
 * (labels: int64 [n_table]).  dlogits [B, 4], logits [B, 4], mask2 / mask3 and the dropout counters are
 * indexed by the batch row b.  Exactly one of labels and dlogits is given; every other argument, the flags,
 * train_from and ws (eegnet_frozen_workspace_bytes(dims)) are eegnet_frozen_step_from's.
 * Every output -- grads on the trainable suffix, loss, logits, params and both Adam moments after the update,
 * the step counter -- is bit-identical to eegnet_frozen_step_from on the batch's windows copied out into a
 * contiguous [B, C, T] x with the labels gathered, for the same (seed, offset) or masks, flags and train_from.
 * rec needs 4-byte alignment only (the load width is chosen per window on the device) and is never written;
 * the host never reads a table.  n_rec and n_table in [1, 2^31), n_samples >= T, pitch >= n_samples, tables
 * aligned to their element size, x_pitch 0 or T, F1*D <= 16 only.  No atomics, no allocation, no host
 * synchronisation: capturable in a hipGraph.  The validation needs no GPU. */
int eegnet_frozen_step_windows(const eegnet_dims* dims, float* params, const float* bn_buffers,
                               const float* rec, int64_t n_rec, int64_t n_samples, int64_t pitch,
                               const int64_t* starts, const int32_t* rec_index, const int64_t* labels,
                               int64_t n_table, const int64_t* sel,
                               const float* dlogits, const uint8_t* mask2, const uint8_t* mask3, uint64_t seed,
                               uint64_t offset, float* grads, float* adam_state, int32_t* step, float lr,
                               float beta1, float beta2, float eps, float* loss, float* logits, void* ws,
                               void* stream, int flags, int train_from);

/* FIR filtering of continuous recordings: the reference's zero-phase band-pass (raw.filter(4., 38.,
 * fir_design='firwin'), dataset.py:113-125; a 213-tap FIR at 128 Hz) for any taps, the step in front of
 * eegnet_ems.  Per row, with taps h[0..L-1] (fp64, on the device; L = n_taps) and M = (L-1)/2,
 *     y[t] = sum_{k=0..L-1} h[k] u[t + M - k]
 * with u the row extended past the recording's ends as mne's 'reflect_limited' padding extends it:
 * u[-j] = 2 x[0] - x[j] and u[N-1+j] = 2 x[N-1] - x[N-1-j] for 1 <= j <= min(M, N-1), zero beyond.  All
 * arithmetic is fp64 -- one fused multiply-add per tap in the order k = 0..L-1 from a zero start -- and y is
 * rounded to fp32 once.  An output's value is a function of the taps and of its L values of u alone: not of
 * the chunking, of n_rows, of a pitch or an alignment, nor of the mode that produced it.
 *   EEGNET_FIR_WHOLE  the zero-phase call on whole rows: n_samples >= 1 in, n_samples out; both ends reflect.
 *   EEGNET_FIR_FIRST  a stream's first block: n_samples >= L in, the n_samples - M outputs whose right
 *                     support is present out (outputs 0 .. n_samples-M-1 of the recording); the left end
 *                     reflects; hist_out receives the block's last L-1 samples as fp64 [n_rows][L-1].
 *   EEGNET_FIR_NEXT   a continuation: n_samples >= 1 in, n_samples out, lagging the input by M samples (the
 *                     first output is the one M samples before the block's first sample); the left context is
 *                     hist_in, and hist_out receives the last L-1 samples of history + block.  A block shorter
 *                     than L-1 leaves a history that is part old history, part block; hist_out must not be
 *                     hist_in (the caller ping-pongs two buffers).  Takes an even L as well.
 *   EEGNET_FIR_TAIL   the stream's end: n_samples = 0 (x is not read and may be NULL), the last M outputs of
 *                     the recording out, the right end reflected about the last sample of hist_in.
 * The outputs of FIRST, NEXT.. and TAIL laid end to end are the WHOLE call's on the concatenated blocks, bit
 * for bit.  x holds n_rows rows of n_samples valid elements, fp32 or fp64 (x_is_f64), row i at x + i*x_pitch
 * elements, any 4- / 8-byte alignment (a time slice of a larger buffer is passed as it lies); y is fp32, row i
 * at y + i*y_pitch; x_pitch >= n_samples, y_pitch >= the outputs of a row.  No byte outside a row's valid
 * samples is read and none outside its outputs is written.  Filtering in place is not supported: a call whose
 * y rows' bounding byte range meets the x rows' is rejected.  1 <= n_taps <= eegnet_fir_max_taps() (2049);
 * WHOLE, FIRST and TAIL need an odd n_taps.  One workgroup per row and chunk of eegnet_fir_chunk() outputs
 * (both compile-time constants, host only); n_rows * chunks <= 2^31 - 1.  One launch for the outputs and one
 * for the history, on `stream`; no atomics, no allocation, no host synchronisation: capturable in a hipGraph.
 * The validation needs no GPU. */
enum { EEGNET_FIR_WHOLE = 0, EEGNET_FIR_FIRST = 1, EEGNET_FIR_NEXT = 2, EEGNET_FIR_TAIL = 3 };
int eegnet_fir_max_taps(void);
int eegnet_fir_chunk(void);
int eegnet_fir(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch,
               const double* taps, int n_taps, float* y, int64_t y_pitch, const double* hist_in,
               double* hist_out, int mode, void* stream);

/* Rational polyphase resampling up/down of continuous recordings: scipy.signal.resample_poly, mne's
 * method="polyphase".  This is NOT the method the reference's raw.resample(128, npad="auto") defaults to (mne's
 * FFT method, a DFT of the whole padded recording, which cannot stream); the two differ at the recording's
 * ends and by the anti-alias filter's response (DESIGN.md 4.8 has the measured difference after the band-pass).
 * up/down is reduced by its gcd first (128/250 -> 64/125).  Per row of N samples, with the prototype taps
 * h[0..L-1] (fp64, on the device; L = n_taps = 2 half + 1), Q = half / up and c = m down + half, output m of the
 * ceil(N up / down) is
 *     y[m] = sum_{n = ceil((c - 2 half) / up) .. floor(c / up)} h[c - n up] u[n]
 * added in the order of ascending tap index c - n up by one fp64 fused multiply-add per term from a zero start
 * (at most ceil(L / up) terms) and rounded to fp32 once.  u is the row extended past its ends by `ends`:
 *   EEGNET_RESAMPLE_ENDS_ZERO     u = 0 outside [0, N): resample_poly's default padtype='constant'
 *   EEGNET_RESAMPLE_ENDS_REFLECT  the band-pass's odd reflection: u[-j] = 2 x[0] - x[j], u[N-1+j] = 2 x[N-1] - x[N-1-j]
 *                                 for 1 <= j <= min(Q + 1, N - 1), zero beyond (no output reaches further)
 * An output's value is a function of the taps and of the values of u in its support alone: not of the chunking,
 * of n_rows, of a pitch or an alignment, nor of the mode that produced it.  n_before is the number of samples of
 * the recording consumed before this block; it alone decides which outputs m of the recording the call emits,
 * and their phases come from m.  With done(t) = the outputs m with m down + half < t up (whole support within
 * the first t samples):
 *   EEGNET_RESAMPLE_WHOLE  whole rows: n_samples >= 1 in, ceil(n_samples up / down) out; n_before = 0.
 *   EEGNET_RESAMPLE_FIRST  a stream's first block: n_samples >= Q + 2 in (the head's reflection is the block's
 *                          own), outputs 0 .. done(n_samples) - 1 out; n_before = 0; hist_out receives the
 *                          last 2 Q + 2 values of u as fp64 [n_rows][2 Q + 2].
 *   EEGNET_RESAMPLE_NEXT   a continuation: n_samples >= 1 in, outputs done(n_before) .. done(n_before +
 *                          n_samples) - 1 out (none, for a short block, is a valid count); the left context is
 *                          hist_in, hist_out receives the last 2 Q + 2 values of history + block; hist_out must
 *                          not be hist_in (the caller ping-pongs two buffers).
 *   EEGNET_RESAMPLE_TAIL   the stream's end: n_samples = 0 (x is not read and may be NULL), n_before = N, outputs
 *                          done(N) .. ceil(N up / down) - 1 out, the right end extended from hist_in.
 * The outputs of FIRST, NEXT.. and TAIL laid end to end are the WHOLE call's on the concatenated blocks, bit for
 * bit.  eegnet_resample_count returns in *n_out the outputs per row a call with these integers writes (host only;
 * it validates them as eegnet_resample does).  x, y, the pitches, the alignment and the overlap rule are
 * eegnet_fir's: x fp32 or fp64 at any element alignment, y fp32, x_pitch >= n_samples, y_pitch >= the outputs of a
 * row, no byte outside a row's valid samples read, none outside its outputs written, and a y that overlaps x
 * rejected.  n_taps is odd and <= eegnet_resample_max_taps() (4097); the reduced up is <= eegnet_resample_max_up()
 * (256), the reduced down <= 2^20, up != down; (n_before + n_samples) max(up, down) <= 2^61.  One workgroup per
 * row and chunk of outputs, the chunk sized by the host to the LDS; n_rows * chunks <= 2^31 - 1.  One launch for
 * the outputs and one for the history, on `stream`; no atomics, no allocation, no host synchronisation:
 * capturable in a hipGraph.  The validation needs no GPU. */
enum { EEGNET_RESAMPLE_WHOLE = 0, EEGNET_RESAMPLE_FIRST = 1, EEGNET_RESAMPLE_NEXT = 2, EEGNET_RESAMPLE_TAIL = 3 };
enum { EEGNET_RESAMPLE_ENDS_ZERO = 0, EEGNET_RESAMPLE_ENDS_REFLECT = 1 };
int eegnet_resample_max_taps(void);
int eegnet_resample_max_up(void);
/* the outputs of one workgroup of a call with this prototype and ratio (> 0), or a negative EEGNET_E* (host only) */
int eegnet_resample_chunk(int n_taps, int up, int down);
int eegnet_resample_count(int64_t n_samples, int64_t n_before, int n_taps, int up, int down, int mode,
                          int64_t* n_out);
int eegnet_resample(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch,
                    const double* taps, int n_taps, int up, int down, int ends, float* y, int64_t y_pitch,
                    int64_t n_before, const double* hist_in, double* hist_out, int mode, void* stream);

/* Exponential moving standardisation of continuous recordings: the reference's
 * raw_exponential_moving_standardize (dataset.py:45-70), the step in front of eegnet_forward_eval_windows.
 * Per row, with a = factor_new:
 *     m_t = (1-a) m_{t-1} + a x_t,  v_t = (1-a) v_{t-1} + a (x_t - m_t)^2,  y_t = (x_t - m_t) / sqrt(v_t + eps)
 * x holds n_rows rows (recordings x channels) of n_samples valid elements, fp32 or fp64 (x_is_f64), row i at
 * x + i*x_pitch elements; y is fp32, row i at y + i*y_pitch; both pitches >= n_samples.  x may have any
 * 4-byte (fp32) or 8-byte (fp64) alignment; no byte outside [row start, row start + n_samples) of a row is
 * read and none outside y's valid samples is written.  y may be x itself (same pointer, same pitch, fp32
 * input only); any other overlap of x and y is not supported.
 *   resume = 0: (m, v) start as the mean and the population variance of the row's first
 *               min(init_block, n_samples) samples (numpy's clamped slice)
 *   resume = 1: (m, v) start from state[i] = (mean, var), which is then required: a recording fed block by
 *               block (a pseudo-online decoder's standardiser)
 * state, fp64 [n_rows][2], is nullable when not resuming; when non-NULL it receives every row's final (m, v).
 * A blocked scan over time in three launches ordered by the stream alone (chunk aggregates, carries, output):
 * all arithmetic fp64, y rounded to fp32 once, no atomics, no workgroup waits on another -- the same inputs
 * give the same bits.  scratch: eegnet_ems_scratch_bytes(n_rows, n_samples) bytes, 8-byte aligned, content
 * irrelevant.  eegnet_ems_chunk: the samples of one chunk of the scan (a compile-time constant).
 * n_rows >= 1, n_samples >= 1, 0 < factor_new < 1, eps >= 0, init_block >= 1 when not resuming, and
 * n_rows * ceil(n_samples / chunk) <= 2^31 - 1 workgroups.  No allocation and no host synchronisation:
 * capturable in a hipGraph.  The validation needs no GPU; eegnet_ems_chunk and eegnet_ems_scratch_bytes are
 * host only. */
int eegnet_ems_chunk(void);
int eegnet_ems_scratch_bytes(int64_t n_rows, int64_t n_samples, size_t* out);
int eegnet_ems(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch,
               float* y, int64_t y_pitch, double factor_new, int64_t init_block, double eps,
               double* state, int resume, void* scratch, void* stream);

/* Per-trial BatchNorm-1 statistics of x that do not depend on the parameters: for each of the n
 * trials x[i] ([C][T] rows at dims->x_pitch), the lag sums of its zero-padded rows summed over the
 * channels G0[d] (d < K1), the window-0 sample sum, and the head / tail products and sums of the
 * 'same' padding's edges -- eegnet_x_stats_width(dims) floats per trial, written to out[n][width].
 * BN1's batch statistics (model.py:32) are w1-quadratic forms of their sums over the batch
 * (DESIGN.md section 3), so a fold whose training set is fixed for all epochs (train.py:87-106,
 * 225-246) computes them once and its fold-indexed steps read the batch's rows through eegnet_fold.
 * xstat instead of recomputing the lag-Gram (180 K of pass A's 423 K MAC per 22 x 256 trial).  The
 * narrow path (F1*D <= 16) only; dims->B is ignored. */
int eegnet_x_stats_width(const eegnet_dims* dims);
int eegnet_x_stats(const eegnet_dims* dims, int64_t n, const float* x, float* out, void* stream);

/* Optional per-kernel device timing for benchmarks: `on` is a bitmask of kernel ids (bit i = the
 * i-th name eegnet_profile_collect reports: k_pass_a, k_pass_b, k_pass_c, k_pass_d, k_pass_e,
 * k_adam, k_infer, memset_tickets, k_infer_bf16, k_wpass_a, k_wpass_b, k_wpass_b2, k_wpass_c,
 * k_wpass_d, k_wpass_e, k_winfer, k_coltail, k_xstats, k_infer_dx; -1 = all, 0 = off; the k_w* kernels are the F2 > 16 path).  Every selected kernel this
 * thread launches through the calls above is bracketed by hipEvents.  eegnet_profile_collect
 * synchronises them and reports, per kernel name (32-byte slots in `names`), launch count and
 * summed device ms; it returns the number of kernels in *n_out.  Not for use under hipGraph
 * capture.  Each bracketed launch costs a few microseconds of stream time, so a benchmark's timed
 * region should select only the kernel it prices. */
int eegnet_profile_enable(int on);
int eegnet_profile_collect(char* names, int* counts, double* total_ms, int cap, int* n_out);

/* Optional timeline instrumentation for kernel tuning: while `buf` (a zeroed device buffer of
 * eegnet_trace_bytes() bytes) is set, every pass kernel stamps phase boundaries into it
 * ([pass][workgroup][16] uint64: wall clock at entry / prologue / loop end / publish / tickets /
 * finalize, shader-clock sums of in-loop phases).  NULL turns it off. */
int eegnet_trace_enable(void* buf);
size_t eegnet_trace_bytes(void);

/* The x row pitch the training entry points (eegnet_train_step, _folds, _forward_train, _backward,
 * _train_stage) load fastest for `dims`: T rounded up to 4 floats when the kernels for these dims take
 * x rows in 16-byte units at such a pitch (22 x 257, the recordings' shape: a 257-float row is not
 * 16-byte aligned), else T.  Only those dims accept a pitch other than T (22 x 256 rows are 16-byte
 * units already; its kernels have the pitch T compiled in).  Every other entry point needs x_pitch = 0
 * or T.  No GPU needed. */
int eegnet_x_pitch(const eegnet_dims* dims);

/* How the launches split a batch of dims->B trials over workgroups: out[0..4] = the number of trial
 * ranges of passes A, B, C, D, E of the train step, out[5] = of the eval forward (eegnet_forward_eval).
 * A range is the set of trials one workgroup runs: contiguous rows [r B / n, (r + 1) B / n), one after
 * the other, in the streaming passes (A, B, E, and D for F1*D <= 16); rows r, r + n, ... in the eval
 * forward and the F1*D > 16 block-2 passes -- floor(B / n) or ceil(B / n) trials either way.  Pass C
 * for F1*D <= 16 deals its trials to the w waves of its g workgroups (workgroup r, wave i: rows
 * r w + i, + g w, ...): out[2] counts those per-wave streams, n = g w, each wave running its rows one
 * after the other.  For F1*D > 16 the streaming passes (A, B's BN2 / ELU half,
 * E) run ceil(F1*D / 16) chunk workgroups per range and the count is workgroups / chunks; pass B's
 * block-2 half runs pass C's grid.  fold_launch != 0: the per-fold grids of eegnet_train_step_folds
 * (F1*D <= 16; a function of dims->B alone, never of nfolds) and out[5] = 0.  Filled by the geometry
 * code the launches themselves use; no launch, no allocation.  No GPU needed (256 CUs are assumed
 * without one). */
int eegnet_launch_grids(const eegnet_dims* dims, int fold_launch, int out[6]);

/* 1 when `dims` run the wide kernels compiled for the EEGNet-16,4 64 x 512 geometry (compile-time
 * bounds and offsets), 0 when they run the generic wide / narrow kernels, < 0 on invalid dims.  No GPU
 * needed. */
int eegnet_wide_spec(const eegnet_dims* dims);

/* sizeof(eegnet_dims), sizeof(eegnet_fold) and sizeof(eegnet_eval_fold) as this library was compiled: a
 * binding checks its struct mirrors against them at load (a stale library with another fold layout
 * would read every fold after the first from the wrong offsets). */
size_t eegnet_dims_bytes(void);
size_t eegnet_fold_bytes(void);
size_t eegnet_eval_fold_bytes(void);

/* The struct layouts above are versioned: EEGNET_ABI_VERSION changes whenever a field of eegnet_dims
 * or eegnet_fold moves (a reordering keeps the size, so eegnet_fold_bytes alone cannot catch it).
 * A caller asserts eegnet_abi_version() == the EEGNET_ABI_VERSION it was compiled against.
 *   4: eegnet_fold.xstat added before seed (round 4)
 *   5: xstat moved after seed -- the round-3 fields at their round-3 offsets again (round 5) */
#define EEGNET_ABI_VERSION 5
int eegnet_abi_version(void);

/* Thread-local description of the last error ("" if none). */
const char* eegnet_last_error(void);

/* Library/build identification string (gfx target, build flags). */
const char* eegnet_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* EEGNET_ABI_H */
