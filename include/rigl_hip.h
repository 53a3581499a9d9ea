/* rigl_hip.h -- C ABI of the MI355X (gfx950) RigL hot path.
 *
 * The reference (google-research/rigl) has no native code and no FFI: its hot
 * path sits behind Python signatures and runs inside TensorFlow ops.  This
 * header is the boundary a maintainer binds INSTEAD of those TF ops; every
 * entry point cites the reference call site it replaces.  Rules:
 *   - plain C, `extern "C"`, no torch / C++ types in any signature;
 *   - the caller owns every buffer and passes raw DEVICE pointers + sizes and
 *     the hipStream_t to enqueue on (as void*); nothing is allocated inside,
 *     scratch comes from a caller-provided workspace (`*_workspace_bytes`);
 *     the workspace must start on a 256-byte boundary (every region inside it
 *     is laid out in 256-byte units from its start) and hold at least the
 *     queried number of bytes; its contents on entry do not matter, every
 *     call initialises what it reads, and nothing is kept there between calls.
 *     The queries follow the run-time knobs (rigl_tune_set) and the device:
 *     ask again after changing a knob.  A workspace that is NULL or shorter
 *     than the query, where the query is not 0, is refused with
 *     RIGL_EWORKSPACE before anything is enqueued; the entry points that take
 *     the argument pair without using it say so below;
 *   - every call only ENQUEUES work on `stream` (no hidden synchronisation);
 *   - return 0 on success, a negative RIGL_E* code otherwise; the message for
 *     the calling thread is available from rigl_last_error(); never throws;
 *   - re-entrant: no mutable global state besides the loaded code object.
 *
 * Layout conventions (the reference's):
 *   activations  NHWC, bf16 (raw uint16 bit patterns)
 *   weights      HWIO  [kh][kw][cin][cout] fp32 master copy (FC: [in][out]);
 *                flat index = C order -- this is the index space in which the
 *                masks, the top-k tie-break ("lower index first") and the
 *                golden vectors are defined
 *   mask         1 bit / weight, bit (i & 31) of uint32 word (i >> 5), i = flat
 *                HWIO index; bits at positions >= n in the last word are 0
 */
#ifndef RIGL_HIP_H_
#define RIGL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point is removed or a signature changes (2: round 4 dropped
 * rigl_masked_conv2d_bwd_deferred / rigl_wgrad_reduce_pending; 3: the batch-norm backward reductions in the dgrad
 * epilogue left with their four entry points and argument block, tools/experiments/ keeps them as a patch). */
#define RIGL_ABI_VERSION 3

typedef void* rigl_stream_t; /* hipStream_t */
typedef uint16_t rigl_bf16;  /* raw bfloat16 bits */

enum {
  RIGL_OK = 0,
  RIGL_EINVAL = -1,       /* bad argument (NULL, negative size, misaligned) */
  RIGL_ELAUNCH = -2,      /* HIP runtime / launch failure */
  RIGL_EWORKSPACE = -3,   /* workspace too small */
  RIGL_EUNSUPPORTED = -4  /* shape / mode not supported by this build */
};

int rigl_version(void);
/* Host utility: CRC-32C (Castagnoli) of a host buffer, continuing from `crc`
 * (0 to start) -- the checksum TensorFlow's checkpoint bundles carry
 * (README.md:34-58 checkpoints; rigl_amd/tf_checkpoint.py).                 */
uint32_t rigl_crc32c(const void* data, size_t n, uint32_t crc);
/* Message of the last failing call made by THIS thread ("" if none). */
const char* rigl_last_error(void);

/* ------------------------------------------------------------------------
 * Mask bitmap <-> 0/1 float mask.
 * Replaces: the fp32 `mask` variable of tf.contrib.model_pruning
 * (registered by layers.masked_conv2d, rigl/imagenet_resnet/pruning_layers.py
 * :139-157) -- the bitmap is the HBM-resident form, the float form exists
 * only at the API surface (get_masks()).
 * ---------------------------------------------------------------------- */
int rigl_mask_pack(const float* mask01, uint32_t* bits, int64_t n,
                   rigl_stream_t stream);
int rigl_mask_unpack(const uint32_t* bits, float* mask01, int64_t n,
                     rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * K2: fused magnitude-prune / gradient-regrow mask update.
 * Replaces: SparseRigLOptimizerBase.generic_mask_update
 *   (rigl/sparse_optimizers_base.py:523-538) + _get_update_op (:276-343)
 *   + get_grow_tensor (:355-400, :540-553) + reset_momentum (:555-564), i.e.
 *   the two full-length nn_ops.top_k sorts, two scatter_nd, where/assign.
 * Also serves SET / Static / Momentum (sparse_optimizers.py:109-214) through
 * the explicit-score pointers.
 *
 * Result (bit-exact with the reference semantics on identical inputs):
 *   n_ones  = popcount(mask);  n_prune = (int32)((float)n_ones * drop_fraction)
 *   n_keep  = n_ones - n_prune
 *   mask1   = the n_keep entries with the largest drop score, equal scores
 *             resolved by LOWER flat index first (tf.nn.top_k order)
 *   lifted  = mask1 ? (min(grow score) - 1) : grow score
 *   mask2   = the n_prune entries with the largest lifted score (same ties)
 *   new     = mask2 & (reinit_when_same ? 1 : ~mask_old)
 *   w[new]  = grow value;  momentum[new] = reset value;  mask = mask1 | mask2
 * drop score = |mask*w| (+ drop_noise[i], one fp32 add) unless score_drop is
 * given; grow score = |dense_grad| unless score_grow is given.
 * Scores may be subnormal, +-inf or signed zeros (-0.0 ties with +0.0); NaN
 * scores are out of scope: tf.nn.top_k's order on NaN is not defined.
 * The fp32 pointers need no alignment beyond 4 bytes; bitmaps are 4-byte words.
 * ---------------------------------------------------------------------- */
typedef struct RiglPruneRegrowLayer {
  int64_t n;               /* number of weights in this tensor (< 2^31)     */
  float* w;                /* in/out fp32 [n]                                */
  float* momentum;         /* in/out fp32 [n], NULL = no slot                */
  uint32_t* mask_bits;     /* in/out ceil(n/32) words                        */
  const float* dense_grad; /* fp32 [n] dense dL/d(mask*W); may be NULL only  */
                           /* if score_grow is given and modes need no grad  */
  const float* drop_noise; /* fp32 [n] or NULL (noise_std = 0)               */
  const float* score_drop; /* fp32 [n] or NULL: explicit drop scores         */
  const float* score_grow; /* fp32 [n] or NULL: explicit grow scores         */
  const float* grow_values;/* fp32 [n] or NULL: explicit grown-weight values */
} RiglPruneRegrowLayer;

enum {
  RIGL_GROW_ZEROS = 0,      /* grow_init='zeros'          (:372-373)         */
  RIGL_GROW_GRAD_SCALE = 1, /* 'grad_scale_d': g / d      (:542-545)         */
  RIGL_GROW_GRAD_SIGN = 2,  /* 'grad_sign_d': sign(g) / d (:546-549), sign(+-0) = +0 as tf.sign */
  RIGL_GROW_EXPLICIT = 3    /* values from grow_values    (random_* / initial_dist_* drawn by the host) */
};
enum {
  RIGL_MOMRESET_ZEROS = 0,  /* SET: zeros                 (:345-353)         */
  RIGL_MOMRESET_GRAD = 1    /* RigL: dense_grad * initial_acc_scale (:555-564) */
};

typedef struct RiglPruneRegrowParams {
  float drop_fraction;
  int32_t grow_init_mode;
  float grow_init_div;
  int32_t momentum_reset_mode;
  float initial_acc_scale;
  int32_t reinit_when_same;
} RiglPruneRegrowParams;

#define RIGL_COUNTS_PER_LAYER 8
/* out_counts[l*8 + ..]: 0 n_ones, 1 n_prune, 2 n_keep, 3 n_new_connections,
 * 4 overlap (!=0 <=> the reference's Assert(mask1*mask2==0) would fire),
 * 5 ties admitted at the drop threshold, 6 ties admitted at the grow
 * threshold, 7 popcount of the new mask.                                   */
size_t rigl_prune_regrow_workspace_bytes(const int64_t* n_per_layer,
                                         int32_t n_layers);
int rigl_prune_regrow(const RiglPruneRegrowLayer* layers /* host */,
                      int32_t n_layers, const RiglPruneRegrowParams* params,
                      int32_t* out_counts /* device, 8*n_layers, nullable */,
                      void* workspace /* device */, size_t workspace_bytes,
                      rigl_stream_t stream);

/* The same update on ONE tensor, with its two selections read back (north
 * star: "masks and top-k indices bit-exact"; SURVEY.md 8(b) sketch
 * `out_topk_idx`): out_mask1_bits = the kept set mask1, out_mask2_bits = the
 * grown set mask2 (bitmaps, either may be NULL) and -- both or neither --
 * out_idx1 / out_idx2 [n] int32: the indices in tf.nn.top_k order of the drop
 * score resp. the lifted grow score (sparse_optimizers_base.py:293, :311),
 * i.e. larger score first, equal scores by lower index; the first n_keep
 * (out_counts[2]) resp. n_prune (out_counts[1]) entries are the selected ones,
 * the entries behind them are the rest of the tensor in the same order.  The
 * tensor is updated exactly as by rigl_prune_regrow.  A test / inspection
 * entry point: one stable 33-bit radix sort of the whole tensor per list.
 * ORDER: the update (weights, mask, momentum) is enqueued FIRST, the two sorts
 * after it; if enqueueing a sort fails the call returns an error with the
 * tensor already updated and out_idx1 / out_idx2 undefined.                 */
size_t rigl_prune_regrow_selections_workspace_bytes(int64_t n);
int rigl_prune_regrow_selections(const RiglPruneRegrowLayer* layer /* host */,
                                 const RiglPruneRegrowParams* params,
                                 uint32_t* out_mask1_bits, uint32_t* out_mask2_bits,
                                 int32_t* out_idx1, int32_t* out_idx2,
                                 int32_t* out_counts /* device, 8, nullable */,
                                 void* workspace, size_t workspace_bytes,
                                 rigl_stream_t stream);

/* Two-slot forms for inner optimizers with a second slot per weight (Adam's m
 * and v).  The reference resets EVERY slot of a grown connection
 * (sparse_optimizers_base.py:345-353 SET, :555-564 RigL): momentum2[l] (a HOST
 * array of n_layers device pointers, entries nullable; fp32 [n] each) receives
 * the same reset value as layers[l].momentum -- 0 (RIGL_MOMRESET_ZEROS) or
 * dense_grad * initial_acc_scale (RIGL_MOMRESET_GRAD; then dense_grad is
 * required when initial_acc_scale != 0, as for momentum).  Everything else is
 * rigl_prune_regrow / rigl_prune_regrow_selections; momentum2 == NULL is
 * exactly those calls.  Workspaces as for the one-slot forms.
 * Replaces: the per-slot tf.where / assign loop of reset_momentum for
 *   tf.train.AdamOptimizer (imagenet_train_eval.py:355-358 --use_adam,
 *   mnist_train_eval.py:247-261 --optimizer=adam).                         */
int rigl_prune_regrow_slots(const RiglPruneRegrowLayer* layers /* host */,
                            float* const* momentum2 /* host [n_layers], nullable */,
                            int32_t n_layers, const RiglPruneRegrowParams* params,
                            int32_t* out_counts /* device, 8*n_layers, nullable */,
                            void* workspace /* device */, size_t workspace_bytes,
                            rigl_stream_t stream);
int rigl_prune_regrow_selections_slots(const RiglPruneRegrowLayer* layer /* host */,
                                       float* momentum2 /* device fp32 [n], nullable */,
                                       const RiglPruneRegrowParams* params,
                                       uint32_t* out_mask1_bits, uint32_t* out_mask2_bits,
                                       int32_t* out_idx1, int32_t* out_idx2,
                                       int32_t* out_counts /* device, 8, nullable */,
                                       void* workspace, size_t workspace_bytes,
                                       rigl_stream_t stream);

/* One-shot "keep the k best" mask (SNIP / DNW, sparse_optimizers.py:287-317,
 * :430-460): mask = the n_keep entries of score with the largest value, ties
 * by lower index.  Uses the same selection kernels as rigl_prune_regrow.    */
int rigl_topk_mask(const float* score, int64_t n, int64_t n_keep,
                   uint32_t* mask_bits, void* workspace,
                   size_t workspace_bytes, rigl_stream_t stream);
/* The same for many tensors in the same launches (DNW re-derives every mask
 * every step).  Workspace: rigl_prune_regrow_workspace_bytes of the sizes.   */
typedef struct RiglTopkLayer {
  const float* score;   /* fp32 [n] */
  int64_t n;
  int64_t n_keep;
  uint32_t* mask_bits;  /* out, ceil(n/32) words */
} RiglTopkLayer;
int rigl_topk_mask_batched(const RiglTopkLayer* layers /* host */,
                           int32_t n_layers, void* workspace,
                           size_t workspace_bytes, rigl_stream_t stream);

/* Gradual magnitude pruning (Zhu & Gupta), the 'prune' training_method of
 * rigl/mnist/mnist_train_eval.py:96-100, 320-337 and
 * rigl/cifar_resnet/resnet_train_eval.py:85, 249-275, which run
 * tf.contrib.model_pruning.  Replaces the mask update of TF 1.15
 * contrib/model_pruning/python/pruning.py (Pruning._update_mask, weight
 * magnitude, 1x1 blocks, no histogram / TPU path), per masked layer with n
 * weights (raw kernel W, not mask*W) and a k the caller derived from the
 * sparsity schedule (k = round_half_even(f32(n) * (1 - s_l))):
 *   cur       = the k-th largest |W|  (top_k of every |W|, gather(values, k-1))
 *   threshold = f32(cur * f32(1 - decay)) + f32(threshold * f32(decay))
 *   mask      = |W| >= threshold      (every tie admitted: popcount >= k)
 * Weights and optimizer slots are not touched.  The selection runs on K2's
 * segmented radix select (all layers in the same launches) over the key
 * bits(w) & 0x7fffffff, then one pass writes every bitmap (tail bits of the
 * last word zero) and the new thresholds are stored.  No host sync.        */
typedef struct RiglMagnitudePruneLayer {
  int64_t n;            /* 1 <= n < 2^31 */
  const float* w;       /* fp32 [n], read only */
  uint32_t* mask_bits;  /* out, ceil(n/32) words */
  float* threshold;     /* device fp32 [1]: in = the stored threshold, out = the new one */
  int64_t k;            /* 1 <= k <= n (contrib's k == 0 fails in gather(values, -1)) */
} RiglMagnitudePruneLayer;
/* Workspace of rigl_magnitude_prune_batched: per-layer state only.         */
size_t rigl_magnitude_prune_batched_workspace_bytes(int32_t n_layers);
/* One call for all masked layers of a model.  threshold_decay = contrib's
 * hparam (fp32 constants f32(decay) and f32(1 - decay) as TF forms them).
 * out_counts (device, RIGL_MAGPRUNE_COUNTS_PER_LAYER * n_layers, nullable):
 * per layer n, k, ones of the new mask, ones of the old mask.  Timed under
 * profiler kind 9 (magnitude_prune).                                      */
#define RIGL_MAGPRUNE_COUNTS_PER_LAYER 4
int rigl_magnitude_prune_batched(const RiglMagnitudePruneLayer* layers /* host */,
                                 int32_t n_layers, double threshold_decay,
                                 int32_t* out_counts, void* workspace,
                                 size_t workspace_bytes, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * K3: masked fused SGD / momentum update (+ bf16 shadow of mask*W).
 * Replaces: the TF ApplyMomentum / ApplyGradientDescent kernels behind
 *   tf.train.MomentumOptimizer(lr, momentum, use_nesterov=True)
 *   (rigl/imagenet_resnet/imagenet_train_eval.py:360-361,
 *    rigl/cifar_resnet/resnet_train_eval.py:202-203) together with the
 *   `mask *` of the masked-weight gradient and the l2_regularizer gradient:
 *     g  = mask * (grad_scale*dense_grad) + weight_decay * w
 *     a  = momentum*a + g
 *     w -= lr*g + lr*momentum*a   (nesterov)   |   w -= lr*a   (plain)
 *   every product / sum rounded to fp32 separately (no FMA contraction).
 *   For finite inputs w and a are bit-identical to oracle/rigl_oracle.py's
 *   masked_grad (on the scaled gradient) followed by momentum_apply /
 *   sgd_apply, the signs of zeros included: the decay product is always added
 *   (a signed zero when weight_decay == 0) and a masked-off element contributes
 *   0 * g, a zero with the gradient's sign -- a momentum of -0.0 (RigL's reset
 *   g * 0.0 of a negative gradient, or a pruned weight's underflowed slot)
 *   keeps the sign the reference would give it.
 *   The one deliberate deviation: a NON-FINITE gradient at a masked-off
 *   position also counts as that signed zero, where the reference's 0 * inf
 *   would write NaN into the pruned weight.  (A non-finite w is outside the
 *   contract: 0 * w is NaN, as in the reference.)
 * mask_bits == NULL means "all ones" (dense tensors: BN, biases, dense stem).
 * momentum == NULL means plain gradient descent (w -= lr*g).
 * w_shadow (nullable) receives bf16(mask ? w_new : 0), same flat order.
 * Alignment: w, momentum, dense_grad 16-byte, w_shadow 8-byte, mask_bits
 * 4-byte (RIGL_EINVAL otherwise, nothing launched).
 * ---------------------------------------------------------------------- */
int rigl_masked_sgd_momentum(int64_t n, float* w, float* momentum,
                             const float* dense_grad, const uint32_t* mask_bits,
                             float lr, float mu, float weight_decay,
                             float grad_scale, int32_t nesterov,
                             rigl_bf16* w_shadow, rigl_stream_t stream);

/* K3-Adam: masked fused Adam update (+ bf16 shadow of mask*W).
 * Replaces: the TF ApplyAdam kernel (training_ops.cc, use_nesterov=false)
 *   behind tf.train.AdamOptimizer (imagenet_train_eval.py:214-215, 355-358
 *   --use_adam; mnist_train_eval.py:247-261 --optimizer=adam), together with
 *   the `mask *` of the masked-weight gradient and the l2 gradient:
 *     alpha = (lr * sqrt(1 - beta_powers[1])) / (1 - beta_powers[0])
 *     g     = mask * (grad_scale*dense_grad) + weight_decay * w
 *     m     = m + (g - m) * (1 - beta1)
 *     v     = v + (g*g - v) * (1 - beta2)
 *     w     = w - (m * alpha) / (sqrt(v) + epsilon)
 *   every product / sum rounded to fp32 separately, sqrt and division
 *   correctly rounded.  For finite inputs w, m and v are bit-identical to
 *   tests/adam_ref.py -- the fp32 restatement of ApplyAdam's CPU functor on
 *   oracle.masked_grad of the scaled gradient, K3's g -- which the
 *   reference-executed trajectories of tests/golden/adam_cases.npz confirm.
 *   (The kernel forms g by selection, which can differ from K3's g in the
 *   sign of a zero only; no bit of m, v or w depends on that sign.)  The same
 *   deliberate deviation: a non-finite gradient at a masked-off position
 *   counts as zero.
 * Masked-off weights are updated too (the reference applies Adam to the raw
 * variable: a pruned weight gets g = weight_decay*w and keeps drifting on its
 * old m); w_shadow (nullable) receives bf16(mask ? w_new : 0).
 * beta_powers is a DEVICE fp32 [2] = {beta1^t, beta2^t} (the optimizer's
 * non-slot variables); alpha is derived from it inside the kernel, so a
 * captured HIP graph replays the current bias correction, not a frozen one.
 * Alignment: w, m, v, dense_grad 16-byte, w_shadow 8-byte, mask_bits and
 * beta_powers 4-byte (RIGL_EINVAL otherwise).  mask_bits == NULL = all ones. */
int rigl_masked_adam(int64_t n, float* w, float* m, float* v,
                     const float* dense_grad, const uint32_t* mask_bits,
                     const float* beta_powers /* device [2] */, float lr,
                     float beta1, float beta2, float epsilon,
                     float weight_decay, float grad_scale,
                     rigl_bf16* w_shadow, rigl_stream_t stream);
/* beta_powers[0] *= beta1; beta_powers[1] *= beta2 (fp32, one rounding each):
 * AdamOptimizer._finish, enqueued once after the last rigl_masked_adam of a
 * step.  One single-lane launch.                                            */
int rigl_adam_advance(float* beta_powers /* device [2] */, float beta1,
                      float beta2, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-resident learning rate.
 * Replaces: the learning-rate subgraph TF evaluates inside every training
 *   step -- lr_schedule(current_epoch) with its tf.where chain
 *   (rigl/imagenet_resnet/imagenet_train_eval.py:317-330, 352-354),
 *   tf.train.piecewise_constant (rigl/cifar_resnet/resnet_train_eval.py:
 *   189-200, rigl/mnist/mnist_train_eval.py:249-256) and
 *   tf.train.cosine_decay_restarts (--use_sgdr, :321-323).
 * A captured HIP graph freezes kernel arguments, so a rate passed by value
 * (rigl_masked_sgd_momentum's / rigl_masked_adam's `lr`) is the rate of the
 * capture for every replay.  Here the step counter and the rate live in
 * device memory: rigl_lr_schedule_step evaluates the schedule at *step, writes
 * *lr_out and advances *step inside the graph, and the _dlr update entry
 * points read the rate from that buffer -- as rigl_masked_adam reads
 * beta_powers and rigl_dropout_fwd reads its step.
 *
 * The schedule is a table of at most RIGL_LR_MAX_SEGMENTS segments in
 * ascending (non-decreasing) `start` order, passed by value to the kernel.
 *   domain RIGL_LR_DOMAIN_STEP : x = *step (int32), compared as an integer
 *                                with start_step; f32(*step) in arithmetic.
 *   domain RIGL_LR_DOMAIN_EPOCH: x = f32(*step) / steps_per_epoch, ONE fp32
 *                                division (:352-353), compared with start.
 * The active segment is the LAST one with !(x < start); below every start the
 * first segment is active.  For ascending starts that is the value the
 * reference's chain `rate = tf.where(x < start, rate, const)` ends with.  A
 * tf.train.piecewise_constant boundary b (x <= b keeps the old value) is the
 * integer start b + 1.  Only the active segment is evaluated: an inactive
 * one whose value would be inf or NaN (the ResNet chain's warm-up divides by
 * its start epoch 0) never reaches the output.
 * Every product, quotient, sum and difference below is rounded to fp32
 * separately (no FMA contraction), in this order:
 *   RIGL_LR_CONST : lr = c
 *   RIGL_LR_WARMUP: lr = (c * x) / d            (:325-326; c = f32(scaled_lr *
 *                   mult0), d = f32(start_epoch0); d == 0 is legal)
 *   RIGL_LR_COSINE: one cycle of TF 1.15's cosine_decay_restarts, alpha = 0:
 *                   frac = ((x / d) - sum_r) / len
 *                   t    = pi32 * frac                     (pi32 = f32(pi))
 *                   lr   = c * ((0.5 * m_fac) * (1 + f32(cos(double(t)))))
 *                   c = the initial rate, d = first_decay_steps, and sum_r /
 *                   len / m_fac the cycle's (1 - t_mul^i) / (1 - t_mul),
 *                   t_mul^i and m_mul^i, written by the host in TF's fp32
 *                   order: the device evaluates no log, pow or floor, and the
 *                   cycle is the segment the comparison selects.  The cosine
 *                   is taken in double and rounded once.
 * rigl_lr_schedule_step: *lr_out = f(*step); *step += 1 (int32 wrap-around,
 * as rigl_dropout_advance).  One single-lane launch.  `sched` is a HOST
 * pointer, consumed before the call returns.  RIGL_EINVAL with nothing
 * launched: a NULL or not 4-byte aligned pointer, n_seg outside
 * 1..RIGL_LR_MAX_SEGMENTS, an unknown domain or kind, starts of the domain
 * that do not ascend (a NaN start included), steps_per_epoch not finite or
 * not > 0 in the epoch domain, a COSINE segment whose len is not > 0.
 * ---------------------------------------------------------------------- */
#define RIGL_LR_MAX_SEGMENTS 32
#define RIGL_LR_DOMAIN_STEP 0
#define RIGL_LR_DOMAIN_EPOCH 1
#define RIGL_LR_CONST 0
#define RIGL_LR_WARMUP 1
#define RIGL_LR_COSINE 2
typedef struct RiglLrSegment {
  int32_t kind;       /* RIGL_LR_CONST / _WARMUP / _COSINE */
  int32_t start_step; /* the start in the step domain */
  float start;        /* the start in the epoch domain */
  float c, d;         /* see the kinds above */
  float sum_r, len, m_fac; /* COSINE only */
} RiglLrSegment;
typedef struct RiglLrSchedule {
  int32_t n_seg;
  int32_t domain;
  float steps_per_epoch; /* epoch domain only */
  int32_t reserved;
  RiglLrSegment seg[RIGL_LR_MAX_SEGMENTS];
} RiglLrSchedule;
int rigl_lr_schedule_step(const RiglLrSchedule* sched /* host */,
                          int32_t* step /* device */,
                          float* lr_out /* device */, rigl_stream_t stream);

/* rigl_masked_sgd_momentum / rigl_masked_adam with `float lr` replaced by a
 * DEVICE pointer to one fp32, read once per lane as a uniform load (the way
 * beta_powers is read).  The same kernel bodies: for the same fp32 value in
 * memory they leave the same bits as the by-value entry points.  Alignment
 * and NULL rules are theirs; in addition lr must be non-NULL and 4-byte
 * aligned (RIGL_EINVAL otherwise).                                          */
int rigl_masked_sgd_momentum_dlr(int64_t n, float* w, float* momentum,
                                 const float* dense_grad,
                                 const uint32_t* mask_bits,
                                 const float* lr /* device */, float mu,
                                 float weight_decay, float grad_scale,
                                 int32_t nesterov, rigl_bf16* w_shadow,
                                 rigl_stream_t stream);
int rigl_masked_adam_dlr(int64_t n, float* w, float* m, float* v,
                         const float* dense_grad, const uint32_t* mask_bits,
                         const float* beta_powers /* device [2] */,
                         const float* lr /* device */, float beta1,
                         float beta2, float epsilon, float weight_decay,
                         float grad_scale, rigl_bf16* w_shadow,
                         rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-step training summaries.
 * Replaces: the scalars every training driver of the reference hands to
 *   tf.summary / host_call on every step -- tf.norm of the gradients and of
 *   the variables, the fw_nz_weight / fw_nz_mask / fw_l1_weight probes and
 *   the per-mask sparsities (rigl/imagenet_resnet/imagenet_train_eval.py:
 *   431-473, rigl/imagenet_resnet/utils.py:59-90) -- with ONE read-only pass
 *   over the arenas per step and a record in a device ring, so a captured
 *   HIP graph leaves a record per replay and the host reads when it likes.
 * One entry per trainable variable, elements [0, n) only (padding between
 * variables is never read).  Per element, with m the mask bit (1 where
 * mask_bits == NULL or apply_mask == 0):
 *   gq = f32(f32(m * f32(grad_scale * g)) + f32(weight_decay * w))
 * -- the gradient rigl_masked_sgd_momentum applies, rounding for rounding,
 * with its documented deviation: a masked-off element contributes the signed
 * zero of the scaled gradient, also where that gradient is not finite.
 * Per entry (fp64 sums, integer counts):
 *   sumsq_g = sum gq^2        sumsq_w = sum w^2 (raw weights)   l1_w = sum |w|
 *   nz_w = #(w != 0)  (-0.0 is zero, subnormals are not)
 *   mask_ones = popcount of bits [0, n)  (n where mask_bits == NULL)
 *   nonfinite_g = #(gq inf or NaN)
 * Non-finite values propagate into the sums as IEEE arithmetic gives them.
 * DETERMINISM: every entry is cut into chunks of RIGL_SUMMARY_CHUNK elements;
 * a chunk is reduced in a fixed order, a second launch sums an entry's chunk
 * partials in a fixed order and the entries likewise.  No atomics; the bits of
 * the result do not depend on max_blocks (the grid cap of the partials
 * launches, 0 = default) or on anything but the table and the data.
 * The finalize launch writes slot (*step mod ring_slots) of `ring`
 * (rigl_summary_slot_bytes(n_entries) bytes per slot, 16-byte aligned):
 *   int32 step, int32 n_entries, fp32 loss (*loss; NaN where loss == NULL),
 *   fp32 learning rate (*lr, or lr_value where lr == NULL)       -- 16 bytes
 *   the totals over all entries, then entry 0, 1 ...: each 3 fp64 (sumsq_g,
 *   sumsq_w, l1_w) and 3 int64 (nz_w, mask_ones, nonfinite_g)    -- 48 bytes
 * and then *step += 1 (int32 wrap-around, as rigl_lr_schedule_step).
 * Capture-safe: `entries` is a HOST array, consumed before the call returns
 * and passed to the kernels by value, 64 entries per launch; no copy is
 * enqueued.  Launches: ceil(n_entries / 64) + 1.
 * Refused with nothing launched: RIGL_EWORKSPACE for a workspace that is NULL
 * or shorter than rigl_summary_workspace_bytes(entries, n_entries);
 * RIGL_EINVAL for w / g not 16-byte aligned, mask_bits / step / loss / lr not
 * 4-byte aligned, ring not 16-byte aligned, ring_slots < 1, n < 0, a NULL
 * w / g with n > 0.
 * ---------------------------------------------------------------------- */
#define RIGL_SUMMARY_CHUNK 8192
typedef struct RiglSummaryEntry {
  int64_t n;
  const float* w;            /* fp32 [n] */
  const float* g;            /* fp32 [n]: the gradient-arena slice (dense for masked kernels) */
  const uint32_t* mask_bits; /* ceil(n/32) words, NULL = all ones */
  float weight_decay;
  int32_t apply_mask;        /* 0: g is used unmasked (DNW); mask_ones still counts the bitmap */
} RiglSummaryEntry;
size_t rigl_summary_slot_bytes(int32_t n_entries);
size_t rigl_summary_workspace_bytes(const RiglSummaryEntry* entries /* host */, int32_t n_entries);
int rigl_summary_step(const RiglSummaryEntry* entries /* host */, int32_t n_entries,
                      float grad_scale, const float* loss /* device, nullable */,
                      const float* lr /* device, nullable */, float lr_value,
                      int32_t* step /* device */, void* ring /* device */,
                      int32_t ring_slots, void* workspace, size_t workspace_size /* bytes */,
                      int32_t max_blocks, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Micro-batch gradient accumulation: k forward/backward passes, one update.
 *   Replaces: the cross-replica sum of every variable gradient at a global
 *   batch of k x the per-core batch (rigl/imagenet_resnet/
 *   imagenet_train_eval.py:363-365, rigl/sparse_optimizers_base.py:472-473),
 *   serialised onto one GPU: the wgrad kernels overwrite their slice of the
 *   gradient arena, so the running sum lives in a second arena and ONE
 *   launch over the whole arena per micro-batch moves it on:
 *     FIRST: acc = g           loss_acc = loss
 *     ADD  : acc = acc + g     loss_acc = loss_acc + loss
 *     LAST : g   = acc + g     loss_mean = (loss_acc + loss) * inv_k
 *   FIRST is a copy (bit for bit, NaN payloads included): no memset, and a
 *   stale acc never reaches a step.  LAST leaves the raw SUM in the gradient
 *   arena, where every consumer reads it; acc and loss_acc are only read.
 * Arithmetic: one IEEE fp32 addition per element (round to nearest even, no
 * FMA, no wider intermediate, no atomics); subnormals are kept, signed zeros,
 * infinities and NaN follow IEEE.  The result bits depend on the operands
 * alone, not on the grid or max_blocks.  The loss scalar is handled by one
 * lane of the same launch; its addition and the product with inv_k are
 * rounded to fp32 separately.  loss == NULL: no loss arithmetic at all.
 * acc and grad are distinct 16-byte aligned buffers of n >= 0 fp32; no
 * element at or beyond n is touched (the n % 4 tail is handled).  n == 0 with
 * a loss still does the loss arithmetic.  max_blocks caps the grid (0 = the
 * default, 8 blocks per CU).
 * RIGL_EINVAL, with nothing launched or written: a NULL or misaligned acc /
 * grad (or acc == grad), an unknown mode, n < 0, max_blocks < 0, loss without
 * loss_acc, LAST with loss but no loss_mean, a loss pointer that is not
 * 4-byte aligned.
 * ---------------------------------------------------------------------- */
#define RIGL_ACC_FIRST 0
#define RIGL_ACC_ADD 1
#define RIGL_ACC_LAST 2
int rigl_grad_accumulate(int64_t n, float* acc, float* grad, int32_t mode,
                         const float* loss /* device [1], nullable */,
                         float* loss_acc /* device [1] */,
                         float* loss_mean /* device [1], written in LAST only */,
                         float inv_k, int32_t max_blocks, rigl_stream_t stream);

/* The same pass over up to RIGL_ACC_MAX_RANGES ranges of the two arenas, in
 * ONE launch: element i of every range [offset, offset + length) takes the
 * arithmetic of rigl_grad_accumulate (one IEEE fp32 addition, FIRST a bit
 * copy); nothing outside the ranges is read or written, in either arena.
 *   Replaces: the same cross-replica sum, where micro-batch accumulation
 *   meets the data-parallel exchange: the LAST pass of one exchange bucket
 *   right before its all-reduce, and the head of the kernel segment plus the
 *   BN / bias segment behind the last backward node (rigl_amd/dist.py).
 * `ranges` is a HOST array, consumed before the call returns and passed to
 * the kernel by value (capture-safe).  Offsets and lengths are in elements of
 * the arenas of n fp32; an offset is a multiple of 4 (so that every range
 * starts 16-byte aligned), a length is arbitrary (its % 4 tail is handled)
 * and may be 0; ranges ascend and do not overlap (they may touch).  Tiles are
 * cut over the concatenation of the ranges -- every range rounded up to whole
 * 16-byte quads -- so a short range behind a long one costs neither a second
 * launch nor a tail of idle workgroups.  The result bits depend on the
 * operands alone: not on the grid, on max_blocks or on how the same elements
 * are cut into ranges.  The loss scalar is handled ONCE per launch by one
 * lane, whatever n_ranges is; n_ranges == 0 with a loss still does the loss
 * arithmetic (and without one launches nothing).
 * RIGL_EINVAL, with nothing launched or written: everything
 * rigl_grad_accumulate refuses, n_ranges < 0 or > RIGL_ACC_MAX_RANGES, a NULL
 * table with n_ranges > 0, a negative offset or length, an offset that is not
 * a multiple of 4, a range that ends beyond n, ranges that overlap or do not
 * ascend. */
#define RIGL_ACC_MAX_RANGES 8
typedef struct RiglAccRange {
  int64_t offset;  /* first element, a multiple of 4 */
  int64_t length;  /* elements, >= 0 */
} RiglAccRange;
int rigl_grad_accumulate_ranges(int64_t n, float* acc, float* grad,
                                const RiglAccRange* ranges /* host */, int32_t n_ranges,
                                int32_t mode, const float* loss /* device [1], nullable */,
                                float* loss_acc /* device [1] */,
                                float* loss_mean /* device [1], written in LAST only */,
                                float inv_k, int32_t max_blocks, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Training-state snapshots: a table of device regions <-> ONE packed device
 * image, at copy rate, with a digest per region.
 *   Replaces: the per-variable save / restore ops of tf.train.Saver, which
 *   the reference's Estimator drivers run every save_checkpoints_steps
 *   (rigl/imagenet_resnet/imagenet_train_eval.py:740-741, rigl/cifar_resnet/
 *   resnet_train_eval.py:517-519) -- one copy per tensor -- with one gather pass into a
 *   staging buffer, after which the training stream is free again.
 * LAYOUT: region r starts in `packed` at the running sum of the earlier
 * regions' byte counts, each rounded up to RIGL_STATE_ALIGN (256).  gather
 * writes the padding behind a region as zero bytes (the image depends on the
 * state alone); scatter never reads the padding and writes nothing outside
 * [ptr, ptr + bytes) of any region.  Copies are bit for bit: NaN payloads,
 * signed zeros and subnormals are kept.
 * DIGEST: per region, over its uint32 words w_0 .. w_{m-1} (m = bytes / 4,
 * padding excluded):  s1 = sum w_i mod 2^64,  s2 = sum (i + 1) * w_i mod 2^64,
 * written as digests[2r], digests[2r + 1].  gather digests the words it read,
 * scatter the words it wrote.  Integer arithmetic only: the bits depend on the
 * data alone, not on the grid, on max_blocks (the grid cap, 0 = default) or on
 * the order of the partial sums.  Every call writes every digest and reads
 * nothing the buffer held before; a zero-length region has digest (0, 0).
 * The digest is an integrity check against truncation, misplacement and bit
 * rot.  It is NOT cryptographic: forging a collision is easy.
 * A region is cut into chunks of RIGL_STATE_CHUNK words, one workgroup per
 * chunk at a time (a long region is spread over the whole grid); the chunk
 * partials live in the workspace and one finalize launch sums them.  16-byte
 * accesses on both sides where the region pointer is 16-byte aligned (every
 * torch allocation and arena slice is; the rates on record were measured on
 * such regions only).  A region pointer that is only 4-byte aligned keeps
 * them on the packed side and takes four 4-byte accesses per lane on its own
 * side: correct and tested, its rate not measured.
 * Capture-safe: `regions` is a HOST array, consumed before the call returns
 * and passed to the kernels by value, RIGL_STATE_BATCH regions per launch.
 * Launches: ceil(n / 64) + 1; none for n == 0.
 * Refused with nothing launched and nothing written: RIGL_EINVAL for a region
 * pointer that is not 4-byte aligned, bytes negative or no multiple of 4, a
 * NULL pointer with bytes > 0, packed not 256-byte aligned, digests not
 * 8-byte aligned, n < 0, max_blocks < 0; RIGL_EWORKSPACE for a workspace that
 * is NULL or shorter than rigl_state_workspace_bytes(regions, n).
 * ---------------------------------------------------------------------- */
#define RIGL_STATE_ALIGN 256
#define RIGL_STATE_CHUNK 16384
#define RIGL_STATE_BATCH 64
typedef struct RiglStateRegion {
  void* ptr;       /* device memory, 4-byte aligned */
  int64_t bytes;   /* a multiple of 4 */
} RiglStateRegion;
size_t rigl_state_packed_bytes(const RiglStateRegion* regions /* host */, int32_t n);
size_t rigl_state_workspace_bytes(const RiglStateRegion* regions /* host */, int32_t n);
int rigl_state_gather(const RiglStateRegion* regions /* host */, int32_t n, void* packed,
                      uint64_t* digests /* device [2n] */, void* workspace,
                      size_t workspace_size /* bytes */, int32_t max_blocks,
                      rigl_stream_t stream);
int rigl_state_scatter(const RiglStateRegion* regions /* host */, int32_t n,
                       const void* packed, uint64_t* digests /* device [2n] */,
                       void* workspace, size_t workspace_size /* bytes */,
                       int32_t max_blocks, rigl_stream_t stream);

/* bf16 shadows of mask*W for the conv kernels:  hwio[i] = bf16(mask_i?w_i:0)
 * in flat HWIO order (dgrad operand) and ohwi = the [cout][kh*kw*cin]
 * transpose (fwd operand).  Either output may be NULL.  k = kh*kw*cin.      */
int rigl_pack_weights(const float* w, const uint32_t* mask_bits /* nullable */,
                      int32_t k, int32_t cout, rigl_bf16* hwio, rigl_bf16* ohwi,
                      rigl_stream_t stream);
/* The same for a whole model in one launch per 64 tensors (`layers` is a host
 * array; it is consumed before the call returns).                          */
typedef struct RiglPackLayer {
  const float* w;
  const uint32_t* mask_bits; /* nullable */
  rigl_bf16* hwio;           /* nullable */
  rigl_bf16* ohwi;           /* nullable */
  int32_t k, cout;
} RiglPackLayer;
int rigl_pack_weights_batched(const RiglPackLayer* layers, int32_t n_layers,
                              rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * K1: masked convolution as an implicit GEMM on MFMA (bf16 in, fp32
 * accumulate).  Replaces: layers.masked_conv2d / masked_fully_connected
 *   (rigl/imagenet_resnet/pruning_layers.py:139-157, :222-233), i.e.
 *   y = conv2d(x, mask*W), and their TF autodiff:
 *   dx = conv2d_backprop_input(dy, mask*W),
 *   dW_dense = conv2d_backprop_filter(x, dy)   (dense: RigL's grow score,
 *   rigl/sparse_optimizers_base.py:478-485).
 * The weight operand is the packed bf16 shadow of mask*W (rigl_pack_weights),
 * so the mask costs no bandwidth inside the conv.
 * Padding is explicit (pad_top/left; bottom/right implied by out size), which
 * covers TF 'SAME' (incl. its asymmetric stride-2 case), 'VALID' and the
 * reference's fixed_padding (resnet_model.py:85-106).  FC = 1x1 conv, H=W=1.
 * ---------------------------------------------------------------------- */
typedef struct RiglConvDesc {
  int32_t n, h, w, cin;      /* input  NHWC  */
  int32_t ho, wo, cout;      /* output NHWC  */
  int32_t kh, kw;
  int32_t stride_h, stride_w;
  int32_t pad_top, pad_left;
} RiglConvDesc;

/* which = 0: the forwards (rigl_masked_conv2d_fwd, _fwd_stats, _fwd_relu).  For the
 * layers with cin <= 4 or cin % 8 != 0 it is the repacked operands and is
 * required (RIGL_EWORKSPACE without it).  For every other layer it is the
 * OPTIONAL scratch of a K-split plan (0 where the layer has none): with less
 * than that, or NULL, the same forward runs unsplit -- the same sum in another
 * order, never an error.
 * which = 1: always 0.  rigl_masked_conv2d_dgrad and rigl_masked_conv2d_dgrad_acc
 * take (workspace, workspace_bytes) and ignore them: pass NULL, 0.
 * which = 2: rigl_masked_conv2d_wgrad and every rigl_masked_conv2d_bwd* form
 * (the maximum over the plans the layer's backward can take), required.       */
size_t rigl_conv2d_workspace_bytes(const RiglConvDesc* d, int32_t which /*0 fwd,1 dgrad,2 wgrad*/);
int rigl_masked_conv2d_fwd(const RiglConvDesc* d, const rigl_bf16* x,
                           const rigl_bf16* w_ohwi, rigl_bf16* y,
                           void* workspace, size_t workspace_bytes,
                           rigl_stream_t stream);
int rigl_masked_conv2d_dgrad(const RiglConvDesc* d, const rigl_bf16* dy,
                             const rigl_bf16* w_hwio, rigl_bf16* dx,
                             void* workspace, size_t workspace_bytes,
                             rigl_stream_t stream);
/* Forward conv that also leaves the batch-norm statistics of its output
 * behind (the reference follows every conv with tf.layers.batch_normalization,
 * resnet_model.py:41-82, whose first pass re-reads the whole activation):
 * stats[p][0][c] = sum, stats[p][1][c] = sum of squares of the bf16-rounded
 * outputs of 128-row tile p, p < rigl_conv2d_stats_parts(d), computed in the
 * epilogue from the tile already in LDS (deterministic, no atomics).  The
 * parts are disjoint row sets that cover the output; which rows a part holds
 * is the kernel's choice: rows [128p, 128p + 128) for every layer but the
 * ImageNet stem (7x7/2, 3 -> 64 channels, knob "stem_direct"), whose kernel
 * works on 16 x 16 output-pixel tiles t = (image, tile row, tile column) and
 * leaves part 2t + h = pixel rows [8h, 8h + 8) of tile t.
 * stats == NULL: plain rigl_masked_conv2d_fwd.                              */
int32_t rigl_conv2d_stats_parts(const RiglConvDesc* d);
int rigl_masked_conv2d_fwd_stats(const RiglConvDesc* d, const rigl_bf16* x,
                                 const rigl_bf16* w_ohwi, rigl_bf16* y,
                                 float* stats, size_t stats_floats,
                                 void* workspace, size_t workspace_bytes,
                                 rigl_stream_t stream);
/* y = conv(relu(bn(x_pre)), mask*W) with the batch norm's APPLY pass done on
 * the conv's operand load (the reference runs batch_norm_relu between every
 * two convs, resnet_model.py:41-82,456-470: conv2 -> bn -> relu -> conv3):
 * x_pre = the pre-batch-norm tensor (the previous conv's output), scale_shift
 * = [2][cin] fp32, the per-channel scale = gamma * invstd and shift = beta -
 * mean * scale (rows 2-3 of rigl_bn_fwd_statistics' outputs, contiguous).
 * Every operand element becomes bf16(max(fma(x, scale, shift), 0)) -- the
 * rounding points of rigl_bn_fwd(relu = 1) -- in registers; a_out (bf16, the
 * shape of x_pre) receives that activated tensor as a side output (the
 * backward's weight-gradient operand and ReLU mask), so the separate apply
 * pass (read x_pre, write a_out) is not run.  y, a_out and the statistics
 * parts are bit-identical to rigl_bn_fwd + rigl_masked_conv2d_fwd_stats.
 * Only where rigl_conv2d_fwd_takes_bn_input(d) == 1 (1x1 / stride-1 layers on
 * the row-streaming body, knob "bn_on_load"); else RIGL_EUNSUPPORTED.  The
 * statistics parts are those of rigl_conv2d_stats_parts(d).  The body has no
 * K-split plan: (workspace, workspace_bytes) are ignored, pass NULL, 0.      */
int32_t rigl_conv2d_fwd_takes_bn_input(const RiglConvDesc* d);
int rigl_masked_conv2d_fwd_bnrelu(const RiglConvDesc* d, const rigl_bf16* x_pre,
                                  const float* scale_shift, rigl_bf16* a_out,
                                  const rigl_bf16* w_ohwi, rigl_bf16* y,
                                  float* stats /* nullable */, size_t stats_floats,
                                  void* workspace, size_t workspace_bytes,
                                  rigl_stream_t stream);
/* dx = conv2d_backprop_input(dy, mask*W) + addend: the gradient accumulation
 * TF's autodiff emits (AddN) where a tensor feeds two consumers -- a residual
 * block's input feeds conv1 and the shortcut (resnet_model.py:300-330, 374-420)
 * -- folded into the dgrad epilogue.  addend: bf16 NHWC like dx, nullable
 * (then identical to rigl_masked_conv2d_dgrad); may alias dx.
 * out = bf16(bf16(dgrad) + addend), bit-identical to dgrad followed by an add. */
int rigl_masked_conv2d_dgrad_acc(const RiglConvDesc* d, const rigl_bf16* dy,
                                 const rigl_bf16* w_hwio, const rigl_bf16* addend,
                                 rigl_bf16* dx, void* workspace,
                                 size_t workspace_bytes, rigl_stream_t stream);
/* dw: fp32 [kh][kw][cin][cout], DENSE (overwritten, not accumulated).       */
int rigl_masked_conv2d_wgrad(const RiglConvDesc* d, const rigl_bf16* x,
                             const rigl_bf16* dy, float* dw, void* workspace,
                             size_t workspace_bytes, rigl_stream_t stream);

/* dW and (dx != NULL) dX = dgrad (+ addend) of one conv in a single call, and
 * for ordinary layers a single launch: the dgrad and the split-K wgrad
 * workgroups share one grid (they are independent and each alone leaves much
 * of the chip idle), followed by the split-K reduce.  dX is bit-identical to
 * rigl_masked_conv2d_dgrad_acc; dW is the same sum split over fewer pixel ranges
 * than rigl_masked_conv2d_wgrad's plan (the weight-gradient workgroups leave
 * room for the dgrad tiles) -- deterministic, equal to it up to fp32 reassociation.
 * workspace: rigl_conv2d_workspace_bytes(d, 2).                              */
int rigl_masked_conv2d_bwd(const RiglConvDesc* d, const rigl_bf16* x,
                           const rigl_bf16* dy, const rigl_bf16* w_hwio,
                           const rigl_bf16* addend /* nullable */, float* dw,
                           rigl_bf16* dx /* nullable */, void* workspace,
                           size_t workspace_bytes, rigl_stream_t stream);

/* rigl_masked_conv2d_bwd whose addend is the gradient of a SUBSAMPLED view of
 * the conv's input: addend = bf16 [n][ceil(h / sub_h)][ceil(w / sub_w)][cin],
 * added to dX at the pixels with h % sub_h == 0 and w % sub_w == 0 (elsewhere
 * dX = dgrad).  The first block of a ResNet group reads its input twice -- conv1
 * and the strided 1x1 projection shortcut (resnet_model.py:456-501,
 * conv2d_fixed_padding with kernel 1: no padding, pixels (2i, 2j)) -- and the
 * projection's input gradient is zero off that grid; it is computed as the dgrad
 * of a stride-1 1x1 conv over the [n, ho, wo] grid (rigl_masked_conv2d_dgrad with
 * such a descriptor) and handed over compact: a quarter of the bytes written and
 * read, and none of the strided dgrad's zero rows.  dX is bit-identical to
 * rigl_masked_conv2d_bwd fed the same gradient scattered into a zero tensor.
 * Runs on the implicit-GEMM body (or, round 6, the channel-sliced single-pass
 * backward where that is the layer's kernel: the only bodies with this
 * addressing); sub_h = sub_w = 1 is rigl_masked_conv2d_bwd.                    */
/* The other half of that hand-over: the backward of a STRIDED 1x1 conv without
 * padding (ho = ceil(h / stride_h), wo likewise) with dX on the conv's own grid:
 * dx_grid = bf16 [n][ho][wo][cin], the gradient at the pixels the conv read (it is
 * zero at every other pixel, which is not written anywhere) = the dgrad of the
 * stride-1 1x1 conv over that grid; dW (dense, overwritten) from x as it lies.
 * One shared launch like rigl_masked_conv2d_bwd; workspace as for it.           */
int rigl_masked_conv2d_bwd_grid(const RiglConvDesc* d, const rigl_bf16* x,
                                const rigl_bf16* dy, const rigl_bf16* w_hwio,
                                float* dw, rigl_bf16* dx_grid, void* workspace,
                                size_t workspace_bytes, rigl_stream_t stream);
int rigl_masked_conv2d_bwd_sub(const RiglConvDesc* d, const rigl_bf16* x,
                               const rigl_bf16* dy, const rigl_bf16* w_hwio,
                               const rigl_bf16* addend, int32_t sub_h, int32_t sub_w,
                               float* dw, rigl_bf16* dx, void* workspace,
                               size_t workspace_bytes, rigl_stream_t stream);
/* rigl_masked_conv2d_bwd whose addend arrives UNMASKED with a 1-bit-per-element
 * mask (addend_bits: [n*h*w][cin / 8] bytes, bit j of a byte = channel 8 b + j;
 * set = the addend counts there): dx = bf16(bf16(dgrad) + (bit ? addend : 0)).
 * Replaces the tf.where / relu-gradient op that masks the shortcut's gradient of
 * relu(bn3 + shortcut) (rigl/imagenet_resnet/resnet_model.py:497-501 through
 * autodiff): the batch norm's backward hands its output gradient over as it is,
 * with the ReLU bits its forward left, and never writes the masked copy.  Only for
 * the layers rigl_conv2d_bwd_takes_masked_addend says 1 for (the channel-sliced
 * single-pass backward, bwdslice.hpp, and the 256 <- 64 row-streaming dgrad,
 * rowstream.hpp MODE 3, from 65 536 rows on -- knob "rs_masked_addend" = 2: from
 * the 4 096 rows that body takes, 0: never) and, beyond the query, every layer
 * whose row-streaming dgrad has the masked form; RIGL_EUNSUPPORTED otherwise.  */
int32_t rigl_conv2d_bwd_takes_masked_addend(const RiglConvDesc* d);
int rigl_masked_conv2d_bwd_masked(const RiglConvDesc* d, const rigl_bf16* x,
                                  const rigl_bf16* dy, const rigl_bf16* w_hwio,
                                  const rigl_bf16* addend, const uint8_t* addend_bits,
                                  float* dw, rigl_bf16* dx, void* workspace,
                                  size_t workspace_bytes, rigl_stream_t stream);

/* rigl_masked_conv2d_bwd of the conv IN FRONT of a batch norm (+ shortcut,
 * ReLU) whose backward apply pass is not run: `dout` is the gradient w.r.t.
 * relu(bn(y) + shortcut) and the kernel forms
 *   dy = bf16(a * (dz - b - xhat * c)),  dz = bit ? dout : 0,
 *   xhat = (y - mean) * invstd
 * on its operand load from dout, y (this conv's forward output), relu_bits
 * (rigl_bn_fwd_stats) and mean / invstd / coef[3][cout] (rigl_bn_bwd_reduce) --
 * the tensor rigl_bn_bwd would have written for this conv to read back once.
 * dX and dW are bit-identical to rigl_bn_bwd followed by rigl_masked_conv2d_bwd.
 * Only the layers rigl_conv2d_bwd_takes_bn_apply says 1 for (bwd1x1.hpp: 1x1,
 * 64 -> 256, the row counts of the single-pass kernel; knob "bn_bwd_on_load" 0:
 * none); RIGL_EUNSUPPORTED otherwise.                                          */
int32_t rigl_conv2d_bwd_takes_bn_apply(const RiglConvDesc* d);
int rigl_masked_conv2d_bwd_bnapply(const RiglConvDesc* d, const rigl_bf16* x,
                                   const rigl_bf16* dout, const rigl_bf16* w_hwio,
                                   const rigl_bf16* addend /* nullable */, float* dw,
                                   rigl_bf16* dx, void* workspace, size_t workspace_bytes,
                                   const rigl_bf16* y, const uint8_t* relu_bits,
                                   const float* mean, const float* invstd,
                                   const float* coef, rigl_stream_t stream);

/* K1d: dense depthwise convolution (depth multiplier 1), NHWC bf16, fp32 HWIO
 * weights [kh][kw][c][1] read directly.  Replaces
 * contrib_layers.separable_conv2d(num_outputs=None)
 * (rigl/imagenet_resnet/mobilenetv1_model.py:81-92) and its autodiff; these
 * layers are NOT masked in the reference.  d->cin == d->cout,
 * channels % 8 == 0.  HBM-bound, no MFMA.  dw is overwritten (dense fp32).   */
size_t rigl_depthwise_conv2d_workspace_bytes(const RiglConvDesc* d);
int rigl_depthwise_conv2d_fwd(const RiglConvDesc* d, const rigl_bf16* x,
                              const float* w, rigl_bf16* y, rigl_stream_t stream);
/* The forward that also leaves the batch-norm statistics of its output (every
 * depthwise conv of mobilenetv1_model.py:188-198 is followed by a batch norm):
 * stats[p][0][c] = sum, stats[p][1][c] = sum of squares of the bf16-rounded
 * outputs of partial row p < rigl_depthwise_conv2d_stats_parts(d) (0: shape has
 * no such epilogue: 3x3, stride 1 / 2, (channels / 8) dividing 256 do).
 * Deterministic; consumed by rigl_bn_fwd_stats.  stats == NULL: plain forward. */
int32_t rigl_depthwise_conv2d_stats_parts(const RiglConvDesc* d);
int rigl_depthwise_conv2d_fwd_stats(const RiglConvDesc* d, const rigl_bf16* x,
                                    const float* w, rigl_bf16* y, float* stats,
                                    size_t stats_floats, rigl_stream_t stream);
int rigl_depthwise_conv2d_dgrad(const RiglConvDesc* d, const rigl_bf16* dy,
                                const float* w, rigl_bf16* dx,
                                rigl_stream_t stream);
int rigl_depthwise_conv2d_wgrad(const RiglConvDesc* d, const rigl_bf16* x,
                                const rigl_bf16* dy, float* dw, void* workspace,
                                size_t workspace_bytes, rigl_stream_t stream);

/* Direct (non-MFMA) kernels, same operand layouts, any channel count: taken
 * for shapes the MFMA path reports RIGL_EUNSUPPORTED for (cin/cout not a
 * multiple of 8 -- MNIST MLP 784-300-100-10, 10-class logits) and used as an
 * independent on-device cross-check.  They validate the descriptor as the
 * MFMA entry points do (RIGL_EINVAL: a non-positive dimension, an output grid
 * inconsistent with input / stride / pad; RIGL_EUNSUPPORTED: a tensor of 2^30
 * elements or more) before a pointer is used or anything is launched.       */
int rigl_conv2d_fwd_ref(const RiglConvDesc* d, const rigl_bf16* x,
                        const rigl_bf16* w_ohwi, rigl_bf16* y,
                        rigl_stream_t stream);
int rigl_conv2d_dgrad_ref(const RiglConvDesc* d, const rigl_bf16* dy,
                          const rigl_bf16* w_hwio, rigl_bf16* dx,
                          rigl_stream_t stream);
int rigl_conv2d_wgrad_ref(const RiglConvDesc* d, const rigl_bf16* x,
                          const rigl_bf16* dy, float* dw, rigl_stream_t stream);

/* K1 in fp32 arithmetic -- the VALIDATION twin of the bf16 kernels, not the
 * measured path.  The reference trains in float32 unless --precision=bfloat16
 * (imagenet_train_eval.py:56-59, 553-554) and the path's float tolerance is
 * quoted against fp32; these three entry points compute conv(x, mask * W), dX
 * (+ addend) and the dense dW from fp32 NHWC activations and the fp32 master
 * weights (HWIO; mask_bits as in rigl_pack_weights, NULL = all ones, applied on
 * the fly) on v_mfma_f32_32x32x2_f32, any shape, deterministic (the weight
 * gradient's position slabs are summed in a fixed order; workspace =
 * rigl_conv2d_wgrad_f32_workspace_bytes(d), may be 0).  The host mirror takes
 * this path when the activations it is handed are fp32 (rigl_amd.workloads:
 * precision='float32', or knob "k1_fp32" = 1); tests/test_k1_fp32_gpu.py trains
 * WRN-22 and ResNet-50 on it against a float64 evaluation of the model.      */
int rigl_masked_conv2d_fwd_f32(const RiglConvDesc* d, const float* x,
                               const float* w_hwio, const uint32_t* mask_bits /* nullable */,
                               float* y, rigl_stream_t stream);
int rigl_masked_conv2d_dgrad_f32(const RiglConvDesc* d, const float* dy,
                                 const float* w_hwio, const uint32_t* mask_bits /* nullable */,
                                 const float* addend /* nullable, may alias dx */,
                                 float* dx, rigl_stream_t stream);
size_t rigl_conv2d_wgrad_f32_workspace_bytes(const RiglConvDesc* d);
int rigl_masked_conv2d_wgrad_f32(const RiglConvDesc* d, const float* x,
                                 const float* dy, float* dw, void* workspace,
                                 size_t workspace_bytes, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Glue between two masked convs: batch-norm with batch statistics (+ residual
 * add) (+ ReLU) on NHWC bf16 rows [m][c], fp32 parameters -- what the reference
 * runs as tf.layers.batch_normalization(fused=True) + tf.nn.relu (+ `inputs +
 * shortcut`), rigl/imagenet_resnet/resnet_model.py:41-82, 456-501.  Not a
 * graded hot-path row; fused here because it is HBM-bound and sits inside the
 * images/s number.  y = relu?(gamma*(x-mean)*invstd + beta (+ residual)).
 * Statistics are deterministic (fixed-order partial sums; the kernel's own pass
 * sums x - k and (x - k)^2 around a per-channel pivot k taken from three rows,
 * so a channel far from zero keeps its variance).  c % 8 == 0.
 * save_* ([c] fp32 each) carry mean, 1/sqrt(var+eps), gamma*invstd and
 * beta-mean*gamma*invstd to the backward call.  running_* may be NULL.
 * Backward: the ReLU mask of (bn + residual) comes from relu_bits (1 bit per
 * element, written by rigl_bn_fwd_stats: 1/16 of the bytes of y) or, failing
 * that, from y; with both NULL it is recomputed from x (no residual).  dresidual (nullable)
 * receives the relu-masked dy.  dgamma / dbeta are overwritten.
 * ---------------------------------------------------------------------- */
size_t rigl_bn_workspace_bytes(int64_t m, int32_t c);
int rigl_bn_fwd(int64_t m, int32_t c, const rigl_bf16* x,
                const rigl_bf16* residual /* nullable */, const float* gamma,
                const float* beta, float* running_mean, float* running_var,
                float momentum, float eps, int32_t relu, rigl_bf16* y,
                float* save_mean, float* save_invstd, float* save_scale,
                float* save_shift, void* workspace, size_t workspace_bytes,
                rigl_stream_t stream);
/* As rigl_bn_fwd, with the statistics pass replaced by the partial sums a
 * producer left behind: stats = [stats_parts][2][c] fp32 (sum x, sum x^2 over
 * disjoint row sets covering all m rows), e.g. from
 * rigl_masked_conv2d_fwd_stats.  stats == NULL behaves like rigl_bn_fwd
 * (workspace required); with stats the workspace may be NULL.               */
int rigl_bn_fwd_stats(int64_t m, int32_t c, const rigl_bf16* x,
                      const rigl_bf16* residual /* nullable */,
                      const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum,
                      float eps, int32_t relu, rigl_bf16* y, float* save_mean,
                      float* save_invstd, float* save_scale, float* save_shift,
                      const float* stats, int32_t stats_parts,
                      uint8_t* relu_bits /* nullable, out: ceil(m*c/8) bytes */,
                      void* workspace, size_t workspace_bytes, rigl_stream_t stream);
int rigl_bn_bwd(int64_t m, int32_t c, const rigl_bf16* x,
                const rigl_bf16* y /* nullable */,
                const uint8_t* relu_bits /* nullable */, const rigl_bf16* dy,
                const float* gamma, const float* save_mean,
                const float* save_invstd, const float* save_scale,
                const float* save_shift, int32_t relu, rigl_bf16* dx,
                rigl_bf16* dresidual /* nullable */, float* dgamma,
                float* dbeta, void* workspace, size_t workspace_bytes,
                rigl_stream_t stream);
/* rigl_bn_bwd without its apply launch: reduce + finalize, leaving dgamma,
 * dbeta and coef[3][c] (a = gamma * invstd, b = mean dz, c = mean dz * xhat) for
 * the consumer that applies dx = a * (dz - b - xhat * c) on its own operand load
 * (rigl_masked_conv2d_bwd_bnapply).  Same geometry and bits as rigl_bn_bwd's.   */
int rigl_bn_bwd_reduce(int64_t m, int32_t c, const rigl_bf16* x,
                       const uint8_t* relu_bits /* required with relu */,
                       const rigl_bf16* dy, const float* gamma, const float* save_mean,
                       const float* save_invstd, int32_t relu, float* dgamma,
                       float* dbeta, float* coef, void* workspace,
                       size_t workspace_bytes, rigl_stream_t stream);

/* Two batch norms meeting in one add: out = relu?(bn(x) + bn2(x2)) -- the first
 * block of every ResNet group, whose shortcut is projection conv + batch norm
 * (resnet_model.py:456-501: `shortcut = projection_shortcut(inputs)` ...
 * `tf.nn.relu(inputs + shortcut)`).  The normalised shortcut and (backward) the
 * relu-masked gradient are never written.  bn2's statistics come from
 * rigl_bn_fwd_statistics (scale2 / shift2 = its save_scale / save_shift); the
 * forward rounds the shortcut to bf16 where bn2 alone would have stored it and
 * the backward keeps rigl_bn_bwd's row partition, so y, relu_bits, dx, dx2 and
 * all four parameter gradients are bit-identical to rigl_bn_fwd(x2) ->
 * rigl_bn_fwd_stats(x, residual) and rigl_bn_bwd(dresidual) -> rigl_bn_bwd.
 * Backward: relu on, relu_bits required.                                      */
int rigl_bn_add_bn_fwd(int64_t m, int32_t c, const rigl_bf16* x, const rigl_bf16* x2,
                       const float* scale2, const float* shift2,
                       const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, int32_t relu,
                       rigl_bf16* y, float* save_mean, float* save_invstd,
                       float* save_scale, float* save_shift, const float* stats,
                       int32_t stats_parts, uint8_t* relu_bits /* nullable */,
                       void* workspace, size_t workspace_bytes, rigl_stream_t stream);
size_t rigl_bn_add_bn_bwd_workspace_bytes(int64_t m, int32_t c);
int rigl_bn_add_bn_bwd(int64_t m, int32_t c, const rigl_bf16* x, const rigl_bf16* x2,
                       const uint8_t* relu_bits, const rigl_bf16* dy,
                       const float* gamma, const float* save_mean, const float* save_invstd,
                       const float* gamma2, const float* save_mean2, const float* save_invstd2,
                       rigl_bf16* dx, rigl_bf16* dx2, float* dgamma, float* dbeta,
                       float* dgamma2, float* dbeta2, void* workspace,
                       size_t workspace_bytes, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Stateless random tensors with TensorFlow's bit layout:
 *   out[i] = rnd_i * scale + shift,  rnd = tf.random.stateless_{uniform,normal}
 *   (shape=[n], seed=[seed0, seed1], float32)  -- Philox-4x32-10 keyed by the
 *   scrambled seed pair, element i = lane i%4 of counter + i/4, Box-Muller for
 *   normals.  Replaces stateless_random_normal (drop noise, stddev = scale) and
 *   stateless_random_uniform (SET grow scores) of
 *   rigl/sparse_optimizers_base.py:402-418; seed0 = int32(offset +
 *   hash(name + 'drop'|'grow')), seed1 = int32(global_step).
 *   dist: 0 uniform [0,1), 1 standard normal.
 * ---------------------------------------------------------------------- */
int rigl_stateless_random(float* out, int64_t n, int32_t seed0, int32_t seed1,
                          int32_t dist, float scale, float shift,
                          rigl_stream_t stream);
/* The same for many tensors in one launch -- every layer's drop noise of one
 * mask update (the reference builds one stateless_random_normal op per layer,
 * rigl/sparse_optimizers_base.py:526-534, :411-416). */
typedef struct {
  float* out;
  int64_t n;
  int32_t seed0, seed1;
  int32_t dist;            /* 0 uniform [0,1), 1 standard normal */
  float scale, shift;
} RiglRandomItem;
int rigl_stateless_random_batched(const RiglRandomItem* items, int32_t n_items,
                                  rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Dropout (the CIFAR WideResNet's bn -> relu -> Dropout(droprate) -> conv2,
 * rigl/cifar_resnet/resnet_model.py:224-231).  TF's keep_mask =
 * random_uniform(shape) >= rate; y = x * 1/(1-rate) * keep_mask, on the
 * stateless stream above:
 *   u       = tf.random.stateless_uniform([n], seed=[seed0, *step], float32),
 *             the bits rigl_stateless_random(dist 0, scale 1, shift 0) writes
 *   keep[i] = u[i] >= rate
 *   scale   = 1.0f / (1.0f - rate)                       (fp32, on the host)
 *   y[i]    = keep[i] ? round_to_dtype(f32(x[i]) * scale) : +0      (RNE)
 *   keep_bits byte i/8, bit i%8 (LSB first) = keep[i]; ceil(n/8) bytes, the
 *   unused high bits of the last byte are 0.
 * A dropped element is a SELECT, not a multiply by 0: a dropped NaN, +-inf or
 * -0 gives +0.  Kept NaN and inf pass through (a kept finite value whose
 * product overflows rounds to inf).  rate == 0: y is bit-identical to x (quiet
 * NaNs included) and every bit is 1.
 * `step` is a DEVICE pointer to one int32, read by the kernel: a captured graph
 * freezes kernel arguments, so a replay draws fresh masks only because
 * rigl_dropout_advance (*step += 1 with int32 wrap-around, one single-lane
 * launch) moves the counter inside the graph.  The backward reads the STORED
 * bits, dx[i] = bit ? round_to_dtype(f32(dy[i]) * scale) : +0, and never
 * regenerates them: the counter may have moved since the forward.
 * dtype: 0 = bf16, 1 = fp32 (x / y, dy / dx).  16 bytes per lane where both
 * tensors are 16-byte aligned, element-wise otherwise and for the last n % 8
 * elements; the same bits either way.  Nothing past y[n-1] or past ceil(n/8)
 * bytes of keep_bits is touched.  n == 0 succeeds without a launch; a rate
 * that is NaN, < 0 or >= 1, or a NULL pointer with n > 0: RIGL_EINVAL.
 * ---------------------------------------------------------------------- */
int rigl_dropout_fwd(const void* x, void* y, uint8_t* keep_bits, int64_t n,
                     int32_t dtype, float rate, int32_t seed0,
                     const int32_t* step /* device */, rigl_stream_t stream);
int rigl_dropout_bwd(const void* dy, const uint8_t* keep_bits, void* dx,
                     int64_t n, int32_t dtype, float rate, rigl_stream_t stream);
int rigl_dropout_advance(int32_t* step /* device */, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * The CIFAR input pipeline on the device (rigl/cifar_resnet/data_helper.py:
 * per_image_standardization, 4-pixel mirror pad, random 32x32 crop, random
 * left-right flip, a reshuffle each pass).  32x32x3 images only.  One launch
 * writes batch `*step` into `out` / `out_labels` / `out_index`; everything that
 * depends on the step is derived on the device from the counter, so a captured
 * graph that holds this launch and rigl_cifar_advance replays fresh,
 * augmented, reshuffled batches across epoch boundaries with no host work.
 * tests/input_ref.py restates all of the following in NumPy, bit for bit.
 *
 * Standardization, over the ORIGINAL image (n = 3072 bytes x), before pad and
 * crop, on exact integer sums:
 *   S1 = sum x, S2 = sum x^2 (int);  D = n*S2 - S1*S1 (int64, >= 0)
 *   den = max(sqrtf((float)D), sqrtf(3072.f));  inv = 1.0f / den
 *   y32 = (float)(n*x - S1) * inv          ((float) conversions and sqrtf, /,
 *                                            * correctly rounded, RNE)
 *   out = y32 (dtype 1, fp32) or y32 rounded to nearest even (dtype 0, bf16)
 * This is tf.image.per_image_standardization, (x - mean) / max(stddev,
 * 1/sqrt(n)), with numerator and denominator scaled by n: n*x - S1 is an exact
 * integer below 2^24, so a low-variance image loses nothing to cancellation;
 * a constant image gives +0 everywhere.
 *
 * Augmentation (mode 0, train), on the standardized image.  The padded image
 * has coordinates 0..39 in both directions and mirrors WITH the edge pixel
 * (NumPy 'symmetric': rows 3,2,1,0 in front, 31,30,29,28 behind):
 *   src(p) = 3 - p (p < 4),  p - 4 (4 <= p < 36),  67 - p (p >= 36)
 *   out[i][r][c] = y[src(r + oy)][src(c' + ox)],  c' = flip ? 31 - c : c
 * (the crop first, then the flip of the cropped image).  Image i of the batch
 * at step s draws from Philox block i -- words w0..w3 = elements 4i..4i+3 -- of
 * tf.random.stateless_uniform's uint32 stream under the seed pair
 * [seed0, s] (the GenerateKey scramble of rigl_stateless_random):
 *   oy = w0 % 9,  ox = w1 % 9,  flip = Uint32ToFloat(w2) < 0.5f;  w3 unused.
 *
 * Sample order (train).  s is *step read as uint32 (a negative step counts as
 * its bit pattern; in the seed pair above it is the int32 itself).
 *   spe = n_images / (batch * n_shards)      steps per epoch; the last
 *         n_images % (batch * n_shards) positions of an epoch's order are skipped
 *   e = s / spe;   p = (s % spe) * batch * n_shards + shard * batch + i
 *   dataset index = pi_e(p), a keyed bijection of [0, n_images):
 *   a balanced Feistel network over 2h bits, h = max(1, ceil(bit_length(
 *   n_images - 1) / 2)), 6 rounds, round keys k0..k5 = the first six uint32 of
 *   the stateless stream under the seed pair [seed0 ^ 0x5eed, int32(e)]:
 *     v = (L << h) | R;  per round r: (L, R) <- (R, L ^ (((R ^ k_r) *
 *     0x9E3779B1u mod 2^32) >> (32 - h)));  result (L << h) | R
 *   re-applied while the result is >= n_images (cycle walking).
 * No permutation is stored anywhere.
 *
 * Eval (mode 1): no crop, flip or shuffle; *step (as uint32) is the batch
 * index b and image i is dataset index (b * n_shards + shard) * batch + i.
 * Images whose index is >= n_images are NOT written: a final partial batch
 * leaves the tail of out / out_labels / out_index untouched.
 *
 * images: uint8 [n_images, 32, 32, 3] (HWC), labels: int32 [n_images]; both
 * are only read.  out: [batch, 32, 32, 3] of dtype; out_labels, out_index:
 * int32 [batch], out_index (the dataset index of each image) may be NULL.
 * Nothing past element `batch` of the three outputs is touched.  images and
 * out must be 16-byte aligned, the int32 arrays 4-byte.  RIGL_EINVAL, with a
 * message and before any launch, for: batch <= 0; a NULL images / labels /
 * step / out / out_labels; n_images <= 0 or > 2^30; mode not 0 / 1; dtype not
 * 0 / 1; shard outside [0, n_shards); train mode with n_images < batch *
 * n_shards; a misaligned pointer.
 * rigl_cifar_advance: *step += 1 with int32 wrap-around, one single-lane
 * launch, as rigl_dropout_advance.
 * ---------------------------------------------------------------------- */
int rigl_cifar_batch(const uint8_t* images, const int32_t* labels,
                     int64_t n_images, int32_t batch, int32_t mode,
                     int32_t shard, int32_t n_shards, int32_t seed0,
                     const int32_t* step /* device */, void* out, int32_t dtype,
                     int32_t* out_labels, int32_t* out_index /* or NULL */,
                     rigl_stream_t stream);
int rigl_cifar_advance(int32_t* step /* device */, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Glue: max pooling, NHWC bf16 (tf.layers.max_pooling2d(3, 2, 'SAME') after the
 * stem, rigl/imagenet_resnet/resnet_model.py:637-644).  The descriptor is a
 * RiglConvDesc with cin == cout (% 8 == 0); padding explicit, windows clipped
 * to the image.  argmax: 1 byte per output element (r*kw+s of the FIRST
 * maximum in row-major window order); the backward is a deterministic gather.
 * ---------------------------------------------------------------------- */
int rigl_maxpool_fwd(const RiglConvDesc* d, const rigl_bf16* x, rigl_bf16* y,
                     uint8_t* argmax, rigl_stream_t stream);
int rigl_maxpool_bwd(const RiglConvDesc* d, const rigl_bf16* dy,
                     const uint8_t* argmax, rigl_bf16* dx, rigl_stream_t stream);
/* The stem's tail in one piece: batch_norm_relu followed by that max pooling
 * (resnet_model.py:631-644) without the activated 112x112x64 tensor -- 205 MB at
 * batch 128 -- ever being written.
 *   rigl_bn_fwd_statistics: the statistics half of rigl_bn_fwd_stats (reduction
 *     pass over x unless `stats` partial sums are given, then mean / invstd /
 *     scale / shift and the moving averages); no apply pass.
 *   rigl_bn_relu_maxpool_fwd: y, argmax = maxpool(bf16(relu(x*scale + shift))),
 *     bit-identical to rigl_bn_fwd followed by rigl_maxpool_fwd.
 *   rigl_bn_relu_maxpool_bwd: dx, dgamma, dbeta of the pair from the pooled
 *     gradient dy: both batch-norm passes gather the pooling's input gradient
 *     (rounded to bf16 as rigl_maxpool_bwd stores it) from dy / argmax on the fly.
 *     dx equals rigl_maxpool_bwd + rigl_bn_bwd up to the fp32 summation order of
 *     the two reductions.  3x3 / stride 2, (channels / 4) dividing 64.          */
int rigl_bn_fwd_statistics(int64_t m, int32_t c, const rigl_bf16* x /* nullable with stats */,
                           const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum,
                           float eps, float* save_mean, float* save_invstd,
                           float* save_scale, float* save_shift,
                           const float* stats, int32_t stats_parts,
                           void* workspace, size_t workspace_bytes, rigl_stream_t stream);
int rigl_bn_relu_maxpool_fwd(const RiglConvDesc* d, const rigl_bf16* x,
                             const float* scale, const float* shift, rigl_bf16* y,
                             uint8_t* argmax, rigl_stream_t stream);
size_t rigl_bn_relu_maxpool_bwd_workspace_bytes(const RiglConvDesc* d);
int rigl_bn_relu_maxpool_bwd(const RiglConvDesc* d, const rigl_bf16* x,
                             const rigl_bf16* dy, const uint8_t* argmax,
                             const float* gamma, const float* save_mean,
                             const float* save_invstd, const float* save_scale,
                             const float* save_shift, rigl_bf16* dx, float* dgamma,
                             float* dbeta, void* workspace, size_t workspace_bytes,
                             rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Glue: classifier head.  Global average pool over `pixels` positions of an
 * NHWC bf16 map (average_pooling2d + reshape, resnet_model.py:701-712; fp32
 * accumulation, c even) and tf.losses.softmax_cross_entropy with label
 * smoothing (imagenet_train_eval.py:578-584) on bf16 logits: row_loss[r] =
 * -sum_k t_k log softmax(z)_k with t = onehot * (1 - eps) + eps / K, and --
 * when dlogits is given -- dlogits = bf16((softmax(z) - t) * grad_scale), the
 * gradient of grad_scale * sum_r row_loss[r] (grad_scale = 1 / rows for the mean).
 * A label outside [0, classes) is not an error: as with tf.one_hot
 * (imagenet_train_eval.py:569-581) its one-hot row is all zero, t = eps / K for
 * every class, so row_loss is the smoothing term alone (0 when eps = 0) and
 * dlogits = bf16((softmax(z) - eps / K) * grad_scale) -- loss and gradient of
 * the same function.  rigl_eval_metrics reports the same row loss.
 * ---------------------------------------------------------------------- */
int rigl_global_avgpool_fwd(int32_t n, int32_t pixels, int32_t c, const rigl_bf16* x,
                            rigl_bf16* y, rigl_stream_t stream);
int rigl_global_avgpool_bwd(int32_t n, int32_t pixels, int32_t c, const rigl_bf16* dy,
                            rigl_bf16* dx, rigl_stream_t stream);
/* The spatial mean's gradient through the ReLU in front of it (VGG's last conv):
 * dx[n,p,c] = bf16(float(dy[n,c]) / P) * [x[n,p,c] > 0], x = the pooled ReLU
 * output; c % 8 == 0, 16-byte aligned tensors. */
int rigl_global_avgpool_bwd_relu(int32_t n, int32_t pixels, int32_t c, const rigl_bf16* dy,
                                 const rigl_bf16* x, rigl_bf16* dx, rigl_stream_t stream);
int rigl_softmax_xent(int32_t rows, int32_t classes, const rigl_bf16* logits,
                      const int64_t* labels, float label_smoothing, float grad_scale,
                      float* row_loss, rigl_bf16* dlogits /* nullable */, rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Masked conv + ReLU without a batch norm (VGG, rigl/imagenet_resnet/vgg.py:
 * 124-134: conv2d_fixed_padding followed by tf.nn.relu).
 *   rigl_masked_conv2d_fwd_relu: y = bf16(max(conv(x, w), 0)), +0 for every
 *     non-positive value, applied after the complete reduction; the
 *     pre-activation is never stored.
 *   rigl_masked_conv2d_bwd_relu: dW (dense fp32) as rigl_masked_conv2d_bwd and
 *     dX = bf16(dgrad(dy)) * [x > 0].  x is the conv's input AND a ReLU output
 *     (or a max pool of one: at the pool winner the ReLU output is the pooled
 *     value), so dX is the gradient the ReLU in front passes on; dy must arrive
 *     gated by this conv's own ReLU (its consumer's dX, or
 *     rigl_global_avgpool_bwd_relu).
 * Both run the ReLU in the epilogue of the body the layer selects where that
 * body has one (rigl_conv2d_fwd_takes_relu_epilogue /
 * rigl_conv2d_bwd_takes_relu_epilogue = 1: the igemm and ping-pong bodies),
 * else the plain kernels followed by the stand-alone passes below; the bits
 * are the same either way.  Knob "relu_fuse" = 0 forces the stand-alone passes.
 *   rigl_relu_fwd: y = relu(x) (in place allowed); rigl_relu_bwd: dx = dy *
 *   [x > 0] (in place on dy allowed).  n % 8 == 0, 16-byte aligned tensors.
 * Shapes whose bf16 tensors reach 2^30 elements: RIGL_EUNSUPPORTED.
 * ---------------------------------------------------------------------- */
int32_t rigl_conv2d_fwd_takes_relu_epilogue(const RiglConvDesc* d);
int32_t rigl_conv2d_bwd_takes_relu_epilogue(const RiglConvDesc* d);
int rigl_masked_conv2d_fwd_relu(const RiglConvDesc* d, const rigl_bf16* x,
                                const rigl_bf16* w_ohwi, rigl_bf16* y, void* workspace,
                                size_t workspace_bytes, rigl_stream_t stream);
int rigl_masked_conv2d_bwd_relu(const RiglConvDesc* d, const rigl_bf16* x,
                                const rigl_bf16* dy, const rigl_bf16* w_hwio, float* dw,
                                rigl_bf16* dx, void* workspace, size_t workspace_bytes,
                                rigl_stream_t stream);
int rigl_relu_fwd(int64_t n, const rigl_bf16* x, rigl_bf16* y, rigl_stream_t stream);
int rigl_relu_bwd(int64_t n, const rigl_bf16* dy, const rigl_bf16* x, rigl_bf16* dx,
                  rigl_stream_t stream);

/* ------------------------------------------------------------------------
 * Evaluation (the reference's EVAL mode, imagenet_train_eval.py:596-615 and
 * :771-790): frozen-statistics batch norm and the eval metrics.
 *   rigl_bn_infer_params_batched: for every item, scale_shift[2][c] =
 *     {gamma * invstd, beta - moving_mean * scale} with invstd =
 *     (float)(1 / sqrt((double)moving_variance + eps)) -- the algebra of the
 *     training finalize with the moving statistics; one launch for all items.
 *   rigl_bn_apply: y = bf16(relu?(fmaf(x, scale, shift) (+ residual))), the
 *     training forward's apply pass (bit-identical to it, no ReLU bits).
 *   rigl_bn_apply_pair: y = bf16(relu?(fmaf(x, scale, shift) +
 *     bf16(fmaf(x2, scale2, shift2)))), the pair kernel of rigl_bn_add_bn_fwd.
 *   rigl_bn_relu_maxpool_infer: rigl_bn_relu_maxpool_fwd without argmax.
 *   rigl_conv2d_fwd_takes_bn_epilogue / rigl_masked_conv2d_fwd_bn_infer: the
 *     1x1 / stride-1 forward of the row-streaming body with the frozen batch
 *     norm behind it in its epilogue, y = bf16(relu?(fmaf(conv(a), scale,
 *     shift) (+ residual))), bit-identical to rigl_masked_conv2d_fwd followed by
 *     rigl_bn_apply; a = x, or with in_scale_shift (bn_on_load) a =
 *     bf16(relu(fmaf(x, in_scale, in_shift))) formed on the operand load as
 *     rigl_masked_conv2d_fwd_bnrelu does (no side output written).  Without
 *     scale_shift (only with in_scale_shift) y is the raw conv.  The transform
 *     with a residual is not taken on the 128-column variants (K <= 256).
 *     Where the query says 0 (knob "eval_fuse" 0: every layer) the entry returns
 *     RIGL_EUNSUPPORTED and the caller runs the separate passes.
 *   rigl_eval_metrics: one workgroup per row of bf16 logits [rows][classes]:
 *     row_loss = rigl_softmax_xent's row loss (the same bits); row_flags[r] =
 *     top-1 hit | top-k hit << 1.  Top-1: the label equals the smallest index
 *     among the row's maxima (tf.argmax; a row with a NaN follows np.argmax --
 *     the reference does not pin that case).  Top-k: TF InTopK -- false for a
 *     label out of range, a non-finite label logit or any non-finite logit in
 *     the row, else #{j : z_j > z_label} < topk.  counts (nullable, int64 [3]:
 *     rows, top-1 hits, top-k hits) are added to atomically.  classes <= 8192.
 * ---------------------------------------------------------------------- */
typedef struct RiglBnInferItem {
  const float* gamma;
  const float* beta;
  const float* moving_mean;
  const float* moving_variance;
  float* scale_shift;        /* [2][c] out */
  int32_t c;
  float eps;
} RiglBnInferItem;
int rigl_bn_infer_params_batched(const RiglBnInferItem* items, int32_t n_items,
                                 rigl_stream_t stream);
int rigl_bn_apply(int64_t m, int32_t c, const rigl_bf16* x,
                  const rigl_bf16* residual /* nullable */, const float* scale_shift,
                  int32_t relu, rigl_bf16* y, rigl_stream_t stream);
int rigl_bn_apply_pair(int64_t m, int32_t c, const rigl_bf16* x, const rigl_bf16* x2,
                       const float* scale_shift, const float* scale_shift2,
                       int32_t relu, rigl_bf16* y, rigl_stream_t stream);
int rigl_bn_relu_maxpool_infer(const RiglConvDesc* d, const rigl_bf16* x,
                               const float* scale_shift, rigl_bf16* y,
                               rigl_stream_t stream);
int32_t rigl_conv2d_fwd_takes_bn_epilogue(const RiglConvDesc* d, int32_t bn_on_load,
                                          int32_t residual);
int rigl_masked_conv2d_fwd_bn_infer(const RiglConvDesc* d, const rigl_bf16* x,
                                    const float* in_scale_shift /* nullable */,
                                    const rigl_bf16* w_ohwi,
                                    const float* scale_shift /* nullable */,
                                    const rigl_bf16* residual /* nullable */,
                                    int32_t relu, rigl_bf16* y, rigl_stream_t stream);
int rigl_eval_metrics(int32_t rows, int32_t classes, const rigl_bf16* logits,
                      const int64_t* labels, float label_smoothing, int32_t topk,
                      float* row_loss, int32_t* row_flags,
                      int64_t* counts /* nullable */, rigl_stream_t stream);

/* Optional per-kernel timing (HIP events recorded on the launch stream around
 * every K1/K2/K3 launch while enabled).  rigl_prof_collect synchronises the
 * recorded events and returns accumulated milliseconds / launch counts per
 * kernel family: 0 conv_fwd, 1 conv_dgrad, 2 conv_wgrad, 3 prune_regrow,
 * 4 sgd_momentum, 5 pack_weights, 6 conv_bwd (the fused dgrad + wgrad launch
 * of rigl_masked_conv2d_bwd, with its split-K reduce), 7 depthwise (K1d, the
 * three rigl_depthwise_conv2d_* entry points).                              */
#define RIGL_PROF_KINDS 8
int rigl_prof_enable(int32_t on);
int rigl_prof_collect(double* ms_per_kind /*[8]*/, int64_t* launches /*[8]*/);
/* The same over the first n_kinds (<= RIGL_PROF_KINDS_ALL) families: kind
 * 8 = masked_adam (rigl_masked_adam and rigl_adam_advance), 9 =
 * magnitude_prune (rigl_magnitude_prune_batched).  rigl_prof_collect keeps
 * its eight-entry contract and drops the events of kinds 8 and up.          */
#define RIGL_PROF_KINDS_ALL 10
int rigl_prof_collect_kinds(double* ms_per_kind, int64_t* launches, int32_t n_kinds);
/* The same events one by one, in launch order (instead of rigl_prof_collect,
 * which consumes them too): kind as above; tag = (h, w, cin, cout, kh, stride_h)
 * of the conv descriptor the launch belongs to (zeros for K2 / K3 / pack); ms =
 * that dispatch's own duration.  Writes at most `cap` records, returns the
 * number of recorded launches in *n_launches (the rest is dropped).  For the
 * per-layer IN-STEP table of tools/instep_table.py.    */
typedef struct RiglProfLaunch {
  int32_t kind;
  int32_t tag[6];
  float ms;
} RiglProfLaunch;
int rigl_prof_collect_launches(RiglProfLaunch* out /* host */, int64_t cap, int64_t* n_launches);

/* Measurement aid (the MFMA peak "re-measured on the box"):
 * enqueues blocks x 4 waves, each issuing iters x 8 independent
 * v_mfma_f32_32x32x16_bf16 (32768 FLOP per wave-instruction) on register
 * operands; the caller brackets it with events.  `sink`: blocks*256 floats.  */
int rigl_probe_mfma_bf16(int32_t blocks, int32_t iters, float* sink, rigl_stream_t stream);

/* Development knobs: the run-time twin of the RIGL_* environment variables, so
 * that one process can A/B kernel selections (tools/pp_sweep.py,
 * tests/k1_check.py).  Process-wide state, NOT part of the drop-in surface: a
 * caller that never sets a knob gets the built-in selection rules; a knob never
 * set reads the environment variable RIGL_<KEY IN UPPER CASE> once.  Keys:
 *   "pp_fwd" / "pp_dgrad"   K1 tile of the 8-wave ping-pong body for the
 *                           forward / stand-alone dgrad GEMM: -1 built-in rule
 *                           (default), 0 never, 1 256x256, 2 128x256,
 *                           3 256x128, 4 512x128 (ignored where the shape does
 *                           not admit the tile);
 *   "pp_bwd"                the shared backward launch on the ping-pong bodies
 *                           (dgrad tiles + 256x256 weight-gradient tiles): -1
 *                           rule, 0 never, 1 / 2 dgrad on 256x256 / 128x256;
 *   "pp_wgrad"              1: stand-alone weight gradient on the ping-pong
 *                           body wherever legal (rule: off);
 *   "pp_slab_mb"            cap on a layer's split-K slab bytes (40);
 *   "pp_bwd_min_kt"         shortest dgrad reduction (K-tiles of 64) the
 *                           pp_bwd rule takes (16);
 *   "wgrad_il"              0: the splits of a weight gradient take contiguous
 *                           pixel ranges instead of interleaved K-tiles (1);
 *   "pp_ksplit"             0: no two-way K split of the few-tile forwards
 *                           (7x7 3x3 layers at batch 128) (1);
 *   "bn_il"                 0: a batch-norm reduction part is a contiguous range
 *                           of rows instead of every parts-th group (1);
 *   "bn_nt"                 non-temporal accesses of the batch-norm apply
 *                           passes: 0 none, 1 stores, 2 loads and stores (2;
 *                           -0.10 ms per ResNet-50 step); "bn_nt_mb" applies it
 *                           only to tensors of at least that many MB (0);
 *   "stem_wgrad"            0: only the stem's forward on stem.hpp (1);
 *   "stem_direct"           0: the ImageNet stem through the generic bodies
 *                           over a padded 4-channel copy instead of the
 *                           LDS-resident-patch kernels (1);
 *   "bwd1x1"                0: the single-pass backward of the 56x56-class 1x1
 *                           layers (64->256, 64->64; dY read once) off (1);
 *   "bwd1x1_il"             0: contiguous pixel ranges per workgroup instead of
 *                           interleaved K-tiles (1); "bn_fin1" 0: the one-level
 *                           forward batch-norm finalize for every size (1);
 *   "c3x3"                  0: the 3x3 / 64 -> 64 / stride-1 layers (24 <= w <=
 *                           62) through the generic bodies instead of the
 *                           LDS-resident-patch kernels of c3x3.hpp (1);
 *   "rowstream"             the row-streaming body of the 1x1 / stride-1 GEMMs
 *                           (rowstream.hpp: rows global -> registers, the
 *                           filter slice stationary in LDS): 0 never, 1 the
 *                           layers it measured faster on in the step (default:
 *                           forwards with reductions <= 256 channels, the
 *                           256 <- 64 dgrad), 2 every legal layer (reductions
 *                           of 64 .. 512 channels, both directions);
 *   "k1_fp32"               1: rigl_amd.workloads hands the models fp32
 *                           activations (the fp32 validation kernels of K1;
 *                           read by the host mirror, not by the library) (0).
 * rigl_conv2d_stats_parts(d) follows these selections: the c3x3 / rowstream kernels
 * leave ONE statistics part per persistent workgroup (of a column slice), not one per 128 rows.
 * Knobs whose A/B measurements said "no" in rounds 2-4 are gone with their
 * kernels (k1_nt_mb, pp_ph, bwd1x1_wgs, bwd1x1_256x64, stem_nt, RIGL_WGRAD_DEFER,
 * RIGL_WGRAD_STREAM, RIGL_CONV_STAGES, RIGL_CONV_W4_KT, RIGL_WGRAD_TR; round 4
 * also measured and did not keep bn_parts / bn_rpl and a side-stream reduce;
 * round 5 replaced x1x1.hpp and its knobs by rowstream.hpp).
 * Round 6: "bwdslice" (0 = off, 1 = default: the channel-sliced single-pass
 * backward of the 1x1 / stride-1 layers with cin % 128 == 0 and cout 128 / 256,
 * bwdslice.hpp) with "bwdslice512" (0 / 1 = default: its 64-channel-slice form
 * for cout 512, cin % 64 == 0); "bn_on_load" (0: rigl_conv2d_fwd_takes_bn_input says 0 for
 * every layer; 1 = default: the row-streaming forwards except the 64-channel /
 * 128-column variant take the transform -- whether a model USES the entry point
 * is the caller's choice: the host mirror does with RIGL_BN_ON_LOAD=1 only, it
 * measured 0.03 ms slower per ResNet-50 step).
 * No reference counterpart (the reference selects cuDNN/TPU algorithms inside
 * TensorFlow: rigl/imagenet_resnet/pruning_layers.py:139-157).              */
int rigl_tune_set(const char* key, int32_t value);
int32_t rigl_tune_get(const char* key, int32_t dflt);
/* Back to "never set" (the RIGL_<KEY> environment variable, else the built-in
 * default); rigl_tune_set(key, INT32_MIN) is the same call.                  */
int rigl_tune_unset(const char* key);
/* Counts the rigl_tune_set / rigl_tune_unset calls of this process: whoever caches
 * a plan-dependent answer of the library (rigl_conv2d_stats_parts,
 * rigl_conv2d_workspace_bytes ...) keys the cache on it -- a knob flipped through
 * ANY binding then invalidates it (the Python mirror does: ops._plan_cached). */
uint64_t rigl_tune_generation(void);
/* The address of that counter (valid for the life of the process; read it as a
 * volatile uint64): a binding that checks it on every call -- launch-bound models
 * make hundreds of cached-plan lookups per step -- reads memory instead of
 * crossing the FFI.                                                           */
const volatile uint64_t* rigl_tune_generation_addr(void);

#ifdef __cplusplus
}
#endif
#endif /* RIGL_HIP_H_ */
