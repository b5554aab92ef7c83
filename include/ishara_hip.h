/* ishara_hip.h — C ABI of libishara_hip.so: the MI355X (gfx950) hot path of the Ishara
 * ASL-fingerspelling recogniser (Conv1D -> Squeezeformer -> Conformer CTC encoder).
 *
 * The reference (tanmayrainanda/ishara) has no native code and no FFI: its hot path is the
 * Keras object built by get_model(...) in `Test Notebooks/conv-hybrid-model.ipynb` and
 * driven by model.fit.  Each entry point below names the reference construct it replaces.
 *
 * Conventions: every function returns 0 on success, <0 on error (ishara_last_error() gives
 * a thread-local message).  The CALLER owns every buffer (parameters, gradients, optimizer
 * slots, workspace, inputs, outputs; torch-ROCm tensors in the Python host).  The library
 * allocates no device memory, never synchronises, and launches everything on the hipStream_t
 * it is given.  A handle is bound to the device current at ishara_bind() and is not
 * thread-safe: one handle per rank.
 */
#ifndef ISHARA_HIP_H
#define ISHARA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ishara_model ishara_model;
typedef void* ishara_stream;              /* hipStream_t */

/* activation storage + MFMA input type.  ISHARA_F16: inference only (the fp16 TFLite export of c14:1-5; ishara_forward(training=1)
 * is refused) — weights and activations in fp16, fp16 MFMA with fp32 accumulation, fp32 statistics / softmax / logits. */
enum { ISHARA_F32 = 0, ISHARA_BF16 = 1, ISHARA_F16 = 2 };
/* model families behind one handle type: the Keras hybrid of get_model (conv-hybrid-model.ipynb c7:1-72), the torch
 * ConformerEncoder of conformer/conformer.py:76-87 (post-LN blocks, encoder stack only) and the torch SqueezeformerEncoder of
 * squeezeformer/encoder.py:26-166 (conv2d subsampling, relative-position MHSA, time reduction / recovery) */
enum { ISHARA_FAMILY_KERAS_HYBRID = 0, ISHARA_FAMILY_TORCH_CONFORMER = 1, ISHARA_FAMILY_TORCH_SQUEEZEFORMER = 2 };

/* get_model(...) kwargs — conv-hybrid-model.ipynb c7:1-11 — plus the notebook globals the
 * function closes over (INPUT_SHAPE c3:119, len(char_to_num) c1:7) and the variant knobs
 * of the sibling notebooks (top_conv width, per-family expansion). 0 / negative = default. */
typedef struct ishara_config {
    int32_t dim;
    int32_t num_conv_squeeze_blocks;
    int32_t num_conv_conform_blocks;
    int32_t num_kernel_sizes;
    int32_t kernel_sizes[8];
    int32_t num_conv_per_block;
    float   dropout_rate;
    int32_t num_heads;
    int32_t expansion_factor;
    int32_t transformer_kernel_size;
    int32_t frames;                 /* T  = INPUT_SHAPE[0] */
    int32_t features;               /* F  = INPUT_SHAPE[1] */
    int32_t num_classes;            /* 60; blank = num_classes-1 */
    int32_t top_dim;                /* 0 -> 2*dim (c7:61) */
    int32_t squeeze_expansion;      /* 0 -> expansion_factor */
    int32_t conformer_expansion;    /* 0 -> expansion_factor */
    float   head_dropout;           /* c7:62: 0.4 */
    float   conformer_attn_dropout; /* c5:312 default 0.1 */
    int32_t dtype;                  /* ISHARA_F32 | ISHARA_BF16 | ISHARA_F16 (inference only): activation storage + MFMA input type */
    int32_t max_batch;              /* workspace is planned for this many clips */
    int32_t max_label_len;          /* MAX_PHRASE_LENGTH = 64 (c1:28) */
    int32_t attn_impl;              /* 0 lane-split VALU, 1 MFMA (bf16 only) */
    int32_t family;                 /* ISHARA_FAMILY_*.  TORCH_CONFORMER reads: dim, num_conv_conform_blocks (= num_layers), num_heads,
                                     * expansion_factor, transformer_kernel_size (= kernel_size, odd), dropout_rate, frames, dtype, max_batch */
    /* ISHARA_FAMILY_TORCH_SQUEEZEFORMER (encoder.py:54-69) reads: features (= input_dim), dim (= encoder_dim), num_conv_conform_blocks
     * (= num_layers), num_heads, expansion_factor (= feed_forward_expansion_factor), transformer_kernel_size (= conv_kernel_size),
     * dropout_rate (all five dropout probabilities), frames (input frames, any count >= 7), dtype, max_batch and: */
    int32_t reduce_layer_index;     /* >= num_layers: no time reduction */
    int32_t recover_layer_index;    /* >= num_layers: no recovery */
    int32_t half_step_residual;     /* 0 | 1 */
} ishara_config;

const char* ishara_last_error(void);

/* tf.keras.Model construction (c7:12-65).  Host only: touches no GPU. */
int  ishara_create(const ishara_config* cfg, ishara_model** out);
void ishara_destroy(ishara_model* m);

/* model.summary() / model.weights (c7:83): flat fp32 parameter buffer layout.  Trainable
 * entries come first (offsets [0, trainable)), BatchNorm moving statistics after them, so
 * the gradient buffer [0, trainable) is one contiguous all-reduce bucket. */
int64_t ishara_param_total(const ishara_model* m);
int64_t ishara_param_trainable(const ishara_model* m);
int32_t ishara_param_entries(const ishara_model* m);
int  ishara_param_info(const ishara_model* m, int32_t i, const char** name, int32_t* ndim,
                       int64_t shape[2], int64_t* offset, int32_t* trainable);
int64_t ishara_workspace_bytes(const ishara_model* m);

/* Debug aids (no reference counterpart).  plan_check: host-side audit of the workspace plan (alignment, bounds, no overlap);
 * returns the buffer count.  guard_check: with ISHARA_WS_GUARD=1 in the environment at ishara_create every workspace buffer is
 * followed by a 256-byte guard zone armed by ishara_bind; returns 0 if all guards are intact (synchronises the device). */
int32_t ishara_workspace_plan_check(const ishara_model* m);
int ishara_workspace_guard_check(ishara_model* m);

/* Bind caller-owned device buffers.  params/grads: ishara_param_total floats (grads only
 * uses the trainable prefix); opt_m/opt_v/opt_slow: ishara_param_trainable floats each
 * (may be NULL for inference); workspace: ishara_workspace_bytes bytes, 256-B aligned. */
int ishara_bind(ishara_model* m, float* params, float* grads, float* opt_m, float* opt_v,
                float* opt_slow, void* workspace, int64_t workspace_bytes);
/* Re-derive the MFMA-typed weight shadows after the caller wrote `params` (load_weights). */
int ishara_sync_weights(ishara_model* m, ishara_stream s);

/* model(x, training=...) — c7:82, c9:15, c13:17.  x [B,T,F] f32, logits [B,T,C] f32. */
int ishara_forward(ishara_model* m, const float* x, int32_t B, float* logits, int32_t training,
                   uint32_t seed, ishara_stream s);
/* CTCLoss (c6:1-13) + tape.gradient of Keras train_step (c12).  Uses the activations saved
 * by the last ishara_forward(training=1).  labels [B,L] int64 padded with blank.
 * loss (device scalar) = mean_b nll_b; gradients of loss*loss_scale fill grads[0,trainable). */
int ishara_loss_backward(ishara_model* m, const float* logits, const int64_t* labels, int32_t B,
                         float* loss, float* nll, float loss_scale, ishara_stream s);
/* The same pair with per-clip frame lengths: the padding mask the reference's layers were written for (Masking(0.0), conv-hybrid-model.ipynb c7;
 * its own get_model loses the mask at x + pe).  frame_len: device int32 [B], 4-byte aligned; clip b has n_b = frame_len[b] real frames, frames
 * t >= n_b are padding; clamped to [0,T] on the device, never read by the host (no synchronise, graph-capturable).  Exactly the three
 * operations the reference's layers mask are masked: the keys j >= n_b of every MultiHeadSelfAttention (c5:109-112), the time mean of the ECA
 * gate of every Conv1DBlock (c5:8-9) and of the Squeeze-Excite gate of the Squeezeformer ConvModule (c5:129-130), each with its backward.
 * Dense, LayerNorm, the depthwise convolutions, BatchNorm (statistics over all B*T rows, as Keras's BatchNormalization ignores the mask), the
 * positional encoding, the head and the CTC loss (logit_length = T, c6:3) see the padded frames as without lengths.  n_b = 0: the clip's
 * attention output and both means are 0 (Keras: NaN).  The caller owns the array and passes it again to ishara_loss_backward_ex; the library
 * keeps only whether the last training forward had lengths and refuses a backward call that disagrees.  frame_len == NULL: the plain calls
 * above, bit for bit, on the kernels they launch.  ISHARA_F16 with lengths and the encoder-only families are refused before any GPU work. */
int ishara_forward_ex(ishara_model* m, const float* x, int32_t B, float* logits, int32_t training, uint32_t seed, const int32_t* frame_len,
                      ishara_stream s);
int ishara_loss_backward_ex(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale,
                            const int32_t* frame_len, ishara_stream s);
/* The same backward pass with a second loss term, minimum-risk training over an n-best list: between the CTC kernel and the head one stage,
 * ishara_ctc_nbest_grad's kernels on the model's own dlogits with accumulate = 1, grad_scale = risk_scale / B, frame_len = NULL (the risk
 * term keeps logit_length = T as the CTC loss does) and the model's padded 16-bit copy as dlb, so the gradients are those of
 * loss_scale * mean_b nll_b + risk_scale / B * sum_b sum_n coef[b,n] * nll(hyp[b,n]).  hyp_idx [B,N,Th], hyp_len [B,N], max_len, coef [B,N]
 * and workspace as ishara_ctc_nbest_grad (T and C are the model's, blank = C - 1), with its refusals; frame_len as ishara_loss_backward_ex
 * (NULL: the unmasked pass).  loss and nll keep their meaning: the CTC loss of the reference label.  Every other launch is
 * ishara_loss_backward_ex's, with the same arguments. */
int ishara_loss_backward_nbest(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale,
                               const int32_t* frame_len /* may be NULL */, const int32_t* hyp_idx, const int32_t* hyp_len, int32_t N, int32_t Th,
                               int32_t max_len, const float* coef, float risk_scale, void* workspace, ishara_stream s);
/* The same backward pass with knowledge distillation as a further loss term, and the risk term beside it when wanted.  The order between the
 * CTC kernel and the head is fixed: the CTC kernel, then the n-best stage when `nbest` is given (exactly ishara_loss_backward_nbest's), then
 * the distillation stage when `kd` is given: ishara_kd_grad's kernels on the model's own dlogits with accumulate = 1,
 * grad_scale = kd_scale / B, frame_len = NULL (the term keeps logit_length = T as the CTC loss and the risk term do) and the model's padded
 * 16-bit copy as dlb; whichever stage runs last leaves that copy.  The gradients are those of
 *     loss_scale * mean_b nll_b  +  risk_scale / B * sum_b sum_n coef[b,n] * nll(hyp[b,n])  +  kd_scale / B * tau * sum_b w_b * sum_t KL_t,
 * tau = 1 / inv_temp: the usual lambda * tau^2 * KL per clip, averaged over the batch, is kd_scale = lambda * tau.
 *   ishara_kd_stage     teacher [B,T,C] fp32 on the device (logits or log-probabilities; it may be the `logits` argument itself), inv_temp,
 *                       mode, kl_frame [B,T] and kl_clip [B] (both may be NULL) as ishara_kd_grad; kd_scale by value.
 *   ishara_nbest_stage  the arguments of ishara_loss_backward_nbest from hyp_idx to workspace, under their names.
 * Either pointer may be NULL: with both NULL the call is ishara_loss_backward_ex, with `kd` NULL it is ishara_loss_backward_nbest, launch for
 * launch.  The refusals of both stages (ishara_ctc_nbest_grad's and ishara_kd_grad's, T and C being the model's) come before anything is
 * launched.  loss and nll keep their meaning: the CTC loss of the reference label. */
typedef struct ishara_kd_stage {
    const float* teacher;
    float inv_temp;
    int32_t mode;
    float kd_scale;
    float* kl_frame;                /* may be NULL */
    float* kl_clip;                 /* may be NULL; needs kl_frame */
} ishara_kd_stage;
typedef struct ishara_nbest_stage {
    const int32_t* hyp_idx;
    const int32_t* hyp_len;
    int32_t N, Th, max_len;
    const float* coef;
    float risk_scale;
    void* workspace;
} ishara_nbest_stage;
int ishara_loss_backward_kd(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale,
                            const int32_t* frame_len /* may be NULL */, const ishara_kd_stage* kd /* may be NULL */,
                            const ishara_nbest_stage* nbest /* may be NULL */, ishara_stream s);
/* frame lengths of a zero-padded batch x [B,T,F] f32 (device): out_len[b] (device int32 [B]) = 1 + the index of the last frame of clip b that
 * has any non-zero feature, 0 if there is none.  The prefix reading of Masking(0.0): an all-zero frame INSIDE a clip stays valid, where Keras
 * masks that frame too.  One workgroup per clip; B, T, F > 0. */
int ishara_frame_lengths(const float* x, int32_t B, int32_t T, int32_t F, int32_t* out_len, ishara_stream s);
/* ConformerEncoder.forward (conformer/conformer.py:84-87) for an ISHARA_FAMILY_TORCH_CONFORMER handle: x, y [B,T,dim] f32.
 * training=1: Dropout active (seed), BatchNorm1d uses batch statistics and updates running_mean / running_var, the
 * activations the backward pass needs stay in the workspace. */
int ishara_encoder_forward(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, ishara_stream s);
/* frames per clip of y: `frames` for the ConformerEncoder; ((T-3)/2+1-3)/2+1, then (.-3)/2+1 after the reduction layer and twice
 * that after the recovery layer for the SqueezeformerEncoder (x is [B, frames, features] there) */
int32_t ishara_encoder_output_frames(const ishara_model* m);
/* loss.backward() through the encoder (conformer.py:99-103): dy [B,T,dim] f32 = dLoss/dy of the last ishara_encoder_forward(training=1);
 * parameter gradients fill grads[0,trainable) (overwritten); dx [B,T,dim] f32 may be NULL. */
int ishara_encoder_backward(ishara_model* m, const float* dy, int32_t B, float* dx, ishara_stream s);
/* The same pair with an attention mask (conformer.py:84-87 hands attn_mask to nn.MultiheadAttention, :30-33, and to nothing else: only the
 * attention is masked, the convolution module and BatchNorm1d see the padded frames as before).  Two forms, usable together, either may be NULL:
 *   attn_bias  device f32 [T,T], row = query, column = key, added to the scaled score: softmax(scale*q.k^T + attn_bias); entries finite or -inf;
 *              shared by every clip and head (nn.MultiheadAttention's 2-D attn_mask; a bool mask's True is -inf here)
 *   key_len    device int32 [B]: the keys j >= key_len[b] of clip b are masked for every query and head (the 3-D attn_mask a torch user builds
 *              for padding); clamped to [0,T] on the device, never read by the host (no synchronise)
 * Dropout acts on the masked probabilities.  A query row whose keys are all masked has o = 0 and dq = 0 and its dO reaches no dk / dv (the
 * reference's own call gives NaN there).  Both NULL: the plain calls above, bit for bit.  ISHARA_FAMILY_TORCH_CONFORMER only: every other family,
 * ISHARA_F16 and a misaligned array are refused before any GPU work.  The caller owns both arrays and passes them again to the backward call
 * (the library keeps no pointer, only whether the last training forward was masked: a backward call that disagrees is refused).  The workspace
 * is the same as without a mask. */
int ishara_encoder_forward_ex(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, const float* attn_bias,
                              const int32_t* key_len, ishara_stream s);
int ishara_encoder_backward_ex(ishara_model* m, const float* dy, int32_t B, float* dx, const float* attn_bias, const int32_t* key_len, ishara_stream s);

/* The padding mask of the ISHARA_FAMILY_TORCH_SQUEEZEFORMER encoder (RelativeMultiHeadAttention.forward(..., mask), attention.py:75-92, in its
 * (batch, 1, time2) form).  input_len: device int32 [B], INPUT frames per clip (not keys: the layers run at three resolutions).  The library derives
 * the keys of each resolution on the device with the reference's own arithmetic, clamped: L to [0, frames]; n2 = clamp((L >> 2) - 1, 0, T2) after the
 * conv2d subsampling; n3 = clamp((n2 >> 1) - 1, 0, T3) in the reduced layers; nrec = clamp(2 * n3, 0, Trec) after recovery.  In every attention layer
 * the keys at or past the clip's length at that layer's resolution are masked, for every query and head; nothing else changes (query rows past the
 * length are computed, the convolution module, BatchNorm statistics, subsampling and time reduction see the padded frames as before).  Dropout acts on
 * the masked probabilities.  A clip whose length is 0 at a resolution gets an all-zero attention output there and takes no part in that layer's
 * attention backward (the reference's -1e9 fill would average the padding uniformly; zeros are this library's convention).
 * input_len NULL: ishara_encoder_forward / _backward, bit for bit, on the same kernels.  The library keeps no pointer: pass the array again to the
 * backward call; a backward call that disagrees with the last training forward about lengths is refused.  The other families are refused (they take
 * frame_len of ishara_forward_ex, key_len of ishara_encoder_forward_ex); a misaligned input_len is refused before any GPU work. */
int ishara_encoder_forward_lengths(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed,
                                   const int32_t* input_len, ishara_stream s);
int ishara_encoder_backward_lengths(ishara_model* m, const float* dy, int32_t B, float* dx, const int32_t* input_len, ishara_stream s);
/* Gradient buckets for data parallelism (replaces what tf.distribute / nn.DataParallel do inside the reference's
 * train step: nb4 c1:63-75, integration.py:1058-1060).  The backward pass completes the flat gradient from its end
 * (head) towards its start (stem); ishara_grad_bucket(i) gives range i in completion order and
 * ishara_grad_bucket_wait(i, side) makes the caller's side stream wait for it, so that the all-reduce of a finished
 * range overlaps the rest of the backward pass.  Call ishara_grad_buckets_enable once before the backward passes
 * whose ranges are waited for. */
int32_t ishara_grad_buckets(const ishara_model* m);
int ishara_grad_bucket(const ishara_model* m, int32_t i, int64_t* offset, int64_t* count);
int ishara_grad_buckets_enable(ishara_model* m);
int ishara_grad_bucket_wait(ishara_model* m, int32_t i, ishara_stream side);
/* Lookahead(RectifiedAdam(sma_threshold=4), sync_period=5) apply_gradients — c7:68-69. */
int ishara_optimizer_step(ishara_model* m, float lr, float weight_decay, ishara_stream s);
int32_t ishara_optimizer_iterations(const ishara_model* m);
int ishara_optimizer_set_iterations(ishara_model* m, int32_t it);

/* Global-norm gradient clipping, the non-finite guard and microbatch accumulation: three device-side pieces a training loop composes
 * without a host synchronise (Keras `global_clipnorm=`; torch clip_grad_norm_ + GradScaler's skipped step, integration.py:433,438,750).
 *
 * ishara_gradient_stats writes norm, coef and nonfinite of the 16-byte device record `out` (it never writes `skipped`; zero the record once):
 *   norm      = grad_scale * sqrt(sum_i (double)g[i]^2): every element squared and summed in fp64, in a fixed order (bit-identical from
 *               run to run; finite for elements up to the fp32 maximum)
 *   coef      = grad_scale * min(1, clip_norm / (norm + 1e-6)) when clip_norm > 0 (the clip_grad_norm_ formula), else grad_scale
 *   nonfinite = number of NaN / +-Inf elements, saturating at INT32_MAX
 * ishara_gradient_accumulate: acc[i] = first ? g[i] : acc[i] + g[i], one fp32 add per element.
 * g, acc: [n] f32 at 16-byte aligned addresses, 1 <= n <= 2^31 - 1; ws: ishara_grad_stats_workspace_bytes(n) bytes, 8-byte aligned, needs no
 * initialisation; grad_scale finite and >= 0; clip_norm not NaN (<= 0: no clipping).  `prof` may be NULL: a handle only lends its
 * profiler (keys grad_stats, 4 n bytes; grad_accumulate, 12 n bytes).  Anything else is refused with a message before any HIP call.
 *
 * ishara_optimizer_step_ex is ishara_optimizer_step with a gradient source (`grad`, 16-byte aligned, NULL: the bound grads), a record
 * (`st`, NULL: none) and the skip switch (needs `st`).  With st the update uses grad[i] * st->coef.  With skip_nonfinite != 0 and
 * st->nonfinite > 0 the step writes nothing to params or the three slots and adds 1 to st->skipped.  A skipped step still consumes
 * its iteration number: the counter and the bias corrections live on the host, which cannot see the record without a synchronise; the
 * weight shadows are refreshed as after any step.  ishara_optimizer_step_ex(m, lr, wd, NULL, NULL, 0, s) is ishara_optimizer_step. */
typedef struct ishara_grad_stats { float norm; float coef; int32_t nonfinite; int32_t skipped; } ishara_grad_stats;
int64_t ishara_grad_stats_workspace_bytes(int64_t n);
int ishara_gradient_stats(ishara_model* prof, const float* g, int64_t n, float grad_scale, float clip_norm, ishara_grad_stats* out, void* ws,
                          ishara_stream s);
int ishara_gradient_accumulate(ishara_model* prof, float* acc, const float* g, int64_t n, int32_t first, ishara_stream s);
int ishara_optimizer_step_ex(ishara_model* m, float lr, float weight_decay, const float* grad, ishara_grad_stats* st, int32_t skip_nonfinite,
                             ishara_stream s);

/* Exponential moving average of the weights (Keras `use_ema`, `ema_momentum`, `ema_overwrite_frequency`): one update of the caller's
 * average `avg` [n] f32 from `theta` [n] f32 behind every applied optimizer step, over the trainable prefix of the parameter buffer
 * (Keras averages trainable variables; the BatchNorm moving statistics stay live).  The caller initialises avg to theta when it
 * switches averaging on (Keras: initial_value=var) and zeroes the 16-byte device record `rec` once.
 *
 *   n     = rec->updates, the updates applied so far
 *   d     = (double)momentum; with warmup != 0: d = min(d, (1.0 + n) / (10.0 + n))  (tf.train.ExponentialMovingAverage's num_updates)
 *   alpha = (float)(1.0 - d), evaluated in fp64
 *   avg[i] = avg[i] + alpha * (theta[i] - avg[i]): three fp32 operations, each rounded to nearest, never contracted into an FMA
 *   overwrite_every = N > 0 and (n + 1) % N == 0: the same launch also writes theta[i] = avg[i] (the optimizer slots are left alone)
 *   then rec->updates = n + 1, rec->alpha = alpha, rec->overwrote = 1 if theta was overwritten, else 0
 * With skip_nonfinite != 0 and st->nonfinite > 0 (the step ishara_optimizer_step_ex skipped) nothing is written to avg or theta,
 * updates and alpha keep their values and overwrote = 0.  The record and `st` are read on the device: no host synchronise, and a
 * captured graph replays correctly.  The record is advanced by a one-thread launch behind the update, never by the update kernel.
 * After a launch that may have overwritten theta the caller runs ishara_sync_weights.
 *
 * ishara_weight_swap exchanges a [n] and b [n] bit for bit (as 32-bit words: NaN payloads included); ishara_sync_weights after it too.
 *
 * avg, theta, a, b: 16-byte aligned, the two ranges of a call disjoint; 1 <= n <= 2^31 - 1; rec 8-byte aligned; 0 <= momentum < 1;
 * overwrite_every >= 0; skip_nonfinite != 0 needs st.  `prof` may be NULL: a handle only lends its profiler (keys weight_average,
 * 12 n bytes, 16 n with overwrite_every > 0; weight_swap, 16 n bytes).  Anything else is refused with a message before any HIP call. */
typedef struct ishara_ema_state { int64_t updates; float alpha; int32_t overwrote; } ishara_ema_state;
int ishara_weight_average(ishara_model* prof, float* avg, float* theta, int64_t n, float momentum, int32_t warmup, int32_t overwrite_every,
                          ishara_ema_state* rec, const ishara_grad_stats* st, int32_t skip_nonfinite, ishara_stream s);
int ishara_weight_swap(ishara_model* prof, float* a, float* b, int64_t n, ishara_stream s);

/* Adversarial weight perturbation (AWP; Wu, Xia, Wang, NeurIPS 2020, in the per-tensor form of the Keras fingerspelling recipes): every
 * weight tensor moves a step up its own gradient, the caller runs forward and backward again at the moved weights, puts the weights back
 * and steps the optimizer on the second gradient.  ishara_awp_perturb moves the weights and keeps a copy; ishara_awp_restore copies it back.
 *
 * The first n elements of w and g (the trainable prefix of the flat buffers) are cut into S segments, one per parameter entry, by
 * seg_off: a DEVICE array int64 [S + 1] with seg_off[0] = 0, strictly increasing, seg_off[S] = n.  The offsets need no alignment.  The
 * host cannot validate the values without a device read, so they are the caller's contract (the kernels clamp every index they derive
 * from the table to [0, n), nothing more).  For every segment s, over its elements i:
 *   ss_g = sum (double)g[i]^2 and, with relative != 0, ss_w = sum (double)w[i]^2: fp64 sums in a fixed order, no float atomics, so the
 *     results are bit-identical from run to run
 *   ss_g not finite (a NaN or Inf in the segment's gradient, or an overflowed sum), or relative != 0 and ss_w not finite:
 *     scale[s] = 0, w keeps every bit over the segment, rec->zeroed counts the segment
 *   else rec->perturbed counts it and, evaluated in fp64 and rounded once,
 *     scale[s] = (float)((double)delta / (sqrt(ss_g) + (double)eps)), with relative != 0
 *     scale[s] = (float)((double)delta * sqrt(ss_w) / (sqrt(ss_g) + (double)eps));
 *     w[i] = w[i] + scale[s] * g[i]: the product rounded to fp32, then the sum rounded to fp32, never contracted into an FMA.
 *     An all-zero gradient gives a finite scale (eps > 0) and a step of 0
 *   backup[i] = w[i] as it was, a copy of the 32-bit word, for every segment, the zeroed ones too; g is only read
 *   rec->grad_norm = (float)sqrt(sum_s ss_g), rec->delta_norm = (float)sqrt(sum_s (double)scale[s]^2 * ss_g), both sums over the
 *     segments that were not zeroed, in segment order
 * scale (device, [S]) and rec are written by the device only: no host synchronise, no allocation, no memset, and a captured graph
 * replays the call.  ws: ishara_awp_workspace_bytes of (n, S) bytes of device memory, every word of which the call writes before it reads it.
 * ishara_awp_restore copies backup [n] over w [n] as 32-bit words (NaN payloads included).  The caller runs ishara_sync_weights behind
 * each of the two when the weights are a model's.
 *
 * Refused with a message before any HIP call: a null w, backup, g, seg_off, scale, rec or ws; w or backup not 16-byte aligned, g or scale
 * not 4-byte, seg_off or ws not 8-byte, rec not 4-byte aligned; w and backup overlapping; n outside 1 .. 2^31 - 1; S outside 1 .. n; delta
 * or eps not a finite value > 0.  `prof` may be NULL: a handle only lends its profiler (keys awp_norms, 4 n bytes, 8 n with relative;
 * awp_perturb, 16 n bytes; awp_restore, 8 n bytes). */
typedef struct ishara_awp_stats { float grad_norm; float delta_norm; int32_t perturbed; int32_t zeroed; } ishara_awp_stats;
int64_t ishara_awp_workspace_bytes(int64_t n, int32_t S);
int ishara_awp_perturb(ishara_model* prof, float* w, float* backup, const float* g, const int64_t* seg_off, int32_t S, int64_t n,
                       float delta, float eps, int32_t relative, float* scale, ishara_awp_stats* rec, void* ws, ishara_stream s);
int ishara_awp_restore(ishara_model* prof, float* w, const float* backup, int64_t n, ishara_stream s);

/* Optimizer parameter groups: frozen tensors, per-tensor learning-rate and weight-decay scales (Keras `layer.trainable = False`, torch
 * `requires_grad_(False)` and optimizer param_groups; the weight-decay exclusion of biases and norm scales of the AdamW recipes).
 *
 * The trainable prefix [0, n) is cut into S segments by seg_off, the DEVICE table of ishara_awp_perturb (int64 [S + 1], seg_off[0] = 0,
 * strictly increasing, seg_off[S] = n, no alignment of the offsets; the values are the caller's contract, indices derived from them are
 * clamped to [0, n)).  `groups` is a DEVICE array of S rows of 16 bytes, row s for segment s.  ishara_optimizer_step_groups is
 * ishara_optimizer_step_ex (iteration counter, weight shadows also behind a skipped step, grad NULL: the bound gradient, st, the skip
 * switch) whose update, over the elements of segment s with row r, is
 *   r.frozen != 0: nothing is written to params or the three slots over the segment (every 32-bit word stays, NaN payloads included) and
 *     the segment's gradient is not read
 *   else the update of ishara_optimizer_step_ex, the same device function, with lr * r.lr_scale and weight_decay * r.wd_scale, each
 *     one fp32 multiply rounded to nearest; a product of 0 is a step without decay (no 0 * theta term: an infinite weight stays
 *     infinite); lr_scale = 0 is not frozen: the slots move and the weights change by -0 * update
 *   with st: grad[i] * st->coef; with skip_nonfinite != 0 and st->nonfinite > 0 nothing at all is written and st->skipped rises by 1
 * So rows that are all (1, 1, 0) give every bit of ishara_optimizer_step_ex, and a segment with row (a, b, 0) gets the bits a plain step
 * with lr' = fp32(lr * a), wd' = fp32(wd * b) gives it.
 * ishara_gradient_mask_groups writes g[i] = +0.0f (the word 0) over the frozen segments and touches no other word: a frozen tensor then
 * counts neither in ishara_gradient_stats (norm, the non-finite guard) nor in the norms of ishara_awp_perturb.
 *
 * The device does all reading of the rows: no host synchronise, no allocation, no memset, no atomics; a captured graph replays the
 * calls, and rows changed on the device between replays take effect without a new capture.  ws: ishara_param_groups_workspace_bytes of
 * (n, S) bytes of device memory; every call writes each word of it before reading it.  Work is cut into chunks of 4096 elements that never
 * cross a segment (the scheme of ishara_awp_perturb); 16-byte accesses over the aligned body of a chunk.
 *
 * ishara_optimizer_op_step is the update of ishara_optimizer_step[_ex] (the same launches) on caller's buffers, for step number
 * `iteration` (1-based); ishara_optimizer_op_step_groups the grouped update likewise.  No handle, no weight shadows.
 *
 * Refused with a message before any HIP call: a null handle, theta, grad (of the op entry points and the mask), m, v, slow, seg_off,
 * groups or ws; theta, grad / g, m, v or slow not 16-byte aligned, seg_off or ws not 8-byte, groups or st not 4-byte aligned; n outside
 * 1 .. 2^31 - 1; S outside 1 .. n; iteration < 1; skip_nonfinite != 0 with a null st.  `prof` may be NULL: a handle only lends its
 * profiler.  Profiler keys: radam_lookahead_groups (28 n bytes), grad_mask_groups (4 n bytes). */
typedef struct ishara_param_group { float lr_scale; float wd_scale; int32_t frozen; int32_t reserved; } ishara_param_group;   /* 16 bytes */
int64_t ishara_param_groups_workspace_bytes(int64_t n, int32_t S);
int ishara_optimizer_step_groups(ishara_model* m, float lr, float weight_decay, const float* grad, ishara_grad_stats* st, int32_t skip_nonfinite,
                                 const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, ishara_stream s);
int ishara_gradient_mask_groups(ishara_model* prof, float* g, int64_t n, const int64_t* seg_off, const ishara_param_group* groups, int32_t S,
                                void* ws, ishara_stream s);
/* model-free operator entry points, for the parity tests */
int ishara_optimizer_op_step(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, int32_t iteration,
                             float lr, float weight_decay, ishara_grad_stats* st, int32_t skip_nonfinite, ishara_stream s);
int ishara_optimizer_op_step_groups(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, int32_t iteration,
                                    float lr, float weight_decay, ishara_grad_stats* st, int32_t skip_nonfinite,
                                    const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, ishara_stream s);

/* HIP-event profiler (no reference counterpart: the reference profiles with %%timeit / Keras
 * progress bars).  When enabled, every kernel launch of forward / loss_backward /
 * optimizer_step is bracketed by events on the launch stream; the report is text, one line per
 * kernel family: "name launches total_ms algorithmic_bytes flops".  Returns bytes written. */
int ishara_profile_enable(ishara_model* m, int32_t on);
int ishara_profile_report(ishara_model* m, char* buf, int32_t cap);

/* decode_phrase (c8:4-12) for a batch: logits [B,T,C] f32 -> out_idx [B,T] int32 (-1 padded), out_len [B].  B >= 0 (0: nothing is launched),
 * 1 <= T <= 4096, C >= 1, 0 <= blank < C, no null buffer; anything else is refused with a message before any HIP call. */
int ishara_greedy_decode(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank,
                         int32_t* out_idx, int32_t* out_len, ishara_stream s);
/* Per-clip frame counts: the four *_ex entry points below take their sibling's arguments plus frame_len [B] int32 in device memory (4-byte
 * aligned; NULL: every sample has T frames and the outputs are bit-equal to the sibling's).  The buffer's T stays the stride of every
 * array and sizes the workspace; sample b uses its first Tb = frame_len[b] frames only and computes, bit for bit, what its sibling computes
 * when launched on that sample alone at T = Tb.  Rows t >= Tb of the logits are not read (they may hold NaN).  Past the sample's end
 * out_idx is -1, frame_pos is -1 and dlogits is +0.  A frame_len[b] outside [1, T] is never used as an index or a bound: the sample has no
 * frames (greedy: out_len 0; beam: every slot len -1, score -inf; align: the no-alignment constants; loss: nll 1e30, dlogits +0) and the
 * other samples' outputs are bit-identical to a launch without it.  Everything the sibling refuses is refused, in the same way; nothing is
 * read on the host, so the calls are graph-capturable.
 * ishara_greedy_decode_ex: the run that is never emitted is the one that ends at frame Tb - 1. */
int ishara_greedy_decode_ex(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank,
                            int32_t* out_idx, int32_t* out_len, const int32_t* frame_len, ishara_stream s);
/* pre_process1(*pre_process00(x)) of the TFLite wrapper (c3:61-115, c13:9-15): raw [max_frames,276] landmarks with NaNs
 * (SEL_COLS order, c1:22-26), clip length read from device memory (*n_frames), mean/std [276] in output order
 * -> out [T,276].  One kernel, graph-capturable. */
int ishara_preprocess(const float* raw, const int32_t* n_frames, int32_t max_frames, const float* mean, const float* stdv,
                      float* out, int32_t T, ishara_stream s);
/* The same for B ragged clips at once (the test-set loop of c18:5-7 runs one clip per call): raw [n_total,276] holds the clips back
 * to back, clip b is rows [offsets[b], offsets[b+1]) of a device-resident int64 table [B+1] (an empty range is a valid, empty clip; rows
 * past max_frames are ignored, as ishara_preprocess ignores them) -> out [B,T,276], each clip bit-identical to ishara_preprocess.  raw
 * and out 16-byte aligned; 1 <= max_frames <= 8192, 1 <= T <= 4096.  One kernel, graph-capturable. */
int ishara_preprocess_batch(const float* raw, int64_t n_total, const int64_t* offsets, int32_t B, int32_t max_frames,
                            const float* mean, const float* stdv, float* out, int32_t T, ishara_stream s);
/* Levenshtein.distance of c18:1-9 on the device: out_idx [B,T] / out_len [B] of ishara_greedy_decode, a decode shorter than 3
 * replaced by the wrapper's constant phrase (c13:22-23); targets [B,L] int32 padded with 59 (PAD_TOKEN_IDX, c1:5), 1 <= L <= 64
 * (MAX_PHRASE_LENGTH, c1:28) -> dist [B], tlen [B] (symbols before the first pad).  Integer-only, deterministic. */
int ishara_edit_distance(const int32_t* out_idx, const int32_t* out_len, int32_t B, int32_t T, const int32_t* targets, int32_t L,
                         int32_t* dist, int32_t* tlen, ishara_stream s);
/* The alignment behind that distance: for every (prediction, target) pair the canonical minimal edit script.  Prediction a[0..na), target
 * b[0..nb) (nb = symbols before the first 59), D the unit-cost Levenshtein table; the script is the walk from (na, nb) to (0, 0) that takes at
 * each cell the FIRST move that applies: diagonal (i, j > 0 and D[i][j] == D[i-1][j-1] + (a[i-1] != b[j-1]): a match or a substitution,
 * aligned[j-1] = a[i-1]), then up (i > 0 and D[i][j] == D[i-1][j] + 1: an insertion, the prediction holds a symbol the target lacks,
 * inserted[j] += 1: slot j counts the extra symbols in front of target position j, slot nb the trailing ones), else left (a deletion:
 * aligned[j-1] = -1).  Inputs and limits as for ishara_edit_distance (out_idx [B,T], out_len [B] clamped to 0..T, targets [B,L] pad-59,
 * 1 <= L <= 64, 1 <= T <= 4096, B = 0 a no-op); fallback != 0 replaces a prediction with out_len < 3 by the wrapper's constant phrase first,
 * as ishara_edit_distance does, fallback == 0 aligns the raw prediction (beam outputs, the torch families).
 * -> ops [B,4] = (matches, substitutions, deletions, insertions); aligned [B,L], -2 at j >= nb; inserted [B,L+1], 0 at j > nb;
 * confusion [60,60] int32 (row = target symbol, column = predicted symbol, index 59 = "nothing"), ACCUMULATED: += 1 at [t][p] per diagonal
 * move, at [59][p] per insertion, at [t][59] per deletion; the caller zeroes it once and sums a whole test set on the device; NULL: not
 * wanted.  A symbol outside 0..58 is counted at index 59 (indexing only: aligned keeps the symbol); nothing is written outside the matrix,
 * and [59][59] stays 0 for predictions inside 0..58.  S + D + I is the edit distance, M + S + D = nb, M + S + I = na (after the fallback).
 * workspace: ishara_edit_alignment_workspace_bytes(B, T) bytes (B * max(T, 11) * 16; -1 for B < 0 or T outside 1..4096), 16-byte aligned,
 * no initialisation needed.  A null or misaligned workspace, a null buffer (other than confusion) and out-of-range L / T / B are refused
 * with a message before any launch.  One kernel, graph-capturable, no allocation, no memset; the matrix's integer atomics are the only
 * atomics: every output is an exact function of the inputs. */
int64_t ishara_edit_alignment_workspace_bytes(int32_t B, int32_t T);
int ishara_edit_alignment(const int32_t* out_idx, const int32_t* out_len, int32_t B, int32_t T, const int32_t* targets, int32_t L,
                          int32_t fallback, int32_t* ops, int32_t* aligned, int32_t* inserted, int32_t* confusion /* may be NULL */,
                          void* workspace, ishara_stream s);

/* ---- streaming sessions (no reference counterpart: this text is the specification) --------------------------------------------------
 * S sessions, one signer each, recognised while the sign is being made.  The state is caller-owned device memory, described by a struct of
 * device pointers that is passed by address (as ishara_gemm_tn_call is); ALL-ZERO MEMORY IS S EMPTY SESSIONS, no init kernel exists:
 *   raw       f32   [S, window, 276]  stored raw frames (16-byte aligned)      hand      u8  [S, window]  1 = that row has a hand
 *   counters  int32 [S, 8]            n (stored frames), active (stored frames with a hand), idle (trailing run of stored frames without
 *                                     one), dropped, done, n_hist, committed_len, 0
 *   hist      int32 [S, agree, T]     the last `agree` hypotheses, oldest first, slots 0..n_hist-1 used, each padded with -1
 *   hist_len  int32 [S, agree]        their lengths                             committed int32 [S, T]  the first committed_len are valid
 * 1 <= window <= 8192, 1 <= T <= 4096, 2 <= agree <= 4, 0 <= S <= 65535 (S == 0: every call is a no-op).
 * "Hand present" is the frame filter's predicate of ishara_preprocess: the 3 x 42 hand columns summed in that kernel's order with NaN read
 * as 0, present iff the sum != 0 (hand values that cancel to exactly 0 are "absent", as in the filter).
 * One tick per session, given a chunk of k >= 0 new frames and a flag word:
 *  1. start   RESET set, or done set by the tick before: counters, history and committed_len become 0 (a phrase that ended restarts by
 *             itself; a final is reported once).
 *  2. append  frame by frame: while active == 0 a frame without a hand is not stored, dropped += 1; a frame arriving at n == window is
 *             not stored, dropped += 1; any other is stored at row n with its hand byte, n += 1, and with a hand active += 1, idle = 0,
 *             without one idle += 1.  fresh = a frame was stored this tick; full = n == window afterwards.
 *  3. recognise  the stored frames are one clip: ishara_preprocess_sessions, ishara_forward(training = 0), ishara_greedy_decode or the
 *             beam's top-1 -> hyp = idx[s, :len[s]] (an empty session is the empty clip).
 *  4. agree   endpoint = active >= min_active_frames && idle >= idle_frames; final = FINISH || full || endpoint.  If fresh, hyp is pushed
 *             into the history (a tick that stored nothing pushes nothing: a waiting session must not agree with itself).  If the history
 *             then holds `agree` entries and their longest common prefix l exceeds committed_len: committed[committed_len:l] =
 *             hyp[committed_len:l], committed_len = l; a committed symbol is never retracted or rewritten.  final: text = hyp, stable_len =
 *             text_len = len, done = 1 (the offline result).  Otherwise text = committed[:committed_len] ++ hyp[committed_len:len] (the
 *             committed part alone when len <= committed_len), stable_len = committed_len, text_len = max(committed_len, len) <= T.
 * record [S, 8] int32 = flag bits (FRESH | FINAL | FULL | ENDPOINT | STARTED, STARTED = active > 0), n, active, idle, dropped, stable_len,
 * text_len, 0; text [S, T] int32 padded with -1.  All three calls are one kernel each, graph-capturable, no allocation, no memset, no host
 * read, no atomics: bit-identical from run to run.  Each refuses, with a message and before any HIP call: a null state, S / window / T /
 * agree out of range, null or misaligned buffers, idle_frames < 1, min_active_frames < 0. */
#define ISHARA_STREAM_COUNTERS 8
#define ISHARA_STREAM_RECORD 8
#define ISHARA_STREAM_RESET 1             /* flag word of a tick */
#define ISHARA_STREAM_FINISH 2
#define ISHARA_STREAM_FRESH 1             /* record[0] */
#define ISHARA_STREAM_FINAL 2
#define ISHARA_STREAM_FULL 4
#define ISHARA_STREAM_ENDPOINT 8
#define ISHARA_STREAM_STARTED 16
typedef struct ishara_stream_state {
    float* raw; uint8_t* hand; int32_t* counters; int32_t* hist; int32_t* hist_len; int32_t* committed;
    int32_t S, window, T, agree;
} ishara_stream_state;
/* Steps 1-2: frames [n_total, 276] (16-byte aligned) holds the sessions' chunks back to back, chunk s = rows [offsets[s], offsets[s+1]) of a
 * device int64 table [S+1] (clamped to the buffer, the idiom of ishara_preprocess_batch; a chunk may be empty or longer than window), flags
 * [S] device int32 -> rows, hand bytes and counters of the state, fresh [S] int32.  Rows at and past n are not touched. */
int ishara_stream_append(const ishara_stream_state* st, const float* frames, int64_t n_total, const int64_t* offsets,
                         const int32_t* flags, int32_t* fresh, ishara_stream s);
/* ishara_preprocess_batch for fixed-stride buffers: session s is rows [0, n[s * n_stride]) of raw + s * window * 276 (n clamped to 0..window;
 * n_stride >= 1 lets n point into the counters: n = counters, n_stride = 8) -> out [S, T, 276], each session bit-identical to
 * ishara_preprocess on the same frames.  hand [S, window] (may be NULL): one byte per frame, != 0 = hand present, as ishara_stream_append
 * writes it; the kept-frame list is then built from the bytes.  NULL: the predicate is evaluated from raw.  raw and out 16-byte aligned. */
int ishara_preprocess_sessions(const float* raw, const int32_t* n, int32_t n_stride, const uint8_t* hand, int32_t S, int32_t window,
                               const float* mean, const float* stdv, float* out, int32_t T, ishara_stream s);
/* Step 4 from the decoder's idx [S, T] / len [S] (len clamped to 0..T), the tick's flags [S] and the fresh [S] of ishara_stream_append:
 * updates history, committed text, done; writes record [S, 8] and text [S, T]. */
int ishara_stream_agree(const ishara_stream_state* st, const int32_t* idx, const int32_t* len, const int32_t* flags, const int32_t* fresh,
                        int32_t idle_frames, int32_t min_active_frames, int32_t* record, int32_t* text, ishara_stream s);

/* CTC prefix beam search (Hannun et al. 2014) with optional character-bigram shallow fusion; the semantics of ishara_amd/ctc_beam.py.
 * logits [B,T,C] fp32 (log_softmax taken on the device), blank index, beam width W, nbest <= W; lm [C,C] natural-log probabilities
 * (row = previous class, row blank = start of phrase; column = next class, column blank = end of phrase) or NULL; ranking key
 * (pb (+) pnb) + alpha * sum(lm) + beta * len.  2 <= C <= 64, 1 <= W <= 32, 1 <= nbest <= W, 1 <= T <= 4096.
 * -> out_idx [B,nbest,T] int32 padded with -1, out_len [B,nbest], out_score [B,nbest]; an n-best slot without a hypothesis has len -1
 * and score -inf.  With nbest = 1 out_idx / out_len have the layout of ishara_greedy_decode (ishara_edit_distance reads them).  Unlike
 * the greedy decoder it uses the last frame too.  workspace: ishara_ctc_beam_workspace_bytes(B, T, C, W), 4-byte aligned, no
 * initialisation needed.  One kernel, graph-capturable, bit-identical from run to run; B = 0 is a no-op. */
int64_t ishara_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t C, int32_t beam_width);
int ishara_ctc_beam_decode(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                           const float* lm, float alpha, float beta, void* workspace,
                           int32_t* out_idx, int32_t* out_len, float* out_score, ishara_stream s);
/* with per-clip frame counts (see ishara_greedy_decode_ex); workspace as for ishara_ctc_beam_decode at the buffer's T */
int ishara_ctc_beam_decode_ex(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                              const float* lm, float alpha, float beta, void* workspace,
                              int32_t* out_idx, int32_t* out_len, float* out_score, const int32_t* frame_len, ishara_stream s);
/* The same search with the LM as a deterministic automaton of S states (a character n-gram with backoff: ishara_amd/ctc_lm.py), both
 * tables on the device: lm_logp [S,C] fp32, row s = the natural-log probability of every next event in state s (column c != blank: next
 * class c; column blank: end of phrase), and lm_next [S,C] int32, the state after class c (column blank unused).  Every beam carries its
 * state from start_state: an extension by c adds alpha * lm_logp[state][c] and moves to lm_next[state][c], the final term is
 * alpha * lm_logp[state][blank].  The bigram table is the case S = C, start_state = blank, lm_next[s][c] = c, lm_logp = lm, and gives
 * ishara_ctc_beam_decode_ex's bits.  Limits, outputs, workspace, total order and frame_len (may be NULL: every clip has T frames) as
 * for ishara_ctc_beam_decode_ex; in addition 1 <= S <= 2^22, 0 <= start_state < S, both tables non-NULL and 16-byte aligned; anything
 * else is refused with a message before any HIP call.  The tables cannot be read on the host: an lm_next value outside [0, S) is read as
 * state 0 and is never used as an index.  One kernel (the rows of the beams' states are fetched once per frame, under the frame's merge
 * detection), graph-capturable, no atomics, bit-identical from run to run; B = 0 is a no-op. */
int ishara_ctc_beam_decode_lm(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                              const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, float alpha, float beta,
                              void* workspace, int32_t* out_idx, int32_t* out_len, float* out_score,
                              const int32_t* frame_len /* may be NULL */, ishara_stream s);

/* CTC forced alignment (Viterbi) of known labels; the semantics of ishara_amd/ctc_align.py.  logits [B,T,C] fp32, labels [B,L] int64 padded
 * with blank (the label of a row ends at its first blank).  The path maximises the sum of the raw logits along it, carried in fp64, ties
 * broken stay > s-1 > s-2: the integer outputs are an exact function of the inputs.
 * -> frame_pos [B,T] int32 (label index emitted at the frame, -1 on a blank frame); start, end [B,L] int32 (symbol i on frames [start, end),
 * -1 past the label); conf [B,L] fp32 (mean softmax value of the symbol over its span, 0 past the label); score [B] fp32 (log-probability
 * of the path).  A sample without an alignment (T < len + repeats, or a label outside [0, C), which is read as blank and never used as an
 * index) gets score -1e30, frame_pos -1, start = end = -1, conf 0; the other samples' outputs are bit-identical to a launch without it.
 * B >= 0 (0: nothing is launched), 1 <= T <= 4096, 1 <= L <= 255, 2 <= C <= 64, 0 <= blank < C, no null buffer; anything else is refused with
 * a message before any HIP call.  ws: the bytes the workspace function returns (128 where the back-pointers fit in LDS and the buffer is
 * not touched, B*T*128 otherwise), 16-byte aligned, no initialisation needed.  One kernel, graph-capturable, bit-identical from run to run. */
int64_t ishara_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t L);
int ishara_ctc_align(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                     void* ws, int32_t* frame_pos, int32_t* start, int32_t* end, float* conf, float* score, ishara_stream s);
/* with per-clip frame counts (see ishara_greedy_decode_ex): feasibility is Tb >= len + repeats; ws as for ishara_ctc_align at the buffer's T */
int ishara_ctc_align_ex(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                        void* ws, int32_t* frame_pos, int32_t* start, int32_t* end, float* conf, float* score,
                        const int32_t* frame_len, ishara_stream s);

/* Model ensembling before the CTC decode: the frame posteriors of M models fused into one normalised log-distribution per frame.
 * logits: a HOST array of M device pointers, each [B,T,C] fp32; the launcher copies them into the kernel's arguments by value (no device
 * pointer table, no allocation, no memset; a captured graph replays the call).  weights: device fp32 [M]; inv_temp: device fp32 [M]
 * (1 / temperature) or NULL for all 1; both are read on the device at every launch, so a caller may rewrite them between replays of a
 * graph without capturing again.  out [B,T,C] fp32.  prof may be NULL; a handle only lends its profiler (key logits_combine,
 * (M + 1) * B*T*C*4 bytes: the weights cannot be read on the host, every model counts as read).
 * Per row (b, t), every step in fp32, for the models with weights[m] > 0 in ascending m:
 *     z = logits_m[row, c] * inv_temp[m]  (one multiply; none with NULL),   lp_m[c] = (z[c] - max_c z) - log(sum_c exp(z[c] - max_c z))
 *   mode 0 (log-linear, product of experts):  s[c] = sum_m weights[m] * lp_m[c]
 *   mode 1 (linear, mixture):                 s[c] = a[c] + log(sum_m exp(log(weights[m]) + lp_m[c] - a[c])),  a[c] = max_m (log(weights[m]) + lp_m[c])
 *   out[row, c] = s[c] - logsumexp_c s[c]:  a normalised log-distribution in both modes, whatever the weights sum to.
 * A model whose weight is not > 0 is not read at all (its buffer may hold NaN); no weight > 0: every row is the uniform -log C.  frame_len:
 * device int32 [B] or NULL (the convention of ishara_greedy_decode_ex): clip b has Tb = frame_len[b] frames, a value outside [1, T] means no
 * frames; rows t >= Tb are not read from any model and are written +0.0.  Inputs are assumed finite; no index is derived from data.
 * One kernel, no atomics, fixed-order class reductions: bit-identical from run to run.  Refused with a message before any HIP call: a null
 * logits, logits[m], weights or out; M outside 1..8; C outside 2..64; T outside 1..4096; B < 0 (B == 0: nothing is launched); mode not 0 or
 * 1; a pointer that is not 4-byte aligned; out overlapping any input range (B*T*C*4 bytes each). */
int ishara_logits_combine(ishara_model* prof, const float* const* logits, int32_t M, int32_t B, int32_t T, int32_t C,
                          const float* weights, const float* inv_temp, int32_t mode, const int32_t* frame_len, float* out, ishara_stream s);

/* Minimum-Bayes-risk selection over an n-best list; the semantics of ishara_amd/mbr.py (mbr_reference).  Per clip, among the live
 * hypotheses, the one whose expected edit distance to the others is smallest, copied into the greedy layout.
 *   hyp_idx [B,N,T] int32 as ishara_ctc_beam_decode writes it (only the first min(len, T) symbols of a live row are read); hyp_len [B,N]:
 *   a slot is live iff hyp_len >= 0, the length is clamped to T; dead slots are neither candidates nor voters.  hyp_score [B,N]
 *   natural-log scores (ignored, and may be NULL, when weights != NULL); weights [B,N] or NULL: explicit votes; inv_temp: ONE float on the
 *   device or NULL for 1.0, read at every launch (a captured graph follows a caller that rewrites it, as it follows rewritten weights).
 * Distance: d[i][j] = the unit-cost Levenshtein distance of the live hypotheses i and j, an integer, symmetric, d[i][i] = 0.
 * Vote of slot j: with weights, w_j = weights[j] where that is finite and > 0, else +0.  Without, x_j = (s_j - s_max) * inv_temp (one fp32
 *   subtraction, one fp32 multiplication), s_max the largest finite score of the live slots, w_j = expf(x_j); a live slot whose score is
 *   not finite (-inf, NaN, +inf) votes +0 and does not enter s_max.  The votes are not normalised.
 * Risk: risk_i = sum_j w_j * c_ij over the live j in ascending slot order from +0; mode 0: c_ij = (float)d_ij; mode 1: c_ij =
 *   (float)d_ij / (float)max(len_j, 1) (the c18 metric, normalised by the voter's length as by a target's).  The division, the
 *   multiplication and every addition are single round-to-nearest fp32 operations without FMA contraction: given w_out, float32 arithmetic
 *   in that order reproduces risk bit for bit.
 * Selection: slots in ascending order, a later slot wins only with a strictly smaller risk (ties go to the lowest slot, the higher score
 *   of a ranked n-best; a NaN never wins).
 * -> out_idx [B,T] (the selected hypothesis, -1 past its end; every element is written), out_len [B], best [B] (the selected slot), and,
 *   each NULL or: risk [B,N] fp32 (NaN in dead slots), w_out [B,N] fp32 (the votes used, +0 in dead slots), dist [B,N,N] int32 (-1 in dead
 *   rows and columns), status [B] int32.
 * Status, for a clip the kernel does not rank: bit 0 a live hypothesis is longer than 64 symbols (MAX_PHRASE_LENGTH, the limit of
 *   ishara_edit_distance's targets); bit 1 a live symbol lies outside [0, C) (among the first 64 of each hypothesis; never used as an
 *   index); bit 2 no live slot.  With bit 0 or 1: best = the lowest live slot, risk of the whole clip NaN, dist of the clip -1, w_out as
 *   above.  With bit 2: best = -1, out_len = 0, out_idx all -1.
 * 1 <= N <= 64, 1 <= T <= 4096, 2 <= C <= 64, mode 0 or 1, B >= 0 (0: nothing is launched), 4-byte alignment of every buffer, out_idx
 * not overlapping hyp_idx, hyp_idx / hyp_len / out_idx / out_len / best non-NULL and hyp_score non-NULL when weights is NULL; anything
 * else is refused with a message before any HIP call.  One kernel (one workgroup per clip, bit-vector edit distances, no workspace), no
 * atomics, graph-capturable, bit-identical from run to run. */
int ishara_mbr_select(const int32_t* hyp_idx, const int32_t* hyp_len, const float* hyp_score, const float* weights, const float* inv_temp,
                      int32_t B, int32_t N, int32_t T, int32_t C, int32_t mode, int32_t* out_idx, int32_t* out_len, int32_t* best,
                      float* risk, float* w_out, int32_t* dist, int32_t* status, ishara_stream s);

/* Second-pass n-best rescoring, part 1: the exact CTC log-likelihood of every hypothesis of every clip under one model; the semantics of
 * ishara_amd/rescore.py (ctc_logp_reference).  out_score of the beam search sums only the alignments that survived the beam; this is the
 * whole sum, logp[b,n] = log sum_alignments prod_t softmax(logits[b,t])[path_t], with tf.nn.ctc_loss semantics as in ishara_ctc_loss.
 *   logits [B,T,C] fp32; hyp_idx [B,N,Th] int32 / hyp_len [B,N] int32 as the beam search and mbr.pool_nbest write them (padded with -1, a slot
 *   is live iff hyp_len >= 0; only the first hyp_len symbols of a live row are read).  Th is the width of the hypothesis rows and need not
 *   equal this model's T (a pooled list is padded to the longest).  frame_len [B] int32 or NULL: the convention of ishara_greedy_decode_ex
 *   (clip b has Tb = frame_len[b] frames, a value outside [1, T] means no frames, rows t >= Tb are never read and may hold NaN).
 * -> logp [B,N] fp32 and status [B,N] int32 (may be NULL).  The empty hypothesis (len 0, the all-blank path) is a hypothesis like any
 *   other and gets its score.  logp is -inf, with exactly one status bit, the first that applies, for:
 *     bit 0 (1)  a dead slot;
 *     bit 3 (8)  hyp_len > Th or hyp_len > 255 (the loss kernel's label limit); the row is not read;
 *     bit 2 (4)  a symbol outside [0, C) or equal to blank among the first hyp_len; it is never used as an index;
 *     bit 1 (2)  no alignment: Tb < len + repeats (repeats = the positions whose symbol equals its predecessor), or the clip has no frames.
 *   Every other slot has status 0 and its logp is bit-identical to a launch without the offending slots.
 * Numerics: the alpha recursion of the loss kernel and nothing else (lse[t] as that kernel computes it, emissions raw - lse, fp64 state with
 *   fp32 exp / log, the final log-sum over the last two lattice states): for every slot with status 0, logp[b,n] == (float)(-nll), bit for
 *   bit, nll being ishara_ctc_loss_ex's on that clip with that hypothesis, padded with blank, as its label row and the same frame_len.
 * One kernel: a workgroup per (clip, group of slots) computes the clip's lse[t] once into LDS, then each wave runs the chains of its slots
 *   with the lattice states in registers.  No lattice in memory, no workspace, no atomics; graph-capturable, bit-identical from run to
 *   run.  Refused with a message before any HIP call: C outside 2..64, T or Th outside 1..4096, N outside 1..64, blank outside [0, C),
 *   B < 0 or B > 65535 (B == 0: nothing is launched), a null logits, hyp_idx, hyp_len or logp, a pointer that is not 4-byte aligned. */
int ishara_ctc_score_nbest(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank,
                           const int32_t* hyp_idx, const int32_t* hyp_len, int32_t N, int32_t Th,
                           const int32_t* frame_len /* may be NULL */, float* logp, int32_t* status /* may be NULL */, ishara_stream s);
/* tests / tools: the slots one wave of that kernel scores one after the other (1..16; a workgroup of four waves takes four times as many
 * slots of one clip and computes its lse once); 0 = the library default.  The results do not depend on it. */
int ishara_debug_set_score_group(int32_t hyps_per_wave);
/* Second-pass n-best rescoring, part 2: combine, dedupe, rerank; the semantics of ishara_amd/rescore.py (rescore_reference).
 *   hyp_idx [B,N,Th] / hyp_len [B,N] as above (the length is clamped to Th).  logp: a HOST array of M device pointers, each [B,N] fp32 (the
 *   logp of ishara_ctc_score_nbest under model m); the launcher copies them into the kernel's arguments by value (no pointer table, no
 *   allocation).  weights: device fp32 [M], read at every launch.  lm_logp [S,C] fp32 / lm_next [S,C] int32 / S / start_state: an LM
 *   automaton with the contract of ishara_ctc_beam_decode_lm (an lm_next value outside [0, S) reads as state 0), or both tables NULL for no
 *   LM (S, start_state, C and blank are then not looked at).  alpha (LM weight) and beta (bonus per symbol) by value, finite.  inv_temp:
 *   ONE float on the device (1 / temperature) or NULL for 1.0, read at every launch.
 * Duplicates: a live slot j dies when a live slot i < j holds the same string (same length, same symbols); the earlier slot stays.
 * Score of a live slot, every step a single round-to-nearest fp32 operation without FMA contraction, in this order: s = +0; for m ascending
 *   with weights[m] > 0: s = s + weights[m] * logp_m[b,n] (a model whose weight is not > 0 is not read: its array may hold NaN).  With an
 *   LM: l = +0, state = start_state; for each symbol c in order l = l + lm_logp[state][c], state = lm_next[state][c]; then
 *   l = l + lm_logp[state][blank]; then s = s + alpha * l (a symbol outside [0, C) is never an index: the slot's score is -inf).  Finally
 *   s = s + beta * (float)len.  A -inf from a participating model gives -inf: the slot stays live and ranks after every finite score.
 * Order: live slots whose score is a number by descending score, ties to the lower input slot; then live slots whose score is NaN, in
 *   input order (a NaN never outranks a number); then the dead slots (dead on input or merged), in input order.
 * Posterior over the live slots with a finite score: x = (s - s_max) * inv_temp (one subtraction, one multiplication), e = expf(x),
 *   p = e / sum e, the sum taken in ascending output order from +0; p = +0 for every other slot, and everywhere when no score is finite.
 * -> out_idx [B,N,Th], out_len [B,N], out_score [B,N]: the beam search's layout in the new order (a dead slot has len -1, score -inf and a
 *   row of -1; every element is written), so ishara_mbr_select, ishara_edit_distance and ishara_edit_alignment take the result as it is;
 *   posterior [B,N] fp32 or NULL (by output slot: usable as ishara_mbr_select's weights); perm [B,N] int32 or NULL: the input slot of each
 *   output slot.
 * One kernel (one workgroup per clip), no workspace, no atomics, graph-capturable, bit-identical from run to run.  Refused with a message
 *   before any HIP call: N outside 1..64, Th outside 1..4096, M outside 1..8, B < 0 (B == 0: nothing is launched), alpha or beta not
 *   finite; with an LM C outside 2..64, blank outside [0, C), S outside 1..2^22, start_state outside [0, S), one table without the other, a
 *   table that is not 16-byte aligned; a null hyp_idx, hyp_len, logp, logp[m], weights, out_idx, out_len or out_score; a pointer that is
 *   not 4-byte aligned; an output that overlaps hyp_idx, hyp_len or a logp[m]. */
int ishara_nbest_rescore(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th,
                         const float* const* logp, int32_t M, const float* weights,
                         const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, int32_t C, int32_t blank,
                         float alpha, float beta, const float* inv_temp,
                         int32_t* out_idx, int32_t* out_len, float* out_score, float* posterior, int32_t* perm, ishara_stream s);
/* The same with the rescoring parameters on the device: params fp32 [M + 2] = (w_0 .. w_{M-1}, alpha, beta), 4-byte aligned, read at every
 * launch, so a captured graph follows a caller that rewrites them.  Every other argument, every output, every refusal (a null params in
 * place of a null weights) and every bit of the arithmetic is ishara_nbest_rescore's: it is the same kernel, and fed the same numbers the
 * two entries write identical bytes.  A non-finite alpha or beta cannot be refused here: the arithmetic proceeds as IEEE 754 says and a
 * NaN score ranks where the order above puts NaN. */
int ishara_nbest_rescore_p(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th,
                           const float* const* logp, int32_t M, const float* params,
                           const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, int32_t C, int32_t blank,
                           const float* inv_temp,
                           int32_t* out_idx, int32_t* out_len, float* out_score, float* posterior, int32_t* perm, ishara_stream s);
/* The weight sweep of the second pass; the semantics of ishara_amd/rescore.py (rescore_sweep_reference).  Row g of best and dist equals
 * perm[:, 0] (-1 where out_len[:, 0] < 0) of ishara_nbest_rescore_p(params = grid[g]) on the same inputs, and ishara_edit_distance of its
 * top row, integer for integer; one launch instead of 2 G.
 *   hyp_idx, hyp_len, B, N, Th, logp (a HOST array of M device pointers), M, lm_logp, lm_next, S, start_state, C, blank: as
 *   ishara_nbest_rescore, same limits and layouts.  targets [B,L] int32 padded with 59, 1 <= L <= 64: ishara_edit_distance's (the target
 *   is the symbols before the first 59).  grid [G, M + 2] fp32 on the device, 1 <= G <= 65536, each row a params vector, read at every launch.
 *   fallback 1: the wrapper's rule as in ishara_edit_distance: a hypothesis shorter than 3 symbols, and a clip without a live slot, is
 *   scored as the constant phrase.  fallback 0: the hypothesis as it is; a clip without a live slot as the empty string (dist = tlen).
 * Duplicates merge into their first slot and a merged slot never wins.  The float32 score of a live slot is ishara_nbest_rescore's, in its
 *   order, without FMA contraction; a model whose weight is not > 0 takes no part (its array may hold NaN).  The top slot holds the largest
 *   number, ties to the lower slot; -inf is a number and ranks last among them; when no live slot holds a number the top is the first live
 *   (NaN) slot; when no slot is live it is -1.  Symbols are compared as integers, as ishara_edit_distance compares them.
 * -> best [G,B] int32: the INPUT slot; dist [G,B] int32; tlen [B] int32; optional (NULL: not wanted) hyp_dist [B,N] int32: what dist would
 *   hold if the slot won (after the fallback rule), -1 in dead or merged slots; lm_score [B,N] fp32: the LM walk's l (-inf for a slot with a
 *   symbol outside [0, C)), +0 without an LM and in slots that are not live.  Every element of every output is written.
 * One kernel: a workgroup per (clip, 256 grid rows) computes the clip's part once (merge, LM walks, lengths, the M scores, every slot's
 *   distance by one 64-bit Myers word with the target as the pattern), then one wave per row.  ws: ishara_rescore_sweep_workspace_bytes
 *   bytes (0 today: ws is not looked at; < 0: B, N or G unsupported).  No atomics, no host read, no allocation, graph-capturable,
 *   bit-identical from run to run; B == 0 launches nothing.  Refused with a message before any HIP call: everything ishara_nbest_rescore
 *   refuses about these arguments, G or L out of range, fallback not 0 or 1, a null targets, grid, best, dist or tlen, a pointer that is not
 *   4-byte aligned, an output that overlaps hyp_idx, hyp_len, a logp[m], targets or grid. */
int64_t ishara_rescore_sweep_workspace_bytes(int32_t B, int32_t N, int32_t G);
int ishara_rescore_sweep(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th,
                         const float* const* logp, int32_t M,
                         const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, int32_t C, int32_t blank,
                         const int32_t* targets, int32_t L, int32_t fallback,
                         const float* grid, int32_t G,
                         int32_t* best, int32_t* dist, int32_t* tlen, int32_t* hyp_dist, float* lm_score,
                         void* ws, ishara_stream s);
/* Minimum-risk (MWER) training, part 1: the gradient of a weighted sum of n-best scores; the semantics of ishara_amd/mwer.py
 * (mwer_reference).  For every clip b, frame t < Tb and class k
 *     G[b,t,k] = grad_scale * acc,  acc = +0, then for n ascending over the participating slots
 *                                   acc = acc + coef[b,n] * (softmax(logits[b,t])[k] - post_n[b,t,k]),
 * post_n being the CTC class posterior of hypothesis n (exp(alpha + bsum - logp) summed over the lattice states that carry class k), so G is
 * the gradient of grad_scale * sum_n coef[b,n] * nll_n with respect to the logits.  Every multiplication and addition is a single
 * round-to-nearest fp32 operation without FMA contraction, in that order.
 *   logits, hyp_idx [B,N,Th], hyp_len [B,N], frame_len (may be NULL): as ishara_ctc_score_nbest.  max_len, 1..255: the longest hypothesis
 *   that takes part; it sizes the workspace, not Th (the beam search's rows have Th = T).  coef [B,N] fp32 on the device (the coef of
 *   ishara_mwer_weights), grad_scale by value.
 * Participation: a slot takes part iff ishara_ctc_score_nbest would give it status 0 and its length is <= max_len; a longer slot gets
 *   status bit 3 (8); every other slot the same bits by the same first-that-applies rule.  A slot whose coef is +0 or -0 is skipped: it
 *   contributes neither its posterior nor its softmax term, and when neither logp nor status is wanted its row is not read.  A clip without
 *   a participating slot contributes acc = +0.
 * -> dlogits [B,T,C] fp32: accumulate 0 writes G, and +0 in the rows t >= Tb; accumulate 1 writes dlogits + G by one fp32 addition and leaves
 *   the rows t >= Tb as they are.  dlb (may be NULL): the bf16 copy of the FINAL dlogits rows, zero padded to 128 classes, [B*T, 64] packed
 *   pairs: the layout the loss kernel writes for the classifier's MFMA operand.  logp [B,N] fp32 (may be NULL): ishara_ctc_score_nbest's
 *   bits (-inf in a slot longer than max_len); status [B,N] int32 (may be NULL).
 * Numerics: the recursions of the loss kernel (lse[t], emissions raw - lse, fp64 state with fp32 exp / log, the alpha wave, the beta wave
 *   that stores bsum, the per-frame LDS scatter-add of the state posteriors).  With N = 1, coef = 1, accumulate = 0, dlogits and dlb equal
 *   those of ishara_op_ctc_loss (ishara_ctc_loss_ex with frame_len) bit for bit, run on that hypothesis, padded with blank, as its label
 *   row with the same grad_scale.
 * Two kernels: grid (N, B) runs the two recursion waves of one slot and writes its fp64 alpha / bsum rows into the workspace (only the
 *   ceil((2 len + 1) / 64) occupied registers, rows of 64 * ceil((2 max_len + 1) / 64) doubles); grid (ceil(T / 16), B) loops n ascending per
 *   frame and writes dlogits / dlb.  No atomics on global memory, no dependence of a slot on its neighbours, bit-identical from run to run,
 *   graph-capturable (no allocation, no memset node, no host read).  workspace: ishara_ctc_nbest_grad_workspace_bytes(B, T, N, max_len)
 *   bytes (-1: an argument out of range), 16-byte aligned, needs no initialisation.
 * Refused with a message before any HIP call: C outside 2..64, T or Th outside 1..4096, N outside 1..64, max_len outside 1..255, blank
 *   outside [0, C), B < 0 or B > 65535 (B == 0: nothing is launched), accumulate not 0 or 1, a null logits, hyp_idx, hyp_len, coef, dlogits
 *   or workspace, a pointer that is not 4-byte aligned (the workspace: 16), dlogits overlapping logits. */
int64_t ishara_ctc_nbest_grad_workspace_bytes(int32_t B, int32_t T, int32_t N, int32_t max_len);
int ishara_ctc_nbest_grad(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank,
                          const int32_t* hyp_idx, const int32_t* hyp_len, int32_t N, int32_t Th, int32_t max_len,
                          const int32_t* frame_len /* may be NULL */, const float* coef, float grad_scale,
                          float* dlogits, int32_t accumulate, void* dlb /* may be NULL */, float* logp /* may be NULL */,
                          int32_t* status /* may be NULL */, void* workspace, ishara_stream s);
/* Minimum-risk training, part 2: the weights.  hyp_idx [B,N,Th] / hyp_len [B,N] as above (the length is clamped to Th); logp [B,N] fp32: the
 * exact scores of ishara_ctc_score_nbest; status [B,N] int32 or NULL; targets [B,L] int32 padded with 59, 1 <= L <= 64
 * (ishara_edit_distance's: the target is the symbols before the first 59); inv_temp: ONE float on the device or NULL for 1.0; mode 0: the
 * plain distance, 1: divided by max(tlen, 1) (the normalisation of the reported metric).
 * A slot is live iff hyp_len >= 0, its status is 0 (when given) and its logp is finite.  Duplicate strings are NOT merged: the prefix beam
 *   search emits distinct prefixes; a pooled list goes through ishara_nbest_rescore first.
 * -> every element of every output is written:
 *   dist [B,N] int32  unit-cost Levenshtein distance to the target (one 64-bit Myers word, the target as the pattern, no fallback phrase),
 *                     -1 in slots that are not live;
 *   post [B,N] fp32   over the live slots x = (logp - max) * inv_temp, e = expf(x), p = e / sum e, the sum ascending from +0; +0 elsewhere;
 *   risk [B] fp32     sum_n p_n * W_n ascending from +0, W_n = (float)dist (mode 1: / (float)max(tlen, 1)); NaN for a clip with no live slot;
 *   coef [B,N] fp32   -inv_temp * (p_n * (W_n - risk)): the derivative of the risk with respect to nll_n; +0 in slots that are not live;
 *   tlen [B] int32.
 *   All arithmetic is fp32, one rounding per operation, no FMA contraction, in the stated order.
 * One kernel, one wave per clip, no workspace, no atomics, graph-capturable, bit-identical from run to run.  Refused with a message before
 *   any HIP call: N outside 1..64, Th outside 1..4096, L outside 1..64, mode not 0 or 1, B < 0 (B == 0: nothing is launched), a null
 *   hyp_idx, hyp_len, logp, targets or output, a pointer that is not 4-byte aligned. */
int ishara_mwer_weights(const int32_t* hyp_idx, const int32_t* hyp_len, const float* logp, const int32_t* status /* may be NULL */,
                        int32_t B, int32_t N, int32_t Th, const int32_t* targets, int32_t L, const float* inv_temp /* may be NULL */,
                        int32_t mode, int32_t* dist, float* post, float* risk, float* coef, int32_t* tlen, ishara_stream s);
/* Knowledge distillation, frame level: the gradient of a temperature-softened KL(teacher || student) with respect to the student's logits;
 * the semantics of ishara_amd/kd.py (kd_reference).  logits and teacher [B,T,C] fp32; the teacher's rows may be raw logits or normalised
 * log-probabilities (ishara_logits_combine's output): the kernel normalises them itself.  frame_len (may be NULL: T each) as
 * ishara_greedy_decode_ex: a value outside [1, T] means the clip has no frames.  Inputs are assumed finite; no index is derived from data.
 * For every clip b and frame t < Tb, lane = class, everything in fp32:
 *     a[c] = logits[c] * inv_temp,  ma = max a,  ea = expf(a - ma),  sa = sum ea,  lps = (a - ma) - logf(sa),  ps = ea / sa;
 *     the teacher's row through the same steps: lpt, pt;
 *     KL_t = sum_c pt[c] * (lpt[c] - lps[c]);
 *     G[b,t,c] = grad_scale * (w_b * (ps[c] - pt[c])),  w_b absent in mode 0 (the clip's sum over frames), 1 / (float)Tb in mode 1 (its mean),
 * so G is the gradient of grad_scale * tau * w_b * sum_t KL_t, tau = 1 / inv_temp: the usual lambda * tau^2 * KL per clip, averaged over the
 * batch, is grad_scale = lambda * tau / B.
 * Arithmetic: max and both sums over the classes are the xor butterfly over the 64 lanes, offsets 32, 16, 8, 4, 2, 1 (x = op(x, x of lane ^
 *   offset)), lanes >= C holding -inf for the max and +0 for a sum: one fixed order, every lane ends with the same bits.  Every
 *   multiplication, subtraction, division and the accumulate addition is a single round-to-nearest fp32 operation without FMA contraction.
 *   Both rows go through the same instructions, so teacher == logits (the same pointer or a copy) gives G = 0 and KL_t = 0 exactly.
 * -> dlogits [B,T,C] fp32: accumulate 0 writes G, and +0 in the rows t >= Tb; accumulate 1 writes dlogits + G by one fp32 addition and leaves
 *   the rows t >= Tb as they are.  dlb (may be NULL): the bf16 copy of the FINAL dlogits rows, zero padded to 128 classes, [B*T, 64] packed
 *   pairs: the layout the loss kernel and ishara_ctc_nbest_grad write.  kl_frame [B,T] (may be NULL): KL_t, +0 past the clip's end.
 *   kl_clip [B] (may be NULL; needs kl_frame): the sum of kl_frame over t ascending from +0, in mode 1 then multiplied by 1 / (float)Tb; +0
 *   for a clip without frames.  Rows past a clip's end are read from neither input.
 * One kernel, grid (ceil(T / 16), B), four waves, a frame per wave at a time and four in flight; with kl_clip a second one, a wave per clip.
 *   No atomics on global memory, no workspace, no allocation, no memset node, no host read: graph-capturable and bit-identical from run to
 *   run.  teacher may alias logits; dlogits must overlap neither.  prof (may be NULL) lends its profiler only.
 * Refused with a message that names the argument, before any HIP call: C outside 2..64, T outside 1..4096, B < 0 or B > 65535 (B == 0:
 *   nothing is launched), mode or accumulate not 0 or 1, inv_temp not finite or <= 0, grad_scale not finite, kl_clip without kl_frame, a
 *   null logits, teacher or dlogits, a pointer that is not 4-byte aligned, an output that overlaps an input or another output. */
int ishara_kd_grad(ishara_model* prof /* may be NULL */, const float* logits, const float* teacher, int32_t B, int32_t T, int32_t C,
                   float inv_temp, int32_t mode, const int32_t* frame_len /* may be NULL */, float grad_scale,
                   float* dlogits, int32_t accumulate, void* dlb /* may be NULL */,
                   float* kl_frame /* may be NULL */, float* kl_clip /* may be NULL; needs kl_frame */, ishara_stream s);

/* Training-side input batch: the per-clip augmentation parameters of ASLDataset._apply_augmentations (data_loader.py:124-166), drawn
 * on the host in the reference's `random` call order (ishara_amd/data.py draw_augmentation).  64 bytes, no padding. */
typedef struct ishara_clip_aug {
    int64_t offset;                 /* first frame of the clip in the store (frames of 124*3 f32) */
    int32_t n;                      /* raw frame count */
    int32_t L1;                     /* length after the time stretch (n when no stretch was drawn) */
    int32_t shift;                  /* frame shift, -10..10; 0 when none was drawn */
    int32_t L2;                     /* length after the shift: L1, or 0 for a drawn shift of 0 (the reference's [:0]) */
    int32_t mirror;                 /* 1: swap the hands, negate x */
    int32_t t0[3];                  /* finger-dropout windows [t0, t1) over the augmented frames */
    int32_t t1[3];
    int32_t fingers[3];             /* 21-bit finger mask per window (bit f zeroes landmarks 76+f and 97+f); 0 = no window */
} ishara_clip_aug;
/* feature layouts of the collated batch */
enum { ISHARA_LAYOUT_FLAT = 0, ISHARA_LAYOUT_HANDS_LIPS_XY = 1 };
/* ASLDataset.__getitem__ (data_loader.py:124-188) + collate for a batch, on device: raw [N_frames,124,3] f32 (16-byte aligned),
 * clips [B] in device memory -> x [B,T,F] f32 (16-byte aligned), F = 372 (FLAT) or 224 (HANDS_LIPS_XY: landmarks 76-117 then
 * 0-69, x and y).  Augment (stretch, shift, mirror, finger dropout), resample / pad to T, z-normalise per clip and coordinate
 * over all T*124 values in fp64.  1 <= T <= 4096.  One kernel, graph-capturable, bit-identical from run to run. */
int ishara_clip_batch(const float* raw, const ishara_clip_aug* clips, int32_t B, int32_t T, int32_t layout,
                      float* x, ishara_stream s);
/* ishara_clip_batch with the two augmentations of the reference's CTC training script (asl-translation-nb4.ipynb
 * spatial_random_affine, temporal_mask; drawn by ishara_amd/data.py draw_augmentation_ex) and the per-clip frame count.  The affine
 * is applied to the raw clip before the four augmentations of `base`, row-vector convention [x' y'] = [x y] * M + shift_xy:
 * x' = f32(f64(M00) x + f64(M10) y + f64(shift_xy)), y' = f32(f64(M01) x + f64(M11) y + f64(shift_xy)), z untouched; the temporal
 * mask zeroes whole augmented frames after them.  A zero frame (padding, shifted out, masked) and a dropped finger landmark stay
 * exactly 0 before the normalisation: the shift is not added to them.  M = identity, shift_xy = 0, m0 == m1 is ishara_clip_batch's
 * batch.  96 bytes, no padding. */
typedef struct ishara_clip_aug_ex {
    ishara_clip_aug base;
    float m[4];                     /* M00, M01, M10, M11 */
    float shift_xy;                 /* one scalar added to x' and y' */
    int32_t m0, m1;                 /* temporal mask [m0, m1) over the augmented frames (the index space of t0 / t1); m0 == m1: none */
    int32_t reserved;               /* 0 */
} ishara_clip_aug_ex;
/* frame_len [B] int32 in device memory or NULL: frame_len[b] = min(L2, T), 0 for an empty clip (n == 0), written by the kernel; x has
 * the same bits either way.  Arguments and refusals as for ishara_clip_batch; B == 0 launches nothing.  One kernel, no atomics,
 * graph-capturable, bit-identical from run to run. */
int ishara_clip_batch_ex(const float* raw, const ishara_clip_aug_ex* clips, int32_t B, int32_t T, int32_t layout,
                         float* x, int32_t* frame_len, ishara_stream s);
/* tf.nn.ctc_loss alone: logits [B,T,C] f32, labels [B,L] int64 padded with blank -> nll [B]; dlogits [B,T,C] = grad_scale * d nll / d logits
 * may be NULL; ws = ishara_ctc_workspace_bytes(B, T, L) bytes, 8-byte aligned, no initialisation needed.  B >= 0 (0: nothing is launched),
 * T >= 1 with 4*T + 256*ceil((2L+1)/64) bytes of LDS within what a launch grants (T <= 14844 at L = 255), 1 <= L <= 255, 2 <= C <= 64,
 * 0 <= blank < C; anything else is refused with a message before any HIP call.
 * A sample with no alignment (T < len + repeats) or with a label outside [0, C) is infeasible: nll[b] = 1e30 (>= 1e29), dlogits[b] =
 * grad_scale * softmax(logits[b]) (every posterior zero, all finite); an out-of-range label is read as blank, never used as an index.  The
 * other samples' outputs are bit-identical to a launch without it. */
int64_t ishara_ctc_workspace_bytes(int32_t B, int32_t T, int32_t L);
int ishara_ctc_loss(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C,
                    int32_t L, int32_t blank, float* nll, float* dlogits, float grad_scale,
                    void* ws, ishara_stream s);
/* with per-clip frame counts (see ishara_greedy_decode_ex): logit_length = frame_len[b], torch's input_lengths.  A sample whose label does
 * not fit its own Tb (Tb < len + repeats) is infeasible as above on its Tb rows; dlogits[b, t >= Tb] = +0 always.  sample_scale [B] f32 in
 * device memory (4-byte aligned, may be NULL) multiplies grad_scale for that sample's dlogits, not its nll: a reduction's per-sample weight.
 * flags: ISHARA_CTC_ZERO_INFEASIBLE makes every dlogits row of an infeasible sample +0 (torch's zero_infinity); nll stays 1e30.  Unknown
 * flag bits are refused.  ws = ishara_ctc_workspace_bytes(B, T, L). */
enum { ISHARA_CTC_ZERO_INFEASIBLE = 1 };
int ishara_ctc_loss_ex(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C,
                       int32_t L, int32_t blank, float* nll, float* dlogits, float grad_scale,
                       void* ws, const int32_t* frame_len, const float* sample_scale, uint32_t flags, ishara_stream s);
/* The dropout mask the kernels draw for (seed, site): out [rows, cols] f32 (0 or 1/(1-rate)). */
int ishara_dropout_mask(uint32_t seed, uint32_t site, int32_t rows, int32_t cols, float rate,
                        float* out, ishara_stream s);

/* tests/ablation: bit0 register-staged NT GEMM, bit1 register-transposing TN GEMM, bit2 LDS-tiled depthwise conv
 * (defaults: LDS-DMA NT, transposed-read TN, register-window depthwise conv); bits 4-11 ablation switches */
/* switches of the A-stationary GEMM family, the bits of ISHARA_AS_FLAGS: 1 paired half-line stores, 2 non-temporal side outputs, 16 / 32 the
 * chunked form at K = 256 / 512, 64 the C-stationary kernel (gemm_cs.hip) for bf16 K = 512 -> N = 256 (and K = 768 -> N = 256 without an
 * epilogue operand) at M > 49152 rows, 128 that kernel at any M (tests), 256 K = 768 stays on the tile kernel.  -1 = library default (115); 51 and 3 select the A-stationary kernels alone, as before bit 64 existed */
int ishara_debug_set_as_flags(int32_t flags);
/* the kernel (profiler key) ishara_op_dense_fwd_ex would run for these arguments, with a bias, under the current switches; host only, launches nothing */
const char* ishara_debug_dense_kernel_name(int32_t dt, int32_t M, int32_t K, int32_t N, int32_t act, int32_t with_resid);
/* the depthwise-conv kernel ishara_op_dwconv_fwd(_ex) (backward != 0: ishara_op_dwconv_bwd, or the model's BatchNorm-folding call) would run
 * for these arguments under the current switches: the prefix of its profiler name, a two-pass backward as "dgrad+wgrad", "" for a refused
 * call.  flags: 1 statistics wanted, 2 scratch given, 4 BatchNorm backward folded in.  Host only, launches nothing; valid until the next call */
const char* ishara_debug_dwconv_kernel_name(int32_t dt, int32_t backward, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, int32_t flags);
/* the same for the attention: the kernel behind ishara_op_attn_fwd (backward != 0: ishara_op_attn_bwd) and the models' attention, with its template
 * arguments, a kernel pair as "dq + dkv<...>", "" for a refused call.  impl: 0 lane-split, 1 MFMA where there is one.  flags: 1 dropout active,
 * 2 keep-bit buffer given, 4 head-major dqkv, 8 masked (an attn_bias table or key lengths given).  Host only, launches nothing; valid until the
 * next call */
const char* ishara_debug_attn_kernel_name(int32_t dt, int32_t backward, int32_t T, int32_t dh, int32_t impl, int32_t flags);
/* the same for a Conv1DBlock of the Keras hybrid (width d, kernel size k) at (B, T): the launch plan of its forward and backward under the current
 * switches as "forward|backward", e.g. "part+fold+prologue+psa|psa+fused_bn" ("-" for the backward half at inference), "" for a refused dtype or
 * shape.  flags: 1 drop-path active, 2 frame lengths given, 4 the per-sample-affine weight gradient switched on (the model: bf16 without
 * ISHARA_NO_PSA).  Host only, launches nothing; valid until the calling thread's next call */
const char* ishara_debug_conv_block_route_name(int32_t dt, int32_t training, int32_t B, int32_t T, int32_t d, int32_t k, int32_t flags);
/* 0: never use the 256 x 256 two-operand tile GEMM (gemm_big.hip) — A/B runs against the A-stationary kernel inside one process; 1: library default */
int ishara_debug_set_nt_big(int32_t on);
int ishara_debug_force_regstage(int32_t on);
/* Module probe (ISHARA_FAMILY_KERAS_HYBRID, bound handle): one module of the sequential graph run alone through the model's own
 * orchestration, so that it lands on the kernels ishara_forward / ishara_loss_backward take for it at (dtype, B).  Modules in forward
 * order: "stem", every Conv1DBlock by its parameter prefix, "squeezeformer_k/{ffn1,mha,conv,ffn2}", "conformer_k/{ffn1,mha,conv,ffn2}",
 * "head"; first_site / n_sites: the dropout site ids the module draws from.  The name is valid until the thread's next module_info call.
 * forward: x f32 [B,T,in_cols] ([B,T,F] for the stem; it must stay alive until the stem's backward) is converted to the handle's dtype
 * where the model holds the module's input, y f32 [B,T,out_cols] (the head: logits).  It invalidates the state of the last ishara_forward.
 * backward: zero-fills grads[0,trainable), then the module's backward on what its last forward(training=1) with the same B left, then the
 * deferred gradient sums; dy f32 [B,T,out_cols], dx f32 [B,T,in_cols] or NULL (the stem: NULL).  The head's backward starts at the CTC
 * kernel (dlogits and their padded 16-bit copy): ishara_debug_head_loss_backward, arguments of ishara_loss_backward plus dx [B,T,dim].
 * Refused with a message before anything is launched: an unbound handle, another family, i out of range, B outside 1..max_batch,
 * ISHARA_F16 with training=1, a backward without the matching training forward. */
int32_t ishara_debug_module_count(ishara_model* m);
int ishara_debug_module_info(ishara_model* m, int32_t i, const char** name, int32_t* in_cols, int32_t* out_cols, int32_t* first_site, int32_t* n_sites);
int ishara_debug_module_forward(ishara_model* m, int32_t i, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, ishara_stream s);
int ishara_debug_module_backward(ishara_model* m, int32_t i, const float* dy, int32_t B, float* dx, ishara_stream s);
int ishara_debug_head_loss_backward(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll,
                                    float loss_scale, float* dx, ishara_stream s);
/* the probe with per-clip frame lengths (ishara_forward_ex): frame_len device int32 [B] or NULL (= the plain probe); the backward call must be
 * given lengths exactly when its training forward was.  Modules without a masked operation (stem, ffn, the Conformer block's conv, head) ignore them. */
int ishara_debug_module_forward_ex(ishara_model* m, int32_t i, const float* x, int32_t B, float* y, int32_t training, uint32_t seed,
                                   const int32_t* frame_len, ishara_stream s);
int ishara_debug_module_backward_ex(ishara_model* m, int32_t i, const float* dy, int32_t B, float* dx, const int32_t* frame_len, ishara_stream s);

/* ---- single-operator entry points (parity tests of the individual kernels) ------------ */
/* dt: ISHARA_F32 / ISHARA_BF16 / ISHARA_F16; the backward operators refuse ISHARA_F16 (inference only), every operator refuses an unknown
 * dtype, both before anything is launched. */
/* y = act(x @ W + b): x [M,K] (dtype dt), W [K,N] f32, y [M,N] (dt); scratch >= ishara_op_scratch_bytes */
int64_t ishara_op_scratch_bytes(int32_t M, int32_t K, int32_t N);
int ishara_op_dense_fwd(int32_t dt, const void* x, const float* W, const float* bias, void* y,
                        int32_t M, int32_t K, int32_t N, int32_t act, void* scratch, ishara_stream s);
/* y = act(x @ W + b) + resid   (resid may be NULL) */
int ishara_op_dense_fwd_ex(int32_t dt, const void* x, const float* W, const float* bias, const void* resid, void* y,
                           int32_t M, int32_t K, int32_t N, int32_t act, void* scratch, ishara_stream s);
/* dx = dy @ W^T ; dW += x^T dy ; db += colsum(dy) */
int ishara_op_dense_bwd(int32_t dt, const void* x, const float* W, const void* dy, void* dx,
                        float* dW, float* db, int32_t M, int32_t K, int32_t N, void* scratch, ishara_stream s);
/* One weight-gradient GEMM with every argument the models' backward passes give it (launch_gemm_tn through gemm_wgrad):
 *   out [ka_valid or Ka, nb_valid or Nb] f32 += A[M, Ka]^T . B[M, Nb];  dbias [nb_valid or Nb] f32 (may be NULL) += sum_m rs[m / bias_T] * B[m, :]
 * dtA / dtB: the operands' storage types, dtM: the MFMA operand type (ISHARA_F32 / ISHARA_BF16; an f32 operand under dtM = bf16 is rounded
 * to bf16 while it is staged).  ka_valid / nb_valid (0: none): columns [ka_valid, Ka) of A / [nb_valid, Nb) of B are zero padding that out and
 * dbias do not have (bf16 transposed-read kernel only; nb_valid % 4 == 0; no dbias with ka_valid).  bias_rowscale (may be NULL: rs = 1):
 * ceil(M / bias_T) f32, bias_T % 32 == 0, transposed-read kernel only.  The per-sample-affine block is present when psa_T != 0 or any of its
 * pointers is set: P, Q [M / psa_T, Ka] f32, W bf16 [Ka][ldw] (ldw >= Nb), outputs G [M / psa_T, Nb] and Rpart [M / psa_T][Nb / 64][Ka] f32
 * (overwritten); then out += sum_b (P[b] (.) A_b)^T B_b + Q[b] (x) colsum(B_b), G[b, n] = sum_t B_b[t, n], Rpart[b][p][k] = sum over the 64
 * columns n of group p of W[k, n] * (A_b^T B_b)[k, n]; a bias_rowscale beside it must have bias_T == psa_T.  A, B 16-byte aligned, every f32
 * buffer 4-byte aligned.  The operand transforms (opA / opB) of launch_gemm_tn are not carried: no weight gradient of the models passes one. */
typedef struct ishara_gemm_tn_call {
    const void* A; const void* B;
    float* out; float* dbias;
    const float* bias_rowscale;
    const float* P; const float* Q; const void* W;
    float* G; float* Rpart;
    int32_t dtA, dtB, dtM;
    int32_t M, Ka, Nb, ka_valid, nb_valid;
    int32_t bias_T, psa_T, ldw, reserved;
} ishara_gemm_tn_call;
/* bytes of ONE slab buffer that takes every call of the list (the largest gemm_tn_slab_floats); -1 for a bad list */
int64_t ishara_op_gemm_tn_scratch_bytes(const ishara_gemm_tn_call* calls, int32_t n);
/* runs the n calls in order on stream s, as a backward pass does.  slab: 16-byte aligned, ishara_op_gemm_tn_scratch_bytes.  defer_slab0 / 1 both
 * NULL: every call sums its M-split partials at once (immediate mode).  Both given (each as large as slab, 16-byte aligned): the calls share one
 * deferred-sum state over them — the partial sums of a transposed-read call ride as extra workgroups of the next one, calls on other kernels
 * use slab — and what is still pending is summed before the entry returns (launch_gemm_tn_flush).  Before any HIP call it refuses, for every
 * call of the list: a NULL or misaligned buffer, an unknown dtype, ISHARA_F16 (no fp16 weight gradients) and whatever launch_gemm_tn refuses,
 * with the launcher's message. */
int ishara_op_gemm_tn(const ishara_gemm_tn_call* calls, int32_t n, void* slab, void* defer_slab0, void* defer_slab1, ishara_stream s);
/* what launch_gemm_tn would do with one call under the current switches, read from the code that launches: route ("TN_BIG", "TN_TR",
 * "TN_TR_BRS", "TN_TR_PSA", "TN_REG"; "TN_REFUSED" with the launcher's message in ishara_last_error), the profiler key of the kernel
 * (gemm_tn_kernel_name; "" for a refused call), the number of M-splits and the rows per split.  The call's pointers are only tested for NULL
 * and alignment; out / dbias / G / Rpart need not be real.  Host only, launches nothing; the strings are static. */
int ishara_debug_gemm_tn_plan(const ishara_gemm_tn_call* call, const char** route, const char** kernel, int32_t* splits, int32_t* rows_per_split);
/* One forward / dgrad GEMM on the tile kernels of gemm_nt.hip with the arguments the models pass (launch_gemm_nt):
 *   C [M, N] (dtC) = epi( op(A) [M, K] (dtA) . Bt [N, K]^T (dtM) )
 * Bt is the CALLER-BUILT weight shadow [bt_rows][ldb] in dtM: bt_rows >= roundup(N, 128), ldb >= roundup(K, K tile) and whole 16-byte pieces
 * (K tile: 32 bf16 / 16 f32 on the LDS-DMA kernels, 64 / 32 on the register-staged one).  Rows n >= N are read and discarded (any value);
 * columns k in [K, ldb) must be zero (the register-staged kernel multiplies them with its zero-filled A tail).
 * op: 0 none, 1 swish(A), 2 A * c1[k] + c0[k] (c1, c0 f32, readable up to roundup(K, K tile) floats), 4 A * dropout mask(op_seed, op_site,
 * op_rate) — the mask of ishara_dropout_mask over [M, K]; 3 (row scale) is not carried.
 * Epilogue, in this order (each part optional): + bias[n] (* rowscale[m / T] when rowscale_bias) ; + addtab[(m % tab_period), n] ; pre_out = the
 * value so far ; act (0 none, 1 swish, 2 ReLU) ; * dropout mask(drop_seed, drop_site, drop_rate) over [M, N] ; * rowscale[m / T] (when not
 * rowscale_bias) ; dact (1: * swish'(aux), 2: 0 where aux <= 0) ; + resid ; then mode 0 stores C, mode 1 (QKV split; C may be NULL) scatters to
 * q, k [M / T, H, T, dh] and vt [M / T, H, dh, T] — head_major 1: columns are [q|k|v] per head, 0: [q of all heads | k | v]; N == 3 * H * dh, T and
 * dh multiples of 8, M a multiple of T.  pre_out, aux, resid, q, k, vt are dtC; bias, addtab, rowscale f32.  A, Bt 16-byte aligned; dtC buffers
 * 16-byte aligned (8-byte for 16-bit dtC on the 128 x 128 tile kernel); addtab 16-byte aligned on that kernel, f32 vectors 4-byte aligned. */
typedef struct ishara_gemm_nt_call {
    const void* A; const void* Bt; void* C;
    const float* c1; const float* c0;
    const float* bias; const float* addtab; void* pre_out;
    const float* rowscale; const void* aux; const void* resid;
    void* q; void* k; void* vt;
    int32_t dtA, dtM, dtC, op;
    int32_t M, N, K, bt_rows, ldb;
    uint32_t op_seed, op_site; float op_rate;
    int32_t tab_period, act;
    uint32_t drop_seed, drop_site; float drop_rate;
    int32_t T, rowscale_bias, dact, mode, H, dh, head_major;
} ishara_gemm_nt_call;
/* runs the call on stream s: exactly one kernel launch, nothing else.  Before any HIP call it refuses, with a message that names the field:
 * unknown dtypes / op / act / dact / mode, a NULL A / Bt / C, a misaligned buffer, a shadow smaller than the contract above, addtab with
 * tab_period < 1, rowscale with T < 1, dact without aux, an incomplete or inconsistent QKV split, a rate outside [0, 1), a call that lands on
 * another kernel family than the three tile kernels (ishara_debug_force_regstage 8192 / 8 / 1 selects them), and whatever launch_gemm_nt
 * refuses, with the launcher's message. */
int ishara_op_gemm_nt(const ishara_gemm_nt_call* call, ishara_stream s);
/* where ishara_op_gemm_nt would run the call under the current switches, read from the code that launches: route ("NT_TILE_T", "NT_GLDS",
 * "NT_REG"; "NT_REFUSED" for every call the entry refuses, with the reason in ishara_last_error) and the profiler key of the kernel
 * (gemm_nt_kernel_name; "" for a refused call).  Pointers are only tested for NULL and alignment.  Host only, launches nothing; the strings are static. */
int ishara_debug_gemm_nt_route(const ishara_gemm_nt_call* call, const char** route, const char** kernel);
/* One forward / dgrad GEMM on the A-stationary kernels (gemm_as.hip; fp16 operands: gemm_as_f16.hip): the call of ishara_op_gemm_nt plus the
 * fields only this family reads.  16-bit operands of one type (dtA == dtM, op 0), K in {256, 512} (bf16 operands with bf16 C also 128 and 1024),
 * N a multiple of 32 up to 1024, C in the operand type or f32.  Bt is the CALLER-BUILT weight shadow [bt_rows][ldb]: bt_rows >= N, ldb >= K and a multiple of 64;
 * rows n >= N and columns k >= K are never read.
 * ln_gamma / ln_beta [K] f32 (with ln_eps): the operand rows are LayerNorm-ed over K in registers, A' = (A - mean) * rstd * gamma + beta;
 *   ln_mean / ln_rstd [M] f32 (both or neither) receive the row statistics.  pa_P / pa_Q [ceil(M / T), K] f32: A' = A * P[m / T] + Q[m / T], T a
 *   multiple of the rows per workgroup (ishara_debug_gemm_as_plan).  At most one of the two; each with C in the operand type, K >= 256 and one of
 *   the epilogues it is compiled with (LayerNorm: none, act + pre_out, act + pre_out + dropout, QKV; affine: resid, resid + rowscale).
 *   pro_out [M, K] (operand type, may be NULL) receives A'.
 * ldc (0: N): elements between rows of C and pre_out, at least the columns a row stores, whole 16-byte pieces.  n_valid (0: all): only the columns below it are stored, bias
 *   is read below it only; a multiple of the 16-byte store group (8 for 16-bit C, 4 for f32).  Neither with resid, aux or a QKV split.
 * as_flags: bit 0 paired half-line stores, bit 1 non-temporal side outputs, bits 4 / 5 the chunked kernel at K = 256 / 512, bits 6 / 7 the
 *   C-stationary kernel's switches (a call that they send there is refused here); -1: the library default. */
typedef struct ishara_gemm_as_ext {
    const float* ln_gamma; const float* ln_beta; float* ln_mean; float* ln_rstd;
    const float* pa_P; const float* pa_Q; void* pro_out;
    float ln_eps;
    int32_t ldc, n_valid, as_flags;
} ishara_gemm_as_ext;
/* runs the call on stream s: exactly one kernel launch, nothing else.  Before any HIP call it refuses, with a message that names the field,
 * what ishara_op_gemm_nt refuses and: a NULL ext, a prologue without an instantiation for its epilogue, pa_P with T off the rows per workgroup,
 * ldc / n_valid with resid, aux or QKV or off their multiples, a misaligned C, pre_out, aux, resid, q, k, pro_out, addtab (16 bytes), a shadow
 * smaller than the contract above, and a call that lands on another kernel than the A-stationary ones (by the route's name). */
int ishara_op_gemm_as(const ishara_gemm_nt_call* call, const ishara_gemm_as_ext* ext, ishara_stream s);
/* what the A-stationary launcher does with the call, read from the function it launches from (gemm_nt_as_plan): route ("NT_AS", "NT_AS_F16";
 * "NT_REFUSED" for every call ishara_op_gemm_as refuses, the reason in ishara_last_error, everything else zero), the profiler key, rows per
 * workgroup, the grid (gx, gy), 32-column steps per workgroup, ring depth, column steps per stage, waves, the sequential row passes of a
 * workgroup and their rows, whether the chunked kernel runs, whether paired stores are active, the compiled epilogue mask (255: all features
 * behind run-time flags) and the prologue (0 none, 1 LayerNorm, 2 affine).  Host only, launches nothing; the strings are static. */
typedef struct ishara_gemm_as_plan {
    const char* route; const char* kernel;
    int32_t rows, gx, gy, nsteps, ring, cs, waves, passes, pass_rows[2], chunked, hold, inst_mask, prologue;
} ishara_gemm_as_plan;
int ishara_debug_gemm_as_plan(const ishara_gemm_nt_call* call, const ishara_gemm_as_ext* ext, ishara_gemm_as_plan* plan);
/* QKV projection of the attention module at inference: LayerNorm of x [B*T, H*dh] (gamma, beta f32; gamma NULL: none; H*dh <= 512 with it),
 * x @ W + b (W [H*dh, 3*H*dh] f32, bias [3*H*dh] or NULL) scattered to q, k [B,H,T,dh] and vt [B,H,dh,T] (dt) — head_major 1: W's columns
 * are [q|k|v] per head, 0: [q of all heads | k | v].  T, dh multiples of 8.  The LayerNorm runs inside the GEMM or as a kernel of its own
 * exactly as in ishara_forward.  scratch >= ishara_op_qkv_scratch_bytes, 16-byte aligned. */
int64_t ishara_op_qkv_scratch_bytes(int32_t B, int32_t T, int32_t H, int32_t dh);
int ishara_op_qkv_fwd(int32_t dt, const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
                      void* q, void* k, void* vt, int32_t B, int32_t T, int32_t H, int32_t dh, int32_t head_major, void* scratch, ishara_stream s);
/* the head's classifier: logits [M, C] f32 = x [M, K] (dt) @ W [K, C] f32 + bias.  route 1: the A-stationary kernel over the zero-padded
 * 64-row weight shadow, storing the C real columns (16-bit dt, C <= 64, C % 4 == 0, K 256 / 512); 2: dense_narrow (16-bit dt, C <= 64,
 * K % 32 == 0); 3: the NT GEMM with fp32 output; 0: the route ishara_forward takes — 1 when it applies and M <= 1536, else 2 when it applies
 * and M <= 4096, else 3.  A route that does not take the shape returns an error and launches nothing.  scratch >=
 * ishara_op_scratch_bytes(M, K, C), 16-byte aligned. */
int ishara_op_classifier_fwd(int32_t dt, const void* x, const float* W, const float* bias, float* logits, int32_t M, int32_t K, int32_t C,
                             int32_t route, void* scratch, ishara_stream s);
/* ishara_ctc_loss as the head runs it: the same arguments, refusals and contract, plus dlb [B*T, 128] bf16 (4-byte aligned, may be NULL): the
 * rows of dlogits rounded to bf16 and zero padded to 128 classes, the MFMA operand of the classifier's backward.  Written only with dlogits. */
int ishara_op_ctc_loss(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                       float* nll, float* dlogits, float grad_scale, void* ws, void* dlb, ishara_stream s);
/* y[m,:C] = x[m,:C] - logsumexp(x[m,:C]) over C fp32 logits in rows of stride ld >= C floats (columns C..ld-1 of the outputs are zeroed: a class
 * count padded to the GEMMs' 16-byte row alignment); dx = dy - exp(y) * rowsum(dy).  Replaces F.log_softmax(self.fc(...), dim=-1) of the
 * reference's torch Squeezeformer (squeezeformer/model.py:448-449). */
int ishara_op_log_softmax_fwd(const float* x, float* y, int32_t M, int32_t C, int32_t ld, ishara_stream s);
int ishara_op_log_softmax_bwd(const float* dy, const float* y, float* dx, int32_t M, int32_t C, int32_t ld, ishara_stream s);
int ishara_op_layernorm_fwd(int32_t dt, const void* x, const float* gamma, const float* beta, float eps,
                            void* y, float* mean, float* rstd, int32_t M, int32_t C, ishara_stream s);
int ishara_op_layernorm_bwd(int32_t dt, const void* dy, const void* x, const float* mean, const float* rstd,
                            const float* gamma, void* dx, float* dgamma, float* dbeta, int32_t M, int32_t C,
                            ishara_stream s);
/* inop: 0 none, 1 swish, 2 GLU (x has 2C channels) */
int ishara_op_dwconv_fwd(int32_t dt, int32_t inop, const void* x, const float* w, const float* bias, void* y,
                         float* ssum, float* ssq, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl,
                         ishara_stream s);
/* the same with caller scratch (ishara_op_dwconv_fwd_scratch_bytes) for the statistics: per-workgroup partial rows summed in a fixed order, no
 * float atomics — the path the model itself takes */
int64_t ishara_op_dwconv_fwd_scratch_bytes(int32_t B, int32_t T, int32_t C);
int ishara_op_dwconv_fwd_ex(int32_t dt, int32_t inop, const void* x, const float* w, const float* bias, void* y,
                            float* ssum, float* ssq, void* scratch, int32_t B, int32_t T, int32_t C, int32_t k,
                            int32_t padl, ishara_stream s);
int64_t ishara_op_dwconv_scratch_bytes(int32_t C, int32_t k);
/* scratch: ishara_op_dwconv_scratch_bytes(C,k) bytes, or NULL (atomic weight-grad path) */
int ishara_op_dwconv_bwd(int32_t dt, int32_t inop, const void* dy, const void* x, const float* w, void* dx,
                         float* dw, float* dbias, void* scratch, int32_t B, int32_t T, int32_t C, int32_t k,
                         int32_t padl, ishara_stream s);
/* the BatchNorm backward as a launch of its own: dx [B,T,C] (dt) = a[c] * (dy * sg[b,c] + E[b or 0, c] - (h - mean[c]) * rstd[c] * Fc[c]); h the
 * BatchNorm input, mean / rstd / a / Fc [C] f32, E [B,C] (e_per_sample 1) or [C] (0), sg [B,C] or NULL (= 1) */
int ishara_op_bn_bwd_apply(int32_t dt, const void* dy, const void* h, const float* mean, const float* rstd, const float* a, const float* sg,
                           const float* E, int32_t e_per_sample, const float* Fc, void* dx, int32_t B, int32_t T, int32_t C, ishara_stream s);
/* ishara_op_dwconv_bwd on the gradient of a BatchNorm output dy, h being the conv's forward output, as the model's conv modules run it:
 * returns 1 when the one-pass kernel applied the BatchNorm backward to every dy row on its way in (tmp untouched), 0 when
 * ishara_op_bn_bwd_apply into tmp [B,T,C] (dt) and ishara_op_dwconv_bwd on tmp ran instead, < 0 on error.  sg, dbias and scratch may be NULL.
 * All three refuse, before any GPU work and each with its own message: ISHARA_F16, B or T < 1, B > 65535, C no positive multiple of 8, k outside
 * 1..31, padl outside [0, k), a NULL required operand, an operand off a 16-byte boundary. */
int ishara_op_dwconv_bwd_bn(int32_t dt, int32_t inop, const void* dy, const void* h, const float* mean, const float* rstd, const float* a,
                            const float* sg, const float* E, int32_t e_per_sample, const float* Fc, const void* x, const float* w, void* dx,
                            float* dw, float* dbias, void* scratch, void* tmp, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl,
                            ishara_stream s);
/* attention on packed qkv [B*T, 3*H*dh] (head-major packing): o [B*T, H*dh]; scratch (256-byte aligned) holds q,k,vt,lse,delta,maskw.
 * ISHARA_F16: rate 0 only.  impl: 0 lane-split (f32 / bf16 / f16; head dim 8, 16, 24, 32, 48, 64; any T), 1 MFMA (bf16 and, forward only, f16;
 * head dim 32 / 64; T % 8 == 0; every other dtype / head dim runs the lane-split kernels) with the dropout keep bits cached in the scratch,
 * 2 the same MFMA kernels with no keep-bit buffer (the backward kernels hash again; bf16 and head dim 32 / 64 only).  B, H, T >= 1,
 * B*H <= 65535, rate in [0, 1), qkv / o / dout / dqkv 16-byte aligned: anything else is refused before any GPU work.
 * ishara_op_attn_scratch_layout_bytes: out[0..5] = byte offset and extent of lse [B*H*T] f32, of delta [B*H*T] f32 and of the keep-bit words inside
 * the scratch; what lies between an extent's end and the next offset (or the scratch's end) is padding no kernel writes. */
int64_t ishara_op_attn_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh);
int ishara_op_attn_scratch_layout_bytes(int32_t B, int32_t H, int32_t T, int32_t dh, int64_t* out);
int ishara_op_attn_fwd(int32_t dt, const void* qkv, void* o, int32_t B, int32_t H, int32_t T, int32_t dh,
                       float scale, uint32_t seed, uint32_t site, float rate, int32_t impl,
                       void* scratch, ishara_stream s);
int ishara_op_attn_bwd(int32_t dt, const void* o, const void* dout, void* dqkv, int32_t B, int32_t H,
                       int32_t T, int32_t dh, float scale, uint32_t seed, uint32_t site, float rate,
                       int32_t impl, void* scratch, ishara_stream s);

/* ---- the torch Squeezeformer family's own kernels, through the launch code ishara_encoder_forward / _backward use.  dt: ISHARA_F32 /
 * ISHARA_BF16 (the family has no fp16 kernels: ISHARA_F16 is refused).  Every buffer 16-byte aligned; shapes, null and alignment are checked
 * before anything is launched; every output, the parameter gradients included, is overwritten. */
/* Relative-position attention.  q, k, v, o, dO, dq, dk, dv [B*T, H*dh] (dt, head h in columns h*dh ..); pe [2T-1, H*dh] f32 the positional
 * table; Wpos [H*dh, H*dh] f32 in [in, out] layout; u, vb, du, dvb [H*dh] f32; dh 8 / 16 / 32 / 64; rate in [0, 1).  The forward converts the
 * table to dt, builds the weight shadow, runs pos_proj (dt operands, f32 output, M = 2T-1) and the attention with scale 1/sqrt(dh) and the
 * dropout of (seed, site, rate); lse [B*H*T] f32 is optional.  The table copy, posp and lse stay in scratch (ishara_op_relattn_scratch_bytes)
 * for the backward call, which takes the forward's q, k, v, u, vb, o again and returns dWpos [H*dh, H*dh] and, optionally, dposp [2T-1, H*dh]. */
int64_t ishara_op_relattn_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh);
int ishara_op_relattn_fwd(int32_t dt, const void* q, const void* k, const void* v, const float* pe, const float* Wpos, const float* u, const float* vb,
                          void* o, float* lse, int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                          void* scratch, ishara_stream s);
int ishara_op_relattn_bwd(int32_t dt, const void* q, const void* k, const void* v, const float* u, const float* vb, const void* o, const void* dO,
                          void* dq, void* dk, void* dv, float* du, float* dvb, float* dWpos, float* dposp,
                          int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate, void* scratch, ishara_stream s);
/* The same pair with per-clip key lengths: key_len device int32 [B], keys at this T (clamped to [0, T]); the keys j >= key_len[b] are masked.
 * route 0: the plan's choice (ishara_debug_relattn_kernel_name reports it), 1: the fp32 lane kernels.  Same checks and messages as the pair above,
 * then a NULL or misaligned key_len and an unknown route.  A clip with key_len 0: o = 0, dq = 0, nothing of its dO in dk / dv / du / dvb / dposp;
 * the dk / dv rows at keys >= key_len[b] are exact zeros.  ishara_debug_relattn_kernel_name: "" for a refused dtype / head dim / T; host only. */
int64_t ishara_relattn_len_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh);
int ishara_relattn_len_fwd(int32_t dt, const void* q, const void* k, const void* v, const float* pe, const float* Wpos, const float* u, const float* vb,
                           void* o, float* lse, int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                           const int32_t* key_len, int32_t route, void* scratch, ishara_stream s);
int ishara_relattn_len_bwd(int32_t dt, const void* q, const void* k, const void* v, const float* u, const float* vb, const void* o, const void* dO,
                           void* dq, void* dk, void* dv, float* du, float* dvb, float* dWpos, float* dposp,
                           int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                           const int32_t* key_len, int32_t route, void* scratch, ishara_stream s);
const char* ishara_debug_relattn_kernel_name(int32_t dt, int32_t backward, int32_t T, int32_t dh, int32_t masked);
/* DepthwiseConv2dSubsampling: x [B,T0,F] f32, w1, w2 [d,9], b1, b2 [d] f32 -> sub [B*T2, d*F2] (dt), T1 = (T0-3)/2+1, T2 = (T1-3)/2+1, same
 * for F; T0, F >= 7.  The first convolution's output stays in scratch for the backward call: dsub (dt) -> dw1, db1, dw2, db2 and dx [B,T0,F]
 * f32 (NULL: not computed). */
int64_t ishara_op_r4_subsample_scratch_bytes(int32_t B, int32_t T0, int32_t F, int32_t d);
int ishara_op_r4_subsample_fwd(int32_t dt, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, void* sub,
                               int32_t B, int32_t T0, int32_t F, int32_t d, void* scratch, ishara_stream s);
int ishara_op_r4_subsample_bwd(int32_t dt, const float* x, const float* w1, const float* w2, const void* sub, const void* dsub,
                               float* dw1, float* db1, float* dw2, float* db2, float* dx, int32_t B, int32_t T0, int32_t F, int32_t d,
                               void* scratch, ishara_stream s);
/* TimeReductionLayer and time_reduction_proj: h [B,Tin,d] (dt), conv_w [9], conv_b [1], Wred [Fr,d] ([in, out]), bred [d] f32 -> red [B*Tr, d]
 * (dt); Tr = (Tin-3)/2+1, Fr = (d-1)/2, the Linear runs over K = Kp = Fr rounded up to 8; Tin, d >= 3, d % 8 == 0.  conv_out [B*Tr, Kp] (dt,
 * optional): the convolution's output with its zero pad columns.  Backward: dred (dt) and extra [B,Tin,d] (dt, NULL: none; added to dh) ->
 * dh [B,Tin,d] (dt), dconv_w [9], dconv_b [1], dWred [Fr,d], dbred [d]. */
int64_t ishara_op_r4_time_reduce_scratch_bytes(int32_t B, int32_t Tin, int32_t d);
int ishara_op_r4_time_reduce_fwd(int32_t dt, const void* h, const float* conv_w, const float* conv_b, const float* Wred, const float* bred,
                                 void* red, void* conv_out, int32_t B, int32_t Tin, int32_t d, void* scratch, ishara_stream s);
int ishara_op_r4_time_reduce_bwd(int32_t dt, const void* h, const float* conv_w, const void* dred, const void* extra, void* dh,
                                 float* dconv_w, float* dconv_b, float* dWred, float* dbred, int32_t B, int32_t Tin, int32_t d,
                                 void* scratch, ishara_stream s);
/* row maps over dst [B,Tdst,d] from src [B,Tsrc,d] (dt).  mode 0: dst[t] = src[t/2]; 1: dst[t] = src[t]; 2: dst[t] = src[2t] + src[2t+1];
 * 3: dst[t] = t < Tsrc ? src[t] : 0; 4: dst = a + src (Tdst == Tsrc; a is read by this mode only) */
int ishara_op_r4_rows(int32_t dt, int32_t mode, const void* src, const void* a, void* dst, int32_t B, int32_t Tdst, int32_t Tsrc, int32_t d,
                      ishara_stream s);

#ifdef __cplusplus
}
#endif
#endif
