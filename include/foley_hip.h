/* libfoley_hip.so - C ABI of the MI355X (gfx950) HunyuanVideo-Foley sampling path.
 *
 * The reference (phazei/ComfyUI-HunyuanVideo-Foley) is pure Python and has no FFI of its own;
 * each entry point below replaces a Python-level interface of the reference's hot path, which a
 * maintainer would bind with ctypes (see INTEGRATION.md for the stub):
 *
 *   foley_ctx_create / foley_set_tensor   <- HunyuanModelLoader.load_model (nodes.py:72-133) and
 *                                            load_dac_any (utils.py:61-87): weights -> device
 *   foley_prepare                         <- the per-run setup of denoise_process_with_generator
 *                                            (utils.py:144-199) + the step-invariant part of
 *                                            HunyuanVideoFoley.forward (hifi_foley.py:744-807)
 *   foley_dit_forward                     <- HunyuanVideoFoley.forward (hifi_foley.py:707-924)
 *   foley_sample                          <- the denoising loop (utils.py:201-247) incl.
 *                                            FlowMatchDiscreteScheduler.step
 *                                            (scheduling_flow_match_discrete.py:210-297)
 *   foley_dac_decode                      <- DAC.decode (dac_vae/model/dac.py:280-303)
 *   foley_op_*                            <- the individual torch ops the reference calls on the
 *                                            path (F.linear, conv1d, SDPA, layer_norm, ...), used
 *                                            by the parity tests and micro-benchmarks
 *
 * Conventions: every function returns 0 on success or a negative error code and never throws;
 * foley_last_error() gives the message of the calling thread's last failure.  All tensor
 * arguments are raw DEVICE pointers (torch `tensor.data_ptr()`), owned by the caller and only
 * borrowed for the duration of the call, except tensors registered with foley_set_tensor, which
 * the caller must keep alive until the context is destroyed.  `stream` is a hipStream_t passed
 * as void* (torch.cuda.current_stream().cuda_stream); work is enqueued, not synchronised, unless
 * stated.  A context is used by one thread at a time.  Plain C types only - no torch types.
 */
#ifndef FOLEY_HIP_H
#define FOLEY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOLEY_ABI_VERSION 13   /* 13: the seven foley_op_solver_step* entries became the one foley_op_solver_step(const foley_step_desc*, stream) - the positional pred .. rows_dtype are the fields of the same names, the gd argument of the _guided entries is .gd, the x0 / x0_clips / noise / mask / mask_clips arguments of the _edit entries and n_win / starts / weights / Ltot of the _windows entries are the fields of those names (x0 != NULL / n_win != 0 select the form), foley_step_hist_desc.hist / .hist_slots are .hist / .hist_slots and its .guidance pointer is the embedded .gd; 12 (additions that leave every existing entry as it was, so the version stays): foley_prepare_sets, foley_op_resample_sinc, foley_op_logmel, head_dim 96 in foley_op_attention_hd (the sync scorer); 12: foley_op_qkv_regroup.n_rows / foley_op_attention_scatter.out_nrows (the caller-supplied row tables are range-checked on the device: source rows clamped, output rows outside the buffer dropped); 11: foley_op_resize_aa_u8 (the frames' antialiased uint8 resize, bit for bit), foley_op_attention_scatter, foley_rowbcast.periodic_cfgs; 10: foley_op_qkv_regroup (token regrouping of the conditioning encoders' attention); 9: foley_bcast_local (single-process grouped broadcast of the arenas); 8: foley_qkv_split_desc.attn_* (cross attention in the epilogue of its q projection), foley_abort / FOLEY_ERR_ABORTED; 7: FOLEY_DT_F16 as a compute dtype (foley_config.compute_dtype, op descriptors); 6: foley_rowbcast.Ls (mode 2: nearest-exact up-sampled operand); 5: reference-keyed loading (foley_weights_*, foley_load_tensor, foley_bcast_weights); 4: fp8 weight storage (dtype codes 3/4, foley_gemm_desc.ldw/.wfmt); 3: foley_profile_forward; 2: foley_gemm_desc gained partials / qkv / rstride; foley_op_ln_mod_pending, foley_dac_encode */

enum foley_dtype {
  FOLEY_DT_F32 = 0, FOLEY_DT_BF16 = 1, FOLEY_DT_I32 = 2,
  FOLEY_DT_F8E4M3 = 3,  /* OCP e4m3fn, weight storage only (reference FP8WeightWrapper, utils.py:316-366: plain cast, no scales) */
  FOLEY_DT_F8E5M2 = 4,  /* OCP e5m2,   weight storage only */
  FOLEY_DT_F16 = 5      /* IEEE fp16: a checkpoint dtype, and a compute dtype (the loader's precision=fp16, which the reference
                           runs under torch.autocast(float16): nodes.py:89-106, utils.py:229-234) */
};

enum foley_status {
  FOLEY_OK = 0,
  FOLEY_ERR_INVALID = -1,   /* bad argument / shape / dtype            */
  FOLEY_ERR_MISSING = -2,   /* a required tensor was never registered  */
  FOLEY_ERR_HIP = -3,       /* HIP runtime failure                      */
  FOLEY_ERR_STATE = -4,     /* call order violated (e.g. no prepare)    */
  FOLEY_ERR_ABORTED = -5    /* foley_abort() ended the sampling loop    */
};

typedef struct foley_ctx foley_ctx;

/* Model dimensions (configs/hunyuanvideo-foley-xxl.yaml model_kwargs; utils.py:32-44 for DAC). */
typedef struct foley_config {
  int32_t depth_triple, depth_single, hidden, heads;
  int32_t mlp_hidden;    /* triple-block MLP hidden  = hidden * mlp_ratio          */
  int32_t conv_hidden;   /* single-block ConvMLP hidden (mlp_layers.py:141-142)     */
  int32_t sync_hidden;   /* sync_in ConvMLP hidden                                 */
  int32_t cond_dim, clip_dim, sync_dim, latent_dim, time_freq_dim;
  int32_t compute_dtype; /* FOLEY_DT_F32 (parity mode), FOLEY_DT_BF16 or FOLEY_DT_F16 (throughput) for DiT GEMM operands */
  int32_t dac_dim;       /* decoder width (2048)                                    */
  int32_t dac_n_rates;   /* 5                                                       */
  int32_t dac_rates[8];  /* 8,5,4,3,2                                               */
  int32_t dac_dilations[3];
} foley_config;

/* One sampling run: conditioning + host-built index/trig tables (all device pointers). */
typedef struct foley_plan {
  int32_t ncfg;          /* 2 with classifier-free guidance ([uncond ; cond]), else 1 (utils.py:193-199); 3: separate video and
                            text guidance ([nothing ; video ; video + prompt], see foley_set_guidance) */
  int32_t clips;         /* batch_size: independent clips sharing the conditioning (per clip: foley_prepare_sets) */
  int32_t La, Lv, Ls, Lt;/* audio / visual / sync / text token counts                */
  int32_t n_iter;        /* loop iterations (= steps; multi-stage solvers still do one model call per iteration) */
  float guidance;
  const float* text;     /* [ncfg, Lt, cond_dim]  zero-padded to Lt (utils.py:103-111) */
  const float* clip;     /* [ncfg, Lv, clip_dim]  */
  const float* sync;     /* [ncfg, Ls, sync_dim]  */
  const float* t_feat;   /* [n_iter, time_freq_dim] sinusoidal timestep features (embed_layers.py:76-101) */
  const float* rope_cos; /* [rope_len, 64] cos(pos * theta^(-2k/128)) (posemb_layers.py:117-172) */
  const float* rope_sin;
  int32_t rope_len;      /* >= 2*La                                                 */
  const int32_t* pos_audio_self;  /* [La]  interleaved-RoPE position of audio token i  (= 2i)        */
  const int32_t* pos_visual_self; /* [Lv]  interleaved-RoPE position of visual token j (hifi_foley.py:35-60) */
  const int32_t* pos_linear;      /* [max(La,Lv,Lt)] 0,1,2,...                          */
  const int32_t* sync_gather;     /* [La]  nearest-exact source row of the sync up-sampling (hifi_foley.py:761) */
  const float* solver_coef;       /* [n_iter, 8] {w_new, w_acc, dt, w_store, flags,0,0,0} per iteration */
} foley_plan;

typedef void (*foley_progress_cb)(int32_t iteration, int32_t n_iter, void* user);

uint32_t foley_abi_version(void);
const char* foley_last_error(void);

int foley_ctx_create(int device, const foley_config* cfg, foley_ctx** out);
void foley_ctx_destroy(foley_ctx* ctx);

/* Register one packed tensor (names and layouts: DESIGN.md "packed weight arena"). */
int foley_set_tensor(foley_ctx* ctx, const char* name, const void* dev_ptr, int dtype, int ndim,
                     const int64_t* shape);

/* ---- Reference-keyed loading (replaces HunyuanModelLoader.load_model nodes.py:72-133 + load_dac_any
 * utils.py:61-87 for a caller that keeps the reference's checkpoints / loader): hand over the tensors under
 * their STATE-DICT KEYS and the library packs them on the device into ONE ctx-owned arena (layouts of
 * (K H D) q/k/v rows, tap-major convs, interleaved SwiGLU pairs, fused single-block
 * modulation, folded weight-norm, transposed convs as phases x 2 taps) and registers the packed tensors.
 *   foley_weights_begin(ctx, fmt)      allocate + register; fmt 0: block matrices in the compute dtype,
 *                                      1 / 2: kept in fp8 e4m3fn / e5m2 (reference _wrap_fp8_inplace,
 *                                      utils.py:408-485; bf16 compute only)
 *   foley_load_tensor(ctx, key, ...)   one checkpoint tensor (f32 / bf16 / f16 / fp8, any order), borrowed for
 *                                      the call; returns 1 for keys the sampling path does not use
 *                                      (DAC encoder / quantizer, final_layer.adaLN_modulation)
 *   foley_weights_end(ctx)             fails with FOLEY_ERR_MISSING if a packed tensor is incomplete
 *   foley_weights_arena                the arena (device pointer, bytes): layout depends on the config only
 *   foley_bcast_weights(ctx, comm, root, stream)   ONE ncclBroadcast (RCCL over xGMI) of the arena on the
 *                                      caller's ncclComm_t; non-root ranks call foley_weights_begin first.
 *                                      (A host that broadcasts the arena itself - e.g. torch.distributed on
 *                                      the pointer - calls foley_weights_mark_received afterwards.) */
int foley_weights_begin(foley_ctx* ctx, int weight_format);
int foley_load_tensor(foley_ctx* ctx, const char* ref_key, const void* dev_ptr, int dtype, int ndim,
                      const int64_t* shape, void* stream);
int foley_weights_end(foley_ctx* ctx, void* stream);
int foley_weights_arena(foley_ctx* ctx, void** dev_ptr, uint64_t* bytes);
/* Read-only slot lookup (additive within ABI 12): where one packed tensor lives in the ctx-owned arena.  name == NULL: slot `index`
 * of the layout's own order (0, 1, ... until the call returns 1); name != NULL: the slot of that packed name (`s0.qkv.w`,
 * `dac.0.up.w`, ...; `index` is ignored), 1 if there is none.  Every output pointer may be NULL.  name_out receives at most
 * FOLEY_SLOT_NAME_MAX bytes including the terminator, shape at most 8 entries; dev_ptr = arena + offset, `bytes` the tensor's own
 * size (slot extents are 256-byte aligned, so the distance to the next slot may be larger).  Valid after foley_weights_begin; the
 * call reads host-side bookkeeping only - no device work, no change of the loader's state. */
#define FOLEY_SLOT_NAME_MAX 64
int foley_weights_slot(foley_ctx* ctx, int index, const char* name, char* name_out, void** dev_ptr, int* dtype, int* ndim,
                       int64_t* shape, uint64_t* offset, uint64_t* bytes);
int foley_weights_mark_received(foley_ctx* ctx);
int foley_bcast_weights(foley_ctx* ctx, void* nccl_comm, int root, void* stream);
/* Single-process form of the same step (one host process that drives all GPUs of the node, e.g. a ComfyUI prompt worker; the
 * reference has no counterpart - its only batching is utils.py:159-162 on one device): buffer i of devices[0] (`bytes[i]` bytes at
 * bufs[0 * nbuf + i]) is broadcast to bufs[d * nbuf + i] on every other device in ONE grouped RCCL launch (ncclCommInitAll over
 * `devices`, cached; ncclGroupStart / ncclBroadcast per (device, buffer) / ncclGroupEnd), then every device is synchronised. */
int foley_bcast_local(int ndev, const int* devices, int nbuf, void* const* bufs, const uint64_t* bytes);

/* ---- Low-rank adapters (LoRA) merged into the packed weights, in place (additive within ABI 13; csrc/lora.hip).  For a
 * checkpoint tensor W[O, I(, k)] named by its REFERENCE state-dict key (`triple_blocks.3.audio_self_attn_qkv.weight`,
 * `single_blocks.7.linear2.w1.weight`, ...) and adapters j = 0..n-1 in the caller's order, down_j [r_j, I(, k)], up_j [O, r_j(, 1)]:
 *     stored'[o, c] = rnd_store( f32(pristine[o, c]) + sum_j scale_j * sum_q up_j[o, q] * down_j[q, c] ),  c over the flattened (I, k)
 * `pristine` is the value the packed tensor held before any adapter (for bf16 / fp16 / fp8 storage: its stored rounding), operands
 * are widened to fp32, accumulation is fp32 in a fixed order, rnd_store is the loader's round-to-nearest-even store of the tensor's
 * dtype.  The destination is the tensor registered under the key's packed name - foley_set_tensor's or the arena of
 * foley_weights_begin - at unchanged addresses, so a captured loop iteration stays valid and an fp8 arena stays fp8.  The first
 * time a packed tensor is touched the library copies it to a buffer of its own (at most one more arena in total); every merge
 * starts from those copies, so a set of adapters gives the same bytes whatever was merged before it.
 *   foley_lora_begin(ctx, stream)       every touched tensor back to its pristine bytes; forget the merged set
 *   foley_lora_merge(ctx, key, n, pairs, stream)   ALL adapters of one key in one call (n in [1, 8]); a second call for the same
 *                                       key before foley_lora_end is refused.  Targets: every weight matrix of the DiT, the
 *                                       embedders included; biases, norm gains, sync_pos_emb, the empty features and the DAC are
 *                                       not targetable.  Unknown or non-targetable keys, shapes that do not match, an `up` with a
 *                                       kernel > 1, rank outside [1, 256], a non-finite scale, operands other than f32 / bf16 /
 *                                       f16: FOLEY_ERR_INVALID with a message naming the key and the reason, nothing written.
 *                                       The operands are device memory, borrowed until foley_lora_end returns.
 *   foley_lora_end(ctx, stream)         waits for the merges; the next run needs foley_prepare (as after foley_set_tensor)
 *   foley_lora_clear(ctx, stream)       foley_lora_begin + free the copies (foley_ctx_destroy frees them too)
 *   foley_lora_backup_bytes(ctx, &n)    bytes the pristine copies hold now
 * Re-registering or rewriting a packed tensor while a set is merged: call foley_lora_clear first (a copy whose tensor has moved
 * is dropped unused; foley_weights_begin drops them all). */
typedef struct {
  const void* down;        /* [rank, I(, k)], contiguous, the checkpoint's own (I, k) order */
  const void* up;          /* [O, rank(, 1)], contiguous */
  int32_t dtype;           /* FOLEY_DT_F32 / FOLEY_DT_BF16 / FOLEY_DT_F16, both operands */
  int32_t rank;
  int32_t down_ndim, up_ndim;            /* 2 or 3 */
  int64_t down_shape[3], up_shape[3];
  float scale;             /* strength * alpha / rank, formed by the caller */
} foley_lora_pair;
int foley_lora_begin(foley_ctx* ctx, void* stream);
int foley_lora_merge(foley_ctx* ctx, const char* ref_key, int n, const foley_lora_pair* pairs, void* stream);
int foley_lora_end(foley_ctx* ctx, void* stream);
int foley_lora_clear(foley_ctx* ctx, void* stream);
int foley_lora_backup_bytes(foley_ctx* ctx, uint64_t* bytes);

/* Step-invariant precompute for one run; allocates/reuses the context workspace. */
int foley_prepare(foley_ctx* ctx, const foley_plan* plan, void* stream);

/* Per-clip conditioning (additive within ABI 12): every batch row (cfg half h, clip k), row b = h*clips + k, reads its own text set
 * text_of[b] in [0, n_text) and its own visual set (clip and sync features together) vis_of[b] in [0, n_vis); plan.text then holds
 * [n_text, Lt, cond_dim], plan.clip [n_vis, Lv, clip_dim] and plan.sync [n_vis, Ls, sync_dim].  The maps are host memory of
 * ncfg*clips entries, read during the call.  The conditioning GEMMs run once per distinct set; a stream whose map gives one set
 * per cfg half (b -> b / clips with n = ncfg) keeps foley_prepare's per-half layout, any other map lays that stream's
 * conditioning out per batch row (visual: at most 32 rows).  sets == NULL is foley_prepare.  A captured loop iteration is keyed
 * on the maps as well. */
typedef struct foley_cond_sets {
  int32_t n_text, n_vis;
  const int32_t* text_of;   /* [ncfg*clips] */
  const int32_t* vis_of;    /* [ncfg*clips] */
} foley_cond_sets;
int foley_prepare_sets(foley_ctx* ctx, const foley_plan* plan, const foley_cond_sets* sets, void* stream);

/* Timed prompts (additive within ABI 12): a prompt timeline through a per-token cross-attention.  plan.text holds n_text text
 * sets [n_text, Lt, cond_dim], n_text in [1, 16] (FOLEY_TIMELINE_MAX_SETS), and every query token of the two-stream blocks'
 * cross-attention - batch row b = h*clips + k, token t in [0, Lv + La): the Lv visual tokens first, then the La audio frames, the
 * order of that attention's queries - reads
 *     out = (1 - alpha) * attention(q; set_a) + alpha * attention(q; set_b),
 * two complete softmaxes over the Lt keys of one set each; where alpha == 0 set_b is not read.  The three tables are HOST memory of
 * ncfg*clips*(Lv + La) entries, read during the call and copied into context-owned buffers.  Otherwise the call is foley_prepare:
 * the VISUAL side is shared per cfg half (plan.clip / plan.sync hold ncfg sets; per-clip visual sets are not carried here), the
 * K / V^T of the n_text sets are cached per block without a per-row gather, and the cross-q projection does not run the fused
 * attention epilogue: the timeline kernel is launched in its place.  A captured loop iteration is keyed on timeline on / off,
 * n_text and the table buffers: a new timeline of the same shape rewrites the tables a replay reads and keeps the graph.
 * foley_prepare / foley_prepare_sets clear the timeline state.  Indices outside [0, n_text), alpha outside [0, 1) (NaN included),
 * n_text outside [1, 16] and NULL tables: FOLEY_ERR_INVALID. */
#define FOLEY_TIMELINE_MAX_SETS 16
typedef struct foley_text_timeline {
  int32_t n_text;
  const int32_t* set_a;     /* [ncfg*clips*(Lv+La)] host */
  const int32_t* set_b;     /* [ncfg*clips*(Lv+La)] host */
  const float* alpha;       /* [ncfg*clips*(Lv+La)] host, in [0, 1) */
} foley_text_timeline;
int foley_prepare_timeline(foley_ctx* ctx, const foley_plan* plan, const foley_text_timeline* timeline, void* stream);

/* One DiT evaluation at loop iteration `iter` (its timestep modulation): latents [clips,C,La]
 * fp32 -> velocity rows [ncfg*clips*La, C] fp32 (row = (cfg*clips + clip)*La + l). */
int foley_dit_forward(foley_ctx* ctx, const float* latents, int iter, float* out_rows, void* stream);

/* Full denoising loop: `latents` [clips,C,La] fp32 holds the initial noise on entry and the final
 * latents on return.  With a progress callback the stream is synchronised once per iteration.
 * use_graph != 0 replays one captured hipGraph per iteration. */
int foley_sample(foley_ctx* ctx, float* latents, int use_graph, foley_progress_cb cb, void* user, void* stream);
/* Cancel a running foley_sample (the ComfyUI "interrupt": comfy.utils.ProgressBar.update raises inside the reference's loop,
 * utils.py:201,247).  Callable from the progress callback or from another thread; the loop stops after the current iteration
 * and foley_sample returns FOLEY_ERR_ABORTED with `latents` holding the state reached.  The request is consumed by the loop it
 * stops; one that arrives while no loop runs is dropped by the next foley_sample on entry. */
int foley_abort(foley_ctx* ctx);

/* Audio editing (additive within ABI 12): audio-to-audio variation and time-span regeneration.  Called after foley_prepare with
 * the plan of the SUFFIX [i0, n_iter) of the plain run's iterations (its t_feat and solver_coef rows); the caller starts the loop
 * from sigma_{k0}*noise + (1 - sigma_{k0})*x0 (foley_op_flow_mix).  Rows of solver_coef whose flags (column 4) carry
 * FOLEY_STEP_BLEND - the iterations that END a solver step, after which the sigma index moves to k+1 - hold sigma_{k+1} in
 * column 5, and after them every element is pulled back onto the source's forward-noised path:
 *   x <- m*x + (1 - m)*(sigma_{k+1}*noise + (1 - sigma_{k+1})*x0)     (m = mask[clip][l], 1 = regenerate)
 * and the next model input is staged from the blended value.  Intermediate stages of multi-stage solvers are not blended.
 * m = 1 leaves x bit for bit (an all-ones mask at i0 = 0 is the plain run exactly), m = 0 gives the target bit for bit.
 *   x0    [x0_clips, latent_dim, La] fp32: source latents (the DAC posterior mean), x0_clips 1 (shared) or plan.clips
 *   noise [plan.clips, latent_dim, La] fp32: the run's initial noise
 *   mask  [mask_clips, La] fp32 in [0, 1] or NULL (all ones), mask_clips 1 or plan.clips
 * The operands are copied into context-owned buffers (captured graphs never hold the caller's pointers); the captured iteration
 * is keyed on plain vs edit, so a context alternates between the two safely.  foley_prepare clears the edit state, as does a call
 * with x0, noise and mask all NULL.  x0 / noise missing with a mask, or clip counts other than 1 / plan.clips: FOLEY_ERR_INVALID;
 * before foley_prepare: FOLEY_ERR_STATE. */
#define FOLEY_STEP_BLEND 8
int foley_set_edit(foley_ctx* ctx, const float* x0, int x0_clips, const float* noise, const float* mask, int mask_clips,
                   void* stream);

/* Long clips as overlapping windows (additive within ABI 12).  Called after foley_prepare / foley_prepare_sets: the plan's clips
 * become `variations` = plan.clips / n_win long clips of Ltot = starts[n_win - 1] + La latent frames each.  Clip v*n_win + k is
 * window k of variation v: it covers the global frames [starts[k], starts[k] + La) with its own conditioning row(s) and RoPE
 * positions 0..La.  After every iteration whose solver_coef row carries FOLEY_STEP_BLEND (the iterations that end a solver step;
 * the plan is built with those rows, as for an edit run from iteration 0), every global frame g is replaced in all the windows
 * that cover it by one weighted mean
 *   xb[v][c][g] = sum_k weights[k][g - starts[k]] * x[v*n_win + k][c][g - starts[k]]      (fp32, in window order)
 * and the next model input of those windows is staged from xb, so the windows agree on their overlaps at every step.  Rows
 * without the flag (intermediate stages of heun-2 / midpoint-2 / kutta-4) leave every window its own value.  Exactness: a frame
 * one window covers has weight 1.0f and a single term and keeps its value bit for bit - disjoint abutting windows are the
 * uncoupled batch exactly; all covering windows hold the identical bits after a blend row.
 *   starts  [n_win] int32 on the HOST, ascending, starts[0] = 0, no gap (starts[k+1] <= starts[k] + La)
 *   weights [n_win, La] fp32 on the device; the weights of every global frame sum to 1, a singly covered frame has 1.0f
 * Both tables are copied into context-owned buffers; the captured iteration is keyed on n_win, Ltot and those buffers, so a
 * context alternates between plain and windowed runs safely.  n_win <= 1 or a NULL table clears the state, as does foley_prepare.
 * plan.clips % n_win != 0, starts that do not ascend from 0, a gap, or an edit state (foley_set_edit, in either call order):
 * FOLEY_ERR_INVALID; before foley_prepare: FOLEY_ERR_STATE.  foley_sample takes and returns the windows [clips, latent_dim, La];
 * foley_op_windows_stitch makes the long clips of them. */
int foley_set_windows(foley_ctx* ctx, int n_win, const int32_t* starts, const float* weights, void* stream);

/* Guidance: how the prediction halves become one velocity (additive within ABI 12).  The plan's row order is [half][clip][token].
 *   ncfg 2  halves [uncond ; cond]:                         v = u + g (c - u)
 *   ncfg 3  halves h0 = negative prompt + the empty visual rows, h1 = negative prompt + the clip's visual features,
 *           h2 = prompt + the same features:                v = p0 + g_video (p1 - p0) + g_text (p2 - p1)      (fp32, left to right)
 * Without this call g = g_video = g_text = plan.guidance for the whole run.  Called after foley_prepare / foley_prepare_sets:
 *   sched   [n_rows, 2] fp32 on the HOST, row i = {g_video, g_text} of loop iteration i (multi-stage solvers: every stage is
 *           an iteration); ncfg 2 reads column 0.  n_rows must equal plan.n_iter.  NULL: no table, the scalar stays.
 *   rescale phi in [0, 1]: every iteration the step uses f v with f = phi s_pos / s_cfg + (1 - phi) per batch clip, s_pos the
 *           standard deviation (about the mean, over the clip's latent_dim x La elements) of the last half, s_cfg that of v;
 *           f = 1 where s_cfg is 0.  In a windowed run every window is a clip and its factor is applied before the blend.
 *           phi > 0 adds two launches per iteration (deterministic: fixed merge order, no atomics); 0 adds none.
 * Table and phi are copied into context-owned buffers (captured graphs never hold the caller's pointers); the captured iteration
 * is keyed on schedule on/off, rescale on/off and those buffers, so new values of the same shape only rewrite what a replay
 * reads.  It combines with foley_set_edit and with foley_set_windows in either order (an edit run passes the rows [i0, steps) of
 * the plain run's table, like its solver_coef rows).  sched NULL with rescale 0 clears the state, as does foley_prepare.
 * plan.ncfg == 1, n_rows != plan.n_iter, rescale outside [0, 1]: FOLEY_ERR_INVALID; before foley_prepare: FOLEY_ERR_STATE. */
int foley_set_guidance(foley_ctx* ctx, const float* sched, int n_rows, float rescale, void* stream);

/* Projected guidance (additive within ABI 13; opt-in): APG (adaptive projected guidance, Sadat et al. 2024) and CFG-Zero* (Fan et al.
 * 2025) in place of the two-half combine.  Per batch clip, u and c are the clip's unconditional and conditional prediction rows,
 * <a,b> the sum over the clip's latent_dim x La elements, g the iteration's scale (the schedule's column 0 under foley_set_guidance,
 * else plan.guidance) and {eta, beta, R, live} row i of `rows` for loop iteration i (multi-stage solvers: every stage is an
 * iteration):
 *   FOLEY_GUIDANCE_APG        m = (c - u) + beta m_prev (an fp32 plane [clips*La, latent_dim], context-owned, updated in place;
 *                             beta == 0 reads nothing, so the first row of a run does not depend on what the plane holds);
 *                             r = (R > 0 && |m| > R) ? R / |m| : 1;  rho = <c,c> > 0 ? <m,c> / <c,c> : 0;
 *                             a_w = live (g - 1) r;  a_c = live (1 + (g - 1)(eta - 1) r rho);  w = m (the plane keeps the unclipped m)
 *   FOLEY_GUIDANCE_ZERO_STAR  s = <u,u> > 0 ? <c,u> / <u,u> : 0;  a_c = live g;  a_w = live (1 - g) s;  w = u
 *   both                      v = fma(a_c, c, rnd(a_w w)) in fp32
 * g == 1 gives v == c exactly (iterations outside a guidance interval), live == 0 a zero velocity (an euler row then leaves x and
 * the staged rows as they are).  APG with eta = 1, beta = 0, R = 0 is plain CFG to rounding, not bit for bit: v = c + (g - 1)(c - u)
 * against the plain step's fma(g, c - u, u).  R is in the model's velocity units.
 *   rows   [n_rows, 4] fp32 on the HOST; n_rows must equal plan.n_iter (an edit run passes the rows [i0, steps) with beta = 0 on
 *          its first).  Copied to a context-owned buffer: new values of the same shape keep the captured graph.
 *   mode 0 clears the state, as does foley_prepare.
 * Two launches per iteration in front of the step, where the rescale launches sit (under the step cache: in the full body and in
 * the skip body), deterministic: fixed merge order, no atomics.  The statistics are per clip, so a clip's result does not depend on
 * what it is batched with; in a windowed run every window is a clip and its coefficients apply before the blend.  It combines with
 * foley_set_edit, foley_set_windows, foley_set_multistep (the ring stores v as the step used it), foley_set_step_cache, a
 * schedule, timed prompts and per-clip conditioning.  The captured iteration is keyed on the mode and the buffers.
 * plan.ncfg != 2, a rescale state next to projection (in either call order; foley_set_guidance refuses rescale > 0 under projection
 * too), n_rows != plan.n_iter, non-finite rows, R < 0, an unknown mode, more than 256 latent channels: FOLEY_ERR_INVALID; before
 * foley_prepare: FOLEY_ERR_STATE. */
#define FOLEY_GUIDANCE_APG 1
#define FOLEY_GUIDANCE_ZERO_STAR 2
int foley_set_projected_guidance(foley_ctx* ctx, int mode, const float* rows, int n_rows, void* stream);

/* Step cache (additive within ABI 12; opt-in): reuse the blocks' residual on iterations whose model input barely moved - what
 * DiT samplers call TeaCache / first-block cache.  For one model call of loop iteration i (multi-stage solvers: every stage is an
 * iteration) let a0 be the audio stream after audio_embedder + add_sync, aN the stream after the last block and m the first
 * block's modulated audio input LayerNorm(a0; eps) * (1 + scale) + shift in fp32 (the eps and modulation rows that block's first
 * LayerNorm gets).  A FULL iteration runs the forward as ever and keeps delta = aN - a0 (fp32).  A SKIPPED iteration computes a0
 * from the current input rows, sets the stream to a0 + delta and runs final.layernorm, final.linear and the unchanged solver step
 * (guided / edit / windows form alike) - no modulation GEMM, no visual gather, no block.  Every iteration replaces m_prev by m and
 * measures rel = max over the batch rows b (half x clip) of sum|m - m_prev| / sum|m_prev| over the row's La x hidden elements
 * (0 where the denominator is 0).  Iteration 0, the last iteration and any iteration without a delta of this loop are full.
 *   mode FOLEY_STEP_CACHE_SCHEDULE   skip exactly the iterations with skip[i] != 0 (n_skip must equal plan.n_iter; an edit run
 *                                    passes the rows [i0, steps) of the plain run's list).  No read-back, no synchronisation.
 *   mode FOLEY_STEP_CACHE_THRESHOLD  every iteration i >= 1 adds poly(rel) to an accumulator (poly: n_poly coefficients, highest
 *                                    degree first; n_poly 0: the identity) and is skipped while the accumulator is < threshold;
 *                                    a full iteration resets it to 0.  interval (NULL: everywhere): iterations [interval[0],
 *                                    interval[1]) may skip; max_consecutive > 0 caps a run of skips.  One device-to-host copy of
 *                                    ncfg*clips floats and one stream synchronisation per iteration; ONE decision serves the
 *                                    whole context, so a clip's result depends on what it is batched with.
 *   mode 0                           clears the state, as does foley_prepare.
 * delta and m_prev ([ncfg*clips*La, hidden] fp32 each) are context-owned.  The captured iteration is keyed on cache on / off (on:
 * three linear graphs - head, full body, skip body); mode, threshold and list are host decisions and keep the graphs.  Off, a run
 * keeps its bits and its single graph.  n_skip != n_iter, a negative or non-finite threshold, non-finite coefficients, an interval
 * outside [0, n_iter]: FOLEY_ERR_INVALID; before foley_prepare: FOLEY_ERR_STATE.
 * foley_step_cache_report: rel[i] (-1: not measured - iteration 0, and every iteration of schedule mode) and skipped[i] of the
 * last foley_sample under the cache; n must equal its plan.n_iter. */
#define FOLEY_STEP_CACHE_SCHEDULE 1
#define FOLEY_STEP_CACHE_THRESHOLD 2
int foley_set_step_cache(foley_ctx* ctx, int mode, const uint8_t* skip, int n_skip, double threshold, const double* poly,
                         int n_poly, const int32_t* interval, int max_consecutive, void* stream);
int foley_step_cache_report(foley_ctx* ctx, float* rel, int32_t* skipped, int n);

/* Multistep solvers (additive within ABI 12; opt-in): variable-step Adams-Bashforth of order 2 or 3 at one model call per sigma
 * step.  The step reuses the velocities of the one or two iterations before it:
 *   x_{n+1} = x_n + dt (c_0 v_n + c_1 v_{n-1} + c_2 v_{n-2})
 * with the weights in the plan's solver_coef rows: c_0 in column 0 (w_new), c_1 in column 6, c_2 in column 7, and
 * FOLEY_STEP_HIST in the flags (column 4) of every row with a non-zero history weight.  The rows are those of a one-stage
 * (euler) table; the first row of a run has no history and is the Euler row, the second row of an order-3 run carries the
 * order-2 weights (host/tables.py builds them on the run's sigma grid; an edit run restarts the warm-up at its first row).
 * Arithmetic, fp32, contraction off:  t = c_0 v;  t = fma(c_1, v_{n-1}, t) if c_1 != 0;  t = fma(c_2, v_{n-2}, t) if c_2 != 0;
 * x = fma(t, dt, x).  A zero weight reads nothing, so warm-up rows do not depend on what the ring holds, and a table without
 * history weights gives the Euler run bit for bit.  v is the guided velocity exactly as the step uses it (schedule and rescale
 * factor included); every iteration stores it to a context-owned ring of order - 1 slots [clips, latent_dim, La] fp32.
 *   order 2 or 3   allocates the ring (grow-only) and switches the step to its history kernel
 *   order 0 or 1   clears the state, as does foley_prepare
 * Called after foley_prepare / foley_prepare_sets / foley_prepare_timeline; it combines with foley_set_edit, foley_set_windows,
 * foley_set_guidance and foley_set_step_cache in any order (a skipped iteration runs the unchanged step and feeds the ring).
 * The captured iteration is keyed on the ring and its slot count.  Order 3 is a third-order local formula behind a first-order
 * first step: its global order is 2, with a smaller constant.  The multi-stage solvers (heun-2, midpoint-2, kutta-4) do not
 * combine with it: their tables carry no history weights.
 * Any other order: FOLEY_ERR_INVALID; before foley_prepare: FOLEY_ERR_STATE. */
#define FOLEY_STEP_HIST 16
int foley_set_multistep(foley_ctx* ctx, int order, void* stream);

/* FlowEdit (additive within ABI 13; opt-in): inversion-free prompt editing of a source clip (Kulikov et al. 2024).  One edited clip
 * occupies TWO clips of the model batch - a source-branch clip under the source prompt and a target-branch clip under the target
 * prompt, sharing the visual features and the negative prompt - and the loop integrates the difference of their guided velocities
 * from the source latents, so what both prompts agree on (here: the timing, which comes from the video) cancels.  With V
 * variations the plan has clips = 2V, ordered [src_0 .. src_{V-1}, tar_0 .. tar_{V-1}], and ncfg = 2 (foley_prepare_sets with one
 * text set per branch); it is the plan of the SUFFIX [i0, n_iter) of an euler run with FOLEY_STEP_BLEND rows (sigma_{k+1} in
 * column 5), as for foley_set_edit.  The state is z [V, latent_dim, La], started at x_src.  Per iteration i, fp32, contraction off:
 *   v_s = fma(g_src, c_s - u_s, u_s);  v_t = fma(g_tar, c_t - u_t, u_t)      (the two-half combine of clips v and V + v)
 *   d = v_t - v_s;  d = m*d under a mask (m = mask[v][l], 1 = edit, 0 = keep);  z = fma(d, dt, z)
 * and the rows of the next model call from s = sigma_{k+1} and n = noise row min(i + 1, noise_rows - 1):
 *   z_src = fma(1 - s, x_src, rnd(s*n)) -> clip v;   z_tar = (z - x_src) + z_src -> clip V + v        (both cfg halves)
 * m == 0 keeps a frame at x_src bit for bit through the whole run, m == 1 gives the unmasked update bit for bit; equal prompts and
 * scales give the identity to rounding (the two clips pass the GEMMs at different rows).  Not built: the paper's n_min tail of
 * plain target sampling, n_avg > 1, frames past the end of the source.
 *   x_src [src_clips, latent_dim, La] fp32, src_clips 1 (shared) or V
 *   noise [noise_rows, V, latent_dim, La] fp32, noise_rows plan.n_iter (fresh noise: row i serves iteration i) or 1 (one fixed draw)
 *   mask  [mask_clips, La] fp32 in [0, 1] or NULL (all ones), mask_clips 1 or V
 *   g_src, g_tar  the CFG scales of the branches, finite and > 1 (plan.guidance is not read)
 *   sigma0        sigma_{k0} of the first iteration: foley_sample stages the first rows at it from noise row 0
 * All operands are on the DEVICE and are copied into context-owned, grow-only buffers (captured graphs never hold the caller's
 * pointers); the captured iteration is keyed on the FlowEdit operands, so a context alternates between plain and FlowEdit runs
 * safely and new values of the same shape only rewrite what a replay reads.  foley_prepare clears the state, as does a call with
 * x_src NULL.  Under the state foley_sample takes and returns z [V, latent_dim, La].
 * plan.ncfg != 2, odd plan.clips, noise_rows not in {1, plan.n_iter}, clip counts other than 1 / V, a scale <= 1 or not finite,
 * sigma0 outside [0, 1], a solver_coef row without FOLEY_STEP_BLEND (a multi-stage table), or an edit, windows, multistep,
 * projected-guidance, guidance-schedule / rescale, step-cache or timeline state on the context: FOLEY_ERR_INVALID - those setters
 * refuse a FlowEdit state in turn.  Before foley_prepare: FOLEY_ERR_STATE. */
int foley_set_flowedit(foley_ctx* ctx, const float* x_src, int src_clips, const float* noise, int noise_rows, const float* mask,
                       int mask_clips, float g_src, float g_tar, float sigma0, void* stream);

/* DAC-VAE decoder: latents [clips, latent_dim, T] fp32 -> waveform [clips, 1, T*hop] fp32. */
int foley_dac_decode(foley_ctx* ctx, const float* latents, int clips, int T, float* wave, void* stream);

/* DAC-VAE encoder (DAC.encode with continuous=True, dac.py:236-278 + Encoder :47-95):
 * waveform [clips, 1, T] fp32, T a multiple of the hop (DAC.preprocess right-pads, :225-234) ->
 * posterior parameters [clips, 2*latent_dim, T/hop] fp32 (rows [:latent] mean, [latent:] logvar of the
 * DiagonalGaussianDistribution, nn/vae_utils.py:24-31).  enc_dim / rates: encoder_dim and
 * encoder_rates of the checkpoint (128, {2,3,4,5,8} for the 48 kHz VAE, utils.py:32-44); needs the
 * packed `enc.*` tensors registered. */
int foley_dac_encode(foley_ctx* ctx, const float* wave, int clips, int T, int enc_dim, const int32_t* rates,
                     int n_rates, float* params, void* stream);

/* Per-kernel profile of the DiT forward (bench.py's live roofline): runs `repeats` EAGER forwards at loop
 * iteration `iter`, every op's kernel launched with start / stop events attached to the dispatch itself
 * (hipExtLaunchKernelGGL on `stream`), and aggregates by op.  `calls`, `total_ms` (kernel time proper),
 * `flop` (algorithmic FLOPs: 2*M*N*K per contraction, 4*B*H*Sq*Skv*128 per attention) and `bytes`
 * (operands + result, read/written once) are totals over all repeats.  *bracket_ms = elapsed time of
 * an empty hipEventRecord bracket, for reference (not contained in total_ms).  Replaces nothing in
 * the reference: it is the measurement hook SURVEY 8(d) asks for. */
typedef struct foley_prof_entry {
  char label[80];
  int32_t calls;
  float total_ms;
  double flop, bytes;
  char kernel[200];   /* ABI 12: demangled symbol of the kernel the op launched - the row name in a rocprofv3 kernel trace ("" if none) */
} foley_prof_entry;
int foley_profile_forward(foley_ctx* ctx, const float* latents, int iter, int repeats, foley_prof_entry* out,
                          int cap, int* n_out, float* bracket_ms, void* stream);

/* HIP-event time (ms) of the last foley_sample / foley_dac_decode / foley_dac_encode call on this context (syncs). */
int foley_last_elapsed_ms(foley_ctx* ctx, float* ms);

/* ------------------------------------------------------------------ op-level entry points */
typedef struct foley_rowbcast {  /* row-broadcast operand (AdaLN shift/scale/gate, addend) */
  const float* p;       /* null => absent */
  int64_t ld;
  int32_t mode;         /* 0: one vector for all rows; 1: rows [cfg][clip][l] use operand row [cfg][l];
                         * 2: the operand has Ls rows per cfg and token l uses row min(floor((l+0.5)*Ls/L), Ls-1),
                         *    float32 as F.interpolate(mode="nearest-exact") computes it (hifi_foley.py:759-762) */
  int32_t rows_per_cfg, L;
  int32_t Ls;           /* mode 2 only */
  int32_t period;       /* mode 2 only: 0, or a power of two - the up-sampled sequence repeats with this period and the
                         * operand stores only `period` rows per cfg (row (nearest_exact(l) mod period)) */
  int32_t periodic_cfgs; /* mode 2 with period > 0: 0 = every cfg half is stored periodically; k > 0 = only the first k halves
                         * (`period` rows each), the others follow with all their Ls rows (ABI 11; fills the struct's padding) */
} foley_rowbcast;

/* Head split applied to a fused q/k/v (or cross-attention q) projection: per (row, head) RMSNorm
 * (norm_layers.py:36-52), interleaved RoPE (attn_layers.py:112-146) and the [clip, H, S_tot, 128]
 * layout of the attention operands; replaces `rearrange` + q_norm/k_norm + apply_rotary_emb of
 * hifi_foley.py:226-262 / 376-382.  Used by foley_gemm_desc.qkv (epilogue 7). */
typedef struct foley_qkv_split_desc {
  int32_t L, H, nK;              /* rows are [clip][l] with L tokens per clip; nK operands of H heads */
  const float* gain[3];          /* RMSNorm gain [128] per operand, null => copy only */
  const int32_t* pos[3];         /* RoPE position per token l, null => no rotation */
  void* dst[3];                  /* [clips, H, S_tot, 128] in out_dtype; see vt_pitch for the last one */
  int32_t out_dtype, vt_pitch;   /* vt_pitch > 0: last operand stored transposed [clips, H, 128, vt_pitch] */
  int32_t S_tot, tok_off;
  float eps;
  const float* cos_tab; const float* sin_tab;   /* [P, 64] */
  /* Optional (nK = 1, 16-bit operands): attention of the projected q rows against <= 96 cached keys in the same epilogue
   * (TwoStreamCABlock cross attention to the text, hifi_foley.py:271-319): attn_out [M, H*128] receives
   * softmax(q k^T / sqrt(128)) v per head, rows ordered like the GEMM's.  Keys attn_k [sets, H, attn_skv, 128], values
   * TRANSPOSED attn_vt [sets, H, 128, attn_pitch] (attn_pitch >= 96, finite beyond attn_skv), both in the operand dtype;
   * the set of row r is (r / L) / attn_bdiv.  The library takes the fused form on small grids only (its 64-row head-split
   * tile) and says so in *attn_fused (may be null): 1 = attn_out written, dst[0] untouched; 0 = plain head split into
   * dst[0], the caller runs foley_op_attention itself. */
  const void* attn_k; const void* attn_vt; void* attn_out;
  int32_t attn_skv, attn_pitch, attn_bdiv;
  int32_t* attn_fused;
} foley_qkv_split_desc;

typedef struct foley_gemm_desc {
  const void* A; const void* W; const float* bias;
  int32_t M, N, K; int64_t lda;
  int32_t segV, segS, taps, tapC, dil, tap0;      /* conv-as-GEMM addressing */
  void* out0; void* out1;
  int32_t osegV; int64_t out_seg, out_row, out_shift; int32_t out_check;
  foley_rowbcast rb; const float* res; const float* alpha; int32_t alphaC;
  int32_t dtype;   /* operand dtype */
  int32_t epilogue;/* 0 store f32, 1 store T, 2 silu T, 3 gelu-tanh T, 4 silu-gate T, 5 gated residual, 6 DAC, 7 head split */
  int32_t tile;    /* 0 auto */
  int32_t ksplit;  /* gated-residual epilogue: K ranges (0 auto, 1 deterministic); ranges are combined with
                    * fp32 atomics, or - when `partials` is set - deferred to the next LayerNorm */
  /* Deferred split-K: K range s stores its raw product to partials[s][M][N] (fp32, 16-byte aligned,
   * room for partial_slabs ranges; caps ksplit) and out0 is NOT touched; the caller then runs
   * foley_op_ln_mod_pending(out0, ..., partials, *ksplit_used, bias, gate), which performs
   * x += gate * (sum_s partials[s] + bias) before normalising.  With *ksplit_used == 1 the GEMM
   * has already updated out0 and nothing is pending. */
  float* partials; int32_t partial_slabs; int32_t* ksplit_used;
  /* epilogue 7 (fused head split): N = nK*H*128, out0 unused, results go to qkv->dst[] */
  const foley_qkv_split_desc* qkv;
  int32_t rstride; /* source rows advanced per virtual row (strided conv, dac.py:55-61); 0 or 1 = dense */
  int64_t ldw;     /* elements between rows of W (0 = K); > K for row-padded weight storage (wave-specialised tiles) */
  int32_t wfmt;    /* storage of W: 0 = `dtype`; 1 = fp8 e4m3fn, 2 = fp8 e5m2 with bf16 activations - widened to bf16
                    * in registers by the wave-specialised tiles (15, 19), bit-identical to widening at load time */
  int32_t partial_dtype; /* dtype of the `partials` slabs: 0 = fp32; or the (16-bit) operand dtype - half the slab traffic, the
                          * sum of k rounded partials carries about the error of one rounding of the total; pass the same
                          * value to foley_op_ln_mod_pending2 */
  int32_t gelu_erf;/* epilogue 3 only: 1 = exact GELU (erf) instead of the tanh form - nn.GELU() of the conditioning
                    * encoders (reference models/synchformer/vit_helper.py:108-125 Mlp, nn.TransformerEncoderLayer) */
} foley_gemm_desc;

int foley_op_gemm(const foley_gemm_desc* d, void* stream);
/* in_dtype f32: q,k,v [B,H,S,128] fp32 (exact fp32 MFMA).  in_dtype bf16: q,k bf16 [B,H,S,128] and v
 * TRANSPOSED bf16 [B,H,128,vt_pitch], vt_pitch >= Skv rounded up to 32 with a finite pad. */
int foley_op_attention(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq, int H,
                       int Sq, int Skv, int kv_bdiv, void* outA, void* outB, int split, int out_dtype,
                       void* stream);
/* The timeline cross-attention at op level (head_dim 128, every operand on the device): q [Bq,H,Sq,128]; k [n_sets,H,Skv,128];
 * v [n_sets,H,Skv,128] (fp32 operands) or TRANSPOSED [n_sets,H,128,vt_pitch] (bf16 / fp16: Skv <= 96, vt_pitch as above); set_a,
 * set_b int32 and alpha fp32 [Bq,Sq].  Set indices are clamped to [0, n_sets) by the kernels before they address anything. */
int foley_op_attention_timeline(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq, int H, int Sq,
                                int Skv, int n_sets, const int32_t* set_a, const int32_t* set_b, const float* alpha, void* outA,
                                void* outB, int split, int out_dtype, void* stream);
/* the same with head_dim 128, 64 (the ViT-B conditioning encoders, feature_utils.py:63-108) or 96 (the Synchformer sync head,
 * models/synchformer/synchformer.py:115-187: 8 heads x 96, scale 1/sqrt(96)): fp32 operands, or 16-bit operands through the
 * LDS-staged 128-query kernel (v transposed [B,H,head_dim,vt_pitch]) */
int foley_op_attention_hd(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq, int H,
                          int Sq, int Skv, int kv_bdiv, void* outA, void* outB, int split, int out_dtype,
                          int head_dim, void* stream);
/* foley_op_attention_hd at head_dim 64 with scattered output rows: query t of group g lands in row out_rows[g*Sq + t] of out
 * [rows, H*64] - normally the table the queries were gathered by (foley_op_qkv_regroup's idx_q), so that the CLS attention and the
 * time / space group attention of a DividedAttention layer (vit_helper.py:37-105: `torch.cat((cls_out, x), dim=1)` after the inverse
 * rearrange) write ONE token-major buffer, ready for the output projection.
 * grp_q / grp_kv > 0 (16-bit operands): block-diagonal attention - the sequence is a pack of small groups, query t attends keys
 * [g*grp_kv, (g+1)*grp_kv) with g = t / grp_q only (DividedAttention over time: 8 frame queries x (CLS + 8 frame keys) per location;
 * 14 locations share one 128-query workgroup instead of taking one each); 0 / 0: every query sees all Skv keys.
 * out has out_nrows rows: a table entry outside [0, out_nrows) drops that query's output instead of writing out of bounds. */
int foley_op_attention_scatter(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int G, int H, int Sq,
                               int Skv, int grp_q, int grp_kv, const int32_t* out_rows, void* out, int out_nrows, int out_dtype, void* stream);
/* Token regrouping between a fused q/k/v projection and foley_op_attention_hd at head_dim 64 - the conditioning encoders
 * (reference models/synchformer/vit_helper.py:37-105 DividedAttention: patch tokens attend over the frames of their location or
 * the locations of their frame with the CLS key / value prepended; transformers' SiglipAttention / ClapTextSelfAttention head split):
 * qkv [rows, 3*H*64] in nn.Linear(dim, 3*dim)'s (K H D) packing; group g reads source rows idx_q[g*Sq + t] as its queries and
 * idx_kv[g*Skv + t] as its keys / values and writes q [G,H,Sq,64], k [G,H,Skv,64] and v [G,H,Skv,64] (vt_pitch 0) or - 16-bit
 * operands - v TRANSPOSED [G,H,64,vt_pitch] with zeros beyond Skv (vt_pitch a multiple of 8 in [Skv, ceil64(Skv)]).
 * qkv has n_rows rows: table entries are clamped to [0, n_rows) on the device, so a bad table cannot read out of bounds. */
int foley_op_qkv_regroup(const void* qkv, int n_rows, int dtype, int H, const int32_t* idx_q, int G, int Sq, const int32_t* idx_kv, int Skv,
                         void* q, void* k, void* v, int vt_pitch, void* stream);
/* One pass of the frames' antialiased bicubic uint8 resize - replaces torchvision's v2.Resize(interpolation=BICUBIC, antialias=True)
 * on uint8 tensors in the nodes' pre-processing (reference nodes.py:184-196, utils.py:262-283; on the CPU that dispatches to ATen's
 * native separable uint8 kernel: horizontal pass, uint8 intermediate, vertical pass).  in [outer, len_in, inner] -> out [outer,
 * len_out, inner] along the middle axis: out = sat8((2^(precision-1) + sum_{j < xsize[x]} in[xmin[x] + j] * weights[x*kmax + j])
 * >> precision).  inner = 1: horizontal pass over rows; inner = W: vertical pass.  Tables (device memory, one row per output
 * sample; host/encoders.py::aa_tables builds them as ATen does - double-precision cubic (a = -0.5) taps over a support of
 * 2*max(scale, 1), normalised, rounded half away from zero at the largest precision whose biggest weight fits int16). */
int foley_op_resize_aa_u8(const uint8_t* in, long outer, int len_in, long inner, int len_out, const int32_t* xmin,
                          const int32_t* xsize, const int16_t* weights, int kmax, int precision, uint8_t* out, void* stream);
/* Rational polyphase windowed-sinc resampling (torchaudio.functional.resample with orig / new reduced by their gcd): x [B, N]
 * fp32 -> out [B, Nout] fp32, out[b, j*new_rate + p] = sum_{t < ntaps} x[b, j*orig + t - width] * taps[p*ntaps + t] (x is zero
 * outside [0, N)), Nout = ceil(N * new_rate / orig) for torchaudio's length (a larger Nout is FOLEY_ERR_INVALID).  taps [new_rate, ntaps] fp32 on the device, built by
 * the caller (host/sync_score.py::sinc_resample_taps: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; 48 kHz -> 16 kHz is
 * orig 3, new_rate 1, width 19, 41 taps).  Used by the sync scorer ahead of foley_op_logmel. */
int foley_op_resample_sinc(const float* x, int B, int N, int orig, int new_rate, const float* taps, int ntaps, int width,
                           float* out, int Nout, void* stream);
/* The fused log-mel front end of the Synchformer audio branch (encode_audio_with_sync, models/synchformer/synchformer.py:294-317):
 * w16 [B, N16] fp32 at 16 kHz -> S = (N16 - 10240) / 5120 + 1 segments per clip, each torch.stft(n_fft 1024, hop 160, win 400
 * periodic Hann, center, reflect) -> |X|^2 -> 128 HTK mel triangles (torchaudio MelSpectrogram defaults, norm None) -> log(x + 1e-6)
 * -> time axis padded 65 -> 66 with 0 -> (x + 4.2677393) / (2 * 4.5689974), written as the im2col matrix of the AST patch
 * embedding: patches [B*S*72, 256] in out_dtype (f32 / bf16 / f16), row (b*S + s)*72 + fi*6 + ti, column kf*16 + kt = spectrogram
 * (mel 10*fi + kf, frame 10*ti + kt) - one GEMM with the Conv2d(1, 768, 16, stride 10) weight [768, 256] is the patch embedding.
 * Tables (device, fp32 / int32, built by host/sync_score.py): basis [2][400][544] = Hann(m) * cos / sin(2 pi k (m + 312) / 1024),
 * bins k >= 513 zero; mel c = sum_{k < mel_len[c]} |X|^2[mel_lo[c] + k] * mel_w[c*mel_wp + k].  mel_out (nullable): the
 * normalised spectrogram [B*S, 128, 66] fp32 as well (its rows 126 and 127 reach no patch). */
int foley_op_logmel(const float* w16, int B, int N16, const float* basis, const int32_t* mel_lo, const int32_t* mel_len,
                    const float* mel_w, int mel_wp, void* patches, int out_dtype, float* mel_out, void* stream);
int foley_op_ln_mod(const float* x, int M, int D, float eps, const foley_rowbcast* shift,
                    const foley_rowbcast* scale, void* out, int out_dtype, void* stream);
/* LayerNorm (+ modulation) of a residual stream that first receives the pending update of a deferred
 * split-K gated-residual GEMM (see foley_gemm_desc.partials); x is updated in place. */
int foley_op_ln_mod_pending(float* x, int M, int D, float eps, const foley_rowbcast* shift,
                            const foley_rowbcast* scale, void* out, int out_dtype, const float* partials,
                            int k, const float* bias, const foley_rowbcast* gate, void* stream);
/* vt_pitch > 0: the last operand is written transposed [clips, H, 128, vt_pitch] (see above). */
/* the same with slabs of `partial_dtype` (0 = fp32, or out_dtype when that is bf16 / fp16: foley_gemm_desc.partial_dtype) */
int foley_op_ln_mod_pending2(float* x, int M, int D, float eps, const foley_rowbcast* shift,
                             const foley_rowbcast* scale, void* out, int out_dtype, const void* partials,
                             int partial_dtype, int k, const float* bias, const foley_rowbcast* gate, void* stream);
int foley_op_qkv_split(const float* qkv, int M, int L, int H, int nK, const float* const* gain,
                       const int32_t* const* pos, void* const* dst, int out_dtype, int vt_pitch, int S_tot,
                       int tok_off, float eps, const float* cos_tab, const float* sin_tab, void* stream);
/* Guidance descriptor (see foley_set_guidance), on the DEVICE: sched [n_iter, 2] read at row *step_ptr (NULL: the scalar
 * `guidance`), clip_scale [clips] multiplied into the guided value (NULL: none). */
typedef struct foley_guidance_desc {
  const float* sched;
  float* clip_scale;
} foley_guidance_desc;
/* One solver step (CFG combine + scheduler update + staging of the next model input rows), every operand on the DEVICE; an absent
 * operand is NULL / 0.  pred [ncfg*clips*L, C], x / x_saved / d_acc [clips, C, L] (x_saved / d_acc NULL for single-stage tables),
 * coef [n_iter, 8] read at row *step_ptr, which a one-thread launch then advances; rows_out NULL: no rows staged, else ncfg copies.
 * gd: both NULL, or ncfg 2 with a table whose rows all hold `guidance` and no factors, give the same bits; ncfg 3 takes the
 *   three-term combine.
 * hist [hist_slots, clips, C, L] fp32 (see foley_set_multistep): rows flagged FOLEY_STEP_HIST add coef column 6 times slot
 *   (*step_ptr - 1) mod hist_slots and column 7 times slot (*step_ptr - 2) mod hist_slots (a zero weight reads nothing); every row
 *   stores its guided velocity to slot *step_ptr mod hist_slots.  NULL with 0 slots: the kernels without history; a ring needs 1
 *   or 2 slots and slots need a ring, anything else is FOLEY_ERR_INVALID.
 * x0 != NULL selects the edit form (see foley_set_edit): the same update, then the blend after FOLEY_STEP_BLEND rows; x0
 *   [x0_clips, C, L], noise [clips, C, L], mask [mask_clips, L] or NULL (all ones); x0_clips / mask_clips 1 or clips.
 * n_win != 0 selects the windows form (see foley_set_windows): clips = variations*n_win; starts [n_win] int32 and weights
 *   [n_win, L] fp32; Ltot = starts[n_win - 1] + L.  Both forms at once: refused. */
typedef struct foley_step_desc {
  const float* pred;
  float* x;
  float* x_saved;
  float* d_acc;
  int32_t clips, C, L, ncfg;
  float guidance;
  int32_t rows_dtype;
  const float* coef;
  int32_t* step_ptr;
  void* rows_out;
  foley_guidance_desc gd;
  float* hist;
  int32_t hist_slots;
  int32_t x0_clips;
  const float* x0;
  const float* noise;
  const float* mask;
  int32_t mask_clips;
  int32_t n_win;
  const int32_t* starts;
  const float* weights;
  int32_t Ltot;
} foley_step_desc;
#if defined(__cplusplus) && defined(__LP64__)
static_assert(sizeof(foley_step_desc) == 168, "foley_step_desc: LP64 layout (the bindings mirror it field by field)");
#endif
int foley_op_solver_step(const foley_step_desc* d, void* stream);
/* The rescale factors of one iteration: gd->clip_scale[b] = rescale * s_pos / s_cfg + (1 - rescale) from pred [ncfg*clips*L, C]
 * at iteration *step_ptr (gd->sched as above), C <= 256.  `work`: device scratch of at least foley_op_guidance_stats_work(clips, L)
 * floats.  Two launches, bit-identical on repetition. */
int64_t foley_op_guidance_stats_work(int clips, int L);
int foley_op_guidance_stats(const foley_guidance_desc* gd, const float* pred, int clips, int C, int L, int ncfg, float guidance,
                            const int32_t* step_ptr, float rescale, float* work, int64_t work_floats, void* stream);
/* Projected guidance at op level (see foley_set_projected_guidance), every operand on the DEVICE: rows [n_iter, 4] {eta, beta, R,
 * live} read at row *step_ptr, coef [clips, 2] {a_c, a_w}, plane [clips*L, C] fp32 (APG; NULL for CFG-Zero*), mode
 * FOLEY_GUIDANCE_APG or FOLEY_GUIDANCE_ZERO_STAR.
 * guidance_project: the two launches of one iteration - the inner products of pred [2*clips*La, C] (C <= 256), APG's plane update,
 *   then proj->coef from them, g (gd->sched column 0 at row *step_ptr when gd and its table are given, else `guidance`) and the
 *   row.  `work`: scratch of at least foley_op_guidance_project_work(clips, La) floats.  Bit-identical on repetition (APG with
 *   beta != 0: from the same plane).
 * solver_step_projected: foley_op_solver_step with v = fma(a_c, c, rnd(a_w w)) from proj->coef, w = proj->plane (APG) or u: every
 *   form and the history ring as there; ncfg must be 2 and d->gd.clip_scale NULL.  proj NULL: foley_op_solver_step bit for bit. */
typedef struct foley_projection_desc {
  const float* rows;
  float* coef;
  float* plane;
  int32_t mode;
} foley_projection_desc;
int64_t foley_op_guidance_project_work(int clips, int La);
int foley_op_guidance_project(const foley_projection_desc* proj, const foley_guidance_desc* gd, const float* pred, int clips, int C,
                              int La, float guidance, const int32_t* step_ptr, float* work, int64_t work_floats, void* stream);
int foley_op_solver_step_projected(const foley_step_desc* d, const foley_projection_desc* proj, void* stream);
/* FlowEdit at op level (see foley_set_flowedit), every operand on the DEVICE: pred [2*2V*L, C] (halves [uncond ; cond] of the clips
 * [src_0 .. src_{V-1}, tar_0 .. tar_{V-1}]), z [V, C, L] updated in place, x_src [src_clips, C, L], noise [noise_rows, V, C, L]
 * (noise_rows 1 or n_iter), mask [mask_clips, L] or NULL, coef [n_iter, 8] read at row *step_ptr, rows_out [2*2V*L, C] in rows_dtype
 * (NULL: nothing staged).
 * flowedit_step: one iteration - the update of z, then the rows of the next model call from coef column 5 and noise row
 *   min(*step_ptr + 1, noise_rows - 1); a one-thread launch then advances *step_ptr.  The coefficient rows are read back and
 *   checked (every row carries FOLEY_STEP_BLEND), which synchronises the stream: an op for tests and tools, not for a hot loop.
 * flowedit_stage: the staging alone, at `sigma` in [0, 1] from noise row `noise_row`: rows_out from z, x_src and the noise (pred,
 *   coef and step_ptr are not read).  sigma 0 stages x_src and z themselves. */
typedef struct foley_flowedit_desc {
  const float* pred;
  float* z;
  const float* x_src;
  const float* noise;
  const float* mask;
  const float* coef;
  int32_t* step_ptr;
  void* rows_out;
  int32_t V, C, L, n_iter, rows_dtype;
  int32_t src_clips, noise_rows, mask_clips;
  float g_src, g_tar;
} foley_flowedit_desc;
#if defined(__cplusplus) && defined(__LP64__)
static_assert(sizeof(foley_flowedit_desc) == 104, "foley_flowedit_desc: LP64 layout (the bindings mirror it field by field)");
#endif
int foley_op_flowedit_step(const foley_flowedit_desc* d, void* stream);
int foley_op_flowedit_stage(const foley_flowedit_desc* d, float sigma, int noise_row, void* stream);
/* The step cache's kernels (see foley_set_step_cache), all operands on the DEVICE, fp32, 16-byte aligned for the probe.
 * cache_probe: a0 [Bc*La, D] (D a multiple of 4 up to 2048) -> m = LayerNorm(a0; eps) * (1 + scale) + shift written over m_prev
 *   [Bc*La, D], rel[b] = sum|m - m_prev| / sum|m_prev| of batch row b (0 when the denominator is 0).
 *   `work`: scratch of at least foley_op_cache_probe_work(Bc, La) floats.  Two launches, bit-identical on repetition.
 * cache_delta: delta[i] = aN[i] - delta[i] for i < n (in place over a copy of a0).  cache_apply: audio[i] += delta[i]. */
int64_t foley_op_cache_probe_work(int Bc, int La);
int foley_op_cache_probe(const float* a0, int Bc, int La, int D, float eps, const foley_rowbcast* shift,
                         const foley_rowbcast* scale, float* m_prev, float* work, int64_t work_floats, float* rel,
                         void* stream);
int foley_op_cache_delta(const float* aN, float* delta, int64_t n, void* stream);
int foley_op_cache_apply(float* audio, const float* delta, int64_t n, void* stream);
/* x [variations*n_win, C, L] -> out [variations, C, Ltot]: the weighted mean above per global frame; where the covering windows
 * hold the identical bits (always after a blend row) that value is copied as it is.  starts / weights on the device. */
int foley_op_windows_stitch(const float* x, int clips, int n_win, int C, int L, int Ltot, const int32_t* starts,
                            const float* weights, float* out, void* stream);
/* Start state of an edit run: out [clips, C, L] = sigma*noise + (1 - sigma)*x0, x0 [x0_clips, C, L] with x0_clips 1 or clips. */
int foley_op_flow_mix(const float* noise, const float* x0, int x0_clips, int clips, int C, int L, float sigma,
                      float* out, void* stream);
int foley_op_latent_rows(const float* x, int clips, int C, int L, int ncfg, void* out, int out_dtype,
                         void* stream);
int foley_op_dac_out(const float* s, const float* w, const float* bias, int B, int T, int C, float* out,
                     void* stream);
/* The remaining row kernels of a run, one entry each (additive: the ABI number is unchanged).  All operands on the device.
 * rows_add_act: out(T) [R, D] = act(a + v), a [R, D] fp32 or NULL (zeros), v [D] fp32 or NULL, act_silu 0 / 1.
 * add_periodic: out(T) [R, D] = x [R, D] + pos [period, D] row r % period.
 * gather_rows: out [groups*n_idx, D] row (g, l) = src row g*src_rows + idx[l] (fp32).
 * cast: n contiguous elements, fp32 <-> bf16, fp32 <-> fp16 or fp32 -> fp32; any other pair is FOLEY_ERR_INVALID.
 * rows_periodic_check: flags[g] |= 1 when, in group g of x [groups, rows, D] (groups <= 32), some row s >= period differs from row
 *   s - period in its BIT PATTERN (+0 and -0 differ, equal NaN patterns agree); rows <= period launches nothing.
 * dac_in: DAC encoder input conv 1 -> C (k = 7, pad 3) over x [B, T]: out0 [B*T, C] = y, out1 = snake(y; alpha); C % 4 == 0.
 * rows_to_planes: rows [B*T, C] -> out [B, C, T]. */
int foley_op_rows_add_act(const float* a, const float* v, int R, int D, int act_silu, void* out, int out_dtype,
                          void* stream);
int foley_op_add_periodic(const float* x, const float* pos, int R, int D, int period, void* out, int out_dtype,
                          void* stream);
int foley_op_gather_rows(const float* src, const int32_t* idx, int n_idx, int groups, int src_rows, int D, float* out,
                         void* stream);
int foley_op_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
int foley_op_rows_periodic_check(const float* x, int groups, int rows, int period, int D, int32_t* flags, void* stream);
int foley_op_dac_in(const float* x, const float* w, const float* bias, const float* alpha, int B, int T, int C,
                    float* out0, float* out1, void* stream);
int foley_op_rows_to_planes(const float* rows, int B, int T, int C, float* out, void* stream);
/* The CLAP audio tower's own kernels (host/clap_score.py; additive: the ABI number is unchanged).  All operands on the device.
 * melspec_db: transformers' ClapFeatureExtractor (rand_trunc / repeatpad) for 48 kHz audio.  x [B, N >= 1024] fp32; window k of
 *   every clip is the 480000 padded samples p -> x[starts[k] + p % seg] for p < (480000 / seg) * seg, 0 beyond, seg = min(N,
 *   480000) (N < 480000: the extractor's repeatpad and n_win must be 1; otherwise a crop at starts[k], clamped into the clip).
 *   Each window: STFT (n_fft 1024, periodic Hann 1024, hop 480, centred, reflect) -> |X|^2 -> 64 mel triangles -> 10 log10(max(mel,
 *   1e-10)) (a value at the floor is exactly -100): out [B * n_win, 1001, 64] fp32, window-minor.  Tables (host/clap_score.py):
 *   basis [2][1024][544] fp32 = Hann(m) * cos / -sin(2 pi k m / 1024), bins k >= 513 zero; mel c = sum_{k < mel_len[c]}
 *   |X|^2[mel_lo[c] + k] * mel_w[c * mel_wp + k] (int32 [64], fp32 [64, mel_wp]).
 * spec_patches: spec [G, T, F] fp32 -> the im2col matrix of the 4x4 / stride 4 patch embedding over reshape_mel2img's image:
 *   v[to, f] = sum_{j < 4} resize_w[to, j] * (spec[resize_idx[to, j], f] * scale[f] + shift[f]) for to < ratio * Tq (BatchNorm2d
 *   in eval mode folded to one affine per bin, then the bicubic resize along time; both tables NULL: no resize, T = ratio * Tq),
 *   img[r * F + f, t] = v[r * Tq + t, f], out [G * (ratio F / 4) * (Tq / 4), Kp] in out_dtype (f32 / bf16 / f16): row
 *   (g, h, w) column kh * 4 + kw = img[4 h + kh, 4 w + kw], columns [16, Kp) zero.  F a multiple of 4 up to 256, Tq of 4, Kp >= 16.
 * window_attention: Swin's windowed attention for 64-token windows at head dim 32, anything else is FOLEY_ERR_INVALID.  qkv
 *   [rows, qkv_cols = 3 * H * 32] (f32 / bf16 / f16; q | k | v, head-major), table [n_win, 64] int32 = the source row of every
 *   window token (roll, then partition), bias [H, 64, 64] fp32 (query-major), mask [n_mask, 64, 64] fp32 or NULL, window g reads
 *   mask g % n_mask.  scores = q . k / sqrt(32) + bias + mask in fp32 (a mask value is added as a number: masked keys are not
 *   skipped), softmax over the 64 keys, times v; query t of window g goes to out row table[g, t] (out [rows, out_pitch] in qkv's
 *   dtype, columns h * 32 .. of each head; out_pitch >= H * 32, a multiple of 8).  No atomics, one fixed summation order. */
int foley_op_melspec_db(const float* x, int B, int N, const int32_t* starts, int n_win, const float* basis, const int32_t* mel_lo,
                        const int32_t* mel_len, const float* mel_w, int mel_wp, float* out, void* stream);
int foley_op_spec_patches(const float* spec, int G, int T, int F, const float* scale, const float* shift, const int32_t* resize_idx,
                          const float* resize_w, int Tq, int ratio, void* out, int out_dtype, int Kp, void* stream);
int foley_op_window_attention(const void* qkv, int dtype, int rows, int qkv_cols, int H, int win_tokens, const int32_t* table,
                              int n_win, const float* bias, const float* mask, int n_mask, void* out, int out_pitch, void* stream);
/* The loudness and true-peak output stage (host/loudness.py; additive: the ABI number is unchanged).  Waveforms x [B, C, N] fp32
 * at 48 kHz on the device, C 1 or 2, row (b, c) at x + (b*C + c)*ld with ld >= N; anything else is FOLEY_ERR_INVALID.  T16 and
 * taps36 are read on the HOST at the call.  No floating-point atomics: every entry gives the same bits on repetition.
 * loudness_energy: the K-weighting of ITU-R BS.1770-4 (two biquads, fp64 state, zero initial state) and e [B, C, nh] fp64, the sum
 *   of y^2 over every complete hop of 4800 samples, nh = N / 4800 (nh = 0 launches nothing).  Chunks of 480 samples run in
 *   parallel: from zero state, then a carry pass s_{k+1} = T s_k + end_k per row (T16: the chunk's 4x4 transition matrix,
 *   row-major fp64, over the transposed-direct-form-II state (s1, s2 of stage 1, s1, s2 of stage 2)), then from the true state.
 *   `work`: device scratch of at least B * C * nh * 40 doubles.  Three launches.
 * loudness_gate: e -> blocks of four hops (400 ms, 75 % overlap), z_j = sum_c sum e / 19200, l_j = -0.691 + 10 log10 z_j ->
 *   block_lufs [B, nh - 3] fp64; gamma [B] = the relative gate (-0.691 + 10 log10 mean z over l_j > -70, minus 10); lufs [B] = the
 *   integrated loudness over the blocks above both gates; -inf where no block passes (gamma too) or nh < 4.  One wave per clip.
 * true_peak: p[n] = max_c max(|x[n]|, |u[4n + r]|, r = 1..3), u[4n + r] = sum_{j = -5..6} x[n + j] * taps36[(r - 1)*12 + j + 5] in
 *   fp32 (x zero outside [0, N)); true_peak [B] = max_n p[n] (linear), sample_peak [B] (nullable) = max |x|, envelope [B, N]
 *   (nullable) = p.
 * loudness_apply: limiter 0: y = gain[b] * x, one fp32 multiply per sample.  limiter 1: r[n] = min(1, ceiling / (gain[b] p[n]))
 *   (fp64, rounded down to fp32; 1 outside [0, N)), gmin[m] = min r[m .. m + lookahead], g[n] = min(r[n], (sum_{m = n -
 *   lookahead .. n} gmin[m]) / (lookahead + 1)) in fp32 in that order, y = (gain[b] * g[n]) * x for every channel, g_out [B, N]
 *   (nullable, limiter 1 only) = g; ceiling linear and positive, 1 <= lookahead <= 480 samples.  gain[b] == 0 copies clip b
 *   unchanged.  y [B, C, N] with row pitch ldy >= N, not overlapping x. */
int foley_op_loudness_energy(const float* x, int B, int C, int N, int64_t ld, const double* T16, double* work,
                             int64_t work_doubles, double* e, void* stream);
int foley_op_loudness_gate(const double* e, int B, int C, int nh, double* lufs, double* gamma, double* block_lufs, void* stream);
int foley_op_true_peak(const float* x, int B, int C, int N, int64_t ld, const float* taps36, float* true_peak,
                       float* sample_peak, float* envelope, void* stream);
int foley_op_loudness_apply(const float* x, int B, int C, int N, int64_t ld, const float* gain, int limiter, double ceiling,
                            int lookahead, const float* taps36, float* y, int64_t ldy, float* g_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FOLEY_HIP_H */
