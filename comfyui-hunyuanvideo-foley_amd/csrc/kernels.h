// Internal launch interface between the kernel files and the runtime (not part of the C ABI).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// GEMM / conv-as-GEMM engine:  D[r, n] = sum_k A'[r, k] * W[n, k]  (+ fused epilogue)
//
// A' is a *virtual* row matrix over a channels-last activation [rows, C]: virtual row r belongs to
// segment b = r / segV at position q = r % segV, and its K axis is `taps` blocks of `tapC`
// channels, block j being source row (q + tap0 + j*dil) of segment b (zero when that row falls
// outside [0, segS)).  taps=1 is a plain linear layer; taps=3,dil=1,tap0=-1 is the DiT's
// channels-last conv k=3 pad=1; taps=7 is the DAC dilated conv; taps=2,tap0=-1 over segV=T+1
// virtual rows is a stride-s transposed conv whose s output phases are the N axis.
// ---------------------------------------------------------------------------------------------
enum GemmEpi {
  EPI_STORE_F32 = 0,  // out0(f32) = acc + bias (+ rb addend)
  EPI_STORE_T = 1,    // out0(T)   = acc + bias
  EPI_SILU_T = 2,     // out0(T)   = silu(acc + bias)
  EPI_GELU_T = 3,     // out0(T)   = gelu_tanh(acc + bias)
  EPI_SILUGATE_T = 4, // out0(T)[.., N/2] = silu(a) * b, (a, b) = alternating 32-column groups
  EPI_GATE_RES = 5,   // out0(f32) += rb gate * (acc + bias)
  EPI_DAC = 6,        // v = acc + bias (+ res); out0(f32) = v; out1(f32) = snake(v)
  EPI_QKV_SPLIT = 7,  // fused head split: per 128-column head tile RMSNorm + RoPE (q, k) or V^T, written
                      // straight to the attention operands (GemmArgs::qs); needs a 128-wide tile
  EPI_QKV_ATTN = 8,   // internal (chosen by the launcher for EPI_QKV_SPLIT problems with qs.attn_out): head split of a q
                      // projection + attention against the cached keys in the same epilogue
  EPI_COUNT
};

struct QkvSplitArgs {
  const float* qkv;  // [M, nK * H * 128]
  int M, L, H, nK;   // rows ordered [clip][l], L tokens per clip
  const float* gain[3];  // RMSNorm gain per operand, null => copy only
  const int* pos[3];     // RoPE position per token l, null => no rotation
  void* dst[3];          // [clips, H, S_tot, 128] (out_dtype); see vt_pitch for the last operand
  int S_tot, tok_off;
  int out_dtype;         // FOLEY_F32 or FOLEY_BF16
  int vt_pitch;          // > 0: the LAST operand (V) is stored transposed [clips, H, 128, vt_pitch]
  float eps;
  const float* cos_tab;  // [P, 64]
  const float* sin_tab;
  // optional, fused GEMM epilogue only: rotation rows already gathered per token, rcos[o][l] = cos_tab[pos[o][l]]
  // ([L, 64] fp32 each) - one load level instead of two dependent ones in front of the stores
  const float* rcos[3];
  const float* rsin[3];
  // optional, fused GEMM epilogue only (nK = 1, 16-bit operands, 64-row tiles: the cross-attention q projection): run the
  // attention against <= 96 cached keys inside the epilogue and write its output rows instead of q.
  const void* attn_k;    // [sets, H, attn_skv, 128] operand type
  const void* attn_vt;   // [sets, H, 128, attn_pitch] operand type, finite beyond attn_skv
  void* attn_out;        // [M, H * 128] operand type; null => plain head split
  int attn_skv, attn_pitch;
  int attn_bdiv;         // text set of row r: (r / L) / attn_bdiv
  int* attn_fused;       // HOST pointer (never read by the device), may be null: the launcher stores 1 when the fused form ran,
                         // 0 when the problem took the plain head split (q in dst[0]; the caller launches the attention)
};
struct GemmArgs {
  const void* A;
  const void* W;      // [N, K] row-major, K contiguous
  const float* bias;  // [N] or null
  int M, N, K;
  long lda;           // elements between source rows of A
  long ldw;           // elements between rows of W (>= K; set by the launcher to K when 0) - padded rows spread the
                      // 128-byte K-slice lines of consecutive rows over the L2 channels
  int segV, segS;     // virtual / source rows per segment
  int taps, tapC, dil, tap0;
  int rstride;        // source rows advanced per virtual row (strided conv: tap t of row q reads q*rstride + tap0 + t*dil); 0 = 1
  // output mapping: element (r, n) -> b*out_seg + q*out_row + n + out_shift with (b, q) taken
  // over osegV rows; skipped when out_check and the in-segment offset leaves [0, out_seg)
  void* out0;
  void* out1;
  int osegV;
  long out_seg, out_row, out_shift;
  int out_check;
  RowBcast rb;        // gate (EPI_GATE_RES) or addend (EPI_STORE_F32)
  const float* res;   // EPI_DAC residual (same mapping as out0) or null
  const float* alpha; // EPI_DAC snake alpha, indexed n % alphaC
  int alphaC;
  unsigned a_bytes, w_bytes;   // operand extents in bytes (buffer-resource range of the direct-to-LDS loop; set by the launcher)
  const void* zeros;  // >= 128 zero bytes in global memory (source of masked rows for the direct-to-LDS loop)
  int ksplit;         // EPI_GATE_RES only: K is cut into `ksplit` ranges whose partial products are
                      // accumulated with hardware fp32 atomics (0 = auto; 1 = deterministic)
  // Deferred split-K (EPI_GATE_RES, ksplit > 1): with `partials` set, K range s stores its raw partial
  // product to partials + s*partial_stride ([M, N] row-major fp32, vector stores) instead of using
  // atomics; the LayerNorm that consumes the residual stream next finishes
  // x += gate * (sum_s partial_s + bias) (LnPending).  partial_cap = slabs available (caps ksplit).
  float* partials;    // slab base (fp32 view; with partial_half the slabs hold the 16-bit OPERAND type, 2 bytes per element)
  int partial_half;   // 1: slabs are stored in the operand type T (bf16 / fp16) - half the slab bytes written here and read by
                      // the LayerNorm; the sum of k rounded partials carries about the error of ONE rounding of the total
  int wt_out;         // set by the launcher (GemmPlan::wt_out): the slabs are stored write-through (common.h GStore<ST_WT>).  It sits in
                      // what was padding next to partial_half: the argument block keeps its size and offsets, and the epilogue
                      // reads both words in one scalar load
  long partial_stride;
  int partial_cap;
  int n_groups;       // set by the launcher, large grids: > 0 = tile order [column-panel group][M tile][panel inside the group] with this many
                      // groups (the workgroups that run together then cover a near-square block of tiles); 0 = [panel][M tile]
  int k_rot;          // set by the launcher (small grids, plain layers): M tile tm of a weight panel starts its K walk at slice tm * nk / tiles_m
                      // and wraps - the M tiles of a panel (neighbours on one XCD) then reach every weight line at different times: ONE of
                      // them takes the HBM miss, the others find the line in their L2 instead of all waiting for the same fill in lockstep
  int krot_ok;        // set by the CALLER: k_rot may be used.  A row's summation order then depends on the M tile it falls into, so rows
                      // with equal inputs no longer come out bit-identical: the DiT forward of a single clip per CFG half opts in
                      // (foley_rt.hip::run_forward); foley_prepare (its row-periodicity check compares bit patterns), batches (clips of a
                      // batch with equal noise stay bit-identical) and the op-level entries do not
  QkvSplitArgs qs;    // EPI_QKV_SPLIT: destination / norm / rotation description (qs.qkv, qs.M unused)
  int vec_out;        // set by the launcher: the problem qualifies for the LDS-transposed vector epilogue
  int wfmt;           // storage of W: 0 = the operand dtype, 1 = fp8 e4m3fn, 2 = fp8 e5m2 (bf16 activations; wave-specialised
                      // tiles only - widened to bf16 in registers, reference FP8WeightWrapper utils.py:316-366)
  int gelu_erf;       // EPI_GELU_T: exact (erf) GELU instead of the tanh form (the conditioning encoders' nn.GELU())
  int dbg_mode;
  long long* dbg;     // tools/gemm_timeline.py: 4 wall-clock stamps per workgroup (entry, first slice
                      // landed, K loop done, epilogue done); null in production
};

// dtype: FOLEY_F32, FOLEY_BF16 or FOLEY_F16 operands (accumulation is always fp32). tile: 0 = auto.
// ksplit_used (optional): the K split the launcher chose (callers of the deferred split-K need it)
int launch_gemm(const GemmArgs& g, int dtype, int epi, int tile, hipStream_t st, int* ksplit_used = nullptr);
// Two independent problems of the same dtype / epilogue in ONE launch (the audio and the visual
// stream of a two-stream block): the small problem's workgroups hide in the large one's shadow.
// Tile shape and K split are chosen for g0.
int launch_gemm_pair(const GemmArgs& g0, const GemmArgs& g1, int dtype, int epi, hipStream_t st, int* ksplit_used = nullptr);
// tap-fused channels-last conv k=3 (gemm_conv3.hip); tile 1 = 128x128, 3 = 64x64; g.ksplit resolved
int launch_gemm_conv3(const GemmArgs& g, int dtype, int epi, int tile, hipStream_t st);
// wave-specialised mainloop (gemm_ws_impl.h; one entry per 16-bit operand type): tile 15 = 128x128, 19 = 256x128; g / g1 resolved by launch_gemm
int launch_gemm_ws_bf16(const GemmArgs& g, const GemmArgs* g1, int epi, int tile, hipStream_t st);
int launch_gemm_ws_f16(const GemmArgs& g, const GemmArgs* g1, int epi, int tile, hipStream_t st);
// 256x256 tiles on the BK = 32 mainloop (gemm_wide_impl.h): tile 31 = tap-fused conv k=3, 32 = plain linear layer (eight waves of
// 128x64); single problem, vector epilogue, any weight storage
int launch_gemm_wide_bf16(const GemmArgs& g, const GemmArgs* g1, int epi, int tile, hipStream_t st);
int launch_gemm_wide_f16(const GemmArgs& g, const GemmArgs* g1, int epi, int tile, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Attention: O = softmax(Q K^T / sqrt(hd)) V, no mask, hd = 128 (or 64: AttnArgs::head_dim).  Q [Bq, H, Sq, hd], K/V [Bkv, H, Skv, hd]
// fp32.  Query batch b reads K/V batch b / kv_bdiv.  Output rows are token-major [.., H*128] in
// dtype `out_dtype`; tokens [0, split) go to outA (clip-major rows of `split` tokens), the rest
// to outB.
// ---------------------------------------------------------------------------------------------
// in_dtype FOLEY_BF16 selects the throughput kernel: Q/K bf16 [B,H,S,128], V transposed bf16
// [B,H,128,vt_pitch] (vt_pitch >= Skv rounded up to 32; the pad must hold finite values).
struct AttnArgs {
  const void* q;
  const void* k;
  const void* v;
  int Bq, H, Sq, Skv, kv_bdiv;
  void* outA;
  void* outB;
  int split;
  int in_dtype;
  int vt_pitch;
  int head_dim;     // 0 / 128: the Foley DiT; 64: the conditioning encoders (fp32 kernel and the 16-bit wide kernel)
  long long* dbg;   // tools/attn_timeline.py: 5 wall-clock stamps per workgroup of the small-grid bf16 kernel; null in production
  int grp_q, grp_kv;     // head_dim 64, 16-bit operands: > 0 = block-diagonal attention - query t attends keys [g*grp_kv, (g+1)*grp_kv), g = t / grp_q
                         // (small groups packed into one sequence: the Synchformer's 8-frame time groups, 14 of them per 128-query workgroup)
  int out_nrows;         // rows of outA when out_rows is set: table entries outside [0, out_nrows) are dropped by the kernels
  const int* out_rows;   // head_dim 64 only: row of outA that query (b, t) is written to - [Bq, Sq]; null: [Bq, Sq] order (split above).
                         // The conditioning encoders scatter every attention of a layer (CLS rows, time / space groups) into ONE
                         // token-major buffer with the table their queries were gathered by - no torch.cat / permute copies.
};
int launch_attention(const AttnArgs& a, int out_dtype, hipStream_t st);

// Timeline attention (attention_timeline.hip; host/prompt_timeline.py states the semantics): every query (b, t) attends the key
// set of its own time, out = (1 - alpha) * attn(q; set_a) + alpha * attn(q; set_b) - two complete softmaxes over the Skv keys of
// one set each, blended in fp32; where alpha == 0 set_b is not read.  head dim 128.  K [n_sets, H, Skv, 128]; V [n_sets, H, Skv,
// 128] (fp32 operands) or transposed [n_sets, H, 128, vt_pitch] (16-bit operands: Skv <= 96, vt_pitch as for launch_attention) -
// the text sets as foley_prepare caches them per block.  set_a / set_b / alpha are DEVICE tables [Bq, Sq]; the kernels clamp the
// set indices to [0, n_sets) before they address anything (caller tables).  Output split as AttnArgs.
struct AttnTimelineArgs {
  const void* q;
  const void* k;
  const void* v;
  const int* set_a;
  const int* set_b;
  const float* alpha;
  int Bq, H, Sq, Skv, n_sets;
  void* outA;
  void* outB;
  int split;
  int in_dtype;
  int vt_pitch;
};
int launch_attention_timeline(const AttnTimelineArgs& a, int out_dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Row kernels
// ---------------------------------------------------------------------------------------------
// out(T)[r, :] = LayerNorm(x[r, :]; eps) * (1 + scale) + shift   (scale/shift optional)
int launch_ln_mod(const float* x, int M, int D, float eps, const RowBcast& shift, const RowBcast& scale,
                  void* out, int out_dtype, hipStream_t st);
// Pending residual update left by a deferred split-K GEMM (GemmArgs::partials): before normalising,
// x += gate * (sum_{s<k} partials[s] + bias) and the new x is written back.
struct LnPending {
  const float* partials;  // null => nothing pending
  int k;
  long stride;
  const float* bias;      // [D] or null
  RowBcast gate;
  int half;               // 0: fp32 slabs; FOLEY_BF16 / FOLEY_F16: slabs in that 16-bit type (GemmArgs::partial_half)
};
struct LnArgs {
  float* x;
  int M;
  RowBcast shift, scale;
  void* out;
  LnPending pend;
};
int launch_ln_mod_pending(float* x, int M, int D, float eps, const RowBcast& shift, const RowBcast& scale,
                          void* out, int out_dtype, const LnPending& pend, hipStream_t st);
// two row sets (same D / eps / dtype) in one launch
int launch_ln_mod_pair(const LnArgs& a0, const LnArgs& a1, int D, float eps, int out_dtype, hipStream_t st);

int launch_qkv_split(const QkvSplitArgs& a, hipStream_t st);
int launch_qkv_split_pair(const QkvSplitArgs& a0, const QkvSplitArgs& a1, hipStream_t st);

// out(T)[r, :] = act(a[r, :] + v[:]) ; a optional [R, D]; v optional broadcast row (step-indexed)
int launch_rows_add_act(const float* a, const RowBcast& v, int R, int D, int act_silu, void* out,
                        int out_dtype, hipStream_t st);
// *flag |= 1 when, in some group of `rows` rows, a row s >= period is not bit-identical to row s - period (fp32 [groups*rows, D])
int launch_rows_periodic_check(const float* x, int groups, int rows, int period, int D, int* flag, hipStream_t st);
// out(T)[r, :] = x[r, :] + pos[r % period, :]
int launch_add_periodic(const float* x, const float* pos, int R, int D, int period, void* out,
                        int out_dtype, hipStream_t st);
// out[r, :] = src[idx[r % n_idx] + (r / n_idx) * src_rows, :]  (fp32 row gather)
int launch_gather_rows(const float* src, const int* idx, int n_idx, int groups, int src_rows, int D,
                       float* out, hipStream_t st);
// generic dtype cast of a contiguous buffer
int launch_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, hipStream_t st);

// latents x [clips, C, L] fp32 -> rows(T) [(cfg*clips + b)*L + l, C] for cfg in [0, ncfg)
int launch_latent_rows(const float* x, int clips, int C, int L, int ncfg, void* out, int out_dtype,
                       hipStream_t st);

// Solver update (CFG combine + flow-match step) and re-staging of the model input rows, in one of three forms that share the
// update's arithmetic bit for bit:
//   edit (audio-to-audio / span regeneration): after a row flagged STEP_BLEND (8) - the iteration that ends a solver step -
//     x <- m*x + (1-m)*(s*noise + (1-s)*x0) with s = coef row column 5 (sigma_{k+1}); mask null = all ones.
//   windows (long clips): clip v*n_win + k is window k of variation v and covers the global frames [starts[k], starts[k] + L);
//     after a row flagged STEP_BLEND every frame is replaced in all the windows that cover it by
//     sum_k weights[k][g - starts[k]] * x_k (fp32, window order), and their next input rows are staged from that value.
enum StepForm { STEP_FORM_PLAIN, STEP_FORM_EDIT, STEP_FORM_WINDOWS };
struct StepArgs {
  const float* pred;   // [ncfg*clips*L, C] model output rows
  float* x;            // [clips, C, L] current sample (updated in place)
  float* x_saved;      // stage-0 sample for multi-stage solvers (or null)
  float* d_acc;        // running derivative combination (or null)
  int clips, C, L, ncfg;   // windows form: clips = variations * n_win, L = frames per window
  float guidance;
  const float* coef;   // per-iteration [n_iter][8]: {w_new, w_acc, dt, w_store, flags, s_next (STEP_BLEND rows), c1, c2 (STEP_HIST rows)}
  int* step_ptr;       // device iteration counter: the row the step reads; the one-thread launch that follows the step advances it
  void* rows_out;      // next model input rows (T), cfg-duplicated (or null)
  int rows_dtype;
  // guidance descriptor (null: the scalar `guidance` and no factor - the plain run's arithmetic bit for bit)
  const float* sched = nullptr;       // [n_iter][2] {g_video, g_text} per iteration, read at row *step_ptr; ncfg 2 reads column 0
  const float* clip_scale = nullptr;  // [clips] CFG-rescale factor of this iteration (launch_guidance_stats), multiplied into v
  StepForm form = STEP_FORM_PLAIN;
  // edit form
  const float* x0 = nullptr;     // [x0_clips, C, L] source latents (clip stride 0 when x0_clips == 1)
  const float* noise = nullptr;  // [clips, C, L] the run's initial noise
  const float* mask = nullptr;   // [mask_clips, L] 1 = regenerate (or null)
  int x0_clips = 0, mask_clips = 0;
  // windows form
  int n_win = 0, Ltot = 0;          // Ltot = starts[n_win - 1] + L
  const int* starts = nullptr;      // [n_win] device, ascending from 0
  const float* weights = nullptr;   // [n_win, L] device; the weights of every global frame sum to 1, a singly covered frame has 1.0f
  // multistep history (null: none - the kernels without it): a ring of hist_slots (order - 1: 1 or 2) slots [clips, C, L] fp32 of
  // the velocities of earlier iterations.  Rows flagged STEP_HIST (16) add coef columns 6 and 7 times the slots (it - 1) and
  // (it - 2) mod hist_slots to the derivative (a zero weight reads nothing); every row stores its own velocity to slot it mod
  // hist_slots after those reads.
  float* hist = nullptr;
  int hist_slots = 0;
  // projected guidance (null: none - the kernels without it; two halves only): proj_coef [clips][2] {a_c, a_w} of this iteration
  // (launch_guidance_project) replaces the combine by v = fma(a_c, c, rnd(a_w * w)) with w = proj_plane [clips*L, C] (APG: the
  // momentum average m, laid out like a pred half) or, without a plane, the unconditional half u (CFG-Zero*)
  const float* proj_coef = nullptr;
  const float* proj_plane = nullptr;
  // memberwise: the runtime keys its captured iteration on what it launches (a C++20 default, accepted under -std=c++17)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc++20-extensions"
  bool operator==(const StepArgs&) const = default;
#pragma clang diagnostic pop
};
int launch_solver_step(const StepArgs& a, hipStream_t st);
// FlowEdit (Kulikov et al. 2024; foley_set_flowedit): one edited clip is a (source, target) pair of batch clips - clip v reads the
// source prompt, clip V + v the target prompt - and the state is z [V, C, L], started at x_src.  One step, at iteration it = *step_ptr
// with row {., ., dt, ., flags, s_next, ., .} of coef:
//   v_s = fma(g_src, c_s - u_s, u_s), v_t = fma(g_tar, c_t - u_t, u_t)        guided_value's two-half expression on clips v and V + v
//   d = v_t - v_s;  d = m*d under a mask (m = mask[v][l]: 1 = edit, 0 = keep);  z = fma(d, dt, z)
// and the rows of the NEXT model call, from s = s_next and n = noise row min(it + 1, noise_rows - 1):
//   z_src = fma(1 - s, x_src, rnd(s*n))      (the edit form's target expression)   -> rows of clip v, both cfg halves
//   z_tar = (z - x_src) + z_src              (z == x_src gives z_src bit for bit)  -> rows of clip V + v, both cfg halves
// m == 0 leaves z bit for bit (d = +-0), m == 1 is the unmasked update.  launch_flowedit_stage is the staging alone, from a scalar
// sigma and a given noise row: the first model input of a run.
struct FlowEditArgs {
  const float* pred = nullptr;    // [2*2V*L, C] model output rows: halves [uncond ; cond] of the clips [src_0.. ; tar_0..]
  float* z = nullptr;             // [V, C, L] the edited latents (updated in place)
  const float* x_src = nullptr;   // [src_clips, C, L] source latents (clip stride 0 when src_clips == 1)
  const float* noise = nullptr;   // [noise_rows, V, C, L]: a row per iteration, or one fixed draw
  const float* mask = nullptr;    // [mask_clips, L] or null (all ones)
  const float* coef = nullptr;    // [n_iter, 8]
  int* step_ptr = nullptr;        // device iteration counter; the one-thread launch that follows the step advances it
  void* rows_out = nullptr;       // next model input rows (T) [2*2V*L, C] (or null: nothing staged)
  int V = 0, C = 0, L = 0, n_iter = 0, rows_dtype = 0;
  int src_clips = 0, noise_rows = 0, mask_clips = 0;
  float g_src = 0.f, g_tar = 0.f;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc++20-extensions"
  bool operator==(const FlowEditArgs&) const = default;
#pragma clang diagnostic pop
};
int launch_flowedit_step(const FlowEditArgs& a, hipStream_t st);
int launch_flowedit_stage(const FlowEditArgs& a, float sigma, int noise_row, hipStream_t st);
// CFG rescale: clip_scale[b] = phi * std(last half of clip b) / std(guided v of clip b) + (1 - phi) over the clip's C x L elements
// (1.0f when the guided std is 0), from `a.pred` at iteration *a.step_ptr with the combine of the step kernels (a.clip_scale is
// not read).  Two launches: per-workgroup centred partial statistics into `part` (guidance_stats_floats(clips, L) floats), then
// one wave per clip merges them in a fixed order - no atomics, repeated runs give the same bits.  phi is read from *phi_ptr when
// that is set (a captured graph then replays with a new value), from `phi` otherwise.
long guidance_stats_floats(int clips, int L);
int launch_guidance_stats(const StepArgs& a, float* part, const float* phi_ptr, float phi, float* clip_scale, hipStream_t st);
// Projected guidance (APG, mode 1; CFG-Zero*, mode 2; two halves): per clip the inner products of this iteration's prediction
// halves over the clip's C x L elements, then coef[b] = {a_c, a_w} from them, the iteration's scale g (a.sched column 0 at row
// *a.step_ptr, else a.guidance) and row *a.step_ptr {eta, beta, R, live} of `rows` [n_iter][4].  APG also leaves the momentum
// average m = (c - u) + beta * m_prev in `plane` [clips*L, C] (in place; beta == 0.0f reads nothing).  Two launches: per-workgroup
// sums into `part` (guidance_project_floats(clips, L) floats), then one wave per clip merges them in a fixed order - no atomics,
// repeated runs give the same bits.  a.proj_coef / a.proj_plane are not read: the operands are the arguments.
constexpr int PROJ_APG = 1, PROJ_ZERO_STAR = 2;
long guidance_project_floats(int clips, int L);
int launch_guidance_project(const StepArgs& a, int mode, const float* rows, float* part, float* coef, float* plane, hipStream_t st);
// Step cache (foley_set_step_cache).  Probe: per row of a0 [Bc*La, D] the first block's modulated input m = LayerNorm(a0; eps) *
// (1 + scale) + shift in fp32; m replaces m_prev [Bc*La, D] in place and rel[b] = sum|m - m_prev| /
// sum|m_prev| over batch row b's La x D elements (0 when the denominator is 0).  Two launches: per-workgroup records into `part`
// (cache_probe_floats(Bc, La) floats), then one wave per batch row merges them in a fixed order - no atomics, repeated runs give
// the same bits.  delta: delta[i] = aN[i] - delta[i] (in place over a copy of a0); apply: audio[i] += delta[i].
long cache_probe_floats(int Bc, int La);
int launch_cache_probe(const float* a0, int Bc, int La, int D, float eps, const RowBcast& shift, const RowBcast& scale, float* m_prev,
                       float* part, float* rel, hipStream_t st);
int launch_cache_delta(const float* aN, float* delta, long n, hipStream_t st);
int launch_cache_apply(float* audio, const float* delta, long n, hipStream_t st);
// x [variations*n_win, C, L] -> out [variations, C, Ltot]: the same weighted mean (windows that agree on a frame: that value as it is)
int launch_windows_stitch(const float* x, int clips, int n_win, int C, int L, int Ltot, const int* starts, const float* weights,
                          float* out, hipStream_t st);
// out [clips, C, L] = sigma*noise + (1-sigma)*x0 (x0 clip stride 0 when x0_clips == 1): the flow-match path's start state
int launch_flow_mix(const float* noise, const float* x0, int x0_clips, int clips, int C, int L, float sigma, float* out,
                    hipStream_t st);

// DAC tail: out[b, t] = tanh(bias + sum_{j<7, c<C} w[j*C + c] * s[b, t + j - 3, c])
// DAC encoder: input conv 1 -> C (k=7) writing y and snake(y); rows [B*T, C] -> planes [B, C, T]
int launch_dac_in(const float* x, const float* w, const float* bias, const float* alpha, int B, int T, int C,
                  float* out0, float* out1, hipStream_t st);
int launch_rows_to_planes(const float* rows, int B, int T, int C, float* out, hipStream_t st);
int launch_qkv_regroup(const void* qkv, int n_rows, int dtype, int H, const int* idx_q, int G, int Sq, const int* idx_kv, int Skv, void* q, void* k,
                       void* v, int vt_pitch, hipStream_t st);
int launch_resize_aa_u8(const uint8_t* in, long outer, int len_in, long inner, int len_out, const int* xmin, const int* xsize,
                        const short* w, int kmax, int prec, uint8_t* out, hipStream_t st);
// audio.hip: the sync scorer's front end (host/sync_score.py)
int launch_resample_sinc(const float* x, int B, int N, int orig, int nnew, const float* taps, int ntaps, int width, float* out,
                         int Nout, hipStream_t st);
int launch_logmel(const float* w16, int B, int N16, const float* basis, const int* mel_lo, const int* mel_len, const float* mel_w,
                  int mel_wp, void* patches, int out_dtype, float* mel_out, hipStream_t st);
// loudness.hip: the BS.1770 meter, the static gain and the look-ahead limiter (host/loudness.py); T16 / taps36 are HOST memory
int launch_loudness_energy(const float* x, int B, int C, int N, long ld, const double* T16, double* work, int64_t work_doubles,
                           double* e, hipStream_t st);
int launch_loudness_gate(const double* e, int B, int C, int nh, double* lufs, double* gamma, double* block_lufs, hipStream_t st);
int launch_true_peak(const float* x, int B, int C, int N, long ld, const float* taps36, float* tp, float* sp, float* env,
                     hipStream_t st);
int launch_loudness_apply(const float* x, int B, int C, int N, long ld, const float* gain, int limiter, double ceil_lin, int W,
                          const float* taps36, float* y, long ldy, float* g_out, hipStream_t st);
int launch_dac_out(const float* s, const float* w, const float* bias, int B, int T, int C, float* out,
                   hipStream_t st);
// clap_audio.hip: the CLAP audio tower's front end and windowed attention (host/clap_score.py)
int launch_melspec_db(const float* x, int B, int N, const int* starts, int n_win, const float* basis, const int* mel_lo,
                      const int* mel_len, const float* mel_w, int mel_wp, float* out, hipStream_t st);
int launch_spec_patches(const float* spec, int G, int T, int F, const float* scale, const float* shift, const int* ridx,
                        const float* rw, int Tq, int ratio, void* out, int out_dtype, int Kp, hipStream_t st);
int launch_window_attention(const void* qkv, int dtype, int rows, int H, const int* table, int n_win, const float* bias,
                            const float* mask, int n_mask, void* out, int out_pitch, hipStream_t st);
