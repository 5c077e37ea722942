// Runtime of libfoley_hip.so: context, packed-weight registry, step-invariant precompute, the DiT
// forward, the device-resident sampler loop and the DAC decoder - all as sequences of launches
// of the kernels in gemm*.hip / attention.hip / rowops.hip on the caller's stream.  C ABI in
// include/foley_hip.h.  No torch types, no CPU fallback.
#include "../../include/foley_hip.h"
#include "kernels.h"
#include "gemm_plan.h"   // foley_debug_gemm_plan

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

thread_local FoleyProfHook g_foley_prof = {nullptr, nullptr};

// Contexts are independent, but several of them may be driven from several threads of one process (node-level data
// parallelism: host/sampler.py::denoise_process_multi runs one context per visible GPU, one thread each).  The set-up phases - workspace allocation and the
// stream capture of the iteration graph - are serialised process-wide (allocation calls from one thread
// while another thread captures are not safe in every HIP runtime); the long replay loops run concurrently.
static std::mutex g_setup_mutex;

// --------------------------------------------------------------------------- errors
static thread_local std::string g_err;
int foley_set_err(const char* msg, const char* file, int line) {
  const char* base = strrchr(file, '/');
  g_err = std::string(msg) + " (" + (base ? base + 1 : file) + ":" + std::to_string(line) + ")";
  return FOLEY_ERR_INVALID;
}
#define FAIL(code, msg) (foley_set_err(msg, __FILE__, __LINE__), (code))
#define TRY(expr)            \
  do {                       \
    int _rc = (expr);        \
    if (_rc != 0) return _rc; \
  } while (0)
#define HIPTRY(expr)                                                     \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      foley_set_err(hipGetErrorString(_e), __FILE__, __LINE__);          \
      return FOLEY_ERR_HIP;                                              \
    }                                                                    \
  } while (0)

// --------------------------------------------------------------------------- context
struct TensorRef {
  const void* p = nullptr;
  int dtype = 0;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct DevBuf {  // context-owned workspace block
  void* p = nullptr;
  size_t bytes = 0;
};

struct Lin {  // a packed linear / conv-as-GEMM layer
  const void* w = nullptr;
  const float* b = nullptr;
  int N = 0, K = 0;
  int wfmt = 0;   // 0: weights in the compute dtype; 1 / 2: stored fp8 e4m3fn / e5m2 (kernels.h GemmArgs::wfmt)
};

// Weights of the DiT forward resolved once per registration (foley_prepare) instead of ~600 string
// lookups per eager iteration; index 0 = audio stream, 1 = visual stream.
struct TripleW {
  Lin qkv[2], proj[2], cq[2], cproj[2], fc1[2], fc2[2];
  const float *qn[2], *kn[2], *cqn[2];
};
struct SingleW {
  Lin qkv, lin1, w13, w2;
  const float *qn, *kn;
};
struct ForwardW {
  std::vector<TripleW> t;
  std::vector<SingleW> s;
  Lin audio_in, fin, smod;
  bool ok = false;
};

// Per-launch HIP-event brackets of one eager forward (foley_profile_forward): label -> time / work.
struct ProfRec {
  const char* label;
  double flop, bytes;
  hipEvent_t e0, e1;
  const void* fn;   // the kernel the op's launch ran (null: the op launched nothing)
};
struct Profiler {
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t get() {
    if (used == pool.size()) {
      hipEvent_t e = nullptr;
      (void)hipEventCreate(&e);
      pool.push_back(e);
    }
    return pool[used++];
  }
};

static int pad32(int x) { return (x + 31) & ~31; }

// Everything ctx_alloc() hands out for the current plan's dimensions.  ctx_free_plan() resets the whole record, so no pointer
// outlives its block; buffers a layout does not need (set_idx, sync_lead_rows, tG) are null in it.
struct PlanBufs {
  // prepared tables
  float* vec_table = nullptr;       // [n_iter, D]
  float* modtab = nullptr;          // [n_triple][2][n_iter][9D]
  void* txt_k = nullptr;            // [n_triple][th, H, Lt, 128]     (same dtype rule as Q/K/V)
  void* txt_v = nullptr;            // [n_triple][th, H, Lt, 128] or transposed [.., 128, ceil32(Lt)]
  float* v_cond0 = nullptr;         // [vh, Lv, D] the distinct visual sets
  float* sync_tok = nullptr;        // [vh, Ls, D] sync tokens after sync_in; audio frame l reads row nearest_exact(l) (RowBcast mode 2)
  int* set_idx = nullptr;           // [ncfg*clips*(Lt + Ls + 8)] row gather tables of the per-row layouts (text, sync, periodic lead)
  float* sync_lead_rows = nullptr;  // per-row visual layout: [ncfg*clips*8, D] the 8 distinct rows of each leading periodic half,
                                    // packed - the per-iteration SiLU(token + vec) of all of them is then one launch
  float* tG = nullptr;              // [ncfg*clips*Lt, 2D] text K/V rows gathered per batch row
  int* flag = nullptr;              // device scratch words of the periodicity check
  // forward workspace
  void* xin = nullptr;              // T [M, C]
  float* audio = nullptr;           // [M, D]
  float* vcond = nullptr;           // [Mv, D]
  void *xn_a = nullptr, *xn_v = nullptr;       // T [M | Mv, D]
  float *qkv_a = nullptr, *qkv_v = nullptr;    // [M | Mv, 3D]
  void *Q = nullptr, *K = nullptr;  // [Bc, H, S, 128]   fp32 (parity mode) or bf16
  void* V = nullptr;                // fp32 [Bc, H, S, 128] or bf16 transposed [Bc, H, 128, ceil32(S)]
  void *att_a = nullptr, *att_v = nullptr;     // T [M | Mv, D]
  void* hid_a = nullptr;            // T [M, max(mlp_hidden, conv_hidden)]
  void* hid_v = nullptr;            // T [Mv, mlp_hidden]
  void* svec = nullptr;             // T [vh*Ls, D]
  float* smod = nullptr;            // [vh*Ls, n_single*6D]
  float* pred = nullptr;            // [M, C]
  float *part_a = nullptr, *part_v = nullptr;   // deferred split-K partial products [PART_CAP][M | Mv][D]
  float *x_saved = nullptr, *d_acc = nullptr;   // [clips, C, La]
  float* x_cur = nullptr;           // [clips, C, La] the sample being denoised (ctx-owned => stable address)
  int* step_ctr = nullptr;
  // ctx-owned copies of the plan's lookup tables (stable addresses across foley_prepare calls)
  float *rope_cos = nullptr, *rope_sin = nullptr, *solver_coef = nullptr;
  int *pos_audio_self = nullptr, *pos_visual_self = nullptr, *pos_linear = nullptr, *sync_gather = nullptr;
  int* rep_idx = nullptr;           // [clips*Lv] j -> j % Lv: replicates the visual projection per clip in one launch
  // rotation rows gathered per token for the fused head-split epilogues: rot_*[k][l] = rope_{cos,sin}[pos_k[l]], [len, 64] fp32
  // (k: 0 audio self, 1 visual self, 2 linear positions)
  float *rot_cos[3] = {nullptr, nullptr, nullptr}, *rot_sin[3] = {nullptr, nullptr, nullptr};
  void *tA = nullptr, *tB = nullptr;  // precompute scratch
  float* tF = nullptr;              // the last block foley_prepare allocates
  bool complete() const { return tF != nullptr; }
};

// How the conditioning of the prepared run is laid out: foley_prepare derives it once (the slots before it sizes the workspace,
// the rest from the sync tokens it computed) and the forward only reads it.  Integral members, no padding: compared bytewise.
struct RunLayout {
  // conditioning sets (foley_prepare_sets): the text K/V sets and the visual halves (sync_tok, svec, smod) are held per cfg half
  // (ncfg slots, read by `clips` batch rows each) or per batch row (ncfg*clips slots)
  int sets = 0, t_rows = 0, v_rows = 0;   // set maps given; text / visual stream laid out per batch row
  int th = 0, vh = 0;               // text K/V slots, visual halves
  int tdiv = 0, vdiv = 0;           // batch row b reads text slot b / tdiv and visual half b / vdiv
  int Sp = 0, Lap = 0, Ltp = 0;     // V^T row pitches of the 16-bit attention: joint, audio-only, text
  // sync tokens: the first `lead` halves repeat with period `per` = 8 (empty sync features): all of them for text-to-audio, 1 of
  // 2 for a video clip under CFG (unconditional half first, utils.py:150-176), 0 (and per = 0) for none
  int lead = 0, per = 0, allper = 0;   // allper: every half is periodic
  // the single-stream blocks' modulation table of one iteration: R distinct rows - `per` of each leading half, then Ls of each
  // dense half, the row order of RowBcast::dense_from / dense_base - of smod_ld floats
  int R = 0;
  long smod_ld = 0;
  // hoisted: the table of EVERY iteration was built by foley_prepare, [n_iter][vh*P][smod_ld] with P = per (all halves periodic)
  // or Ls rows per half (a hoisted table that is not all-periodic is dense); consumers add step * smod_step to their row address
  int hoisted = 0, P = 0;
  int mod_per = 0, mod_lead = 0;    // rb_up() arguments of the table the blocks read (0: dense rows; lead -1: every half periodic)
  long smod_step = 0;
  bool operator==(const RunLayout& o) const { return memcmp(this, &o, sizeof(o)) == 0; }
};
static_assert(std::has_unique_object_representations_v<RunLayout>, "RunLayout is compared bytewise");

// The option-dependent operands of one loop iteration's launches, as iter_args() derives them from the context: the ONE statement
// of what an iteration is launched with under the current run options.  The launches and the key of the captured iteration both
// take them from here, so an operand a foley_set_* call or foley_prepare_timeline can change is in the key because it is
// launched.  A new option adds its operands to this record and to iter_args(), and nothing else.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc++20-extensions"   // defaulted comparisons under -std=c++17
struct IterArgs {
  // the solver step, complete: the guidance scalar (0 under a schedule table, which replaces it: guided_value never reads it
  // then), the table, the edit / windows form with its operands, the multistep ring and its slot count
  StepArgs step{};
  // CFG rescale: the statistics launches in front of the step - their scratch, phi behind the schedule table and the factors they
  // write, which the step reads as step.clip_scale (all null: off - no such launches, another topology)
  float *guid_part = nullptr, *guid_scale = nullptr;
  const float* guid_phi = nullptr;
  // projected guidance: the two launches in front of the step, in the rescale launches' place - the mode, the per-iteration
  // rows, the scratch, and what they write: the coefficients and (APG) the plane, which the step reads as step.proj_coef /
  // step.proj_plane (mode 0: off - no such launches, the step kernels without projection)
  int proj_mode = 0;
  const float* proj_rows = nullptr;
  float *proj_part = nullptr, *proj_coef = nullptr, *proj_plane = nullptr;
  // step cache: the residual the two bodies address and the probe's buffers (all null: off - the one straight-line iteration; on:
  // the three graphs head / full body / skip body).  Mode, threshold and skip list are host decisions between replays: not here.
  float *sc_delta = nullptr, *sc_mprev = nullptr, *sc_part = nullptr, *sc_rel = nullptr;
  // prompt timeline: the text sets the timeline kernel addresses (0: off - the plain cross-attention, fused into its q projection
  // where that applies: another topology) and the ctx-owned per-token tables
  int tl_sets = 0;
  const int *tl_a = nullptr, *tl_b = nullptr;
  const float* tl_alpha = nullptr;
  // FlowEdit: the step of a (source, target) pair batch in place of the solver step, complete (z null: off - the solver step)
  FlowEditArgs flowedit{};
  bool operator==(const IterArgs&) const = default;
};

// Everything a captured loop iteration depends on beyond the workspace dimensions (a change of those frees the plan and the
// graph with it): what it is launched with, and what is not a launch operand.  foley_sample compares the key of the capture
// with the current one; nothing else decides a graph's validity.  New values behind an unchanged address (a schedule, a mask, a
// timeline of the same shape) only rewrite what a replay reads.
struct GraphKey {
  IterArgs args;
  std::vector<int32_t> set_maps;    // text_of ++ vis_of (empty: foley_prepare); for safety, not layout: the tables are rewritten in place
  RunLayout layout;
  const void* smod_tab = nullptr;   // the hoisted table (null: the per-iteration GEMM)
  uint64_t tensor_gen = 0;          // bumped when a registered tensor moves (foley_set_tensor)
  uint64_t plan_gen = 0;            // bumped when the workspace is freed (ctx_free_plan)
  bool operator==(const GraphKey&) const = default;
};
#pragma clang diagnostic pop

// The option values of the prepared run: foley_prepare resets them as one value, the foley_set_* calls (and foley_prepare_timeline)
// set their own.  Values only - the buffers they speak of are the context's, grow-only, and outlive a prepare.
struct RunOptions {
  bool edit = false;                      // foley_set_edit; off: a plain run
  int edit_x0_clips = 1, edit_mask_clips = 0;   // mask clips 0: no mask (all ones)
  int n_win = 0, win_Ltot = 0;            // foley_set_windows; n_win 0: the clips are independent
  bool guid_sched_on = false, guid_rescale_on = false;   // foley_set_guidance; off: the plan's scalar, no factors
  int sc_mode = 0;                        // foley_set_step_cache: 0 off, FOLEY_STEP_CACHE_SCHEDULE, FOLEY_STEP_CACHE_THRESHOLD
  std::vector<uint8_t> sc_skip;           // schedule mode: [n_iter]
  double sc_threshold = 0.0;
  std::vector<double> sc_poly;            // highest degree first (empty: identity)
  int sc_lo = 0, sc_hi = 0, sc_maxc = 0;  // iterations [lo, hi) may skip; longest run of skips (0: no cap)
  int tl_sets = 0;                        // foley_prepare_timeline: the number of text sets (0: one text set per batch row)
  int ms_order = 0;                       // foley_set_multistep: 0 a one-step method, 2 or 3
  int proj_mode = 0;                      // foley_set_projected_guidance: 0 off, FOLEY_GUIDANCE_APG, FOLEY_GUIDANCE_ZERO_STAR
  bool flowedit = false;                  // foley_set_flowedit; on: plan.clips = 2V pair clips, the state is z [V, latent_dim, La]
  int fe_src_clips = 1, fe_noise_rows = 1, fe_mask_clips = 0;   // mask clips 0: no mask (all ones)
  float fe_g_src = 0.f, fe_g_tar = 0.f, fe_sigma0 = 1.f;
};

struct foley_ctx {
  int device = 0;
  foley_config cfg{};
  std::unordered_map<std::string, TensorRef> tensors;
  uint64_t tensor_gen = 0;
  ForwardW fw;
  Profiler prof;
  // run state (valid after foley_prepare)
  bool prepared = false;
  foley_plan plan{};
  std::vector<DevBuf> owned;        // everything hipMalloc'ed for the current plan
  uint64_t plan_gen = 0;
  PlanBufs buf;
  RunLayout layout;
  int vis_src = 0;                  // sets in v_cond0 (the source stride of a one-group gather: no captured kernel reads it)
  std::vector<int32_t> set_maps;    // text_of ++ vis_of of the prepared run (empty: foley_prepare)
  DevBuf smod_tab, svec_tab;        // the hoisted modulation table and its SiLU(token + vec) input (layout.hoisted), grown on demand
  // one captured loop iteration and what it was captured for
  hipGraphExec_t graph_exec = nullptr;
  GraphKey graph_key;
  uint64_t graph_captures = 0;      // iterations captured so far (foley_debug_run_state)
  RunOptions opt;                   // what the foley_set_* calls asked for (reset by foley_prepare)
  // ctx-owned copies behind the options, grown on demand.  Edit: the source latents, the run's noise and the mask
  DevBuf edit_x0, edit_noise, edit_mask;
  // windows: the starts and the blend weights
  DevBuf win_starts, win_weights;
  std::vector<int32_t> win_starts_host;   // the source of the asynchronous copy stays alive with the context
  // guidance: the schedule table [n_iter][2] followed by phi, the per-workgroup statistics and the per-clip factors
  DevBuf guid_sched, guid_part, guid_scale;
  std::vector<float> guid_host;           // [n_iter*2 + 1] source of the copy
  // step cache: the residual / probe buffers, the pinned read-back of the per-row change measure and the report of the last loop
  DevBuf sc_delta, sc_mprev, sc_part, sc_rel;
  float* sc_rel_host = nullptr;           // pinned, sc_rel_cap floats
  int sc_rel_cap = 0;
  std::vector<float> sc_rep_rel;          // [n_iter] of the last loop (-1: not measured)
  std::vector<int32_t> sc_rep_skip;
  hipGraphExec_t graph_head = nullptr, graph_skip = nullptr;   // with graph_exec (the full body) the three graphs of a cached loop
  // prompt timeline: the per-token tables [ncfg*clips*(Lv+La)]; ws_tl_sets: the set count the workspace was sized for
  int ws_tl_sets = 0;
  DevBuf tl_a, tl_b, tl_alpha;
  // multistep: the ring of order - 1 velocity slots [clips, latent_dim, La] fp32 that the history step kernels read and feed
  DevBuf ms_hist;
  // projected guidance: the rows [n_iter][4], the per-workgroup sums, the coefficients [clips][2] and APG's plane [clips*La, latent_dim]
  DevBuf proj_rows, proj_part, proj_coef, proj_plane;
  std::vector<float> proj_host;           // [n_iter*4] source of the copy
  // FlowEdit: the source latents, the noise table [noise_rows, V, latent_dim, La] and the mask
  DevBuf fe_x_src, fe_noise, fe_mask;
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  std::atomic<int> abort_req{0};   // foley_abort(): checked by foley_sample between iterations
  // DAC workspace (grown on demand)
  DevBuf dacP, dacQ, dacR, dacZ;
  // reference-keyed weight store (weights.hip): ctx-owned packed arena
  void* wstore = nullptr;
  void (*wstore_free)(void*) = nullptr;
  // low-rank adapters merged into the registered weights (lora.hip): pristine copies of the touched packed tensors
  void* lora = nullptr;
  void (*lora_free)(void*) = nullptr;
};

// What an iteration of the prepared run is launched with under the current options (IterArgs).  No launches; reads the context only.
static IterArgs iter_args(const foley_ctx* c) {
  const foley_plan& pl = c->plan;
  const RunOptions& o = c->opt;
  IterArgs a{StepArgs{c->buf.pred, c->buf.x_cur, c->buf.x_saved, c->buf.d_acc, pl.clips, c->cfg.latent_dim, pl.La, pl.ncfg,
                      o.guid_sched_on ? 0.f : pl.guidance, pl.solver_coef, c->buf.step_ctr, c->buf.xin, c->cfg.compute_dtype}};
  StepArgs& s = a.step;
  if (o.guid_sched_on) s.sched = (const float*)c->guid_sched.p;
  if (o.guid_rescale_on) {   // the factors of this iteration's prediction, before the step applies them (a window is a clip)
    a.guid_part = (float*)c->guid_part.p;
    a.guid_phi = (const float*)c->guid_sched.p + 2 * (size_t)pl.n_iter;
    s.clip_scale = a.guid_scale = (float*)c->guid_scale.p;
  }
  if (o.proj_mode) {   // this iteration's coefficients (and APG's plane), before the step applies them (a window is a clip)
    a.proj_mode = o.proj_mode;
    a.proj_rows = (const float*)c->proj_rows.p;
    a.proj_part = (float*)c->proj_part.p;
    s.proj_coef = a.proj_coef = (float*)c->proj_coef.p;
    s.proj_plane = a.proj_plane = o.proj_mode == FOLEY_GUIDANCE_APG ? (float*)c->proj_plane.p : nullptr;
  }
  if (o.edit) {   // the edit operands are ctx-owned copies, so their addresses stand for them; so do those of the windows tables
    s.form = STEP_FORM_EDIT;
    s.x0 = (const float*)c->edit_x0.p; s.noise = (const float*)c->edit_noise.p;
    s.mask = o.edit_mask_clips ? (const float*)c->edit_mask.p : nullptr;
    s.x0_clips = o.edit_x0_clips; s.mask_clips = o.edit_mask_clips;
  } else if (o.n_win) {
    s.form = STEP_FORM_WINDOWS;
    s.n_win = o.n_win; s.Ltot = o.win_Ltot;
    s.starts = (const int*)c->win_starts.p; s.weights = (const float*)c->win_weights.p;
  }
  if (o.ms_order >= 2) {   // the history instantiation of the same form; a skipped (cached) iteration feeds the ring like any other
    s.hist = (float*)c->ms_hist.p;
    s.hist_slots = o.ms_order - 1;
  }
  if (o.sc_mode) {
    a.sc_delta = (float*)c->sc_delta.p; a.sc_mprev = (float*)c->sc_mprev.p;
    a.sc_part = (float*)c->sc_part.p; a.sc_rel = (float*)c->sc_rel.p;
  }
  if (o.tl_sets) {
    a.tl_sets = o.tl_sets; a.tl_a = (const int*)c->tl_a.p; a.tl_b = (const int*)c->tl_b.p; a.tl_alpha = (const float*)c->tl_alpha.p;
  }
  if (o.flowedit) {   // ctx-owned copies again: their addresses, the counts and the scales stand for the operands
    FlowEditArgs& f = a.flowedit;
    f.pred = c->buf.pred; f.z = c->buf.x_cur; f.coef = pl.solver_coef; f.step_ptr = c->buf.step_ctr;
    f.rows_out = c->buf.xin; f.rows_dtype = c->cfg.compute_dtype;
    f.V = pl.clips / 2; f.C = c->cfg.latent_dim; f.L = pl.La; f.n_iter = pl.n_iter;
    f.x_src = (const float*)c->fe_x_src.p; f.noise = (const float*)c->fe_noise.p;
    f.mask = o.fe_mask_clips ? (const float*)c->fe_mask.p : nullptr;
    f.src_clips = o.fe_src_clips; f.noise_rows = o.fe_noise_rows; f.mask_clips = o.fe_mask_clips;
    f.g_src = o.fe_g_src; f.g_tar = o.fe_g_tar;
  }
  return a;
}

// internal hooks for weights.hip (not part of the C ABI)
void** foley_ctx_wstore_slot(foley_ctx* c) { return &c->wstore; }
void foley_ctx_set_wstore_free(foley_ctx* c, void (*fn)(void*)) { c->wstore_free = fn; }
const foley_config* foley_ctx_config(foley_ctx* c) { return &c->cfg; }
int foley_ctx_device(foley_ctx* c) { return c->device; }
// internal hooks for lora.hip (not part of the C ABI)
void** foley_ctx_lora_slot(foley_ctx* c) { return &c->lora; }
void foley_ctx_set_lora_free(foley_ctx* c, void (*fn)(void*)) { c->lora_free = fn; }
bool foley_ctx_tensor(foley_ctx* c, const char* name, void** p, int* dtype, std::vector<int64_t>* shape) {
  auto it = c->tensors.find(name);
  if (it == c->tensors.end()) return false;
  *p = const_cast<void*>(it->second.p);
  *dtype = it->second.dtype;
  *shape = it->second.shape;
  return true;
}
void foley_ctx_weights_changed(foley_ctx* c) { c->prepared = false; }   // cached tables depend on the weights (as in foley_set_tensor)

static size_t esize(int dtype) { return foley_is_half(dtype) ? 2 : (dtype == FOLEY_F8E4M3 || dtype == FOLEY_F8E5M2) ? 1 : 4; }

static int ctx_alloc(foley_ctx* c, size_t bytes, void** out) {
  void* p = nullptr;
  bytes = (bytes + 255) & ~(size_t)255;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 256);
  if (e != hipSuccess) return FAIL(FOLEY_ERR_HIP, hipGetErrorString(e));
  c->owned.push_back({p, bytes});
  *out = p;
  return 0;
}

static void ctx_drop_graph(foley_ctx* c) {
  if (c->graph_exec) {
    hipGraphExecDestroy(c->graph_exec);
    c->graph_exec = nullptr;
  }
  for (hipGraphExec_t* g : {&c->graph_head, &c->graph_skip})
    if (*g) {
      hipGraphExecDestroy(*g);
      *g = nullptr;
    }
}

static void ctx_free_plan(foley_ctx* c) {
  ctx_drop_graph(c);   // eagerly, with the memory its kernels address; plan_gen keeps a later comparison from matching
  ++c->plan_gen;
  for (auto& b : c->owned) hipFree(b.p);
  c->owned.clear();
  c->buf = {};
  c->layout = {};
  c->ws_tl_sets = 0;
  c->prepared = false;
}

static bool same_dims(const foley_plan& a, const foley_plan& b) {
  return a.ncfg == b.ncfg && a.clips == b.clips && a.La == b.La && a.Lv == b.Lv && a.Ls == b.Ls && a.Lt == b.Lt &&
         a.n_iter == b.n_iter && a.rope_len == b.rope_len;
}

static void release(DevBuf& b) {
  if (b.p) hipFree(b.p);
  b = DevBuf{};
}

static int grow(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes) return 0;
  release(b);
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) return FAIL(FOLEY_ERR_HIP, hipGetErrorString(e));
  b.bytes = bytes;
  return 0;
}

static int get_tensor(foley_ctx* c, const std::string& name, int dtype, std::initializer_list<int64_t> shape,
                      const void** out) {
  auto it = c->tensors.find(name);
  if (it == c->tensors.end()) {
    g_err = "tensor '" + name + "' was not registered";
    return FOLEY_ERR_MISSING;
  }
  const TensorRef& t = it->second;
  bool ok = t.dtype == dtype && t.shape.size() == shape.size();
  if (ok) {
    size_t i = 0;
    for (auto s : shape) ok = ok && (t.shape[i++] == s);
  }
  if (!ok) {
    g_err = "tensor '" + name + "' has the wrong dtype/shape";
    return FOLEY_ERR_INVALID;
  }
  *out = t.p;
  return 0;
}

// --------------------------------------------------------------------------- zero page
// 256 zero bytes per device: the direct-to-LDS GEMM loop reads masked rows from here.
static const void* zero_page() {
  static void* pages[64] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!pages[dev]) {
    void* p = nullptr;
    if (hipMalloc(&p, 256) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, 256) != hipSuccess) return nullptr;
    pages[dev] = p;
  }
  return pages[dev];
}

// --------------------------------------------------------------------------- launch helpers
static RowBcast rb_none() { return RowBcast{nullptr, 0, 0, 1, 1, nullptr, 0}; }
static RowBcast rb_vec(const float* base, long step_stride, const int* step_ptr);

// K ranges whose partial products a gated-residual GEMM may leave for the next LayerNorm to sum
// (deferred split-K, kernels.h GemmArgs::partials)
constexpr int PART_CAP = 8;

static int get_lin(foley_ctx* c, const std::string& name, int dtype, int N, int K, bool bias, Lin* out) {
  const void* w;
  out->wfmt = 0;
  auto it = c->tensors.find(name + ".w");
  if (it != c->tensors.end() && foley_is_half(dtype) && (it->second.dtype == FOLEY_F8E4M3 || it->second.dtype == FOLEY_F8E5M2)) {
    // fp8 weight-only storage (reference FP8WeightWrapper): the GEMM widens in registers
    out->wfmt = it->second.dtype == FOLEY_F8E4M3 ? 1 : 2;
    TRY(get_tensor(c, name + ".w", it->second.dtype, {N, K}, &w));
  } else {
    TRY(get_tensor(c, name + ".w", dtype, {N, K}, &w));
  }
  out->w = w;
  out->N = N;
  out->K = K;
  out->b = nullptr;
  if (bias) {
    const void* b;
    TRY(get_tensor(c, name + ".b", FOLEY_F32, {N}, &b));
    out->b = (const float*)b;
  }
  return 0;
}

// plain linear layer over M rows
static GemmArgs gemm_plain(const void* A, int M, const Lin& l, void* out, long ldc) {
  GemmArgs g{};
  g.A = A; g.W = l.w; g.bias = l.b;
  g.M = M; g.N = l.N; g.K = l.K; g.lda = l.K;
  g.wfmt = l.wfmt;
  g.segV = M > 0 ? M : 1; g.segS = g.segV; g.taps = 1; g.tapC = l.K; g.dil = 1; g.tap0 = 0;
  g.out0 = out; g.out1 = nullptr;
  g.osegV = g.segV; g.out_seg = 0; g.out_row = ldc; g.out_shift = 0; g.out_check = 0;
  g.rb = rb_none(); g.res = nullptr; g.alpha = nullptr; g.alphaC = 1;
  g.zeros = zero_page();
  return g;
}

// channels-last conv (k taps, dilation d, 'same' padding) over segments of `seg` rows
static GemmArgs gemm_conv(const void* A, int M, int seg, int C, int taps, int dil, const Lin& l, void* out,
                          long ldc) {
  GemmArgs g = gemm_plain(A, M, l, out, ldc);
  g.lda = C;
  g.segV = seg; g.segS = seg; g.taps = taps; g.tapC = C; g.dil = dil; g.tap0 = -((taps - 1) / 2) * dil;
  return g;
}

// Head-split arguments of the text K/V (foley_prepare), the two-stream and the single-stream blocks.  An output with a gain is
// RMS-normalised and rotated at the positions of rotation slot `rot` (0 audio self, 1 visual self, 2 linear positions); rot_rows:
// the fused GEMM epilogues read the rotation from the per-token rows foley_prepare gathered for that slot.
static QkvSplitArgs qkv_split_args(const foley_ctx* c, const float* qkv, int M, int L, int nK, const float* gain0, const float* gain1,
                                   int rot, bool rot_rows, void* const dst[3], int S_tot, int tok_off, int vt_pitch, float eps) {
  const foley_plan& pl = c->plan;
  const int* const pos[3] = {pl.pos_audio_self, pl.pos_visual_self, pl.pos_linear};
  QkvSplitArgs q{};
  q.qkv = qkv; q.M = M; q.L = L; q.H = c->cfg.heads; q.nK = nK;
  q.gain[0] = gain0; q.gain[1] = gain1;
  for (int i = 0; i < 2; ++i) {
    if (!q.gain[i]) continue;
    q.pos[i] = pos[rot];
    if (rot_rows) { q.rcos[i] = c->buf.rot_cos[rot]; q.rsin[i] = c->buf.rot_sin[rot]; }
  }
  for (int i = 0; i < 3; ++i) q.dst[i] = dst[i];
  q.out_dtype = c->cfg.compute_dtype; q.vt_pitch = vt_pitch;
  q.S_tot = S_tot; q.tok_off = tok_off; q.eps = eps; q.cos_tab = pl.rope_cos; q.sin_tab = pl.rope_sin;
  return q;
}

// --------------------------------------------------------------------------- C ABI: context
extern "C" uint32_t foley_abi_version(void) { return FOLEY_ABI_VERSION; }
extern "C" const char* foley_last_error(void) { return g_err.c_str(); }

extern "C" int foley_ctx_create(int device, const foley_config* cfg, foley_ctx** out) {
  if (!cfg || !out) return FAIL(FOLEY_ERR_INVALID, "null argument");
  // (the sampling path needs head_dim 128 and says so in foley_prepare; loading and merging weights work at any head_dim)
  if (cfg->heads < 1 || cfg->hidden < 1 || cfg->hidden % cfg->heads) return FAIL(FOLEY_ERR_INVALID, "hidden must be a multiple of heads");
  if (cfg->compute_dtype != FOLEY_DT_F32 && cfg->compute_dtype != FOLEY_DT_BF16 && cfg->compute_dtype != FOLEY_DT_F16)
    return FAIL(FOLEY_ERR_INVALID, "compute_dtype must be f32, bf16 or f16");
  if (cfg->dac_n_rates < 1 || cfg->dac_n_rates > 8) return FAIL(FOLEY_ERR_INVALID, "bad dac_n_rates");
  int ndev = 0;
  HIPTRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return FAIL(FOLEY_ERR_INVALID, "no such HIP device");
  HIPTRY(hipSetDevice(device));
  foley_ctx* c = new foley_ctx();
  c->device = device;
  c->cfg = *cfg;
  (void)hipEventCreate(&c->ev0);
  (void)hipEventCreate(&c->ev1);
  *out = c;
  return 0;
}

extern "C" void foley_ctx_destroy(foley_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  ctx_free_plan(c);
  for (DevBuf* b : {&c->dacP, &c->dacQ, &c->dacR, &c->dacZ, &c->smod_tab, &c->svec_tab, &c->edit_x0, &c->edit_noise, &c->edit_mask, &c->win_starts, &c->win_weights, &c->guid_sched,
                    &c->guid_part, &c->guid_scale, &c->sc_delta, &c->sc_mprev, &c->sc_part, &c->sc_rel, &c->tl_a, &c->tl_b, &c->tl_alpha, &c->ms_hist, &c->fe_x_src, &c->fe_noise, &c->fe_mask}) release(*b);
  if (c->sc_rel_host) (void)hipHostFree(c->sc_rel_host);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  for (auto e : c->prof.pool) hipEventDestroy(e);
  if (c->lora && c->lora_free) c->lora_free(c->lora);
  if (c->wstore && c->wstore_free) c->wstore_free(c->wstore);
  delete c;
}

extern "C" int foley_set_tensor(foley_ctx* c, const char* name, const void* p, int dtype, int ndim,
                                const int64_t* shape) {
  if (!c || !name || !p || ndim < 0 || ndim > 8) return FAIL(FOLEY_ERR_INVALID, "bad tensor registration");
  if (((uintptr_t)p) & 15) return FAIL(FOLEY_ERR_INVALID, "tensor pointers must be 16-byte aligned");
  TensorRef t;
  t.p = p;
  t.dtype = dtype;
  t.shape.assign(shape, shape + ndim);
  auto it = c->tensors.find(name);
  if (it != c->tensors.end() && it->second.p != p) ++c->tensor_gen;  // captured kernels hold the old address
  c->tensors[name] = t;
  c->fw.ok = false;     // resolved pointers are refreshed by the next foley_prepare
  c->prepared = false;  // cached tables depend on the weights
  return 0;
}

extern "C" int foley_last_elapsed_ms(foley_ctx* c, float* ms) {
  if (!c || !ms || !c->timed) return FAIL(FOLEY_ERR_STATE, "nothing timed yet");
  HIPTRY(hipEventSynchronize(c->ev1));
  HIPTRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return 0;
}

// --------------------------------------------------------------------------- resolved weights
static int get_vec(foley_ctx* c, const std::string& name, int n, const float** out) {
  const void* p;
  TRY(get_tensor(c, name, FOLEY_F32, {n}, &p));
  *out = (const float*)p;
  return 0;
}

static int resolve_forward_weights(foley_ctx* c) {
  const foley_config& f = c->cfg;
  const int D = f.hidden, T = f.compute_dtype, Hc = f.conv_hidden;
  ForwardW& w = c->fw;
  w.ok = false;
  w.t.assign(f.depth_triple, TripleW{});
  w.s.assign(f.depth_single, SingleW{});
  for (int b = 0; b < f.depth_triple; ++b) {
    TripleW& t = w.t[b];
    for (int s = 0; s < 2; ++s) {
      const std::string p = "t" + std::to_string(b) + (s ? ".v_" : ".a_");
      TRY(get_lin(c, p + "qkv", T, 3 * D, D, true, &t.qkv[s]));
      TRY(get_lin(c, p + "proj", T, D, D, true, &t.proj[s]));
      TRY(get_lin(c, p + "cq", T, D, D, true, &t.cq[s]));
      TRY(get_lin(c, p + "cproj", T, D, D, true, &t.cproj[s]));
      TRY(get_lin(c, p + "fc1", T, f.mlp_hidden, D, true, &t.fc1[s]));
      TRY(get_lin(c, p + "fc2", T, D, f.mlp_hidden, true, &t.fc2[s]));
      TRY(get_vec(c, p + "qn", 128, &t.qn[s]));
      TRY(get_vec(c, p + "kn", 128, &t.kn[s]));
      TRY(get_vec(c, p + "cqn", 128, &t.cqn[s]));
    }
  }
  for (int b = 0; b < f.depth_single; ++b) {
    SingleW& q = w.s[b];
    const std::string p = "s" + std::to_string(b) + ".";
    TRY(get_lin(c, p + "qkv", T, 3 * D, D, true, &q.qkv));
    TRY(get_lin(c, p + "lin1", T, D, 3 * D, true, &q.lin1));
    TRY(get_lin(c, p + "w13", T, 2 * Hc, 3 * D, false, &q.w13));
    TRY(get_lin(c, p + "w2", T, D, 3 * Hc, false, &q.w2));
    TRY(get_vec(c, p + "qn", 128, &q.qn));
    TRY(get_vec(c, p + "kn", 128, &q.kn));
  }
  TRY(get_lin(c, "audio_in", T, D, f.latent_dim, true, &w.audio_in));
  TRY(get_lin(c, "final", T, f.latent_dim, D, true, &w.fin));
  if (f.depth_single > 0) TRY(get_lin(c, "smod_all", T, f.depth_single * 6 * D, D, true, &w.smod));
  w.ok = true;
  return 0;
}

// --------------------------------------------------------------------------- prepare
// Everything that does not depend on the latents: time embedding for every loop
// iteration, the triple blocks' AdaLN tables, text K/V per block, cond/visual/sync embedders.
static int prepare_impl(foley_ctx* c, const foley_plan* pl, const foley_cond_sets* sets, const foley_text_timeline* tl, void* stream_v);

extern "C" int foley_prepare(foley_ctx* c, const foley_plan* pl, void* stream_v) {
  return prepare_impl(c, pl, nullptr, nullptr, stream_v);
}

extern "C" int foley_prepare_sets(foley_ctx* c, const foley_plan* pl, const foley_cond_sets* sets, void* stream_v) {
  if (!sets) return prepare_impl(c, pl, nullptr, nullptr, stream_v);
  if (!sets->text_of || !sets->vis_of) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_sets: null set map");
  return prepare_impl(c, pl, sets, nullptr, stream_v);
}

// Prompt timeline: plan.text holds tl->n_text sets, cached per block without a per-row gather (th = n_text slots); every query token
// of the cross-attention picks its one or two sets through the tables (attention_timeline.hip).  The visual side is foley_prepare's.
extern "C" int foley_prepare_timeline(foley_ctx* c, const foley_plan* pl, const foley_text_timeline* tl, void* stream_v) {
  if (!c || !pl || !tl) return FAIL(FOLEY_ERR_INVALID, "null argument");
  if (!tl->set_a || !tl->set_b || !tl->alpha) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_timeline: null table");
  if (tl->n_text < 1 || tl->n_text > FOLEY_TIMELINE_MAX_SETS) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_timeline: n_text must be in [1, 16]");
  if (pl->ncfg < 1 || pl->clips < 1 || pl->La < 1 || pl->Lv < 1) return FAIL(FOLEY_ERR_INVALID, "bad plan dimensions");
  if (foley_is_half(c->cfg.compute_dtype) && pl->Lt > 96)
    return FAIL(FOLEY_ERR_INVALID, "foley_prepare_timeline: 16-bit compute takes at most 96 text tokens per set");
  const size_t n = (size_t)pl->ncfg * pl->clips * ((size_t)pl->Lv + pl->La);
  for (size_t i = 0; i < n; ++i) {
    if (tl->set_a[i] < 0 || tl->set_a[i] >= tl->n_text || tl->set_b[i] < 0 || tl->set_b[i] >= tl->n_text)
      return FAIL(FOLEY_ERR_INVALID, "foley_prepare_timeline: set index out of range");
    if (!(tl->alpha[i] >= 0.f && tl->alpha[i] < 1.f)) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_timeline: alpha outside [0, 1)");
  }
  return prepare_impl(c, pl, nullptr, tl, stream_v);
}

static int prepare_impl(foley_ctx* c, const foley_plan* pl, const foley_cond_sets* sets, const foley_text_timeline* tl, void* stream_v) {
  if (!c || !pl) return FAIL(FOLEY_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  const foley_config& f = c->cfg;
  if (f.hidden / f.heads != 128) return FAIL(FOLEY_ERR_INVALID, "head_dim must be 128");
  if (pl->ncfg < 1 || pl->ncfg > 3 || pl->clips < 1 || pl->La < 1 || pl->Lv < 1 || pl->Ls < 8 || pl->Ls % 8 ||
      pl->Lt < 1 || pl->n_iter < 1)
    return FAIL(FOLEY_ERR_INVALID, "bad plan dimensions");
  if (pl->rope_len < 2 * pl->La) return FAIL(FOLEY_ERR_INVALID, "rope table shorter than 2*La");
  // Conditioning sets: foley_prepare has one text set and one visual set per cfg half.  With set maps, a stream whose map is
  // b -> b / clips over ncfg sets keeps that layout; any other map lays the stream out per batch row.
  int n_text = pl->ncfg, n_vis = pl->ncfg;
  bool t_rows = false, v_rows = false;
  std::vector<int32_t> maps;
  if (sets) {
    const int Bc0 = pl->ncfg * pl->clips;
    if (sets->n_text < 1 || sets->n_vis < 1 || sets->n_text > Bc0 || sets->n_vis > Bc0)
      return FAIL(FOLEY_ERR_INVALID, "foley_prepare_sets: set counts must be in [1, ncfg*clips]");
    maps.assign(sets->text_of, sets->text_of + Bc0);
    maps.insert(maps.end(), sets->vis_of, sets->vis_of + Bc0);
    bool t_half = sets->n_text == pl->ncfg, v_half = sets->n_vis == pl->ncfg;
    for (int b = 0; b < Bc0; ++b) {
      const int t = maps[b], v = maps[Bc0 + b];
      if (t < 0 || t >= sets->n_text || v < 0 || v >= sets->n_vis) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_sets: set index out of range");
      t_half = t_half && t == b / pl->clips;
      v_half = v_half && v == b / pl->clips;
    }
    n_text = sets->n_text;
    n_vis = sets->n_vis;
    t_rows = !t_half;
    v_rows = !v_half;
    if (v_rows && Bc0 > 32) return FAIL(FOLEY_ERR_INVALID, "foley_prepare_sets: per-clip visual features take at most 32 batch rows");
  }
  if (tl) n_text = tl->n_text;   // validated by foley_prepare_timeline
  const int D = f.hidden, H = f.heads, C = f.latent_dim, T = f.compute_dtype;
  const size_t es = esize(T);
  const int ncfg = pl->ncfg, clips = pl->clips, La = pl->La, Lv = pl->Lv, Ls = pl->Ls, Lt = pl->Lt;
  const int Bc = ncfg * clips, M = Bc * La, Mv = Bc * Lv, S = La + Lv, NI = pl->n_iter;
  RunLayout slots;   // the part of the layout that sizes the workspace
  slots.sets = sets != nullptr; slots.t_rows = t_rows; slots.v_rows = v_rows;
  slots.th = t_rows ? Bc : ncfg; slots.vh = v_rows ? Bc : ncfg;
  slots.tdiv = Bc / slots.th; slots.vdiv = Bc / slots.vh;
  if (tl) { slots.th = n_text; slots.tdiv = 1; }   // one slot per text set; the timeline kernel addresses them through its tables
  slots.Sp = pad32(S); slots.Lap = pad32(La); slots.Ltp = pad32(Lt);
  slots.smod_ld = (long)f.depth_single * 6 * D;
  HIPTRY(hipStreamSynchronize(st));
  const bool reuse = c->buf.complete() && same_dims(c->plan, *pl) && c->layout.sets == slots.sets &&
                     c->layout.t_rows == slots.t_rows && c->layout.v_rows == slots.v_rows && c->ws_tl_sets == (tl ? n_text : 0);
  if (!reuse) ctx_free_plan(c);
  c->prepared = false;
  c->opt = RunOptions{};            // a plan without foley_set_* calls is a plain run (a timeline sets its set count below)
  RunLayout& ly = (c->layout = slots);   // the sync-token part follows below; complete where `prepared` is set
  c->vis_src = n_vis;
  const int th = ly.th, vh = ly.vh;
  const int hidmax = f.mlp_hidden > f.conv_hidden ? f.mlp_hidden : f.conv_hidden;
  const int Lmax = std::max(std::max(La, Lv), Lt);
  const int rl[3] = {La, Lv, Lmax};   // rows of the rotation tables rot_*[k]
  const int rsets = sets ? Bc : tl ? std::max(ncfg, n_text) : ncfg;   // set maps: sized for the most sets a plan of these dimensions can carry
  const int rmax = std::max(std::max(NI, rsets * Lt), std::max(rsets * Lv, rsets * Ls));
  // widest row any precompute stage writes into the scratch (every configurable feature width)
  const size_t tcols = std::max({D, f.sync_hidden, f.cond_dim, f.clip_dim, f.sync_dim, f.time_freq_dim});

  // the plan's lookup tables, copied below so that captured kernels keep valid addresses
#define PLAN_TABLES(X)                                                                                          \
  X(rope_cos, (size_t)pl->rope_len * 64 * 4) X(rope_sin, (size_t)pl->rope_len * 64 * 4) X(solver_coef, (size_t)NI * 8 * 4) \
  X(pos_audio_self, (size_t)La * 4) X(pos_visual_self, (size_t)Lv * 4) X(pos_linear, (size_t)Lmax * 4) X(sync_gather, (size_t)La * 4)
#define ALLOC(ptr, bytes) TRY(ctx_alloc(c, (bytes), (void**)&(ptr)))
#define ALLOCTAB(field, bytes) ALLOC(c->buf.field, bytes);
  if (!reuse) {
    ALLOC(c->buf.vec_table, (size_t)NI * D * 4);
    ALLOC(c->buf.modtab, (size_t)f.depth_triple * 2 * NI * 9 * D * 4);
    ALLOC(c->buf.txt_k, (size_t)f.depth_triple * th * H * Lt * 128 * es);
    const size_t txt_v_bytes = (size_t)f.depth_triple * th * H * ly.Ltp * 128 * es, V_bytes = (size_t)Bc * H * ly.Sp * 128 * es;
    ALLOC(c->buf.txt_v, txt_v_bytes);
    HIPTRY(hipMemsetAsync(c->buf.txt_v, 0, txt_v_bytes, st));
    ALLOC(c->buf.v_cond0, (size_t)vh * Lv * D * 4);
    ALLOC(c->buf.sync_tok, (size_t)vh * Ls * D * 4);
    if (sets) ALLOC(c->buf.set_idx, (size_t)Bc * (Lt + Ls + 8) * 4);
    if (v_rows) ALLOC(c->buf.sync_lead_rows, (size_t)Bc * 8 * D * 4);
    if (t_rows) ALLOC(c->buf.tG, (size_t)Bc * Lt * 2 * D * 4);
    ALLOC(c->buf.flag, 256);
    ALLOC(c->buf.xin, (size_t)M * C * es);
    ALLOC(c->buf.audio, (size_t)M * D * 4);
    ALLOC(c->buf.vcond, (size_t)Mv * D * 4);
    ALLOC(c->buf.xn_a, (size_t)M * D * es);
    ALLOC(c->buf.xn_v, (size_t)Mv * D * es);
    ALLOC(c->buf.qkv_a, (size_t)M * 3 * D * 4);
    ALLOC(c->buf.qkv_v, (size_t)Mv * 3 * D * 4);
    ALLOC(c->buf.Q, (size_t)Bc * H * S * 128 * es);
    ALLOC(c->buf.K, (size_t)Bc * H * S * 128 * es);
    ALLOC(c->buf.V, V_bytes);
    HIPTRY(hipMemsetAsync(c->buf.V, 0, V_bytes, st));  // V^T pad stays finite
    ALLOC(c->buf.att_a, (size_t)M * D * es);
    ALLOC(c->buf.att_v, (size_t)Mv * D * es);
    ALLOC(c->buf.hid_a, (size_t)M * hidmax * es);
    ALLOC(c->buf.hid_v, (size_t)Mv * f.mlp_hidden * es);
    ALLOC(c->buf.svec, (size_t)vh * Ls * D * es);
    ALLOC(c->buf.smod, (size_t)f.depth_single * vh * Ls * 6 * D * 4);
    ALLOC(c->buf.pred, (size_t)M * C * 4);
    ALLOC(c->buf.part_a, (size_t)PART_CAP * M * D * 4);     // sized for fp32 slabs; 16-bit slabs (slab16()) use half of it
    ALLOC(c->buf.part_v, (size_t)PART_CAP * Mv * D * 4);
    ALLOC(c->buf.x_saved, (size_t)clips * C * La * 4);
    ALLOC(c->buf.d_acc, (size_t)clips * C * La * 4);
    ALLOC(c->buf.x_cur, (size_t)clips * C * La * 4);
    ALLOC(c->buf.step_ctr, 256);
    PLAN_TABLES(ALLOCTAB)
    ALLOC(c->buf.rep_idx, (size_t)(v_rows ? Bc : clips) * Lv * 4);
    for (int k = 0; k < 3; ++k) {
      ALLOC(c->buf.rot_cos[k], (size_t)rl[k] * 64 * 4);
      ALLOC(c->buf.rot_sin[k], (size_t)rl[k] * 64 * 4);
    }
    if (!v_rows) {
      std::vector<int> idx((size_t)clips * Lv);
      for (size_t j = 0; j < idx.size(); ++j) idx[j] = (int)(j % Lv);
      HIPTRY(hipMemcpy(c->buf.rep_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    }
    // scratch of the precompute
    ALLOC(c->buf.tA, (size_t)rmax * tcols * es);
    ALLOC(c->buf.tB, (size_t)rmax * tcols * es);
    ALLOC(c->buf.tF, (size_t)rmax * 2 * D * 4);
  }
  if (sets) {
    // per-row gather tables: text K/V rows (row b, token t) <- set text_of[b]; sync token rows and the visual stream's start
    // rows (rep_idx, read by every forward) <- set vis_of[b].  Copied while nothing on `st` reads them (synchronised above).
    std::vector<int> idx((size_t)Bc * (Lt + Ls));
    for (int b = 0; b < Bc; ++b) {
      for (int t = 0; t < Lt; ++t) idx[(size_t)b * Lt + t] = maps[b] * Lt + t;
      for (int s = 0; s < Ls; ++s) idx[(size_t)Bc * Lt + (size_t)b * Ls + s] = maps[Bc + b] * Ls + s;
    }
    HIPTRY(hipMemcpy(c->buf.set_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    if (v_rows) {
      std::vector<int> rep((size_t)Bc * Lv);
      for (int b = 0; b < Bc; ++b)
        for (int j = 0; j < Lv; ++j) rep[(size_t)b * Lv + j] = maps[Bc + b] * Lv + j;
      HIPTRY(hipMemcpy(c->buf.rep_idx, rep.data(), rep.size() * 4, hipMemcpyHostToDevice));
    }
  }
  c->set_maps = std::move(maps);
  c->ws_tl_sets = tl ? n_text : 0;
  if (tl) {
    // the per-token tables, copied while nothing on `st` reads them (synchronised above); the buffers only grow, so a timeline of
    // the same shape keeps their addresses and with them the captured graph
    const size_t nb = (size_t)Bc * S * 4;
    TRY(grow(c->tl_a, nb));
    TRY(grow(c->tl_b, nb));
    TRY(grow(c->tl_alpha, nb));
    HIPTRY(hipMemcpy(c->tl_a.p, tl->set_a, nb, hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(c->tl_b.p, tl->set_b, nb, hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(c->tl_alpha.p, tl->alpha, nb, hipMemcpyHostToDevice));
    c->opt.tl_sets = n_text;
  }
  c->plan = *pl;
#define COPYTAB(field, bytes) \
  HIPTRY(hipMemcpyAsync((void*)c->buf.field, pl->field, (bytes), hipMemcpyDeviceToDevice, st)); \
  c->plan.field = c->buf.field;
  PLAN_TABLES(COPYTAB)
#undef COPYTAB
#undef PLAN_TABLES
  pl = &c->plan;
  const int* pt[3] = {pl->pos_audio_self, pl->pos_visual_self, pl->pos_linear};
  for (int k = 0; k < 3; ++k) {
    TRY(launch_gather_rows(pl->rope_cos, pt[k], rl[k], 1, pl->rope_len, 64, c->buf.rot_cos[k], st));
    TRY(launch_gather_rows(pl->rope_sin, pt[k], rl[k], 1, pl->rope_len, 64, c->buf.rot_sin[k], st));
  }
  HIPTRY(hipMemsetAsync(c->buf.step_ctr, 0, 256, st));
  void *tA = c->buf.tA, *tB = c->buf.tB;
  float* tF = c->buf.tF;

  // 1. time embedding table: t_feat -> Linear -> SiLU -> Linear   (embed_layers.py:104-136)
  Lin time0, time2;
  TRY(get_lin(c, "time0", T, D, f.time_freq_dim, true, &time0));
  TRY(get_lin(c, "time2", T, D, D, true, &time2));
  TRY(launch_cast(pl->t_feat, FOLEY_F32, tA, T, (long)NI * f.time_freq_dim, st));
  TRY(launch_gemm(gemm_plain(tA, NI, time0, tB, D), T, EPI_SILU_T, 0, st));
  TRY(launch_gemm(gemm_plain(tB, NI, time2, c->buf.vec_table, D), T, EPI_STORE_F32, 0, st));

  // 2. AdaLN tables of the triple blocks: Linear(SiLU(vec)) for every iteration (modulate_layers.py:15-16)
  TRY(launch_rows_add_act(c->buf.vec_table, rb_none(), NI, D, 1, tA, T, st));
  for (int b = 0; b < f.depth_triple; ++b)
    for (int s = 0; s < 2; ++s) {
      Lin m;
      TRY(get_lin(c, "t" + std::to_string(b) + (s ? ".v_mod" : ".a_mod"), T, 9 * D, D, true, &m));
      float* dst = c->buf.modtab + ((size_t)(b * 2 + s) * NI) * 9 * D;
      TRY(launch_gemm(gemm_plain(tA, NI, m, dst, 9 * D), T, EPI_STORE_F32, 0, st));
    }

  // 3. text: cond_in, then per block text_cross_kv -> k RMSNorm + RoPE (hifi_foley.py:289-308, 765)
  {
    Lin c1, c2;
    TRY(get_lin(c, "cond1", T, D, f.cond_dim, true, &c1));
    TRY(get_lin(c, "cond2", T, D, D, true, &c2));
    TRY(launch_cast(pl->text, FOLEY_F32, tA, T, (long)n_text * Lt * f.cond_dim, st));
    TRY(launch_gemm(gemm_plain(tA, n_text * Lt, c1, tB, D), T, EPI_SILU_T, 0, st));
    TRY(launch_gemm(gemm_plain(tB, n_text * Lt, c2, tA, D), T, EPI_STORE_T, 0, st));  // tA = cond embedding
    for (int b = 0; b < f.depth_triple; ++b) {
      Lin kv;
      const void* kn;
      TRY(get_lin(c, "t" + std::to_string(b) + ".t_kv", T, 2 * D, D, true, &kv));
      TRY(get_tensor(c, "t" + std::to_string(b) + ".t_kn", FOLEY_F32, {128}, &kn));
      TRY(launch_gemm(gemm_plain(tA, n_text * Lt, kv, tF, 2 * D), T, EPI_STORE_F32, 0, st));
      // per-row layout: the distinct sets' K/V rows are gathered into one set per batch row before the head split
      if (t_rows) TRY(launch_gather_rows(tF, c->buf.set_idx, Bc * Lt, 1, n_text * Lt, 2 * D, c->buf.tG, st));
      const bool vt = foley_is_half(T);
      void* dst[3] = {(char*)c->buf.txt_k + (size_t)b * th * H * Lt * 128 * es,
                      (char*)c->buf.txt_v + (size_t)b * th * H * (vt ? ly.Ltp : Lt) * 128 * es, nullptr};
      TRY(launch_qkv_split(qkv_split_args(c, t_rows ? c->buf.tG : tF, th * Lt, Lt, 2, (const float*)kn, nullptr, 2, false, dst, Lt, 0,
                                          vt ? ly.Ltp : 0, 1e-6f), st));
    }
  }

  // 4. visual stream input: SwiGLU projection (activation_layers.py:43-44, hifi_foley.py:770)
  {
    Lin w13, w2;
    TRY(get_lin(c, "vis.w13", T, 2 * D, f.clip_dim, false, &w13));
    TRY(get_lin(c, "vis.w2", T, D, D, false, &w2));
    TRY(launch_cast(pl->clip, FOLEY_F32, tA, T, (long)n_vis * Lv * f.clip_dim, st));
    TRY(launch_gemm(gemm_plain(tA, n_vis * Lv, w13, tB, D), T, EPI_SILUGATE_T, 0, st));
    TRY(launch_gemm(gemm_plain(tB, n_vis * Lv, w2, c->buf.v_cond0, D), T, EPI_STORE_F32, 0, st));
  }

  // 5. sync features: + pos emb, Linear, SiLU, ConvMLP(k=1), nearest-exact up-sampling (hifi_foley.py:755-762)
  {
    Lin s0, w13, w2;
    const void* pos;
    TRY(get_lin(c, "sync0", T, D, f.sync_dim, true, &s0));
    TRY(get_lin(c, "sync.w13", T, 2 * f.sync_hidden, D, false, &w13));
    TRY(get_lin(c, "sync.w2", T, D, f.sync_hidden, false, &w2));
    TRY(get_tensor(c, "sync_pos", FOLEY_F32, {8, f.sync_dim}, &pos));
    TRY(launch_add_periodic(pl->sync, (const float*)pos, n_vis * Ls, f.sync_dim, 8, tA, T, st));
    TRY(launch_gemm(gemm_plain(tA, n_vis * Ls, s0, tB, D), T, EPI_SILU_T, 0, st));
    TRY(launch_gemm(gemm_plain(tB, n_vis * Ls, w13, tA, f.sync_hidden), T, EPI_SILUGATE_T, 0, st));
    // The up-sampling to the audio frame rate is not materialised: consumers address the Ls token rows
    // through RowBcast mode 2 (common.h), so everything derived from the tokens alone - SiLU(token + vec)
    // and the single-stream blocks' modulation GEMM - runs on ncfg*Ls rows instead of ncfg*La.
    // Per-row layout: the distinct sets' token rows are gathered into one half per batch row.
    TRY(launch_gemm(gemm_plain(tA, n_vis * Ls, w2, v_rows ? tF : c->buf.sync_tok, D), T, EPI_STORE_F32, 0, st));
    if (v_rows) TRY(launch_gather_rows(tF, c->buf.set_idx + (size_t)Bc * Lt, Bc * Ls, 1, n_vis * Ls, D, c->buf.sync_tok, st));
    // Empty sync features (text-to-audio; the unconditional half of a CFG pair) are one learned row plus
    // sync_pos_emb, which repeats every 8 tokens: the token rows are then 8-periodic and the per-token work of the
    // single-stream blocks only has 8 distinct rows per half.  Detected on the data (bit patterns), not assumed.
    // One flag per cfg half: under CFG a video clip's unconditional half carries the empty features (periodic) next to the dense
    // conditional half - the modulation GEMM then runs on 8 + Ls rows instead of 2 Ls (round 5).
    // (per-row layout: one "half" per batch row, the unconditional rows first)
    if (vh > 32) return FAIL(FOLEY_ERR_INVALID, "more than 32 cfg halves");
    HIPTRY(hipMemsetAsync(c->buf.flag, 0, 4 * 32, st));
    TRY(launch_rows_periodic_check(c->buf.sync_tok, vh, Ls, 8, D, c->buf.flag, st));
  }
  HIPTRY(hipStreamSynchronize(st));
  {
    int differs[32];
    HIPTRY(hipMemcpy(differs, c->buf.flag, 4 * 32, hipMemcpyDeviceToHost));
    int lead = 0;
    while (Ls > 8 && lead < vh && !differs[lead]) ++lead;
    ly.lead = lead;
    ly.per = lead > 0 ? 8 : 0;
    ly.allper = lead > 0 && lead == vh;
    ly.R = lead * ly.per + (vh - lead) * Ls;
    ly.P = ly.allper ? ly.per : Ls;   // hoisting serves the all-periodic case
    ly.smod_step = (long)vh * ly.P * ly.smod_ld;
    if (v_rows && lead > 1) {   // pack the leading periodic halves' rows (st is idle: synchronised above)
      std::vector<int> idx((size_t)lead * 8);
      for (int h = 0; h < lead; ++h)
        for (int r = 0; r < 8; ++r) idx[(size_t)h * 8 + r] = h * Ls + r;
      int* lead_idx = c->buf.set_idx + (size_t)Bc * (Lt + Ls);
      HIPTRY(hipMemcpy(lead_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
      TRY(launch_gather_rows(c->buf.sync_tok, lead_idx, lead * 8, 1, vh * Ls, D, c->buf.sync_lead_rows, st));
    }
  }
  if (!c->fw.ok) TRY(resolve_forward_weights(c));
  {
    // 6. The single-stream blocks' modulation, Linear(SiLU(add_sync + vec)) (hifi_foley.py:366, 866-867), depends on the loop
    // iteration only (vec) and on the sync tokens - not on the latents.  Like the two-stream blocks' AdaLN tables it is therefore
    // computed HERE for all n_iter iterations in one GEMM ([n_iter*ncfg*P, D] x [n_single*6D, D]^T; the 1.02 GB weight panel is
    // streamed once per run instead of once per iteration: 0.21 ms x 50 -> ~1 ms at 5 s text-to-audio) when the table fits
    // SMOD_TABLE_CAP (1.06 GB for the 16 distinct rows of text-to-audio, 14.9 GB for the 224 rows of a 5 s video clip); longer
    // clips keep the per-iteration GEMM of run_forward.
    constexpr size_t SMOD_TABLE_CAP = (size_t)24 << 30;   // 24 GiB
    const int P = ly.P;
    const size_t tab_bytes = (size_t)NI * ly.smod_step * 4;
    // ... and only where the weight stream is what the per-iteration GEMM costs (a few distinct rows: the 8-periodic empty sync
    // features).  With the 224 dense rows of a video clip the batched GEMM costs what the 50 small ones do (18.3 vs 19 ms).
    bool hoist = f.depth_single > 0 && vh * P <= 64 && tab_bytes <= SMOD_TABLE_CAP;
    const size_t svec_bytes = (size_t)NI * vh * Ls * D * es;
    if (hoist) {
      // ... and only while the tables (they scale with n_iter: 1.06 GB at 50 steps, 4.2 GB at 200) take at most half of what the
      // device has free, counting what this context already holds - every data-parallel replica keeps its own
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { hipGetLastError(); free_b = 0; }
      const size_t held = c->smod_tab.bytes + c->svec_tab.bytes;
      if (tab_bytes + svec_bytes > held && (tab_bytes + svec_bytes - held) > free_b / 2) hoist = false;
    }
    if (hoist && (grow(c->smod_tab, tab_bytes) != 0 || grow(c->svec_tab, svec_bytes) != 0)) {
      hipGetLastError();     // allocation failed: not an error - the per-iteration GEMM of run_forward is still there
      hoist = false;
    }
    if (!hoist && (c->smod_tab.p || c->svec_tab.p)) {   // a plan that does not hoist gives the tables back
      HIPTRY(hipStreamSynchronize(st));
      release(c->smod_tab);
      release(c->svec_tab);
    }
    if (hoist) {
      for (int it = 0; it < NI; ++it)
        TRY(launch_rows_add_act(c->buf.sync_tok, rb_vec(c->buf.vec_table + (size_t)it * D, 0, nullptr), vh * Ls, D, 1,
                                (char*)c->svec_tab.p + (size_t)it * vh * Ls * D * es, T, st));
      GemmArgs gm = gemm_plain(c->svec_tab.p, NI * vh * P, c->fw.smod, c->smod_tab.p, ly.smod_ld);
      gm.segV = P; gm.segS = Ls;     // virtual rows: row r of the product is token r % P of (iteration, half) r / P
      TRY(launch_gemm(gm, T, EPI_STORE_F32, 0, st));
    }
    // the table the blocks read: hoisted, or run_forward's of this iteration with the leading halves' 8 rows packed
    ly.hoisted = hoist;
    ly.mod_per = (ly.allper || !hoist) ? ly.per : 0;
    ly.mod_lead = ly.allper ? -1 : ly.lead;
  }
  {
    // the plan's table must be the nearest-exact map the kernels compute in their addressing
    std::vector<int> tab((size_t)La);
    HIPTRY(hipMemcpy(tab.data(), pl->sync_gather, (size_t)La * 4, hipMemcpyDeviceToHost));
    const float scale = (float)Ls / (float)La;
    for (int l = 0; l < La; ++l)
      if (tab[l] != rb_nearest_exact(l, scale, Ls)) return FAIL(FOLEY_ERR_INVALID, "plan.sync_gather is not the nearest-exact up-sampling table");
  }
  c->prepared = true;
  return 0;
}

// --------------------------------------------------------------------------- DiT forward
static RowBcast rb_vec(const float* base, long step_stride, const int* step_ptr) {
  return RowBcast{base, 0, 0, 1, 1, step_ptr, step_stride};
}
static RowBcast rb_tok(const float* base, long ld, int rows_per_cfg, int L) {
  return RowBcast{base, ld, 1, rows_per_cfg, L, nullptr, 0, 0, 0.f, 0};
}
// operand with Ls rows per cfg, read by audio frame l at its nearest-exact source row (common.h RowBcast mode 2)
// per > 0: the first `lead` cfg halves store `per` rows each (8-periodic token rows), the others all Ls rows behind them;
// lead < 0: every half periodic
static RowBcast rb_up(const float* base, long ld, int rows_per_cfg, int L, int Ls, int per = 0, int lead = -1) {
  RowBcast r{base, ld, 2, rows_per_cfg, L, nullptr, 0, Ls, (float)Ls / (float)L, per, 0, 0};
  if (per > 0) {
    r.dense_from = lead < 0 ? INT_MAX : lead;
    r.dense_base = lead < 0 ? 0 : lead * per;
  }
  return r;
}

// Per-kernel profile (foley_profile_forward): the op's kernel launch carries two events as its own
// start / stop timestamps (common.h FOLEY_LAUNCH), tagged with the op's algorithmic FLOPs / bytes.
static int prof_begin(foley_ctx* c, hipStream_t st, const char* label, double flop, double bytes) {
  if (!c->prof.on) return 0;
  ProfRec r{label, flop, bytes, c->prof.get(), c->prof.get(), nullptr};
  c->prof.recs.push_back(r);
  g_foley_prof = FoleyProfHook{r.e0, r.e1, nullptr};   // consumed by the op's (first) kernel launch
  return 0;
}
static int prof_end(foley_ctx* c, hipStream_t st) {
  if (!c->prof.on) return 0;
  if (g_foley_prof.e0) {   // the op launched nothing: keep the record well-formed with a plain (empty) bracket
    g_foley_prof.e0 = nullptr;
    HIPTRY(hipEventRecord(c->prof.recs.back().e0, st));
    HIPTRY(hipEventRecord(c->prof.recs.back().e1, st));
  } else {
    c->prof.recs.back().fn = g_foley_prof.fn;
  }
  return 0;
}
#define PROF(label, flop, bytes, call)            \
  do {                                            \
    TRY(prof_begin(c, st, (label), (flop), (bytes))); \
    TRY(call);                                    \
    TRY(prof_end(c, st));                         \
  } while (0)

// The single-block modulation GEMM (510 GFLOP, depends on the iteration index only) runs IN LINE at the head
// of the forward.  Round 1 overlapped it with the two-stream blocks on a side stream; with the faster block
// kernels of round 2 its 5184 workgroups only steal CUs from them (A/B in one box: 448.5 -> 439.5 ms per
// 50-iteration loop at bs=1, 1753 -> 1741 ms at bs=8).
// `part` (step cache): FWD_ALL is the straight line - the launches below in their order, whenever the cache is off.  Under the
// cache an iteration is FWD_HEAD (audio_embedder, then the probe of the first block's modulated input), and
// either FWD_BODY (everything else; foley_sample then takes delta = aN - a0) or, on a skipped iteration, audio += delta and
// FWD_FINAL (final.layernorm + final.linear, nothing pending).  The single blocks' per-iteration modulation section belongs to the
// body; without two-stream blocks the probe reads its table, so it then runs in the head.
enum FwdPart { FWD_ALL = 0, FWD_HEAD, FWD_BODY, FWD_FINAL };

static int run_forward(foley_ctx* c, hipStream_t st, FwdPart part = FWD_ALL) {
  const foley_config& f = c->cfg;
  const foley_plan& pl = c->plan;
  const ForwardW& W = c->fw;
  if (!W.ok) return FAIL(FOLEY_ERR_STATE, "forward weights are not resolved (foley_prepare)");
  // one clip per CFG half: the small-grid GEMMs may rotate their K origin per M tile (GemmArgs::krot_ok) - with several clips
  // in the batch, clips with equal noise must stay bit-identical, so their rows keep one summation order
  auto krot = [&pl](GemmArgs g) {
    g.krot_ok = pl.clips == 1 ? 1 : 0;
    return g;
  };
  const int D = f.hidden, H = f.heads, C = f.latent_dim, T = f.compute_dtype;
  const int ncfg = pl.ncfg, clips = pl.clips, La = pl.La, Lv = pl.Lv, Ls = pl.Ls, Lt = pl.Lt, NI = pl.n_iter;
  const int Bc = ncfg * clips, M = Bc * La, Mv = Bc * Lv, S = La + Lv;
  const RunLayout& ly = c->layout;
  const IterArgs ia = iter_args(c);   // the probe's buffers and the timeline's tables
  const int th = ly.th, vh = ly.vh, lead = ly.lead;
  const bool bf = foley_is_half(T);   // 16-bit throughput mode (bf16 or fp16 operands): transposed V, fused head split
  const size_t es = esize(T);
  const int* sp = c->buf.step_ctr;
  void* const qkv_dst[3] = {c->buf.Q, c->buf.K, c->buf.V};
  // algorithmic work of one launch (profile labels): dense contraction FLOPs, operand + result bytes
  auto gf = [](double m, double n, double k) { return 2.0 * m * n * k; };
  auto gb = [&](double m, double n, double k, double out_es) { return (m * k + n * k) * (double)es + m * n * out_es; };
  auto af = [&](double b, double sq, double skv) { return 4.0 * b * H * sq * skv * 128.0; };
  auto ab = [&](double b, double sq, double skv) { return (2.0 * b * H * sq * 128.0 + 2.0 * b * H * skv * 128.0) * (double)es; };

  // ---- per-token conditioning of the single-stream blocks, SiLU(add_sync + vec) (hifi_foley.py:866-867),
  // and every single block's modulation GEMM (hifi_foley.py:366).  They depend on the iteration only, are
  // identical for every clip of a CFG half, and - add_sync being an up-sampling of the Ls sync tokens - have
  // only Ls distinct rows per half: M = ncfg*Ls (224 instead of 500 at 5 s).
  // which piece the single blocks' modulation section runs in: the body - or the head, when the probe reads its table
  const FwdPart smod_part = f.depth_triple == 0 ? FWD_HEAD : FWD_BODY;
  if (!ly.hoisted && (part == FWD_ALL || part == smod_part)) {
    // distinct rows only: 8 per 8-periodic half (the leading halves), Ls per dense half - packed back to back (RunLayout::R)
    if (ly.v_rows && lead > 1)   // per-row layout: the leading halves' rows were packed by foley_prepare_sets - one launch
      TRY(launch_rows_add_act(c->buf.sync_lead_rows, rb_vec(c->buf.vec_table, D, sp), lead * ly.per, D, 1, c->buf.svec, T, st));
    else
      for (int h = 0; h < lead; ++h)
        TRY(launch_rows_add_act(c->buf.sync_tok + (size_t)h * Ls * D, rb_vec(c->buf.vec_table, D, sp), ly.per, D, 1,
                                (char*)c->buf.svec + (size_t)h * ly.per * D * es, T, st));
    if (lead < vh)
      TRY(launch_rows_add_act(c->buf.sync_tok + (size_t)lead * Ls * D, rb_vec(c->buf.vec_table, D, sp), (vh - lead) * Ls, D, 1,
                              (char*)c->buf.svec + (size_t)lead * ly.per * D * es, T, st));
    if (f.depth_single > 0) {
      const double n = (double)ly.smod_ld;   // one GEMM for all blocks: [R, D] x [n_single*6D, D]^T -> smod [R, n_single*6D]
      GemmArgs gm = krot(gemm_plain(c->buf.svec, ly.R, W.smod, c->buf.smod, ly.smod_ld));
      PROF("single.modulation (all blocks, one GEMM)", gf(ly.R, n, D), gb(ly.R, n, D, 4), launch_gemm(gm, T, EPI_STORE_F32, 0, st));
    }
  }

  // audio_embedder (conv k=1 == linear over the transposed latents) + add_sync (hifi_foley.py:768, 838-839)
  if (part == FWD_ALL || part == FWD_HEAD) {
    GemmArgs g = krot(gemm_plain(c->buf.xin, M, W.audio_in, c->buf.audio, D));
    g.rb = rb_up(c->buf.sync_tok, D, ly.vdiv * La, La, Ls);
    PROF("audio_embedder", gf(M, D, C), gb(M, D, C, 4), launch_gemm(g, T, EPI_STORE_F32, 0, st));
  }
  // the single blocks' modulation rows (RunLayout): every half periodic (8 rows each) | the leading halves periodic, the others
  // dense (the per-iteration GEMM only) | every half dense
  auto sm_of = [&](int blk, int chunk) {
    const float* smod_b = (ly.hoisted ? (const float*)c->smod_tab.p : c->buf.smod) + (size_t)blk * 6 * D;   // column block of the fused table
    RowBcast r = rb_up(smod_b + (size_t)chunk * D, ly.smod_ld, ly.vdiv * La, La, Ls, ly.mod_per, ly.mod_lead);
    if (ly.hoisted) {   // the table of every iteration: this iteration's rows start at step * smod_step
      r.step_ptr = sp;
      r.step_stride = ly.smod_step;
    }
    return r;
  };
  if (part == FWD_HEAD) {
    // step cache probe: exactly the eps and operands the first block's first LayerNorm gets below
    const bool tri = f.depth_triple > 0;
    auto tb0 = [&](int chunk) { return rb_vec(c->buf.modtab + (size_t)chunk * D, 9L * D, sp); };
    TRY(launch_cache_probe(c->buf.audio, Bc, La, D, tri ? 1e-6f : 1e-5f, tri ? tb0(0) : sm_of(0, 0), tri ? tb0(1) : sm_of(0, 1),
                           ia.sc_mprev, ia.sc_part, ia.sc_rel, st));
    return 0;
  }
  // FinalLayer1D: adaLN is a no-op with 3-D conditioning => linear(LayerNorm(x)); the LayerNorm applies what the last
  // gated-residual GEMM left pending
  auto final_layer = [&](const LnPending& pending) -> int {
    PROF("final.layernorm", 0.0, (double)M * D * (4 + 4 + es),
         launch_ln_mod_pending(c->buf.audio, M, D, 1e-6f, rb_none(), rb_none(), c->buf.xn_a, T, pending, st));
    PROF("final.linear", gf(M, C, D), gb(M, C, D, 4), launch_gemm(krot(gemm_plain(c->buf.xn_a, M, W.fin, c->buf.pred, C)), T, EPI_STORE_F32, 0, st));
    return 0;
  };
  if (part == FWD_FINAL) return final_layer(LnPending{});
  // visual stream starts from the step-invariant projection, replicated per clip (one gather launch); per-row layout: every
  // batch row gathers its own set's rows of the distinct projections
  if (ly.v_rows)
    TRY(launch_gather_rows(c->buf.v_cond0, c->buf.rep_idx, Bc * Lv, 1, c->vis_src * Lv, D, c->buf.vcond, st));
  else
    TRY(launch_gather_rows(c->buf.v_cond0, c->buf.rep_idx, clips * Lv, ncfg, Lv, D, c->buf.vcond, st));

  // residual updates left pending by deferred split-K GEMMs, per stream (audio, visual); the next
  // LayerNorm of that stream applies them
  LnPending pend[2] = {LnPending{}, LnPending{}};
  // deferred split-K slabs in the operand type (bf16 / fp16 compute): half the bytes the GEMM epilogues write and the next
  // LayerNorm reads (that kernel runs at the fabric's bandwidth: 22 MB in 3.4 us at M = 500).  fp32 compute keeps fp32 slabs.
  const int slab_half = bf ? T : 0;
  auto with_partials = [&](GemmArgs& g, float* slabs) {
    g.partial_half = slab_half ? 1 : 0;
    g.partials = slabs;
    g.partial_stride = (long)g.M * g.N;
    g.partial_cap = PART_CAP;
  };
  const double ln_bytes_t = (double)(M + Mv) * D * (4 + 4 + es), ln_bytes_s = (double)M * D * (4 + 4 + es);
  for (int blk = 0; blk < f.depth_triple; ++blk) {
    const TripleW& w = W.t[blk];
    auto tb = [&](int s, int chunk) {
      return rb_vec(c->buf.modtab + ((size_t)(blk * 2 + s) * NI) * 9 * D + (size_t)chunk * D, 9L * D, sp);
    };
    struct Stream { float* x; void* xn; float* qkv; void* att; void* hid; int rows, L, tok_off; };
    Stream ss[2] = {{c->buf.audio, c->buf.xn_a, c->buf.qkv_a, c->buf.att_a, c->buf.hid_a, M, La, Lv},
                    {c->buf.vcond, c->buf.xn_v, c->buf.qkv_v, c->buf.att_v, c->buf.hid_v, Mv, Lv, 0}};
    // Both streams go through the same sequence of ops with their own weights; each op is ONE
    // launch covering the audio problem and the (much smaller) visual problem.
    auto ln2 = [&](int c_shift, int c_scale) -> int {
      LnArgs a0{ss[0].x, ss[0].rows, tb(0, c_shift), tb(0, c_scale), ss[0].xn, pend[0]};
      LnArgs a1{ss[1].x, ss[1].rows, tb(1, c_shift), tb(1, c_scale), ss[1].xn, pend[1]};
      pend[0] = pend[1] = LnPending{};
      PROF("triple.layernorm+modulate (+pending split-K sum)", 0.0, ln_bytes_t, launch_ln_mod_pair(a0, a1, D, 1e-6f, T, st));
      return 0;
    };
    auto gated2 = [&](const char* label, const Lin& la, const Lin& lv, bool from_hid, int c_gate) -> int {
      GemmArgs g0 = krot(gemm_plain(from_hid ? ss[0].hid : ss[0].att, ss[0].rows, la, ss[0].x, D));
      GemmArgs g1 = krot(gemm_plain(from_hid ? ss[1].hid : ss[1].att, ss[1].rows, lv, ss[1].x, D));
      g0.rb = tb(0, c_gate);
      g1.rb = tb(1, c_gate);
      with_partials(g0, c->buf.part_a);
      with_partials(g1, c->buf.part_v);
      int ks = 1;
      PROF(label, gf(M + Mv, la.N, la.K), gb(M + Mv, la.N, la.K, 4) + (double)la.N * la.K * es,
           launch_gemm_pair(g0, g1, T, EPI_GATE_RES, st, &ks));
      if (ks > 1) {
        pend[0] = LnPending{c->buf.part_a, ks, g0.partial_stride, la.b, g0.rb, slab_half};
        pend[1] = LnPending{c->buf.part_v, ks, g1.partial_stride, lv.b, g1.rb, slab_half};
      }
      return 0;
    };
    auto split_args = [&](int s, int nK, const float* gq, const float* gk, int rot) {   // of stream s into the joint Q/K/V
      return qkv_split_args(c, ss[s].qkv, ss[s].rows, ss[s].L, nK, gq, gk, rot, true, qkv_dst, S, ss[s].tok_off,
                            (bf && nK == 3) ? ly.Sp : 0, 1e-6f);
    };
    // 1. joint self attention (hifi_foley.py:215-269)
    {
      TRY(ln2(0, 1));
      GemmArgs g0 = krot(gemm_plain(ss[0].xn, ss[0].rows, w.qkv[0], ss[0].qkv, 3 * D));
      GemmArgs g1 = krot(gemm_plain(ss[1].xn, ss[1].rows, w.qkv[1], ss[1].qkv, 3 * D));
      g0.qs = split_args(0, 3, w.qn[0], w.kn[0], 0);
      g1.qs = split_args(1, 3, w.qn[1], w.kn[1], 1);
      PROF("triple.qkv GEMM + RMSNorm/RoPE head split", gf(M + Mv, 3 * D, D), gb(M + Mv, 3 * D, D, es) + 3.0 * D * D * es,
           launch_gemm_pair(g0, g1, T, EPI_QKV_SPLIT, st));   // head split fused into the projection
      AttnArgs a{c->buf.Q, c->buf.K, c->buf.V, Bc, H, S, S, 1, c->buf.att_v, c->buf.att_a, Lv, T, bf ? ly.Sp : 0};
      PROF("triple.self attention", af(Bc, S, S), ab(Bc, S, S), launch_attention(a, T, st));
      TRY(gated2("triple.self proj GEMM (gated residual)", w.proj[0], w.proj[1], false, 2));
    }
    // 2. cross attention to the (cached) text keys/values (hifi_foley.py:271-319)
    {
      TRY(ln2(3, 4));
      GemmArgs g0 = krot(gemm_plain(ss[0].xn, ss[0].rows, w.cq[0], ss[0].qkv, D));
      GemmArgs g1 = krot(gemm_plain(ss[1].xn, ss[1].rows, w.cq[1], ss[1].qkv, D));
      g0.qs = split_args(0, 1, w.cqn[0], nullptr, 2);
      g1.qs = split_args(1, 1, w.cqn[1], nullptr, 2);
      const int Ltp = ly.Ltp, tdiv = ly.tdiv;
      const size_t offk = (size_t)blk * th * H * Lt * 128 * es;
      const size_t offv = (size_t)blk * th * H * (bf ? Ltp : Lt) * 128 * es;
      // 16-bit modes: the projection may run the attention against the <= 96 cached text keys in its epilogue (small grids:
      // gemm_impl.h decides and reports through attn_fused); the q tensor and the attention launch are then gone
      int fused = 0;
      if (bf && Lt <= 96 && Ltp >= 96 && !ia.tl_sets) {   // a prompt timeline leaves attn_* unset: its own kernel follows
        for (int s = 0; s < 2; ++s) {
          QkvSplitArgs& q = s ? g1.qs : g0.qs;
          q.attn_k = (char*)c->buf.txt_k + offk; q.attn_vt = (char*)c->buf.txt_v + offv; q.attn_out = ss[s].att;
          q.attn_skv = Lt; q.attn_pitch = Ltp; q.attn_bdiv = tdiv; q.attn_fused = &fused;   // gemm_plan.h: <= 2 sets per tile
        }
      }
      PROF("triple.cross q GEMM + head split (+ cross attention on small grids)", gf(M + Mv, D, D),
           gb(M + Mv, D, D, es) + 1.0 * D * D * es, launch_gemm_pair(g0, g1, T, EPI_QKV_SPLIT, st));
      if (ia.tl_sets) {
        AttnTimelineArgs ta{c->buf.Q, (char*)c->buf.txt_k + offk, (char*)c->buf.txt_v + offv, ia.tl_a, ia.tl_b,
                            ia.tl_alpha, Bc, H, S, Lt, ia.tl_sets, c->buf.att_v, c->buf.att_a, Lv, T, bf ? Ltp : 0};
        PROF("triple.cross attention (prompt timeline)", 2.0 * af(Bc, S, Lt), 2.0 * ab(Bc, S, Lt), launch_attention_timeline(ta, T, st));
      } else if (!fused) {
        AttnArgs a{c->buf.Q, (char*)c->buf.txt_k + offk, (char*)c->buf.txt_v + offv, Bc, H, S, Lt, tdiv, c->buf.att_v, c->buf.att_a, Lv,
                   T, bf ? Ltp : 0};
        PROF("triple.cross attention", af(Bc, S, Lt), ab(Bc, S, Lt), launch_attention(a, T, st));
      }
      TRY(gated2("triple.cross proj GEMM (gated residual)", w.cproj[0], w.cproj[1], false, 5));
    }
    // 3. GELU-tanh MLPs (hifi_foley.py:321-331)
    {
      TRY(ln2(6, 7));
      PROF("triple.mlp fc1 GEMM + GELU", gf(M + Mv, f.mlp_hidden, D), gb(M + Mv, f.mlp_hidden, D, es) + (double)f.mlp_hidden * D * es,
           launch_gemm_pair(krot(gemm_plain(ss[0].xn, ss[0].rows, w.fc1[0], ss[0].hid, f.mlp_hidden)),
                            krot(gemm_plain(ss[1].xn, ss[1].rows, w.fc1[1], ss[1].hid, f.mlp_hidden)), T, EPI_GELU_T, st));
      TRY(gated2("triple.mlp fc2 GEMM (gated residual)", w.fc2[0], w.fc2[1], true, 8));
    }
  }

  const int Hc = f.conv_hidden;
  for (int blk = 0; blk < f.depth_single; ++blk) {
    const SingleW& w = W.s[blk];
    auto sm = [&](int chunk) { return sm_of(blk, chunk); };
    PROF("single.layernorm+modulate (+pending split-K sum)", 0.0, ln_bytes_s,
         launch_ln_mod_pending(c->buf.audio, M, D, 1e-5f, sm(0), sm(1), c->buf.xn_a, T, pend[0], st));
    pend[0] = LnPending{};
    GemmArgs gq = krot(gemm_plain(c->buf.xn_a, M, w.qkv, c->buf.qkv_a, 3 * D));
    gq.qs = qkv_split_args(c, c->buf.qkv_a, M, La, 3, w.qn, w.kn, 2, true, qkv_dst, La, 0, bf ? ly.Lap : 0,
                           1.1920928955078125e-07f);  // nn.RMSNorm(eps=None) -> finfo(fp32).eps
    PROF("single.qkv GEMM + RMSNorm/RoPE head split", gf(M, 3 * D, D), gb(M, 3 * D, D, es), launch_gemm(gq, T, EPI_QKV_SPLIT, 0, st));
    {
      AttnArgs a{c->buf.Q, c->buf.K, c->buf.V, Bc, H, La, La, 1, c->buf.att_a, c->buf.att_a, 0, T, bf ? ly.Lap : 0};
      PROF("single.self attention", af(Bc, La, La), ab(Bc, La, La), launch_attention(a, T, st));
    }
    {
      GemmArgs g = krot(gemm_conv(c->buf.att_a, M, La, D, 3, 1, w.lin1, c->buf.audio, D));
      g.rb = sm(2);
      with_partials(g, c->buf.part_a);
      int ks = 1;
      PROF("single.linear1 conv3 GEMM (gated residual)", gf(M, D, 3 * D), gb(M, D, 3 * D, 4), launch_gemm(g, T, EPI_GATE_RES, 0, st, &ks));
      if (ks > 1) pend[0] = LnPending{c->buf.part_a, ks, g.partial_stride, w.lin1.b, g.rb, slab_half};
    }
    PROF("single.layernorm+modulate (+pending split-K sum)", 0.0, ln_bytes_s,
         launch_ln_mod_pending(c->buf.audio, M, D, 1e-5f, sm(3), sm(4), c->buf.xn_a, T, pend[0], st));
    pend[0] = LnPending{};
    PROF("single.w1/w3 conv3 GEMM + SiLU gate", gf(M, 2 * Hc, 3 * D), gb(M, 2 * Hc, 3 * D, es) - (double)M * Hc * es,
         launch_gemm(krot(gemm_conv(c->buf.xn_a, M, La, D, 3, 1, w.w13, c->buf.hid_a, Hc)), T, EPI_SILUGATE_T, 0, st));
    {
      GemmArgs g = krot(gemm_conv(c->buf.hid_a, M, La, Hc, 3, 1, w.w2, c->buf.audio, D));
      g.rb = sm(5);
      with_partials(g, c->buf.part_a);
      int ks = 1;
      PROF("single.w2 conv3 GEMM (gated residual)", gf(M, D, 3 * Hc), gb(M, D, 3 * Hc, 4), launch_gemm(g, T, EPI_GATE_RES, 0, st, &ks));
      if (ks > 1) pend[0] = LnPending{c->buf.part_a, ks, g.partial_stride, w.w2.b, g.rb, slab_half};
    }
  }

  return final_layer(pend[0]);
}

// One eager forward of `latents` at loop iteration `iter` (foley_dit_forward, foley_profile_forward): the prediction is in buf.pred
static int forward_at(foley_ctx* c, const float* latents, int iter, hipStream_t st) {
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_prepare has not been called");
  if (iter < 0 || iter >= c->plan.n_iter) return FAIL(FOLEY_ERR_INVALID, "iteration out of range");
  HIPTRY(hipSetDevice(c->device));
  const foley_plan& pl = c->plan;
  HIPTRY(hipMemcpyAsync(c->buf.step_ctr, &iter, sizeof(int), hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));  // `iter` lives on the caller's stack
  TRY(launch_latent_rows(latents, pl.clips, c->cfg.latent_dim, pl.La, pl.ncfg, c->buf.xin, c->cfg.compute_dtype, st));
  return run_forward(c, st);
}

extern "C" int foley_dit_forward(foley_ctx* c, const float* latents, int iter, float* out_rows, void* stream_v) {
  if (!c || !latents || !out_rows) return FAIL(FOLEY_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream_v;
  TRY(forward_at(c, latents, iter, st));
  const foley_plan& pl = c->plan;
  HIPTRY(hipMemcpyAsync(out_rows, c->buf.pred, (size_t)pl.ncfg * pl.clips * pl.La * c->cfg.latent_dim * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

// --------------------------------------------------------------------------- per-kernel profile
// `repeats` eager forwards at loop iteration `iter`; every op's kernel is launched with start / stop
// events attached to the dispatch itself (hipExtLaunchKernelGGL on the launch stream), aggregated by
// op label - total_ms is kernel time proper, the quantity rocprofv3's kernel trace reports.
// bracket_ms = mean elapsed time of an EMPTY event bracket (two back-to-back hipEventRecord), reported
// for reference only: it is NOT contained in total_ms.
extern "C" int foley_profile_forward(foley_ctx* c, const float* latents, int iter, int repeats, foley_prof_entry* out,
                                     int cap, int* n_out, float* bracket_ms, void* stream_v) {
  if (!c || !latents || !out || !n_out || cap < 1 || repeats < 1) return FAIL(FOLEY_ERR_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream_v;
  TRY(forward_at(c, latents, iter, st));   // warm: code objects loaded, caches in their steady state
  c->prof.recs.clear();
  c->prof.used = 0;
  c->prof.on = true;
  int rc = 0;
  for (int r = 0; r < repeats && rc == 0; ++r) rc = run_forward(c, st);
  c->prof.on = false;
  g_foley_prof = FoleyProfHook{nullptr, nullptr, nullptr};   // an op that failed between prof_begin and its launch leaves the hook armed
  if (rc) return rc;
  // empty brackets for the calibration
  constexpr int NCAL = 32;
  hipEvent_t cal[2 * NCAL];
  for (int i = 0; i < 2 * NCAL; ++i) cal[i] = c->prof.get();
  for (int i = 0; i < NCAL; ++i) {
    HIPTRY(hipEventRecord(cal[2 * i], st));
    HIPTRY(hipEventRecord(cal[2 * i + 1], st));
  }
  HIPTRY(hipStreamSynchronize(st));
  double cal_ms = 0.0;
  for (int i = 0; i < NCAL; ++i) {
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, cal[2 * i], cal[2 * i + 1]));
    cal_ms += ms;
  }
  if (bracket_ms) *bracket_ms = (float)(cal_ms / NCAL);
  int n = 0;
  for (const ProfRec& r : c->prof.recs) {
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, r.e0, r.e1));
    int j = 0;
    for (; j < n; ++j)
      if (!strcmp(out[j].label, r.label)) break;
    if (j == n) {
      if (n == cap) return FAIL(FOLEY_ERR_INVALID, "profile: entry buffer too small");
      memset(&out[n], 0, sizeof(out[n]));
      strncpy(out[n].label, r.label, sizeof(out[n].label) - 1);
      if (r.fn) {   // the kernel's symbol, demangled - the name rocprofv3's kernel trace lists it under
        const char* mangled = hipKernelNameRefByPtr(r.fn, st);
        if (mangled) {
          int status = 0;
          char* dm = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
          strncpy(out[n].kernel, status == 0 && dm ? dm : mangled, sizeof(out[n].kernel) - 1);
          free(dm);
        }
      }
      ++n;
    }
    out[j].calls += 1;
    out[j].total_ms += ms;
    out[j].flop += r.flop;
    out[j].bytes += r.bytes;
  }
  *n_out = n;
  return 0;
}

// --------------------------------------------------------------------------- sampler loop
// The solver update of the prediction in buf.pred, as iter_args() states it (guided / edit / windows form, with or without
// history), behind the statistics of CFG rescale or the two launches of projected guidance: shared by the plain iteration and the
// two bodies of a cached one.
static int run_step(const IterArgs& a, hipStream_t st) {
  if (a.guid_scale) TRY(launch_guidance_stats(a.step, a.guid_part, a.guid_phi, 0.f, a.guid_scale, st));
  if (a.proj_mode) TRY(launch_guidance_project(a.step, a.proj_mode, a.proj_rows, a.proj_part, a.proj_coef, a.proj_plane, st));
  if (a.flowedit.z) return launch_flowedit_step(a.flowedit, st);   // a pair batch: the difference step, which stages both branches
  return launch_solver_step(a.step, st);
}

static int run_iteration(foley_ctx* c, hipStream_t st) {
  TRY(run_forward(c, st));
  return run_step(iter_args(c), st);
}

// The three pieces of an iteration under the step cache (each a linear captured graph): the head, the full body (a copy of a0 into
// the residual buffer - only now, the head runs before the decision and a skip needs the old delta -, the blocks, then delta =
// aN - a0 over that copy: the final LayerNorm has written the finished stream back) and the skip body.
enum { SC_HEAD = 0, SC_FULL = 1, SC_SKIP = 2 };
static int run_cached_piece(foley_ctx* c, int piece, hipStream_t st) {
  const long n = (long)c->plan.ncfg * c->plan.clips * c->plan.La * c->cfg.hidden;
  const IterArgs a = iter_args(c);
  if (piece == SC_HEAD) return run_forward(c, st, FWD_HEAD);
  if (piece == SC_FULL) {
    TRY(launch_cast(c->buf.audio, FOLEY_F32, a.sc_delta, FOLEY_F32, n, st));
    TRY(run_forward(c, st, FWD_BODY));
    TRY(launch_cache_delta(c->buf.audio, a.sc_delta, n, st));
    return run_step(a, st);
  }
  TRY(launch_cache_apply(c->buf.audio, a.sc_delta, n, st));
  TRY(run_forward(c, st, FWD_FINAL));
  return run_step(a, st);
}

// The skip policy of one loop (host/step_cache.py states the same machine in Python): iteration 0, the last one and any without a
// valid delta are full; schedule mode skips the listed iterations; threshold mode adds poly(rel) to `acc` on every measured
// iteration and skips while acc < threshold, inside [lo, hi) and below the cap on consecutive skips; a full iteration resets acc.
struct StepCachePolicy {
  double acc = 0.0;
  int run = 0;
  bool have_delta = false;
  bool decide(const RunOptions& o, int i, int n, float rel) {
    const bool forced = i == 0 || i == n - 1 || !have_delta;
    bool skip = false;
    if (o.sc_mode == FOLEY_STEP_CACHE_SCHEDULE) {
      skip = !forced && o.sc_skip[i] != 0;
    } else {
      if (i > 0) {
        double v = (double)rel;
        if (!o.sc_poly.empty()) {
          v = 0.0;
          for (double k : o.sc_poly) v = v * (double)rel + k;
        }
        acc += v;
      }
      skip = !forced && acc < o.sc_threshold && i >= o.sc_lo && i < o.sc_hi && (o.sc_maxc <= 0 || run < o.sc_maxc);
    }
    if (skip) {
      ++run;
    } else {
      acc = 0.0;
      run = 0;
      have_delta = true;
    }
    return skip;
  }
};

// The key of an iteration captured now: its launch operands, and what is not one.
static GraphKey graph_key_now(const foley_ctx* c) {
  return GraphKey{iter_args(c), c->set_maps, c->layout, c->smod_tab.p, c->tensor_gen, c->plan_gen};
}

extern "C" int foley_set_edit(foley_ctx* c, const float* x0, int x0_clips, const float* noise, const float* mask, int mask_clips,
                              void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_edit: foley_prepare has not been called");
  if (!x0 && !noise && !mask) {
    c->opt.edit = false;
    return 0;
  }
  if (!x0 || !noise) return FAIL(FOLEY_ERR_INVALID, "foley_set_edit: x0 and noise are required (all three null clears the edit state)");
  if (c->opt.n_win) return FAIL(FOLEY_ERR_INVALID, "foley_set_edit: the run has windows (foley_set_windows); editing a long clip is not supported");
  if (c->opt.flowedit) return FAIL(FOLEY_ERR_INVALID, "foley_set_edit: the run has a FlowEdit state (foley_set_flowedit); the two edits do not combine");
  const foley_plan& pl = c->plan;
  if (x0_clips != 1 && x0_clips != pl.clips) return FAIL(FOLEY_ERR_INVALID, "foley_set_edit: x0_clips must be 1 or the plan's clips");
  if (mask && mask_clips != 1 && mask_clips != pl.clips)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_edit: mask_clips must be 1 or the plan's clips");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the buffers may be in use by a previous loop on this stream
  const size_t plane = (size_t)c->cfg.latent_dim * pl.La * 4;
  TRY(grow(c->edit_x0, (size_t)x0_clips * plane));
  TRY(grow(c->edit_noise, (size_t)pl.clips * plane));
  if (mask) TRY(grow(c->edit_mask, (size_t)mask_clips * pl.La * 4));
  HIPTRY(hipMemcpyAsync(c->edit_x0.p, x0, (size_t)x0_clips * plane, hipMemcpyDeviceToDevice, st));
  HIPTRY(hipMemcpyAsync(c->edit_noise.p, noise, (size_t)pl.clips * plane, hipMemcpyDeviceToDevice, st));
  if (mask) HIPTRY(hipMemcpyAsync(c->edit_mask.p, mask, (size_t)mask_clips * pl.La * 4, hipMemcpyDeviceToDevice, st));
  c->opt.edit = true;
  c->opt.edit_x0_clips = x0_clips;
  c->opt.edit_mask_clips = mask ? mask_clips : 0;
  return 0;
}

extern "C" int foley_set_flowedit(foley_ctx* c, const float* x_src, int src_clips, const float* noise, int noise_rows, const float* mask,
                                  int mask_clips, float g_src, float g_tar, float sigma0, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_flowedit: foley_prepare has not been called");
  if (!x_src) {
    c->opt.flowedit = false;
    return 0;
  }
  const foley_plan& pl = c->plan;
  const RunOptions& o = c->opt;
  if (!noise) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the noise table is required (x_src NULL clears the state)");
  if (pl.ncfg != 2 || pl.clips % 2 != 0)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the plan is a CFG batch of (source, target) pairs: plan.ncfg must be 2 and plan.clips even");
  const int V = pl.clips / 2;
  if (noise_rows != 1 && noise_rows != pl.n_iter)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: noise_rows must be 1 (one fixed draw) or the plan's n_iter (fresh noise)");
  if (src_clips != 1 && src_clips != V) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: src_clips must be 1 or V = plan.clips / 2");
  if (mask && mask_clips != 1 && mask_clips != V) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: mask_clips must be 1 or V = plan.clips / 2");
  if (!std::isfinite(g_src) || !std::isfinite(g_tar) || !(g_src > 1.f) || !(g_tar > 1.f))
    return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: g_src and g_tar must be finite and > 1 (both branches run under CFG)");
  if (!(sigma0 >= 0.f && sigma0 <= 1.f)) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: sigma0 must lie in [0, 1]");
  if (o.edit) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run is an edit run (foley_set_edit); the two edits do not combine");
  if (o.n_win) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has windows (foley_set_windows); editing a long clip is not supported");
  if (o.ms_order) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has a multistep state (foley_set_multistep); the step keeps no velocity history");
  if (o.proj_mode) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has a projected-guidance state (foley_set_projected_guidance)");
  if (o.guid_sched_on || o.guid_rescale_on)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has a guidance schedule / rescale state (foley_set_guidance); the branches take their own constant scales");
  if (o.sc_mode) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has a step-cache state (foley_set_step_cache)");
  if (o.tl_sets) return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: the run has a prompt timeline (foley_prepare_timeline)");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the buffers may be in use by a previous loop on this stream
  std::vector<float> rows((size_t)pl.n_iter * 8);
  HIPTRY(hipMemcpy(rows.data(), pl.solver_coef, rows.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < pl.n_iter; ++i)
    if (!((int)rows[8 * (size_t)i + 4] & FOLEY_STEP_BLEND))
      return FAIL(FOLEY_ERR_INVALID, "foley_set_flowedit: every solver_coef row must carry FOLEY_STEP_BLEND with sigma_{k+1} in column 5 (an euler edit table; multi-stage solvers are not supported)");
  const size_t plane = (size_t)c->cfg.latent_dim * pl.La * 4;
  TRY(grow(c->fe_x_src, (size_t)src_clips * plane));
  TRY(grow(c->fe_noise, (size_t)noise_rows * V * plane));
  if (mask) TRY(grow(c->fe_mask, (size_t)mask_clips * pl.La * 4));
  HIPTRY(hipMemcpyAsync(c->fe_x_src.p, x_src, (size_t)src_clips * plane, hipMemcpyDeviceToDevice, st));
  HIPTRY(hipMemcpyAsync(c->fe_noise.p, noise, (size_t)noise_rows * V * plane, hipMemcpyDeviceToDevice, st));
  if (mask) HIPTRY(hipMemcpyAsync(c->fe_mask.p, mask, (size_t)mask_clips * pl.La * 4, hipMemcpyDeviceToDevice, st));
  c->opt.flowedit = true;
  c->opt.fe_src_clips = src_clips;
  c->opt.fe_noise_rows = noise_rows;
  c->opt.fe_mask_clips = mask ? mask_clips : 0;
  c->opt.fe_g_src = g_src; c->opt.fe_g_tar = g_tar; c->opt.fe_sigma0 = sigma0;
  return 0;
}

extern "C" int foley_set_windows(foley_ctx* c, int n_win, const int32_t* starts, const float* weights, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_windows: foley_prepare has not been called");
  if (n_win <= 1 || !starts || !weights) {
    c->opt.n_win = 0;
    return 0;
  }
  if (c->opt.edit) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: the run is an edit run (foley_set_edit); editing a long clip is not supported");
  if (c->opt.flowedit) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: the run has a FlowEdit state (foley_set_flowedit); editing a long clip is not supported");
  const foley_plan& pl = c->plan;
  if (pl.clips % n_win != 0) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: the plan's clips must be a multiple of n_win");
  if (starts[0] != 0) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: starts[0] must be 0");
  for (int k = 1; k < n_win; ++k) {
    if (starts[k] <= starts[k - 1]) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: starts must ascend from 0");
    if (starts[k] > starts[k - 1] + pl.La) return FAIL(FOLEY_ERR_INVALID, "foley_set_windows: gap between consecutive windows");
  }
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the tables may be in use by a previous loop on this stream
  TRY(grow(c->win_starts, (size_t)n_win * 4));
  TRY(grow(c->win_weights, (size_t)n_win * pl.La * 4));
  c->win_starts_host.assign(starts, starts + n_win);
  HIPTRY(hipMemcpyAsync(c->win_starts.p, c->win_starts_host.data(), (size_t)n_win * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipMemcpyAsync(c->win_weights.p, weights, (size_t)n_win * pl.La * 4, hipMemcpyDeviceToDevice, st));
  HIPTRY(hipStreamSynchronize(st));   // win_starts_host may be rewritten by the next call
  c->opt.n_win = n_win;
  c->opt.win_Ltot = starts[n_win - 1] + pl.La;
  return 0;
}

extern "C" int foley_set_guidance(foley_ctx* c, const float* sched, int n_rows, float rescale, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_guidance: foley_prepare has not been called");
  if (!sched && rescale == 0.f) {   // nothing to apply: the plan's scalar guidance
    c->opt.guid_sched_on = c->opt.guid_rescale_on = false;
    return 0;
  }
  const foley_plan& pl = c->plan;
  if (c->opt.flowedit)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: the run has a FlowEdit state (foley_set_flowedit); its branches take their own constant scales");
  if (pl.ncfg == 1) return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: the plan has one half (ncfg 1): there is nothing to guide");
  if (sched && n_rows != pl.n_iter)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: the schedule must have one row per iteration of the plan (n_rows == n_iter)");
  if (!(rescale >= 0.f && rescale <= 1.f)) return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: rescale must lie in [0, 1]");
  if (rescale > 0.f && c->cfg.latent_dim > 256)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: rescale serves at most 256 latent channels (guidance_stats_kernel)");
  if (rescale > 0.f && c->opt.proj_mode)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_guidance: rescale does not combine with projected guidance (foley_set_projected_guidance)");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the buffers may be in use by a previous loop on this stream
  const size_t nf = 2 * (size_t)pl.n_iter + 1;
  TRY(grow(c->guid_sched, nf * 4));
  if (rescale > 0.f) {
    TRY(grow(c->guid_part, (size_t)guidance_stats_floats(pl.clips, pl.La) * 4));
    TRY(grow(c->guid_scale, (size_t)pl.clips * 4));
  }
  c->guid_host.assign(nf, pl.guidance);   // without a table the rows are never read
  if (sched) std::copy(sched, sched + 2 * (size_t)pl.n_iter, c->guid_host.begin());
  c->guid_host[nf - 1] = rescale;
  HIPTRY(hipMemcpyAsync(c->guid_sched.p, c->guid_host.data(), nf * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));   // guid_host may be rewritten by the next call
  c->opt.guid_sched_on = sched != nullptr;
  c->opt.guid_rescale_on = rescale > 0.f;
  return 0;
}

extern "C" int foley_set_projected_guidance(foley_ctx* c, int mode, const float* rows, int n_rows, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_projected_guidance: foley_prepare has not been called");
  if (mode == 0) {   // the plain combine
    c->opt.proj_mode = 0;
    return 0;
  }
  if (mode != FOLEY_GUIDANCE_APG && mode != FOLEY_GUIDANCE_ZERO_STAR)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: unknown mode (0 off, 1 APG, 2 CFG-Zero*)");
  const foley_plan& pl = c->plan;
  if (c->opt.flowedit)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: the run has a FlowEdit state (foley_set_flowedit); projection does not combine with it");
  if (pl.ncfg != 2) return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: projection takes two halves (plan.ncfg != 2)");
  if (c->opt.guid_rescale_on)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: the run has a rescale state (foley_set_guidance); projection does not combine with it");
  if (!rows || n_rows != pl.n_iter)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: the table must have one row per iteration of the plan (n_rows != n_iter)");
  for (size_t k = 0; k < 4 * (size_t)n_rows; ++k)
    if (!std::isfinite(rows[k])) return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: non-finite rows");
  for (int i = 0; i < n_rows; ++i)
    if (rows[4 * i + 2] < 0.f) return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: the norm threshold must not be negative (R < 0)");
  if (c->cfg.latent_dim > 256)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_projected_guidance: projection serves at most 256 latent channels (guidance_proj_stats_kernel)");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the buffers may be in use by a previous loop on this stream
  const size_t nf = 4 * (size_t)pl.n_iter;
  TRY(grow(c->proj_rows, nf * 4));
  TRY(grow(c->proj_part, (size_t)guidance_project_floats(pl.clips, pl.La) * 4));
  TRY(grow(c->proj_coef, (size_t)pl.clips * 2 * 4));
  if (mode == FOLEY_GUIDANCE_APG) TRY(grow(c->proj_plane, (size_t)pl.clips * pl.La * c->cfg.latent_dim * 4));
  c->proj_host.assign(rows, rows + nf);
  HIPTRY(hipMemcpyAsync(c->proj_rows.p, c->proj_host.data(), nf * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));   // proj_host may be rewritten by the next call
  c->opt.proj_mode = mode;
  return 0;
}

extern "C" int foley_set_multistep(foley_ctx* c, int order, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_multistep: foley_prepare has not been called");
  if (order == 0 || order == 1) {   // a one-step method: the step kernels without history
    c->opt.ms_order = 0;
    return 0;
  }
  if (order != 2 && order != 3) return FAIL(FOLEY_ERR_INVALID, "foley_set_multistep: order must be 0 or 1 (off), 2 or 3");
  if (c->opt.flowedit)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_multistep: the run has a FlowEdit state (foley_set_flowedit); its step keeps no velocity history");
  const foley_plan& pl = c->plan;
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the ring may be in use by a previous loop on this stream
  TRY(grow(c->ms_hist, (size_t)(order - 1) * pl.clips * c->cfg.latent_dim * pl.La * 4));
  c->opt.ms_order = order;
  return 0;
}

extern "C" int foley_set_step_cache(foley_ctx* c, int mode, const uint8_t* skip, int n_skip, double threshold, const double* poly,
                                    int n_poly, const int32_t* interval, int max_consecutive, void* stream_v) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_set_step_cache: foley_prepare has not been called");
  if (mode == 0) {
    c->opt.sc_mode = 0;
    c->sc_rep_rel.clear();
    c->sc_rep_skip.clear();
    return 0;
  }
  const foley_plan& pl = c->plan;
  if (c->opt.flowedit)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: the run has a FlowEdit state (foley_set_flowedit); the step cache does not combine with it");
  if (mode != FOLEY_STEP_CACHE_SCHEDULE && mode != FOLEY_STEP_CACHE_THRESHOLD)
    return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: mode must be 0 (off), 1 (schedule) or 2 (threshold)");
  if (mode == FOLEY_STEP_CACHE_SCHEDULE && (!skip || n_skip != pl.n_iter))
    return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: the skip list must have one entry per iteration of the plan (n_skip == n_iter)");
  if (mode == FOLEY_STEP_CACHE_THRESHOLD && !(threshold >= 0.0 && std::isfinite(threshold)))
    return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: the threshold must be finite and >= 0");
  if (n_poly < 0 || (n_poly > 0 && !poly)) return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: bad polynomial");
  for (int k = 0; k < n_poly; ++k)
    if (!std::isfinite(poly[k])) return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: polynomial coefficients must be finite");
  if (interval && (interval[0] < 0 || interval[1] < interval[0] || interval[1] > pl.n_iter))
    return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: the interval is a range of iterations inside [0, n_iter]");
  if (max_consecutive < 0) return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: max_consecutive must be >= 0 (0: no cap)");
  if (c->cfg.depth_triple + c->cfg.depth_single < 1) return FAIL(FOLEY_ERR_INVALID, "foley_set_step_cache: the model has no blocks to skip");
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  HIPTRY(hipStreamSynchronize(st));   // the buffers may be in use by a previous loop on this stream
  const int Bc = pl.ncfg * pl.clips;
  const size_t bytes = (size_t)Bc * pl.La * c->cfg.hidden * 4;
  TRY(grow(c->sc_delta, bytes));
  TRY(grow(c->sc_mprev, bytes));
  TRY(grow(c->sc_part, (size_t)cache_probe_floats(Bc, pl.La) * 4));
  TRY(grow(c->sc_rel, (size_t)Bc * 4));
  if (c->sc_rel_cap < Bc) {
    if (c->sc_rel_host) (void)hipHostFree(c->sc_rel_host);
    c->sc_rel_host = nullptr;
    c->sc_rel_cap = 0;
    HIPTRY(hipHostMalloc((void**)&c->sc_rel_host, (size_t)Bc * 4, hipHostMallocDefault));
    c->sc_rel_cap = Bc;
  }
  c->opt.sc_skip.clear();
  if (mode == FOLEY_STEP_CACHE_SCHEDULE) c->opt.sc_skip.assign(skip, skip + n_skip);
  c->opt.sc_threshold = threshold;
  c->opt.sc_poly.assign(poly, poly + n_poly);
  c->opt.sc_lo = interval ? interval[0] : 0;
  c->opt.sc_hi = interval ? interval[1] : pl.n_iter;
  c->opt.sc_maxc = max_consecutive;
  c->sc_rep_rel.clear();
  c->sc_rep_skip.clear();
  c->opt.sc_mode = mode;
  return 0;
}

extern "C" int foley_step_cache_report(foley_ctx* c, float* rel, int32_t* skipped, int n) {
  if (!c || !rel || !skipped) return FAIL(FOLEY_ERR_INVALID, "null argument");
  if (c->sc_rep_skip.empty() || n != (int)c->sc_rep_skip.size())
    return FAIL(FOLEY_ERR_STATE, "foley_step_cache_report: no cached loop of n iterations has run since foley_set_step_cache");
  std::copy(c->sc_rep_rel.begin(), c->sc_rep_rel.end(), rel);
  std::copy(c->sc_rep_skip.begin(), c->sc_rep_skip.end(), skipped);
  return 0;
}

// Test-only (not in include/foley_hip.h): out[0] = iterations captured into a graph so far, out[1..3] = addresses of the model
// input rows (the workspace), the schedule table and the rescale factors - what a replay of the captured iteration addresses.
extern "C" int foley_debug_run_state(foley_ctx* c, uint64_t* out) {
  if (!c || !out) return FAIL(FOLEY_ERR_INVALID, "null argument");
  out[0] = c->graph_captures;
  out[1] = (uint64_t)(uintptr_t)c->buf.xin;
  out[2] = (uint64_t)(uintptr_t)c->guid_sched.p;
  out[3] = (uint64_t)(uintptr_t)c->guid_scale.p;
  return 0;
}

extern "C" int foley_sample(foley_ctx* c, float* latents, int use_graph, foley_progress_cb cb, void* user,
                            void* stream_v) {
  if (!c || !latents) return FAIL(FOLEY_ERR_INVALID, "null argument");
  if (!c->prepared) return FAIL(FOLEY_ERR_STATE, "foley_prepare has not been called");
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  const foley_plan& pl = c->plan;
  // under a FlowEdit state the latents are z [V, latent_dim, La], V = clips / 2: the first V planes of the state buffer
  const size_t xbytes = (size_t)(c->opt.flowedit ? pl.clips / 2 : pl.clips) * c->cfg.latent_dim * pl.La * 4;
  GraphKey key = graph_key_now(c);
  const bool cached = c->opt.sc_mode != 0;
  if (c->graph_exec && !(c->graph_key == key)) ctx_drop_graph(c);
  if (use_graph && !c->graph_exec) {
    // Every per-iteration value is read from device memory (step counter, tables) and every
    // buffer is context-owned, so ONE captured iteration replays for the whole loop and for
    // later runs of the same shape.
    // Under the step cache the iteration is three such graphs (head, full body, skip body); the host picks a body per iteration.
    std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
    hipStream_t cs;
    HIPTRY(hipStreamSynchronize(st));
    HIPTRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraphExec_t* const slots[3] = {&c->graph_head, &c->graph_exec, &c->graph_skip};
    int rc = 0;
    hipError_t e = hipSuccess;
    for (int piece = cached ? SC_HEAD : SC_FULL; piece <= (cached ? SC_SKIP : SC_FULL) && rc == 0 && e == hipSuccess; ++piece) {
      hipGraph_t graph = nullptr;
      e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        rc = cached ? run_cached_piece(c, piece, cs) : run_iteration(c, cs);
        hipError_t e2 = hipStreamEndCapture(cs, &graph);
        if (e == hipSuccess) e = e2;
      }
      if (e == hipSuccess && rc == 0) e = hipGraphInstantiate(slots[piece], graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
    }
    (void)hipStreamDestroy(cs);
    if (rc != 0 || e != hipSuccess) ctx_drop_graph(c);   // never a partial set
    if (rc != 0) return rc;
    if (e != hipSuccess) return FAIL(FOLEY_ERR_HIP, hipGetErrorString(e));
    c->graph_key = std::move(key);
    ++c->graph_captures;
  }
  c->abort_req.store(0, std::memory_order_relaxed);   // a request left over from before this loop is not for it
  HIPTRY(hipEventRecord(c->ev0, st));
  HIPTRY(hipMemcpyAsync(c->buf.x_cur, latents, xbytes, hipMemcpyDeviceToDevice, st));
  HIPTRY(hipMemsetAsync(c->buf.step_ctr, 0, sizeof(int), st));
  if (c->opt.flowedit) TRY(launch_flowedit_stage(key.args.flowedit, c->opt.fe_sigma0, 0, st));   // both branches at sigma_{k0}
  else TRY(launch_latent_rows(c->buf.x_cur, pl.clips, c->cfg.latent_dim, pl.La, pl.ncfg, c->buf.xin, c->cfg.compute_dtype, st));
  StepCachePolicy policy;
  if (cached) {
    c->sc_rep_rel.assign(pl.n_iter, -1.f);
    c->sc_rep_skip.assign(pl.n_iter, 0);
  }
  auto piece = [&](int which) -> int {
    if (use_graph) HIPTRY(hipGraphLaunch(which == SC_HEAD ? c->graph_head : which == SC_FULL ? c->graph_exec : c->graph_skip, st));
    else TRY(run_cached_piece(c, which, st));
    return 0;
  };
  for (int it = 0; it < pl.n_iter; ++it) {
    if (cached) {
      TRY(piece(SC_HEAD));
      float rel = -1.f;
      if (c->opt.sc_mode == FOLEY_STEP_CACHE_THRESHOLD) {   // the one read-back and synchronisation per iteration; schedule mode has none
        const int Bc = pl.ncfg * pl.clips;
        HIPTRY(hipMemcpyAsync(c->sc_rel_host, c->sc_rel.p, (size_t)Bc * 4, hipMemcpyDeviceToHost, st));
        HIPTRY(hipStreamSynchronize(st));
        if (it > 0) {   // iteration 0 has no previous m: not measured
          rel = c->sc_rel_host[0];
          for (int b = 1; b < Bc; ++b) rel = c->sc_rel_host[b] > rel ? c->sc_rel_host[b] : rel;   // one decision for the context
          c->sc_rep_rel[it] = rel;
        }
      }
      const bool skip = policy.decide(c->opt, it, pl.n_iter, rel);
      c->sc_rep_skip[it] = skip ? 1 : 0;
      TRY(piece(skip ? SC_SKIP : SC_FULL));
    } else if (use_graph) HIPTRY(hipGraphLaunch(c->graph_exec, st));
    else TRY(run_iteration(c, st));
    if (cb) {
      HIPTRY(hipMemcpyAsync(latents, c->buf.x_cur, xbytes, hipMemcpyDeviceToDevice, st));
      HIPTRY(hipStreamSynchronize(st));
      cb(it + 1, pl.n_iter, user);
    }
    if (c->abort_req.exchange(0, std::memory_order_acq_rel)) {   // latents hold the state after iteration it + 1
      if (!cb) {
        HIPTRY(hipMemcpyAsync(latents, c->buf.x_cur, xbytes, hipMemcpyDeviceToDevice, st));
        HIPTRY(hipStreamSynchronize(st));
      }
      return FAIL(FOLEY_ERR_ABORTED, "sampling loop aborted by foley_abort()");
    }
  }
  HIPTRY(hipMemcpyAsync(latents, c->buf.x_cur, xbytes, hipMemcpyDeviceToDevice, st));
  HIPTRY(hipEventRecord(c->ev1, st));
  c->timed = true;
  return 0;
}

extern "C" int foley_abort(foley_ctx* c) {
  if (!c) return FAIL(FOLEY_ERR_INVALID, "null context");
  c->abort_req.store(1, std::memory_order_release);
  return 0;
}

// --------------------------------------------------------------------------- DAC decoder
// Activations are kept time-major [clip, T, C] so that every conv is a GEMM over contiguous
// channel vectors; weight-norm is folded at pack time; each snake is evaluated once, in the
// epilogue of the op that produces its input.  (dac.py:28-44, 98-149, 280-303)
// activation buffers of `act_bytes` each and the latent-rate scratch, grown while nothing on `st` reads them
static int dac_grow(foley_ctx* c, size_t act_bytes, size_t z_bytes, hipStream_t st) {
  std::lock_guard<std::mutex> setup_lock(g_setup_mutex);
  HIPTRY(hipStreamSynchronize(st));
  TRY(grow(c->dacP, act_bytes));
  TRY(grow(c->dacQ, act_bytes));
  TRY(grow(c->dacR, act_bytes));
  return grow(c->dacZ, z_bytes);
}

// Residual unit `u` (dac.py:28-44) over `clips` segments of T rows, C channels: conv7 of dilation d with its snake (S_in -> S_alt),
// then the 1x1 with the residual add into the trunk X and the snake of whatever consumes the unit's output next (-> S_in)
static int dac_res_unit(foley_ctx* c, const std::string& u, const std::string& next_alpha, int clips, int T, int C, int d,
                        float* S_in, float* S_alt, float* X, hipStream_t st) {
  Lin c7, c1;
  const void *a2, *an;
  TRY(get_lin(c, u + "c7", FOLEY_F32, C, 7 * C, true, &c7));
  TRY(get_lin(c, u + "c1", FOLEY_F32, C, C, true, &c1));
  TRY(get_tensor(c, u + "a2", FOLEY_F32, {C}, &a2));
  TRY(get_tensor(c, next_alpha, FOLEY_F32, {C}, &an));
  GemmArgs g = gemm_conv(S_in, clips * T, T, C, 7, d, c7, nullptr, C);
  g.out1 = S_alt; g.alpha = (const float*)a2; g.alphaC = C;
  TRY(launch_gemm(g, FOLEY_F32, EPI_DAC, 0, st));
  g = gemm_plain(S_alt, clips * T, c1, X, C);
  g.res = X; g.out1 = S_in; g.alpha = (const float*)an; g.alphaC = C;
  return launch_gemm(g, FOLEY_F32, EPI_DAC, 0, st);
}

extern "C" int foley_dac_decode(foley_ctx* c, const float* latents, int clips, int T, float* wave, void* stream_v) {
  if (!c || !latents || !wave || clips < 1 || T < 1) return FAIL(FOLEY_ERR_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  const foley_config& f = c->cfg;
  const int L = f.latent_dim, NR = f.dac_n_rates;
  // largest activation
  size_t maxel = (size_t)T * f.dac_dim;
  for (long i = 0, t = T, ch = f.dac_dim; i < NR; ++i) {
    t *= f.dac_rates[i];
    ch /= 2;
    maxel = std::max(maxel, (size_t)t * ch);
  }
  TRY(dac_grow(c, maxel * clips * 4, (size_t)clips * T * L * 4 * 2, st));
  // snake-activated input of the next op, residual trunk, the other snake buffer
  float *S_in = (float*)c->dacP.p, *X = (float*)c->dacQ.p, *S_alt = (float*)c->dacR.p;
  float *Z0 = (float*)c->dacZ.p, *Z1 = Z0 + (size_t)clips * T * L;
  HIPTRY(hipEventRecord(c->ev0, st));

  TRY(launch_latent_rows(latents, clips, L, T, 1, Z0, FOLEY_F32, st));
  Lin pq, cin;
  TRY(get_lin(c, "dac.pq", FOLEY_F32, L, L, true, &pq));
  TRY(get_lin(c, "dac.in", FOLEY_F32, f.dac_dim, 7 * L, true, &cin));
  TRY(launch_gemm(gemm_plain(Z0, clips * T, pq, Z1, L), FOLEY_F32, EPI_STORE_F32, 0, st));
  const void* al;
  TRY(get_tensor(c, "dac.0.alpha0", FOLEY_F32, {f.dac_dim}, &al));
  {
    GemmArgs g = gemm_conv(Z1, clips * T, T, L, 7, 1, cin, nullptr, f.dac_dim);
    g.out1 = S_in; g.alpha = (const float*)al; g.alphaC = f.dac_dim;
    TRY(launch_gemm(g, FOLEY_F32, EPI_DAC, 0, st));
  }
  int Tin = T, Cin = f.dac_dim;
  for (int i = 0; i < NR; ++i) {
    const int s = f.dac_rates[i], Cout = Cin / 2, Tout = Tin * s, pad = (s + 1) / 2;
    const std::string p = "dac." + std::to_string(i) + ".";
    Lin up;
    TRY(get_lin(c, p + "up", FOLEY_F32, s * Cout, 2 * Cin, true, &up));
    const void* a1;
    TRY(get_tensor(c, p + "0.a1", FOLEY_F32, {Cout}, &a1));
    {
      // transposed conv: virtual row q of segment (Tin+1) = [x[q-1] ; x[q]], N axis = (phase, Cout),
      // output sample t = q*s + phase - pad  (dac.py:102-109)
      GemmArgs g = gemm_plain(S_in, clips * (Tin + 1), up, X, (long)s * Cout);
      g.lda = Cin; g.segV = Tin + 1; g.segS = Tin; g.taps = 2; g.tapC = Cin; g.dil = 1; g.tap0 = -1;
      g.osegV = Tin + 1; g.out_seg = (long)Tout * Cout; g.out_row = (long)s * Cout; g.out_shift = -(long)pad * Cout;
      g.out_check = 1;
      g.out1 = S_alt; g.alpha = (const float*)a1; g.alphaC = Cout;
      TRY(launch_gemm(g, FOLEY_F32, EPI_DAC, 0, st));
    }
    std::swap(S_in, S_alt);  // S_in now holds snake(x) for unit 0
    for (int j = 0; j < 3; ++j) {
      // alpha of whatever consumes this unit's output next
      std::string nxt = (j < 2) ? p + std::to_string(j + 1) + ".a1"
                                : (i + 1 < NR ? "dac." + std::to_string(i + 1) + ".alpha0" : std::string("dac.out.alpha"));
      TRY(dac_res_unit(c, p + std::to_string(j) + ".", nxt, clips, Tout, Cout, f.dac_dilations[j], S_in, S_alt, X, st));
    }
    Tin = Tout;
    Cin = Cout;
  }
  const void *ow, *ob;
  TRY(get_tensor(c, "dac.out.w", FOLEY_F32, {7 * Cin}, &ow));
  TRY(get_tensor(c, "dac.out.b", FOLEY_F32, {1}, &ob));
  TRY(launch_dac_out(S_in, (const float*)ow, (const float*)ob, clips, Tin, Cin, wave, st));
  HIPTRY(hipEventRecord(c->ev1, st));
  c->timed = true;
  return 0;
}

// --------------------------------------------------------------------------- DAC encoder (row N4)
// DAC.encode, continuous=True (dac.py:236-278): waveform [clips, 1, T] (T a multiple of the hop) ->
// posterior parameters [clips, 2*latent, T/hop] = quant_conv(encoder(x)).  Same engine as the
// decoder: time-major fp32 activations, conv-as-GEMM with the residual + snake epilogue; the strided
// down-sampling convs (k = 2s, stride s, pad ceil(s/2)) are GEMMs over virtual rows that advance s
// source rows (GemmArgs::rstride).
extern "C" int foley_dac_encode(foley_ctx* c, const float* wave, int clips, int T, int enc_dim, const int32_t* rates,
                                int n_rates, float* params, void* stream_v) {
  if (!c || !wave || !params || !rates || clips < 1 || T < 1 || n_rates < 1 || n_rates > 8 || enc_dim < 1)
    return FAIL(FOLEY_ERR_INVALID, "bad argument");
  long hop = 1;
  for (int i = 0; i < n_rates; ++i) hop *= rates[i];
  if (T % hop) return FAIL(FOLEY_ERR_INVALID, "waveform length must be a multiple of the codec hop (DAC.preprocess pads it)");
  hipStream_t st = (hipStream_t)stream_v;
  HIPTRY(hipSetDevice(c->device));
  const foley_config& f = c->cfg;
  const int L = f.latent_dim;
  size_t maxel = 0;
  for (long i = 0, t = T, ch = enc_dim; i <= n_rates; ++i) {
    maxel = std::max(maxel, (size_t)t * ch);
    if (i < n_rates) { t /= rates[i]; ch *= 2; }
  }
  const int Tz = (int)(T / hop);
  TRY(dac_grow(c, maxel * clips * 4, (size_t)clips * Tz * L * 4 * 3, st));
  float *S_in = (float*)c->dacP.p, *X = (float*)c->dacQ.p, *S_alt = (float*)c->dacR.p;
  float *Z0 = (float*)c->dacZ.p, *Z1 = Z0 + (size_t)clips * Tz * L;
  HIPTRY(hipEventRecord(c->ev0, st));

  int Tin = T, C = enc_dim;
  {
    const void *w, *b, *a;
    TRY(get_tensor(c, "enc.in.w", FOLEY_F32, {7 * C}, &w));
    TRY(get_tensor(c, "enc.in.b", FOLEY_F32, {C}, &b));
    TRY(get_tensor(c, "enc.0.0.a1", FOLEY_F32, {C}, &a));
    TRY(launch_dac_in(wave, (const float*)w, (const float*)b, (const float*)a, clips, T, C, X, S_in, st));
  }
  for (int i = 0; i < n_rates; ++i) {
    const int s = rates[i], Cout = 2 * C, Tout = Tin / s, pad = (s + 1) / 2;
    const std::string p = "enc." + std::to_string(i) + ".";
    for (int j = 0; j < 3; ++j) {
      // alpha of whatever consumes this unit's output next: the next unit, or the snake before the strided conv
      TRY(dac_res_unit(c, p + std::to_string(j) + ".", j < 2 ? p + std::to_string(j + 1) + ".a1" : p + "alpha", clips, Tin, C,
                       f.dac_dilations[j], S_in, S_alt, X, st));
    }
    {
      // strided conv: output row q of a clip reads source rows q*s - pad + j, j < 2s  (dac.py:55-61)
      Lin down;
      const void* an;
      TRY(get_lin(c, p + "down", FOLEY_F32, Cout, 2 * s * C, true, &down));
      TRY(get_tensor(c, i + 1 < n_rates ? "enc." + std::to_string(i + 1) + ".0.a1" : std::string("enc.out.alpha"), FOLEY_F32,
                     {Cout}, &an));
      GemmArgs g = gemm_plain(S_in, clips * Tout, down, X, Cout);
      g.lda = C; g.segV = Tout; g.segS = Tin; g.taps = 2 * s; g.tapC = C; g.dil = 1; g.tap0 = -pad; g.rstride = s;
      g.out1 = S_alt; g.alpha = (const float*)an; g.alphaC = Cout;
      TRY(launch_gemm(g, FOLEY_F32, EPI_DAC, 0, st));
      std::swap(S_in, S_alt);
    }
    Tin = Tout;
    C = Cout;
  }
  {
    Lin co, qc;
    TRY(get_lin(c, "enc.out", FOLEY_F32, L, 3 * C, true, &co));
    TRY(get_lin(c, "enc.qc", FOLEY_F32, 2 * L, L, true, &qc));
    TRY(launch_gemm(gemm_conv(S_in, clips * Tin, Tin, C, 3, 1, co, Z0, L), FOLEY_F32, EPI_STORE_F32, 0, st));
    TRY(launch_gemm(gemm_plain(Z0, clips * Tin, qc, Z1, 2 * L), FOLEY_F32, EPI_STORE_F32, 0, st));
    TRY(launch_rows_to_planes(Z1, clips, Tin, 2 * L, params, st));
  }
  HIPTRY(hipEventRecord(c->ev1, st));
  c->timed = true;
  return 0;
}

// --------------------------------------------------------------------------- op-level entry points
// Test-only hook (tests/test_rowbcast_entry_gpu.py; not part of include/foley_hip.h): while set, every row-broadcast operand the
// calling thread's op entries convert carries a device counter and a step stride, as run_forward's operands do - the operand
// reads base + *counter * step_stride.  The conversions take p0 and p1 in turn (p1 null: always p0), so two different words
// give one launch operands with different counters; p0 null switches the hook off.
static thread_local const int* g_rb_step_ptr[2] = {nullptr, nullptr};
static thread_local long g_rb_step_stride = 0;
static thread_local unsigned g_rb_step_n = 0;
extern "C" void foley_debug_rowbcast_step(const int32_t* p0, const int32_t* p1, int64_t step_stride) {
  g_rb_step_ptr[0] = p0;
  g_rb_step_ptr[1] = p1 ? p1 : p0;
  g_rb_step_stride = (long)step_stride;
  g_rb_step_n = 0;
}
static RowBcast rb_debug_step(RowBcast b) {
  if (b.p && g_rb_step_ptr[0]) {
    b.step_ptr = g_rb_step_ptr[g_rb_step_n++ & 1];
    b.step_stride = g_rb_step_stride;
  }
  return b;
}

static RowBcast to_rb(const foley_rowbcast* r) {
  if (!r || !r->p) return rb_none();
  const int L = r->L > 0 ? r->L : 1, Ls = r->mode == 2 ? (r->Ls > 0 ? r->Ls : 1) : 0;
  const int per = (r->mode == 2 && r->period > 0 && !(r->period & (r->period - 1))) ? r->period : 0;
  RowBcast b{r->p, (long)r->ld, r->mode, r->rows_per_cfg > 0 ? r->rows_per_cfg : 1, L, nullptr, 0, Ls, Ls ? (float)Ls / (float)L : 0.f, per, 0, 0};
  if (per > 0) {
    b.dense_from = r->periodic_cfgs > 0 ? r->periodic_cfgs : INT_MAX;
    b.dense_base = r->periodic_cfgs > 0 ? r->periodic_cfgs * per : 0;
  }
  return rb_debug_step(b);
}

// descriptor -> GemmArgs (foley_op_gemm and the test-only pair entry below)
static int gemm_args_of(const foley_gemm_desc* d, GemmArgs& g) {
  if (!d) return FAIL(FOLEY_ERR_INVALID, "null descriptor");
  g = GemmArgs{};
  g.A = d->A; g.W = d->W; g.bias = d->bias; g.M = d->M; g.N = d->N; g.K = d->K; g.lda = d->lda;
  g.segV = d->segV; g.segS = d->segS; g.taps = d->taps; g.tapC = d->tapC; g.dil = d->dil; g.tap0 = d->tap0;
  g.out0 = d->out0; g.out1 = d->out1; g.osegV = d->osegV; g.out_seg = d->out_seg; g.out_row = d->out_row;
  g.out_shift = d->out_shift; g.out_check = d->out_check; g.rb = to_rb(&d->rb); g.res = d->res;
  g.alpha = d->alpha; g.alphaC = d->alphaC > 0 ? d->alphaC : 1;
  g.ksplit = d->ksplit;
  g.rstride = d->rstride;
  g.ldw = d->ldw;
  g.wfmt = d->wfmt;
  g.gelu_erf = d->gelu_erf;
  if (d->partials) {
    if (d->partial_slabs < 1) return FAIL(FOLEY_ERR_INVALID, "partials need partial_slabs >= 1");
    g.partials = d->partials; g.partial_stride = (long)d->M * d->N; g.partial_cap = d->partial_slabs;
    g.partial_half = d->partial_dtype != 0;
    if (d->partial_dtype != 0 && d->partial_dtype != d->dtype) return FAIL(FOLEY_ERR_INVALID, "partial_dtype must be 0 (fp32) or the operand dtype");
  }
  if (g.segV < 1 || g.segS < 1 || g.osegV < 1 || g.taps < 1) return FAIL(FOLEY_ERR_INVALID, "bad GEMM descriptor");
  if (d->epilogue == EPI_QKV_SPLIT) {
    const foley_qkv_split_desc* q = d->qkv;
    if (!q) return FAIL(FOLEY_ERR_INVALID, "epilogue 7 needs a head-split descriptor");
    QkvSplitArgs& a = g.qs;
    a.qkv = nullptr; a.M = d->M; a.L = q->L; a.H = q->H; a.nK = q->nK;
    for (int i = 0; i < 3; ++i) { a.gain[i] = q->gain[i]; a.pos[i] = q->pos[i]; a.dst[i] = q->dst[i]; }
    a.S_tot = q->S_tot; a.tok_off = q->tok_off; a.out_dtype = q->out_dtype; a.vt_pitch = q->vt_pitch;
    a.eps = q->eps; a.cos_tab = q->cos_tab; a.sin_tab = q->sin_tab;
    a.attn_k = q->attn_k; a.attn_vt = q->attn_vt; a.attn_out = q->attn_out;
    a.attn_skv = q->attn_skv; a.attn_pitch = q->attn_pitch; a.attn_bdiv = q->attn_bdiv; a.attn_fused = q->attn_fused;
    if (q->attn_fused) *q->attn_fused = 0;
  }
  return 0;
}

// Test-only hook (tests/test_pairs_gpu.py; not part of include/foley_hip.h): the op-level GEMM entries of the calling thread opt in
// to K-origin rotation (GemmArgs::krot_ok) as run_forward does for single-clip forwards; returns the previous setting.
static thread_local int g_gemm_krot_ok = 0;
extern "C" int foley_debug_gemm_krot(int on) {
  const int prev = g_gemm_krot_ok;
  g_gemm_krot_ok = on ? 1 : 0;
  return prev;
}

extern "C" int foley_op_gemm(const foley_gemm_desc* d, void* stream) {
  GemmArgs g;
  if (int rc = gemm_args_of(d, g)) return rc;
  g.zeros = zero_page();
  g.krot_ok = g_gemm_krot_ok;
  int ks = 1;
  const int rc = launch_gemm(g, d->dtype, d->epilogue, d->tile, (hipStream_t)stream, &ks);
  if (d->ksplit_used) *d->ksplit_used = ks;
  return rc;
}

// Test-only entries (not part of include/foley_hip.h; tests/test_pairs_gpu.py types them with ctypes): the two-problem launches
// of run_forward's two-stream blocks at op level.  launch_gemm_pair picks its own tile and one K split for both problems (written
// to d0->ksplit_used); both descriptors must name the same operand dtype and epilogue.
static int gemm_pair_args_of(const foley_gemm_desc* d0, const foley_gemm_desc* d1, GemmArgs& g0, GemmArgs& g1) {
  if (!d0 || !d1) return FAIL(FOLEY_ERR_INVALID, "null descriptor");
  if (d0->dtype != d1->dtype || d0->epilogue != d1->epilogue)
    return FAIL(FOLEY_ERR_INVALID, "GEMM pair: the two problems must share the operand dtype and the epilogue");
  if (d0->tile != 0 || d1->tile != 0) return FAIL(FOLEY_ERR_INVALID, "GEMM pair: the pair launcher picks its own tile (tile must be 0)");
  if (int rc = gemm_args_of(d0, g0)) return rc;
  return gemm_args_of(d1, g1);
}

extern "C" int foley_debug_gemm_pair(const foley_gemm_desc* d0, const foley_gemm_desc* d1, void* stream) {
  GemmArgs g0, g1;
  if (int rc = gemm_pair_args_of(d0, d1, g0, g1)) return rc;
  g0.zeros = g1.zeros = zero_page();
  g0.krot_ok = g1.krot_ok = g_gemm_krot_ok;
  int ks = 1;
  const int rc = launch_gemm_pair(g0, g1, d0->dtype, d0->epilogue, (hipStream_t)stream, &ks);
  if (d0->ksplit_used) *d0->ksplit_used = ks;
  return rc;
}

// Test-only (tests/test_gemm_plan_cpu.py): the launcher's plan for one problem (d1 null) or a pair, without touching the device -
// descriptors may carry fake (16-byte aligned) addresses.  out = {tile, K split, panel groups, k_rot}; krot_ok opts in to K-origin
// rotation as run_forward does for single-clip forwards.
// out[0..3] = tile, K split, panel groups, K-origin rotation; n_out > 4 adds out[4] = write-through output stores (GemmPlan::wt_out)
static int debug_gemm_plan(const foley_gemm_desc* d0, const foley_gemm_desc* d1, int krot_ok, int32_t* out, int n_out) {
  if (!out) return FAIL(FOLEY_ERR_INVALID, "null output");
  GemmArgs g0, g1;
  if (int rc = d1 ? gemm_pair_args_of(d0, d1, g0, g1) : gemm_args_of(d0, g0)) return rc;
  GemmPlan p;
  switch (d0->dtype) {
    case FOLEY_F32: p = plan_gemm<float>(g0, d1 ? &g1 : nullptr, d0->epilogue, d0->tile, krot_ok); break;
    case FOLEY_BF16: p = plan_gemm<bf16_t>(g0, d1 ? &g1 : nullptr, d0->epilogue, d0->tile, krot_ok); break;
    case FOLEY_F16: p = plan_gemm<f16_t>(g0, d1 ? &g1 : nullptr, d0->epilogue, d0->tile, krot_ok); break;
    default: return FAIL(FOLEY_ERR_INVALID, "GEMM: unsupported operand dtype");
  }
  if (p.err) return FAIL(FOLEY_ERR_INVALID, p.err);
  out[0] = p.tile; out[1] = p.ksplit; out[2] = p.n_groups; out[3] = p.k_rot;
  if (n_out > 4) out[4] = p.wt_out;
  return 0;
}
extern "C" int foley_debug_gemm_plan(const foley_gemm_desc* d0, const foley_gemm_desc* d1, int krot_ok, int32_t out[4]) {
  return debug_gemm_plan(d0, d1, krot_ok, out, 4);
}
// the same plan with the fields added since the four-word form was fixed
extern "C" int foley_debug_gemm_plan_ex(const foley_gemm_desc* d0, const foley_gemm_desc* d1, int krot_ok, int32_t out[8]) {
  if (out) for (int i = 4; i < 8; ++i) out[i] = 0;
  return debug_gemm_plan(d0, d1, krot_ok, out, 8);
}
// tests: 1 = every launch keeps the default stores whatever it planned (bit-equality twins of the write-through launches); 0 = as planned
int g_foley_store_default = 0;
extern "C" void foley_debug_store_policy(int keep_default) { g_foley_store_default = keep_default ? 1 : 0; }

extern "C" int foley_op_attention_hd(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq,
                                     int H, int Sq, int Skv, int kv_bdiv, void* outA, void* outB, int split,
                                     int out_dtype, int head_dim, void* stream) {
  AttnArgs a{q, k, v, Bq, H, Sq, Skv, kv_bdiv > 0 ? kv_bdiv : 1, outA, outB, split, in_dtype, vt_pitch, head_dim};
  return launch_attention(a, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_attention_scatter(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int G, int H, int Sq,
                                          int Skv, int grp_q, int grp_kv, const int32_t* out_rows, void* out, int out_nrows, int out_dtype, void* stream) {
  if (!out_rows || !out) return FAIL(FOLEY_ERR_INVALID, "null argument");
  if (out_nrows < 1) return FAIL(FOLEY_ERR_INVALID, "attention_scatter: out has no rows");
  AttnArgs a{q, k, v, G, H, Sq, Skv, 1, out, out, 0, in_dtype, vt_pitch, 64};
  a.grp_q = grp_q; a.grp_kv = grp_kv;
  a.out_rows = out_rows;
  a.out_nrows = out_nrows;
  return launch_attention(a, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_attention(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq,
                                  int H, int Sq, int Skv, int kv_bdiv, void* outA, void* outB, int split,
                                  int out_dtype, void* stream) {
  return foley_op_attention_hd(q, k, v, in_dtype, vt_pitch, Bq, H, Sq, Skv, kv_bdiv, outA, outB, split, out_dtype, 128, stream);
}

extern "C" int foley_op_attention_timeline(const void* q, const void* k, const void* v, int in_dtype, int vt_pitch, int Bq, int H, int Sq,
                                           int Skv, int n_sets, const int32_t* set_a, const int32_t* set_b, const float* alpha, void* outA,
                                           void* outB, int split, int out_dtype, void* stream) {
  AttnTimelineArgs a{q, k, v, set_a, set_b, alpha, Bq, H, Sq, Skv, n_sets, outA, outB, split, in_dtype, vt_pitch};
  return launch_attention_timeline(a, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_qkv_regroup(const void* qkv, int n_rows, int dtype, int H, const int32_t* idx_q, int G, int Sq, const int32_t* idx_kv, int Skv,
                                    void* q, void* k, void* v, int vt_pitch, void* stream) {
  if (!qkv || !idx_q || !idx_kv || !q || !k || !v) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_qkv_regroup(qkv, n_rows, dtype, H, idx_q, G, Sq, idx_kv, Skv, q, k, v, vt_pitch, (hipStream_t)stream);
}

extern "C" int foley_op_resample_sinc(const float* x, int B, int N, int orig, int new_rate, const float* taps, int ntaps, int width,
                                      float* out, int Nout, void* stream) {
  if (!x || !taps || !out) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_resample_sinc(x, B, N, orig, new_rate, taps, ntaps, width, out, Nout, (hipStream_t)stream);
}

extern "C" int foley_op_logmel(const float* w16, int B, int N16, const float* basis, const int32_t* mel_lo, const int32_t* mel_len,
                               const float* mel_w, int mel_wp, void* patches, int out_dtype, float* mel_out, void* stream) {
  if (!w16 || !basis || !mel_lo || !mel_len || !mel_w || !patches) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_logmel(w16, B, N16, basis, mel_lo, mel_len, mel_w, mel_wp, patches, out_dtype, mel_out, (hipStream_t)stream);
}

extern "C" int foley_op_loudness_energy(const float* x, int B, int C, int N, int64_t ld, const double* T16, double* work,
                                        int64_t work_doubles, double* e, void* stream) {
  if (!x || !T16) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_loudness_energy(x, B, C, N, (long)ld, T16, work, work_doubles, e, (hipStream_t)stream);
}

extern "C" int foley_op_loudness_gate(const double* e, int B, int C, int nh, double* lufs, double* gamma, double* block_lufs,
                                      void* stream) {
  return launch_loudness_gate(e, B, C, nh, lufs, gamma, block_lufs, (hipStream_t)stream);
}

extern "C" int foley_op_true_peak(const float* x, int B, int C, int N, int64_t ld, const float* taps36, float* true_peak,
                                  float* sample_peak, float* envelope, void* stream) {
  if (!x || !taps36 || !true_peak) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_true_peak(x, B, C, N, (long)ld, taps36, true_peak, sample_peak, envelope, (hipStream_t)stream);
}

extern "C" int foley_op_loudness_apply(const float* x, int B, int C, int N, int64_t ld, const float* gain, int limiter,
                                       double ceiling, int lookahead, const float* taps36, float* y, int64_t ldy, float* g_out,
                                       void* stream) {
  if (!x || !gain || !y) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_loudness_apply(x, B, C, N, (long)ld, gain, limiter, ceiling, lookahead, taps36, y, (long)ldy, g_out,
                               (hipStream_t)stream);
}

extern "C" int foley_op_resize_aa_u8(const uint8_t* in, long outer, int len_in, long inner, int len_out, const int32_t* xmin,
                                     const int32_t* xsize, const int16_t* weights, int kmax, int precision, uint8_t* out, void* stream) {
  if (!in || !xmin || !xsize || !weights || !out) return FAIL(FOLEY_ERR_INVALID, "null argument");
  return launch_resize_aa_u8(in, outer, len_in, inner, len_out, xmin, xsize, weights, kmax, precision, out, (hipStream_t)stream);
}

extern "C" int foley_op_ln_mod(const float* x, int M, int D, float eps, const foley_rowbcast* shift,
                               const foley_rowbcast* scale, void* out, int out_dtype, void* stream) {
  return launch_ln_mod(x, M, D, eps, to_rb(shift), to_rb(scale), out, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_ln_mod_pending2(float* x, int M, int D, float eps, const foley_rowbcast* shift,
                                        const foley_rowbcast* scale, void* out, int out_dtype, const void* partials,
                                        int partial_dtype, int k, const float* bias, const foley_rowbcast* gate, void* stream) {
  if (!partials || k < 1 || !gate) return FAIL(FOLEY_ERR_INVALID, "pending split-K: partials, k >= 1 and a gate are required");
  if (partial_dtype != 0 && partial_dtype != out_dtype) return FAIL(FOLEY_ERR_INVALID, "pending split-K: 16-bit slabs must have the output dtype");
  LnPending p{(const float*)partials, k, (long)M * D, bias, to_rb(gate), partial_dtype};
  return launch_ln_mod_pending(x, M, D, eps, to_rb(shift), to_rb(scale), out, out_dtype, p, (hipStream_t)stream);
}

// Test-only (see foley_debug_gemm_pair): launch_ln_mod_pair over two row sets, each with the arguments of foley_op_ln_mod_pending2;
// a null `partials` means nothing is pending for that set
extern "C" int foley_debug_ln_mod_pair(float* x0, int M0, const foley_rowbcast* shift0, const foley_rowbcast* scale0, void* out0,
                                       const void* partials0, int partial_dtype0, int k0, const float* bias0, const foley_rowbcast* gate0,
                                       float* x1, int M1, const foley_rowbcast* shift1, const foley_rowbcast* scale1, void* out1,
                                       const void* partials1, int partial_dtype1, int k1, const float* bias1, const foley_rowbcast* gate1,
                                       int D, float eps, int out_dtype, void* stream) {
  LnArgs a[2] = {{x0, M0, to_rb(shift0), to_rb(scale0), out0, LnPending{}}, {x1, M1, to_rb(shift1), to_rb(scale1), out1, LnPending{}}};
  const void* parts[2] = {partials0, partials1};
  const int pdt[2] = {partial_dtype0, partial_dtype1}, ks[2] = {k0, k1};
  const float* bias[2] = {bias0, bias1};
  const foley_rowbcast* gate[2] = {gate0, gate1};
  for (int i = 0; i < 2; ++i) {
    if (a[i].M < 0) return FAIL(FOLEY_ERR_INVALID, "ln_mod pair: negative row count");
    if (!parts[i]) continue;
    if (ks[i] < 1 || !gate[i]) return FAIL(FOLEY_ERR_INVALID, "pending split-K: partials, k >= 1 and a gate are required");
    if (pdt[i] != 0 && pdt[i] != out_dtype) return FAIL(FOLEY_ERR_INVALID, "pending split-K: 16-bit slabs must have the output dtype");
    a[i].pend = LnPending{(const float*)parts[i], ks[i], (long)a[i].M * D, bias[i], to_rb(gate[i]), pdt[i]};
  }
  return launch_ln_mod_pair(a[0], a[1], D, eps, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_ln_mod_pending(float* x, int M, int D, float eps, const foley_rowbcast* shift,
                                       const foley_rowbcast* scale, void* out, int out_dtype, const float* partials,
                                       int k, const float* bias, const foley_rowbcast* gate, void* stream) {
  return foley_op_ln_mod_pending2(x, M, D, eps, shift, scale, out, out_dtype, partials, 0, k, bias, gate, stream);
}

extern "C" int foley_op_qkv_split(const float* qkv, int M, int L, int H, int nK, const float* const* gain,
                                  const int32_t* const* pos, void* const* dst, int out_dtype, int vt_pitch,
                                  int S_tot, int tok_off, float eps, const float* cos_tab, const float* sin_tab,
                                  void* stream) {
  if (nK < 1 || nK > 3) return FAIL(FOLEY_ERR_INVALID, "nK must be 1..3");
  QkvSplitArgs a{};
  a.qkv = qkv; a.M = M; a.L = L; a.H = H; a.nK = nK;
  for (int i = 0; i < nK; ++i) {
    a.gain[i] = gain ? gain[i] : nullptr;
    a.pos[i] = pos ? pos[i] : nullptr;
    a.dst[i] = dst[i];
  }
  a.out_dtype = out_dtype; a.vt_pitch = vt_pitch;
  a.S_tot = S_tot; a.tok_off = tok_off; a.eps = eps; a.cos_tab = cos_tab; a.sin_tab = sin_tab;
  return launch_qkv_split(a, (hipStream_t)stream);
}

// The solver step, one entry for every form and option: the descriptor translated into the StepArgs the sampler loop launches
// with.  launch_solver_step checks the form's operands and the ring (a buffer with 1 or 2 slots, or neither).
static int op_solver_step(const foley_step_desc* d, const foley_projection_desc* proj, void* stream) {
  if (!d) return FAIL(FOLEY_ERR_INVALID, "foley_op_solver_step: null descriptor");
  if (d->x0 && d->n_win) return FAIL(FOLEY_ERR_INVALID, "foley_op_solver_step: edit and windows operands exclude each other");
  if (proj) {
    if (proj->mode != FOLEY_GUIDANCE_APG && proj->mode != FOLEY_GUIDANCE_ZERO_STAR)
      return FAIL(FOLEY_ERR_INVALID, "foley_op_solver_step_projected: unknown mode (1 APG, 2 CFG-Zero*)");
    if (!proj->coef || (proj->mode == FOLEY_GUIDANCE_APG && !proj->plane))
      return FAIL(FOLEY_ERR_INVALID, "foley_op_solver_step_projected: the descriptor needs its coefficients and, for APG, its plane");
  }
  StepArgs s{d->pred, d->x, d->x_saved, d->d_acc, d->clips, d->C, d->L, d->ncfg, d->guidance, d->coef, d->step_ptr, d->rows_out, d->rows_dtype};
  s.sched = d->gd.sched; s.clip_scale = d->gd.clip_scale;
  s.form = d->x0 ? STEP_FORM_EDIT : d->n_win ? STEP_FORM_WINDOWS : STEP_FORM_PLAIN;
  s.x0 = d->x0; s.noise = d->noise; s.mask = d->mask; s.x0_clips = d->x0_clips; s.mask_clips = d->mask_clips;
  s.n_win = d->n_win; s.Ltot = d->Ltot; s.starts = d->starts; s.weights = d->weights;
  s.hist = d->hist; s.hist_slots = d->hist_slots;
  if (proj) {
    s.proj_coef = proj->coef;
    s.proj_plane = proj->mode == FOLEY_GUIDANCE_APG ? proj->plane : nullptr;
  }
  return launch_solver_step(s, (hipStream_t)stream);
}
extern "C" int foley_op_solver_step(const foley_step_desc* d, void* stream) { return op_solver_step(d, nullptr, stream); }
extern "C" int foley_op_solver_step_projected(const foley_step_desc* d, const foley_projection_desc* proj, void* stream) {
  return op_solver_step(d, proj, stream);
}

// FlowEdit at op level: the descriptor translated into the FlowEditArgs the sampler loop launches with
static FlowEditArgs flowedit_args_of(const foley_flowedit_desc* d) {
  FlowEditArgs a;
  a.pred = d->pred; a.z = d->z; a.x_src = d->x_src; a.noise = d->noise; a.mask = d->mask; a.coef = d->coef;
  a.step_ptr = d->step_ptr; a.rows_out = d->rows_out;
  a.V = d->V; a.C = d->C; a.L = d->L; a.n_iter = d->n_iter; a.rows_dtype = d->rows_dtype;
  a.src_clips = d->src_clips; a.noise_rows = d->noise_rows; a.mask_clips = d->mask_clips;
  a.g_src = d->g_src; a.g_tar = d->g_tar;
  return a;
}
extern "C" int foley_op_flowedit_step(const foley_flowedit_desc* d, void* stream) {
  if (!d) return FAIL(FOLEY_ERR_INVALID, "foley_op_flowedit_step: null descriptor");
  if (!d->coef || d->n_iter < 1) return FAIL(FOLEY_ERR_INVALID, "foley_op_flowedit_step: coef [n_iter, 8] is required");
  HIPTRY(hipStreamSynchronize((hipStream_t)stream));
  std::vector<float> rows((size_t)d->n_iter * 8);
  HIPTRY(hipMemcpy(rows.data(), d->coef, rows.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < d->n_iter; ++i)
    if (!((int)rows[8 * (size_t)i + 4] & FOLEY_STEP_BLEND))
      return FAIL(FOLEY_ERR_INVALID, "foley_op_flowedit_step: every coef row must carry FOLEY_STEP_BLEND with sigma_{k+1} in column 5");
  return launch_flowedit_step(flowedit_args_of(d), (hipStream_t)stream);
}
extern "C" int foley_op_flowedit_stage(const foley_flowedit_desc* d, float sigma, int noise_row, void* stream) {
  if (!d) return FAIL(FOLEY_ERR_INVALID, "foley_op_flowedit_stage: null descriptor");
  return launch_flowedit_stage(flowedit_args_of(d), sigma, noise_row, (hipStream_t)stream);
}

extern "C" int64_t foley_op_guidance_project_work(int clips, int La) {
  return clips < 1 || La < 1 ? 0 : (int64_t)guidance_project_floats(clips, La);
}

extern "C" int foley_op_guidance_project(const foley_projection_desc* proj, const foley_guidance_desc* gd, const float* pred, int clips,
                                         int C, int La, float guidance, const int32_t* step_ptr, float* work, int64_t work_floats,
                                         void* stream) {
  if (!proj || !proj->rows || !proj->coef)
    return FAIL(FOLEY_ERR_INVALID, "foley_op_guidance_project: the descriptor's rows are read and its coef receives the coefficients");
  if (clips < 1 || La < 1 || !work || work_floats < (int64_t)guidance_project_floats(clips, La))
    return FAIL(FOLEY_ERR_INVALID, "foley_op_guidance_project: work buffer smaller than foley_op_guidance_project_work(clips, La) floats");
  StepArgs s{pred, nullptr, nullptr, nullptr, clips, C, La, 2, guidance, nullptr, (int32_t*)step_ptr, nullptr, FOLEY_F32};
  if (gd) s.sched = gd->sched;
  return launch_guidance_project(s, proj->mode, proj->rows, work, proj->coef, proj->plane, (hipStream_t)stream);
}

extern "C" int64_t foley_op_cache_probe_work(int Bc, int La) { return Bc < 1 || La < 1 ? 0 : (int64_t)cache_probe_floats(Bc, La); }

extern "C" int foley_op_cache_probe(const float* a0, int Bc, int La, int D, float eps, const foley_rowbcast* shift,
                                    const foley_rowbcast* scale, float* m_prev, float* work, int64_t work_floats, float* rel,
                                    void* stream) {
  if (Bc < 1 || La < 1 || work_floats < (int64_t)cache_probe_floats(Bc, La))
    return FAIL(FOLEY_ERR_INVALID, "foley_op_cache_probe: work is smaller than foley_op_cache_probe_work(Bc, La)");
  TRY(launch_cache_probe(a0, Bc, La, D, eps, to_rb(shift), to_rb(scale), m_prev, work, rel, (hipStream_t)stream));
  return 0;
}
extern "C" int foley_op_cache_delta(const float* aN, float* delta, int64_t n, void* stream) {
  TRY(launch_cache_delta(aN, delta, (long)n, (hipStream_t)stream));
  return 0;
}
extern "C" int foley_op_cache_apply(float* audio, const float* delta, int64_t n, void* stream) {
  TRY(launch_cache_apply(audio, delta, (long)n, (hipStream_t)stream));
  return 0;
}

extern "C" int64_t foley_op_guidance_stats_work(int clips, int L) { return clips < 1 || L < 1 ? 0 : (int64_t)guidance_stats_floats(clips, L); }

extern "C" int foley_op_guidance_stats(const foley_guidance_desc* gd, const float* pred, int clips, int C, int L, int ncfg, float guidance,
                                       const int32_t* step_ptr, float rescale, float* work, int64_t work_floats, void* stream) {
  if (!gd || !gd->clip_scale) return FAIL(FOLEY_ERR_INVALID, "foley_op_guidance_stats: the descriptor's clip_scale receives the factors");
  if (clips < 1 || L < 1 || !work || work_floats < (int64_t)guidance_stats_floats(clips, L))
    return FAIL(FOLEY_ERR_INVALID, "foley_op_guidance_stats: work buffer smaller than foley_op_guidance_stats_work(clips, L) floats");
  StepArgs s{pred, nullptr, nullptr, nullptr, clips, C, L, ncfg, guidance, nullptr, (int32_t*)step_ptr, nullptr, FOLEY_F32};
  s.sched = gd->sched; s.clip_scale = gd->clip_scale;
  return launch_guidance_stats(s, work, nullptr, rescale, (float*)gd->clip_scale, (hipStream_t)stream);
}

extern "C" int foley_op_windows_stitch(const float* x, int clips, int n_win, int C, int L, int Ltot, const int32_t* starts,
                                       const float* weights, float* out, void* stream) {
  return launch_windows_stitch(x, clips, n_win, C, L, Ltot, starts, weights, out, (hipStream_t)stream);
}

extern "C" int foley_op_flow_mix(const float* noise, const float* x0, int x0_clips, int clips, int C, int L, float sigma,
                                 float* out, void* stream) {
  return launch_flow_mix(noise, x0, x0_clips, clips, C, L, sigma, out, (hipStream_t)stream);
}

extern "C" int foley_op_latent_rows(const float* x, int clips, int C, int L, int ncfg, void* out, int out_dtype,
                                    void* stream) {
  return launch_latent_rows(x, clips, C, L, ncfg, out, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_dac_out(const float* s, const float* w, const float* bias, int B, int T, int C, float* out,
                                void* stream) {
  return launch_dac_out(s, w, bias, B, T, C, out, (hipStream_t)stream);
}

// Op entries of the row kernels that a sample launches between the GEMM, LayerNorm and attention families (tests/opcheck.py holds
// each of them to a per-element bound): argument checks, then the launcher the runtime itself calls.
extern "C" int foley_op_rows_add_act(const float* a, const float* v, int R, int D, int act_silu, void* out, int out_dtype,
                                     void* stream) {
  if (!out || R < 1 || D < 1) return FAIL(FOLEY_ERR_INVALID, "rows_add_act: null output or empty problem");
  return launch_rows_add_act(a, v ? rb_debug_step(rb_vec(v, 0, nullptr)) : rb_none(), R, D, act_silu ? 1 : 0, out, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_add_periodic(const float* x, const float* pos, int R, int D, int period, void* out, int out_dtype,
                                     void* stream) {
  if (!x || !pos || !out || R < 1 || D < 1 || period < 1) return FAIL(FOLEY_ERR_INVALID, "add_periodic: null argument or empty problem");
  return launch_add_periodic(x, pos, R, D, period, out, out_dtype, (hipStream_t)stream);
}

extern "C" int foley_op_gather_rows(const float* src, const int32_t* idx, int n_idx, int groups, int src_rows, int D, float* out,
                                    void* stream) {
  if (!src || !idx || !out || n_idx < 1 || groups < 1 || src_rows < 1 || D < 1)
    return FAIL(FOLEY_ERR_INVALID, "gather_rows: null argument or empty problem");
  return launch_gather_rows(src, idx, n_idx, groups, src_rows, D, out, (hipStream_t)stream);
}

extern "C" int foley_op_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream) {
  if (!src || !dst || n < 1) return FAIL(FOLEY_ERR_INVALID, "cast: null argument or empty problem");
  return launch_cast(src, src_dtype, dst, dst_dtype, n, (hipStream_t)stream);
}

extern "C" int foley_op_rows_periodic_check(const float* x, int groups, int rows, int period, int D, int32_t* flags, void* stream) {
  if (!x || !flags || groups < 1 || rows < 1 || period < 1 || D < 1)
    return FAIL(FOLEY_ERR_INVALID, "rows_periodic_check: null argument or empty problem");
  return launch_rows_periodic_check(x, groups, rows, period, D, flags, (hipStream_t)stream);
}

extern "C" int foley_op_dac_in(const float* x, const float* w, const float* bias, const float* alpha, int B, int T, int C,
                               float* out0, float* out1, void* stream) {
  if (!x || !w || !bias || !alpha || !out0 || !out1 || B < 1 || T < 1 || C < 1)
    return FAIL(FOLEY_ERR_INVALID, "dac_in: null argument or empty problem");
  if (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)alpha | (uintptr_t)out0 | (uintptr_t)out1) & 15)
    return FAIL(FOLEY_ERR_INVALID, "dac_in: weights, bias, alpha and outputs must be 16-byte aligned");
  return launch_dac_in(x, w, bias, alpha, B, T, C, out0, out1, (hipStream_t)stream);
}

extern "C" int foley_op_rows_to_planes(const float* rows, int B, int T, int C, float* out, void* stream) {
  if (!rows || !out || B < 1 || T < 1 || C < 1) return FAIL(FOLEY_ERR_INVALID, "rows_to_planes: null argument or empty problem");
  return launch_rows_to_planes(rows, B, T, C, out, (hipStream_t)stream);
}

// The CLAP audio tower's kernels (clap_audio.hip; host/clap_score.py)
extern "C" int foley_op_melspec_db(const float* x, int B, int N, const int32_t* starts, int n_win, const float* basis,
                                   const int32_t* mel_lo, const int32_t* mel_len, const float* mel_w, int mel_wp, float* out,
                                   void* stream) {
  if (!x || !starts || !basis || !mel_lo || !mel_len || !mel_w || !out) return FAIL(FOLEY_ERR_INVALID, "melspec_db: null argument");
  return launch_melspec_db(x, B, N, starts, n_win, basis, mel_lo, mel_len, mel_w, mel_wp, out, (hipStream_t)stream);
}

extern "C" int foley_op_spec_patches(const float* spec, int G, int T, int F, const float* scale, const float* shift,
                                     const int32_t* resize_idx, const float* resize_w, int Tq, int ratio, void* out, int out_dtype,
                                     int Kp, void* stream) {
  if (!spec || !scale || !shift || !out || (resize_idx != nullptr) != (resize_w != nullptr))
    return FAIL(FOLEY_ERR_INVALID, "spec_patches: null argument (the resize table is index and weight together)");
  return launch_spec_patches(spec, G, T, F, scale, shift, resize_idx, resize_w, Tq, ratio, out, out_dtype, Kp, (hipStream_t)stream);
}

extern "C" int foley_op_window_attention(const void* qkv, int dtype, int rows, int qkv_cols, int H, int win_tokens,
                                         const int32_t* table, int n_win, const float* bias, const float* mask, int n_mask,
                                         void* out, int out_pitch, void* stream) {
  if (!qkv || !table || !bias || !out) return FAIL(FOLEY_ERR_INVALID, "window_attention: null argument");
  if (win_tokens != 64) return FAIL(FOLEY_ERR_INVALID, "window_attention: serves 64-token windows (8 x 8)");
  if (H < 1 || qkv_cols != 3 * H * 32) return FAIL(FOLEY_ERR_INVALID, "window_attention: serves head dim 32 (qkv [rows, 3 * H * 32])");
  return launch_window_attention(qkv, dtype, rows, H, table, n_win, bias, mask, n_mask, out, out_pitch, (hipStream_t)stream);
}
