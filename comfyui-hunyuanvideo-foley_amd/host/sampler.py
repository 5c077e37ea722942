"""Host orchestration of one sampling run - the MI355X counterpart of
`denoise_process_with_generator` (/utils.py:125-258): draw the noise like the reference does,
replicate / pad the conditioning, hand everything to libfoley_hip.so, decode with the DAC.

PyTorch here only allocates device memory, draws the CPU-generator noise and builds tiny index
tables; every FLOP of the hot path runs in the HIP library.
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import audio_edit as _audio_edit, cond_sets, packers, prompt_timeline as _ptl, runtime, step_cache as _sc, tables
from .config import DAC48K, DACConfig, DiTConfig
from .runtime import FoleyContext, FoleyRuntimeError
from .step_cache import StepCacheSpec


class FoleyModel:
    """The HUNYUAN_MODEL socket payload: packed DiT weights resident on one GPU + its context.

    Mirrors what the reference sampler touches on its nn.Module: `.dtype`,
    `get_empty_clip_sequence`, `get_empty_sync_sequence` (hifi_foley.py:620-632).
    """

    def __init__(self, cfg: DiTConfig, dit_state: Dict[str, torch.Tensor], compute_dtype: torch.dtype,
                 device, dac_cfg: DACConfig = DAC48K, quantization: str = "none"):
        self.cfg, self.dac_cfg = cfg, dac_cfg
        self.dtype = compute_dtype
        self.device = torch.device(device)
        self.quantization = quantization
        # fp8 weight-only storage stays fp8 in HBM (bf16 / fp16 compute); `dit_state` then holds fp8-rounded values
        store = packers.FP8_DTYPES.get(quantization) if compute_dtype in packers.HALF_DTYPES else None
        packed = packers.pack_dit(dit_state, cfg, compute_dtype, weight_store=store)
        self.arena = packers.Arena.from_packed(packed, self.device)
        self._finish_init()

    @classmethod
    def from_arena(cls, cfg: DiTConfig, arena: "packers.Arena", compute_dtype: torch.dtype, device,
                   dac_cfg: DACConfig = DAC48K, quantization: str = "none") -> "FoleyModel":
        """Adopt an already packed arena (e.g. one received by broadcast on a non-root rank)."""
        self = cls.__new__(cls)
        self.cfg, self.dac_cfg, self.dtype, self.device = cfg, dac_cfg, compute_dtype, torch.device(device)
        self.quantization = quantization
        self.arena = arena
        self._finish_init()
        return self

    @classmethod
    def from_reference_state(cls, cfg: DiTConfig, dit_state: Dict[str, torch.Tensor], compute_dtype: torch.dtype, device,
                             dac_state: Dict[str, torch.Tensor], dac_cfg: DACConfig = DAC48K,
                             quantization: str = "none") -> "FoleyModel":
        """Load through the C ABI's reference-keyed path (foley_load_tensor): the library packs the checkpoint
        tensors on the device into its own arena - no host/packers.py involved.  `dit_state` is expected to hold
        the parameter values the reference module would hold (nodes.round_params / fp8_round_state_dict)."""
        self = cls.__new__(cls)
        self.cfg, self.dac_cfg, self.dtype, self.device = cfg, dac_cfg, compute_dtype, torch.device(device)
        self.quantization = quantization
        self.arena = None
        self.ctx = FoleyContext(cfg, dac_cfg, compute_dtype, self.device)
        fmt = {"fp8_e4m3fn": 1, "fp8_e5m2": 2}.get(quantization, 0) if compute_dtype in packers.HALF_DTYPES else 0
        self.ctx.load_reference_state([dit_state, dac_state], fmt)
        self.empty_clip_feat = dit_state["empty_clip_feat"].detach().to(self.device, torch.float32).reshape(1, -1)
        self.empty_sync_feat = dit_state["empty_sync_feat"].detach().to(self.device, torch.float32).reshape(1, -1)
        self._dac_arena = "ctx-owned"
        self._text_len_fixed = None
        return self

    def _finish_init(self):
        self.ctx = FoleyContext(self.cfg, self.dac_cfg, self.dtype, self.device)
        self.ctx.set_tensors((k, v) for k, v in self.arena.items() if not k.startswith("empty_"))
        self.empty_clip_feat = self.arena.view("empty_clip").view(1, -1)
        self.empty_sync_feat = self.arena.view("empty_sync").view(1, -1)
        self._dac_arena = None
        self._text_len_fixed = None

    def get_empty_clip_sequence(self, bs=None, len=None):
        e = self.empty_clip_feat
        return e.expand(len, -1) if bs is None else e.unsqueeze(0).expand(bs, len, -1)

    def get_empty_sync_sequence(self, bs=None, len=None):
        e = self.empty_sync_feat
        return e.expand(len, -1) if bs is None else e.unsqueeze(0).expand(bs, len, -1)

    def attach_dac(self, dac: "FoleyDAC"):
        if dac is None:
            if self._dac_arena != "ctx-owned":
                raise FoleyRuntimeError("no DAC decoder: pass a FoleyDAC or load it by reference key")
            return                                                 # decoder weights were loaded by reference key
        if self._dac_arena is not dac.arena:
            self.ctx.set_tensors(dac.arena.items())
            self._dac_arena = dac.arena

    def to(self, *a, **k):   # placement is fixed at load time; kept for reference-API compatibility
        return self


class FoleyDAC:
    """Packed DAC-VAE decoder (the `dac_model` entry of HUNYUAN_DEPS)."""

    sample_rate = 48000

    def __init__(self, dac_state: Dict[str, torch.Tensor], device, cfg: DACConfig = DAC48K):
        self.cfg = cfg
        self.sample_rate = cfg.sample_rate
        self.device = torch.device(device)
        packed = packers.pack_dac(dac_state, cfg)
        self.has_encoder = packers.has_dac_encoder(dac_state)
        if self.has_encoder:     # full checkpoints (the reference loads them strict=True) also carry the encoder
            packed.update(packers.pack_dac_encoder(dac_state, cfg))
        self.arena = packers.Arena.from_packed(packed, self.device)

    @classmethod
    def from_arena(cls, arena, device, cfg: DACConfig = DAC48K):
        self = cls.__new__(cls)
        self.cfg, self.sample_rate, self.device, self.arena = cfg, cfg.sample_rate, torch.device(device), arena
        self.has_encoder = "enc.in.w" in arena.table
        return self


def pad_or_trim_text(x: torch.Tensor, t_fixed: int) -> torch.Tensor:
    T = x.shape[1]
    if T == t_fixed:
        return x
    if T > t_fixed:
        return x[:, :t_fixed]
    return F.pad(x, (0, 0, 0, t_fixed - T))


def draw_noise(batch_size: int, channels: int, length: int, dtype: torch.dtype,
               generator: Optional[torch.Generator]) -> torch.Tensor:
    """prepare_latents_with_generator (utils.py:114-121): CPU generator, *model* dtype."""
    return torch.randn((batch_size, channels, int(length)), generator=generator, device="cpu", dtype=dtype)


def fp8_time_dtype(model):
    """fp8 type the timestep features are rounded through, or None: an fp8-wrapped reference model
    under bf16/fp16 autocast casts them to fp8 (embed_layers.py:134, golden g8)."""
    if getattr(model, "quantization", "none") == "none" or model.dtype == torch.float32:
        return None
    return torch.float8_e4m3fn if model.quantization == "fp8_e4m3fn" else torch.float8_e5m2


@dataclass(frozen=True)
class ProjectionSpec:
    """Projected guidance in place of the two-half combine (foley_set_projected_guidance, tables.projection_rows).
      mode            "apg": adaptive projected guidance (Sadat et al. 2024) - the guidance difference c - u is averaged over the
                      iterations with weight `momentum`, clipped to the norm `norm_threshold` and split into the part parallel to
                      the conditional prediction, which `eta` scales, and the orthogonal part.  eta = 1, momentum = 0 and no
                      threshold is plain CFG to rounding (not bit for bit).
                      "cfg_zero_star": CFG-Zero* (Fan et al. 2025) - the unconditional prediction is scaled by <c,u>/<u,u> per
                      clip before the combine.
      eta             APG, in [0, 1].
      momentum        APG, |momentum| < 1 (the paper's default is negative).
      norm_threshold  APG, >= 0, in the model's velocity units (uncalibrated for this model); 0: no clip.
      zero_init       the first `zero_init` loop iterations of the full run use a zero velocity (both modes)."""
    mode: str
    eta: float = 0.0
    momentum: float = -0.5
    norm_threshold: float = 0.0
    zero_init: int = 0

    def check(self, steps: Optional[int] = None) -> None:
        if self.mode not in tables.PROJECTION_MODES:
            raise ValueError(f"guidance_mode must be one of {list(tables.PROJECTION_MODES)}, got {self.mode!r}")
        for name in ("eta", "momentum", "norm_threshold"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"projection {name} must be a finite number, got {v!r}")
        if not 0.0 <= float(self.eta) <= 1.0:
            raise ValueError(f"apg eta must lie in [0, 1], got {self.eta}")
        if not abs(float(self.momentum)) < 1.0:
            raise ValueError(f"apg momentum must satisfy |momentum| < 1, got {self.momentum}")
        if float(self.norm_threshold) < 0.0:
            raise ValueError(f"apg norm_threshold must be >= 0, got {self.norm_threshold}")
        z = self.zero_init
        if isinstance(z, bool) or not isinstance(z, int) or z < 0:
            raise ValueError(f"zero_init_steps must be an integer >= 0, got {z!r}")
        if steps is not None and z >= int(steps):
            raise ValueError(f"zero_init_steps ({z}) must be smaller than the number of steps ({int(steps)})")


@dataclass(frozen=True)
class GuidanceSpec:
    """How the prediction halves become one velocity, beyond the scalar `guidance_scale` (which stays the text scale and the
    only scale of a two-half run).
      g_video   not None: three halves - h0 negative prompt + the learned empty visual rows, h1 negative prompt + the clip's
                visual features, h2 prompt + the same features - combined as v = p0 + g_video (p1 - p0) + g_text (p2 - p1).
      interval  (start, end) in fractions of the loop: the scales hold on the iterations with start <= i / n_iter < end, the
                others use (1, 1).  Every half still runs on every iteration (the run keeps its shape).
      rescale   phi in [0, 1]: the step uses f v, f = phi std(h_last) / std(v) + (1 - phi) per clip (windows: per window).
      projection  a ProjectionSpec: APG or CFG-Zero* in place of the two-half combine (two halves only: no video scale, no
                rescale, guidance_scale > 1); it combines with the interval."""
    g_video: Optional[float] = None
    interval: Optional[Tuple[float, float]] = None
    rescale: float = 0.0
    projection: Optional[ProjectionSpec] = None

    def check(self, guidance_scale: float, steps: Optional[int] = None) -> None:
        if self.projection is not None:
            self.projection.check(steps)
            if self.g_video is not None:
                raise ValueError("projected guidance takes two halves: it does not combine with a video scale (video_cfg_scale)")
            if float(self.rescale) > 0.0:
                raise ValueError("projected guidance does not combine with cfg_rescale > 0")
            if not guidance_scale > 1.0:
                raise ValueError(f"projected guidance needs guidance: cfg_scale > 1, got {guidance_scale}")
        if not 0.0 <= float(self.rescale) <= 1.0:
            raise ValueError(f"guidance rescale must lie in [0, 1], got {self.rescale}")
        if self.g_video is None and not guidance_scale > 1.0 and (self.interval is not None or self.rescale > 0.0):
            raise ValueError("a guidance interval / rescale needs guidance: guidance_scale > 1 or a video scale (g_video)")


@dataclass(frozen=True)
class MultistepSpec:
    """A linear multistep solver on top of `euler`: variable-step Adams-Bashforth of `order` 2 or 3 at one model call per sigma
    step (tables.solver_table(multistep_order=), foley_set_multistep).  The first step of a run is Euler's and the second step of
    an order-3 run is order 2, so order 3 is a third-order local formula behind a first-order first step: globally second order,
    with a smaller constant.  It does not combine with the multi-stage solvers."""
    order: int = 2

    def check(self, sampler: str) -> None:
        o = self.order
        if isinstance(o, bool) or not isinstance(o, (int, float)) or int(o) != o or int(o) not in tables.MULTISTEP_ORDERS:
            raise ValueError(f"multistep order must be one of {list(tables.MULTISTEP_ORDERS)}, got {o!r}")
        if sampler != "euler":
            raise ValueError(f"a multistep order needs the euler solver (one model call per sigma step), got {sampler!r}: "
                             "heun-2, midpoint-2 and kutta-4 do not combine with it")


def apply_multistep(ctx: FoleyContext, plan: dict) -> None:
    """foley_set_multistep with what build_plan put into the plan (after prepare, next to the other apply_* calls)."""
    if plan.get("multistep_order"):
        ctx.set_multistep(int(plan["multistep_order"]))


def _ms_kw(multistep) -> dict:
    """The multistep keyword for a callee, only when it is set: an unset one adds nothing to the call."""
    return {} if multistep is None else {"multistep": multistep}


def apply_guidance(ctx: FoleyContext, plan: dict) -> None:
    """foley_set_guidance with what build_plan put into the plan (after prepare, next to set_edit / set_windows)."""
    if plan.get("guid_sched") is not None or plan.get("guid_rescale", 0.0) > 0.0:
        ctx.set_guidance(plan.get("guid_sched"), plan.get("guid_rescale", 0.0))
    if plan.get("proj_rows") is not None:
        ctx.set_projected_guidance(int(plan["proj_mode"]), plan["proj_rows"])


def apply_step_cache(ctx: FoleyContext, plan: dict) -> None:
    """foley_set_step_cache with what build_plan put into the plan (after prepare, next to apply_guidance / set_edit / set_windows)."""
    sc = plan.get("step_cache")
    if sc is not None:
        ctx.set_step_cache(**sc)


def prepare_run(model: "FoleyModel", dac, plan: dict) -> None:
    """The start of every run: the DAC weights, foley_prepare of the plan, then the options build_plan put into it (set_edit /
    set_windows follow at the caller, with their operands)."""
    model.attach_dac(dac)
    model.ctx.prepare(plan)
    apply_guidance(model.ctx, plan)
    apply_step_cache(model.ctx, plan)
    apply_multistep(model.ctx, plan)


def keep_step_cache_report(ctx: FoleyContext, plan: dict) -> None:
    """After the loop: plan["step_cache_report"] = {"rel": [...], "skipped": [...]} (the node logs it)."""
    if plan.get("step_cache") is None:
        return
    rel, skipped = ctx.step_cache_report()
    plan["step_cache_report"] = {"rel": rel, "skipped": skipped}


def build_plan(model: FoleyModel, visual_feats: Dict[str, torch.Tensor], text_feats: Dict[str, torch.Tensor],
               La: int, guidance_scale: float, steps: int, batch_size: int, sampler: str,
               edit_i0: Optional[int] = None, guidance: Optional[GuidanceSpec] = None,
               step_cache: Optional[StepCacheSpec] = None, timeline=None, timeline_starts=None,
               multistep: Optional[MultistepSpec] = None) -> dict:
    """Conditioning replication / padding / CFG stacking of utils.py:159-199 + the run's tables.
    edit_i0 (edit runs, host/audio_edit.py): the tables of the suffix [edit_i0, steps) with the blend rows.
    Each conditioning tensor has batch 1 (shared by all clips) or batch_size (one row per clip, host/cond_sets.py): the plan
    then holds the distinct sets and the maps `text_of` / `vis_of` (None when every clip shares its conditioning).
    guidance (GuidanceSpec): three halves when it carries a video scale, and the schedule table / rescale value that
    apply_guidance hands to the library after prepare (`guid_sched`, `guid_rescale`).
    step_cache (StepCacheSpec, host/step_cache.py): the arguments apply_step_cache hands to the library after prepare
    (`step_cache`); an edit run takes the rows [edit_i0, steps) of a skip list and of an interval, as of the guidance table.
    timeline (host/prompt_timeline.Timeline): text_feats["text_feat"] holds one row per distinct prompt of the timeline, in its
    order, and the visual features are shared (batch 1); the plan then carries the text sets [negative ; prompts...] and the
    per-token table `timeline` that prepare hands to foley_prepare_timeline.  timeline_starts: the latent-frame starts of a
    windowed run - clip v*n_win + k reads the timeline shifted by starts[k].  None is today's path, bit for bit.
    multistep (MultistepSpec): Adams-Bashforth rows in solver_coef (an edit run's warm-up begins at edit_i0) and the order that
    apply_multistep hands to the library after prepare (`multistep_order`)."""
    cfg, dev = model.cfg, model.device
    if multistep is not None:
        multistep.check(sampler)
    if step_cache is not None:
        step_cache.check(int(steps))
    if guidance is not None:
        guidance.check(guidance_scale, int(steps))
    three = guidance is not None and guidance.g_video is not None
    use_cfg = guidance_scale > 1.0 or three
    f32 = lambda t: t.to(device=dev, dtype=torch.float32)
    clip, sync = f32(visual_feats["siglip2_feat"]), f32(visual_feats["syncformer_feat"])
    text, unc = f32(text_feats["text_feat"]), f32(text_feats["uncond_text_feat"])
    text_sets = None
    if timeline is not None:
        if text.dim() != 3 or text.shape[0] != len(timeline.prompts):
            raise FoleyRuntimeError(f"timeline=: text_feat carries {tuple(text.shape)}, one row per distinct prompt of the timeline "
                                    f"({len(timeline.prompts)}) is needed")
        if clip.shape[0] != 1 or sync.shape[0] != 1 or unc.shape[0] != 1:
            raise FoleyRuntimeError("timeline=: the visual features and the negative prompt are shared by the clips (batch 1); "
                                    "a timeline does not combine with per-clip conditioning")
        text_sets, text = text, text[:1]
    try:
        per_clip = any(cond_sets.batch_of(t, batch_size, n) > 1 for t, n in (
            (clip, "siglip2_feat"), (sync, "syncformer_feat"), (text, "text_feat"), (unc, "uncond_text_feat")))
    except cond_sets.CondSetsError as e:
        raise FoleyRuntimeError(str(e)) from None
    Lv, Ls = clip.shape[1], sync.shape[1]
    # two-bucket text length policy, sticky per model (utils.py:166-188)
    t_fixed = min(77 if text.shape[1] <= 77 else 128, cfg.text_len)
    model._text_len_fixed = max(model._text_len_fixed or 0, t_fixed)
    Lt = model._text_len_fixed
    text, unc = pad_or_trim_text(text, Lt), pad_or_trim_text(unc, Lt)
    if text_sets is not None:
        text_sets = pad_or_trim_text(text_sets, Lt)
    text_of = vis_of = None
    if per_clip:
        sets = cond_sets.build(text, unc, clip, sync, model.empty_clip_feat, model.empty_sync_feat, batch_size,
                               use_cfg, three)
        if sets.homogeneous:          # every clip shares its conditioning: the batch-1 plan exactly
            h = sets.text.shape[0] - 1
            text, clip, sync = sets.text[h:h + 1], sets.clip[h:h + 1], sets.sync[h:h + 1]
            unc = sets.text[:1]
            per_clip = False
        else:
            text_in, clip_in, sync_in, text_of, vis_of = sets.text, sets.clip, sets.sync, sets.text_of, sets.vis_of
    ncfg = 3 if three else 2 if use_cfg else 1
    if per_clip:                                  # distinct sets in [uncond ; cond] order, the maps say which row reads which
        pass
    elif three:                                   # [negative + empty rows ; negative + video ; prompt + video]
        text_in = torch.cat([unc, unc, text])
        clip_in = torch.cat([model.get_empty_clip_sequence(bs=1, len=Lv).float(), clip, clip])
        sync_in = torch.cat([model.get_empty_sync_sequence(bs=1, len=Ls).float(), sync, sync])
    elif use_cfg:                                 # [uncond ; cond]  (utils.py:193-195)
        text_in = torch.cat([unc, text])
        clip_in = torch.cat([model.get_empty_clip_sequence(bs=1, len=Lv).float(), clip])
        sync_in = torch.cat([model.get_empty_sync_sequence(bs=1, len=Ls).float(), sync])
    else:
        text_in, clip_in, sync_in = text, clip, sync
    if text_sets is not None:                     # [negative ; prompts...]: the halves below the last read set 0 (prompt_timeline.batch_table)
        text_in = torch.cat([unc, text_sets]) if ncfg > 1 else text_sets
    fp8_time = fp8_time_dtype(model)
    # The run's tables (schedule, solver coefficients, RoPE rows, position / up-sampling maps) depend on these scalars
    # only: built once per distinct run shape and kept on the device (host-side table building is milliseconds of
    # Python per call - more than the whole precompute on the GPU)
    ms_order = int(multistep.order) if multistep is not None else None
    key = (La, Lv, Ls, Lt, steps, sampler, ms_order, float(cfg.flow_shift), cfg.time_freq_dim, str(fp8_time), str(dev), edit_i0)
    cache = model.__dict__.setdefault("_tables_cache", {})
    tabs = cache.get(key)
    if tabs is None:
        ms = {} if ms_order is None else {"multistep_order": ms_order, "start": edit_i0 or 0}
        tb = tables.build_tables(La, Lv, Ls, Lt, steps, sampler, cfg.flow_shift, cfg.time_freq_dim, fp8_time=fp8_time,
                                 edit_i0=edit_i0, **ms)
        tabs = {k: tb[k].to(dev).contiguous() for k in ("t_feat", "rope_cos", "rope_sin", "pos_audio_self", "pos_visual_self",
                                                        "pos_linear", "sync_gather", "solver_coef")}
        if len(cache) >= 16:
            cache.pop(next(iter(cache)))
        cache[key] = tabs
    plan = {"ncfg": ncfg, "clips": batch_size, "La": La, "Lv": Lv, "Ls": Ls, "Lt": Lt, "n_iter": tabs["solver_coef"].shape[0],
            "guidance": float(guidance_scale), "rope_len": tabs["rope_cos"].shape[0],
            "text": text_in.contiguous(), "clip": clip_in.contiguous(), "sync": sync_in.contiguous(),
            "text_of": text_of, "vis_of": vis_of}
    plan.update(tabs)
    if timeline is not None:
        # the per-token tables depend on the timeline and the run's shape only: kept per model, keyed on both
        tkey = (timeline.key(), Lv, La, ncfg, batch_size, tuple(timeline_starts) if timeline_starts is not None else None)
        tcache = model.__dict__.setdefault("_timeline_cache", {})
        if tkey not in tcache:
            if len(tcache) >= 16:
                tcache.pop(next(iter(tcache)))
            tcache[tkey] = _ptl.batch_table(timeline, Lv, La, ncfg, batch_size, timeline_starts)
        plan["timeline"] = tcache[tkey]
    if guidance is not None and (three or guidance.interval is not None):
        # two halves read column 0: the one scale of the run; an edit run takes the suffix of the plain run's rows
        sched = tables.guidance_schedule(steps, guidance.g_video if three else guidance_scale, guidance_scale, guidance.interval)
        plan["guid_sched"] = sched[edit_i0 or 0:].contiguous()
    if guidance is not None:
        plan["guid_rescale"] = float(guidance.rescale)
    if guidance is not None and guidance.projection is not None:
        # an edit run takes the suffix of the plain run's rows; its first row starts the momentum average
        pj = guidance.projection
        plan["proj_mode"] = tables.PROJECTION_MODES[pj.mode]
        plan["proj_rows"] = tables.projection_rows(steps, pj.mode, pj.eta, pj.momentum, pj.norm_threshold, pj.zero_init,
                                                   start=edit_i0 or 0)
    if ms_order is not None:
        plan["multistep_order"] = ms_order
    if step_cache is not None:
        i0 = edit_i0 or 0
        if step_cache.mode == _sc.MODE_SCHEDULE:
            plan["step_cache"] = {"mode": _sc.MODE_SCHEDULE, "skip": step_cache.skip_rows(int(steps), i0)}
        else:
            plan["step_cache"] = {"mode": _sc.MODE_THRESHOLD, "threshold": float(step_cache.threshold), "poly": step_cache.poly,
                                  "interval": step_cache.interval_rows(int(steps), i0),
                                  "max_consecutive": int(step_cache.max_consecutive or 0)}
    return plan


def denoise_process_with_generator(visual_feats, text_feats, audio_len_in_s, model: FoleyModel, dac: FoleyDAC,
                                   guidance_scale: float, num_inference_steps: int, batch_size: int, sampler: str,
                                   generator: Optional[torch.Generator] = None, use_graph: bool = True,
                                   progress: Optional[Callable[[int, int], None]] = None,
                                   return_latents: bool = False, noise: Optional[torch.Tensor] = None,
                                   _abort_event: Optional[threading.Event] = None, edit=None, windows=None,
                                   guidance: Optional[GuidanceSpec] = None, step_cache: Optional[StepCacheSpec] = None,
                                   timeline=None, multistep: Optional[MultistepSpec] = None):
    """Same contract as the reference function of this name (utils.py:125-258):
    returns (audio [bs, 1, T] fp32 on the model's device, sample_rate).

    edit (host/audio_edit.EditSpec: x0, strength, mask): audio-to-audio / span regeneration - the suffix of the plain run's
    iterations that `strength` selects, started from the source latents x0 noised to that point, with the kept frames of the
    mask held on the source's forward-noised path (foley_set_edit).  The noise is drawn exactly as for a plain run.
    A host/audio_edit.FlowEditSpec (x0, strength, mask, source_scale, noise) is a FlowEdit run instead - see _denoise_flowedit:
    text_feats carries `source_text_feat` (batch 1) next to `text_feat` (the target, batch 1), batch_size is the number of
    variations V, and the model runs a batch of 2V clips.  It takes none of the other options.

    windows (host/long_form.WindowPlan): a long clip as one batch of overlapping windows - see _denoise_windows.  A plan of
    one window takes the plain path exactly; `windows` together with `edit` is refused.

    guidance (GuidanceSpec): separate video / text scales (three halves), a guidance interval and CFG rescale; it combines
    with `edit` and with `windows`.  None is the plain run, bit for bit.

    step_cache (StepCacheSpec): skip the blocks on iterations whose model input barely moved (threshold mode) or on listed
    iterations (schedule mode) and reuse their last residual; it combines with guidance, `edit` and `windows`.  The decisions of
    the run are kept in model.ctx.plan["step_cache_report"].  None runs every block on every iteration, bit for bit.

    timeline (host/prompt_timeline.Timeline): timed prompts - text_feats["text_feat"] holds one row per distinct prompt of the
    timeline and every token of the cross-attention reads the text set(s) of its own time (build_plan).  It combines with `edit`,
    `windows` (the timeline is given in the long clip's time), guidance and the step cache; the visual features are shared
    (batch 1).  None is the plain run, bit for bit.

    multistep (MultistepSpec): Adams-Bashforth order 2 or 3 on the `euler` schedule, one model call per step; it combines with
    `edit` (the warm-up begins where the edit run does), `windows`, guidance, the step cache and a timeline.  None is the plain
    run, bit for bit, with its single captured graph."""
    if multistep is not None:
        multistep.check(sampler)
    if isinstance(edit, _audio_edit.FlowEditSpec):
        if any(o is not None for o in (windows, guidance, step_cache, timeline, multistep, noise)):
            raise ValueError("a FlowEdit run (edit=FlowEditSpec) takes no windows, guidance controls, step cache, timeline, multistep "
                             "order or preset noise: it draws its own noise table from the generator")
        return _denoise_flowedit(visual_feats, text_feats, audio_len_in_s, model, dac, guidance_scale, num_inference_steps, batch_size,
                                 sampler, edit, generator, use_graph, progress, return_latents, _abort_event)
    if windows is not None and windows.n_win > 1:
        if edit is not None:
            raise ValueError("windows= and edit= together: editing a long clip is not supported")
        return _denoise_windows(visual_feats, text_feats, model, dac, guidance_scale, num_inference_steps, batch_size, sampler,
                                windows, generator, use_graph, progress, return_latents, noise, _abort_event, guidance, step_cache,
                                timeline, **_ms_kw(multistep))
    cfg = model.cfg
    La = int(audio_len_in_s * cfg.frame_rate)
    if noise is None:
        noise = draw_noise(batch_size, cfg.latent_dim, La, model.dtype, generator)
    latents = noise.to(device=model.device, dtype=torch.float32).contiguous()
    if edit is None:
        plan = build_plan(model, visual_feats, text_feats, La, guidance_scale, num_inference_steps, batch_size, sampler,
                          guidance=guidance, step_cache=step_cache, timeline=timeline, **_ms_kw(multistep))
        prepare_run(model, dac, plan)
    else:
        k0, i0 = tables.edit_start(num_inference_steps, sampler, edit.strength)
        x0, mask = edit.device_operands(model.device, batch_size, La)
        plan = build_plan(model, visual_feats, text_feats, La, guidance_scale, num_inference_steps, batch_size, sampler,
                          edit_i0=i0, guidance=guidance, step_cache=step_cache, timeline=timeline, **_ms_kw(multistep))
        prepare_run(model, dac, plan)
        model.ctx.set_edit(x0, latents, mask)
        sigma0 = float(tables.sigma_grid(num_inference_steps, cfg.flow_shift)[k0])
        latents = runtime.op_flow_mix(latents, x0, sigma0)
    if _abort_event is not None and _abort_event.is_set():      # another replica of a data-parallel run failed meanwhile
        raise FoleyRuntimeError("sampling aborted: another replica failed")
    model.ctx.sample(latents, use_graph=use_graph, progress=progress)
    keep_step_cache_report(model.ctx, plan)
    audio = model.ctx.dac_decode(latents)
    # (the reference's "trim to exact length" slices the size-1 channel axis: a no-op)
    sr = dac.sample_rate if dac is not None else model.dac_cfg.sample_rate
    if return_latents:
        return audio, sr, latents
    return audio, sr


def flowedit_features(visual_feats, text_feats, V: int):
    """The conditioning of the 2V-clip pair batch [src_0 .. src_{V-1}, tar_0 .. tar_{V-1}]: the source prompt's row for the first V
    clips, the target's for the others; the visual features and the negative prompt are shared (batch 1)."""
    src, tar, unc = text_feats.get("source_text_feat"), text_feats["text_feat"], text_feats["uncond_text_feat"]
    if src is None:
        raise ValueError("a FlowEdit run needs text_feats['source_text_feat'] (the source prompt, batch 1) next to 'text_feat' (the target)")
    for t, what in ((src, "source_text_feat"), (tar, "text_feat"), (unc, "uncond_text_feat"), (visual_feats["siglip2_feat"], "siglip2_feat"),
                    (visual_feats["syncformer_feat"], "syncformer_feat")):
        if t.dim() != 3 or t.shape[0] != 1:
            raise ValueError(f"a FlowEdit run shares its conditioning among the variations: {what} must have batch 1, got {tuple(t.shape)}")
    Lt = max(src.shape[1], tar.shape[1])
    src, tar = pad_or_trim_text(src, Lt), pad_or_trim_text(tar.to(src), Lt)
    text = torch.cat([src.expand(V, -1, -1), tar.expand(V, -1, -1)])
    return dict(visual_feats), {"text_feat": text, "uncond_text_feat": unc}


def _denoise_flowedit(visual_feats, text_feats, audio_len_in_s, model: FoleyModel, dac: FoleyDAC, guidance_scale, num_inference_steps,
                      variations, sampler, edit, generator, use_graph, progress, return_latents, _abort_event):
    """FlowEdit (host/audio_edit.FlowEditSpec): every variation is a (source-prompt, target-prompt) pair of batch clips, so the
    plan is a 2V-clip per-clip-prompt CFG batch over the suffix [i0, steps) of the euler run with the blend rows; the state is
    z [V, C, La], started at the source latents, and the library's step integrates the difference of the pair's guided velocities
    (foley_set_flowedit).  The noise table is ONE draw [n_iter | 1, V, C, La] from the run's generator (audio_edit.flowedit_noise).
    The run takes one device: denoise_process_multi does not shard it, a pair must not be split."""
    edit.check(sampler, guidance_scale)
    cfg = model.cfg
    V = int(variations)
    La = int(audio_len_in_s * cfg.frame_rate)
    k0, i0 = tables.edit_start(num_inference_steps, sampler, edit.strength)
    x0, mask = edit.device_operands(model.device, V, La)
    vis, txt = flowedit_features(visual_feats, text_feats, V)
    plan = build_plan(model, vis, txt, La, guidance_scale, num_inference_steps, 2 * V, sampler, edit_i0=i0)
    prepare_run(model, dac, plan)
    table = _audio_edit.flowedit_noise(generator, edit.n_rows(plan["n_iter"]), V, cfg.latent_dim, La, model.dtype)
    table = table.to(device=model.device, dtype=torch.float32, non_blocking=True).contiguous()
    sigma0 = float(tables.sigma_grid(num_inference_steps, cfg.flow_shift)[k0])
    model.ctx.set_flowedit(x0, table, mask, g_src=float(edit.source_scale), g_tar=float(guidance_scale), sigma0=sigma0)
    latents = x0.expand(V, -1, -1).contiguous().clone()
    if _abort_event is not None and _abort_event.is_set():
        raise FoleyRuntimeError("sampling aborted: another replica failed")
    model.ctx.sample(latents, use_graph=use_graph, progress=progress)
    audio = model.ctx.dac_decode(latents)
    sr = dac.sample_rate if dac is not None else model.dac_cfg.sample_rate
    if return_latents:
        return audio, sr, latents
    return audio, sr


def window_rows(t: torch.Tensor, variations: int, n_win: int, what: str) -> torch.Tensor:
    """A conditioning tensor of a windowed run -> 1 row (shared) or variations*n_win rows (clip v*n_win + k): it carries 1 row,
    n_win rows (one per window, repeated for every variation) or variations*n_win rows."""
    if t.dim() != 3 or t.shape[0] not in (1, n_win, variations * n_win):
        raise ValueError(f"{what} has shape {tuple(t.shape)}: a windowed run takes 1 row, n_win ({n_win}) rows or "
                         f"variations*n_win ({variations * n_win}) rows of [tokens, channels]")
    if t.shape[0] == n_win and variations > 1:
        return t.repeat(variations, 1, 1)
    return t


def _denoise_windows(visual_feats, text_feats, model: FoleyModel, dac: FoleyDAC, guidance_scale, num_inference_steps,
                     variations, sampler, windows, generator, use_graph, progress, return_latents, noise, _abort_event,
                     guidance=None, step_cache=None, timeline=None, multistep=None):
    """One long clip per variation as a batch of variations*n_win coupled windows (clip v*n_win + k = window k of variation v).
    The noise is drawn ONCE as [variations, C, Ltot] - draw_noise, the same generator and dtype rule as a plain run - and every
    window takes its slice, so overlapping frames start equal.  The plan carries the blend rows (edit_i0 = 0 tables); after every
    solver step the library replaces the frames several windows cover by their weighted mean (foley_set_windows).  After the loop
    the windows are stitched and decoded in ONE dac_decode of [variations, C, Ltot]; return_latents gives the stitched latents.
    The length of the run is the plan's (Ltot), not audio_len_in_s.  denoise_process_multi does not shard such a run: the windows
    of a variation are coupled.  timeline: given in the long clip's time; window k's rows are the timeline shifted by starts[k]
    latent frames, which lifts the "one prompt for all windows" limit - the visual features are then one shared row.
    multistep: every window keeps the history of its own velocities; the blend leaves them as the step used them."""
    cfg = model.cfg
    n_win, La, Ltot = windows.n_win, windows.La, windows.Ltot
    windows.check_extent(variations)
    clips = variations * n_win
    vis = {k: window_rows(visual_feats[k], variations, n_win, k) for k in ("siglip2_feat", "syncformer_feat")}
    if timeline is not None:                      # text rows are the timeline's prompts, not windows (build_plan checks them)
        if any(v.shape[0] != 1 for v in vis.values()):
            raise ValueError("windows= with timeline=: the visual features are one shared row (per-window video features are not carried)")
        txt = dict(text_feats)
    else:
        txt = {k: window_rows(text_feats[k], variations, n_win, k) for k in ("text_feat", "uncond_text_feat")}
    if noise is None:
        noise = draw_noise(variations, cfg.latent_dim, Ltot, model.dtype, generator)
    if tuple(noise.shape) != (variations, cfg.latent_dim, Ltot):
        raise ValueError(f"noise of a windowed run is [variations, C, Ltot] = {(variations, cfg.latent_dim, Ltot)}, got {tuple(noise.shape)}")
    noise = noise.to(device=model.device, dtype=torch.float32)
    latents = torch.stack([noise[v, :, s:s + La] for v in range(variations) for s in windows.starts]).contiguous()
    plan = build_plan(model, vis, txt, La, guidance_scale, num_inference_steps, clips, sampler, edit_i0=0, guidance=guidance,
                      step_cache=step_cache, timeline=timeline, timeline_starts=windows.starts if timeline is not None else None,
                      **_ms_kw(multistep))
    prepare_run(model, dac, plan)
    weights = windows.weights.to(model.device)
    model.ctx.set_windows(windows.starts, weights)
    if _abort_event is not None and _abort_event.is_set():
        raise FoleyRuntimeError("sampling aborted: another replica failed")
    model.ctx.sample(latents, use_graph=use_graph, progress=progress)
    keep_step_cache_report(model.ctx, plan)
    starts = torch.tensor(windows.starts, dtype=torch.int32, device=model.device)
    stitched = runtime.op_windows_stitch(latents, starts, weights, Ltot)
    audio = model.ctx.dac_decode(stitched)
    sr = dac.sample_rate if dac is not None else model.dac_cfg.sample_rate
    if return_latents:
        return audio, sr, stitched
    return audio, sr


# ----------------------------------------------------------------------------- node-level data parallelism
def replicate(model: FoleyModel, dac: Optional[FoleyDAC], devices: Sequence) -> List:
    """One (FoleyModel, FoleyDAC) pair per device of `devices` for clip-level data parallelism inside ONE
    process (the ComfyUI case: a single prompt-worker process that sees all GPUs of the node).  The pair of the
    device the model already lives on is reused; all other devices receive the packed DiT arena and the DAC arena in
    ONE grouped RCCL broadcast over xGMI (`runtime.bcast_local` -> foley_bcast_local: ncclCommInitAll over the device
    list, one ncclBroadcast per (device, arena) inside ncclGroupStart / End) - the in-process counterpart of the single
    broadcast of host/distributed.py; `model.last_broadcast_s` keeps its wall time.  A second context on a device that
    already holds one (the 1-GPU test set-up: RCCL communicators want distinct devices) takes a device-local copy.
    Replicas are cached on the model.  A root that carries merged LoRA adapters (host/lora.py) is restored before its arena
    is copied, and the set is then ensured on the root and on every replica returned, so each context owns its pristine copies."""
    from . import runtime as _rt
    if model.arena is None:
        raise FoleyRuntimeError("replicate() needs a model packed by the host packers (an arena it can copy)")
    cache = model.__dict__.setdefault("_replicas", {})
    lora_specs = getattr(model, "_lora_specs", None)
    slots, pending = [], []                         # per requested device: ("own", ) | ("cached", key) ; new replicas to fill
    for d in devices:
        d = torch.device(d)
        if d.type != "cuda":
            raise FoleyRuntimeError("replicas live on HIP devices")
        if d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        if d == model.device and not any(sl[0] == "own" for sl in slots):
            slots.append(("own", None))
            continue
        key = (str(d), sum(1 for sl in slots if sl[1] is not None and sl[1][0] == str(d)) + 0)   # the same device twice = two contexts on it
        slots.append(("cached", key))
        if key not in cache and key not in [p[0] for p in pending]:
            pending.append((key, d))
    if pending and lora_specs is not None:      # new replicas copy the loaded weights, not the merged ones
        from . import lora as _lora
        _lora.ensure(model, None)
    if pending:
        bufs = {}
        for key, d in pending:
            bufs[key] = (torch.empty_like(model.arena.buffer, device=d),
                         torch.empty_like(dac.arena.buffer, device=d) if dac is not None else None)
        # one grouped broadcast to the first new replica of every device that does not hold the model yet
        first = {}
        for key, d in pending:
            if d != model.device and d not in first:
                first[d] = key
        model.last_broadcast_s = 0.0
        model.last_broadcast_path = None           # 'rccl' | 'peer-copy' | None (nothing crossed a device boundary)
        if first:
            per_dev = [[model.arena.buffer.view(torch.uint8).reshape(-1)] + ([dac.arena.buffer.view(torch.uint8).reshape(-1)] if dac is not None else [])]
            for d, key in first.items():
                per_dev.append([bufs[key][0].view(torch.uint8).reshape(-1)] + ([bufs[key][1].view(torch.uint8).reshape(-1)] if dac is not None else []))
            try:
                model.last_broadcast_s = _rt.bcast_local(per_dev)
                model.last_broadcast_path = "rccl"
            except FoleyRuntimeError as e:          # no librccl in the process / ncclCommInitAll refused the device list
                import logging
                import time as _time
                logging.getLogger("foley_amd").warning("grouped RCCL broadcast unavailable (%s): falling back to peer copies", e)
                t0 = _time.perf_counter()
                for dst in per_dev[1:]:
                    for s_buf, d_buf in zip(per_dev[0], dst):
                        d_buf.copy_(s_buf, non_blocking=True)
                for d in first:
                    torch.cuda.synchronize(d)
                model.last_broadcast_s = _time.perf_counter() - t0
                model.last_broadcast_path = "peer-copy"    # so no record attributes this time to RCCL
        for key, d in pending:                      # further contexts on a device: device-local copies of what is there already
            if first.get(d) == key:
                continue
            src = (model.arena.buffer, dac.arena.buffer if dac is not None else None) if d == model.device else bufs[first[d]]
            bufs[key][0].copy_(src[0])
            if dac is not None:
                bufs[key][1].copy_(src[1])
        for key, d in pending:
            arena = packers.Arena(model.arena.buffer.numel(), model.arena.table, d, buffer=bufs[key][0])
            m = FoleyModel.from_arena(model.cfg, arena, model.dtype, d, dac_cfg=model.dac_cfg, quantization=model.quantization)
            m._text_len_fixed = model._text_len_fixed      # the sticky text bucket is per MODEL in the reference (utils.py:166-188)
            dd = None
            if dac is not None:
                dd = FoleyDAC.from_arena(packers.Arena(dac.arena.buffer.numel(), dac.arena.table, d, buffer=bufs[key][1]), d, dac.cfg)
            cache[key] = (m, dd)
    reps = [(model, dac) if kind == "own" else cache[key] for kind, key in slots]
    if lora_specs is not None or any(getattr(m, "_lora_fp", None) is not None for m, _ in reps):
        from . import lora as _lora
        for m in dict.fromkeys([model] + [m for m, _ in reps]):   # a no-op wherever the set is merged already
            _lora.ensure(m, lora_specs)
    return reps


def denoise_process_multi(visual_feats, text_feats, audio_len_in_s, replicas: Sequence, guidance_scale: float,
                          num_inference_steps: int, batch_size: int, sampler: str,
                          generator: Optional[torch.Generator] = None, use_graph: bool = True,
                          progress: Optional[Callable[[int, int], None]] = None, return_latents: bool = False, edit=None,
                          guidance: Optional[GuidanceSpec] = None, step_cache: Optional[StepCacheSpec] = None, timeline=None,
                          multistep: Optional[MultistepSpec] = None):
    """`denoise_process_with_generator` with the clips of the batch sharded over `replicas` (the pairs
    `replicate()` returns), one host thread per GPU.  Clips are independent (reference utils.py:159-199 batches clips that
    share their conditioning; per-clip conditioning, host/cond_sets.py, only changes what each clip reads), so there is no
    collective: the noise of the WHOLE batch is drawn once from `generator` exactly like the single-GPU call does and sliced
    (`distributed.shard_range`), and per-clip conditioning tensors are sliced with their clips (`cond_sets.shard`).  With
    shared conditioning the result is bit-identical to one GPU running the full batch whenever the shards use the same tile
    shapes and the same summation order - and equal to bf16 / fp32 accuracy otherwise.  With per-clip conditioning a shard
    de-duplicates its own clips and may take another layout than the full batch (per cfg half instead of per batch row, when
    the clips of the shard share their conditioning): the results then agree to bf16 / fp32 accuracy.  A shard of ONE clip never is bit-identical to that
    clip inside a larger shard: single-clip forwards rotate the K origin of their small-grid GEMMs per M tile (K-origin
    rotation, gemm.hip g_gemm_krot_ok), a different but deterministic summation order (tests/test_pairs_gpu.py pins how
    far it moves a result).  `edit` as for denoise_process_with_generator: per-clip source latents and masks are sharded with
    the noise.  A windowed run (denoise_process_with_generator's `windows`) is not sharded here: the windows of one variation
    are coupled after every step, so it runs on one device.  `step_cache` is forwarded to every shard: a skip list gives what one GPU
    gives; in threshold mode every shard decides from the rows it holds (the max over them), so the decisions - and with them the
    clips - depend on the sharding.  `timeline` (one for the whole batch) is forwarded with the prompts' text rows, unsliced: every
    shard builds the table rows of its own clips.  `multistep` is forwarded to every shard (each keeps the history of its own clips).  Returns (audio [bs, 1, T] fp32 on the first replica's device, sr)."""
    from .distributed import shard_range
    if multistep is not None:
        multistep.check(sampler)
    if isinstance(edit, _audio_edit.FlowEditSpec):
        raise ValueError("a FlowEdit run is not sharded over replicas: every variation is a (source, target) pair of batch clips that "
                         "must stay on one device; call denoise_process_with_generator")
    if not replicas:
        raise FoleyRuntimeError("no replicas")
    m0 = replicas[0][0]
    cfg = m0.cfg
    La = int(audio_len_in_s * cfg.frame_rate)
    # The sticky text bucket is ONE value per model in the reference (utils.py:166-188): every replica pads this batch to the
    # same length - the largest bucket any replica has seen so far or this prompt asks for - whichever shards it gets.
    t_now = min(77 if text_feats["text_feat"].shape[1] <= 77 else 128, cfg.text_len)
    sticky = max([t_now] + [m._text_len_fixed or 0 for m, _ in replicas])
    for m, _ in replicas:
        m._text_len_fixed = sticky
    noise = draw_noise(batch_size, cfg.latent_dim, La, m0.dtype, generator)
    shards = [shard_range(batch_size, r, len(replicas)) for r in range(len(replicas))]
    results: List = [None] * len(replicas)
    errors: List = []
    # The conditioning tensors may still be in flight on the CALLER's streams (the CLAP / SigLIP2 / Synchformer kernels of
    # the node run on the default stream of their device): every worker runs on a fresh non-blocking stream, which orders
    # nothing against them by itself - one event per producing device, recorded here on the calling thread, and waited for
    # by each worker's stream before it touches a feature.
    ready = []
    for dv in {t.device for t in list(visual_feats.values()) + list(text_feats.values()) if torch.is_tensor(t) and t.is_cuda}:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dv))
        ready.append(ev)

    failed = threading.Event()              # set by the first failing worker; the others do not start (or stop at their next iteration)
    running = [False] * len(replicas)
    fail_lock = threading.Lock()

    def work(r):
        lo, hi = shards[r]
        if hi <= lo:
            return
        model, dac = replicas[r]
        try:
            stream = torch.cuda.Stream(model.device)
            with torch.cuda.device(model.device), torch.cuda.stream(stream):
                for ev in ready:
                    stream.wait_event(ev)
                if failed.is_set():
                    return
                running[r] = True
                results[r] = denoise_process_with_generator(     # per-clip conditioning travels with its clips
                    cond_sets.shard(visual_feats, lo, hi, batch_size),
                    text_feats if timeline is not None else cond_sets.shard(text_feats, lo, hi, batch_size),
                    audio_len_in_s, model, dac, guidance_scale, num_inference_steps, hi - lo,
                    sampler, use_graph=use_graph, noise=noise[lo:hi], return_latents=True,
                    progress=progress if r == 0 else None, _abort_event=failed,
                    edit=edit.shard(lo, hi, batch_size) if edit is not None else None, guidance=guidance,
                    step_cache=step_cache, timeline=timeline, **_ms_kw(multistep))
                torch.cuda.current_stream().synchronize()
        except Exception as e:          # surfaced on the calling thread
            running[r] = False          # FIRST: a second failing (or aborted) worker must not keep the first one waiting on it
            with fail_lock:
                first_failure = not failed.is_set()
                errors.append(e)
                failed.set()            # replicas still in prepare / warm-up see it before their loop starts (foley_sample
            if first_failure:           # clears a stale abort request at entry); the ones inside the loop stop at the next iteration.
                import time as _time    # Only the FIRST failing worker asks, and keeps asking until every other worker has left
                while True:             # (closes the check-then-clear window); workers that fail because of the abort just leave.
                    busy = [i for i in range(len(replicas)) if i != r and running[i]]
                    for i in busy:
                        try:
                            replicas[i][0].ctx.abort()
                        except Exception:   # noqa: BLE001 - best effort; the first error is the one reported
                            pass
                    if not busy:
                        break
                    _time.sleep(0.005)
        finally:
            running[r] = False

    threads = [threading.Thread(target=work, args=(r,), name=f"foley-dp-{r}") for r in range(len(replicas))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    done = [x for x in results if x is not None]
    audio = torch.cat([x[0].to(m0.device) for x in done])
    sr = done[0][1]
    if return_latents:
        return audio, sr, torch.cat([x[2].to(m0.device) for x in done])
    return audio, sr
