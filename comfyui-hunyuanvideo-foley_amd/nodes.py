"""ComfyUI node layer of the MI355X-native Foley path.

Drop-in boundary: the six node keys, display names, socket type strings, widget
names / order / defaults / ranges and return tuples below are those of the reference's
`nodes.py` (node classes at :57-70, :156-168, :211-242, :433-457, :609-631, :636-663; mappings
:668-683), so `example_workflows/HunyuanVideoFoleyExample.json` loads unchanged.  What sits
behind them is new: the loaders pack checkpoints into a device arena for libfoley_hip.so, the
sampler enqueues the whole denoising loop + DAC decode on the GPU.  The `TORCH_COMPILE_CFG` and
`BLOCKSWAPARGS` sockets are accepted and ignored: there is no tracing compiler on this path and
the 288 GB of HBM make block swapping pointless.

ComfyUI modules (`folder_paths`, `comfy.*`) are imported lazily so the package also imports in
test environments without ComfyUI.
"""
from __future__ import annotations

import logging
import os

import torch

from .host import cond_sets as _cond_sets
from .host import config as _cfg
from .host import encoders as _enc
from .host import sampler as _sampler

log = logging.getLogger("HunyuanVideo-Foley[MI355X]")


def log_step_cache(models) -> None:
    """One line per context that ran under the step cache: `skipped k of n` (its plan["step_cache_report"])."""
    for m in models:
        rep = (getattr(m.ctx, "plan", None) or {}).get("step_cache_report")
        if rep is not None:
            log.info("step cache: skipped %d of %d iterations", sum(rep["skipped"]), len(rep["skipped"]))


def _fmt_db(t) -> str:
    return "[" + ", ".join("%.2f" % v for v in t.tolist()) + "]"


_SOLVERS = ["euler", "heun-2", "midpoint-2", "kutta-4"]
_PKG_DIR = os.path.dirname(os.path.abspath(__file__))


# ----------------------------------------------------------------------------- ComfyUI glue
def _folder_paths():
    try:
        import folder_paths  # type: ignore
    except Exception:
        return None
    foley_dir = os.path.join(folder_paths.models_dir, "foley")
    if "foley" not in folder_paths.folder_names_and_paths:      # models/foley/ like the reference
        folder_paths.folder_names_and_paths["foley"] = ([foley_dir], folder_paths.supported_pt_extensions)
    return folder_paths


def _foley_files(substr=None):
    fp = _folder_paths()
    names = fp.get_filename_list("foley") if fp is not None else []
    return [f for f in names if substr is None or substr in f]


def _torch_device():
    try:
        import comfy.model_management as mm  # type: ignore
        return mm.get_torch_device()
    except Exception:
        return torch.device("cuda:0")


def _load_state_dict(path):
    try:
        from comfy.utils import load_torch_file  # type: ignore
    except ImportError:
        load_torch_file = None
    if load_torch_file is not None:
        obj = load_torch_file(path, device=torch.device("cpu"))
    elif str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        obj = load_file(path)
    else:
        # tensors only: never unpickle arbitrary objects from a downloaded .pth (comfy's loader does the same)
        obj = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(obj, dict) and isinstance(obj.get("state_dict"), dict):   # utils.py:49-59
        obj = obj["state_dict"]
    return {k: v for k, v in obj.items() if isinstance(v, torch.Tensor)}


def fp8_wrapped_key(key: str, tensor) -> bool:
    """Does the reference's _wrap_fp8_inplace (utils.py:408-485) store this tensor in fp8?  Its deny
    list never matches, so: the weight of EVERY nn.Linear / nn.Conv1d and nothing else -
    learned feature rows, position tables, norm gains and biases stay full precision
    (tests/golden/g8_fp8.npz lists the 56 wrapped modules of the tiny config)."""
    return key.endswith(".weight") and tensor.dim() >= 2 and tensor.is_floating_point()


def fp8_round_state_dict(state_dict, qmode: str, autocast: bool = True, param_dtype=torch.float32):
    """Weight-only fp8 storage = plain cast, no scales; values are rounded once here and the kernels
    run on the exactly representable bf16/fp32 images.  Order as in the reference loader
    (nodes.py:96-124): checkpoint -> parameters of the requested precision (`param_dtype`; fp8
    checkpoint tensors are upcast exactly) -> cast to the fp8 storage type, so an fp32 checkpoint is
    rounded twice and an fp8 checkpoint of the other flavour is re-rounded.  Under autocast
    (bf16/fp16 compute, the only way the reference runs fp8 models) the first TimestepEmbedder bias
    is rounded too: the wrapper casts it to the activation dtype, which embed_layers.py:134 has made
    fp8 (golden g8, "Q14"); the matching feature rounding lives in host/sampler.py::build_plan."""
    out = {}
    qd = {"fp8_e4m3fn": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}.get(qmode)
    for k, v in state_dict.items():
        if v.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
            v = v.to(torch.float32)
        if qd is not None and v.is_floating_point() and (fp8_wrapped_key(k, v) or (autocast and k == "time_in.mlp.0.bias")):
            v = v.to(torch.float32).to(param_dtype).to(qd).to(torch.float32)
        out[k] = v
    return out


def round_params(state_dict, param_dtype):
    """The reference loads the checkpoint into parameters of the requested precision
    (`foley_model.to(dtype)`, nodes.py:96-106): EVERY floating tensor - biases, norm gains, the sync
    position table, the learned empty-feature rows - is rounded to bf16 / fp16, not only the matrices.
    The packed arena keeps those small tensors in fp32 storage, so the rounding is applied to their
    values here (exact for fp8 / already-rounded checkpoints)."""
    if param_dtype == torch.float32:
        return state_dict
    out = {}
    for k, v in state_dict.items():
        if v.is_floating_point() and v.dtype not in (torch.float8_e4m3fn, torch.float8_e5m2):
            v = v.to(param_dtype).to(torch.float32)
        out[k] = v
    return out


def resolve_quantization(quantization: str, detected):
    """Reference nodes.py:109-122: 'auto' honours fp8 tensors found in the checkpoint, else e4m3fn
    (its e5m2 fallback is for compute capability < 9; gfx950 reports 9.x and implements OCP e4m3fn /
    e5m2 natively) - i.e. the DEFAULT widget value rounds every Linear / Conv weight through fp8,
    exactly like the reference does on a capable device."""
    if quantization == "none":
        return "none"
    if quantization == "auto":
        return detected or "fp8_e4m3fn"
    return quantization


def detect_ckpt_fp8(state_dict):
    """'fp8_e5m2' / 'fp8_e4m3fn' if the checkpoint stores such tensors, else None (utils.py:492-504)."""
    for v in state_dict.values():
        if v.dtype == torch.float8_e5m2:
            return "fp8_e5m2"
        if v.dtype == torch.float8_e4m3fn:
            return "fp8_e4m3fn"
    return None


def detect_ckpt_major_precision(state_dict):
    """Dominant dtype among bf16 / fp16 / fp32 by element count (utils.py:507-515)."""
    counts = {torch.bfloat16: 0, torch.float16: 0, torch.float32: 0}
    for v in state_dict.values():
        if v.dtype in counts:
            counts[v.dtype] += v.numel()
    if not any(counts.values()):
        return torch.bfloat16
    return max(counts, key=counts.get)


class AttributeDict(dict):
    """dict with attribute access - the HUNYUAN_DEPS payload type."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


# ----------------------------------------------------------------------------- NODE 1: model loader
class HunyuanModelLoader:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "model_name": (_foley_files(),),
                "precision": (["auto", "bf16", "fp16", "fp32"], {"default": "bf16", "tooltip": "Compute dtype of the GEMM operands (fp32 = parity mode on fp32 MFMA; auto = detect from checkpoint)"}),
                "quantization": (["none", "fp8_e4m3fn", "fp8_e5m2", "auto"], {"default": "auto", "tooltip": "FP8 weight-only storage of the checkpoint (values are rounded through fp8 like the reference, compute stays bf16 / fp16)"}),
            },
        }

    RETURN_TYPES = ("HUNYUAN_MODEL",)
    FUNCTION = "build_model"
    CATEGORY = "audio/HunyuanFoley"

    @staticmethod
    def pack_state_dict(state_dict, precision="bf16", quantization="auto", device=None, cfg=None, dac_cfg=None):
        """state dict -> FoleyModel.  precision=fp16 (and `auto` on an fp16 checkpoint) computes in fp16 like the
        reference does (parameters .to(float16), torch.autocast(float16): nodes.py:89-106, utils.py:229-234) - the
        v_mfma_f32_32x32x16_f16 instantiation of the same kernels."""
        cfg = cfg or _cfg.load_yaml_config(os.path.join(_PKG_DIR, "configs", "hunyuanvideo-foley-xxl.yaml"))
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}.get(precision)
        detected = detect_ckpt_fp8(state_dict)
        if precision == "auto" or dtype is None:
            major = detect_ckpt_major_precision(state_dict)
            dtype = major       # the checkpoint's dominant dtype: fp32, bf16 or fp16 (utils.py:507-515)
        qmode = resolve_quantization(quantization, detected)
        param_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}.get(precision, dtype)
        sd = round_params(state_dict, param_dtype)
        sd = fp8_round_state_dict(sd, qmode, autocast=dtype != torch.float32, param_dtype=param_dtype)
        return _sampler.FoleyModel(cfg, sd, dtype, device or _torch_device(), dac_cfg=dac_cfg or _cfg.DAC48K,
                                   quantization=qmode)

    def build_model(self, model_name, precision, quantization):
        fp = _folder_paths()
        if fp is None:
            raise RuntimeError("ComfyUI's folder_paths module is required to resolve model files")
        sd = _load_state_dict(fp.get_full_path("foley", model_name))
        model = self.pack_state_dict(sd, precision, quantization)
        log.info("Loaded HunyuanVideoFoley main model: %s", model_name)
        return (model,)


# ----------------------------------------------------------------------------- NODE 2: dependencies loader
class HunyuanDependenciesLoader:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "vae_name": (_foley_files("vae"),),
                "synchformer_name": (_foley_files("synch"),),
            }
        }

    RETURN_TYPES = ("HUNYUAN_DEPS",)
    FUNCTION = "load_dependencies"
    CATEGORY = "audio/HunyuanFoley"

    def load_dependencies(self, vae_name, synchformer_name):
        fp = _folder_paths()
        if fp is None:
            raise RuntimeError("ComfyUI's folder_paths module is required to resolve model files")
        device = _torch_device()
        deps = AttributeDict()
        deps["dac_model"] = _sampler.FoleyDAC(_load_state_dict(fp.get_full_path("foley", vae_name)), device)
        deps["synchformer_path"] = fp.get_full_path("foley", synchformer_name)
        # Conditioning encoders stay on PyTorch-ROCm and are created on first use: the
        # Synchformer visual extractor is this repo's functional restatement over the checkpoint's
        # tensors (host/encoders.py), SigLIP2 and CLAP come from `transformers` like in the reference
        # (nodes.py:198-201).
        deps["syncformer_model"] = None      # state dict of the visual extractor once loaded
        deps["siglip2_model"] = None
        deps["clap_tokenizer"] = None
        deps["clap_model"] = None
        deps["device"] = device
        return (deps,)


SIGLIP2_REPO, CLAP_REPO = "google/siglip2-base-patch16-512", "laion/larger_clap_general"


def _ensure_text_encoder(deps):
    if deps.get("clap_model") is None:
        from transformers import AutoTokenizer, ClapTextModelWithProjection
        deps["clap_tokenizer"] = AutoTokenizer.from_pretrained(CLAP_REPO)
        deps["clap_model"] = ClapTextModelWithProjection.from_pretrained(CLAP_REPO).eval()
    return deps


def _ensure_visual_encoders(deps, device, dtype):
    """SigLIP2 through transformers, Synchformer from the file the Dependencies Loader resolved.  Both
    live on the GPU in the model's dtype like in the reference sampler (nodes.py:283-284)."""
    if deps.get("siglip2_model") is None:
        from transformers import AutoModel
        deps["siglip2_model"] = AutoModel.from_pretrained(SIGLIP2_REPO).eval()
    deps["siglip2_model"].to(device=device, dtype=dtype)
    sync = deps.get("syncformer_model")
    if sync is None:
        path = deps.get("synchformer_path")
        if not path:
            raise RuntimeError("HUNYUAN_DEPS carries no Synchformer checkpoint (synchformer_path)")
        sync = _load_state_dict(path)
    if not isinstance(sync, dict):
        raise RuntimeError("HUNYUAN_DEPS['syncformer_model'] must be the Synchformer state dict")
    first = next(iter(sync.values()))
    if first.device != torch.device(device) or first.dtype != dtype or any(not k.startswith("vfeat_extractor.") for k in sync):
        sync = _enc.load_synchformer_state(sync, device, dtype)
    deps["syncformer_model"] = sync
    return deps


@torch.inference_mode()
def encode_text_feat(prompts, deps, device, dtype=None):
    """CLAP last_hidden_state for [negative, positive] (feature_utils.py:133-138)."""
    _ensure_text_encoder(deps)
    deps["clap_model"].to(device=device, dtype=dtype) if dtype is not None else deps["clap_model"].to(device)
    return _enc.encode_text_feat(deps["clap_tokenizer"], deps["clap_model"], prompts, device)


select_frames = _enc.select_frames


# ----------------------------------------------------------------------------- NODE 3: sampler
class HunyuanFoleySampler:
    SAMPLER_NAMES = _SOLVERS

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "hunyuan_model": ("HUNYUAN_MODEL",),
                "hunyuan_deps": ("HUNYUAN_DEPS",),
                "frame_rate": ("FLOAT", {"default": 16, "min": 1, "max": 120, "step": 0.1, "tooltip": "The framerate of the input image sequence"}),
                "duration": ("FLOAT", {"default": 5.0, "min": 1, "max": 60.0, "step": 0.1, "tooltip": "Duration of the audio to generate in seconds"}),
                "prompt": ("STRING", {"multiline": True, "default": "A person walks on frozen ice"}),
                "negative_prompt": ("STRING", {"multiline": True, "default": "noisy, harsh"}),
                "cfg_scale": ("FLOAT", {"default": 4.5, "min": 1.0, "max": 10.0, "step": 0.1, "tooltip": "Classifier-Free Guidance scale"}),
                "steps": ("INT", {"default": 50, "min": 10, "max": 100, "step": 1, "tooltip": "Number of denoising steps"}),
                "sampler": (cls.SAMPLER_NAMES, {"default": "euler", "tooltip": "Flow-match ODE solver"}),
                "batch_size": ("INT", {"default": 1, "min": 1, "max": 6, "step": 1, "tooltip": "Number of audio variations to generate at once"}),
                "seed": ("INT", {"default": 0, "min": 0, "max": 0xffffffffffffffff}),
                "force_offload": ("BOOLEAN", {"default": True, "tooltip": "Kept for workflow compatibility; weights stay resident in HBM"}),
            },
            "optional": {
                "image": ("IMAGE",),
                "torch_compile_cfg": ("TORCH_COMPILE_CFG", {"tooltip": "Accepted for workflow compatibility and ignored (no tracing compiler on this path)."}),
                "block_swap_args": ("BLOCKSWAPARGS", {"tooltip": "Accepted for workflow compatibility and ignored (288 GB HBM: nothing to swap)."}),
            }
        }

    RETURN_TYPES = ("AUDIO", "AUDIO")
    RETURN_NAMES = ("audio_first", "audio_batch")
    FUNCTION = "generate_audio"
    CATEGORY = "audio/HunyuanFoley"

    def generate_audio(self, hunyuan_model, hunyuan_deps, frame_rate, duration, prompt, negative_prompt, cfg_scale,
                       steps, sampler, batch_size, seed, force_offload, image=None, torch_compile_cfg=None,
                       block_swap_args=None, features=None, *, audio=None, strength=1.0, regenerate=None, crossfade_s=0.1,
                       prompts=None, negative_prompts=None, images=None, window_s=None, window_overlap_s=2.0,
                       video_cfg_scale=None, guidance_interval=None, cfg_rescale=0.0, cache_threshold=None, cache_skip=None,
                       cache_interval=None, cache_max_consecutive=None, prompt_timeline=None, prompt_crossfade_s=0.25,
                       loudness_lufs=None, true_peak_dbtp=-1.0, peak_limiter=False, multistep_order=None,
                       guidance_mode=None, apg_eta=0.0, apg_momentum=-0.5, apg_norm_threshold=0.0, zero_init_steps=0,
                       source_prompt=None, source_cfg_scale=2.0, edit_noise="fresh", loras=None):
        """`features` (not a ComfyUI socket) lets callers inject precomputed conditioning
        {'siglip2_feat','syncformer_feat','text_feat','uncond_text_feat'} - used by tests/bench.  Each may have batch 1 (shared)
        or batch_size (one row per clip).

        Per-clip conditioning (keyword-only, not sockets; host/cond_sets.py): `prompts` / `negative_prompts` - one string per clip
        (CLAP runs on each clip's [negative, prompt] pair, as for that clip alone) - and `images` - one IMAGE frame batch per clip,
        all of one resulting duration.  A list replaces its widget; the clips of the batch then differ in what they are conditioned
        on, not only in their noise.  Different videos take per-row buffers: at most 32 batch rows (16 clips under
        CFG, 10 with video_cfg_scale), and the single blocks' modulation rows grow with the clips (about 15 GB at 30 s x 8 clips under CFG).

        Audio editing (keyword-only, not sockets; host/audio_edit.py): `audio` (an AUDIO dict, batch 1 or batch_size) is
        re-sampled from part-way down the schedule - `strength` in (0, 1] selects how far (1.0: from pure noise) - and
        `regenerate` [(start_s, end_s), ...] limits the change to those spans (crossfade_s linear ramps at their edges; the
        rest of the clip keeps the source).  A duration past the end of `audio` extends it (strength 1.0 only).

        Long clips (keyword-only, not sockets; host/long_form.py): with `window_s` (whole seconds; None: off) and a duration
        beyond it, the clip is generated as overlapping windows of window_s seconds - at least `window_overlap_s` seconds shared
        by neighbours - that run as ONE batch and are blended after every solver step, then decoded as one waveform of the whole
        length.  Every window sees its own slice of the video (text-to-audio: the learned empty rows); one prompt and one negative
        prompt serve all windows.  `duration` may exceed the widget's 60 s here; for video the total follows the frames, cut to
        whole seconds.  batch_size stays the number of variations.  The run takes the single-device path (the windows of a clip
        are coupled), and does not combine with audio= / regenerate= or prompts= / images= / features=.

        Guidance (keyword-only, not sockets; host/sampler.py::GuidanceSpec): `video_cfg_scale` - a guidance scale of its own
        for the video features; the `cfg_scale` widget stays the prompt's scale, and the model then runs three passes per
        iteration (nothing / video / video + prompt) instead of two.  `guidance_interval` (start, end) in fractions of the
        loop - guidance acts on the iterations inside it, the others take the conditional prediction (every pass still runs).
        `cfg_rescale` in [0, 1] pulls the guided prediction's spread back to the conditional one's (0: off).  They combine with
        audio editing and long clips.

        Step cache (keyword-only, not sockets; host/step_cache.py::StepCacheSpec): reuse the blocks' residual on iterations
        whose model input barely moved, instead of running the blocks.  `cache_threshold` - skip while the accumulated relative
        change of the first block's input stays below it (uncalibrated: start near 0.2; one decision serves the whole batch, so a
        clip's result depends on its batch), limited by `cache_interval` (start, end) in fractions of the loop and
        `cache_max_consecutive`; or `cache_skip` - the list of iteration indices to skip.  The first and the last iteration always
        run in full.  It combines with guidance, audio editing, per-clip conditioning and long clips; the log says how many
        iterations were skipped.

        Timed prompts (keyword-only, not sockets; host/prompt_timeline.py): `prompt_timeline` [(start_s, end_s, prompt), ...] -
        every moment of the clip reads the prompt of its own time; time no span covers takes the `prompt` widget, and
        `prompt_crossfade_s` blends neighbouring prompts linearly across each boundary (0: hard cuts).  At most 16 distinct
        text sets, the negative prompt included.  With `window_s` the timeline is given in the long clip's time (text-to-audio;
        per-window video features are not carried).  It combines with audio= / regenerate=, guidance and the step cache, and
        does not combine with prompts= / negative_prompts= / images= / features=.

        Loudness (keyword-only, not sockets; host/loudness.py): `loudness_lufs` (None: off) brings every clip of the batch, each
        on its own, to that integrated loudness (ITU-R BS.1770-4; about -16 for the web, -23 for EBU R128) on the device before
        the waveform leaves it.  `true_peak_dbtp` is the true-peak ceiling: without `peak_limiter` the gain is lowered where the
        peak would pass it; with it the full gain is applied and a 5 ms look-ahead limiter holds the peaks under the ceiling.
        A silent clip is returned as it is.  It combines with every other option.

        Multistep solver (keyword-only, not a socket; host/sampler.py::MultistepSpec): `multistep_order` 2 or 3 (None: off) with
        the `euler` solver - Adams-Bashforth on the run's sigma grid, which reuses the velocities of the one or two steps before
        and so reaches second order at Euler's price of one model call per step.  Order 3 is a third-order formula behind a
        first-order first step: second order overall, with a smaller constant.  It combines with every other option and does not
        combine with heun-2 / midpoint-2 / kutta-4.

        Projected guidance (keyword-only, not sockets; host/sampler.py::ProjectionSpec): `guidance_mode` "apg" (adaptive projected
        guidance: `apg_eta` in [0, 1] scales the part of the guidance difference parallel to the conditional prediction,
        `apg_momentum`, |.| < 1, averages the difference over the iterations, `apg_norm_threshold` >= 0 clips its norm - in the
        model's velocity units, uncalibrated; 0: off) or "cfg_zero_star" (the unconditional prediction is rescaled per clip before
        the combine); `zero_init_steps` iterations at the start use a zero velocity.  Two halves with cfg_scale > 1 only: it does
        not combine with video_cfg_scale or cfg_rescale > 0.  None: the plain combine, bit for bit, and nothing new is launched.

        FlowEdit (keyword-only, not sockets; host/audio_edit.py::FlowEditSpec): `source_prompt` describes what `audio` sounds like
        and the `prompt` widget what it should sound like instead; the clip keeps its timing, which both prompts share through the
        video.  `cfg_scale` is the target prompt's guidance scale, `source_cfg_scale` the source prompt's (2.0: uncalibrated for
        this model); `strength` is how far up the schedule the edit starts, `regenerate` / `crossfade_s` restrict it in time, and
        `edit_noise` "fresh" noises the source anew every step, "fixed" with one draw.  Every variation runs as two clips of the
        model batch, so the run costs what a CFG batch of 2 x batch_size clips costs, on one device.  euler only, both scales > 1; it
        does not combine with window_s, prompts= / negative_prompts= / images= / features=, prompt_timeline, the guidance controls,
        multistep_order or the step cache, and a duration past the end of `audio` is refused.  The loudness stage combines with it.
        None: every run is what it was, bit for bit, and nothing new is launched.

        LoRA adapters (keyword-only, not a socket; host/lora.py): `loras` [(file name or state dict, strength), ...] - the
        adapters are merged into the model's packed weights, in list order, before anything else runs (a refused file costs no
        encoder pass), and stay merged until a call asks for another set.  A bare file name is looked up in ComfyUI's `loras`
        folder, then in `foley`.  PEFT / diffusers, ComfyUI-native and kohya spellings are served; DoRA, LoHa, LoKr and weight
        diffs are refused by name.  Strength 0 drops an adapter, negative strengths are allowed.  The merge is in place, so the
        loop runs at its plain speed and fp8 weights stay fp8; it combines with every other option.  None on a model with nothing
        merged: nothing is imported or launched and the run is the plain one, bit for bit; None on a model that carries a set
        restores the loaded weights first (logged)."""
        model, deps = hunyuan_model, hunyuan_deps
        if loras is not None or getattr(model, "_lora_fp", None) is not None:      # first: refused before the encoders run
            from .host import lora as _lora
            want = [(self._lora_path(src), strength) for src, strength in _lora.normalize(loras)]
            if _lora.ensure(model, want):
                log.info("LoRA: %s", "merged %d adapter(s) into the packed weights" % len(want) if want else
                         "restored the loaded weights (no loras= on a model that carried a set)")
        flowedit = None
        if source_prompt is not None:              # refused here, before the encoders run
            flowedit = self._check_flowedit(audio, duration, sampler, cfg_scale, source_cfg_scale, edit_noise, deps, dict(
                window_s=window_s, prompts=prompts, negative_prompts=negative_prompts, images=images, features=features,
                prompt_timeline=prompt_timeline, video_cfg_scale=video_cfg_scale, guidance_interval=guidance_interval,
                cfg_rescale=cfg_rescale or None, guidance_mode=guidance_mode, multistep_order=multistep_order,
                cache_threshold=cache_threshold, cache_skip=cache_skip, cache_interval=cache_interval,
                cache_max_consecutive=cache_max_consecutive))
        elif source_cfg_scale != 2.0 or edit_noise != "fresh":
            raise ValueError("source_cfg_scale / edit_noise belong to FlowEdit: pass source_prompt")
        text_prompts = None if flowedit is None else [source_prompt, prompt]     # CLAP then encodes [negative, source, target] in one call
        ms_kw = {}
        if multistep_order is not None:            # refused here, before the encoders run
            _sampler.MultistepSpec(multistep_order).check(sampler)
            ms_kw = {"multistep": _sampler.MultistepSpec(int(multistep_order))}   # unset: the calls as they were
        if loudness_lufs is not None:              # refused here, before the encoders run
            from .host import loudness as _loud
            _loud.check_args(loudness_lufs, true_peak_dbtp, peak_limiter)
            dac_sr = getattr(deps.get("dac_model"), "sample_rate", _loud.SAMPLE_RATE)
            if dac_sr != _loud.SAMPLE_RATE:
                raise ValueError(f"loudness_lufs needs a {_loud.SAMPLE_RATE} Hz decoder, this one gives {dac_sr} Hz")
        timeline = None
        if prompt_timeline is not None:            # refused here, before the encoders run
            if prompts is not None or negative_prompts is not None or images is not None or features is not None:
                raise ValueError("prompt_timeline does not combine with prompts= / negative_prompts= / images= / features=: one "
                                 "timeline serves the whole batch")
            if window_s is not None and duration > window_s and image is not None:
                raise ValueError("prompt_timeline with window_s takes text-to-audio: per-window video features are not carried")
            from .host import prompt_timeline as _ptl
            timeline = _ptl.parse(prompt_timeline, prompt, duration, prompt_crossfade_s)
        step_cache = None
        if cache_threshold is not None or cache_skip is not None:
            if cache_threshold is not None and cache_skip is not None:
                raise ValueError("cache_threshold and cache_skip together: choose threshold mode or a skip list")
            step_cache = _sampler.StepCacheSpec(
                threshold=None if cache_threshold is None else float(cache_threshold),
                skip=None if cache_skip is None else tuple(int(i) for i in cache_skip), interval=cache_interval,
                max_consecutive=cache_max_consecutive)
            step_cache.check(int(steps))       # refused here, before the encoders run
        elif cache_interval is not None or cache_max_consecutive is not None:
            raise ValueError("cache_interval / cache_max_consecutive limit threshold mode: pass cache_threshold")
        guidance = None
        projection = None
        if guidance_mode is not None:              # refused here, before the encoders run
            projection = _sampler.ProjectionSpec(guidance_mode, apg_eta, apg_momentum, apg_norm_threshold, zero_init_steps)
        elif apg_eta != 0.0 or apg_momentum != -0.5 or apg_norm_threshold != 0.0 or zero_init_steps != 0:
            raise ValueError("apg_eta / apg_momentum / apg_norm_threshold / zero_init_steps belong to projected guidance: pass guidance_mode")
        if projection is not None:
            guidance = _sampler.GuidanceSpec(None if video_cfg_scale is None else float(video_cfg_scale),
                                             None if guidance_interval is None else tuple(float(t) for t in guidance_interval),
                                             float(cfg_rescale), projection)
            guidance.check(cfg_scale, int(steps))
        elif video_cfg_scale is not None or guidance_interval is not None or cfg_rescale:
            if video_cfg_scale is not None and image is None and images is None and features is None:
                raise ValueError("video_cfg_scale needs visual input (image / images): without it the two lower guidance "
                                 "halves are identical")
            guidance = _sampler.GuidanceSpec(None if video_cfg_scale is None else float(video_cfg_scale),
                                             None if guidance_interval is None else tuple(float(t) for t in guidance_interval),
                                             float(cfg_rescale))
            guidance.check(cfg_scale)          # refused here, before the encoders run
        device = model.device
        rng = torch.Generator(device="cpu").manual_seed(seed)          # nodes.py:273
        audio_len_in_s = duration
        for name, lst in (("prompts", prompts), ("negative_prompts", negative_prompts), ("images", images)):
            if lst is not None and len(lst) != batch_size:
                raise ValueError(f"{name} has {len(lst)} entries: one per clip, batch_size = {batch_size}")
        if features is not None and (prompts is not None or negative_prompts is not None or images is not None):
            raise ValueError("features= already holds the conditioning: pass prompts / negative_prompts / images without it")
        windows = None
        if window_s is not None:
            if audio is not None or regenerate is not None or strength != 1.0:
                raise ValueError("window_s does not combine with audio= / strength / regenerate=: editing a long clip is not supported")
            if features is not None or prompts is not None or negative_prompts is not None or images is not None:
                raise ValueError("window_s does not combine with prompts= / negative_prompts= / images= / features=: one prompt "
                                 "and one video serve all windows")
            if float(window_s) != int(window_s) or int(window_s) < 1:
                raise ValueError(f"window_s must be a whole number of seconds >= 1, got {window_s}")
        if window_s is not None and duration > window_s:
            visual, text, windows = self._window_features(image, duration, frame_rate, prompt, negative_prompt, model, deps,
                                                          device, int(window_s), window_overlap_s, batch_size,
                                                          **({"prompt_list": list(timeline.prompts)} if timeline is not None else {}))
            audio_len_in_s = windows.Ltot / model.cfg.frame_rate
            if windows.n_win == 1:              # the frames gave no more than one window: an ordinary run of that length
                windows = None
        elif features is not None:
            visual = {k: features[k] for k in ("siglip2_feat", "syncformer_feat")}
            text = {k: features[k] for k in ("text_feat", "uncond_text_feat")}
            audio_len_in_s = features.get("audio_len_in_s", duration)
        elif prompts is not None or negative_prompts is not None or images is not None:
            visual, text, audio_len_in_s = self._per_clip_features(
                images if images is not None else ([image] if image is not None else None), duration, frame_rate, prompts or [prompt] * batch_size, negative_prompts or [negative_prompt] * batch_size,
                model, deps, device)
        elif image is not None:
            visual, text, audio_len_in_s = self._video_features(image, duration, frame_rate, prompt,
                                                                negative_prompt, deps, device, model.dtype,
                                                                **({"prompt_list": list(timeline.prompts)} if timeline is not None else
                                                                   {"prompt_list": text_prompts} if text_prompts is not None else {}))
        else:
            # text-to-audio: learned "empty" visual rows (nodes.py:326-333)
            clip_len = int(duration * 8)
            sync_len = int(((int(duration * 25) - 16) // 8 + 1) * 8)
            visual = {"siglip2_feat": model.get_empty_clip_sequence(bs=1, len=clip_len),
                      "syncformer_feat": model.get_empty_sync_sequence(bs=1, len=sync_len)}
            # a timeline: all its distinct prompts in ONE call, one row each behind the negative prompt's
            res = encode_text_feat([negative_prompt] + (list(timeline.prompts) if timeline is not None else text_prompts or [prompt]),
                                   deps, device, model.dtype)
            text = {"text_feat": res[1:], "uncond_text_feat": res[:1]}
        if flowedit is not None:                # rows [source, target] of the one CLAP call
            text = {"source_text_feat": text["text_feat"][:1], "text_feat": text["text_feat"][1:2], "uncond_text_feat": text["uncond_text_feat"]}
        edit = None
        if audio is not None:
            from .host import audio_edit as _edit
            edit = _edit.prepare_edit(audio, model, deps["dac_model"], audio_len_in_s, steps, sampler, batch_size,
                                      strength=strength, regenerate=regenerate, crossfade_s=crossfade_s,
                                      **({"flowedit": flowedit} if flowedit is not None else {}))
        elif strength != 1.0 or regenerate is not None:
            raise ValueError("strength / regenerate edit an input clip: pass it as audio=")
        pbar = None
        try:
            import comfy.utils  # type: ignore
            pbar = comfy.utils.ProgressBar(steps)
        except Exception:
            pass
        progress = (lambda i, n: pbar.update_absolute(i, n)) if pbar is not None else None
        n_dev = torch.cuda.device_count() if os.environ.get("FOLEY_DATA_PARALLEL", "0") == "1" else 1
        tl_kw = {"timeline": timeline} if timeline is not None else {}      # no timeline: the calls as they were
        ran_on = [model]                        # the models whose contexts ran a shard (the step cache's log line)
        if windows is not None:                 # coupled windows: one device
            audio, sr = _sampler.denoise_process_with_generator(
                visual, text, audio_len_in_s, model, deps["dac_model"], guidance_scale=cfg_scale,
                num_inference_steps=steps, batch_size=batch_size, sampler=sampler, generator=rng, progress=progress,
                windows=windows, guidance=guidance, step_cache=step_cache, **tl_kw, **ms_kw)
        elif batch_size > 1 and n_dev > 1 and model.arena is not None and flowedit is None:   # a FlowEdit pair is not split
            # clips are independent: shard them over the node's GPUs (host/sampler.py::denoise_process_multi; the widget
            # list is the reference's, so the switch is an environment variable - INTEGRATION.md)
            devs = [model.device] + [torch.device("cuda", i) for i in range(n_dev) if i != model.device.index]
            reps = _sampler.replicate(model, deps["dac_model"], devs[:batch_size])
            ran_on = [m for m, _ in reps]
            audio, sr = _sampler.denoise_process_multi(visual, text, audio_len_in_s, reps, cfg_scale, steps, batch_size,
                                                       sampler, generator=rng, progress=progress, edit=edit, guidance=guidance,
                                                       step_cache=step_cache, **tl_kw, **ms_kw)
        else:
            audio, sr = _sampler.denoise_process_with_generator(
                visual, text, audio_len_in_s, model, deps["dac_model"], guidance_scale=cfg_scale,
                num_inference_steps=steps, batch_size=batch_size, sampler=sampler, generator=rng, progress=progress,
                edit=edit, guidance=guidance, step_cache=step_cache, **tl_kw, **ms_kw)
        if step_cache is not None:
            log_step_cache(ran_on)
        if loudness_lufs is not None:           # on the device, each clip on its own
            out, before, after = _loud.normalize({"waveform": audio, "sample_rate": sr}, float(loudness_lufs), float(true_peak_dbtp),
                                                 bool(peak_limiter))
            audio = out["waveform"]
            log.info("loudness: %s LUFS before, gain %s dB, true peak %s dBTP after", _fmt_db(before.lufs), _fmt_db(before.gain_db),
                     _fmt_db(after.true_peak_dbtp))
        waveform_batch = audio.float().cpu()
        first = {"waveform": waveform_batch[0].unsqueeze(0), "sample_rate": sr}
        return (first, {"waveform": waveform_batch, "sample_rate": sr})

    @staticmethod
    def _lora_path(src):
        """A state dict or an existing path as it is; a bare file name through ComfyUI's `loras` folder, then `foley`."""
        if not isinstance(src, (str, os.PathLike)) or os.path.exists(src):
            return src
        fp = _folder_paths()
        for folder in ("loras", "foley"):
            full = fp.get_full_path(folder, os.fspath(src)) if fp is not None and folder in fp.folder_names_and_paths else None
            if full:
                return full
        raise FileNotFoundError(f"LoRA file '{src}' not found (looked in the loras and foley model folders)")

    @staticmethod
    def _check_flowedit(audio, duration, sampler, cfg_scale, source_cfg_scale, edit_noise, deps, others):
        """Every refusal of a FlowEdit call that needs no encoder, with its reason; returns prepare_edit's `flowedit` argument."""
        from .host import audio_edit as _edit
        if audio is None:
            raise ValueError("source_prompt edits an input clip: pass it as audio=")
        _edit.FlowEditSpec(None, source_scale=source_cfg_scale, noise=edit_noise).check(sampler, cfg_scale)
        reasons = {
            "window_s": "editing a long clip is not supported",
            "prompts": "one source and one target prompt serve the batch", "negative_prompts": "one negative prompt serves both branches",
            "images": "the variations share one video", "features": "the node encodes [negative, source, target] itself",
            "prompt_timeline": "the prompts of the two branches are constant in time",
            "video_cfg_scale": "each branch takes two halves with its own constant scale",
            "guidance_interval": "each branch takes two halves with its own constant scale",
            "cfg_rescale": "each branch takes two halves with its own constant scale",
            "guidance_mode": "projected guidance is not built for the velocity difference",
            "multistep_order": "the step keeps no velocity history",
            "cache_threshold": "the step cache is not built for the pair batch", "cache_skip": "the step cache is not built for the pair batch",
            "cache_interval": "the step cache is not built for the pair batch",
            "cache_max_consecutive": "the step cache is not built for the pair batch"}
        for name, why in reasons.items():
            if others.get(name) is not None:
                raise ValueError(f"source_prompt (FlowEdit) does not combine with {name}: {why}")
        wave, sr = audio["waveform"], int(audio["sample_rate"])
        dac = deps.get("dac_model")
        rate, hop = int(getattr(dac, "sample_rate", 48000)), int(getattr(getattr(dac, "cfg", None), "hop", 960))
        _edit.check_flowedit_length(int(duration * rate / hop), rate // hop, wave.shape[-1] * rate // sr, hop, rate)
        return {"source_scale": float(source_cfg_scale), "noise": edit_noise}

    @staticmethod
    @torch.inference_mode()
    def _video_features(image, duration, frame_rate, prompt, negative_prompt, deps, device, dtype=torch.float32, prompt_list=None):
        """Video-to-Audio conditioning (nodes.py:290-320 + utils.py:262-292): resample the IMAGE batch to
        8 fps / 25 fps, run SigLIP2 and the Synchformer visual extractor, CLAP for the two prompts.  The
        audio length follows the sync stream: len(frames_25fps) / 25."""
        _ensure_visual_encoders(deps, device, dtype)
        f8, f25 = _enc.select_frames(image, duration, frame_rate, device=device if torch.device(device).type == "cuda" else None)
        visual, audio_len_in_s = _enc.video_features(f8, f25, deps["siglip2_model"], deps["syncformer_model"], device,
                                                     model_dtype=dtype)
        res = encode_text_feat([negative_prompt] + (prompt_list or [prompt]), deps, device, dtype)   # prompt_list: a timeline's prompts
        return visual, {"text_feat": res[1:], "uncond_text_feat": res[:1]}, audio_len_in_s

    @staticmethod
    @torch.inference_mode()
    def _window_features(image, duration, frame_rate, prompt, negative_prompt, model, deps, device, window_s, overlap_s, variations,
                         prompt_list=None):
        """Conditioning of a long clip's windows (host/long_form.plan_windows): the frames are selected ONCE for the whole clip
        and the 8 fps / 25 fps streams sliced per window at start_s*8 / start_s*25 (the starts fall on whole seconds), then
        SigLIP2 / Synchformer run per window as _per_clip_features runs them per clip - n_win rows; text-to-audio takes the
        learned empty rows at the window's lengths - one shared row.  CLAP runs once: one [negative, prompt] pair for all."""
        from .host import long_form as _long
        if image is not None:
            _ensure_visual_encoders(deps, device, model.dtype)
            f8, f25 = _enc.select_frames(image, duration, frame_rate, device=device if torch.device(device).type == "cuda" else None)
            plan = _long.plan_windows(len(f25) / _enc.FPS_SYNC, window_s, overlap_s, model.cfg.frame_rate, variations)
            W = plan.La // model.cfg.frame_rate
            parts = []
            for st in plan.starts:
                s0 = st // model.cfg.frame_rate
                v, _len = _enc.video_features(f8[s0 * _enc.FPS_SIGLIP:(s0 + W) * _enc.FPS_SIGLIP],
                                              f25[s0 * _enc.FPS_SYNC:(s0 + W) * _enc.FPS_SYNC],
                                              deps["siglip2_model"], deps["syncformer_model"], device, model_dtype=model.dtype)
                parts.append(v)
            visual = _cond_sets.stack_features(parts, ("siglip2_feat", "syncformer_feat"))
        else:
            plan = _long.plan_windows(duration, window_s, overlap_s, model.cfg.frame_rate, variations)
            W = plan.La // model.cfg.frame_rate
            clip_len = int(W * 8)
            sync_len = int(((int(W * 25) - 16) // 8 + 1) * 8)
            visual = {"siglip2_feat": model.get_empty_clip_sequence(bs=1, len=clip_len),
                      "syncformer_feat": model.get_empty_sync_sequence(bs=1, len=sync_len)}
        res = encode_text_feat([negative_prompt] + (prompt_list or [prompt]), deps, device, model.dtype)   # prompt_list: a timeline's prompts
        return visual, {"text_feat": res[1:], "uncond_text_feat": res[:1]}, plan

    @staticmethod
    @torch.inference_mode()
    def _per_clip_features(images, duration, frame_rate, prompts, negative_prompts, model, deps, device):
        """Per-clip conditioning: CLAP per clip over its [negative, prompt] pair (what the single-clip branches encode, so a clip
        is conditioned on what a run of that clip alone gives); SigLIP2 / Synchformer per clip of `images` (each as
        _video_features), or the learned empty rows for text-to-audio.  Clips whose durations differ are refused."""
        if images is not None:
            _ensure_visual_encoders(deps, device, model.dtype)
            parts, lens = [], []
            for img in images:
                f8, f25 = _enc.select_frames(img, duration, frame_rate,
                                             device=device if torch.device(device).type == "cuda" else None)
                v, a_len = _enc.video_features(f8, f25, deps["siglip2_model"], deps["syncformer_model"], device,
                                               model_dtype=model.dtype)
                parts.append(v)
                lens.append(a_len)
            if len(set(lens)) != 1:
                raise ValueError(f"the clips of one batch share one duration: images give audio_len_in_s {lens}")
            visual, audio_len_in_s = _cond_sets.stack_features(parts, ("siglip2_feat", "syncformer_feat")), lens[0]
        else:
            clip_len = int(duration * 8)
            sync_len = int(((int(duration * 25) - 16) // 8 + 1) * 8)
            visual = {"siglip2_feat": model.get_empty_clip_sequence(bs=1, len=clip_len),
                      "syncformer_feat": model.get_empty_sync_sequence(bs=1, len=sync_len)}
            audio_len_in_s = duration
        # CLAP pads a call's prompts to its longest one and those pad rows reach the DiT unmasked: one call per distinct pair keeps
        # each clip's rows what its own [negative, prompt] call gives.  The pairs are then stacked with ZERO rows up to the longest
        # pair - the rows pad_or_trim_text adds on the way to the run's text length anyway.
        pairs = list(zip(negative_prompts, prompts))
        enc = {p: encode_text_feat(list(p), deps, device, model.dtype) for p in dict.fromkeys(pairs)}
        T = max(e.shape[1] for e in enc.values())
        res = [torch.nn.functional.pad(enc[p], (0, 0, 0, T - enc[p].shape[1])) for p in pairs]
        return visual, {"text_feat": torch.cat([r[1:] for r in res]), "uncond_text_feat": torch.cat([r[:1] for r in res])}, \
            audio_len_in_s


# ----------------------------------------------------------------------------- compat nodes
class HunyuanFoleyTorchCompile:
    """Kept so existing workflows load; the resulting config is ignored by the sampler."""

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "backend": (["inductor"], {"default": "inductor"}),
                "fullgraph": ("BOOLEAN", {"default": False}),
                "mode": (["default", "reduce-overhead", "max-autotune"], {"default": "default"}),
                "dynamic": (["true", "false", "None"], {"default": "false"}),
                "dynamo_cache_limit": ("INT", {"default": 64, "min": 64, "max": 8192, "step": 64}),
            }
        }

    RETURN_TYPES = ("TORCH_COMPILE_CFG",)
    FUNCTION = "make_config"
    CATEGORY = "audio/HunyuanFoley"

    def make_config(self, backend, mode, dynamic, fullgraph, dynamo_cache_limit):
        dyn = {"true": True, "false": False, "None": None}.get(str(dynamic), False)
        return ({"backend": backend, "mode": mode, "dynamic": dyn, "fullgraph": fullgraph,
                 "dynamo_cache_limit": int(dynamo_cache_limit)},)


class HunyuanBlockSwap:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "blocks_to_swap": ("INT", {"default": 30, "min": 0, "max": 57, "step": 1}),
            },
            "optional": {
                "use_non_blocking": ("BOOLEAN", {"default": False}),
                "prefetch_blocks": ("INT", {"default": 1, "min": 0, "max": 10, "step": 1}),
                "block_swap_debug": ("BOOLEAN", {"default": False}),
            },
        }

    RETURN_TYPES = ("BLOCKSWAPARGS",)
    RETURN_NAMES = ("block_swap_args",)
    FUNCTION = "set_args"
    CATEGORY = "audio/HunyuanFoley"
    DESCRIPTION = "Accepted for compatibility; the MI355X path keeps all 57 blocks resident in HBM."

    def set_args(self, **kwargs):
        return (kwargs,)


class SelectAudioFromBatch:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "audio_batch": ("AUDIO", {"tooltip": "An audio object containing a batch of waveforms."}),
                "index": ("INT", {"default": 0, "min": 0, "max": 63, "tooltip": "The 0-based index of the audio to select from the batch."}),
            }
        }

    RETURN_TYPES = ("AUDIO",)
    FUNCTION = "select_audio"
    CATEGORY = "audio/utils"

    def select_audio(self, audio_batch, index):
        wave, sr = audio_batch["waveform"], audio_batch["sample_rate"]
        if index >= wave.shape[0]:
            log.warning("Index %d is out of bounds for audio batch of size %d. Clamping to last item.", index,
                        wave.shape[0])
            index = wave.shape[0] - 1
        return ({"waveform": wave[index].unsqueeze(0), "sample_rate": sr},)


NODE_CLASS_MAPPINGS = {
    "HunyuanModelLoader": HunyuanModelLoader,
    "HunyuanDependenciesLoader": HunyuanDependenciesLoader,
    "HunyuanFoleySampler": HunyuanFoleySampler,
    "HunyuanFoleyTorchCompile": HunyuanFoleyTorchCompile,
    "HunyuanBlockSwap": HunyuanBlockSwap,
    "SelectAudioFromBatch": SelectAudioFromBatch,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "HunyuanModelLoader": "Hunyuan-Foley Model Loader",
    "HunyuanDependenciesLoader": "Hunyuan-Foley Dependencies Loader",
    "HunyuanFoleySampler": "Hunyuan-Foley Sampler",
    "HunyuanFoleyTorchCompile": "Hunyuan-Foley Torch Compile",
    "HunyuanBlockSwap": "Hunyuan-Foley BlockSwap Settings",
    "SelectAudioFromBatch": "Select Audio From Batch",
}
