"""Audio-to-audio sampling and time-span regeneration (inpainting / extension) on the HIP engine.

The flow-match path is x(sigma) = sigma*noise + (1 - sigma)*x0 with sigma running from 1 to 0 (tables.sigma_grid).  An edit run
  * encodes the user's clip to source latents x0 = the DAC posterior MEAN (foley_dac_encode, rows [:latent_dim]) after a mono
    downmix, a resample to 48 kHz (foley_op_resample_sinc) and a trim / zero-pad to La * hop samples - no loudness
    normalisation, as the reference decodes DiT latents with no scaling factor;
  * runs the suffix [i0, steps) of the plain run's iterations that `strength` selects (tables.edit_start), starting from
    sigma_{k0}*noise + (1 - sigma_{k0})*x0 (foley_op_flow_mix);
  * after every iteration that ends a solver step, pulls the frames the mask keeps (m = 0) back onto the source's
    forward-noised path: x <- m*x + (1 - m)*(sigma_{k+1}*noise + (1 - sigma_{k+1})*x0) (foley_set_edit, rowops.hip).
With a multistep order (sampler.MultistepSpec) the suffix has no velocity history at i0: its Adams-Bashforth rows warm up from
there (tables.edit_solver_table(..., multistep_order=)), and the ring keeps the velocities, not the blended samples.
Under euler the last sigma is 0, so kept frames end at exactly x0; the multi-stage solvers end where the plain run ends
(sigma > 0 for them: every loop iteration is one solver stage, the reference's quirk that SolverState reproduces).

FlowEdit (FlowEditSpec; Kulikov et al. 2024, inversion-free text-based editing) changes WHAT the clip sounds like and keeps its
timing: every variation is a (source-prompt, target-prompt) pair of batch clips, and the loop integrates the difference of the two
guided velocities from z = x0 over the same suffix [i0, steps) of the euler run (foley_set_flowedit, rowops.hip).  What both
prompts agree on - the timing, which comes from the video and sync features - cancels.  Each iteration noises the source afresh
(noise="fresh": one row of flowedit_noise per iteration) or with one fixed draw (noise="fixed").  Frames the mask keeps (m = 0)
stay at x0 bit for bit.  Not built: the paper's n_min tail of plain target sampling, n_avg > 1, and frames past the end of the
source audio (refused: they have no source).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import runtime as rt
from . import tables
from .runtime import FoleyRuntimeError
from .sync_score import sinc_resample_taps

edit_start = tables.edit_start          # strength -> (k0, i0)


@dataclass
class EditSpec:
    """What `sampler.denoise_process_with_generator(..., edit=)` needs: source latents x0 [1 | clips, C, La] fp32 (1: shared by
    every clip), strength in (0, 1] and the regeneration mask [La] or [1 | clips, La] in [0, 1] (None: all ones)."""
    x0: torch.Tensor
    strength: float = 1.0
    mask: Optional[torch.Tensor] = None

    def device_operands(self, device, clips: int, La: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        x0 = self.x0.to(device=device, dtype=torch.float32).contiguous()
        if x0.dim() != 3 or x0.shape[0] not in (1, clips) or x0.shape[2] != La:
            raise FoleyRuntimeError(f"edit: x0 {tuple(x0.shape)} must be [1 or {clips}, C, {La}]")
        mask = self.mask
        if mask is not None:
            mask = mask.to(device=device, dtype=torch.float32).contiguous()
            if mask.shape[-1] != La or mask.dim() > 2 or (mask.dim() == 2 and mask.shape[0] not in (1, clips)):
                raise FoleyRuntimeError(f"edit: mask {tuple(mask.shape)} must be [{La}] or [1 or {clips}, {La}]")
        return x0, mask

    def shard(self, lo: int, hi: int, clips: int) -> "EditSpec":
        """The edit of clips [lo, hi) of a `clips`-clip batch (data-parallel sharding, distributed.shard_range)."""
        x0 = self.x0[lo:hi] if self.x0.shape[0] == clips and clips > 1 else self.x0
        mask = self.mask
        if mask is not None and mask.dim() == 2 and mask.shape[0] == clips and clips > 1:
            mask = mask[lo:hi]
        return EditSpec(x0, self.strength, mask)


FLOWEDIT_NOISE = ("fresh", "fixed")


@dataclass
class FlowEditSpec:
    """What `sampler.denoise_process_with_generator(..., edit=)` needs for a FlowEdit run: source latents x0 [1 | V, C, La] fp32
    (1: shared by every variation), strength in (0, 1] (how far up the schedule the edit starts), the edit mask [La] or
    [1 | V, La] in [0, 1] (1 = edit, 0 = keep; None: all ones), the CFG scale of the source branch (the run's guidance_scale is the
    target branch's) and the noise policy: "fresh" draws a row per iteration, "fixed" one row for the run."""
    x0: torch.Tensor
    strength: float = 1.0
    mask: Optional[torch.Tensor] = None
    source_scale: float = 2.0
    noise: str = "fresh"

    def check(self, sampler: str, guidance_scale: float) -> None:
        if sampler != "euler":
            raise ValueError(f"FlowEdit needs the euler solver (its step integrates one velocity difference per sigma step), got {sampler!r}")
        if self.noise not in FLOWEDIT_NOISE:
            raise ValueError(f"edit_noise must be one of {list(FLOWEDIT_NOISE)}, got {self.noise!r}")
        for name, v in (("cfg_scale", guidance_scale), ("source_cfg_scale", self.source_scale)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 1.0:
                raise ValueError(f"FlowEdit runs both branches under classifier-free guidance: {name} must be finite and > 1, got {v!r}")

    def n_rows(self, n_iter: int) -> int:
        return int(n_iter) if self.noise == "fresh" else 1

    device_operands = EditSpec.device_operands


def flowedit_noise(generator: Optional[torch.Generator], n_rows: int, V: int, C: int, La: int, dtype: torch.dtype) -> torch.Tensor:
    """The noise table of a FlowEdit run [n_rows, V, C, La]: ONE torch.randn draw from the run's CPU generator in the model's dtype
    (the rule of sampler.draw_noise), in pinned memory where the host can pin."""
    pin = torch.cuda.is_available()
    return torch.randn((int(n_rows), int(V), int(C), int(La)), generator=generator, device="cpu", dtype=dtype, pin_memory=pin)


# ----------------------------------------------------------------------------- mask
def build_mask(La: int, regenerate: Optional[Sequence[Tuple[float, float]]] = None, crossfade_s: float = 0.1,
               src_frames: Optional[int] = None, frame_rate: int = 50) -> torch.Tensor:
    """Regeneration mask [La] fp32 (1 = regenerate) at `frame_rate` latent frames per second.

    Frame l stands for the time (l + 0.5) / frame_rate.  A span (start_s, end_s) is 1 over [start_s, end_s], with a linear ramp
    of crossfade_s seconds on each side OUTSIDE the span (so the span itself is regenerated in full); spans are clamped to the
    clip and overlapping spans take the larger value.  No `regenerate`: all ones (audio-to-audio variation).  Frames at or past
    `src_frames` (the end of the source audio) are always 1 (extension)."""
    if crossfade_s < 0:
        raise ValueError(f"crossfade_s must be >= 0, got {crossfade_s}")
    dur = La / float(frame_rate)
    if regenerate is None:
        m = torch.ones(La, dtype=torch.float64)
    else:
        t = (torch.arange(La, dtype=torch.float64) + 0.5) / frame_rate
        m = torch.zeros(La, dtype=torch.float64)
        for span in regenerate:
            s, e = float(span[0]), float(span[1])
            if not e > s:
                raise ValueError(f"regenerate span ({s}, {e}) is empty: the end must lie after the start")
            if e <= 0.0 or s >= dur:
                raise ValueError(f"regenerate span ({s}, {e}) lies outside the {dur:g} s clip")
            s, e = max(s, 0.0), min(e, dur)
            inside = ((t >= s) & (t <= e)).double()
            if crossfade_s > 0:
                ramp = torch.minimum((t - (s - crossfade_s)) / crossfade_s, ((e + crossfade_s) - t) / crossfade_s)
                inside = torch.maximum(inside, ramp.clamp(0.0, 1.0))
            m = torch.maximum(m, inside)
    if src_frames is not None and src_frames < La:
        m[max(int(src_frames), 0):] = 1.0
    return m.to(torch.float32)


# ----------------------------------------------------------------------------- source latents
def _taps(model, sr: int, target: int):
    cache = model.__dict__.setdefault("_edit_resample_taps", {})
    key = (sr, target, str(model.device))
    if key not in cache:
        taps, o, n, width = sinc_resample_taps(sr, target)
        cache[key] = (taps.to(model.device), o, n, width)
    return cache[key]


def prepare_waveform(audio: dict, model, dac) -> torch.Tensor:
    """ComfyUI AUDIO {'waveform': [B, ch, N] (or [ch, N]), 'sample_rate'} -> mono [B, N48] fp32 on the model's device at the
    codec's rate (mean over channels, then foley_op_resample_sinc with torchaudio's default kernel)."""
    wave, sr = audio["waveform"], int(audio["sample_rate"])
    if wave.dim() == 2:
        wave = wave.unsqueeze(0)
    if wave.dim() != 3 or wave.shape[-1] < 1:
        raise ValueError(f"audio waveform must be [batch, channels, samples], got {tuple(wave.shape)}")
    wave = wave.to(device=model.device, dtype=torch.float32).mean(dim=1).contiguous()
    target = int(dac.sample_rate)
    if sr != target:
        taps, o, n, width = _taps(model, sr, target)
        wave = rt.op_resample_sinc(wave, o, n, taps, width)
    return wave


def check_encoder(dac) -> None:
    if dac is None or not getattr(dac, "has_encoder", False):
        raise FoleyRuntimeError("audio editing encodes the input clip with the DAC-VAE encoder, and this DAC checkpoint has no "
                                "encoder weights: load the full VAE checkpoint (encoder + decoder) as the DAC model")


def encode_source(wave48: torch.Tensor, model, dac, La: int) -> torch.Tensor:
    """Mono 48 kHz [B, N] -> x0 [B, latent_dim, La]: trim / zero-pad to La * hop samples, foley_dac_encode, posterior mean."""
    check_encoder(dac)
    T = La * dac.cfg.hop
    n = wave48.shape[1]
    w = wave48[:, :T] if n >= T else torch.nn.functional.pad(wave48, (0, T - n))
    model.attach_dac(dac)
    params = model.ctx.dac_encode(w.unsqueeze(1).contiguous())
    return params[:, :model.cfg.latent_dim].contiguous()


def check_flowedit_length(La: int, frame_rate: int, n_samples: int, hop: int, sample_rate: int) -> None:
    """FlowEdit edits what is there: a clip longer than the source audio is refused (those frames have no source)."""
    if n_samples // hop < La:
        raise ValueError(f"the clip ({La / frame_rate:g} s) is longer than the input audio ({n_samples / sample_rate:.3f} s): FlowEdit "
                         "edits the source and the frames past its end have none; shorten the duration or use audio= without source_prompt")


def prepare_edit(audio: dict, model, dac, audio_len_in_s: float, steps: int, solver: str, batch_size: int,
                 strength: float = 1.0, regenerate: Optional[Sequence[Tuple[float, float]]] = None,
                 crossfade_s: float = 0.1, flowedit: Optional[dict] = None):
    """The EditSpec of a node call: source latents of `audio`, the mask of `regenerate` (plus the extension tail when the clip
    is longer than the audio) and the strength, with every refusal raised before any sampling work.
    flowedit ({"source_scale", "noise"}): the FlowEditSpec of the call instead - the mask of `regenerate` restricts the edit in time
    (None without spans: the whole clip), and a clip longer than the source audio is refused."""
    check_encoder(dac)
    tables.edit_start(steps, solver, strength)                # refuses n_keep = 0 / strength outside (0, 1]
    B = audio["waveform"].shape[0] if audio["waveform"].dim() == 3 else 1
    if B not in (1, batch_size):
        raise ValueError(f"audio batch {B} must be 1 (shared by all clips) or batch_size ({batch_size})")
    fr = model.cfg.frame_rate
    La = int(audio_len_in_s * fr)
    hop = dac.cfg.hop
    wave = prepare_waveform(audio, model, dac)
    src_frames = wave.shape[1] // hop
    if flowedit is not None:
        check_flowedit_length(La, fr, wave.shape[1], hop, dac.sample_rate)
        mask = build_mask(La, regenerate, crossfade_s, frame_rate=fr) if regenerate is not None else None
        x0 = encode_source(wave, model, dac, La)
        return FlowEditSpec(x0=x0, strength=float(strength), mask=mask, source_scale=float(flowedit.get("source_scale", 2.0)),
                            noise=flowedit.get("noise", "fresh"))
    if src_frames < La and float(strength) != 1.0:
        raise ValueError(f"the clip ({La / fr:g} s) is longer than the input audio ({wave.shape[1] / dac.sample_rate:.3f} s): "
                         "the frames past its end have no source to noise, so extension needs strength 1.0")
    mask = build_mask(La, regenerate, crossfade_s, src_frames=src_frames, frame_rate=fr)
    x0 = encode_source(wave, model, dac, La)
    return EditSpec(x0=x0, strength=float(strength), mask=mask)
