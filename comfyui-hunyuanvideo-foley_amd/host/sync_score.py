"""Audio-visual sync score of generated clips on the HIP engine (the DeSync measure of V2A papers).

The Synchformer checkpoint the Dependencies Loader resolves holds, next to the visual extractor the sampler conditions on, an
audio branch and a sync head; together they classify the offset between a video and its audio over the grid -2 .. 2 s in 0.2 s
steps.  Reference (/root/reference/hunyuanvideo_foley/models/synchformer): `encode_audio_with_sync` (synchformer.py:294-317: 16 kHz
audio -> 0.64 s segments at a 0.32 s stride -> log-mel -> AST features), `Synchformer.compare_v_a` (:54-68) + `GlobalTransformer`
(:115-187), `make_class_grid(-2, 2, 21)`; compute_desync_score.py runs them under fp16 autocast.

Everything runs on libfoley_hip.so:
  * foley_op_resample_sinc   48 kHz -> 16 kHz (torchaudio.functional.resample's sinc_interp_hann, taps built here);
  * foley_op_logmel          segments -> STFT power -> HTK mel -> log -> AST normalisation, written as the im2col matrix of the
                             AST patch embedding, so that the embedding is one foley_op_gemm;
  * the AST (12 pre-LN ViT-B layers, 74 tokens), the frequency aggregation layer (a CLS over the 12 frequency tokens of each time
    step, the visual extractor's spatial aggregation layer) and the sync head (3 blocks, 8 heads x 96 through
    foley_op_attention_hd at head_dim 96) on the engine of host/encoders_hip.py.
PyTorch only re-views / concatenates tensors between the ops.  There is no fallback: CPU tensors raise.

Windows: the head's position table has 198 rows = OFF + 14 segments x 8 visual tokens + MOD + 14 x 6 audio tokens, so a window is
14 segments (4.8 s).  With S = min(S_v, S_a) segments aligned at segment 0, the window at segment 0 is scored and, when S > 14,
the one at S - 14 (the first and the last 4.8 s); `window_stride` adds the windows in between.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from . import encoders_hip as EH
from . import runtime as rt

Tensor = torch.Tensor
SD = Dict[str, Tensor]

SR_SYNC = 16000
SEG_SAMPLES, SEG_STEP = 10240, 5120            # synchformer.py:299-300
N_FFT, HOP, WIN, N_MELS, T_SPEC = 1024, 160, 400, 128, 66
MEL_PITCH = 32                                 # widest HTK triangle of the 513-bin, 128-mel table: 23 bins
WIN_SEGMENTS = 14                              # GlobalTransformer pos_emb_block_shape 198 = 1 + 14*8 + 1 + 14*6
WIN_SECONDS = 4.8
VIS_TOK, AUD_TOK = 8, 6                        # tokens per segment
AST_HEADS, SYNC_HEADS = 12, 8
OFFSET_GRID = torch.linspace(-2.0, 2.0, 21)    # make_class_grid(-2, 2, 21) (np.linspace -> float32)


# ----------------------------------------------------------------------------- host-built tables
def sinc_resample_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """torchaudio.functional.resample's default kernel (sinc_interp_hann): returns (taps [new, 2*width + orig] fp32, orig, new,
    width) with orig / new reduced by their gcd.  Computed in float64 and rounded once to fp32.  For 48000 -> 16000: orig 3,
    new 1, base = 0.99, width = ceil(6 * 3 / 0.99) = 19, t = clamp((arange(-19, 22) / 3) * base, -6, 6),
    k = sinc(pi t) * cos(pi t / 12)^2 * base / 3 (41 taps)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return k.to(torch.float32), orig, new, width


def htk_mel_filterbank(n_freqs: int = N_FFT // 2 + 1, n_mels: int = N_MELS, sample_rate: int = SR_SYNC, f_min: float = 0.0,
                       f_max: Optional[float] = None) -> Tensor:
    """torchaudio MelSpectrogram's filter bank at its defaults (mel_scale 'htk', norm None): [n_freqs, n_mels] fp32."""
    f_max = sample_rate / 2 if f_max is None else f_max
    hz2mel = lambda f: 2595.0 * torch.log10(1.0 + f / 700.0)
    mel2hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m = torch.linspace(float(hz2mel(torch.tensor(f_min, dtype=torch.float64))), float(hz2mel(torch.tensor(f_max, dtype=torch.float64))),
                       n_mels + 2, dtype=torch.float64)
    f_pts = mel2hz(m)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0).to(torch.float32)


def logmel_tables(device) -> Dict[str, Tensor]:
    """The device tables of foley_op_logmel: basis [2, 400, 544] = periodic Hann(400) placed at offset 312 of the 1024-point frame
    times cos / sin of the real DFT (angles reduced exactly: 2 pi ((m + 312) k mod 1024) / 1024, float64 -> fp32), and the mel
    triangles as contiguous bin ranges (mel_lo, mel_len int32 [128], mel_w [128, 32] fp32)."""
    m = torch.arange(WIN, dtype=torch.int64)
    k = torch.arange(N_FFT // 2 + 1, dtype=torch.int64)
    off = (N_FFT - WIN) // 2
    win = 0.5 - 0.5 * torch.cos(2 * math.pi * m.to(torch.float64) / WIN)      # torch.hann_window(400, periodic=True)
    ang = 2 * math.pi * (((m[:, None] + off) * k[None, :]) % N_FFT).to(torch.float64) / N_FFT
    basis = torch.zeros(2, WIN, 544, dtype=torch.float64)
    basis[0, :, :k.numel()] = win[:, None] * torch.cos(ang)
    basis[1, :, :k.numel()] = -win[:, None] * torch.sin(ang)
    fb = htk_mel_filterbank()                                                  # [513, 128]
    lo = torch.zeros(N_MELS, dtype=torch.int32)
    ln = torch.zeros(N_MELS, dtype=torch.int32)
    w = torch.zeros(N_MELS, MEL_PITCH, dtype=torch.float32)
    for c in range(N_MELS):
        nz = torch.nonzero(fb[:, c] > 0).flatten()
        if nz.numel() == 0:
            continue
        a, b = int(nz[0]), int(nz[-1]) + 1
        if b - a > MEL_PITCH:
            raise ValueError("mel triangle wider than the table pitch")
        lo[c], ln[c] = a, b - a
        w[c, :b - a] = fb[a:b, c]
    return {"basis": basis.to(torch.float32).to(device).contiguous(), "mel_lo": lo.to(device), "mel_len": ln.to(device),
            "mel_w": w.to(device).contiguous()}


# ----------------------------------------------------------------------------- segments and windows
def num_audio_segments(n16: int) -> int:
    """0.64 s segments at a 0.32 s stride of a 16 kHz signal (synchformer.py:298-301)."""
    return (n16 - SEG_SAMPLES) // SEG_STEP + 1 if n16 >= SEG_SAMPLES else 0


def resampled_length(n: int, sample_rate: int) -> int:
    g = math.gcd(int(sample_rate), SR_SYNC)
    return -(-n * (SR_SYNC // g) // (int(sample_rate) // g))


def window_starts(s_v: int, s_a: int, window_stride: Optional[int] = None) -> List[int]:
    """First segment of every scored window: S = min(S_v, S_a) aligned at segment 0; the window at 0 and, when S > 14, the one at
    S - 14; `window_stride` > 0 adds 0, stride, 2*stride, ... below S - 14."""
    S = min(s_v, s_a)
    if S < WIN_SEGMENTS:
        raise ValueError(f"the sync score needs at least {WIN_SECONDS} s of audio and video ({WIN_SEGMENTS} segments of 0.64 s at "
                         f"a 0.32 s stride); got {S} segment(s) (video {s_v}, audio {s_a})")
    last = S - WIN_SEGMENTS
    starts = {0, last}
    if window_stride:
        if window_stride < 1:
            raise ValueError("window_stride must be a positive number of segments")
        starts.update(range(0, last, int(window_stride)))
    return sorted(starts)


# ----------------------------------------------------------------------------- the networks on the engine
def audio_features_hip(sd: SD, w16: Tensor, E: "EH._Engine", tables: Dict[str, Tensor]) -> Tensor:
    """16 kHz waveform [B, N16] fp32 on the GPU -> afeats [B, S_a, 6, 768] fp32 (encode_audio_with_sync + AST with
    frequency aggregation, ast_model.py:147-254)."""
    B, N16 = w16.shape
    S = num_audio_segments(N16)
    a = "afeat_extractor.ast."
    patches = rt.op_logmel(w16.contiguous(), tables["basis"], tables["mel_lo"], tables["mel_len"], tables["mel_w"], E.dtype)
    tok = E.linear(patches, sd, a + "embeddings.patch_embeddings.projection.weight", a + "embeddings.patch_embeddings.projection.bias",
                   out_f32=True)                                                          # [B*S*72, D]
    D = tok.shape[1]
    G, N = B * S, 74
    f32 = lambda k: sd[k].to(E.dev, torch.float32)
    pos = f32(a + "embeddings.position_embeddings")                                        # [1, 74, D]
    x = torch.cat((f32(a + "embeddings.cls_token").expand(G, 1, D), f32(a + "embeddings.distillation_token").expand(G, 1, D),
                   tok.view(G, 72, D)), dim=1)
    x = (x + pos).reshape(G * N, D).contiguous()                                          # fp32 residual stream
    rows = E.index(("all", G, N), lambda: (torch.arange(G) * N)[:, None] + torch.arange(N)[None])
    depth = 1 + max(int(k[len(a) + 14:].split(".")[0]) for k in sd if k.startswith(a + "encoder.layer."))
    for i in range(depth):                                                                 # ASTLayer (pre-LN, eps 1e-12, exact GELU)
        l = f"{a}encoder.layer.{i}."
        h = E.ln(x, sd, l + "layernorm_before", 1e-12)
        q_ = l + "attention.attention."
        fq = E.fused(sd, q_ + "qkv#", [q_ + n + ".weight" for n in ("query", "key", "value")], [q_ + n + ".bias" for n in ("query", "key", "value")])
        att = E.attention_regrouped(E.linear(h, fq, q_ + "qkv#.w", q_ + "qkv#.b"), AST_HEADS, rows, rows).reshape(G * N, D)
        E.linear_residual(x, att, sd, l + "attention.output.dense.weight", l + "attention.output.dense.bias")
        hid = E.linear(E.ln(x, sd, l + "layernorm_after", 1e-12), sd, l + "intermediate.dense.weight", l + "intermediate.dense.bias",
                       act="gelu_erf")
        E.linear_residual(x, hid, sd, l + "output.dense.weight", l + "output.dense.bias")
    h = E.ln(x, sd, a + "layernorm", 1e-12, out_dtype=torch.float32)                      # last_hidden_state
    # restore_freq_temp_dims + FrequencyTransformerEncoderLayer: tokens 2 + f*6 + t -> groups (segment, t) of the 12 frequencies
    body = h.view(G, N, D)[:, 2:].reshape(G, 12, 6, D).permute(0, 2, 1, 3).reshape(G * 6, 12, D)
    f_ = "afeat_extractor.freq_attn_agg."
    Gf, L = G * 6, 13
    y = torch.cat((f32(f_ + "cls_token").expand(Gf, 1, D), body), dim=1).reshape(Gf * L, D).contiguous()
    rows_f = E.index(("all", Gf, L), lambda: (torch.arange(Gf) * L)[:, None] + torch.arange(L)[None])
    att = E.attention_regrouped(E.linear(E.ln(y, sd, f_ + "norm1"), sd, f_ + "self_attn.in_proj_weight", f_ + "self_attn.in_proj_bias"),
                                AST_HEADS, rows_f, rows_f).reshape(Gf * L, D)
    E.linear_residual(y, att, sd, f_ + "self_attn.out_proj.weight", f_ + "self_attn.out_proj.bias")
    hid = E.linear(E.ln(y, sd, f_ + "norm2"), sd, f_ + "linear1.weight", f_ + "linear1.bias", act="gelu_erf")
    E.linear_residual(y, hid, sd, f_ + "linear2.weight", f_ + "linear2.bias")
    return y.view(Gf, L, D)[:, 0].reshape(B, S, 6, D).clone()


def sync_logits_hip(sd: SD, vfeat: Tensor, afeat: Tensor, starts: List[int], E: "EH._Engine") -> Tensor:
    """Synchformer.compare_v_a over windows: vfeat [B, S_v*8, D] / afeat [B, S_a, 6, D] fp32 on the GPU -> logits [B, W, 21] fp32.
    vproj / aproj and the two input LayerNorms act per token, so they run once over all segments; every window then is one
    198-token sequence of the head (the windows of all clips are the batch of its GEMMs and attentions)."""
    B, D = vfeat.shape[0], vfeat.shape[-1]
    t = "transformer."
    vis = E.linear(vfeat.reshape(-1, D).to(E.dtype).contiguous(), sd, "vproj.weight", "vproj.bias", out_f32=True)
    aud = E.linear(afeat.reshape(-1, D).to(E.dtype).contiguous(), sd, "aproj.weight", "aproj.bias", out_f32=True)
    vis = E.ln(vis, sd, t + "vis_in_lnorm", 1e-5, out_dtype=torch.float32).view(B, -1, D)
    aud = E.ln(aud, sd, t + "aud_in_lnorm", 1e-5, out_dtype=torch.float32).view(B, -1, D)
    W, Nv, Na = len(starts), WIN_SEGMENTS * VIS_TOK, WIN_SEGMENTS * AUD_TOK
    L = 2 + Nv + Na
    G = B * W
    f32 = lambda k: sd[k].to(E.dev, torch.float32)
    x = torch.cat((f32(t + "OFF_tok").expand(B, W, 1, D),
                   torch.stack([vis[:, s * VIS_TOK:s * VIS_TOK + Nv] for s in starts], dim=1),
                   f32(t + "MOD_tok").expand(B, W, 1, D),
                   torch.stack([aud[:, s * AUD_TOK:s * AUD_TOK + Na] for s in starts], dim=1)), dim=2)   # [B, W, 198, D]
    x = (x + f32(t + "pos_emb_cfg.pos_emb")).reshape(G * L, D).contiguous()
    hd = D // SYNC_HEADS
    depth = 1 + max(int(k[len(t) + 7:].split(".")[0]) for k in sd if k.startswith(t + "blocks."))
    for i in range(depth):                                                                 # Block: pre-LN, eps 1e-5, exact GELU
        b = f"{t}blocks.{i}."
        fq = E.fused(sd, b + "attn.qkv#", [b + f"attn.{n}.weight" for n in ("query", "key", "value")],
                     [b + f"attn.{n}.bias" for n in ("query", "key", "value")])
        qkv = E.linear(E.ln(x, sd, b + "ln1", 1e-5), fq, b + "attn.qkv#.w", b + "attn.qkv#.b").view(G, L, 3, SYNC_HEADS, hd)
        qkv = qkv.permute(2, 0, 3, 1, 4)                                                   # [3, G, H, L, 96]
        att = E.attention(qkv[0], qkv[1], qkv[2]).reshape(G * L, D)
        E.linear_residual(x, att, sd, b + "attn.proj.weight", b + "attn.proj.bias")
        hid = E.linear(E.ln(x, sd, b + "ln2", 1e-5), sd, b + "mlp.0.weight", b + "mlp.0.bias", act="gelu_erf")
        E.linear_residual(x, hid, sd, b + "mlp.2.weight", b + "mlp.2.bias")
    x0 = x.view(G, L, D)[:, 0].contiguous()                                               # ln_f acts per row: the OFF row only
    h = E.ln(x0, sd, t + "ln_f", 1e-5)
    # off_head: 21 outputs staged as 32 zero-padded rows (aligned output rows for the GEMM epilogue)
    n_off = sd[t + "off_head.weight"].shape[0]
    pad = (n_off + 31) // 32 * 32
    if t + "off_head#w" not in E.mats:
        wp = torch.zeros(pad, D, dtype=torch.float32)
        bp = torch.zeros(pad, dtype=torch.float32)
        wp[:n_off] = sd[t + "off_head.weight"].detach().float().cpu()
        bp[:n_off] = sd[t + "off_head.bias"].detach().float().cpu()
        E.mat(t + "off_head#w", wp)
        E.vec(t + "off_head#b", bp)
    logits = E.linear(h, {t + "off_head#w": E.mats[t + "off_head#w"], t + "off_head#b": E.vecs[t + "off_head#b"]},
                      t + "off_head#w", t + "off_head#b", out_f32=True)
    return logits[:, :n_off].reshape(B, W, n_off).contiguous()


# ----------------------------------------------------------------------------- public API
@dataclass
class SyncResult:
    """logits / probs [B, W, 21] over the offset grid (-2 .. 2 s, 0.2 s steps) for the windows starting at segments `starts`
    (0.32 s each); offset_s [B, W] the grid value of each window's argmax; desync_s [B] the mean |offset_s| over the windows;
    order: batch indices by ascending desync_s, ties broken by the larger probability of offset 0 (averaged over windows)."""
    logits: Tensor
    probs: Tensor
    offset_s: Tensor
    desync_s: Tensor
    order: List[int]
    starts: List[int]
    grid: Tensor


def _sync_state(deps, device, dtype) -> SD:
    """The audio branch + sync head of the Synchformer checkpoint, loaded once from deps['synchformer_path'] and cached on the
    deps (deps['sync_score_model'] may also be preset to a state dict, e.g. synthesised weights)."""
    from . import encoders as _enc
    sd = deps.get("sync_score_model")
    if sd is None:
        path = deps.get("synchformer_path")
        if not path:
            raise RuntimeError("HUNYUAN_DEPS carries no Synchformer checkpoint (synchformer_path)")
        from ..nodes import _load_state_dict
        sd = _load_state_dict(path)
    first = next(iter(sd.values()))
    if first.device != torch.device(device) or any(not k.startswith(_enc.SYNC_PREFIXES) for k in sd):
        sd = _enc.load_synchformer_sync_state(sd, device, torch.float32)
    deps["sync_score_model"] = sd
    return sd


def _visual_state(deps, device) -> SD:
    """The visual extractor's state for IMAGE input: the one the sampler already holds (deps['syncformer_model']), or loaded from
    the checkpoint like the sampler loads it (nodes._ensure_visual_encoders)."""
    from . import encoders as _enc
    sd = deps.get("syncformer_model")
    if not isinstance(sd, dict):
        path = deps.get("synchformer_path")
        if not path:
            raise RuntimeError("HUNYUAN_DEPS carries no Synchformer checkpoint (synchformer_path)")
        from ..nodes import _load_state_dict
        sd = _load_state_dict(path)
    if next(iter(sd.values())).device != torch.device(device) or any(not k.startswith("vfeat_extractor.") for k in sd):
        sd = _enc.load_synchformer_state(sd, device, torch.float32)
    return sd


def _tables(deps, device) -> Dict[str, Tensor]:
    key = ("sync_score_tables", str(device))
    t = deps.get(key)
    if t is None:
        t = deps[key] = logmel_tables(device)
    return t


@torch.inference_mode()
def sync_scores(deps, waveform: Tensor, sample_rate: int, *, syncformer_feat: Optional[Tensor] = None, image: Optional[Tensor] = None,
                frame_rate: Optional[float] = None, dtype: torch.dtype = torch.float16,
                window_stride: Optional[int] = None) -> SyncResult:
    """Score how well each clip of an AUDIO batch is in sync with its video.

    waveform [B, 1, N] or [B, N] (the sampler's AUDIO tensor) at sample_rate 48000 (resampled on the device) or 16000.  The visual
    features are `syncformer_feat` [1 or B, S_v*8, 768] (what the sampler conditions on) or, from IMAGE frames [T, H, W, C] at
    `frame_rate`, the HIP-engine Synchformer visual extractor.  dtype: GEMM / attention operands - float16 as the reference's
    autocast, float32 the parity mode."""
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError("dtype must be float16, bfloat16 or float32")
    wav = waveform.reshape(waveform.shape[0], -1) if waveform.dim() == 3 else waveform
    if wav.dim() != 2 or (waveform.dim() == 3 and waveform.shape[1] != 1):
        raise ValueError("waveform must be [B, 1, N] (mono) or [B, N]")
    if not wav.is_cuda:
        raise rt.FoleyRuntimeError("the sync score runs on the HIP engine: the waveform must be on the GPU")
    device = wav.device
    B = wav.shape[0]
    if syncformer_feat is None:
        if image is None or frame_rate is None:
            raise ValueError("pass syncformer_feat, or image frames with their frame_rate")
        from . import encoders as _enc
        _, f25 = _enc.select_frames(image, image.shape[0] / float(frame_rate), frame_rate, device=device)
        syncformer_feat = EH.encode_video_with_sync_hip(_visual_state(deps, device), _enc.synchformer_preprocess(f25.to(device)), dtype)
    vfeat = syncformer_feat.to(device=device, dtype=torch.float32)
    if vfeat.dim() != 3 or vfeat.shape[1] % VIS_TOK or vfeat.shape[0] not in (1, B):
        raise ValueError("syncformer_feat must be [1 or B, S_v*8, 768]")
    s_v = vfeat.shape[1] // VIS_TOK
    n16 = wav.shape[1] if int(sample_rate) == SR_SYNC else resampled_length(wav.shape[1], sample_rate)
    s_a = num_audio_segments(n16)
    starts = window_starts(s_v, s_a, window_stride)            # raises below 4.8 s before any GPU work
    sd = _sync_state(deps, device, dtype)
    E = EH._engine_for(sd, device, dtype)
    wav = wav.to(torch.float32).contiguous()
    if int(sample_rate) != SR_SYNC:
        key = ("sync_score_taps", int(sample_rate), str(device))
        if key not in deps:
            taps, o, n, width = sinc_resample_taps(int(sample_rate), SR_SYNC)
            deps[key] = (taps.to(device), o, n, width)
        taps, o, n, width = deps[key]
        wav = rt.op_resample_sinc(wav, o, n, taps, width)
    afeat = audio_features_hip(sd, wav, E, _tables(deps, device))
    if vfeat.shape[0] != B:
        vfeat = vfeat.expand(B, -1, -1)
    logits = sync_logits_hip(sd, vfeat.contiguous(), afeat, starts, E)
    return summarize(logits, starts)


def summarize(logits: Tensor, starts: List[int]) -> SyncResult:
    """SyncResult of logits [B, W, 21] (the argmax, mean |offset| and ranking of the public API)."""
    grid = OFFSET_GRID.to(logits.device)
    probs = torch.softmax(logits, dim=-1)
    offset = grid[logits.argmax(dim=-1)]
    desync = offset.abs().mean(dim=1)
    p0 = probs[..., int(torch.argmin(grid.abs()))].mean(dim=1)
    d, p = desync.tolist(), p0.tolist()
    order = sorted(range(len(d)), key=lambda i: (d[i], -p[i], i))
    return SyncResult(logits=logits, probs=probs, offset_s=offset, desync_s=desync, order=order, starts=list(starts), grid=grid)


def best_synced(audio_batch: dict, result: SyncResult) -> dict:
    """The AUDIO dict of the best-synced clip (result.order[0]) - what SelectAudioFromBatch does for an index."""
    wf = audio_batch["waveform"]
    i = result.order[0]
    if not 0 <= i < wf.shape[0]:
        raise ValueError("the sync result does not belong to this audio batch")
    return {"waveform": wf[i].unsqueeze(0), "sample_rate": audio_batch["sample_rate"]}
