"""CLAP score of generated clips on the HIP engine: how well each clip matches its prompt.

The score is the cosine between the CLAP audio embedding of a clip and the CLAP text embedding of its prompt - the metric V2A
papers report next to DeSync (host/sync_score.py).  The definition restated here is `transformers`' ClapModel:
ClapFeatureExtractor (truncation "rand_trunc", padding "repeatpad") -> ClapAudioModel (HTSAT: a Swin transformer over a
log-mel image) -> audio_projection -> L2 normalisation, against ClapTextModel -> pooler -> text_projection -> L2 normalisation.
The checkpoint is the one the Dependencies Loader already pulls for the text encoder (nodes.CLAP_REPO).

Everything runs on libfoley_hip.so:
  * foley_op_resample_sinc     other sample rates -> 48 kHz (taps from sync_score.sinc_resample_taps);
  * foley_op_melspec_db        ten-second windows -> STFT power -> Slaney mel -> dB, [windows, 1001, 64];
  * foley_op_spec_patches      BatchNorm affine -> bicubic time resize 1001 -> 1024 -> reshape_mel2img fold -> im2col of the 4x4
                               patch embedding, so that the embedding is one foley_op_gemm;
  * the Swin stages on the engine of host/encoders_hip.py: foley_op_ln_mod, foley_op_gemm (fused q/k/v, exact-GELU and residual
    epilogues), foley_op_window_attention (64-token windows, head dim 32, relative-position bias, shift mask) and, between
    stages, foley_op_gather_rows for the patch merging;
  * the text tower is encoders_hip.clap_text_hidden_hip.
PyTorch re-views tensors between the ops and, on the few pooled rows (one per window / prompt), does the token mean, tanh, ReLU
and the L2 normalisation.  There is no fallback: CPU tensors raise.

Deviation from the extractor, on purpose: a clip longer than ten seconds is cropped AT RANDOM by the extractor (rand_trunc).
Here the windows start at k * 480000 for every whole window and, if a remainder is left, one more window ends at the clip's
end; every window is embedded and the clip's score is the mean of its windows' cosines - the same clip always gets the same score.

Served configurations: the non-fusion tower (enable_fusion False), 64-token windows (window_size 8), head dim 32, 4x4 patches
at stride 4, grids that are a multiple of the window at every stage.  Anything else is refused with a message.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import encoders_hip as EH
from . import runtime as rt

Tensor = torch.Tensor
SD = Dict[str, Tensor]

SR_CLAP = 48000
WIN_SAMPLES, N_FFT, HOP, N_FRAMES = 480000, 1024, 480, 1001
N_BINS, BINP, N_MELS, MEL_PITCH = 513, 544, 64, 32
WINDOW, WIN_TOKENS, HEAD_DIM = 8, 64, 32
AUDIO_PREFIX = "audio_model.audio_encoder."
BN_EPS = 1e-5          # ClapAudioEncoder builds nn.BatchNorm2d(num_mel_bins) with its default eps; no config field sets it (nor the 1e-5 of the
                       # patch / merging / final nn.LayerNorm, which are built with defaults too)


# ----------------------------------------------------------------------------- host-built tables
def _hz_to_mel_slaney(f: Tensor) -> Tensor:
    lin = 3.0 * f / 200.0
    log = 15.0 + torch.log(f.clamp_min(1e-300) / 1000.0) * (27.0 / math.log(6.4))
    return torch.where(f >= 1000.0, log, lin)


def _mel_to_hz_slaney(m: Tensor) -> Tensor:
    lin = 200.0 * m / 3.0
    log = 1000.0 * torch.exp((math.log(6.4) / 27.0) * (m - 15.0))
    return torch.where(m >= 15.0, log, lin)


def slaney_mel_tables(frequency_min: float = 0.0, frequency_max: float = 14000.0, n_mels: int = N_MELS, n_freqs: int = N_BINS,
                      sampling_rate: int = SR_CLAP, pitch: int = MEL_PITCH):
    """The extractor's `mel_filters_slaney` (audio_utils.mel_filter_bank, mel_scale "slaney", norm "slaney") in float64, and its
    triangles as contiguous bin runs for the kernel's short dot: returns (fb [n_freqs, n_mels] fp64, lo int32 [n_mels],
    length int32 [n_mels], w fp32 [n_mels, pitch])."""
    fft_freqs = torch.linspace(0, sampling_rate // 2, n_freqs, dtype=torch.float64)
    edge = torch.tensor([frequency_min, frequency_max], dtype=torch.float64)
    mel = _hz_to_mel_slaney(edge)
    f_pts = _mel_to_hz_slaney(torch.linspace(float(mel[0]), float(mel[1]), n_mels + 2, dtype=torch.float64))
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - fft_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0)
    fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    lo = torch.zeros(n_mels, dtype=torch.int32)
    ln = torch.zeros(n_mels, dtype=torch.int32)
    w = torch.zeros(n_mels, pitch, dtype=torch.float32)
    for c in range(n_mels):
        nz = torch.nonzero(fb[:, c] > 0).flatten()
        if nz.numel() == 0:
            continue
        a, b = int(nz[0]), int(nz[-1]) + 1
        if b - a > pitch or int((fb[a:b, c] > 0).sum()) != b - a:
            raise ValueError("mel triangle wider than the table pitch, or not one contiguous run of bins")
        lo[c], ln[c] = a, b - a
        w[c, :b - a] = fb[a:b, c].to(torch.float32)
    return fb, lo, ln, w


def melspec_tables(device, frequency_min: float, frequency_max: float) -> Dict[str, Tensor]:
    """The device tables of foley_op_melspec_db: basis [2, 1024, 544] = periodic Hann(1024) times cos / -sin of the real DFT
    (angles reduced exactly: 2 pi (m k mod 1024) / 1024, float64 -> fp32, bins >= 513 zero) and the Slaney triangles."""
    m = torch.arange(N_FFT, dtype=torch.int64)
    k = torch.arange(N_BINS, dtype=torch.int64)
    win = 0.5 - 0.5 * torch.cos(2 * math.pi * m.to(torch.float64) / N_FFT)
    ang = 2 * math.pi * ((m[:, None] * k[None, :]) % N_FFT).to(torch.float64) / N_FFT
    basis = torch.zeros(2, N_FFT, BINP, dtype=torch.float64)
    basis[0, :, :N_BINS] = win[:, None] * torch.cos(ang)
    basis[1, :, :N_BINS] = -win[:, None] * torch.sin(ang)
    _, lo, ln, w = slaney_mel_tables(frequency_min, frequency_max)
    return {"basis": basis.to(torch.float32).to(device).contiguous(), "mel_lo": lo.to(device), "mel_len": ln.to(device),
            "mel_w": w.to(device).contiguous()}


def cubic_resize_table(n_in: int, n_out: int, dtype: torch.dtype = torch.float64) -> Tuple[Tensor, Tensor]:
    """F.interpolate(mode="bicubic", align_corners=True) along one axis as a 4-tap table: (idx int64 [n_out, 4], w `dtype`
    [n_out, 4]) with PyTorch's A = -0.75 kernel and border indices clamped; out[o] = sum_j w[o, j] * in[idx[o, j]].  n_in == n_out
    is the identity (weights 0, 1, 0, 0).

    `dtype` is the type ATen computes the source coordinate in - the type of the tensor it resizes: scale = (n_in - 1) / (n_out - 1),
    src = scale * o, t = src - floor(src), then the cubic coefficients, all in that type (UpSample.h: area_pixel_compute_scale,
    guard_index_and_lambda, get_cubic_upsample_coefficients).  float64 is the exact table.  The tower resizes an fp32 spectrogram,
    so transformers' result carries t rounded in fp32 (an error up to 1e-4 at the far end of the 1001-frame axis, 1.6e-4 on the
    normalised image): the scorer builds the table in float32 to reproduce the arithmetic of the model it restates."""
    A = -0.75
    o = torch.arange(n_out, dtype=dtype)
    scale = torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(max(n_out - 1, 1), dtype=dtype)
    src = scale * o
    i0 = torch.floor(src).clamp(max=n_in - 1)
    t = (src - i0).clamp(0.0, 1.0)
    near = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0              # cubic_convolution1, |x| <= 1
    far = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A          # cubic_convolution2, 1 < |x| < 2
    x2 = 1.0 - t
    w = torch.stack((far(t + 1.0), near(t), near(x2), far(x2 + 1.0)), dim=1)
    idx = (i0.to(torch.int64)[:, None] + torch.arange(-1, 3)[None, :]).clamp(0, n_in - 1)
    return idx, w


def window_tables(B: int, h: int, w: int, shift: int, window: int = WINDOW) -> Tuple[Tensor, Optional[Tensor]]:
    """Source rows of Swin's shifted windows: (table int32 [B * nW, window^2], mask fp32 [nW, window^2, window^2] or None).
    Token (b, y, x) of a [B, h, w] grid is row (b h + y) w + x; table = window_partition(torch.roll(rows, (-shift, -shift)))
    (ClapAudioLayer.forward), so the same table scatters the outputs back (the reverse roll).  mask = get_attn_mask: -100 between
    tokens of different cyclic-shift regions, 0 otherwise; None without a shift."""
    if h % window or w % window:
        raise ValueError(f"a {h} x {w} grid is not a multiple of the {window}-token window side (the tower's padding path is not built)")
    rows = torch.arange(B * h * w, dtype=torch.int64).view(B, h, w)
    if shift:
        rows = torch.roll(rows, shifts=(-shift, -shift), dims=(1, 2))
    part = lambda t: t.reshape(t.shape[0], h // window, window, w // window, window).permute(0, 1, 3, 2, 4).reshape(-1, window * window)
    table = part(rows).to(torch.int32).contiguous()
    mask = None
    if shift:
        region = lambda n: (torch.arange(n) >= n - window).long() + (torch.arange(n) >= n - shift).long()
        img = (region(h)[:, None] * 3 + region(w)[None, :])[None]
        mw = part(img).to(torch.float32)
        diff = mw[:, None, :] - mw[:, :, None]
        mask = torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff)).contiguous()
    return table, mask


def merge_table(h: int, w: int) -> Tensor:
    """ClapAudioPatchMerging's interleave as source rows of ONE image: int32 [(h/2) (w/2) 4]; merged token (i, j) reads rows
    (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) in that order (the x0..x3 concatenation along the channels)."""
    if h % 2 or w % 2:
        raise ValueError("patch merging needs an even grid")
    i = torch.arange(h // 2)[:, None, None]
    j = torch.arange(w // 2)[None, :, None]
    dy = torch.tensor([0, 1, 0, 1])[None, None, :]
    dx = torch.tensor([0, 0, 1, 1])[None, None, :]
    return ((2 * i + dy) * w + 2 * j + dx).reshape(-1).to(torch.int32)


def clap_windows(n: int) -> List[int]:
    """First sample of every ten-second window of an n-sample clip at 48 kHz: [0] up to ten seconds (the extractor's repeatpad
    fills the window); beyond, k * 480000 for every whole window and, if a remainder is left, one more window ending at n."""
    if n < N_FFT:
        raise ValueError(f"the CLAP score needs at least one FFT frame ({N_FFT} samples at 48 kHz); got {n}")
    if n <= WIN_SAMPLES:
        return [0]
    starts = [k * WIN_SAMPLES for k in range(n // WIN_SAMPLES)]
    if n % WIN_SAMPLES:
        starts.append(n - WIN_SAMPLES)
    return starts


def fold_index(spec_size: int, freq_ratio: int, n_freq: int) -> Tensor:
    """reshape_mel2img as an index map: int64 [freq_ratio * n_freq, spec_size, 2], img[r * n_freq + f, t] = spec[r * spec_size + t, f]
    (time index, frequency index) of a [spec_size * freq_ratio, n_freq] resized spectrogram."""
    R = torch.arange(freq_ratio * n_freq)[:, None]
    t = torch.arange(spec_size)[None, :]
    return torch.stack(((R // n_freq) * spec_size + t, (R % n_freq).expand(-1, spec_size)), dim=-1)


# ----------------------------------------------------------------------------- engine helpers
def _granule(E: "EH._Engine") -> int:
    return 64 if E.half else 32      # elements of the GEMM's 128-byte K slice


def _meta(E: "EH._Engine") -> dict:
    """What the scorer keeps on an engine for as long as the staged weights live: the unpadded widths of the layers and the resize
    table.  A dict of its own - E.tabs is the bounded, evicting cache of _Engine.index and must only hold what can be rebuilt."""
    m = getattr(E, "clap_meta", None)
    if m is None:
        m = E.clap_meta = {}
    return m


def _staged(E: "EH._Engine", wkey: str, build):
    """A linear layer staged once for foley_op_gemm with K zero-padded to the K-slice granule and N to 32 rows (the tiny test
    configurations have 32-wide stages and a 48-wide projection; the released sizes need no padding).  build() -> (weight
    [N, K...], bias [N] or None) on first use.  Returns (W [Np, Kp] compute dtype, b [Np] fp32, N)."""
    key = wkey + "#pad"
    if key not in E.mats:
        w, bias = build()
        w = w.detach().to(torch.float32).reshape(w.shape[0], -1).cpu()
        N, K = w.shape
        g = _granule(E)
        Kp, Np = -(-K // g) * g, -(-N // 32) * 32
        wp = torch.zeros(Np, Kp, dtype=torch.float32)
        wp[:N, :K] = w
        bp = torch.zeros(Np, dtype=torch.float32)
        if bias is not None:
            bp[:N] = bias.detach().to(torch.float32).reshape(-1).cpu()
        E.mat(key, wp)
        E.vec(key + ".b", bp)
        _meta(E)[key] = N
    return E.mats[key], E.vecs[key + ".b"], _meta(E)[key]


def _lin(E: "EH._Engine", a: Tensor, sd: SD, wkey, bkey: Optional[str] = None, act: Optional[str] = None, out_f32: bool = False,
         residual: Optional[Tensor] = None) -> Tensor:
    """a [M, K] (compute dtype) @ W^T + b on foley_op_gemm; act 'gelu_erf'; residual: x += ... in place (fp32 stream).  wkey: a
    key of sd, or a tuple of keys whose layers are fused row-wise into ONE matrix (q / k / v: one launch, one read of a)."""
    if isinstance(wkey, tuple):
        bkeys = tuple(k[:-len("weight")] + "bias" for k in wkey)
        W, b, N = _staged(E, "+".join(wkey), lambda: (torch.cat([sd[k].detach().float().cpu() for k in wkey]),
                                                      torch.cat([sd[k].detach().float().cpu() for k in bkeys]) if bkeys[0] in sd else None))
    else:
        W, b, N = _staged(E, wkey, lambda: (sd[wkey], sd[bkey] if bkey else None))
    Np, Kp = W.shape
    if a.shape[1] != Kp:
        a = torch.nn.functional.pad(a, (0, Kp - a.shape[1]))
    a = a.contiguous()
    if residual is not None:
        if Np != N:
            raise rt.FoleyRuntimeError("a residual layer's width must be a multiple of 32")
        rt.op_gemm(a, W, b, out0=residual, epilogue=rt.EPI_GATE_RES, rb=rt.rowbcast(E.one(Np), 0), ksplit=1)
        return residual
    out = torch.empty(a.shape[0], Np, device=E.dev, dtype=torch.float32 if out_f32 else E.dtype)
    if out_f32:
        rt.op_gemm(a, W, b, out0=out)
    elif act:
        rt.op_gemm(a, W, b, out0=out, epilogue=rt.EPI_GELU_T, gelu_erf=(act == "gelu_erf"))
    else:
        rt.op_gemm(a, W, b, out0=out, epilogue=rt.EPI_STORE_T)
    return out if Np == N else out[:, :N].contiguous()


def _gather_rows(src: Tensor, idx: Tensor, groups: int, out: Tensor) -> None:
    """foley_op_gather_rows without runtime.op_gather_rows' per-call read-back of the table: `idx` was validated when it was built."""
    lib = rt.load_library()
    rt._check(lib, lib.foley_op_gather_rows(rt._ptr(src), rt._ptr(idx), idx.numel(), groups, src.shape[0] // groups, src.shape[1],
                                            rt._ptr(out), rt._stream()), "foley_op_gather_rows")


def _checked_index(E: "EH._Engine", key, build, rows: int) -> Tensor:
    """E.index with the table's values validated ONCE, before it is cached: every entry a row of the matrix it will address."""
    def checked():
        t = build()
        if t.numel() == 0 or int(t.min()) < 0 or int(t.max()) >= rows:
            raise rt.FoleyRuntimeError(f"index table {key} leaves [0, {rows})")
        return t
    return E.index(key, checked)


def _rel_bias(E: "EH._Engine", sd: SD, p: str, heads: int) -> Tensor:
    """[H, 64, 64] fp32: relative_position_bias_table gathered through relative_position_index, once per block."""
    key = p + "relative_position_bias#"
    t = E.vecs.get(key)
    if t is None:
        table = sd[p + "relative_position_bias_table"].detach().to(torch.float32).cpu()
        idx = sd.get(p + "relative_position_index")
        if idx is None:
            c = torch.stack(torch.meshgrid(torch.arange(WINDOW), torch.arange(WINDOW), indexing="ij")).flatten(1)
            rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (WINDOW - 1)
            idx = rel[..., 0] * (2 * WINDOW - 1) + rel[..., 1]
        idx = idx.detach().cpu().long().reshape(-1)
        if table.shape != ((2 * WINDOW - 1) ** 2, heads) or idx.numel() != WIN_TOKENS * WIN_TOKENS or int(idx.min()) < 0 or \
                int(idx.max()) >= table.shape[0]:
            raise rt.FoleyRuntimeError("relative position bias: the engine serves 8 x 8 windows")
        t = E.vecs[key] = table[idx].view(WIN_TOKENS, WIN_TOKENS, heads).permute(2, 0, 1).contiguous().to(E.dev)
    return t


def check_audio_config(cfg: dict) -> dict:
    """The numbers of a ClapAudioConfig the engine needs, refused where the kernels do not serve them."""
    a = cfg["audio"]
    if a.get("enable_fusion", False):
        raise rt.FoleyRuntimeError("the CLAP score serves the non-fusion audio tower (enable_fusion False); this checkpoint is a fusion model")
    ps, st = a.get("patch_size", 4), a.get("patch_stride", [4, 4])
    st = [st, st] if isinstance(st, int) else list(st)
    if ps != 4 or st != [4, 4]:
        raise rt.FoleyRuntimeError("the CLAP score serves 4x4 patches at stride 4")
    if a.get("window_size", 8) != WINDOW:
        raise rt.FoleyRuntimeError("the CLAP score serves 8 x 8 (64-token) attention windows")
    spec, mels = int(a.get("spec_size", 256)), int(a.get("num_mel_bins", 64))
    if mels != N_MELS or spec % mels:
        raise rt.FoleyRuntimeError("the CLAP score serves 64 mel bins and a spec_size that is a multiple of them")
    depths, heads, c0 = list(a["depths"]), list(a["num_attention_heads"]), int(a["patch_embeds_hidden_size"])
    if len(depths) != len(heads):
        raise rt.FoleyRuntimeError("depths and num_attention_heads must have one entry per stage")
    grid = spec // 4
    for i, (d, h) in enumerate(zip(depths, heads)):
        if (c0 << i) != h * HEAD_DIM:
            raise rt.FoleyRuntimeError(f"stage {i}: the windowed attention serves head dim 32 (width {c0 << i}, {h} heads)")
        if (grid >> i) % WINDOW or (grid >> i) < WINDOW:
            raise rt.FoleyRuntimeError(f"stage {i}: a {grid >> i}-token grid side is not a multiple of the window (the tower's padding path is not built)")
    if a.get("hidden_act", "gelu") != "gelu":
        raise rt.FoleyRuntimeError("the CLAP score serves the exact-GELU MLP (hidden_act 'gelu')")
    if a.get("projection_hidden_act", "relu") != "relu" or cfg.get("text", {}).get("projection_hidden_act", "relu") != "relu":
        raise rt.FoleyRuntimeError("the CLAP score serves ReLU projection heads")
    return {"spec": spec, "ratio": spec // mels, "depths": depths, "heads": heads, "c0": c0, "eps": float(a.get("layer_norm_eps", 1e-5)),
            "patch_norm": bool(a.get("enable_patch_layer_norm", True))}


# ----------------------------------------------------------------------------- the towers on the engine
def audio_embeds_hip(sd: SD, cfg: dict, wave48: Tensor, E: "EH._Engine", tables: Dict[str, Tensor],
                     starts: Optional[Sequence[int]] = None) -> Tensor:
    """48 kHz waveform [B, N] fp32 on the GPU -> L2-normalised audio embeddings [B, W, P] fp32 of its ten-second windows
    (`starts`, default clap_windows(N)): ClapFeatureExtractor -> ClapAudioEncoder.forward -> audio_projection -> F.normalize."""
    c = check_audio_config(cfg)
    B, N = wave48.shape
    starts = list(clap_windows(N) if starts is None else starts)
    W = len(starts)
    G = B * W
    p = AUDIO_PREFIX
    f64 = lambda k: sd[k].detach().to(torch.float64).cpu()
    spec = rt.op_melspec_db(wave48.contiguous(), torch.tensor(starts, dtype=torch.int32, device=E.dev),
                            tables["basis"], tables["mel_lo"], tables["mel_len"], tables["mel_w"])          # [G, 1001, 64]
    # BatchNorm2d(num_mel_bins) in eval mode: one affine per mel bin, folded in float64
    if p + "batch_norm#scale" not in E.vecs:
        sc = f64(p + "batch_norm.weight") / torch.sqrt(f64(p + "batch_norm.running_var") + BN_EPS)
        E.vec(p + "batch_norm#scale", sc.to(torch.float32))
        E.vec(p + "batch_norm#shift", (f64(p + "batch_norm.bias") - f64(p + "batch_norm.running_mean") * sc).to(torch.float32))
    S, ratio = c["spec"], c["ratio"]
    t_out = S * ratio
    if N_FRAMES > t_out:
        raise rt.FoleyRuntimeError("the spectrogram is longer than the tower's image (spec_size * freq_ratio)")
    ridx = rw = None
    if N_FRAMES != t_out:
        if ("resize", t_out) not in _meta(E):
            idx, w = cubic_resize_table(N_FRAMES, t_out, torch.float32)
            _meta(E)[("resize", t_out)] = (idx.to(E.dev, torch.int32).contiguous(), w.to(torch.float32).to(E.dev).contiguous())
        ridx, rw = _meta(E)[("resize", t_out)]
    patches = rt.op_spec_patches(spec, E.vecs[p + "batch_norm#scale"], E.vecs[p + "batch_norm#shift"], ridx, rw, S, ratio, E.dtype,
                                 _granule(E))
    x = _lin(E, patches, sd, p + "patch_embed.proj.weight", p + "patch_embed.proj.bias", out_f32=True)        # [G * gh * gw, C0]
    if c["patch_norm"]:
        x = E.ln(x, sd, p + "patch_embed.norm", 1e-5, out_dtype=torch.float32)
    h = w = S // 4
    C = c["c0"]
    n_stage = len(c["depths"])
    for i in range(n_stage):
        heads = c["heads"][i]
        rows = G * h * w
        for jb in range(c["depths"][i]):
            l = f"{p}layers.{i}.blocks.{jb}."
            shift = 0 if (jb % 2 == 0 or min(h, w) <= WINDOW) else WINDOW // 2       # set_shift_and_window_size
            key = ("clap-win", G, h, w, shift)
            table = _checked_index(E, key, lambda: window_tables(G, h, w, shift)[0], rows)
            mask = None
            if shift:                                  # the mask is one image's: it does not depend on the batch
                mkey = f"clap-mask#{h}x{w}/{shift}"
                mask = E.vecs.get(mkey)
                if mask is None:
                    mask = E.vecs[mkey] = window_tables(1, h, w, shift)[1].to(E.dev)
            a_ = l + "attention.self."
            qkv = _lin(E, E.ln(x, sd, l + "layernorm_before", c["eps"]), sd, tuple(a_ + n + ".weight" for n in ("query", "key", "value")))
            g = _granule(E)
            Cp = -(-C // g) * g
            att = torch.empty(rows, C, device=E.dev, dtype=E.dtype) if Cp == C else torch.zeros(rows, Cp, device=E.dev, dtype=E.dtype)
            rt.op_window_attention(qkv, heads, table, _rel_bias(E, sd, a_, heads), mask, out=att)
            _lin(E, att, sd, l + "attention.output.dense.weight", l + "attention.output.dense.bias", residual=x)
            hid = _lin(E, E.ln(x, sd, l + "layernorm_after", c["eps"]), sd, l + "intermediate.dense.weight", l + "intermediate.dense.bias",
                       act="gelu_erf")
            _lin(E, hid, sd, l + "output.dense.weight", l + "output.dense.bias", residual=x)
        if i < n_stage - 1:                                                      # ClapAudioPatchMerging
            d = f"{p}layers.{i}.downsample."
            idx = _checked_index(E, ("clap-merge", h, w), lambda: merge_table(h, w), h * w)
            merged = torch.empty(rows, C, device=E.dev, dtype=torch.float32)
            _gather_rows(x, idx, G, merged)
            y = E.ln(merged.view(rows // 4, 4 * C), sd, d + "norm", 1e-5)
            x = _lin(E, y, sd, d + "reduction.weight", None, out_f32=True)
            h, w, C = h // 2, w // 2, 2 * C
    hs = E.ln(x, sd, p + "norm", 1e-5, out_dtype=torch.float32)
    # ClapAudioEncoder.forward reshapes the tokens to [C, freq, time], regroups the frequency axis and feeds
    # AdaptiveAvgPool1d(1) the flattened result: every token of a channel enters the average once - the mean over all tokens
    pooled = hs.view(G, h * w, C).mean(dim=1)
    a1 = torch.relu(_lin(E, pooled.to(E.dtype), sd, "audio_projection.linear1.weight", "audio_projection.linear1.bias", out_f32=True))
    a2 = _lin(E, a1.to(E.dtype), sd, "audio_projection.linear2.weight", "audio_projection.linear2.bias", out_f32=True)
    return torch.nn.functional.normalize(a2, dim=-1).view(B, W, -1)


def text_embeds_hip(sd: SD, cfg: dict, input_ids: Tensor, attention_mask: Tensor, E: "EH._Engine") -> Tensor:
    """ClapModel.get_text_features: the text tower's hidden states (clap_text_hidden_hip) -> pooler (dense + tanh on token 0) ->
    text_projection -> F.normalize.  input_ids / attention_mask [n, T] on the GPU -> [n, P] fp32."""
    t = cfg.get("text", {})
    hidden = EH.clap_text_hidden_hip(sd, input_ids, attention_mask, E.dtype, heads=int(t.get("num_attention_heads", 12)),
                                     eps=float(t.get("layer_norm_eps", 1e-12)), pad_id=int(t.get("pad_token_id", 1)))
    first = hidden[:, 0].to(E.dtype).contiguous()
    pooled = torch.tanh(_lin(E, first, sd, "text_model.pooler.dense.weight", "text_model.pooler.dense.bias", out_f32=True))
    t1 = torch.relu(_lin(E, pooled.to(E.dtype), sd, "text_projection.linear1.weight", "text_projection.linear1.bias", out_f32=True))
    t2 = _lin(E, t1.to(E.dtype), sd, "text_projection.linear2.weight", "text_projection.linear2.bias", out_f32=True)
    return torch.nn.functional.normalize(t2, dim=-1)


# ----------------------------------------------------------------------------- public API
@dataclass
class ClapResult:
    """score [B]: the mean over a clip's windows of cos(audio embedding, text embedding); window_score [B, W]; audio_embeds
    [B, W, P] and text_embeds [B, P] L2-normalised fp32; order: batch indices by DESCENDING score (ties: the lower index);
    starts: first 48 kHz sample of every window."""
    score: Tensor
    window_score: Tensor
    audio_embeds: Tensor
    text_embeds: Tensor
    order: List[int]
    starts: List[int]


def config_dict(model_config, extractor=None) -> dict:
    """The plain numbers the scorer keeps of a transformers ClapConfig (and ClapFeatureExtractor)."""
    a, t = model_config.audio_config, model_config.text_config
    keys = ("enable_fusion", "patch_size", "patch_stride", "window_size", "spec_size", "num_mel_bins", "depths", "num_attention_heads",
            "patch_embeds_hidden_size", "layer_norm_eps", "enable_patch_layer_norm", "qkv_bias", "projection_hidden_act", "hidden_act",
            "mlp_ratio")
    cfg = {"audio": {k: getattr(a, k) for k in keys if hasattr(a, k)},
           "text": {k: getattr(t, k) for k in ("num_attention_heads", "layer_norm_eps", "pad_token_id", "projection_hidden_act") if hasattr(t, k)}}
    if extractor is not None:
        cfg["extractor"] = {k: getattr(extractor, k) for k in EXTRACTOR_KEYS}
    return cfg


def _clap_state(deps, device) -> Tuple[SD, dict]:
    """(state dict on the device in fp32, config dict): deps['clap_score_model'] preset to (state_dict, config_dict) - e.g.
    synthesised weights - or ClapModel / ClapFeatureExtractor loaded once from nodes.CLAP_REPO.  Kept: the audio tower, the text
    tower, the two projections and the extractor's numbers."""
    entry = deps.get("clap_score_model")
    if entry is None:
        from transformers import ClapFeatureExtractor, ClapModel
        from ..nodes import CLAP_REPO
        model = ClapModel.from_pretrained(CLAP_REPO).eval()
        entry = (model.state_dict(), config_dict(model.config, ClapFeatureExtractor.from_pretrained(CLAP_REPO)))
    sd, cfg = entry
    keep = ("audio_model.", "audio_projection.", "text_model.", "text_projection.")
    if any(not k.startswith(keep) for k in sd) or any(v.device != torch.device(device) for v in sd.values()):
        sd = {k: (v.detach().to(device, torch.float32) if v.is_floating_point() else v.detach().to(device))
              for k, v in sd.items() if k.startswith(keep)}
    ex = extractor_numbers(cfg)
    if int(ex["sampling_rate"]) != SR_CLAP or int(ex["hop_length"]) != HOP or int(ex["fft_window_size"]) != N_FFT or \
            int(ex["feature_size"]) != N_MELS or int(ex["max_length_s"]) != 10:
        raise rt.FoleyRuntimeError("the CLAP score serves the 48 kHz extractor (n_fft 1024, hop 480, 64 mel bins, 10 s windows)")
    check_audio_config(cfg)
    deps["clap_score_model"] = (sd, cfg)
    return sd, cfg


EXTRACTOR_KEYS = ("frequency_min", "frequency_max", "sampling_rate", "hop_length", "fft_window_size", "feature_size", "max_length_s")


def extractor_numbers(cfg: dict) -> dict:
    """The extractor's numbers of a config dict; none of them has a default here - they come from the checkpoint's extractor."""
    ex = cfg.get("extractor")
    missing = [k for k in EXTRACTOR_KEYS if ex is None or k not in ex]
    if missing:
        raise rt.FoleyRuntimeError(f"the CLAP score's config carries no extractor numbers ({', '.join(missing)}): build it with "
                                   "clap_score.config_dict(model.config, ClapFeatureExtractor)")
    return ex


def _tables(deps, device, cfg: dict) -> Dict[str, Tensor]:
    ex = extractor_numbers(cfg)
    fmin, fmax = float(ex["frequency_min"]), float(ex["frequency_max"])
    key = ("clap_score_tables", str(device), fmin, fmax)
    t = deps.get(key)
    if t is None:
        t = deps[key] = melspec_tables(device, fmin, fmax)
    return t


def prepare_waveform(deps, waveform: Tensor, sample_rate: int) -> Tensor:
    """[B, C, N] or [B, N] on the GPU -> mono [B, N48] fp32 at 48 kHz: the mean over channels, then foley_op_resample_sinc."""
    if waveform.dim() not in (2, 3):
        raise ValueError("waveform must be [B, C, N] or [B, N]")
    if not waveform.is_cuda:
        raise rt.FoleyRuntimeError("the CLAP score runs on the HIP engine: the waveform must be on the GPU")
    wav = waveform.to(torch.float32)
    wav = (wav.mean(dim=1) if wav.dim() == 3 else wav).contiguous()
    if int(sample_rate) != SR_CLAP:
        from .sync_score import sinc_resample_taps
        key = ("clap_score_taps", int(sample_rate), str(wav.device))
        if key not in deps:
            taps, o, n, width = sinc_resample_taps(int(sample_rate), SR_CLAP)
            deps[key] = (taps.to(wav.device), o, n, width)
        taps, o, n, width = deps[key]
        wav = rt.op_resample_sinc(wav, o, n, taps, width)
    return wav


@torch.inference_mode()
def clap_scores(deps, waveform: Tensor, sample_rate: int, prompts: Union[str, Sequence[str]], dtype: torch.dtype = torch.float16) -> ClapResult:
    """Score how well each clip of an AUDIO batch matches its prompt.

    waveform [B, C, N] or [B, N] (the sampler's AUDIO tensor) at any sample rate (resampled to 48 kHz on the device); prompts: one
    string for the whole batch or one per clip, tokenised by deps['clap_tokenizer'].  dtype: GEMM / attention operands -
    float16 (default), bfloat16, or float32 the parity mode.  Clips longer than ten seconds are scored window by window at FIXED
    positions (see the module docstring - the extractor would crop at random); shorter ones are repeat-padded like the extractor."""
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError("dtype must be float16, bfloat16 or float32")
    wav = prepare_waveform(deps, waveform, sample_rate)
    B = wav.shape[0]
    plist = [prompts] if isinstance(prompts, str) else list(prompts)
    if len(plist) not in (1, B):
        raise ValueError("prompts must be one string or one per clip")
    starts = clap_windows(wav.shape[1])                        # raises below one FFT frame before any tower work
    device = wav.device
    sd, cfg = _clap_state(deps, device)
    tok = deps.get("clap_tokenizer")
    if tok is None:
        from transformers import AutoTokenizer
        from ..nodes import CLAP_REPO
        tok = deps["clap_tokenizer"] = AutoTokenizer.from_pretrained(CLAP_REPO)
    E = EH._engine_for(sd, device, dtype)
    audio = audio_embeds_hip(sd, cfg, wav, E, _tables(deps, device, cfg), starts)
    inputs = tok(plist, padding=True, return_tensors="pt").to(device)
    text = text_embeds_hip(sd, cfg, inputs["input_ids"], inputs["attention_mask"], E)
    return summarize(audio, text if len(plist) == B else text.expand(B, -1), starts)


def summarize(audio_embeds: Tensor, text_embeds: Tensor, starts: Sequence[int]) -> ClapResult:
    """ClapResult of audio embeddings [B, W, P] and text embeddings [B, P] (both L2-normalised)."""
    return summarize_scores((audio_embeds * text_embeds[:, None, :]).sum(dim=-1), audio_embeds, text_embeds, starts)


def summarize_scores(window_score: Tensor, audio_embeds: Tensor, text_embeds: Tensor, starts: Sequence[int]) -> ClapResult:
    """ClapResult of per-window cosines [B, W]: the clip's score is their mean, the order descends by it."""
    score = window_score.mean(dim=1)
    s = score.tolist()
    order = sorted(range(len(s)), key=lambda i: (-s[i], i))
    return ClapResult(score=score, window_score=window_score, audio_embeds=audio_embeds, text_embeds=text_embeds, order=order,
                      starts=list(starts))


def best_matching(audio_batch: dict, result: ClapResult) -> dict:
    """The AUDIO dict of the clip that matches its prompt best (result.order[0])."""
    wf = audio_batch["waveform"]
    i = result.order[0]
    if not 0 <= i < wf.shape[0] or len(result.order) != wf.shape[0]:
        raise ValueError("the CLAP result does not belong to this audio batch")
    return {"waveform": wf[i].unsqueeze(0), "sample_rate": audio_batch["sample_rate"]}


def rank(sync=None, clap: Optional[ClapResult] = None, weights: Tuple[float, float] = (1.0, 1.0)) -> List[int]:
    """Batch indices, best first.  One result: its own order.  Both (a sync_score.SyncResult and a ClapResult of the same batch):
    ascending weights[0] * (rank by sync) + weights[1] * (rank by CLAP score), ranks counted from 0 along each result's order;
    ties go to the lower desync_s, then the lower index."""
    if sync is None and clap is None:
        raise ValueError("rank needs a SyncResult, a ClapResult or both")
    if clap is None:
        return list(sync.order)
    if sync is None:
        return list(clap.order)
    n = len(sync.order)
    if len(clap.order) != n or sorted(sync.order) != list(range(n)) or sorted(clap.order) != list(range(n)):
        raise ValueError("the two results do not rank the same batch")
    rs = {b: r for r, b in enumerate(sync.order)}
    rc = {b: r for r, b in enumerate(clap.order)}
    d = [float(v) for v in sync.desync_s.tolist()]
    return sorted(range(n), key=lambda i: (weights[0] * rs[i] + weights[1] * rc[i], d[i], i))
