"""References for the CLAP scorer's tests: the tiny `transformers` ClapModel, the test clips, CPU restatements of the front end and
the fp64 window-attention reference with its per-element bound."""
import math

import torch
import torch.nn.functional as F

from opcheck import U16, U32, Bound

TINY_AUDIO = dict(patch_embeds_hidden_size=32, depths=[2, 2, 2, 1], num_attention_heads=[1, 2, 4, 8], hidden_size=256,
                  enable_fusion=False)
FULL_AUDIO = dict(patch_embeds_hidden_size=128, depths=[2, 2, 12, 2], num_attention_heads=[4, 8, 16, 32], hidden_size=1024,
                  enable_fusion=False)
_CACHE = {}


def build_model(audio_kw=None, seed=0):
    """A ClapModel on the CPU in fp32 / eval: the given audio tower, a one-layer text tower (2 heads of 64), projection dim 48.
    After construction everything default initialisation leaves trivial is randomised - BatchNorm running statistics (mean about
    -20, variance about 100: the dB values span -100 .. +20), the relative-position bias tables (normal, std 0.5) and every
    LayerNorm / BatchNorm affine - otherwise the fold, the bias gather and the affines go untested."""
    from transformers import ClapConfig, ClapModel
    key = ("model", tuple(sorted((k, str(v)) for k, v in (audio_kw or TINY_AUDIO).items())), seed)
    if key in _CACHE:
        return _CACHE[key]
    torch.manual_seed(seed)
    cfg = ClapConfig(audio_config=dict(audio_kw or TINY_AUDIO),
                     text_config=dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=300,
                                      max_position_embeddings=90), projection_dim=48)
    model = ClapModel(cfg).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    rnd = lambda t, mean, std: t.copy_(mean + std * torch.randn(t.shape, generator=gen))
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                rnd(m.running_mean, -20.0, 3.0)
                m.running_var.copy_(100.0 * (0.5 + torch.rand(m.running_var.shape, generator=gen)))
                rnd(m.weight, 1.0, 0.1)
                rnd(m.bias, 0.0, 0.1)
            elif isinstance(m, torch.nn.LayerNorm):
                rnd(m.weight, 1.0, 0.1)
                rnd(m.bias, 0.0, 0.1)
            if hasattr(m, "relative_position_bias_table"):
                rnd(m.relative_position_bias_table, 0.0, 0.5)
    _CACHE[key] = model
    return model


def extractor(fmin=0.0, fmax=14000.0):
    from transformers import ClapFeatureExtractor
    return ClapFeatureExtractor(frequency_min=fmin, frequency_max=fmax, truncation="rand_trunc", padding="repeatpad")


class Tok:
    """Byte-level stand-in for the CLAP (Roberta) tokenizer: <s> bytes </s>, right-padded with <pad> = 1."""

    def __call__(self, texts, padding=True, return_tensors="pt"):
        ids = [[0] + [3 + (b % 250) for b in t.encode()][:75] + [2] for t in texts]
        n = max(len(i) for i in ids)
        batch = {"input_ids": torch.tensor([i + [1] * (n - len(i)) for i in ids]),
                 "attention_mask": torch.tensor([[1] * len(i) + [0] * (n - len(i)) for i in ids])}

        class B(dict):
            def to(self, dev):
                return B({k: v.to(dev) for k, v in self.items()})
        return B(batch)


def clip(seconds, seed=0, n=None):
    """Noise of amplitude 0.05 plus a chirp of amplitude 0.3 (200 Hz -> 9 kHz over the clip), fp32 [n] at 48 kHz."""
    n = int(seconds * 48000) if n is None else n
    gen = torch.Generator().manual_seed(100 + seed)
    t = torch.arange(n, dtype=torch.float64) / 48000.0
    dur = n / 48000.0
    f0, f1 = 200.0 + 150.0 * seed, 9000.0 - 900.0 * seed
    phase = 2 * math.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t)
    return (0.05 * torch.randn(n, generator=gen, dtype=torch.float64) + 0.3 * torch.sin(phase)).to(torch.float32)


def extractor_features(waves, ex=None):
    """The extractor's input_features for a list of <= 10 s fp32 clips: [B, 1, 1001, 64] fp32."""
    ex = ex or extractor()
    out = ex([w.numpy() for w in waves], sampling_rate=48000, return_tensors="pt")
    return out["input_features"].to(torch.float32)


def repeatpad(w):
    """_get_input_mel's padding of a clip of at most 480000 samples: int(480000 / n) copies, then zeros."""
    n = w.numel()
    return F.pad(w.repeat(480000 // n), (0, 480000 - (480000 // n) * n))


def melspec_fp32(wave480k, fb64):
    """The kernel's recipe restated with PyTorch in fp32: torch.stft (n_fft 1024, periodic Hann, hop 480, centred, reflect) ->
    power -> mel matmul -> 10 log10(max(., 1e-10)).  wave [B, 480000] fp32 -> [B, 1001, 64] fp32."""
    st = torch.stft(wave480k, 1024, hop_length=480, window=torch.hann_window(1024, periodic=True), center=True, pad_mode="reflect",
                    return_complex=True)
    power = st.real ** 2 + st.imag ** 2                          # [B, 513, 1001]
    mel = power.transpose(1, 2) @ fb64.to(torch.float32)
    return 10.0 * torch.log10(mel.clamp_min(1e-10))


def patches_ref(model, feats):
    """BatchNorm + reshape_mel2img + the patch embedding's unfold on the CPU: feats [G, 1, 1001, 64] -> [G * 4096, 16] fp32, token
    h * 64 + w, K in (kh, kw) order."""
    enc = model.audio_model.audio_encoder
    with torch.no_grad():
        x = enc.batch_norm(feats.transpose(1, 3)).transpose(1, 3)
        img = enc.reshape_mel2img(x)                             # [G, 1, 256, 256]
    cols = F.unfold(img, kernel_size=4, stride=4)                # [G, 16, 4096]
    return cols.transpose(1, 2).reshape(-1, 16)


def audio_embeds_ref(model, feats, dtype=torch.float32):
    """audio_model + audio_projection + normalisation of transformers on the CPU: feats [G, 1, 1001, 64] -> [G, P] fp32."""
    m = model if dtype == torch.float32 else _as_dtype(model, dtype)
    with torch.no_grad():
        pooled = m.audio_model(input_features=feats.to(dtype)).pooler_output
        return F.normalize(m.audio_projection(pooled).float(), dim=-1)


def text_embeds_ref(model, ids, mask):
    with torch.no_grad():
        return model.get_text_features(input_ids=ids, attention_mask=mask).pooler_output.float()


def _as_dtype(model, dtype):
    import copy
    key = ("cast", id(model), dtype)
    if key not in _CACHE:
        _CACHE[key] = copy.deepcopy(model).to(dtype)
    return _CACHE[key]


def scorer_deps(model, ex=None):
    """deps for clap_scores over a transformers model: (state dict, config dict) and the byte tokenizer."""
    from foley_amd.host import clap_score as CS
    return {"clap_score_model": (model.state_dict(), CS.config_dict(model.config, ex or extractor())), "clap_tokenizer": Tok()}


# ----------------------------------------------------------------------------- window attention
def window_attention_ref_and_bound(qkv, heads, table, bias, mask, dtype):
    """softmax(q k^T / sqrt(32) + bias + mask) v of foley_op_window_attention in fp64 from the operands as rounded to `dtype`
    (qkv [rows, 3 H 32], table [n_win, 64] int64 source rows, bias [H, 64, 64], mask [nW, 64, 64] or None; window g reads mask
    g % nW), scattered to out [rows, H 32], with a per-element bound built like opcheck.attention_ref_and_bound:

        e = (u_p + 2 d_s + (Skv + 8) U32) (P @ |V|)  (+ the output term of a 16-bit store)

    d_s   = (hd + 4) U32 max_keys(|q| . |k|) / sqrt(hd) + 4 U32 max_keys(|s| + |bias| + |mask|): hd fp32 products summed in any
            order and the scale; then the two fp32 additions (bias, mask) and the subtraction of the row maximum, each rounding a
            value no larger than |s| + |bias| + |mask| (the maximum is one of the row's scores: twice that for the difference).
            A score error d shifts exp by a factor e^d ~ 1 + d; it is felt once in the numerator and once in the row sum: 2 d_s.
    u_p   = the rounding of a probability to the operand type before the P V MFMA, relative to P: the WORST-CASE unit round-off
            of the type, 2 U16[dtype] = 2^-8 (bf16) / 2^-11 (fp16); fp32: U32.  opcheck's U16 is half of that on the argument that
            many rounded terms share a sum; a window's row can be carried by ONE probability (case (c): scores of +-60), and
            then that single rounding is the whole error.
    (Skv + 8) U32: with 64 keys the terms attention_ref_and_bound leaves out are cheap, so they are IN and the bound is rigorous
            to first order: the Skv fp32 additions of the P V product and of the row sum ((Skv + 4) U32 on sums of non-negative
            terms bounded by P @ |V|, resp. 1), the exponential itself (expf: 2 ulp, taken as 2 U32) and the final reciprocal
            and product (2 U32).
    Rows no window names are NaN in ref (the caller leaves them out)."""
    rows = qkv.shape[0]
    H, hd, S = heads, 32, 64
    x = qkv.double().cpu()
    q, k, v = (x[:, i * H * hd:(i + 1) * H * hd].view(rows, H, hd) for i in range(3))
    tab = table.long().cpu()
    b64 = bias.double().cpu()
    ref = torch.full((rows, H * hd), float("nan"), dtype=torch.float64)
    e = torch.zeros(rows, H * hd, dtype=torch.float64)
    u_p = 2 * U16[dtype] if dtype in U16 else U32
    for g in range(tab.shape[0]):
        r = tab[g]
        qg, kg, vg = (t[r].transpose(0, 1) for t in (q, k, v))           # [H, 64, hd]
        s = qg @ kg.transpose(1, 2) / math.sqrt(hd)
        m = mask[g % mask.shape[0]].double().cpu()[None] if mask is not None else torch.zeros(1, S, S, dtype=torch.float64)
        mag = (qg.abs() @ kg.abs().transpose(1, 2)) / math.sqrt(hd)
        d_s = ((hd + 4) * U32 * mag + 4 * U32 * (s.abs() + b64.abs() + m.abs())).amax(-1, keepdim=True)
        p = torch.softmax(s + b64 + m, -1)
        o = p @ vg
        eo = (u_p + 2 * d_s + (S + 8) * U32) * (p @ vg.abs())
        ref[r] = o.transpose(0, 1).reshape(S, H * hd)
        e[r] = eo.transpose(0, 1).reshape(S, H * hd)
    return ref, Bound(e, dtype)
