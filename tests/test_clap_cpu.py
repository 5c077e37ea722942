"""The CLAP scorer's host side without a GPU: every host-built table against the `transformers` code it restates, the window
positions, the pooling identity and the ranking helpers."""
import types

import pytest
import torch
import torch.nn.functional as F

import clap_ref as R
from foley_amd.host import clap_score as CS, runtime as rt
from foley_amd.host.sync_score import SyncResult
from opcheck import U32


@pytest.mark.parametrize("fmin,fmax", [(0.0, 14000.0), (50.0, 14000.0)])
def test_slaney_table_equals_the_extractor(fmin, fmax):
    ex = R.extractor(fmin, fmax)
    fb, lo, ln, w = CS.slaney_mel_tables(fmin, fmax)
    ref = torch.from_numpy(ex.mel_filters_slaney)
    assert fb.shape == ref.shape == (513, 64)
    assert float((fb - ref).abs().max()) <= 1e-14 * float(ref.abs().max())      # float64 both; numpy and torch differ in the last bits of log / exp
    # the kernel's form: one contiguous run of at most 32 bins per triangle, rebuilt exactly (to the fp32 rounding of the weights)
    assert int(ln.min()) >= 2 and int(ln.max()) <= CS.MEL_PITCH
    back = torch.zeros(513, 64)
    for c in range(64):
        back[int(lo[c]):int(lo[c]) + int(ln[c]), c] = w[c, :int(ln[c])]
    assert torch.equal(back, fb.to(torch.float32))


def test_cubic_table_equals_interpolate():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 1, 1001, 64, generator=gen, dtype=torch.float64) * 20 - 40
    idx, w = CS.cubic_resize_table(1001, 1024)
    got = (x[:, :, idx] * w[None, None, :, :, None]).sum(3)
    ref = F.interpolate(x, (1024, 64), mode="bicubic", align_corners=True)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) < 1e-11
    # in the type ATen resizes an fp32 spectrogram in: its fp32 result to the fp32 bound of a 4-tap sum, 8 U32 sum|w x|, plus
    # the rounding of the cubic coefficients themselves - polynomials with intermediate values up to 7.5 evaluated in fp32 on
    # either side (ATen's and the table's): 16 U32 ABSOLUTE per weight, so 16 U32 sum|x| (the table's weights were seen 4 U32 from
    # ATen's impulse response; a coordinate off by one fp32 ulp of 1000 would be 500 U32)
    idx32, w32 = CS.cubic_resize_table(1001, 1024, torch.float32)
    x32 = x.to(torch.float32)
    taps = x32.double()[:, :, idx32]
    got32 = (taps * w32.double()[None, None, :, :, None]).sum(3)
    mag = (taps.abs() * w32.double().abs()[None, None, :, :, None]).sum(3)
    ref32 = F.interpolate(x32, (1024, 64), mode="bicubic", align_corners=True).double()
    assert bool(((got32 - ref32).abs() <= 8 * U32 * mag + 16 * U32 * taps.abs().sum(3)).all())
    assert float((got - ref32).abs().max()) > 1e-4          # the exact table is NOT what the fp32 model computes (see cubic_resize_table)
    # equal lengths: the identity
    idx1, w1 = CS.cubic_resize_table(1024, 1024)
    assert torch.equal(idx1[:, 1], torch.arange(1024)) and torch.equal(w1, torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64).expand(1024, 4))


@pytest.mark.parametrize("h,w", [(16, 24), (64, 64), (8, 8)])
def test_window_tables_reproduce_roll_partition_and_mask(h, w):
    from transformers.models.clap.modeling_clap import ClapAudioLayer, window_partition
    B, shift = 3, 4
    rows = torch.arange(B * h * w, dtype=torch.float32).view(B, h, w, 1)
    for s in (0, shift):
        table, mask = CS.window_tables(B, h, w, s)
        rolled = torch.roll(rows, shifts=(-s, -s), dims=(1, 2)) if s else rows
        ref = window_partition(rolled, 8).view(-1, 64).long()
        assert table.dtype == torch.int32 and torch.equal(table.long(), ref)
        if s:
            layer = types.SimpleNamespace(shift_size=s, window_size=8)
            ref_mask = ClapAudioLayer.get_attn_mask(layer, h, w, torch.float32, torch.device("cpu"))
            assert mask.shape == ref_mask.shape == ((h // 8) * (w // 8), 64, 64) and torch.equal(mask, ref_mask)
        else:
            assert mask is None
    with pytest.raises(ValueError, match="multiple"):
        CS.window_tables(1, 12, 16, 0)


def test_merge_table_reproduces_the_concatenation():
    from transformers.models.clap.modeling_clap import ClapAudioPatchMerging
    h, w, C, B = 16, 24, 5, 2
    m = ClapAudioPatchMerging(C)
    m.norm, m.reduction = torch.nn.Identity(), torch.nn.Identity()
    x = torch.randn(B, h * w, C)
    ref = m(x, (h, w))                                         # [B, h/2 * w/2, 4C]
    idx = CS.merge_table(h, w).long()
    got = torch.stack([x[b][idx] for b in range(B)]).view(B, (h // 2) * (w // 2), 4 * C)
    assert torch.equal(got, ref)


def test_token_mean_equals_the_pooler_output():
    """ClapAudioEncoder.forward's reshape + regroup + AdaptiveAvgPool1d(1) is the mean over all tokens of the final LayerNorm."""
    model = R.build_model()
    enc = model.audio_model.audio_encoder
    seen = {}
    hook = enc.norm.register_forward_hook(lambda mod, inp, out: seen.__setitem__("tokens", out.detach()))
    feats = R.extractor_features([R.clip(3, 0)])
    with torch.no_grad():
        pooled = model.audio_model(input_features=feats).pooler_output
    hook.remove()
    assert seen["tokens"].shape == (1, 64, 256)
    assert torch.allclose(seen["tokens"].mean(1), pooled, rtol=0, atol=1e-6)


def test_clap_windows_and_fold():
    assert CS.clap_windows(1024) == [0]
    assert CS.clap_windows(240000) == [0]
    assert CS.clap_windows(480000) == [0]
    assert CS.clap_windows(480001) == [0, 1]
    assert CS.clap_windows(1_100_000) == [0, 480000, 1_100_000 - 480000]
    assert CS.clap_windows(960000) == [0, 480000]
    with pytest.raises(ValueError, match="FFT frame"):
        CS.clap_windows(1023)
    # the fold map against reshape_mel2img on a tensor that carries its own (time, frequency) index
    enc = R.build_model().audio_model.audio_encoder
    t = torch.arange(1024, dtype=torch.float32)[:, None] * 64 + torch.arange(64, dtype=torch.float32)[None, :]
    img = enc.reshape_mel2img(t[None, None])[0, 0]
    fold = CS.fold_index(256, 4, 64)
    assert img.shape == (256, 256) and torch.equal(img.long(), fold[..., 0] * 64 + fold[..., 1])


def _sync(desync, order):
    z = torch.zeros(len(order), 1, 21)
    return SyncResult(logits=z, probs=z, offset_s=z[..., 0], desync_s=torch.tensor(desync), order=order, starts=[0], grid=torch.zeros(21))


def _clap(scores):
    a = torch.zeros(len(scores), 1, 4)
    return CS.summarize_scores(torch.tensor(scores)[:, None], a, a[:, 0], [0])


def test_rank_and_best_matching():
    clap = _clap([0.1, 0.4, 0.3, 0.4])
    assert clap.order == [1, 3, 2, 0]                          # descending score, ties to the lower index
    assert CS.rank(clap=clap) == [1, 3, 2, 0]
    sync = _sync([0.2, 0.4, 0.0, 0.2], [2, 0, 3, 1])
    assert CS.rank(sync=sync) == [2, 0, 3, 1]
    # rank sums: clip0 1+3, clip1 3+0, clip2 0+2, clip3 2+1 -> 2 first (sum 2); 1 and 3 tie at 3: the lower desync_s (clip 3) first
    assert CS.rank(sync, clap) == [2, 3, 1, 0]
    assert CS.rank(sync, clap, weights=(0.0, 1.0)) == [1, 3, 2, 0]
    assert CS.rank(sync, clap, weights=(1.0, 0.0)) == [2, 0, 3, 1]
    with pytest.raises(ValueError):
        CS.rank()
    with pytest.raises(ValueError, match="same batch"):
        CS.rank(_sync([0.0, 0.2], [0, 1]), clap)
    batch = {"waveform": torch.arange(4.0)[:, None, None].expand(4, 1, 8), "sample_rate": 48000}
    assert torch.equal(CS.best_matching(batch, clap)["waveform"], batch["waveform"][1:2])
    with pytest.raises(ValueError, match="belong"):
        CS.best_matching({"waveform": torch.zeros(2, 1, 8), "sample_rate": 48000}, clap)


def test_unserved_configurations_are_refused():
    from transformers import ClapConfig
    ex = R.extractor()
    cfg = CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO, enable_fusion=True)), ex)
    with pytest.raises(rt.FoleyRuntimeError, match="fusion"):
        CS.check_audio_config(cfg)
    cfg = CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO, num_attention_heads=[2, 2, 4, 8])), ex)
    with pytest.raises(rt.FoleyRuntimeError, match="head dim 32"):
        CS.check_audio_config(cfg)
    cfg = CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO, depths=[2, 2, 2, 1, 1], num_attention_heads=[1, 2, 4, 8, 16])), ex)
    with pytest.raises(rt.FoleyRuntimeError, match="multiple of the window"):
        CS.check_audio_config(cfg)
    ok = CS.check_audio_config(CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO)), ex))
    assert ok["depths"] == [2, 2, 2, 1] and ok["ratio"] == 4 and ok["spec"] == 256
    with pytest.raises(rt.FoleyRuntimeError, match="GPU"):
        CS.clap_scores({}, torch.zeros(1, 1, 48000), 48000, "x")


def test_config_without_extractor_numbers_is_refused_and_widths_survive_the_index_cache():
    from transformers import ClapConfig
    from foley_amd.host import encoders_hip as EH
    cfg = CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO)))
    with pytest.raises(rt.FoleyRuntimeError, match="extractor numbers"):
        CS.extractor_numbers(cfg)
    with pytest.raises(rt.FoleyRuntimeError, match="frequency_max"):
        CS.extractor_numbers({"extractor": {k: 1 for k in CS.EXTRACTOR_KEYS if k != "frequency_max"}})
    cfg = CS.config_dict(ClapConfig(audio_config=dict(R.TINY_AUDIO, hidden_act="relu")), R.extractor())
    with pytest.raises(rt.FoleyRuntimeError, match="GELU"):
        CS.check_audio_config(cfg)
    # a staged layer's width must outlive any number of evictions of the engine's bounded index cache
    E = EH._Engine("cpu", torch.float32)
    W, b, N = CS._staged(E, "w", lambda: (torch.ones(48, 20), torch.ones(48)))
    assert (tuple(W.shape), tuple(b.shape), N) == ((64, 32), (64,), 48)
    for i in range(600):
        E.index(("filler", i), lambda: torch.zeros(1))
    assert len(E.tabs) <= 512
    assert CS._staged(E, "w", lambda: pytest.fail("staged twice"))[2] == 48

