"""Sync scorer (host/sync_score.py), the parts that need no GPU: the host-built tables of the two audio kernels against their
definitions, the segment / window rules, the checkpoint filter, the C ABI surface, and a CPU emulation of foley_op_logmel's
arithmetic (tables + patch layout) against the golden g19 frozen from the reference."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from abi_pin import assert_abi_version
from conftest import ROOT, golden, rel_err
from foley_amd.host import encoders as E, runtime as rt, sync_score as S, synth
from opcheck import logmel_emulation as _logmel_emulation


def _resample_formula(x, orig=48000, new=16000):
    """torchaudio.functional.resample's default, restated (the pin: torchaudio is not installed): sinc_interp_hann,
    lowpass_filter_width 6, rolloff 0.99; kernel in float64, zero padding (width, width + orig), stride-orig conv1d."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = ((torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx) * base).clamp(-6, 6)
    k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), torch.sin(math.pi * t) / (math.pi * t)) \
        * torch.cos(math.pi * t / 12) ** 2 * base / orig
    y = F.conv1d(F.pad(x[:, None], (width, width + orig)), k.to(x.dtype), stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[..., :math.ceil(new * x.shape[-1] / orig)]


def _vfeat(g, sec):
    """The visual features of golden g19 (make_golden_sync.py does not store them: synth_tensor regenerates them bit for bit;
    the stored first 768 values check that it still does)."""
    v = synth.synth_tensor("g19.vfeat%d" % sec, (1, {5: 14, 8: 24}[sec] * 8, 768), 1.0)
    assert torch.equal(v.reshape(-1)[:768], g[f"vfeat_{sec}_head"])
    return v


def test_golden_visual_features_regenerate():
    g = golden("g19_sync")
    for sec in (5, 8):
        assert _vfeat(g, sec).shape == (1, {5: 14, 8: 24}[sec] * 8, 768)


def test_resample_taps_match_the_formula():
    taps, orig, new, width = S.sinc_resample_taps(48000, 16000)
    assert (orig, new, width) == (3, 1, 19) and taps.shape == (1, 41) and taps.dtype == torch.float32
    base = 0.99
    t = (torch.arange(-19, 22, dtype=torch.float64) / 3 * base).clamp(-6, 6)
    k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), torch.sin(math.pi * t) / (math.pi * t)) \
        * torch.cos(math.pi * t / 12) ** 2 * base / 3
    assert torch.allclose(taps[0].double(), k, rtol=0, atol=1e-7)
    # a general ratio: 44.1 kHz -> 16 kHz is 441 -> 160 polyphase
    taps2, o2, n2, w2 = S.sinc_resample_taps(44100, 16000)
    assert (o2, n2) == (441, 160) and taps2.shape == (160, 2 * w2 + 441)


def test_resample_restatement_matches_golden_head():
    g = golden("g19_sync")
    for sec in (5, 8):
        w48 = synth.synth_click_audio(2, sec * 48000, 48000)
        w16 = _resample_formula(w48)
        assert w16.shape == (2, sec * 16000)
        assert rel_err(w16[:, :4096], g[f"w16_{sec}_head"]) < 1e-6


def test_mel_table_matches_transformers_mel_filter_bank():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    ref = torch.from_numpy(audio_utils.mel_filter_bank(num_frequency_bins=513, num_mel_filters=128, min_frequency=0.0,
                                                       max_frequency=8000.0, sampling_rate=16000, norm=None, mel_scale="htk")).float()
    fb = S.htk_mel_filterbank()
    assert fb.shape == (513, 128)
    assert (fb - ref).abs().max() < 1e-6
    tb = S.logmel_tables("cpu")
    dense = torch.zeros(513, 128)
    for c in range(128):
        lo, n = int(tb["mel_lo"][c]), int(tb["mel_len"][c])
        assert 1 <= n <= S.MEL_PITCH and lo + n <= 513
        dense[lo:lo + n, c] = tb["mel_w"][c, :n]
    assert torch.equal(dense, fb)          # every triangle is one contiguous bin range


def test_logmel_tables_reproduce_the_reference_spectrogram():
    """The kernel's tables + arithmetic (CPU emulation) against the reference's normalised log-mel (g19: torch.stft +
    mel_filter_bank inside encode_audio_with_sync)."""
    g = golden("g19_sync")
    w16 = _resample_formula(synth.synth_click_audio(2, 5 * 48000, 48000))
    mel, patches = _logmel_emulation(w16)
    idx = g["mel_5_idx"].long()
    ref = g["mel_5"]
    got = mel.view(2, 14, 128, 66)[idx[:, 0], idx[:, 1]]
    assert rel_err(got, ref) < 1e-5
    assert torch.allclose(got[..., 65], torch.full_like(got[..., 65], 4.2677393 / (2 * 4.5689974)))
    # the im2col layout IS the AST patch embedding: Conv2d(1, D, 16, stride 10) over [F, T] (ASTPatchEmbeddings transposes
    # the (T, F) input first)
    w = torch.randn(8, 1, 16, 16, generator=torch.Generator().manual_seed(3))
    conv = F.conv2d(mel[:2, None], w, stride=10).flatten(2).transpose(1, 2)           # [2, 72, 8], token = fi*6 + ti
    gem = (patches[:144] @ w.reshape(8, 256).T).view(2, 72, 8)
    assert rel_err(gem, conv) < 1e-5


@pytest.mark.parametrize("seconds", [4.8, 4.9, 5.0, 5.12, 6.0, 8.0, 10.0, 15.5, 30.0])
def test_segment_and_window_counts(seconds):
    n16 = int(round(seconds * 16000))
    s_a = S.num_audio_segments(n16)
    assert s_a == (n16 - 10240) // 5120 + 1
    frames = int(seconds * 25)
    s_v = (frames - 16) // 8 + 1                                                       # encode_video_with_sync's segments
    assert S.resampled_length(int(round(seconds * 48000)), 48000) == n16
    st = S.window_starts(s_v, s_a)
    s = min(s_v, s_a)
    assert st[0] == 0 and st[-1] == s - 14 and len(st) == (1 if s == 14 else 2)
    strided = S.window_starts(s_v, s_a, window_stride=3)
    assert strided[0] == 0 and strided[-1] == s - 14 and all(0 < b - a <= 3 for a, b in zip(strided, strided[1:]))
    assert set(st) <= set(strided)


def test_window_edges():
    assert S.window_starts(14, 20) == [0]              # video shorter than audio: S = S_v
    assert S.window_starts(20, 14) == [0]
    assert S.window_starts(15, 40) == [0, 1]
    assert S.window_starts(40, 30, window_stride=8) == [0, 8, 16]
    with pytest.raises(ValueError, match="4.8 s"):
        S.window_starts(13, 30)
    with pytest.raises(ValueError, match="4.8 s"):
        S.window_starts(30, S.num_audio_segments(int(4.7 * 16000)))
    assert S.num_audio_segments(10239) == 0


def test_sync_state_filter():
    sched = E.synchformer_sync_schema()
    keys = list(sched)
    assert "afeat_extractor.ast.embeddings.position_embeddings" in sched
    assert sched["afeat_extractor.ast.embeddings.position_embeddings"][0] == (1, 74, 768)
    assert sched["transformer.pos_emb_cfg.pos_emb"][0] == (1, 198, 768)
    n_audio = sum(math.prod(sched[k][0]) for k in keys if k.startswith("afeat_extractor."))
    assert n_audio == 92400384
    sd = {k: torch.zeros(1) for k in keys}
    sd.update({k: torch.zeros(1) for k in list(E.synchformer_schema())[:5]})
    sd["afeat_extractor.step"] = torch.zeros(1, dtype=torch.long)           # non-float entries are dropped
    kept = E.load_synchformer_sync_state(sd, "cpu", torch.float32)
    assert set(kept) == set(keys)
    with pytest.raises(ValueError, match="audio branch and the sync head"):
        E.load_synchformer_sync_state({k: torch.zeros(1) for k in E.synchformer_schema()}, "cpu", torch.float32)


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    for name in ("foley_op_resample_sinc", "foley_op_logmel"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in rt.EXPORTED_SYMBOLS
        assert getattr(rt.load_library(), name) is not None
    assert "head_dim must be 128, 96 or 64" in open(os.path.join(ROOT, "comfyui-hunyuanvideo-foley_amd", "csrc", "attention.hip")).read()
    assert_abi_version()


def test_sync_scores_rejects_cpu_and_short_inputs():
    deps = {}
    with pytest.raises(rt.FoleyRuntimeError):
        S.sync_scores(deps, torch.zeros(1, 1, 48000 * 5), 48000, syncformer_feat=torch.zeros(1, 112, 768))


def test_summary_and_best_synced():
    logits = torch.full((3, 2, 21), -5.0)
    logits[0, :, 12] = 5.0          # +0.4 s
    logits[1, :, 10] = 5.0          # 0 s
    logits[2, 0, 10] = 5.0          # 0 s / -0.2 s
    logits[2, 1, 9] = 5.0
    r = S.summarize(logits, [0, 3])
    assert torch.allclose(r.offset_s, torch.tensor([[0.4, 0.4], [0.0, 0.0], [0.0, -0.2]]), atol=1e-6)
    assert r.order == [1, 2, 0]
    wf = torch.arange(3.0).view(3, 1, 1).expand(3, 1, 8).contiguous()
    best = S.best_synced({"waveform": wf, "sample_rate": 48000}, r)
    assert best["waveform"].shape == (1, 1, 8) and float(best["waveform"][0, 0, 0]) == 1.0
