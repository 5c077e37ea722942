"""Sync scorer on the GPU through the C ABI: the two audio kernels, attention at head_dim 96, the audio features and the sync
logits against the golden g19 frozen from the reference's Synchformer (tests/golden/make_golden_sync.py), batch invariance, and
a sampler run scored end to end."""
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, rel_err
from foley_amd.host import encoders as E, encoders_hip as EH, runtime as rt, sync_score as S, synth
from opcheck import logmel_emulation as _logmel_emulation
from test_sync_cpu import _resample_formula, _vfeat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sync_sd():
    return synth.materialize(E.synchformer_sync_schema())


def _deps(sd):
    return {"sync_score_model": sd}


def test_resample_sinc_op(dev):
    for sec in (5, 8):
        w48 = synth.synth_click_audio(2, sec * 48000 + 7, 48000)         # a length that is no multiple of 3
        taps, o, n, width = S.sinc_resample_taps(48000, 16000)
        got = rt.op_resample_sinc(w48.to(dev), o, n, taps.to(dev), width)
        ref = _resample_formula(w48)
        assert got.shape == ref.shape
        assert rel_err(got.cpu(), ref) < 1e-6


def test_logmel_op(dev):
    g = golden("g19_sync")
    w16 = _resample_formula(synth.synth_click_audio(2, 5 * 48000, 48000))
    tb = S.logmel_tables(dev)
    patches, mel = rt.op_logmel(w16.to(dev), tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"], torch.float32, with_mel=True)
    idx = g["mel_5_idx"].long()
    got = mel.cpu().view(2, 14, 128, 66)[idx[:, 0], idx[:, 1]]
    assert rel_err(got, g["mel_5"]) < 1e-5
    _mel_ref, patches_ref = _logmel_emulation(w16)
    assert patches.shape == (2 * 14 * 72, 256)
    assert rel_err(patches.cpu(), patches_ref) < 1e-5
    p16 = rt.op_logmel(w16.to(dev), tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"], torch.float16)
    assert torch.equal(p16, patches.to(torch.float16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("sq,skv", [(198, 198), (77, 150), (198, 33)])
def test_attention_head_dim_96(dev, dtype, sq, skv):
    gen = torch.Generator().manual_seed(sq * 7 + skv)
    G, H, hd = 3, 8, 96
    q, k, v = (torch.randn(G, H, s, hd, generator=gen) for s in (sq, skv, skv))
    ref = F.scaled_dot_product_attention(q.double(), k.double(), v.double()).transpose(1, 2).reshape(G, sq, H * hd)
    eng = EH._Engine(dev, dtype)
    out = eng.attention(q.to(dev, dtype), k.to(dev, dtype), v.to(dev, dtype))
    tol = 1e-5 if dtype == torch.float32 else (2e-3 if dtype == torch.float16 else 1e-2)
    assert rel_err(out.float().cpu(), ref.float()) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float16, 5e-3)])
def test_audio_features_against_golden(dev, sync_sd, dtype, tol):
    g = golden("g19_sync")
    sd = {k: v.to(dev) for k, v in sync_sd.items()}
    eng = EH._Engine(dev, dtype)
    tb = S.logmel_tables(dev)
    w16 = _resample_formula(synth.synth_click_audio(2, 5 * 48000, 48000)).to(dev)
    af = S.audio_features_hip(sd, w16, eng, tb)
    assert af.shape == (2, 14, 6, 768)
    assert rel_err(af.cpu()[:, g["afeat_5_idx"].long()], g["afeat_5_sel"]) < tol
    w16 = _resample_formula(synth.synth_click_audio(2, 8 * 48000, 48000)).to(dev)
    af8 = S.audio_features_hip(sd, w16, eng, tb)
    assert af8.shape == (2, 24, 6, 768)
    assert rel_err(af8.cpu()[:, g["afeat_8_idx"].long()], g["afeat_8_sel"]) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_sync_scores_against_golden(dev, sync_sd, dtype):
    g = golden("g19_sync")
    deps = _deps(sync_sd)
    for sec, stride in ((5, None), (8, 5)):
        wav = synth.synth_click_audio(2, sec * 48000, 48000).unsqueeze(1).to(dev)
        r = S.sync_scores(deps, wav, 48000, syncformer_feat=_vfeat(g, sec).to(dev), dtype=dtype, window_stride=stride)
        ref = g[f"logits_{sec}"]
        assert r.starts == g[f"starts_{sec}"].tolist()
        assert r.logits.shape == ref.shape
        err = rel_err(r.logits.cpu(), ref)
        assert err < (1e-5 if dtype == torch.float32 else 5e-3), err
        if dtype == torch.float32:
            assert torch.equal(r.logits.argmax(-1).cpu(), ref.argmax(-1))
        assert torch.allclose(r.probs.sum(-1), torch.ones_like(r.probs[..., 0]))
        assert r.desync_s.shape == (2,) and sorted(r.order) == [0, 1]


def test_sync_scores_batch_invariance(dev, sync_sd):
    """A clip scored alone and inside a batch of 6 gives the same logits within a stated tolerance, NOT bit for bit: the GEMM
    engine picks its tile by M (the rows of all clips), so a different batch sums the same products in another order.  Measured
    on the MI355X: 7e-4 absolute on logits of magnitude ~1 in fp16; the gate is 2e-3 relative, argmax identical."""
    g = golden("g19_sync")
    deps = _deps(sync_sd)
    wav = synth.synth_click_audio(6, 5 * 48000, 48000).to(dev)
    feat = _vfeat(g, 5).to(dev)
    for dtype, tol in ((torch.float16, 2e-3), (torch.float32, 1e-5)):
        batch = S.sync_scores(deps, wav, 48000, syncformer_feat=feat, dtype=dtype)
        alone = S.sync_scores(deps, wav[3:4], 48000, syncformer_feat=feat, dtype=dtype)
        assert batch.logits.shape == (6, 1, 21)
        assert rel_err(alone.logits[0].cpu(), batch.logits[3].cpu()) < tol
        assert torch.equal(alone.logits[0].argmax(-1), batch.logits[3].argmax(-1))


def test_sync_scores_input_checks(dev, sync_sd):
    deps = _deps(sync_sd)
    with pytest.raises(ValueError, match="4.8 s"):
        S.sync_scores(deps, torch.zeros(1, 1, int(4.7 * 48000), device=dev), 48000, syncformer_feat=torch.zeros(1, 112, 768, device=dev))
    w16 = _resample_formula(synth.synth_click_audio(1, 5 * 48000, 48000)).to(dev)
    w48 = synth.synth_click_audio(1, 5 * 48000, 48000).to(dev)
    feat = _vfeat(golden("g19_sync"), 5).to(dev)
    a = S.sync_scores(deps, w16, 16000, syncformer_feat=feat, dtype=torch.float32)
    b = S.sync_scores(deps, w48, 48000, syncformer_feat=feat, dtype=torch.float32)
    assert rel_err(a.logits.cpu(), b.logits.cpu()) < 1e-5


def test_sampler_output_scored_end_to_end(dev, sync_sd):
    """A V2A run of the sampler node (tiny DiT, 5 s, batch 2, 10 steps, features injected) and the scorer on its AUDIO output and
    its syncformer_feat: shapes, windows and order consistent; the scorer's own work stays on the device."""
    from foley_amd import nodes
    from foley_amd.host import config as C, sampler
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    model = sampler.FoleyModel(c, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    deps = nodes.AttributeDict(dac_model=sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY))
    deps["sync_score_model"] = sync_sd
    cond = synth.synth_conditioning(c, 5.0, t2a=False, sd=sd)
    sync_feat = synth.synth_tensor("e2e.syncformer_feat", (1, 112, 768), 1.0)
    feats = {"siglip2_feat": cond["clip"], "syncformer_feat": sync_feat, "text_feat": cond["text"],
             "uncond_text_feat": cond["uncond_text"]}
    _first, batch = nodes.HunyuanFoleySampler().generate_audio(
        model, deps, frame_rate=25, duration=5.0, prompt="x", negative_prompt="y", cfg_scale=4.5, steps=10, sampler="euler",
        batch_size=2, seed=3, force_offload=True, features=feats)
    wav = batch["waveform"]
    assert wav.shape == (2, 1, 5 * 48000)
    r = S.sync_scores(deps, wav.to(dev), batch["sample_rate"], syncformer_feat=feats["syncformer_feat"].to(dev))
    assert r.logits.shape == (2, 1, 21) and r.logits.is_cuda and r.starts == [0]
    assert sorted(r.order) == [0, 1]
    d = r.desync_s.tolist()
    assert d[r.order[0]] <= d[r.order[1]]
    best = S.best_synced(batch, r)
    assert torch.equal(best["waveform"][0], wav[r.order[0]])
