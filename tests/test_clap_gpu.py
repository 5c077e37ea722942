"""The CLAP scorer on the GPU through the C ABI: the three new kernels per element, the audio tower against `transformers` on the
CPU (tiny and full architecture), the scores, long clips, batch invariance and a sampler run scored end to end."""
import math

import pytest
import torch

import clap_ref as R
from conftest import record_parity, rel_err
from foley_amd.host import clap_score as CS, encoders_hip as EH, runtime as rt
from opcheck import U32, assert_elementwise, guarded

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
GATE = {torch.float32: 1e-5, torch.float16: 5e-3}       # the gates test_sync_gpu.py holds the AST audio branch to (same engine, same layers)


# ----------------------------------------------------------------------------- window attention
def _wa_case(case, dtype):
    gen = torch.Generator().manual_seed({"a": 1, "b": 2, "c": 3}[case])
    if case == "b":                                  # one 8 x 8 grid, four heads, no mask: 4 (window, head) pairs
        B, h, w, H, shift = 1, 8, 8, 4, 0
    else:                                            # 3 images of a 16 x 24 grid, shift 4: 18 pairs (no multiple of the packing), 6 masks
        B, h, w, H, shift = 3, 16, 24, 1, 4
    rows = B * h * w
    qkv = torch.randn(rows, 3 * H * 32, generator=gen)
    table, mask = CS.window_tables(B, h, w, shift)
    if case == "c":                                  # scores up to +-60: a softmax without the maximum subtraction overflows / loses everything
        q, k = qkv[:, :32], qkv[:, 32:64]
        smax = max(float((q[r.long()] @ k[r.long()].t()).abs().max()) for r in table) / math.sqrt(32)
        qkv[:, :32] *= 60.0 / smax
    bias = 0.5 * torch.randn(H, 64, 64, generator=gen)
    return qkv.to(dtype), H, table, bias, mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_window_attention_op(dev, dtype, case):
    qkv, H, table, bias, mask = _wa_case(case, dtype)
    ref, bound = R.window_attention_ref_and_bound(qkv, H, table, bias, mask, dtype)
    assert not bool(torch.isnan(ref).any())          # every row belongs to exactly one window
    rows = qkv.shape[0]
    outs = []
    for _ in range(2):
        g = guarded((rows, H * 32), dtype, dev, pad_cols=8)
        rt.op_window_attention(qkv.to(dev), H, table.to(dev), bias.to(dev), mask.to(dev) if mask is not None else None, out=g.view)
        torch.cuda.synchronize()
        g.check(f"window attention {case} {dtype}")
        outs.append(g.view.clone())
    worst = assert_elementwise(outs[0], ref, bound, f"window attention {case} {dtype}")
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))      # two calls: the same bits
    record_parity(f"clap_window_attention_{case}_{str(dtype).split('.')[-1]}", worst_err_over_bound=worst)


def test_window_attention_refusals(dev):
    lib = rt.load_library()
    qkv = torch.zeros(64, 3 * 2 * 48, device=dev)
    table = torch.arange(64, dtype=torch.int32, device=dev).view(1, 64)
    bias = torch.zeros(2, 64, 64, device=dev)
    out = torch.zeros(64, 96, device=dev)
    call = lambda cols, H, tokens, tab: lib.foley_op_window_attention(
        qkv.data_ptr(), rt.DT_F32, 64, cols, H, tokens, tab.data_ptr(), tab.shape[0], bias.data_ptr(), None, 0, out.data_ptr(), 96, None)
    assert call(3 * 2 * 48, 2, 64, table) == -1                  # head dim 48: FOLEY_ERR_INVALID
    assert b"head dim 32" in lib.foley_last_error()
    assert call(3 * 2 * 32, 2, 16, table.view(4, 16)) == -1      # a 16-token window
    assert b"64-token" in lib.foley_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ----------------------------------------------------------------------------- front end
@pytest.fixture(scope="module")
def front():
    """Extractor features of the two front-end clips (4 s: repeated twice, then 2 s of zeros; 10 s) and the fp32 restatement."""
    ex = R.extractor()
    waves = [R.clip(4, 2), R.clip(10, 1)]
    feats = R.extractor_features(waves, ex)                       # [2, 1, 1001, 64]
    fb = CS.slaney_mel_tables(ex.frequency_min, ex.frequency_max)[0]
    restated = R.melspec_fp32(torch.stack([R.repeatpad(w) for w in waves]), fb)
    return ex, waves, feats, restated


def test_melspec_db_op(dev, front):
    """Absolute dB error against the extractor (float64 numpy).  The gate is 4 x the error of the SAME recipe restated in fp32 on
    the CPU (torch.stft + matmul): another summation order over 1024 taps and up to 32 bins moves that error by a small factor."""
    ex, waves, feats, restated = front
    tb = CS.melspec_tables(dev, ex.frequency_min, ex.frequency_max)
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    got = torch.cat([rt.op_melspec_db(w[None].to(dev), z, tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"]) for w in waves]).cpu()
    assert got.shape == (2, 1001, 64)
    d_ref = float((restated - feats[:, 0]).abs().max())
    d_got = float((got - feats[:, 0]).abs().max())
    print(f"dB-mel: fp32 CPU restatement {d_ref:.3e} dB, kernel {d_got:.3e} dB, gate {4 * d_ref:.3e}")
    record_parity("clap_melspec_db", restatement_db=d_ref, kernel_db=d_got, ratio=d_got / d_ref)
    # the 4 s clip: samples [384000, 480000) are zero, so the frames whose 1024 taps lie inside are silent: exactly -100
    silent = torch.arange(1001)[(torch.arange(1001) * 480 - 512 >= 384000) & (torch.arange(1001) * 480 + 512 <= 480000 - 512)]
    assert silent.numel() > 190 and bool((feats[0, 0, silent] == -100.0).all())
    assert bool((got[0, silent] == -100.0).all())
    assert d_got <= 4 * d_ref, (d_got, d_ref)
    # B = 2 in ONE call (the clip index of the kernel's grid): the same two signals at equal length - the 4 s clip as the extractor
    # pads it - against the extractor at the same gate
    pair = torch.stack([R.repeatpad(waves[0]), waves[1]])
    got_b = rt.op_melspec_db(pair.to(dev), z, tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"]).cpu()
    d_b = float((got_b - feats[:, 0]).abs().max())
    assert got_b.shape == (2, 1001, 64) and d_b <= 4 * d_ref, (d_b, d_ref)
    # clip index x window index: two windows (0 s and 5 s) of two 15 s clips in one call carry the bits of each crop run alone
    long = torch.stack([R.clip(15, 3), R.clip(15, 5)])
    starts = [0, 240000]
    got2 = rt.op_melspec_db(long.to(dev), torch.tensor(starts, dtype=torch.int32, device=dev), tb["basis"], tb["mel_lo"], tb["mel_len"],
                            tb["mel_w"])
    assert got2.shape == (4, 1001, 64)
    crops = [long[b, s:s + 480000].contiguous() for b in range(2) for s in starts]
    for i, c in enumerate(crops):
        alone = rt.op_melspec_db(c[None].to(dev), z, tb["basis"], tb["mel_lo"], tb["mel_len"], tb["mel_w"])
        assert torch.equal(got2[i], alone[0]), i
    # their distance from the extractor is recorded, not gated: the direct DFT rounds once per tap where the FFT of the restatement
    # rounds once per level, and next to a strong chirp that shows
    f2 = R.extractor_features(crops, ex)[:, 0]
    fb = CS.slaney_mel_tables(ex.frequency_min, ex.frequency_max)[0]
    d_ref2 = float((R.melspec_fp32(torch.stack(crops), fb) - f2).abs().max())
    d_got2 = float((got2.cpu() - f2).abs().max())
    print(f"dB-mel 15 s crops: restatement {d_ref2:.3e} dB, kernel {d_got2:.3e} dB")
    record_parity("clap_melspec_db_15s_crops", restatement_db=d_ref2, kernel_db=d_got2, ratio=d_got2 / d_ref2)


def test_spec_patches_op(dev, front):
    """BatchNorm + bicubic resize + reshape_mel2img + unfold of `transformers` on the CPU from the extractor's spectrogram.  Per
    element: both sides round an affine and a 4-tap sum in fp32, 8 U32 sum_j |w_j| (|x_j s| + |t|) each, and evaluate the cubic
    coefficients in fp32 (16 U32 absolute per weight, see test_cubic_table_equals_interpolate)."""
    _ex, _waves, feats, _ = front
    model = R.build_model()
    ref = R.patches_ref(model, feats)                              # [2 * 4096, 16]
    bn = model.audio_model.audio_encoder.batch_norm
    sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    sh = bn.bias.detach().double() - bn.running_mean.double() * sc
    idx, w = CS.cubic_resize_table(1001, 1024, torch.float32)
    taps = (feats[:, 0].double() * sc).abs()[:, idx] + sh.abs()    # [2, 1024, 4, 64]
    e = 16 * U32 * (taps * w.double().abs()[None, :, :, None]).sum(2) + 16 * U32 * taps.sum(2)
    e_img = e.view(2, 4, 256, 64).permute(0, 1, 3, 2).reshape(2, 1, 256, 256)
    e_cols = torch.nn.functional.unfold(e_img, 4, stride=4).transpose(1, 2).reshape(-1, 16)
    args = (sc.float().to(dev), sh.float().to(dev), idx.to(dev, torch.int32), w.to(dev), 256, 4)
    got = rt.op_spec_patches(feats[:, 0].contiguous().to(dev), *args, torch.float32, 32)
    assert got.shape == (2 * 4096, 32)
    assert float(got[:, 16:].abs().max()) == 0.0
    assert_elementwise(got[:, :16], ref, e_cols, "spec patches")
    for dt in (torch.float16, torch.bfloat16):
        g16 = rt.op_spec_patches(feats[:, 0].contiguous().to(dev), *args, dt, 64)
        assert g16.shape == (2 * 4096, 64) and torch.equal(g16[:, :16], got[:, :16].to(dt)) and float(g16[:, 16:].abs().max()) == 0.0
    # equal lengths: no resize table
    spec = torch.randn(1, 1024, 64)
    g0 = rt.op_spec_patches(spec.to(dev), args[0], args[1], None, None, 256, 4, torch.float32, 32)
    v = torch.addcmul(sh.float(), spec, sc.float())
    img = v.view(1, 4, 256, 64).permute(0, 1, 3, 2).reshape(1, 1, 256, 256)
    assert torch.allclose(g0[:, :16].cpu(), torch.nn.functional.unfold(img, 4, stride=4).transpose(1, 2).reshape(-1, 16), rtol=0, atol=4 * U32 * 8)


# ----------------------------------------------------------------------------- the tower
def _engine_embeds(model, waves, dev, dtype):
    ex = R.extractor()
    sd = {k: v.to(dev) for k, v in model.state_dict().items()}
    key = ("sd", id(model))
    sd = R._CACHE.setdefault(key, sd)
    cfg = CS.config_dict(model.config, ex)
    E = EH._engine_for(sd, dev, dtype)
    tb = R._CACHE.setdefault(("tables", str(dev)), CS.melspec_tables(dev, ex.frequency_min, ex.frequency_max))
    return torch.cat([CS.audio_embeds_hip(sd, cfg, w[None].to(dev), E, tb)[:, 0] for w in waves]).cpu()


@pytest.fixture(scope="module")
def tiny():
    model = R.build_model()
    waves = [R.clip(5, 0), R.clip(10, 1)]
    feats = R.extractor_features(waves)
    ref = R.audio_embeds_ref(model, feats)
    d0 = rel_err(R.audio_embeds_ref(model, feats, torch.bfloat16), ref)        # transformers' own bf16 CPU run against its fp32 run
    return model, waves, ref, d0


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_tower_against_transformers(dev, tiny, dtype):
    model, waves, ref, d0 = tiny
    got = _engine_embeds(model, waves, dev, dtype)
    err = rel_err(got, ref)
    gate = GATE.get(dtype, 1.5 * d0)
    print(f"tiny tower {dtype}: rel-L2 {err:.3e}, gate {gate:.3e} (bf16 d0 {d0:.3e})")
    record_parity(f"clap_tiny_tower_{str(dtype).split('.')[-1]}", err=err, gate=gate, d0=d0)
    assert got.shape == ref.shape == (2, 48)
    assert err < gate, (err, gate)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_full_architecture_once(dev, dtype):
    """patch_embeds_hidden_size 128, hidden 1024, depths 2 / 2 / 12 / 2 (the released HTSAT-base shape), synthesised weights."""
    model = R.build_model(R.FULL_AUDIO, seed=3)
    waves = [R.clip(7, 4)]
    key = ("full-ref",)
    if key not in R._CACHE:
        R._CACHE[key] = R.audio_embeds_ref(model, R.extractor_features(waves))
    ref = R._CACHE[key]
    got = _engine_embeds(model, waves, dev, dtype)
    err = rel_err(got, ref)
    print(f"full tower {dtype}: rel-L2 {err:.3e}")
    record_parity(f"clap_full_tower_{str(dtype).split('.')[-1]}", err=err, gate=GATE[dtype])
    assert err < GATE[dtype], err


# ----------------------------------------------------------------------------- scores
def _tone(f, a=0.5, n=480000):
    return (a * torch.sin(2 * math.pi * f * torch.arange(n, dtype=torch.float64) / 48000.0)).to(torch.float32)


@pytest.fixture(scope="module")
def scored():
    """A pool of ten-second clips with their reference embeddings and scores against one prompt, and the text references."""
    model = R.build_model()
    # tones over a noise floor of amplitude 0.005: a pure tone leaves most mel bins to the STFT's rounding noise (fp32 here, float64
    # in the extractor), which no fp32 front end reproduces
    tones = [_tone(440, 0.4) + _tone(1000, 0.4), _tone(440), _tone(3000), _tone(5000), _tone(1500) + _tone(60), _tone(1500)]
    pool = [t + 0.005 * torch.randn(t.numel(), generator=torch.Generator().manual_seed(i)) for i, t in enumerate(tones)]
    a_ref = R.audio_embeds_ref(model, R.extractor_features(pool))
    tok = R.Tok()(["rain on a tin roof"])
    t_ref = R.text_embeds_ref(model, tok["input_ids"], tok["attention_mask"])
    t_b16 = R.text_embeds_ref(R._as_dtype(model, torch.bfloat16), tok["input_ids"], tok["attention_mask"])
    a_b16 = R.audio_embeds_ref(model, R.extractor_features(pool), torch.bfloat16)
    d0 = {"audio": float((a_b16 - a_ref).norm(dim=-1).max()), "text": float((t_b16 - t_ref).norm(dim=-1).max())}
    return model, pool, a_ref, t_ref, (a_ref @ t_ref[0]), d0


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_against_transformers(dev, scored, dtype):
    """For unit vectors |cos(a, t) - cos(a', t')| <= ||a - a'|| + ||t - t'||: each score is held to tol = audio tolerance + text
    tolerance of its dtype (the tower gates; bf16: 1.5 x transformers' own bf16 distance), absolute, and both tolerances are
    asserted on the embeddings themselves, per vector.  The order of 4 clips equals the reference order; the clips are picked
    from the pool on the REFERENCE alone so that its scores are pairwise further apart than 4 tol.  bf16: 4 tol is 0.1, wider than
    any four scores of this tiny model lie apart (transformers' own bf16 run moves a score by 0.01), so no order is claimed for
    it: its scores are held to tol on the clips picked for fp16."""
    model, pool, a_ref, t_ref, s_ref, d0 = scored
    tol_a = GATE.get(dtype, 1.5 * d0["audio"])
    tol_t = GATE.get(dtype, 1.5 * d0["text"])
    tol = tol_a + tol_t
    ordered = dtype in GATE
    sep = 4 * tol if ordered else 8 * GATE[torch.float16]
    pick = []
    for i in sorted(range(len(pool)), key=lambda i: -float(s_ref[i])):
        if all(abs(float(s_ref[i] - s_ref[j])) > sep for j in pick):
            pick.append(i)
    pick = sorted(pick[:4])
    assert len(pick) == 4, f"the reference scores {s_ref.tolist()} hold no 4 clips further apart than {sep:.3e}"
    deps = R.scorer_deps(model)
    wav = torch.stack([pool[i] for i in pick])[:, None].to(dev)
    r = CS.clap_scores(deps, wav, 48000, "rain on a tin roof", dtype=dtype)
    assert r.score.shape == (4,) and r.window_score.shape == (4, 1) and r.audio_embeds.shape == (4, 1, 48) and r.starts == [0]
    e_a = float((r.audio_embeds[:, 0].cpu() - a_ref[pick]).norm(dim=-1).max())
    e_t = float((r.text_embeds.cpu() - t_ref).norm(dim=-1).max())
    e_s = float((r.score.cpu() - s_ref[pick]).abs().max())
    print(f"scores {dtype}: audio {e_a:.3e} (tol {tol_a:.3e}), text {e_t:.3e} (tol {tol_t:.3e}), score {e_s:.3e} (tol {tol:.3e})")
    record_parity(f"clap_scores_{str(dtype).split('.')[-1]}", audio=e_a, text=e_t, score=e_s, tol=tol)
    assert e_a < tol_a and e_t < tol_t
    assert e_s <= tol
    ref_order = sorted(range(4), key=lambda i: -float(s_ref[pick[i]]))
    if ordered:
        assert r.order == ref_order
        best = CS.best_matching({"waveform": wav, "sample_rate": 48000}, r)
        assert torch.equal(best["waveform"][0], wav[ref_order[0]])
    # one prompt per clip: the same prompt four times gives the same scores
    r4 = CS.clap_scores(deps, wav, 48000, ["rain on a tin roof"] * 4, dtype=dtype)
    assert float((r4.score - r.score).abs().max()) <= tol
    with pytest.raises(ValueError, match="one per clip"):
        CS.clap_scores(deps, wav, 48000, ["a", "b"], dtype=dtype)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float16, 2e-3)])
def test_long_clip_windows(dev, dtype, tol):
    """A 23 s clip gives 3 windows (0 s, 10 s and the last ten seconds); each window's score equals the score of that crop scored
    as a clip of its own, within the batch-invariance tolerance the sync scorer states (the GEMM tile choice depends on M)."""
    model = R.build_model()
    deps = R.scorer_deps(model)
    n = 23 * 48000
    long = R.clip(23, 6)
    r = CS.clap_scores(deps, long[None, None].to(dev), 48000, "a door slams", dtype=dtype)
    assert r.starts == [0, 480000, n - 480000] and r.window_score.shape == (1, 3)
    crops = torch.stack([long[s:s + 480000] for s in r.starts])
    rc = CS.clap_scores(deps, crops[:, None].to(dev), 48000, "a door slams", dtype=dtype)
    assert float((rc.score.cpu() - r.window_score[0].cpu()).abs().max()) < tol
    assert abs(float(r.score[0]) - float(r.window_score.mean())) < 1e-6
    with pytest.raises(ValueError, match="FFT frame"):
        CS.clap_scores(deps, torch.zeros(1, 1, 1000, device=dev), 48000, "x")


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float16, 2e-3)])
def test_batch_invariance_and_resampling(dev, dtype, tol):
    """A clip scored alone against position 3 of 6: equal within the stated tolerance, not bit for bit (tile choice depends on M).
    Stereo input is averaged, and a 44.1 kHz input goes through foley_op_resample_sinc to 48 kHz."""
    deps = R.scorer_deps(R.build_model())
    wav = torch.stack([R.clip(5, s) for s in range(6)])[:, None].to(dev)
    batch = CS.clap_scores(deps, wav, 48000, "footsteps on gravel", dtype=dtype)
    alone = CS.clap_scores(deps, wav[3:4], 48000, "footsteps on gravel", dtype=dtype)
    assert rel_err(alone.audio_embeds[0], batch.audio_embeds[3]) < tol
    assert abs(float(alone.score[0] - batch.score[3])) < tol
    stereo = torch.cat((wav[3:4] * 1.5, wav[3:4] * 0.5), dim=1)
    assert rel_err(CS.clap_scores(deps, stereo, 48000, "footsteps on gravel", dtype=dtype).audio_embeds, alone.audio_embeds) < tol
    if dtype == torch.float32:
        r44 = CS.clap_scores(deps, wav[:1, :, :44100 * 4].contiguous(), 44100, "footsteps on gravel", dtype=dtype)
        assert r44.audio_embeds.shape == (1, 1, 48) and bool(torch.isfinite(r44.score).all())


def test_sampler_output_ranked_end_to_end(dev):
    """A V2A run of the sampler node (tiny DiT, 5 s, batch 2, features injected), scored for sync and for prompt agreement, ranked
    by both."""
    from foley_amd import nodes
    from foley_amd.host import config as C, encoders as E, sampler, sync_score as S, synth
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    model = sampler.FoleyModel(c, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    deps = nodes.AttributeDict(dac_model=sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY))
    deps["sync_score_model"] = synth.materialize(E.synchformer_sync_schema())
    deps.update(R.scorer_deps(R.build_model()))
    cond = synth.synth_conditioning(c, 5.0, t2a=False, sd=sd)
    feats = {"siglip2_feat": cond["clip"], "syncformer_feat": synth.synth_tensor("e2e.syncformer_feat", (1, 112, 768), 1.0),
             "text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    _first, batch = nodes.HunyuanFoleySampler().generate_audio(
        model, deps, frame_rate=25, duration=5.0, prompt="x", negative_prompt="y", cfg_scale=4.5, steps=10, sampler="euler",
        batch_size=2, seed=3, force_offload=True, features=feats)
    wav = batch["waveform"].to(dev)
    clap = CS.clap_scores(deps, wav, batch["sample_rate"], "x")
    sync = S.sync_scores(deps, wav, batch["sample_rate"], syncformer_feat=feats["syncformer_feat"].to(dev))
    assert clap.score.shape == (2,) and clap.score.is_cuda and bool(torch.isfinite(clap.score).all())
    assert sorted(CS.rank(sync, clap)) == [0, 1] and sorted(CS.rank(clap=clap)) == [0, 1]
    assert CS.rank(sync, clap, weights=(0.0, 1.0)) == clap.order
