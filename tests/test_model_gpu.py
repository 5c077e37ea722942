"""End-to-end parity of the HIP path (through the C ABI) against golden vectors frozen from the
reference (tests/golden/*.npz) and against the CPU oracle: DiT forward, blocks at full width,
sampler loop with all solvers, DAC decoder, and the config-C1 gate at real xxl dimensions.
"""
import os

import pytest
import torch

from conftest import golden, record_parity, rel_err
from foley_amd.host import config as C, sampler, synth, tables
from loop_harness import tiny_run
from oracle import foley_oracle as O

pytestmark = pytest.mark.gpu


def _plan_single(model, text, clip, sync, La, t_values):
    """ncfg=1, clips=1 plan evaluating the model at explicit timesteps."""
    dev = model.device
    Lv, Ls, Lt = clip.shape[1], sync.shape[1], text.shape[1]
    n = len(t_values)
    tb = tables.build_tables(La, Lv, Ls, Lt, max(n, 1), "euler", 1.0, model.cfg.time_freq_dim)
    tb["t_feat"] = tables.timestep_features(torch.tensor(t_values, dtype=torch.float32), model.cfg.time_freq_dim)
    if sampler.fp8_time_dtype(model) is not None:
        tb["t_feat"] = tb["t_feat"].to(sampler.fp8_time_dtype(model)).float()
    plan = {"ncfg": 1, "clips": 1, "La": La, "Lv": Lv, "Ls": Ls, "Lt": Lt, "n_iter": n, "guidance": 1.0,
            "rope_len": tb["rope_cos"].shape[0], "text": text.float().to(dev).contiguous(),
            "clip": clip.float().to(dev).contiguous(), "sync": sync.float().to(dev).contiguous()}
    for k in ("t_feat", "rope_cos", "rope_sin", "pos_audio_self", "pos_visual_self", "pos_linear", "sync_gather",
              "solver_coef"):
        plan[k] = tb[k].to(dev).contiguous()
    return plan


def _forward(model, x, t, cond, clip, sync):
    """Reference-shaped forward: x [B,128,La] (per-sample conditioning) -> [B,128,La]."""
    outs = []
    for b in range(x.shape[0]):
        plan = _plan_single(model, cond[b:b + 1], clip[b:b + 1], sync[b:b + 1], x.shape[2], [float(t[b])])
        model.ctx.prepare(plan)
        rows = model.ctx.dit_forward(x[b:b + 1].to(model.device).contiguous(), 0)
        outs.append(rows.view(1, x.shape[2], -1).transpose(1, 2))
    return torch.cat(outs).cpu()


@pytest.fixture(scope="module")
def tiny(dev):
    return tiny_run(dev, 0)[:4]


def test_dit_forward_tiny_golden(tiny):
    """G5: tiny-config full forward, two length sets incl. non-multiple-of-32 token counts."""
    _sd, _dsd, model, _dac = tiny
    g = golden("g5_dit_tiny")
    for tag in ("a", "b"):
        y = _forward(model, g[tag + "_x"], g[tag + "_t"], g[tag + "_cond"], g[tag + "_clip"], g[tag + "_sync"])
        assert rel_err(y, g[tag + "_y"]) < 2e-5, tag


def test_blocks_full_width_golden(dev):
    """G4: one triple + one single block at D=1536 (exercises every production GEMM shape class)."""
    c = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1)
    model = sampler.FoleyModel(c, synth.synth_dit_state_dict(c, device=dev), torch.float32, dev)
    g = golden("g4_blocks")
    y = _forward(model, g["x"], g["t"], g["cond"], g["clip"], g["sync"])
    assert rel_err(y, g["y"]) < 2e-5


@pytest.mark.parametrize("tag,t2a,dur,guid,bs,solver,steps", [
    ("cfg_euler", False, 1.0, 4.5, 2, "euler", 10),
    ("t2a_nocfg", True, 1.0, 1.0, 1, "euler", 10),
    ("heun", False, 1.0, 4.5, 1, "heun-2", 10),
    ("midpoint", False, 1.0, 4.5, 1, "midpoint-2", 10),
    ("kutta", False, 1.0, 4.5, 1, "kutta-4", 12),
    ("v2a_2s", False, 2.0, 3.0, 2, "euler", 12)])
@pytest.mark.parametrize("use_graph", [False, True])
def test_sampler_golden(tiny, tag, t2a, dur, guid, bs, solver, steps, use_graph):
    """G7: whole loop + DAC vs the reference's denoise_process_with_generator (1e-3 gate)."""
    sd, _dsd, model, dac = tiny
    g = golden("g7_sampler")
    cond = synth.synth_conditioning(C.TINY, dur, t2a=t2a, sd=sd)
    audio, sr, lat = sampler.denoise_process_with_generator(
        {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]},
        {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]},
        dur, model, dac, guid, steps, bs, solver, noise=g[tag + "_noise"], use_graph=use_graph,
        return_latents=True)
    assert sr == 48000 and audio.shape == (bs, 1, int(dur * 50) * 960)
    assert rel_err(lat, g[tag + "_latents"]) < 1e-4
    assert rel_err(audio[..., ::5], g[tag + "_wave_s5"]) < 1e-3


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("bf16", 6e-2)])
def test_long_clip_matches_oracle(tiny, dev, precision, tol):
    """C5-shaped sequence lengths (30 s: La=1500, Lv=240, Ls=736; S=1740 joint tokens, several
    256/128-row tiles, ragged last tiles) with negative-prompt CFG, 3 Euler steps, against the
    oracle evaluated here on the same noise.  bf16: loose gate only (operand rounding)."""
    sd, _dsd, model32, _dac = tiny
    model = model32 if precision == "fp32" else sampler.FoleyModel(C.TINY, sd, torch.bfloat16, dev, dac_cfg=C.DAC_TINY)
    dur, steps, g = 30.0, 3, 4.5
    cond = synth.synth_conditioning(C.TINY, dur, t2a=False, sd=sd)
    noise = torch.randn(1, 128, int(dur * 50), generator=torch.Generator().manual_seed(30))
    plan = sampler.build_plan(model, {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]},
                              {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}, int(dur * 50), g,
                              steps, 1, "euler")
    model.ctx.prepare(plan)
    lat = noise.clone().to(dev)
    model.ctx.sample(lat, use_graph=True)
    with torch.inference_mode():
        ref = O.sample_latents(sd, C.TINY.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"],
                               steps, g, "euler")
    assert rel_err(lat, ref) < tol


@pytest.mark.parametrize("bs,solver,steps", [(6, "euler", 100), (2, "kutta-4", 10)])
def test_widget_extremes_match_oracle(tiny, dev, bs, solver, steps):
    """The sampler node's extremes on the tiny model (fp32 parity mode, gate of test_long_clip_matches_oracle): 60 s clips
    (S = 3480 joint tokens) with negative-prompt CFG 4.5 - six clips for 100 Euler steps (the top of both widgets: 100-entry
    timestep / solver tables, a 100-iteration graph) and two clips for 10 kutta-4 steps (the step widget's minimum, four model
    calls per step).  The oracle runs on each clip's own noise.  Its cost at 100 steps (0.5 s per CFG pair per step on 16 CPUs)
    bounds it to the first and the last clip of the six; the middle ones are held to the same run of each clip on its own
    (batch of one), which the first and last clip tie to the oracle."""
    sd, _dsd, model, _dac = tiny
    dur, g = 60.0, 4.5
    La = int(dur * 50)
    cond = synth.synth_conditioning(C.TINY, dur, t2a=False, sd=sd)
    noise = torch.randn(bs, 128, La, generator=torch.Generator().manual_seed(60))
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}

    def run(nz):
        model.ctx.prepare(sampler.build_plan(model, vis, txt, La, g, steps, nz.shape[0], solver))
        lat = nz.clone().to(dev).contiguous()
        model.ctx.sample(lat, use_graph=True)
        return lat.cpu()

    lat = run(noise)
    assert bool(torch.isfinite(lat).all())
    oracle_clips = [0, bs - 1]
    errs = {}
    with torch.inference_mode():
        ref = O.sample_latents(sd, C.TINY.heads, noise[oracle_clips], cond["text"], cond["uncond_text"], cond["clip"], cond["sync"],
                               steps, g, solver)
    for i, b in enumerate(oracle_clips):
        errs[b] = rel_err(lat[b], ref[i])
    for b in range(1, bs - 1):
        errs[b] = rel_err(lat[b], run(noise[b:b + 1])[0])
    record_parity("widget_extremes_tiny_%s_%d_steps_bs%d" % (solver, steps, bs), worst=max(errs.values()))
    print("tiny 60 s x %d, %s %d steps: %s" % (bs, solver, steps, " ".join("%.2e" % e for e in errs.values())))
    for b, e in errs.items():
        assert e < 2e-4, (b, e)


def test_sampler_noise_matches_reference_draw(tiny):
    """The CPU-generator draw (utils.py:114-121) must reproduce the committed golden noise."""
    g = golden("g7_sampler")
    gen = torch.Generator("cpu").manual_seed(1234)
    n = sampler.draw_noise(2, 128, 50, torch.float32, gen)
    assert torch.equal(n, g["cfg_euler_noise"])


def test_dac_golden_narrow(dev):
    """G3: rates (5, 2) decoder - odd stride exercises output_padding."""
    dc = C.DACConfig(decoder_dim=128, rates=(5, 2))
    dit = C.TINY
    model = sampler.FoleyModel(dit, synth.synth_dit_state_dict(dit), torch.float32, dev, dac_cfg=dc)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(dc), dev, dc)
    model.attach_dac(dac)
    g = golden("g3_layers")
    y = model.ctx.dac_decode(g["dac52_z"].to(dev).contiguous())
    assert rel_err(y, g["dac52_y"]) < 2e-5


def test_dac_golden_full_width(dev):
    """G9: the real 2048-wide decoder, rates (8,5,4,3,2), on 10 latent frames -> 9600 samples."""
    model = sampler.FoleyModel(C.TINY, synth.synth_dit_state_dict(C.TINY), torch.float32, dev, dac_cfg=C.DAC48K)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev, C.DAC48K)
    model.attach_dac(dac)
    g = golden("g9_dac")
    y = model.ctx.dac_decode(g["z"].to(dev).contiguous())
    assert y.shape == (1, 1, 9600)
    assert rel_err(y, g["y"]) < 2e-5
    # batch of 3 with different latents == three independent decodes (segment handling)
    z3 = torch.randn(3, 128, 7, generator=torch.Generator().manual_seed(4)).to(dev)
    y3 = model.ctx.dac_decode(z3)
    for i in range(3):
        assert rel_err(y3[i:i + 1], model.ctx.dac_decode(z3[i:i + 1].contiguous())) < 1e-6


DAC_WINDOW_MARGIN = 16      # latent frames: tests/test_dac_window_cpu.py shows that it covers the decoder's receptive field


def test_dac_decode_60s_six_clips(dev):
    """The full-width decoder at the node's maximum: latents [6, 128, 3000] -> [6, 1, 2 880 000].  The last stage's activations
    (dacP / Q / R) are 6 x 2 880 000 x 64 fp32 = 4.4 GB: past 2^31 and 2^32 bytes.  (a) every clip equals its own decode, also at
    its edges (no bleeding across clip boundaries); (b) latent windows against the oracle, each with a margin of DAC_WINDOW_MARGIN
    frames cut off before comparing: the head of clip 0, both sides of the clip 2 / 3 boundary, an interior window of clip 4 and
    the tail of clip 5 (activations past 4 GiB)."""
    clips, T, hop, m, w = 6, 3000, C.DAC48K.hop, DAC_WINDOW_MARGIN, 16
    dsd = synth.synth_dac_state_dict(C.DAC48K)
    model = sampler.FoleyModel(C.TINY, synth.synth_dit_state_dict(C.TINY), torch.float32, dev, dac_cfg=C.DAC48K)
    model.attach_dac(sampler.FoleyDAC(dsd, dev, C.DAC48K))
    z = torch.randn(clips, 128, T, generator=torch.Generator().manual_seed(66))
    y = model.ctx.dac_decode(z.to(dev).contiguous()).cpu()
    assert y.shape == (clips, 1, T * hop) and bool(torch.isfinite(y).all())
    edge = m * hop
    for i in range(clips):                                                                        # (a)
        yi = model.ctx.dac_decode(z[i:i + 1].to(dev).contiguous()).cpu()
        assert rel_err(y[i], yi[0]) <= 1e-6, i
        assert rel_err(y[i, :, :edge], yi[0, :, :edge]) <= 1e-6 and rel_err(y[i, :, -edge:], yi[0, :, -edge:]) <= 1e-6, i
    del model
    torch.cuda.empty_cache()
    errs = {}
    with torch.inference_mode():                                                                  # (b)
        heads = O.dac_decode(dsd, torch.stack([z[0, :, :w + m], z[3, :, :w + m]]), C.DAC48K.rates, C.DAC48K.dilations)
        tails = O.dac_decode(dsd, torch.stack([z[2, :, -(w + m):], z[5, :, -(w + m):]]), C.DAC48K.rates, C.DAC48K.dilations)
        mid = O.dac_decode(dsd, z[4:5, :, 1500 - m:1500 + w + m].contiguous(), C.DAC48K.rates, C.DAC48K.dilations)
    errs["clip0_head"] = rel_err(y[0, :, :w * hop], heads[0, :, :w * hop])
    errs["clip3_head"] = rel_err(y[3, :, :w * hop], heads[1, :, :w * hop])
    errs["clip2_tail"] = rel_err(y[2, :, -w * hop:], tails[0, :, -w * hop:])
    errs["clip5_tail"] = rel_err(y[5, :, -w * hop:], tails[1, :, -w * hop:])
    errs["clip4_mid"] = rel_err(y[4, :, 1500 * hop:(1500 + w) * hop], mid[0, :, m * hop:(m + w) * hop])
    record_parity("dac_60s_x6_windows", worst=max(errs.values()))
    print("DAC 60 s x 6 windows: %s" % " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < 2e-5, (k, e)


def test_dac_encoder_golden(dev):
    """G10: DAC.encode on the HIP engine vs the reference - narrow codec on ragged-length
    audio (right-padded to the hop like DAC.preprocess) and the real 128 -> 4096-channel encoder; then
    decode(encode(x).mode()) keeps the waveform length (codec round trip through both halves)."""
    g = golden("g10_dac_encode")
    for tag, dc in (("tiny", C.DAC_ENC_TINY), ("full", C.DAC48K)):
        dsd = synth.synth_dac_state_dict(dc, device=dev, encoder=True)
        model = sampler.FoleyModel(C.TINY, synth.synth_dit_state_dict(C.TINY), torch.float32, dev, dac_cfg=dc)
        dac = sampler.FoleyDAC(dsd, dev, dc)
        assert dac.has_encoder
        model.attach_dac(dac)
        params = model.ctx.dac_encode(g[tag + "_audio"].to(dev))
        assert params.shape == g[tag + "_params"].shape
        assert rel_err(params, g[tag + "_params"]) < 2e-5, tag
        mean, std = O.gaussian_posterior(params.cpu())
        assert rel_err(std, g[tag + "_std"]) < 2e-5
        if dc.latent_dim == C.TINY.latent_dim:      # the decoder of this context consumes latent_dim-wide codes
            wave = model.ctx.dac_decode(mean.to(dev).contiguous())
            assert wave.shape == (params.shape[0], 1, params.shape[2] * dc.hop) and bool(torch.isfinite(wave).all())
    # batch of clips == independent clips (segment handling of the strided convs)
    a3 = 0.3 * torch.randn(3, 1, 6 * 11, generator=torch.Generator().manual_seed(3))
    dc = C.DAC_ENC_TINY
    model = sampler.FoleyModel(C.TINY, synth.synth_dit_state_dict(C.TINY), torch.float32, dev, dac_cfg=dc)
    model.attach_dac(sampler.FoleyDAC(synth.synth_dac_state_dict(dc, device=dev, encoder=True), dev, dc))
    p3 = model.ctx.dac_encode(a3.to(dev))
    for i in range(3):
        assert rel_err(model.ctx.dac_encode(a3[i:i + 1].to(dev)), p3[i:i + 1]) < 1e-6


def test_batch_equals_independent_clips(tiny):
    """Clips in a batch are independent: bs=3 must equal three bs=1 runs."""
    sd, _dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    feats = ({"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]},
             {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]})
    noise = torch.randn(3, 128, 50, generator=torch.Generator().manual_seed(8))
    _a, _sr, lat3 = sampler.denoise_process_with_generator(*feats, 1.0, model, dac, 4.5, 10, 3, "euler",
                                                           noise=noise, return_latents=True)
    for i in range(3):
        _a, _sr, lat1 = sampler.denoise_process_with_generator(*feats, 1.0, model, dac, 4.5, 10, 1, "euler",
                                                               noise=noise[i:i + 1], return_latents=True)
        assert rel_err(lat3[i:i + 1], lat1) < 1e-5


def test_bf16_mode_forward(dev):
    """Throughput mode: bf16 GEMM operands, fp32 accumulate/residual.  Checked against the oracle
    run on bf16-rounded weights with a bf16-appropriate tolerance (the 1e-3 gate is an fp32-mode
    gate)."""
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    sdq = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 and "pos_emb" not in k and "empty" not in k else v)
           for k, v in sd.items()}
    model = sampler.FoleyModel(c, sd, torch.bfloat16, dev, dac_cfg=C.DAC_TINY)
    g = golden("g5_dit_tiny")
    x, t, cond, clip, sync = (g["a_" + k] for k in ("x", "t", "cond", "clip", "sync"))
    xq = x.to(torch.bfloat16).float()
    y = _forward(model, xq, t, cond, clip, sync)
    with torch.inference_mode():
        ref = O.dit_forward(sdq, c.heads, xq, t, cond, clip, sync)
    assert rel_err(y, ref) < 3e-2


def test_c1_xxl_golden(dev):
    """G6 - the parity gate of BASELINE.json: config C1 (T2A 1 s, 10 Euler steps, CFG off, bs 1)
    at real xxl dimensions, HIP fp32 mode vs the reference fp32 CPU sampler: 1e-3 relative on
    the 48 kHz waveform; per-step latents localise any drift."""
    g = golden("g6_c1_xxl")
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 1.0, t2a=True, sd=sd, device=dev)
    model = sampler.FoleyModel(cfg, sd, torch.float32, dev)
    del sd
    torch.cuda.empty_cache()
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    trace = []
    La = 50
    plan = sampler.build_plan(model, {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]},
                              {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}, La, 1.0, 10, 1,
                              "euler")
    model.attach_dac(dac)
    model.ctx.prepare(plan)
    lat = g["noise"].to(dev).contiguous()
    model.ctx.sample(lat, use_graph=False, progress=lambda i, n: trace.append(lat.clone().cpu()))
    errs = [rel_err(trace[i], g["latents"][i]) for i in range(10)]
    print("per-step latent rel err:", ["%.2e" % e for e in errs])
    wave = model.ctx.dac_decode(lat)
    werr = rel_err(wave, g["waveform"])
    print("waveform rel err: %.3e" % werr)
    assert max(errs) < 1e-4
    assert werr < 1e-3


def test_full_size_properties(dev):
    """BASELINE.json's full-size workload (C2: xxl, 5 s, CFG 4.5, bf16) through size-independent properties of the
    sampler (the reference comparison at this size is test_full_size_against_reference_fixture, goldens g14 / g15):
    (1) clips of a batch are independent: identical noise rows give bit-identical latents
        (deterministic reductions, no atomics); a batch row equals the single-clip run to 1e-5 in
        fp32 mode (tile shapes / K splits depend on the row count, the K order per element does
        not) and to bf16 accuracy in bf16 mode (different split points round differently);
    (2) replaying the captured hipGraph equals eager launches bit for bit;
    (3) the Euler update is affine in the model output: x_end - x_0 = sum_i v_i * dt_i, so running
        n steps equals two consecutive runs of the same schedule halves only through the model -
        checked here as: cfg scale 1.0 (single branch) equals the cond half of the CFG pair at g=1;
    (4) fp32 parity mode and bf16 agree to bf16 accuracy after a few steps."""
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    La, steps = 250, 3
    n1 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(11))
    n2 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(12))

    def run(noise, g, graph, m=model):
        plan = sampler.build_plan(m, visual, text, La, g, steps, noise.shape[0], "euler")
        m.ctx.prepare(plan)
        lat = noise.clone().to(dev).contiguous()
        m.ctx.sample(lat, use_graph=graph)
        return lat.cpu()

    b3 = run(torch.cat([n1, n2, n1]), 4.5, True)
    assert torch.equal(b3[0], b3[2]) and not torch.equal(b3[0], b3[1])          # (1) same noise, same result
    s1 = run(n1, 4.5, True)
    assert rel_err(s1[0], b3[0]) < 5e-2                                          # (1) batch row ~ single clip (bf16)
    assert torch.equal(run(n1, 4.5, False), s1)                                  # (2) graph replay == eager
    assert torch.isfinite(b3).all() and float((s1 - n1).abs().max()) > 1e-3      # the loop did move the sample
    g1 = run(n1, 1.0, True)                                                      # (3) CFG off: single branch
    assert rel_err(g1, s1) > 1e-4                                                # ... differs from guided
    model32 = sampler.FoleyModel(cfg, sd, torch.float32, dev)
    f32 = run(n1, 4.5, False, model32)
    assert rel_err(s1, f32) < 5e-2                                               # (4) bf16 vs fp32 after 3 steps
    f32b = run(torch.cat([n2, n1]), 4.5, False, model32)
    assert rel_err(f32b[1], f32[0]) < 1e-5                                       # (1) fp32: batch row == single clip
    print("bf16 single-vs-batch %.2e, bf16-vs-fp32 %.2e, fp32 single-vs-batch %.2e" %
          (rel_err(s1[0], b3[0]), rel_err(s1, f32), rel_err(f32b[1], f32[0])))
    # (5) the bs=8 configuration (256x128 tiles, wide attention kernel, no K split): every clip of the
    #     batch against its own single-clip run
    n8 = torch.randn(8, 128, La, generator=torch.Generator().manual_seed(13))
    b8 = run(n8, 4.5, True)
    errs = [rel_err(b8[i], run(n8[i:i + 1], 4.5, True)[0]) for i in (0, 3, 7)]
    print("bs=8 rows vs single-clip runs:", ["%.2e" % e for e in errs])
    assert max(errs) < 5e-2


def test_full_size_properties_v2a(dev):
    """BASELINE config C3 at full size: xxl, 5 s, CFG 4.5 with NON-empty SigLIP2 / Synchformer features
    (reference utils.py:159-199: the unconditional half carries the learned empty rows, hifi_foley.py:755-762
    up-samples the 112 sync tokens).  Unlike C2 the conditional half keeps all Ls = 112 distinct sync rows
    while the unconditional half is 8-periodic, so the plan must NOT take the periodic shortcut: the
    single-block modulation GEMM runs on M = 2*112 rows and the per-token operands are addressed through
    RowBcast mode 2 with per = 0.  Checked
    (0) against the oracle: one xxl-width (depth 1+1) forward of the [uncond ; cond] x 2-clip batch, fp32, 2e-5,
        and the bf16 mode of the same forward;
    (1)-(4) at full depth through the properties of test_full_size_properties (the reference comparison at full
        depth is test_full_size_against_reference_fixture, golden g15): batch independence, graph replay == eager, bf16 vs fp32, and that the dense features
        are really in use (differs from the text-only run on the same noise)."""
    cfg = C.XXL
    La, Lv, Ls = C.lengths(5.0, cfg)
    assert (La, Lv, Ls) == (250, 40, 112)
    # ---- (0) oracle comparison at full width, depth 1+1
    c11 = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1)
    sd11 = synth.synth_dit_state_dict(c11)
    cond11 = synth.synth_conditioning(c11, 5.0, t2a=False, sd=sd11)
    vis11 = {"siglip2_feat": cond11["clip"], "syncformer_feat": cond11["sync"]}
    txt11 = {"text_feat": cond11["text"], "uncond_text_feat": cond11["uncond_text"]}
    x = torch.randn(2, 128, La, generator=torch.Generator().manual_seed(31))
    it, steps = 3, 10
    t_it = tables.model_timesteps(tables.sigma_grid(steps))[it]
    text77 = O.pad_or_trim_text(cond11["text"])
    unc77 = O.pad_or_trim_text(cond11["uncond_text"])
    e_clip = sd11["empty_clip_feat"].view(1, 1, -1).expand(1, Lv, -1)
    e_sync = sd11["empty_sync_feat"].view(1, 1, -1).expand(1, Ls, -1)
    with torch.inference_mode():       # rows ordered [cfg][clip]: uncond x 2 clips, then cond x 2 clips
        ref = O.dit_forward(sd11, c11.heads, torch.cat([x, x]), t_it.expand(4),
                            torch.cat([unc77, unc77, text77, text77]),
                            torch.cat([e_clip, e_clip, cond11["clip"], cond11["clip"]]),
                            torch.cat([e_sync, e_sync, cond11["sync"], cond11["sync"]]))
    ref_rows = ref.transpose(1, 2).reshape(4 * La, 128)
    for dtype, tol in ((torch.float32, 2e-5), (torch.bfloat16, 4e-2)):
        m = sampler.FoleyModel(c11, sd11, dtype, dev)
        m.ctx.prepare(sampler.build_plan(m, vis11, txt11, La, 4.5, steps, 2, "euler"))
        xin = x.to(dtype).float() if dtype != torch.float32 else x
        rows = m.ctx.dit_forward(xin.to(dev).contiguous(), it)
        e = rel_err(rows, ref_rows)
        print("xxl-1-1 V2A forward, CFG pair x 2 clips, %s: %.2e" % (dtype, e))
        assert e < tol
        del m
    # ---- (1)-(4) full depth
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=False, sd=sd, device=dev)
    assert cond["clip"].shape[1] == Lv and cond["sync"].shape[1] == Ls
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    steps = 3
    n1 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(11))
    n2 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(12))

    def run(noise, graph, m=model, vis=visual):
        plan = sampler.build_plan(m, vis, text, La, 4.5, steps, noise.shape[0], "euler")
        m.ctx.prepare(plan)
        lat = noise.clone().to(dev).contiguous()
        m.ctx.sample(lat, use_graph=graph)
        return lat.cpu()

    b3 = run(torch.cat([n1, n2, n1]), True)
    assert torch.isfinite(b3).all()
    assert torch.equal(b3[0], b3[2]) and not torch.equal(b3[0], b3[1])          # (1) clips are independent
    s1 = run(n1, True)
    assert rel_err(s1[0], b3[0]) < 5e-2
    assert torch.equal(run(n1, False), s1)                                       # (2) graph replay == eager
    ct = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    t2a = run(n1, True, vis={"siglip2_feat": ct["clip"], "syncformer_feat": ct["sync"]})
    assert rel_err(t2a, s1) > 1e-3                                               # (4) the features matter
    assert torch.equal(run(n1, True), s1)                                        # ... and the switch back leaves no stale periodic plan
    model32 = sampler.FoleyModel(cfg, sd, torch.float32, dev)
    f32 = run(n1, False, model32)
    print("C3 full size: bf16 single-vs-batch %.2e, bf16-vs-fp32 %.2e" % (rel_err(s1[0], b3[0]), rel_err(s1, f32)))
    assert rel_err(s1, f32) < 5e-2                                               # (3) bf16 vs fp32 after 3 steps
    # the bs=8 shapes of C4 (what each GPU of the 8-GPU job runs): rows against their single-clip runs
    n8 = torch.randn(8, 128, La, generator=torch.Generator().manual_seed(13))
    b8 = run(n8, True)
    errs = [rel_err(b8[i], run(n8[i:i + 1], True)[0]) for i in (0, 5)]
    print("C4 per-GPU batch (bs=8) rows vs single-clip runs:", ["%.2e" % e for e in errs])
    assert max(errs) < 5e-2


def test_c5_full_size_properties(dev):
    """BASELINE config C5 as a whole: xxl + fp8_e4m3fn weight storage + 30 s (La=1500, Lv=240, Ls=736)
    + negative-prompt CFG 4.5, through the loader's own entry point, pinned by size-independent properties of the
    3-step run (the reference comparison of one model call at this size is test_c5_full_size_against_reference_fixture, g16):
    (1) clips of a batch are independent (identical noise rows -> bit-identical latents);
    (2) hipGraph replay == eager launches, bit for bit;
    (3) the fp8-rounded weights are really in use (differs from the un-quantised model) and the
        delta stays at fp8-rounding scale after a few steps;
    (4) the waveform has the 30 s length and is finite."""
    from foley_amd import nodes
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 30.0, t2a=True, sd=sd, device=dev)
    assert cond["clip"].shape[1] == 240 and cond["sync"].shape[1] == 736
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    m8 = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "fp8_e4m3fn", device=dev, cfg=cfg)
    assert m8.quantization == "fp8_e4m3fn"
    La, steps = 1500, 3
    n1 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(21))
    n2 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(22))

    def run(m, noise, graph):
        plan = sampler.build_plan(m, visual, text, La, 4.5, steps, noise.shape[0], "euler")
        m.ctx.prepare(plan)
        lat = noise.clone().to(dev).contiguous()
        m.ctx.sample(lat, use_graph=graph)
        return lat.cpu()

    b3 = run(m8, torch.cat([n1, n2, n1]), True)
    assert torch.isfinite(b3).all()
    assert torch.equal(b3[0], b3[2]) and not torch.equal(b3[0], b3[1])                  # (1)
    s1 = run(m8, n1, True)
    assert torch.equal(run(m8, n1, False), s1)                                           # (2)
    assert rel_err(s1[0], b3[0]) < 5e-2
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    m8.attach_dac(dac)
    wave = m8.ctx.dac_decode(s1.to(dev))
    assert wave.shape == (1, 1, 30 * 48000) and bool(torch.isfinite(wave).all())        # (4)
    del m8
    m16 = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=cfg)
    d = rel_err(run(m16, n1, True), s1)
    print("C5: fp8_e4m3fn vs unquantised bf16 after %d steps: %.3e" % (steps, d))
    assert 1e-4 < d < 0.2                                                                # (3)


def test_full_depth_at_node_maximum(dev):
    """The node's maximum through its own sampler entry point: xxl at full depth, bf16, text-to-audio 60 s x 6 clips with CFG 4.5,
    10 Euler steps, then the full-width DAC -> audio [6, 1, 2 880 000], every value finite.  Each clip is then generated again in a
    run of its own (batch of one, same noise).  The two are not bit-identical - K-origin rotation applies at one clip only, and the
    tile choice depends on M - so each clip is held to the batch-of-one waveform.  Measured on an MI355X: the engine runs this
    configuration (no limit refuses it) and every clip lands at 1.55e-2 from its batch-of-one run; the gate 3e-2 is twice that and
    stays below the bf16 mode's own distance from fp32 on a waveform (d0 = 4.5e-2, g18_c2_loop_bf16)."""
    from foley_amd import nodes
    cfg, dur, bs, steps, g = C.XXL, 60.0, 6, 10, 4.5
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, dur, t2a=True, sd=sd, device=dev)
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=cfg)
    del sd
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    La = int(dur * cfg.frame_rate)
    noise = sampler.draw_noise(bs, cfg.latent_dim, La, model.dtype, torch.Generator("cpu").manual_seed(6060))
    audio, sr = sampler.denoise_process_with_generator(visual, text, dur, model, dac, g, steps, bs, "euler", noise=noise)
    assert sr == 48000 and audio.shape == (bs, 1, 2_880_000)
    assert bool(torch.isfinite(audio).all())
    audio = audio.cpu()
    errs = {}
    for b in range(bs):
        solo, _ = sampler.denoise_process_with_generator(visual, text, dur, model, dac, g, steps, 1, "euler", noise=noise[b:b + 1])
        errs[b] = rel_err(audio[b], solo[0])
    record_parity("node_maximum_xxl_60s_x6_batch_vs_solo", worst=max(errs.values()))
    print("xxl 60 s x 6, batch vs batch of one: %s" % " ".join("%.2e" % e for e in errs.values()))
    for b, e in errs.items():
        assert e < 3e-2, (b, e)


def _pair_forward(model, cond, La, noise, it, steps, dev):
    """The [uncond ; cond] model call of loop iteration `it` (CFG 4.5, one clip) -> [2, 128, La] on the CPU."""
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model.ctx.prepare(sampler.build_plan(model, visual, text, La, 4.5, steps, 1, "euler"))
    rows = model.ctx.dit_forward(noise.to(dev).contiguous(), it)
    return rows.view(2, La, 128).transpose(1, 2).float().cpu()


@pytest.mark.parametrize("fix,tag,t2a", [("g14_c2_full", "c2", True), ("g15_c3_full", "c3", False)])
def test_full_size_against_reference_fixture(dev, fix, tag, t2a):
    """BASELINE configs C2 (text-to-audio) and C3 (video-to-audio) REFERENCE-checked at the benchmarked size: xxl width,
    all 18 + 36 blocks, 5 s (La 250, Lv 40, Ls 112), the [uncond ; cond] model call of loop iteration 25 of 50 at CFG 4.5 -
    goldens g14 / g15 hold what the reference's own sampler loop (utils.py:125-258) fed to and got from
    HunyuanVideoFoley.forward (hifi_foley.py:707-924) there, in fp32 and as the sampler runs a bf16 model (parameters
    .to(bfloat16), bf16 inputs, torch.autocast(bfloat16); noise drawn in bf16).  fp32 mode: <= 1e-4 against the fp32
    output; bf16 mode: within 1.5 d0 of the reference's bf16 output and of its fp32 output, d0 = the reference's own
    bf16-vs-fp32 distance on these inputs (1.9e-2 at full depth)."""
    from foley_amd import nodes
    g = golden(fix)
    cfg = C.XXL
    La, steps, it = 250, 50, 25
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=t2a, sd=sd, device=dev)
    noise = sampler.draw_noise(1, 128, La, torch.bfloat16, torch.Generator("cpu").manual_seed(1234)).float()
    assert torch.equal((2 * noise.double().sum(dim=(0, 1))).float(), g[tag + "_x_sum"])          # the reference's model input
    assert float(g[tag + "_t"][0]) == float(tables.model_timesteps(tables.sigma_grid(steps))[it])
    y32, y16 = g[tag + "_y32"], g[tag + "_y16"]
    d0 = rel_err(y16, y32)
    m32 = nodes.HunyuanModelLoader.pack_state_dict(sd, "fp32", "none", device=dev, cfg=cfg)
    e = rel_err(_pair_forward(m32, cond, La, noise, it, steps, dev)[:, :, ::2], y32)
    print("%s full depth fp32 mode vs reference fp32: %.2e" % (tag, e))
    assert e < 1e-4
    del m32
    torch.cuda.empty_cache()
    m16 = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=cfg)
    y = _pair_forward(m16, cond, La, noise, it, steps, dev)[:, :, ::2]
    e16, e32 = rel_err(y, y16), rel_err(y, y32)
    print("%s full depth bf16 mode: d0 %.2e, vs reference bf16 %.2e, vs reference fp32 %.2e" % (tag, d0, e16, e32))
    record_parity(fix, fp32_vs_ref_fp32=e, d0=d0, bf16_vs_ref_bf16=e16, bf16_vs_ref_fp32=e32, e16_over_d0=e16 / d0, e32_over_d0=e32 / d0, gate="1e-4 / 1.5 d0")
    assert 5e-3 < d0 < 5e-2 and e16 < 1.5 * d0 and e32 < 1.5 * d0


def _c2_loop(model, dac, cond, noise, dev, checkpoints):
    """The headline run (C2: 5 s, 50 Euler iterations, CFG 4.5, one clip) on `noise` -> (latents after `checkpoints`, final
    latents, waveform), all on the CPU."""
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model.attach_dac(dac)
    model.ctx.prepare(sampler.build_plan(model, visual, text, 250, 4.5, 50, 1, "euler"))
    lat = noise.to(dev, torch.float32).contiguous()
    keep = {}
    model.ctx.sample(lat, use_graph=True, progress=lambda i, n: keep.__setitem__(i, lat.clone().cpu()) if i in checkpoints else None)
    wave = model.ctx.dac_decode(lat)
    return keep, lat.cpu(), wave.cpu()


def test_c2_full_loop_fp32_against_reference_fixture(dev):
    """north_star's gate AT THE HEADLINE CONFIGURATION (golden g17): the reference's own fp32 sampler loop - xxl, all 18 + 36
    blocks, text-to-audio 5 s, 50 Euler iterations, CFG 4.5, bs 1, seed 1234, through its DAC decoder (utils.py:125-258,
    scheduling_flow_match_discrete.py:210-297, dac.py:280-303) - against the HIP fp32 mode on the same drawn noise:
    <= 1e-3 relative on the 48 kHz waveform.  The latents after iterations 1 / 10 / 25 / 40 / 50 localise any drift."""
    from foley_amd import nodes
    g = golden("g17_c2_loop")
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    noise = sampler.draw_noise(1, 128, 250, torch.float32, torch.Generator("cpu").manual_seed(1234))
    assert torch.equal(noise, g["noise"])                                  # the reference drew exactly this
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "fp32", "none", device=dev, cfg=cfg)
    del sd
    torch.cuda.empty_cache()
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    cps = [int(c) for c in g["checkpoints"]]
    keep, lat, wave = _c2_loop(model, dac, cond, noise, dev, set(cps))
    errs = [rel_err(keep[c], g["latents"][i]) for i, c in enumerate(cps)]
    werr = rel_err(wave[..., ::5], g["wave_s5"])
    print("C2 full loop fp32 mode vs reference fp32: latents after %s: %s; waveform %.3e" % (cps, ["%.2e" % e for e in errs], werr))
    record_parity("g17_c2_loop_fp32", waveform=werr, gate="1e-3 (north_star)", **{"latents_it%d" % c: e for c, e in zip(cps, errs)})
    assert wave.shape == (1, 1, 240000)
    assert max(errs) < 1e-3
    assert werr < 1e-3


def test_c2_full_loop_bf16_against_reference_fixture(dev):
    """The BENCHMARKED precision over the whole headline run (golden g18): the loop as the reference runs a bf16 model
    (parameters .to(bfloat16), bf16 inputs, torch.autocast(bfloat16), noise drawn in bf16; utils.py:141-239) next to its fp32
    model on the same noise.  d0 = the reference's own 50-iteration bf16-vs-fp32 distance (latents 1.0e-2, waveform 4.5e-2);
    the HIP bf16 mode must land within 1.5 d0 of the reference's bf16 result and of its fp32 result.  The measured ratios go
    to the parity record (a regression from 0.6 d0 to 1.4 d0 passes the gate - the record shows it)."""
    from foley_amd import nodes
    g = golden("g18_c2_bf16_loop")
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    noise = sampler.draw_noise(1, 128, 250, torch.bfloat16, torch.Generator("cpu").manual_seed(1234)).float()
    assert torch.equal(noise, g["noise_b16"])
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=cfg)
    del sd
    torch.cuda.empty_cache()
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    cps = [int(c) for c in g["checkpoints"]]
    keep, lat, wave = _c2_loop(model, dac, cond, noise, dev, set(cps))
    d0_lat, d0_w = float(g["d0_latents"][-1]), float(g["d0_wave"])
    assert abs(rel_err(g["latents_b16"][-1], g["latents_f32"][-1]) - d0_lat) < 1e-6
    e16 = [rel_err(keep[c], g["latents_b16"][i]) for i, c in enumerate(cps)]
    e32 = [rel_err(keep[c], g["latents_f32"][i]) for i, c in enumerate(cps)]
    w16, w32 = rel_err(wave[..., ::5], g["wave_b16_s5"]), rel_err(wave[..., ::5], g["wave_f32_s5"])
    print("C2 full loop bf16 mode: d0 latents %s / waveform %.2e" % (["%.2e" % float(d) for d in g["d0_latents"]], d0_w))
    print("   vs reference bf16: latents %s, waveform %.2e (%.2f d0)" % (["%.2e" % e for e in e16], w16, w16 / d0_w))
    print("   vs reference fp32: latents %s, waveform %.2e (%.2f d0)" % (["%.2e" % e for e in e32], w32, w32 / d0_w))
    record_parity("g18_c2_loop_bf16", d0_latents=d0_lat, d0_waveform=d0_w, latents_vs_ref_bf16=e16[-1], latents_vs_ref_fp32=e32[-1],
                  waveform_vs_ref_bf16=w16, waveform_vs_ref_fp32=w32, e16_over_d0_latents=e16[-1] / d0_lat, e32_over_d0_latents=e32[-1] / d0_lat,
                  e16_over_d0_waveform=w16 / d0_w, e32_over_d0_waveform=w32 / d0_w, gate="1.5 d0")
    assert 5e-3 < d0_lat < 2e-2 and 2e-2 < d0_w < 8e-2
    assert e16[-1] < 1.5 * d0_lat and e32[-1] < 1.5 * d0_lat
    assert w16 < 1.5 * d0_w and w32 < 1.5 * d0_w


@pytest.mark.parametrize("depth", ["d1", "full"])
def test_c5_full_size_against_reference_fixture(dev, depth):
    """BASELINE config C5 REFERENCE-checked at its own size: xxl width, 30 s (La 1500, Lv 240, Ls 736), negative-prompt
    CFG pair, fp8_e4m3fn weight storage under bf16 compute - golden g16 holds the model call of loop iteration 25 of 50 as
    the reference runs it on bf16 parameters wrapped by its own _wrap_fp8_inplace (utils.py:316-485) under bf16 autocast,
    next to the fp32 run of the un-quantised model, at depth 1+1 and at full depth.  This is where the 256-row fp8 tiles and
    the wide attention kernel run INSIDE the model at their benchmarked shapes.  fp32 mode <= 1e-4 against the fp32
    output; fp8 + bf16 mode within 1.5 d0 of the reference's fp8 + bf16 output and of its fp32 output (d0 = their
    distance: 4.3e-2 at depth 1+1, 6.0e-2 at full depth)."""
    from foley_amd import nodes
    g = golden("g16_c5_full")
    cfg = C.XXL if depth == "full" else C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1)
    La, steps, it = 1500, 50, 25
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 30.0, t2a=True, sd=sd, device=dev)
    assert cond["clip"].shape[1] == 240 and cond["sync"].shape[1] == 736
    noise = sampler.draw_noise(1, 128, La, torch.bfloat16, torch.Generator("cpu").manual_seed(1234)).float()
    assert torch.equal((2 * noise.double().sum(dim=(0, 1))).float(), g[depth + "_x_sum"])
    y32, y8 = g[depth + "_y32"], g[depth + "_y16"]
    d0 = rel_err(y8, y32)
    m32 = nodes.HunyuanModelLoader.pack_state_dict(sd, "fp32", "none", device=dev, cfg=cfg)
    e = rel_err(_pair_forward(m32, cond, La, noise, it, steps, dev)[:, :, ::16], y32)
    print("C5 %s fp32 mode vs reference fp32: %.2e" % (depth, e))
    assert e < 1e-4
    del m32
    torch.cuda.empty_cache()
    m8 = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "fp8_e4m3fn", device=dev, cfg=cfg)
    assert m8.quantization == "fp8_e4m3fn"
    y = _pair_forward(m8, cond, La, noise, it, steps, dev)[:, :, ::16]
    e8, e32 = rel_err(y, y8), rel_err(y, y32)
    print("C5 %s fp8 + bf16 mode: d0 %.2e, vs reference fp8 + bf16 %.2e, vs reference fp32 %.2e" % (depth, d0, e8, e32))
    record_parity("g16_c5_" + depth, fp32_vs_ref_fp32=e, d0=d0, fp8_vs_ref_fp8=e8, fp8_vs_ref_fp32=e32, e8_over_d0=e8 / d0, e32_over_d0=e32 / d0, gate="1e-4 / 1.5 d0")
    assert 1e-2 < d0 < 1e-1 and e8 < 1.5 * d0 and e32 < 1.5 * d0


@pytest.mark.parametrize("name,hidden,heads", [("xxl-1-1", 1536, 12), ("xl-1-1", 1408, 11)])
@pytest.mark.parametrize("dtype,fmt", [(torch.bfloat16, "none"), (torch.float16, "none"), (torch.bfloat16, "fp8_e4m3fn"), (torch.float16, "fp8_e5m2")])
def test_large_grid_tiles_against_the_oracle(dev, name, hidden, heads, dtype, fmt):
    """The large-grid GEMM tiles INSIDE the model (256x256 BK = 32 tiles for w1/w3, the 256-row tiles with the second barrier,
    256x256 split-K tiles at mid-size grids) in every operand / storage combination, at both model widths (D = 1408: a ragged
    last column tile and 44 chunks of 32 channels): one depth-1+1 forward of a CFG pair x 8 clips at 5 s (M = 4000) and of a CFG
    pair at 30 s (M = 3000), each against the fp32 oracle on the same (storage-rounded) weights."""
    from foley_amd import nodes
    c = C.DiTConfig(name=name, depth_triple=1, depth_single=1, hidden=hidden, heads=heads)
    sd = synth.synth_dit_state_dict(c)
    prec = "bf16" if dtype == torch.bfloat16 else "fp16"
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, prec, fmt, device=dev, cfg=c)
    sdq = nodes.fp8_round_state_dict(nodes.round_params(sd, dtype), fmt, autocast=True, param_dtype=dtype) if fmt != "none" else nodes.round_params(sd, dtype)
    sdq = {k: v.float() for k, v in sdq.items()}
    tol = (5e-3 if dtype == torch.bfloat16 else 8e-4) if fmt == "none" else 8e-3      # measured 1.8e-3 / 2.2e-4 / 2.2 - 2.8e-3
    for dur, clips in ((5.0, 8), (30.0, 1)):
        La, Lv, Ls = C.lengths(dur, c)
        cond = synth.synth_conditioning(c, dur, t2a=False, sd=sd)
        x = torch.randn(clips, 128, La, generator=torch.Generator().manual_seed(41)).to(dtype).float()
        steps, it = 10, 4
        vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
        txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
        model.ctx.prepare(sampler.build_plan(model, vis, txt, La, 4.5, steps, clips, "euler"))
        rows = model.ctx.dit_forward(x.to(dev).contiguous(), it).float().cpu()          # [(cfg, clip, l), 128]
        # round 6: the short-K layers whose epilogue rules out a K split take the 256x256 tile where it saves whole rounds of
        # workgroups - fc1 of the two-stream pair at M = 4000 + 640 (two-problem launch), q/k/v at M = 3000 (one round)
        kern = {e["label"]: e["kernel"] for e in model.ctx.profile_forward(x.to(dev).contiguous(), it=it, repeats=1)[0]}
        want = ["triple.mlp fc1 GEMM + GELU"] if clips == 8 else ["single.qkv GEMM + RMSNorm/RoPE head split", "triple.qkv GEMM + RMSNorm/RoPE head split"]
        for lab in want:
            assert "gemm_wide_kernel" in kern[lab], (dur, lab, kern[lab])
        t_it = tables.model_timesteps(tables.sigma_grid(steps))[it]
        text77, unc77 = O.pad_or_trim_text(cond["text"]), O.pad_or_trim_text(cond["uncond_text"])
        e_clip = sd["empty_clip_feat"].view(1, 1, -1).expand(1, Lv, -1)
        e_sync = sd["empty_sync_feat"].view(1, 1, -1).expand(1, Ls, -1)
        sel = [0, clips - 1] if clips > 1 else [0]                                       # first and last clip of the batch
        with torch.inference_mode():
            for b in sel:
                ref = O.dit_forward(sdq, c.heads, torch.cat([x[b:b + 1], x[b:b + 1]]), t_it.expand(2), torch.cat([unc77, text77]),
                                    torch.cat([e_clip, cond["clip"]]), torch.cat([e_sync, cond["sync"]]))
                got = torch.stack([rows.view(2, clips, La, 128)[0, b], rows.view(2, clips, La, 128)[1, b]]).transpose(1, 2)
                e = rel_err(got, ref)
                print("%s %s/%s %gs clip %d: %.2e" % (name, prec, fmt, dur, b, e))
                assert e < tol, (name, prec, fmt, dur, b, e)


@pytest.fixture(scope="module")
def xxl11_weights():
    """Depth-1+1 full-width weights and their bf16 / fp8-rounded fp32 copies for the oracle, built once per storage format."""
    from foley_amd import nodes
    c = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1, hidden=1536, heads=12)
    sd = synth.synth_dit_state_dict(c)
    rounded = {}

    def sdq(fmt):
        if fmt not in rounded:
            q = nodes.fp8_round_state_dict(nodes.round_params(sd, torch.bfloat16), fmt, autocast=True, param_dtype=torch.bfloat16) \
                if fmt != "none" else nodes.round_params(sd, torch.bfloat16)
            rounded[fmt] = {k: v.float() for k, v in q.items()}
        return rounded[fmt]
    return c, sd, sdq


def _depth11_forward_vs_oracle(dev, weights, dur, clips, fmt, sel=None):
    """One depth-1+1 full-width bf16 forward of `clips` clips under CFG (iteration 6 of 10), each selected clip's two CFG halves
    against the fp32 oracle on the same rounded weights; returns the relative error per clip."""
    from foley_amd import nodes
    c, sd, sdq = weights
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", fmt, device=dev, cfg=c)
    La, Lv, Ls = C.lengths(dur, c)
    cond = synth.synth_conditioning(c, dur, t2a=False, sd=sd)
    x = torch.randn(clips, 128, La, generator=torch.Generator().manual_seed(43)).to(torch.bfloat16).float()
    steps, it = 10, 6
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model.ctx.prepare(sampler.build_plan(model, vis, txt, La, 4.5, steps, clips, "euler"))
    rows = model.ctx.dit_forward(x.to(dev).contiguous(), it).float().cpu().view(2, clips, La, 128)
    del model
    t_it = tables.model_timesteps(tables.sigma_grid(steps))[it]
    text77, unc77 = O.pad_or_trim_text(cond["text"]), O.pad_or_trim_text(cond["uncond_text"])
    e_clip = sd["empty_clip_feat"].view(1, 1, -1).expand(1, Lv, -1)
    e_sync = sd["empty_sync_feat"].view(1, 1, -1).expand(1, Ls, -1)
    errs = {}
    with torch.inference_mode():
        for b in (range(clips) if sel is None else sel):
            ref = O.dit_forward(sdq(fmt), c.heads, torch.cat([x[b:b + 1], x[b:b + 1]]), t_it.expand(2), torch.cat([unc77, text77]),
                                torch.cat([e_clip, cond["clip"]]), torch.cat([e_sync, cond["sync"]]))
            errs[b] = rel_err(torch.stack([rows[0, b], rows[1, b]]).transpose(1, 2), ref)
    return errs


@pytest.mark.parametrize("dur,clips,fmt", [(8.0, 2, "none"), (12.0, 3, "none"), (3.7, 5, "none"), (20.0, 1, "none"), (1.0, 16, "none"),
                                           (12.0, 3, "fp8_e4m3fn"), (20.0, 1, "fp8_e4m3fn")])
def test_tile_rules_across_shapes(dev, xxl11_weights, dur, clips, fmt):
    """The launcher's tile rules change with the grid (one- vs multi-round launches, two-problem launches on the 256x256 tiles, the
    pair-counting head-split rule, K-origin rotation for single clips): one depth-1+1 full-width forward per shape BETWEEN the benchmarked
    ones (M = 800 ... 3600 audio rows, ragged durations), bf16 and fp8 storage, against the fp32 oracle on the same rounded weights -
    every clip of the batch (a clip-offset error in a two-problem launch, a K-split slab or a head-split epilogue shows in one clip)."""
    errs = _depth11_forward_vs_oracle(dev, xxl11_weights, dur, clips, fmt)
    print("%gs x %d clips %s: %s" % (dur, clips, fmt, " ".join("%.2e" % e for e in errs.values())))
    for b, e in errs.items():
        assert e < (5e-3 if fmt == "none" else 8e-3), (dur, clips, fmt, b, e)


@pytest.mark.parametrize("dur,clips,fmt", [(60.0, 1, "none"), (59.9, 2, "none"), (45.0, 3, "none"), (30.0, 6, "none"), (60.0, 6, "none"),
                                           (60.0, 1, "fp8_e4m3fn"), (60.0, 6, "fp8_e4m3fn")])
def test_forward_at_widget_extremes(dev, xxl11_weights, dur, clips, fmt):
    """The node's widget extremes (duration up to 60 s, batch up to 6): S = La + Lv = 3480 joint tokens, an odd Lv = 479 at 59.9 s,
    up to 36 000 audio rows per forward.  Depth-1+1 full width, bf16 / fp8 storage, every clip and both CFG halves against the fp32
    oracle (gates of test_tile_rules_across_shapes)."""
    errs = _depth11_forward_vs_oracle(dev, xxl11_weights, dur, clips, fmt)
    record_parity("widget_extremes_%gs_x%d_%s" % (dur, clips, fmt), worst=max(errs.values()))
    print("%gs x %d clips %s: %s" % (dur, clips, fmt, " ".join("%.2e" % e for e in errs.values())))
    for b, e in errs.items():
        assert e < (5e-3 if fmt == "none" else 8e-3), (dur, clips, fmt, b, e)


def test_xl_dimensions_forward(dev):
    """The xl model family (D=1408, 11 heads: N/K not multiples of 128/256) at depth 1+1 against the
    oracle - exercises the N-edge masking of every GEMM tile and the 11-head split."""
    c = C.DiTConfig(name="xl-1-1", depth_triple=1, depth_single=1, hidden=1408, heads=11)
    sd = synth.synth_dit_state_dict(c)
    model = sampler.FoleyModel(c, sd, torch.float32, dev)
    g = torch.Generator().manual_seed(17)
    La, Lv, Ls = C.lengths(1.5, c)
    x = torch.randn(1, 128, La, generator=g)
    t = torch.tensor([500.0])
    cond, clip, sync = torch.randn(1, 77, 768, generator=g), torch.randn(1, Lv, 768, generator=g), torch.randn(1, Ls, 768, generator=g)
    y = _forward(model, x, t, cond, clip, sync)
    with torch.inference_mode():
        ref = O.dit_forward(sd, c.heads, x, t, cond, clip, sync)
    assert rel_err(y, ref) < 2e-5
    # and the bf16 throughput mode of the same model
    model16 = sampler.FoleyModel(c, sd, torch.bfloat16, dev)
    y16 = _forward(model16, x.to(torch.bfloat16).float(), t, cond, clip, sync)
    assert rel_err(y16, ref) < 4e-2


def test_fp8_weight_only_loader(dev):
    """Config C5 semantics (reference utils.py:316-485, SURVEY Q11, golden g8): every Linear / Conv1d
    weight is rounded through fp8 (plain cast, no scales), everything else untouched - except that
    under bf16 autocast the timestep features and the first time-embedding bias pass through fp8
    too.  Checked against the oracle run on the same fp8-rounded weights."""
    from foley_amd import nodes
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    for q in ("fp8_e4m3fn", "fp8_e5m2"):
        model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", q, device=dev, cfg=c)
        assert model.quantization == q and model.dtype == torch.bfloat16
        qd = torch.float8_e4m3fn if q == "fp8_e4m3fn" else torch.float8_e5m2
        sdq = nodes.fp8_round_state_dict(sd, q, autocast=False, param_dtype=torch.bfloat16)
        assert sum(1 for k in sd if not torch.equal(sd[k], sdq[k])) == 56     # the 56 wrapped modules of golden g8
        g = golden("g5_dit_tiny")
        x, t, cond, clip, sync = (g["a_" + k] for k in ("x", "t", "cond", "clip", "sync"))
        xq = x.to(torch.bfloat16).float()
        y = _forward(model, xq, t, cond, clip, sync)
        with torch.inference_mode():
            ref = O.dit_forward(sdq, c.heads, xq, t, cond, clip, sync, fp8_time=qd)
            ref_no_quirk = O.dit_forward(sdq, c.heads, xq, t, cond, clip, sync)
        assert rel_err(y, ref) < 4e-2, q
        assert rel_err(y, ref) < rel_err(y, ref_no_quirk), q    # the fp8-rounded time features are really in use
        # the block weights STAY fp8 in HBM (39 matrices of the tiny config) and give what load-time widening gives
        n8 = [k for k, v in model.arena.items() if v.dtype == qd]
        assert len(n8) == 15 * c.depth_triple + 4 * c.depth_single + 1 and all(k.endswith(".w") for k in n8)
        wide = sampler.FoleyModel(c, nodes.fp8_round_state_dict(nodes.round_params(sd, torch.bfloat16), q, autocast=True,
                                                                param_dtype=torch.bfloat16), torch.bfloat16, dev)
        wide.quantization = q                                   # same fp8-rounded time features, weights widened at load
        assert model.arena.buffer.numel() < 0.62 * wide.arena.buffer.numel()
        assert rel_err(y, _forward(wide, xq, t, cond, clip, sync)) < 5e-3, q
    # a checkpoint that already stores fp8 tensors is honoured by quantization="auto"
    sd8 = {k: (v.to(torch.float8_e4m3fn) if nodes.fp8_wrapped_key(k, v) else v) for k, v in sd.items()}
    m = nodes.HunyuanModelLoader.pack_state_dict(sd8, "bf16", "auto", device=dev, cfg=c)
    assert m.quantization == "fp8_e4m3fn" and m.dtype == torch.bfloat16
    # ... and without fp8 tensors 'auto' (the widget default) still means e4m3fn, as in the reference
    assert nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "auto", device=dev, cfg=c).quantization == "fp8_e4m3fn"
    assert nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=c).quantization == "none"
    # precision="auto" looks at bf16/fp16/fp32 tensors only (reference utils.py:507-515): here the
    # fp32 biases dominate, exactly as the reference would decide
    assert nodes.detect_ckpt_major_precision(sd8) == torch.float32


def test_sampler_node_end_to_end(dev):
    """HunyuanFoleySampler.generate_audio with injected conditioning: AUDIO dict shapes / dtypes /
    device of the reference node (nodes.py:420-427) and seed determinism."""
    from foley_amd import nodes
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    model = sampler.FoleyModel(c, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    deps = nodes.AttributeDict(dac_model=sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY))
    cond = synth.synth_conditioning(c, 1.0, t2a=True, sd=sd)
    feats = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"], "text_feat": cond["text"],
             "uncond_text_feat": cond["uncond_text"]}
    node = nodes.HunyuanFoleySampler()
    kw = dict(frame_rate=16, duration=1.0, prompt="x", negative_prompt="y", cfg_scale=4.5, steps=10, sampler="euler",
              batch_size=2, seed=55574, force_offload=True, torch_compile_cfg={"backend": "inductor"},
              block_swap_args={"blocks_to_swap": 30}, features=feats)
    first, batch = node.generate_audio(model, deps, **kw)
    assert first["sample_rate"] == 48000 and first["waveform"].shape == (1, 1, 48000)
    assert batch["waveform"].shape == (2, 1, 48000) and batch["waveform"].dtype == torch.float32
    assert batch["waveform"].device.type == "cpu" and torch.equal(first["waveform"][0], batch["waveform"][0])
    # the node's waveform against the CPU oracle on the same seed: generator -> noise -> loop -> decode
    noise = torch.randn((2, 128, 50), generator=torch.Generator("cpu").manual_seed(55574), dtype=torch.float32)
    with torch.inference_mode():
        ref = O.sample_waveform(sd, synth.synth_dac_state_dict(C.DAC_TINY), c.heads, noise, cond, 10, 4.5, "euler",
                                rates=C.DAC_TINY.rates)
    assert rel_err(batch["waveform"], ref) < 1e-3
    _f2, batch2 = node.generate_audio(model, deps, **kw)
    assert rel_err(batch2["waveform"], batch["waveform"]) < 1e-6
    kw["seed"] = 1
    _f3, batch3 = node.generate_audio(model, deps, **kw)
    assert rel_err(batch3["waveform"], batch["waveform"]) > 1e-2


def test_progress_callback_path(tiny):
    """What ComfyUI actually runs: the eager loop with a per-iteration progress callback (one stream
    sync per iteration, foley_sample with cb != NULL).  Must report every iteration in order and give
    the same latents as the callback-free graph replay, bit for bit."""
    sd, dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    seen = []
    gen = torch.Generator("cpu").manual_seed(7)
    a1, _sr, l1 = sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 12, 2, "heun-2", generator=gen,
                                                        use_graph=False, progress=lambda i, n: seen.append((i, n)),
                                                        return_latents=True)
    assert seen == [(i + 1, 12) for i in range(12)]
    gen = torch.Generator("cpu").manual_seed(7)
    a2, _sr, l2 = sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 12, 2, "heun-2", generator=gen,
                                                        use_graph=True, return_latents=True)
    assert torch.equal(l1, l2) and torch.equal(a1, a2)


def test_interrupt_from_the_progress_callback(tiny):
    """ComfyUI's interrupt: comfy.utils.ProgressBar.update raises inside the sampling loop (reference utils.py:247) and the
    exception ends the run.  Here the callback's exception crosses the C frame by way of foley_abort: the loop stops after that
    iteration, the SAME exception reaches the caller, and the context samples normally afterwards."""
    sd, dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}

    class Interrupted(Exception):
        pass

    for graph in (False, True):
        seen = []

        def tick(i, n):
            seen.append(i)
            if i == 3:
                raise Interrupted("stop")

        with pytest.raises(Interrupted):
            sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 12, 2, "euler",
                                                   generator=torch.Generator("cpu").manual_seed(7), use_graph=graph, progress=tick)
        assert seen == [1, 2, 3]
    # a request that arrives while no loop runs is dropped; the context is intact
    model.ctx.abort()
    outs = []
    for kw in (dict(use_graph=False, progress=lambda i, n: None), dict(use_graph=True)):
        a, _sr, lat = sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 12, 2, "euler",
                                                            generator=torch.Generator("cpu").manual_seed(7), return_latents=True, **kw)
        outs.append(lat)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_zero_depth_single_joins_side_stream(dev):
    """depth_single == 0: the forward has no single-stream blocks and skips their modulation GEMM (it runs in line on the
    caller's stream; an early version forked a side stream for it, which had to be joined here too): a captured loop equals
    the eager one bit for bit and both match the oracle."""
    c = C.DiTConfig(name="triple-only", depth_triple=1, depth_single=0, hidden=256, heads=2)
    sd = synth.synth_dit_state_dict(c)
    model = sampler.FoleyModel(c, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY)
    cond = synth.synth_conditioning(c, 1.0, t2a=False)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    outs = []
    for graph in (True, False):
        gen = torch.Generator("cpu").manual_seed(3)
        _a, _sr, lat = sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 4, 1, "euler", generator=gen,
                                                             use_graph=graph, return_latents=True)
        outs.append(lat.cpu())
    assert torch.equal(outs[0], outs[1])
    noise = torch.randn((1, 128, 50), generator=torch.Generator("cpu").manual_seed(3))
    with torch.inference_mode():
        ref = O.sample_latents(sd, c.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"], 4, 4.5,
                               "euler")
    assert rel_err(outs[0], ref) < 1e-4


def _graph_vs_eager(model, dac, cond, dur, noise):
    """(graph, eager) latents of one 6-step CFG run of `cond` on the shared context."""
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    return [sampler.denoise_process_with_generator(vis, txt, dur, model, dac, 4.5, 6, 1, "euler", noise=noise, use_graph=g,
                                                   return_latents=True)[2].cpu().clone() for g in (True, False)]


def test_graph_replay_across_text_and_video_at_one_shape(tiny):
    """One context, use_graph=True, one shape (2 s, CFG 4.5): text-to-audio -> video -> text-to-audio -> video.  The two differ
    in what the captured iteration launches - text-to-audio has both halves' sync tokens 8-periodic and reads the modulation
    table foley_prepare hoisted, a video clip has one periodic and one dense half and runs the modulation GEMM in the loop -
    so a replay of the other one's graph would be wrong.  Every graph run equals the eager run of the same inputs bit for
    bit, and the second round equals the first bit for bit."""
    sd, _dsd, model, dac = tiny
    dur = 2.0
    noise = torch.randn(1, 128, int(dur * 50), generator=torch.Generator().manual_seed(21))
    conds = [synth.synth_conditioning(C.TINY, dur, t2a=t2a, sd=sd) for t2a in (True, False)]
    first = {}
    for k in (0, 1, 0, 1):
        got, want = _graph_vs_eager(model, dac, conds[k], dur, noise)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), k
        assert torch.equal(got, first.setdefault(k, got)), k
    assert rel_err(first[0], first[1]) > 1e-2


def test_graph_replay_after_weight_reregistration(tiny):
    """One context, use_graph=True, one plan: the final projection's weight registered at its own address -> a scaled copy at
    another address -> the first again -> the copy again.  The captured kernels hold the address that was registered at
    capture, so each move must end in a new capture: every graph run equals the eager run under the same registration bit
    for bit, the second round equals the first, and the two weights give different latents."""
    sd, _dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(22))
    w0 = model.ctx._keep["final.w"]
    weights = [w0, (0.5 * w0).contiguous()]
    assert weights[1].data_ptr() != w0.data_ptr()
    first = {}
    try:
        for k in (0, 1, 0, 1):
            model.ctx.set_tensor("final.w", weights[k])
            got, want = _graph_vs_eager(model, dac, cond, 1.0, noise)
            assert torch.equal(got, want) and bool(torch.isfinite(got).all()), k
            assert torch.equal(got, first.setdefault(k, got)), k
    finally:
        model.ctx.set_tensor("final.w", w0)
    assert rel_err(first[0], first[1]) > 1e-2


def test_profile_forward_brackets(tiny):
    """foley_profile_forward (bench.py's per-kernel roofline source): every op of the forward is
    bracketed, call counts follow the block structure, FLOPs add up to the algorithmic count."""
    sd, dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
    plan = sampler.build_plan(model, {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]},
                              {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}, 50, 4.5, 4, 1, "euler")
    model.ctx.prepare(plan)
    lat = torch.randn(1, 128, 50, device=model.device)
    prof, bracket_us = model.ctx.profile_forward(lat, it=1, repeats=2)
    by = {e["label"]: e for e in prof}
    nt, ns = C.TINY.depth_triple, C.TINY.depth_single
    assert by["single.qkv GEMM + RMSNorm/RoPE head split"]["calls_per_forward"] == ns
    assert by["single.layernorm+modulate (+pending split-K sum)"]["calls_per_forward"] == 2 * ns
    assert by["triple.layernorm+modulate (+pending split-K sum)"]["calls_per_forward"] == 3 * nt
    assert by["triple.self attention"]["calls_per_forward"] == nt and by["final.linear"]["calls_per_forward"] == 1
    assert all(e["avg_us"] > 0 for e in prof) and 0 <= bracket_us < 100
    # bracketed FLOPs == the per-forward algorithmic count minus the step-invariant (hoisted) part.  At 1 s the single blocks'
    # modulation has 2 x 16 distinct rows (the sync tokens): few enough that foley_prepare computes it for ALL iterations in one
    # GEMM (foley_rt.hip step 6), so it is not part of the forward any more
    D, M, Mv, Lt, H, Hc = 256, 2 * 50, 2 * 8, 77, 2, C.TINY.conv_hidden
    assert "single.modulation (all blocks, one GEMM)" not in by
    lin = (2 * D * D * nt * 14 * (M + Mv) + ns * 2 * M * (6 * D * D + 9 * Hc * D)    # qkv, lin1(k3), w1/w3(k3), w2(k3)
           + 2 * (M * 128 * D * 2))                                                    # audio_in + final
    att = 4 * H * 128 * (nt * 2 * ((50 + 8) ** 2 + (50 + 8) * Lt) + ns * 2 * 50 * 50)
    total = sum(e["flop_per_launch"] * e["calls_per_forward"] for e in prof)
    assert abs(total - (lin + att)) / (lin + att) < 1e-6
    # profiling must not disturb the regular path
    y1 = model.ctx.dit_forward(lat, 1)
    y2 = model.ctx.dit_forward(lat, 1)
    assert torch.equal(y1, y2)
    # 5 s of video: the modulation GEMM stays in the loop, on the DISTINCT sync-token rows (not on the 250 audio frames): the 8
    # periodic rows of the unconditional half (empty sync features) + the 112 dense rows of the conditional half
    La5, _lv5, Ls5 = C.lengths(5.0)
    lat5 = torch.randn(1, 128, La5, device=model.device)
    cond5 = synth.synth_conditioning(C.TINY, 5.0, t2a=False)
    plan5 = sampler.build_plan(model, {"siglip2_feat": cond5["clip"], "syncformer_feat": cond5["sync"]},
                               {"text_feat": cond5["text"], "uncond_text_feat": cond5["uncond_text"]}, La5, 4.5, 4, 1, "euler")
    model.ctx.prepare(plan5)
    prof5, _ = model.ctx.profile_forward(lat5, it=1, repeats=1)
    smod = {e["label"]: e for e in prof5}["single.modulation (all blocks, one GEMM)"]
    assert abs(smod["flop_per_launch"] - 2 * (8 + Ls5) * D * ns * 6 * D) < 1
    y5 = model.ctx.dit_forward(lat5, 1)
    # 5 s text-to-audio: both halves carry the empty sync feature, whose tokens repeat every 8 (sync_pos_emb) - foley_prepare finds
    # that on the data: 2 x 8 distinct rows, hoisted out of the loop
    cond_t = synth.synth_conditioning(C.TINY, 5.0, t2a=True, sd=sd)
    plan_t = sampler.build_plan(model, {"siglip2_feat": cond_t["clip"], "syncformer_feat": cond_t["sync"]},
                                {"text_feat": cond_t["text"], "uncond_text_feat": cond_t["uncond_text"]}, La5, 4.5, 4, 1, "euler")
    model.ctx.prepare(plan_t)
    prof_t, _ = model.ctx.profile_forward(lat5, it=1, repeats=1)
    assert "single.modulation (all blocks, one GEMM)" not in {e["label"] for e in prof_t}
    model.ctx.prepare(plan5)     # back to the video-conditioned plan: the full token set, the in-loop GEMM again
    assert torch.equal(model.ctx.dit_forward(lat5, 1), y5)
    model.ctx.prepare(plan)
    assert torch.equal(model.ctx.dit_forward(lat, 1), y1)


def test_single_rank_nccl_bundle_adoption(tiny, dev):
    """The data-parallel setup under the REAL `nccl` (= RCCL) backend with world_size 1 on this GPU:
    bundle layout from the config, fill on rank 0, ONE broadcast, arenas adopted from the bundle -
    latents bit-identical to the directly packed model."""
    import socket
    import torch.distributed as dist
    from foley_amd.host import distributed as D, packers
    sd, dsd, model, dac = tiny
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        spec = D.bundle_spec(C.TINY, C.DAC_TINY, torch.float32, 1.0)
        bundle = D.Bundle(spec, dev)
        cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
        bundle.fill(packers.pack_dit(sd, C.TINY, torch.float32), packers.pack_dac(dsd, C.DAC_TINY), cond)
        secs = D.broadcast_bundle(bundle)
        assert secs >= 0.0
    finally:
        dist.destroy_process_group()
    m2 = sampler.FoleyModel.from_arena(C.TINY, bundle.dit_arena(), torch.float32, dev, dac_cfg=C.DAC_TINY)
    d2 = sampler.FoleyDAC.from_arena(bundle.dac_arena(), dev, C.DAC_TINY)
    cv = bundle.cond_views()
    outs = []
    for mm, dd, cc in ((model, dac, cond), (m2, d2, cv)):
        gen = torch.Generator("cpu").manual_seed(99)
        a, _sr, lat = sampler.denoise_process_with_generator(
            {"siglip2_feat": cc["clip"], "syncformer_feat": cc["sync"]},
            {"text_feat": cc["text"], "uncond_text_feat": cc["uncond_text"]}, 1.0, mm, dd, 4.5, 6, 2, "euler",
            generator=gen, return_latents=True)
        outs.append((a.cpu(), lat.cpu()))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])


def test_bench_single_rank_forced_dist(dev):
    """bench.py --full under a launcher-style environment (RANK/WORLD_SIZE set, nccl process group, the single
    broadcast) on one GPU: exits 0 and prints the JSON line with the per-kernel roofline."""
    import json, os, socket, subprocess, sys
    from conftest import ROOT
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               FOLEY_BENCH_FORCE_DIST="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny", "--duration", "1",
                        "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.strip()]) == 1, r.stdout[:500]     # RCCL's banner went to stderr
    out = json.loads(r.stdout)
    assert out["n_gpus"] == 1 and out["config"]["collectives"] == 1 and out["value"] > 0
    assert out["roofline"]["kernels"] and out["roofline"]["frac"] > 0
    assert out["config"]["rccl_nranks"] == 1 and out["config"]["backend"] == "nccl" and len(out["config"]["ranks"]) == 1
    assert out["config"]["ranks"][0]["clips"] == 1 and out["config"]["ranks"][0]["uuid"]


def test_bench_dump_outputs(dev, tmp_path):
    """bench.py --dump-outputs: the waveform of the last timed step lands in DIR/audio.npy (float32, the clip's full shape), the
    line reports the timed steps it was asked for, and two runs with the same arguments (different step counts) dump the same
    waveform - the inputs are a pure function of the arguments."""
    import json, os, subprocess, sys
    import numpy as np
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    outs = []
    for i, (steps, warmup) in enumerate([(2, 0), (1, 1)]):
        d = str(tmp_path / f"run{i}")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny", "--duration", "1",
                            "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra", "--dump-outputs", d],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads(r.stdout)
        assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
        assert out["dump_outputs"]["arrays"]["audio"] == {"shape": [1, 1, 48000], "written": [1, 1, 48000], "sampled": False}
        a = np.load(os.path.join(d, "audio.npy"))
        assert a.dtype == np.float32 and a.shape == (1, 1, 48000) and np.isfinite(a).all() and np.abs(a).max() > 0
        outs.append(a)
    assert np.array_equal(outs[0], outs[1])


def test_bench_plain_run_is_lean(dev):
    """A plain bench.py run (no --full) on the default configuration prints the headline line and nothing that takes runs of its
    own: no roofline (per-kernel profile, event-timed loop), no extra configurations, no CPU baseline."""
    import json, os, subprocess, sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny", "--duration", "1",
                        "--steps", "2", "--warmup", "1"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout)
    assert out["metric"].startswith("audio-sec/sec (1s clip") and out["unit"] == "audio-sec/sec" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1.0 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]       # one 1 s clip per step
    assert not {"roofline", "extra", "cpu_baseline"} & set(out), sorted(out)
    assert out["config"]["ranks"][0]["clips"] == 2 and "loop_ms" not in out["config"]["ranks"][0]


def test_denoise_process_multi_shards_the_batch(tiny, dev):
    """Node-level data parallelism inside one process (host/sampler.py::replicate / denoise_process_multi): the
    clips of a batch are sharded over replicas, one host thread and one context each, with no collective.  On a
    1-GPU box the two replicas are two contexts on the same device (the threading, the per-thread stream capture
    and the process-wide set-up lock are what is exercised); with two GPUs the second replica lives on cuda:1
    after ONE grouped RCCL broadcast of the two arenas (runtime.bcast_local).  The sharded run must equal the single-context
    run of the full batch."""
    sd, dsd, model, dac = tiny
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    full, sr, lat_full = sampler.denoise_process_with_generator(
        vis, txt, 1.0, model, dac, 4.5, 10, 3, "euler", generator=torch.Generator("cpu").manual_seed(7), return_latents=True)
    second = torch.device("cuda:1") if torch.cuda.device_count() >= 2 else dev
    reps = sampler.replicate(model, dac, [dev, second])
    assert reps[0][0] is model and reps[1][0] is not model and reps[1][0].device == second
    assert sampler.replicate(model, dac, [dev, second])[1][0] is reps[1][0]          # cached
    ticks = []
    multi, sr2, lat_multi = sampler.denoise_process_multi(
        vis, txt, 1.0, reps, 4.5, 10, 3, "euler", generator=torch.Generator("cpu").manual_seed(7), return_latents=True,
        progress=lambda i, n: ticks.append(i))
    assert sr2 == sr and multi.shape == full.shape and ticks == list(range(1, 11))
    assert rel_err(lat_multi, lat_full) < 1e-5 and rel_err(multi, full) < 1e-5
    # a shard count above the batch size leaves the surplus replicas idle
    one, _sr = sampler.denoise_process_multi(vis, txt, 1.0, reps, 4.5, 10, 1, "euler",
                                             generator=torch.Generator("cpu").manual_seed(7))
    assert rel_err(one, full[:1]) < 1e-5


def test_eight_contexts_on_one_device_full_size(dev):
    """What an 8-GPU ComfyUI run asks of ONE host process (sampler.denoise_process_multi, FOLEY_DATA_PARALLEL=1), de-risked
    on one GPU: EIGHT contexts of the full xxl model on this device (device-local arena copies), eight host threads, each
    replaying its own ~440-node hipGraph 50 times under one GIL with the process-wide set-up lock, an 8-clip batch sharded one
    clip per context.  Checks: every clip equals the single-context run of the same clip (bf16 mode: bit-identical - same
    tiles, same shapes), and the threaded run's wall time against the same eight clips run one after the other on ONE
    context - the difference per loop iteration is the host-side price of the eight concurrent launch streams (reported;
    gate: the threaded run may not be slower than the sequential one by more than 15 %)."""
    import time
    from foley_amd import nodes
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=False, sd=sd, device=dev)
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=cfg)
    del sd
    torch.cuda.empty_cache()
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    n = 8
    noise = sampler.draw_noise(n, 128, 250, torch.bfloat16, torch.Generator("cpu").manual_seed(1234))
    seq = []
    for rep in range(2):            # the first round captures the graph and warms the device up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = [sampler.denoise_process_with_generator(vis, txt, 5.0, model, dac, 4.5, 50, 1, "euler", noise=noise[i:i + 1])[0] for i in range(n)]
        torch.cuda.synchronize()
        t_seq = time.perf_counter() - t0
    reps = sampler.replicate(model, dac, [dev] * n)
    assert len({id(m) for m, _ in reps}) == n and model.last_broadcast_s == 0.0       # one device: local copies, no RCCL
    gen = lambda: torch.Generator("cpu").manual_seed(1234)
    t_multi = None
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        multi, _sr = sampler.denoise_process_multi(vis, txt, 5.0, reps, 4.5, 50, n, "euler", generator=gen())
        torch.cuda.synchronize()
        t_multi = time.perf_counter() - t0
    assert multi.shape == (n, 1, 240000)
    for i in range(n):
        assert torch.equal(multi[i], seq[i][0]), i
    per_it_us = 1e6 * (t_multi - t_seq) / 50
    print("8 contexts / 8 threads on one device: %.3f s; the same 8 clips sequentially on one context: %.3f s; "
          "difference per loop iteration %.0f us (8 concurrent ~440-node graph launches)" % (t_multi, t_seq, per_it_us))
    record_parity("eight_contexts_one_device", threaded_s=t_multi, sequential_s=t_seq, host_overhead_us_per_iteration=per_it_us)
    assert t_multi < 1.15 * t_seq


def test_replicas_share_the_sticky_text_bucket(tiny, dev):
    """The sticky text length is ONE value per model in the reference (utils.py:166-188).  A replica that sat out a
    long-prompt batch (empty shard) must still pad the next short prompt to 128 like the replica that saw it - otherwise clips
    of one batch are padded differently (text padding is unmasked) and differ from a single-GPU run."""
    import dataclasses
    sd, dsd, _model, _dac = tiny
    cfg128 = dataclasses.replace(C.TINY, text_len=128)          # the yaml's text_length caps the bucket (utils.py:95-99); 128 lets it trigger
    model = sampler.FoleyModel(cfg128, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    dac = sampler.FoleyDAC(dsd, dev, C.DAC_TINY)
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    long_txt = {"text_feat": synth.synth_tensor("t.long", (1, 90, 768), 1.0), "uncond_text_feat": cond["uncond_text"]}
    short_txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    reps = sampler.replicate(model, dac, [dev, dev])
    sampler.denoise_process_multi(vis, long_txt, 1.0, reps, 4.5, 4, 1, "euler", generator=torch.Generator("cpu").manual_seed(3))   # replica 1 idle
    assert [m._text_len_fixed for m, _ in reps] == [128, 128]
    multi, _sr = sampler.denoise_process_multi(vis, short_txt, 1.0, reps, 4.5, 4, 2, "euler", generator=torch.Generator("cpu").manual_seed(3))
    single, _sr = sampler.denoise_process_with_generator(vis, short_txt, 1.0, model, dac, 4.5, 4, 2, "euler",
                                                          generator=torch.Generator("cpu").manual_seed(3))
    assert model._text_len_fixed == 128 and rel_err(multi, single) < 1e-5


def test_bcast_local_grouped_rccl_launch(dev):
    """foley_bcast_local (the in-process form of the single weight broadcast, used by sampler.replicate): ncclCommInitAll over
    every visible device + ONE grouped launch carrying two buffers per device.  On the 1-GPU boxes the communicator has one
    rank (RCCL resolution, communicator cache, group semantics and the in-place root call are what runs); with more devices
    every replica must hold the root's bytes afterwards."""
    from foley_amd.host import runtime as rt
    n = torch.cuda.device_count()
    g = torch.Generator().manual_seed(3)
    a0 = torch.randint(0, 255, (3_000_001,), dtype=torch.uint8, generator=g).to(dev)
    b0 = torch.randint(0, 255, (4097,), dtype=torch.uint8, generator=g).to(dev)
    per_dev = [[a0, b0]] + [[torch.zeros_like(a0, device=f"cuda:{i}"), torch.zeros_like(b0, device=f"cuda:{i}")] for i in range(1, n)]
    want_a, want_b = a0.cpu(), b0.cpu()
    for _ in range(2):                                    # the second call takes the cached communicators
        secs = rt.bcast_local(per_dev)
        assert secs >= 0.0
        for bufs in per_dev:
            assert torch.equal(bufs[0].cpu(), want_a) and torch.equal(bufs[1].cpu(), want_b)


def test_bench_two_ranks_over_rccl(dev):
    """The N > 1 path on real hardware, when the box has it: `bench.py --gpus 2` spawns its own two ranks (one per
    GPU), rank 0 packs into the bundle, ONE ncclBroadcast over xGMI ships it, every rank samples its own clips.
    Skips on a 1-GPU box (the driver's 8-GPU scaling run is then the only hardware evidence)."""
    import json, os, subprocess, sys
    from conftest import ROOT
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c4", "--model", "tiny",
                        "--duration", "1", "--bs", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-extra"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["config"]["collectives"] == 1 and out["config"]["clips_per_gpu"] == 2
    assert out["config"]["workload"].startswith("c4") and out["value"] > 0 and out["config"]["broadcast_s"] > 0


def test_bench_two_ranks_sharing_one_gpu(dev):
    """The spawner + two concurrently sampling ranks on real hardware when only one GPU is visible: both ranks sit on
    cuda:0 (FOLEY_BENCH_SHARE_DEVICE), the bundle travels by ONE gloo broadcast of the device buffer, the timing
    all-reduce / barriers run as in the RCCL job.  Everything but RCCL itself (covered at world 1 above and by
    test_bench_two_ranks_over_rccl on a multi-GPU box)."""
    import json, os, subprocess, sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["FOLEY_BENCH_SHARE_DEVICE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--config", "c4",
                        "--model", "tiny", "--duration", "1", "--bs", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                        "--no-extra", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["config"]["collectives"] == 1 and out["config"]["clips_per_gpu"] == 2
    assert out["config"]["workload"].startswith("c4") and out["value"] > 0 and out["config"]["broadcast_s"] > 0
    # the per-rank evidence of a multi-rank line: the communicator's size and every rank's own record, all-gathered
    ranks = out["config"]["ranks"]
    assert out["config"]["rccl_nranks"] == 2 and out["config"]["backend"] == "gloo"
    assert [r_["rank"] for r_ in ranks] == [0, 1] and [r_["shard"] for r_ in ranks] == [[0, 2], [2, 4]]
    assert all(r_["clips"] == 2 and r_["pass_ms"] > 0 and r_["loop_ms"] > 0 and r_["uuid"] for r_ in ranks)


def test_v2a_node_with_image_input(dev):
    """The reference's example workflow wires a VHS IMAGE batch into the sampler (link 114): the node
    must EXECUTE with an IMAGE input - frame resampling, SigLIP2 / Synchformer / CLAP on the GPU, then the
    HIP sampler + DAC.  Encoders are small stand-ins / synthesised weights (no checkpoints in the image);
    the result is checked against the CPU oracle fed with features computed on the CPU in fp32."""
    from foley_amd import nodes
    from foley_amd.host import encoders as E
    from test_v2a_cpu import tiny_clap, tiny_siglip
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY)
    model = sampler.FoleyModel(c, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    tok, clap = tiny_clap()
    sync_sd = synth.materialize(E.synchformer_schema())
    deps = nodes.AttributeDict(dac_model=sampler.FoleyDAC(dsd, dev, C.DAC_TINY), siglip2_model=tiny_siglip(),
                               syncformer_model={k: v.clone() for k, v in sync_sd.items()}, clap_tokenizer=tok, clap_model=clap)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(30, 90, 120, 3, generator=g)                     # IMAGE [N,H,W,C] float 0-1: 30 frames at 24 fps
    kw = dict(frame_rate=24.0, duration=2.0, prompt="rain on a tin roof", negative_prompt="noisy, harsh", cfg_scale=4.5,
              steps=10, sampler="euler", batch_size=1, seed=55574, force_offload=False,
              torch_compile_cfg={"backend": "inductor"}, block_swap_args={"blocks_to_swap": 30}, image=image)
    first, batch = nodes.HunyuanFoleySampler().generate_audio(model, deps, **kw)
    assert batch["waveform"].shape == (1, 1, 2 * 48000) and first["sample_rate"] == 48000
    assert torch.isfinite(batch["waveform"]).all()
    # features as the node computed them (GPU: frames pre-processed on the device, both encoders on the HIP engine - SigLIP2 in
    # the model dtype, Synchformer with fp16 operands) vs an fp32 CPU evaluation through transformers / the torch restatement
    # (CPU uint8 resize: the GPU resize differs by a grey level on < 1 % of the pixels, hence 5e-3 on the SigLIP2 features)
    cpu_deps = nodes.AttributeDict(siglip2_model=tiny_siglip(), syncformer_model=sync_sd, clap_tokenizer=tok, clap_model=tiny_clap()[1])
    vis_c, txt_c, alen = nodes.HunyuanFoleySampler._video_features(image, 2.0, 24.0, kw["prompt"], kw["negative_prompt"],
                                                                   cpu_deps, torch.device("cpu"), torch.float32)
    vis_g, txt_g, alen_g = nodes.HunyuanFoleySampler._video_features(image, 2.0, 24.0, kw["prompt"], kw["negative_prompt"],
                                                                     deps, dev, torch.float32)
    assert alen == alen_g == 2.0 and vis_g["siglip2_feat"].shape == (1, 16, 768) and vis_g["syncformer_feat"].shape == (1, 40, 768)
    e_sig, e_syn = rel_err(vis_g["siglip2_feat"], vis_c["siglip2_feat"]), rel_err(vis_g["syncformer_feat"], vis_c["syncformer_feat"])
    print("node features GPU engine vs CPU: siglip2 %.2e, synchformer %.2e" % (e_sig, e_syn))
    assert e_sig < 5e-3
    assert e_syn < 2e-2      # fp16 operands, like the reference's fp16 autocast
    assert rel_err(txt_g["text_feat"], txt_c["text_feat"]) < 1e-3
    # the whole node against the oracle on the node's own (GPU) features: isolates the HIP sampler from encoder precision
    noise = torch.randn((1, 128, 100), generator=torch.Generator("cpu").manual_seed(55574), dtype=torch.float32)
    cond = {"text": txt_g["text_feat"].float().cpu(), "uncond_text": txt_g["uncond_text_feat"].float().cpu(),
            "clip": vis_g["siglip2_feat"].float().cpu(), "sync": vis_g["syncformer_feat"].float().cpu()}
    with torch.inference_mode():
        ref = O.sample_waveform(sd, dsd, c.heads, noise, cond, 10, 4.5, "euler", rates=C.DAC_TINY.rates)
    assert rel_err(batch["waveform"], ref) < 1e-3


def test_bf16_mode_against_reference_bf16(dev):
    """The benchmarked precision pinned to the REFERENCE's own bf16 execution (golden g12: parameters
    .to(bfloat16), inputs in the parameter dtype, torch.autocast(bfloat16), utils.py:222-234 - generated by
    running the reference on the build container's CPU).  bf16 arithmetic is not reproducible bit for bit
    across devices, so the gates are stated against the reference's own bf16-vs-fp32 distance d0 on the
    same inputs (stored in the fixture): the HIP bf16 mode must be as close to the reference's bf16 output
    as bf16 rounding allows (<= 1.5 d0; measured 0.94 - 1.02 d0: two correct
    bf16 executions of one computation differ by about d0) and no further from the fp32 truth than the reference's own bf16
    run is (<= 1.5 d0).  Tolerances: forward d0 = 7.0e-3; 10-step CFG latents d0 = 9.1e-3, waveform
    d0 = 4.0e-2; C5 (fp8-wrapped, 30 s shapes) gate 2.5e-2 against the fp8-wrapped reference."""
    from foley_amd import nodes
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY)
    g12, g5 = golden("g12_bf16_ref"), golden("g5_dit_tiny")
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "none", device=dev, cfg=c, dac_cfg=C.DAC_TINY)
    r16 = lambda t: t.to(torch.bfloat16).float()
    # ---- one forward on g5's inputs
    x, t, cond, clip, sync = (g5["a_" + k] for k in ("x", "t", "cond", "clip", "sync"))
    y = _forward(model, r16(x), t, r16(cond), r16(clip), r16(sync))
    d0 = rel_err(g12["fwd_y16"], g12["fwd_y32"])
    e16, e32 = rel_err(y, g12["fwd_y16"]), rel_err(y, g12["fwd_y32"])
    print("forward: d0 %.2e, vs reference bf16 %.2e, vs reference fp32 %.2e" % (d0, e16, e32))
    assert 5e-3 < d0 < 1e-2 and e16 < 1.5 * d0 and e32 < 1.5 * d0
    # ---- 10-step CFG 4.5 Euler run, bs 2, same seed -> same bf16 noise draw as the reference
    dac = sampler.FoleyDAC(dsd, dev, C.DAC_TINY)
    cnd = synth.synth_conditioning(c, 1.0, t2a=False, sd=sd)
    gen = torch.Generator("cpu").manual_seed(1234)
    audio, _sr, lat = sampler.denoise_process_with_generator(
        {"siglip2_feat": cnd["clip"], "syncformer_feat": cnd["sync"]},
        {"text_feat": cnd["text"], "uncond_text_feat": cnd["uncond_text"]}, 1.0, model, dac, 4.5, 10, 2, "euler",
        generator=gen, return_latents=True)
    gen = torch.Generator("cpu").manual_seed(1234)
    assert torch.equal(sampler.draw_noise(2, 128, 50, torch.bfloat16, gen).float(), g12["cfg_noise_b16"])
    dl = rel_err(g12["cfg_b16_latents"], g12["cfg_f32_latents"])
    dw = rel_err(g12["cfg_b16_wave_s5"], g12["cfg_f32_wave_s5"])
    el16, el32 = rel_err(lat, g12["cfg_b16_latents"]), rel_err(lat, g12["cfg_f32_latents"])
    ew16, ew32 = rel_err(audio[..., ::5], g12["cfg_b16_wave_s5"]), rel_err(audio[..., ::5], g12["cfg_f32_wave_s5"])
    print("10-step CFG: latents d0 %.2e (ours vs ref-bf16 %.2e, vs ref-fp32 %.2e); waveform d0 %.2e (%.2e, %.2e)"
          % (dl, el16, el32, dw, ew16, ew32))
    assert el16 < 1.5 * dl and el32 < 1.5 * dl and ew16 < 1.5 * dw and ew32 < 1.5 * dw
    # ---- C5 structure: fp8_e4m3fn storage + bf16 compute, 30 s shapes, the cond half of the CFG pair
    m8 = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16", "fp8_e4m3fn", device=dev, cfg=c)
    La, Lv, Ls = C.lengths(30.0, c)
    x5 = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(55))
    cn5 = synth.synth_conditioning(c, 30.0, t2a=True, sd=sd)
    text5 = sampler.pad_or_trim_text(cn5["text"], 77)
    y8 = _forward(m8, r16(x5), g12["c5_t"][1:], r16(text5), r16(cn5["clip"]), r16(cn5["sync"]))[..., ::8]
    e8 = rel_err(y8, g12["c5_y8"])
    d8 = rel_err(g12["c5_y8"], g12["c5_y32"])
    print("C5 shapes: ours(fp8+bf16) vs reference(fp8+bf16) %.2e; reference fp8-vs-fp32 %.2e, ours vs fp32 %.2e"
          % (e8, d8, rel_err(y8, g12["c5_y32"])))
    assert e8 < 2.5e-2 and rel_err(y8, g12["c5_y32"]) < 1.5 * d8
    assert rel_err(y8, g12["c5_y16"]) > e8          # the fp8-rounded weights are really what runs


def test_fp16_mode_against_reference_fp16(dev):
    """precision=fp16 computes in fp16 (v_mfma_f32_32x32x16_f16 instantiation of every 16-bit kernel), pinned to the
    REFERENCE's own fp16 execution (golden g13: parameters .to(float16), inputs in the parameter dtype,
    torch.autocast(float16) - nodes.py:89-106, utils.py:229-234 - run on the build container's CPU).  Gates as for
    bf16 (g12), against the reference's own fp16-vs-fp32 distance d0 on the same inputs: within 1.5 d0 of the
    reference's fp16 output and within 1.5 d0 of its fp32 output.  d0 is ~8x smaller than bf16's (8.8e-4 forward,
    1.2e-3 latents, 5.2e-3 waveform), so a run that silently took the bf16 kernels (d ~ 7e-3) fails these gates."""
    from foley_amd import nodes
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY)
    g13, g12, g5 = golden("g13_fp16_ref"), golden("g12_bf16_ref"), golden("g5_dit_tiny")
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "fp16", "none", device=dev, cfg=c, dac_cfg=C.DAC_TINY)
    assert model.dtype == torch.float16
    r16 = lambda t: t.to(torch.float16).float()
    x, t, cond, clip, sync = (g5["a_" + k] for k in ("x", "t", "cond", "clip", "sync"))
    y = _forward(model, r16(x), t, r16(cond), r16(clip), r16(sync))
    assert torch.equal(g13["fwd_y32"], g12["fwd_y32"])                       # same inputs as the bf16 fixture
    d0 = rel_err(g13["fwd_y16"], g13["fwd_y32"])
    e16, e32 = rel_err(y, g13["fwd_y16"]), rel_err(y, g13["fwd_y32"])
    print("forward: d0 %.2e, vs reference fp16 %.2e, vs reference fp32 %.2e" % (d0, e16, e32))
    assert 5e-4 < d0 < 2e-3 and e16 < 1.5 * d0 and e32 < 1.5 * d0
    dac = sampler.FoleyDAC(dsd, dev, C.DAC_TINY)
    cnd = synth.synth_conditioning(c, 1.0, t2a=False, sd=sd)
    gen = torch.Generator("cpu").manual_seed(1234)
    audio, _sr, lat = sampler.denoise_process_with_generator(
        {"siglip2_feat": cnd["clip"], "syncformer_feat": cnd["sync"]},
        {"text_feat": cnd["text"], "uncond_text_feat": cnd["uncond_text"]}, 1.0, model, dac, 4.5, 10, 2, "euler",
        generator=gen, return_latents=True)
    gen = torch.Generator("cpu").manual_seed(1234)
    assert torch.equal(sampler.draw_noise(2, 128, 50, torch.float16, gen).float(), g13["cfg_noise_f16"])
    dl = rel_err(g13["cfg_f16_latents"], g13["cfg_f32_latents"])
    dw = rel_err(g13["cfg_f16_wave_s5"], g13["cfg_f32_wave_s5"])
    el16, el32 = rel_err(lat, g13["cfg_f16_latents"]), rel_err(lat, g13["cfg_f32_latents"])
    ew16, ew32 = rel_err(audio[..., ::5], g13["cfg_f16_wave_s5"]), rel_err(audio[..., ::5], g13["cfg_f32_wave_s5"])
    print("10-step CFG: latents d0 %.2e (ours vs ref-fp16 %.2e, vs ref-fp32 %.2e); waveform d0 %.2e (%.2e, %.2e)"
          % (dl, el16, el32, dw, ew16, ew32))
    assert el16 < 1.5 * dl and el32 < 1.5 * dl and ew16 < 1.5 * dw and ew32 < 1.5 * dw
    # precision=auto on an fp16 checkpoint resolves to fp16 compute as well (utils.py:507-515)
    sd16 = {k: v.to(torch.float16) for k, v in sd.items()}
    m_auto = nodes.HunyuanModelLoader.pack_state_dict(sd16, "auto", "none", device=dev, cfg=c, dac_cfg=C.DAC_TINY)
    assert m_auto.dtype == torch.float16
    # fp8 weight storage under fp16 compute (quantization widget + precision=fp16): stays fp8 in the arena, widened to fp16
    # in registers; equals the same model with the fp8-rounded weights stored as fp16
    m8 = nodes.HunyuanModelLoader.pack_state_dict(sd, "fp16", "fp8_e4m3fn", device=dev, cfg=c, dac_cfg=C.DAC_TINY)
    assert m8.dtype == torch.float16 and m8.arena.view("t0.a_qkv.w").dtype == torch.float8_e4m3fn
    y8 = _forward(m8, r16(x), t, r16(cond), r16(clip), r16(sync))
    assert 1e-3 < rel_err(y8, y) < 0.2


def _legacy_wn(dsd):
    """The same DAC checkpoint spelled with legacy weight_g / weight_v keys, and fully folded."""
    g = {k.replace(".parametrizations.weight.original0", ".weight_g").replace(".parametrizations.weight.original1", ".weight_v"): v
         for k, v in dsd.items()}
    from foley_amd.host import packers
    folded = {k: v for k, v in dsd.items() if ".parametrizations." not in k}
    for k in dsd:
        if k.endswith(".parametrizations.weight.original0"):
            base = k[:-len(".parametrizations.weight.original0")]
            folded[base + ".weight"] = packers.fold_weight_norm(dsd, base)
    return g, folded


def test_reference_keyed_loader_matches_python_packers(dev):
    """foley_load_tensor (weights.hip): checkpoint tensors handed over under the REFERENCE's state-dict keys are packed
    on the device by the library.  Same arena content as host/packers.py: DiT forward and sampler latents
    bit-identical (fp32, bf16 and fp8-stored weights); DAC waveform to fp32 round-off (the weight-norm fold
    reduces in a different order).  All three weight-norm spellings, arbitrary tensor order, missing tensors."""
    from foley_amd import nodes
    from foley_amd.host import runtime as rt
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY, encoder=True)           # encoder keys must be ignored (returns 1)
    cond = synth.synth_conditioning(c, 1.0, t2a=False)
    visual = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    text = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}

    def run(model, dac):
        gen = torch.Generator("cpu").manual_seed(77)
        a, _sr, lat = sampler.denoise_process_with_generator(visual, text, 1.0, model, dac, 4.5, 6, 2, "heun-2", generator=gen,
                                                           return_latents=True)
        return a.cpu(), lat.cpu()

    dsd_g, dsd_folded = _legacy_wn(dsd)
    rev = lambda d: dict(reversed(list(d.items())))                       # loading order must not matter
    for dtype, quant, dac_sd in ((torch.float32, "none", dsd), (torch.bfloat16, "none", rev(dsd_g)),
                                 (torch.bfloat16, "fp8_e4m3fn", dsd_folded), (torch.bfloat16, "fp8_e5m2", dsd)):
        sdq = nodes.round_params(sd, dtype)
        if quant != "none":
            sdq = nodes.fp8_round_state_dict(sdq, quant, autocast=True, param_dtype=dtype)
        ref_model = sampler.FoleyModel(c, sdq, dtype, dev, dac_cfg=C.DAC_TINY, quantization=quant)
        ref_dac = sampler.FoleyDAC(dsd, dev, C.DAC_TINY)
        a0, l0 = run(ref_model, ref_dac)
        m = sampler.FoleyModel.from_reference_state(c, rev(sdq) if quant == "none" else sdq, dtype, dev, dac_sd,
                                                    dac_cfg=C.DAC_TINY, quantization=quant)
        a1, l1 = run(m, None)
        assert torch.equal(l0, l1), (dtype, quant)                          # identical packed DiT weights
        assert rel_err(a1, a0) < 1e-5, (dtype, quant)                       # DAC: fold order only
        ptr, nbytes = m.ctx.weights_arena()
        assert ptr % 256 == 0 and nbytes > 0
        if quant != "none":
            assert nbytes < 0.62 * sampler.FoleyModel(c, sdq, dtype, dev, dac_cfg=C.DAC_TINY).arena.buffer.numel() + \
                ref_dac.arena.buffer.numel()
    # a missing tensor is reported by name, never silently zero
    ctx = rt.FoleyContext(c, C.DAC_TINY, torch.float32, dev)
    part = {k: v for k, v in sd.items() if k != "single_blocks.1.linear2.w3.weight"}
    with pytest.raises(rt.FoleyRuntimeError, match="s1.w13"):
        ctx.load_reference_state([part, dsd], 0)
    bad = dict(sd)
    bad["triple_blocks.0.audio_mlp.fc1.weight"] = torch.zeros(7, 5)
    with pytest.raises(rt.FoleyRuntimeError, match="unexpected shape"):
        rt.FoleyContext(c, C.DAC_TINY, torch.float32, dev).load_reference_state([bad, dsd], 0)


def test_bcast_weights_on_a_real_rccl_communicator(dev):
    """foley_bcast_weights: ONE ncclBroadcast of the ctx-owned arena on the caller's ncclComm_t (here a 1-rank RCCL
    communicator created through the same librccl torch has loaded).  The arena is unchanged and usable."""
    import ctypes as CT, os
    c = C.TINY
    sd = synth.synth_dit_state_dict(c)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY)
    m = sampler.FoleyModel.from_reference_state(c, sd, torch.float32, dev, dsd, dac_cfg=C.DAC_TINY)
    torch.zeros(1, device=dev)
    rccl = CT.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), mode=CT.RTLD_GLOBAL)

    class UID(CT.Structure):
        _fields_ = [("internal", CT.c_char * 128)]
    uid, comm = UID(), CT.c_void_p()
    rccl.ncclGetUniqueId.argtypes = [CT.POINTER(UID)]
    rccl.ncclCommInitRank.argtypes = [CT.POINTER(CT.c_void_p), CT.c_int, UID, CT.c_int]
    rccl.ncclCommDestroy.argtypes = [CT.c_void_p]
    assert rccl.ncclGetUniqueId(CT.byref(uid)) == 0
    with torch.cuda.device(dev):
        assert rccl.ncclCommInitRank(CT.byref(comm), 1, uid, 0) == 0
    try:
        ptr, nbytes = m.ctx.weights_arena()
        before = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        CT.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(CT.c_void_p(before.data_ptr()), CT.c_void_p(ptr), CT.c_size_t(nbytes), 3)
        m.ctx.bcast_weights(comm.value, root=0)
        torch.cuda.synchronize()
        after = torch.empty_like(before)
        CT.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(CT.c_void_p(after.data_ptr()), CT.c_void_p(ptr), CT.c_size_t(nbytes), 3)
        assert torch.equal(before, after)
    finally:
        rccl.ncclCommDestroy(comm)
    g5 = golden("g5_dit_tiny")
    x, t, cond, clip, sync = (g5["a_" + k] for k in ("x", "t", "cond", "clip", "sync"))
    assert rel_err(_forward(m, x, t, cond, clip, sync), g5["a_y"]) < 2e-5
