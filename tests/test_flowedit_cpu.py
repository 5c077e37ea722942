"""FlowEdit without a GPU: the restated loop (tests/flowedit_ref.py) on an analytic velocity field where Euler is exact, the
mask's keep exactness, the noise table, the pair plan, and every refusal of the node and the sampler with its reason."""
import types

import pytest
import torch

import flowedit_ref as FR
from foley_amd import nodes
from foley_amd.host import audio_edit, config as C, sampler, tables
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- analytic transport
def _transport(mu_src, mu_tar, steps, shift=1.0):
    """v(z, sigma, c) = (z - mu_c) / sigma: the field that carries any z straight to mu_c at sigma = 0."""
    sig = O.flow_sigmas(steps, shift).double()
    return lambda z_src, z_tar, i: ((z_src - mu_src) / sig[i], (z_tar - mu_tar) / sig[i])


@pytest.mark.parametrize("steps", [2, 7, 10])
@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("rows", ["fresh", "fixed"])
def test_analytic_transport_is_exact_under_euler(steps, strength, rows):
    """With x_src = mu_src:  v_s = n - mu_src  and  v_t = (z - sigma mu_src + sigma n - mu_tar) / sigma,  so the difference is
    d = (z - mu_tar) / sigma whatever the noise: z - mu_tar = K sigma, linear in sigma, and an Euler step multiplies it by
    sigma_{k+1} / sigma_k exactly.  From z = mu_src at sigma_{k0}:
        z after the step to sigma_k  =  mu_tar + (mu_src - mu_tar) sigma_k / sigma_{k0}
    and the loop ends at sigma = 0 on mu_tar for any noise table, step count and strength."""
    g = torch.Generator().manual_seed(steps)
    V, Cc, L = 2, 6, 9
    mu_src, mu_tar = torch.randn(1, Cc, L, generator=g, dtype=torch.float64), torch.randn(1, Cc, L, generator=g, dtype=torch.float64)
    k0, i0 = tables.edit_start(steps, "euler", strength)
    noise = 5.0 * torch.randn(steps - i0 if rows == "fresh" else 1, V, Cc, L, generator=g, dtype=torch.float64)
    trace = []
    z = FR.restated_flowedit(_transport(mu_src, mu_tar, steps), mu_src, noise, steps, strength=strength, dtype=torch.float64, trace=trace)
    scale = float(mu_tar.norm())
    assert float((z - mu_tar).norm()) / scale <= 1e-10
    sig = O.flow_sigmas(steps).double()
    for j, zj in enumerate(trace):
        want = mu_tar + (mu_src - mu_tar) * sig[i0 + j + 1] / sig[k0]
        assert float((zj - want).norm()) / scale <= 1e-10, j


# ----------------------------------------------------------------------------- mask
def _any_field(z_src, z_tar, i):
    return torch.sin(3.0 * z_src) + 0.1 * i, torch.cos(2.0 * z_tar) - z_tar


def test_mask_of_zeros_returns_x_src_and_a_binary_mask_keeps_its_frames():
    g = torch.Generator().manual_seed(3)
    V, Cc, L, steps = 2, 8, 20, 6
    x_src = torch.randn(V, Cc, L, generator=g)
    noise = torch.randn(steps, V, Cc, L, generator=g)
    assert torch.equal(FR.restated_flowedit(_any_field, x_src, noise, steps, mask=torch.zeros(L)), x_src)
    m = (torch.rand(V, L, generator=g) > 0.5).float()
    z = FR.restated_flowedit(_any_field, x_src, noise, steps, mask=m)
    free = FR.restated_flowedit(_any_field, x_src, noise, steps)
    keep = (m == 0).view(V, 1, L).expand(V, Cc, L)
    assert torch.equal(z[keep], x_src[keep]) and not torch.equal(z[~keep], x_src[~keep])
    assert not torch.equal(free[keep], x_src[keep])


def test_step_reference_keeps_masked_frames_and_takes_the_unmasked_update():
    g = torch.Generator().manual_seed(4)
    V, Cc, L = 2, 8, 12
    z, x_src, n = (torch.randn(V, Cc, L, generator=g) for _ in range(3))
    pred = torch.randn(4 * V * L, Cc, generator=g)
    row = tables.edit_solver_table(tables.sigma_grid(6), "euler", 6)[2]
    m = (torch.rand(L, generator=g) > 0.5).float()
    zm, zs, zt = FR.ref_flowedit_step(pred, z, x_src, n, m, row, 2.0, 4.5)
    zu, _s, _t = FR.ref_flowedit_step(pred, z, x_src, n, None, row, 2.0, 4.5)
    assert torch.equal(zm[..., m == 0], z[..., m == 0]) and torch.equal(zm[..., m == 1], zu[..., m == 1])
    s = float(row[5])
    assert float((zs - ((1 - s) * x_src + s * n)).abs().max()) < 1e-6 and torch.equal(zt, (zm - x_src) + zs)
    zs2, zt2 = FR.ref_inputs(x_src, x_src, n, 0.4)
    assert torch.equal(zs2, zt2)                                       # z == x_src: the branches start equal
    assert FR.rows_of(zs, zt).shape == (4 * V * L, Cc)


# ----------------------------------------------------------------------------- noise table, spec
def test_flowedit_noise_is_one_draw():
    a = audio_edit.flowedit_noise(torch.Generator("cpu").manual_seed(9), 7, 2, 128, 50, torch.float32)
    b = torch.randn((7, 2, 128, 50), generator=torch.Generator("cpu").manual_seed(9))
    assert torch.equal(a, b) and a.dtype == torch.float32
    h = audio_edit.flowedit_noise(torch.Generator("cpu").manual_seed(9), 1, 2, 128, 50, torch.bfloat16)
    assert torch.equal(h, torch.randn((1, 2, 128, 50), generator=torch.Generator("cpu").manual_seed(9), dtype=torch.bfloat16))
    x0 = torch.zeros(1, 128, 50)
    assert audio_edit.FlowEditSpec(x0, noise="fixed").n_rows(10) == 1 and audio_edit.FlowEditSpec(x0).n_rows(10) == 10
    spec = audio_edit.FlowEditSpec(x0)
    assert spec.source_scale == 2.0 and spec.noise == "fresh" and spec.strength == 1.0 and spec.mask is None


@pytest.mark.parametrize("kw,scale,solver,match", [
    ({}, 4.5, "heun-2", "euler"), ({}, 1.0, "euler", "cfg_scale"), ({"source_scale": 1.0}, 4.5, "euler", "source_cfg_scale"),
    ({"source_scale": float("inf")}, 4.5, "euler", "source_cfg_scale"), ({"noise": "new"}, 4.5, "euler", "edit_noise")])
def test_spec_refusals(kw, scale, solver, match):
    with pytest.raises(ValueError, match=match):
        audio_edit.FlowEditSpec(torch.zeros(1, 128, 50), **kw).check(solver, scale)


# ----------------------------------------------------------------------------- the pair plan
def _cpu_model():
    cfg = C.TINY
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, quantization="none", _text_len_fixed=None,
                                 empty_clip_feat=torch.ones(cfg.clip_dim), empty_sync_feat=torch.ones(cfg.sync_dim),
                                 get_empty_clip_sequence=lambda bs, len: torch.ones(bs, len, cfg.clip_dim),
                                 get_empty_sync_sequence=lambda bs, len: torch.ones(bs, len, cfg.sync_dim))


def _feats(cfg, same=False):
    g = torch.Generator().manual_seed(1)
    vis = {"siglip2_feat": torch.randn(1, 8, cfg.clip_dim, generator=g), "syncformer_feat": torch.randn(1, 24, cfg.sync_dim, generator=g)}
    src = torch.randn(1, 5, cfg.cond_dim, generator=g)
    txt = {"source_text_feat": src, "text_feat": src.clone() if same else torch.randn(1, 7, cfg.cond_dim, generator=g),
           "uncond_text_feat": torch.randn(1, 4, cfg.cond_dim, generator=g)}
    return vis, txt


def test_pair_plan_of_three_variations():
    model = _cpu_model()
    vis, txt = _feats(model.cfg)
    v2, t2 = sampler.flowedit_features(vis, txt, 3)
    assert t2["text_feat"].shape[0] == 6 and torch.equal(t2["text_feat"][0], t2["text_feat"][2])
    assert torch.equal(t2["text_feat"][3, :7], txt["text_feat"][0]) and torch.equal(t2["text_feat"][0, :5], txt["source_text_feat"][0])
    plan = sampler.build_plan(model, v2, t2, 50, 4.5, 10, 6, "euler", edit_i0=4)
    assert plan["clips"] == 6 and plan["ncfg"] == 2 and plan["n_iter"] == 6
    assert plan["text_of"] == [0] * 6 + [1] * 3 + [2] * 3
    assert plan["vis_of"] == [0] * 6 + [1] * 6 and plan["clip"].shape[0] == 2              # shared visual sets, one per half
    assert all(int(f) & tables.STEP_BLEND for f in plan["solver_coef"][:, 4])
    # equal prompts: every clip shares its conditioning, the plan is the batch-1 plan of six clips
    v2, t2 = sampler.flowedit_features(*_feats(model.cfg, same=True), 3)
    assert sampler.build_plan(model, v2, t2, 50, 4.5, 10, 6, "euler", edit_i0=0)["text_of"] is None
    with pytest.raises(ValueError, match="source_text_feat"):
        sampler.flowedit_features(vis, {k: v for k, v in txt.items() if k != "source_text_feat"}, 3)
    with pytest.raises(ValueError, match="batch 1"):
        sampler.flowedit_features(vis, dict(txt, text_feat=txt["text_feat"].repeat(3, 1, 1)), 3)


def test_sampler_refuses_options_and_sharding():
    spec = audio_edit.FlowEditSpec(torch.zeros(1, 128, 50))
    for kw in ({"multistep": sampler.MultistepSpec(2)}, {"guidance": sampler.GuidanceSpec(rescale=0.5)}, {"noise": torch.zeros(2, 128, 50)},
               {"step_cache": sampler.StepCacheSpec(threshold=0.2)}):
        with pytest.raises(ValueError, match="FlowEdit"):
            sampler.denoise_process_with_generator({}, {}, 1.0, None, None, 4.5, 10, 2, "euler", edit=spec, **kw)
    with pytest.raises(ValueError, match="one device"):
        sampler.denoise_process_multi({}, {}, 1.0, [(None, None)], 4.5, 10, 2, "euler", edit=spec)


# ----------------------------------------------------------------------------- node
def _fake_model_dac():
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None,
                                  get_empty_clip_sequence=lambda bs, len: torch.zeros(bs, len, 768),
                                  get_empty_sync_sequence=lambda bs, len: torch.zeros(bs, len, 768))
    dac = types.SimpleNamespace(has_encoder=True, cfg=C.DAC48K, sample_rate=48000)
    return model, dac


def _audio(seconds, sr=48000):
    return {"waveform": 0.1 * torch.randn(1, 2, int(seconds * sr), generator=torch.Generator().manual_seed(2)), "sample_rate": sr}


def _node_call(monkeypatch, encoders_ok=True, **kw):
    model, dac = _fake_model_dac()
    seen = {"clap": []}

    def fake(visual, text, secs, m, d, **k):
        seen.update(k)
        seen["text"] = text
        return torch.zeros(k["batch_size"], 1, 960), 48000

    def clap(prompts, deps, device, dtype=None):
        assert encoders_ok, "the refusal must come before the encoders run"
        seen["clap"].append(list(prompts))
        return torch.arange(len(prompts), dtype=torch.float32).view(-1, 1, 1).expand(-1, 5, 768).contiguous()

    def encode(w, m, d, La):
        assert encoders_ok, "the refusal must come before the encoders run"
        return torch.full((w.shape[0], 128, La), 0.25)
    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake)
    monkeypatch.setattr(sampler, "denoise_process_multi", fake)
    monkeypatch.setattr(nodes, "encode_text_feat", clap)
    monkeypatch.setattr(audio_edit, "encode_source", encode)
    args = dict(sampler="euler", cfg_scale=4.5, duration=5.0)
    args.update({k: kw.pop(k) for k in list(kw) if k in args})
    out = nodes.HunyuanFoleySampler().generate_audio(model, {"dac_model": dac}, 16, args["duration"], "snow", "noisy", args["cfg_scale"], 10,
                                                     args["sampler"], 2, 0, True, **kw)
    return out, seen


def test_node_builds_the_flowedit_call(monkeypatch):
    out, seen = _node_call(monkeypatch, audio=_audio(5.0), source_prompt="gravel", strength=0.6, regenerate=[(2.0, 3.0)],
                           crossfade_s=0.1, source_cfg_scale=2.5, edit_noise="fixed", loudness_lufs=None)
    assert seen["clap"] == [["noisy", "gravel", "snow"]]                     # one CLAP call: [negative, source, target]
    t = seen["text"]
    assert float(t["uncond_text_feat"].mean()) == 0.0 and float(t["source_text_feat"].mean()) == 1.0 and float(t["text_feat"].mean()) == 2.0
    assert all(v.shape[0] == 1 for v in t.values())
    e = seen["edit"]
    assert isinstance(e, audio_edit.FlowEditSpec) and e.strength == 0.6 and e.source_scale == 2.5 and e.noise == "fixed"
    assert torch.equal(e.mask, audio_edit.build_mask(250, [(2.0, 3.0)], 0.1)) and e.x0.shape == (1, 128, 250)
    assert seen["guidance_scale"] == 4.5 and seen["sampler"] == "euler" and seen["batch_size"] == 2
    assert out[1]["waveform"].shape == (2, 1, 960)
    _out, seen = _node_call(monkeypatch, audio=_audio(5.0), source_prompt="gravel")
    assert seen["edit"].mask is None and seen["edit"].noise == "fresh" and seen["edit"].source_scale == 2.0
    _out, seen = _node_call(monkeypatch)                                      # unset: the call as it was
    assert seen["edit"] is None and seen["clap"] == [["noisy", "snow"]] and "source_text_feat" not in seen["text"]


@pytest.mark.parametrize("kw,match", [
    ({"audio": None}, "audio="),
    ({"sampler": "heun-2"}, "euler"),
    ({"cfg_scale": 1.0}, "cfg_scale"),
    ({"source_cfg_scale": 1.0}, "source_cfg_scale"),
    ({"edit_noise": "white"}, "edit_noise"),
    ({"window_s": 4}, "window_s"),
    ({"prompts": ["a", "b"]}, "prompts"),
    ({"negative_prompts": ["a", "b"]}, "negative_prompts"),
    ({"images": [None, None]}, "images"),
    ({"features": {}}, "features"),
    ({"prompt_timeline": [(0.0, 1.0, "x")]}, "prompt_timeline"),
    ({"video_cfg_scale": 2.0}, "video_cfg_scale"),
    ({"guidance_interval": (0.0, 0.5)}, "guidance_interval"),
    ({"cfg_rescale": 0.5}, "cfg_rescale"),
    ({"guidance_mode": "apg"}, "guidance_mode"),
    ({"multistep_order": 2}, "multistep_order"),
    ({"cache_threshold": 0.2}, "cache_threshold"),
    ({"cache_skip": [2]}, "cache_skip"),
    ({"cache_interval": (0.0, 0.5)}, "cache_interval"),
    ({"cache_max_consecutive": 2}, "cache_max_consecutive"),
    ({"duration": 6.0}, "longer than the input audio"),
])
def test_node_refusals_come_before_the_encoders(monkeypatch, kw, match):
    call = {"audio": _audio(5.0), "source_prompt": "gravel"}
    call.update(kw)
    with pytest.raises(ValueError, match=match):
        _node_call(monkeypatch, encoders_ok=False, **call)


def test_node_refuses_flowedit_options_without_a_source_prompt(monkeypatch):
    for kw in ({"source_cfg_scale": 3.0}, {"edit_noise": "fixed"}):
        with pytest.raises(ValueError, match="pass source_prompt"):
            _node_call(monkeypatch, encoders_ok=False, audio=_audio(5.0), **kw)


def test_prepare_edit_refuses_a_clip_longer_than_the_source(monkeypatch):
    model, dac = _fake_model_dac()
    monkeypatch.setattr(audio_edit, "encode_source", lambda w, m, d, La: torch.zeros(w.shape[0], 128, La))
    with pytest.raises(ValueError, match="longer than the input audio"):
        audio_edit.prepare_edit(_audio(4.0), model, dac, 5.0, 10, "euler", 1, flowedit={"source_scale": 2.0, "noise": "fresh"})
    e = audio_edit.prepare_edit(_audio(5.0), model, dac, 5.0, 10, "euler", 1, strength=0.5, flowedit={"source_scale": 3.0, "noise": "fixed"})
    assert isinstance(e, audio_edit.FlowEditSpec) and e.mask is None and e.source_scale == 3.0 and e.noise == "fixed" and e.strength == 0.5


def test_node_sockets_stay_the_references():
    it = nodes.HunyuanFoleySampler.INPUT_TYPES()
    names = set(it["required"]) | set(it.get("optional", {}))
    assert not names & {"source_prompt", "source_cfg_scale", "edit_noise"}
    assert len(nodes.NODE_CLASS_MAPPINGS) == 6
