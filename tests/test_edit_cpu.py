"""Audio editing without a GPU: the strength -> (k0, i0) rule, the suffix / blend tables, mask building, the refusals, the
node's keyword plumbing, and the edit of the restated loop (tests/loop_ref.py) that tests/test_edit_gpu.py compares against."""
import contextlib
import types

import pytest
import torch

import loop_ref as L
from conftest import rel_err
from foley_amd import nodes
from foley_amd.host import audio_edit, config as C, sampler, synth, tables
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- restatement of the masked loop
@pytest.fixture(scope="module")
def tiny_cpu():
    """The arguments of loop_ref.restated_loop up to the noise, the conditioning's four tensors, x0."""
    sd = synth.synth_dit_state_dict(C.TINY)
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(2, 128, 50, generator=g)
    x0 = 0.7 * torch.randn(1, 128, 50, generator=g)
    return (sd, C.TINY.heads, noise), (cond["text"], cond["uncond_text"], cond["clip"], cond["sync"]), x0


def test_restatement_all_ones_at_strength_1_is_the_plain_loop(tiny_cpu):
    a, c, x0 = tiny_cpu
    for solver, steps in (("euler", 6), ("heun-2", 6)):
        ref = O.sample_latents(*a, *c, steps, 4.5, solver)
        ed = L.restated_loop(*a, *c, steps, 4.5, solver, edit=(x0, torch.ones(50), 1.0)).x
        assert torch.equal(ed, ref), solver


def test_restatement_all_zeros_under_euler_ends_at_x0(tiny_cpu):
    a, c, x0 = tiny_cpu
    for strength in (1.0, 0.5):
        ed = L.restated_loop(*a, *c, 6, 4.5, "euler", edit=(x0, torch.zeros(50), strength)).x
        assert torch.equal(ed, x0.expand_as(ed)), strength
    # a span regenerates its frames and keeps the others at x0
    m = audio_edit.build_mask(50, [(0.4, 0.6)], 0.0)
    ed = L.restated_loop(*a, *c, 6, 4.5, "euler", edit=(x0, m, 0.6)).x
    keep = m == 0
    assert torch.equal(ed[..., keep], x0[..., keep].expand(2, -1, -1)) and rel_err(ed[..., ~keep], x0[..., ~keep].expand(2, -1, -1)) > 1e-3


# ----------------------------------------------------------------------------- strength rule and tables
@pytest.mark.parametrize("solver,steps,strength,expect", [
    ("euler", 10, 1.0, (0, 0)), ("euler", 10, 0.6, (4, 4)), ("euler", 10, 0.35, (7, 7)), ("euler", 50, 0.999, (1, 1)),
    ("heun-2", 10, 1.0, (0, 0)), ("heun-2", 10, 0.6, (2, 4)), ("heun-2", 11, 0.5, (3, 6)), ("heun-2", 11, 1.0, (0, 0)),
    ("midpoint-2", 12, 0.5, (3, 6)), ("midpoint-2", 13, 0.3, (5, 10)),
    ("kutta-4", 12, 1.0, (0, 0)), ("kutta-4", 12, 0.5, (2, 8)), ("kutta-4", 14, 0.7, (1, 4)), ("kutta-4", 15, 0.34, (2, 8))])
def test_edit_start_rule(solver, steps, strength, expect):
    assert tables.edit_start(steps, solver, strength) == expect


@pytest.mark.parametrize("solver,steps,strength", [("euler", 10, 0.05), ("heun-2", 10, 0.19), ("kutta-4", 12, 0.3),
                                                   ("kutta-4", 3, 1.0), ("euler", 10, 0.0), ("euler", 10, 1.5),
                                                   ("euler", 10, -0.5), ("rk9", 10, 1.0)])
def test_edit_start_refusals(solver, steps, strength):
    with pytest.raises(ValueError):
        tables.edit_start(steps, solver, strength)


def _advances(solver, steps):
    """Iterations after which SolverState moves its sigma index (a real step ends), via the oracle's own state machine."""
    sig = O.flow_sigmas(steps)
    st = O.SolverState(sig, solver)
    x = torch.zeros(1)
    out = []
    for i in range(steps):
        k = st.idx
        x = st.step(torch.zeros(1), x)
        if st.idx != k:
            out.append((i, st.idx))
    return out


@pytest.mark.parametrize("solver", tables.SOLVERS)
@pytest.mark.parametrize("steps", [10, 11, 12])
def test_edit_tables_are_the_plain_suffix_with_blend_rows(solver, steps):
    plain_before = tables.solver_table(tables.sigma_grid(steps), solver, steps).clone()
    plain = tables.build_tables(50, 8, 24, 77, steps, solver, 1.0)
    assert torch.equal(plain["solver_coef"], plain_before)
    assert float(plain["solver_coef"][:, 5:].abs().max()) == 0.0
    assert all(int(f) & tables.STEP_BLEND == 0 for f in plain["solver_coef"][:, 4])
    sig = tables.sigma_grid(steps)
    adv = dict(_advances(solver, steps))
    stages = tables.SOLVER_STAGES[solver]
    for strength in (1.0, 0.6, 0.5):
        try:
            k0, i0 = tables.edit_start(steps, solver, strength)
        except ValueError:
            continue
        ed = tables.build_tables(50, 8, 24, 77, steps, solver, 1.0, edit_i0=i0)
        assert i0 == k0 * stages and ed["solver_coef"].shape == (steps - i0, 8)
        assert torch.equal(ed["t_feat"], plain["t_feat"][i0:])
        for key in ("rope_cos", "pos_audio_self", "sync_gather"):
            assert torch.equal(ed[key], plain[key])
        pc, ec = plain["solver_coef"][i0:], ed["solver_coef"]
        assert torch.equal(ec[:, :4], pc[:, :4]) and float(ec[:, 6:].abs().max()) == 0.0
        for j in range(ec.shape[0]):
            i, f = i0 + j, int(ec[j, 4])
            assert f & ~tables.STEP_BLEND == int(pc[j, 4])
            if i in adv:
                assert f & tables.STEP_BLEND and float(ec[j, 5]) == float(sig[adv[i]]), (i, adv[i])
            else:
                assert not f & tables.STEP_BLEND and float(ec[j, 5]) == 0.0
    # building the edit tables left the plain ones as they were
    assert torch.equal(tables.solver_table(tables.sigma_grid(steps), solver, steps), plain_before)


def test_build_plan_cache_keys_on_the_edit():
    """The device-table cache of build_plan keys on i0 and the blend: a plain plan after an edit plan of the same shape gets
    the plain tables back (and vice versa)."""
    cfg = C.TINY
    model = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, quantization="none", _text_len_fixed=None,
                                  get_empty_clip_sequence=lambda bs, len: torch.zeros(bs, len, cfg.clip_dim),
                                  get_empty_sync_sequence=lambda bs, len: torch.zeros(bs, len, cfg.sync_dim))
    vis = {"siglip2_feat": torch.zeros(1, 8, cfg.clip_dim), "syncformer_feat": torch.zeros(1, 24, cfg.sync_dim)}
    txt = {"text_feat": torch.zeros(1, 5, cfg.cond_dim), "uncond_text_feat": torch.zeros(1, 5, cfg.cond_dim)}
    p0 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "heun-2")
    p1 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "heun-2", edit_i0=0)
    p2 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "heun-2", edit_i0=4)
    p3 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "heun-2")
    assert p0["n_iter"] == p1["n_iter"] == 10 and p2["n_iter"] == 6
    assert torch.equal(p3["solver_coef"], p0["solver_coef"]) and not torch.equal(p1["solver_coef"], p0["solver_coef"])
    assert torch.equal(p2["solver_coef"], p1["solver_coef"][4:]) and torch.equal(p2["t_feat"], p0["t_feat"][4:])


# ----------------------------------------------------------------------------- masks
def test_mask_spans_to_frames():
    m = audio_edit.build_mask(250, [(2.0, 3.0)], 0.0)
    assert m.dtype == torch.float32 and m.shape == (250,)
    assert torch.equal(m.nonzero().flatten(), torch.arange(100, 150))
    assert torch.equal(audio_edit.build_mask(250), torch.ones(250))
    assert torch.equal(audio_edit.build_mask(250, None, 0.3), torch.ones(250))


def test_mask_crossfade_ramps():
    m = audio_edit.build_mask(250, [(2.0, 3.0)], 0.1)
    assert torch.equal(m[100:150], torch.ones(50))
    up = m[95:100].double()
    assert torch.allclose(up, torch.tensor([0.1, 0.3, 0.5, 0.7, 0.9], dtype=torch.float64), atol=1e-6)
    assert torch.allclose(m[150:155].double(), up.flip(0), atol=1e-6)
    assert float(m[:95].abs().max()) == 0.0 and float(m[155:].abs().max()) == 0.0


def test_mask_overlapping_spans_and_clamping():
    m = audio_edit.build_mask(250, [(1.0, 2.0), (1.5, 2.5)], 0.0)
    assert torch.equal(m.nonzero().flatten(), torch.arange(50, 125))
    m = audio_edit.build_mask(250, [(1.0, 1.5), (1.4, 1.45)], 0.2)     # a span inside another one's support: the larger value
    assert torch.equal(m, audio_edit.build_mask(250, [(1.0, 1.5)], 0.2))
    m = audio_edit.build_mask(250, [(-1.0, 0.5), (4.5, 9.0)], 0.1)       # clamped at both ends of the clip
    assert torch.equal(m[:25], torch.ones(25)) and torch.equal(m[225:], torch.ones(25))
    assert float(m[30:220].abs().max()) == 0.0 and 0 < float(m[26]) < 1


def test_mask_extension_tail():
    m = audio_edit.build_mask(250, [(1.0, 1.2)], 0.0, src_frames=200)
    assert torch.equal(m[200:], torch.ones(50)) and torch.equal(m[50:60], torch.ones(10))
    assert float(m[60:200].abs().max()) == 0.0
    assert torch.equal(audio_edit.build_mask(250, None, 0.1, src_frames=100), torch.ones(250))


@pytest.mark.parametrize("spans", [[(2.0, 2.0)], [(3.0, 2.0)], [(6.0, 7.0)], [(-2.0, 0.0)]])
def test_mask_refuses_empty_or_outside_spans(spans):
    with pytest.raises(ValueError):
        audio_edit.build_mask(250, spans, 0.1)
    with pytest.raises(ValueError):
        audio_edit.build_mask(250, [(1.0, 2.0)], -0.1)


# ----------------------------------------------------------------------------- refusals and node plumbing
def _fake_model_dac(has_encoder=True):
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
    dac = types.SimpleNamespace(has_encoder=has_encoder, cfg=C.DAC48K, sample_rate=48000)
    return model, dac


def _audio(seconds, batch=1, channels=2, sr=48000):
    return {"waveform": 0.1 * torch.randn(batch, channels, int(seconds * sr), generator=torch.Generator().manual_seed(2)),
            "sample_rate": sr}


def test_prepare_edit_refusals(monkeypatch):
    model, dac = _fake_model_dac()
    monkeypatch.setattr(audio_edit, "encode_source", lambda w, m, d, La: torch.zeros(w.shape[0], 128, La))
    with pytest.raises(RuntimeError, match="full VAE checkpoint"):
        audio_edit.prepare_edit(_audio(5.0), model, _fake_model_dac(False)[1], 5.0, 10, "euler", 1)
    with pytest.raises(RuntimeError, match="full VAE checkpoint"):
        audio_edit.prepare_edit(_audio(5.0), model, None, 5.0, 10, "euler", 1)
    with pytest.raises(ValueError, match="strength 1.0"):
        audio_edit.prepare_edit(_audio(4.0), model, dac, 5.0, 10, "euler", 1, strength=0.5)
    with pytest.raises(ValueError, match="empty"):
        audio_edit.prepare_edit(_audio(5.0), model, dac, 5.0, 10, "euler", 1, regenerate=[(2.0, 1.0)])
    with pytest.raises(ValueError, match="batch"):
        audio_edit.prepare_edit(_audio(5.0, batch=2), model, dac, 5.0, 10, "euler", 3)
    with pytest.raises(ValueError):
        audio_edit.prepare_edit(_audio(5.0), model, dac, 5.0, 10, "euler", 1, strength=0.05)
    # accepted: extension at strength 1 (tail regenerated), a per-clip batch, a downmix of the channels
    e = audio_edit.prepare_edit(_audio(4.0), model, dac, 5.0, 10, "euler", 1, regenerate=[(1.0, 2.0)], crossfade_s=0.0)
    assert torch.equal(e.mask[200:], torch.ones(50)) and torch.equal(e.mask[50:100], torch.ones(50)) and e.strength == 1.0
    e = audio_edit.prepare_edit(_audio(5.0, batch=3), model, dac, 5.0, 10, "euler", 3, strength=0.4)
    assert e.x0.shape == (3, 128, 250) and torch.equal(e.mask, torch.ones(250))


def test_prepare_waveform_downmix_and_trim(monkeypatch):
    model, dac = _fake_model_dac()
    a = _audio(5.5, channels=2)
    w = audio_edit.prepare_waveform(a, model, dac)
    assert torch.equal(w, a["waveform"].mean(dim=1))
    seen = {}

    def enc(x):
        seen["x"] = x
        return torch.zeros(x.shape[0], 256, x.shape[2] // 960)
    model.ctx = types.SimpleNamespace(dac_encode=enc)
    model.attach_dac = lambda d: None
    x0 = audio_edit.encode_source(w, model, dac, 250)
    assert x0.shape == (1, 128, 250) and torch.equal(seen["x"][:, 0], w[:, :240000])
    audio_edit.encode_source(w[:, :1000], model, dac, 250)                 # zero-padded to La * hop
    assert seen["x"].shape == (1, 1, 240000)


def test_edit_spec_shards_per_clip_operands():
    x0, mask = torch.randn(4, 128, 50), torch.rand(4, 50)
    e = audio_edit.EditSpec(x0, 0.5, mask)
    s = e.shard(1, 3, 4)
    assert torch.equal(s.x0, x0[1:3]) and torch.equal(s.mask, mask[1:3]) and s.strength == 0.5
    shared = audio_edit.EditSpec(x0[:1], 1.0, mask[0]).shard(2, 4, 4)
    assert torch.equal(shared.x0, x0[:1]) and torch.equal(shared.mask, mask[0])
    with pytest.raises(RuntimeError):
        audio_edit.EditSpec(torch.zeros(2, 128, 50)).device_operands("cpu", 3, 50)
    with pytest.raises(RuntimeError):
        audio_edit.EditSpec(torch.zeros(1, 128, 50), 1.0, torch.zeros(2, 50)).device_operands("cpu", 3, 50)


def test_denoise_process_multi_shards_the_edit(monkeypatch):
    class _Stream:
        def __init__(self, *_a, **_k): pass
        def wait_event(self, _ev): pass
        def synchronize(self): pass
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "device", lambda _d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda _s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *_a: _Stream())
    cfg = types.SimpleNamespace(frame_rate=50, text_len=128, latent_dim=128)
    reps = [(types.SimpleNamespace(cfg=cfg, dtype=torch.float32, device=torch.device("cpu"), _text_len_fixed=None, rank=r), None)
            for r in range(2)]
    got = {}

    def fake(visual, text, secs, model, dac, cfg_scale, steps, bs, solver, **kw):
        got[model.rank] = kw["edit"]
        return torch.zeros(bs, 1, 8), 48000, torch.zeros(bs, 128, 50)
    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake)
    x0, mask = torch.randn(5, 128, 50), torch.rand(5, 50)
    feats = {"text_feat": torch.zeros(1, 5, 8), "uncond_text_feat": torch.zeros(1, 5, 8)}
    sampler.denoise_process_multi({}, feats, 1.0, reps, 4.5, 10, 5, "euler", generator=torch.Generator().manual_seed(0),
                                  edit=audio_edit.EditSpec(x0, 0.7, mask))
    assert torch.equal(got[0].x0, x0[:3]) and torch.equal(got[1].x0, x0[3:]) and got[1].strength == 0.7
    assert torch.equal(got[0].mask, mask[:3]) and torch.equal(got[1].mask, mask[3:])


def _node_call(monkeypatch, **kw):
    model, dac = _fake_model_dac()
    model.get_empty_clip_sequence = model.get_empty_sync_sequence = None
    seen = {}

    def fake(visual, text, secs, m, d, **k):
        seen.update(k)
        seen["secs"] = secs
        return torch.zeros(k["batch_size"], 1, 960), 48000
    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake)
    monkeypatch.setattr(audio_edit, "encode_source", lambda w, m, d, La: torch.full((w.shape[0], 128, La), 0.25))
    feats = {"siglip2_feat": torch.zeros(1, 40, 768), "syncformer_feat": torch.zeros(1, 120, 768),
             "text_feat": torch.zeros(1, 5, 768), "uncond_text_feat": torch.zeros(1, 5, 768), "audio_len_in_s": 5.0}
    out = nodes.HunyuanFoleySampler().generate_audio(model, {"dac_model": dac}, 16, 5.0, "p", "n", 4.5, 10, "euler", 2, 0, True,
                                                     features=feats, **kw)
    return out, seen


def test_generate_audio_edit_kwargs(monkeypatch):
    out, seen = _node_call(monkeypatch)
    assert seen["edit"] is None and out[1]["waveform"].shape == (2, 1, 960)
    out, seen = _node_call(monkeypatch, audio=_audio(5.0), strength=0.6, regenerate=[(2.0, 3.0)], crossfade_s=0.1)
    e = seen["edit"]
    assert isinstance(e, audio_edit.EditSpec) and e.strength == 0.6 and float(e.x0.mean()) == 0.25
    assert torch.equal(e.mask, audio_edit.build_mask(250, [(2.0, 3.0)], 0.1))
    assert seen["num_inference_steps"] == 10 and seen["sampler"] == "euler" and out[0]["waveform"].shape == (1, 1, 960)
    with pytest.raises(ValueError, match="audio="):
        _node_call(monkeypatch, strength=0.5)
    with pytest.raises(ValueError, match="audio="):
        _node_call(monkeypatch, regenerate=[(1.0, 2.0)])
    with pytest.raises(TypeError):              # keyword-only: no positional slot past `features`
        nodes.HunyuanFoleySampler().generate_audio(*([None] * 17))


def test_node_sockets_stay_the_references():
    """Editing is keyword-only on generate_audio: no new socket, no new node."""
    it = nodes.HunyuanFoleySampler.INPUT_TYPES()
    names = set(it["required"]) | set(it.get("optional", {}))
    assert not names & {"audio", "strength", "regenerate", "crossfade_s"}
    assert len(nodes.NODE_CLASS_MAPPINGS) == 6
