"""Long clips as overlapping windows without a GPU: where the windows start, the blend weights, the refusals, the node's keyword
plumbing, and the windows of the restated loop (tests/loop_ref.py) that tests/test_windows_gpu.py compares against."""
import types

import pytest
import torch

import loop_ref as L
from conftest import rel_err
from foley_amd import nodes
from foley_amd.host import config as C, long_form, sampler, synth
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- restatement of the coupled loop
KEYS = ("text", "uncond_text", "clip", "sync")


@pytest.fixture(scope="module")
def tiny_cpu():
    sd = synth.synth_dit_state_dict(C.TINY)
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    return sd, cond


def test_restatement_one_window_is_the_plain_loop(tiny_cpu):
    sd, cond = tiny_cpu
    noise = torch.randn(2, 128, 50, generator=torch.Generator().manual_seed(5))
    plan = long_form.WindowPlan.from_frames([0], 50)
    c = [cond[k] for k in KEYS]
    for solver, steps in (("euler", 6), ("heun-2", 6)):
        ref = O.sample_latents(sd, C.TINY.heads, noise, *c, steps, 4.5, solver)
        got = L.restated_loop(sd, C.TINY.heads, noise, *c, steps, 4.5, solver, windows=plan).x
        assert torch.equal(got, ref), solver


def test_restatement_two_disjoint_windows_are_two_runs(tiny_cpu):
    """Abutting windows share no frame: every weight is 1 and the coupled loop is two independent runs.  (The two clips run in one
    batch here and alone in the reference, so the claim is to fp32 accuracy of the oracle's batched matmuls, not bitwise.)"""
    sd, cond = tiny_cpu
    cond2 = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd, seed=31)
    noise = torch.randn(1, 128, 100, generator=torch.Generator().manual_seed(6))
    plan = long_form.WindowPlan.from_frames([0, 50], 50)
    assert torch.equal(plan.weights, torch.ones(2, 50))
    got = L.restated_loop(sd, C.TINY.heads, noise, *[torch.cat([cond[k], cond2[k]]) for k in KEYS], 6, 4.5, "heun-2", windows=plan).x
    for k, c in enumerate((cond, cond2)):
        ref = O.sample_latents(sd, C.TINY.heads, noise[:, :, 50 * k:50 * k + 50], c["text"], c["uncond_text"], c["clip"], c["sync"],
                               6, 4.5, "heun-2")
        assert rel_err(got[:, :, 50 * k:50 * k + 50], ref) < 1e-5, k


def test_restatement_windows_agree_after_euler(tiny_cpu):
    sd, cond = tiny_cpu
    plan = long_form.WindowPlan.from_frames([0, 30], 50)
    noise = torch.randn(1, 128, 80, generator=torch.Generator().manual_seed(7))
    g, x, _info = L.restated_loop(sd, C.TINY.heads, noise, *[cond[k] for k in KEYS], 4, 4.5, "euler", windows=plan)
    assert torch.equal(x[0, :, 30:], x[1, :, :20])
    assert rel_err(g[0, :, 30:50], x[0, :, 30:]) < 1e-6


# ----------------------------------------------------------------------------- planning
CASES = [(8, 10, 2), (11, 10, 2), (19, 10, 2), (34, 10, 2), (130, 10, 2)]


@pytest.mark.parametrize("T,W,O_", CASES)
def test_plan_windows_geometry(T, W, O_):
    p = long_form.plan_windows(T, W, O_)
    Weff = min(T, W)
    assert p.starts[0] == 0 and p.La == Weff * 50 and p.Ltot == T * 50 and p.starts[-1] + Weff * 50 == T * 50
    assert all(s % 50 == 0 for s in p.starts)                                  # whole seconds
    for a, b in zip(p.starts, p.starts[1:]):
        assert b > a and a + p.La - b >= O_ * 50
    assert p.weights.shape == (p.n_win, p.La) and p.weights.dtype == torch.float32
    if T == 8:
        assert p.n_win == 1 and torch.equal(p.weights, torch.ones(1, 400))
    if T == 11:
        assert p.starts == [0, 50]
    if T == 19:
        assert p.starts == [0, 250, 450] and int(p.coverage().max()) == 3
        assert torch.equal((p.coverage() == 3).nonzero().flatten(), torch.arange(450, 500))
    if T == 34:
        assert p.starts == [0, 400, 800, 1200] and int(p.coverage().max()) == 2
    if T == 130:
        assert p.n_win == 16 and p.starts == [400 * k for k in range(16)]


def test_plan_windows_cuts_total_to_whole_seconds_and_keeps_fractional_overlaps():
    assert long_form.plan_windows(34.9, 10, 2).Ltot == 34 * 50
    assert long_form.plan_windows(34, 10.0, 2).starts == [0, 400, 800, 1200]
    for O_ in (0.0, 0.5, 2.5, 7.5, 9.9):
        for T in (11, 17, 23, 60):
            p = long_form.plan_windows(T, 10, O_)
            assert p.Ltot == T * 50
            assert all(a + p.La - b >= min(O_, 9) * 50 for a, b in zip(p.starts, p.starts[1:])), (T, O_, p.starts)
    assert long_form.plan_windows(13, 10, 9.9).starts == [0, 50, 100, 150]     # one second apart is the deepest overlap there is
    assert long_form.plan_windows(20, 10, 0).starts == [0, 500]                # abutting


@pytest.mark.parametrize("starts,La", [([0, 45, 61, 110], 75), ([0, 30, 45], 50), ([0, 250, 450], 500), ([0, 400, 800, 1200], 500),
                                       ([0, 50, 100], 50), ([0, 1], 50), ([0], 37)])
def test_weights_sum_to_one_and_single_coverage_is_exactly_one(starts, La):
    p = long_form.WindowPlan.from_frames(starts, La)
    total = torch.zeros(p.Ltot, dtype=torch.float64)
    for k, s in enumerate(starts):
        total[s:s + La] += p.weights[k].double()
    assert float((total - 1).abs().max()) < 1e-6
    assert float(p.weights.min()) > 0.0                                         # frame centres: no covered frame drops out
    cov = p.coverage()
    for k, s in enumerate(starts):
        single = cov[s:s + La] == 1
        assert torch.equal(p.weights[k][single], torch.ones(int(single.sum())))
        assert bool((p.weights[k][~single] < 1).all())


@pytest.mark.parametrize("starts,La", [([0, 400, 800, 1200], 500), ([0, 30], 50), ([0, 50], 500), ([0, 45, 110], 75)])
def test_weights_are_monotone_across_each_ramp(starts, La):
    """Two-deep overlaps: the earlier window's weight falls strictly over the overlap, the later one's rises, and they mirror."""
    p = long_form.WindowPlan.from_frames(starts, La)
    for k in range(p.n_win - 1):
        ov = starts[k] + La - starts[k + 1]
        down, up = p.weights[k][La - ov:].double(), p.weights[k + 1][:ov].double()
        assert bool((down[1:] < down[:-1]).all()) and bool((up[1:] > up[:-1]).all())
        assert torch.allclose(down, up.flip(0), atol=1e-6)
        assert abs(float(up[0]) - 0.5 / ov) < 1e-6                              # frame centre (l + 0.5) / overlap


def test_plan_refusals():
    with pytest.raises(ValueError, match="gap"):
        long_form.WindowPlan.from_frames([0, 51], 50)
    with pytest.raises(ValueError, match="ascend"):
        long_form.WindowPlan.from_frames([0, 30, 20], 50)
    with pytest.raises(ValueError, match="ascend"):
        long_form.WindowPlan.from_frames([0, 30, 30], 50)
    with pytest.raises(ValueError, match="frame 0"):
        long_form.WindowPlan.from_frames([5, 30], 50)
    with pytest.raises(ValueError, match="whole number"):
        long_form.plan_windows(34, 9.5, 2)
    with pytest.raises(ValueError, match="whole number"):
        long_form.plan_windows(34, 0, 0)
    with pytest.raises(ValueError, match="overlap_s"):
        long_form.plan_windows(34, 10, 10)
    with pytest.raises(ValueError, match="overlap_s"):
        long_form.plan_windows(34, 10, -1)
    long_form.plan_windows(360, 10, 2)                                           # 18000 frames: the cap itself
    with pytest.raises(ValueError, match="18000"):
        long_form.plan_windows(361, 10, 2)
    with pytest.raises(ValueError, match="18000"):
        long_form.plan_windows(130, 10, 2, variations=3)
    long_form.plan_windows(120, 10, 2, variations=3)
    p = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    assert [p.clip_index(v, k) for v in range(2) for k in range(3)] == list(range(6))


# ----------------------------------------------------------------------------- sampler plumbing
def test_window_rows_layouts():
    t1, t3, t6 = torch.zeros(1, 4, 8), torch.arange(3.).view(3, 1, 1).expand(3, 4, 8), torch.zeros(6, 4, 8)
    assert sampler.window_rows(t1, 2, 3, "x") is t1 and sampler.window_rows(t6, 2, 3, "x") is t6
    r = sampler.window_rows(t3, 2, 3, "x")
    assert r.shape == (6, 4, 8) and r[:, 0, 0].tolist() == [0, 1, 2, 0, 1, 2]     # clip v*n_win + k reads window k's row
    with pytest.raises(ValueError, match="n_win"):
        sampler.window_rows(torch.zeros(2, 4, 8), 2, 3, "x")


def test_sampler_refuses_windows_with_an_edit():
    p = long_form.WindowPlan.from_frames([0, 30], 50)
    with pytest.raises(ValueError, match="edit"):
        sampler.denoise_process_with_generator({}, {}, 1.6, None, None, 4.5, 10, 1, "euler", edit=object(), windows=p)


# ----------------------------------------------------------------------------- node plumbing
def _node(monkeypatch, image=None, duration=34.0, batch_size=2, **kw):
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
    model.get_empty_clip_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    model.get_empty_sync_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    dac = types.SimpleNamespace(has_encoder=True, cfg=C.DAC48K, sample_rate=48000)
    seen = {"slices": []}

    def fake_sample(visual, text, secs, m, d, **k):
        seen.update(k)
        seen.update(secs=secs, visual=visual, text=text)
        n = int(round(secs * 50)) * 960
        return torch.zeros(k["batch_size"], 1, n), 48000

    def fake_select(img, dur, fr, device=None):
        seen["select_calls"] = seen.get("select_calls", 0) + 1
        n8, n25 = int(dur * 8), int(dur * 25)
        return torch.arange(n8).view(n8, 1, 1, 1), torch.arange(n25).view(n25, 1, 1, 1)

    def fake_video(f8, f25, _sig, _sync, _dev, model_dtype=None):
        seen["slices"].append((int(f8[0]), len(f8), int(f25[0]), len(f25)))
        return ({"siglip2_feat": torch.full((1, len(f8), 768), float(f8[0])),
                 "syncformer_feat": torch.full((1, ((len(f25) - 16) // 8 + 1) * 8, 768), float(f25[0]))}, len(f25) / 25.0)

    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake_sample)
    monkeypatch.setattr(nodes._enc, "select_frames", fake_select)
    monkeypatch.setattr(nodes._enc, "video_features", fake_video)
    monkeypatch.setattr(nodes, "_ensure_visual_encoders", lambda deps, dev, dt: deps)
    monkeypatch.setattr(nodes, "encode_text_feat", lambda prompts, deps, dev, dt=None: torch.zeros(2, 5, 768))
    deps = {"dac_model": dac, "siglip2_model": None, "syncformer_model": None}
    out = nodes.HunyuanFoleySampler().generate_audio(model, deps, 16, duration, "p", "n", 4.5, 10, "euler", batch_size, 0, True,
                                                     image=image, **kw)
    return out, seen


def test_node_windows_text_to_audio(monkeypatch):
    out, seen = _node(monkeypatch, window_s=10)
    p = seen["windows"]
    assert p.starts == [0, 400, 800, 1200] and p.La == 500 and seen["batch_size"] == 2 and seen["secs"] == 34.0
    assert seen["visual"]["siglip2_feat"].shape == (1, 80, 768) and seen["visual"]["syncformer_feat"].shape == (1, 240, 768)
    assert seen["text"]["text_feat"].shape[0] == 1
    assert out[1]["waveform"].shape == (2, 1, 34 * 48000) and out[0]["waveform"].shape == (1, 1, 34 * 48000)
    _out, seen = _node(monkeypatch, duration=130.0, batch_size=1, window_s=10, window_overlap_s=2)     # past the widget's 60 s
    assert seen["windows"].n_win == 16 and seen["secs"] == 130.0


def test_node_windows_slice_the_video_per_window(monkeypatch):
    image = torch.zeros(19 * 16, 2, 2, 3)
    _out, seen = _node(monkeypatch, image=image, duration=19.0, batch_size=1, window_s=10, window_overlap_s=2.0)
    assert seen["select_calls"] == 1                                              # once, for the whole clip
    assert seen["windows"].starts == [0, 250, 450]
    assert seen["slices"] == [(0, 80, 0, 250), (40, 80, 125, 250), (72, 80, 225, 250)]
    v = seen["visual"]
    assert v["siglip2_feat"].shape == (3, 80, 768) and v["siglip2_feat"][:, 0, 0].tolist() == [0.0, 40.0, 72.0]
    assert v["syncformer_feat"].shape == (3, 240, 768) and seen["text"]["text_feat"].shape[0] == 1


def test_node_window_s_off_or_not_exceeded_is_todays_call(monkeypatch):
    _out, seen = _node(monkeypatch, duration=8.0)
    assert "windows" not in seen and seen["secs"] == 8.0
    _out, seen = _node(monkeypatch, duration=8.0, window_s=10)
    assert "windows" not in seen and seen["secs"] == 8.0 and seen["visual"]["siglip2_feat"].shape == (1, 64, 768)
    _out, seen = _node(monkeypatch, duration=10.5, window_s=10)                     # cut to whole seconds: one window
    assert "windows" not in seen and seen["secs"] == 10.0


def test_node_window_refusals(monkeypatch):
    audio = {"waveform": torch.zeros(1, 1, 48000), "sample_rate": 48000}
    with pytest.raises(ValueError, match="audio="):
        _node(monkeypatch, window_s=10, audio=audio)
    with pytest.raises(ValueError, match="audio="):
        _node(monkeypatch, window_s=10, regenerate=[(1.0, 2.0)])
    with pytest.raises(ValueError, match="prompts="):
        _node(monkeypatch, window_s=10, prompts=["a", "b"])
    with pytest.raises(ValueError, match="prompts="):
        _node(monkeypatch, window_s=10, images=[torch.zeros(4, 2, 2, 3)] * 2)
    with pytest.raises(ValueError, match="prompts="):
        _node(monkeypatch, window_s=10, features={})
    with pytest.raises(ValueError, match="whole number"):
        _node(monkeypatch, window_s=9.5)
    with pytest.raises(ValueError, match="18000"):
        _node(monkeypatch, duration=130.0, batch_size=3, window_s=10)
    with pytest.raises(TypeError):                                                 # keyword-only
        nodes.HunyuanFoleySampler().generate_audio(*([None] * 17))


def test_node_sockets_stay_the_references():
    it = nodes.HunyuanFoleySampler.INPUT_TYPES()
    names = list(it["required"]) + list(it.get("optional", {}))
    assert names == ["hunyuan_model", "hunyuan_deps", "frame_rate", "duration", "prompt", "negative_prompt", "cfg_scale", "steps",
                     "sampler", "batch_size", "seed", "force_offload", "image", "torch_compile_cfg", "block_swap_args"]
    assert it["required"]["duration"][1]["max"] == 60.0
    assert len(nodes.NODE_CLASS_MAPPINGS) == 6
