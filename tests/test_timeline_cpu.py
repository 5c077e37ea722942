"""The prompt timeline without a GPU: parsing and refusals, the ramp geometry, token times, the window shift, the unconditional
halves, the oracle restatement (tests/timeline_ref.py) pinned against O.sample_latents, and the node's keyword plumbing."""
import os
import re
import types

import pytest
import torch

from foley_amd import nodes
from foley_amd.host import config as C, prompt_timeline as PT, runtime as rt, sampler, synth
from oracle import foley_oracle as O
import timeline_ref as TR
from abi_pin import assert_abi_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


# ----------------------------------------------------------------------------- parsing
def test_refusals():
    for bad, word in (([(0.0, 3.0, "a"), (2.0, 4.0, "b")], "overlap"), ([(2.0, 2.0, "a")], "<= start"), ([(3.0, 1.0, "a")], "<= start"),
                      ([(-1.0, 2.0, "a")], "negative"), ([(0.0, 1.0)], "not (start_s"), ([], "empty")):
        with pytest.raises(PT.TimelineError, match=re.escape(word)):
            PT.parse(bad, "base", 5.0, 0.25)
    with pytest.raises(PT.TimelineError, match="crossfade"):
        PT.parse([(0.0, 1.0, "a")], "base", 5.0, -0.1)
    many = [(float(i), float(i + 1), "p%d" % i) for i in range(16)]
    with pytest.raises(PT.TimelineError, match="exceed 16"):
        PT.parse(many, "p0", 16.0, 0.0)                       # 16 prompts + the negative prompt
    assert len(PT.parse(many[:15], "p0", 15.0, 0.0).prompts) == 15
    assert PT.MAX_SETS == 16 and "#define FOLEY_TIMELINE_MAX_SETS 16" in open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    assert isinstance(PT.TimelineError("x"), ValueError)


def test_gaps_sharing_merging_and_the_cut_at_the_end():
    tl = PT.parse([(3.0, 4.0, "b"), (1.0, 2.0, "a"), (4.0, 9.0, "a")], "base", 5.0, 0.0)         # given out of order: sorted by start
    assert [(s.start_s, s.end_s, s.prompt) for s in tl.segments] == [
        (0.0, 1.0, "base"), (1.0, 2.0, "a"), (2.0, 3.0, "base"), (3.0, 4.0, "b"), (4.0, 5.0, "a")]          # 9 s cut at 5 s
    assert tl.prompts == ("base", "a", "b") and [s.set for s in tl.segments] == [0, 1, 0, 2, 1]             # equal texts: one set
    tl = PT.parse([(0.0, 2.0, "a"), (2.0, 3.0, "a"), (3.5, 5.0, "base")], "base", 5.0, 0.0)
    assert [(s.start_s, s.end_s, s.prompt) for s in tl.segments] == [(0.0, 3.0, "a"), (3.0, 5.0, "base")]   # neighbours merge, gap too
    tl = PT.parse([(6.0, 7.0, "late")], "base", 5.0, 0.0)                                                   # a span past the clip
    assert [(s.start_s, s.end_s, s.prompt) for s in tl.segments] == [(0.0, 5.0, "base")] and tl.prompts == ("base",)


# ----------------------------------------------------------------------------- ramps and token times
def test_token_times():
    t = PT.token_times(8, 50)
    assert t[:8] == [(j + 0.5) / 8 for j in range(8)] and t[8:] == [(l + 0.5) / 50 for l in range(50)]
    t = PT.token_times(2, 2, start_frame=400)
    assert t == [8.0 + 0.5 / 8, 8.0 + 1.5 / 8, 8.01, 8.03]


def test_ramp_geometry():
    # segments of 3 s, 0.25 s and 1.75 s under a 1 s crossfade: h = 0.125 at both boundaries of the short one (times exact in binary)
    tl = PT.parse([(0.0, 3.0, "a"), (3.0, 3.25, "b"), (3.25, 5.0, "c")], "base", 5.0, 1.0)
    s = tl.segments
    assert (s[0].h_lo, s[0].h_hi) == (0.0, 0.125) and (s[1].h_lo, s[1].h_hi) == (0.125, 0.125) and (s[2].h_lo, s[2].h_hi) == (0.125, 0.0)
    tl = PT.parse([(0.0, 3.0, "a"), (3.0, 5.0, "b")], "base", 5.0, 0.5)
    assert tl.segments[0].h_hi == 0.25 == tl.segments[1].h_lo
    sa, sb, al = PT.token_table(tl.segments, 40, 250)
    times = PT.token_times(40, 250)
    for t, a, b, x in zip(times, sa, sb, al):
        assert a == (0 if t < 3.0 else 1)                                  # set_a: the token's own segment
        if abs(t - 3.0) >= 0.25:
            assert x == 0.0 and b == a
        else:
            assert b == 1 - a and abs(x - 0.5 * (0.25 - abs(t - 3.0)) / 0.25) < 1e-12 and 0.0 < x <= 0.5
    assert PT._triple(tl.segments, 3.0) == (1, 0, 0.5)                      # the boundary from above ...
    assert PT._triple(tl.segments, 3.0 - 1e-12)[:2] == (0, 1) and abs(PT._triple(tl.segments, 3.0 - 1e-12)[2] - 0.5) < 1e-9   # ... and below
    assert PT._triple(tl.segments, 2.75) == (0, 0, 0.0) and PT._triple(tl.segments, 3.25) == (1, 1, 0.0)     # the outer edges
    assert PT._triple(tl.segments, 2.875)[2] == 0.25 and PT._triple(tl.segments, 3.125)[2] == 0.25
    hard = PT.parse([(0.0, 3.0, "a"), (3.0, 5.0, "b")], "base", 5.0, 0.0)
    sa, sb, al = PT.token_table(hard.segments, 40, 250)
    assert all(x == 0.0 for x in al) and sa == sb and sa[40 + 149] == 0 and sa[40 + 150] == 1


def test_window_shift_agrees_at_equal_global_time():
    tl = PT.parse([(2.0, 9.3, "a"), (9.3, 12.0, "b"), (12.0, 20.5, "c"), (27.0, 34.0, "a")], "base", 34.0, 1.5)
    Lv, La = 80, 500                                                        # 10 s windows at 0 s and 8 s: 2 s shared
    w0, w8 = PT.token_table(tl.segments, Lv, La, 0), PT.token_table(tl.segments, Lv, La, 400)
    for x0, x8 in zip(w0, w8):
        assert x0[Lv + 400:] == x8[Lv:Lv + 100]                             # audio frames 400..499
        assert x0[64:Lv] == x8[:16]                                         # SigLIP2 tokens 64..79
    assert any(v > 0 for v in w0[2][Lv + 400:]) and len(set(w0[0][Lv + 400:])) > 1     # the shared stretch holds a ramp
    flat = PT.batch_table(tl, Lv, La, 2, 4, starts=[0, 400])               # 2 variations x 2 windows under CFG
    sa = torch.tensor(flat[0]).view(8, Lv + La)
    assert torch.equal(sa[4], sa[6]) and torch.equal(sa[5], sa[7]) and sa[5].tolist() == [v + 1 for v in w8[0]]


@pytest.mark.parametrize("ncfg", [1, 2, 3])
def test_unconditional_halves_read_the_negative_set(ncfg):
    tl = PT.parse([(0.0, 0.5, "a")], "base", 1.0, 0.2)
    S, clips = 8 + 50, 2
    sa, sb, al = (torch.tensor(x).view(ncfg * clips, S) for x in PT.batch_table(tl, 8, 50, ncfg, clips))
    n_unc = (ncfg - 1) * clips
    assert not sa[:n_unc].any() and not sb[:n_unc].any() and not al[:n_unc].any()
    off = 1 if ncfg > 1 else 0
    one = PT.token_table(tl.segments, 8, 50)
    for r in range(n_unc, ncfg * clips):
        assert sa[r].tolist() == [v + off for v in one[0]] and sb[r].tolist() == [v + off for v in one[1]]
        assert torch.equal(al[r], torch.tensor(one[2])) and float(al[r].max()) > 0


# ----------------------------------------------------------------------------- the restatement
def test_one_span_restatement_is_the_plain_oracle_loop():
    """Pins tests/timeline_ref.py: a timeline of one span (and the negative set on the unconditional half) is O.sample_latents bit for bit."""
    cfg = C.TINY
    sd = synth.synth_dit_state_dict(cfg)
    cond = synth.synth_conditioning(cfg, 1.0, t2a=False, sd=sd, seed=10)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
    tl = PT.parse([(0.0, 1.0, "a")], "a", 1.0, 0.25)
    assert len(tl.segments) == 1
    sets = torch.cat([O.pad_or_trim_text(cond["uncond_text"], 77), O.pad_or_trim_text(cond["text"], 77)])
    flat = PT.batch_table(tl, cond["clip"].shape[1], 50, 2, 1)
    with torch.inference_mode():
        want = O.sample_latents(sd, cfg.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"], 3, 4.5, "heun-2")
        keep = O.triple_block
        got = TR.oracle_timeline_latents(sd, cfg.heads, noise, sets, flat, cond["clip"], cond["sync"], 3, 4.5, "heun-2")
    assert O.triple_block is keep and torch.equal(got, want)


def test_timeline_ref_blend_bound_reduces_to_the_plain_bound():
    import opcheck as oc
    g = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(2, 2, 7, 128, generator=g), torch.randn(3, 2, 5, 128, generator=g), torch.randn(3, 2, 5, 128, generator=g)
    sa = torch.tensor([[0] * 7, [2] * 7])
    al = torch.zeros(2, 7)
    ref, b = TR.timeline_attention_ref_and_bound(q, k, v, sa, torch.ones_like(sa), al, torch.float32)
    for row, s in ((0, 0), (1, 2)):
        r1, b1 = oc.attention_ref_and_bound(q[row:row + 1], k[s:s + 1], v[s:s + 1], torch.float32)
        assert torch.equal(ref[row], r1[0]) and torch.equal(b.e[row], b1.e[0] + 3 * oc.U32 * r1[0].abs())
    al2 = torch.full((2, 7), 0.5)
    ref2, _ = TR.timeline_attention_ref_and_bound(q, k, v, sa, torch.ones_like(sa), al2, torch.float32)
    r_b, _ = oc.attention_ref_and_bound(q, k[1:2], v[1:2], torch.float32)
    assert torch.allclose(ref2, 0.5 * ref + 0.5 * r_b, atol=1e-14)


# ----------------------------------------------------------------------------- ABI surface and node plumbing
def test_abi_declares_the_timeline_entries():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    for name in ("foley_prepare_timeline", "foley_op_attention_timeline"):
        assert name in rt.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    assert_abi_version()


def _node(monkeypatch, duration=5.0, batch_size=2, **kw):
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
    model.get_empty_clip_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    model.get_empty_sync_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    dac = types.SimpleNamespace(has_encoder=True, cfg=C.DAC48K, sample_rate=48000)
    seen = {"encoded": []}

    def fake_sample(visual, text, secs, m, d, **k):
        seen.update(k)
        seen.update(secs=secs, visual=visual, text=text)
        return torch.zeros(k["batch_size"], 1, int(round(secs * 50)) * 960), 48000

    def fake_encode(prompts, deps, dev, dt=None):
        seen["encoded"].append(list(prompts))
        return torch.arange(len(prompts), dtype=torch.float32).view(-1, 1, 1).expand(len(prompts), 5, 768).clone()

    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake_sample)
    monkeypatch.setattr(nodes, "encode_text_feat", fake_encode)
    deps = {"dac_model": dac, "siglip2_model": None, "syncformer_model": None}
    out = nodes.HunyuanFoleySampler().generate_audio(model, deps, 16, duration, "p", "n", 4.5, 10, "euler", batch_size, 0, True, **kw)
    return out, seen


def test_node_timeline_reaches_the_sampler_and_encodes_once(monkeypatch):
    spans = [(0.0, 3.0, "footsteps on gravel"), (3.0, 4.0, "a car door slams")]
    _out, seen = _node(monkeypatch, prompt_timeline=spans)
    tl = seen["timeline"]
    assert isinstance(tl, PT.Timeline) and tl.prompts == ("footsteps on gravel", "a car door slams", "p")        # 4..5 s: the widget's
    assert seen["encoded"] == [["n", "footsteps on gravel", "a car door slams", "p"]]                              # ONE call
    assert seen["text"]["text_feat"].shape[0] == 3 and seen["text"]["uncond_text_feat"].shape[0] == 1
    assert seen["text"]["text_feat"][:, 0, 0].tolist() == [1.0, 2.0, 3.0] and float(seen["text"]["uncond_text_feat"][0, 0, 0]) == 0.0
    assert tl.segments[0].h_hi == 0.125 and "windows" not in seen                                                  # the default crossfade: 0.25 s
    _out, seen = _node(monkeypatch, prompt_timeline=spans, prompt_crossfade_s=0.0)
    assert all(s.h_lo == 0.0 and s.h_hi == 0.0 for s in seen["timeline"].segments)
    _out, seen = _node(monkeypatch)                                                                                # no timeline: today's call
    assert "timeline" not in seen and seen["encoded"] == [["n", "p"]]


def test_node_timeline_with_windows_is_given_in_the_long_clips_time(monkeypatch):
    _out, seen = _node(monkeypatch, duration=34.0, window_s=10, prompt_timeline=[(12.0, 20.0, "rain")])
    assert seen["windows"].starts == [0, 400, 800, 1200] and seen["timeline"].prompts == ("p", "rain")
    assert [(s.start_s, s.end_s) for s in seen["timeline"].segments] == [(0.0, 12.0), (12.0, 20.0), (20.0, 34.0)]
    assert seen["encoded"] == [["n", "p", "rain"]] and seen["text"]["text_feat"].shape[0] == 2


def test_node_timeline_refusals_come_before_the_encoders(monkeypatch):
    spans = [(0.0, 3.0, "a")]
    for kw in (dict(prompts=["x", "y"]), dict(negative_prompts=["x", "y"]), dict(features={})):
        seen_calls = []
        monkeypatch.setattr(nodes, "_ensure_text_encoder", lambda deps: seen_calls.append(1))
        with pytest.raises(ValueError, match="prompt_timeline does not combine"):
            _node(monkeypatch, prompt_timeline=spans, **kw)
    with pytest.raises(ValueError, match="overlap"):
        _out, seen = _node(monkeypatch, prompt_timeline=[(0.0, 3.0, "a"), (2.0, 4.0, "b")])
    with pytest.raises(ValueError, match="per-window video"):
        _node(monkeypatch, duration=34.0, window_s=10, prompt_timeline=spans, image=torch.zeros(34 * 16, 2, 2, 3))


def test_build_plan_refuses_a_mismatched_text_batch():
    model = types.SimpleNamespace(cfg=C.TINY, device=torch.device("cpu"), _text_len_fixed=None)
    tl = PT.parse([(0.0, 0.5, "a")], "base", 1.0, 0.0)
    vis = {"siglip2_feat": torch.zeros(1, 8, 768), "syncformer_feat": torch.zeros(1, 16, 768)}
    txt = {"text_feat": torch.zeros(3, 5, 768), "uncond_text_feat": torch.zeros(1, 5, 768)}
    with pytest.raises(rt.FoleyRuntimeError, match="one row per distinct prompt"):
        sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler", timeline=tl)
    vis2 = {"siglip2_feat": torch.zeros(2, 8, 768), "syncformer_feat": torch.zeros(2, 16, 768)}
    with pytest.raises(rt.FoleyRuntimeError, match="shared by the clips"):
        sampler.build_plan(model, vis2, {**txt, "text_feat": torch.zeros(2, 5, 768)}, 50, 4.5, 10, 2, "euler", timeline=tl)
