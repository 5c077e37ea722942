"""Per-clip conditioning, host side (host/cond_sets.py): set building and de-duplication, refusals, the node's argument plumbing
(mocked sampler and encoders) and the data-parallel sharding of per-clip features.  No GPU, no HIP library."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (also puts the repo root on sys.path)
from foley_amd.host import cond_sets as CS
from foley_amd.host import distributed as D

E_CLIP, E_SYNC = torch.full((8,), 0.5), torch.full((6,), -0.25)


def _text(n, seed, T=7):
    return torch.randn(n, T, 4, generator=torch.Generator().manual_seed(seed))


def _vis(n, seed, Lv=5, Ls=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, Lv, 8, generator=g), torch.randn(n, Ls, 6, generator=g)


def test_identical_conditioning_gives_one_set_per_half():
    t, u = _text(1, 1), _text(1, 2)
    c, s = _vis(1, 3)
    for bs in (1, 4):
        rep = lambda x: x.expand(bs, -1, -1).clone()
        for cfg in (True, False):
            sets = CS.build(rep(t), rep(u), rep(c), rep(s), E_CLIP, E_SYNC, bs, cfg)
            n = 2 if cfg else 1
            assert sets.homogeneous and sets.text_of is None and sets.vis_of is None
            assert sets.text.shape[0] == n and sets.clip.shape[0] == n and sets.sync.shape[0] == n
            assert torch.equal(sets.text[-1], t[0]) and torch.equal(sets.clip[-1], c[0])
            if cfg:
                assert torch.equal(sets.text[0], u[0]) and torch.equal(sets.clip[0], E_CLIP.expand(5, -1))


def test_t2a_with_distinct_prompts_keeps_one_visual_set_per_half():
    bs = 6
    c = E_CLIP.expand(1, 5, -1).clone()
    s = E_SYNC.expand(1, 16, -1).clone()
    sets = CS.build(_text(bs, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, bs, True)
    assert not sets.homogeneous
    assert sets.text.shape[0] == 1 + bs and sets.text_of == [0] * bs + list(range(1, bs + 1))
    assert sets.clip.shape[0] == 2 and sets.vis_of == [0] * bs + [1] * bs          # one visual set per half: the per-half layout


def test_video_batch_under_cfg_collapses_the_unconditional_rows():
    bs = 6
    c, s = _vis(bs, 4)
    sets = CS.build(_text(1, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, bs, True)
    assert sets.clip.shape[0] == 1 + bs and sets.sync.shape[0] == 1 + bs            # 1 + 6 visual sets, not 12
    assert sets.vis_of == [0] * bs + list(range(1, bs + 1))
    assert sets.text.shape[0] == 2 and sets.text_of == [0] * bs + [1] * bs
    for k in range(bs):
        assert torch.equal(sets.clip[sets.vis_of[bs + k]], c[k]) and torch.equal(sets.sync[sets.vis_of[bs + k]], s[k])
    # repeated clips share their set; without CFG there is no unconditional half
    c2, s2 = c[[0, 1, 0, 2]], s[[0, 1, 0, 2]]
    sets = CS.build(_text(1, 1), _text(1, 2), c2, s2, E_CLIP, E_SYNC, 4, False)
    assert sets.vis_of == [0, 1, 0, 2] and sets.clip.shape[0] == 3 and sets.text_of == [0, 0, 0, 0]


def test_a_clip_and_sync_pair_is_one_set():
    """Clips that share their SigLIP2 rows but not their Synchformer rows are different visual sets."""
    c, s = _vis(1, 5)
    s2 = torch.cat([s, s + 1])
    sets = CS.build(_text(1, 1), _text(1, 2), c.expand(2, -1, -1), s2, E_CLIP, E_SYNC, 2, False)
    assert sets.vis_of == [0, 1]


def test_refusals():
    c, s = _vis(1, 3)
    with pytest.raises(CS.CondSetsError, match="batch 3"):
        CS.build(_text(3, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, 4, True)
    with pytest.raises(CS.CondSetsError, match="padded"):
        CS.build(_text(1, 1, T=7), _text(1, 2, T=9), c, s, E_CLIP, E_SYNC, 1, True)
    parts = [{"siglip2_feat": _vis(1, i, Lv=lv)[0], "syncformer_feat": _vis(1, i, Ls=ls)[1]} for i, (lv, ls) in
             enumerate([(5, 16), (5, 16)])]
    out = CS.stack_features(parts, ("siglip2_feat", "syncformer_feat"))
    assert out["siglip2_feat"].shape == (2, 5, 8) and out["syncformer_feat"].shape == (2, 16, 6)
    for lv, ls in ((6, 16), (5, 24)):                                               # mismatched Lv / Ls
        bad = parts + [{"siglip2_feat": _vis(1, 9, Lv=lv)[0], "syncformer_feat": _vis(1, 9, Ls=ls)[1]}]
        with pytest.raises(CS.CondSetsError, match="share one duration"):
            CS.stack_features(bad, ("siglip2_feat", "syncformer_feat"))


def test_visual_row_cap():
    """Different videos lay the visual stream out per batch row, at most 32 rows: 16 clips under CFG, 32 without.  Prompts
    alone keep one visual set per half and have no cap."""
    for bs, cfg, ok in ((16, True, True), (17, True, False), (32, False, True), (33, False, False)):
        c, s = _vis(bs, 6)
        if ok:
            assert not CS.build(_text(1, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, bs, cfg).homogeneous
        else:
            with pytest.raises(CS.CondSetsError, match="at most 32 batch rows"):
                CS.build(_text(1, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, bs, cfg)
    c, s = _vis(1, 6)
    assert CS.build(_text(40, 1), _text(1, 2), c, s, E_CLIP, E_SYNC, 40, True).vis_of == [0] * 40 + [1] * 40


def test_sampler_refuses_other_batches():
    from foley_amd.host import sampler
    from foley_amd.host.runtime import FoleyRuntimeError

    class M:
        cfg = type("cfg", (), {"text_len": 77})()
        device = torch.device("cpu")
        _text_len_fixed = None

    c, s = _vis(2, 3)
    with pytest.raises(FoleyRuntimeError, match="batch 2"):
        sampler.build_plan(M(), {"siglip2_feat": c, "syncformer_feat": s}, {"text_feat": _text(1, 1), "uncond_text_feat": _text(1, 2)},
                           50, 4.5, 10, 3, "euler")


def test_data_parallel_shards_carry_their_clips():
    """denoise_process_multi's slices (distributed.shard_range): per-clip tensors travel with their clips, shared ones stay, and
    the set maps each shard builds point at its own clips' rows."""
    bs, world = 5, 2
    c, s = _vis(bs, 4)
    t = _text(bs, 1)
    vis = {"siglip2_feat": c, "syncformer_feat": s}
    txt = {"text_feat": t, "uncond_text_feat": _text(1, 2)}
    for r in range(world):
        lo, hi = D.shard_range(bs, r, world)
        v, x = CS.shard(vis, lo, hi, bs), CS.shard(txt, lo, hi, bs)
        assert torch.equal(v["siglip2_feat"], c[lo:hi]) and torch.equal(x["text_feat"], t[lo:hi])
        assert x["uncond_text_feat"].shape[0] == 1
        sets = CS.build(x["text_feat"], x["uncond_text_feat"], v["siglip2_feat"], v["syncformer_feat"], E_CLIP, E_SYNC, hi - lo, True)
        n = hi - lo
        assert sets.vis_of == [0] * n + list(range(1, n + 1)) and sets.text_of == [0] * n + list(range(1, n + 1))
        for k in range(n):
            assert torch.equal(sets.clip[sets.vis_of[n + k]], c[lo + k]) and torch.equal(sets.text[sets.text_of[n + k]], t[lo + k])
    assert CS.shard(vis, 0, 1, 1) is not vis and torch.equal(CS.shard(vis, 0, 1, 1)["siglip2_feat"], c)   # batch 1: untouched


# ----------------------------------------------------------------------------- node plumbing
class _Model:
    device = torch.device("cpu")
    dtype = torch.float32
    arena = None

    def get_empty_clip_sequence(self, bs=None, len=None):
        return E_CLIP.view(1, 1, -1).expand(bs, len, -1)

    def get_empty_sync_sequence(self, bs=None, len=None):
        return E_SYNC.view(1, 1, -1).expand(bs, len, -1)


def _fake_clap(prompts):
    """CLAP's shape of behaviour: one call pads its prompts to the longest one (padding=True), and the pad rows carry hidden
    states of their own (unmasked downstream) that depend on that padded length - not zeros."""
    T = max(len(p) for p in prompts) + 2
    out = torch.empty(len(prompts), T, 4)
    for i, p in enumerate(prompts):
        n = len(p) + 2
        for t in range(T):
            out[i, t] = (float(sum(map(ord, p)) % 97) + t) if t < n else -(T + 0.5 * t)
    return out


@pytest.fixture
def node(monkeypatch):
    from foley_amd import nodes
    calls = {}

    def fake_text(prompts, deps, device, dtype=None):
        calls.setdefault("clap", []).append(list(prompts))
        return _fake_clap(prompts)

    def fake_denoise(visual, text, audio_len_in_s, model, dac, **kw):
        calls["denoise"] = (visual, text, audio_len_in_s, kw)
        return torch.zeros(kw["batch_size"], 1, 8), 48000

    def fake_frames(img, duration, frame_rate, device=None):
        return img, img

    def fake_video(f8, f25, sig, syn, device, model_dtype=None):
        n = int(f8.shape[0])
        return {"siglip2_feat": torch.full((1, n, 8), float(n)), "syncformer_feat": torch.full((1, 16, 6), float(n))}, n / 8.0

    monkeypatch.setattr(nodes, "encode_text_feat", fake_text)
    monkeypatch.setattr(nodes._sampler, "denoise_process_with_generator", fake_denoise)
    monkeypatch.setattr(nodes._enc, "select_frames", fake_frames)
    monkeypatch.setattr(nodes._enc, "video_features", fake_video)
    monkeypatch.setattr(nodes, "_ensure_visual_encoders", lambda *a, **k: None)
    n = nodes.HunyuanFoleySampler()

    def run(bs, **kw):
        return n.generate_audio(_Model(), {"dac_model": None, "siglip2_model": None, "syncformer_model": None}, 8.0, 2.0, "p", "neg", 4.5, 10, "euler", bs, 0, True, **kw)
    return run, calls


def test_node_prompts_encode_like_each_clip_alone(node):
    """Clip k's text rows are what a run of clip k alone conditions on: CLAP over its own [negative, prompt] pair, then
    pad_or_trim_text - whatever the other clips' prompts are (a short prompt next to a long one keeps its own padding)."""
    from foley_amd.host.sampler import pad_or_trim_text
    run, calls = node
    prompts = ["a", "footsteps on gravel, then a long creaking door", "a"]
    negs = ["n", "noisy, harsh", "n"]
    run(3, prompts=prompts, negative_prompts=negs)
    assert calls["clap"] == [["n", "a"], ["noisy, harsh", "footsteps on gravel, then a long creaking door"]]   # distinct pairs once
    visual, text, dur, kw = calls["denoise"]
    assert text["text_feat"].shape[0] == 3 and text["uncond_text_feat"].shape[0] == 3
    for k in range(3):
        solo = _fake_clap([negs[k], prompts[k]])
        assert torch.equal(pad_or_trim_text(text["text_feat"][k:k + 1], 77), pad_or_trim_text(solo[1:], 77)), k
        assert torch.equal(pad_or_trim_text(text["uncond_text_feat"][k:k + 1], 77), pad_or_trim_text(solo[:1], 77)), k
    assert visual["siglip2_feat"].shape == (1, 16, 8) and dur == 2.0 and kw["batch_size"] == 3   # text-to-audio: shared empty rows
    run(2, prompts=["x", "yy"])                                                      # the widget's negative prompt for every clip
    assert calls["clap"][-2:] == [["neg", "x"], ["neg", "yy"]]


def test_node_images_per_clip(node):
    run, calls = node
    run(2, images=[torch.zeros(16, 4, 4, 3), torch.ones(16, 4, 4, 3)], prompts=["a", "b"])
    visual, text, dur, _kw = calls["denoise"]
    assert visual["siglip2_feat"].shape == (2, 16, 8) and dur == 2.0
    with pytest.raises(ValueError, match="share one duration"):
        run(2, images=[torch.zeros(16, 4, 4, 3), torch.zeros(24, 4, 4, 3)])


def test_node_refusals(node):
    run, calls = node
    with pytest.raises(ValueError, match="one per clip"):
        run(3, prompts=["a", "b"])
    with pytest.raises(ValueError, match="one per clip"):
        run(2, images=[torch.zeros(16, 4, 4, 3)])
    with pytest.raises(ValueError, match="features="):
        run(2, prompts=["a", "b"], features={})
    run(2)                                                                          # none given: the widgets, as before
    assert calls["clap"][-1] == ["neg", "p"]
