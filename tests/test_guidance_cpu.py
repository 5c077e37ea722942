"""Separate video / text guidance, guidance schedules and CFG rescale without a GPU: the restated loop of tests/loop_ref.py under
them against the oracle, that every control moves it, the schedule tables, the three-half set maps, the refusals, the C surface."""
import os
import re

import pytest
import torch

import loop_ref as L
from abi_pin import assert_abi_version
from conftest import ROOT, rel_err
from foley_amd import nodes
from foley_amd.host import cond_sets, config as C, runtime as rt, sampler, synth, tables
from loop_harness import ref_loop
from oracle import foley_oracle as O

SOLVERS = ["euler", "heun-2"]


@pytest.fixture(scope="module")
def tiny():
    sd = synth.synth_dit_state_dict(C.TINY)
    c = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
    return sd, c, noise


def _loop(tiny, solver, g_text, **kw):
    """The restated loop of the fixture's clip (memoised by the harness: once per distinct argument set)."""
    sd, c, noise = tiny
    return ref_loop(sd, [c], noise, 10, g_text, solver, **kw).x


@pytest.mark.parametrize("solver", SOLVERS)
def test_restated_loop_at_equal_scales_is_the_oracle_loop(tiny, solver):
    """Three halves at g_video = g_text = 4.5 telescope to u + 4.5 (c - u): the oracle's loop to fp32 rounding; two halves with
    no schedule are its expression exactly."""
    sd, c, noise = tiny
    with torch.inference_mode():
        ref = O.sample_latents(sd, C.TINY.heads, noise, c["text"], c["uncond_text"], c["clip"], c["sync"], 10, 4.5, solver)
    e3 = rel_err(_loop(tiny, solver, g_text=4.5, g_video=4.5), ref)
    print("%s three halves 4.5 / 4.5 vs oracle: %.2e" % (solver, e3))
    assert e3 <= 1e-5, (solver, e3)
    assert torch.equal(_loop(tiny, solver, g_text=4.5), ref)


@pytest.mark.parametrize("solver", SOLVERS)
def test_every_control_moves_the_loop(tiny, solver):
    base3, base2 = _loop(tiny, solver, g_text=4.5, g_video=4.5), _loop(tiny, solver, g_text=4.5)
    moved = {
        "scales 7 / 2": rel_err(_loop(tiny, solver, g_text=2.0, g_video=7.0), base3),
        "interval, iterations 2-6": rel_err(_loop(tiny, solver, g_text=4.5, interval=(0.2, 0.7)), base2),
        "rescale 0.7": rel_err(_loop(tiny, solver, g_text=4.5, rescale=0.7), base2),
    }
    print(solver, {k: "%.2e" % v for k, v in moved.items()})
    for k, v in moved.items():
        assert v > 1e-2, (solver, k, v)


@pytest.mark.parametrize("solver", list(tables.SOLVERS))
def test_schedule_tables(solver):
    """One row per LOOP iteration (a multi-stage solver counts its stages, as its coefficient rows do), the run's scales inside
    start <= i / n_iter < end and (1, 1) outside, fp32."""
    for steps in (10, 12, 7):
        n_iter = tables.build_tables(50, 8, 24, 77, steps, solver, 1.0)["solver_coef"].shape[0]
        for interval in (None, (0.0, 1.0), (0.2, 0.7), (0.0, 0.5), (0.35, 1.0)):
            t = tables.guidance_schedule(n_iter, 7.0, 2.5, interval)
            assert t.dtype == torch.float32 and tuple(t.shape) == (n_iter, 2) and n_iter == steps
            assert t.tolist() == [list(r) for r in L.schedule_ref(n_iter, 7.0, 2.5, interval)], (solver, steps, interval)
    t = tables.guidance_schedule(10, 7.0, 2.0, (0.2, 0.7))
    assert [i for i in range(10) if t[i, 0] == 7.0] == [2, 3, 4, 5, 6] and bool((t[[0, 1, 7, 8, 9]] == 1.0).all())
    for bad in ((0.5, 0.5), (-0.1, 0.5), (0.2, 1.1), (0.7, 0.2)):
        with pytest.raises(ValueError):
            tables.guidance_schedule(10, 7.0, 2.0, bad)
    with pytest.raises(ValueError):
        tables.guidance_schedule(0, 7.0, 2.0)


def _feats(n, seed, Lt=77, Lv=8, Ls=24, D=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(n, Lt, D), r(n, Lt, D), r(n, Lv, D), r(n, Ls, D)


def test_three_half_set_maps():
    e_clip, e_sync = torch.full((16,), 0.25), torch.full((16,), -0.5)
    # shared conditioning (given as identical rows): the homogeneous plan, now with three sets
    text, unc, clip, sync = (t.repeat(3, 1, 1) for t in _feats(1, 1))
    s = cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 3, True, three=True)
    assert s.homogeneous and s.text.shape[0] == 3 and s.clip.shape[0] == 3 and s.sync.shape[0] == 3
    assert torch.equal(s.text[0], unc[0]) and torch.equal(s.text[1], unc[0]) and torch.equal(s.text[2], text[0])
    assert torch.equal(s.clip[0], e_clip.expand(8, -1)) and torch.equal(s.clip[1], clip[0]) and torch.equal(s.clip[2], clip[0])
    assert torch.equal(s.sync[0], e_sync.expand(24, -1)) and torch.equal(s.sync[1], sync[0]) and torch.equal(s.sync[2], sync[0])
    # per-clip prompts, one video: text per row (de-duplicated per half), visual per half
    text, unc, _, _ = _feats(3, 2)
    unc[2] = unc[0]
    _, _, clip, sync = _feats(1, 3)
    s = cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 3, True, three=True)
    assert s.vis_of == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert s.text_of == [0, 1, 0, 2, 3, 2, 4, 5, 6] and s.text.shape[0] == 7
    for b, k in enumerate([0, 1, 2] * 3):
        assert torch.equal(s.text[s.text_of[b]], (unc if b < 6 else text)[k])
    # per-clip videos, one prompt: visual per row - one empty set, then every clip's features once per upper half
    text, unc, _, _ = _feats(1, 4)
    _, _, clip, sync = _feats(2, 5)
    s = cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 2, True, three=True)
    assert s.text_of == [0, 0, 1, 1, 2, 2] and s.vis_of == [0, 0, 1, 2, 3, 4] and s.clip.shape[0] == 5
    for b, k in ((2, 0), (3, 1), (4, 0), (5, 1)):
        assert torch.equal(s.clip[s.vis_of[b]], clip[k]) and torch.equal(s.sync[s.vis_of[b]], sync[k])
    assert torch.equal(s.clip[0], e_clip.expand(8, -1))
    # the default is the two-half build, and three halves are a form of CFG
    s2 = cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 2, True)
    assert s2.text_of == [0, 0, 1, 1] and s2.vis_of == [0, 0, 1, 2]
    with pytest.raises(cond_sets.CondSetsError):
        cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 2, False, three=True)


def test_per_clip_videos_take_at_most_ten_clips_under_three_halves():
    e_clip, e_sync = torch.zeros(16), torch.zeros(16)
    text, unc, _, _ = _feats(1, 6)
    _, _, clip, sync = _feats(11, 7)
    with pytest.raises(cond_sets.CondSetsError, match=r"10 clips with three guidance halves"):
        cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 11, True, three=True)
    s = cond_sets.build(text, unc, clip[:10], sync[:10], e_clip, e_sync, 10, True, three=True)
    assert len(s.vis_of) == 30 and s.clip.shape[0] == 21
    assert len(cond_sets.build(text, unc, clip, sync, e_clip, e_sync, 11, True).vis_of) == 22     # two halves: 16 clips, as before


def test_node_and_spec_refusals():
    node = nodes.HunyuanFoleySampler()
    args = (None, None, 16, 1.0, "p", "n")
    tail = (10, "euler", 1, 0, True)
    with pytest.raises(ValueError, match="video_cfg_scale needs visual input"):
        node.generate_audio(*args, 4.5, *tail, video_cfg_scale=3.0)
    for kw in ({"guidance_interval": (0.2, 0.7)}, {"cfg_rescale": 0.7}, {"guidance_interval": (0.0, 0.5), "cfg_rescale": 0.3}):
        with pytest.raises(ValueError, match="needs guidance: guidance_scale > 1 or a video scale"):
            node.generate_audio(*args, 1.0, *tail, **kw)
    with pytest.raises(ValueError, match=r"rescale must lie in \[0, 1\]"):
        node.generate_audio(*args, 4.5, *tail, cfg_rescale=1.5)
    with pytest.raises(ValueError):
        sampler.GuidanceSpec(rescale=0.5).check(1.0)
    with pytest.raises(ValueError):
        sampler.GuidanceSpec(interval=(0.1, 0.9)).check(1.0)
    sampler.GuidanceSpec(g_video=3.0, rescale=0.5).check(1.0)          # a video scale alone is guidance
    sampler.GuidanceSpec(interval=(0.1, 0.9), rescale=1.0).check(4.5)


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    lib = rt.load_library()
    for name in ("foley_set_guidance", "foley_op_solver_step", "foley_op_guidance_stats", "foley_op_guidance_stats_work"):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", hdr), name
        assert name in rt.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "typedef struct foley_guidance_desc" in hdr and "typedef struct foley_step_desc" in hdr
    assert re.search(r"\bfoley_guidance_desc gd;", hdr)          # the step's descriptor carries the guidance descriptor
    assert_abi_version()
    assert lib.foley_op_guidance_stats_work(1, 50) == 2 * 5 and lib.foley_op_guidance_stats_work(8, 3000) == 8 * 94 * 5
