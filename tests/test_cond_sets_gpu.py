"""Per-clip conditioning on the HIP engine (foley_prepare_sets): a batch whose clips have their own prompts, negative prompts and
visual features against the oracle run on each clip alone; batches whose clips share their conditioning on the unchanged path bit
for bit; the captured graph keyed on the set maps; full-width forwards where 64-row tiles cross many text sets; edit runs."""
import pytest
import torch

import loop_harness as H
from conftest import rel_err
from foley_amd.host import audio_edit, config as C, sampler, synth, tables
from oracle import foley_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 0)


def _conds(cfg, dur, sd, kinds, seed0=10):
    """One synthetic conditioning per clip ('v2a' / 't2a'), each from its own seed."""
    return [synth.synth_conditioning(cfg, dur, t2a=(k == "t2a"), sd=sd, seed=seed0 + 3 * i) for i, k in enumerate(kinds)]


def _run(model, dac, conds, noise, solver, use_graph, edit=None):
    return H.run(model, dac, conds, noise, solver, 10, 4.5, use_graph, edit=edit)


_ORACLE = {}


@pytest.mark.parametrize("solver", ["euler", "heun-2"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_per_clip_batch_matches_oracle(tiny, solver, use_graph):
    """fp32, 3 clips under CFG 4.5, every clip with its own text, negative text, clip and sync features: each clip's latents
    against oracle.sample_latents on that clip alone."""
    sd, _dsd, model, dac, _ = tiny
    conds = _conds(C.TINY, 1.0, sd, ["v2a", "v2a", "v2a"])
    noise = H.noise(3)
    vis, txt = H.batched(conds)
    plan = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 3, solver)
    assert plan["text"].shape[0] == 6 and plan["clip"].shape[0] == 4          # 3 + 3 text sets, 1 + 3 visual sets
    _a, _sr, lat = _run(model, dac, conds, noise, solver, use_graph)
    for k, c in enumerate(conds):
        key = (solver, k)
        if key not in _ORACLE:
            _ORACLE[key] = O.sample_latents(sd, C.TINY.heads, noise[k:k + 1], c["text"], c["uncond_text"], c["clip"], c["sync"],
                                            10, 4.5, solver)
        e = rel_err(lat[k:k + 1], _ORACLE[key])
        print("%s graph=%d clip %d: %.2e" % (solver, use_graph, k, e))
        assert e < 1e-4, (solver, use_graph, k, e)


@pytest.mark.parametrize("use_graph", [False, True])
def test_identical_rows_take_the_unchanged_path(tiny, use_graph):
    """The same conditioning passed as batch_size identical rows equals the batch-1 call bit for bit (latents and audio)."""
    sd, _dsd, model, dac, _ = tiny
    c = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    noise = H.noise(3, 6)
    visn, txtn = H.batched([c, c, c])
    plan = sampler.build_plan(model, visn, txtn, 50, 4.5, 10, 3, "euler")
    assert plan["text_of"] is None and plan["vis_of"] is None and plan["text"].shape[0] == 2
    a1, _, l1 = _run(model, dac, [c], noise, "euler", use_graph)
    an, _, ln = _run(model, dac, [c, c, c], noise, "euler", use_graph)
    assert torch.equal(l1, ln) and torch.equal(a1, an)


def test_graph_replay_across_set_maps_and_layouts(tiny):
    """One context, use_graph=True, one shape, a sequence of set maps that moves between every conditioning layout: per batch
    row for text and visual, permuted; shared conditioning (foley_prepare); per-row text with per-half visual; per-half text
    with per-row visual; and back.  Every run equals its eager run.  A layout change re-allocates the workspace and drops the
    captured iteration (a kept graph would replay the old divisors and buffers); within a layout the maps only change the
    tables and sets foley_prepare_sets rewrites in place, which a replay must read afresh."""
    sd, _dsd, model, dac, _ = tiny
    conds = _conds(C.TINY, 1.0, sd, ["v2a", "t2a", "v2a"], seed0=40)
    conds.append(dict(conds[0], text=conds[1]["text"], uncond_text=conds[1]["uncond_text"]))   # 3: clip 0's video, clip 1's text
    conds.append(dict(conds[2], text=conds[0]["text"], uncond_text=conds[0]["uncond_text"]))   # 4: clip 2's video, clip 0's text
    noise = H.noise(3, 7)
    orders = ((0, 1, 2), (2, 0, 1), (0, 0, 0), (0, 3, 0), (0, 4, 0), (0, 0, 1))
    layouts = {(0, 0, 0): None, (0, 3, 0): "text per row", (0, 4, 0): "visual per row"}
    want = {}
    for o in orders:
        vis, txt = H.batched([conds[i] for i in o])
        plan = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 3, "euler")
        if o in layouts:                                   # the sequence does cover every layout
            per_half = [0, 0, 0, 1, 1, 1]
            assert (plan["text_of"] is None) == (layouts[o] is None)
            if layouts[o] == "text per row":
                assert plan["vis_of"] == per_half and plan["text_of"] != per_half
            if layouts[o] == "visual per row":
                assert plan["text_of"] == per_half and plan["vis_of"] != per_half
        want[o] = _run(model, dac, [conds[i] for i in o], noise, "euler", False)[2].clone()
    for o in orders + orders[:2]:
        got = _run(model, dac, [conds[i] for i in o], noise, "euler", True)[2]
        assert rel_err(got, want[o]) < 1e-6, o
    assert rel_err(want[(0, 1, 2)], want[(2, 0, 1)]) > 1e-2


def test_edit_with_per_clip_prompts(tiny):
    """Strength 0.6 with a span mask and per-clip conditioning: each clip against the oracle edit run of that clip alone."""
    sd, _dsd, model, dac, _ = tiny
    conds = _conds(C.TINY, 1.0, sd, ["v2a", "t2a"], seed0=70)
    g = torch.Generator().manual_seed(8)
    noise, x0 = torch.randn(2, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    mask = audio_edit.build_mask(50, [(0.3, 0.6)], 0.1)
    _a, _sr, lat = _run(model, dac, conds, noise, "heun-2", True, edit=audio_edit.EditSpec(x0, 0.6, mask))
    for k, c in enumerate(conds):
        ref = H.ref_loop(sd, [c], noise[k:k + 1], 10, 4.5, "heun-2", edit=(x0, mask, 0.6)).x
        assert rel_err(lat[k:k + 1], ref) < 1e-4, k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("dur,kinds,sel", [
    (1.0, ["v2a"] * 6, None),                                        # La = 50: a 64-row tile meets up to three text sets
    (2.0, ["t2a", "v2a"], None),                                     # a small grid; Lv = 16 < 64 keeps the attention unfused
    (5.0, ["t2a", "v2a", "v2a", "t2a", "v2a", "t2a", "v2a", "v2a"], [0, 1, 3, 7])])
def test_full_width_forward_with_per_clip_sets(dev, dtype, dur, kinds, sel):
    """xxl width, depth 1+1: one forward (iteration 4 of 10) of a CFG batch whose clips each have their own text (and, for
    'v2a', their own visual features), every selected clip's two halves against the fp32 oracle on the same rounded weights;
    gates of test_model_gpu.py's full-width depth-1+1 tests for the dtype."""
    from foley_amd import nodes
    c = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1, hidden=1536, heads=12)
    sd = synth.synth_dit_state_dict(c)
    model = nodes.HunyuanModelLoader.pack_state_dict(sd, "bf16" if dtype == torch.bfloat16 else "fp16", "none", device=dev, cfg=c)
    sdq = {k: v.float() for k, v in nodes.round_params(sd, dtype).items()}
    tol = 5e-3 if dtype == torch.bfloat16 else 8e-4
    clips = len(kinds)
    La, Lv, Ls = C.lengths(dur, c)
    conds = _conds(c, dur, sd, kinds, seed0=100)
    vis, txt = H.batched(conds)
    x = torch.randn(clips, 128, La, generator=torch.Generator().manual_seed(44)).to(dtype).float()
    steps, it = 10, 4
    model.ctx.prepare(sampler.build_plan(model, vis, txt, La, 4.5, steps, clips, "euler"))
    rows = model.ctx.dit_forward(x.to(dev).contiguous(), it).float().cpu().view(2, clips, La, 128)
    del model
    t_it = tables.model_timesteps(tables.sigma_grid(steps))[it]
    e_clip = sd["empty_clip_feat"].view(1, 1, -1).expand(1, Lv, -1)
    e_sync = sd["empty_sync_feat"].view(1, 1, -1).expand(1, Ls, -1)
    with torch.inference_mode():
        for b in (range(clips) if sel is None else sel):
            cb = conds[b]
            ref = O.dit_forward(sdq, c.heads, torch.cat([x[b:b + 1], x[b:b + 1]]), t_it.expand(2),
                                torch.cat([O.pad_or_trim_text(cb["uncond_text"]), O.pad_or_trim_text(cb["text"])]),
                                torch.cat([e_clip, cb["clip"]]), torch.cat([e_sync, cb["sync"]]))
            e = rel_err(torch.stack([rows[0, b], rows[1, b]]).transpose(1, 2), ref)
            print("%gs x %d %s clip %d (%s): %.2e" % (dur, clips, dtype, b, kinds[b], e))
            assert e < tol, (dur, dtype, b, e)
