"""Separate video / text guidance, guidance schedules and CFG rescale on the HIP engine, end to end: against the restated loop
of tests/loop_ref.py (the oracle's forward under the new combine), per-clip conditioning under three halves, the unset and
the constant-schedule states bit for bit, the keying of the captured graph, three halves at full width, the refusals."""
import pytest
import torch

import loop_harness as H
from abi_pin import assert_abi_version
from conftest import record_parity, rel_err
from foley_amd.host import audio_edit, config as C, long_form, runtime as rt, sampler, synth, tables
from oracle import foley_oracle as O

pytestmark = pytest.mark.gpu

Spec = sampler.GuidanceSpec
CASES = {                                                   # name -> (cfg_scale = text scale, spec)
    "three halves 7 / 2": (2.0, Spec(g_video=7.0)),
    "interval": (4.5, Spec(interval=(0.2, 0.7))),
    "rescale 0.7": (4.5, Spec(rescale=0.7)),
    "all three": (2.0, Spec(g_video=7.0, interval=(0.2, 0.7), rescale=0.7)),
}


@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 2)


def _run(model, dac, conds, noise, solver, scale, spec, use_graph=False, **kw):
    return H.run(model, dac, conds, noise, solver, 10, scale, use_graph, guidance=spec, **kw)


def _loop(sd, conds, noise, solver, scale, spec, **kw):
    """The restated loop of 10 iterations under a GuidanceSpec's controls."""
    return H.ref_loop(sd, conds, noise, 10, scale, solver, g_video=spec.g_video, interval=spec.interval, rescale=spec.rescale, **kw).x


# ----------------------------------------------------------------------------- against the restated loop
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("solver", ["euler", "heun-2"])
def test_matches_the_restated_loop(tiny, solver, use_graph, case):
    sd, _dsd, model, dac, conds = tiny
    scale, spec = CASES[case]
    noise = H.noise(1)
    want = _loop(sd, conds[:1], noise, solver, scale, spec)
    _a, _sr, lat = _run(model, dac, conds[:1], noise, solver, scale, spec, use_graph)
    assert model.ctx.plan["ncfg"] == (3 if spec.g_video is not None else 2)
    e = rel_err(lat, want)
    print("%s %s graph=%d: %.2e" % (case, solver, use_graph, e))
    assert e < 1e-4, (case, solver, use_graph, e)
    plain = _loop(sd, conds[:1], noise, solver, 4.5, Spec())
    assert rel_err(want, plain) > 1e-2                       # the control is far above the gate


@pytest.mark.parametrize("use_graph", [False, True])
def test_per_clip_conditioning_under_three_halves(tiny, use_graph):
    """Two clips with their own videos and prompts: six batch rows laid out per row, each clip against the loop on it alone."""
    sd, _dsd, model, dac, conds = tiny
    scale, spec = CASES["all three"]
    noise = H.noise(2, 6)
    vis, txt = H.batched(conds)
    plan = sampler.build_plan(model, vis, txt, 50, scale, 10, 2, "heun-2", guidance=spec)
    assert plan["ncfg"] == 3 and plan["vis_of"] == [0, 0, 1, 2, 3, 4] and plan["text_of"] == [0, 1, 2, 3, 4, 5]
    _a, _sr, lat = _run(model, dac, conds, noise, "heun-2", scale, spec, use_graph)
    for k, c in enumerate(conds):
        e = rel_err(lat[k:k + 1], _loop(sd, [c], noise[k:k + 1], "heun-2", scale, spec))
        print("graph=%d clip %d: %.2e" % (use_graph, k, e))
        assert e < 1e-4, (use_graph, k, e)


# ----------------------------------------------------------------------------- the unset state and the constant table: the plain bits
@pytest.mark.parametrize("use_graph", [False, True])
def test_constant_schedule_is_the_plain_run(tiny, use_graph):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(2, 7)
    a0, _, l0 = _run(model, dac, conds[:1], noise, "heun-2", 4.5, None, use_graph)
    a1, _, l1 = _run(model, dac, conds[:1], noise, "heun-2", 4.5, Spec(interval=(0.0, 1.0)), use_graph)
    assert model.ctx.plan.get("guid_sched") is not None and bool((model.ctx.plan["guid_sched"] == 4.5).all())
    assert torch.equal(l0, l1) and torch.equal(a0, a1)
    a2, _, l2 = _run(model, dac, conds[:1], noise, "heun-2", 4.5, Spec(), use_graph)       # an empty spec sets nothing
    assert torch.equal(l0, l2) and torch.equal(a0, a2)


def test_constant_schedule_is_the_plain_edit_run_and_windowed_run(tiny):
    sd, _dsd, model, dac, conds = tiny
    const = Spec(interval=(0.0, 1.0))
    g = torch.Generator().manual_seed(8)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    edit = audio_edit.EditSpec(x0, 0.6, audio_edit.build_mask(50, [(0.3, 0.6)], 0.1))
    for use_graph in (False, True):
        a0, _, l0 = _run(model, dac, conds[:1], noise, "heun-2", 4.5, None, use_graph, edit=edit)
        a1, _, l1 = _run(model, dac, conds[:1], noise, "heun-2", 4.5, const, use_graph, edit=edit)
        assert model.ctx.plan["guid_sched"].shape[0] == model.ctx.plan["n_iter"] < 10       # the suffix of the plain run's rows
        assert torch.equal(l0, l1) and torch.equal(a0, a1)
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    wn = torch.randn(1, 128, plan.Ltot, generator=g)
    three = [conds[0], conds[1], conds[0]]
    for use_graph in (False, True):
        a0, _, l0 = _run(model, dac, three, wn, "euler", 4.5, None, use_graph, windows=plan)
        a1, _, l1 = _run(model, dac, three, wn, "euler", 4.5, const, use_graph, windows=plan)
        assert l0.shape == (1, 128, 95) and torch.equal(l0, l1) and torch.equal(a0, a1)


def test_guidance_with_edit_and_with_windows(tiny):
    """The controls act in edit runs and windowed runs (set in either order with their state), graph replay equals eager, and
    the eager run lies within the loop gate of the restated loop under the same options."""
    sd, _dsd, model, dac, conds = tiny
    scale, spec = CASES["all three"]
    g = torch.Generator().manual_seed(9)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    edit = audio_edit.EditSpec(x0, 0.6, audio_edit.build_mask(50, [(0.3, 0.6)], 0.1))
    e0 = _run(model, dac, conds[:1], noise, "heun-2", scale, spec, False, edit=edit)[2]
    e1 = _run(model, dac, conds[:1], noise, "heun-2", scale, spec, True, edit=edit)[2]
    base = _run(model, dac, conds[:1], noise, "heun-2", 4.5, None, False, edit=edit)[2]
    assert rel_err(e1, e0) < 1e-6 and rel_err(e0, base) > 1e-2
    e_edit = rel_err(e0, _loop(sd, conds[:1], noise, "heun-2", scale, spec, edit=(x0, edit.mask, 0.6)))
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    wn = torch.randn(1, 128, plan.Ltot, generator=g)
    three = [conds[0], conds[1], conds[0]]
    w0 = _run(model, dac, three, wn, "euler", scale, spec, False, windows=plan)[2]
    w1 = _run(model, dac, three, wn, "euler", scale, spec, True, windows=plan)[2]
    wb = _run(model, dac, three, wn, "euler", 4.5, None, False, windows=plan)[2]
    assert rel_err(w1, w0) < 1e-6 and rel_err(w0, wb) > 1e-2
    e_win = rel_err(w0, _loop(sd, three, wn, "euler", scale, spec, windows=plan))
    print("guidance with an edit: %.2e, with windows: %.2e" % (e_edit, e_win))
    record_parity("loop.guidance.edit", rel_err=e_edit)
    record_parity("loop.guidance.windows", rel_err=e_win)
    assert e_edit < 1e-4 and e_win < 1e-4, (e_edit, e_win)
    # the other call order on the context itself: windows first, guidance second
    vis, txt = H.batched(three)
    vis = {k: sampler.window_rows(v, 1, 3, k) for k, v in vis.items()}
    txt = {k: sampler.window_rows(v, 1, 3, k) for k, v in txt.items()}
    pl = sampler.build_plan(model, vis, txt, 50, scale, 10, 3, "euler", edit_i0=0, guidance=spec)
    model.ctx.prepare(pl)
    model.ctx.set_windows(plan.starts, plan.weights.to(model.device))
    sampler.apply_guidance(model.ctx, pl)
    lat = torch.stack([wn[0, :, s:s + 50] for s in plan.starts]).to(model.device).contiguous()
    model.ctx.sample(lat, use_graph=True)
    st = rt.op_windows_stitch(lat, torch.tensor(plan.starts, dtype=torch.int32, device=model.device), plan.weights.to(model.device), plan.Ltot)
    assert rel_err(st, w0) < 1e-6


# ----------------------------------------------------------------------------- graph keying
def test_graph_keyed_on_the_guidance_state(tiny):
    """One context, use_graph=True: plain -> three halves -> rescale on -> new schedule values -> plain; every run equals its eager
    run.  New values of the same shape only rewrite the table a replay reads: the captured iteration and every buffer stay."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1, 11)
    seq = [(4.5, None), (2.0, Spec(g_video=7.0)), (2.0, Spec(g_video=7.0, rescale=0.7)), (3.0, Spec(g_video=5.0, rescale=0.4, interval=(0.1, 0.8))),
           (4.5, None)]
    want = [_run(model, dac, conds[:1], noise, "euler", s, sp, False)[2].clone() for s, sp in seq]
    for (s, sp), w in zip(seq, want):
        got = _run(model, dac, conds[:1], noise, "euler", s, sp, True)[2]
        assert rel_err(got, w) < 1e-6, (s, sp)
    for i in range(len(seq)):
        for j in range(i + 1, len(seq) - 1):
            assert rel_err(want[i], want[j]) > 1e-3, (i, j)
    assert torch.equal(want[0], want[-1])

    state = lambda: H.run_state(model)
    # the same shape with new values - the text scale included, which a table replaces: no new capture, every buffer where it was
    a = _run(model, dac, conds[:1], noise, "euler", 2.0, Spec(g_video=7.0, rescale=0.7), True)[2].clone()
    s0 = state()
    b = _run(model, dac, conds[:1], noise, "euler", 3.0, Spec(g_video=5.0, rescale=0.4, interval=(0.1, 0.8)), True)[2].clone()
    assert state() == s0 and all(s0[1:])
    assert rel_err(a, want[2]) < 1e-6 and rel_err(b, want[3]) < 1e-6
    # the rewrite-only path: the prepared plan stays, a new table through set_guidance, and the replay reads it
    model.ctx.set_guidance(tables.guidance_schedule(10, 7.0, 2.0), 0.7)
    lat = noise.to(model.device).contiguous()
    model.ctx.sample(lat, use_graph=True)
    assert state() == s0 and rel_err(lat, want[2]) < 1e-6
    # without a table the scalar is a launch argument: another text scale is another capture
    _run(model, dac, conds[:1], noise, "euler", 4.5, None, True)
    s1 = state()
    _run(model, dac, conds[:1], noise, "euler", 3.5, None, True)
    assert state()[0] == s1[0] + 1
    assert_abi_version()


def test_set_guidance_refusals(tiny, dev):
    sd, _dsd, model, dac, conds = tiny
    vis, txt = H.batched(conds[:1])
    ctx = model.ctx
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, 1.0, 10, 1, "euler"))                # one half
    with pytest.raises(rt.FoleyRuntimeError, match="one half"):
        ctx.set_guidance(tables.guidance_schedule(10, 2.0, 2.0), 0.0)
    ctx.set_guidance(None, 0.0)                                                              # clearing is always allowed
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler"))
    with pytest.raises(rt.FoleyRuntimeError, match="n_rows == n_iter"):
        ctx.set_guidance(tables.guidance_schedule(9, 2.0, 2.0), 0.0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(rt.FoleyRuntimeError, match="rescale must lie"):
            ctx.set_guidance(None, bad)
    with pytest.raises(rt.FoleyRuntimeError, match=r"\[n_iter, 2\]"):
        ctx.set_guidance(torch.zeros(10, 3), 0.0)
    fresh = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        fresh.set_guidance(None, 0.5)
    with pytest.raises(ValueError):
        sampler.build_plan(model, vis, txt, 50, 1.0, 10, 1, "euler", guidance=Spec(rescale=0.5))


# ----------------------------------------------------------------------------- full width
def test_three_halves_at_full_width(dev):
    """xxl width, depth 1+1: one forward of a three-half batch at 5 s (M = 750 rows) and at 1 s (La = 50: 150 rows, three text
    sets under 64-row tiles - the cross-attention takes the unfused path by gemm_plan.h's rule) against O.dit_forward on
    [nothing ; video ; video + prompt]; gates of test_model_gpu.py::test_full_size_properties_v2a."""
    c11 = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1)
    sd11 = synth.synth_dit_state_dict(c11)
    it, steps = 3, 10
    t_it = tables.model_timesteps(tables.sigma_grid(steps))[it]
    models = {dt: sampler.FoleyModel(c11, sd11, dt, dev) for dt in (torch.float32, torch.bfloat16)}
    for dur in (5.0, 1.0):
        La, Lv, Ls = C.lengths(dur, c11)
        cond = synth.synth_conditioning(c11, dur, t2a=False, sd=sd11)
        vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
        txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
        x = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(31))
        text77, unc77 = O.pad_or_trim_text(cond["text"]), O.pad_or_trim_text(cond["uncond_text"])
        e_clip = sd11["empty_clip_feat"].view(1, 1, -1).expand(1, Lv, -1)
        e_sync = sd11["empty_sync_feat"].view(1, 1, -1).expand(1, Ls, -1)
        with torch.inference_mode():
            ref = O.dit_forward(sd11, c11.heads, torch.cat([x, x, x]), t_it.expand(3), torch.cat([unc77, unc77, text77]),
                                torch.cat([e_clip, cond["clip"], cond["clip"]]), torch.cat([e_sync, cond["sync"], cond["sync"]]))
        ref_rows = ref.transpose(1, 2).reshape(3 * La, 128)
        assert rel_err(ref_rows[La:2 * La], ref_rows[:La]) > 1e-3 and rel_err(ref_rows[2 * La:], ref_rows[La:2 * La]) > 1e-3
        for dtype, tol in ((torch.float32, 2e-5), (torch.bfloat16, 4e-2)):
            m = models[dtype]
            plan = sampler.build_plan(m, vis, txt, La, 2.0, steps, 1, "euler", guidance=Spec(g_video=7.0))
            assert plan["ncfg"] == 3 and plan["text"].shape[0] == 3
            m.ctx.prepare(plan)
            xin = x.to(dtype).float() if dtype != torch.float32 else x
            rows = m.ctx.dit_forward(xin.to(dev).contiguous(), it)
            assert rows.shape[0] == 3 * La
            e = rel_err(rows, ref_rows)
            print("xxl-1-1 three halves, %g s (M = %d), %s: %.2e" % (dur, 3 * La, dtype, e))
            assert e < tol, (dur, dtype, e)
