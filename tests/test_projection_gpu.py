"""Projected guidance on the HIP engine, end to end (tiny config, fp32, La = 50, 10 steps): APG and CFG-Zero*, eager and graph,
against the loop restated in tests/projection_ref.py at the project's 1e-4 gate; combined with a guidance interval, heun-2, the
multistep history, windows and a step-cache skip list; the per-clip (sharding) claim; the unset state bit for bit with its single
graph; the refusals of foley_set_projected_guidance."""
import pytest
import torch

import loop_harness as H
import projection_ref as P
from conftest import record_parity, rel_err
from foley_amd.host import config as C, long_form, runtime as rt, sampler, tables

pytestmark = pytest.mark.gpu

STEPS, G_SCALE = 10, 4.5
GS, PS = sampler.GuidanceSpec, sampler.ProjectionSpec


@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 3)


_REFS = {}


def _ref(sd, conds, noise, solver="euler", norms=None, **kw):
    """projection_ref.restated_loop under the given conditionings, once per distinct argument set."""
    key = (tuple(id(c) for c in conds), H._key(noise), solver, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFS or norms is not None:
        cat = lambda k: torch.cat([c[k] for c in conds])
        with torch.inference_mode():
            _REFS[key] = P.restated_loop(sd, C.TINY.heads, noise, cat("text"), cat("uncond_text"), cat("clip"), cat("sync"), STEPS, G_SCALE,
                                         solver, shift=C.TINY.flow_shift, norms=norms, **kw)
    return _REFS[key]


def _run(model, dac, conds, noise, spec, solver="euler", use_graph=False, interval=None, **kw):
    g = GS(interval=interval, projection=spec) if spec is not None or interval is not None else None
    return H.run(model, dac, conds, noise, solver, STEPS, G_SCALE, use_graph, **({"guidance": g} if g is not None else {}), **kw)[2].clone()


def _threshold(sd, conds, noise, solver):
    """A norm threshold that clips: half the smallest |m| of the unclipped reference run (momentum -0.5, eta 0)."""
    norms = []
    _ref(sd, conds, noise, solver, norms=norms, mode=P.APG, eta=0.0, momentum=-0.5)
    return 0.5 * float(torch.stack(norms).min())


def _case(name, sd, conds, noise, solver):
    """(ProjectionSpec, the reference loop's keywords) of a named case."""
    if name == "apg":
        return PS("apg", 0.0, -0.5), dict(mode=P.APG, eta=0.0, momentum=-0.5)
    if name == "apg_clip":
        R = _threshold(sd, conds, noise, solver)
        return PS("apg", 0.0, -0.5, R), dict(mode=P.APG, eta=0.0, momentum=-0.5, norm_threshold=R)
    return PS("cfg_zero_star", zero_init=1), dict(mode=P.ZERO_STAR, zero_init=1)


# ----------------------------------------------------------------------------- against the restated loop
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("interval", [None, (0.2, 0.7)])
@pytest.mark.parametrize("solver", ["euler", "heun-2"])
@pytest.mark.parametrize("case", ["apg", "apg_clip", "zero_star"])
def test_matches_the_restated_loop(tiny, case, solver, interval, use_graph):
    """The gate is the project's own for a HIP loop against a restated CPU loop (test_guidance_gpu.py): 1e-4."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    spec, kw = _case(case, sd, conds[:1], noise, solver)
    want = _ref(sd, conds[:1], noise, solver, interval=interval, **kw)
    got = _run(model, dac, conds[:1], noise, spec, solver, use_graph, interval)
    plan = model.ctx.plan
    assert plan["proj_mode"] == tables.PROJECTION_MODES[spec.mode] and tuple(plan["proj_rows"].shape) == (STEPS, 4)
    assert (plan.get("guid_sched") is not None) == (interval is not None)
    e = rel_err(got, want)
    print("%s %s interval %s graph=%d: %.2e" % (case, solver, interval, use_graph, e))
    record_parity("projection.loop.%s.%s%s.%s" % (case, solver, ".interval" if interval else "", "graph" if use_graph else "eager"), rel_err=e)
    assert e < 1e-4, (case, solver, interval, use_graph, e)
    if not use_graph:                                           # the control is far above the gate
        plain = H.ref_loop(sd, conds[:1], noise, STEPS, G_SCALE, solver, shift=C.TINY.flow_shift, **({"interval": interval} if interval else {})).x
        assert rel_err(want, plain) > 1e-2, (case, rel_err(want, plain))


def test_the_threshold_case_clips(tiny):
    sd, _dsd, _model, _dac, conds = tiny
    noise = H.noise()
    R = _threshold(sd, conds[:1], noise, "euler")
    free = _ref(sd, conds[:1], noise, "euler", mode=P.APG, eta=0.0, momentum=-0.5)
    clipped = _ref(sd, conds[:1], noise, "euler", mode=P.APG, eta=0.0, momentum=-0.5, norm_threshold=R)
    assert R > 0 and rel_err(clipped, free) > 1e-2


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("case", ["apg", "zero_star"])
def test_multistep_order_two(tiny, case, use_graph):
    """The ring stores v as the step used it: the projected velocity enters the Adams-Bashforth history."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    spec, kw = _case(case, sd, conds[:1], noise, "euler")
    want = _ref(sd, conds[:1], noise, "euler", order=2, **kw)
    got = _run(model, dac, conds[:1], noise, spec, "euler", use_graph, multistep=sampler.MultistepSpec(2))
    e = rel_err(got, want)
    print("%s multistep 2 graph=%d: %.2e" % (case, use_graph, e))
    assert e < 1e-4, (case, use_graph, e)
    assert rel_err(want, _ref(sd, conds[:1], noise, "euler", **kw)) > 1e-3


# ----------------------------------------------------------------------------- per clip
def test_disjoint_windows_are_the_uncoupled_batch(tiny):
    """Two abutting windows (0, 50): every weight is 1.0 and a window is a clip with its own coefficients and plane rows - the
    latents equal the per-clip batch bit for bit under APG."""
    _sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames([0, 50], 50)
    noise = torch.randn(1, 128, 100, generator=torch.Generator().manual_seed(6))
    spec = PS("apg", 0.25, -0.5, 0.0)
    for solver in ("euler", "heun-2"):
        lat = _run(model, dac, conds[:2], noise, spec, solver, windows=plan)
        per_clip = torch.stack([noise[0, :, s:s + 50] for s in plan.starts])
        l_ref = _run(model, dac, conds[:2], per_clip, spec, solver)
        got = torch.stack([lat[0, :, s:s + 50] for s in plan.starts]).contiguous()
        assert torch.equal(got, l_ref), solver


@pytest.mark.parametrize("case", ["apg", "zero_star"])
def test_a_batch_is_its_clips_one_by_one(tiny, case):
    """The statistics are per clip: three clips in one batch against the same clips (own noise, own conditioning) run alone, each
    at the loop's gate - what sharding a batch over devices relies on."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(3, 7)
    spec, _kw = _case(case, sd, conds[:1], noise[:1], "euler")
    batch = _run(model, dac, conds, noise, spec)
    for b in range(3):
        alone = _run(model, dac, conds[b:b + 1], noise[b:b + 1], spec)
        e = rel_err(batch[b:b + 1], alone)
        print("%s clip %d batch vs alone: %.2e" % (case, b, e))
        assert e < 1e-4, (case, b, e)
    assert rel_err(batch[0:1], batch[1:2]) > 1e-2


# ----------------------------------------------------------------------------- the unset state
def test_unset_is_the_plain_run_with_its_single_graph(tiny):
    """Without a projection the plan carries nothing new, the run keeps its bits - before and after a projected run on the same
    context - and one captured graph serves it; a projected run is another graph, and new row values of its shape keep it."""
    _sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1, 9)
    eager = _run(model, dac, conds[:1], noise, None)
    assert "proj_rows" not in model.ctx.plan and "proj_mode" not in model.ctx.plan
    c0 = H.captures(model)
    plain = _run(model, dac, conds[:1], noise, None, use_graph=True)
    assert H.captures(model) == c0 + 1
    assert torch.equal(_run(model, dac, conds[:1], noise, None, use_graph=True), plain) and H.captures(model) == c0 + 1
    assert rel_err(plain, eager) < 1e-6
    apg = _run(model, dac, conds[:1], noise, PS("apg", 0.0, -0.5), use_graph=True)
    assert H.captures(model) == c0 + 2 and rel_err(apg, plain) > 1e-2
    apg2 = _run(model, dac, conds[:1], noise, PS("apg", 0.5, 0.25, 0.0, 1), use_graph=True)        # new rows, the same graph
    assert H.captures(model) == c0 + 2 and rel_err(apg2, apg) > 1e-3
    assert torch.equal(_run(model, dac, conds[:1], noise, PS("apg", 0.0, -0.5), use_graph=True), apg)
    zs = _run(model, dac, conds[:1], noise, PS("cfg_zero_star"), use_graph=True)                    # another mode: another graph
    assert H.captures(model) == c0 + 3 and rel_err(zs, apg) > 1e-3
    again = _run(model, dac, conds[:1], noise, None, use_graph=True)
    assert torch.equal(again, plain) and H.captures(model) == c0 + 4
    assert torch.equal(_run(model, dac, conds[:1], noise, None, interval=None), eager)


# ----------------------------------------------------------------------------- the step cache
@pytest.mark.parametrize("use_graph", [False, True])
def test_step_cache_skip_list(tiny, use_graph):
    """A skip list under APG: the two launches and the unchanged combine run on skipped iterations too (the momentum average
    advances there), against the restated loop that does the same."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    cache = sampler.StepCacheSpec(skip=(3, 6))
    want = _ref(sd, conds[:1], noise, "euler", mode=P.APG, eta=0.0, momentum=-0.5, cache=cache)
    got = _run(model, dac, conds[:1], noise, PS("apg", 0.0, -0.5), "euler", use_graph, step_cache=cache)
    assert model.ctx.plan["step_cache_report"]["skipped"] == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    e = rel_err(got, want)
    print("apg skip list graph=%d: %.2e" % (use_graph, e))
    assert e < 1e-4, (use_graph, e)
    assert rel_err(want, _ref(sd, conds[:1], noise, "euler", mode=P.APG, eta=0.0, momentum=-0.5)) > 1e-4      # the skips moved the run


# ----------------------------------------------------------------------------- refusals
def test_set_projected_guidance_refusals(tiny, dev):
    sd, _dsd, model, dac, conds = tiny
    vis, txt = H.batched(conds[:1])
    fresh = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    rows = tables.projection_rows(STEPS, "apg")
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        fresh.ctx.set_projected_guidance(1, rows)
    ctx = model.ctx
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, G_SCALE, STEPS, 1, "euler"))
    ctx.set_projected_guidance(1, rows)
    ctx.set_projected_guidance(0)                                  # clears
    bad = rows.clone()
    bad[3, 0] = float("nan")
    neg = rows.clone()
    neg[2, 2] = -1.0
    for mode, r, msg in ((3, rows, "unknown mode"), (1, rows[:-1].contiguous(), "n_rows != n_iter"), (1, None, "n_rows != n_iter"),
                         (2, bad, "non-finite rows"), (1, neg, "R < 0")):
        with pytest.raises(rt.FoleyRuntimeError, match=msg):
            ctx.set_projected_guidance(mode, r)
    # a rescale state next to projection, in either call order
    ctx.set_guidance(None, 0.5)
    with pytest.raises(rt.FoleyRuntimeError, match="rescale state"):
        ctx.set_projected_guidance(1, rows)
    ctx.set_guidance(None, 0.0)
    ctx.set_projected_guidance(1, rows)
    with pytest.raises(rt.FoleyRuntimeError, match="does not combine with projected guidance"):
        ctx.set_guidance(None, 0.5)
    ctx.set_guidance(tables.guidance_schedule(STEPS, G_SCALE, G_SCALE, (0.2, 0.7)), 0.0)     # a schedule does combine
    # foley_prepare clears the state
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, G_SCALE, STEPS, 1, "euler"))
    ctx.set_guidance(None, 0.5)
    ctx.set_guidance(None, 0.0)
    # one half, three halves
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, 1.0, STEPS, 1, "euler"))
    with pytest.raises(rt.FoleyRuntimeError, match="ncfg != 2"):
        ctx.set_projected_guidance(2, rows)
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, G_SCALE, STEPS, 1, "euler", guidance=GS(g_video=3.0)))
    with pytest.raises(rt.FoleyRuntimeError, match="ncfg != 2"):
        ctx.set_projected_guidance(1, rows)
