"""The step cache on the HIP engine, end to end: schedule and threshold mode against the restated loop of tests/loop_ref.py
(the oracle's forward under the cached iteration), the armed-but-idle and unset states bit for bit, the keying of the captured
graphs, the combinations with guidance and per-clip conditioning, full width in fp32 and bf16, the refusals.

Fixtures of tests/test_guidance_gpu.py: C.TINY in fp32, La = 50, conditioning seed 10, noise seed 5, CFG 4.5.  On them the
per-iteration change is 0.10 - 0.16 and an alternate-skip run lies 1.8e-2 (20 euler steps) / 1.5e-2 (10 heun-2 steps) from the plain
run - two orders above the 1e-4 gate of the end-to-end comparisons (the gate of the guidance tests)."""
import ctypes

import pytest
import torch

import loop_harness as H
import loop_ref as L
from abi_pin import assert_abi_version
from conftest import record_parity, rel_err
from foley_amd.host import audio_edit, config as C, long_form, runtime as rt, sampler, step_cache as S, synth

pytestmark = pytest.mark.gpu

Spec, Guid = sampler.StepCacheSpec, sampler.GuidanceSpec
RUNS = {"euler": 20, "heun-2": 10}                          # solver -> model calls
THRESHOLDS = {"euler": 0.25, "heun-2": 0.3}                 # chosen from the reference loop alone: see test_threshold_mode


def alternate(n):
    return Spec(skip=tuple(range(1, n, 2)))


@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 2)


def _run(model, dac, conds, noise, solver, steps, spec, use_graph=False, scale=4.5, **kw):
    return H.run(model, dac, conds, noise, solver, steps, scale, use_graph, step_cache=spec, **kw)


def _ref(sd, conds, noise, solver, steps, spec, scale=4.5, **kw):
    """The restated loop of the given clips (conditioning batched per clip) under the spec: (x, info)."""
    ref = H.ref_loop(sd, conds, noise, steps, scale, solver, cache=spec, **kw)
    return ref.x, ref.info


# ----------------------------------------------------------------------------- schedule mode against the restated loop
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("solver", list(RUNS))
def test_schedule_mode_matches_the_restated_loop(tiny, solver, use_graph):
    sd, _dsd, model, dac, conds = tiny
    n = RUNS[solver]
    noise = H.noise(1)
    want, info = _ref(sd, conds[:1], noise, solver, n, alternate(n))
    plain, _ = _ref(sd, conds[:1], noise, solver, n, None)
    assert rel_err(want, plain) > 1e-2                       # the control, on the references alone: far above the gate
    _a, _sr, lat = _run(model, dac, conds[:1], noise, solver, n, alternate(n), use_graph)
    rep = model.ctx.plan["step_cache_report"]
    e = rel_err(lat, want)
    print("%s / %d graph=%d: %.2e (cached vs plain reference %.2e)" % (solver, n, use_graph, e, rel_err(want, plain)))
    assert rep["skipped"] == info["skipped"] and sum(rep["skipped"]) == n // 2 - 1 + n % 2
    assert all(r == -1.0 for r in rep["rel"])               # schedule mode reads nothing back
    assert e < 1e-4, (solver, use_graph, e)


# ----------------------------------------------------------------------------- threshold mode
def _run_lengths(skipped):
    runs, k = [], 0
    for s in skipped + [0]:
        if s:
            k += 1
        elif k:
            runs.append(k)
            k = 0
    return runs


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("solver", list(RUNS))
def test_threshold_mode(tiny, solver, use_graph):
    """The threshold of each run is one whose accumulated sums stay >= 2 % away from it on every decided iteration of the REFERENCE
    loop (euler / 20 at 0.25: 4.1 %; heun-2 / 10 at 0.3: 6.5 %): the library's fp32 change measure is ~1e-6 from fp64, so no decision
    can flip.  The margin is re-derived here - a changed synthesiser fails loudly instead of silently flipping."""
    sd, _dsd, model, dac, conds = tiny
    n, th = RUNS[solver], THRESHOLDS[solver]
    noise = H.noise(1)
    want, info = _ref(sd, conds[:1], noise, solver, n, Spec(threshold=th))
    mg = L.margin(info, th)
    assert mg >= 0.02, (solver, th, mg)
    sk = info["skipped"]
    assert sum(sk) >= 3 and sk.count(0) >= 3 and 2 in _run_lengths(sk), sk
    _a, _sr, lat = _run(model, dac, conds[:1], noise, solver, n, Spec(threshold=th), use_graph)
    rep = model.ctx.plan["step_cache_report"]
    e = rel_err(lat, want)
    worst = max(abs(g - w) / w for g, w in zip(rep["rel"][1:], info["rel"][1:]))
    print("%s / %d threshold %g graph=%d: margin %.3f, pattern %s, rel within %.2e, latents %.2e" % (solver, n, th, use_graph, mg, sk, worst, e))
    assert rep["skipped"] == sk
    assert rep["rel"][0] == -1.0 and worst < 1e-4
    assert e < 1e-4, (solver, use_graph, e)


# ----------------------------------------------------------------------------- unset / armed but idle: the plain bits
IDLE = {"threshold 0": Spec(threshold=0.0), "empty list": Spec(skip=())}


@pytest.mark.parametrize("idle", list(IDLE))
@pytest.mark.parametrize("use_graph", [False, True])
def test_armed_but_idle_is_the_plain_run(tiny, use_graph, idle):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(2, 7)
    a0, _, l0 = _run(model, dac, conds[:1], noise, "heun-2", 10, None, use_graph)
    a1, _, l1 = _run(model, dac, conds[:1], noise, "heun-2", 10, IDLE[idle], use_graph)
    assert model.ctx.plan["step_cache_report"]["skipped"] == [0] * 10
    assert torch.equal(l0, l1) and torch.equal(a0, a1)


def test_armed_but_idle_is_the_plain_edit_run_and_windowed_run(tiny):
    sd, _dsd, model, dac, conds = tiny
    g = torch.Generator().manual_seed(8)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    edit = audio_edit.EditSpec(x0, 0.6, audio_edit.build_mask(50, [(0.3, 0.6)], 0.1))
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    wn = torch.randn(1, 128, plan.Ltot, generator=g)
    three = [conds[0], conds[1], conds[0]]
    for use_graph in (False, True):
        a0, _, l0 = _run(model, dac, conds[:1], noise, "heun-2", 10, None, use_graph, edit=edit)
        w0a, _, w0 = _run(model, dac, three, wn, "euler", 10, None, use_graph, windows=plan)
        for spec in IDLE.values():
            a1, _, l1 = _run(model, dac, conds[:1], noise, "heun-2", 10, spec, use_graph, edit=edit)
            assert len(model.ctx.plan["step_cache_report"]["skipped"]) == model.ctx.plan["n_iter"] < 10   # the suffix of the plain run
            assert torch.equal(l0, l1) and torch.equal(a0, a1)
            w1a, _, w1 = _run(model, dac, three, wn, "euler", 10, spec, use_graph, windows=plan)
            assert w0.shape == (1, 128, 95) and torch.equal(w0, w1) and torch.equal(w0a, w1a)


def test_skipping_acts_in_edit_and_windowed_runs(tiny):
    """The cache moves edit runs and windowed runs too (their step forms follow a skipped iteration), graph replay equals eager."""
    sd, _dsd, model, dac, conds = tiny
    g = torch.Generator().manual_seed(9)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    edit = audio_edit.EditSpec(x0, 0.6, audio_edit.build_mask(50, [(0.3, 0.6)], 0.1))
    spec = alternate(10)
    e0 = _run(model, dac, conds[:1], noise, "heun-2", 10, spec, False, edit=edit)[2]
    sk = model.ctx.plan["step_cache_report"]["skipped"]
    i0 = 10 - len(sk)
    assert sk == [0] + [(i0 + i) % 2 for i in range(1, len(sk) - 1)] + [0]      # rows [i0, 10) of the list, the first one full
    e1 = _run(model, dac, conds[:1], noise, "heun-2", 10, spec, True, edit=edit)[2]
    base = _run(model, dac, conds[:1], noise, "heun-2", 10, None, False, edit=edit)[2]
    assert rel_err(e1, e0) < 1e-6 and rel_err(e0, base) > 1e-3
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    wn = torch.randn(1, 128, plan.Ltot, generator=g)
    three = [conds[0], conds[1], conds[0]]
    w0 = _run(model, dac, three, wn, "euler", 10, spec, False, windows=plan)[2]
    w1 = _run(model, dac, three, wn, "euler", 10, spec, True, windows=plan)[2]
    wb = _run(model, dac, three, wn, "euler", 10, None, False, windows=plan)[2]
    assert rel_err(w1, w0) < 1e-6 and rel_err(w0, wb) > 1e-3


# ----------------------------------------------------------------------------- graph keying
def test_graphs_keyed_on_cache_on_off_only(tiny):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1, 11)
    p0 = _run(model, dac, conds[:1], noise, "euler", 20, None, True)[2].clone()
    s0 = H.run_state(model)
    assert torch.equal(_run(model, dac, conds[:1], noise, "euler", 20, None, True)[2], p0)
    assert H.run_state(model) == s0                               # unset: one captured iteration, replayed - as ever
    c0 = _run(model, dac, conds[:1], noise, "euler", 20, alternate(20), True)[2].clone()
    s1 = H.run_state(model)
    assert s1[0] == s0[0] + 1                                # cache on: another key, one new capture (of the three graphs)
    # a new list, then threshold mode with two thresholds: host decisions between the replays - the captured graphs stay
    c1 = _run(model, dac, conds[:1], noise, "euler", 20, Spec(skip=(3, 4, 9)), True)[2].clone()
    c2 = _run(model, dac, conds[:1], noise, "euler", 20, Spec(threshold=0.25), True)[2].clone()
    c3 = _run(model, dac, conds[:1], noise, "euler", 20, Spec(threshold=0.4, max_consecutive=3), True)[2].clone()
    assert H.run_state(model) == s1
    outs = [p0, c0, c1, c2, c3]
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert rel_err(outs[i], outs[j]) > 1e-3, (i, j)
    for spec, w in ((alternate(20), c0), (Spec(skip=(3, 4, 9)), c1), (Spec(threshold=0.25), c2)):
        assert rel_err(_run(model, dac, conds[:1], noise, "euler", 20, spec, False)[2], w) < 1e-6       # each equals its eager run
    # plain -> cached -> plain on one context: the two plain runs are bit-equal
    assert torch.equal(_run(model, dac, conds[:1], noise, "euler", 20, None, True)[2], p0)
    assert_abi_version()


# ----------------------------------------------------------------------------- combinations
@pytest.mark.parametrize("use_graph", [False, True])
def test_three_halves_and_rescale_under_a_schedule(tiny, use_graph):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1)
    guid = dict(g_video=7.0, rescale=0.7)
    want, info = _ref(sd, conds[:1], noise, "heun-2", 10, alternate(10), scale=2.0, **guid)
    plain, _ = _ref(sd, conds[:1], noise, "heun-2", 10, None, scale=2.0, **guid)
    assert rel_err(want, plain) > 1e-2
    _a, _sr, lat = _run(model, dac, conds[:1], noise, "heun-2", 10, alternate(10), use_graph, scale=2.0, guidance=Guid(**guid))
    assert model.ctx.plan["ncfg"] == 3 and model.ctx.plan["step_cache_report"]["skipped"] == info["skipped"]
    e = rel_err(lat, want)
    print("three halves + rescale, alternate, graph=%d: %.2e" % (use_graph, e))
    assert e < 1e-4, (use_graph, e)


def test_three_halves_threshold_mode_takes_the_max_over_three_rows(tiny):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1)
    guid = dict(g_video=7.0, rescale=0.7)
    th = _pick_threshold(lambda t: _ref(sd, conds[:1], noise, "heun-2", 10, Spec(threshold=t), scale=2.0, **guid)[1])
    want, info = _ref(sd, conds[:1], noise, "heun-2", 10, Spec(threshold=th), scale=2.0, **guid)
    _a, _sr, lat = _run(model, dac, conds[:1], noise, "heun-2", 10, Spec(threshold=th), True, scale=2.0, guidance=Guid(**guid))
    rep = model.ctx.plan["step_cache_report"]
    assert rep["skipped"] == info["skipped"] and sum(rep["skipped"]) >= 2
    assert max(abs(g - w) / w for g, w in zip(rep["rel"][1:], info["rel"][1:])) < 1e-4
    assert rel_err(lat, want) < 1e-4


def _pick_threshold(info_of, candidates=(0.3, 0.25, 0.2, 0.35, 0.4, 0.15)):
    """The first candidate whose reference loop skips at least twice and keeps every decided sum >= 2 % from the threshold."""
    for t in candidates:
        info = info_of(t)
        if sum(info["skipped"]) >= 2 and L.margin(info, t) >= 0.02:
            return t
    raise AssertionError("no candidate threshold keeps a 2 % margin on the reference loop")


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_clips_with_their_own_videos_in_threshold_mode(tiny, use_graph):
    """Two clips, different videos and prompts: four batch rows, ONE decision per iteration - the max over the four.  The reference
    runs the two clips as one batch for that reason; the pattern differs from what either clip would get alone only through it."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(2, 6)
    th = _pick_threshold(lambda t: _ref(sd, conds, noise, "heun-2", 10, Spec(threshold=t))[1])
    want, info = _ref(sd, conds, noise, "heun-2", 10, Spec(threshold=th))
    _a, _sr, lat = _run(model, dac, conds, noise, "heun-2", 10, Spec(threshold=th), use_graph)
    assert model.ctx.plan["vis_of"] is not None             # laid out per batch row
    rep = model.ctx.plan["step_cache_report"]
    print("two clips, threshold %g graph=%d: %s margin %.3f" % (th, use_graph, info["skipped"], L.margin(info, th)))
    assert rep["skipped"] == info["skipped"]
    assert max(abs(g - w) / w for g, w in zip(rep["rel"][1:], info["rel"][1:])) < 1e-4
    for k in range(2):
        assert rel_err(lat[k:k + 1], want[k:k + 1]) < 1e-4, k


# ----------------------------------------------------------------------------- refusals of the library
def test_set_step_cache_refusals(tiny, dev):
    sd, _dsd, model, dac, conds = tiny
    vis, txt = H.batched(conds[:1])
    ctx = model.ctx
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler"))
    with pytest.raises(rt.FoleyRuntimeError, match="n_skip == n_iter"):
        ctx.set_step_cache(1, skip=[0] * 9)
    with pytest.raises(rt.FoleyRuntimeError, match="n_skip == n_iter"):
        ctx.set_step_cache(1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(rt.FoleyRuntimeError, match="finite and >= 0"):
            ctx.set_step_cache(2, threshold=bad)
    with pytest.raises(rt.FoleyRuntimeError, match="range of iterations"):
        ctx.set_step_cache(2, threshold=0.1, interval=(2, 11))
    with pytest.raises(rt.FoleyRuntimeError, match="mode must be"):
        ctx.set_step_cache(3)
    ctx.set_step_cache(0)                                    # clearing is always allowed after prepare
    with pytest.raises(rt.FoleyRuntimeError, match="no cached loop"):
        ctx.step_cache_report()
    fresh = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        fresh.set_step_cache(2, threshold=0.1)
    # the codes: a call before foley_prepare is a call-order error (FOLEY_ERR_STATE, -4, as foley_set_guidance answers it); bad
    # arguments are FOLEY_ERR_INVALID (-1)
    lib = rt.load_library()
    assert lib.foley_set_step_cache(fresh._h, 2, None, 0, 0.1, None, 0, None, 0, None) == -4
    assert lib.foley_set_step_cache(ctx._h, 2, None, 0, -0.1, None, 0, None, 0, None) == -1
    assert lib.foley_set_step_cache(ctx._h, 1, (ctypes.c_uint8 * 9)(), 9, 0.0, None, 0, None, 0, None) == -1


def test_interval_cap_and_polynomial_decide_as_the_python_machine(tiny):
    """The library's own policy (csrc/foley_rt.hip StepCachePolicy) with every option at once - polynomial, interval, cap - against
    host/step_cache.StepCachePolicy fed the change the library REPORTED: both work in double precision from the same fp32 values,
    so the patterns are equal with no margin.  The options bind: no skip outside the interval, no run longer than the cap, and
    the run without them skips elsewhere."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1)
    spec = Spec(threshold=1.0, poly=(8.0, 1.0, 0.0), interval=(0.2, 0.8), max_consecutive=2)     # 8 rel^2 + rel: ~0.2 per iteration
    for use_graph in (False, True):
        _run(model, dac, conds[:1], noise, "euler", 20, spec, use_graph)
        rep = model.ctx.plan["step_cache_report"]
        assert rep["skipped"] == S.StepCachePolicy.from_spec(spec, 20).pattern(rep["rel"]), rep
        sk = rep["skipped"]
        assert sum(sk) >= 4 and not any(sk[:4]) and not any(sk[16:]) and max(_run_lengths(sk)) == 2, sk
    _run(model, dac, conds[:1], noise, "euler", 20, Spec(threshold=1.0, poly=(8.0, 1.0, 0.0)), True)
    free = model.ctx.plan["step_cache_report"]
    assert free["skipped"] == S.StepCachePolicy.from_spec(Spec(threshold=1.0, poly=(8.0, 1.0, 0.0)), 20).pattern(free["rel"])
    assert max(_run_lengths(free["skipped"])) > 2 and any(free["skipped"][:4])


# ----------------------------------------------------------------------------- full width
def test_alternate_schedule_at_full_width(dev):
    """xxl width (D = 1536: the probe's six float4 per lane), depth 1 + 1, 1 s, 6 euler steps, alternate schedule.  fp32 against the
    restated loop under the 1e-4 gate.  bf16: a skip adds no 16-bit rounding of its own (the stream and delta stay fp32), so the
    cached bf16 run lies no further from ITS fp32 reference than twice what the plain bf16 run lies from the plain fp32 reference
    (existing behaviour, measured in this test; the factor allows for the different trajectory)."""
    c11 = C.DiTConfig(name="xxl-1-1", depth_triple=1, depth_single=1)
    sd = synth.synth_dit_state_dict(c11)
    cond = synth.synth_conditioning(c11, 1.0, t2a=False, sd=sd)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(31)).to(torch.bfloat16).float()
    a = (sd, c11.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"], 6, 4.5, "euler")
    with torch.inference_mode():
        want, _, info = L.restated_loop(*a, cache=alternate(6))
        plain = L.restated_loop(*a).x
    assert info["skipped"] == [0, 1, 0, 1, 0, 0] and rel_err(want, plain) > 1e-3
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    err = {}
    for dtype in (torch.float32, torch.bfloat16):
        m = sampler.FoleyModel(c11, sd, dtype, dev)         # latents only: no decoder is attached and none is run
        for name, spec, ref in (("plain", None, plain), ("cached", alternate(6), want)):
            plan = sampler.build_plan(m, vis, txt, 50, 4.5, 6, 1, "euler", step_cache=spec)
            m.ctx.prepare(plan)
            sampler.apply_step_cache(m.ctx, plan)
            lat = noise.to(dev).contiguous()
            m.ctx.sample(lat, use_graph=True)
            if spec is not None:
                assert m.ctx.step_cache_report()[1] == info["skipped"]
            err[(dtype, name)] = rel_err(lat, ref)
    print("xxl-1-1, 1 s, 6 euler steps: " + ", ".join("%s %s %.2e" % (str(k[0])[6:], k[1], v) for k, v in err.items()))
    record_parity("step_cache_xxl_1_1", fp32_plain=err[(torch.float32, "plain")], fp32_cached=err[(torch.float32, "cached")],
                  bf16_plain=err[(torch.bfloat16, "plain")], bf16_cached=err[(torch.bfloat16, "cached")])
    assert err[(torch.float32, "cached")] < 1e-4 and err[(torch.float32, "plain")] < 1e-4
    assert err[(torch.bfloat16, "cached")] <= 2 * err[(torch.bfloat16, "plain")]
