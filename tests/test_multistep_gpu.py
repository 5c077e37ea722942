"""Multistep solvers on the HIP engine, end to end (tiny config, fp32, 10 steps): orders 2 and 3, eager and graph, against the
restated loop of tests/loop_ref.py; combined with an edit, windows, CFG rescale and the step cache, each against that loop under
the same options; the keying of the captured graph on the ring; the unset state bit for bit; the refusals of foley_set_multistep."""
import pytest
import torch

import loop_harness as H
from abi_pin import assert_abi_version
from conftest import record_parity, rel_err
from foley_amd.host import audio_edit, config as C, long_form, runtime as rt, sampler, tables

pytestmark = pytest.mark.gpu

MS = sampler.MultistepSpec
STEPS, G_SCALE = 10, 4.5


@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 2)


def _run(model, dac, conds, noise, order, use_graph=False, **kw):
    if order is not None:
        kw["multistep"] = MS(order)
    return H.run(model, dac, conds, noise, "euler", STEPS, G_SCALE, use_graph, **kw)[2].clone()


def _loop(sd, conds, noise, **kw):
    return H.ref_loop(sd, conds, noise, STEPS, G_SCALE, shift=C.TINY.flow_shift, **kw)


# ----------------------------------------------------------------------------- against the restated loop
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("order", [2, 3])
def test_matches_the_restated_loop(tiny, order, use_graph):
    """The gate is the project's own for a HIP loop against a restated CPU loop (test_guidance_gpu.py): 1e-4."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    want = _loop(sd, conds[:1], noise, order=order).x
    got = _run(model, dac, conds[:1], noise, order, use_graph)
    assert model.ctx.plan["multistep_order"] == order
    e = rel_err(got, want)
    print("order %d graph=%d: %.2e" % (order, use_graph, e))
    record_parity("multistep.loop.order%d.%s" % (order, "graph" if use_graph else "eager"), rel_err=e)
    assert e < 1e-4, (order, use_graph, e)
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    euler = _loop(sd, conds[:1], noise, weights=[(one, zero, zero)] * STEPS).x
    assert rel_err(want, euler) > 1e-2                        # the control is far above the gate


@pytest.mark.parametrize("order", [2, 3])
def test_differs_from_euler_and_graph_equals_eager(tiny, order):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(2, 6)
    plain = _run(model, dac, conds[:1], noise, None)
    eager = _run(model, dac, conds[:1], noise, order)
    graph = _run(model, dac, conds[:1], noise, order, True)
    assert rel_err(eager, plain) > 1e-2 and rel_err(graph, eager) < 1e-6


# ----------------------------------------------------------------------------- combined runs
@pytest.mark.parametrize("order,spans", [pytest.param(2, None, id="2"), pytest.param(3, None, id="3"),
                                         pytest.param(3, [(0.3, 0.6)], id="3-fractional mask")])
def test_edit_restarts_the_warm_up_at_its_first_iteration(tiny, order, spans):
    """Strength 0.5: the suffix [5, 10) from the source noised to sigma_5, all frames regenerated or a span with 0.1 s ramps -
    against the restated loop under the same edit, whose first row is Euler's."""
    sd, _dsd, model, dac, conds = tiny
    g = torch.Generator().manual_seed(8)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    mask = audio_edit.build_mask(50, spans, 0.1) if spans else None
    edit = audio_edit.EditSpec(x0, 0.5, mask)
    eager = _run(model, dac, conds[:1], noise, order, edit=edit)
    coef = model.ctx.plan["solver_coef"].cpu()
    assert coef.shape[0] == 5 and coef[0, 0] == 1.0 and coef[0, 6] == 0.0 and int(coef[1, 4]) == tables.STEP_BLEND | tables.STEP_HIST
    graph = _run(model, dac, conds[:1], noise, order, True, edit=edit)
    want = _loop(sd, conds[:1], noise, order=order, edit=(x0, mask, 0.5)).x
    e = rel_err(eager, want)
    print("edit order %d%s: %.2e" % (order, ", fractional mask" if spans else "", e))
    assert e < 1e-4 and rel_err(graph, eager) < 1e-6
    assert rel_err(eager, _run(model, dac, conds[:1], noise, None, edit=edit)) > 1e-3


def test_windowed_run(tiny):
    sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    wn = H.noise(1, 9, plan.Ltot)
    three = [conds[0], conds[1], conds[0]]
    eager = _run(model, dac, three, wn, 3, windows=plan)
    graph = _run(model, dac, three, wn, 3, True, windows=plan)
    base = _run(model, dac, three, wn, None, windows=plan)
    assert eager.shape == (1, 128, 95) and rel_err(graph, eager) < 1e-6 and rel_err(eager, base) > 1e-2
    e = rel_err(eager, _loop(sd, three, wn, order=3, windows=plan).x)
    print("order 3 with windows: %.2e" % e)
    record_parity("loop.multistep3.windows", rel_err=e)
    assert e < 1e-4, e


def test_with_cfg_rescale(tiny):
    """The history holds the velocity as the step used it, the rescale factor included: against the restated loop with it."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    spec = sampler.GuidanceSpec(rescale=0.7)
    want = _loop(sd, conds[:1], noise, order=2, rescale=0.7).x
    eager = _run(model, dac, conds[:1], noise, 2, guidance=spec)
    graph = _run(model, dac, conds[:1], noise, 2, True, guidance=spec)
    e = rel_err(eager, want)
    print("order 2 with rescale 0.7: %.2e" % e)
    assert e < 1e-4 and rel_err(graph, eager) < 1e-6
    assert rel_err(want, _loop(sd, conds[:1], noise, order=2).x) > 1e-3


def test_with_a_step_cache_skip_list(tiny):
    """A skipped iteration runs the unchanged step: it reads and feeds the ring like any other."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise()
    sc = sampler.StepCacheSpec(skip=(3, 6))
    eager = _run(model, dac, conds[:1], noise, 3, step_cache=sc)
    report = model.ctx.plan["step_cache_report"]["skipped"]
    assert report == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    graph = _run(model, dac, conds[:1], noise, 3, True, step_cache=sc)
    assert rel_err(graph, eager) < 1e-6
    full = _run(model, dac, conds[:1], noise, 3)
    assert rel_err(eager, full) > 1e-6                        # the skips did reuse a residual
    assert not bool(torch.isnan(eager).any())
    want = _loop(sd, conds[:1], noise, order=3, cache=sc)
    e = rel_err(eager, want.x)
    print("order 3 with a skip list: %.2e" % e)
    record_parity("loop.multistep3.skip_list", rel_err=e)
    assert want.info["skipped"] == report and e < 1e-4, e


# ----------------------------------------------------------------------------- graph keying, the unset state
def test_graph_keyed_on_the_ring(tiny):
    """plain, order 2, order 2 again, order 3, plain on one context under use_graph: the second order-2 run captures nothing new,
    orders 2 and 3 have rings of different slot counts, and the last plain run carries the bits of the first."""
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(1, 11)
    want = {o: _run(model, dac, conds[:1], noise, o) for o in (None, 2, 3)}
    first = _run(model, dac, conds[:1], noise, None, True)
    c0 = H.captures(model)
    a = _run(model, dac, conds[:1], noise, 2, True)
    c1 = H.captures(model)
    b = _run(model, dac, conds[:1], noise, 2, True)
    c2 = H.captures(model)
    c = _run(model, dac, conds[:1], noise, 3, True)
    c3 = H.captures(model)
    last = _run(model, dac, conds[:1], noise, None, True)
    assert c1 == c0 + 1 and c2 == c1 and c3 == c2 + 1
    assert torch.equal(a, b) and rel_err(a, want[2]) < 1e-6 and rel_err(c, want[3]) < 1e-6 and rel_err(a, c) > 1e-4
    assert torch.equal(last, first) and rel_err(first, want[None]) < 1e-6


@pytest.mark.parametrize("use_graph", [False, True])
def test_unset_is_the_plain_run(tiny, use_graph):
    sd, _dsd, model, dac, conds = tiny
    noise = H.noise(2, 7)
    call = lambda **kw: H.run(model, dac, conds[:1], noise, "euler", STEPS, G_SCALE, use_graph, **kw)
    a0, _, l0 = call()
    _run(model, dac, conds[:1], noise, 2, use_graph)          # a multistep run in between leaves nothing behind
    a1, _, l1 = call(multistep=None)
    assert "multistep_order" not in model.ctx.plan
    assert torch.equal(l0, l1) and torch.equal(a0, a1)


def test_set_multistep_refusals(tiny, dev):
    sd, _dsd, model, dac, conds = tiny
    vis, txt = H.batched(conds[:1])
    ctx = model.ctx
    ctx.prepare(sampler.build_plan(model, vis, txt, 50, G_SCALE, STEPS, 1, "euler"))
    lib = rt.load_library()
    for bad in (-1, 4, 5):
        assert lib.foley_set_multistep(ctx._h, bad, None) == -1                               # FOLEY_ERR_INVALID
        with pytest.raises(rt.FoleyRuntimeError, match="order must be"):
            ctx.set_multistep(bad)
    for ok in (2, 3, 1, 0):
        ctx.set_multistep(ok)
    fresh = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    assert lib.foley_set_multistep(fresh._h, 2, None) == -4                                   # FOLEY_ERR_STATE
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        fresh.set_multistep(2)
    assert_abi_version()
