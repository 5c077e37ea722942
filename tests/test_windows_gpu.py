"""Long clips as overlapping windows on the HIP engine: the windows step and the stitch against torch and against the plain step,
the coupled loop against the restated loop (tests/loop_ref.py), the exactness properties (disjoint windows = the
uncoupled batch, one window = the plain call, bit for bit), the keying of the captured graph, the refusals of the ABI, the decode."""
import pytest
import torch

import loop_harness as H
from conftest import rel_err
from foley_amd.host import audio_edit, config as C, long_form, runtime as rt, sampler, tables
from oracle import foley_oracle as O
from step_harness import ref_step

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- ops
def _ref_blend(xn, plan, weights):
    """Every global frame replaced in all covering windows by sum_k w[k] * xn_k (fp32, window order)."""
    V = xn.shape[0] // plan.n_win
    out = xn.clone()
    for v in range(V):
        g = torch.zeros(xn.shape[1], plan.Ltot, device=xn.device)
        first = torch.ones(plan.Ltot, dtype=torch.bool, device=xn.device)
        for k, s in enumerate(plan.starts):
            term = weights[k] * xn[v * plan.n_win + k]
            g[:, s:s + plan.La] = torch.where(first[s:s + plan.La], term, g[:, s:s + plan.La] + term)
            first[s:s + plan.La] = False
        for k, s in enumerate(plan.starts):
            out[v * plan.n_win + k] = g[:, s:s + plan.La]
    return out


def _run_step_op(dev, solver, steps, rows_dtype, variations, starts, La):
    g = torch.Generator().manual_seed(11)
    plan = long_form.WindowPlan.from_frames(starts, La)
    n_win, Ltot = plan.n_win, plan.Ltot
    clips, Cc, ncfg, guid = variations * n_win, 128, 2, 4.5
    coef = tables.edit_solver_table(tables.sigma_grid(steps), solver, steps).to(dev)
    st_t = torch.tensor(starts, dtype=torch.int32, device=dev)
    w_t = plan.weights.to(dev)
    cov = plan.coverage().to(dev)
    x = torch.randn(clips, Cc, La, generator=g).to(dev)
    x_saved, d_acc = torch.zeros_like(x), torch.zeros_like(x)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    step_p = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = torch.empty(ncfg * clips * La, Cc, dtype=rows_dtype, device=dev)
    rows_p = torch.empty_like(rows)
    for it in range(steps):
        pred = torch.randn(ncfg * clips * La, Cc, generator=g).to(dev)
        xn, xs, da = ref_step(pred, x, x_saved, d_acc, coef[it].cpu(), ncfg, guid)
        blend = bool(int(coef[it, 4]) & tables.STEP_BLEND)
        want_x = _ref_blend(xn, plan, w_t) if blend else xn
        xp, xsp, dap = x.clone(), x_saved.clone(), d_acc.clone()
        step_p.fill_(it)
        rt.op_solver_step(pred, xp, xsp, dap, ncfg, guid, coef, step_p, rows_p)          # the plain step on the same state
        rt.op_solver_step(pred, x, x_saved, d_acc, ncfg, guid, coef, step, rows, windows=(st_t, w_t, Ltot))
        torch.cuda.synchronize()
        assert int(step) == it + 1
        for name, got, want in (("x", x, want_x), ("x_saved", x_saved, xs), ("d_acc", d_acc, da)):
            e = rel_err(got, want)
            assert e < 1e-6, (it, name, e)
        assert torch.equal(x_saved, xsp) and torch.equal(d_acc, dap)
        if not blend or n_win == 1:
            assert torch.equal(x, xp) and torch.equal(rows, rows_p), it               # no blend: the plain step exactly
        else:
            for k, s in enumerate(starts):
                single = cov[s:s + La] == 1
                for v in range(variations):
                    b = v * n_win + k
                    assert torch.equal(x[b][:, single], xp[b][:, single]), (it, b)     # one window: the plain update bit for bit
                    for k2 in range(k + 1, n_win):                                    # every other window that covers a frame
                        lo, hi = max(s, starts[k2]), min(s, starts[k2]) + La
                        if lo < hi:
                            assert torch.equal(x[b][:, lo - s:hi - s], x[v * n_win + k2][:, lo - starts[k2]:hi - starts[k2]]), (it, k, k2)
            assert not torch.equal(x, xp)
        want_rows = x.permute(0, 2, 1).reshape(clips * La, Cc).to(rows_dtype)
        for c in range(ncfg):
            r = rows[c * clips * La:(c + 1) * clips * La]
            if rows_dtype == torch.float32:
                assert torch.equal(r, want_rows), (it, c)
            else:
                assert rel_err(r.float(), want_rows.float()) < 1e-2, (it, c)


@pytest.mark.parametrize("solver,steps", [("euler", 6), ("heun-2", 6), ("midpoint-2", 7), ("kutta-4", 8)])
@pytest.mark.parametrize("rows_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_windows_step_op(dev, solver, steps, rows_dtype):
    """2 variations x 4 windows of 75 frames at 0, 45, 61, 110 (Ltot 185): neither length a multiple of the 32-frame tile, frames
    61..74 in three windows, windows 2 and 3 meeting only through window 2's tail (110 < 61 + 75), CFG 4.5."""
    _run_step_op(dev, solver, steps, rows_dtype, 2, [0, 45, 61, 110], 75)


@pytest.mark.parametrize("solver,steps", [("euler", 6), ("kutta-4", 8)])
@pytest.mark.parametrize("rows_dtype", [torch.float32, torch.bfloat16])
def test_windows_step_op_one_window_is_the_plain_step(dev, solver, steps, rows_dtype):
    _run_step_op(dev, solver, steps, rows_dtype, 3, [0], 75)


def test_windows_stitch_op(dev):
    g = torch.Generator().manual_seed(12)
    starts, La = [0, 45, 61, 110], 75
    plan = long_form.WindowPlan.from_frames(starts, La)
    st_t, w_t = torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
    x = torch.randn(2 * 4, 128, La, generator=g).to(dev)
    got = rt.op_windows_stitch(x, st_t, w_t, plan.Ltot)
    want = torch.zeros(2, 128, plan.Ltot, device=dev)
    for v in range(2):
        for k, s in enumerate(starts):
            want[v, :, s:s + La] += w_t[k] * x[v * 4 + k]
    assert got.shape == want.shape and rel_err(got, want) < 1e-6
    single = (plan.coverage() == 1).to(dev)
    for v in range(2):                                                         # singly covered frames are copies
        for k, s in enumerate(starts):
            m = single[s:s + La]
            assert torch.equal(got[v, :, s:s + La][:, m], x[v * 4 + k][:, m])
    # windows that agree on their overlaps: the stitch equals any window's slice bit for bit
    G = torch.randn(2, 128, plan.Ltot, generator=g).to(dev)
    xa = torch.stack([G[v, :, s:s + La] for v in range(2) for s in starts]).contiguous()
    assert torch.equal(rt.op_windows_stitch(xa, st_t, w_t, plan.Ltot), G)
    with pytest.raises(rt.FoleyRuntimeError):
        rt.op_windows_stitch(x[:7].contiguous(), st_t, w_t, plan.Ltot)


# ----------------------------------------------------------------------------- loop
@pytest.fixture(scope="module")
def tiny(dev):
    return H.tiny_run(dev, 3)


def _run(model, dac, conds, noise, solver, plan, use_graph=False, edit=None):
    return H.run(model, dac, conds, noise, solver, 10, 4.5, use_graph, windows=plan, edit=edit)


PLAN = dict(starts=[0, 30, 45], La=50)             # Ltot 95, frames 45..49 in all three windows


@pytest.mark.parametrize("solver", ["euler", "heun-2"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_windowed_loop_matches_oracle(tiny, solver, use_graph):
    sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames(**PLAN)
    noise = H.noise(1, 5, plan.Ltot)
    want = H.ref_loop(sd, conds, noise, 10, 4.5, solver, windows=plan).x
    audio, _sr, lat = _run(model, dac, conds, noise, solver, plan, use_graph)
    assert lat.shape == (1, 128, 95) and audio.shape == (1, 1, 95 * C.DAC_TINY.hop)
    e = rel_err(lat, want)
    print("%s graph=%d: %.2e" % (solver, use_graph, e))
    assert e < 1e-4, (solver, use_graph, e)


def test_windows_agree_on_overlaps_after_euler(tiny, dev):
    """The library's own final window states (foley_sample's output before the stitch): bit-equal on every overlap."""
    _sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames(**PLAN)
    noise = torch.randn(1, 128, plan.Ltot, generator=torch.Generator().manual_seed(5)).to(dev)
    vis, txt = H.batched(conds)
    model.ctx.prepare(sampler.build_plan(model, vis, txt, 50, 4.5, 10, 3, "euler", edit_i0=0))
    model.ctx.set_windows(plan.starts, plan.weights.to(dev))
    x = torch.stack([noise[0, :, s:s + 50] for s in plan.starts]).contiguous()
    model.ctx.sample(x, use_graph=False)
    assert torch.equal(x[0, :, 30:], x[1, :, :20]) and torch.equal(x[1, :, 15:], x[2, :, :35]) and torch.equal(x[0, :, 45:], x[2, :, :5])
    assert not torch.equal(x[0, :, :20], x[1, :, :20])


def test_disjoint_windows_are_the_uncoupled_batch(tiny):
    """Abutting windows (0, 50, 100): every weight is 1.0 - latents and a per-window decode equal the per-clip batch bit for bit."""
    _sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames([0, 50, 100], 50)
    noise = torch.randn(1, 128, 150, generator=torch.Generator().manual_seed(6))
    for solver in ("euler", "heun-2"):
        _a, _sr, lat = _run(model, dac, conds, noise, solver, plan)
        per_clip = torch.stack([noise[0, :, s:s + 50] for s in plan.starts])
        a_ref, _sr, l_ref = _run(model, dac, conds, per_clip, solver, None)
        got = torch.stack([lat[0, :, s:s + 50] for s in plan.starts]).contiguous()
        assert torch.equal(got, l_ref), solver
        assert torch.equal(model.ctx.dac_decode(got), a_ref), solver


def test_one_window_is_the_plain_call(tiny):
    _sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames([0], 50)
    for use_graph in (False, True):
        gen = lambda: torch.Generator("cpu").manual_seed(99)
        vis, txt = H.batched(conds[:1])
        a0, _, l0 = sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, 4.5, 10, 2, "euler", generator=gen(),
                                                           use_graph=use_graph, return_latents=True)
        a1, _, l1 = sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, 4.5, 10, 2, "euler", generator=gen(),
                                                           use_graph=use_graph, return_latents=True, windows=plan)
        assert torch.equal(l0, l1) and torch.equal(a0, a1)


def test_two_variations(tiny):
    """Two variations share the windows' conditioning (n_win rows) and differ in their noise: two different long clips, each equal
    to its single-variation run (the GEMM tile choice moves with the row count, so to fp32 accuracy, not bitwise).  The noise of a
    windowed run is one draw of [variations, C, Ltot] from the generator, like a plain run's."""
    _sd, _dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames(**PLAN)
    vis, txt = H.batched(conds)
    _a, _sr, both = sampler.denoise_process_with_generator(vis, txt, 1.9, model, dac, 4.5, 10, 2, "euler", return_latents=True,
                                                           generator=torch.Generator("cpu").manual_seed(7), windows=plan)
    noise = sampler.draw_noise(2, 128, plan.Ltot, torch.float32, torch.Generator("cpu").manual_seed(7))
    assert both.shape == (2, 128, 95) and rel_err(both[0], both[1]) > 1e-2
    for v in range(2):
        _a, _sr, one = _run(model, dac, conds, noise[v:v + 1], "euler", plan)
        assert rel_err(both[v:v + 1], one) < 1e-6, v


def test_graph_keyed_on_the_windows_state(tiny):
    """One context, use_graph=True: plain, windowed, windowed with other starts, plain, edit, windowed - all of 3 clips x 50 frames,
    so a graph that was not keyed on the windows state would be replayed across them.  Every run equals its eager run."""
    _sd, _dsd, model, dac, conds = tiny
    g = torch.Generator().manual_seed(8)
    p1, p2 = long_form.WindowPlan.from_frames(**PLAN), long_form.WindowPlan.from_frames([0, 20, 60], 50)
    n3 = torch.randn(3, 128, 50, generator=g)
    n1, n2 = torch.randn(1, 128, p1.Ltot, generator=g), torch.randn(1, 128, p2.Ltot, generator=g)
    ed = audio_edit.EditSpec(0.7 * torch.randn(1, 128, 50, generator=g), 1.0, audio_edit.build_mask(50, [(0.2, 0.5)], 0.1))
    seq = [("plain", n3, None, None), ("win1", n1, p1, None), ("win2", n2, p2, None), ("plain", n3, None, None),
           ("edit", n3, None, ed), ("win1", n1, p1, None)]
    want = {}
    for name, noise, plan, edit in seq:
        if name not in want:
            want[name] = _run(model, dac, conds, noise, "euler", plan, False, edit=edit)[2].clone()
    assert rel_err(want["plain"], want["edit"]) > 1e-3
    for name, noise, plan, edit in seq:
        got = _run(model, dac, conds, noise, "euler", plan, True, edit=edit)[2]
        assert rel_err(got, want[name]) < 1e-6, name


def test_set_windows_refusals(tiny, dev):
    sd, _dsd, model, dac, conds = tiny
    vis, txt = H.batched(conds)
    w3, w2 = torch.ones(3, 50, device=dev), torch.ones(2, 50, device=dev)
    fresh = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        fresh.ctx.set_windows([0, 30, 45], w3)
    del fresh
    model.ctx.prepare(sampler.build_plan(model, vis, txt, 50, 4.5, 10, 3, "euler", edit_i0=0))
    with pytest.raises(rt.FoleyRuntimeError, match="multiple of n_win"):
        model.ctx.set_windows([0, 30], w2)
    with pytest.raises(rt.FoleyRuntimeError, match="gap"):
        model.ctx.set_windows([0, 30, 81], w3)
    with pytest.raises(rt.FoleyRuntimeError, match="ascend"):
        model.ctx.set_windows([0, 30, 30], w3)
    with pytest.raises(rt.FoleyRuntimeError, match=r"starts\[0\]"):
        model.ctx.set_windows([-5, 30, 45], w3)
    z = torch.zeros(3, 128, 50, device=dev)
    model.ctx.set_windows([0, 30, 45], w3)
    with pytest.raises(rt.FoleyRuntimeError, match="windows"):                   # windows, then an edit
        model.ctx.set_edit(z, z)
    model.ctx.set_windows(None, None)                                            # clears
    model.ctx.set_edit(z, z)
    with pytest.raises(rt.FoleyRuntimeError, match="edit run"):                  # an edit, then windows
        model.ctx.set_windows([0, 30, 45], w3)
    model.ctx.set_edit(None, None)
    model.ctx.set_windows([0, 30, 45], w3)
    with pytest.raises(ValueError, match="edit"):
        _run(model, dac, conds, torch.zeros(1, 128, 95), "euler", long_form.WindowPlan.from_frames(**PLAN),
             edit=audio_edit.EditSpec(torch.zeros(1, 128, 50), 1.0, None))


def test_stitched_latent_decodes_like_the_oracle_dac(tiny):
    sd, dsd, model, dac, conds = tiny
    plan = long_form.WindowPlan.from_frames(**PLAN)
    noise = torch.randn(1, 128, plan.Ltot, generator=torch.Generator().manual_seed(5))
    audio, sr, lat = _run(model, dac, conds, noise, "euler", plan)
    with torch.inference_mode():
        ref = O.dac_decode(dsd, lat.cpu(), C.DAC_TINY.rates)
    assert sr == C.DAC_TINY.sample_rate and audio.shape == ref.shape
    assert rel_err(audio, ref) < 2e-5
