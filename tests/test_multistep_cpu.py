"""Multistep solvers without a GPU: the Adams-Bashforth tables of host/tables.py (exactness on polynomials, warm-up, the edit
suffix), the order of the table-driven loop on an analytic problem (tests/multistep_ref.py), the restated model loop (tests/loop_ref.py) against the
oracle's Euler loop, the refusals, the ABI surface and the keyword plumbing of the sampler entry points and the node."""
import contextlib
import ctypes
import os
import re
import types

import pytest
import torch

from abi_pin import assert_abi_version
import loop_ref as L
import multistep_ref as M
from foley_amd import nodes
from foley_amd.host import config as C, long_form, runtime as rt, sampler, synth, tables
from oracle import foley_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(steps, shift) for steps in (7, 10, 50) for shift in (1.0, 3.0)]


# ----------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("steps,shift", GRIDS)
def test_weights_integrate_polynomials_exactly(steps, shift, order):
    """Every row with full history integrates sigma^m, m = 0 .. order - 1, exactly: sum_j c_j sigma_{n-j}^m equals
    (sigma_{n+1}^{m+1} - sigma_n^{m+1}) / ((m + 1) dt) within 2^-23 sum|c_j| - one fp32 rounding per weight (2^-24 relative,
    sigma <= 1), doubled."""
    sig = tables.sigma_grid(steps, shift)
    t = tables.solver_table(sig, "euler", steps, multistep_order=order)
    s = sig.double()
    worst = 0.0
    for n in range(order - 1, steps):
        c = [float(t[n, 0].double()), float(t[n, 6].double()), float(t[n, 7].double())][:order]
        assert int(t[n, 4]) == tables.STEP_HIST and (order == 3 or float(t[n, 7]) == 0.0)
        dt = float(s[n + 1] - s[n])
        mag = sum(abs(v) for v in c)
        for m in range(order):
            lhs = sum(c[j] * float(s[n - j]) ** m for j in range(order))
            rhs = (float(s[n + 1]) ** (m + 1) - float(s[n]) ** (m + 1)) / ((m + 1) * dt)
            worst = max(worst, abs(lhs - rhs) / (2.0 ** -24 * mag))
            assert abs(lhs - rhs) <= 2.0 ** -23 * mag, (steps, shift, order, n, m, lhs, rhs)
    print("steps %d shift %g order %d: worst %.2f of 2^-24 sum|c|" % (steps, shift, order, worst))


@pytest.mark.parametrize("steps,shift", GRIDS)
def test_warm_up_rows_and_untouched_columns(steps, shift):
    sig = tables.sigma_grid(steps, shift)
    plain = tables.solver_table(sig, "euler", steps)
    t2, t3 = (tables.solver_table(sig, "euler", steps, multistep_order=k) for k in (2, 3))
    for t in (t2, t3):
        assert t[0].tolist() == plain[0].tolist() and t[0, 0] == 1.0 and t[0, 4] == 0.0          # Euler, no flag
        assert torch.equal(t[:, 1:4], plain[:, 1:4]) and torch.equal(t[:, 5], plain[:, 5])       # dt and the rest as they were
        assert bool((t[1:, 4] == tables.STEP_HIST).all())
    assert torch.equal(t3[1], t2[1]) and torch.equal(t3[:2, 7], torch.zeros(2))                  # order 3 warms up through order 2
    assert bool((t2[:, 7] == 0).all()) and bool((t3[2:, 7] != 0).all())
    r = (sig[2].double() - sig[1].double()) / (sig[1].double() - sig[0].double())                # the closed form of order 2
    assert float(t2[1, 0]) == float((1 + r / 2).float()) and float(t2[1, 6]) == float((-r / 2).float())
    # without the option the table is the one-step table, value for value
    assert torch.equal(tables.solver_table(sig, "euler", steps, multistep_order=None), plain) and bool((plain[:, 5:] == 0).all())
    assert torch.equal(tables.build_tables(50, 8, 24, 77, steps, "euler", shift)["solver_coef"], plain)


def test_uniform_grid_gives_the_textbook_weights():
    sig = tables.sigma_grid(50)
    t2, t3 = (tables.solver_table(sig, "euler", 50, multistep_order=k) for k in (2, 3))
    assert torch.allclose(t2[1:, [0, 6]], torch.tensor([1.5, -0.5]).expand(49, 2), atol=1e-5, rtol=0)
    assert torch.allclose(t3[2:, [0, 6, 7]], torch.tensor([23.0, -16.0, 5.0]).expand(48, 3) / 12, atol=1e-5, rtol=0)


@pytest.mark.parametrize("order", [2, 3])
def test_start_restarts_the_warm_up(order):
    sig = tables.sigma_grid(10, 3.0)
    full = tables.solver_table(sig, "euler", 10, multistep_order=order)
    i0 = 4
    t = tables.solver_table(sig, "euler", 10, multistep_order=order, start=i0)
    assert t[i0, 0] == 1.0 and t[i0, 4] == 0.0 and t[i0, 6] == 0.0 and t[i0, 7] == 0.0
    t2 = tables.solver_table(sig, "euler", 10, multistep_order=2)
    assert torch.equal(t[i0 + 1], t2[i0 + 1])
    keep = [i for i in range(10) if not i0 <= i < i0 + order - 1]
    assert torch.equal(t[keep], full[keep]) and torch.equal(t[:, [2, 5]], full[:, [2, 5]])
    e = tables.edit_solver_table(sig, "euler", 10, i0, multistep_order=order)
    assert e.shape[0] == 6 and torch.equal(e[:, [0, 6, 7]], t[i0:, [0, 6, 7]])
    assert e[0, 4] == tables.STEP_BLEND and bool((e[1:, 4] == tables.STEP_BLEND + tables.STEP_HIST).all())
    assert torch.equal(e[:, 5], sig[i0 + 1:])
    b = tables.build_tables(50, 8, 24, 77, 10, "euler", 3.0, edit_i0=i0, multistep_order=order, start=i0)
    assert torch.equal(b["solver_coef"], e)


def test_table_refusals():
    sig = tables.sigma_grid(12)
    for solver in ("heun-2", "midpoint-2", "kutta-4"):
        with pytest.raises(ValueError, match="euler"):
            tables.solver_table(sig, solver, 12, multistep_order=2)
    for bad in (0, 1, 4, 2.5, True):
        with pytest.raises(ValueError, match="multistep_order"):
            tables.solver_table(sig, "euler", 12, multistep_order=bad)


# ----------------------------------------------------------------------------- the order, on an analytic problem
@pytest.fixture(scope="module")
def truth():
    return M.rk4_reference()


def _err(n, shift, order, truth):
    sig = tables.sigma_grid(n, shift)
    return abs(M.table_loop64(sig, tables.solver_table(sig, "euler", n, multistep_order=order)) - truth)


@pytest.mark.parametrize("shift,ns", [(1.0, (20, 40, 80)), (3.0, (40, 80, 160))])
def test_order_2_halves_the_step_and_quarters_the_error(truth, shift, ns):
    e = [_err(n, shift, 2, truth) for n in ns]
    ratios = [e[i] / e[i + 1] for i in range(2)]
    print("shift %g: errors %s ratios %s" % (shift, ["%.3e" % v for v in e], ["%.2f" % v for v in ratios]))
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios


def test_order_3_beats_order_2_at_every_step_count(truth):
    """No ratio is asserted: the Euler first step holds order 3 at global order 2, with a smaller constant."""
    for n in (10, 20, 40, 80, 160):
        e2, e3 = _err(n, 1.0, 2, truth), _err(n, 1.0, 3, truth)
        print("N %d: order 2 %.3e order 3 %.3e (%.2f x)" % (n, e2, e3, e2 / e3))
        assert e3 < e2, (n, e2, e3)
    sig = tables.sigma_grid(40)
    assert abs(M.table_loop64(sig, tables.solver_table(sig, "euler", 40)) - truth) > 5 * _err(40, 1.0, 2, truth)   # Euler is far behind


# ----------------------------------------------------------------------------- the restated model loop
def test_restated_loop_is_the_oracle_without_history_and_moves_with_it():
    cfg = C.TINY
    sd = synth.synth_dit_state_dict(cfg)
    c = synth.synth_conditioning(cfg, 1.0, t2a=False, sd=sd, seed=10)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
    args = (sd, cfg.heads, noise, c["text"], c["uncond_text"], c["clip"], c["sync"], 10, 4.5)
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    with torch.inference_mode():
        want = O.sample_latents(*args, "euler")
        assert torch.equal(L.restated_loop(*args, weights=[(one, zero, zero)] * 10).x, want)
        for order in (2, 3):
            got = L.restated_loop(*args, order=order).x
            rel = float((got - want).norm() / want.norm())
            print("order %d against euler: %.3e" % (order, rel))
            assert rel > 1e-2, (order, rel)


# ----------------------------------------------------------------------------- refusals, ABI surface
def test_spec_refusals():
    for bad in (1, 4, 2.5, 0, None, "2", True):
        with pytest.raises(ValueError, match="order"):
            sampler.MultistepSpec(bad).check("euler")
    for solver in ("heun-2", "midpoint-2", "kutta-4"):
        with pytest.raises(ValueError, match="euler"):
            sampler.MultistepSpec(2).check(solver)
    sampler.MultistepSpec(2).check("euler")
    sampler.MultistepSpec(3).check("euler")


def test_abi_declares_the_multistep_entries():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    lib = rt.load_library()
    for name in ("foley_set_multistep", "foley_op_solver_step"):
        assert name in rt.EXPORTED_SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr)
        assert getattr(lib, name) is not None
    assert_abi_version()
    assert "#define FOLEY_STEP_HIST 16" in hdr and tables.STEP_HIST == 16
    assert callable(rt.op_solver_step) and callable(rt.FoleyContext.set_multistep)
    rc = lib.foley_set_multistep(None, 2, None)
    assert rc != 0 and lib.foley_last_error()
    assert lib.foley_op_solver_step(None, None) != 0 and b"descriptor" in lib.foley_last_error()
    assert lib.foley_op_solver_step(ctypes.byref(rt.StepDescC(hist_slots=1)), None) != 0          # slots without a ring: refused before any launch
    assert b"ring" in lib.foley_last_error()
    assert "typedef struct foley_step_desc" in hdr
    size = int(re.search(r"static_assert\(sizeof\(foley_step_desc\) == (\d+),", hdr).group(1))
    assert ctypes.sizeof(rt.StepDescC) == size == 168       # the header's struct on LP64: pointers 8-aligned, int32 fields paired
    src = open(os.path.join(ROOT, "comfyui-hunyuanvideo-foley_amd", "csrc", "rowops.hip")).read()
    assert "solver_step_hist_kernel" in src and "getenv" not in src
    assert "oracle" not in open(os.path.join(ROOT, "comfyui-hunyuanvideo-foley_amd", "host", "sampler.py")).read()


def test_earlier_step_names_forward_to_the_one_wrapper(monkeypatch):
    seen = []
    monkeypatch.setattr(rt, "op_solver_step", lambda *a, **kw: seen.append((a, {k: v for k, v in kw.items() if v is not None})))
    core = tuple("pred x x_saved d_acc ncfg guidance coef step_ptr rows_out".split())
    rt.op_solver_step_edit(*core, "x0", "noise")
    rt.op_solver_step_edit(*core, "x0", "noise", "mask")
    rt.op_solver_step_windows(*core, "starts", "weights", 7)
    rt.op_solver_step_guided("gd", *core, edit=("x0", "noise", None))
    rt.op_solver_step_hist("ring", *core, gd="gd", windows=("starts", "weights", 7), slots=2)
    assert seen == [(core, dict(edit=("x0", "noise", None))), (core, dict(edit=("x0", "noise", "mask"))),
                    (core, dict(windows=("starts", "weights", 7))), (core, dict(gd="gd", edit=("x0", "noise", None))),
                    (core, dict(gd="gd", hist="ring", slots=2, windows=("starts", "weights", 7)))]


# ----------------------------------------------------------------------------- plumbing: the sampler entry points
def test_spec_reaches_windows_and_shards_and_the_plan(monkeypatch):
    spec = sampler.MultistepSpec(3)
    seen = {}

    def fake_windows(*a, **k):
        seen["windows"] = (a, k)
        return "w"
    monkeypatch.setattr(sampler, "_denoise_windows", fake_windows)
    plan = long_form.WindowPlan.from_frames([0, 30], 50)
    model = types.SimpleNamespace(cfg=C.TINY)
    assert sampler.denoise_process_with_generator({}, {}, 1.0, model, None, 4.5, 10, 1, "euler", windows=plan, multistep=spec) == "w"
    assert seen["windows"][1] == {"multistep": spec}
    sampler.denoise_process_with_generator({}, {}, 1.0, model, None, 4.5, 10, 1, "euler", windows=plan)
    assert seen["windows"][1] == {}                          # unset: the call as it was
    with pytest.raises(ValueError, match="euler"):           # refused before anything runs
        sampler.denoise_process_with_generator({}, {}, 1.0, model, None, 4.5, 10, 1, "heun-2", multistep=spec)

    class _Stream:
        def __init__(self, *_a, **_k): pass
        def wait_event(self, _ev): pass
        def synchronize(self): pass
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "device", lambda _d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda _s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *_a: _Stream())
    cfg = types.SimpleNamespace(frame_rate=50, text_len=128, latent_dim=128)
    reps = [(types.SimpleNamespace(cfg=cfg, dtype=torch.float32, device=torch.device("cpu"), _text_len_fixed=None, rank=r), None)
            for r in range(2)]
    got = {}

    def fake(visual, text, secs, model, dac, cfg_scale, steps, bs, solver, **kw):
        got[model.rank] = kw
        return torch.zeros(bs, 1, 8), 48000, torch.zeros(bs, 128, 50)
    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake)
    feats = {"text_feat": torch.zeros(1, 5, 8), "uncond_text_feat": torch.zeros(1, 5, 8)}
    sampler.denoise_process_multi({}, feats, 1.0, reps, 4.5, 10, 4, "euler", generator=torch.Generator().manual_seed(0), multistep=spec)
    assert got[0]["multistep"] is spec and got[1]["multistep"] is spec
    sampler.denoise_process_multi({}, feats, 1.0, reps, 4.5, 10, 4, "euler", generator=torch.Generator().manual_seed(0))
    assert "multistep" not in got[0] and "multistep" not in got[1]
    with pytest.raises(ValueError, match="euler"):
        sampler.denoise_process_multi({}, feats, 1.0, reps, 4.5, 10, 4, "kutta-4", multistep=spec)


def test_build_plan_carries_the_order_and_keys_its_tables():
    cfg = C.TINY
    sd = synth.synth_dit_state_dict(cfg)
    c = synth.synth_conditioning(cfg, 1.0, t2a=False, sd=sd, seed=10)
    model = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), _text_len_fixed=None, dtype=torch.float32, quantization=None,
                                  get_empty_clip_sequence=lambda bs, len: torch.zeros(bs, len, c["clip"].shape[2]),
                                  get_empty_sync_sequence=lambda bs, len: torch.zeros(bs, len, c["sync"].shape[2]))
    vis = {"siglip2_feat": c["clip"], "syncformer_feat": c["sync"]}
    txt = {"text_feat": c["text"], "uncond_text_feat": c["uncond_text"]}
    sig = tables.sigma_grid(10, cfg.flow_shift)
    plain = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler")
    assert "multistep_order" not in plain and torch.equal(plain["solver_coef"], tables.solver_table(sig, "euler", 10))
    p3 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler", multistep=sampler.MultistepSpec(3))
    assert p3["multistep_order"] == 3 and torch.equal(p3["solver_coef"], tables.solver_table(sig, "euler", 10, multistep_order=3))
    p2 = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler", multistep=sampler.MultistepSpec(2), edit_i0=5)
    assert torch.equal(p2["solver_coef"], tables.edit_solver_table(sig, "euler", 10, 5, multistep_order=2)) and p2["n_iter"] == 5
    again = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "euler")
    assert again["solver_coef"] is plain["solver_coef"]       # the plain tables stay cached under their own key
    with pytest.raises(ValueError, match="euler"):
        sampler.build_plan(model, vis, txt, 50, 4.5, 10, 1, "heun-2", multistep=sampler.MultistepSpec(2))
    calls = []
    ctx = types.SimpleNamespace(set_multistep=lambda order: calls.append(order))
    sampler.apply_multistep(ctx, plain)
    sampler.apply_multistep(ctx, p3)
    assert calls == [3]


# ----------------------------------------------------------------------------- plumbing: the node
def _node(monkeypatch, sampler_name="euler", **kw):
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
    model.get_empty_clip_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    model.get_empty_sync_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    dac = types.SimpleNamespace(has_encoder=True, cfg=C.DAC48K, sample_rate=48000)
    seen = {"encoded": [], "calls": []}

    def fake_sample(visual, text, secs, m, d, **k):
        seen["calls"].append(k)
        return torch.zeros(k["batch_size"], 1, int(round(secs * 48000))), 48000

    def fake_encode(prompts, deps, dev, dt=None):
        seen["encoded"].append(list(prompts))
        return torch.zeros(len(prompts), 5, 768)
    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake_sample)
    monkeypatch.setattr(nodes, "encode_text_feat", fake_encode)
    deps = {"dac_model": dac, "siglip2_model": None, "syncformer_model": None}
    out = nodes.HunyuanFoleySampler().generate_audio(model, deps, 16, 5.0, "p", "n", 4.5, 10, sampler_name, 2, 0, True, **kw)
    return out, seen


def test_node_passes_the_order_only_when_set(monkeypatch):
    _out, seen = _node(monkeypatch)
    assert "multistep" not in seen["calls"][0]
    _out, seen = _node(monkeypatch, multistep_order=None)
    assert "multistep" not in seen["calls"][0]
    for order in (2, 3):
        _out, seen = _node(monkeypatch, multistep_order=order)
        assert seen["calls"][0]["multistep"] == sampler.MultistepSpec(order) and seen["calls"][0]["sampler"] == "euler"
    _out, seen = _node(monkeypatch, multistep_order=2, window_s=3, window_overlap_s=1.0)       # the windowed call carries it too
    assert seen["calls"][0]["windows"] is not None and seen["calls"][0]["multistep"] == sampler.MultistepSpec(2)
    it = nodes.HunyuanFoleySampler.INPUT_TYPES()
    assert "multistep_order" not in set(it["required"]) | set(it.get("optional", {}))          # a keyword, not a socket
    with pytest.raises(TypeError):
        nodes.HunyuanFoleySampler().generate_audio(*([None] * 17))


def test_node_refuses_before_the_encoders(monkeypatch):
    for kw, name, word in ((dict(multistep_order=2), "heun-2", "euler"), (dict(multistep_order=3), "kutta-4", "euler"),
                           (dict(multistep_order=1), "euler", "order"), (dict(multistep_order=4), "euler", "order"),
                           (dict(multistep_order=2.5), "euler", "order")):
        calls = []
        monkeypatch.setattr(nodes, "encode_text_feat", lambda *a, **k: calls.append(1))
        model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
        with pytest.raises(ValueError, match=word):
            nodes.HunyuanFoleySampler().generate_audio(model, {"dac_model": None}, 16, 5.0, "p", "n", 4.5, 10, name, 1, 0, True, **kw)
        assert calls == []
