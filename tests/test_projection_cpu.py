"""Projected guidance (APG, CFG-Zero*) without a GPU: the per-iteration rows, every refusal of the spec, the node and the plan, the
fp64 identities of tests/projection_ref.py, and the C surface."""
import os
import re
import types

import pytest
import torch

import projection_ref as P
from abi_pin import assert_abi_version
from conftest import ROOT
from foley_amd import nodes
from foley_amd.host import config as C, runtime as rt, sampler, tables


# ----------------------------------------------------------------------------- tables.projection_rows
def test_projection_rows_first_row_start_and_zero_init():
    r = tables.projection_rows(10, "apg", 0.25, -0.5, 3.0, 2)
    assert r.dtype == torch.float32 and tuple(r.shape) == (10, 4)
    assert r[0].tolist() == [0.25, 0.0, 3.0, 0.0]                           # the first row reads no plane
    assert r[1].tolist() == [0.25, -0.5, 3.0, 0.0] and r[2].tolist() == [0.25, -0.5, 3.0, 1.0]
    assert bool((r[1:, 1] == -0.5).all()) and r[:, 3].tolist() == [0.0, 0.0] + [1.0] * 8
    # an edit run: the rows [i0, steps) of the full run, the first of them without momentum; zero_init counts the full run's iterations
    e = tables.projection_rows(10, "apg", 0.25, -0.5, 3.0, 5, start=4)
    assert tuple(e.shape) == (6, 4) and e[0, 1] == 0.0 and bool((e[1:, 1] == -0.5).all())
    assert e[:, 3].tolist() == [0.0] + [1.0] * 5
    assert torch.equal(tables.projection_rows(10, 1, 0.25, -0.5, 3.0, 2), r)  # the mode as the library's number
    # fp64, rounded once
    assert float(tables.projection_rows(3, "apg", 0.1, 0.3, 0.7, 0)[1, 1]) == float(torch.tensor(0.3, dtype=torch.float64).float())
    z = tables.projection_rows(6, "cfg_zero_star", 0.9, 0.9, 9.0, 1)          # CFG-Zero* reads live alone
    assert bool((z[:, :3] == 0.0).all()) and z[:, 3].tolist() == [0.0] + [1.0] * 5
    assert tables.PROJECTION_MODES == {"apg": 1, "cfg_zero_star": 2}
    for bad in (dict(mode="pag"), dict(mode=3), dict(start=10), dict(start=-1), dict(zero_init=-1)):
        kw = {"mode": "apg", **bad}
        with pytest.raises(ValueError):
            tables.projection_rows(10, kw.pop("mode"), **kw)
    with pytest.raises(ValueError):
        tables.projection_rows(0, "apg")


# ----------------------------------------------------------------------------- refusals
def test_spec_refusals():
    S = sampler.ProjectionSpec
    assert S("apg") == S("apg", 0.0, -0.5, 0.0, 0)
    S("apg", 1.0, 0.99, 0.0, 9).check(10)
    S("cfg_zero_star", zero_init=1).check(10)
    for bad, msg in ((S("pag"), "guidance_mode must be one of"), (S("apg", eta=1.5), r"eta must lie in \[0, 1\]"),
                     (S("apg", eta=-0.1), r"eta must lie in \[0, 1\]"), (S("apg", momentum=1.0), r"\|momentum\| < 1"),
                     (S("apg", momentum=-1.5), r"\|momentum\| < 1"), (S("apg", norm_threshold=-1.0), "norm_threshold must be >= 0"),
                     (S("apg", eta=float("nan")), "finite"), (S("apg", zero_init=10), "smaller than the number of steps"),
                     (S("apg", zero_init=-1), "integer >= 0"), (S("apg", zero_init=1.5), "integer >= 0")):
        with pytest.raises(ValueError, match=msg):
            bad.check(10)
    G = sampler.GuidanceSpec
    G(projection=S("apg")).check(4.5, 10)
    G(interval=(0.2, 0.7), projection=S("cfg_zero_star")).check(4.5, 10)
    with pytest.raises(ValueError, match="video scale"):
        G(g_video=3.0, projection=S("apg")).check(4.5, 10)
    with pytest.raises(ValueError, match="cfg_rescale > 0"):
        G(rescale=0.5, projection=S("apg")).check(4.5, 10)
    with pytest.raises(ValueError, match="cfg_scale > 1"):
        G(projection=S("apg")).check(1.0, 10)
    assert G().projection is None and G(3.0, (0.1, 0.9), 0.5) == G(3.0, (0.1, 0.9), 0.5, None)     # the fields before it keep their places


def test_node_refusals():
    """Before the encoders run: the node is called without a model."""
    node = nodes.HunyuanFoleySampler()
    args = (None, None, 16, 1.0, "p", "n")
    tail = (10, "euler", 1, 0, True)
    for kw, scale, msg in (({"guidance_mode": "apg", "video_cfg_scale": 3.0}, 4.5, "video scale"),
                           ({"guidance_mode": "apg", "cfg_rescale": 0.5}, 4.5, "cfg_rescale > 0"),
                           ({"guidance_mode": "cfg_zero_star"}, 1.0, "cfg_scale > 1"),
                           ({"guidance_mode": "apg", "apg_eta": 1.25}, 4.5, r"eta must lie in \[0, 1\]"),
                           ({"guidance_mode": "apg", "apg_momentum": -1.0}, 4.5, r"\|momentum\| < 1"),
                           ({"guidance_mode": "apg", "zero_init_steps": 10}, 4.5, "smaller than the number of steps"),
                           ({"guidance_mode": "apg", "apg_norm_threshold": -2.0}, 4.5, "norm_threshold must be >= 0"),
                           ({"guidance_mode": "perp"}, 4.5, "guidance_mode must be one of"),
                           ({"apg_eta": 0.5}, 4.5, "pass guidance_mode"), ({"zero_init_steps": 1}, 4.5, "pass guidance_mode")):
        with pytest.raises(ValueError, match=msg):
            node.generate_audio(*args, scale, *tail, **kw)


def test_plan_refusals():
    """build_plan validates before it touches the model or the features."""
    model = types.SimpleNamespace(cfg=C.TINY, device=torch.device("cpu"))
    S, G = sampler.ProjectionSpec, sampler.GuidanceSpec
    for g, scale, msg in ((G(projection=S("apg", zero_init=10)), 4.5, "smaller than the number of steps"),
                          (G(rescale=0.3, projection=S("apg")), 4.5, "cfg_rescale > 0"),
                          (G(g_video=2.0, projection=S("cfg_zero_star")), 4.5, "video scale"),
                          (G(projection=S("apg")), 1.0, "cfg_scale > 1")):
        with pytest.raises(ValueError, match=msg):
            sampler.build_plan(model, {}, {}, 50, scale, 10, 1, "euler", guidance=g)


# ----------------------------------------------------------------------------- the fp64 identities
def _pred(clips, La, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2 * clips * La, C, generator=g) + 0.25


def test_apg_eta_one_is_cfg():
    """eta = 1, beta = 0, R = 0: a_c = 1, a_w = g - 1, w = c - u: v = c + (g - 1)(c - u) = u + g (c - u) in exact arithmetic."""
    clips, La, Cc, g = 3, 33, 100, 4.5
    pred = _pred(clips, La, Cc, 1)
    ref = P.coef_ref(pred, clips, La, g, (1.0, 0.0, 0.0, 1.0), P.APG)
    assert torch.equal(ref["coef"][:, 0], torch.ones(clips, dtype=torch.float64)) and torch.equal(ref["coef"][:, 1], torch.full((clips,), 3.5, dtype=torch.float64))
    v, _ = P.projected_value(pred, clips, La, ref, P.APG)
    u, c = P.halves(pred, clips, La)
    cfg = P.cfg_value64(u, c, g).transpose(1, 2)
    assert float((v - cfg).abs().max()) <= 1e-13 * float(cfg.abs().max())


@pytest.mark.parametrize("mode", [P.APG, P.ZERO_STAR])
def test_scale_one_gives_the_conditional_prediction(mode):
    clips, La, Cc = 2, 50, 128
    pred = _pred(clips, La, Cc, 2)
    prev = torch.randn(clips, La, Cc, generator=torch.Generator().manual_seed(3))
    ref = P.coef_ref(pred, clips, La, 1.0, (0.3, -0.5, 2.0, 1.0), mode, m_prev=prev)
    assert ref["coef"][:, 0].tolist() == [1.0] * clips and ref["coef"][:, 1].tolist() == [0.0] * clips
    v, _ = P.projected_value(pred, clips, La, ref, mode)
    assert torch.equal(v, P.halves(pred, clips, La)[1].transpose(1, 2))
    dead = P.coef_ref(pred, clips, La, 4.5, (0.3, -0.5, 2.0, 0.0), mode, m_prev=prev)     # live = 0: a zero velocity
    assert bool((dead["coef"] == 0).all()) and bool((P.projected_value(pred, clips, La, dead, mode)[0] == 0).all())


def test_zero_star_of_parallel_halves_is_the_conditional_prediction():
    """u = k c: s = <c,u>/<u,u> = 1/k and v = g c + (1 - g) s u = c."""
    clips, La, Cc, g, k = 2, 31, 64, 6.0, 0.5
    c = torch.randn(clips * La, Cc, generator=torch.Generator().manual_seed(4))
    pred = torch.cat([k * c, c])
    ref = P.coef_ref(pred, clips, La, g, (0.0, 0.0, 0.0, 1.0), P.ZERO_STAR)
    assert float((ref["s"] - 1.0 / k).abs().max()) <= 1e-14
    v, _ = P.projected_value(pred, clips, La, ref, P.ZERO_STAR)
    want = c.double().view(clips, La, Cc).transpose(1, 2)
    assert float((v - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_apg_clip_and_momentum_in_the_reference():
    clips, La, Cc = 2, 33, 96
    pred = _pred(clips, La, Cc, 5)
    prev = torch.randn(clips, La, Cc, generator=torch.Generator().manual_seed(6))
    free = P.coef_ref(pred, clips, La, 4.5, (0.0, -0.5, 0.0, 1.0), P.APG, m_prev=prev)
    u, c = P.halves(pred, clips, La)
    assert torch.equal(free["m"], (c - u) - 0.5 * prev.double())
    R = float(free["norm"].min()) / 2
    clipped = P.coef_ref(pred, clips, La, 4.5, (0.0, -0.5, R, 1.0), P.APG, m_prev=prev)
    assert torch.allclose(clipped["r"], R / free["norm"]) and torch.equal(clipped["m"], free["m"])      # the plane keeps the unclipped m
    assert torch.allclose(clipped["coef"][:, 1], 3.5 * R / free["norm"])
    assert P.chain_length(128, 50) == 16 + 6 + 4 + 1 + 64 and P.chain_length(256, 2081) == 32 + 6 + 4 + 2 + 64


# ----------------------------------------------------------------------------- the restated loop
@pytest.mark.parametrize("solver", ["euler", "heun-2"])
def test_restated_loop_identities(solver):
    """APG with eta = 1 and no momentum is the plain guided loop of tests/loop_ref.py to rounding; every control moves the loop; a
    scale of 1 outside the interval and inside it makes the projected loop the conditional one exactly."""
    from foley_amd.host import synth
    from loop_harness import ref_loop
    sd = synth.synth_dit_state_dict(C.TINY)
    c = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
    run = lambda **kw: P.restated_loop(sd, C.TINY.heads, noise, c["text"], c["uncond_text"], c["clip"], c["sync"], 10, 4.5, solver, **kw)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    with torch.inference_mode():
        plain = ref_loop(sd, [c], noise, 10, 4.5, solver).x
        cfg = run(mode=P.APG, eta=1.0, momentum=0.0)
        assert rel(cfg, plain) < 1e-5
        apg, zs = run(mode=P.APG, eta=0.0, momentum=-0.5), run(mode=P.ZERO_STAR)
        assert rel(apg, plain) > 1e-2 and rel(zs, plain) > 1e-3
        assert rel(run(mode=P.APG, eta=0.0, momentum=0.0), apg) > 1e-3 and rel(run(mode=P.ZERO_STAR, zero_init=1), zs) > 1e-3
        if solver == "euler":
            norms = []
            run(mode=P.APG, eta=0.0, momentum=-0.5, norms=norms)
            assert len(norms) == 10 and rel(run(mode=P.APG, eta=0.0, momentum=-0.5, norm_threshold=0.5 * float(torch.stack(norms).min())), apg) > 1e-2
            part = run(mode=P.APG, eta=0.0, momentum=-0.5, interval=(0.2, 0.7))
            assert rel(part, apg) > 1e-2 and rel(part, ref_loop(sd, [c], noise, 10, 4.5, solver, interval=(0.2, 0.7)).x) > 1e-3


# ----------------------------------------------------------------------------- the C surface
def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    lib = rt.load_library()
    for name in ("foley_set_projected_guidance", "foley_op_guidance_project_work", "foley_op_guidance_project",
                 "foley_op_solver_step_projected"):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", hdr), name
        assert name in rt.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "#define FOLEY_GUIDANCE_APG 1" in hdr and "#define FOLEY_GUIDANCE_ZERO_STAR 2" in hdr
    assert re.search(r"typedef struct foley_projection_desc \{\s+const float\* rows;\s+float\* coef;\s+float\* plane;\s+int32_t mode;\s+\} foley_projection_desc;", hdr)
    assert re.search(r"int foley_set_projected_guidance\(foley_ctx\* ctx, int mode, const float\* rows, int n_rows, void\* stream\);", hdr)
    assert re.search(r"int foley_op_solver_step_projected\(const foley_step_desc\* d, const foley_projection_desc\* proj, void\* stream\);", hdr)
    assert_abi_version()
    assert lib.foley_op_guidance_project_work(1, 50) == 2 * 3 and lib.foley_op_guidance_project_work(3, 2081) == 3 * 66 * 3
    assert lib.foley_op_guidance_project_work(0, 50) == 0
    assert callable(rt.op_guidance_project) and callable(rt.projection_desc) and callable(rt.FoleyContext.set_projected_guidance)
    rc = lib.foley_set_projected_guidance(None, 1, None, 0, None)
    assert rc != 0 and lib.foley_last_error()
    import ctypes
    assert ctypes.sizeof(rt.ProjectionDescC) == 32 and ctypes.sizeof(rt.StepDescC) == 168
