"""FlowEdit on the HIP engine: the loop against the restated loop (tests/flowedit_ref.py), the keep exactness of the mask, the
keying of the captured graph on plain vs FlowEdit runs, every refusal of foley_set_flowedit, and one full-size edit."""
import math

import pytest
import torch

import flowedit_ref as FR
import loop_harness as H
from conftest import rel_err
from foley_amd.host import audio_edit, config as C, prompt_timeline, runtime as rt, sampler, synth, tables

pytestmark = pytest.mark.gpu

DAC_WINDOW_MARGIN = 16      # latent frames: tests/test_dac_window_cpu.py shows that it covers the decoder's receptive field
V, STEPS, G_SRC, G_TAR, SEED = 2, 10, 2.0, 4.5, 31


@pytest.fixture(scope="module")
def tiny(dev):
    sd, dsd, model, dac, conds = H.tiny_run(dev, 2)
    x0 = 0.7 * torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(21))
    return sd, dsd, model, dac, conds, x0


def _feats(conds, target=1):
    """Visual features and the negative prompt of conditioning 0; the source text of conditioning 0, the target's of `target`."""
    c0 = conds[0]
    return ({"siglip2_feat": c0["clip"], "syncformer_feat": c0["sync"]},
            {"source_text_feat": c0["text"], "text_feat": conds[target]["text"], "uncond_text_feat": c0["uncond_text"]})


def _run(model, dac, conds, spec, use_graph=False, target=1, g_tar=G_TAR):
    vis, txt = _feats(conds, target)
    return sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, g_tar, STEPS, V, "euler", use_graph=use_graph,
                                                  generator=torch.Generator("cpu").manual_seed(SEED), return_latents=True, edit=spec)[2].cpu()


_REFS = {}


def _ref(sd, conds, x0, strength, kind, mask, target=1, g_tar=G_TAR):
    key = (strength, kind, mask is not None, target, g_tar)
    if key not in _REFS:
        n_iter = STEPS - tables.edit_start(STEPS, "euler", strength)[1]
        table = audio_edit.flowedit_noise(torch.Generator("cpu").manual_seed(SEED), n_iter if kind == "fresh" else 1, V, 128, 50, torch.float32)
        c0 = conds[0]
        with torch.inference_mode():
            vel = FR.model_velocity(sd, C.TINY.heads, c0["text"], conds[target]["text"], c0["uncond_text"], c0["clip"], c0["sync"], G_SRC, g_tar,
                                    V, STEPS)
            _REFS[key] = FR.restated_flowedit(vel, x0, table, STEPS, strength=strength, mask=mask)
    return _REFS[key]


SPAN = lambda: audio_edit.build_mask(50, [(0.3, 0.6)], 0.1)


@pytest.mark.parametrize("strength", [1.0, 0.6])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind", ["fresh", "fixed"])
@pytest.mark.parametrize("masked", [False, True])
def test_flowedit_loop_matches_the_restated_loop(tiny, strength, use_graph, kind, masked):
    sd, _dsd, model, dac, conds, x0 = tiny
    mask = SPAN() if masked else None
    want = _ref(sd, conds, x0, strength, kind, mask)
    got = _run(model, dac, conds, audio_edit.FlowEditSpec(x0, strength, mask, G_SRC, kind), use_graph)
    assert rel_err(got, want) < 1e-4
    if masked:                                   # the kept frames are x0 bit for bit
        keep = mask == 0
        assert bool(keep.any()) and torch.equal(got[..., keep], x0[..., keep].expand(V, -1, -1))


def test_equal_prompts_and_scales_are_the_identity_to_rounding(tiny):
    """Target text == source text and equal scales: checked against the reference like every other case.  The deviation from
    x0 is printed - the two clips of a pair pass the GEMMs at different rows, so it is rounding, not zero - and no bound is set."""
    sd, _dsd, model, dac, conds, x0 = tiny
    want = _ref(sd, conds, x0, 1.0, "fresh", None, target=0, g_tar=G_SRC)
    got = _run(model, dac, conds, audio_edit.FlowEditSpec(x0, 1.0, None, G_SRC, "fresh"), target=0, g_tar=G_SRC)
    assert rel_err(got, want) < 1e-4
    print("equal prompts and scales: |z - x0| / |x0| = %.3e (device), %.3e (reference)" %
          (rel_err(got, x0.expand(V, -1, -1)), rel_err(want, x0.expand(V, -1, -1))))


def test_the_edit_does_something(tiny):
    _sd, _dsd, model, dac, conds, x0 = tiny
    got = _run(model, dac, conds, audio_edit.FlowEditSpec(x0, 1.0, None, G_SRC, "fresh"))
    assert rel_err(got, x0.expand(V, -1, -1)) > 1e-3
    vis, txt = _feats(conds)
    plain = sampler.denoise_process_with_generator(vis, {k: txt[k] for k in ("text_feat", "uncond_text_feat")}, 1.0, model, dac, G_TAR,
                                                   STEPS, V, "euler", generator=torch.Generator("cpu").manual_seed(SEED),
                                                   return_latents=True)[2].cpu()
    assert rel_err(got, plain) > 1e-3


def test_graph_keyed_on_plain_vs_flowedit(tiny, dev):
    """One context, use_graph=True: a plain 2V-clip per-clip-prompt run -> FlowEdit -> plain -> FlowEdit of the same shape
    (strength 1: the same dimensions, so the captured iteration would be reused if it were not keyed on the FlowEdit operands);
    each run equals a fresh context's bit for bit."""
    sd, dsd, model, dac, conds, x0 = tiny
    vis, txt = _feats(conds)
    _v, pair_txt = sampler.flowedit_features(vis, txt, V)
    noise = H.noise(2 * V, seed=8)
    spec = audio_edit.FlowEditSpec(x0, 1.0, SPAN(), G_SRC, "fresh")

    def run(m, d, flowedit):
        if flowedit:
            return _run(m, d, conds, spec, use_graph=True)
        return sampler.denoise_process_with_generator(vis, pair_txt, 1.0, m, d, G_TAR, STEPS, 2 * V, "euler", noise=noise, use_graph=True,
                                                      return_latents=True)[2].cpu()

    def fresh(flowedit):
        m = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
        return run(m, sampler.FoleyDAC(dsd, dev, C.DAC_TINY), flowedit)

    want = {False: fresh(False), True: fresh(True)}
    assert want[False].shape == (2 * V, 128, 50) and want[True].shape == (V, 128, 50)
    for flowedit in (False, True, False, True):
        assert torch.equal(run(model, dac, flowedit), want[flowedit]), flowedit


def test_set_flowedit_refusals(tiny, dev):
    sd, _dsd, model, dac, conds, _x0 = tiny
    vis, txt = _feats(conds)
    _v, pair_txt = sampler.flowedit_features(vis, txt, V)
    ctx = model.ctx
    z = lambda *s: torch.zeros(*s, device=dev)
    x, n, n1 = z(1, 128, 50), z(STEPS, V, 128, 50), z(1, V, 128, 50)

    def prepare(clips=2 * V, scale=G_TAR, solver="euler", edit_i0=0, text=pair_txt, **kw):
        ctx.prepare(sampler.build_plan(model, vis, text, 50, scale, STEPS, clips, solver, edit_i0=edit_i0, **kw))

    unprepared = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    with pytest.raises(rt.FoleyRuntimeError, match="foley_prepare has not been called"):
        unprepared.ctx.set_flowedit(x, n)
    shared = {k: txt[k] for k in ("text_feat", "uncond_text_feat")}
    prepare(scale=1.0, text=shared)
    with pytest.raises(rt.FoleyRuntimeError, match="plan.ncfg must be 2"):
        ctx.set_flowedit(x, n)
    prepare(clips=3, text=shared)
    with pytest.raises(rt.FoleyRuntimeError, match="plan.clips even"):
        rt._check(ctx.lib, ctx.lib.foley_set_flowedit(ctx._h, x.data_ptr(), 1, n.data_ptr(), STEPS, None, 0, G_SRC, G_TAR, 1.0, None), "set")
    prepare(edit_i0=None)
    with pytest.raises(rt.FoleyRuntimeError, match="FOLEY_STEP_BLEND"):
        ctx.set_flowedit(x, n)
    prepare(solver="heun-2")
    with pytest.raises(rt.FoleyRuntimeError, match="FOLEY_STEP_BLEND"):
        ctx.set_flowedit(x, n)
    prepare()
    with pytest.raises(rt.FoleyRuntimeError, match="noise_rows"):
        ctx.set_flowedit(x, z(3, V, 128, 50))
    with pytest.raises(rt.FoleyRuntimeError, match="src_clips"):
        ctx.set_flowedit(z(3, 128, 50), n)
    with pytest.raises(rt.FoleyRuntimeError, match="mask_clips"):
        ctx.set_flowedit(x, n, z(3, 50))
    with pytest.raises(rt.FoleyRuntimeError, match="noise table is required"):
        rt._check(ctx.lib, ctx.lib.foley_set_flowedit(ctx._h, x.data_ptr(), 1, None, STEPS, None, 0, G_SRC, G_TAR, 1.0, None), "set")
    for gs, gt in ((1.0, G_TAR), (G_SRC, 1.0), (float("inf"), G_TAR), (G_SRC, float("nan"))):
        with pytest.raises(rt.FoleyRuntimeError, match="finite and > 1"):
            ctx.set_flowedit(x, n, g_src=gs, g_tar=gt)
    with pytest.raises(rt.FoleyRuntimeError, match="sigma0"):
        ctx.set_flowedit(x, n, sigma0=1.5)
    # a state of another option refuses FlowEdit, and a FlowEdit state refuses the option: either call order
    x4, n4, w = z(1, 128, 50), z(2 * V, 128, 50), torch.full((2, 50), 0.5, device=dev)
    sched = tables.guidance_schedule(STEPS, G_TAR, G_TAR, (0.0, 0.5))
    proj = tables.projection_rows(STEPS, "apg")
    options = [("edit run", lambda: ctx.set_edit(x4, n4)), ("windows", lambda: ctx.set_windows([0, 25], w)),
               ("multistep", lambda: ctx.set_multistep(2)), ("schedule / rescale", lambda: ctx.set_guidance(sched)),
               ("schedule / rescale", lambda: ctx.set_guidance(None, 0.5)), ("projected-guidance", lambda: ctx.set_projected_guidance(1, proj)),
               ("step-cache", lambda: ctx.set_step_cache(mode=1, skip=[0] * STEPS))]
    for reason, set_option in options:
        prepare()
        set_option()
        with pytest.raises(rt.FoleyRuntimeError, match="foley_set_flowedit.*" + reason):
            ctx.set_flowedit(x, n1)
        prepare()
        ctx.set_flowedit(x, n1)
        with pytest.raises(rt.FoleyRuntimeError, match="FlowEdit state"):
            set_option()
    tl = prompt_timeline.parse([(0.0, 0.5, "a")], "b", 1.0, 0.1)
    assert len(tl.prompts) == 2
    prepare(clips=2 * V, text={"text_feat": torch.cat([conds[0]["text"], conds[1]["text"]]), "uncond_text_feat": conds[0]["uncond_text"]},
            timeline=tl)
    with pytest.raises(rt.FoleyRuntimeError, match="prompt timeline"):
        ctx.set_flowedit(x, n1)
    # clearing: a NULL source, and foley_prepare
    prepare()
    ctx.set_flowedit(x, n1)
    ctx.set_flowedit(None)
    ctx.set_multistep(2)
    ctx.set_multistep(0)
    ctx.set_flowedit(x, n, z(50))
    prepare()
    ctx.set_edit(x4, n4)
    ctx.set_edit(None, None)


# ----------------------------------------------------------------------------- full size
def test_full_size_flowedit_of_a_span(dev):
    """xxl, bf16, 5 s, one variation, 10 euler steps, a 44.1 kHz stereo sine source, regenerate [(2.0, 3.0)] with a 0.1 s crossfade.
    The kept latent frames are x0 bit for bit; outside the span, its crossfade and DAC_WINDOW_MARGIN frames the waveform equals
    decode(x0) to 1e-3 relative (test_edit_gpu.test_full_size_span_regeneration's bound, for the same reason); inside the span
    the latents differ from x0."""
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    other = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev, seed=17)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"source_text_feat": cond["text"], "text_feat": other["text"], "uncond_text_feat": cond["uncond_text"]}
    assert not torch.equal(cond["text"], other["text"])
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev, encoder=True), dev, C.DAC48K)
    t = torch.arange(int(5.2 * 44100), dtype=torch.float32) / 44100
    wave = torch.stack([0.3 * torch.sin(2 * math.pi * 220 * t), 0.2 * torch.sin(2 * math.pi * 1300 * t + 0.5)])[None]
    spec = audio_edit.prepare_edit({"waveform": wave, "sample_rate": 44100}, model, dac, 5.0, 10, "euler", 1, regenerate=[(2.0, 3.0)],
                                   crossfade_s=0.1, flowedit={"source_scale": G_SRC, "noise": "fresh"})
    assert isinstance(spec, audio_edit.FlowEditSpec) and spec.x0.shape == (1, 128, 250) and torch.isfinite(spec.x0).all()
    out, _sr, lat = sampler.denoise_process_with_generator(vis, txt, 5.0, model, dac, G_TAR, 10, 1, "euler",
                                                           generator=torch.Generator("cpu").manual_seed(5), return_latents=True, edit=spec)
    assert out.shape == (1, 1, 250 * 960) and torch.isfinite(out).all()
    keep = (spec.mask == 0).to(lat.device)
    assert torch.equal(lat[..., keep], spec.x0[..., keep])
    src = model.ctx.dac_decode(spec.x0)
    hop, M = 960, DAC_WINDOW_MARGIN
    lo_end, hi_start = (95 - M) * hop, (155 + M) * hop
    errs = [rel_err(out[0, :, :lo_end], src[0, :, :lo_end]), rel_err(out[0, :, hi_start:], src[0, :, hi_start:])]
    print("outside-span waveform vs decode(x0): max rel %.2e" % max(errs))
    assert max(errs) < 1e-3
    assert rel_err(lat[..., 100:150], spec.x0[..., 100:150]) > 1e-3
