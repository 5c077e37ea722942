"""Audio editing on the HIP engine: the blend step and start-state ops against torch, the 44.1 -> 48 kHz resample against a float64
restatement, the edit loop against the restated loop (tests/loop_ref.py), the exactness properties (all-ones mask =
plain run bit for bit, all-zeros mask under euler = x0), the plain / edit keying of the captured graph, and one full-size edit."""
import math

import pytest
import torch

import loop_harness as H
from conftest import rel_err
from foley_amd.host import audio_edit, config as C, runtime as rt, sampler, synth, tables
from foley_amd.host.sync_score import sinc_resample_taps
from step_harness import ref_step

pytestmark = pytest.mark.gpu

DAC_WINDOW_MARGIN = 16      # latent frames: tests/test_dac_window_cpu.py shows that it covers the decoder's receptive field


# ----------------------------------------------------------------------------- ops
@pytest.mark.parametrize("solver,steps", [("euler", 6), ("heun-2", 6), ("midpoint-2", 7), ("kutta-4", 8)])
@pytest.mark.parametrize("rows_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("x0_clips,mask_kind", [(1, "none"), (1, "binary"), (3, "fractional"), (3, "per_clip_binary")])
def test_blend_step_op(dev, solver, steps, rows_dtype, x0_clips, mask_kind):
    g = torch.Generator().manual_seed(7)
    clips, Cc, L, ncfg, guid = 3, 128, 75, 2, 4.5
    coef = tables.edit_solver_table(tables.sigma_grid(steps), solver, steps).to(dev)
    x = torch.randn(clips, Cc, L, generator=g).to(dev)
    x_saved, d_acc = torch.zeros_like(x), torch.zeros_like(x)
    x0 = torch.randn(x0_clips, Cc, L, generator=g).to(dev)
    noise = torch.randn(clips, Cc, L, generator=g).to(dev)
    mask = {"none": None,
            "binary": (torch.rand(L, generator=g) > 0.5).float(),
            "fractional": torch.rand(clips, L, generator=g),
            "per_clip_binary": (torch.rand(clips, L, generator=g) > 0.5).float()}[mask_kind]
    if mask is not None:
        mask = mask.to(dev)
        if mask_kind == "fractional":
            mask[:, :5] = 0.0
            mask[:, 5:10] = 1.0
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    step_p = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = torch.empty(ncfg * clips * L, Cc, dtype=rows_dtype, device=dev)
    rows_p = torch.empty_like(rows)
    for it in range(steps):
        pred = torch.randn(ncfg * clips * L, Cc, generator=g).to(dev)
        ref = ref_step(pred, x, x_saved, d_acc, coef[it].cpu(), ncfg, guid, x0, noise, mask)
        xp, xsp, dap = x.clone(), x_saved.clone(), d_acc.clone()
        step_p.fill_(it)
        rt.op_solver_step(pred, xp, xsp, dap, ncfg, guid, coef, step_p, rows_p)          # the plain step on the same state
        rt.op_solver_step(pred, x, x_saved, d_acc, ncfg, guid, coef, step, rows, edit=(x0, noise, mask))
        torch.cuda.synchronize()
        assert int(step) == it + 1
        for got, want in zip((x, x_saved, d_acc), ref):
            assert rel_err(got, want) < 1e-6, (it, mask_kind)
        assert torch.equal(x_saved, xsp) and torch.equal(d_acc, dap)
        blend = int(coef[it, 4]) & tables.STEP_BLEND
        keep_plain = torch.ones(L, dtype=torch.bool, device=dev) if mask is None or not blend else None
        if keep_plain is not None:
            assert torch.equal(x, xp)                                                     # no blend / all ones: the plain step exactly
            assert torch.equal(rows, rows_p)
        else:
            mm = mask.view(-1, 1, L).expand(clips, Cc, L)
            assert torch.equal(x[mm == 1], xp[mm == 1])                                    # m = 1: the plain update bit for bit
            if float(coef[it, 5]) == 0.0:
                assert torch.equal(x[mm == 0], x0.expand(clips, -1, -1)[mm == 0])          # m = 0 at sigma 0: exactly x0
        want_rows = x.permute(0, 2, 1).reshape(clips * L, Cc).to(rows_dtype)
        tol = 0 if rows_dtype == torch.float32 else 1e-2
        for c in range(ncfg):
            r = rows[c * clips * L:(c + 1) * clips * L]
            assert (torch.equal(r, want_rows) if tol == 0 else rel_err(r.float(), want_rows.float()) < tol)


def test_flow_mix_op(dev):
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(3, 128, 77, generator=g).to(dev)
    for x0c in (1, 3):
        x0 = torch.randn(x0c, 128, 77, generator=g).to(dev)
        for s in (1.0, 0.73, 0.25, 0.0):
            out = rt.op_flow_mix(noise, x0, s)
            assert rel_err(out, s * noise + (1 - s) * x0) < 1e-6
            if s == 1.0:
                assert torch.equal(out, noise)
            if s == 0.0:
                assert torch.equal(out, x0.expand_as(out))
    with pytest.raises(rt.FoleyRuntimeError):
        rt.op_flow_mix(noise, torch.zeros(2, 128, 77, device=dev), 0.5)


def test_resample_44k1_to_48k(dev):
    """foley_op_resample_sinc at 44.1 -> 48 kHz (orig 147, new 160) against a float64 restatement of torchaudio's polyphase sum."""
    taps, o, n, width = sinc_resample_taps(44100, 48000)
    assert (o, n) == (147, 160) and taps.shape == (160, 2 * width + 147)
    N = 44100 // 4 + 37
    t = torch.arange(N, dtype=torch.float64) / 44100
    x = torch.stack([torch.sin(2 * math.pi * 440 * t) + 0.3 * torch.sin(2 * math.pi * 9000 * t),
                     0.1 * torch.randn(N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)]).float()
    out = rt.op_resample_sinc(x.to(dev), o, n, taps.to(dev), width).cpu()
    n_out = -(-N * n // o)
    assert out.shape == (2, n_out)
    xp = torch.nn.functional.pad(x.double(), (width, width + o))
    frames = xp.unfold(1, taps.shape[1], o)                                # [2, n_frames, ntaps]
    ref = torch.einsum("bft,pt->bfp", frames, taps.double()).reshape(2, -1)[:, :n_out]
    assert rel_err(out, ref) < 1e-6


# ----------------------------------------------------------------------------- loop
@pytest.fixture(scope="module")
def tiny(dev):
    sd, dsd, model, dac, _ = H.tiny_run(dev, 0)
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd)
    g = torch.Generator().manual_seed(21)
    noise = torch.randn(2, 128, 50, generator=g)
    x0 = 0.7 * torch.randn(1, 128, 50, generator=g)
    return sd, dsd, model, dac, cond, noise, x0


@pytest.mark.parametrize("solver,steps", [("euler", 10), ("heun-2", 10), ("kutta-4", 16)])
@pytest.mark.parametrize("strength", [1.0, 0.6, 0.3])
@pytest.mark.parametrize("use_graph", [False, True])
def test_edit_loop_matches_oracle(tiny, solver, steps, strength, use_graph):
    sd, _dsd, model, dac, cond, noise, x0 = tiny
    mask = audio_edit.build_mask(50, [(0.3, 0.6)], 0.1)
    want = H.ref_loop(sd, [cond], noise, steps, 4.5, solver, edit=(x0, mask, strength)).x
    lat = H.run(model, dac, [cond], noise, solver, steps, 4.5, use_graph, edit=audio_edit.EditSpec(x0, strength, mask))[2]
    assert rel_err(lat, want) < 1e-4


def test_edit_loop_matches_oracle_past_the_flow_mix_grid_cap(tiny):
    """Six clips of 30 s: batch * La = 9000 frames, 1 152 000 latent elements - more than 4096 workgroups of 256 reach without
    striding - at strength 0.5, so the run starts from foley_op_flow_mix's output (host/sampler.py) and not from the noise.  A start
    state whose tail was never written (the kernel before it became a grid-stride loop) does not match the oracle."""
    sd, _dsd, model, dac, _cond, _noise, _x0 = tiny
    dur, clips, steps = 30.0, 6, 4
    La = C.lengths(dur)[0]
    assert clips * La > 8192
    cond = synth.synth_conditioning(C.TINY, dur, t2a=False, sd=sd)
    g = torch.Generator().manual_seed(22)
    noise, x0 = torch.randn(clips, 128, La, generator=g), 0.7 * torch.randn(1, 128, La, generator=g)
    mask = audio_edit.build_mask(La, [(0.3 * dur, 0.6 * dur)], 0.1)
    want = H.ref_loop(sd, [cond], noise, steps, 4.5, "euler", edit=(x0, mask, 0.5)).x
    vis, txt = H.batched([cond])
    _a, _sr, lat = sampler.denoise_process_with_generator(vis, txt, dur, model, dac, 4.5, steps, clips, "euler", noise=noise,
                                                          return_latents=True, edit=audio_edit.EditSpec(x0, 0.5, mask))
    assert rel_err(lat, want) < 1e-4


@pytest.mark.parametrize("use_graph", [False, True])
def test_all_ones_at_strength_1_is_the_plain_run(tiny, use_graph):
    _sd, _dsd, model, dac, cond, _noise, x0 = tiny
    vis, txt = H.batched([cond])
    for solver in ("euler", "heun-2"):
        a0, _, l0 = sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, 4.5, 10, 2, solver, return_latents=True,
                                                           generator=torch.Generator("cpu").manual_seed(99), use_graph=use_graph)
        a1, _, l1 = sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, 4.5, 10, 2, solver, return_latents=True,
                                                           generator=torch.Generator("cpu").manual_seed(99), use_graph=use_graph,
                                                           edit=audio_edit.EditSpec(x0, 1.0, torch.ones(50)))
        assert torch.equal(l0, l1) and torch.equal(a0, a1), solver


def test_all_zeros_under_euler_returns_x0(tiny):
    _sd, _dsd, model, dac, cond, noise, _x0 = tiny
    vis, txt = H.batched([cond])
    x0 = torch.randn(2, 128, 50, generator=torch.Generator().manual_seed(4))
    for strength in (1.0, 0.5):
        _a, _, lat = sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, 4.5, 10, 2, "euler", noise=noise,
                                                            return_latents=True, edit=audio_edit.EditSpec(x0, strength, torch.zeros(2, 50)))
        assert torch.equal(lat.cpu(), x0), strength


def test_graph_keyed_on_plain_vs_edit(tiny, dev):
    """One context, use_graph=True: plain -> edit -> plain -> edit of the same shape (strength 1: the same plan, so the
    captured iteration would be reused if it were not keyed); each run equals a fresh context's bit for bit."""
    sd, dsd, model, dac, cond, noise, x0 = tiny
    vis, txt = H.batched([cond])
    ed = audio_edit.EditSpec(x0, 1.0, audio_edit.build_mask(50, [(0.2, 0.5)], 0.1))

    def run(m, d, edit):
        return sampler.denoise_process_with_generator(vis, txt, 1.0, m, d, 4.5, 10, 2, "euler", noise=noise, use_graph=True,
                                                      return_latents=True, edit=edit)[2].cpu()

    def fresh(edit):
        m = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
        return run(m, sampler.FoleyDAC(dsd, dev, C.DAC_TINY), edit)

    want_plain, want_edit = fresh(None), fresh(ed)
    assert not torch.equal(want_plain, want_edit)
    for edit, want in ((None, want_plain), (ed, want_edit), (None, want_plain), (ed, want_edit)):
        assert torch.equal(run(model, dac, edit), want)


def test_set_edit_refusals(tiny, dev):
    _sd, _dsd, model, dac, cond, noise, x0 = tiny
    vis, txt = H.batched([cond])
    plan = sampler.build_plan(model, vis, txt, 50, 4.5, 10, 2, "euler", edit_i0=0)
    model.ctx.prepare(plan)
    z = torch.zeros(2, 128, 50, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="x0 and noise"):
        model.ctx.set_edit(None, z, torch.ones(50, device=dev))
    with pytest.raises(rt.FoleyRuntimeError, match="x0_clips"):
        model.ctx.set_edit(torch.zeros(3, 128, 50, device=dev), z)
    with pytest.raises(rt.FoleyRuntimeError, match="mask_clips"):
        model.ctx.set_edit(z, z, torch.ones(3, 50, device=dev))
    model.ctx.set_edit(None, None)                                       # clears


# ----------------------------------------------------------------------------- full size
def test_full_size_span_regeneration(dev):
    """xxl, bf16, 5 s, two clips, regenerate [(2.0, 3.0)] with a 0.1 s crossfade, euler, source audio at 44.1 kHz stereo.
    Kept latent frames end at exactly x0; outside the span, its crossfade and DAC_WINDOW_MARGIN frames, the waveform equals
    decode(encode(source)) to 1e-3 relative; inside the span it differs from it.  The same edit through denoise_process_multi
    (one replica) gives the same result bit for bit."""
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    vis, txt = H.batched([cond])
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev, encoder=True), dev, C.DAC48K)
    t = torch.arange(int(5.2 * 44100), dtype=torch.float32) / 44100
    wave = torch.stack([0.3 * torch.sin(2 * math.pi * 220 * t), 0.2 * torch.sin(2 * math.pi * 1300 * t + 0.5)])[None]
    audio = {"waveform": wave, "sample_rate": 44100}
    edit = audio_edit.prepare_edit(audio, model, dac, 5.0, 10, "euler", 2, regenerate=[(2.0, 3.0)], crossfade_s=0.1)
    assert edit.x0.shape == (1, 128, 250) and torch.isfinite(edit.x0).all()
    out, sr, lat = sampler.denoise_process_with_generator(vis, txt, 5.0, model, dac, 4.5, 10, 2, "euler",
                                                          generator=torch.Generator("cpu").manual_seed(5), return_latents=True,
                                                          edit=edit)
    assert out.shape == (2, 1, 250 * 960) and torch.isfinite(out).all()
    keep = edit.mask == 0
    assert torch.equal(lat[..., keep.to(lat.device)], edit.x0[..., keep.to(lat.device)].expand(2, -1, -1))
    src = model.ctx.dac_decode(edit.x0)
    hop, M = 960, DAC_WINDOW_MARGIN
    lo_end, hi_start = (95 - M) * hop, (155 + M) * hop
    errs = []
    for c in range(2):
        errs.append(rel_err(out[c, :, :lo_end], src[0, :, :lo_end]))
        errs.append(rel_err(out[c, :, hi_start:], src[0, :, hi_start:]))
        assert rel_err(out[c, :, 100 * hop:150 * hop], src[0, :, 100 * hop:150 * hop]) > 0.05
    print("outside-span waveform vs decode(encode(source)): max rel %.2e" % max(errs))
    assert max(errs) < 1e-3
    reps = sampler.replicate(model, dac, [dev])
    out2, _sr, lat2 = sampler.denoise_process_multi(vis, txt, 5.0, reps, 4.5, 10, 2, "euler",
                                                    generator=torch.Generator("cpu").manual_seed(5), return_latents=True,
                                                    edit=edit)
    assert torch.equal(lat2, lat) and torch.equal(out2, out)
