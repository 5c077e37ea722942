"""LoRA adapters merged into the packed weights on the GPU (csrc/lora.hip through host/lora.py).

Every element of a touched packed tensor is held to  |got - ref64| <= (R_tot + 4) * U32 * mag + output term  against the fp64
restatement of tests/lora_ref.py, placed in the packed layout by host/packers.py itself; everything an adapter does not target
must keep its bytes.  Then the state machine (clear, replace, repeat, refusals), both load paths, the sampling loop with its
captured graph, and the node."""
import dataclasses
import logging
import re
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

import lora_ref as LR
import opcheck as oc
import weights_ref as W
from foley_amd import nodes
from foley_amd.host import config as C, lora, packers, runtime as rt, sampler, synth
from oracle import foley_oracle as O

pytestmark = pytest.mark.gpu
MINI, DAC_MINI = LR.MINI, LR.DAC_MINI

MINI_KEYS = OrderedDict([                                     # one key of each layout kind -> rank
    ("triple_blocks.0.audio_cross_q.weight", 1),              # plain
    ("triple_blocks.0.v_cond_attn_qkv.weight", 5),            # triple qkv
    ("single_blocks.1.linear_qkv.weight", 16),                # (H D K) -> (K H D)
    ("single_blocks.1.linear1.weight", 5),                    # conv, tap-major
    ("single_blocks.0.linear2.w1.weight", 16),                # gate half alone
    ("single_blocks.0.linear2.w2.weight", 1),
    ("single_blocks.1.modulation.linear.weight", 5),          # stacked, block 1 only
    ("visual_proj.w3.weight", 16),                            # compute-dtype embedder, odd width (clip_dim 5)
    ("final_layer.linear.weight", 1),
])


def _shapes(cfg):
    return {k: v[0] for k, v in synth.dit_schema(cfg).items()}


def _state(cfg, dev):
    return W.make_state(synth.dit_schema(cfg), dev, gen=W.value_tensor, emin=-3, emax=1)


def _dac_state(dac_cfg, dev):
    dsd = W.make_state(synth.dac_decoder_schema(dac_cfg), dev, gen=W.value_tensor, emin=-3, emax=1)
    folded, pairs = W.respell_dac(dsd, dac_cfg, lambda i: 2)
    assert not pairs
    return folded


def _ctx_model(cfg, dac_cfg, cdt, fmt, sd, dsd, dev):
    ctx = rt.FoleyContext(cfg, dac_cfg, cdt, dev)
    ctx.load_reference_state([sd, dsd], fmt)
    return SimpleNamespace(ctx=ctx, cfg=cfg, device=dev)


def _slots(ctx):
    return OrderedDict((s["name"], ctx.weights_slot_tensor(s["name"])) for s in ctx.weights_slots())


def _check_merge(cfg, pre, post, specs, what):
    """Touched elements inside the bound, everything else bit-identical.  Returns the largest error / bound."""
    plan = lora.plan_merge(lora.normalize(specs), cfg)
    keys, shapes = list(plan), _shapes(cfg)
    dev = next(iter(pre.values())).device
    index = LR.slot_index(cfg, keys, dev)
    stored = LR.unroute(index, keys, shapes, pre)
    plan_dev = OrderedDict((k, [(d.to(dev), u.to(dev), s) for d, u, s in v]) for k, v in plan.items())
    ref, mag = LR.merge64(stored, plan_dev)
    ranks = {k: torch.full(shapes[k], float(sum(int(d.shape[0]) for d, _u, _s in plan[k])), dtype=torch.float64, device=dev) for k in keys}
    worst, touched = 0.0, 0
    for name, before in pre.items():
        after = post[name]
        if name not in index:
            assert torch.equal(W.bits(after), W.bits(before)), f"{what}: untargeted packed tensor {name} changed"
            continue
        which = index[name][0]
        keep = which == 0
        assert torch.equal(W.bits(after)[keep], W.bits(before)[keep]), f"{what}: {name}: elements outside the targeted rows changed"
        base = before.to(torch.float32).double()
        exp = LR.route(index, keys, name, base, ref)
        m = LR.route(index, keys, name, base.abs(), mag)
        r_tot = LR.route(index, keys, name, torch.zeros_like(base), ranks)
        got = after.to(torch.float32).double()
        b = LR.bound(exp, got, m, r_tot, after.dtype)
        err = (got - exp).abs()
        bad = ~(err <= b) & ~keep
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            r, c = divmod(i, before.shape[-1])
            raise AssertionError(f"{what}: {name}: {int(bad.sum())} of {int((~keep).sum())} merged elements outside their bound; first at "
                                 f"(row {r}, col {c}): got {float(got.flatten()[i])!r} ref {float(exp.flatten()[i])!r} "
                                 f"bound {float(b.flatten()[i]):.3e} pristine {float(base.flatten()[i])!r}")
        assert bool((got[~keep] != base[~keep]).any()), f"{what}: {name}: the merge changed nothing"
        worst = max(worst, float((err / b.clamp_min(1e-300))[~keep].max()))
        touched += 1
    assert touched == len(index)
    return worst


# ----------------------------------------------------------------------------- per-element merge on MINI, every arena
_MINI = {}


def _mini_specs():
    """Three adapter files: fp32 over every layout kind (ranks 1 / 5 / 16), a bf16 kohya file with alpha on two of the keys (two
    adapters on one key) and an fp16 one on the conv (three on that key)."""
    if "specs" not in _MINI:
        sh = _shapes(MINI)
        a = LR.spell(LR.make_adapter(sh, MINI_KEYS, torch.float32, seed=1), "peft", "base_model.model.")
        b = LR.spell(LR.make_adapter(sh, {"single_blocks.1.linear1.weight": 16, "single_blocks.1.linear_qkv.weight": 1}, torch.bfloat16,
                                     seed=2, alpha=8.0), "kohya")
        c = LR.spell(LR.make_adapter(sh, {"single_blocks.1.linear1.weight": 1}, torch.float16, seed=3, alpha=0.5), "comfy", "diffusion_model.")
        _MINI["specs"] = [(a, 0.8), (b, -0.5), (c, 1.0)]
    return _MINI["specs"]


@pytest.mark.parametrize("arena", [a[0] for a in W.ARENAS])
def test_merge_per_element_every_layout(dev, arena):
    _label, cdt, fmt = next(a for a in W.ARENAS if a[0] == arena)
    if "sd" not in _MINI:
        _MINI["sd"], _MINI["dsd"] = _state(MINI, dev), _dac_state(DAC_MINI, dev)
    model = _ctx_model(MINI, DAC_MINI, cdt, fmt, _MINI["sd"], _MINI["dsd"], dev)
    try:
        pre = _slots(model.ctx)
        assert pre["s0.w13.w"].dtype == (W.F8[fmt] or cdt) and pre["vis.w13.w"].dtype == cdt
        assert lora.ensure(model, _mini_specs()) is True
        post = _slots(model.ctx)
        worst = _check_merge(MINI, pre, post, _mini_specs(), f"mini {arena}")
        assert model.ctx.lora_backup_bytes() == sum(pre[n].numel() * pre[n].element_size() for n in
                                                    LR.slot_index(MINI, list(lora.plan_merge(lora.normalize(_mini_specs()), MINI))))
        assert lora.ensure(model, None) is True and model.ctx.lora_backup_bytes() == 0
        back = _slots(model.ctx)
        assert all(torch.equal(W.bits(back[n]), W.bits(pre[n])) for n in pre)
    finally:
        model.ctx.close()
    print(f"mini {arena}: worst error / bound {worst:.3f}")


# ----------------------------------------------------------------------------- real width, ragged tiles
_XL = {}
XL_KEYS = ("single_blocks.1.linear_qkv.weight", "single_blocks.0.linear2.w1.weight", "single_blocks.0.linear2.w2.weight",
           "triple_blocks.0.audio_mlp.fc1.weight")


@pytest.mark.parametrize("rank", [16, 256])
@pytest.mark.parametrize("arena", ["bf16", "bf16+e4m3fn"])
def test_merge_at_real_width(dev, arena, rank):
    """xl: 1408 = 11 x 128 columns (no multiple of the 256-column fp8 tile), 3840-row SwiGLU halves, 4224-row qkv."""
    _label, cdt, fmt = next(a for a in W.ARENAS if a[0] == arena)
    cfg = dataclasses.replace(C.XL, depth_triple=1, depth_single=2)
    if "sd" not in _XL:
        _XL["sd"], _XL["dsd"] = _state(cfg, dev), _dac_state(C.DAC_TINY, dev)
    ad = LR.make_adapter(_shapes(cfg), {k: rank for k in XL_KEYS}, torch.bfloat16, seed=rank, alpha=float(rank) / 2)
    specs = [(LR.spell(ad, "comfy"), 0.7)]
    model = _ctx_model(cfg, C.DAC_TINY, cdt, fmt, _XL["sd"], _XL["dsd"], dev)
    try:
        pre = _slots(model.ctx)
        lora.ensure(model, specs)
        post = _slots(model.ctx)
        worst = _check_merge(cfg, pre, post, specs, f"xl {arena} rank {rank}")
    finally:
        model.ctx.close()
        del pre, post
        torch.cuda.empty_cache()
    print(f"xl {arena} rank {rank}: worst error / bound {worst:.3f}")


# ----------------------------------------------------------------------------- state machine on the packers' arena
G = 4096


def _guarded_model(cfg, dac_cfg, sd, cdt, dev):
    packed = packers.pack_dit(sd, cfg, cdt)
    total, _table = packers.arena_layout(packed)
    big = torch.full((total + 2 * G,), oc.GUARD_BITS[1], dtype=torch.uint8, device=dev)
    arena = packers.Arena.from_packed(packed, dev, buffer=big[G:G + total])
    return sampler.FoleyModel.from_arena(cfg, arena, cdt, dev, dac_cfg=dac_cfg), big, total


def _guards_ok(big, total):
    return bool((big[:G] == oc.GUARD_BITS[1]).all()) and bool((big[G + total:] == oc.GUARD_BITS[1]).all())


def test_state_machine_and_guards(dev):
    sd = OrderedDict((k, v.cpu()) for k, v in _state(MINI, dev).items())
    sh = _shapes(MINI)
    A = [(LR.spell(LR.make_adapter(sh, MINI_KEYS, torch.float32, seed=5), "peft"), 0.6)]
    B = [(LR.spell(LR.make_adapter(sh, {"single_blocks.0.linear2.w3.weight": 5, "triple_blocks.0.audio_cross_q.weight": 16},
                                   torch.bfloat16, seed=6, alpha=3.0), "kohya"), -1.2)]
    model, big, total = _guarded_model(MINI, DAC_MINI, sd, torch.bfloat16, dev)
    fresh, big2, _t = _guarded_model(MINI, DAC_MINI, sd, torch.bfloat16, dev)
    orig = model.arena.buffer.clone()
    lora.ensure(model, A)
    with_a = model.arena.buffer.clone()
    assert not torch.equal(with_a, orig)
    lora.ensure(model, None)
    assert torch.equal(model.arena.buffer, orig)                     # clear: the original bytes
    lora.ensure(model, A)
    assert torch.equal(model.arena.buffer, with_a)                   # A again: identical bytes
    lora.ensure(model, B)                                            # A, then B ...
    lora.ensure(fresh, B)
    assert torch.equal(model.arena.buffer, fresh.arena.buffer)       # ... equals a fresh model that merged B
    assert not torch.equal(model.arena.buffer, orig)
    lora.ensure(model, A + B)
    ab = model.arena.buffer.clone()
    lora.ensure(model, B + A)                                        # the order is part of the request (and of the sum's rounding)
    lora.ensure(model, A + B)
    assert torch.equal(model.arena.buffer, ab)
    lora.ensure(model, None)
    assert torch.equal(model.arena.buffer, orig)
    assert _guards_ok(big, total) and _guards_ok(big2, total)


def test_library_refusals_leave_the_arena_untouched(dev):
    sd = OrderedDict((k, v.cpu()) for k, v in _state(MINI, dev).items())
    model, big, total = _guarded_model(MINI, DAC_MINI, sd, torch.float16, dev)
    orig = model.arena.buffer.clone()
    ctx = model.ctx
    key = "single_blocks.0.linear1.weight"                          # [32, 32, 3]
    t = lambda *s, dt=torch.float32: torch.ones(*s, dtype=dt, device=dev)
    good = (t(2, 32, 3), t(32, 2, 1), 1.0)
    with pytest.raises(rt.FoleyRuntimeError, match="foley_lora_begin has not been called"):
        ctx.lora_merge(key, [good])
    ctx.lora_begin()
    cases = [
        ("single_blocks.0.linear9.weight", [good], "unknown key"),
        ("single_blocks.5.linear1.weight", [good], "unknown key"),
        ("single_blocks.0.linear1.bias", [good], "not targetable"),
        ("single_blocks.0.q_norm.weight", [good], "not targetable"),
        ("sync_pos_emb", [good], "not targetable"),
        ("empty_clip_feat", [good], "not targetable"),
        ("decoder.model.0.weight", [good], "not targetable"),
        (key, [(t(2, 32, 2), t(32, 2, 1), 1.0)], "shape does not match"),
        (key, [(t(2, 32), t(32, 2), 1.0)], "shape does not match"),
        (key, [(t(2, 32, 3), t(31, 2, 1), 1.0)], "shape does not match"),
        (key, [(t(2, 32, 3), t(32, 2, 3), 1.0)], "kernel > 1"),
        (key, [(t(257, 32, 3), t(32, 257, 1), 1.0)], r"rank must be in \[1, 256\]"),
        (key, [(t(0, 32, 3), t(32, 0, 1), 1.0)], r"rank must be in \[1, 256\]"),
        (key, [good] * 9, "more than 8 adapters"),
        (key, [(good[0], good[1], float("nan"))], "non-finite scale"),
        (key, [(good[0], good[1], float("inf"))], "non-finite scale"),
        (key, [(t(2, 32, 3, dt=torch.float64), t(32, 2, 1, dt=torch.float64), 1.0)], "operand dtype"),
    ]
    for k, adapters, reason in cases:
        with pytest.raises(rt.FoleyRuntimeError, match=re.escape(k) + ".*" + reason):
            ctx.lora_merge(k, adapters)
    ctx.lora_end()
    assert torch.equal(model.arena.buffer, orig) and ctx.lora_backup_bytes() == 0
    ctx.lora_begin()
    ctx.lora_merge(key, [good] * 8)                                  # eight is allowed
    with pytest.raises(rt.FoleyRuntimeError, match=re.escape(key) + ".*merged twice"):
        ctx.lora_merge(key, [good])
    ctx.lora_end()
    assert not torch.equal(model.arena.buffer, orig)
    ctx.lora_clear()
    assert torch.equal(model.arena.buffer, orig) and _guards_ok(big, total)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_both_load_paths_give_the_same_bytes(dev, cdt):
    sd = OrderedDict((k, v.cpu()) for k, v in _state(MINI, dev).items())
    dsd = OrderedDict((k, v.cpu()) for k, v in _dac_state(DAC_MINI, dev).items())
    a = sampler.FoleyModel(MINI, sd, cdt, dev, dac_cfg=DAC_MINI)
    b = sampler.FoleyModel.from_reference_state(MINI, sd, cdt, dev, dsd, dac_cfg=DAC_MINI)
    specs = _mini_specs()
    lora.ensure(a, specs)
    lora.ensure(b, specs)
    changed = 0
    for name, t in a.arena.items():
        if not name.endswith(".w"):
            continue
        assert torch.equal(W.bits(t), W.bits(b.ctx.weights_slot_tensor(name))), name
        changed += 1
    assert changed > 20


# ----------------------------------------------------------------------------- the loop sees the new weights
def _tiny_adapter(seed=9):
    sh = _shapes(C.TINY)
    keys = {"triple_blocks.0.audio_self_attn_qkv.weight": 4, "triple_blocks.1.audio_mlp.fc2.weight": 8, "single_blocks.0.linear_qkv.weight": 4,
            "single_blocks.1.linear2.w1.weight": 8, "single_blocks.1.linear2.w2.weight": 4, "single_blocks.0.modulation.linear.weight": 2,
            "final_layer.linear.weight": 4, "audio_embedder.proj.weight": 2}
    return LR.spell(LR.make_adapter(sh, keys, torch.float32, seed=seed, amp=0.05), "peft", "transformer.")


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_loop_runs_on_the_merged_weights(dev, cdt):
    cfg, dcfg, steps, guid = C.TINY, C.DAC_TINY, 10, 4.5
    sd = synth.synth_dit_state_dict(cfg)
    cond = synth.synth_conditioning(cfg, 1.0, t2a=False, sd=sd)
    model = sampler.FoleyModel(cfg, sd, cdt, dev, dac_cfg=dcfg)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(dcfg), dev, dcfg)
    noise = torch.randn(1, cfg.latent_dim, 50, generator=torch.Generator().manual_seed(77))

    def run(m):
        _audio, _sr, lat = sampler.denoise_process_with_generator(
            {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}, {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]},
            1.0, m, dac, guid, steps, 1, "euler", noise=noise, use_graph=True, return_latents=True)
        return lat.clone()

    plain = run(model)
    assert torch.equal(run(model), plain)
    adapter = _tiny_adapter()
    assert lora.ensure(model, [(adapter, 1.0)]) is True
    merged = run(model)
    assert not torch.equal(merged, plain) and bool(torch.isfinite(merged).all())
    twin_arena = packers.Arena(model.arena.buffer.numel(), model.arena.table, dev, buffer=model.arena.buffer.clone())
    twin = sampler.FoleyModel.from_arena(cfg, twin_arena, cdt, dev, dac_cfg=dcfg)
    assert torch.equal(run(twin), merged)                     # prepared tables and the captured graph follow the weights
    if cdt == torch.float32:                                  # the merged forward is the oracle's on the fp64-merged state dict
        plan = lora.plan_merge([(adapter, 1.0)], cfg)
        ref64, _mag = LR.merge64(sd, plan)
        sd_m = OrderedDict(sd)
        sd_m.update((k, v.to(torch.float32)) for k, v in ref64.items())
        with torch.inference_mode():
            ref = O.sample_latents(sd_m, cfg.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"], steps, guid, "euler")
            ref_plain = O.sample_latents(sd, cfg.heads, noise, cond["text"], cond["uncond_text"], cond["clip"], cond["sync"], steps, guid, "euler")
        e, e0, moved = oc_rel(merged, ref), oc_rel(plain, ref_plain), oc_rel(ref, ref_plain)
        print(f"fp32 loop vs oracle: merged {e:.2e}, plain {e0:.2e}; the adapter moves the result by {moved:.2e}")
        assert e < 1e-4 and moved > 1e-3                      # test_model_gpu.py::test_sampler_golden's latent gate for this configuration;
                                                              # the adapter moves the result by far more than the gate
    assert lora.ensure(model, None) is True
    assert torch.equal(run(model), plain)


def oc_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ----------------------------------------------------------------------------- the node
def test_node_takes_loras(dev, caplog, monkeypatch):
    sd = synth.synth_dit_state_dict(C.TINY)
    model = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    deps = nodes.AttributeDict(dac_model=sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY))
    cond = synth.synth_conditioning(C.TINY, 1.0, t2a=True, sd=sd)
    feats = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"], "text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    kw = dict(frame_rate=16, duration=1.0, prompt="x", negative_prompt="y", cfg_scale=4.5, steps=10, sampler="euler", batch_size=1,
              seed=5, force_offload=True)
    node = nodes.HunyuanFoleySampler()
    plain = node.generate_audio(model, deps, **kw, features=feats)[1]["waveform"]
    assert not lora.merged(model)
    adapter = _tiny_adapter()
    with caplog.at_level(logging.INFO):
        first = node.generate_audio(model, deps, **kw, features=feats, loras=[(adapter, 0.5)])[1]["waveform"]
    assert any("LoRA: merged 1 adapter" in r.getMessage() for r in caplog.records)
    assert lora.merged(model) and not torch.equal(first, plain) and len(nodes.NODE_CLASS_MAPPINGS) == 6
    again = node.generate_audio(model, deps, **kw, features=feats, loras=[(adapter, 0.5)])[1]["waveform"]
    assert torch.equal(again, first)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        back = node.generate_audio(model, deps, **kw, features=feats)[1]["waveform"]          # unset on a model that carries a set
    assert any("restored the loaded weights" in r.getMessage() for r in caplog.records)
    assert torch.equal(back, plain) and not lora.merged(model)
    calls = []

    def encoder_stub(*a, **k):
        calls.append(a)
        raise RuntimeError("the encoder ran")
    monkeypatch.setattr(nodes, "encode_text_feat", encoder_stub)
    bad = OrderedDict(adapter)
    bad["transformer.final_layer.linear.dora_scale"] = torch.ones(1)
    with pytest.raises(lora.LoraError, match="dora_scale"):
        node.generate_audio(model, deps, **kw, loras=[(bad, 1.0)])                            # text-to-audio: would call the encoder
    with pytest.raises(FileNotFoundError, match="no_such_style.safetensors"):
        node.generate_audio(model, deps, **kw, loras=[("no_such_style.safetensors", 1.0)])
    assert calls == [] and not lora.merged(model)
