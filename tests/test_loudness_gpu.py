"""The loudness stage through the sampler node: C.TINY / C.DAC_TINY, fp32, 1 s, two clips, 10 euler steps.  The plain run's
waveform is measured by the fp64 restatement (tests/loudness_ref.py); the node's normalised output must be that waveform times one
fp32 gain per clip, bit for bit, and land on the target."""
import math

import numpy as np
import pytest
import torch

from foley_amd import nodes
from foley_amd.host import config as C, loudness as L, runtime as rt, sampler, synth
import loudness_ref as LR
from test_loudness_ops_gpu import _energy_cases, _lufs_tol

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
_RUN = {}


def _node_run(dev, **extra):
    if "model" not in _RUN:
        sd = synth.synth_dit_state_dict(C.TINY)
        _RUN["model"] = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
        _RUN["deps"] = nodes.AttributeDict(dac_model=sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC_TINY), dev, C.DAC_TINY))
        cond = synth.synth_conditioning(C.TINY, 1.0, t2a=True, sd=sd)
        _RUN["feats"] = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"], "text_feat": cond["text"],
                         "uncond_text_feat": cond["uncond_text"]}
    kw = dict(frame_rate=16, duration=1.0, prompt="x", negative_prompt="y", cfg_scale=4.5, steps=10, sampler="euler", batch_size=2,
              seed=55574, force_offload=True, features=_RUN["feats"])
    _first, batch = nodes.HunyuanFoleySampler().generate_audio(_RUN["model"], _RUN["deps"], **kw, **extra)
    return batch["waveform"]


def _plain(dev):
    """The plain run and the oracle's reading of it, once: (waveform [2, 1, 48000] on the CPU, [(lufs, tp, tp_bound)] per clip)."""
    if "plain" not in _RUN:
        wave = _node_run(dev)
        read = []
        for b in range(wave.shape[0]):
            x = wave[b].numpy()
            p, bound = LR.envelope(x)
            i = int(p.argmax())
            read.append((LR.integrated_loudness(x), float(p[i]), float(bound.max())))
        _RUN["plain"] = (wave, read)
        print("plain run:", [(round(l, 3), round(LR.db(tp), 3)) for l, tp, _ in read], "(LUFS, dBTP)")
    return _RUN["plain"]


def _f32_between(lo, hi):
    """Every fp32 value in [fl32(lo), fl32(hi)]."""
    v, end, out = np.float32(lo), np.float32(hi), []
    while v <= end:
        out.append(v)
        v = np.nextafter(v, np.float32(np.inf))
    return out


def _gain_candidates(lufs, tp, tp_bound, target, ceiling, limiter, floor):
    """The fp32 gains the contract allows for a clip the oracle reads at (lufs, tp +/- tp_bound): G_dB = target - L, in gain-only
    mode held under ceiling - TP; L within the energy gate carried through the logarithm, TP within the envelope's fp32 bound."""
    tol = _lufs_tol(floor, lufs)
    lo, hi = target - (lufs + tol), target - (lufs - tol)
    if not limiter:
        lo, hi = min(lo, ceiling - LR.db(tp + tp_bound)), min(hi, ceiling - LR.db(tp - tp_bound))
    return _f32_between(10.0 ** (lo / 20.0) * (1 - 2.0 ** -50), 10.0 ** (hi / 20.0) * (1 + 2.0 ** -50)), (lo, hi)


def test_defaults_are_the_plain_run(dev):
    wave, read = _plain(dev)
    assert tuple(wave.shape) == (2, 1, 48000) and all(math.isfinite(l) for l, _tp, _b in read)       # no silent clip: nothing scaled
    again = _node_run(dev, loudness_lufs=None, true_peak_dbtp=-1.0, peak_limiter=False)
    assert torch.equal(again, wave)


def test_node_normalises_each_clip_to_the_target(dev):
    _c, _s, floor = _energy_cases()
    wave, read = _plain(dev)
    out = _node_run(dev, loudness_lufs=-20.0)
    assert out.dtype == torch.float32 and out.device.type == "cpu" and out.shape == wave.shape
    for b, (lufs, tp, tp_bound) in enumerate(read):
        cands, (lo, hi) = _gain_candidates(lufs, tp, tp_bound, -20.0, -1.0, False, floor)
        hits = [g for g in cands if torch.equal(out[b], wave[b] * torch.tensor(g))]
        print(f"clip {b}: {lufs:.4f} LUFS, {LR.db(tp):.3f} dBTP, gain in [{lo:.6f}, {hi:.6f}] dB, {len(cands)} fp32 candidate(s), {len(hits)} match")
        assert len(cands) <= 64 and len(hits) == 1                              # the plain waveform times ONE fp32 gain, bit for bit
        got = LR.integrated_loudness(out[b].numpy())
        if -20.0 - lufs <= -1.0 - LR.db(tp + tp_bound):                         # the target decided the gain
            assert abs(got - (-20.0)) <= 2 * _lufs_tol(floor, lufs) + 40 * math.log10(1 + U32)
        else:                                                                   # the ceiling did: the true peak reads it
            tp_out = LR.db(LR.true_peak(out[b].numpy()))
            assert abs(tp_out - (-1.0)) <= 20 * math.log10((tp + tp_bound) / (tp - tp_bound)) + 40 * math.log10(1 + U32)


def test_node_limiter_holds_the_ceiling(dev):
    wave, read = _plain(dev)
    # a target that asks every clip for at least 6 dB more than the ceiling allows (and no more than 0 LUFS)
    target = max(l + (-1.0 - LR.db(tp)) + 6.0 for l, tp, _b in read)
    assert target <= 0.0, target
    out = _node_run(dev, loudness_lufs=target, true_peak_dbtp=-1.0, peak_limiter=True)
    # the same stage, op by op, on the plain waveform: the node's output is its output, and its gain curve can be examined
    xd = wave.to(dev)
    m = L.measure(xd, 48000)
    g_db, gain = L.static_gain(m.lufs, m.true_peak_dbtp, target, -1.0, True)
    taps = L.true_peak_taps().to(torch.float32)
    c = 10.0 ** (-1.0 / 20.0)
    W = L.lookahead_samples(5.0)
    y, g = rt.op_loudness_apply(xd, gain.to(dev), limiter=True, ceiling=c, lookahead=W, taps=taps, with_gain_curve=True)
    assert torch.equal(y.cpu(), out)
    _tp, _sp, env = rt.op_true_peak(xd, taps, with_envelope=True)
    for b in range(2):
        assert float(m.true_peak_dbtp[b]) + float(g_db[b]) > -1.0               # the ceiling binds
        G = float(gain[b])
        g_h, p_d = g[b].cpu().numpy().astype(np.float64), env[b].cpu().numpy().astype(np.float64)
        r_d = LR.reduction(p_d, G, c)
        free = LR.untouched(r_d, W)
        print(f"clip {b}: gain {float(g_db[b]):.2f} dB, min g {g_h.min():.4f}, {int((r_d < 1).sum())} samples over, {int(free.sum())} untouched")
        assert (r_d < 1).any()
        assert (g_h <= r_d).all()
        assert (G * g_h * p_d <= c * (1 + 2.0 ** -50)).all()
        assert (g_h[free] == 1.0).all()
        ft = torch.from_numpy(free)
        assert torch.equal(out[b][:, ft], (wave[b] * torch.tensor(np.float32(G)))[:, ft])
