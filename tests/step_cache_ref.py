"""Reference of the step cache (host/step_cache.py, foley_set_step_cache) - the reference project has no such thing, so the
definition lives here: the sampling loop of tests/guidance_ref.py restated with the cached iteration, over O.dit_forward.

For one model call: a0 = the audio stream after audio_embedder + add_sync (taps["audio_in"]), aN = the stream after the last block
(taps["single{n-1}"]), m = the first block's modulated audio input LayerNorm(a0) * (1 + scale) + shift in fp64 from the fp32
operands.  A full iteration keeps delta = aN - a0; a skipped one predicts F.linear(LayerNorm(a0 + delta; 1e-6), final) and runs
the unchanged combine and solver step.  rel = max over the batch rows of sum|m - m_prev| / sum|m_prev|; the decisions come from
host/step_cache.StepCachePolicy."""
import torch
import torch.nn.functional as F

import guidance_ref as G
from foley_amd.host import step_cache as S
from oracle import foley_oracle as O


def depths(sd):
    nt = 1 + max((int(k.split(".")[1]) for k in sd if k.startswith("triple_blocks.")), default=-1)
    ns = 1 + max((int(k.split(".")[1]) for k in sd if k.startswith("single_blocks.")), default=-1)
    return nt, ns


def first_block_input64(sd, taps):
    """m [B, La, D] fp64 of the model call whose taps (audio_in, vec) are given, for a model with two-stream blocks: block 0's
    audio_mod chunks 0 (shift) / 1 (scale), eps 1e-6.  (A model of single blocks only takes single block 0's modulation rows at eps
    1e-5; this reference does not cover it - the probe's up-sampled per-token operands are checked at op level.)"""
    a0, vec = taps["audio_in"], taps["vec"]
    assert depths(sd)[0] > 0, "the restated loop covers models with two-stream blocks"
    am = F.linear(F.silu(vec), sd["triple_blocks.0.audio_mod.linear.weight"], sd["triple_blocks.0.audio_mod.linear.bias"]).chunk(9, dim=-1)
    shift, scale, eps = am[0][:, None], am[1][:, None], 1e-6
    x = a0.double()
    d = x - x.mean(-1, keepdim=True)
    xhat = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    return xhat * (1 + scale.double()) + shift.double()


def rel64(m, m_prev):
    """[B] fp64: sum|m - m_prev| / sum|m_prev| per batch row, 0 where the denominator is 0."""
    num, den = (m - m_prev).abs().flatten(1).sum(1), m_prev.abs().flatten(1).sum(1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(den))


def cached_loop(sd, heads, noise, text, uncond_text, clip, sync, steps, g_text, solver="euler", spec=None, g_video=None,
                interval=None, rescale=0.0, text_len=77, shift=1.0):
    """guidance_ref.restated_loop under a StepCacheSpec (None: every iteration full).  Conditioning with batch 1 (shared) or bs
    (per clip).  Returns (x, info) with info = {"rel": [...], "skipped": [...], "acc": [...]}: per iteration the measured change
    (-1.0 at iteration 0), the decision, and the accumulator the decision compared with the threshold (threshold mode)."""
    assert depths(sd)[0] > 0, "the restated loop covers models with two-stream blocks"
    bs = noise.shape[0]
    sig = O.flow_sigmas(steps, shift)
    ts = O.flow_timesteps(sig)
    st = O.SolverState(sig, solver)
    rep = lambda a: a if a.shape[0] == bs else a.repeat(bs, 1, 1)
    text_r, unc_r = O.pad_or_trim_text(rep(text), text_len), O.pad_or_trim_text(rep(uncond_text), text_len)
    clip_r, sync_r = rep(clip), rep(sync)
    e_clip = sd["empty_clip_feat"].unsqueeze(0).expand(bs, clip.shape[1], -1)
    e_sync = sd["empty_sync_feat"].unsqueeze(0).expand(bs, sync.shape[1], -1)
    three = g_video is not None
    if three:
        text_in, clip_in, sync_in = torch.cat([unc_r, unc_r, text_r]), torch.cat([e_clip, clip_r, clip_r]), torch.cat([e_sync, sync_r, sync_r])
    else:
        text_in, clip_in, sync_in = torch.cat([unc_r, text_r]), torch.cat([e_clip, clip_r]), torch.cat([e_sync, sync_r])
    n_half = 3 if three else 2
    n = len(ts)
    sched = G.schedule_ref(n, g_video if three else g_text, g_text, interval)
    policy = S.StepCachePolicy.from_spec(spec, n) if spec is not None else None
    _nt, ns = depths(sd)
    last = "single%d" % (ns - 1) if ns > 0 else "triple%d" % (_nt - 1)
    x = noise.float()
    m_prev, delta = None, None
    info = {"rel": [], "skipped": [], "acc": []}
    for i, t in enumerate(ts):
        xin = torch.cat([x] * n_half)
        tt = t.expand(xin.shape[0])
        skip, rel = False, -1.0
        if policy is not None:
            head = {}
            O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, n_triple=0, n_single=0, taps=head)
            m = first_block_input64(sd, head)
            if m_prev is not None:
                rel = float(rel64(m, m_prev).max())
            m_prev = m
            skip = policy.decide(i, rel)
            info["acc"].append(policy.last_acc)
        info["rel"].append(rel)
        info["skipped"].append(int(skip))
        if skip:
            xs = head["audio_in"] + delta
            p = F.linear(O.layer_norm(xs, 1e-6), sd["final_layer.linear.weight"], sd["final_layer.linear.bias"]).transpose(1, 2)
        else:
            taps = {}
            p = O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, taps=taps)
            delta = taps[last] - taps["audio_in"]
        p = p.chunk(n_half)
        gv, gt = sched[i]
        v = p[0] + gv * (p[1] - p[0]) + gt * (p[2] - p[1]) if three else p[0] + gv * (p[1] - p[0])
        if rescale > 0.0:
            v = (G.rescale_factor64(v, p[-1], rescale) * v.double()).float()
        x = st.step(v, x)
    return x, info


def margin(info, threshold):
    """Closest approach |acc - threshold| / threshold over the iterations the threshold decided (not 0, not the last one)."""
    acc = info["acc"][1:-1]
    return min(abs(a - threshold) / threshold for a in acc)
