"""The one CPU restatement of the sampling loop, every sampler option a keyword: guidance controls (separate video / text scales,
schedule, CFG rescale), multistep (Adams-Bashforth) weights, an edit, overlapping windows, the step cache.  The reference project
has none of them, so the definition lives here, over O.dit_forward / O.SolverState / O.flow_sigmas / O.flow_timesteps in fp32 as
the oracle's sampler; with every option unset it is O.sample_latents.  timeline_ref.timed_text runs it with timed text."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from foley_amd.host import step_cache as S, tables
from oracle import foley_oracle as O

Loop = namedtuple("Loop", "x windows info")     # latents (stitched in a windowed run), the windows' final states, the cache's record


# ----------------------------------------------------------------------------- guidance
def schedule_ref(n_iter, g_video, g_text, interval=None):
    """[n_iter][2] Python floats: (g_video, g_text) on the iterations with start <= i / n_iter < end, (1, 1) on the others."""
    rows = []
    for i in range(n_iter):
        inside = interval is None or interval[0] <= i / n_iter < interval[1]
        rows.append((float(g_video), float(g_text)) if inside else (1.0, 1.0))
    return rows


def rescale_factor64(v, p_last, phi):
    """[B, 1, 1] fp64: phi s_pos / s_cfg + (1 - phi) per batch clip over its C x L elements, 1 where s_cfg is 0."""
    v, p = v.double().flatten(1), p_last.double().flatten(1)
    s_cfg, s_pos = v.std(1, unbiased=False), p.std(1, unbiased=False)
    f = torch.where(s_cfg > 0, phi * s_pos / s_cfg.clamp_min(1e-300) + (1.0 - phi), torch.ones_like(s_cfg))
    return f.view(-1, 1, 1)


# ----------------------------------------------------------------------------- multistep
def weight_rows(sigmas, order, start=0, n=None):
    """[(c_0, c_1, c_2)] as fp32 tensors' entries: the rows of tables.solver_table(multistep_order=order, start=start)[start:]."""
    n = len(sigmas) - 1 if n is None else n
    t = tables.solver_table(sigmas, "euler", n, multistep_order=order, start=start)[start:]
    return [(t[i, 0], t[i, 6], t[i, 7]) for i in range(t.shape[0])]


# ----------------------------------------------------------------------------- windows
def stitch(x, plan):
    """x [variations*n_win, C, La] -> [variations, C, Ltot]: the weighted mean per global frame, in window order (fp32)."""
    V = x.shape[0] // plan.n_win
    out = torch.zeros(V, x.shape[1], plan.Ltot, dtype=torch.float32)
    for v in range(V):
        for k, s in enumerate(plan.starts):
            out[v, :, s:s + plan.La] += plan.weights[k] * x[plan.clip_index(v, k)]
    return out


def _slices(g, plan):
    return torch.stack([g[v, :, s:s + plan.La] for v in range(g.shape[0]) for s in plan.starts])


# ----------------------------------------------------------------------------- step cache
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


def margin(info, threshold):
    """Closest approach |acc - threshold| / threshold over the iterations the threshold decided (not 0, not the last one)."""
    acc = info["acc"][1:-1]
    return min(abs(a - threshold) / threshold for a in acc)


# ----------------------------------------------------------------------------- the loop
def restated_loop(sd, heads, noise, text, uncond_text, clip, sync, steps, g_text, solver="euler", *, g_video=None, interval=None,
                  rescale=0.0, order=None, weights=None, edit=None, windows=None, cache=None, shift=1.0, text_len=77):
    """noise [bs, 128, La] ([variations, 128, Ltot] with windows); text / uncond_text / clip / sync with batch 1 (shared), one row
    per batch clip, or - windows - n_win rows, clip v*n_win + k reading row k.  Returns Loop(x, windows, info).

    Halves      g_video given: three - h0 negative prompt + the learned empty rows, h1 negative prompt + the visual features, h2
                prompt + the features - and v = p0 + g_video (p1 - p0) + g_text (p2 - p1).  Otherwise [uncond ; cond] and
                v = u + g_text (c - u) when g_text > 1, else the one conditional half (O.sample_latents' rule).  interval: the
                scales hold on the iterations of schedule_ref, (1, 1) on the others, indexed by the iteration of the FULL run.
                rescale: v times rescale_factor64 (fp64 statistics against the last half).
    Step        O.SolverState.step; with order / weights (euler) deriv = c_0 v (+ c_1 v_{n-1}) (+ c_2 v_{n-2}) in fp32, left to right,
                c_0 == 1 taking v itself and a zero weight skipped, then x + deriv * (sigma_{n+1} - sigma_n); the guided velocity,
                rescale included, enters the history.  weights: [(c_0, c_1, c_2)] per iteration run (default weight_rows(order)).
    edit        (x0, mask, strength), mask [La] or [clips, La] or None (all ones): the iterations [i0, steps) from
                sigma_{k0} noise + (1 - sigma_{k0}) x0 with (k0, i0) = tables.edit_start, the multistep warm-up restarting at i0; after
                every iteration that advances the sigma index to k, x <- m x + (1 - m) (sigma_k noise + (1 - sigma_k) x0).
    windows     a long_form.WindowPlan: the batch is the variations*n_win windows of the noise; after every iteration that advances
                the sigma index every global frame is replaced in all the windows that cover it by stitch's weighted mean.
    cache       a StepCacheSpec: per iteration the head call (no blocks), m = first_block_input64, rel = max rel64 against the
                previous iteration, StepCachePolicy.decide; a skipped iteration predicts final_layer(LayerNorm(audio_in + delta)) with
                the last full iteration's delta = stream after the last block - audio_in, and runs the unchanged combine and step.
                info = {"rel", "skipped", "acc"} per iteration run (rel -1.0 where nothing was measured, acc in threshold mode)."""
    if windows is not None and edit is not None:
        raise ValueError("windows cannot be combined with an edit")
    sig = O.flow_sigmas(steps, shift)
    ts = O.flow_timesteps(sig)
    st = O.SolverState(sig, solver)
    noise = noise.float()
    n_win = windows.n_win if windows is not None else 1
    x, i0 = (_slices(noise, windows) if n_win > 1 else noise), 0
    if edit is not None:
        x0, mask, strength = edit
        st.idx, i0 = tables.edit_start(steps, solver, strength)
        La = noise.shape[2]
        m = torch.ones(1, 1, La) if mask is None else (mask.view(1, 1, La) if mask.dim() == 1 else mask.view(-1, 1, La))
        x0 = x0.float()
        x = sig[st.idx] * noise + (1 - sig[st.idx]) * x0
    bs = x.shape[0]

    def rows(a):
        assert a.shape[0] in (1, n_win, bs), (a.shape[0], n_win, bs)
        return a.repeat(bs // a.shape[0], 1, 1)
    text_r, unc_r = O.pad_or_trim_text(rows(text), text_len), O.pad_or_trim_text(rows(uncond_text), text_len)
    clip_r, sync_r = rows(clip), rows(sync)
    e_clip = sd["empty_clip_feat"].unsqueeze(0).expand(bs, clip.shape[1], -1)
    e_sync = sd["empty_sync_feat"].unsqueeze(0).expand(bs, sync.shape[1], -1)
    n_half = 3 if g_video is not None else 2 if g_text > 1.0 else 1
    if n_half == 3:
        text_in, clip_in, sync_in = torch.cat([unc_r, unc_r, text_r]), torch.cat([e_clip, clip_r, clip_r]), torch.cat([e_sync, sync_r, sync_r])
    elif n_half == 2:
        text_in, clip_in, sync_in = torch.cat([unc_r, text_r]), torch.cat([e_clip, clip_r]), torch.cat([e_sync, sync_r])
    else:
        assert interval is None and rescale == 0.0, "one half has nothing to schedule or rescale"
        text_in, clip_in, sync_in = text_r, clip_r, sync_r
    sched = schedule_ref(steps, g_video if n_half == 3 else g_text, g_text, interval)
    multistep = order is not None or weights is not None
    if multistep:
        assert solver == "euler"
        weights, hist = weight_rows(sig, order, i0) if weights is None else weights, []
    policy = S.StepCachePolicy.from_spec(cache, steps, i0) if cache is not None else None
    nt, ns = depths(sd)
    last = "single%d" % (ns - 1) if ns > 0 else "triple%d" % (nt - 1)
    m_prev, delta = None, None
    info = {"rel": [], "skipped": [], "acc": []}
    for i in range(i0, steps):
        xin = torch.cat([x] * n_half) if n_half > 1 else x
        tt = ts[i].expand(xin.shape[0])
        skip, rel = False, -1.0
        if policy is not None:
            head = {}
            O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, n_triple=0, n_single=0, taps=head)
            mi = first_block_input64(sd, head)
            if m_prev is not None:
                rel = float(rel64(mi, m_prev).max())
            m_prev = mi
            skip = policy.decide(i - i0, rel)
            info["acc"].append(policy.last_acc)
        info["rel"].append(rel)
        info["skipped"].append(int(skip))
        if skip:
            xs = head["audio_in"] + delta
            p = F.linear(O.layer_norm(xs, 1e-6), sd["final_layer.linear.weight"], sd["final_layer.linear.bias"]).transpose(1, 2)
        else:
            taps = {} if policy is not None else None
            p = O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, taps=taps)
            if policy is not None:
                delta = taps[last] - taps["audio_in"]
        p = p.chunk(n_half)
        gv, gt = sched[i]
        v = p[0] if n_half == 1 else p[0] + gv * (p[1] - p[0]) + gt * (p[2] - p[1]) if n_half == 3 else p[0] + gv * (p[1] - p[0])
        if rescale > 0.0:
            v = (rescale_factor64(v, p[-1], rescale) * v.double()).float()
        k = st.idx
        if multistep:
            c0, c1, c2 = weights[i - i0]
            deriv = v if float(c0) == 1.0 else c0 * v
            if float(c1) != 0.0:
                deriv = deriv + c1 * hist[-1]
            if float(c2) != 0.0:
                deriv = deriv + c2 * hist[-2]
            x = x + deriv * (sig[i + 1] - sig[i])
            hist.append(v)
            st.idx += 1
        else:
            x = st.step(v, x)
        if st.idx != k and edit is not None:
            s = sig[st.idx]
            x = m * x + (1 - m) * (s * noise + (1 - s) * x0)
        if st.idx != k and n_win > 1:
            x = _slices(stitch(x, windows), windows)
    return Loop(stitch(x, windows) if n_win > 1 else x, x, info)
