"""References of the guidance controls (separate video / text scales, schedules, CFG rescale) - the reference project has none
of them, so the definition lives here.

restated_loop   the sampling loop of oracle.sample_latents restated over two or three prediction halves with a per-iteration
                schedule and the rescale factor (fp64 statistics), over O.dit_forward / O.SolverState / O.flow_sigmas.
factor_ref      fp64 rescale factors and their bound, over opcheck.combine_ref (the guided value and its bound; the solver
                update behind it is opcheck.step_ref_and_bounds).
"""
import torch

import opcheck as oc
from opcheck import U32
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- the loop
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


def restated_loop(sd, heads, noise, text, uncond_text, clip, sync, steps, g_text, solver="euler", g_video=None, interval=None,
                  rescale=0.0, text_len=77, shift=1.0):
    """noise [bs, 128, La]; text / uncond_text / clip / sync with batch 1 (shared) or bs.  g_video None: two halves
    [uncond ; cond] and v = u + g (c - u) with g = g_text; otherwise three halves - h0 negative prompt + the learned empty rows,
    h1 negative prompt + the visual features, h2 prompt + the features - and v = p0 + g_video (p1 - p0) + g_text (p2 - p1)."""
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
    sched = schedule_ref(len(ts), g_video if three else g_text, g_text, interval)
    x = noise.float()
    for i, t in enumerate(ts):
        xin = torch.cat([x] * n_half)
        p = O.dit_forward(sd, heads, xin, t.expand(xin.shape[0]), text_in, clip_in, sync_in).chunk(n_half)
        gv, gt = sched[i]
        v = p[0] + gv * (p[1] - p[0]) + gt * (p[2] - p[1]) if three else p[0] + gv * (p[1] - p[0])
        if rescale > 0.0:
            v = (rescale_factor64(v, p[-1], rescale) * v.double()).float()
        x = st.step(v, x)
    return x


# ----------------------------------------------------------------------------- the factor
def _m2_and_bound(x, e_x):
    """x [clips, n] fp64, e_x its per-element bound -> (M2 = sum (x - mean)^2, bound) for an fp32 evaluation that centres every
    partial sum on a computed mean and adds in ANY order:
        (n + 8) U32 M2                      n additions of non-negative squares in any order, each square with the roundings of
                                            its difference, its product and the merge terms
        2 d sqrt(n M2) + n d^2              a centre off the true mean by d leaves the cross term 2 (c - mean) sum (x - c); a
                                            computed mean of any order is within d = U32 sum|x| of the exact one
        2 sqrt(M2 sum e^2) + sum e^2        the elements themselves carry e (the combine's roundings)."""
    n = x.shape[1]
    m2 = ((x - x.mean(1, keepdim=True)) ** 2).sum(1)
    d = U32 * x.abs().sum(1)
    se = (e_x ** 2).sum(1)
    return m2, (n + 8) * U32 * m2 + 2 * d * (n * m2).sqrt() + n * d * d + 2 * (m2 * se).sqrt() + se


def factor_ref(pred, clips, L, ncfg, gv, gt, phi, keep=None):
    """(f [clips] fp64, bound [clips]) of the rescale factor from pred [ncfg clips L, C]; keep [clips, C, L] bool (or None)
    limits the statistics to those elements - what a kernel that loses the others would compute.
    f = phi sqrt(M2_p / M2_v) + (1 - phi); with relative bounds r_p, r_v of the two sums the ratio of the deviations moves by at
    most (r_p + r_v) / (2 (1 - r_v)) relatively; division, square root, product and sum add 4 U32 of |phi ratio| + |1 - phi|."""
    v, e_v = oc.combine_ref(pred, clips, L, ncfg, gv, gt)
    p = pred.double().cpu().view(ncfg, clips, L, -1).transpose(2, 3)[ncfg - 1]
    if keep is not None:
        sel = lambda t: torch.stack([t[b][keep[b]] for b in range(clips)])     # the same count in every clip
        v, e_v, p = sel(v), sel(e_v), sel(p)
    else:
        v, e_v, p = v.flatten(1), e_v.flatten(1), p.flatten(1)
    m2v, bv = _m2_and_bound(v, e_v)
    m2p, bp = _m2_and_bound(p, torch.zeros_like(p))
    ok = m2v > 0
    ratio = torch.where(ok, (m2p / m2v.clamp_min(1e-300)).sqrt(), torch.ones_like(m2v))
    phi = oc.f32(phi)
    f = torch.where(ok, phi * ratio + (1.0 - phi), torch.ones_like(ratio))
    r_v, r_p = bv / m2v.clamp_min(1e-300), bp / m2p.clamp_min(1e-300)
    bound = phi * ratio * 0.5 * (r_p + r_v) / (1 - r_v).clamp_min(0.5) + 4 * U32 * (phi * ratio + abs(1.0 - phi))
    return f, torch.where(ok, bound, torch.zeros_like(bound))
