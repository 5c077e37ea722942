"""References of projected guidance (APG, CFG-Zero*; csrc/rowops.hip, foley_set_projected_guidance): the fp64 coefficients of
one iteration with the bound the kernels' documented summation chain gives, the projected velocity with its bound for
opcheck.step_ref_and_bounds, and the sampling loop restated with projection over O.dit_forward / O.SolverState (interval,
multistep history as loop_ref has it, a step-cache skip list)."""
import torch
import torch.nn.functional as F

import loop_ref as L
import opcheck as oc
from foley_amd.host import step_cache as S, tables
from oracle import foley_oracle as O

APG, ZERO_STAR = 1, 2
U = 2.0 ** -24          # unit round-off of fp32
GS_ROWS, GS_RW = 32, 8  # rows per workgroup and per wave of launch 1


def chain_length(C, La):
    """The longest chain of fp32 additions a product passes through on its way into a clip's sum, as rowops.hip documents it: a
    lane's GS_RW x JC fused accumulations (JC = 1, 2 or 4 channels per lane), wave_sum's 6 levels, the 4 waves in wave order, the
    ceil(nblk / 64) records of a lane of launch 2 and its 64 lanes in lane order."""
    jc = 1 if C <= 64 else 2 if C <= 128 else 4
    nblk = (La + GS_ROWS - 1) // GS_ROWS
    return GS_RW * jc + 6 + 4 + (nblk + 63) // 64 + 64


def halves(pred, clips, La):
    """pred [2 clips La, C] fp32 -> (u, c) [clips, La, C] fp64."""
    P = pred.double().cpu().view(2, clips, La, -1)
    return P[0], P[1]


def coef_ref(pred, clips, La, g, row, mode, m_prev=None, keep=None):
    """One iteration in fp64 from fp32 operands: g the fp32 scale, row = (eta, beta, R, live) fp32 entries, m_prev [clips, La, C]
    the plane as the device held it before the launch (read only when beta != 0), keep [clips, La, C] bool: elements left out of the
    sums (None: all in).  Returns a dict: coef [clips, 2] {a_c, a_w}, bound [clips, 2], m (APG: the new plane) and e_m (its bound:
    the difference and the fused average, one rounding each), and the sums.
    Bound: every sum S = sum_k p_k carries chain_length x 2^-24 x sum_k |p_k| (each of the chain's additions rounds a partial sum
    no larger than sum |p_k|; the products are fused into their additions), APG's sums also the error of m itself, sum e_m |c| and
    2 sum e_m |m|.  To first order they propagate through the closing arithmetic, whose own operations (a square root, a division,
    a difference, the products) add one or two relative roundings each, as written below."""
    u, c = halves(pred, clips, La)
    C = u.shape[-1]
    D = chain_length(C, La)
    eta, beta, R, live = (float(v) for v in row)
    k = torch.ones_like(u) if keep is None else keep.double()
    tot = lambda a, b: (k * a * b).flatten(1).sum(1)
    mag = lambda a, b: D * U * (k * (a * b).abs()).flatten(1).sum(1)
    out = {}
    if mode == APG:
        d = c - u
        m = d + beta * m_prev.double().cpu() if beta != 0.0 else d
        e_m = U * (d.abs() + m.abs())
        smc, scc, smm = tot(m, c), tot(c, c), tot(m, m)
        e_mc = mag(m, c) + (k * e_m * c.abs()).flatten(1).sum(1)
        e_cc = mag(c, c)
        e_mm = mag(m, m) + 2 * (k * e_m * m.abs()).flatten(1).sum(1)
        n = smm.sqrt()
        e_n = e_mm / (2 * n.clamp_min(1e-300)) + 2 * U * n
        clip = (n > R) if R > 0 else torch.zeros_like(n, dtype=torch.bool)
        r = torch.where(clip, R / n.clamp_min(1e-300), torch.ones_like(n))
        e_r = torch.where(clip, R * e_n / n.clamp_min(1e-300) ** 2 + 2 * U * r, torch.zeros_like(n))
        pos = scc > 0
        rho = torch.where(pos, smc / scc.clamp_min(1e-300), torch.zeros_like(scc))
        e_rho = torch.where(pos, e_mc / scc.clamp_min(1e-300) + smc.abs() * e_cc / scc.clamp_min(1e-300) ** 2 + 2 * U * rho.abs(),
                            torch.zeros_like(scc))
        t, q = (g - 1.0) * r, (eta - 1.0) * rho
        e_t = abs(g - 1.0) * e_r + 2 * U * t.abs()
        e_q = abs(eta - 1.0) * e_rho + 2 * U * q.abs()
        a_w, e_w = live * t, live * (e_t + U * t.abs())
        a_c = live * (1.0 + t * q)
        e_c = live * (q.abs() * e_t + t.abs() * e_q + 2 * U * (1.0 + (t * q).abs()))
        out.update(m=m, e_m=e_m, smc=smc, scc=scc, smm=smm, norm=n, r=r, rho=rho)
    elif mode == ZERO_STAR:
        scu, suu = tot(c, u), tot(u, u)
        e_cu, e_uu = mag(c, u), mag(u, u)
        pos = suu > 0
        s = torch.where(pos, scu / suu.clamp_min(1e-300), torch.zeros_like(suu))
        e_s = torch.where(pos, e_cu / suu.clamp_min(1e-300) + scu.abs() * e_uu / suu.clamp_min(1e-300) ** 2 + 2 * U * s.abs(), torch.zeros_like(suu))
        a_c = torch.full_like(s, live * g)
        e_c = torch.full_like(s, live * U * abs(g))
        a_w = live * (1.0 - g) * s
        e_w = live * (abs(1.0 - g) * e_s + 3 * U * a_w.abs())
        out.update(m=None, e_m=None, scu=scu, suu=suu, s=s)
    else:
        raise ValueError(mode)
    out["coef"], out["bound"] = torch.stack([a_c, a_w], 1), torch.stack([e_c, e_w], 1)
    return out


def projected_value(pred, clips, La, ref, mode):
    """(v, e_v) [clips, C, La] fp64 of the step's v = fma(a_c, c, rnd(a_w w)) from coef_ref's dict: the coefficients' and the
    plane's bounds propagated, plus the product and the fused sum (two roundings relative to the magnitudes that enter)."""
    u, c = halves(pred, clips, La)
    w, e_w = (ref["m"], ref["e_m"]) if mode == APG else (u, torch.zeros_like(u))
    a_c, a_w = (ref["coef"][:, j].view(-1, 1, 1) for j in (0, 1))
    e_c, e_a = (ref["bound"][:, j].view(-1, 1, 1) for j in (0, 1))
    v = a_c * c + a_w * w
    e = c.abs() * e_c + w.abs() * e_a + a_w.abs() * e_w + 2 * oc.U32 * ((a_c * c).abs() + (a_w * w).abs())
    return v.transpose(1, 2).contiguous(), e.transpose(1, 2).contiguous()


def cfg_value64(u, c, g):
    return u + g * (c - u)


# ----------------------------------------------------------------------------- the loop
def restated_loop(sd, heads, noise, text, uncond_text, clip, sync, steps, g, solver="euler", *, mode, eta=0.0, momentum=-0.5,
                  norm_threshold=0.0, zero_init=0, interval=None, order=None, cache=None, shift=1.0, text_len=77, norms=None):
    """The two-half sampling loop with projected guidance: O.dit_forward for [uncond ; cond], the per-clip statistics in fp64 from
    the fp32 predictions, v = a_c c + a_w w rounded to fp32 once, then O.SolverState.step - or, with `order`, the Adams-Bashforth
    history of loop_ref (the projected v enters it).  The rows are tables.projection_rows' meaning restated: beta = 0 on the first
    iteration, `momentum` after; live = 0 on the iterations i < zero_init.  interval: g on the iterations of L.schedule_ref, 1 on
    the others.  cache: a StepCacheSpec with a skip list - a skipped iteration predicts from the last full iteration's residual as
    loop_ref does and runs the unchanged statistics, combine and step.  norms: a list that receives every iteration's |m| per clip
    (APG).  noise [bs, 128, La]; the conditionings have batch 1 or bs.  Returns the latents."""
    sig = O.flow_sigmas(steps, shift)
    ts = O.flow_timesteps(sig)
    st = O.SolverState(sig, solver)
    x = noise.float()
    bs = x.shape[0]
    rows = lambda a: a.repeat(bs // a.shape[0], 1, 1)
    text_r, unc_r = O.pad_or_trim_text(rows(text), text_len), O.pad_or_trim_text(rows(uncond_text), text_len)
    clip_r, sync_r = rows(clip), rows(sync)
    e_clip = sd["empty_clip_feat"].unsqueeze(0).expand(bs, clip.shape[1], -1)
    e_sync = sd["empty_sync_feat"].unsqueeze(0).expand(bs, sync.shape[1], -1)
    text_in, clip_in, sync_in = torch.cat([unc_r, text_r]), torch.cat([e_clip, clip_r]), torch.cat([e_sync, sync_r])
    sched = L.schedule_ref(steps, g, g, interval)
    if order is not None:
        assert solver == "euler"
        weights, hist = L.weight_rows(sig, order, 0), []
    policy = S.StepCachePolicy.from_spec(cache, steps, 0) if cache is not None else None
    nt, ns = L.depths(sd)
    last = "single%d" % (ns - 1) if ns > 0 else "triple%d" % (nt - 1)
    delta, m = None, None
    dot = lambda a, b: (a * b).flatten(1).sum(1).view(-1, 1, 1)
    for i in range(steps):
        xin = torch.cat([x, x])
        tt = ts[i].expand(xin.shape[0])
        skip = False
        if policy is not None:
            head = {}
            O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, n_triple=0, n_single=0, taps=head)
            skip = policy.decide(i, -1.0)
        if skip:
            xs = head["audio_in"] + delta
            p = F.linear(O.layer_norm(xs, 1e-6), sd["final_layer.linear.weight"], sd["final_layer.linear.bias"]).transpose(1, 2)
        else:
            taps = {} if policy is not None else None
            p = O.dit_forward(sd, heads, xin, tt, text_in, clip_in, sync_in, taps=taps)
            if policy is not None:
                delta = taps[last] - taps["audio_in"]
        u, c = (h.double() for h in p.chunk(2))
        gi = float(torch.tensor(sched[i][0], dtype=torch.float32))
        live = 0.0 if i < zero_init else 1.0
        if mode == APG:
            beta = 0.0 if i == 0 else float(torch.tensor(momentum, dtype=torch.float32))
            R = float(torch.tensor(norm_threshold, dtype=torch.float32))
            m = (c - u) + beta * m if beta != 0.0 else c - u
            n = dot(m, m).sqrt()
            if norms is not None:
                norms.append(n.flatten().clone())
            r = torch.where((n > R) & (R > 0), R / n.clamp_min(1e-300), torch.ones_like(n))
            scc = dot(c, c)
            rho = torch.where(scc > 0, dot(m, c) / scc.clamp_min(1e-300), torch.zeros_like(scc))
            a_w = live * (gi - 1.0) * r
            a_c = live * (1.0 + (gi - 1.0) * (float(torch.tensor(eta, dtype=torch.float32)) - 1.0) * r * rho)
            w = m
        else:
            suu = dot(u, u)
            s = torch.where(suu > 0, dot(c, u) / suu.clamp_min(1e-300), torch.zeros_like(suu))
            a_c, a_w, w = live * gi * torch.ones_like(s), live * (1.0 - gi) * s, u
        v = (a_c * c + a_w * w).float()
        if order is not None:
            c0, c1, c2 = weights[i]
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
    return x
