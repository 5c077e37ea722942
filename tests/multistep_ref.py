"""References of the multistep (Adams-Bashforth 2 / 3) solvers - the reference project has none, so the definition lives here.

table_loop64         the table-driven loop in fp64 for a scalar ODE dx/dsigma = f(sigma, x): what the device does with a coefficient
                     table of host/tables.solver_table(multistep_order=), without its roundings.
rk4_reference        the same ODE by classical Runge-Kutta in fp64 (the order tests' truth).
restated_loop        the fp32 CPU sampling loop over O.dit_forward with a velocity history, in the manner of
                     guidance_ref.restated_loop; with all history weights zero it is O.sample_latents(..., "euler").
The per-element reference of one step with a history ring is opcheck.step_ref_and_bounds(..., ring, it).
"""
import math

import torch

import guidance_ref as G
from opcheck import STEP_HIST
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- scalar problems
def ode_f(s, x):
    """dx/dsigma = x cos(3 sigma) + 0.5 sin(5 sigma): the order tests' problem, x(1) = 1, integrated down to sigma = 0."""
    return x * math.cos(3.0 * s) + 0.5 * math.sin(5.0 * s)


def rk4_reference(f=ode_f, x0=1.0, s0=1.0, s1=0.0, n=20000):
    h, x, s = (s1 - s0) / n, float(x0), float(s0)
    for _ in range(n):
        k1 = f(s, x)
        k2 = f(s + h / 2, x + h / 2 * k1)
        k3 = f(s + h / 2, x + h / 2 * k2)
        k4 = f(s + h, x + h * k3)
        x += h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        s += h
    return x


def table_loop64(sigmas, table, f=ode_f, x0=1.0):
    """x after the rows of `table` ([n, 8] fp32: c_0 in column 0, dt in column 2, flags in column 4, c_1 / c_2 in columns 6 / 7),
    every entry taken as the fp64 number it is, the velocity of row i evaluated at sigmas[i]."""
    x, hist = float(x0), []
    for i in range(table.shape[0]):
        row = [float(t) for t in table[i].double()]
        v = f(float(sigmas[i].double()), x)
        deriv = row[0] * v
        if int(row[4]) & STEP_HIST:
            if row[6] != 0.0:
                deriv += row[6] * hist[-1]
            if row[7] != 0.0:
                deriv += row[7] * hist[-2]
        x += deriv * row[2]
        hist.append(v)
    return x


# ----------------------------------------------------------------------------- the model loop
def weight_rows(sigmas, order, start=0, n=None):
    """[(c_0, c_1, c_2)] as fp32 tensors' entries: the rows of tables.solver_table(multistep_order=order, start=start)[start:]."""
    from foley_amd.host import tables
    n = len(sigmas) - 1 if n is None else n
    t = tables.solver_table(sigmas, "euler", n, multistep_order=order, start=start)[start:]
    return [(t[i, 0], t[i, 6], t[i, 7]) for i in range(t.shape[0])]


def restated_loop(sd, heads, noise, text, uncond_text, clip, sync, steps, guidance, order=2, weights=None, rescale=0.0, text_len=77,
                  shift=1.0, skip_first=0):
    """noise [bs, 128, La]; conditioning with batch 1.  Two halves [uncond ; cond], v = u + g (c - u) as O.sample_latents writes
    it; then deriv = c_0 v (+ c_1 v_{n-1}) (+ c_2 v_{n-2}) in fp32, left to right, a zero weight skipped, and x + deriv * dt with
    dt = sigma_{n+1} - sigma_n in fp32 - O.SolverState's euler line.  weights: [(c_0, c_1, c_2)] per iteration (default: the
    table's rows for `order`); rescale: the CFG-rescale factor of guidance_ref on v before it enters the history.
    skip_first = i0: the suffix [i0, steps) of the iterations from `noise` as the state at i0 (weights then has steps - i0 rows)."""
    bs = noise.shape[0]
    sig = O.flow_sigmas(steps, shift)
    ts = O.flow_timesteps(sig)
    if weights is None:
        weights = weight_rows(sig, order, skip_first)
    rep = lambda a: a.repeat(bs, 1, 1)
    text_r, unc_r = O.pad_or_trim_text(rep(text), text_len), O.pad_or_trim_text(rep(uncond_text), text_len)
    clip_r, sync_r = rep(clip), rep(sync)
    e_clip = sd["empty_clip_feat"].unsqueeze(0).expand(bs, clip.shape[1], -1)
    e_sync = sd["empty_sync_feat"].unsqueeze(0).expand(bs, sync.shape[1], -1)
    clip_in, sync_in, text_in = torch.cat([e_clip, clip_r]), torch.cat([e_sync, sync_r]), torch.cat([unc_r, text_r])
    x, hist = noise.float(), []
    for i, t in enumerate(ts):
        if i < skip_first:
            continue
        xin = torch.cat([x, x])
        vu, vc = O.dit_forward(sd, heads, xin, t.expand(xin.shape[0]), text_in, clip_in, sync_in).chunk(2)
        v = vu + guidance * (vc - vu)
        if rescale > 0.0:
            v = (G.rescale_factor64(v, vc, rescale) * v.double()).float()
        c0, c1, c2 = weights[i - skip_first]
        deriv = v if float(c0) == 1.0 else c0 * v
        if float(c1) != 0.0:
            deriv = deriv + c1 * hist[-1]
        if float(c2) != 0.0:
            deriv = deriv + c2 * hist[-2]
        dt = sig[i + 1] - sig[i]
        x = x + deriv * dt
        hist.append(v)
    return x
