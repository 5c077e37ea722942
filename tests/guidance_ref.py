"""Op-level reference of the guidance controls (the loop under them, its schedule and its fp64 rescale factor are in loop_ref.py).

factor_ref      fp64 rescale factors and their bound, over opcheck.combine_ref (the guided value and its bound; the solver
                update behind it is opcheck.step_ref_and_bounds).
"""
import torch

import opcheck as oc
from opcheck import U32


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
