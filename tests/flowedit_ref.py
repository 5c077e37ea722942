"""CPU reference of FlowEdit (host/audio_edit.FlowEditSpec, foley_set_flowedit): one step on the kernel's state with the device's
expression order, and the loop restated over O.dit_forward / O.flow_sigmas / O.flow_timesteps in the manner of
loop_ref.restated_loop - the same [uncond ; cond] combine, the noise table an input, a dtype argument - or over a velocity function
given directly (the analytic transport test)."""
import torch

from foley_amd.host import tables
from oracle import foley_oracle as O


def fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors (or scalars): the product is exact in fp64 and the sum is rounded to fp64, then to
    fp32 - the fused result except where the fp64 sum falls on an fp32 rounding boundary (about one element in 2^29)."""
    t = lambda v: torch.as_tensor(v, dtype=torch.float32).double()
    return (t(a) * t(b) + t(c)).float()


def ref_inputs(z, x_src, n, s):
    """(z_src, z_tar) [V, C, L] fp32 at sigma s from noise n [V, C, L]: z_src = fma(1 - s, x_src, rnd(s n)), z_tar = (z - x_src) + z_src."""
    s = torch.tensor(float(s), dtype=torch.float32)
    z_src = fma32(1 - s, x_src.expand_as(z), s * n)
    return z_src, (z - x_src) + z_src


def rows_of(z_src, z_tar, dtype=torch.float32):
    """The staged model input rows [2*2V*L, C]: [half][clip][l][c] with clips [src_0 .. src_{V-1}, tar_0 .. tar_{V-1}], both halves alike."""
    half = torch.cat([z_src, z_tar]).permute(0, 2, 1).reshape(-1, z_src.shape[1])
    return torch.cat([half, half]).to(dtype)


def ref_flowedit_step(pred, z, x_src, n_next, mask, row, g_src, g_tar):
    """One FlowEdit step in fp32 on the kernel's state: pred [2*2V*L, C], z [V, C, L], x_src [1 | V, C, L], n_next [V, C, L] the
    noise of the NEXT iteration, mask [L] or [1 | V, L] or None, row the coefficient row -> (z_new, z_src, z_tar).
      v_s = fma(g_src, c_s - u_s, u_s); v_t = fma(g_tar, c_t - u_t, u_t); d = v_t - v_s; d = m d; z = fma(d, dt, z)
    and the inputs of the next call at s = row[5] from z_new."""
    V, Cc, L = z.shape
    dt, s = torch.tensor(float(row[2]), dtype=torch.float32), float(row[5])
    P = pred.view(2, 2 * V, L, Cc).permute(0, 1, 3, 2)
    u_s, c_s, u_t, c_t = P[0, :V], P[1, :V], P[0, V:], P[1, V:]
    v_s = fma32(torch.tensor(float(g_src)), c_s - u_s, u_s)
    v_t = fma32(torch.tensor(float(g_tar)), c_t - u_t, u_t)
    d = v_t - v_s
    if mask is not None:
        d = mask.view(-1, 1, L) * d
    z_new = fma32(d, dt, z)
    z_src, z_tar = ref_inputs(z_new, x_src, n_next, s)
    return z_new, z_src, z_tar


def model_velocity(sd, heads, text_src, text_tar, uncond_text, clip, sync, g_src, g_tar, V, steps, shift=1.0, text_len=77):
    """velocity_fn(z_src, z_tar, i) -> (v_s, v_t) over ONE O.dit_forward of the 2V-clip CFG batch [uncond ; cond] x [src.. ; tar..] at
    iteration i of the full run, each branch combined as u + g (c - u) with its own scale (loop_ref's two-half combine)."""
    ts = O.flow_timesteps(O.flow_sigmas(steps, shift))
    B = 2 * V
    src, tar = O.pad_or_trim_text(text_src, text_len), O.pad_or_trim_text(text_tar, text_len)
    unc = O.pad_or_trim_text(uncond_text, text_len).repeat(B, 1, 1)
    text_in = torch.cat([unc, src.repeat(V, 1, 1), tar.repeat(V, 1, 1)])
    e_clip = sd["empty_clip_feat"].unsqueeze(0).expand(B, clip.shape[1], -1)
    e_sync = sd["empty_sync_feat"].unsqueeze(0).expand(B, sync.shape[1], -1)
    clip_in, sync_in = torch.cat([e_clip, clip.repeat(B, 1, 1)]), torch.cat([e_sync, sync.repeat(B, 1, 1)])

    def fn(z_src, z_tar, i):
        x = torch.cat([z_src, z_tar]).float()
        xin = torch.cat([x, x])
        p = O.dit_forward(sd, heads, xin, ts[i].expand(xin.shape[0]), text_in, clip_in, sync_in)
        u, c = p.chunk(2)
        v = torch.cat([u[:V] + g_src * (c[:V] - u[:V]), u[V:] + g_tar * (c[V:] - u[V:])])
        return v[:V], v[V:]
    return fn


def restated_flowedit(velocity_fn, x_src, noise, steps, *, strength=1.0, mask=None, shift=1.0, dtype=torch.float32, trace=None):
    """The FlowEdit loop: x_src [1 | V, C, L], noise [n_iter | 1, V, C, L] (row j serves the j-th iteration run; one row: the fixed
    draw), velocity_fn(z_src, z_tar, i) -> (v_s, v_t) the guided velocities of the branches at iteration i of the FULL run (a model:
    model_velocity; or any function of the two states).  The iterations [i0, steps) with (k0, i0) = tables.edit_start under euler:
        z_src = (1 - sigma_i) x_src + sigma_i n;  z_tar = (z - x_src) + z_src;  d = v_t - v_s;  d = m d;  z += d (sigma_{i+1} - sigma_i)
    from z = x_src.  trace: a list that receives z after every iteration.  Returns z [V, C, L] in `dtype`."""
    sig = O.flow_sigmas(steps, shift).to(dtype)
    _k0, i0 = tables.edit_start(steps, "euler", strength)
    V = noise.shape[1]
    noise, xs = noise.to(dtype), x_src.to(dtype).expand(V, -1, -1)
    assert noise.shape[0] in (1, steps - i0), (noise.shape[0], steps - i0)
    m = None if mask is None else mask.to(dtype).view(-1, 1, mask.shape[-1])
    z = xs.clone()
    for i in range(i0, steps):
        n = noise[i - i0] if noise.shape[0] > 1 else noise[0]
        z_src = (1 - sig[i]) * xs + sig[i] * n
        z_tar = (z - xs) + z_src
        v_s, v_t = velocity_fn(z_src, z_tar, i)
        d = v_t.to(dtype) - v_s.to(dtype)
        if m is not None:
            d = m * d
        z = z + d * (sig[i + 1] - sig[i])
        if trace is not None:
            trace.append(z.clone())
    return z
