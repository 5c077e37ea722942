"""References for the prompt timeline (host/prompt_timeline.py, csrc/attention_timeline.hip): the fp64 reference and the derived
per-element bound of the timeline attention, and the restatement of the denoising loop on the CPU oracle with timed text."""
import contextlib

import torch
import torch.nn.functional as F

import loop_ref as L
import opcheck as oc
from oracle import foley_oracle as O


# ----------------------------------------------------------------------------- op level
def timeline_attention_ref_and_bound(q, k, v, set_a, set_b, alpha, out_dtype, p_dtype=None):
    """out = (1 - alpha) A_a + alpha A_b in fp64, A_s = softmax(q k_s^T / sqrt(hd)) v_s from the operands as rounded: q [Bq, H, Sq, hd],
    k / v [n_sets, H, Skv, hd] (v NOT transposed), set_a / set_b / alpha [Bq, Sq] (indices already inside [0, n_sets)); where
    alpha == 0 the result is A_a and set_b is not read.  Returns ([Bq, Sq, H hd], Bound).

    The bound is derived, not measured: per set (A_s, e_s) = opcheck.attention_ref_and_bound (before any store), and the blend - the
    kernel computes fl(fl(1 - alpha) A_a) + fl(alpha A_b) in fp32: one rounding of 1 - alpha, one per product, one for the sum, each
    relative to a term no larger than |(1 - alpha) A_a| + |alpha A_b| - adds 3 U32 of that sum to the propagated errors:
        e = (1 - alpha) e_a + alpha e_b + 3 U32 (|(1 - alpha) A_a| + |alpha A_b|)       (+ the output rounding term of Bound),
    the form of opcheck.edit_blend_ref_and_bound."""
    Bq, H, Sq, hd = q.shape
    n_sets = k.shape[0]
    sa, sb, al = set_a.long().cpu().view(Bq, Sq), set_b.long().cpu().view(Bq, Sq), alpha.double().cpu().view(Bq, Sq)
    used = set(sa.unique().tolist()) | set(sb[al != 0].unique().tolist())
    A = torch.zeros(n_sets, Bq, Sq, H * hd, dtype=torch.float64)
    E = torch.zeros_like(A)
    for s in sorted(used):
        r, b = oc.attention_ref_and_bound(q.cpu(), k[s:s + 1].cpu(), v[s:s + 1].cpu(), torch.float32, p_dtype)
        A[s], E[s] = r, b.e
    pick = lambda T, idx: torch.gather(T, 0, idx.view(1, Bq, Sq, 1).expand(1, Bq, Sq, H * hd))[0]
    Aa, Ea = pick(A, sa), pick(E, sa)
    sb_eff = torch.where(al != 0, sb, sa)                  # alpha == 0: set_b is not read
    Ab, Eb = pick(A, sb_eff), pick(E, sb_eff)
    w = al.unsqueeze(-1)
    pa, pb = (1.0 - w) * Aa, w * Ab
    return pa + pb, oc.Bound((1.0 - w) * Ea + w * Eb + 3 * oc.U32 * (pa.abs() + pb.abs()), out_dtype)


# ----------------------------------------------------------------------------- the loop on the CPU oracle
def _timed_triple_block(sets_raw, table):
    """A copy of O.triple_block whose cross-attention applies the table.  sets_raw [n_sets, Lt, cond_dim]: the text sets as the
    loop feeds them (padded to the text length); table: (set_a, set_b, alpha) tensors [B, Lv + La] of the batch the loop runs (CFG
    halves stacked).  Every set goes through cond_in and text_cross_kv with the shapes O uses for its one set per row, and its K is
    rotated with positions 0..Lt - so a table that names one set per row reproduces O.triple_block bit for bit."""
    sa, sb, al = table

    def block(sd, p, H, audio, cond, v_cond, vec, rope_a, rope_v, rope_aq, rope_vq, rope_t):
        W = lambda k: sd[p + k]
        La, Lv = audio.shape[1], v_cond.shape[1]
        B = audio.shape[0]
        Lt = sets_raw.shape[1]
        assert sa.shape == (B, Lv + La) and cond.shape[1] == Lt
        sv = F.silu(vec)
        am = F.linear(sv, W("audio_mod.linear.weight"), W("audio_mod.linear.bias")).chunk(9, dim=-1)
        vm = F.linear(sv, W("v_cond_mod.linear.weight"), W("v_cond_mod.linear.bias")).chunk(9, dim=-1)
        mod = lambda x, sh, sc: x * (1 + sc[:, None]) + sh[:, None]
        # 1. joint self attention: as O.triple_block
        aq, ak, av = O._heads(F.linear(mod(O.layer_norm(audio, 1e-6), am[0], am[1]),
                                       W("audio_self_attn_qkv.weight"), W("audio_self_attn_qkv.bias")), 3, H)
        aq = O.rms_norm(aq, W("audio_self_q_norm.weight"), 1e-6)
        ak = O.rms_norm(ak, W("audio_self_k_norm.weight"), 1e-6)
        vq, vk, vv = O._heads(F.linear(mod(O.layer_norm(v_cond, 1e-6), vm[0], vm[1]),
                                       W("v_cond_attn_qkv.weight"), W("v_cond_attn_qkv.bias")), 3, H)
        vq = O.rms_norm(vq, W("v_cond_attn_q_norm.weight"), 1e-6)
        vk = O.rms_norm(vk, W("v_cond_attn_k_norm.weight"), 1e-6)
        aq, ak = O.apply_rope(aq, *rope_a), O.apply_rope(ak, *rope_a)
        vq, vk = O.apply_rope(vq, *rope_v), O.apply_rope(vk, *rope_v)
        q = torch.cat((vq, aq), dim=1).transpose(1, 2)
        k = torch.cat((vk, ak), dim=1).transpose(1, 2)
        v = torch.cat((vv, av), dim=1).transpose(1, 2)
        att = O.sdpa(q, k, v).transpose(1, 2).flatten(2)
        v_att, a_att = att[:, :Lv], att[:, Lv:]
        audio = audio + F.linear(a_att, W("audio_self_proj.weight"), W("audio_self_proj.bias")) * am[2][:, None]
        v_cond = v_cond + F.linear(v_att, W("v_cond_self_proj.weight"), W("v_cond_self_proj.bias")) * vm[2][:, None]
        # 2. cross attention, query = [v_cond ; audio]: every token against the text set(s) of its own time
        aq = O._heads(F.linear(mod(O.layer_norm(audio, 1e-6), am[3], am[4]),
                               W("audio_cross_q.weight"), W("audio_cross_q.bias")), 1, H)[0]
        aq = O.apply_rope(O.rms_norm(aq, W("audio_cross_q_norm.weight"), 1e-6), *rope_aq)
        vq = O._heads(F.linear(mod(O.layer_norm(v_cond, 1e-6), vm[3], vm[4]),
                               W("v_cond_cross_q.weight"), W("v_cond_cross_q.bias")), 1, H)[0]
        vq = O.apply_rope(O.rms_norm(vq, W("v_cond_cross_q_norm.weight"), 1e-6), *rope_vq)
        q = torch.cat((vq, aq), dim=1).transpose(1, 2)
        used = sorted(set(sa.unique().tolist()) | set(sb[al != 0].unique().tolist()))
        per_set = {}
        for s in used:
            c_s = sets_raw[s:s + 1].expand(B, Lt, -1).contiguous()
            c_s = F.linear(F.silu(F.linear(c_s, sd["cond_in.linear_1.weight"], sd["cond_in.linear_1.bias"])),
                           sd["cond_in.linear_2.weight"], sd["cond_in.linear_2.bias"])
            tk, tv = O._heads(F.linear(c_s, W("text_cross_kv.weight"), W("text_cross_kv.bias")), 2, H)
            tk = O.apply_rope(O.rms_norm(tk, W("text_cross_k_norm.weight"), 1e-6), *rope_t)
            per_set[s] = O.sdpa(q, tk.transpose(1, 2), tv.transpose(1, 2)).transpose(1, 2).flatten(2)      # [B, S, D]
        att = torch.zeros_like(per_set[used[0]])
        w = al.unsqueeze(-1).to(att.dtype)
        for s in used:                               # (1 - alpha) A_a + alpha A_b; alpha == 0: A_a as it is
            ua, ub = (sa == s).unsqueeze(-1), ((sb == s) & (al != 0)).unsqueeze(-1)
            att = torch.where(ua, torch.where(w == 0, per_set[s], att + (1 - w) * per_set[s]), att)
            att = torch.where(ub, att + w * per_set[s], att)
        v_att, a_att = att[:, :Lv], att[:, Lv:]
        audio = audio + F.linear(a_att, W("audio_cross_proj.weight"), W("audio_cross_proj.bias")) * am[5][:, None]
        v_cond = v_cond + F.linear(v_att, W("v_cond_cross_proj.weight"), W("v_cond_cross_proj.bias")) * vm[5][:, None]

        # 3. GELU-tanh MLPs: as O.triple_block
        def mlp(x, pre):
            h = F.gelu(F.linear(x, W(pre + ".fc1.weight"), W(pre + ".fc1.bias")), approximate="tanh")
            return F.linear(h, W(pre + ".fc2.weight"), W(pre + ".fc2.bias"))
        audio = audio + mlp(mod(O.layer_norm(audio, 1e-6), am[6], am[7]), "audio_mlp") * am[8][:, None]
        v_cond = v_cond + mlp(mod(O.layer_norm(v_cond, 1e-6), vm[6], vm[7]), "v_cond_mlp") * vm[8][:, None]
        return audio, v_cond

    return block


@contextlib.contextmanager
def timed_text(sets_raw, table):
    """For the duration of the block, O.triple_block is the copy that applies `table` to the text sets `sets_raw` (O.dit_forward
    and the loops built on it - O.sample_latents, loop_ref.restated_loop - then run with timed text; the `cond` they pass is only
    used for its shape)."""
    keep = O.triple_block
    O.triple_block = _timed_triple_block(sets_raw, table)
    try:
        yield
    finally:
        O.triple_block = keep


def table_tensors(flat, rows):
    """prompt_timeline.batch_table's flat lists -> (set_a, set_b int64, alpha fp32-rounded float32) tensors [rows, S]."""
    sa, sb, al = flat
    return (torch.tensor(sa, dtype=torch.int64).view(rows, -1), torch.tensor(sb, dtype=torch.int64).view(rows, -1),
            torch.tensor(al, dtype=torch.float64).to(torch.float32).view(rows, -1))


def oracle_timeline_latents(sd, heads, noise, sets, flat_table, clip, sync, steps, guidance, solver, text_len=77):
    """The restated loop with timed text.  sets [n_sets, T, cond_dim]: with guidance > 1 [negative ; prompts...], as the plan holds
    them; flat_table: prompt_timeline.batch_table(..., ncfg, clips) of the same run."""
    ncfg = 2 if guidance > 1.0 else 1
    raw = O.pad_or_trim_text(sets, text_len)
    with timed_text(raw, table_tensors(flat_table, ncfg * noise.shape[0])):
        return L.restated_loop(sd, heads, noise, sets[-1:], sets[:1], clip, sync, steps, guidance, solver, text_len=text_len).x
