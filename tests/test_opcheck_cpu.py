"""The element-wise checker (tests/opcheck.py) tested on the CPU.

For each bound, a CPU "kernel" that does what the HIP kernel does in a different order (fp32 accumulation over 4 K ranges summed
in reverse; a tiled online softmax with P rounded to the operand type; a two-pass fp32 LayerNorm with the lane / butterfly
reduction order) must stay inside it, and each planted defect - the kind a ragged tile, one wave's fragment or a skipped K
range leaves - must be MISSED by the norm gate the GPU suites use (conftest.rel_err against the per-dtype tolerance) and CAUGHT
by the element-wise check.  For fp32 operands, whose 2e-6 gate already sees most of them, only the catch is asserted.

Shapes: 500 x 1536 x 1536 for bf16 and fp32 operands.  fp16 operands use the bs = 8 grid 4000 x 6144 x 1536: at 500 x 1536 the fp16
gate (8e-4) already sees a 64-wide K slice lost on a 1 x 16 strip (0.2 * 4 / 876 = 9e-4), so "missed by the old gate" can only be
stated for fp16 where the grid is large - which is where the 256x256 tiles and the panel-group order run.
"""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

import opcheck as oc
import test_attention_edges_gpu as ae
from conftest import rel_err

F32_TOL, BF16_TOL, F16_TOL = 2e-6, 6e-3, 8e-4                         # test_ops_gpu.py: the per-dtype GEMM gates
GATE = {torch.float32: F32_TOL, torch.bfloat16: BF16_TOL, torch.float16: F16_TOL}
LN_TOL = {torch.float32: 1e-4, torch.bfloat16: 4e-3, torch.float16: 5e-4}       # test_pairs_gpu.py
ATTN_TOL = {torch.float32: 3e-6, torch.bfloat16: 1e-2, torch.float16: 2e-3}     # test_attention / test_attention_bf16
SHAPE = {torch.bfloat16: (500, 1536, 1536), torch.float32: (500, 1536, 1536), torch.float16: (4000, 6144, 1536)}
DT = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "f16", "f32"]


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _gemm_kernel(A, W, b, drop=None):
    """fp32 accumulation over 4 K ranges, the ranges summed in reverse, then the bias.  drop = (rows, cols, k0): those outputs lose
    the 64-wide K slice at k0."""
    A, W = A.float(), W.float()
    K = A.shape[1]
    edges = [0, K // 4 // 64 * 64, K // 2 // 64 * 64, 3 * K // 4 // 64 * 64, K]
    parts = [A[:, lo:hi] @ W[:, lo:hi].t() for lo, hi in zip(edges[:-1], edges[1:])]
    y = parts[3]
    for p in parts[2::-1]:
        y = y + p
    if drop is not None:
        rows, cols, k0 = drop
        y[rows, cols] -= A[rows, k0:k0 + 64] @ W[cols, k0:k0 + 64].t()
    return y + b if b is not None else y


_cache = {}


def _problem(dt):
    """Operands rounded to dt, the emulated fp32 result, ref64 and mag - once per dtype."""
    if dt not in _cache:
        M, N, K = SHAPE[dt]
        A, W, b = _rand((M, K), 1).to(dt), _rand((N, K), 2, 1 / math.sqrt(K)).to(dt), _rand((N,), 3, 0.1)
        ref, mag = oc.gemm_ref64(A, W, b)
        _cache[dt] = dict(A=A, W=W, b=b, ref=ref, mag=mag, y=_gemm_kernel(A, W, b), M=M, N=N, K=K)
    return _cache[dt]


def _missed_and_caught(dt, got, ref, bound, what, gate=None, box=None):
    """The planted defect passes the norm gate (16-bit operands) and fails the element-wise check, inside `box`."""
    if dt != torch.float32:
        e = rel_err(got, ref)
        assert e < (gate or GATE[dt]), (what, "the old gate sees this defect already", e)
    with pytest.raises(AssertionError) as ei:
        oc.assert_elementwise(got, ref, bound, what)
    msg = str(ei.value)
    assert "outside their bound" in msg
    if box is not None:      # every offender lies inside the planted region (an element whose own error is tiny may stay inside its bound)
        r0, r1, c0, c1 = (int(v) for v in re.search(r"rows \[(-?\d+), (-?\d+)\] x cols \[(-?\d+), (-?\d+)\]", msg).groups())
        assert box[0] <= r0 <= r1 <= box[1] and box[2] <= c0 <= c1 <= box[3], msg


# ----------------------------------------------------------------------------- helpers of the checker
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_ulp16_is_the_spacing_of_the_type(dt):
    x = torch.cat((_rand((4096,), 5).double() * 10, torch.tensor([1.0, 2.0, 0.5, 3e-5, 1e-7, 65504.0 if dt == torch.float16 else 1e30],
                                                                  dtype=torch.float64)))
    xq = x.to(dt)
    up = (xq.abs().view(torch.int16) + 1).view(dt)                       # the next representable value: one step in the bit pattern
    ok = torch.isfinite(up.float())
    assert torch.equal((up.double() - xq.abs().double())[ok], oc.ulp16(xq.double(), dt)[ok])
    # rounding any fp64 value to the type stays within the output term
    assert bool(((xq.double() - x).abs() <= oc.output_term(x, xq, dt)).all())


def test_guard_band_reports_strays_and_keeps_quiet_otherwise():
    dev = torch.device("cpu")
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        g = oc.guarded((5, 24), dt, dev, rows=(2, 3), pad_cols=8)
        assert g.pitch == 32 and g.view.shape == (5, 24) and bool(torch.isnan(g.view).all())
        assert bool(torch.isfinite(g.buf[:2 * 32].float()).all()), "the guard pattern must not be NaN"
        g.view.copy_(torch.ones(5, 24))
        g.check()
        for off, where in ((g.n0 - 1, "row -1, col 31"), (g.n0 + 24, "row 0, col 24"), (g.n0 + 5 * 32, "row 5, col 0")):
            g2 = oc.guarded((5, 24), dt, dev, rows=(2, 3), pad_cols=8)
            g2.buf[off] = 1.0
            with pytest.raises(AssertionError, match=where):
                g2.check()
    g = oc.guarded((8, 4, 6), torch.float32, dev, rows=(1, 1))       # guard slabs around [ks, M, N]
    assert g.view.is_contiguous() and g.view.shape == (8, 4, 6)
    g.view.zero_()
    g.check()
    m = oc.guarded((5, 24), torch.float32, dev, pad_cols=8, misalign=2)
    assert (m.view.data_ptr() - m.buf.data_ptr()) % 16 == 8


def test_assert_elementwise_reports_box_and_nan():
    ref = torch.zeros(10, 20, dtype=torch.float64)
    got = ref.clone()
    assert oc.assert_elementwise(got, ref, 1e-3, "clean") == 0.0
    got[3:5, 7:9] = 1.0
    got[4, 8] = float("nan")
    with pytest.raises(AssertionError) as ei:
        oc.assert_elementwise(got, ref, 1e-3, "planted")
    assert "4 of 200" in str(ei.value) and "rows [3, 4] x cols [7, 8]" in str(ei.value) and "(row 4, col 8)" in str(ei.value)


# ----------------------------------------------------------------------------- GEMM bounds
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("shape", [(500, 1536, 1536), (1000, 1536, 6144)], ids=["k1536", "k6144"])
def test_reordered_accumulation_stays_inside(dt, shape):
    M, N, K = shape
    A, W, b = _rand((M, K), 11).to(dt), _rand((N, K), 12, 1 / math.sqrt(K)).to(dt), _rand((N,), 13, 0.1)
    ref, mag = oc.gemm_ref64(A, W, b)
    y = _gemm_kernel(A, W, b)
    r32 = oc.assert_elementwise(y, ref, oc.elementwise_gemm_bound(A, W, b, K, mag=mag), "fp32 store")
    assert r32 < 0.05, r32            # the bound is worst-case: a real accumulation uses a sliver of it
    if dt != torch.float32:
        r16 = oc.assert_elementwise(y.to(dt), ref, oc.elementwise_gemm_bound(A, W, b, K, dt, mag=mag), "16-bit store")
        assert r16 <= 1.0


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rows", [1, 16], ids=["strip_1x16", "patch_16x16"])
def test_dropped_k_slice(dt, rows):
    """One 64-wide K slice lost on a 1 x 16 strip of the last row / on a 16 x 16 patch at the ragged corner."""
    p = _problem(dt)
    M, N, K = p["M"], p["N"], p["K"]
    rs, cs = slice(M - rows, M), slice(N - 16, N)
    y = _gemm_kernel(p["A"], p["W"], p["b"], drop=(rs, cs, K - 128))
    bound = oc.elementwise_gemm_bound(p["A"], p["W"], p["b"], K, mag=p["mag"])
    _missed_and_caught(dt, y, p["ref"], bound, "dropped K slice", box=(M - rows, M - 1, N - 16, N - 1))


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_dropped_bias_on_one_element(dt):
    p = _problem(dt)
    y = p["y"].clone()
    c = int(p["b"].abs().argmax())                      # the tail column whose bias matters most (|b| ~ 0.3)
    r = p["M"] - 1
    y[r, c] -= p["b"][c]
    bound = oc.elementwise_gemm_bound(p["A"], p["W"], p["b"], p["K"], mag=p["mag"])
    _missed_and_caught(dt, y, p["ref"], bound, "dropped bias", box=(r, r, c, c))


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gate_of_the_other_cfg_half_on_a_strip(dt):
    """Gated residual x0 + g * y with per-(cfg, token) gate rows: a 1 x 16 strip of the first half reads the second half's gate."""
    p = _problem(dt)
    M, N = p["M"], p["N"]
    L = M // 2
    x0, gate = _rand((M, N), 21), _rand((2, L, N), 22, 0.3)
    g = gate.reshape(M, N)
    out = x0 + g * p["y"]
    r, cs = L - 1, slice(N - 16, N)
    out[r, cs] = x0[r, cs] + gate[1, L - 1, cs] * p["y"][r, cs]
    ref = x0.double() + g.double() * p["ref"]
    e_y = oc.elementwise_gemm_bound(p["A"], p["W"], p["b"], p["K"], mag=p["mag"]).e
    bound = oc.gated_residual_bound(e_y, g, x0, p["ref"])
    oc.assert_elementwise(x0 + g * p["y"], ref, bound, "clean gated residual")
    _missed_and_caught(dt, out, ref, bound, "wrong CFG half's gate", box=(r, r, N - 16, N - 1))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_store_off_by_four_ulp(dt):
    """One stored element moved by 4 ulp of the output type, planted on the element of largest |y| (|y| ~ 5: 4 ulp = 0.125 bf16, 0.0156 fp16).
    Limits, stated rather than hidden: the accumulation term (K + 4) 2^-23 mag is ~ 4.6e-3 at K = 1536 (mag ~ 0.64 sqrt(K)) - that is
    4.7 ulp of fp16 for |y| in [1, 2), so on fp16 a 4-ulp error is caught only where |y| >= 2; at K = 6144 it is 3.7e-2 = 4.7 ulp of
    bf16 in [1, 2) and the same holds for bf16.  Smaller stray errors on a 16-bit store need the fp32-store epilogue of the same tile."""
    p = _problem(dt)
    y16 = p["y"].to(dt)
    bound = oc.elementwise_gemm_bound(p["A"], p["W"], p["b"], p["K"], dt, mag=p["mag"])
    assert oc.assert_elementwise(y16, p["ref"], bound, "clean 16-bit store") <= 1.0
    flat = int(p["ref"].abs().argmax())
    r, c = divmod(flat, p["N"])
    bad = y16.clone()
    bad[r, c] = (y16[r, c].double() + 4 * oc.ulp16(y16[r, c].double(), dt)).to(dt)
    assert float((bad[r, c].double() - y16[r, c].double()).abs()) == float(4 * oc.ulp16(y16[r, c].double(), dt))
    _missed_and_caught(dt, bad, p["ref"], bound, "4 ulp", box=(r, r, c, c))
    # a TYPICAL element (|y| in [1, 2)): caught on bf16 (4 ulp = 3.1e-2 against ~ 4.6e-3 + half an ulp); on fp16 it is the stated limit -
    # 4 ulp = 3.9e-3 lies inside the accumulation term, and the check must NOT claim it
    idx = ((p["ref"].abs() >= 1.25) & (p["ref"].abs() < 1.75)).nonzero()[0]
    r, c = int(idx[0]), int(idx[1])
    typ = y16.clone()
    typ[r, c] = (y16[r, c].double() + 4 * oc.ulp16(y16[r, c].double(), dt)).to(dt)
    if dt == torch.bfloat16:
        _missed_and_caught(dt, typ, p["ref"], bound, "4 ulp on a typical element", box=(r, r, c, c))
    else:
        assert oc.assert_elementwise(typ, p["ref"], bound, "4 ulp of fp16 at |y| ~ 1.5: inside the bound") <= 1.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_slabs_and_activations_stay_inside(dt):
    """Deferred split-K slabs rounded once each to the operand type, and the activation epilogues on the fp32 accumulator."""
    M, N, K, ks = 300, 512, 1536, 3
    A, W, b = _rand((M, K), 31).to(dt), _rand((N, K), 32, 1 / math.sqrt(K)).to(dt), _rand((N,), 33, 0.5)
    ref, mag = oc.gemm_ref64(A, W, None)
    e_y = oc.elementwise_gemm_bound(A, W, None, K, mag=mag).e
    slabs = torch.stack([(A.float()[:, i * 512:(i + 1) * 512] @ W.float()[:, i * 512:(i + 1) * 512].t()).to(dt) for i in range(ks)])
    r = oc.assert_elementwise(slabs.double().sum(0), ref, oc.slab_bound(e_y, mag, ks, dt), "16-bit slabs")
    assert r < 1.0
    lost = slabs.clone()
    lost[2, M - 1, N - 16:] = 0                                      # one K range missing on a strip
    with pytest.raises(AssertionError, match=rf"rows \[{M - 1}, {M - 1}\] x cols \[{N - 16}, {N - 1}\]"):
        oc.assert_elementwise(lost.double().sum(0), ref, oc.slab_bound(e_y, mag, ks, dt), "slab strip lost")
    refb, magb = ref + b.double(), mag + b.double().abs()
    e_b = (K + 4) * oc.U32 * magb
    y32 = (A.float() @ W.float().t()) + b
    for name, fn in (("silu", F.silu), ("gelu", lambda t: F.gelu(t, approximate="tanh")), ("gelu_erf", F.gelu)):
        a_act = oc.measure_a_act(name, refb, torch.device("cpu"))
        assert 0 < a_act < 1e-5, (name, a_act)
        oc.assert_elementwise(fn(y32).to(dt), oc.act64(name, refb), oc.act_bound(name, e_b, a_act, dt), name)
    h = N // 2
    a_act = oc.measure_a_act("silu", refb[:, :h], torch.device("cpu"))
    bound = oc.silugate_bound(refb[:, :h], refb[:, h:], e_b[:, :h], e_b[:, h:], a_act, dt)
    oc.assert_elementwise((F.silu(y32[:, :h]) * y32[:, h:]).to(dt), oc.act64("silu", refb[:, :h]) * refb[:, h:], bound, "silu gate")


# ----------------------------------------------------------------------------- LayerNorm
def _ln_kernel(x, shift, scale, eps, odt):
    """Two-pass fp32 LayerNorm in the kernel's reduction order: every lane sums its D / 64 elements (stride 64 float4) in turn, a
    butterfly adds the 64 lanes."""
    M, D = x.shape

    def wave_sum(t):                                   # t [M, D] fp32
        lanes = t.view(M, D // 256, 64, 4).permute(0, 2, 1, 3)            # [M, lane, i, e]
        s = torch.zeros(M, 64)
        for i in range(D // 256):
            s = s + ((lanes[:, :, i, 0] + lanes[:, :, i, 1]) + (lanes[:, :, i, 2] + lanes[:, :, i, 3]))
        w = 64
        while w > 1:
            w //= 2
            s = s[:, :w] + s[:, w:2 * w]
        return s                                       # [M, 1]
    mean = wave_sum(x) / float(D)
    d = x - mean
    rstd = 1.0 / torch.sqrt(wave_sum(d * d) / float(D) + eps)
    return (d * rstd * (1.0 + scale) + shift).to(odt), mean


@pytest.mark.parametrize("odt", DT, ids=IDS)
def test_layernorm_two_pass_inside_and_neighbours_mean_caught(odt):
    """Rows of 1e3 + N(0, 1) at D = 1536, M = 6000 (test_ln_mod_width's grid).  The planted row is normalised with the next row's
    mean; it is the row whose mean differs from its neighbour's by the amount closest to 0.02 - large against the bound (~ 4e-3 + the
    output term), small enough (0.02 / sqrt(6000) = 2.6e-4) for the fp16 norm gate of 5e-4 to miss."""
    M, D, eps = 6000, 1536, 1e-6
    x = 1e3 + _rand((M, D), 41)
    shift, scale = _rand((D,), 42, 0.3), _rand((D,), 43, 0.3)
    out, mean = _ln_kernel(x, shift, scale, eps, odt)
    _, ref, _, bound = oc.layernorm_ref_and_bound(x, shift, scale, eps, odt)
    assert oc.assert_elementwise(out, ref, bound, "two-pass fp32 LayerNorm") <= 1.0
    one_pass = ((x * x).mean(-1, keepdim=True) - x.mean(-1, keepdim=True) ** 2)      # E[x^2] - E[x]^2 in fp32: garbage at |x| ~ 1e3
    bad1 = ((x - x.mean(-1, keepdim=True)) * torch.rsqrt(one_pass.clamp_min(0) + eps) * (1 + scale) + shift).to(odt)
    with pytest.raises(AssertionError):
        oc.assert_elementwise(bad1, ref, bound, "one-pass variance")
    dm = (mean[1:, 0] - mean[:-1, 0]).abs()
    r = int((dm - 0.02).abs().argmin())
    assert 0.015 < float(dm[r]) < 0.025
    d = x[r] - mean[r + 1]
    var = ((x[r] - mean[r]) ** 2).mean()
    bad = out.clone()
    bad[r] = (d / torch.sqrt(var + eps) * (1 + scale) + shift).to(odt)
    _missed_and_caught(odt, bad, ref, bound, "neighbour's mean", gate=LN_TOL[odt])
    with pytest.raises(AssertionError, match=rf"rows \[{r}, {r}\]"):
        oc.assert_elementwise(bad, ref, bound, "neighbour's mean")


def test_layernorm_pending_slabs_inside():
    M, D, k = 64, 1536, 7
    x0 = 1e3 + _rand((M, D), 44)
    slabs, bias, gate = _rand((k, M, D), 45, 0.5).to(torch.bfloat16), _rand((D,), 46, 0.1), _rand((M, D), 47, 0.3)
    acc = bias.expand(M, D).clone()
    for s in range(k):
        acc = acc + slabs[s].float()
    x = x0 + gate * acc
    out, _ = _ln_kernel(x, torch.zeros(D), torch.zeros(D), 1e-6, torch.bfloat16)
    x64, ref, bx, bo = oc.layernorm_ref_and_bound(x0, None, None, 1e-6, torch.bfloat16, slabs, bias, gate)
    assert oc.assert_elementwise(x, x64, bx, "x written back") <= 1.0
    assert oc.assert_elementwise(out, ref, bo, "LayerNorm after the pending slabs") <= 1.0


# ----------------------------------------------------------------------------- attention
def _attn_kernel(q, k, v, dt, skip_last_tile_of=None, kt=32, part=None, out_dt=None, psplit=False, lose_second_half_of=None, drop_wave=None):
    """Tiled online softmax in fp32 over key tiles of `kt` keys (32; 64: attn_bf16_long_kernel, ONE maximum per 64 keys), P rounded
    ONCE to the operand type before P V, the row sum from the unrounded P (attention.hip); the store in out_dt (default dt).
    part: the keys are partitioned, every part walks its tiles on its own and the parts' (m, l, O) are merged at the end, in the
    kernels' own order -
        'runs4'   four contiguous runs of 32-key tiles, run w = tiles [nt w / 4, nt (w + 1) / 4) in integers (attn_bf16_kernel,
                  attn_lds_kernel; a run may be empty: m = -inf, l = 0): m* = max m, w_x = exp(m_x - m*), L = sum w_x l_x,
                  O = (sum_x w_x O_x) (1 / L), x = 0 .. 3
        'halves'  keys [64 t, 64 t + 32) of every 64-key tile / keys [64 t + 32, 64 t + 64) (attn_bf16_pair_kernel; the second
                  half of the last tile may hold no key): m = max(m_a, m_b), l = l_a f_a + l_b f_b, O = O_a f_a + O_b f_b.
    psplit: P travels as its rounding plus the rounded residual (attn_bf16_wide_kernel<64> in bf16).
    Planted defects: skip_last_tile_of = (b, h, row): that query never sees the last key tile; lose_second_half_of = (b, h, row):
    ('halves') it never sees the second key half of the last 64-key tile; drop_wave = (w, (b, h, row)): ('runs4') the merge of
    that query leaves out run w."""
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    qf, kf, vf = q.float(), k.float(), v.float()

    def walk(tiles, width, last_defect=None):
        m = torch.full((B, H, Sq, 1), float("-inf"))
        l = torch.zeros(B, H, Sq, 1)
        o = torch.zeros(B, H, Sq, hd)
        for k0 in tiles:
            s = qf @ kf[:, :, k0:k0 + width].transpose(2, 3) / math.sqrt(hd)
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            p = torch.exp(s - m_new)
            if last_defect is not None and k0 == tiles[-1]:
                b, h, r = last_defect
                p[b, h, r] = 0.0
                m_new[b, h, r] = m[b, h, r]
            alpha = torch.where(m_new == m, torch.ones_like(m), torch.exp(m - m_new))      # the rescale is skipped where no maximum moved
            l = l * alpha + p.sum(-1, keepdim=True)
            pr = p.to(dt).float() if dt != torch.float32 else p
            o = o * alpha + pr @ vf[:, :, k0:k0 + width]
            if psplit:
                o = o + (p - pr).to(dt).float() @ vf[:, :, k0:k0 + width]
            m = m_new
        return m, l, o

    if part is None:
        m, l, o = walk(list(range(0, Skv, kt)), kt, skip_last_tile_of)
        res = o * (1.0 / l)
    elif part == "runs4":
        nt = (Skv + 31) // 32
        runs = [walk([32 * t for t in range(nt * w // 4, nt * (w + 1) // 4)], 32) for w in range(4)]
        mstar = functools.reduce(torch.maximum, [r[0] for r in runs])
        wt = [torch.exp(r[0] - mstar) for r in runs]
        if drop_wave is not None:
            w, (b, h, r) = drop_wave
            wt[w][b, h, r] = 0.0
        L, acc = torch.zeros(B, H, Sq, 1), torch.zeros(B, H, Sq, hd)
        for x in range(4):
            L = L + wt[x] * runs[x][1]
            acc = acc + wt[x] * runs[x][2]
        res = acc * (1.0 / L)
    else:
        assert part == "halves"
        (ma, la, oa), (mb, lb, ob) = (walk(list(range(32 * half, Skv, 64)), 32, lose_second_half_of if half else None) for half in (0, 1))
        m = torch.maximum(ma, mb)
        fa, fb = torch.exp(ma - m), torch.exp(mb - m)
        res = (oa * fa + ob * fb) * (1.0 / (la * fa + lb * fb))
    return res.transpose(1, 2).reshape(B, Sq, H * hd).to(out_dt or dt)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_attention_tiled_inside_and_missing_key_tile_caught(dt):
    # 5 s self-attention under CFG, two clips: ten key tiles, 2 keys in the ragged last one - the planted row loses ~ 2 / 290 of its
    # weights (error ~ 7e-3 against outputs of ~ 6e-2), one row of 13 920: 1e-3 in the norm
    B, H, Sq, Skv, hd = 4, 12, 290, 290, 128
    q, k, v = (_rand((B, H, S, hd), 50 + i).to(dt) for i, S in enumerate((Sq, Skv, Skv)))
    ref, bound = oc.attention_ref_and_bound(q, k, v, dt, p_dtype=dt)
    assert oc.assert_elementwise(_attn_kernel(q, k, v, dt), ref, bound, "tiled attention") <= 1.0
    bad = _attn_kernel(q, k, v, dt, skip_last_tile_of=(1, 2, 289))
    _missed_and_caught(dt, bad, ref, bound, "last key tile missing", gate=ATTN_TOL[dt], box=(290 + 289, 290 + 289, 2 * hd, 3 * hd - 1))


def _edge_emulation(form, kind):
    """The arithmetic of a 16-bit form of tests/test_attention_edges_gpu.py FORMS as _attn_kernel options."""
    if form == "attn_bf16_kernel" or form.startswith("attn_lds_kernel"):
        return dict(part="runs4")
    if "pair" in form:
        return dict(part="halves")
    if "long" in form:
        return dict(kt=64)
    return dict(psplit=form == "attn_bf16_wide_kernel<64>" and kind == "bf16")


def _edge_ratio(c):
    """err / bound of the form's emulation on the operands of edge case c (long / pair forms: the first clip's heads)."""
    dt, odt = ae.DTS[c["kind"]], ae.DTS[c["out"]]
    q, k, v = ae.operands(c)
    if c["form"] in ae.LONG:
        q, k, v = q[:1], k[:1], v[:1]
    ref, bound = oc.attention_ref_and_bound(q, k, v, odt, p_dtype=dt)
    got = _attn_kernel(q.to(dt), k.to(dt), v.to(dt), dt, out_dt=odt, **_edge_emulation(c["form"], c["kind"]))
    return float(((got.double() - ref).abs() / bound.total(ref, got.double())).max())


@pytest.mark.parametrize("form", [f for f, v in ae.FORMS.items() if v[1] != ["f32"]], ids=ae._slug)
def test_attention_edge_inputs_are_fair(form):
    """The condition under which the GPU cases may assert 1.0: the form's own arithmetic - fp32, its key tiles and partition, P
    rounded once - stays within the bound on the very operands of the scores cases, the fp32-output cases and the cases of 2 .. 96
    keys, in bf16 and fp16.  (A few keys average little, and u_p is half the unit round-off: see
    test_grouped_attention_reference_and_leaking_query.)"""
    cases = ae.sweep_cases("scores", form) + ae.sweep_cases("out", form) + [c for c in ae.sweep_cases("skv", form) if 2 <= c["Skv"] <= 96]
    worst = {}
    for c in cases:
        r = _edge_ratio(c)
        worst[(c["name"], c["kind"])] = r
        print(f"{form} {c['name']} {c['kind']} -> {c['out']}: emulation err / bound {r:.3f}")
    over = {k: round(r, 3) for k, r in worst.items() if not r <= 1.0}
    assert not over, over


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_attention_lost_second_key_half_missed_by_the_norm_gate_and_caught(dt):
    """attn_bf16_pair_kernel: 548 keys, four of them in the second half of the last 64-key tile; one query of 2 x 12 x 400 loses them
    (0.7 % of its weights): 9e-4 in the norm, one row of one head outside the bound."""
    B, H, Sq, Skv, hd = 2, 12, 400, 548, 128
    q, k, v = (_rand((B, H, S, hd), 60 + i).to(dt) for i, S in enumerate((Sq, Skv, Skv)))
    ref, bound = oc.attention_ref_and_bound(q, k, v, dt, p_dtype=dt)
    assert oc.assert_elementwise(_attn_kernel(q, k, v, dt, part="halves"), ref, bound, "key halves merged") <= 1.0
    bad = _attn_kernel(q, k, v, dt, part="halves", lose_second_half_of=(1, 5, 399))
    _missed_and_caught(dt, bad, ref, bound, "second key half of the last tile lost", gate=ATTN_TOL[dt], box=(400 + 399, 400 + 399, 5 * hd, 6 * hd - 1))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_attention_dropped_wave_in_the_merge_missed_by_the_norm_gate_and_caught(dt):
    """attn_bf16_kernel / attn_lds_kernel: 98 keys = four key tiles, one per wave, the last with 2 keys; the merge of one query of
    4 x 12 x 580 leaves out the last wave's state (2 % of its weights): ~ 1e-3 in the norm, one row of one head outside the bound."""
    B, H, Sq, Skv, hd = 4, 12, 580, 98, 128
    q, k, v = (_rand((B, H, S, hd), 70 + i).to(dt) for i, S in enumerate((Sq, Skv, Skv)))
    ref, bound = oc.attention_ref_and_bound(q, k, v, dt, p_dtype=dt)
    assert oc.assert_elementwise(_attn_kernel(q, k, v, dt, part="runs4"), ref, bound, "four key runs merged") <= 1.0
    bad = _attn_kernel(q, k, v, dt, part="runs4", drop_wave=(3, (2, 7, 311)))
    _missed_and_caught(dt, bad, ref, bound, "one wave's state dropped in the merge", gate=ATTN_TOL[dt], box=(2 * 580 + 311, 2 * 580 + 311, 7 * hd, 8 * hd - 1))


# ----------------------------------------------------------------------------- cross attention fused into the q projection
CROSS_TOL = {torch.bfloat16: 6e-3, torch.float16: 1e-3}      # ATTN_TOL of test_pairs_gpu.py / test_gemm_cross_q_with_attention_epilogue
CROSS_GATE_SEEN = {}                                         # defect -> dtype -> would the norm gate have seen it (printed, and asserted for the lost tile)


def _cross_epilogue(c, dt, lost_tile=None, drop_last_key=False, wrong_set=None, skip_rescale_rows=None):
    """The ATTN branch of gemm_common.h's head-split epilogue in fp32 on the CPU: projection (fp32 accumulation), bias, RMSNorm
    (rsqrt of the mean square + eps, times gain), RoPE, q rounded to the operand type; then per row 32-key tiles of the row's text
    set, keys >= Skv masked, online softmax with P rounded ONCE and the row sum from the unrounded values, accumulators rescaled
    when the running maximum moved.  Defects: lost_tile = (row, head): that query never sees the last tile; drop_last_key: key
    Skv - 1 masked for everybody; wrong_set = row: served from the neighbouring text set; skip_rescale_rows = (r0, r1): on tile 1
    those rows' accumulators are not rescaled where the maximum moved."""
    M, H, L, Skv = c["M"], c["H"], c["L"], c["Skv"]
    y = (c["A"].to(dt).float() @ c["W"].to(dt).float().t() + c["b"]).view(M, H, 128)
    rinv = torch.rsqrt((y * y).sum(-1, keepdim=True) * (1.0 / 128.0) + _f(1e-6))
    qn = y * rinv * c["gain"]
    pl = c["pos"].long().repeat(M // L)
    cs, sn = c["cos"][pl][:, None], c["sin"][pl][:, None]
    q0, q1 = qn[..., 0::2], qn[..., 1::2]
    q = torch.stack((q0 * cs - q1 * sn, q1 * cs + q0 * sn), -1).flatten(-2).to(dt).float()
    sets = c["sets"].clone()
    if wrong_set is not None:
        sets[wrong_set] = sets[wrong_set] + (1 if sets[wrong_set] == 0 else -1)
    kf, vf = c["k"][sets], c["v"][sets]                                   # [M, H, Skv, 128]
    kend = Skv - 1 if drop_last_key else Skv
    m = torch.full((M, H, 1), float("-inf"))
    l = torch.zeros(M, H, 1)
    o = torch.zeros(M, H, 128)
    tiles = list(range(0, Skv, 32))
    for kt in tiles:
        hi = min(kt + 32, kend)
        if hi <= kt:
            continue
        s = torch.einsum("mhd,mhjd->mhj", q, kf[:, :, kt:hi]) * _f(1 / math.sqrt(128))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp(s - m_new)
        if lost_tile is not None and kt == tiles[-1]:
            r, h = lost_tile
            p[r, h] = 0.0
            m_new[r, h] = m[r, h]
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        a_o = alpha
        if skip_rescale_rows is not None and kt == 32:
            a_o = alpha.clone()
            a_o[skip_rescale_rows[0]:skip_rescale_rows[1]] = 1.0
        o = o * a_o + torch.einsum("mhj,mhjd->mhd", p.to(dt).float(), vf[:, :, kt:hi])
        m = m_new
    return (o * (1.0 / l)).reshape(M, H * 128).to(dt)


_cross_cache = {}
CROSS_EMUL = ["sharp"] + [n for n in oc.CROSS_CASES if n != "auto_plan"]      # auto_plan: skv77's operands at 12 heads


def _cross_case(name):
    """'sharp': two text sets of 250 tokens (clips 1), 8 query tiles of 64 rows, the fourth straddles the sets; M H = 2000 (row, head)
    pairs for the norm gate to average over.  Every other name: the operands of the GPU case of that name (opcheck.CROSS_CASES)."""
    if name != "sharp":
        return oc.cross_case(name)
    if name not in _cross_cache:
        _cross_cache[name] = oc.cross_dyadic_case(Bc=2, L=250, H=4, bdiv=1, Skv=77, seed=7100, k_scale=2.0)
    return _cross_cache[name]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["sharp"] + list(oc.CROSS_CASES))
def test_cross_dyadic_operands_are_exact_and_rarely_ambiguous(name, dt):
    """The conditions the sharp cases rest on, decided by the reference alone: the projection of the dyadic operands is exact in
    fp32 (e_y = 0), at most 1 % of the q elements are ambiguous, and every ambiguous element's span is one ulp of its value."""
    c = _cross_case(name)
    assert torch.equal(c["A"].to(dt).float(), c["A"]) and torch.equal(c["W"].to(dt).float(), c["W"])
    assert torch.equal(c["k"].to(dt).float(), c["k"]) and torch.equal(c["v"].to(dt).float(), c["v"])
    y32 = c["A"] @ c["W"].t() + c["b"]
    assert torch.equal(y32.double().view_as(c["y64"]), c["y64"]), "the projection must be exact in fp32"
    yr = (c["A"].flip(1) @ c["W"].flip(1).t()) + c["b"]                      # ... in another order too
    assert torch.equal(yr, y32)
    lo, hi = oc.rounding_span16(c["q64"], c["e_q"], dt)
    amb = hi != lo
    share = float(amb.double().mean())
    print(f"cross {name} {dt}: ambiguous share of q {share:.3e}")
    assert share <= 0.01, share
    assert bool(((hi - lo)[amb] <= oc.ulp16(torch.maximum(hi.abs(), lo.abs()), dt)[amb]).all()), "an ambiguous element moves by one ulp"
    s = torch.einsum("mhd,mhjd->mhj", c["q64"], c["k"].double()[c["sets"]]) / math.sqrt(128)
    if name == "large_scores":
        assert float(s.amax()) > 35 and float(s.amin()) < -35, (float(s.amax()), float(s.amin()))
    elif c["Skv"] >= 32:      # neither flat nor one-hot: the largest probability of a row between 2 / Skv and 0.9 for nearly every row
        pmax = torch.softmax(s, -1).amax(-1)
        assert float((pmax > 2.0 / c["Skv"]).double().mean()) > 0.95 and float((pmax < 0.9).double().mean()) > 0.95


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", CROSS_EMUL)
def test_cross_epilogue_emulation_stays_inside(name, dt):
    c = _cross_case(name)
    ref, bound, share = oc.cross_attention_ref_and_bound(c["q64"], c["e_q"], c["k"], c["v"], c["sets"], dt)
    r = oc.assert_elementwise(_cross_epilogue(c, dt), ref, bound, f"cross epilogue emulation {name}")
    print(f"cross {name} {dt}: emulation err / bound {r:.3f}")
    assert r <= 1.0


def _cross_defect(dt, name, what, box_rows, gate_must_miss=False, **defect):
    c = _cross_case(name)
    ref, bound, _ = oc.cross_attention_ref_and_bound(c["q64"], c["e_q"], c["k"], c["v"], c["sets"], dt)
    bad = _cross_epilogue(c, dt, **defect)
    e = rel_err(bad, ref)
    CROSS_GATE_SEEN.setdefault(what, {})[str(dt)] = e >= CROSS_TOL[dt]
    print(f"cross defect '{what}' {dt}: norm error {e:.3e} against the gate {CROSS_TOL[dt]:.0e} ({'seen' if e >= CROSS_TOL[dt] else 'MISSED'})")
    if gate_must_miss:
        assert e < CROSS_TOL[dt], (what, "the norm gate sees this defect already", e)
    with pytest.raises(AssertionError) as ei:
        oc.assert_elementwise(bad, ref, bound, what)
    r0, r1 = (int(v) for v in re.search(r"rows \[(-?\d+), (-?\d+)\]", str(ei.value)).groups())
    assert box_rows[0] <= r0 <= r1 <= box_rows[1], str(ei.value)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_cross_lost_ragged_tile_missed_by_the_norm_gate_and_caught(dt):
    """One (row, head) never sees keys 64 .. 76 of Skv = 77.  The pair is chosen by the REFERENCE (as the LayerNorm defect's row is):
    the one whose last tile carries the softmax weight closest to 2 % (bf16) / 0.5 % (fp16) - an error of ~ 1e-2 / 2.5e-3 on outputs
    of ~ 0.3, far above the bound (~ 2e-3 / 2.5e-4) and, over 2000 (row, head) pairs, ~ 1e-3 / 2e-4 in the norm: under ATTN_TOL."""
    c = _cross_case("sharp")
    s = torch.einsum("mhd,mhjd->mhj", c["q64"], c["k"].double()[c["sets"]]) / math.sqrt(128)
    w_last = torch.softmax(s, -1)[..., 64:].sum(-1)                        # [M, H]
    target = 0.02 if dt == torch.bfloat16 else 0.005
    r, h = divmod(int((w_last - target).abs().argmin()), c["H"])
    assert 0.5 * target < float(w_last[r, h]) < 2 * target
    _cross_defect(dt, "sharp", "lost ragged key tile", (r, r), gate_must_miss=True, lost_tile=(r, h))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_cross_planted_defects_exceed_the_bound(dt):
    c = _cross_case("sharp")
    M = c["M"]
    _cross_defect(dt, "sharp", "key Skv - 1 dropped", (0, M - 1), drop_last_key=True)
    # row 249 is the last row of text set 0, inside the straddling tile [192, 256): served from set 1
    assert int(c["sets"][249]) == 0 and int(c["sets"][250]) == 1
    _cross_defect(dt, "sharp", "row of a straddling tile served from the other set", (249, 249), wrong_set=249)
    _cross_defect(dt, "sharp", "accumulator rescale skipped on tile 1", (64, 95), skip_rescale_rows=(64, 96))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_cross_general_form_is_weak_but_catches_a_wrong_set_and_a_lost_tile(dt):
    """The form test_pairs_gpu.py asserts on the fused pair launch: random operands at K = 1536, real RoPE angles, the projection's
    real accumulation bound e_y.  Nearly every bf16 element of q is then ambiguous and the bound is a few per cent of P @ |V| -
    the emulation stays far inside, a row served from the other text set and a (row, head) of MEDIAN last-tile weight that lost
    its ragged tile still fail it."""
    tb = _tables()
    Bc, L, H, K, Skv = 2, 80, 2, 1536, 77
    M = Bc * L
    A, W, b = _rand((M, K), 700).to(dt).float(), _rand((H * 128, K), 701, 1 / math.sqrt(K)).to(dt).float(), _rand((H * 128,), 702, 0.1)
    gain = 1 + 0.1 * _rand((128,), 703)
    cos, sin = tb.rope_table(L + 1)
    pos = torch.arange(L, dtype=torch.int32)
    k, v = _rand((2, H, Skv, 128), 704).to(dt).float(), _rand((2, H, Skv, 128), 705).to(dt).float()
    y64, mag = oc.gemm_ref64(A, W, b)
    y64, e_y = y64.view(M, H, 128), ((K + 4) * oc.U32 * mag).view(M, H, 128)
    pl = pos.long().repeat(Bc)
    q64 = oc.head_q64(y64, gain, cos[pl], sin[pl], 1e-6)
    e_q = oc.head_split_pre_bound(e_y, y64, gain)
    sets = torch.arange(M) // L
    c = dict(A=A, W=W, b=b, gain=gain, cos=cos, sin=sin, pos=pos, k=k, v=v, sets=sets, M=M, L=L, H=H, Skv=Skv)
    ref, bound, share = oc.cross_attention_ref_and_bound(q64, e_q, k, v, sets, dt)
    pv = torch.einsum("mhj,mhjd->mhd", torch.softmax(torch.einsum("mhd,mhjd->mhj", q64, k.double()[sets]) / math.sqrt(128), -1),
                      v.double()[sets].abs()).reshape(M, H * 128)
    rel = float((bound.e / pv).max())
    r = oc.assert_elementwise(_cross_epilogue(c, dt), ref, bound, "general form")
    print(f"cross general form {dt}: ambiguous share {share:.3f}, bound <= {rel:.3e} of P @ |V|, emulation err / bound {r:.3f}")
    assert r <= 1.0 and rel < 0.2
    if dt == torch.bfloat16:
        assert share > 0.5
    with pytest.raises(AssertionError, match=rf"rows \[{L - 1}, {L - 1}\]"):
        oc.assert_elementwise(_cross_epilogue(c, dt, wrong_set=L - 1), ref, bound, "wrong set")
    s = torch.einsum("mhd,mhjd->mhj", q64, k.double()[sets]) / math.sqrt(128)
    w_last = torch.softmax(s, -1)[..., 64:].sum(-1).flatten()
    rr, hh = divmod(int(w_last.argsort()[w_last.numel() // 2]), H)
    with pytest.raises(AssertionError, match=rf"rows \[{rr}, {rr}\]"):
        oc.assert_elementwise(_cross_epilogue(c, dt, lost_tile=(rr, hh)), ref, bound, "lost tile")


# ----------------------------------------------------------------------------- block-diagonal (grouped) attention, head dim 64
def _grouped_kernel(q, k, v, gq, gkv, dt, leak_query=None, split=False):
    """32-key tiles over the whole packed sequence, every query masked to its own group's keys, a tile with no visible key
    contributing nothing (the m_new == -inf guards of attn_bf16_wide_kernel<64, GRP>); P rounded once, or with split as the
    head-dim-64 bf16 kernel carries it: the rounding plus the rounded residual, P V over both.  leak_query = t: that query also
    sees the first key of the NEXT group."""
    G, H, Sq, hd = q.shape
    Skv = k.shape[2]
    qf, kf, vf = q.float(), k.float(), v.float()
    t = torch.arange(Sq)
    klo = (t // gq) * gkv
    key = torch.arange(Skv)
    vis = (key[None, :] >= klo[:, None]) & (key[None, :] < (klo + gkv)[:, None])        # [Sq, Skv]
    if leak_query is not None:
        vis[leak_query, int(klo[leak_query]) + gkv] = True
    m = torch.full((G, H, Sq, 1), float("-inf"))
    l = torch.zeros(G, H, Sq, 1)
    o = torch.zeros(G, H, Sq, hd)
    for kt in range(0, Skv, 32):
        s = qf @ kf[:, :, kt:kt + 32].transpose(2, 3) / math.sqrt(hd)
        s = torch.where(vis[:, kt:kt + 32], s, torch.full_like(s, float("-inf")))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        m_exp = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        p = torch.exp(s - m_exp)
        alpha = torch.where(torch.isinf(m_new), torch.ones_like(m_new), torch.exp(m - m_new))
        l = l * alpha + p.sum(-1, keepdim=True)
        hi = p.to(dt).float()
        o = o * alpha + hi @ vf[:, :, kt:kt + 32]
        if split:
            o = o + (p - hi).to(dt).float() @ vf[:, :, kt:kt + 32]
        m = m_new
    return (o / l).transpose(1, 2).reshape(G, Sq, H * hd).to(dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("p,gq,gkv,cut,surplus", [(14, 8, 9, 0, 0), (5, 8, 9, 3, 0), (5, 8, 9, 0, 7), (3, 33, 40, 3, 7), (4, 1, 9, 0, 0),
                                                   (5, 20, 32, 0, 0), (5, 20, 33, 0, 0)])
def test_grouped_attention_reference_and_leaking_query(dt, p, gq, gkv, cut, surplus):
    """opcheck.grouped_attention_ref_and_bound against the tiled emulation (ragged last group: Sq = p gq - cut; surplus keys beyond
    the last group carry V = 1e4 and must weigh exactly nothing), and a query that also sees the first key of the next group.
    A limit, stated rather than hidden: u_p = U16 is HALF the unit round-off of the type (opcheck's conventions), an allowance that
    rests on many rounded probabilities averaging under P @ |V|.  A group of 9 keys averages little: this emulation - fp32
    throughout, P rounded once, nothing else - reaches 1.25 of the bound on ~ 1e-4 of the bf16 elements at 6 x 12 x 14 groups
    (0.96 in fp16, whose output term is larger against u_p; 0.93 from 32 keys per group on).  What is rigorous for ANY group size
    is twice u_p, so that is what the once-rounded emulation is held to below 32 keys per group.  The GPU cases assert 1.0
    throughout, and the bf16 kernel meets it by carrying the rounding's residual too: that arithmetic (split) is held to 1.0 here."""
    G, H, Sq, Skv = 2, 3, p * gq - cut, p * gkv + surplus
    q, k, v = (_rand((G, H, S, 64), 520 + i).to(dt) for i, S in enumerate((Sq, Skv, Skv)))
    v[:, :, p * gkv:] = 1e4
    ref, bound = oc.grouped_attention_ref_and_bound(q, k, v, gq, gkv, dt, p_dtype=dt)
    assert ref.shape == (G, Sq, H * 64) and float(ref.abs().max()) < 100
    got = _grouped_kernel(q, k, v, gq, gkv, dt)
    r = float(((got.double() - ref).abs() / bound.total(ref, got.double())).max())
    assert r <= (1.0 if gkv >= 32 else 2.0), r
    if dt == torch.bfloat16:
        gs = _grouped_kernel(q, k, v, gq, gkv, dt, split=True)
        rs = float(((gs.double() - ref).abs() / bound.total(ref, gs.double())).max())
        print(f"grouped emulation, P as rounding + residual: err / bound {rs:.3f}")
        assert rs <= 1.0, rs
    print(f"grouped emulation p{p} gq{gq} gkv{gkv} cut{cut} surplus{surplus} {dt}: err / bound {r:.3f}")
    t = gq - 1                                                            # the last query of the first group
    if p > 1:
        bad = _grouped_kernel(q, k, v, gq, gkv, dt, leak_query=t)
        with pytest.raises(AssertionError) as ei:
            oc.assert_elementwise(bad.view(G, Sq, H * 64)[0], ref[0], oc.Bound(2 * bound.e[0], dt), "query sees the next group's first key")
        assert f"rows [{t}, {t}]" in str(ei.value), str(ei.value)


# ----------------------------------------------------------------------------- DAC residual epilogue
def test_dac_residual_and_snake_inside_and_defects_caught():
    """Dilated conv k = 7 in fp32 with the taps summed in reverse, + residual, + snake (what EPI_DAC does in another order) stays inside
    opcheck.dac_bounds; a residual dropped on one element and a 1 x 16 strip whose snake reads the NEXT channel's alpha fail the
    element-wise check (fp32 operands: only the catch is asserted, as for the other fp32 defects)."""
    B, T, C, dil = 2, 2000, 64, 3
    x, w, b = _rand((B, C, T), 61), _rand((C, C, 7), 62, 1 / math.sqrt(7 * C)), _rand((C,), 63, 0.1)
    alpha, res = 1 + 0.2 * _rand((C,), 64), _rand((B * T, C), 65, 0.01)
    conv = lambda a, ww: F.conv1d(a, ww, None, dilation=dil, padding=3 * dil)
    rows = lambda t: t.transpose(1, 2).reshape(B * T, C)
    y = rows(conv(x.double(), w.double()) + b.double().view(1, C, 1))
    mag = rows(conv(x.double().abs(), w.double().abs()) + b.double().abs().view(1, C, 1))
    acc = torch.zeros(B, C, T)
    xp = F.pad(x, (3 * dil, 3 * dil))
    for t in reversed(range(7)):                                   # fp32, one tap at a time, last tap first
        acc = acc + torch.einsum("oc,bct->bot", w[:, :, t], xp[:, :, t * dil:t * dil + T])
    v32 = rows(acc + b.view(1, C, 1)) + res
    s32 = v32 + (1.0 / (alpha + 1e-9)) * torch.sin(alpha * v32) ** 2
    v = y + res.double()
    a_act = oc.measure_a_act_snake(v, alpha, torch.device("cpu"))
    assert 0 < a_act < 1e-5, a_act
    b0, b1 = oc.dac_bounds((7 * C + 4) * oc.U32 * mag, v, res, a_act)
    assert oc.assert_elementwise(v32, v, b0, "out0") <= 1.0
    assert oc.assert_elementwise(s32, oc.snake64(v, alpha), b1, "out1") <= 1.0
    r = B * T - 1
    bad0 = v32.clone()
    bad0[r, 5] -= res[r, 5]
    _missed_and_caught(torch.float32, bad0, v, b0, "residual dropped", box=(r, r, 5, 5))
    bad1 = s32.clone()
    a_next = alpha.roll(-1)
    bad1[r, 16:32] = (v32 + (1.0 / (a_next + 1e-9)) * torch.sin(a_next * v32) ** 2)[r, 16:32]
    _missed_and_caught(torch.float32, bad1, oc.snake64(v, alpha), b1, "neighbour channel's alpha", box=(r, r, 16, 31))


# ----------------------------------------------------------------------------- row, solver and DAC edge kernels
# fp32 CPU emulations of each expression in more than one order - with and without the product contracted into an FMA, window and
# tap sums forward and reversed - must stay inside the bounds of opcheck.py at the shapes tests/test_rowops_elementwise_gpu.py
# launches: this is the arbiter of each constant.  Planted defects: where an old gate exists and is a norm, the defect must pass it;
# where the old test could not see the defect because of its SHAPE or of where it looked, the defective emulation is run at the old
# shape through the old assertion (it passes) and at the new shape through the new check (it fails).
STEP_SHAPES = [(2, 128, 50), (3, 128, 33), (1, 128, 1), (2, 96, 31), (2, 40, 65)]


def _fma(a, b, c):
    """fp32 a * b + c with one rounding (the fp64 product of two fp32 values is exact)."""
    a, b, c = (t if torch.is_tensor(t) else torch.tensor(t, dtype=torch.float32) for t in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _step_emul(pred, x, x_saved, d_acc, row, ncfg, g, fma):
    """solver_step_kernel's expressions in fp32: (xn, x_saved', d_acc')."""
    clips, C, L = x.shape
    w_new, w_acc, dt, w_store = row[0], row[1], row[2], row[3]
    flags = int(row[4])
    P = pred.view(ncfg, clips, L, C).transpose(2, 3)
    if ncfg == 2:
        v = _fma(_f(g), P[1] - P[0], P[0]) if fma else P[0] + _f(g) * (P[1] - P[0])
    else:
        v = P[0]
    acc = torch.zeros_like(x) if (d_acc is None or flags & oc.STEP_ACC_RESET) else d_acc
    if float(w_acc) != 0:
        deriv = _fma(w_new, v, w_acc * acc) if fma else w_new * v + w_acc * acc
    else:
        deriv = w_new * v
    base = x_saved if flags & oc.STEP_USE_SAVED else x
    xn = _fma(deriv, dt, base) if fma else base + deriv * dt
    da = _fma(w_store, v, acc) if fma else acc + w_store * v
    return xn, (x.clone() if flags & oc.STEP_SAVE_X else x_saved), da


def _tables():
    from foley_amd.host import tables
    return tables


@pytest.mark.parametrize("solver,steps", [("euler", 3), ("heun-2", 4), ("midpoint-2", 4), ("kutta-4", 8)])
@pytest.mark.parametrize("ncfg", [1, 2])
@pytest.mark.parametrize("fma", [False, True], ids=["mul_add", "fma"])
def test_solver_step_emulations_stay_inside(solver, steps, ncfg, fma):
    tb = _tables()
    coef = tb.edit_solver_table(tb.sigma_grid(steps), solver, steps)
    for si, (clips, C, L) in enumerate(STEP_SHAPES):
        x, xs, da = _rand((clips, C, L), 200 + si), torch.zeros(clips, C, L), torch.zeros(clips, C, L)
        x0, noise, mask = _rand((clips, C, L), 210 + si, 0.7), _rand((clips, C, L), 220 + si), torch.rand(clips, L, generator=torch.Generator().manual_seed(si))
        for it in range(steps):
            pred = _rand((ncfg * clips * L, C), 230 + 10 * si + it)
            r = oc.solver_step_ref_and_bounds(pred, x, xs, da, coef[it], ncfg, 4.5)
            xn, xs2, da2 = _step_emul(pred, x, xs, da, coef[it], ncfg, 4.5, fma)
            assert oc.assert_elementwise(xn, *r["x"], f"x {solver} it {it}") <= 1.0
            assert oc.assert_elementwise(da2, *r["d_acc"], f"d_acc {solver} it {it}") <= 1.0
            assert torch.equal(xs2.double(), r["x_saved"])
            if r["flags"] & oc.STEP_BLEND:                     # the edit form's blend on the same iteration
                s = coef[it][5]
                tgt = _fma(s, noise, (1.0 - s) * x0) if fma else s * noise + (1.0 - s) * x0
                m = mask.view(clips, 1, L)
                xb = _fma(m, xn, (1.0 - m) * tgt) if fma else m * xn + (1.0 - m) * tgt
                ref, bound = oc.edit_blend_ref_and_bound(r["x"][0], r["x"][1].e, r["s_next"], x0, noise, mask)
                assert oc.assert_elementwise(xb, ref, bound, f"blend {solver} it {it}") <= 1.0
                xn = xb
            x, xs, da = xn, xs2, da2


def _windows_emul(xn, n_win, starts, weights, fma, reverse):
    V, C, L = xn.shape[0] // n_win, xn.shape[1], xn.shape[2]
    Ltot = starts[-1] + L
    G = torch.zeros(V, C, Ltot)
    first = torch.ones(Ltot, dtype=torch.bool)
    order = list(range(n_win))[::-1] if reverse else list(range(n_win))
    for k in order:
        s, xk = starts[k], xn.view(V, n_win, C, L)[:, k]
        cur = G[..., s:s + L]
        add = _fma(weights[k], xk, cur) if fma else cur + weights[k] * xk
        G[..., s:s + L] = torch.where(first[s:s + L], weights[k] * xk, add)
        first[s:s + L] = False
    return G


WIN_PLANS = [([0], 50), ([0, 50], 50), ([0, 20], 50), ([0, 32, 40], 65), ([0, 10, 20], 33)]   # Ltot = L, = n_win L, an edge inside a tile / on one, three deep


@pytest.mark.parametrize("fma", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("reverse", [False, True], ids=["window_order", "reversed"])
def test_windows_mean_and_stitch_emulations_stay_inside(fma, reverse):
    from foley_amd.host import long_form
    for pi, (starts, L) in enumerate(WIN_PLANS):
        plan = long_form.WindowPlan.from_frames(starts, L)
        xn = _rand((2 * plan.n_win, 40, L), 300 + pi)
        e_x = 2 * oc.U32 * xn.double().abs()
        G32 = _windows_emul(xn, plan.n_win, starts, plan.weights, fma, reverse)
        ref, e, G, e_G, cov = oc.windows_mean_ref_and_bound(xn.double(), None, plan.n_win, starts, plan.weights)
        assert oc.assert_elementwise(G32, G, e_G, f"stitch {starts}") <= 1.0
        ref2, e2, _, _, _ = oc.windows_mean_ref_and_bound(xn.double(), e_x, plan.n_win, starts, plan.weights)
        assert bool((e2 >= e).all()) and torch.equal(ref2, ref)
        single = cov == 1
        assert torch.equal(G32[..., single].double(), G[..., single]), "a singly covered frame has weight 1.0 and keeps its bits"


def test_flow_mix_emulations_stay_inside_and_unwritten_tail_caught():
    noise, x0 = _rand((3, 128, 77), 400), _rand((1, 128, 77), 401)
    for s in (1.0, 0.73, 0.25, 0.0):
        ref, bound = oc.flow_mix_ref_and_bound(noise, x0, s)
        sf = _f(s)
        for name, got in (("mul_add", sf * noise + (1.0 - sf) * x0), ("fma_a", _fma(sf, noise, (1.0 - sf) * x0)),
                          ("fma_b", _fma(1.0 - sf, x0, sf * noise))):
            assert oc.assert_elementwise(got, ref, bound, f"flow_mix {name} sigma {s}") <= 1.0
            if s in (0.0, 1.0):
                oc.assert_bits_equal(got, (noise if s == 1.0 else x0.expand_as(noise)).contiguous(), f"flow_mix exact {s}")

    def capped(noise, x0, s):      # a kernel whose grid stops at 4096 workgroups of 256: the tail keeps what the buffer held
        out = torch.full_like(noise, float("nan"))
        n = min(noise.numel(), 4096 * 256)
        out.view(-1)[:n] = (_f(s) * noise + (1.0 - _f(s)) * x0).reshape(-1)[:n]
        return out
    got = capped(noise, x0, 0.73)                                               # the old shape: nothing to see
    assert rel_err(got, 0.73 * noise + (1 - 0.73) * x0) < 1e-6
    big_n, big_x0 = _rand((3, 128, 2800), 402), _rand((1, 128, 2800), 403)
    ref, bound = oc.flow_mix_ref_and_bound(big_n, big_x0, 0.73)
    with pytest.raises(AssertionError, match=r"26624 of 1075200 elements outside"):
        oc.assert_elementwise(capped(big_n, big_x0, 0.73), ref, bound, "flow_mix tail")


@pytest.mark.parametrize("odt", DT, ids=IDS)
def test_rows_add_act_and_add_periodic_emulations(odt):
    cpu = torch.device("cpu")
    a, v = _rand((70, 1536), 410, 3.0), _rand((1536,), 411)
    for aa, vv in ((a, v), (a, None), (None, v)):
        ref, bound = oc.rows_add_act_ref_and_bound(aa, vv, True, odt, cpu)
        y = oc.sum32_cast(aa, vv, torch.float32)
        for name, got in (("division", y / (1.0 + torch.exp(-y))), ("torch", F.silu(y)), ("sigmoid", y * torch.sigmoid(y))):
            assert oc.assert_elementwise(got.expand(70, 1536).to(odt), ref.expand(70, 1536), bound, f"silu {name}") <= 1.0
        ref, bound = oc.rows_add_act_ref_and_bound(aa, vv, False, odt, cpu)
        assert bound is None and torch.equal(oc.sum32_cast(aa, vv, odt).double(), ref.float().to(odt).double())
    # a row that reads the NEXT row's broadcast element on one tile corner: 1 of 107 520 elements, invisible in a 6e-2 model gate
    ref, bound = oc.rows_add_act_ref_and_bound(a, v, True, odt, cpu)
    y = a + v
    y[69, 1535] = a[69, 1535] + v[0]
    _missed_and_caught(odt, F.silu(y).to(odt), ref, bound, "wrong broadcast element", gate=6e-2, box=(69, 69, 1535, 1535))


def _dac_out_emul(s, w, bias, reverse, drop=None):
    """dac_out_kernel in fp32: four channel quarters per output, each summed over the taps (forward or reversed), then combined.
    drop = (b, t): the staged sample row t is missing (zero) for the 64-sample workgroup that starts at t + 1."""
    B, T, C = s.shape
    sp = F.pad(s, (0, 0, 3, 3))
    out = torch.empty(B, T)
    cq = C // 4
    taps = list(range(7))[::-1] if reverse else list(range(7))
    parts = []
    for p in range(4):
        acc = torch.zeros(B, T)
        for j in taps:
            for c in (range(p * cq, (p + 1) * cq) if not reverse else reversed(range(p * cq, (p + 1) * cq))):
                acc = acc + sp[:, j:j + T, c] * w[j * C + c]
        parts.append(acc)
    acc = (parts[0] + parts[1]) + (parts[2] + parts[3])
    if drop is not None:
        b, t = drop
        for o in range(t + 1, min(t + 4, T)):      # outputs of the next workgroup that read sample t
            acc[b, o] -= (s[b, t] * w[(t - o + 3) * C:(t - o + 4) * C]).sum()
    return torch.tanh(acc + bias[0])


@pytest.mark.parametrize("T,C", [(1, 64), (3, 64), (63, 64), (64, 96), (65, 64), (300, 64), (300, 96)])
def test_dac_out_emulations_stay_inside(T, C):
    s, w, b = _rand((2, T, C), 420), _rand((7 * C,), 421, 0.1), _rand((1,), 422, 0.1)
    ref, bound, a_act = oc.dac_out_ref_and_bound(s, w, b, torch.device("cpu"))
    assert a_act < 1e-5
    for rev in (False, True):
        assert oc.assert_elementwise(_dac_out_emul(s, w, b, rev), ref, bound, f"dac_out T{T} C{C} reversed {rev}") <= 1.0


def test_dac_out_halo_sample_dropped_at_a_seam_is_caught():
    """Sample 63 of clip 1 missing from the halo of the workgroup that starts at 64: outputs 64..66 lose one tap each (~ 0.05 each).
    fp32 only, so - as for the other fp32 defects of this file - only the catch is asserted: the 2e-6 norm gate of test_dac_out
    does see a whole missing tap at T = 300 (the defect moves the norm by ~ 5e-3); what it never looked at are T < 64, T = 64 / 65
    and C = 96."""
    T, C = 300, 64
    s, w, b = _rand((2, T, C), 420), _rand((7 * C,), 421, 0.1), _rand((1,), 422, 0.1)
    ref, bound, _ = oc.dac_out_ref_and_bound(s, w, b, torch.device("cpu"))
    bad = _dac_out_emul(s, w, b, False, drop=(1, 63))
    _missed_and_caught(torch.float32, bad, ref, bound, "halo sample dropped", box=(1, 1, 64, 66))


@pytest.mark.parametrize("T", [1, 3, 63, 64, 65, 300])
def test_dac_in_emulations_stay_inside(T):
    C = 64
    x, w, b = _rand((2, T), 430), _rand((7, C), 431, 0.4), _rand((C,), 432, 0.1)
    alpha = torch.cat((torch.tensor([1e-3, 1e-2, 0.05, 0.3]), 1 + 0.2 * _rand((C - 4,), 433).abs()))
    y64, s64, b0, b1, a_act = oc.dac_in_ref_and_bounds(x, w, b, alpha, torch.device("cpu"))
    xp = F.pad(x, (3, 3))
    for fma, rev in ((True, False), (False, True)):
        acc = b.expand(2, T, C).clone()
        for j in (range(6, -1, -1) if rev else range(7)):
            xv = xp[:, j:j + T, None]
            acc = _fma(xv, w[j], acc) if fma else acc + xv * w[j]
        y = acc.reshape(2 * T, C)
        sn = torch.sin(alpha * y)
        inv = 1.0 / (alpha + 1e-9)
        snake = _fma(inv, sn * sn, y) if fma else y + inv * (sn * sn)
        assert oc.assert_elementwise(y, y64, b0, f"dac_in out0 T{T}") <= 1.0
        assert oc.assert_elementwise(snake, s64, b1, f"dac_in out1 T{T}") <= 1.0


def _wave_sum(t):
    """Butterfly over the 64 lanes (last dimension), fp32."""
    w = 64
    while w > 1:
        w //= 2
        t = t[..., :w] + t[..., w:2 * w]
    return t


def _qkv_emul(y, gain, cos, sin, eps, fma, butterfly):
    """qkv_split_kernel's role (1) in fp32 on y [n, H, 128]."""
    y0, y1 = y[..., 0::2], y[..., 1::2]
    if gain is not None:
        sq = _fma(y0, y0, y1 * y1) if fma else y0 * y0 + y1 * y1
        ss = _wave_sum(sq) if butterfly else sq.sum(-1, keepdim=True)
        rinv = torch.rsqrt(ss * (1.0 / 128.0) + _f(eps))
        y0, y1 = y0 * rinv * gain[0::2], y1 * rinv * gain[1::2]
    if cos is not None:
        c, s = cos[:, None], sin[:, None]
        z0 = _fma(y0, c, -(y1 * s)) if fma else y0 * c - y1 * s
        z1 = _fma(y1, c, y0 * s) if fma else y1 * c + y0 * s
        y0, y1 = z0, z1
    return torch.stack((y0, y1), -1).flatten(-2)


@pytest.mark.parametrize("odt", DT, ids=IDS)
@pytest.mark.parametrize("eps", [1e-6, 1.1920928955078125e-07])
def test_qkv_split_standalone_emulations_stay_inside(odt, eps):
    """The constant 8 of head_split_bound's rounding term on its own (e_y = 0): every order stays inside, heads of very different
    scale and a gain of mixed sign included."""
    tb = _tables()
    n, H = 77 * 2, 3
    y = _rand((n, H, 128), 440) * torch.logspace(-3, 3, n * H).view(n, H, 1)
    gain = (1 + 0.1 * _rand((128,), 441)) * torch.where(torch.arange(128) % 5 == 0, -1.0, 1.0)
    cos, sin = tb.rope_table(400)
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(1)) * 2
    for g, p in ((gain, pos), (gain, None), (None, pos), (None, None)):
        c, s = (cos[p], sin[p]) if p is not None else (None, None)
        ref, bound = oc.qkv_head_ref_and_bound(y, g, c, s, eps, odt)
        worst = 0.0
        for fma in (False, True):
            for fly in (False, True):
                got = _qkv_emul(y, g, c, s, eps, fma, fly).to(odt)
                worst = max(worst, oc.assert_elementwise(got, ref, bound, f"qkv gain {g is not None} pos {p is not None} fma {fma}"))
        assert worst <= 1.0
    # one wrong element at a tile corner: the last pair of the last head of the last row rotated with the NEXT position's angle
    ref, bound = oc.qkv_head_ref_and_bound(y[:, :, :], gain, cos[pos], sin[pos], eps, odt)
    bad = _qkv_emul(y, gain, cos[pos], sin[pos], eps, False, True)
    p2 = pos.clone()
    p2[-1] += 1
    bad[-1, -1, 126:] = _qkv_emul(y, gain, cos[p2], sin[p2], eps, False, True)[-1, -1, 126:]
    if odt == torch.float32:
        _missed_and_caught(odt, bad.to(odt).view(n * H, 128), ref.view(n * H, 128), oc.Bound(bound.e.reshape(n * H, 128), odt), "neighbour's angle",
                           box=(n * H - 1, n * H - 1, 126, 127))


def _vt_emul(qkv, B, L, H, nK, pitch, tok_off, dt, skip_second_half=False):
    """Role (2) of qkv_split_kernel: V tiles of 32 tokens written transposed, 16 tokens per thread half; the destination starts as
    zeros (what the old tests allocate)."""
    v = qkv.view(B, L, nK, H, 128)[:, :, nK - 1].to(dt)                     # [B, L, H, 128]
    out = torch.zeros(B, H, 128, pitch, dtype=dt)
    for l0 in range(0, L, 32):
        for half in range(2):
            if skip_second_half and half == 1:
                continue
            lo, hi = l0 + half * 16, min(l0 + half * 16 + 16, L)
            if lo < hi:
                out[..., tok_off + lo:tok_off + hi] = v[:, lo:hi].permute(0, 2, 3, 1)
    return out


def test_vt_half_tile_not_written_passes_the_old_shape_and_fails_the_new():
    dt = torch.bfloat16
    for L, seen in ((11, False), (17, True), (33, True), (77, True)):
        qkv = _rand((2 * L, 3 * 3 * 128), 450)
        want = _vt_emul(qkv, 2, L, 3, 3, 96, 4, dt)
        assert torch.equal(want[..., 4:4 + L], qkv.view(2, L, 3, 3, 128)[:, :, 2].permute(0, 2, 3, 1).to(dt))
        bad = _vt_emul(qkv, 2, L, 3, 3, 96, 4, dt, skip_second_half=True)
        if not seen:      # test_qkv_split_bf16_transposed_v's L = 11: no token ever reaches the second half
            assert torch.equal(bad, want)
        else:
            with pytest.raises(AssertionError, match="differ in their bits"):
                oc.assert_bits_equal(bad, want, f"V^T L {L}")


def test_stale_first_cfg_copy_of_rows_passes_the_old_assertion_and_fails_the_new():
    clips, C, L = 2, 128, 50
    x_prev, x = _rand((clips, C, L), 460), _rand((clips, C, L), 461)
    for dt in DT:
        rows = oc.rows_of(x, 2, dt)
        rows.view(2, clips, L, C)[0] = oc.rows_of(x_prev, 1, dt).view(clips, L, C)      # the unconditional half still holds the last step
        assert rel_err(rows.view(2, clips, L, C)[-1].float(), x.transpose(1, 2)) < (2e-6 if dt == torch.float32 else 1e-2)   # all the old test looked at
        with pytest.raises(AssertionError, match=r"rows \[0, 99\]"):
            oc.assert_bits_equal(rows, oc.rows_of(x, 2, dt), "rows_out")


def test_tile_corner_off_by_64_ulp_passes_the_step_gates_and_is_caught():
    """x[1, 31, 31] - the last element of the first 32 x 32 tile - moved by 64 ulp: 8e-6 of a tensor whose norm is ~ 113, far inside
    the 2e-6 / 1e-6 relative norm gates of test_solver_step / test_blend_step_op / test_windows_step_op."""
    tb = _tables()
    clips, C, L, ncfg = 2, 128, 50, 2
    coef = tb.solver_table(tb.sigma_grid(8), "euler", 8)
    x, pred = _rand((clips, C, L), 470), _rand((ncfg * clips * L, C), 471)
    r = oc.solver_step_ref_and_bounds(pred, x, None, None, coef[0], ncfg, 4.5)
    xn, _, _ = _step_emul(pred, x, None, None, coef[0], ncfg, 4.5, False)
    bad = xn.clone()
    bad[1, 31, 31] = (bad[1, 31, 31].view(torch.int32) + 64).view(torch.float32)
    assert rel_err(bad, r["x"][0]) < 1e-6
    with pytest.raises(AssertionError, match=r"1 of 12800 elements outside"):
        oc.assert_elementwise(bad, *r["x"], "x")


def test_periodic_flags_reference_and_a_checker_that_skips_the_last_row():
    """opcheck.periodic_flags compares BIT PATTERNS: + 0.0 against - 0.0 differs, equal NaN patterns agree.  A checker that never
    reaches the last row of the last group (a grid one workgroup short) misses one flipped bit there."""
    groups, rows, D = 3, 16, 1536
    base = _rand((groups, 8, D), 480)
    base[1, 3, 5] = float("nan")
    base[2, 0, 0] = 0.0
    x = base.repeat(1, 2, 1)
    assert oc.periodic_flags(x, 8).tolist() == [0, 0, 0]
    z = x.clone()
    z[2, 8, 0] = -0.0
    assert oc.periodic_flags(z, 8).tolist() == [0, 0, 1]
    y = x.clone()
    y.view(torch.int32)[2, 15, D - 1] ^= 1
    assert oc.periodic_flags(y, 8).tolist() == [0, 0, 1]
    assert oc.periodic_flags(y[:, :8], 8).tolist() == [0, 0, 0]                 # rows <= period: nothing is compared
    skipping = (y.view(torch.int32)[:, 8:15] != y.view(torch.int32)[:, :7]).flatten(1).any(1).to(torch.int32)
    assert skipping.tolist() == [0, 0, 0] != oc.periodic_flags(y, 8).tolist()


def test_assert_bits_equal_nan_and_signed_zero():
    a = torch.tensor([[1.0, 0.0, float("nan")]])
    oc.assert_bits_equal(a, a.clone(), "same")
    with pytest.raises(AssertionError, match=r"\(row 0, col 1\)"):
        oc.assert_bits_equal(torch.tensor([[1.0, -0.0, float("nan")]]), a, "signed zero")
    other_nan = a.clone()
    other_nan.view(torch.int32)[0, 2] ^= 1
    with pytest.raises(AssertionError):
        oc.assert_bits_equal(other_nan, a, "payload")
    oc.assert_bits_equal(other_nan, a, "payload", nan_ok=True)


# ----------------------------------------------------------------------------- audio front end (tests/test_audio_front_elementwise_gpu.py)
# fp32 emulations of the three kernels' own summation orders on the operands of the GPU cases, and planted defects.  These kernels
# store fp32, so their old norm gates (rel_err 1e-6 for the resampler, 1e-5 for the log-mel patches) are sharp: each test below
# states - and asserts - whether that gate, HAD THE SHAPE BEEN RUN, would have seen the defect too.  The record is: it would, for
# every defect here but one (a spectrogram channel that no patch reads, in a segment the old test does not look at).  What the suite lacked was the cases (a ratio with new > 1 going down, inputs shorter than the filter, one
# segment, repeat counts above 2, a clamped start), a check of EVERY element of the spectrogram (the old one looks at frozen
# indices on click audio, most of it on the log floor), and a look at the memory around the outputs; the per-element check adds
# the report of where a defect lies and a gate that does not thin out as the tensor grows.
RESAMPLE_GATE, LOGMEL_GATE = 1e-6, 1e-5          # test_sync_gpu.py / test_edit_gpu.py
DBMEL_GATE = 4 * 4.6e-5                          # test_melspec_db_op: 4 x the restatement's distance from the extractor (dB, max-abs)


def _resample_emul(x, taps, orig, new, width, n_out, drop_last=False, wrong_phase_at=None):
    """resample_sinc_kernel: ntaps sequential fp32 FMAs per output.  drop_last: the bound check reads `i < N - 1`;
    wrong_phase_at: that output takes the taps of phase (o + 1) % new."""
    B, N = x.shape
    o = torch.arange(n_out)
    j = o // new
    p = o - j * new
    if wrong_phase_at is not None:
        p[wrong_phase_at] = (wrong_phase_at + 1) % new
    acc = torch.zeros(B, n_out)
    for t in range(taps.shape[1]):
        i = j * orig - width + t
        ok = (i >= 0) & (i < (N - 1 if drop_last else N))
        xv = torch.where(ok, x[:, i.clamp(0, N - 1)], torch.zeros(()))
        acc = _fma(xv, taps[p, t], acc)
    return acc


@pytest.mark.parametrize("name", list(oc.RESAMPLE_CASES))
def test_resample_emulation_stays_inside(name):
    x, taps, orig, new, width = oc.resample_case(name)
    ref, bound = oc.resample_ref_and_bound(x, taps, orig, new, width)
    assert ref.shape == (x.shape[0], -(-x.shape[1] * new // orig))
    r = oc.assert_elementwise(_resample_emul(x, taps, orig, new, width, ref.shape[1]), ref, bound, name)
    assert r < 0.2, r


def test_resample_reference_is_the_restated_formula_and_zero_where_nothing_is_read():
    """The fp64 reference against test_sync_cpu's conv1d restatement of torchaudio (another formulation of the same sum), and
    mag == 0 - bound 0, the output must be 0 - where every tap meets a zero sample."""
    from test_sync_cpu import _resample_formula
    x, taps, orig, new, width = oc.resample_case("441to160")
    ref, _ = oc.resample_ref_and_bound(x, taps, orig, new, width)
    assert rel_err(_resample_formula(x.double(), 44100, 16000), ref) < 1e-7          # taps rounded to fp32 here, fp64 there
    z = torch.zeros(1, 300)
    z[0, 0] = 1.0
    t3, o, n, w = oc.resample_case("3to1_two_blocks")[1:]
    ref, bound = oc.resample_ref_and_bound(z, t3, o, n, w)
    dead = bound.e[0] == 0
    assert int(dead.sum()) == 100 - 7 and bool((ref[0][dead] == 0).all())           # outputs 0 .. 6 reach sample 0 (width 19, stride 3)
    with pytest.raises(AssertionError, match="1 of 100"):
        bad = ref.clone()
        bad[0, 50] = 1e-30
        oc.assert_elementwise(bad, ref, bound, "a value where nothing may be")


def test_resample_last_sample_dropped_is_caught():
    """`i < N - 1`: the unit impulse at N - 1 vanishes from the outputs whose taps reach it.  The 1e-6 norm gate sees it as well
    (rel_err 0.23 - 0.33: the impulse is most of the signal's energy); the old cases end on quiet click audio."""
    for name in ("3to1_two_blocks", "441to160", "1to3"):
        x, taps, orig, new, width = oc.resample_case(name)
        ref, bound = oc.resample_ref_and_bound(x, taps, orig, new, width)
        bad = _resample_emul(x, taps, orig, new, width, ref.shape[1], drop_last=True)
        assert rel_err(bad, ref) > RESAMPLE_GATE                    # the norm gate would have caught it
        with pytest.raises(AssertionError, match="outside their bound") as ei:
            oc.assert_elementwise(bad, ref, bound, name)
        c0 = int(re.search(r"cols \[(\d+), (\d+)\]", str(ei.value)).group(1))
        assert c0 >= ref.shape[1] - (2 * width + orig) * new // orig - new, str(ei.value)      # offenders lie at the clip's end only


def test_resample_wrong_phase_on_one_output_is_caught():
    """Output o takes the taps of phase (o + 1) % new, on ONE output: impossible to see at new = 1 (the only down-sampling ratio the
    old suite runs), 1 of 1461 elements at 441:160.  rel_err is 5.6e-2 there: the norm gate would have caught it at this shape."""
    x, taps, orig, new, width = oc.resample_case("441to160")
    ref, bound = oc.resample_ref_and_bound(x, taps, orig, new, width)
    bad = _resample_emul(x, taps, orig, new, width, ref.shape[1], wrong_phase_at=torch.tensor([300]))
    assert rel_err(bad, ref) > RESAMPLE_GATE
    with pytest.raises(AssertionError, match=r"x cols \[300, 300\]"):
        oc.assert_elementwise(bad, ref, bound, "phase")
    x1, t1, o1, n1, w1 = oc.resample_case("3to1_two_blocks")       # new = 1: the defect is no defect
    assert torch.equal(_resample_emul(x1, t1, o1, n1, w1, 515, wrong_phase_at=torch.tensor([300])), _resample_emul(x1, t1, o1, n1, w1, 515))


def _dft_emul(fr, basis, halves):
    """The kernels' real DFT: v_mfma_f32_32x32x2_f32 steps of two taps (exact products, one fp32 rounding per step) into an fp32
    accumulator; halves 2: taps [0, n / 2) and [n / 2, n) run as chains of their own and are added at the end (melspec_db_kernel)."""
    n = fr.shape[-1]
    C, Sn = basis[0][:, :513].double(), basis[1][:, :513].double()
    f = fr.double()
    h = n // halves
    re = [torch.zeros(fr.shape[:-1] + (513,)) for _ in range(halves)]
    im = [torch.zeros(fr.shape[:-1] + (513,)) for _ in range(halves)]
    for k in range(0, h, 2):
        for q in range(halves):
            s = slice(q * h + k, q * h + k + 2)
            re[q] = (re[q].double() + f[..., s] @ C[s]).float()
            im[q] = (im[q].double() + f[..., s] @ Sn[s]).float()
    re, im = (t[0] if halves == 1 else t[0] + t[1] for t in (re, im))
    return re * re + im * im


def _mel_emul(pw, tb, lo_shift=None):
    """mel[c] = sum_k pw[lo_c + k] w[c][k] as sequential fp32 FMAs over the table's pitch (weights beyond a triangle are 0).
    lo_shift = (c, d): triangle c starts d bins late."""
    lo = tb["mel_lo"].long().clone()
    if lo_shift is not None:
        lo[lo_shift[0]] += lo_shift[1]
    acc = torch.zeros(pw.shape[:-1] + (lo.numel(),))
    for k in range(int(tb["mel_len"].max())):
        acc = _fma(pw[..., (lo + k).clamp_max(512)], tb["mel_w"][:, k], acc)
    return acc


def _logmel_emul(fr, tb):
    """logmel_kernel from its staged frames fr [G, 65, 400] fp32 -> the normalised spectrogram [G, 128, 66] fp32."""
    mel = _mel_emul(_dft_emul(fr, tb["basis"], 1), tb)
    inv2std = _f(1.0) / (_f(2.0) * _f(4.5689974))
    v = (torch.log(mel + _f(1e-6)) + _f(4.2677393)) * inv2std
    return F.pad(v.transpose(1, 2), (0, 1), value=float(_f(4.2677393) * inv2std))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(oc.LOGMEL_CASES))
def test_logmel_emulation_stays_inside(name, B):
    tb = oc.logmel_tables()
    w = oc.logmel_case(name, B)
    ref, bound, share, a_log, silent = oc.logmel_ref_and_bound(w, tb)
    assert share <= 1e-3 and ref.shape == (B * ((w.shape[1] - 10240) // 5120 + 1), 128, 66)
    got = _logmel_emul(oc.logmel_frames(w), tb)
    r = oc.assert_elementwise(got, ref, bound, f"{name} B {B}")
    assert r < 0.5, r
    assert int(silent.sum()) >= 13
    floor = got.transpose(1, 2)[:, :65][silent]
    assert bool((floor == floor[0, 0]).all())                      # a silent frame: one value in all 128 channels
    # the unrounded reference IS the emulation test_sync_cpu states, before its cast to fp32
    assert float((oc.logmel_emulation(w, tb)[0].double() - ref).abs().max()) < 1e-6
    # and the diffuse gate is meetable: this emulation against the fp32 matmul recipe
    assert rel_err(got, ref) <= 4 * rel_err(oc.logmel_emulation(w, tb, torch.float32)[0], ref)


def _logmel_defect(frames_edit=None):
    """The s3_ragged B = 3 case, its staged frames edited by frames_edit(frames, w16): (emulated spectrogram, ref64, bound)."""
    tb = oc.logmel_tables()
    w = oc.logmel_case("s3_ragged", 3)
    ref, bound, _, _, _ = oc.logmel_ref_and_bound(w, tb)
    fr = oc.logmel_frames(w).clone()
    if frames_edit is not None:
        frames_edit(fr, w)
    return _logmel_emul(fr, tb), ref, bound


def test_logmel_edge_repeat_instead_of_reflect_is_caught():
    """Frame 0 of ONE segment (clip 2, segment 2: it begins right after a stretch of zeros, inside noise) stages sample -i - 1 for
    i < 0 instead of -i.  127 of its 128 elements (of 76 032) leave their bound, by up to 0.5; rel_err 6.7e-3: the 1e-5 norm gate would have caught it.  Where
    the reflect region is silent (clip 2, segment 0: zeros [0, 201)) the defect is invisible to any check: a documented blind spot
    of that input, which is why clip 2's later segments begin in noise."""
    def edit(fr, w):
        i = torch.arange(400) - 200
        fr[8, 0] = w[2, 10240:20480][torch.where(i < 0, -i - 1, i)]
    got, ref, bound = _logmel_defect(edit)
    assert rel_err(got, ref) > LOGMEL_GATE
    with pytest.raises(AssertionError, match="outside their bound") as ei:
        oc.assert_elementwise(got.reshape(9 * 128, 66), ref.reshape(9 * 128, 66), oc.Bound(bound.e.reshape(9 * 128, 66)), "edge repeat")
    assert re.search(r"rows \[10\d\d, 11\d\d\] x cols \[0, 0\]", str(ei.value)), str(ei.value)


def test_logmel_frame_64_from_the_next_segment_is_caught():
    """Frame 64 - alone in the third frame tile - of segment 0 of clip 0 read from segment 1.  rel_err 8.9e-2: the norm gate would
    have caught it."""
    def edit(fr, w):
        fr[0, 64] = fr[1, 64]
    got, ref, bound = _logmel_defect(edit)
    assert rel_err(got, ref) > LOGMEL_GATE
    with pytest.raises(AssertionError, match="outside their bound") as ei:
        oc.assert_elementwise(got.reshape(9 * 128, 66), ref.reshape(9 * 128, 66), oc.Bound(bound.e.reshape(9 * 128, 66)), "frame 64")
    assert re.search(r"rows \[\d+, 1\d\d\] x cols \[64, 64\]", str(ei.value)), str(ei.value)


def test_logmel_patch_element_from_the_next_frame_is_caught_bit_for_bit():
    """One patch element (fi, ti, kf, kt) carries (c, t + 1).  The GPU test compares the patches with mel_out.unfold bit for bit, so
    any such element is reported; rel_err of the patch matrix is 5e-4 for one element of 165 888: the 1e-5 norm gate would have
    caught this one too - unless (c, t) and (c, t + 1) are both on the log floor, where both checks pass and nothing is wrong."""
    got, ref, _ = _logmel_defect()
    patches = got.unfold(1, 16, 10).unfold(2, 16, 10).reshape(-1, 256).contiguous()
    bad = patches.clone()
    fi, ti, kf, kt, g = 7, 3, 5, 9, 7                              # clip 2, segment 1 (clip 1 is silent: every element on the floor)
    bad[(g * 12 + fi) * 6 + ti, kf * 16 + kt] = got[g, 10 * fi + kf, 10 * ti + kt + 1]
    assert rel_err(bad, patches) > LOGMEL_GATE
    with pytest.raises(AssertionError, match=r"1 of \d+ elements differ in their bits; first at \(row %d, col %d\)" % ((g * 12 + fi) * 6 + ti, kf * 16 + kt)):
        oc.assert_bits_equal(bad, patches, "patch")


def _dbmel_tb():
    from foley_amd.host import clap_score
    return clap_score.melspec_tables("cpu", 0.0, 14000.0)


def _dbmel_emul(fr, tb, lo_shift=None):
    """melspec_db_kernel from its frames fr [G, T, 1024] fp32 -> dB [G, T, 64] fp32."""
    mel = _mel_emul(_dft_emul(fr, tb["basis"], 2), tb, lo_shift)
    return torch.where(mel > _f(1e-10), _f(10.0) * torch.log10(mel), _f(-100.0))


def _distinct(wins):
    """Rows of wins without repetitions (the clamped starts repeat a window), in order of first appearance."""
    keep = [i for i in range(wins.shape[0]) if not any(torch.equal(wins[i], wins[j]) for j in range(i))]
    return wins[keep]


@pytest.mark.parametrize("name", list(oc.DBMEL_CASES))
def test_dbmel_emulation_stays_inside(name):
    tb = _dbmel_tb()
    x, starts, wins = oc.dbmel_case(name)
    wins = _distinct(wins)
    ref, bound, share, a_log10, amb = oc.dbmel_ref_and_bound(wins, tb)
    assert share <= 1e-3 and ref.shape == (wins.shape[0], 1001, 64)
    fr = oc.dbmel_frames(wins)
    got = _dbmel_emul(fr, tb)
    r = oc.assert_dbmel(got, ref, bound, amb, name)
    assert r < 0.5, r
    dead = (fr == 0).all(-1)
    assert bool((got[dead] == -100.0).all()) and bool((ref[dead] == -100.0).all())


def test_dbmel_reference_matches_the_restatement():
    """dbmel_ref_and_bound against clap_ref.melspec_fp32 (torch.stft in fp32) on the n1500 window: the two recipes are one."""
    import clap_ref
    from foley_amd.host import clap_score
    _, _, wins = oc.dbmel_case("n1500")
    ref, bound, _, _, _ = oc.dbmel_ref_and_bound(wins, _dbmel_tb())
    rest = clap_ref.melspec_fp32(wins, clap_score.slaney_mel_tables(0.0, 14000.0)[0])
    assert float((rest.double() - ref).abs().max()) < 1e-3


def test_dbmel_seam_off_by_one_and_late_triangle_are_caught():
    """(a) ONE frame of the n1500 window staged with the repeat seam one sample late (p % (seg + 1), the sample past the clip read
    as 0): every sample after the first seam shifts - the frame's 64 values move by up to 0.5 dB.  (b) ONE mel triangle starts one bin
    late in every frame: up to 1.4 dB on one column.  The old dB gate (largest distance from the extractor at most 4 x 4.6e-5 dB) would
    have caught both HAD A CLIP BELOW 4 s BEEN RUN; its two clips have repeat counts 2 and 1."""
    tb = _dbmel_tb()
    x, _, wins = oc.dbmel_case("n1500")
    ref, bound, _, _, amb = oc.dbmel_ref_and_bound(wins, tb)
    sel = torch.arange(8, 14)
    fr = oc.dbmel_frames(wins)[:, sel].clone()
    clean = _dbmel_emul(fr, tb)
    oc.assert_dbmel(clean, ref[:, sel], oc.Bound(bound.e[:, sel]), amb[:, sel], "clean")
    p = torch.arange(1024) + 10 * 480 - 512                        # frame 10 covers padded samples [4288, 5312): seam at 4500
    fr[0, 2] = torch.cat((x[0], torch.zeros(1)))[p % 1501]
    bad = _dbmel_emul(fr, tb)
    assert float((bad - ref[:, sel]).abs().max()) > DBMEL_GATE
    with pytest.raises(AssertionError, match=r"offenders lie in rows \[2, 2\]"):
        oc.assert_dbmel(bad[0], ref[0, sel], oc.Bound(bound.e[0, sel]), amb[0, sel], "seam")
    late = _dbmel_emul(oc.dbmel_frames(wins)[:, sel], tb, lo_shift=(20, 1))
    assert float((late - ref[:, sel]).abs().max()) > DBMEL_GATE
    with pytest.raises(AssertionError, match=r"x cols \[20, 20\]"):
        oc.assert_dbmel(late[0], ref[0, sel], oc.Bound(bound.e[0, sel]), amb[0, sel], "triangle")


def test_logmel_channel_127_is_seen_by_no_patch_and_caught_per_element():
    """Channels 126 and 127 of the spectrogram reach no patch (12 patches of 16 at stride 10 end at channel 125), and the old test
    compares mel_out at three frozen segments only.  Channel 127 of ANOTHER segment shifted by one frame leaves the patch matrix
    bit for bit as it was - the old 1e-5 norm gate on the patches reads 0 - and fails the per-element check on that one row: the
    one planted defect here that the old gates would have MISSED at any shape."""
    got, ref, bound = _logmel_defect()
    bad = got.clone()
    bad[7, 127, :64] = got[7, 127, 1:65]
    unfold = lambda m: m.unfold(1, 16, 10).unfold(2, 16, 10).reshape(-1, 256)
    assert rel_err(unfold(bad), unfold(got)) == 0.0 < LOGMEL_GATE
    with pytest.raises(AssertionError, match=r"offenders lie in rows \[1023, 1023\]"):
        oc.assert_elementwise(bad.reshape(9 * 128, 66), ref.reshape(9 * 128, 66), oc.Bound(bound.e.reshape(9 * 128, 66)), "channel 127")
