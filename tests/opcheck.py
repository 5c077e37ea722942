"""Per-element error bounds and guard bands for the op-level kernel tests.

The norm gates of test_ops_gpu.py / test_pairs_gpu.py (conftest.rel_err against a per-dtype tolerance) average an error over the
whole tensor: a wrong tile corner, a K slice skipped on a few rows or a bias missed on one column vanish in them.  The checks
here hold EVERY element against a bound that is derived from the arithmetic (never from what a kernel was seen to do), and
look at the memory around an output.

Conventions
    ref64     the fp64 result computed from the operands AS ROUNDED to the compute dtype (16-bit operands are exact in fp64).
    U32       2^-23: the fp32 unit round-off (2^-24) doubled, so that a bound also holds for an accumulator that truncates.
    U16       per-rounding relative error taken for a value rounded once to a 16-bit type: 2^-9 (bf16), 2^-12 (fp16) - half
              the worst-case unit round-off (2^-8 / 2^-11), which the terms below may use because each of them multiplies it
              with a magnitude (`mag`, P @ |V|) that bounds the rounded value by its sum of absolute products, not by the value.
    output    a 16-bit store adds half an ulp of max(|ref|, |got|) in that type, times (1 + 2^-6) for the double rounding
              of an fp32 value that sits on a tie (fp16: ulp never below the subnormal spacing 2^-24).

GEMM accumulation term: e_y = (K + 4) * U32 * mag, mag = |A| @ |W|^T + |bias| - the deterministic worst case of K fp32
additions in ANY order (split-K, K-origin rotation, atomics, tap fusion), plus the bias add and the epilogue's own roundings.
"""
import functools
import math

import torch

from conftest import record_parity, rel_err  # noqa: F401  (re-exported: the test files import them from here or conftest)

U32 = 2.0 ** -23
U16 = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
MANT = {torch.bfloat16: 8, torch.float16: 11}      # significand bits, the implicit one included
LIP_SILU, LIP_GELU = 1.1, 1.13                     # Lipschitz constants: max |silu'| = 1.0998, max |gelu'| = 1.129
LIP_SNAKE = 2.0                                    # snake(v) = v + sin(a v)^2 / a: |1 + sin(2 a v)| <= 2 for every a
A_ACT_ERF16 = 8e-7                                 # common.h::gelu_erf_fast, absolute (test_exact_gelu_fast_form_error_bound)
GUARD_BITS = {4: 0x5A5A5A5A, 2: 0x5A5A, 1: 0x5A}   # finite, non-NaN in fp32 (1.5e16), bf16 (1.5e16), fp16 (203.25)
_INT = {4: torch.int32, 2: torch.int16, 1: torch.int8}


# ----------------------------------------------------------------------------- ulps and the output term
def ulp16(x, dtype):
    """Spacing of the 16-bit `dtype` at |x| (fp64 tensor): 2^(floor(log2 |x|) - (mant - 1)); fp16 never below its subnormal
    spacing 2^-24, bf16 (8 exponent bits) never below 2^-133."""
    x = x.double().abs()
    _, e = torch.frexp(x.clamp_min(1e-300))          # |x| = m * 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(x), e - MANT[dtype])
    return ulp.clamp_min(2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133)


def output_term(ref, got, out_dtype):
    """Error a correctly rounded store of the exact fp32 result may add: 0 for fp32 (covered by the accumulation term)."""
    if out_dtype not in MANT:
        return torch.zeros_like(ref, dtype=torch.float64)
    return 0.5 * (1 + 2.0 ** -6) * ulp16(torch.maximum(ref.double().abs(), got.double().abs()), out_dtype)


class Bound:
    """An absolute per-element bound `e` (fp64) on the value BEFORE the store, plus the store's type."""

    def __init__(self, e, out_dtype=torch.float32):
        self.e, self.out_dtype = e, out_dtype

    def total(self, ref, got):
        return self.e + output_term(ref, got, self.out_dtype)


# ----------------------------------------------------------------------------- GEMM
def gemm_ref64(A, W, bias=None):
    """(ref64, mag) of y = A @ W^T + bias from the operands as given (already rounded to the compute dtype), in fp64."""
    A, W = A.double().cpu(), W.double().cpu()
    ref, mag = A @ W.t(), A.abs() @ W.abs().t()
    if bias is not None:
        b = bias.double().cpu()
        ref, mag = ref + b, mag + b.abs()
    return ref, mag


def conv3_cols(x):
    """x [B, L, C] -> the [B*L, 3C] rows a channels-last conv k = 3, pad 1 multiplies with packers.conv_to_gemm(w) (K = tap*C + c)."""
    B, L, C = x.shape
    p = torch.nn.functional.pad(x, (0, 0, 1, 1))
    return torch.cat((p[:, :L], p[:, 1:L + 1], p[:, 2:L + 2]), dim=-1).reshape(B * L, 3 * C)


def elementwise_gemm_bound(A, W, bias, K, out_dtype=torch.float32, extra=None, mag=None):
    """Bound on y = A @ W^T + bias accumulated in fp32 in any order: (K + 4) * U32 * mag (+ extra), stored as out_dtype.
    `mag` may be passed when gemm_ref64 already computed it (the 4000-row cases share it across dtypes)."""
    if mag is None:
        _, mag = gemm_ref64(A, W, bias)
    e = (K + 4) * U32 * mag
    if extra is not None:
        e = e + extra
    return Bound(e, out_dtype)


def gated_residual_bound(e_y, gate, x0, y):
    """x0 + g * y in fp32: |g| * e_y + U32 * (|x0| + |g * y|)."""
    g = gate.double().abs()
    return Bound(g * e_y + U32 * (x0.double().abs() + g * y.double().abs()))


def slab_bound(e_y, mag, ks, slab_dtype):
    """Sum over the ks deferred split-K slabs against y - bias (e_y, mag computed WITHOUT the bias): e_y for fp32 slabs; 16-bit
    slabs add ks * U16 * mag - each partial is bounded by mag and rounded once."""
    return Bound(e_y + (ks * U16[slab_dtype] * mag if slab_dtype in U16 else 0.0))


def act64(name, y):
    y = y.double()
    if name == "silu":
        return y * torch.sigmoid(y)
    return torch.nn.functional.gelu(y, approximate="tanh" if name == "gelu" else "none")


def measure_a_act(name, y64, dev):
    """4 x the largest |PyTorch's fp32 device activation of fp32(y) - the fp64 activation of y|: reference against reference
    (the factor 4 covers one more approximate instruction each for the exponential and the reciprocal of a fast form)."""
    y32 = y64.float().to(dev)
    if name == "silu":
        a32 = torch.nn.functional.silu(y32)
    else:
        a32 = torch.nn.functional.gelu(y32, approximate="tanh" if name == "gelu" else "none")
    return 4.0 * float((a32.double().cpu() - act64(name, y64)).abs().max())


def act_bound(name, e_y, a_act, out_dtype):
    """act(y): Lipschitz constant of the activation times e_y, plus the activation's own error a_act."""
    return Bound((LIP_SILU if name == "silu" else LIP_GELU) * e_y + a_act, out_dtype)


def silugate_bound(a, b, e_a, e_b, a_act, out_dtype):
    """silu(a) * b: |silu(a)| e_b + 1.1 |b| e_a, and - beyond that first-order expression, each needed and tiny against it - the
    second-order product 1.1 e_a e_b, the activation's error a_act scaled by the factor it multiplies (|b| + e_b, not 1), and the
    fp32 product's own rounding U32 |silu(a) b|."""
    sa, bb = act64("silu", a).abs(), b.double().abs()
    return Bound(sa * e_b + LIP_SILU * bb * e_a + LIP_SILU * e_a * e_b + a_act * (bb + e_b) + U32 * sa * bb, out_dtype)


def snake64(v, alpha):
    """DAC snake in fp64: v + sin(alpha v)^2 / (alpha + 1e-9), alpha broadcast over the last (channel) dimension."""
    v, a = v.double(), alpha.double()
    return v + torch.sin(a * v) ** 2 / (a + 1e-9)


def measure_a_act_snake(v64, alpha, dev):
    """4 x the largest |PyTorch's fp32 device snake of fp32(v) - the fp64 snake of v| (reference against reference, as measure_a_act)."""
    v32, a32 = v64.float().to(dev), alpha.float().to(dev)
    s32 = v32 + (1.0 / (a32 + 1e-9)) * torch.sin(a32 * v32) ** 2
    return 4.0 * float((s32.double().cpu() - snake64(v64, alpha)).abs().max())


def dac_bounds(e_y, v, res, a_act):
    """DAC residual epilogue (fp32 only): out0 = v = y (+ res), out1 = snake(v).  out0: e_y, plus one fp32 addition U32 (|res| + |v|)
    when a residual is added; out1: the snake's Lipschitz constant 2 times that, plus the activation's own error a_act."""
    e_v = e_y + (U32 * (res.double().abs() + v.double().abs()) if res is not None else 0.0)
    return Bound(e_v), Bound(LIP_SNAKE * e_v + a_act)


def head_split_bound(e_y, y_head, out_dtype, gain=None):
    """RMSNorm (+ RoPE, a rotation of pairs: it moves an error vector without stretching it beyond the two partners' sum) of a
    128-wide head: the GEMM term pushed through the norm, 2 * e_y / rms per element, times |gain|; V (gain None) passes e_y
    through unchanged.  Two departures from the plain '2 e_y / rms per element', both needed for the bound to be true: e_y is
    the head's LARGEST (RoPE mixes an element with its pair partner, the rms with all 128), and 8 U32 |gain| max|y| / rms covers
    the fp32 roundings of the norm, the gain and the rotation themselves (at e_y ~ 1e-3 it is four orders below the first term)."""
    return Bound(head_split_pre_bound(e_y, y_head, gain), out_dtype)


def head_split_pre_bound(e_y, y_head, gain=None):
    """The part of head_split_bound BEFORE the final rounding to the output type: the bound on the fp32 value a head-split
    epilogue holds in registers (what the fused cross attention rounds to 16 bit on chip, cross_attention_ref_and_bound)."""
    if gain is None:
        return e_y
    rms = y_head.double().pow(2).mean(-1, keepdim=True).sqrt()
    g = float(gain.double().abs().max())
    return (2.0 * g * e_y.amax(-1, keepdim=True) / rms).expand_as(e_y).clone() + 8 * U32 * g * (y_head.double().abs() / rms).amax(-1, keepdim=True)


# ----------------------------------------------------------------------------- the check
def assert_elementwise(got, ref64, bound, what):
    """Every element of `got` within `bound` (a Bound, a tensor or a number) of ref64.  A failure reports the count of offending
    elements, the worst (row, col) with its got / ref / bound, and the bounding box of all offenders (what tells a tile edge from
    a stray lane); NaN offends.  Returns the largest err / bound."""
    got, ref = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if isinstance(bound, Bound):
        b = bound.total(ref, got)
    else:
        b = torch.as_tensor(bound, dtype=torch.float64)
    b = b.expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= b)
    if bool(bad.any()):
        cols = ref.shape[-1] if ref.dim() else 1
        bad2, ratio = bad.reshape(-1, cols), torch.nan_to_num(err / b.clamp_min(1e-300), nan=float("inf")).reshape(-1, cols)
        idx = bad2.nonzero()
        r0, c0 = (int(v) for v in idx.min(0).values)
        r1, c1 = (int(v) for v in idx.max(0).values)
        w = int(ratio.argmax())
        wr, wc = divmod(w, cols)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; worst at (row {wr}, col {wc}) of "
            f"[{bad2.shape[0]}, {cols}]: got {float(got.reshape(-1, cols)[wr, wc])!r} ref {float(ref.reshape(-1, cols)[wr, wc])!r} "
            f"bound {float(b.reshape(-1, cols)[wr, wc]):.3e} (err / bound {float(ratio[wr, wc]):.3g}); offenders lie in rows "
            f"[{r0}, {r1}] x cols [{c0}, {c1}]")
    return float((err / b.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ----------------------------------------------------------------------------- guard bands
class Guarded:
    """A [rows, cols] interior (NaN-filled, row pitch cols + pad_cols) inside a larger buffer filled with a fixed non-NaN bit
    pattern: `before` / `after` guard rows (or guard slabs: a row is everything but the leading dimension) and pad columns.
    `view` is the interior to launch into (its data_ptr() and `pitch` go into the descriptor), check() asserts that every guard
    word is bit-identical afterwards (compared through an integer view)."""

    def __init__(self, shape, dtype, dev, rows=(2, 3), pad_cols=0, misalign=0, fill=float("nan")):
        lead, rest = shape[0], tuple(shape[1:])
        inner = 1
        for s in rest:
            inner *= s
        self.pitch = inner + pad_cols
        es = torch.empty((), dtype=dtype).element_size()
        self.n0 = rows[0] * self.pitch + misalign
        total = self.n0 + lead * self.pitch + rows[1] * self.pitch
        self.ibuf = torch.full((total,), GUARD_BITS[es], dtype=_INT[es], device=dev)
        self.buf = self.ibuf.view(dtype)
        self.view = torch.as_strided(self.buf, (lead,) + rest, (self.pitch,) + tuple(torch.empty(rest).stride()), self.n0)
        self.view.fill_(fill)
        mask = torch.ones(total, dtype=torch.bool, device=dev)
        torch.as_strided(mask, (lead, inner), (self.pitch, 1), self.n0).fill_(False)
        self.mask, self.bits, self.lead, self.inner = mask, GUARD_BITS[es], lead, inner

    def check(self, what="guard"):
        hit = (self.ibuf != self.bits) & self.mask
        if bool(hit.any()):
            at = hit.nonzero().flatten().cpu() - self.n0
            r, c = at // self.pitch, at % self.pitch       # floor division: rows before the interior are negative
            raise AssertionError(
                f"{what}: {at.numel()} guard words overwritten around the [{self.lead}, {self.inner}] interior (pitch {self.pitch}); "
                f"rows [{int(r.min())}, {int(r.max())}] x cols [{int(c.min())}, {int(c.max())}], first at (row {int(r[0])}, col {int(c[0])})")


def guarded(shape, dtype, dev, rows=(2, 3), pad_cols=0, misalign=0, fill=float("nan")):
    return Guarded(shape, dtype, dev, rows, pad_cols, misalign, fill)


# ----------------------------------------------------------------------------- LayerNorm (+ pending split-K slabs)
def layernorm_ref_and_bound(x0, shift, scale, eps, out_dtype, slabs=None, bias=None, gate=None):
    """fp64 reference and per-element bounds of  x = x0 + gate * (sum_s slabs[s] + bias)  (written back in place) and
    out = (x - mean) * rstd * (1 + scale) + shift  from the fp32 inputs; all arguments fp64-convertible CPU tensors broadcastable
    to [M, D] (slabs [k, M, D]).  Returns (x64, out64, bound_x, bound_out).

    Derivation (u = U32; c = D / 64 + 8 is the longest chain of fp32 additions a row reduction of either kernel form has: a lane
    sums its D / 64 elements one after the other, the butterfly over 64 lanes adds 6 levels, the two-wave form one more, the
    division by D one rounding - a reduction of depth c has an error of at most c u sum|terms|):
        e_x   = (k + 3) u (|x0| + |g| (sum|slab| + |bias|))      k + 1 sequential adds, the product with g, the add to x0
        d_m   = c u mean|x| + mean(e_x)                          the mean
        e_d   = d_m + e_x + u |x - mean|                         one centred element
        d_var = (c + 4) u var + 2 mean(|d| e_d) + mean(e_d^2)    squares, their reduction, the division
        d_r   = d_var / (2 (var + eps) (1 - d_var / (var + eps))) + 3 u      relative, on rstd (add eps, sqrt, reciprocal)
        e_out = (e_d rstd + |xhat| (d_r + 4 u)) (1 + |scale|) + u |out|
    With rows of 1e3 + N(0, 1) the leading term is d_m ~ 32 * 1.2e-7 * 1e3 = 4e-3: a one-pass variance (error ~ 1e6 u D) or a
    neighbour's mean (|difference| ~ 0.04) lie far outside, the reduction order of either kernel form inside.
    This departs from a bound c u |xhat| (1 + |scale|) with c = D: that expression is zero at xhat = 0, where the rounding of the
    mean (absolute, ~ u |mean|) still lands, so no fp32 kernel meets it at |x| ~ 1e3.  Two limits follow and are meant to be known:
    (1) c is read from TODAY's reduction shape (rowops.hip: D / 64 elements per lane, a 64-lane butterfly, two waves at most).  A
    kernel that legitimately lets a lane sum more elements raises its own worst case above this c (MI355X uses 0.54 of the bound
    now): c must then be re-derived from the new data path, not scaled to fit.  (2) At |x| ~ 1e3 the bound is ~ 4e-3 ABSOLUTE, so
    for an fp32 output it is weaker than the 1e-4 norm gate of test_ln_mod_width for an error spread over the whole tensor; what
    it adds is the localised defect (one row, one lane's columns), the written-back x and the guards.  The norm gates stay."""
    x0 = x0.double()
    M, D = x0.shape
    u, c = U32, D / 64 + 8
    if slabs is not None:
        k = slabs.shape[0]
        s, g = slabs.double(), gate.double().expand(M, D)
        b = bias.double().expand(M, D) if bias is not None else torch.zeros(M, D, dtype=torch.float64)
        x = x0 + g * (s.sum(0) + b)
        e_x = (k + 3) * u * (x0.abs() + g.abs() * (s.abs().sum(0) + b.abs()))
    else:
        x, e_x = x0, torch.zeros_like(x0)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = d.pow(2).mean(-1, keepdim=True)
    d_m = c * u * x.abs().mean(-1, keepdim=True) + e_x.mean(-1, keepdim=True)
    e_d = d_m + e_x + u * d.abs()
    d_var = (c + 4) * u * var + 2 * (d.abs() * e_d).mean(-1, keepdim=True) + e_d.pow(2).mean(-1, keepdim=True)
    rel = d_var / (var + eps)
    d_r = torch.where(rel < 0.5, 0.5 * rel / (1 - rel.clamp_max(0.5)), torch.full_like(rel, float("inf"))) + 3 * u
    rstd = torch.rsqrt(var + eps)
    xhat = d * rstd
    sc = scale.double().expand(M, D) if scale is not None else torch.zeros(M, D, dtype=torch.float64)
    sh = shift.double().expand(M, D) if shift is not None else torch.zeros(M, D, dtype=torch.float64)
    out = xhat * (1 + sc) + sh
    e_out = (e_d * rstd + xhat.abs() * (d_r + 4 * u)) * (1 + sc.abs()) + u * out.abs()
    return x, out, Bound(e_x + u * x.abs()), Bound(e_out, out_dtype)


# ----------------------------------------------------------------------------- attention
def attention_ref_and_bound(q, k, v, out_dtype, p_dtype=None):
    """softmax(q k^T / sqrt(hd)) v in fp64 from the operands as rounded (q [B, H, Sq, hd], k / v [Bk, H, Skv, hd], Bk divides B:
    batch b reads k / v entry b // (B / Bk)), as [B, Sq, H * hd], with the bound
        (c_p u_p + 2 d_s) (P @ |V|)  (+ output term),
    d_s = (hd + 4) U32 max_keys(|q| . |k|) / sqrt(hd) the worst-case error of a score (hd fp32 additions in any order), felt once
    in the numerator and once in the row sum; u_p the rounding of a probability to the operand type before the P V MFMA.
    Read from attention.hip: every 16-bit kernel (attn_bf16 / lds / wide / long / pair) rounds P ONCE, right after the
    exponential (to_carrier), and sums the row from the UNROUNDED fp32 values, so c_p = 1 and u_p = U16[p_dtype]; the fp32 kernel
    rounds nothing: c_p = 1 with u_p = U32.  (attn_bf16_wide_kernel at head dim 64 in bf16 also multiplies V with the rounding's
    residual, so its P carries ~ 2^-16; the bound does not count on it.)
    NOT rigorous for the fp32 kernel (and, to a lesser degree, the others): the expression leaves out the Skv fp32 additions of the
    P V product and of the row sum (worst case (Skv + 4) U32 P @ |V|: 4e-4 at Skv = 3480 against 2 d_s ~ 2e-4) and the error of the
    exponential.  It holds in practice because those errors add like a random walk while d_s is a worst case (MI355X: fp32 kernel at
    7e-3 of the bound); a kernel that exceeds it on long keys with a clean score path must be judged against the full expression."""
    B, H, Sq, hd = q.shape
    div = B // k.shape[0]
    u_p = U16[p_dtype] if p_dtype in U16 else U32
    ref = torch.empty(B, Sq, H * hd, dtype=torch.float64)
    e = torch.empty_like(ref)
    for b in range(B):
        qb, kb, vb = q[b].double(), k[b // div].double(), v[b // div].double()
        s = qb @ kb.transpose(1, 2) / math.sqrt(hd)
        d_s = (hd + 4) * U32 * (qb.abs() @ kb.abs().transpose(1, 2)).amax(-1, keepdim=True) / math.sqrt(hd)
        p = torch.softmax(s, -1)
        ref[b] = (p @ vb).transpose(0, 1).reshape(Sq, H * hd)
        e[b] = ((u_p + 2 * d_s) * (p @ vb.abs())).transpose(0, 1).reshape(Sq, H * hd)
    return ref, Bound(e, out_dtype)


def grouped_attention_ref_and_bound(q, k, v, grp_q, grp_kv, out_dtype, p_dtype=None):
    """Block-diagonal attention in fp64 from the operands as rounded: q [G, H, Sq, hd], k / v [G, H, Skv, hd]; query t of a sequence
    sees keys [(t // grp_q) grp_kv, (t // grp_q + 1) grp_kv) only - the last group may be ragged (fewer than grp_q queries), keys
    beyond the last group are seen by nobody.  attention_ref_and_bound applied group by group; returns ([G, Sq, H hd], Bound)."""
    G, H, Sq, hd = q.shape
    ref = torch.empty(G, Sq, H * hd, dtype=torch.float64)
    e = torch.empty_like(ref)
    for i in range((Sq + grp_q - 1) // grp_q):
        qs, ks = slice(i * grp_q, min((i + 1) * grp_q, Sq)), slice(i * grp_kv, (i + 1) * grp_kv)
        assert ks.stop <= k.shape[2], "every query group's keys lie inside Skv"
        r, b = attention_ref_and_bound(q[:, :, qs], k[:, :, ks], v[:, :, ks], out_dtype, p_dtype)
        ref[:, qs], e[:, qs] = r, b.e
    return ref, Bound(e, out_dtype)


def round16(x, dtype):
    """An fp64 tensor rounded to the 16-bit `dtype` (through fp32, as torch converts), back in fp64."""
    return x.double().float().to(dtype).double()


def rounding_span16(x, e, dtype):
    """For a value known to lie within `e` of the fp64 `x` and then rounded to the 16-bit `dtype`: (lo, hi), the smallest and
    largest results the rounding can give (rounding is monotone).  e is widened by 2^-23 |x| + 1e-30 so that the fp32 step of
    round16 cannot hide a boundary.  lo == hi: the rounded value is known exactly, whatever fp32 value the kernel held."""
    x, e = x.double(), torch.as_tensor(e, dtype=torch.float64) + U32 * x.double().abs() + 1e-30
    return round16(x - e, dtype), round16(x + e, dtype)


def cross_attention_ref_and_bound(q64, e_q, k, v, sets, dtype):
    """The cross attention fused into the q projection's head-split epilogue (gemm_common.h, EPI_QKV_ATTN), head dim 128.
        q64   [M, H, 128] fp64: q BEFORE its rounding to the operand type, RoPE(RMSNorm(x W^T + b))
        e_q   [M, H, 128] bound on the kernel's fp32 q against q64 (head_split_pre_bound)
        k, v  [sets, H, Skv, 128] as rounded to the operand type `dtype`; sets [M]: the text set of each row, (row // L) // bdiv
    Returns (ref64 [M, H 128], Bound, ambiguous share of the q elements).

    The kernel rounds q to 16 bit on chip, so the reference's rounded q may differ from the kernel's.  An element is AMBIGUOUS when
    q64 lies within e_q of a rounding boundary of the type, i.e. when round(q64 - e_q) != round(q64 + e_q) (rounding_span16).  An
    unambiguous element is the same number in the kernel and here and adds nothing.  An ambiguous element d may land on the
    neighbouring value, ulp16(q_d) away, and moves score j by at most ulp16(q_d) |k_jd| / sqrt(128):
        d_s' = d_s + max_j sum_{d ambiguous} ulp16(q_d) |k_jd| / sqrt(128),       d_s as in attention_ref_and_bound
        bound = (u_p + 2 d_s') (P @ |V|)  (+ output term),                          u_p = U16[dtype]
    u_p enters once, read from the code: the epilogue rounds a probability ONCE, right after the exponential (to_carrier, the B
    operand of the P V MFMA), and adds the UNROUNDED fp32 value into l_run; the accumulators are rescaled in fp32.
    Left out, as in attention_ref_and_bound: the <= 96 fp32 additions of P V and of the row sum (worst case 100 U32 P @ |V| = 1.2e-5
    P @ |V|, against u_p >= 2.4e-4), the error of v_exp_f32 (1 ulp of fp32), and the second order of the score error, (2 d_s')^2 / 2
    (below 1e-6 of P @ |V| in the dyadic cases, where d_s' < 1e-3).  One ulp per ambiguous element is exact while e_q stays below
    half an ulp - every dyadic case, where the span of the two roundings IS one ulp (asserted in test_opcheck_cpu.py).  In the
    general form (random operands at K = 1536) the worst-case e_q reaches a few bf16 ulps; the expression then presumes that the
    kernel's fp32 q lies within one ulp of q64, which a real accumulation (~ 1e-2 of its worst case) does by a wide margin."""
    M, H, hd = q64.shape
    q64, e_q = q64.double(), e_q.double().expand_as(q64)
    lo, hi = rounding_span16(q64, e_q, dtype)
    qr = round16(q64, dtype)
    amb = hi != lo
    dq = torch.where(amb, ulp16(qr, dtype), torch.zeros_like(qr))       # 0 where unambiguous
    share = float(amb.double().mean())
    ref = torch.empty(M, H, hd, dtype=torch.float64)
    e = torch.empty_like(ref)
    sets = torch.as_tensor(sets).long()
    for t in sets.unique().tolist():
        rows = (sets == t).nonzero().flatten()
        kk, vv, qq, dd = k[t].double(), v[t].double(), qr[rows], dq[rows]          # [H, Skv, 128], [n, H, 128]
        s = torch.einsum("mhd,hjd->mhj", qq, kk) / math.sqrt(hd)
        d_s = (hd + 4) * U32 * torch.einsum("mhd,hjd->mhj", qq.abs() + dd, kk.abs()).amax(-1, keepdim=True) / math.sqrt(hd)
        slack = torch.einsum("mhd,hjd->mhj", dd, kk.abs()).amax(-1, keepdim=True) / math.sqrt(hd)
        p = torch.softmax(s, -1)
        ref[rows] = torch.einsum("mhj,hjd->mhd", p, vv)
        e[rows] = (U16[dtype] + 2 * (d_s + slack)) * torch.einsum("mhj,hjd->mhd", p, vv.abs())
    return ref.reshape(M, H * hd), Bound(e.reshape(M, H * hd), dtype), share


def both16(t):
    """Round to bf16 and flush what fp16 cannot hold exactly (|x| < 2^-17): the result is exact in bf16 AND fp16."""
    t = t.to(torch.bfloat16).float()
    t = torch.where(t.abs() < 2.0 ** -17, torch.zeros_like(t), t)
    assert torch.equal(t.to(torch.float16).float(), t)
    return t


ATTN_SCORE_CLASSES = ("rise", "first", "last_half", "hole")


@functools.lru_cache(maxsize=4)
def attn_edge_operands(ops, B, H, Sq, Skv, hd, div, seed, f32=False):
    """q [B, H, Sq, hd], k / v [B // div, H, Skv, hd] of an attention edge case (tests/test_attention_edges_gpu.py and the emulation
    checks of tests/test_opcheck_cpu.py share them): fp32 tensors, exact in bf16 AND fp16 unless f32 - one fp64 reference serves
    both 16-bit types.  Every (batch, head) entry of k and v is drawn on its own, so shared entries (div > 1) are distinct.
    ops = 'rand': i.i.d. normal.
    ops = 'onoff': every probability is 1 or ~ e^-12 before the division by the row sum, so the rounding of P to 16 bits costs
    nothing and the case is fair at ANY key count (u_p is HALF the unit round-off, an allowance that rests on a row averaging over
    many rounded probabilities: with two i.i.d. keys the once-rounded arithmetic itself reaches 1.3 of the bound, see
    tests/test_opcheck_cpu.py::test_attention_edge_inputs_are_fair).  Even queries carry q[..., 0] = 8, odd ones q[..., 1] = 8;
    k[..., 0] and k[..., 1] are 0 (the key is ON for those queries: score exactly 0) or -12 sqrt(hd) / 8 (OFF: score -12), drawn per
    key; q is otherwise non-zero in dimensions [2, hd / 2) only and k in [hd / 2, hd): their products vanish unless a kernel pairs
    the wrong dimensions.  A query with no ON key sees equal scores, again exact.
    Else a score class: dimension 0 carries a profile t[key] (q[..., 0] = 8 and
    k[..., 0] = t sqrt(hd) / 8, so the score is t[key] plus noise), the other dimensions i.i.d. normal / 2 (noise of ~ 0.25 in the
    score; with |t| <= 32 the bound's d_s stays below 3e-4):
        rise       t steps up by 1.5 from one 32-key block to the next, centred on 0 (|t| <= 13 at 18 blocks): the running maximum
                   rises in every key tile of every kernel (32- and 64-key tiles, the four key runs, each key half of the pair kernel),
                   the ragged last tile included, and a block weighs e^-1.5 of the next, so a row still averages over ~ 40 keys.
                   Every third query carries q[..., 0] = -8: its maximum is in the FIRST block, so the lanes of one wave disagree
                   about the rescale.
        first      t = 10 in the first 32-key block, -5 behind it: no later tile raises the maximum.
        last_half  t = 0 but t[Skv - 1] = ln(Skv - 1): the last key carries about half of each row's weight.
        hole       t = 31, but t = -32 in one tile in the middle (64 keys from 64 (n64 // 2); 32 keys from 32 (n32 // 2) where fewer
                   than three 64-key tiles exist): 63 below the maximum, its probabilities are 0 in fp16 and ~ 1e-27 in bf16."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rnd(B, H, Sq, hd), rnd(B // div, H, Skv, hd), rnd(B // div, H, Skv, hd)
    if ops == "onoff":
        q, k = q * 0.5, k * 0.5
        q[..., :2], q[..., hd // 2:], k[..., :hd // 2] = 0.0, 0.0, 0.0
        q[:, :, 0::2, 0] = 8.0
        q[:, :, 1::2, 1] = 8.0
        k[..., :2] = torch.where(torch.rand(B // div, H, Skv, 2, generator=g) < 0.5, 0.0, -12.0 * math.sqrt(hd) / 8.0)
    elif ops != "rand":
        assert ops in ATTN_SCORE_CLASSES, ops
        key, n32, n64 = torch.arange(Skv), (Skv + 31) // 32, (Skv + 63) // 64
        if ops == "rise":
            t = 1.5 * ((key // 32).double() - (n32 - 1) / 2)
        elif ops == "first":
            t = torch.where(key < 32, 10.0, -5.0).double()
        elif ops == "last_half":
            t = torch.zeros(Skv, dtype=torch.float64)
            t[-1] = math.log(max(Skv - 1, 1))
        else:
            lo, w = (64 * (n64 // 2), 64) if n64 >= 3 else (32 * (n32 // 2), 32)
            t = torch.where((key >= lo) & (key < lo + w), -32.0, 31.0).double()
        q, k = q * 0.5, k * 0.5
        q[..., 0] = 8.0
        if ops == "rise":
            q[:, :, 2::3, 0] = -8.0
        k[..., 0] = (t * math.sqrt(hd) / 8.0).float()
    if not f32:
        q, k, v = both16(q), both16(k), both16(v)
    return q, k, v


def head_q64(y, gain, cos, sin, eps):
    """RoPE(RMSNorm(y)) in fp64: y [M, H, 128], gain [128], cos / sin [M, 64] (the table rows of each row's position)."""
    y = y.double()
    q = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + f32(eps)) * gain.double()
    return rope64(q, cos.double()[:, None], sin.double()[:, None])


def cross_dyadic_case(Bc, L, H, bdiv, Skv, seed, k_scale=1.0, K=256, v_floor=0.0):
    """Operands of a SHARP case of the fused cross attention: Bc batch rows of L tokens (M = Bc L), text set (row // L) // bdiv.
    Everything lies on a coarse dyadic grid so that the projection is exact in fp32 in ANY order (e_y = 0) and only the roundings
    of RMSNorm and RoPE remain before q is rounded to 16 bit; and |q| is nearly uniform, because an element is ambiguous with
    probability ~ 2 e_q / ulp16(q) and e_q (head_split_pre_bound) is relative to the head's LARGEST element: Gaussian q (many
    small elements, whose ulp is small) would be ambiguous in 5 % of its fp16 elements.  So:
        A     +- a_m, a_m in {1/2, 1, 2} by row, random signs per element
        W     one entry +- 1/2 per row, column (37 n + 11) mod K: y[m, n] = +- a_m / 2, signs random per (m, n)
        bias  +- 1/32: two magnitudes per row, 1.29 apart at most
        RoPE  a table of QUARTER TURNS, (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)} drawn per (position, pair): the rotation
              swaps and negates partners (different gains: a wrong partner, sign or table row shows) and never makes an element small
        gain  1 + 0.1 N(0, 1), positions 2 l (table rows 0, 2, 4, ...)
        K, V  N(0, k_scale^2) and N(0, 1), exact in bf16 and fp16: |q|^2 = 128, so a score is ~ N(0, k_scale^2)
              v_floor > 0: |v| >= v_floor (sign(n) (|n| + v_floor)).  For the one-hot rows of the large-score case: there an output
              element is ONE v value plus probabilities of ~ 1e-6, which fp16 holds as subnormals - rounded to an ABSOLUTE 2^-25, not
              to the relative u_p of the bound.  Where that v is 0 the output is nothing but such terms and the CPU emulation
              (test_opcheck_cpu.py, no kernel involved) lands at 1.85 of the bound; away from 0 they vanish under the output's ulp.
    Returns a dict (fp32 tensors exact in both 16-bit types; y64, q64 [M, H, 128], e_q, sets [M])."""
    g = torch.Generator().manual_seed(seed)
    M, N = Bc * L, H * 128
    sgn = lambda *shape: torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    a_m = torch.tensor([0.5, 1.0, 2.0])[torch.arange(M) % 3]
    A = sgn(M, K) * a_m[:, None]
    W = torch.zeros(N, K)
    W[torch.arange(N), (37 * torch.arange(N) + 11) % K] = 0.5 * sgn(N)
    b = sgn(N) / 32
    gain = 1 + 0.1 * torch.randn(128, generator=g)
    turn = torch.randint(0, 4, (2 * L + 1, 64), generator=g)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
    pos = (2 * torch.arange(L)).to(torch.int32)
    nsets = (Bc + bdiv - 1) // bdiv
    k = both16(torch.randn(nsets, H, Skv, 128, generator=g) * k_scale)
    v = torch.randn(nsets, H, Skv, 128, generator=g)
    v = both16(torch.where(v < 0, v - v_floor, v + v_floor))
    y64 = (A.double() @ W.double().t() + b.double()).view(M, H, 128)
    pl = pos.long().repeat(Bc)
    q64 = head_q64(y64, gain, cos[pl], sin[pl], 1e-6)
    e_q = head_split_pre_bound(torch.zeros_like(y64), y64, gain)
    sets = (torch.arange(M) // L) // bdiv
    return dict(A=A, W=W, b=b, gain=gain, cos=cos, sin=sin, pos=pos, k=k, v=v, y64=y64, q64=q64, e_q=e_q, sets=sets,
                M=M, L=L, H=H, K=K, bdiv=bdiv, Skv=Skv)


# ----------------------------------------------------------------------------- bit-for-bit checks (pure data movement)
def assert_bits_equal(got, want, what, nan_ok=False):
    """Every element of `got` carries the bit pattern of `want` (same dtype), compared through an integer view so that NaN and
    the sign of zero count.  nan_ok: where `want` is a NaN any NaN will do (the payload of a converted NaN is not pinned:
    tests/weights_ref.py states the same limit).  A failure reports the count and the bounding box like assert_elementwise."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    it = _INT[got.element_size()]
    bad = got.view(it) != want.view(it)
    if nan_ok:
        bad &= ~(torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        cols = got.shape[-1] if got.dim() else 1
        idx = bad.reshape(-1, cols).nonzero()
        r0, c0 = (int(v) for v in idx.min(0).values)
        r1, c1 = (int(v) for v in idx.max(0).values)
        r, c = (int(v) for v in idx[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first at (row {r}, col {c}) of "
            f"[{bad.numel() // cols}, {cols}]: got {float(got.reshape(-1, cols)[r, c])!r} want {float(want.reshape(-1, cols)[r, c])!r}; "
            f"offenders lie in rows [{r0}, {r1}] x cols [{c0}, {c1}]")


def f32(v):
    """A Python number as the fp32 value a kernel argument carries, in fp64."""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ----------------------------------------------------------------------------- small row kernels
def flow_mix_ref_and_bound(noise, x0, sigma):
    """sigma * noise + (1 - sigma) * x0 (x0 [1 | clips, C, L]): three fp32 roundings beyond the exact result - 1 - sigma, and one per
    product or their sum when the compiler contracts one product into an FMA, two products and a sum otherwise - each relative
    to a value no larger than |sigma noise| + |(1 - sigma) x0|: 3 U32 of that."""
    s = f32(sigma)
    a, b = s * noise.double().cpu(), (1.0 - s) * x0.double().cpu()
    return a + b, Bound(3 * U32 * (a.abs() + b.abs()))


def rows_add_act_ref_and_bound(a, v, act_silu, out_dtype, dev):
    """act(a + v), a [R, D] or None (zeros), v [D] or None.  Returns (ref64, bound): without the activation the fp32 addition is
    correctly rounded, so the bound is None and the caller compares bits with the CPU's fp32 sum cast to out_dtype; with SiLU
    the addition is exact to U32 |a + v|, pushed through act_bound."""
    y = torch.zeros(1, dtype=torch.float64)
    if a is not None:
        y = y + a.double().cpu()
    if v is not None:
        y = y + v.double().cpu()
    if not act_silu:
        return y, None
    e_y = U32 * y.abs() if (a is not None and v is not None) else torch.zeros_like(y)
    return act64("silu", y), act_bound("silu", e_y, measure_a_act("silu", y, dev), out_dtype)


def sum32_cast(a, v, out_dtype):
    """The CPU's fp32 a + v (either may be None) cast to out_dtype: what a correctly rounded add-and-store must give bit for bit."""
    y = a.float().cpu() if a is not None else None
    if v is not None:
        y = v.float().cpu() + (y if y is not None else 0.0)
    return y.to(out_dtype)


def measure_a_act_tanh(y64, dev):
    """4 x the largest |PyTorch's fp32 device tanh of fp32(y) - the fp64 tanh of y| (reference against reference, as measure_a_act)."""
    return 4.0 * float((torch.tanh(y64.float().to(dev)).double().cpu() - torch.tanh(y64)).abs().max())


def _conv7(x, w):
    """x [B, Cin, T], w [Cout, Cin, 7] fp64 -> [B, Cout, T], zero padding 3."""
    return torch.nn.functional.conv1d(x, w, None, padding=3)


def dac_out_ref_and_bound(s, w, bias, dev):
    """tanh(bias + sum_{j < 7, c < C} w[j C + c] s[b, t + j - 3, c]), s [B, T, C], w [7 C] tap-major.  Pre-activation: 7 C products
    summed in fp32 in any order plus the bias, (7 C + 4) U32 mag with mag = sum |s w| + |bias|; tanh has Lipschitz constant 1 and
    its own error a_act.  Returns (ref64 [B, T], bound, a_act)."""
    B, T, C = s.shape
    x, ww = s.double().cpu().transpose(1, 2), w.double().cpu().view(7, C).t().reshape(1, C, 7)
    b = bias.double().cpu().view(1, 1, 1)
    y, mag = (_conv7(x, ww) + b)[:, 0], (_conv7(x.abs(), ww.abs()) + b.abs())[:, 0]
    a_act = measure_a_act_tanh(y, dev)
    return torch.tanh(y), Bound((7 * C + 4) * U32 * mag + a_act), a_act


def dac_in_ref_and_bounds(x, w, bias, alpha, dev):
    """DAC encoder input conv 1 -> C (k = 7): y[b, t, c] = bias[c] + sum_j w[j C + c] x[b, t + j - 3], out0 = y, out1 = snake(y).
    Seven products and the bias in fp32: (7 + 4) U32 mag; the snake through dac_bounds.  Returns (y64, snake64, b0, b1, a_act),
    rows [B T, C]."""
    B, T = x.shape
    C = bias.numel()
    xx, ww = x.double().cpu().view(B, 1, T), w.double().cpu().view(7, C).t().reshape(C, 1, 7)
    b = bias.double().cpu().view(1, C, 1)
    rows = lambda t: t.transpose(1, 2).reshape(B * T, C)
    y, mag = rows(_conv7(xx, ww) + b), rows(_conv7(xx.abs(), ww.abs()) + b.abs())
    a_act = measure_a_act_snake(y, alpha.cpu(), dev)
    b0, b1 = dac_bounds((7 + 4) * U32 * mag, y, None, a_act)
    return y, snake64(y, alpha.cpu()), b0, b1, a_act


# ----------------------------------------------------------------------------- stand-alone head split
def rope64(x, cos, sin):
    """x [..., 128] fp64, cos / sin broadcastable [..., 64]: the pair (2 i, 2 i + 1) rotated by angle i."""
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x0 * cos - x1 * sin, x1 * cos + x0 * sin), dim=-1).flatten(-2)


def qkv_head_ref_and_bound(y, gain, cos, sin, eps, out_dtype):
    """One operand of the stand-alone head split: y [n, H, 128] as given (fp32 rows of the fused projection), gain [128] or None,
    cos / sin [n, 64] or None.  RMSNorm (when gain) then RoPE (when cos) in fp64, with head_split_bound at e_y = 0, which leaves
        8 U32 |gain|max max|y| / rms.
    Why 8 covers the roundings (u = 2^-24 = U32 / 2): the sum of squares is a chain of positive terms - two roundings in the lane
    (a product and an FMA), six butterfly levels - 8 u relative, + eps 9 u; its inverse square root halves that and adds the
    instruction's own <= 1 ulp = 2 u: 6.5 u; times y, times gain: 8.5 u on the normalised value (4.25 U32 without a rotation).  The
    rotation multiplies by cos / sin (9.5 u on each product) and adds (+ u of the sum): <= 10.5 u (|a cos| + |b sin|) <= 10.5 u
    sqrt(2) max(|a|, |b|) = 14.9 u = 7.4 U32 of |gain| max|y| / rms.  No gain: a rotation alone rounds two products and their sum,
    2 u (|y0 cos| + |y1 sin|) <= U32 sqrt(2) max|y| < 2 U32 max|y|; neither: a copy (exact before the store)."""
    y = y.double().cpu()
    ref = y
    if gain is not None:
        ref = ref * torch.rsqrt(ref.pow(2).mean(-1, keepdim=True) + f32(eps)) * gain.double().cpu()
    if cos is not None:
        ref = rope64(ref, cos.double().cpu()[:, None], sin.double().cpu()[:, None])
    zero = torch.zeros_like(y)
    if gain is not None:
        return ref, head_split_bound(zero, y, out_dtype, gain.cpu())
    if cos is not None:
        return ref, Bound(2 * U32 * y.abs().amax(-1, keepdim=True).expand_as(y).clone(), out_dtype)
    return ref, Bound(zero, out_dtype)


# ----------------------------------------------------------------------------- solver steps (one iteration, seeded from the device)
STEP_SAVE_X, STEP_USE_SAVED, STEP_ACC_RESET, STEP_BLEND, STEP_HIST = 1, 2, 4, 8, 16


def combine_ref(pred, clips, L, ncfg, gv, gt, scale=None, e_scale=None):
    """pred [ncfg clips L, C] -> (v [clips, C, L] fp64, e_v): the guided value and its bound from the fp32 operands.
        one half        v = pred                                   e = 0
        two halves      v = u + g (c - u)                          e = 3 U32 (|u| + |g| (|c| + |u|))
        three halves    v = p0 + gv (p1 - p0) + gt (p2 - p1)       e = 3 U32 (|p0| + |gv| (|p1| + |p0|)) + 3 U32 (|a| + |gt| (|p2| + |p1|))
                        with a = p0 + gv (p1 - p0): each added term is a difference (one rounding), a product and a sum (two
                        roundings, fused or not) - three roundings relative to the magnitudes that enter, U32 twice the
                        unit round-off.
        factor          v f: one more rounding, U32 |v f|, plus the propagated |f| e and |v| e_f (e_f: the factor's own bound
                        when the reference factor is not the device's).
    gv / gt: the fp32 table entries (or f32(guidance)) as fp64 numbers; scale [clips] fp32 or None."""
    P = pred.double().cpu().view(ncfg, clips, L, -1).transpose(2, 3)
    if ncfg == 2:
        u, c = P[0], P[1]
        v, e = u + gv * (c - u), 3 * U32 * (u.abs() + abs(gv) * (c.abs() + u.abs()))
    elif ncfg == 3:
        p0, p1, p2 = P[0], P[1], P[2]
        a = p0 + gv * (p1 - p0)
        v = a + gt * (p2 - p1)
        e = 3 * U32 * (p0.abs() + abs(gv) * (p1.abs() + p0.abs())) + 3 * U32 * (a.abs() + abs(gt) * (p2.abs() + p1.abs()))
    else:
        v, e = P[0], torch.zeros_like(P[0])
    if scale is not None:
        f = scale.double().cpu().view(-1, 1, 1)
        ef = torch.zeros_like(f) if e_scale is None else e_scale.double().cpu().view(-1, 1, 1)
        v, e = v * f, f.abs() * e + v.abs() * ef + U32 * (v * f).abs()
    return v, e


def step_ref_and_bounds(v, e_v, x, x_saved, d_acc, row, ring=None, it=None):
    """ONE iteration of the solver update in fp64 from the guided value (v, e_v of combine_ref) and the state the device holds (x,
    x_saved, d_acc [clips, C, L] copied back; x_saved / d_acc may be None), row = the iteration's coefficient row.  Returns a dict
    of (ref64, Bound) for 'x' and 'd_acc' and ref64 alone for 'x_saved' (a copy: exact), with
        deriv = w_new v + w_acc acc                    e_d = |w_new| e_v + 2 U32 (|w_new v| + |w_acc acc|)
        deriv += c_j h_j  (flagged rows, c_j != 0)     e_d += 2 U32 (|deriv| + |c_j h_j|): the product and the sum relative to
                                                       the magnitudes that enter; h_j = slot (it - j) mod slots
        xn = base + deriv dt                           e_x = |dt| e_d + 2 U32 (|base| + |deriv dt|)
        d_acc' = acc + w_store v                       e_a = |w_store| e_v + 2 U32 (|acc| + |w_store v|)
    two roundings per line whether or not the product is contracted into an FMA (U32 is twice the unit round-off).
    ring [slots, clips, C, L] (or None: no history): the device's ring as read back BEFORE the step (exact operands), `it` the
    iteration.  A term whose weight is zero is not read (the ring may hold NaN there); the slot it mod slots receives v itself,
    bound e_v: with a ring the dict also has 'slot' (index) and 'hist' ((v, Bound(e_v)))."""
    w_new, w_acc, dt, w_store = (float(t) for t in row[:4].double())
    flags = int(row[4])
    xd = x.double().cpu()
    acc = torch.zeros_like(xd) if (d_acc is None or flags & STEP_ACC_RESET) else d_acc.double().cpu()
    deriv = w_new * v + w_acc * acc
    e_d = abs(w_new) * e_v + 2 * U32 * ((w_new * v).abs() + (w_acc * acc).abs())
    if ring is not None and flags & STEP_HIST:
        for j in (1, 2):
            c = float(row[5 + j].double())
            if c != 0.0:
                term = c * ring[(it - j) % ring.shape[0]].double().cpu()
                e_d = e_d + 2 * U32 * (deriv.abs() + term.abs())
                deriv = deriv + term
    base = x_saved.double().cpu() if flags & STEP_USE_SAVED else xd
    xn = base + deriv * dt
    e_x = abs(dt) * e_d + 2 * U32 * (base.abs() + (deriv * dt).abs())
    out = {"x": (xn, Bound(e_x)), "flags": flags, "s_next": float(row[5].double())}
    if ring is not None:
        out["slot"], out["hist"] = it % ring.shape[0], (v, Bound(e_v))
    if d_acc is not None:
        out["d_acc"] = (acc + w_store * v, Bound(abs(w_store) * e_v + 2 * U32 * (acc.abs() + (w_store * v).abs())))
    if x_saved is not None:
        out["x_saved"] = xd if flags & STEP_SAVE_X else x_saved.double().cpu()
    return out


def solver_step_ref_and_bounds(pred, x, x_saved, d_acc, row, ncfg, guidance):
    """step_ref_and_bounds behind the two-half (or one-half) combine with the scalar `guidance`, pred [ncfg clips L, C]."""
    v, e_v = combine_ref(pred, x.shape[0], x.shape[2], ncfg, f32(guidance), f32(guidance))
    return step_ref_and_bounds(v, e_v, x, x_saved, d_acc, row)


def edit_blend_ref_and_bound(xn, e_x, s_next, x0, noise, mask):
    """The edit form's blend on a STEP_BLEND row: tgt = s noise + (1 - s) x0 (three roundings, as flow_mix), then
    m xn + (1 - m) tgt: the propagated terms |m| e_x + |1 - m| e_t plus (2 + 1) U32 (|m xn| + |(1 - m) tgt|).
    x0 [1 | clips, C, L], noise [clips, C, L], mask [1 | clips, L] or [L] or None (all ones)."""
    s = float(s_next)
    a, b = s * noise.double().cpu(), (1.0 - s) * x0.double().cpu()
    tgt, e_t = a + b, 3 * U32 * (a.abs() + b.abs())
    m = torch.ones(1, 1, xn.shape[-1], dtype=torch.float64) if mask is None else mask.double().cpu().view(-1, 1, xn.shape[-1])
    p, q = m * xn, (1.0 - m) * tgt
    return p + q, Bound(m.abs() * e_x + (1.0 - m).abs() * e_t + 3 * U32 * (p.abs() + q.abs()))


def windows_mean_ref_and_bound(xn, e_x, n_win, starts, weights):
    """The windows form's blend: every global frame g replaced in all its covering windows by sum_k w[k][g - starts[k]] xn_k (window
    order).  xn / e_x [variations n_win, C, L] fp64 (e_x None: the operands are exact, as in the stitch).  n covering windows:
    the propagated sum |w_k| e_k plus (n + 1) U32 sum |w_k x_k|.  Returns (per-window ref64, per-window e, G [variations, C, Ltot],
    e_G, coverage [Ltot])."""
    V, C, L = xn.shape[0] // n_win, xn.shape[1], xn.shape[2]
    Ltot = int(starts[-1]) + L
    w = weights.double().cpu()
    G, mag, prop = (torch.zeros(V, C, Ltot, dtype=torch.float64) for _ in range(3))
    cov = torch.zeros(Ltot, dtype=torch.float64)
    for k, s in enumerate(int(t) for t in starts):
        xk = xn.reshape(V, n_win, C, L)[:, k]
        G[..., s:s + L] += w[k] * xk
        mag[..., s:s + L] += (w[k] * xk).abs()
        if e_x is not None:
            prop[..., s:s + L] += w[k].abs() * e_x.reshape(V, n_win, C, L)[:, k]
        cov[s:s + L] += 1
    e_G = prop + (cov + 1) * U32 * mag
    ref = torch.stack([G[v, :, s:s + L] for v in range(V) for s in (int(t) for t in starts)])
    e = torch.stack([e_G[v, :, s:s + L] for v in range(V) for s in (int(t) for t in starts)])
    return ref, e, G, e_G, cov


def rows_of(x, ncfg, rows_dtype):
    """The next model input rows a step stages from the sample it wrote: x [clips, C, L] -> [ncfg clips L, C] in rows_dtype, the same
    bits in every CFG copy."""
    r = x.detach().cpu().transpose(1, 2).reshape(-1, x.shape[1]).to(rows_dtype)
    return r.repeat(ncfg, 1)


def periodic_flags(x, period):
    """[groups] int32: 1 where some row s >= period of the group differs in its BIT PATTERN from row s - period (so +0.0 against
    -0.0 differs and equal NaN patterns agree), x [groups, rows, D] fp32."""
    xi = x.detach().cpu().contiguous().view(torch.int32)
    if xi.shape[1] <= period:
        return torch.zeros(xi.shape[0], dtype=torch.int32)
    return (xi[:, period:] != xi[:, :-period]).flatten(1).any(1).to(torch.int32)


# The GPU cases of the fused cross attention (tests/test_ops_elementwise_gpu.py); the CPU emulation of test_opcheck_cpu.py runs the
# same operands, so that what the kernel is held to has been met by plain fp32 arithmetic first.
# name -> (Bc batch rows, L, H, bdiv, Skv, V^T pitch, forced tile, K scale).  Text set of a row: (row // L) // bdiv.
def _edge(Skv, pitch=96):
    return (2, 250, 2, 1, Skv, pitch, 27, 2.0)


CROSS_CASES = {
    # key edges, two sets (clips 1, L 250: the tile [192, 256) straddles them): one key, tile-aligned, one past, the ragged production length, full image
    **{f"skv{s}": _edge(s) for s in (1, 32, 33, 64, 65, 77, 95, 96)},
    "skv77_pitch104": _edge(77, 104),
    "straddle_small": (6, 8, 3, 3, 77, 96, 27, 2.0),          # clips 3, L 8: L bdiv = 24 < 64, M = 48 <= 2 L bdiv: 24 + 24 rows in ONE tile, 16 dead rows
    "sets3_L64": (3, 64, 2, 1, 77, 96, 27, 2.0),              # one set per batch row (per-clip conditioning): boundaries on tile boundaries
    "sets3_L65": (3, 65, 2, 1, 77, 96, 27, 2.0),              # tile [64, 128): its first set owns ONE row
    "sets5_L70": (5, 70, 3, 1, 77, 96, 27, 2.0),              # boundaries at 70, 140, 210, 280: every offset class inside a tile
    "sets3_L127": (3, 127, 2, 1, 77, 96, 27, 2.0),            # a set that ends one row before a tile does
    "sets3_bdiv2_L40": (6, 40, 2, 2, 77, 96, 27, 2.0),        # two batch rows per set: 80 rows per set
    "large_scores": (2, 100, 2, 1, 77, 96, 27, 15.0),         # scores near +- 40: the running maximum must be subtracted
    "auto_plan": (2, 250, 12, 1, 77, 96, 0, 2.0),             # the bs = 1 production problem: the automatic plan must land on tile 27 and fuse
}


@functools.lru_cache(maxsize=4)
def cross_case(name):
    Bc, L, H, bdiv, Skv, _, _, ks = CROSS_CASES[name]
    return cross_dyadic_case(Bc, L, H, bdiv, Skv, seed=8000 + 7 * L + Skv, k_scale=ks, v_floor=0.25 if ks >= 15 else 0.0)


# ----------------------------------------------------------------------------- audio front end: resampler, log-mel, dB-mel
# (csrc/audio.hip, csrc/clap_audio.hip).  None of the three rounds to 16 bits before its output, so every bound below is a few
# hundred U32 of a sum of absolute products: a wrong sample, frame, bin or repeat seam lies orders of magnitude outside.
LOGMEL_MEAN, LOGMEL_2STD, LOGMEL_FLOOR = 4.2677393, 2 * 4.5689974, 1e-6       # the AST normalisation and the log's floor
DBMEL_FLOOR = 1e-10


def resample_ref_and_bound(x, taps, orig, new, width):
    """foley_op_resample_sinc in fp64 from the fp32 samples x [B, N] and taps [new, ntaps]:
        ref[b, j new + p] = sum_t x[b, j orig + t - width] taps[p][t]          (x zero outside [0, N)), cut to ceil(N new / orig)
    mag is the same sum over absolute values; the bound (ntaps + 2) U32 mag covers ntaps fp32 FMAs in any order.  Where mag == 0
    (every tap of the window hangs over the clip's edge or meets a zero sample) the bound is 0: the output must be 0."""
    x, k = x.double().cpu(), taps.double().cpu()
    B, N = x.shape
    ntaps = k.shape[1]
    n_out = -(-N * new // orig)
    J = -(-n_out // new)
    right = max(0, (J - 1) * orig + ntaps - width - N)
    win = torch.nn.functional.pad(x, (width, right)).unfold(1, ntaps, orig)[:, :J]          # [B, J, ntaps]
    ref = (win @ k.t()).reshape(B, -1)[:, :n_out]
    mag = (win.abs() @ k.abs().t()).reshape(B, -1)[:, :n_out]
    return ref, Bound((ntaps + 2) * U32 * mag)


def mel_dense(tables, n_bins=513):
    """The sparse mel table (mel_lo, mel_len, mel_w) as a dense fp64 [n_bins, n_mels] matrix."""
    lo, ln, w = tables["mel_lo"].cpu(), tables["mel_len"].cpu(), tables["mel_w"].cpu()
    fb = torch.zeros(n_bins, lo.numel(), dtype=torch.float64)
    for c in range(lo.numel()):
        a, n = int(lo[c]), int(ln[c])
        fb[a:a + n, c] = w[c, :n].double()
    return fb


def logmel_frames(w16):
    """The frames foley_op_logmel stages: w16 [B, N16] -> [B S, 65, 400] (same dtype); segment s of a clip is samples [5120 s,
    5120 s + 10240), tap m of frame f reads segment sample 160 f + m - 200, reflected at the segment's edges (no edge repeat)."""
    B, N = w16.shape
    nseg = (N - 10240) // 5120 + 1
    segs = torch.stack([w16[:, s * 5120:s * 5120 + 10240] for s in range(nseg)], 1).reshape(B * nseg, 10240)
    i = torch.arange(65)[:, None] * 160 + torch.arange(400)[None] - 200
    i = torch.where(i < 0, -i, torch.where(i >= 10240, 2 * 10239 - i, i))
    return segs[:, i]


def logmel_tables():
    from foley_amd.host import sync_score
    return sync_score.logmel_tables("cpu")


def logmel_emulation(w16, tables=None, dtype=torch.float64):
    """foley_op_logmel's arithmetic on the CPU from logmel_tables: reflect-padded 400-sample frames x basis -> power -> sparse mel
    -> log -> pad -> normalise, computed in `dtype` (fp64: the reference; fp32: the same recipe as a second fp32 implementation).
    Returns the spectrogram [B*S, 128, 66] fp32 and the im2col patches [B*S*72, 256] in the kernel's layout."""
    tb = tables or logmel_tables()
    fr = logmel_frames(w16.cpu()).to(dtype)                                           # [G, 65, 400]
    re = fr @ tb["basis"][0].cpu().to(dtype)
    im = fr @ tb["basis"][1].cpu().to(dtype)
    pw = (re * re + im * im)[..., :513]
    mel = torch.log(pw @ mel_dense(tb).to(dtype) + LOGMEL_FLOOR).transpose(1, 2)      # [G, 128, 65]
    mel = torch.nn.functional.pad(mel, (0, 1))
    mel = ((mel + LOGMEL_MEAN) / LOGMEL_2STD).float()
    patches = mel.unfold(1, 16, 10).unfold(2, 16, 10)                                 # [G, 12, 6, 16, 16]: (fi, ti, kf, kt)
    return mel, patches.reshape(-1, 256)


def _dft_mel_ref_and_error(fr, tables, ntaps):
    """Shared chain of the two spectrogram kernels, in fp64 from the staged frames fr [G, T, ntaps] and the fp32 tables:
        re = s @ C, im = s @ S                        e_re = (ntaps + 2) U32 (|s| @ |C|), e_im likewise: ntaps fp32 FMAs in any order
        pw = re^2 + im^2                              e_pw = 2 |re| e_re + e_re^2 + 2 |im| e_im + e_im^2 + 3 U32 pw
        mel[c] = sum_k w[c][k] pw[lo_c + k]           e_mel = sum_k w[c][k] e_pw[lo_c + k] + (len_c + 2) U32 mel
    Returns (mel, e_mel) [G, T, n_mels]."""
    fr = fr.double().cpu()
    C, Sn = (tables["basis"].cpu()[i].double()[:, :513] for i in (0, 1))
    re, im = fr @ C, fr @ Sn
    a = fr.abs()
    e_re, e_im = (ntaps + 2) * U32 * (a @ C.abs()), (ntaps + 2) * U32 * (a @ Sn.abs())
    pw = re * re + im * im
    e_pw = 2 * re.abs() * e_re + e_re * e_re + 2 * im.abs() * e_im + e_im * e_im + 3 * U32 * pw
    fb = mel_dense(tables)
    mel = pw @ fb
    e_mel = e_pw @ fb + (tables["mel_len"].cpu().double() + 2) * U32 * mel
    return mel, e_mel


def logmel_ref_and_bound(w16, tables, dev="cpu"):
    """The normalised log-mel spectrogram [B S, 128, 66] of foley_op_logmel in fp64 (logmel_emulation's recipe, unrounded) with a
    per-element bound.  With (mel, e_mel) from _dft_mel_ref_and_error at 400 taps, m = mel + 1e-6, r = e_mel / m, L = log m,
    v = (L + 4.2677393) / (2 * 4.5689974):
        e_v = (r / (1 - r) + a_log + 4 U32 |L|) / 9.1379948 + U32 4.2677393 / 9.1379948 + 2 U32 |v|
      r / (1 - r)   |log(1 +- r)| <= r / (1 - r): the relative error of m pushed through the logarithm;
      a_log         the logarithm's own error, measured reference against reference as measure_a_act does: 4 x the largest
                    |torch's fp32 log on `dev` of fp32(m) - the fp64 log of m| over this case's m; it also pays for the rounding of
                    the sum mel + 1e-6 and of the constant 1e-6 (each half a U32 relative to m: the same size as the fp32(m) inside
                    the measurement, which the factor 4 multiplies);
      4 U32 |L|     the rounding of L + mean and of the product, relative to L;
      the constants mean is rounded to fp32 and the sum's rounding has a share relative to it (U32 mean together); 1 / (2 std) carries
                    two roundings (the constant, the reciprocal) and the product a third: 3 half-U32 <= 2 U32, relative to v.
    Column 65 (the time pad) is mean / (2 std), held within 2 U32 of it (four roundings: two constants, reciprocal, product).
    Elements with r >= 0.5 get an infinite bound (NaN still offends) and are LEFT OUT; their share of the [B S, 128, 65] computed
    elements is returned and the caller caps it.  Returns (ref64, Bound, share, a_log, silent) - silent [B S, 65] marks the frames
    whose 400 staged samples are all zero."""
    fr = logmel_frames(w16.cpu())
    mel, e_mel = _dft_mel_ref_and_error(fr, tables, 400)
    m = mel + LOGMEL_FLOOR
    r, L = e_mel / m, torch.log(m)
    a_log = 4.0 * float((torch.log(m.float().to(dev)).double().cpu() - L).abs().max())
    v = (L + LOGMEL_MEAN) / LOGMEL_2STD
    ok = r < 0.5
    e = (r / (1 - r.clamp_max(0.5)) + a_log + 4 * U32 * L.abs()) / LOGMEL_2STD + U32 * LOGMEL_MEAN / LOGMEL_2STD + 2 * U32 * v.abs()
    e = torch.where(ok, e, torch.full_like(e, float("inf")))
    pad = LOGMEL_MEAN / LOGMEL_2STD
    ref = torch.nn.functional.pad(v.transpose(1, 2), (0, 1), value=pad)
    e = torch.nn.functional.pad(e.transpose(1, 2), (0, 1), value=2 * U32 * pad)
    return ref, Bound(e), float((~ok).double().mean()), a_log, (fr == 0).all(-1)


def dbmel_frames(padded):
    """The frames foley_op_melspec_db transforms: padded [G, 480000] (a window as the extractor pads it, or a crop) -> [G, 1001,
    1024]: centred STFT framing, 512 samples of reflect padding (no edge repeat) on either side, hop 480."""
    p = torch.nn.functional.pad(padded[:, None], (512, 512), mode="reflect")[:, 0]
    return p.unfold(1, 1024, 480)


def dbmel_ref_and_bound(padded480k, tables, dev="cpu"):
    """foley_op_melspec_db's dB-mel spectrogram [G, 1001, 64] in fp64 from the windows as padded, with a per-element bound in dB.
    (mel, e_mel) from _dft_mel_ref_and_error at 1024 taps (the kernel's two half-sums and their addition are one of the orders
    (1024 + 2) U32 covers), ref = 10 log10(max(mel, 1e-10)), r = e_mel / mel:
        e_db = 10 / ln 10 * r / (1 - r) + a_log10 + 4 U32 |ref|
    a_log10 is measured like a_log: 4 x the largest |torch's fp32 10 log10 on `dev` of fp32(mel) - ref| over the elements above
    the floor.  mel == 0 (a silent frame) must give -100.0 exactly (bound 0).  An element whose [mel - e_mel, mel + e_mel] contains
    1e-10 may be -100.0 or inside the bound (`amb`, see assert_dbmel); amb elements and those with r >= 0.5 (infinite bound) are
    LEFT OUT and their share is returned.  Returns (ref64, Bound, share, a_log10, amb)."""
    mel, e_mel = _dft_mel_ref_and_error(dbmel_frames(padded480k.cpu()), tables, 1024)
    ref = 10.0 * torch.log10(mel.clamp_min(DBMEL_FLOOR))
    live = mel > DBMEL_FLOOR
    a_log10 = 0.0
    if bool(live.any()):
        ml = mel[live]
        a_log10 = 4.0 * float((10.0 * torch.log10(ml.float().to(dev)).double().cpu() - 10.0 * torch.log10(ml)).abs().max())
    r = torch.where(mel > 0, e_mel / mel.clamp_min(1e-300), torch.zeros_like(mel))
    ok = r < 0.5
    e = 10.0 / math.log(10.0) * r / (1 - r.clamp_max(0.5)) + a_log10 + 4 * U32 * ref.abs()
    e = torch.where(ok, e, torch.full_like(e, float("inf")))
    e = torch.where(mel == 0, torch.zeros_like(e), e)
    amb = (mel > 0) & (mel - e_mel <= DBMEL_FLOOR) & (mel + e_mel >= DBMEL_FLOOR)
    return ref, Bound(e), float((amb | ~ok).double().mean()), a_log10, amb


def assert_dbmel(got, ref, bound, amb, what):
    """assert_elementwise for the dB-mel: an ambiguous element (dbmel_ref_and_bound) may also be -100.0 exactly."""
    got = got.detach().double().cpu()
    return assert_elementwise(torch.where(amb & (got == -100.0), ref, got), ref, bound, what)


# The cases of tests/test_audio_front_elementwise_gpu.py; the CPU emulations of test_opcheck_cpu.py run the same operands.
# name -> (source rate, target rate, N, clips, taps, Nout); taps / Nout None: whatever the tap builder and the length rule give
RESAMPLE_CASES = {
    "3to1_two_blocks": (48000, 16000, 1543, 3, 41, 515),        # two full 256-output blocks + 3
    "3to1_shorter_than_filter": (48000, 16000, 5, 1, 41, 2),    # every tap window hangs over both edges
    "441to160": (44100, 16000, 1340, 3, 475, 487),              # the down-sampling ratio sync_scores takes for 44.1 kHz audio
    "147to160": (44100, 48000, 1000, 3, None, 1089),
    "1to3": (16000, 48000, 700, 3, 15, 2100),
    "2to3": (32000, 48000, 513, 3, None, None),
}
LOGMEL_CASES = {"s1": 10240, "s1_long": 15359, "s2": 15360, "s3_ragged": 10240 + 2 * 5120 + 777}      # name -> N16
# name -> (N, clips, starts)
DBMEL_CASES = {
    "n1024": (1024, 1, [0]),                 # n_rep 468, tail 768 zeros
    "n1500": (1500, 1, [0]),
    "n158400": (158400, 1, [0]),             # 3.3 s: n_rep 3, tail 4800 zeros
    "n479999": (479999, 1, [0]),             # n_rep 1, one zero sample that the end reflect reads
    "n480001_starts": (480001, 1, [0, 1, 5, -3]),      # 5 and -3 are clamped to 1 and 0
    "n158400_b2": (158400, 2, [0]),
}


@functools.lru_cache(maxsize=None)
def resample_case(name):
    """(x [B, N] fp32, taps, orig, new, width): noise of amplitude 0.1 plus unit impulses at samples 0 and N - 1, per clip."""
    from foley_amd.host import sync_score
    src, dst, N, B, ntaps, n_out = RESAMPLE_CASES[name]
    taps, orig, new, width = sync_score.sinc_resample_taps(src, dst)
    assert ntaps is None or taps.shape[1] == ntaps, (name, taps.shape)
    assert n_out is None or -(-N * new // orig) == n_out, name
    x = 0.1 * torch.randn(B, N, generator=torch.Generator().manual_seed(4100 + N))
    x[:, 0] += 1.0
    x[:, N - 1] += 1.0
    return x, taps, orig, new, width


@functools.lru_cache(maxsize=None)
def logmel_case(name, B):
    """w16 [B, N16] fp32: noise of amplitude 0.1 plus a 1 kHz tone of 0.4, different per clip, with stretches of exact zeros:
        every clip   [4500, 5900): crosses sample 5120, where segment 1 begins (frames 30 .. 35 of segment 0 and 0 .. 3 of segment 1
                     are silent)
        clip 0       [0, 680): frames 0 .. 3 of segment 0 are silent and frame 3 reads sample 679 last; [9600, 10900): crosses
                     the end of segment 0 (its end reflect) and the start of segment 2
        clip 1       (B = 3) all zeros
        clip 2       [0, 201): frame 0 reads samples 0 .. 200 through the reflect and no further; [10039, 10240): frame 64 of
                     segment 0 reads 10039 .. 10239 through the end reflect and nothing before."""
    N = LOGMEL_CASES[name]
    gen = torch.Generator().manual_seed(5200 + N + B)
    t = torch.arange(N, dtype=torch.float64)
    w = 0.1 * torch.randn(B, N, generator=gen, dtype=torch.float64)
    w += 0.4 * torch.sin(2 * math.pi * 1000.0 * t / 16000.0 + torch.arange(B, dtype=torch.float64)[:, None])
    w = w.float()
    w[:, 4500:5900] = 0
    w[0, :680] = 0
    w[0, 9600:10900] = 0
    if B > 1:
        w[1] = 0
    if B > 2:
        w[2, :201] = 0
        w[2, 10039:10240] = 0
    return w


@functools.lru_cache(maxsize=None)
def dbmel_case(name):
    """(x [B, N] fp32 noise of amplitude 0.05, starts, windows [B W, 480000]: every window as the kernel must pad or crop it)."""
    import clap_ref
    N, B, starts = DBMEL_CASES[name]
    x = 0.05 * torch.randn(B, N, generator=torch.Generator().manual_seed(6300 + N + B))
    if N < 480000:
        wins = torch.stack([clap_ref.repeatpad(x[b]) for b in range(B)])
    else:
        wins = torch.stack([x[b, s:s + 480000] for b in range(B) for s in (min(max(s, 0), N - 480000) for s in starts)])
    return x, starts, wins
