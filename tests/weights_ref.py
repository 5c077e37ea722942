"""Expected content of the reference-keyed loader's arena (csrc/weights.hip), slot by slot.

The expected value of every packed tensor is host/packers.py applied to the same state dict in fp32 (an exact upcast of every
checkpoint dtype), followed by torch's own CPU cast to the slot's dtype.  Slot dtypes and shapes come from the packers' layout
tables (dit_arena_layout / dac_arena_layout); nothing here knows the library's slot order or offsets.

Everything is compared bit for bit on an integer view, with one stated exception: an element whose expected bf16 value is a NaN
only has to be a NaN.  torch's own fp32 -> bf16 cast of a NaN is 0xffff in its vectorised CPU path and 0x7fc0 in its scalar
and device paths, so there is no single reference payload to hold the library to.

Weight-normed DAC layers handed over as (g, v) are the one non-bitwise case: reference float64 v * (g / ||v||), bound per
element in `wn_bound_factor` below.  Layers handed over folded (`.weight`) are bitwise like everything else.
"""
import re
import zlib
from collections import OrderedDict

import numpy as np
import torch

from foley_amd import nodes
from foley_amd.host import packers, synth

F8 = {0: None, 1: torch.float8_e4m3fn, 2: torch.float8_e5m2}
QMODE = {1: "fp8_e4m3fn", 2: "fp8_e5m2"}
# arena configurations: (label, compute dtype, weight format of foley_weights_begin)
ARENAS = (("fp32", torch.float32, 0), ("bf16", torch.bfloat16, 0), ("fp16", torch.float16, 0),
          ("bf16+e4m3fn", torch.bfloat16, 1), ("bf16+e5m2", torch.bfloat16, 2),
          ("fp16+e4m3fn", torch.float16, 1), ("fp16+e5m2", torch.float16, 2))
SOURCES = (torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2)
_IVIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_M32 = 0xFFFFFFFF


def bits(t):
    """Integer view of a tensor's storage (uint8 / int16 / int32): NaN payloads and signed zeros count."""
    t = t.contiguous()
    return t.view(_IVIEW[t.element_size()])


# ----------------------------------------------------------------------------- state dicts whose values name their position
def _hash32(seed, n, device, start=0):
    i = torch.arange(start, start + n, dtype=torch.int64, device=device)
    x = (i * 0x9E3779B1 + seed) & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def ident_tensor(key, shape, device):
    """fp32 values that identify their source position: the flat index where that is exact in fp32 (count below 2^24), rotated
    by a per-key constant modulo 2^24 so that tensors fused into one slot (w1 / w3, the modulation blocks) differ as well;
    otherwise a 24-bit integer hash of (key, index).  A permutation error cannot cancel against such values."""
    n = _numel(shape)
    seed = zlib.crc32(key.encode())
    if n < (1 << 24):
        i = torch.arange(n, dtype=torch.int64, device=device)
        return ((i + (seed & 0xFFFFFF)) % (1 << 24)).to(torch.float32).view(*shape)
    out = torch.empty(n, dtype=torch.float32, device=device)
    for s0 in range(0, n, 1 << 24):
        m = min(1 << 24, n - s0)
        out[s0:s0 + m] = ((_hash32(seed, m, device, s0) >> 8) - (1 << 23)).to(torch.float32)
    return out.view(*shape)


def value_tensor(key, shape, device, emin=-26, emax=17):
    """fp32 values hashed from (key, index) with a full 23-bit mantissa, a random sign and an exponent uniform in [emin, emax]:
    not representable in any narrower type, and with the defaults they reach the subnormals of fp16 / e5m2 / e4m3fn, the e4m3fn
    NaN range (> 464) and the fp16 / e5m2 overflow (>= 65520 / 61440)."""
    n = _numel(shape)
    seed = zlib.crc32(key.encode())
    a = _hash32(seed, n, device)
    b = _hash32(seed ^ 0x5BD1E995, n, device)
    e = (b >> 9) % (emax - emin + 1) + emin + 127
    u = ((a & 1) << 31) | (e << 23) | (b & 0x7FFFFF)
    u = torch.where(u >= (1 << 31), u - (1 << 32), u)
    return u.to(torch.int32).view(torch.float32).view(*shape)


def make_state(schema, device, gen=ident_tensor, keys=None, **kw):
    return OrderedDict((k, gen(k, schema[k][0], device, **kw)) for k in (keys if keys is not None else schema))


# ----------------------------------------------------------------------------- DAC weight-norm layers
def wn_layers(dac_cfg):
    """(state-dict base key, packed slot, kind, stride) of every weight-normed decoder conv (dac.py:120-149; the same walk as
    packers.pack_dac).  kind: 'conv' [O, I, k], 'convT' [Cin, Cout, 2s] (g per INPUT channel), 'out' [1, C, 7]."""
    out = [("decoder.model.0", "dac.in.w", "conv", 0)]
    n = len(dac_cfg.rates)
    for i, s in enumerate(dac_cfg.rates):
        r, p = f"decoder.model.{i + 1}.block.", f"dac.{i}."
        out.append((r + "1", p + "up.w", "convT", s))
        for j in range(3):
            out.append((r + f"{j + 2}.block.1", p + f"{j}.c7.w", "conv", 0))
            out.append((r + f"{j + 2}.block.3", p + f"{j}.c1.w", "conv", 0))
    out.append((f"decoder.model.{n + 2}", "dac.out.w", "out", 0))
    return out


def wn_layout(w, kind, stride):
    """Folded weight (any dtype) -> its packed layout, with the packers' own layout functions."""
    if kind == "conv":
        return packers.conv_to_gemm(w)
    if kind == "convT":
        return packers.convT_to_gemm(w, stride)
    return w[0].permute(1, 0).reshape(-1).contiguous()


_G, _V = ".parametrizations.weight.original0", ".parametrizations.weight.original1"
SPELLINGS = ("param", "legacy", "folded")


def fold64(g, v):
    g, v = g.to(torch.float32).double(), v.to(torch.float32).double()     # exact upcasts of any checkpoint dtype
    n = v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))
    return v * (g.view(-1, *([1] * (v.dim() - 1))) / n)


def respell_dac(dsd, dac_cfg, spelling_of, v_first_of=lambda i: False):
    """The parametrised DAC state dict `dsd` with layer i spelled SPELLINGS[spelling_of(i)]: original0/1, weight_g/v, or a folded
    `.weight` (fp32 torch fold: that value IS the checkpoint then).  v_first_of(i): v precedes g in the dict's order.
    Returns (state dict, {slot: (g, v, kind, stride)} of the layers that still arrive as a pair)."""
    layer = {base: (i, slot, kind, s) for i, (base, slot, kind, s) in enumerate(wn_layers(dac_cfg))}
    out, pairs = OrderedDict(), {}
    for k, t in dsd.items():
        if k.endswith(_V):
            continue
        if not k.endswith(_G):
            out[k] = t
            continue
        base = k[:-len(_G)]
        i, slot, kind, s = layer[base]
        g, v = t, dsd[base + _V]
        sp = SPELLINGS[spelling_of(i) % 3]
        if sp == "folded":
            out[base + ".weight"] = packers.fold_weight_norm({base + ".weight_g": g, base + ".weight_v": v}, base)
            continue
        kg, kv = (base + _G, base + _V) if sp == "param" else (base + ".weight_g", base + ".weight_v")
        for kk, tt in (((kv, v), (kg, g)) if v_first_of(i) else ((kg, g), (kv, v))):
            out[kk] = tt
        pairs[slot] = (g, v, kind, s)
    return out, pairs


def wn_bound_factor(cols):
    """Per-element bound of the device fold against float64 v * (g / ||v||): |got - ref| <= |ref| * (cols/2 + 6) * 2^-24.

    u = 2^-24.  The sum of `cols` non-negative squares, each rounded once and added in any order, is within (cols - 1) u of the
    exact sum relatively (cols roundings of the squares and cols - 1 of the additions never exceed a chain of cols factors on any
    term, minus nothing cancels because all terms are >= 0; first order cols u, the issue's count of cols - 1 plus the square's
    own rounding); the square root halves a relative error: cols/2 u.  Then one rounding each for the square root, the division
    g / ||v|| and the product with v: 3 u.  The upcasts of g and v are exact.  (cols/2 + 3) u to first order; the remaining
    3 u cover the second-order terms (cols u <= 2^-10 at cols = 16384, squared 2^-20 relative of the first-order term) and a
    division or square root that is correct to 1 ulp instead of 1/2."""
    return (cols / 2.0 + 6.0) * 2.0 ** -24


def wn_check(slot, got, g, v, kind, stride):
    """Returns (largest error/bound ratio, message or None)."""
    ref = wn_layout(fold64(g, v), kind, stride)
    cols = v.numel() // v.shape[0]
    got64 = got.double().reshape(ref.shape)
    bound = ref.abs() * wn_bound_factor(cols)
    err = (got64 - ref).abs()
    bad = ~(err <= bound)                       # NaN counts as bad
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        return ratio, (f"slot {slot}: weight-norm fold out of bound at flat index {i} (got {float(got64.flatten()[i])!r}, "
                       f"ref {float(ref.flatten()[i])!r}, cols {cols}), {int(bad.sum())} of {bad.numel()} elements, "
                       f"worst error/bound {ratio:.3f}")
    return ratio, None


# ----------------------------------------------------------------------------- the expected arena
def upcast(sd):
    return OrderedDict((k, v.detach().to(torch.float32)) for k, v in sd.items())


def torch_cast(t, dtype):
    """torch's CPU cast of an fp32 tensor, returned on the tensor's device."""
    if dtype == torch.float32:
        return t
    return t.cpu().to(dtype).to(t.device)


def slot_table(cfg, dac_cfg, compute_dtype, wfmt):
    """name -> (dtype, shape) of every packed tensor, from the packers' own layout tables."""
    _n, dit = packers.dit_arena_layout(cfg, compute_dtype, F8[wfmt])
    _n, dac = packers.dac_arena_layout(dac_cfg)
    table = OrderedDict((k, (dt, tuple(shape))) for k, (_off, dt, shape) in dit.items())
    table.update((k, (dt, tuple(shape))) for k, (_off, dt, shape) in dac.items())
    return table


def expected_slot(name, packed32, table, compute_dtype, wfmt):
    """One expected packed tensor: the packers' fp32 result cast by torch to the slot's dtype.  `time0.b` of an fp8 arena passes
    through the fp8 type first (nodes.fp8_round_state_dict's autocast rule, golden g8 "Q14"): a double rounding."""
    dt, shape = table[name]
    t = packed32[name]
    assert tuple(t.shape) == shape and t.dtype == torch.float32, (name, t.shape, shape, t.dtype)
    if name == "time0.b" and wfmt:
        r = nodes.fp8_round_state_dict({"time_in.mlp.0.bias": t.cpu()}, QMODE[wfmt], autocast=True, param_dtype=torch.float32)
        return r["time_in.mlp.0.bias"].to(t.device)
    return torch_cast(t, dt)


def expected_packed32(dit_sd, dac_sd, cfg, dac_cfg):
    """packers.pack_dit / pack_dac of the exactly upcast state dicts, everything in fp32.  Weight-normed layers that arrive as
    pairs get the packers' fp32 fold here; callers check those slots with wn_check instead."""
    out = OrderedDict()
    if dit_sd is not None:
        out.update(packers.pack_dit(upcast(dit_sd), cfg, torch.float32))
    if dac_sd is not None:
        out.update(packers.pack_dac(upcast(dac_sd), dac_cfg))
    return out


def mismatch(name, got, exp):
    """None if the two tensors are identical bit for bit (see the module docstring for the bf16 NaN rule), else a message with
    the slot name, the first differing flat index and the number of differing elements."""
    if got.dtype != exp.dtype or tuple(got.shape) != tuple(exp.shape):
        return f"slot {name}: got {got.dtype} {tuple(got.shape)}, expected {exp.dtype} {tuple(exp.shape)}"
    gb, eb = bits(got).flatten(), bits(exp.to(got.device)).flatten()
    if torch.equal(gb, eb):
        return None
    diff = gb != eb
    if got.dtype == torch.bfloat16:
        diff &= ~(torch.isnan(got.flatten()) & torch.isnan(exp.to(got.device).flatten()))
        if not bool(diff.any()):
            return None
    i = int(torch.nonzero(diff)[0])
    mask = (1 << (8 * got.element_size())) - 1
    return (f"slot {name}: first difference at flat index {i} of {diff.numel()} (got bits 0x{int(gb[i]) & mask:x}, expected "
            f"0x{int(eb[i]) & mask:x}), {int(diff.sum())} elements differ")


# ----------------------------------------------------------------------------- directed fp32 inputs for a rounding target
# thresholds of the narrow types: e4m3fn largest finite 448, 464 is the tie that still rounds to 448, above it NaN (480 would be
# the next value); e5m2 largest finite 57344, 61440 the tie that rounds to infinity; fp16 65504 / 65520.
THRESHOLDS = (448.0, 464.0, 480.0, 57344.0, 61440.0, 65504.0, 65520.0, 65536.0)


def representable(target):
    """Every finite non-negative value of `target`, ascending, as fp32 (all of them are exact in fp32)."""
    if target.itemsize == 1:
        pat = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    else:
        pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = pat.view(target).to(torch.float32)
    v = v[torch.isfinite(v) & (v >= 0)]
    return torch.unique(v)                       # sorted; +0 and -0 collapse


def _next(x, up):
    a = x.numpy()
    return torch.from_numpy(np.nextafter(a, np.float32(np.inf if up else -np.inf), dtype=np.float32))


def directed_f32(target):
    """fp32 inputs that decide a conversion to `target` (bf16 / fp16 / e4m3fn / e5m2; fp32: the specials only): every
    representable value, every midpoint between neighbours (the subnormal grid included: it is part of the value list), one
    fp32 ulp either side of each midpoint, the first value beyond the largest finite one with its midpoint, the thresholds of
    all narrow types with their fp32 neighbours, signed zeros, infinities, NaNs of both signs and fp32 subnormals; each with
    both signs.  Returns (inputs, mids, lo_neighbour, hi_neighbour): the last three are the positive midpoints and the two
    representable values each lies between (self-checked in test_weights_cpu.py)."""
    sub = torch.tensor([1, 2, 0x7FFFFF, 0x400000, 0x800000, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    special = torch.cat((thr, _next(thr, False), _next(thr, True), sub,
                         torch.tensor([0.0, float("inf")], dtype=torch.float32),
                         torch.tensor([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA55AA5], dtype=torch.int32).view(torch.float32)))
    if target == torch.float32:
        x = special
        mids = lo = hi = torch.empty(0)
    else:
        v = representable(target)
        lo, hi = v[:-1], v[1:]
        mids = ((lo.double() + hi.double()) / 2).to(torch.float32)
        assert torch.equal(mids.double(), (lo.double() + hi.double()) / 2)       # midpoints are exact in fp32
        top = v[-1].double() + (v[-1].double() - v[-2].double())                 # where the next value would be
        over = torch.tensor([float((v[-1].double() + top) / 2), float(top)], dtype=torch.float32)
        over = over[torch.isfinite(over)]
        x = torch.cat((v, mids, _next(mids, False), _next(mids, True), over, _next(over, False), _next(over, True), special))
    return torch.cat((x, -x)), mids, lo, hi


def weight_order(sd, reverse):
    items = list(sd.items())
    return OrderedDict(reversed(items) if reverse else items)


BLOCK_W = re.compile(r"^(t\d+\.|s\d+\.|smod_all).*\.w$")      # the matrices an fp8 weight format keeps in fp8
