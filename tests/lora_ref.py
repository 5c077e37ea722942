"""CPU restatement of the LoRA merge (csrc/lora.hip, host/lora.py) and the helpers the two lora test files share.

    stored'[o, c] = rnd_store( f32(pristine[o, c]) + sum_j s_j * sum_q up_j[o, q] * down_j[q, c] ),   c over the flattened (I, k)
    s_j = fl32(strength_j * alpha_j / r_j)   (no alpha: fl32(strength_j))

merge64 states the sum in fp64 in CHECKPOINT layout; the packed position of every element comes from host/packers.py itself
(slot_index packs tensors whose values name their source), never from a second copy of the layout rules.

Bound per element (derived, no share of elements exempt):  |got - ref64| <= (R_tot + 4) * U32 * mag + output term, with
mag = |pristine| + sum_j |s_j| * (|up_j| @ |down_j|), R_tot the summed ranks, U32 = 2^-23 (opcheck.U32, twice the fp32 unit
roundoff).  The kernel rounds s_j * up once per term (1 u each), runs one FMA chain of R_tot roundings over partial sums that
never exceed mag - |pristine|, and adds the pristine value once: (R_tot + 2) u * mag to first order with u = 2^-24, so the
factor R_tot + 4 in units of 2 u leaves more than a factor of two for the second-order terms.  The output term is half an ulp of
the store type at max(|ref|, |got|) times (1 + 2^-6): opcheck.output_term for the 16-bit types and fp32 (zero), ulp8 below for
the fp8 types (significand 4 bits for e4m3fn, 3 for e5m2, floors at the subnormal spacings 2^-9 and 2^-16)."""
from collections import OrderedDict

import torch

import opcheck as oc
from foley_amd.host import packers, synth
from test_weights_cpu import DAC_MINI, MINI  # noqa: F401  (the one definition of the mini configuration)

F8_SIG = {torch.float8_e4m3fn: (4, 2.0 ** -9), torch.float8_e5m2: (3, 2.0 ** -16)}   # significand bits (implicit one included), subnormal spacing


def fl32(x):
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


def scale_of(strength, alpha, rank):
    """s = fl32(strength * alpha / rank) formed in fp64; no alpha: fl32(strength)."""
    return fl32(strength) if alpha is None else fl32(float(strength) * float(alpha) / int(rank))


def merge64(sd_stored, adapters):
    """sd_stored {key: W[O, I(, k)]} - the values the arena holds (already rounded to the store type), checkpoint layout;
    adapters {key: [(down [r, I(, k)], up [O, r(, 1)], s), ...]} in list order.  Returns ({key: fp64 merged}, {key: mag})."""
    ref, mag = OrderedDict(), OrderedDict()
    for key, lst in adapters.items():
        w = sd_stored[key].to(torch.float32).double()
        flat = w.reshape(w.shape[0], -1)
        r64, m64 = flat.clone(), flat.abs()
        for down, up, s in lst:
            d = down.to(torch.float32).double().reshape(down.shape[0], -1)
            u = up.to(torch.float32).double().reshape(up.shape[0], -1)
            r64 = r64 + float(s) * (u @ d)
            m64 = m64 + abs(float(s)) * (u.abs() @ d.abs())
        ref[key], mag[key] = r64.reshape(w.shape), m64.reshape(w.shape)
    return ref, mag


def ulp8(x, dtype):
    sig, floor = F8_SIG[dtype]
    x = x.double().abs()
    _, e = torch.frexp(x.clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x), e - sig).clamp_min(floor)


def output_term(ref, got, dtype):
    if dtype in F8_SIG:
        return 0.5 * (1 + 2.0 ** -6) * ulp8(torch.maximum(ref.double().abs(), got.double().abs()), dtype)
    return oc.output_term(ref, got, dtype)


def bound(ref, got, mag, r_tot, dtype):
    return (r_tot + 4) * oc.U32 * mag + output_term(ref, got, dtype)


def seq_merge32(w_stored, lst, dtype):
    """A sequential fp32 merge as a kernel may run it: s * up rounded, one fused chain over (j, q), one add, one store rounding."""
    w = w_stored.to(torch.float32)
    acc = torch.zeros(w.shape[0], w[0].numel(), dtype=torch.float64)
    for down, up, s in lst:
        d = down.to(torch.float32).reshape(down.shape[0], -1)
        u = (up.to(torch.float32).reshape(up.shape[0], -1) * torch.tensor(s, dtype=torch.float32))
        for q in range(d.shape[0]):      # fma: the exact product added in fp64, rounded once to fp32
            acc = (acc + u[:, q:q + 1].double() * d[q:q + 1].double()).to(torch.float32).double()
    return (w.reshape(acc.shape) + acc.to(torch.float32)).to(dtype).reshape(w.shape)


# ----------------------------------------------------------------------------- packed positions, through the packers
def slot_index(cfg, keys, device="cpu"):
    """{packed name: (which, flat)} for the packed tensors that hold an element of any of `keys`: which[i] = 1 + the ordinal in
    `keys` of the checkpoint tensor element i comes from (0: none of them), flat[i] = its flat index in that tensor.  Built by
    running host/packers.pack_dit on tensors whose values say where they come from (exact in fp32: below 2^24)."""
    schema = synth.dit_schema(cfg)
    which, flat = OrderedDict(), OrderedDict()
    for k, (shape, _s, _m) in schema.items():
        n = 1
        for v in shape:
            n *= int(v)
        if k in keys:
            assert n < (1 << 24), (k, n)
            which[k] = torch.full(shape, float(keys.index(k) + 1), device=device)
            flat[k] = torch.arange(n, dtype=torch.float32, device=device).view(shape)
        else:
            which[k] = flat[k] = torch.zeros(shape, device=device)
    pw, pf = packers.pack_dit(which, cfg, torch.float32), packers.pack_dit(flat, cfg, torch.float32)
    return OrderedDict((name, (pw[name].long(), pf[name].long())) for name in pw if bool((pw[name] != 0).any()))


def unroute(index, keys, shapes, slots):
    """Checkpoint-layout tensors of `keys` read out of packed tensors `slots` {name: tensor} (fp32 values of what is stored)."""
    out = OrderedDict()
    for i, k in enumerate(keys):
        n = 1
        for v in shapes[k]:
            n *= int(v)
        t = torch.zeros(n, dtype=torch.float32, device=next(iter(slots.values())).device)
        for name, (which, flat) in index.items():
            m = which == i + 1
            if bool(m.any()):
                t[flat[m]] = slots[name].to(torch.float32)[m]
        out[k] = t.view(shapes[k])
    return out


def route(index, keys, name, base, per_key):
    """Packed image of `name`: `base` (fp64, packed shape) with the elements of every key replaced by per_key[key] (checkpoint layout)."""
    which, flat = index[name]
    out = base.double().clone()
    for i, k in enumerate(keys):
        m = which == i + 1
        if bool(m.any()):
            out[m] = per_key[k].double().reshape(-1).to(out.device)[flat[m]]
    return out


# ----------------------------------------------------------------------------- synthetic adapters
def make_adapter(shapes, key_ranks, dtype=torch.float32, seed=0, alpha=None, amp=0.5):
    """{key: (down, up, alpha)} for {key: rank}: down [r, I(, k)], up [O, r(, 1)] with entries of order amp / sqrt(r), so that the
    product is a visible fraction of an order-one weight."""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    for key, r in key_ranks.items():
        shape = tuple(shapes[key])
        down = torch.randn((r,) + shape[1:], generator=g) * amp
        up = torch.randn((shape[0], r) + (1,) * (len(shape) - 2), generator=g) * (amp / r ** 0.5)
        out[key] = (down.to(dtype), up.to(dtype), alpha)
    return out


def spell(adapter, style, prefix=""):
    """One parsed adapter {ref key: (down, up, alpha)} written in one of the spellings in circulation."""
    sd = OrderedDict()
    for key, (down, up, alpha) in adapter.items():
        module = key[:-len(".weight")]
        if style == "peft":
            sd[prefix + module + ".lora_A.weight"], sd[prefix + module + ".lora_B.weight"] = down, up
            assert alpha is None
            continue
        base = (prefix + module) if style == "comfy" else "lora_unet_" + module.replace(".", "_")
        sd[base + ".lora_down.weight"], sd[base + ".lora_up.weight"] = down, up
        if alpha is not None:
            sd[base + ".alpha"] = torch.tensor(float(alpha))
    return sd
