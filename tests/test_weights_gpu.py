"""The reference-keyed loader (csrc/weights.hip: foley_weights_begin / foley_load_tensor / foley_weights_end) slot by slot.

Every slot of the ctx-owned arena, found through foley_weights_slot, is compared BIT FOR BIT with host/packers.py applied to the
same state dict plus torch's CPU casts (tests/weights_ref.py, itself checked in test_weights_cpu.py); weight-normed DAC layers that
arrive as (g, v) pairs are held to a per-element bound against a float64 fold.  Real widths (1536 / 12 heads, 1408 / 11 heads,
the 2048-wide DAC decoder), the whole checkpoint-dtype x arena-configuration matrix on the tiny model, exhaustive conversion
tables, and the loader's refusals."""
import ctypes as CT
import dataclasses
from collections import OrderedDict

import pytest
import torch

import weights_ref as W
from conftest import record_parity
from foley_amd import nodes
from foley_amd.host import config as C, runtime as rt, synth

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- plumbing
def _begin(ctx, fmt=0):
    rt._check(ctx.lib, ctx.lib.foley_weights_begin(ctx._h, int(fmt)), "foley_weights_begin")


def _load(ctx, key, t):
    """One foley_load_tensor call; returns 0 / 1, raises FoleyRuntimeError on a refusal."""
    t = t.detach().to(ctx.device).contiguous()
    shape = (CT.c_int64 * max(t.dim(), 1))(*t.shape)
    with torch.cuda.device(ctx.device):
        rc = ctx.lib.foley_load_tensor(ctx._h, key.encode(), t.data_ptr(), rt.dt_of(t), t.dim(), shape, rt._stream())
        torch.cuda.current_stream().synchronize()
    if rc not in (0, 1):
        rt._check(ctx.lib, rc, f"foley_load_tensor({key})")
    return rc


def _end(ctx):
    with torch.cuda.device(ctx.device):
        rt._check(ctx.lib, ctx.lib.foley_weights_end(ctx._h, rt._stream()), "foley_weights_end")


def _arena_bytes(ctx):
    ptr, n = ctx.weights_arena()
    out = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    assert rt._hip().hipMemcpy(CT.c_void_p(out.data_ptr()), CT.c_void_p(ptr), CT.c_size_t(n), 3) == 0
    return out


def _check_geometry(ctx, table):
    """Slot set == the packers' key set with the same dtype and shape; extents 256-byte aligned, disjoint, inside the arena;
    lookup by name agrees with the enumeration."""
    slots = ctx.weights_slots()
    ptr, nbytes = ctx.weights_arena()
    assert ptr % 256 == 0
    names = [s["name"] for s in slots]
    assert len(set(names)) == len(names)
    assert set(names) == set(table), sorted(set(names) ^ set(table))
    for s in slots:
        dt, shape = table[s["name"]]
        assert (s["dtype"], s["shape"]) == (dt, shape), (s, dt, shape)
        assert s["bytes"] == W._numel(shape) * torch.empty((), dtype=dt).element_size() and s["bytes"] > 0
        assert s["offset"] % 256 == 0 and s["ptr"] == ptr + s["offset"], s
        assert ctx.weights_slot(s["name"]) == s
    by_off = sorted(slots, key=lambda s: s["offset"])
    for a, b in zip(by_off, by_off[1:]):
        assert a["offset"] + a["bytes"] <= b["offset"], (a, b)
    assert by_off[-1]["offset"] + by_off[-1]["bytes"] <= nbytes
    assert ctx.weights_slot("no.such.slot") is None and ctx.weights_slot(len(slots)) is None
    return slots


def _expected(packed32, table, cdt, fmt, dev, skip=()):
    return {k: W.expected_slot(k, packed32, table, cdt, fmt).to(dev) for k in table if k not in skip}


def _check_slots(ctx, slots, exp, pairs, tag):
    """Every slot against its expectation; returns {slot: error/bound ratio} of the weight-norm pairs."""
    fails, ratios = [], {}
    for s in slots:
        got = ctx.weights_slot_tensor(s["name"])
        if s["name"] in pairs:
            ratios[s["name"]], msg = W.wn_check(s["name"], got, *pairs[s["name"]])
        else:
            msg = W.mismatch(s["name"], got, exp[s["name"]])
        if msg:
            fails.append(msg)
    assert not fails, "%s: %d of %d slots wrong\n%s" % (tag, len(fails), len(slots), "\n".join(fails[:12]))
    return ratios


def _dac_state(dac_cfg, dev, gen, src=torch.float32, shift=0):
    """DAC decoder state dict: layer i spelled SPELLINGS[(i + shift) % 3], v before g on odd layers; (g, v) of moderate range so
    that a norm exists in every checkpoint dtype, everything else from `gen`."""
    schema = synth.dac_decoder_schema(dac_cfg)
    raw = OrderedDict()
    for k in schema:
        if ".parametrizations." in k:
            raw[k] = W.value_tensor(k, schema[k][0], dev, emin=-4, emax=4).to(src)
        else:
            raw[k] = gen(k, schema[k][0], dev)
    sp, pairs = W.respell_dac(raw, dac_cfg, lambda i: i + shift, v_first_of=lambda i: i % 2 == 1)
    return OrderedDict((k, v.to(src)) for k, v in sp.items()), pairs


def _two_orders(ctx, fmt, sd, dsd, exp, pairs, table, tag):
    """Load in schema order, then reversed on a second begin of the same context (a fresh arena); all slots after each: a store
    that strays into a neighbouring slot is caught by whichever order writes the neighbour first."""
    ratios = {}
    for rev in (False, True):
        n_ignored = ctx.load_reference_state([W.weight_order(sd, rev), W.weight_order(dsd, rev)], fmt)
        assert n_ignored == 0
        slots = _check_geometry(ctx, table)
        r = _check_slots(ctx, slots, exp, pairs, "%s, %s order" % (tag, "reversed" if rev else "schema"))
        ratios = {k: max(v, ratios.get(k, 0.0)) for k, v in r.items()}
    return ratios


# ----------------------------------------------------------------------------- (a) layout at real widths
@pytest.mark.parametrize("width,arena", [("xxl", "fp32"), ("xl", "fp32"), ("xl", "bf16+e4m3fn")])
def test_layout_at_real_widths(dev, width, arena):
    """XXL (1536, 12 heads) and XL (1408, 11 heads) at depth 1 + 2 with the full 2048-wide DAC decoder: the (H D K) -> (K H D)
    permutation, the 32-row SwiGLU interleave, tap-major convs, the smod_all block offset and the two-tap transposed-conv phases
    at their real strides.  fp32 arenas carry position-identifying values; the fp8 arena carries unrounded hashed values."""
    cfg = dataclasses.replace({"xxl": C.XXL, "xl": C.XL}[width], depth_triple=1, depth_single=2)
    _label, cdt, fmt = next(a for a in W.ARENAS if a[0] == arena)
    gen = W.ident_tensor if cdt == torch.float32 else W.value_tensor
    sd = W.make_state(synth.dit_schema(cfg), dev, gen=gen)
    dsd, pairs = _dac_state(C.DAC48K, dev, gen, shift={"xxl": 0, "xl": 1}[width])
    assert sum(k.endswith(".weight_g") for k in dsd) and sum(k.endswith(".weight") and k.startswith("decoder") for k in dsd)
    table = W.slot_table(cfg, C.DAC48K, cdt, fmt)
    p32 = W.expected_packed32(sd, dsd, cfg, C.DAC48K)
    exp = _expected(p32, table, cdt, fmt, dev, skip=pairs)
    del p32
    ctx = rt.FoleyContext(cfg, C.DAC48K, cdt, dev)
    try:
        ratios = _two_orders(ctx, fmt, sd, dsd, exp, pairs, table, f"{width} {arena}")
    finally:
        ctx.close()
        del exp, sd, dsd
        torch.cuda.empty_cache()
    print(f"{width} {arena}: {len(table)} slots, worst weight-norm error/bound {max(ratios.values()):.3f}")


# ----------------------------------------------------------------------------- (b) checkpoint dtype x arena configuration
_TINY_SRC = {}


def _tiny_source(dev, src):
    """TINY 2+2 + DAC_TINY checkpoint in dtype `src`: unrounded hashed values cast once by torch; (state dicts, pairs, packed32)."""
    if src not in _TINY_SRC:
        sd = OrderedDict((k, v.to(src)) for k, v in W.make_state(synth.dit_schema(C.TINY), dev, gen=W.value_tensor).items())
        dsd, pairs = _dac_state(C.DAC_TINY, dev, W.value_tensor, src=src, shift=2)
        _TINY_SRC[src] = (sd, dsd, pairs, W.expected_packed32(sd, dsd, C.TINY, C.DAC_TINY))
    return _TINY_SRC[src]


@pytest.mark.parametrize("arena", [a[0] for a in W.ARENAS])
@pytest.mark.parametrize("src", W.SOURCES, ids=lambda d: str(d).replace("torch.", ""))
def test_dtype_matrix(dev, src, arena):
    """Every checkpoint dtype into every arena configuration: the slot holds the tensor upcast exactly to fp32, then torch's cast
    to the slot dtype.  Nothing is pre-rounded to fp8; time0.b of an fp8 arena passes through fp8 first."""
    _label, cdt, fmt = next(a for a in W.ARENAS if a[0] == arena)
    sd, dsd, pairs, p32 = _tiny_source(dev, src)
    table = W.slot_table(C.TINY, C.DAC_TINY, cdt, fmt)
    assert table["cond1.w"][0] == cdt and table["audio_in.w"][0] == cdt and table["t0.a_qkv.w"][0] == (W.F8[fmt] or cdt)
    exp = _expected(p32, table, cdt, fmt, dev, skip=pairs)
    if fmt and src.itemsize > 1:                                               # the double rounding is part of the expectation
        assert not torch.equal(W.bits(exp["time0.b"]), W.bits(p32["time0.b"]))
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, cdt, dev)
    try:
        _two_orders(ctx, fmt, sd, dsd, exp, pairs, table, f"{src} -> {arena}")
    finally:
        ctx.close()


@pytest.mark.parametrize("arena", [a[0] for a in W.ARENAS if a[2]])
def test_fp8_arena_from_parameter_rounded_values(dev, arena):
    """The documented contract of the fp8 arenas: the caller hands over the values the reference module would hold - rounded to
    the parameter dtype (nodes.round_params), NOT to fp8.  The block matrices are torch's .to(float8_*) of those values and
    time0.b shows the double rounding parameter dtype -> fp8."""
    _label, cdt, fmt = next(a for a in W.ARENAS if a[0] == arena)
    raw, dsd, pairs, _p = _tiny_source(dev, torch.float32)
    # just above an fp8 tie: 1.0625 / 1.125 are the e4m3fn / e5m2 ties over 1.0; the 16-bit rounding lands ON the tie, which then
    # goes to the even 1.0, while a single rounding of the raw value goes up to 1.125 / 1.25
    raw, tb = OrderedDict(raw), "time_in.mlp.0.bias"
    raw[tb] = raw[tb].clone()
    raw[tb][:4] = torch.tensor([1.0625 + 2.0 ** -20, 1.125 + 2.0 ** -20, -1.0625 - 2.0 ** -20, -1.125 - 2.0 ** -20], device=dev)
    sd = nodes.round_params(raw, cdt)
    p32 = W.expected_packed32(sd, dsd, C.TINY, C.DAC_TINY)
    table = W.slot_table(C.TINY, C.DAC_TINY, cdt, fmt)
    exp = _expected(p32, table, cdt, fmt, dev, skip=pairs)
    once, i = raw[tb].cpu().to(W.F8[fmt]).to(torch.float32), fmt - 1
    assert float(exp["time0.b"][i]) == 1.0 and float(exp["time0.b"][i + 2]) == -1.0 and float(once[i]) == (1.125, 1.25)[i]
    w = exp["t0.a_qkv.w"]
    assert w.dtype == W.F8[fmt] and not torch.equal(w.float().cpu(), p32["t0.a_qkv.w"].cpu())   # the cast does round
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, cdt, dev)
    try:
        _two_orders(ctx, fmt, sd, dsd, exp, pairs, table, f"round_params({cdt}) -> {arena}")
    finally:
        ctx.close()


# ----------------------------------------------------------------------------- (c) conversion tables
_STORE = {  # store dtype -> (compute dtype, weight format, checkpoint key, slot): a slot of at least 65536 elements in that dtype
    torch.float32: (torch.float32, 0, "cond_in.linear_1.weight", "cond1.w"),
    torch.bfloat16: (torch.bfloat16, 0, "cond_in.linear_1.weight", "cond1.w"),
    torch.float16: (torch.float16, 0, "cond_in.linear_1.weight", "cond1.w"),
    torch.float8_e4m3fn: (torch.bfloat16, 1, "triple_blocks.0.audio_self_proj.weight", "t0.a_proj.w"),
    torch.float8_e5m2: (torch.float16, 2, "triple_blocks.0.audio_self_proj.weight", "t0.a_proj.w"),
}


@pytest.mark.parametrize("store", list(_STORE), ids=lambda d: str(d).replace("torch.", ""))
def test_conversion_tables(dev, store):
    """All 65536 bf16 and all 65536 fp16 bit patterns, all 256 patterns of each fp8 type and the directed fp32 set of the store
    type (weights_ref.directed_f32: every representable value, every midpoint and its fp32 neighbours, subnormals, thresholds,
    zeros, infinities, NaNs) through one slot into each of the five store dtypes; bytes against torch's CPU cast."""
    cdt, fmt, key, slot = _STORE[store]
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, cdt, dev)
    try:
        _begin(ctx, fmt)
        info = ctx.weights_slot(slot)
        n = W._numel(info["shape"])
        assert info["dtype"] == store and n >= 65536
        p16 = torch.arange(65536, dtype=torch.int32).to(torch.int16)
        p8 = torch.arange(256, dtype=torch.int32).to(torch.uint8)
        sources = [("bf16 patterns", p16.view(torch.bfloat16)), ("fp16 patterns", p16.view(torch.float16)),
                   ("e4m3fn patterns", p8.view(torch.float8_e4m3fn)), ("e5m2 patterns", p8.view(torch.float8_e5m2)),
                   ("directed fp32", W.directed_f32(store)[0])]
        fails, count = [], 0
        for label, pats in sources:
            for c0 in range(0, pats.numel(), n):
                chunk = pats[c0:c0 + n]
                count += chunk.numel()
                src = bits_tile(chunk, n).view(info["shape"])
                assert _load(ctx, key, src) == 0
                got = ctx.weights_slot_tensor(slot).cpu()
                msg = W.mismatch(f"{slot} <- {label}[{c0}:]", got, src.to(torch.float32).to(store))
                if msg and "flat index " not in msg:
                    fails.append(msg)
                elif msg:
                    i = int(msg.split("flat index ")[1].split(" ")[0])
                    fails.append("%s; source bits 0x%x" % (msg, int(W.bits(src).flatten()[i]) & ((1 << 8 * src.element_size()) - 1)))
        assert not fails, "\n".join(fails)
        print(f"{store}: {count} source values")
    finally:
        ctx.close()


def bits_tile(chunk, n):
    """`chunk` repeated to n elements (same dtype), on the CPU."""
    b = W.bits(chunk)
    return b.repeat((n + b.numel() - 1) // b.numel())[:n].contiguous().view(chunk.dtype)


# ----------------------------------------------------------------------------- (d) weight-norm fold
def test_weight_norm_fold_bound(dev):
    """Every weight-normed conv of the full DAC48K decoder handed over as a (g, v) pair, against float64 v * (g / ||v||):
    |got - ref| <= |ref| * (cols/2 + 6) * 2^-24 per element (derivation: weights_ref.wn_bound_factor), cols = numel(v) /
    v.shape[0].  The largest case is the first up-sampling transposed conv [2048, 1024, 16] (cols 16384, g per INPUT channel).
    The elements of each row of v span 2^40 in magnitude.  Both pair spellings, g first on even layers, v first on odd ones."""
    schema = synth.dac_decoder_schema(C.DAC48K)
    raw = OrderedDict()
    for k in schema:
        if k.endswith(W._V):
            raw[k] = W.value_tensor(k, schema[k][0], dev, emin=-20, emax=20)
        elif k.endswith(W._G):
            raw[k] = W.value_tensor(k, schema[k][0], dev, emin=-3, emax=3)
    assert tuple(raw["decoder.model.1.block.1" + W._V].shape) == (2048, 1024, 16)
    dsd, pairs = W.respell_dac(raw, C.DAC48K, lambda i: i % 2, v_first_of=lambda i: i % 2 == 1)
    assert len(pairs) == len(W.wn_layers(C.DAC48K)) == 1 + 5 * 7 + 1
    ctx = rt.FoleyContext(C.TINY, C.DAC48K, torch.float32, dev)
    worst, fails = {}, []
    try:
        _begin(ctx, 0)
        for k, t in dsd.items():
            assert _load(ctx, k, t) == 0, k
        for slot, (g, v, kind, s) in pairs.items():
            ratio, msg = W.wn_check(slot, ctx.weights_slot_tensor(slot), g, v, kind, s)
            label = "c7" if slot.endswith("c7.w") else "c1" if slot.endswith("c1.w") else slot.split(".")[-2] if kind != "out" else "out"
            label = {"up": "convT", "in": "in"}.get(label, label)
            worst[label] = max(worst.get(label, 0.0), ratio)
            if slot == "dac.0.up.w":
                worst["convT_2048x1024x16"] = ratio
            if msg:
                fails.append(msg)
    finally:
        ctx.close()
    print("weight-norm fold, largest error/bound per layer kind:", {k: round(v, 4) for k, v in sorted(worst.items())})
    record_parity("weights_wn_fold", **worst)
    assert not fails, "\n".join(fails)


# ----------------------------------------------------------------------------- (e) loader state machine
@pytest.fixture(scope="module")
def tiny32(dev):
    sd = W.make_state(synth.dit_schema(C.TINY), dev)
    dsd, pairs = _dac_state(C.DAC_TINY, dev, W.ident_tensor)
    table = W.slot_table(C.TINY, C.DAC_TINY, torch.float32, 0)
    exp = _expected(W.expected_packed32(sd, dsd, C.TINY, C.DAC_TINY), table, torch.float32, 0, dev, skip=pairs)
    return sd, dsd, pairs, table, exp


def _load_except(ctx, sds, drop=()):
    _begin(ctx, 0)
    for sd in sds:
        for k, t in sd.items():
            if k not in drop:
                assert _load(ctx, k, t) == 0, k


def test_repeated_key_overwrites_and_does_not_complete_twice(dev, tiny32):
    sd, dsd, pairs, table, exp = tiny32
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    try:
        w1, w3 = "single_blocks.0.linear2.w1.weight", "single_blocks.0.linear2.w3.weight"
        _load_except(ctx, [sd, dsd], drop=(w3,))
        assert _load(ctx, w1, sd[w1] + 1.0) == 0 and _load(ctx, w1, sd[w1]) == 0        # the same half three times
        with pytest.raises(rt.FoleyRuntimeError, match=r"'s0\.w13\.w'"):
            _end(ctx)
        assert _load(ctx, w3, sd[w3]) == 0
        _end(ctx)
        _check_slots(ctx, _check_geometry(ctx, table), exp, pairs, "after the repeated key")  # the last delivery of w1 holds
    finally:
        ctx.close()


@pytest.mark.parametrize("missing,named", [
    ("single_blocks.1.linear2.w3.weight", r"'s1\.w13\.w'"),                   # one half of a SwiGLU pair
    ("single_blocks.1.modulation.linear.weight", r"'smod_all\.w'"),          # one block of the fused modulation matrix
    ("single_blocks.0.modulation.linear.bias", r"'smod_all\.b'"),
    ("decoder.model.2.block.1.weight", r"'dac\.1\.up\.w'"),                   # both tap halves come from this one tensor
    ("decoder.model.1.block.1.weight_v", r"pair incomplete: decoder\.model\.1\.block\.1\."),     # g without its v
    ("decoder.model.3.block.1.parametrizations.weight.original0", r"pair incomplete: decoder\.model\.3\.block\.1\."),
])
def test_weights_end_names_what_is_missing(dev, tiny32, missing, named):
    """foley_weights_end names an incomplete slot or a half-delivered weight-norm pair.  (The two tap halves of an up.w are
    written by one call from one tensor, so the interface cannot deliver one without the other: the missing tensor and the
    half-delivered pair of a transposed conv are the cases that exist.)"""
    sd, dsd, _pairs, _table, _exp = tiny32
    assert missing in sd or missing in dsd
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    try:
        _load_except(ctx, [sd, dsd], drop=(missing,))
        with pytest.raises(rt.FoleyRuntimeError, match=named):
            _end(ctx)
    finally:
        ctx.close()


def test_shapes_indices_and_foreign_keys(dev, tiny32):
    """Trailing singleton dimensions are accepted; wrong shapes and block indices beyond the depth are refused by name; keys
    outside the sampling path return 1 and change no byte of the arena; a second foley_weights_begin gives a fresh arena that
    loads completely; an fp8 weight format on an fp32 context is refused."""
    sd, dsd, pairs, table, exp = tiny32
    ctx = rt.FoleyContext(C.TINY, C.DAC_TINY, torch.float32, dev)
    try:
        with pytest.raises(rt.FoleyRuntimeError, match="foley_weights_begin has not been called"):
            _load(ctx, "cond_in.linear_1.bias", sd["cond_in.linear_1.bias"])
        with pytest.raises(rt.FoleyRuntimeError, match="fp8 weight storage needs"):
            _begin(ctx, 1)
        _begin(ctx, 0)
        for k, t in list(sd.items()) + list(dsd.items()):                     # every tensor with trailing singleton dimensions
            assert _load(ctx, k, t.reshape(*t.shape, 1, 1) if t.dim() <= 6 else t) == 0, k
        _end(ctx)
        slots = _check_geometry(ctx, table)
        _check_slots(ctx, slots, exp, pairs, "trailing singleton dimensions")
        before = _arena_bytes(ctx)
        D = C.TINY.hidden
        for key, t in (("triple_blocks.0.audio_mlp.fc1.weight", torch.zeros(7, 5)),
                       ("single_blocks.0.linear_qkv.weight", torch.zeros(D, 3 * D)),
                       ("single_blocks.1.linear2.w1.weight", torch.zeros(C.TINY.conv_hidden, D)),
                       ("single_blocks.0.modulation.linear.bias", torch.zeros(6 * D + 1)),
                       ("cond_in.linear_1.weight", torch.zeros(1, D, C.TINY.cond_dim)),
                       ("decoder.model.1.block.1.weight", torch.zeros(512, 1024, 16)),
                       ("decoder.model.0.bias", torch.zeros(3))):
            with pytest.raises(rt.FoleyRuntimeError, match=f"'{key}' has an unexpected shape".replace(".", r"\.")):
                _load(ctx, key, t)
        for key in ("triple_blocks.2.audio_mod.linear.weight", "single_blocks.2.linear1.bias", "single_blocks.36.q_norm.weight",
                    "triple_blocks.-1.audio_mod.linear.bias"):
            with pytest.raises(rt.FoleyRuntimeError, match="block index out of range: " + key.replace(".", r"\.")):
                _load(ctx, key, torch.zeros(4))
        enc = W.make_state(synth.dac_encoder_schema(C.DAC_TINY), dev, gen=W.value_tensor)
        foreign = list(enc.items()) + [("quantizer.in_proj.weight", torch.ones(8, 8)), ("triple_blocks.0.no_such.weight", torch.ones(3)),
                                       ("decoder.model.9.weight", torch.ones(4)), ("single_blocks.0.linear2.w4.weight", torch.ones(2))]
        for k, t in foreign:
            assert _load(ctx, k, t) == 1, k
        assert _load(ctx, "final_layer.adaLN_modulation.1.weight", torch.ones(2)) == 0          # dead weights: accepted, unused
        assert torch.equal(_arena_bytes(ctx), before)                                            # none of them touched a slot
        _end(ctx)
        # a second begin on the same context: fresh arena, nothing counted from before
        _begin(ctx, 0)
        with pytest.raises(rt.FoleyRuntimeError, match="was not \\(fully\\) loaded"):
            _end(ctx)
        assert ctx.load_reference_state([W.weight_order(sd, True), dsd], 0) == 0
        _check_slots(ctx, _check_geometry(ctx, table), exp, pairs, "second foley_weights_begin")
    finally:
        ctx.close()
