"""The expected-arena helper of the loader tests (tests/weights_ref.py), checked without a GPU.

test_weights_gpu.py trusts weights_ref for the value every slot must hold.  Here the helper is held against plain per-element
index formulas written as loops from the layout descriptions (DESIGN.md "data layout", include/foley_hip.h, the docstrings
of host/packers.py) - no tensor permutes - and the directed fp32 rounding set is checked against torch's own casts."""
import dataclasses
import zlib

import pytest
import torch

import weights_ref as W
from foley_amd.host import config as C, packers, synth

# shapes small enough for Python loops, but with every stride distinct: 2 heads x head_dim 16, hidden 32 (the SwiGLU group), conv
# hidden 256 = four 64-row groups
MINI = dataclasses.replace(C.TINY, name="mini", depth_triple=1, depth_single=2, hidden=32, heads=2, mlp_ratio=1, cond_dim=6,
                           clip_dim=5, sync_dim=7, latent_dim=3, time_freq_dim=4)
DAC_MINI = C.DACConfig(latent_dim=3, decoder_dim=8, rates=(3, 2), encoder_dim=4, encoder_rates=(2, 3))


@pytest.fixture(scope="module")
def mini():
    assert MINI.conv_hidden % 64 == 0 and MINI.sync_hidden % 64 == 0
    sd = W.make_state(synth.dit_schema(MINI), "cpu")
    dsd = W.make_state(synth.dac_decoder_schema(DAC_MINI), "cpu")
    folded, pairs = W.respell_dac(dsd, DAC_MINI, lambda i: 2)          # every layer folded: bitwise everywhere
    assert not pairs
    return sd, folded, W.expected_packed32(sd, folded, MINI, DAC_MINI)


def test_ident_values_name_their_position():
    t, u = W.ident_tensor("k", (3, 5, 7), "cpu"), W.ident_tensor("other", (3, 5, 7), "cpu")
    rot = lambda key: zlib.crc32(key.encode()) & 0xFFFFFF
    assert t.flatten().tolist() == [(i + rot("k")) % (1 << 24) for i in range(105)] and not torch.equal(t, u)
    a, b = W.value_tensor("a", (4096,), "cpu"), W.value_tensor("b", (4096,), "cpu")
    assert torch.isfinite(a).all() and not torch.equal(a, b) and a.unique().numel() == 4096
    for dt in (torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2):       # not pre-rounded to anything
        assert (a.to(dt).to(torch.float32) != a).float().mean() > 0.9
    assert a.abs().max() > 65520 and a.abs().min() < 2.0 ** -24 and bool((a < 0).any())


def test_qkv_rows_hdk_to_khd(mini):
    """linear_qkv rows arrive packed (H D K) - q/k/v innermost - and are stored (K H D)."""
    sd, _dsd, exp = mini
    D, H, hd = MINI.hidden, MINI.heads, MINI.head_dim
    for b in range(MINI.depth_single):
        w, bias = sd[f"single_blocks.{b}.linear_qkv.weight"], sd[f"single_blocks.{b}.linear_qkv.bias"]
        for k in range(3):
            for h in range(H):
                for d in range(hd):
                    src, dst = (h * hd + d) * 3 + k, (k * H + h) * hd + d
                    assert float(exp[f"s{b}.qkv.b"][dst]) == float(bias[src])
                    for c in range(D):
                        assert float(exp[f"s{b}.qkv.w"][dst, c]) == float(w[src, c])


def test_conv_tap_major(mini):
    """[out, in, k] conv weights become [out, k*in] with K index = tap*in + c (linear1, w2, every DAC conv)."""
    sd, dsd, exp = mini
    cases = [(sd["single_blocks.1.linear1.weight"], exp["s1.lin1.w"]), (sd["single_blocks.0.linear2.w2.weight"], exp["s0.w2.w"]),
             (dsd["decoder.model.0.weight"], exp["dac.in.w"]), (dsd["decoder.model.1.block.2.block.1.weight"], exp["dac.0.0.c7.w"]),
             (dsd["decoder.model.2.block.4.block.3.weight"], exp["dac.1.2.c1.w"])]
    for w, p in cases:
        O, I, K = w.shape
        assert tuple(p.shape) == (O, K * I)
        for o in range(O):
            for t in range(K):
                for c in range(I):
                    assert float(p[o, t * I + c]) == float(w[o, c, t])


def test_gate_interleave_32_rows(mini):
    """SwiGLU pairs: packed row 64*g + r is w1 row 32*g + r, packed row 64*g + 32 + r is w3 row 32*g + r (r < 32); conv pairs are
    tap-major first."""
    sd, _dsd, exp = mini
    for name, k1, k3 in (("s1.w13.w", "single_blocks.1.linear2.w1.weight", "single_blocks.1.linear2.w3.weight"),
                         ("vis.w13.w", "visual_proj.w1.weight", "visual_proj.w3.weight"),
                         ("sync.w13.w", "sync_in.2.w1.weight", "sync_in.2.w3.weight")):
        w1, w3, p = sd[k1], sd[k3], exp[name]
        Hh, I = w1.shape[0], w1.shape[1]
        K = w1.shape[2] if w1.dim() == 3 else 1
        assert tuple(p.shape) == (2 * Hh, K * I)
        for row in range(2 * Hh):
            g, r = divmod(row, 64)
            src = (w1 if r < 32 else w3).reshape(Hh, I, K)
            for t in range(K):
                for c in range(I):
                    assert float(p[row, t * I + c]) == float(src[32 * g + r % 32, c, t])


def test_smod_blocks_are_stacked(mini):
    sd, _dsd, exp = mini
    D = MINI.hidden
    for b in range(MINI.depth_single):
        for r in range(6 * D):
            assert float(exp["smod_all.b"][b * 6 * D + r]) == float(sd[f"single_blocks.{b}.modulation.linear.bias"][r])
            for c in range(D):
                assert float(exp["smod_all.w"][b * 6 * D + r, c]) == float(sd[f"single_blocks.{b}.modulation.linear.weight"][r, c])


def test_transposed_conv_phases_bias_repeat_and_output_conv(mini):
    """ConvTranspose1d [Cin, Cout, 2s] -> [s*Cout, 2*Cin]: row p*Cout + co, columns [x[q-1] | x[q]] hold taps (p + s | p); its bias
    is repeated once per phase; the output conv [1, C, 7] is stored [7][C]."""
    _sd, dsd, exp = mini
    cin = DAC_MINI.decoder_dim
    for i, s in enumerate(DAC_MINI.rates):
        cout = cin // 2
        w, bias = dsd[f"decoder.model.{i + 1}.block.1.weight"], dsd[f"decoder.model.{i + 1}.block.1.bias"]
        p, pb = exp[f"dac.{i}.up.w"], exp[f"dac.{i}.up.b"]
        assert tuple(w.shape) == (cin, cout, 2 * s) and tuple(p.shape) == (s * cout, 2 * cin) and tuple(pb.shape) == (s * cout,)
        for ph in range(s):
            for co in range(cout):
                assert float(pb[ph * cout + co]) == float(bias[co])
                for ci in range(cin):
                    assert float(p[ph * cout + co, ci]) == float(w[ci, co, ph + s])
                    assert float(p[ph * cout + co, cin + ci]) == float(w[ci, co, ph])
        cin = cout
    wo, po = dsd[f"decoder.model.{len(DAC_MINI.rates) + 2}.weight"], exp["dac.out.w"]
    assert tuple(wo.shape) == (1, cin, 7) and tuple(po.shape) == (7 * cin,)
    for t in range(7):
        for c in range(cin):
            assert float(po[t * cin + c]) == float(wo[0, c, t])


def test_wn_layout_map_agrees_with_pack_dac(mini):
    """wn_layers / wn_layout (the float64 reference's route into the packed layout) give pack_dac's own slots on a folded
    checkpoint, and every weight-normed key of the schema is in the map."""
    _sd, dsd, exp = mini
    layers = W.wn_layers(DAC_MINI)
    assert {b for b, *_ in layers} == {k[:-len(".weight")] for k in dsd if k.endswith(".weight") and k.startswith("decoder.")}
    for base, slot, kind, s in layers:
        assert torch.equal(W.wn_layout(dsd[base + ".weight"], kind, s), exp[slot]), slot
    # a pair spelled either way folds to the same float64 reference, and the packers' fp32 fold is inside the bound
    raw = W.make_state(synth.dac_decoder_schema(DAC_MINI), "cpu", gen=W.value_tensor, emin=-6, emax=6)
    sp, pairs = W.respell_dac(raw, DAC_MINI, lambda i: i, v_first_of=lambda i: i % 2 == 1)
    assert len(pairs) == len(layers) - (len(layers) + 0) // 3 and any(k.endswith(".weight_g") for k in sp)
    keys = list(sp)
    assert keys.index("decoder.model.0.parametrizations.weight.original0") < keys.index("decoder.model.0.parametrizations.weight.original1")
    assert keys.index("decoder.model.1.block.1.weight_v") < keys.index("decoder.model.1.block.1.weight_g")
    packed = packers.pack_dac(sp, DAC_MINI)
    for slot, (g, v, kind, s) in pairs.items():
        ratio, msg = W.wn_check(slot, packed[slot], g, v, kind, s)
        assert msg is None and ratio <= 1.0, msg
        _r, msg = W.wn_check(slot, packed[slot] * (1 + 2.0 ** -12), g, v, kind, s)
        assert msg is not None and slot in msg                              # the bound is tight enough to see a 2^-12 error


def test_expected_slot_dtypes_and_time0_double_rounding():
    sd = W.make_state(synth.dit_schema(MINI), "cpu", gen=W.value_tensor, emin=-12, emax=8)
    p32 = W.expected_packed32(sd, None, MINI, DAC_MINI)
    for _label, cdt, fmt in W.ARENAS:
        table = W.slot_table(MINI, DAC_MINI, cdt, fmt)
        assert set(p32) <= set(table)
        for name in p32:
            e = W.expected_slot(name, p32, table, cdt, fmt)
            want = W.F8[fmt] if (fmt and W.BLOCK_W.match(name)) else cdt if name.endswith(".w") else torch.float32
            assert e.dtype == want == table[name][0], (name, e.dtype, want)
        for name in ("cond1.w", "audio_in.w", "final.w", "vis.w13.w"):      # the small embedders stay in the compute dtype
            assert table[name][0] == cdt
        b = W.expected_slot("time0.b", p32, table, cdt, fmt)
        if fmt:
            twice = p32["time0.b"].to(W.F8[fmt]).to(torch.float32)
            assert torch.equal(W.bits(b), W.bits(twice)) and not torch.equal(W.bits(b), W.bits(p32["time0.b"]))
        else:
            assert torch.equal(b, p32["time0.b"])


def test_mismatch_reports_slot_index_and_count():
    a = torch.arange(12, dtype=torch.float32).view(3, 4)
    b = a.clone()
    assert W.mismatch("x", a, b) is None
    b[1, 2] = -b[1, 2]
    b[2, 3] += 1
    msg = W.mismatch("s0.qkv.w", a, b)
    assert "s0.qkv.w" in msg and "index 6 " in msg and "2 elements" in msg
    z = torch.zeros(4)
    assert W.mismatch("z", z, -z) is not None                               # signed zeros count
    n1 = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)
    n2 = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert W.mismatch("n", n1, n2) is not None                              # NaN payloads count ...
    h1 = torch.tensor([0x7FC0], dtype=torch.int16).view(torch.bfloat16)
    h2 = torch.tensor([-1], dtype=torch.int16).view(torch.bfloat16)
    assert W.mismatch("h", h1, h2) is None                                  # ... except bf16, where torch has two answers
    assert W.mismatch("h", h1, torch.tensor([1.0], dtype=torch.bfloat16)) is not None


@pytest.mark.parametrize("target", [torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2])
def test_directed_set_self_check(target):
    """Every midpoint lies between two ADJACENT representable values under torch's cast: one fp32 ulp below it rounds to the
    lower, one above to the upper, the tie itself to the one with the even mantissa."""
    x, mids, lo, hi = W.directed_f32(target)
    cast = lambda t: t.to(target).to(torch.float32)
    v = W.representable(target)
    assert torch.equal(cast(v), v) and mids.numel() == v.numel() - 1
    assert torch.equal(cast(W._next(mids, False)), lo) and torch.equal(cast(W._next(mids, True)), hi)
    assert bool(((lo < mids) & (mids < hi)).all())
    tie = cast(mids)
    assert bool(((tie == lo) | (tie == hi)).all())
    even = (W.bits(tie.to(target)).to(torch.int32) & 1) == 0
    assert bool(even.all())
    # no representable value between the two neighbours
    assert torch.equal(lo, v[:-1]) and torch.equal(hi, v[1:])
    # subnormal grid and first normal are in the list
    sub = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float8_e4m3fn: 2.0 ** -9, torch.float8_e5m2: 2.0 ** -16}
    assert float(v[1]) == sub[target]
    xs = set(x.tolist())
    for t in W.THRESHOLDS:
        assert t in xs and -t in xs
    assert float("inf") in xs and float("-inf") in xs and bool(torch.isnan(x).any())
    assert bool((W.bits(x) == -(1 << 31)).any()) and bool((W.bits(x) == 0).any())          # -0 and +0


def test_threshold_behaviour_of_the_reference_casts():
    """The torch casts the GPU test compares with: 464 -> 448 and anything above is NaN (e4m3fn); 61440 and up -> inf (e5m2)."""
    f = lambda v, dt: torch.tensor([v], dtype=torch.float32).to(dt).to(torch.float32)
    up = lambda v: float(W._next(torch.tensor([v], dtype=torch.float32), True))
    dn = lambda v: float(W._next(torch.tensor([v], dtype=torch.float32), False))
    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    assert float(f(448.0, e4)) == 448 and float(f(464.0, e4)) == 448 and bool(torch.isnan(f(up(464.0), e4)))
    assert bool(torch.isnan(f(480.0, e4))) and bool(torch.isnan(f(float("inf"), e4)))
    assert float(f(57344.0, e5)) == 57344 and float(f(dn(61440.0), e5)) == 57344 and float(f(61440.0, e5)) == float("inf")
    assert float(f(65520.0, torch.float16)) == float("inf") and float(f(dn(65520.0), torch.float16)) == 65504
