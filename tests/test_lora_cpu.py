"""LoRA on the host, without a GPU: the three adapter spellings, every refusal that needs no device, the fingerprint logic of
lora.ensure against a stub context, and the fp64 restatement (tests/lora_ref.py) by hand and against a sequential fp32 merge."""
import os
import re
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

import lora_ref as LR
from abi_pin import assert_abi_version
from foley_amd.host import lora, runtime as rt, synth

MINI = LR.MINI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {k: v[0] for k, v in synth.dit_schema(MINI).items()}
KEYS = {"single_blocks.1.linear2.w1.weight": 5, "triple_blocks.0.v_cond_attn_qkv.weight": 1, "triple_blocks.0.audio_mlp.fc1.weight": 16,
        "visual_proj.w3.weight": 2, "single_blocks.0.linear1.weight": 3}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) and a[k][2] == b[k][2], k


# ----------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_three_spellings_parse_to_the_same_adapter(dtype):
    plain = LR.make_adapter(SHAPES, KEYS, dtype)
    with_alpha = LR.make_adapter(SHAPES, KEYS, dtype, alpha=4.0)
    for prefix in ("",) + lora.PREFIXES + ("base_model.model.diffusion_model.",):
        _same(lora.load(LR.spell(plain, "peft", prefix), MINI), plain)
        _same(lora.load(LR.spell(with_alpha, "comfy", prefix), MINI), with_alpha)
    _same(lora.load(LR.spell(with_alpha, "kohya"), MINI), with_alpha)
    _same(lora.load(LR.spell(plain, "kohya"), MINI), plain)
    got = lora.load(LR.spell(plain, "kohya"), MINI)
    assert all(v[0].dtype == dtype for v in got.values())


def test_kohya_names_resolve_through_the_module_table():
    table = lora.kohya_table(MINI)
    assert table["single_blocks_1_linear2_w1"] == "single_blocks.1.linear2.w1"
    assert table["triple_blocks_0_v_cond_attn_qkv"] == "triple_blocks.0.v_cond_attn_qkv"
    assert table["triple_blocks_0_audio_mlp_fc1"] == "triple_blocks.0.audio_mlp.fc1"
    assert len(table) == len(lora.modules(MINI))                      # no two modules collapse to one spelling
    ad = LR.make_adapter(SHAPES, {"triple_blocks.0.audio_mlp.fc1.weight": 2})
    assert list(lora.load(LR.spell(ad, "kohya"), MINI)) == ["triple_blocks.0.audio_mlp.fc1.weight"]
    assert all(not m.endswith("norm") and "bias" not in m for m in lora.modules(MINI))


def test_alpha_over_rank_and_missing_alpha():
    assert lora.scale_of(0.8, None, 16) == LR.fl32(0.8) == LR.scale_of(0.8, None, 16)
    assert lora.scale_of(0.8, 4.0, 16) == LR.fl32(0.8 * 4.0 / 16) == LR.scale_of(0.8, 4.0, 16)
    assert lora.scale_of(-0.3, 7.0, 3) == LR.fl32(-0.3 * 7.0 / 3)
    key = "single_blocks.1.linear2.w1.weight"
    for alpha, want in ((None, LR.fl32(0.5)), (10.0, LR.fl32(0.5 * 10.0 / 5))):
        sd = LR.spell(LR.make_adapter(SHAPES, {key: 5}, alpha=alpha), "comfy")
        (_d, _u, s), = lora.plan_merge([(sd, 0.5)], MINI)[key]
        assert s == want


# ----------------------------------------------------------------------------- refusals that need no device
def _one(key="triple_blocks.0.audio_cross_q.weight", r=2, **kw):
    return LR.make_adapter(SHAPES, {key: r}, **kw)


@pytest.mark.parametrize("extra,reason", [
    ("triple_blocks.0.audio_cross_q.dora_scale", "DoRA"), ("triple_blocks.0.audio_cross_q.lokr_w1", "LoKr"),
    ("triple_blocks.0.audio_cross_q.hada_w1_a", "LoHa"), ("triple_blocks.0.audio_cross_q.lora_mid.weight", "lora_mid"),
    ("triple_blocks.0.audio_cross_q.diff", "diffs"), ("triple_blocks.0.audio_cross_q.diff_b", "diffs"),
    ("triple_blocks.0.audio_cross_q.weight", "not an adapter tensor"),
    ("triple_blocks.7.audio_cross_q.lora_A.weight", "resolves to no module"),                 # block beyond the depth
    ("triple_blocks.0.audio_cross_q_norm.lora_A.weight", "resolves to no module"),            # a norm gain
    ("lora_unet_triple_blocks_0_audio_cross.lora_down.weight", "resolves to no module"),
    ("decoder.model.0.lora_A.weight", "resolves to no module"),                               # the DAC
    ("sync_pos_emb.lora_A.weight", "resolves to no module"),
])
def test_parser_refuses_by_name(extra, reason):
    sd = LR.spell(_one(), "peft")
    sd[extra] = torch.zeros(2, 2)
    with pytest.raises(lora.LoraError, match=re.escape(extra) + ".*" + reason):
        lora.load(sd, MINI)


def test_one_half_of_a_pair_is_refused():
    sd = LR.spell(_one(), "peft")
    del sd["triple_blocks.0.audio_cross_q.lora_B.weight"]
    with pytest.raises(lora.LoraError, match=r"triple_blocks\.0\.audio_cross_q\.weight.*only one half"):
        lora.load(sd, MINI)


def test_plan_refuses_what_the_library_would():
    key = "single_blocks.0.linear1.weight"                     # [32, 32, 3]
    good = _one(key, 2)
    d, u, _a = good[key]

    def refused(down, up, reason, n=1, strength=1.0):
        sd = LR.spell({key: (down, up, None)}, "peft")
        with pytest.raises(lora.LoraError, match=re.escape(key) + ".*" + reason):
            lora.plan_merge([(sd, strength)] * n, MINI)

    refused(d[:, :, :2].contiguous(), u, "shape does not match")
    refused(d, u[:5].contiguous(), "shape does not match")
    refused(d, u.expand(-1, -1, 3).contiguous(), "kernel > 1")
    refused(torch.zeros(0, 32, 3), torch.zeros(32, 0, 1), r"rank must be in \[1, 256\]")
    refused(torch.zeros(257, 32, 3), torch.zeros(32, 257, 1), r"rank must be in \[1, 256\]")
    refused(d.double(), u.double(), "operand dtype")
    refused(d.half(), u, "operand dtype")
    refused(d, u, "more than 8 adapters", n=9)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(lora.LoraError, match="not finite"):
            lora.normalize([(LR.spell(good, "peft"), bad)])
    assert len(lora.plan_merge([(LR.spell(good, "peft"), 1.0)] * 8, MINI)[key]) == 8


# ----------------------------------------------------------------------------- ensure: the fingerprint logic
class StubCtx:
    def __init__(self):
        self.calls = []

    def lora_begin(self):
        self.calls.append(("begin",))

    def lora_merge(self, key, adapters):
        self.calls.append(("merge", key, [float(s) for _d, _u, s in adapters], [id(d) for d, _u, _s in adapters]))

    def lora_end(self):
        self.calls.append(("end",))

    def lora_clear(self):
        self.calls.append(("clear",))

    def lora_backup_bytes(self):
        return 0


def _stub():
    return SimpleNamespace(ctx=StubCtx(), cfg=MINI, device=torch.device("cpu"))


def test_ensure_merges_once_per_distinct_request(tmp_path):
    a = LR.spell(_one(r=2), "peft")
    b = LR.spell(_one("single_blocks.0.linear2.w2.weight", 3, alpha=6.0), "kohya")
    b.update(LR.spell(_one(r=1, alpha=2.0, seed=3), "kohya"))          # b touches audio_cross_q as well
    q = "triple_blocks.0.audio_cross_q.weight"
    m = _stub()
    assert lora.ensure(m, None) is False and lora.ensure(m, []) is False and m.ctx.calls == []      # nothing merged: a no-op
    assert lora.ensure(m, [(a, 0.5)]) is True
    assert [c[0] for c in m.ctx.calls] == ["begin", "merge", "end"] and m.ctx.calls[1][1:3] == (q, [0.5])
    n = len(m.ctx.calls)
    assert lora.ensure(m, [(a, 0.5)]) is False and len(m.ctx.calls) == n                                # same set: nothing
    assert lora.ensure(m, [(a, 0.25)]) is True and m.ctx.calls[n + 1][2] == [0.25]                      # changed strength
    m.ctx.calls.clear()
    assert lora.ensure(m, [(a, 0.5), (b, -1.0)]) is True
    merges = {c[1]: c[2] for c in m.ctx.calls if c[0] == "merge"}
    assert merges[q] == [0.5, LR.fl32(-1.0 * 2.0 / 1)] and merges["single_blocks.0.linear2.w2.weight"] == [LR.fl32(-1.0 * 6.0 / 3)]
    assert [c[0] for c in m.ctx.calls] == ["begin", "merge", "merge", "end"]        # ONE merge per key, all its adapters in it
    m.ctx.calls.clear()
    assert lora.ensure(m, [(b, -1.0), (a, 0.5)]) is True                           # changed order: merged again, b first
    assert {c[1]: c[2] for c in m.ctx.calls if c[0] == "merge"}[q] == [-2.0, 0.5]
    m.ctx.calls.clear()
    assert lora.ensure(m, [(b, -1.0), (a, 0.0)]) is True                           # strength 0 drops the adapter
    assert {c[1]: c[2] for c in m.ctx.calls if c[0] == "merge"}[q] == [-2.0]
    assert lora.ensure(m, [(b, -1.0)]) is False                                    # ... and is the same request as without it
    m.ctx.calls.clear()
    assert lora.ensure(m, None) is True and m.ctx.calls == [("clear",)] and not lora.merged(m)
    assert lora.ensure(m, [(a, 0.0)]) is False and m.ctx.calls == [("clear",)]
    # files: path + size + mtime
    path = tmp_path / "style.pt"
    torch.save(dict(a), path)
    assert lora.ensure(m, [(str(path), 1.0)]) is True and lora.ensure(m, [(str(path), 1.0)]) is False
    os.utime(path, ns=(1, 1))
    assert lora.ensure(m, [(str(path), 1.0)]) is True


def test_a_refusal_reaches_no_device_call_and_a_failed_merge_clears():
    m = _stub()
    bad = LR.spell(_one(), "peft")
    bad["x.dora_scale"] = torch.zeros(1)
    with pytest.raises(lora.LoraError, match="dora_scale"):
        lora.ensure(m, [(bad, 1.0)])
    assert m.ctx.calls == [] and not lora.merged(m)

    def boom(key, adapters):
        raise rt.FoleyRuntimeError("refused")
    m.ctx.lora_merge = boom
    with pytest.raises(rt.FoleyRuntimeError):
        lora.ensure(m, [(LR.spell(_one(), "peft"), 1.0)])
    assert m.ctx.calls == [("begin",), ("clear",)] and not lora.merged(m)


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    for name in ("foley_lora_begin", "foley_lora_merge", "foley_lora_end", "foley_lora_clear", "foley_lora_backup_bytes"):
        assert name in rt.EXPORTED_SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr)
    assert "foley_lora_pair" in hdr
    assert_abi_version()


# ----------------------------------------------------------------------------- the fp64 restatement
def test_merge64_by_hand():
    w = torch.tensor([[1.0, -2.0, 0.5], [0.0, 4.0, -1.0]])
    down, up = torch.tensor([[2.0, -1.0, 3.0]]), torch.tensor([[0.5], [-2.0]])
    ref, mag = LR.merge64({"k": w}, {"k": [(down, up, 0.25)]})
    assert ref["k"].dtype == torch.float64
    assert ref["k"].tolist() == [[1.0 + 0.25 * 1.0, -2.0 - 0.25 * 0.5, 0.5 + 0.25 * 1.5], [0.0 - 0.25 * 4.0, 4.0 + 0.25 * 2.0, -1.0 - 0.25 * 6.0]]
    assert mag["k"].tolist() == [[1.25, 2.125, 0.875], [1.0, 4.5, 2.5]]
    ref2, mag2 = LR.merge64({"k": w}, {"k": [(down, up, 0.25), (down, up, -0.25)]})          # two adapters: the sum, |.| in mag
    assert torch.equal(ref2["k"], w.double()) and mag2["k"].tolist() == [[1.5, 2.25, 1.25], [2.0, 5.0, 4.0]]
    w3 = torch.arange(12.0).view(2, 2, 3)                                                     # conv: c runs over the flattened (I, k)
    d3, u3 = torch.ones(1, 2, 3), torch.tensor([[[1.0]], [[2.0]]])
    assert LR.merge64({"k": w3}, {"k": [(d3, u3, 1.0)]})[0]["k"].tolist() == (w3 + torch.tensor([1.0, 2.0]).view(2, 1, 1)).tolist()


def test_fp8_ulp_helper():
    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    x = torch.tensor([1.0, 1.9, 2.0, 448.0, 2.0 ** -7, 2.0 ** -12, 0.0], dtype=torch.float64)
    assert LR.ulp8(x, e4).tolist() == [2.0 ** -3, 2.0 ** -3, 2.0 ** -2, 32.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9]
    assert LR.ulp8(x, e5).tolist() == [0.25, 0.25, 0.5, 64.0, 2.0 ** -9, 2.0 ** -14, 2.0 ** -16]
    for dt in (e4, e5):                              # the spacing torch's own cast shows between neighbouring values
        v = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dt).float()
        v = torch.unique(v[torch.isfinite(v) & (v >= 0)]).double()
        assert torch.equal(LR.ulp8(v[:-1], dt), v[1:] - v[:-1])


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2],
                         ids=lambda d: str(d).replace("torch.", ""))
def test_sequential_fp32_merge_stays_inside_the_bound(store):
    """The bound is derived, not fitted: a sequential fp32 merge on 96 x 96 with a delta of about 15 % of the weight stays
    inside it at rank 1, 16 and 256, two adapters included, for every store type."""
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(96, 96, generator=g)).to(store)
    for ranks in ((1,), (16,), (256,), (5, 16)):
        lst = []
        for r in ranks:
            lst.append(((torch.randn(r, 96, generator=g) * 0.4).bfloat16(), (torch.randn(96, r, generator=g) * 0.4 / r ** 0.5).bfloat16(),
                        LR.fl32(0.9)))
        ref, mag = LR.merge64({"k": w}, {"k": lst})
        got = LR.seq_merge32(w, lst, store).to(torch.float32).double()
        delta = (ref["k"] - w.float().double()).norm() / w.float().double().norm()
        assert 0.05 < float(delta) < 0.5
        b = LR.bound(ref["k"], got, mag["k"], sum(ranks), store)
        assert bool(((got - ref["k"]).abs() <= b).all()), (ranks, float(((got - ref["k"]).abs() / b).max()))
