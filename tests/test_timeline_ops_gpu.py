"""The timeline cross-attention at op level (csrc/attention_timeline.hip through foley_op_attention_timeline), element by element
under the derived bound of tests/timeline_ref.py, plus the exactness properties: a set a row does not use is not read, a row does
not depend on its tile-mates, caller tables are clamped, repeated runs give the same bits."""
import pytest
import torch

import opcheck as oc
import timeline_ref as TR
from foley_amd.host import runtime as rt

pytestmark = pytest.mark.gpu

DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
H, LV, LA, BQ, NSETS, PITCH = 2, 8, 75, 3, 4, 96
SQ = LV + LA                      # 83 queries: tiles [0, 32), [32, 64), [64, 83) - neither token count a multiple of 32


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables():
    """Row 0: one set for every token (an unconditional half).  Row 1: tile 0 holds one set; hard cuts at queries 40 and 41 put
    three sets into tile 1; a ramp 56..71 straddles the tile boundary at query 64 and meets at 0.5 / 0.5.  Row 2: alpha 0.5 on
    every token, with a hard cut of set_a at query 20."""
    sa, sb, al = torch.zeros(BQ, SQ, dtype=torch.int32), torch.zeros(BQ, SQ, dtype=torch.int32), torch.zeros(BQ, SQ)
    sa[1, :40], sa[1, 40], sa[1, 41:64], sa[1, 64:] = 1, 2, 3, 0
    sb[1] = sa[1]
    sb[1, 56:64], sb[1, 64:72] = 0, 3
    ramp = torch.arange(1, 9, dtype=torch.float64) / 16.0                   # 1/16 .. 8/16 = 0.5 at the boundary
    al[1, 56:64], al[1, 64:72] = ramp.float(), ramp.flip(0).float()
    sa[2, :20], sa[2, 20:], sb[2], al[2] = 2, 3, 1, 0.5
    return sa, sb, al


def _operands(dt, Skv, seed=0):
    q = _rand((BQ, H, SQ, 128), 70 + seed).to(dt)
    k = _rand((NSETS, H, Skv, 128), 71 + seed).to(dt)
    v = _rand((NSETS, H, Skv, 128), 72 + seed).to(dt)
    return q, k, v


def _device_v(v, dt, fill=1e4):
    """What the kernel reads: v as it is (fp32), or transposed at pitch 96 with LARGE finite pad values (16-bit) - a pad column
    leaking into P V fails an element."""
    if dt == torch.float32:
        return v
    vd = torch.full((v.shape[0], v.shape[1], 128, PITCH), fill, dtype=dt)
    vd[..., :v.shape[2]] = v.transpose(2, 3)
    return vd


def _run(dev, q, k, vd, sa, sb, al, dt):
    ga = oc.guarded((BQ, LV, H * 128), dt, dev, rows=(1, 1))
    gb = oc.guarded((BQ, LA, H * 128), dt, dev, rows=(1, 1))
    rt.op_attention_timeline(q.to(dev), k.to(dev), vd.to(dev), sa.to(dev).contiguous(), sb.to(dev).contiguous(), al.to(dev).contiguous(),
                             ga.view, gb.view, LV)
    torch.cuda.synchronize()
    ga.check("around outA")
    gb.check("around outB")
    return torch.cat([ga.view.clone(), gb.view.clone()], dim=1).cpu()       # [Bq, Sq, H*128]


@pytest.mark.parametrize("Skv", [77, 96, 5])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_timeline_attention_elementwise(dev, kind, Skv):
    dt = DTS[kind]
    half = dt != torch.float32
    q, k, v = _operands(dt, Skv)
    sa, sb, al = _tables()
    ref, bound = TR.timeline_attention_ref_and_bound(q, k, v, sa, sb, al, dt, p_dtype=dt if half else None)
    got = _run(dev, q, k, _device_v(v, dt), sa, sb, al, dt)
    r = oc.assert_elementwise(got, ref, bound, f"timeline attention Skv={Skv} {kind}")
    print(f"timeline attention Skv={Skv} {kind}: max err / bound = {r:.3g}")
    # and the table is applied: row 1's queries 40 and 41 read different sets than query 39
    plain, _ = TR.timeline_attention_ref_and_bound(q, k, v, torch.ones_like(sa), torch.ones_like(sa), torch.zeros_like(al), dt)
    assert float((ref[1, 41] - plain[1, 41]).abs().max()) > 20 * float(bound.total(ref, got)[1, 41].max())


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_unused_set_b_is_not_read(dev, kind):
    """Set 3 is NaN in K and V^T (pad included); rows with alpha == 0 name it as set_b: finite, and the bits of set_b = a clean set."""
    dt = DTS[kind]
    q, k, v = _operands(dt, 77, seed=10)
    k[3], v[3] = float("nan"), float("nan")
    vd = _device_v(v, dt)
    vd[3] = float("nan")
    sa = (torch.arange(BQ * SQ, dtype=torch.int32).view(BQ, SQ) // 13) % 3   # sets 0..2, changing inside tiles
    al = torch.zeros(BQ, SQ)
    got = _run(dev, q, k, vd, sa, torch.full_like(sa, 3), al, dt)
    want = _run(dev, q, k, vd, sa, torch.zeros_like(sa), al, dt)
    assert bool(torch.isfinite(got.float()).all())
    oc.assert_bits_equal(got, want, f"set_b unread {kind}")


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_a_row_does_not_depend_on_its_tile_mates(dev, kind):
    """Sets 0 and 1 hold the same values; a hard cut between them inside a tile gives the bits of the single-set table."""
    dt = DTS[kind]
    q, k, v = _operands(dt, 77, seed=20)
    k[1], v[1] = k[0], v[0]
    vd = _device_v(v, dt)
    sa = torch.zeros(BQ, SQ, dtype=torch.int32)
    sa[:, 45:] = 1
    al = torch.zeros(BQ, SQ)
    got = _run(dev, q, k, vd, sa, sa.clone(), al, dt)
    want = _run(dev, q, k, vd, torch.zeros_like(sa), torch.zeros_like(sa), al, dt)
    oc.assert_bits_equal(got, want, f"hard cut between equal sets {kind}")
    again = _run(dev, q, k, vd, sa, sa.clone(), al, dt)                      # and repeated runs give the same bits
    oc.assert_bits_equal(again, got, f"repetition {kind}")


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_table_indices_are_clamped(dev, kind):
    """Indices outside [0, n_sets) in the device table are clamped before they address anything: the bits of the clamped table."""
    dt = DTS[kind]
    q, k, v = _operands(dt, 77, seed=30)
    vd = _device_v(v, dt)
    sa, sb, al = _tables()
    wild_a, wild_b = sa.clone(), sb.clone()
    wild_a[0, 3], wild_a[0, 50], wild_a[1, 70], wild_a[2, 82] = -7, 2 ** 30, NSETS, -2 ** 31
    wild_b[1, 60], wild_b[2, 5] = 1000, -1
    got = _run(dev, q, k, vd, wild_a, wild_b, al, dt)
    want = _run(dev, q, k, vd, wild_a.clamp(0, NSETS - 1), wild_b.clamp(0, NSETS - 1), al, dt)
    oc.assert_bits_equal(got, want, f"clamped table {kind}")
    rep = _run(dev, q, k, vd, sa, sb, al, dt)
    oc.assert_bits_equal(rep, _run(dev, q, k, vd, sa, sb, al, dt), f"repetition {kind}")


def test_launcher_refusals(dev):
    q, k, v = (t.to(dev) for t in _operands(torch.bfloat16, 97))
    sa, sb, al = (t.to(dev) for t in _tables())
    vd = torch.zeros(NSETS, H, 128, 128, dtype=torch.bfloat16, device=dev)
    oa, ob = torch.empty(BQ, LV, H * 128, dtype=torch.bfloat16, device=dev), torch.empty(BQ, LA, H * 128, dtype=torch.bfloat16, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="at most 96 keys"):
        rt.op_attention_timeline(q, k, vd, sa, sb, al, oa, ob, LV)
    with pytest.raises(rt.FoleyRuntimeError, match="pitch"):
        rt.op_attention_timeline(q, k[:, :, :77].contiguous(), vd[..., :88].contiguous(), sa, sb, al, oa, ob, LV)
