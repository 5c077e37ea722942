"""The HIP kernels under per-element bounds and guard bands (tests/opcheck.py).

Every case launches into a NaN-filled interior inside a guard band (two rows before, three after, eight pad columns where the
descriptor has an output pitch; the interior pointer and the pitch stay 16-byte aligned so that the vector epilogue is the one
taken - the misaligned twin cases excepted), checks EVERY element against a bound derived from the arithmetic, checks the guard
bit for bit, and records the largest err / bound.  Outputs without a pitch (head-split destinations, attention, slabs, LayerNorm
rows) get guard rows / guard slabs only.

Coverage is asserted: test_every_tile_has_a_case asks the library which tile ids exist, the automatic-tile cases assert the
(tile, K split, panel groups) of tests/test_gemm_plan_cpu.py through foley_debug_gemm_plan on the descriptor they launch.
tests/test_gemm_edges_gpu.py takes run_gemm_case to every tile's M, N, K and segment edges and to the mapped operands (virtual
rows, strided conv); tests/test_attention_edges_gpu.py takes every attention form (_attn_form_of) to its query, key and split edges.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import opcheck as oc
from conftest import record_parity
from foley_amd.host import packers, runtime as rt, tables
from test_pairs_gpu import _rms64, _rope64, gemm_last, ln_mod_pair

pytestmark = pytest.mark.gpu

DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPI_CODE = {"store": rt.EPI_STORE_F32, "addend": rt.EPI_STORE_F32, "store_t": rt.EPI_STORE_T, "silu": rt.EPI_SILU_T,
            "gelu": rt.EPI_GELU_T, "gelu_erf": rt.EPI_GELU_T, "silugate": rt.EPI_SILUGATE_T, "gate": rt.EPI_GATE_RES,
            "gate_split": rt.EPI_GATE_RES, "gate_split_f32slabs": rt.EPI_GATE_RES, "qkv": rt.EPI_QKV_SPLIT, "dac": rt.EPI_DAC}


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _lib():
    lib = rt.load_library()
    lib.foley_debug_gemm_plan.argtypes = [C.POINTER(rt.GemmDescC), C.POINTER(rt.GemmDescC), C.c_int, C.POINTER(C.c_int32)]
    lib.foley_debug_gemm_plan.restype = C.c_int
    return lib


def _plan(d):
    """(tile, K split, panel groups) the launcher plans for descriptor d, or the error text."""
    out = (C.c_int32 * 4)()
    lib = _lib()
    if lib.foley_debug_gemm_plan(C.byref(d), None, 0, out) != 0:
        return lib.foley_last_error().decode()
    return tuple(out)[:3]


def _launch(d):
    lib = _lib()
    rt._check(lib, lib.foley_op_gemm(C.byref(d), rt._stream()), "foley_op_gemm")
    return int(d._used.value)


# ----------------------------------------------------------------------------- operands and fp64 references (once per case)
def _both16(t):
    """Round to bf16 and flush what fp16 cannot hold exactly (|x| < 2^-17): the result is exact in bf16 AND fp16, so the fp64
    reference of a 4000-row case is computed once and shared by both 16-bit types."""
    t = t.to(torch.bfloat16).float()
    t = torch.where(t.abs() < 2.0 ** -17, torch.zeros_like(t), t)
    assert torch.equal(t.to(torch.float16).float(), t)
    return t


@functools.lru_cache(maxsize=3)
def _operands(M, N, K, conv, kind, gated, seed, mapped=None):
    """kind: 'f32' | 'h' (values exact in bf16 and fp16) | 'fp8' (weights additionally exact in e4m3fn).  conv = (B, L, C) or None.
    mapped = ('vrows', segV, segS): M = segs segV product rows over segs segS source rows, row r reads source row
    (r // segV) segS + r % segV;  mapped = ('sconv', B, Tin, Cin, stride): the strided conv k = 2 stride, pad ceil(stride / 2), of B
    clips of Tin rows (K = 2 stride Cin, M = B (Tin // stride)), reference F.conv1d in fp64, mag the same conv on absolute values.
    Returns a dict: src (rows as the kernel reads them), W, b, ref0 / mag0 (without the bias)."""
    if conv:
        B, L, Cc = conv
        src = _rand((B * L, Cc), seed)
    elif mapped and mapped[0] == "vrows":
        src = _rand((M // mapped[1] * mapped[2], K), seed)
    elif mapped:
        src = _rand((mapped[1] * mapped[2], mapped[3]), seed)
    else:
        src = _rand((M, K), seed)
    W = _rand((N, K), seed + 1, 1 / math.sqrt(K))
    if gated:      # SwiGLU pair: rows of w1 and w3 interleaved in groups of 32
        W = packers.interleave_gate(W[: N // 2].contiguous(), W[N // 2:].contiguous())
    b = None if gated else _rand((N,), seed + 2, 0.1)
    if kind != "f32":
        src, W = _both16(src), _both16(W)
    if kind == "fp8":
        W = W.to(torch.float8_e4m3fn).float()
    if mapped and mapped[0] == "sconv":      # W [N, 2 stride Cin] is packers.conv_to_gemm of the conv weight w [N, Cin, 2 stride]
        _, B, Tin, Cin, st = mapped
        w = W.view(N, 2 * st, Cin).transpose(1, 2).double()
        assert torch.equal(packers.conv_to_gemm(w.float()).double(), W.double())
        x = src.view(B, Tin, Cin).transpose(1, 2).double()
        cv = lambda a, ww: torch.nn.functional.conv1d(a, ww, None, stride=st, padding=math.ceil(st / 2)).transpose(1, 2).reshape(M, N)
        ref0, mag0 = cv(x, w), cv(x.abs(), w.abs())
        return dict(src=src, W=W, b=b, ref0=ref0, mag0=mag0)
    if mapped:
        segV, segS = mapped[1:]
        cols = src[(torch.arange(M // segV)[:, None] * segS + torch.arange(segV)[None]).reshape(-1)]
    else:
        cols = oc.conv3_cols(src.view(*conv)) if conv else src
    ref0, mag0 = oc.gemm_ref64(cols, W, None)
    return dict(src=src, W=W, b=b, ref0=ref0, mag0=mag0)


def _ref(ops):
    if ops["b"] is None:
        return ops["ref0"], ops["mag0"]
    b = ops["b"].double()
    return ops["ref0"] + b, ops["mag0"] + b.abs()


# ----------------------------------------------------------------------------- one GEMM under the checks
def run_gemm_case(dev, name, epi, mnk, dt, tile=0, conv=None, fp8=False, misalign=False, want_plan=None, want_tile=None, ksplit=None,
                  qkv=None, slabs16=True, seed=100, vrows=None, sconv=None, n_slabs=8):
    """Launch one problem and check it; any M >= 1 (an odd M gives the row-broadcast operands - addend, gate - ONE half of M rows).
    qkv = (B, L, H, Lv, nK): the fused head split of B clips of L tokens at token offset Lv.
    vrows = (segV, segS): virtual rows - product row r reads source row (r // segV) segS + r % segV; source rows [segV, segS) of
    every segment, which the mapping never reads, are NaN on the device.
    sconv = (B, Tin, Cin, stride): the DAC encoder's strided conv (K = 2 stride Cin, M = B (Tin // stride)); the B clips sit
    between two guard segments of Tin NaN rows: a tap that leaves its clip must read a zero, never the neighbouring rows."""
    M, N, K = mnk
    kind = "f32" if dt == torch.float32 else ("fp8" if fp8 else "h")
    rec_epi = epi
    if epi == "gate_split_f32slabs":      # deferred split-K of 16-bit operands into fp32 slabs (slab_bound's plain e_y branch)
        epi, slabs16 = "gate_split", False
    gated = epi == "silugate"
    mapped = ("vrows",) + tuple(vrows) if vrows else (("sconv",) + tuple(sconv) if sconv else None)
    assert sum(m is not None for m in (conv, vrows, sconv)) <= 1
    ops = _operands(M, N, K, conv, kind, gated, seed, mapped) if mapped else _operands(M, N, K, conv, kind, gated, seed)
    ref, mag = _ref(ops)
    e_y = (K + 4) * oc.U32 * mag
    Ad = ops["src"].to(dev, dt)
    Wd = ops["W"].to(torch.float8_e4m3fn).to(dev) if fp8 else ops["W"].to(dev, dt)
    assert torch.equal(Ad.double().cpu(), ops["src"].double()) and torch.equal(Wd.float().double().cpu(), ops["W"].double())
    bd = ops["b"].to(dev) if ops["b"] is not None else None
    kw = dict(epilogue=EPI_CODE[epi], tile=tile, gelu_erf=(epi == "gelu_erf"))
    if conv:
        kw["conv"] = (conv[1], conv[2], 3, 1)
    if vrows:
        assert M % vrows[0] == 0 and vrows[0] <= vrows[1]
        Ad.view(M // vrows[0], vrows[1], K)[:, vrows[0]:] = float("nan")
        kw.update(vrows=tuple(vrows), M=M)
    if sconv:
        B, Tin, Cin, st = sconv
        assert M == B * (Tin // st) and K == 2 * st * Cin
        hold = torch.full(((B + 2) * Tin, Cin), float("nan"), dtype=dt, device=dev)
        hold[Tin:(B + 1) * Tin] = Ad
        Ad = hold[Tin:(B + 1) * Tin]
        assert Ad.data_ptr() % 16 == 0
        kw["sconv"] = (Tin, Cin, st)
    guards, checks = [], []
    h16 = dt != torch.float32
    if epi == "qkv":
        return _run_head_split(dev, name, ops, ref, e_y, dt, qkv, kw, Ad, Wd, bd, want_plan, want_tile)
    odt = torch.float32 if epi in ("store", "addend", "gate", "gate_split") else dt
    No = N // 2 if gated else N
    es = 4 if odt == torch.float32 else 2
    g = oc.guarded((M, No), odt, dev, rows=(2, 3), pad_cols=8, misalign=(8 // es if misalign else 0))
    assert g.view.data_ptr() % 16 == (8 if misalign else 0) and (g.pitch * es) % 16 == 0
    guards.append(g)
    kw["ldc"] = g.pitch
    halves, L2 = (2, M // 2) if M % 2 == 0 else (1, M)      # an odd M: one half of M rows (rows_per_cfg = M)
    if epi == "addend":
        add = _rand((halves, L2, N), seed + 5)
        kw["rb"] = rt.rowbcast(add.to(dev), 1, rows_per_cfg=L2, L=L2)
    if epi in ("gate", "gate_split"):
        x0, gate = _rand((M, N), seed + 6), _rand((halves, L2, N), seed + 7, 0.5)
        g.view.copy_(x0.to(dev))
        kw["rb"] = rt.rowbcast(gate.to(dev), 1, rows_per_cfg=L2, L=L2)
        kw["ksplit"] = 1 if epi == "gate" else (2 if ksplit is None else ksplit)
        if epi == "gate_split" and h16:
            gs = oc.guarded((n_slabs, M, N), dt if slabs16 else torch.float32, dev, rows=(1, 1))
            guards.append(gs)
            kw["partials"] = gs.view
        elif ksplit == 0:
            kw["ksplit"] = 0
    d = rt.gemm_desc(Ad, Wd, bd, **kw)
    d.out0 = g.view.data_ptr()
    plan = _plan(d)
    assert not isinstance(plan, str), (name, plan)
    if want_plan is not None:
        assert plan == want_plan, (name, plan, want_plan)
    if want_tile is not None:
        assert plan[0] == want_tile, (name, plan, want_tile)
    ks = _launch(d)
    assert gemm_last()[0] == plan[0] and ks == plan[1], (name, gemm_last(), plan)
    out = g.view
    what = f"{name} [{epi}, tile {plan[0]}, ks {ks}, groups {plan[2]}]"
    rec = {}
    if epi == "store":
        ratio = oc.assert_elementwise(out, ref, oc.Bound(e_y), what)
    elif epi == "addend":
        a = add.double().reshape(M, N)
        ratio = oc.assert_elementwise(out, ref + a, oc.Bound(e_y + oc.U32 * (ref + a).abs()), what)
    elif epi == "store_t":
        ratio = oc.assert_elementwise(out, ref, oc.Bound(e_y, odt), what)
    elif epi in ("silu", "gelu", "gelu_erf"):
        a_act = oc.A_ACT_ERF16 if (epi == "gelu_erf" and h16) else oc.measure_a_act(epi, ref, dev)
        rec["a_act"] = a_act
        ratio = oc.assert_elementwise(out, oc.act64(epi, ref), oc.act_bound(epi, e_y, a_act, odt), what)
    elif epi == "silugate":
        w = lambda t: t.view(M, N // 64, 2, 32)
        a, b2, ea, eb = w(ref)[:, :, 0].reshape(M, No), w(ref)[:, :, 1].reshape(M, No), w(e_y)[:, :, 0].reshape(M, No), w(e_y)[:, :, 1].reshape(M, No)
        a_act = oc.measure_a_act("silu", a, dev)
        rec["a_act"] = a_act
        ratio = oc.assert_elementwise(out, oc.act64("silu", a) * b2, oc.silugate_bound(a, b2, ea, eb, a_act, odt), what)
    else:
        gf = gate.double().reshape(M, N)
        want_x = x0.double() + gf * ref
        if epi == "gate_split" and h16 and ks > 1:
            assert torch.equal(out.cpu(), x0), f"{what}: residual touched by a deferred split-K launch"
            sl = guards[1].view
            assert bool(torch.isnan(sl[ks:]).all()), f"{what}: slabs beyond the K split written"
            e0 = (K + 4) * oc.U32 * ops["mag0"]
            ratio = oc.assert_elementwise(sl[:ks].double().sum(0), ops["ref0"], oc.slab_bound(e0, ops["mag0"], ks, sl.dtype), what)
        else:
            if len(guards) > 1:
                assert bool(torch.isnan(guards[1].view).all()), f"{what}: slabs written without a K split"
            ratio = oc.assert_elementwise(out, want_x, oc.gated_residual_bound(e_y, gf, x0, ref), what)
    for gg in guards:
        gg.check(what)
    record_parity(f"elementwise.gemm.{name}.{rec_epi}.{str(dt)[6:]}{'.fp8' if fp8 else ''}{'.misaligned' if misalign else ''}",
                  err_over_bound=ratio, tile=plan[0], ksplit=ks, n_groups=plan[2], **rec)
    return ratio


def _run_head_split(dev, name, ops, ref, e_y, dt, qkv, kw, Ad, Wd, bd, want_plan, want_tile):
    B, L, H, Lv, nK = qkv
    M = B * L
    S = L + Lv
    h16 = dt != torch.float32
    pitch = (S + 31) // 32 * 32
    gains = [1 + 0.1 * _rand((128,), 900 + j) for j in range(2)]
    pos = (2 * torch.arange(L)).to(torch.int32)
    cos, sin = tables.rope_table(2 * L + 1)
    gq = oc.guarded((B, H, S, 128), dt, dev, rows=(1, 1))
    dsts, guards = [gq.view], [gq]
    if nK == 3:
        gk = oc.guarded((B, H, S, 128), dt, dev, rows=(1, 1))
        gv = oc.guarded((B, H, 128, pitch) if h16 else (B, H, S, 128), dt, dev, rows=(1, 1), fill=1e4 if h16 else float("nan"))
        if h16:
            gv.view[..., Lv:S] = float("nan")      # token columns NaN; the columns before Lv and the pad keep 1e4
        dsts += [gk.view, gv.view]
        guards += [gk, gv]
    gl = [gains[0].to(dev), gains[1].to(dev), None][:nK]
    pl = [pos.to(dev), pos.to(dev), None][:nK]
    desc = rt.qkv_split_desc(L, H, gl, pl, dsts, S, Lv, 1e-6, cos.to(dev), sin.to(dev), vt_pitch=pitch if (h16 and nK == 3) else 0)
    d = rt.gemm_desc(Ad, Wd, bd, qkv=desc, **kw)
    plan = _plan(d)
    assert not isinstance(plan, str), (name, plan)
    if want_plan is not None:
        assert plan == want_plan, (name, plan, want_plan)
    if want_tile is not None:
        assert plan[0] == want_tile, (name, plan, want_tile)
    _launch(d)
    assert gemm_last()[0] == plan[0]
    what = f"{name} [qkv, tile {plan[0]}, groups {plan[2]}]"
    y = ref.view(B, L, nK, H, 128)
    ey = e_y.view(B, L, nK, H, 128)
    c, s = cos[pos.long()].double(), sin[pos.long()].double()
    worst = 0.0
    for j in range(min(nK, 2)):
        yy = y[:, :, j].reshape(M, H, 128)
        want = _rope64(_rms64(yy, gains[j].double(), 1e-6), c.repeat(B, 1), s.repeat(B, 1)).view(B, L, H, 128).transpose(1, 2)
        bound = oc.head_split_bound(ey[:, :, j], y[:, :, j], dt, gains[j])
        bound.e = bound.e.transpose(1, 2)
        got = dsts[j]
        worst = max(worst, oc.assert_elementwise(got[:, :, Lv:], want, bound, f"{what} {'qk'[j]}"))
        assert bool(torch.isnan(got[:, :, :Lv]).all()), f"{what}: rows before the token offset written"
    if nK == 3:
        got, yv = dsts[2], y[:, :, 2].transpose(1, 2)           # [B, H, L, 128]
        bv = oc.Bound(ey[:, :, 2].transpose(1, 2), dt)
        if h16:
            bv.e = bv.e.transpose(2, 3)
            worst = max(worst, oc.assert_elementwise(got[..., Lv:S], yv.transpose(2, 3), bv, f"{what} V^T"))
            pad = torch.cat((got[..., :Lv], got[..., S:]), -1)
            assert bool((pad == 1e4).all()), f"{what}: V^T columns outside the tokens overwritten"
        else:
            worst = max(worst, oc.assert_elementwise(got[:, :, Lv:], yv, bv, f"{what} V"))
    for gg in guards:
        gg.check(what)
    record_parity(f"elementwise.gemm.{name}.qkv.{str(dt)[6:]}", err_over_bound=worst, tile=plan[0], n_groups=plan[2])
    return worst


# ----------------------------------------------------------------------------- explicit tiles
PLAIN, PLAIN_G, WIDE_SHAPE = (1000, 136, 320), (1000, 320, 320), (700, 640, 4608)     # ragged M, N (136 = 128 + 8, 320 = 2.5 x 128, 640 = 2.5 x 256); K = 5 / 72 slices
CONV = (4, 129, 192)                                                                  # conv k = 3: M = 516, K = 576 (three chunks of 64 per tap)
CONV_N = 320
BASIC = ["store", "addend", "store_t", "silu", "gelu", "gelu_erf", "gate", "gate_split"]      # gelu_erf: a flag of EPI_GELU_T wherever GELU is served
ALL3, H16 = ["f32", "bf16", "f16"], ["bf16", "f16"]
# tile id -> (dtypes, epilogues its family serves, conv?)  (gemm_impl.h launch_tile / gemm_ws_impl.h / gemm_wide_impl.h / gemm_conv3.hip)
TILE_CASES = {
    1: (ALL3, BASIC + ["silugate", "qkv"], False), 2: (ALL3, BASIC + ["silugate", "qkv"], False),
    3: (ALL3, BASIC, False), 4: (ALL3, BASIC + ["silugate"], False),
    5: (ALL3, BASIC + ["silugate", "qkv"], False), 6: (ALL3, BASIC, False),
    7: (H16, BASIC + ["silugate", "qkv"], False), 8: (ALL3, BASIC + ["silugate", "qkv"], False),
    9: (H16, BASIC + ["silugate", "qkv"], False),
    11: (ALL3, ["store", "gate", "gate_split", "silugate"], True), 13: (ALL3, ["store", "gate", "gate_split"], True),
    15: (H16, BASIC + ["silugate", "qkv", "gate_split_f32slabs"], False), 19: (H16, BASIC + ["silugate", "qkv"], False),
    21: (H16, ["store", "gate", "gate_split", "gate_split_f32slabs", "silugate"], True), 22: (H16, ["store", "gate", "gate_split", "silugate"], True),
    23: (H16, ["store", "gate", "gate_split", "silugate"], True), 24: (H16, ["store", "gate", "gate_split"], True),
    25: (H16, BASIC + ["silugate", "qkv", "gate_split_f32slabs"], False), 26: (H16, ["qkv"], False), 27: (H16, ["qkv"], False),
    28: (H16, ["qkv"], False), 29: (H16, BASIC + ["silugate", "qkv"], False),
    31: (H16, ["store", "gate", "gate_split", "silugate"], True),
    32: (H16, ["store", "addend", "gelu", "gelu_erf", "gate", "gate_split", "gate_split_f32slabs", "silugate", "qkv"], False),
}
_FP8_PLAIN, _FP8_CONV = ["store", "gelu", "gate", "gate_split", "silugate"], ["store", "gate_split", "silugate"]
FP8_TILES = {15: _FP8_PLAIN, 19: _FP8_PLAIN, 21: _FP8_CONV, 23: _FP8_CONV, 31: _FP8_CONV, 32: _FP8_PLAIN}
SCALAR_TWIN = {25: 15, 29: 19}
# a misaligned output pointer (8 bytes off a 16-byte boundary) rules out the vector epilogue: tiles 25 / 29 hand the problem to their
# scalar twins, the register-staged and direct-to-LDS tiles run their own in-kernel scalar epilogue (gemm_common.h gemm_epilogue)
MISALIGNED = {1: ALL3[:2], 3: ALL3[:2], 5: ALL3[:2], 25: ["bf16"], 29: ["bf16"]}


def _tile_params():
    out = []
    for tile, (dts, epis, conv) in TILE_CASES.items():
        for epi in epis:
            for dt in dts:
                out.append(pytest.param(tile, epi, dt, False, False, id=f"t{tile}-{epi}-{dt}"))
        for epi in FP8_TILES.get(tile, []):
            out.append(pytest.param(tile, epi, "bf16", True, False, id=f"t{tile}-{epi}-bf16-fp8"))
        for dt in MISALIGNED.get(tile, []):
            for epi in ("store", "gelu", "gate"):
                out.append(pytest.param(tile, epi, dt, False, True, id=f"t{tile}-{epi}-{dt}-misaligned"))
    return out


def test_every_tile_has_a_case():
    """The library's tile table (gemm_plan.h kTiles) against TILE_CASES: an id exists unless the planner calls it unknown."""
    from test_gemm_plan_cpu import plan
    exist = {t for t in range(1, 48) if "unknown tile" not in str(plan(dict(epi="gate", mnk=(500, 1536, 1536), tile=t)))}
    assert exist == set(TILE_CASES), (exist - set(TILE_CASES), set(TILE_CASES) - exist)
    assert exist == set(range(1, 10)) | {11, 13, 15, 19, 31, 32} | set(range(21, 30))
    fp8 = {t for t in exist if not isinstance(plan(dict(epi="store", mnk=(516, 320, 576), conv=129, tile=t, wfmt=1)), str) or
           not isinstance(plan(dict(epi="store", mnk=(1000, 136, 320), tile=t, wfmt=1)), str)}
    assert fp8 == set(FP8_TILES), fp8
    # the DAC residual epilogue is served by every fp32 register-staged / direct-to-LDS tile (gemm_impl.h launch_tile): all of them, all mappings
    assert set(DAC_TILES) - {0} == {t for t, (dts, epis, conv) in TILE_CASES.items() if "f32" in dts and not conv}
    assert {c[0] for c in DAC_CASES.values()} == {"conv7", "conv1_res", "convT"}


@pytest.mark.parametrize("tile,epi,dt,fp8,misalign", _tile_params())
def test_gemm_explicit_tile(dev, tile, epi, dt, fp8, misalign):
    dtype = DTS[dt]
    conv = TILE_CASES[tile][2]
    want = SCALAR_TWIN.get(tile, tile) if misalign else tile
    if epi == "qkv":
        q = (5, 250, 3, 40, 3) if tile == 32 else (3, 70, 1, 3, 3)         # N = 1152 = 4.5 x 256 / N = 384; M = 1250 / 210
        mnk = (q[0] * q[1], 3 * q[2] * 128, 256)
        run_gemm_case(dev, f"t{tile}", epi, mnk, dtype, tile=tile, qkv=q, want_tile=want)
        return
    if conv:
        mnk = (CONV[0] * CONV[1], CONV_N, 3 * CONV[2])
        run_gemm_case(dev, f"t{tile}", epi, mnk, dtype, tile=tile, conv=CONV, fp8=fp8, want_tile=want)
        return
    shapes = [PLAIN_G if epi == "silugate" else PLAIN] + ([WIDE_SHAPE] if tile == 32 and epi != "addend" else [])
    for mnk in shapes:
        run_gemm_case(dev, f"t{tile}.{mnk[0]}x{mnk[1]}x{mnk[2]}", epi, mnk, dtype, tile=tile, fp8=fp8, misalign=misalign, want_tile=want)


# ----------------------------------------------------------------------------- DAC residual epilogue (fp32 only)
# the mappings of test_dac_conv7_snake / test_dac_conv_transpose: dilated conv k = 7 (plain-mapped), the residual 1x1 conv whose
# residual is read and written in place, the transposed conv (segment-mapped output, guard rows only: no pitch of its own).
# name -> (mapping, B, T, C (in), Cout, dilation or stride)
DAC_CASES = {
    "conv7_d1": ("conv7", 2, 100, 64, 64, 1), "conv7_d3": ("conv7", 1, 37, 128, 128, 3), "conv7_d9": ("conv7", 2, 100, 64, 64, 9),
    "conv1_res_64": ("conv1_res", 2, 100, 64, 64, 1), "conv1_res_128": ("conv1_res", 1, 37, 128, 128, 1),
    "convT_s2": ("convT", 2, 23, 128, 64, 2), "convT_s3": ("convT", 2, 23, 128, 64, 3), "convT_s4": ("convT", 2, 23, 128, 64, 4),
    "convT_s5": ("convT", 2, 23, 128, 64, 5), "convT_s8": ("convT", 2, 23, 128, 64, 8),
    # tiny T: T <= 3 dil - every outer tap of the k = 7 conv leaves the clip on BOTH sides (T = 5 at dilation 9, T = 2 at dilation 3: the
    # centre tap alone is ever in range) - and the transposed conv of ONE input row (M = clips (Tin + 1) = 4 virtual rows)
    "conv7_d9_T5": ("conv7", 2, 5, 64, 64, 9), "conv7_d3_T2": ("conv7", 2, 2, 64, 64, 3),
    "convT_s2_T1": ("convT", 2, 1, 128, 64, 2), "convT_s5_T1": ("convT", 2, 1, 128, 64, 5),
}
DAC_TILES = [0, 1, 2, 3, 4, 5, 6, 8]


@pytest.mark.parametrize("tile", DAC_TILES)
@pytest.mark.parametrize("name", list(DAC_CASES))
def test_gemm_dac_epilogue(dev, name, tile):
    """out0 = v = conv(x) + bias (+ res), out1 = snake(v), both guarded and checked element by element (opcheck.dac_bounds)."""
    import torch.nn.functional as F
    kind, B, T, C, Co, p = DAC_CASES[name]
    seed = 700 + p
    x, b, alpha = _rand((B, C, T), seed), _rand((Co,), seed + 2, 0.1), 1 + 0.2 * _rand((Co,), seed + 3)
    xs = x.transpose(1, 2).contiguous().to(dev)                                   # [B, T, C] time-major
    res = None
    if kind == "conv7":
        w = _rand((Co, C, 7), seed + 1, 1 / math.sqrt(7 * C))
        conv = lambda a, ww: F.conv1d(a, ww, None, dilation=p, padding=3 * p)
        Wd, rows, kw, K = packers.conv_to_gemm(w).to(dev), B * T, dict(conv=(T, C, 7, p)), 7 * C
    elif kind == "conv1_res":
        w = _rand((Co, C, 1), seed + 1, 1 / math.sqrt(C))
        conv = lambda a, ww: F.conv1d(a, ww, None)
        Wd, rows, kw, K = w.squeeze(-1).contiguous().to(dev), B * T, {}, C
        res = _rand((B * T, Co), seed + 4)
    else:
        w = _rand((C, Co, 2 * p), seed + 1, 1 / math.sqrt(2 * C))
        conv = lambda a, ww: F.conv_transpose1d(a, ww, None, stride=p, padding=math.ceil(p / 2), output_padding=p % 2)
        Wd, rows, kw, K = packers.convT_to_gemm(w, p).to(dev), B * T * p, dict(convT=(T, C, p, Co)), 2 * C
    y = (conv(x.double(), w.double()) + b.double().view(1, Co, 1)).transpose(1, 2).reshape(rows, Co)
    mag = (conv(x.double().abs(), w.double().abs()) + b.double().abs().view(1, Co, 1)).transpose(1, 2).reshape(rows, Co)
    e_y = (K + 4) * oc.U32 * mag
    v = y + res.double() if res is not None else y
    pad = 0 if kind == "convT" else 8
    g0 = oc.guarded((rows, Co), torch.float32, dev, rows=(2, 3), pad_cols=pad)
    g1 = oc.guarded((rows, Co), torch.float32, dev, rows=(2, 3), pad_cols=pad)
    if pad:
        kw["ldc"] = g0.pitch
    if res is not None:
        g0.view.copy_(res.to(dev))
    bd = (b.repeat(p) if kind == "convT" else b).to(dev)
    A = xs.view(B * T, C) if kind == "conv1_res" else xs
    d = rt.gemm_desc(A, Wd, bd, epilogue=rt.EPI_DAC, alpha=alpha.to(dev), alphaC=Co, tile=tile, **kw)
    d.out0, d.out1 = g0.view.data_ptr(), g1.view.data_ptr()
    if res is not None:
        d.res = g0.view.data_ptr()
    plan = _plan(d)
    assert not isinstance(plan, str) and (tile == 0 or plan[0] == tile), (name, plan)
    _launch(d)
    assert gemm_last()[0] == plan[0]
    what = f"dac {name} [tile {plan[0]}]"
    a_act = oc.measure_a_act_snake(v, alpha, dev)
    b0, b1 = oc.dac_bounds(e_y, v, res, a_act)
    r0 = oc.assert_elementwise(g0.view, v, b0, what + " out0")
    r1 = oc.assert_elementwise(g1.view, oc.snake64(v, alpha), b1, what + " out1 (snake)")
    g0.check(what + " around out0")
    g1.check(what + " around out1")
    record_parity(f"elementwise.gemm.dac.{name}.t{tile}", err_over_bound=max(r0, r1), tile=plan[0], a_act=a_act)


# ----------------------------------------------------------------------------- automatic tile at the production shapes
# name -> (epilogue, (M, N, K), options, (tile, K split, panel groups)) as tests/test_gemm_plan_cpu.py pins them: one-problem launches, the
# whole output checked.  These are the only op-level launches that reach the panel-group tile order (n_groups > 0).
AUTO_CASES = {
    "gelu_fc1_4000": ("gelu", (4000, 6144, 1536), {}, (29, 1, 6)),
    "qkv_4000": ("qkv", (4000, 4608, 1536), {"H": 12, "nK": 3}, (28, 1, 6)),
    "qkv_2000": ("qkv", (2000, 4608, 1536), {"H": 12, "nK": 3}, (28, 1, 6)),
    "cross_q_3000": ("qkv", (3000, 1536, 1536), {"H": 12, "nK": 1}, (25, 1, 2)),
    "conv_w13_3000": ("silugate", (3000, 8192, 4608), {"conv": True}, (23, 1, 8)),
    "conv_w13_4000": ("silugate", (4000, 8192, 4608), {"conv": True}, (31, 1, 6)),
    "conv_lin_3000_store": ("store", (3000, 1536, 4608), {"conv": True}, (21, 1, 2)),
    "gate_proj_1536_atomic": ("gate_split", (1536, 1536, 1536), {"atomic": True}, (15, 2, 2)),
    "vit_fc1_22000": ("gelu_erf", (22000, 3072, 768), {}, (29, 1, 3)),
    "gate_fc2_3000": ("gate_split", (3000, 1536, 6144), {}, (32, 3, 0)),
    "gate_fc2_3000_f32slabs": ("gate_split_f32slabs", (3000, 1536, 6144), {}, (32, 3, 0)),
    "conv_w2_4000_h16": ("gate_split", (4000, 1536, 12288), {"conv": True}, (24, 1, 0)),
    # the single-block modulation panel cut to the smallest N that still takes tile 32 by the weight-streaming rule (N >= 16 384):
    # asserted below through the planner for 16 384 / 32 768 / 65 536
    "mod_panel_224": ("store", (224, 65536, 1536), {}, (32, 1, 0)),
}


def test_mod_panel_cut_is_the_smallest_that_keeps_tile_32():
    from test_gemm_plan_cpu import plan
    got = {n: plan(dict(epi="store", mnk=(224, n, 1536)))[0] for n in (16384, 32768, 65536, 331776)}
    assert got[331776] == 32 and got[65536] == 32, got
    assert AUTO_CASES["mod_panel_224"][1][1] == min(n for n, t in got.items() if t == 32), got


def test_auto_cases_reach_the_panel_group_order():
    assert sum(1 for c in AUTO_CASES.values() if c[3][2] > 0) >= 8
    assert {c[3][0] for c in AUTO_CASES.values()} >= {15, 21, 23, 24, 25, 28, 29, 31, 32}


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("name", list(AUTO_CASES))
def test_gemm_auto_tile_full_output(dev, name, dt):
    epi, mnk, o, want = AUTO_CASES[name]
    M, N, K = mnk
    kw = dict(want_plan=want, seed=300)
    if o.get("conv"):
        kw["conv"] = (1, M, K // 3)
    if epi == "qkv":
        kw["qkv"] = (1, M, o["H"], 0, o["nK"])
    if epi.startswith("gate_split"):
        kw["ksplit"] = 0
    if o.get("atomic"):       # no slabs: the K ranges meet in fp32 atomics on x
        run_gemm_case(dev, name, "gate", mnk, DTS[dt], **kw)
        return
    run_gemm_case(dev, name, epi, mnk, DTS[dt], **kw)


# ----------------------------------------------------------------------------- LayerNorm (+ pending slabs)
LN_SHAPES = [(500, 1536), (4096, 1536), (4097, 1536), (6000, 1536), (500, 1408)]
LN_K = [(0, None), (1, "f32"), (2, "h"), (6, "f32"), (7, "h"), (8, "f32"), (8, "h")]


def _ln_form(M, D):
    """rowops.hip's launcher: two waves per row (ln_mod_wide_kernel) at D = 1536 up to 4096 rows, one wave per row above and at D = 1408."""
    return "wide" if (D == 1536 and M <= 4096) else "one_wave"


def test_both_layernorm_forms_have_cases():
    assert {_ln_form(M, D) for M, D in LN_SHAPES} == {"wide", "one_wave"}


def _ln_set(dev, M, D, seed, odt, k, slab, tok):
    """Rows of 1e3 + N(0, 1) (test_ln_mod_width), operands per (cfg, token) with tok else vectors, k pending slabs; x and out guarded."""
    gen = torch.Generator().manual_seed(seed)
    s = {"M": M, "D": D, "x0": 1e3 + torch.randn(M, D, generator=gen)}
    if tok and M % 2 == 0 and M > 0:
        L = M // 2
        tab = torch.randn(2, L, 3 * D, generator=gen) * 0.3
        s["tabd"] = tab.to(dev)
        s["op"] = [rt.rowbcast(s["tabd"][..., c * D:], 1, L, L, ld=3 * D) for c in range(3)]
        s["full"] = [tab[..., c * D:(c + 1) * D].reshape(M, D) for c in range(3)]
    else:
        vec = torch.randn(3, D, generator=gen) * 0.3
        s["tabd"] = vec.to(dev)
        s["op"] = [rt.rowbcast(s["tabd"][c], 0) for c in range(3)]
        s["full"] = [vec[c].expand(M, D) for c in range(3)]
    if k:
        sdt = torch.float32 if (slab == "f32" or odt == torch.float32) else odt
        s["slabs"] = (torch.randn(k, M, D, generator=gen) * 0.5).to(sdt)
        s["bias"] = torch.randn(D, generator=gen) * 0.1
    s["gx"] = oc.guarded((M, D), torch.float32, dev, rows=(2, 3))
    s["gx"].view.copy_(s["x0"].to(dev))
    s["go"] = oc.guarded((M, D), odt, dev, rows=(2, 3))
    a = {"M": M, "x": s["gx"].view, "out": s["go"].view, "shift": s["op"][0], "scale": s["op"][1]}
    if k:
        s["slabs_d"], s["bias_d"] = s["slabs"].to(dev), s["bias"].to(dev)
        a.update(partials=s["slabs_d"], k=k, bias=s["bias_d"], gate=s["op"][2])
    return s, a


def _ln_check(s, a, odt, what):
    if s["M"] == 0:      # an empty row set: nothing may be written at all - the guards around it are the whole check
        s["gx"].check(f"{what}: around the empty x")
        s["go"].check(f"{what}: around the empty out")
        return 0.0
    x64, ref, bx, bo = oc.layernorm_ref_and_bound(s["x0"], s["full"][0], s["full"][1], 1e-6, odt, s.get("slabs"), s.get("bias"),
                                                  s["full"][2] if "slabs" in s else None)
    if "slabs" in s:
        rx = oc.assert_elementwise(a["x"], x64, bx, f"{what}: x written back")
    else:
        assert torch.equal(a["x"].cpu(), s["x0"]), f"{what}: x changed without pending work"
        rx = 0.0
    r = oc.assert_elementwise(a["out"], ref, bo, f"{what}: out")
    s["gx"].check(f"{what}: around x")
    s["go"].check(f"{what}: around out")
    return max(r, rx)


@pytest.mark.parametrize("odt", ALL3)
@pytest.mark.parametrize("M,D", LN_SHAPES)
@pytest.mark.parametrize("k,slab", LN_K)
def test_layernorm_elementwise(dev, M, D, odt, k, slab):
    s, a = _ln_set(dev, M, D, 5000 + k, DTS[odt], k, slab, tok=(k % 2 == 0))
    if k:
        rt.op_ln_mod_pending(a["x"], 1e-6, a["shift"], a["scale"], a["out"], a["partials"], a["k"], a["bias"], a["gate"])
    else:
        rt.op_ln_mod(a["x"], 1e-6, a["shift"], a["scale"], a["out"])
    r = _ln_check(s, a, DTS[odt], f"ln {_ln_form(M, D)} M{M} D{D} k{k}{slab or ''} {odt}")
    record_parity(f"elementwise.ln.{_ln_form(M, D)}.M{M}.D{D}.k{k}{slab or ''}.{odt}", err_over_bound=r)


@pytest.mark.parametrize("odt", ALL3)
@pytest.mark.parametrize("M0,M1,ks", [(3000, 480, (2, 8)), (0, 80, (0, 7))])
def test_layernorm_pair_elementwise(dev, M0, M1, ks, odt):
    """launch_ln_mod_pair over the audio + visual row sets ((0, 80): an empty first set), pending slabs as test_ln_mod_pair's 'both' / 'second'."""
    D = 1536
    sets = [_ln_set(dev, M, D, 6000 + 10 * i, DTS[odt], ks[i], "h", tok=(i == 0)) for i, M in enumerate((M0, M1))]
    ln_mod_pair([a for _, a in sets], D, 1e-6, rt.dt_of(sets[0][1]["out"]))
    r = max(_ln_check(s, a, DTS[odt], f"ln pair {M0}+{M1} set {i} {odt}") for i, (s, a) in enumerate(sets))
    record_parity(f"elementwise.ln_pair.{M0}+{M1}.{odt}", err_over_bound=r)


# ----------------------------------------------------------------------------- attention
def _attn_kernel_of(B, H, Sq, Skv, hd, half, pitch):
    """The kernel launch_attention (attention.hip) selects - its rule restated, so that a case names the kernel it was written for."""
    if not half:
        return "attn_kernel"
    gw = (Sq + 127) // 128 * H * B
    wide = gw >= 256 or hd != 128
    longk = wide and hd == 128 and Skv >= 512 and gw * 4 <= 2048
    nq_best, best = 0, 0
    if longk:
        for nq in (6, 5, 4):
            wgs = (Sq + 32 * nq - 1) // (32 * nq) * H * B
            if wgs <= 256 and wgs > best:
                best, nq_best = wgs, nq
        if best < 160:
            nq_best = 0
    nt = (Skv + 31) // 32
    img = nt * 32 * 256 + (128 << ((5 if pitch > 128 else 4) + 4)) + 32 * 256
    if (not wide) and hd == 128 and nt >= 4 and pitch <= 256 and img <= 160 * 1024:
        return "attn_lds_kernel"
    if nq_best:
        return f"attn_bf16_pair_kernel<{nq_best}>"
    if longk:
        return "attn_bf16_long_kernel"
    if wide:
        return f"attn_bf16_wide_kernel<{hd}>"
    return "attn_bf16_kernel"


ATTN_LDS_MAX = 160 * 1024                            # launch_attention: the LDS a staged launch may ask for
ATTN_MERGE_BYTES = 4 * 3 * 16 * 64 * 4 + 2 * 4 * 32 * 4      # its `mrg`: four waves' partial O (three fragments each) + their m and l = 50 176 B


def _attn_lds_layout(Skv, pitch):
    """launch_attention's LDS arithmetic for attn_lds_kernel: (img, merge_off, lgCV) - the operand images [K | V^T | Q] in bytes,
    where the merge records go (behind the images when img + mrg fits 160 KiB, else 0: over them, after a barrier), and the log2
    of the 16-byte chunks per LDS row of the V^T image (16 chunks up to a pitch of 128, else 32)."""
    nt, lgcv = (Skv + 31) // 32, 5 if pitch > 128 else 4
    img = nt * 32 * 256 + (128 << (lgcv + 4)) + 32 * 256
    return img, (img if img + ATTN_MERGE_BYTES <= ATTN_LDS_MAX else 0), lgcv


def _attn_form_of(B, H, Sq, Skv, hd, half, pitch):
    """_attn_kernel_of down to the selectable FORM: the fp32 kernel by head dim, attn_lds_kernel by where its merge records lie
    and by the width of its V^T image (tests/test_attention_edges_gpu.py names every form and takes each to its edges)."""
    kernel = _attn_kernel_of(B, H, Sq, Skv, hd, half, pitch)
    if kernel == "attn_kernel":
        return f"attn_kernel<{hd}>"
    if kernel == "attn_lds_kernel":
        img, merge_off, lgcv = _attn_lds_layout(Skv, pitch)
        assert img == (Skv + 31) // 32 * 32 * 256 + (128 << ((5 if pitch > 128 else 4) + 4)) + 32 * 256      # the term _attn_kernel_of stages by
        return f"attn_lds_kernel[merge_off {'!=' if merge_off else '=='} 0, lgCV {lgcv}]"
    return kernel


# name -> (B, H, Sq, Skv, split, kv_bdiv, head dim, operand kinds, kernel).  Every case: a ragged last key tile, `split` inside a query
# tile.  Workgroup counts: gw = ceil(Sq / 128) H B 128-query workgroups decide the 16-bit kernel -
#   bf16_small   gw 36 < 256, 3 key tiles (< 4: not LDS-staged)                                   -> attn_bf16_kernel
#   lds          gw 48 < 256, 8 key tiles, K + V^T + Q images 136 KiB <= 160 KiB                  -> attn_lds_kernel (head dim 128 only)
#   wide128      gw 576, Skv 77 < 512                                                             -> attn_bf16_wide_kernel<128>
#   wide64/96    head dims 64 / 96 exist in the wide form only, whatever the grid                 -> attn_bf16_wide_kernel<64 / 96>
#   long         gw 396 (x 4 <= 2048), Skv 545; 160 / 192-query workgroups 324 / 288 > 256        -> attn_bf16_long_kernel
#   pair4/5/6    gw 256 / 264 / 324; the largest workgroup count <= 256 is 256 (NQ 4) / 216 (NQ 5) / 216 (NQ 6)
ATTN_CASES = {
    "fp32_128": (4, 3, 290, 77, 40, 2, 128, ["f32"], "attn_kernel"),
    "fp32_64": (5, 3, 37, 70, 5, 1, 64, ["f32"], "attn_kernel"),
    "fp32_96": (2, 8, 70, 45, 9, 1, 96, ["f32"], "attn_kernel"),
    "bf16_small": (4, 3, 290, 77, 40, 2, 128, H16, "attn_bf16_kernel"),
    "lds": (2, 12, 250, 250, 40, 1, 128, H16, "attn_lds_kernel"),
    "wide128": (16, 12, 290, 77, 40, 8, 128, H16, "attn_bf16_wide_kernel<128>"),
    "wide64": (4, 2, 130, 33, 7, 2, 64, H16, "attn_bf16_wide_kernel<64>"),
    "wide96": (2, 8, 70, 45, 9, 1, 96, H16, "attn_bf16_wide_kernel<96>"),
    "long": (3, 12, 1350, 545, 100, 1, 128, H16, "attn_bf16_long_kernel"),
    "pair4": (2, 8, 2000, 600, 100, 1, 128, H16, "attn_bf16_pair_kernel<4>"),
    "pair5": (2, 12, 1400, 600, 100, 1, 128, H16, "attn_bf16_pair_kernel<5>"),
    "pair6": (3, 12, 1130, 545, 100, 1, 128, H16, "attn_bf16_pair_kernel<6>"),
}


def test_every_attention_kernel_has_a_case():
    """The launcher's choice cannot be read back without a profiler: its rule is restated in _attn_kernel_of and every case must
    land on the kernel it names; together they cover every kernel (and head dim / NQ form) of attention.hip."""
    for name, (B, H, Sq, Skv, split, div, hd, kinds, kernel) in ATTN_CASES.items():
        half = kinds != ["f32"]
        assert _attn_kernel_of(B, H, Sq, Skv, hd, half, (Skv + 31) // 32 * 32) == kernel, name
        assert Skv % 32 and 0 < split < Sq and split % 32, name
    have = {c[8] for c in ATTN_CASES.values()} | {f"attn_kernel<{c[6]}>" for c in ATTN_CASES.values() if c[8] == "attn_kernel"}
    need = {"attn_kernel<128>", "attn_kernel<64>", "attn_kernel<96>", "attn_bf16_kernel", "attn_lds_kernel", "attn_bf16_long_kernel"} | \
           {f"attn_bf16_wide_kernel<{h}>" for h in (64, 96, 128)} | {f"attn_bf16_pair_kernel<{n}>" for n in (4, 5, 6)}
    assert need <= have, need - have


def _attn_params():
    return [pytest.param(n, k, id=f"{n}-{k}") for n, c in ATTN_CASES.items() for k in c[7]]


@pytest.mark.parametrize("name,kind", _attn_params())
def test_attention_elementwise(dev, name, kind):
    B, H, Sq, Skv, split, div, hd, _, kernel = ATTN_CASES[name]
    dt = DTS[kind]
    half = dt != torch.float32
    q, k, v = (_rand(s, 30 + i).to(dt) for i, s in enumerate(((B, H, Sq, hd), (B // div, H, Skv, hd), (B // div, H, Skv, hd))))
    ref, bound = oc.attention_ref_and_bound(q, k, v, dt, p_dtype=dt if half else None)
    if half:      # V transposed with a padded pitch; the pad holds LARGE finite values: a pad column leaking into P V fails an element
        pitch = (Skv + 31) // 32 * 32
        vd = torch.full((B // div, H, hd, pitch), 1e4, dtype=dt)
        vd[..., :Skv] = v.transpose(2, 3)
    else:
        vd = v
    ga = oc.guarded((B, split, H * hd), dt, dev, rows=(1, 1))
    gb = oc.guarded((B, Sq - split, H * hd), dt, dev, rows=(1, 1))
    rt.op_attention(q.to(dev), k.to(dev), vd.to(dev), ga.view, gb.view, split, div)
    what = f"attention {name} ({kernel}) {kind}"
    ra = oc.assert_elementwise(ga.view, ref[:, :split], oc.Bound(bound.e[:, :split], dt), what + " outA")
    rb = oc.assert_elementwise(gb.view, ref[:, split:], oc.Bound(bound.e[:, split:], dt), what + " outB")
    ga.check(what + " around outA")
    gb.check(what + " around outB")
    record_parity(f"elementwise.attention.{name}.{kind}", err_over_bound=max(ra, rb), kernel=kernel)


# ----------------------------------------------------------------------------- cross attention fused into the q-projection GEMM
# The ATTN branch of the head-split epilogue (gemm_common.h, EPI_QKV_ATTN; tile 27, chosen by gemm_plan.h `fuses`): an attention of
# its own - K / V^T LDS images, ragged-key mask, online softmax, the second text set of a straddling 64-row tile under a per-lane
# predicate.  Sharp cases: opcheck.cross_dyadic_case (the projection exact, <= 1 % of q ambiguous in its 16-bit rounding).
# The cases (opcheck.CROSS_CASES) are shared with the CPU emulation of test_opcheck_cpu.py.
CROSS_CASES = oc.CROSS_CASES
# name -> (Bc, L, H, bdiv, Skv, pitch, tile, operand kind, attn_out 8 bytes off): the launcher must refuse to fuse (gemm_plan.h `fuses`)
CROSS_FALLBACKS = {
    "skv97": (2, 100, 2, 1, 97, 128, 27, "h", False),
    "pitch88": (2, 100, 2, 1, 77, 88, 27, "h", False),
    "out_misaligned": (2, 100, 2, 1, 77, 96, 27, "h", True),
    "three_sets_in_a_tile": (9, 8, 2, 3, 77, 96, 27, "h", False),      # L bdiv = 24 < 64 and M = 72 > 2 L bdiv
    "fp32_operands": (2, 100, 2, 1, 77, 96, 0, "f32", False),
}


@functools.lru_cache(maxsize=4)
def _fallback_case(Bc, L, H, bdiv, Skv):
    return oc.cross_dyadic_case(Bc, L, H, bdiv, Skv, seed=8500 + 7 * L + Skv, k_scale=2.0)


def _bits(t):
    return t.detach().contiguous().view(oc._INT[t.element_size()]).cpu().clone()


def _cross_launch(dev, c, dt, pitch, tile, misalign=False):
    """Buffers (all guarded or snapshotted), descriptor and launch of one cross-q problem; returns a dict."""
    Bc, L, H, M, Skv = c["M"] // c["L"], c["L"], c["H"], c["M"], c["Skv"]
    h16 = dt != torch.float32
    kd = c["k"].to(dev, dt)
    if h16:      # V^T [sets, H, 128, pitch]; the columns beyond Skv hold LARGE finite values: a masked key must weigh exactly nothing
        vt = torch.full((kd.shape[0], H, 128, pitch), 1e4, dtype=dt)
        vt[..., :Skv] = c["v"].transpose(2, 3).to(dt)
        vt = vt.to(dev)
    else:
        vt = c["v"].to(dev)
    gq = oc.guarded((Bc, H, L, 128), dt, dev, rows=(1, 1))
    go = oc.guarded((M, H * 128), dt, dev, rows=(2, 3), misalign=(8 // gq.view.element_size() if misalign else 0))
    assert go.view.data_ptr() % 16 == (8 if misalign else 0) and kd.data_ptr() % 16 == 0 and vt.data_ptr() % 16 == 0
    snap = dict(k=_bits(kd), v=_bits(vt), q=_bits(gq.view), out=_bits(go.view))
    desc = rt.qkv_split_desc(L, H, [c["gain"].to(dev)], [c["pos"].to(dev)], [gq.view], L, 0, 1e-6, c["cos"].to(dev), c["sin"].to(dev),
                             attn=(kd, vt, go.view, c["bdiv"]))
    d = rt.gemm_desc(c["A"].to(dev, dt), c["W"].to(dev, dt), c["b"].to(dev), epilogue=rt.EPI_QKV_SPLIT, qkv=desc, tile=tile)
    plan = _plan(d)
    assert not isinstance(plan, str), plan
    _launch(d)
    assert gemm_last()[0] == plan[0]
    return dict(kd=kd, vt=vt, gq=gq, go=go, snap=snap, desc=desc, plan=plan)


def _cross_params(table):
    return [pytest.param(n, k, id=f"{n}-{k}") for n in table for k in H16]


@pytest.mark.parametrize("name,kind", _cross_params(CROSS_CASES))
def test_gemm_cross_attention_epilogue_elementwise(dev, name, kind):
    """Every element of the fused epilogue's attention rows against opcheck.cross_attention_ref_and_bound; q never leaves the chip;
    K, V^T and everything around the output keep their bits.
    MI355X: bf16 0.59 .. 0.93 of the bound, fp16 0.11 .. 0.53 - the CPU emulation of test_opcheck_cpu.py gives the SAME figures to
    three digits on the same operands, so they are the arithmetic's, not the kernel's.  Above 0.5 because u_p is half the unit
    round-off of the type and, with scores of spread 2, a few probabilities carry a row; fp16 is lower because its output term
    (half an ulp of the result) is of u_p's own size."""
    Bc, L, H, bdiv, Skv, pitch, tile, ks = CROSS_CASES[name]
    dt = DTS[kind]
    c = oc.cross_case(name)
    r = _cross_launch(dev, c, dt, pitch, tile)
    what = f"cross attention epilogue {name} {kind}"
    assert r["desc"].fused() and r["plan"][0] == 27 and gemm_last()[0] == 27, (what, r["plan"], r["desc"].fused())
    ref, bound, share = oc.cross_attention_ref_and_bound(c["q64"], c["e_q"], c["k"], c["v"], c["sets"], dt)
    assert share <= 0.01, share
    ratio = oc.assert_elementwise(r["go"].view, ref, bound, what)
    print(f"{what}: err / bound {ratio:.3f}, ambiguous share {share:.2e}")
    r["go"].check(what + ": around attn_out")
    r["gq"].check(what + ": around q")
    assert torch.equal(_bits(r["gq"].view), r["snap"]["q"]), f"{what}: q written by a fused launch (it never leaves the chip)"
    assert torch.equal(_bits(r["kd"]), r["snap"]["k"]) and torch.equal(_bits(r["vt"]), r["snap"]["v"]), f"{what}: K / V^T changed"
    assert bool((r["vt"][..., Skv:] == 1e4).all()), f"{what}: V^T columns [Skv, pitch) must hold 1e4"
    record_parity(f"elementwise.gemm.cross_attn.{name}.{kind}", err_over_bound=ratio, ambiguous_share=share, tile=r["plan"][0])


@pytest.mark.parametrize("name,kind", [pytest.param(n, k, id=f"{n}-{k}") for n, c in CROSS_FALLBACKS.items() for k in (["f32"] if c[7] == "f32" else H16)])
def test_gemm_cross_attention_fallbacks(dev, name, kind):
    """Problems the fused form does not serve: the plain head split runs (fused() False), attn_out keeps every bit, q is written and
    correct under the head-split bound."""
    Bc, L, H, bdiv, Skv, pitch, tile, ok, misalign = CROSS_FALLBACKS[name]
    dt = DTS[kind]
    c = _fallback_case(Bc, L, H, bdiv, Skv)
    r = _cross_launch(dev, c, dt, pitch, tile, misalign)
    what = f"cross attention fallback {name} {dt}"
    assert not r["desc"].fused(), what
    assert torch.equal(_bits(r["go"].view), r["snap"]["out"]), f"{what}: attn_out written by a plain head split"
    r["go"].check(what + ": around attn_out")
    want = c["q64"].view(Bc, L, H, 128).transpose(1, 2)
    bound = oc.head_split_bound(torch.zeros_like(c["y64"]), c["y64"], dt, c["gain"])
    bound.e = bound.e.view(Bc, L, H, 128).transpose(1, 2)
    ratio = oc.assert_elementwise(r["gq"].view, want, bound, what + ": q")
    r["gq"].check(what + ": around q")
    assert torch.equal(_bits(r["kd"]), r["snap"]["k"]) and torch.equal(_bits(r["vt"]), r["snap"]["v"])
    record_parity(f"elementwise.gemm.cross_attn_fallback.{name}.{str(dt)[6:]}", err_over_bound=ratio, tile=r["plan"][0])


# ----------------------------------------------------------------------------- the conditioning encoders' attention (head dim 64)
# foley_op_attention_scatter: query (g, t) lands in row out_rows[g, t] of a token-major buffer.  fp32 operands: attn_kernel<*, 64>;
# 16-bit: attn_bf16_wide_kernel<*, *, 64> (head dim 64 exists in the wide form only); grp_q / grp_kv: its block-diagonal
# instantiation <.., 64, GRP = true>.  (G, H, Sq, Skv) of test_attention_scatter:
SCATTER_CASES = [(3, 12, 8, 9), (2, 12, 1, 197), (5, 4, 196, 197), (1, 12, 130, 77)]
# name -> (G, H, p groups per sequence, grp_q, grp_kv, queries cut from the last group, surplus keys beyond the last group)
GROUPED_CASES = {
    # the five of test_attention_scatter_grouped
    "time_attn_14": (6, 12, 14, 8, 9, 0, 0), "p16": (3, 4, 16, 8, 9, 0, 0), "p5": (2, 12, 5, 8, 9, 0, 0), "straddling_33_40": (4, 2, 3, 33, 40, 0, 0),
    "p1": (1, 12, 1, 8, 9, 0, 0),
    # new: legal by the launcher's check ceil(Sq / grp_q) grp_kv <= Skv, reached by no other test
    "ragged_last_group": (3, 4, 16, 8, 9, 3, 0),          # Sq = p grp_q - 3
    "surplus_keys": (2, 12, 5, 8, 9, 0, 7),                # Skv = p grp_kv + 7: keys nobody may see (their V is 1e4)
    "ragged_and_surplus": (2, 2, 3, 33, 40, 3, 7),
    "gkv32": (2, 4, 5, 20, 32, 0, 0),                      # groups aligned to the 32-key tile
    "gkv33": (2, 4, 5, 20, 33, 0, 0),                      # ... and one key past it
    "gq1": (2, 12, 14, 1, 9, 0, 0),                        # one query per group
}


def _scatter_setup(dev, dt, G, H, Sq, Skv, rows, seed, v_fill_from=None):
    """qkv rows -> (q, k, v as the kernel reads it, v [G, H, Skv, 64] for the reference, out_rows, guarded NaN out, its prefill bits)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * H * 64, generator=g).to(dt).to(dev)
    iq = torch.randperm(rows, generator=g)[: G * Sq].view(G, Sq).to(torch.int32).to(dev)
    ikv = torch.randint(0, rows, (G, Skv), generator=g, dtype=torch.int32).to(dev)
    q, k, v = rt.op_qkv_regroup(qkv, H, iq, ikv)
    if dt != torch.float32:
        v[..., (Skv if v_fill_from is None else v_fill_from):] = 1e4          # the pad up to the pitch (and surplus keys): large and finite
        vref = v[..., :Skv].transpose(2, 3)
    else:
        vref = v
    out = oc.guarded((rows, H * 64), dt, dev, rows=(2, 3))
    return q, k, v, vref, iq, out, _bits(out.view)


def _scatter_check(out, prefill, iq, ref, bound, dt, what):
    rows_i = iq.view(-1).long().cpu()
    n = ref.shape[0] * ref.shape[1]
    ratio = oc.assert_elementwise(out.view[rows_i.to(out.view.device)], ref.reshape(n, -1), oc.Bound(bound.e.reshape(n, -1), dt), what)
    keep = torch.ones(out.view.shape[0], dtype=torch.bool)
    keep[rows_i] = False
    assert int(keep.sum()) >= 5, "rows must exceed the mapped queries"
    assert torch.equal(_bits(out.view)[keep], prefill[keep]), f"{what}: rows no query maps to were written"
    out.check(what + ": around out")
    return ratio


@pytest.mark.parametrize("kind", ALL3)
@pytest.mark.parametrize("G,H,Sq,Skv", SCATTER_CASES)
def test_attention_scatter_elementwise(dev, kind, G, H, Sq, Skv):
    """The scatter store of attn_kernel<*, 64> (fp32) and attn_bf16_wide_kernel<*, *, 64> (16 bit) against the fp64 softmax
    (opcheck.attention_ref_and_bound); rows no query maps to and the guards keep their bits; the V^T pad holds 1e4.
    (3, 12, 8, 9) in bf16 is what made attn_bf16_wide_kernel<*, *, 64> carry a probability as its bf16 rounding PLUS the residual:
    with P rounded once, 5 of 18 432 elements lay outside the bound (worst 1.10) - see test_attention_scatter_grouped_elementwise."""
    dt = DTS[kind]
    half = dt != torch.float32
    q, k, v, vref, iq, out, prefill = _scatter_setup(dev, dt, G, H, Sq, Skv, G * Sq + 7, 9000 + G * 100 + Sq)
    ref, bound = oc.attention_ref_and_bound(q.cpu(), k.cpu(), vref.cpu(), dt, p_dtype=dt if half else None)
    rt.op_attention_scatter(q, k, v, iq, out.view)
    kernel = "attn_bf16_wide_kernel<64> + out_rows" if half else "attn_kernel<64> + out_rows"
    ratio = _scatter_check(out, prefill, iq, ref, bound, dt, f"attention scatter ({kernel}) G{G} H{H} Sq{Sq} Skv{Skv} {kind}")
    print(f"scatter G{G} H{H} Sq{Sq} Skv{Skv} {kind}: err / bound {ratio:.3f}")
    record_parity(f"elementwise.attention_scatter.G{G}_H{H}_Sq{Sq}_Skv{Skv}.{kind}", err_over_bound=ratio, kernel=kernel)


@pytest.mark.parametrize("kind", H16)
@pytest.mark.parametrize("name", list(GROUPED_CASES))
def test_attention_scatter_grouped_elementwise(dev, name, kind):
    """The block-diagonal instantiation attn_bf16_wide_kernel<T, O, 64, GRP> against the fp64 block-diagonal softmax, the bound of
    opcheck.attention_ref_and_bound applied group by group (opcheck.grouped_attention_ref_and_bound).
    A finding of these cases, fixed in the kernel: with a probability rounded ONCE to bf16, every case of 9 keys per group had
    elements outside the bound - err / bound (offenders of elements):
        time_attn_14 1.19 (39 of 516 096)   p16 1.36 (6 of 98 304)   p5 1.07 (7 of 61 440)   p1 1.06 (1 of 6 144)
        ragged_last_group 1.13 (6 of 96 000)   surplus_keys 1.09 (12 of 61 440)   gq1 1.05 (2 of 21 504)
    scattered over all rows and columns, fp16 inside (worst 0.98), bf16 inside from 32 keys per group on.  u_p = U16 is half the
    unit round-off of bf16; nine probabilities do not average, and one of them can carry a row's whole error (the CPU emulation
    of test_opcheck_cpu.py shows the same at 1.25).  The head-dim-64 bf16 kernel now multiplies V with the rounding's residual
    as well (attention.hip PSPLIT), which takes the rounding of P down to 2^-16; the bound is unchanged."""
    G, H, p, gq, gkv, cut, surplus = GROUPED_CASES[name]
    dt = DTS[kind]
    Sq, Skv = p * gq - cut, p * gkv + surplus
    q, k, v, vref, iq, out, prefill = _scatter_setup(dev, dt, G, H, Sq, Skv, G * p * max(gq, gkv) + 5, 9500 + G * 100 + p, v_fill_from=p * gkv)
    ref, bound = oc.grouped_attention_ref_and_bound(q.cpu(), k.cpu(), vref.cpu(), gq, gkv, dt, p_dtype=dt)
    rt.op_attention_scatter(q, k, v, iq, out.view, gq, gkv)
    ratio = _scatter_check(out, prefill, iq, ref, bound, dt, f"grouped attention scatter {name} {kind}")
    print(f"grouped {name} {kind}: err / bound {ratio:.3f}")
    record_parity(f"elementwise.attention_scatter_grouped.{name}.{kind}", err_over_bound=ratio, kernel="attn_bf16_wide_kernel<64, grp>")


def test_every_fused_and_encoder_attention_form_has_a_case():
    """The attention forms outside foley_op_attention (test_every_attention_kernel_has_a_case covers those), each tied to the table
    whose cases reach it; removing a case the coverage rests on fails here."""
    forms = {
        "attn_kernel<64> + out_rows": [("f32",) + s for s in SCATTER_CASES if "f32" in ALL3],
        "attn_bf16_wide_kernel<64> + out_rows": [(kd,) + s for s in SCATTER_CASES for kd in H16],
        "attn_bf16_wide_kernel<64, grp>": list(GROUPED_CASES),
        "gemm epilogue EPI_QKV_ATTN": list(CROSS_CASES),
    }
    assert all(forms.values()), [n for n, v in forms.items() if not v]
    assert set(SCATTER_CASES) >= {(3, 12, 8, 9), (2, 12, 1, 197), (5, 4, 196, 197), (1, 12, 130, 77)}
    for G, H, Sq, Skv in SCATTER_CASES:       # 16-bit operands at head dim 64 always take the wide form (attention.hip launch_attention)
        assert _attn_kernel_of(G, H, Sq, Skv, 64, True, (Skv + 31) // 32 * 32) == "attn_bf16_wide_kernel<64>"
    gc = set(GROUPED_CASES.values())
    assert gc >= {(6, 12, 14, 8, 9, 0, 0), (3, 4, 16, 8, 9, 0, 0), (2, 12, 5, 8, 9, 0, 0), (4, 2, 3, 33, 40, 0, 0), (1, 12, 1, 8, 9, 0, 0)}
    assert any(c[5] > 0 for c in gc) and any(c[6] > 0 for c in gc) and any(c[3] == 1 for c in gc), "ragged last group, surplus keys, grp_q = 1"
    assert {32, 33} <= {c[4] for c in gc}, "groups aligned to the key tile and one key past it"
    for G, H, p, gq, gkv, cut, surplus in gc:                     # legal by the launcher's check
        assert (p * gq - cut + gq - 1) // gq * gkv <= p * gkv + surplus and 0 <= cut < gq
    edges = {c[4] for n, c in CROSS_CASES.items() if c[:4] == (2, 250, 2, 1) and c[5] == 96}
    assert edges >= {1, 32, 33, 64, 65, 77, 95, 96} and any(c[5] == 104 for c in CROSS_CASES.values())
    multi = {(c[1], c[3], (c[0] + c[3] - 1) // c[3]) for c in CROSS_CASES.values() if (c[0] + c[3] - 1) // c[3] > 2}      # (L, bdiv, sets)
    assert multi >= {(64, 1, 3), (65, 1, 3), (70, 1, 5), (127, 1, 3), (40, 2, 3)}, multi
    assert any(c[1] * c[3] < 64 and c[0] * c[1] <= 2 * c[1] * c[3] for c in CROSS_CASES.values()), "straddling small problem"
    assert any(c[7] >= 15 for c in CROSS_CASES.values()), "large scores"
    assert CROSS_CASES["auto_plan"] == (2, 250, 12, 1, 77, 96, 0, 2.0)
    assert all(c[6] in (0, 27) and c[4] <= 96 and c[5] >= 96 and c[5] % 8 == 0 for c in CROSS_CASES.values())
    assert set(CROSS_FALLBACKS) == {"skv97", "pitch88", "out_misaligned", "three_sets_in_a_tile", "fp32_operands"}
