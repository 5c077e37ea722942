"""Row-broadcast operands that read a device counter (RowBcast::step_ptr), at op level.

run_forward gives every shift / scale / gate / addend of the sampler loop a counter and a step stride: the operand reads
base + *counter * step_stride.  The op entries' descriptor (foley_rowbcast) has no such field, so the test-only hook
foley_debug_rowbcast_step (foley_rt.hip; not in include/foley_hip.h, typed here with ctypes) attaches one to the operands the
calling thread's op entries convert.  Two checks per case:
  * the fp64 reference and per-element bounds of the LayerNorm / GEMM / row-kernel op tests (opcheck), guards intact;
  * bit for bit, the call with the counter at s against the same call without a counter and the bases advanced by
    s * step_stride on the host - the counter only moves addresses.
The LayerNorm launches whose operands share one counter and one row map take the resolved kernels (one scalar counter load,
one row offset per row: rowops.hip ln_mod_kernel / ln_mod_wide_kernel); operands with different counters take the per-operand
kernels (ln_mod_each_kernel / ln_mod_wide_each_kernel)."""
import ctypes as C
import math

import pytest
import torch

import opcheck as oc
from foley_amd.host import runtime as rt, tables
from test_pairs_gpu import ln_mod_pair

pytestmark = pytest.mark.gpu

N_ITER = 4                      # iterations the step-indexed tables hold
COUNTERS = (0, 1, N_ITER - 1)
L, RPC, LS, PER = 3, 3, 16, 8   # two (or, at M = 7, three) CFG halves of L = 3 tokens; mode 2: 16 source rows, period 8; 3 is no multiple of 16
_typed = []


def _hook(p0=None, p1=None, stride=0):
    lib = rt.load_library()
    if not _typed:
        lib.foley_debug_rowbcast_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.foley_debug_rowbcast_step.restype = None
        _typed.append(True)
    lib.foley_debug_rowbcast_step(p0.data_ptr() if p0 is not None else None, p1.data_ptr() if p1 is not None else None, stride)


class stepping:
    """with stepping(counter words, stride): the op entries of this thread attach the counter(s) to their operands."""

    def __init__(self, stride, p0, p1=None):
        self.a = (p0, p1, stride)

    def __enter__(self):
        _hook(*self.a)

    def __exit__(self, *exc):
        _hook()


def _rows_of(kind, M):
    """(operand rows, index of the operand row stream row r reads) of the layouts: vec | tok | up_periodic | up_dense | up_mixed."""
    r = torch.arange(M)
    cfg, l = r // RPC, r % L
    ncfg = (M + RPC - 1) // RPC
    if kind == "vec":
        return 1, torch.zeros(M, dtype=torch.long)
    if kind == "tok":
        return ncfg * L, cfg * L + l
    s = tables.nearest_exact_index(L, LS)[l]
    if kind == "up_periodic":
        return ncfg * PER, cfg * PER + (s & (PER - 1))
    if kind == "up_dense":
        return ncfg * LS, cfg * LS + s
    assert kind == "up_mixed"     # half 0 periodic (PER rows), the others with all their LS rows from row PER on
    return PER + (ncfg - 1) * LS, torch.where(cfg < 1, cfg * PER + (s & (PER - 1)), PER + (cfg - 1) * LS + s)


def _rb(kind, t, ld):
    if kind == "vec":
        return rt.rowbcast(t, 0, ld=ld)
    if kind == "tok":
        return rt.rowbcast(t, 1, RPC, L, ld=ld)
    period, pc = {"up_periodic": (PER, 0), "up_dense": (0, 0), "up_mixed": (PER, 1)}[kind]
    return rt.rowbcast(t, 2, RPC, L, ld=ld, Ls=LS, period=period, periodic_cfgs=pc)


def _table(dev, kind, M, D, seed, chunks=3):
    """Step-indexed operand table [N_ITER, rows, chunks * D] (fp32, device) with the row index of every stream row."""
    rows, idx = _rows_of(kind, M)
    g = torch.Generator().manual_seed(seed)
    tab = (torch.randn(N_ITER, rows, chunks * D, generator=g) * 0.3).to(dev)
    return tab, idx


def _ln_case(dev, M, D, odt, kind, k, slab, present, seed):
    """Inputs of one LayerNorm row set; operands: chunk 0 shift, 1 scale, 2 gate of one step-indexed table."""
    g = torch.Generator().manual_seed(seed)
    s = {"M": M, "D": D, "kind": kind, "present": present, "x0": 1e3 + torch.randn(M, D, generator=g)}
    s["tab"], s["idx"] = _table(dev, kind, M, D, seed + 1)
    if k:
        sdt = torch.float32 if (slab == "f32" or odt == torch.float32) else odt
        s["slabs"] = (torch.randn(k, M, D, generator=g) * 0.5).to(sdt)
        s["bias"] = torch.randn(D, generator=g) * 0.1
        s["slabs_d"], s["bias_d"] = s["slabs"].to(dev), s["bias"].to(dev)
    return s


def _ln_args(s, dev, odt, it):
    """Launch arguments with the operand bases at iteration `it` of the table (0: where a counter starts from)."""
    D, tab = s["D"], s["tab"]
    gx = oc.guarded((s["M"], D), torch.float32, dev, rows=(2, 3))
    gx.view.copy_(s["x0"].to(dev))
    go = oc.guarded((s["M"], D), odt, dev, rows=(2, 3))
    op = [_rb(s["kind"], tab[it][:, c * D:], tab.shape[-1]) for c in range(3)]
    a = {"M": s["M"], "x": gx.view, "out": go.view, "shift": op[0] if s["present"] else None, "scale": op[1] if s["present"] else None,
         "gx": gx, "go": go}
    if "slabs" in s:
        a.update(partials=s["slabs_d"], k=s["slabs"].shape[0], bias=s["bias_d"], gate=op[2])
    return a


def _ln_launch(a, eps):
    if "partials" in a:
        rt.op_ln_mod_pending(a["x"], eps, a["shift"], a["scale"], a["out"], a["partials"], a["k"], a["bias"], a["gate"])
    else:
        rt.op_ln_mod(a["x"], eps, a["shift"], a["scale"], a["out"])


def _ln_check(s, a, odt, it, eps, what):
    D, rows = s["D"], s["tab"][it].cpu()[s["idx"]]
    full = [rows[:, c * D:(c + 1) * D] for c in range(3)]
    x64, ref, bx, bo = oc.layernorm_ref_and_bound(s["x0"], full[0] if s["present"] else None, full[1] if s["present"] else None, eps, odt,
                                                  s.get("slabs"), s.get("bias"), full[2] if "slabs" in s else None)
    if "slabs" in s:
        r = oc.assert_elementwise(a["x"], x64, bx, f"{what}: x written back")
    else:
        assert torch.equal(a["x"].cpu(), s["x0"]), f"{what}: x changed without pending work"
        r = 0.0
    r = max(r, oc.assert_elementwise(a["out"], ref, bo, f"{what}: out"))
    a["gx"].check(f"{what}: around x")
    a["go"].check(f"{what}: around out")
    return r


def _stride(s):
    return s["tab"].shape[1] * s["tab"].shape[2]


KINDS = ["vec", "tok", "up_periodic", "up_dense", "up_mixed"]
LN_K = [(0, None), (1, "h"), (6, "f32"), (7, "h"), (7, "f32")]      # 6 fills the slab loop's batch, 7 starts a second one


# bf16 output (the sampler's): everything; fp32 output (fp32 slabs only): the two-wave kernel at both ends of the layouts
LN_CASES = [(D, torch.bfloat16, kind, k, slab) for D in (1536, 512) for kind in KINDS for k, slab in LN_K]
LN_CASES += [(1536, torch.float32, kind, k, slab) for kind in ("vec", "up_mixed") for k, slab in ((0, None), (7, "f32"))]


@pytest.mark.parametrize("D,odt,kind,k,slab", LN_CASES, ids=[f"D{c[0]}-{str(c[1])[6:]}-{c[2]}-k{c[3]}{c[4] or ''}" for c in LN_CASES])
def test_ln_counter(dev, D, odt, kind, k, slab):
    """D = 1536: the two-wave kernel at three float4 per lane; D = 512: at one.  M = 1, 3, 7; shift / scale present and absent;
    counter 0, 1 and N_ITER - 1."""
    eps, worst = 1e-6, 0.0
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    for M in (1, 3, 7):
        for present in (True, False):
            if not present and not k:
                continue      # no operand at all: nothing of this test's left
            s = _ln_case(dev, M, D, odt, kind, k, slab, present, 100 * M + k)
            for it in COUNTERS:
                what = f"ln D{D} M{M} {kind} k{k}{slab or ''} {'mod' if present else 'plain'} counter {it}"
                ctr.fill_(it)
                a = _ln_args(s, dev, odt, 0)
                with stepping(_stride(s), ctr):
                    _ln_launch(a, eps)
                worst = max(worst, _ln_check(s, a, odt, it, eps, what))
                b = _ln_args(s, dev, odt, it)      # no counter, bases advanced on the host
                _ln_launch(b, eps)
                oc.assert_bits_equal(a["out"], b["out"], f"{what}: out, counter against advanced bases")
                oc.assert_bits_equal(a["x"], b["x"], f"{what}: x, counter against advanced bases")
    oc.record_parity(f"rowbcast_entry.ln.D{D}.{kind}.k{k}{slab or ''}.{str(odt)[6:]}", err_over_bound=worst)


@pytest.mark.parametrize("D", [1536, 512])
@pytest.mark.parametrize("kind0,kind1", [("up_mixed", "vec"), ("tok", "tok"), ("vec", "up_periodic")])
@pytest.mark.parametrize("k0,k1", [(7, 1), (0, 6), (0, 0)])
def test_ln_pair_counter(dev, D, kind0, kind1, k0, k1):
    """launch_ln_mod_pair: a first row set of 7 rows and a second of ONE row, each with its own row map, one counter for both."""
    odt, eps, worst = torch.bfloat16, 1e-6, 0.0
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    sets = [_ln_case(dev, 7, D, odt, kind0, k0, "h", True, 700 + k0), _ln_case(dev, 1, D, odt, kind1, k1, "h", True, 900 + k1)]
    # one step stride for the whole launch (the hook's, as run_forward's tables have one): the larger table's; the smaller one is
    # laid out with it
    stride = max(_stride(s) for s in sets)
    for s in sets:
        t = torch.zeros(N_ITER, stride, device=dev)
        t[:, :_stride(s)] = s["tab"].reshape(N_ITER, -1)
        s["tab"] = t[:, :_stride(s)].view(N_ITER, s["tab"].shape[1], s["tab"].shape[2])
    for it in COUNTERS:
        ctr.fill_(it)
        a = [_ln_args(s, dev, odt, 0) for s in sets]
        with stepping(stride, ctr):
            ln_mod_pair(a, D, eps, rt.dt_of(a[0]["out"]))
        b = [_ln_args(s, dev, odt, it) for s in sets]
        ln_mod_pair(b, D, eps, rt.dt_of(b[0]["out"]))
        for i, s in enumerate(sets):
            what = f"ln pair D{D} set {i} ({s['kind']}, k {(k0, k1)[i]}) counter {it}"
            worst = max(worst, _ln_check(s, a[i], odt, it, eps, what))
            oc.assert_bits_equal(a[i]["out"], b[i]["out"], f"{what}: out, counter against advanced bases")
            oc.assert_bits_equal(a[i]["x"], b[i]["x"], f"{what}: x, counter against advanced bases")
    oc.record_parity(f"rowbcast_entry.ln_pair.D{D}.{kind0}+{kind1}.k{k0}+{k1}", err_over_bound=worst)


@pytest.mark.parametrize("D", [1536, 512])
@pytest.mark.parametrize("kind", ["vec", "up_mixed"])
@pytest.mark.parametrize("k", [0, 7])
def test_ln_operands_with_different_counters(dev, D, kind, k):
    """Shift and scale (and gate) carry DIFFERENT counter words (holding the same value): the launcher's host check sends the
    launch down the per-operand path, which still meets the reference."""
    odt, eps, it = torch.bfloat16, 1e-6, N_ITER - 1
    c0 = torch.full((1,), it, dtype=torch.int32, device=dev)
    c1 = torch.full((1,), it, dtype=torch.int32, device=dev)
    s = _ln_case(dev, 7, D, odt, kind, k, "h", True, 1300 + k)
    a = _ln_args(s, dev, odt, 0)
    with stepping(_stride(s), c0, c1):
        _ln_launch(a, eps)
    r = _ln_check(s, a, odt, it, eps, f"ln D{D} {kind} k{k}, two counter words")
    oc.record_parity(f"rowbcast_entry.ln_each.D{D}.{kind}.k{k}", err_over_bound=r)


# ----------------------------------------------------------------------------- gated-residual GEMM
GM, GN, GK = 64, 128, 256      # the smallest tile-legal gated-residual problem


def _both16(t):
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -17, torch.zeros_like(t), t)


@pytest.mark.parametrize("kind", ["vec", "up_mixed"])
@pytest.mark.parametrize("form", ["direct", "deferred"])
def test_gemm_gate_counter(dev, kind, form):
    """x += gate * (A W^T + b) with a step-indexed gate: the direct form applies the gate in the epilogue; the deferred split-K
    (ks = 2) stores its slabs and leaves the residual alone - gate and counter then belong to the LayerNorm that follows, run
    here on the GEMM's own slabs."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(31)
    A, W = _both16(torch.randn(GM, GK, generator=g)), _both16(torch.randn(GN, GK, generator=g) / math.sqrt(GK))
    bias, x0 = torch.randn(GN, generator=g) * 0.1, torch.randn(GM, GN, generator=g)
    # GM rows as CFG halves of L tokens: the gate table is laid out for ceil(GM / RPC) halves
    rows, idx = _rows_of(kind, GM)
    tab = (torch.randn(N_ITER, rows, GN, generator=g) * 0.5).to(dev)
    ref, mag = oc.gemm_ref64(A, W, None)
    Ad, Wd, bd = A.to(dev, dt), W.to(dev, dt), bias.to(dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    stride, worst = rows * GN, 0.0

    def launch(it_base, counter):
        gx = oc.guarded((GM, GN), torch.float32, dev, rows=(2, 3))
        gx.view.copy_(x0.to(dev))
        kw = dict(epilogue=rt.EPI_GATE_RES, rb=_rb(kind, tab[it_base], GN), out0=gx.view, ksplit=1)
        gs = None
        if form == "deferred":
            gs = oc.guarded((2, GM, GN), dt, dev, rows=(1, 1))
            kw.update(ksplit=2, partials=gs.view)
        if counter is None:
            ks = rt.op_gemm(Ad, Wd, bd, **kw)
        else:
            with stepping(stride, counter):
                ks = rt.op_gemm(Ad, Wd, bd, **kw)
        return gx, gs, ks

    for it in COUNTERS:
        ctr.fill_(it)
        what = f"gemm gate {kind} {form} counter {it}"
        gx, gs, ks = launch(0, ctr)
        hx, hs, ks_h = launch(it, None)
        assert ks == ks_h == (2 if form == "deferred" else 1), (what, ks, ks_h)
        gate = tab[it].cpu()[idx].double()
        oc.assert_bits_equal(gx.view, hx.view, f"{what}: x, counter against advanced bases")
        if form == "direct":
            e_y = (GK + 4) * oc.U32 * (mag + bias.double().abs())
            y = ref + bias.double()
            worst = max(worst, oc.assert_elementwise(gx.view, x0.double() + gate * y, oc.gated_residual_bound(e_y, gate, x0, y), what))
        else:
            assert torch.equal(gx.view.cpu(), x0), f"{what}: residual touched by a deferred split-K launch"
            oc.assert_bits_equal(gs.view, hs.view, f"{what}: slabs, counter against advanced bases")
            e0 = (GK + 4) * oc.U32 * mag
            worst = max(worst, oc.assert_elementwise(gs.view.double().sum(0), ref, oc.slab_bound(e0, mag, 2, dt), what))
            # the LayerNorm that finishes the update, with the same gate and counter
            outs = []
            for base, counter in ((0, ctr), (it, None)):
                go = oc.guarded((GM, GN), dt, dev, rows=(2, 3))
                xg = gx if counter is not None else hx
                gate_rb = _rb(kind, tab[base], GN)
                if counter is None:
                    rt.op_ln_mod_pending(xg.view, 1e-6, None, None, go.view, gs.view, 2, bd, gate_rb)
                else:
                    with stepping(stride, counter):
                        rt.op_ln_mod_pending(xg.view, 1e-6, None, None, go.view, gs.view, 2, bd, gate_rb)
                outs.append((xg, go))
            x64, o64, bx, bo = oc.layernorm_ref_and_bound(x0, None, None, 1e-6, dt, gs.view.cpu(), bias, gate)
            worst = max(worst, oc.assert_elementwise(outs[0][0].view, x64, bx, f"{what}: x after the LayerNorm"),
                        oc.assert_elementwise(outs[0][1].view, o64, bo, f"{what}: LayerNorm out"))
            oc.assert_bits_equal(outs[0][0].view, outs[1][0].view, f"{what}: x after the LayerNorm, counter against advanced bases")
            oc.assert_bits_equal(outs[0][1].view, outs[1][1].view, f"{what}: LayerNorm out, counter against advanced bases")
            for xg, go in outs:
                go.check(f"{what}: around the LayerNorm out")
            gs.check(f"{what}: around the slabs")
            hs.check(f"{what}: around the slabs")
        gx.check(f"{what}: around x")
        hx.check(f"{what}: around x")
    oc.record_parity(f"rowbcast_entry.gemm.{kind}.{form}", err_over_bound=worst)


# ----------------------------------------------------------------------------- rows_add_act
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["add", "silu"])
@pytest.mark.parametrize("R,D", [(1, 512), (7, 1536), (300, 100)])      # (300, 100): more than one workgroup, rows no multiple of 4
def test_rows_add_act_counter(dev, R, D, act, odt):
    g = torch.Generator().manual_seed(17)
    a, tab = torch.randn(R, D, generator=g), torch.randn(N_ITER, D, generator=g)
    ad, tabd = a.to(dev), tab.to(dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    worst = 0.0
    for it in COUNTERS:
        ctr.fill_(it)
        what = f"rows_add_act R{R} D{D} {'silu' if act else 'add'} counter {it}"
        go, ho = oc.guarded((R, D), odt, dev), oc.guarded((R, D), odt, dev)
        with stepping(D, ctr):
            rt.op_rows_add_act(ad, tabd[0], go.view, act)
        rt.op_rows_add_act(ad, tabd[it], ho.view, act)
        oc.assert_bits_equal(go.view, ho.view, f"{what}: counter against advanced base")
        ref, bound = oc.rows_add_act_ref_and_bound(a, tab[it], act, odt, dev)
        if bound is None:
            oc.assert_bits_equal(go.view, oc.sum32_cast(a, tab[it], odt), what)
        else:
            worst = max(worst, oc.assert_elementwise(go.view, ref, bound, what))
        go.check(what)
        ho.check(what)
    oc.record_parity(f"rowbcast_entry.rows_add_act.R{R}.D{D}.{'silu' if act else 'add'}.{str(odt)[6:]}", err_over_bound=worst)
