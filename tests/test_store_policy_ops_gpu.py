"""The write-through output stores (csrc/common.h GStore<ST_WT>) at op level.

One-round launches - the single-clip regime - store two classes of output write-through: the deferred split-K slabs of the
gated-residual GEMMs, and the LayerNorm's x write-back and output rows.  (The 16-bit output rows / head-split destinations of the
GEMM epilogues and the attention output rows were built and measured too; they lost in the loop and are not in the tree, so
there is no such path to test: DESIGN.md section 4, "Round 8".)  The policy changes no value and no address, so every case here
runs the op TWICE through the existing harnesses (tests/test_ops_elementwise_gpu.py, tests/test_pairs_gpu.py): as planned - every
element against the fp64 reference and its bound, every guard band bit for bit - and again with foley_debug_store_policy(1),
which keeps the default stores in every launch; all buffers the two runs wrote must agree bit for bit.  Shapes: the smallest at
which a store path can go wrong - one row, a ragged last tile, M = 500 (several workgroups per panel), ragged K ranges, slab
counts across the LayerNorm's six-slab batch.

The chains at the end replay producer -> consumer launches (slab GEMM -> pending LayerNorm -> q/k/v GEMM -> attention -> conv k=3
GEMM) as a captured graph, eagerly back to back and with a device synchronise between the launches; all outputs start as NaN and
the three runs must agree bit for bit: a line that was never written, or read stale by the next launch, shows.
"""
import contextlib
import ctypes as C

import pytest
import torch

import opcheck as oc
import test_ops_elementwise_gpu as ew
import test_pairs_gpu as tp
from foley_amd.host import runtime as rt, tables

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _lib():
    lib = rt.load_library()
    lib.foley_debug_store_policy.argtypes = [C.c_int]
    lib.foley_debug_store_policy.restype = None
    lib.foley_debug_gemm_plan_ex.argtypes = [C.POINTER(rt.GemmDescC), C.POINTER(rt.GemmDescC), C.c_int, C.POINTER(C.c_int32)]
    lib.foley_debug_gemm_plan_ex.restype = C.c_int
    lib.foley_debug_ln_last_wt.argtypes = []
    lib.foley_debug_ln_last_wt.restype = C.c_int
    return lib


def ln_last_wt():
    """1 when this thread's last LayerNorm launch ran the write-through kernel (ln_mod_wide_wt_kernel), else 0."""
    return _lib().foley_debug_ln_last_wt()


@contextlib.contextmanager
def default_stores():
    lib = _lib()
    lib.foley_debug_store_policy(1)
    try:
        yield
    finally:
        lib.foley_debug_store_policy(0)


def _bits(t):
    return t.detach().contiguous().view(oc._INT[t.element_size()]).cpu().clone()


@contextlib.contextmanager
def recorded():
    """Every guarded buffer the harness allocates (opcheck.guarded) and every GEMM descriptor it launches, in order."""
    made, flags = [], []
    guarded, launch = oc.guarded, ew._launch

    def g(*a, **k):
        r = guarded(*a, **k)
        made.append(r)
        return r

    def l(d):
        out = (C.c_int32 * 8)()
        assert _lib().foley_debug_gemm_plan_ex(C.byref(d), None, 0, out) == 0
        flags.append(out[4])
        return launch(d)

    oc.guarded, ew._launch = g, l
    try:
        yield made, flags
    finally:
        oc.guarded, ew._launch = guarded, launch


def both_policies(run, want_flag=None):
    """run(): launch + full check of the harness.  As planned, then with the default stores; the buffers must agree bit for bit."""
    with recorded() as (made, flags):
        r = run()
    if want_flag is not None:
        assert flags and all(f == want_flag for f in flags), flags
    on = [_bits(g.view) for g in made]
    with default_stores(), recorded() as (made_off, _):
        run()
    off = [_bits(g.view) for g in made_off]
    assert len(on) == len(off) and len(on) >= 1
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), f"buffer {i}: write-through and default stores differ"
    return r


# ----------------------------------------------------------------------------- deferred split-K slabs
# K = 704 = 11 slices: 2 ranges of 6 + 5, 5 ranges of 3 + 2 + 2 + 2 + 2 (uneven either way); K = 640 = 10 slices: even ranges
SLAB_M, SLAB_N = [1, 33, 250, 500], [128, 1536]


@pytest.mark.parametrize("slab", ["gate_split", "gate_split_f32slabs"])
@pytest.mark.parametrize("ks", [2, 5])
@pytest.mark.parametrize("N", SLAB_N)
@pytest.mark.parametrize("M", SLAB_M)
def test_slab_stores(dev, M, N, ks, slab):
    K = 704
    both_policies(lambda: ew.run_gemm_case(dev, f"wt_slab_M{M}_N{N}", slab, (M, N, K), BF16, ksplit=ks, seed=7100 + M), want_flag=1)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("ks", [2, 5])
def test_slab_stores_even_ranges(dev, ks, dt):
    both_policies(lambda: ew.run_gemm_case(dev, "wt_slab_even", "gate_split", (500, 1536, 640), dt, ksplit=ks, seed=7200), want_flag=1)


@pytest.mark.parametrize("ks,C_", [(2, 192), (5, 320), (2, 320)])
@pytest.mark.parametrize("L", [33, 250])
def test_slab_stores_conv3(dev, L, ks, C_):
    """The tap-fused conv k = 3 tiles (w2 / linear1 at one clip): K ranges over the 64-channel chunks of a tap - 3 chunks in 2 ranges
    (2 + 1), 5 in 5 and in 2 (3 + 2)."""
    conv = (2, L, C_)
    both_policies(lambda: ew.run_gemm_case(dev, f"wt_slab_conv_L{L}_C{C_}", "gate_split", (2 * L, 1536, 3 * C_), BF16, conv=conv, ksplit=ks,
                                           seed=7300 + L), want_flag=1)


def _pair_run(dev, case, dt):
    """One pair launch of tests/test_pairs_gpu.py's case under its own reference check; returns every output's bits."""
    pc = tp.PairCase(dev, case, dt)
    assert tp.gemm_krot(False) == 0
    b = pc.buffers()
    if pc.epi == "qkv" and pc.h16:
        pc.vt_pad = b["v"][..., pc.S:].cpu().clone()
    d = pc.descs(b)
    out = (C.c_int32 * 8)()
    assert _lib().foley_debug_gemm_plan_ex(C.byref(d[0]), C.byref(d[1]), 0, out) == 0
    ks = tp.gemm_pair(*d)
    fused = pc.epi == "cross" and d[0]._q.fused()
    pc.check_reference(b, ks, fused, [])
    return out[4], [_bits(t) for t in pc.outputs(b, fused)]


@pytest.mark.parametrize("case", ["gate_5s_h16slabs", "gate_5s_f32slabs", "gate_fc2_5s"])
def test_pair_launch(dev, case):
    """The audio + 80-row visual problem in one launch: bf16 and fp32 slabs, K = 1536 and 6144."""
    flag, on = _pair_run(dev, case, BF16)
    assert flag == 1, case
    with default_stores():
        _, off = _pair_run(dev, case, BF16)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), f"{case} output {i}: write-through and default stores differ"


# ----------------------------------------------------------------------------- LayerNorm (+ pending slabs)
@pytest.mark.parametrize("odt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("k,slab", [(0, None), (1, "h"), (5, "h"), (7, "h"), (5, "f32"), (7, "f32")])
@pytest.mark.parametrize("M", [1, 2, 499, 500])
def test_layernorm_stores(dev, M, k, slab, odt):
    """ln_mod_wide_kernel (D = 1536): the x write-back and the output rows; k = 7 crosses the six-slab batch."""
    D = 1536

    def run():
        s, a = ew._ln_set(dev, M, D, 7400 + k, ew.DTS[odt], k, slab, tok=(k % 2 == 0))
        if k:
            rt.op_ln_mod_pending(a["x"], 1e-6, a["shift"], a["scale"], a["out"], a["partials"], a["k"], a["bias"], a["gate"])
        else:
            rt.op_ln_mod(a["x"], 1e-6, a["shift"], a["scale"], a["out"])
        took.append(ln_last_wt())
        return ew._ln_check(s, a, ew.DTS[odt], f"wt ln M{M} k{k}{slab or ''} {odt}")

    took = []
    both_policies(run)
    assert took == [1, 0], took      # as planned: the write-through kernel; the twin: the default one


@pytest.mark.parametrize("odt", ["bf16", "f32"])
@pytest.mark.parametrize("M0,M1,ks", [(499, 79, (5, 7)), (500, 80, (7, 0)), (0, 81, (0, 5))])
def test_layernorm_pair_stores(dev, M0, M1, ks, odt):
    """The two row sets of a launch; an odd row count leaves the last workgroup's rows without a neighbour (the dead tail)."""
    D = 1536

    def run():
        sets = [ew._ln_set(dev, M, D, 7500 + 10 * i, ew.DTS[odt], ks[i], "h", tok=(i == 0)) for i, M in enumerate((M0, M1))]
        tp.ln_mod_pair([a for _, a in sets], D, 1e-6, rt.dt_of(sets[0][1]["out"]))
        took.append(ln_last_wt())
        return max(ew._ln_check(s, a, ew.DTS[odt], f"wt ln pair {M0}+{M1} set {i} {odt}") for i, (s, a) in enumerate(sets))

    took = []
    both_policies(run)
    assert took == [1, 0], took


@pytest.mark.parametrize("M,want", [(1024, 1), (1025, 0)])
def test_layernorm_flag_is_a_small_grid_rule(dev, M, want):
    """One workgroup per row: 1024 workgroups take the write-through kernel, 1025 keep the default one."""
    s, a = ew._ln_set(dev, M, 1536, 7600, BF16, 2, "h", tok=True)
    rt.op_ln_mod_pending(a["x"], 1e-6, a["shift"], a["scale"], a["out"], a["partials"], a["k"], a["bias"], a["gate"])
    assert ln_last_wt() == want
    ew._ln_check(s, a, BF16, f"wt ln M{M}")


# ----------------------------------------------------------------------------- producer -> consumer chains
D, H = 1536, 12


class Chain:
    """slab GEMM (proj) -> pending LayerNorm -> q/k/v GEMM (head split) -> self attention -> conv k = 3 GEMM (linear1) of one clip."""

    def __init__(self, dev, M):
        g = torch.Generator().manual_seed(9000 + M)
        r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
        self.dev, self.M = dev, M
        self.pitch = (M + 31) // 32 * 32
        self.att0 = r(M, D).to(dev, BF16)
        self.Wp, self.bp = r(D, D, sc=D ** -0.5).to(dev, BF16), r(D, sc=0.1).to(dev)
        self.Wq, self.bq = r(3 * D, D, sc=D ** -0.5).to(dev, BF16), r(3 * D, sc=0.1).to(dev)
        self.Wl = r(D, 3 * D, sc=(3 * D) ** -0.5).to(dev, BF16)
        self.x0 = r(M, D).to(dev)
        self.vec = r(3, D, sc=0.3).to(dev)
        self.gains = [(1 + 0.1 * r(128)).to(dev) for _ in range(2)]
        self.pos = torch.arange(M, dtype=torch.int32, device=dev)
        cos, sin = tables.rope_table(M + 1)
        self.cos, self.sin = cos.to(dev), sin.to(dev)

    def fresh(self):
        dev, M, nan = self.dev, self.M, float("nan")
        f = lambda shape, dt: torch.full(shape, nan, device=dev, dtype=dt)
        b = dict(x=self.x0.clone(), slabs=f((8, M, D), BF16), xn=f((M, D), BF16), q=f((1, H, M, 128), BF16), k=f((1, H, M, 128), BF16),
                 vt=torch.ones((1, H, 128, self.pitch), device=dev, dtype=BF16), att=f((M, D), BF16), x2=self.x0.clone(), slabs2=f((8, M, D), BF16))
        b["vt"][..., :M] = nan
        return b

    def launch(self, b, between=lambda: None):
        M = self.M
        gate = rt.rowbcast(self.vec[2], 0)
        ks = rt.op_gemm(self.att0, self.Wp, None, epilogue=rt.EPI_GATE_RES, out0=b["x"], rb=gate, partials=b["slabs"])
        between()
        rt.op_ln_mod_pending(b["x"], 1e-6, rt.rowbcast(self.vec[0], 0), rt.rowbcast(self.vec[1], 0), b["xn"], b["slabs"], ks, self.bp, gate)
        between()
        desc = rt.qkv_split_desc(M, H, [self.gains[0], self.gains[1], None], [self.pos, self.pos, None], [b["q"], b["k"], b["vt"]], M, 0, 1e-6,
                                 self.cos, self.sin, vt_pitch=self.pitch)
        rt.op_gemm(b["xn"], self.Wq, self.bq, epilogue=rt.EPI_QKV_SPLIT, qkv=desc)
        between()
        split = 40
        rt.op_attention(b["q"], b["k"], b["vt"], b["att"][:split].view(1, split, D), b["att"][split:].view(1, M - split, D), split, 1)
        between()
        ks2 = rt.op_gemm(b["att"], self.Wl, None, epilogue=rt.EPI_GATE_RES, out0=b["x2"], rb=gate, partials=b["slabs2"], conv=(M, D, 3, 1))
        return ks, ks2


@pytest.mark.parametrize("M", [250, 500])
def test_chain_three_ways(dev, M):
    ch = Chain(dev, M)
    ch.launch(ch.fresh())      # warm-up: code objects loaded, LDS limits raised - nothing of that inside the capture
    torch.cuda.synchronize()
    runs = {}
    b = ch.fresh()
    ks = ch.launch(b)
    torch.cuda.synchronize()
    runs["eager"] = b
    b = ch.fresh()
    assert ch.launch(b, between=torch.cuda.synchronize) == ks
    torch.cuda.synchronize()
    runs["synchronised"] = b
    b = ch.fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # (the ops launch on torch's current stream: the capture stream inside this block)
        assert ch.launch(b) == ks
    torch.cuda.synchronize()
    assert bool(torch.isnan(b["xn"]).all()), "the capture ran the launches"
    graph.replay()
    torch.cuda.synchronize()
    runs["graph"] = b
    assert ks[0] > 1 and ks[1] > 1, ks      # both gated-residual launches left slabs (the write-through class with the largest footprint)
    e = runs["eager"]
    for name in ("x", "xn", "q", "k", "att"):
        assert bool(torch.isfinite(e[name]).all()), f"{name}: elements never written (or computed from stale lines)"
    assert bool(torch.isfinite(e["vt"][..., :M]).all()) and bool((e["vt"][..., M:] == 1).all())
    assert bool(torch.isfinite(e["slabs"][:ks[0]]).all()) and bool(torch.isnan(e["slabs"][ks[0]:]).all())
    assert bool(torch.isfinite(e["slabs2"][:ks[1]]).all()) and bool(torch.isnan(e["slabs2"][ks[1]:]).all())
    assert torch.equal(e["x2"], ch.x0), "a deferred split-K launch touched its residual"
    for way in ("synchronised", "graph"):
        for name, t in runs[way].items():
            assert torch.equal(_bits(t), _bits(e[name])), f"{name}: the {way} run differs from the eager one"
    with default_stores():      # and the same chain on the default stores
        b = ch.fresh()
        assert ch.launch(b) == ks
        torch.cuda.synchronize()
    for name, t in b.items():
        assert torch.equal(_bits(t), _bits(e[name])), f"{name}: write-through and default stores differ"
