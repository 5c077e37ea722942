"""Every GEMM tile per element at its M, N, K and segment edges (the harness of tests/test_ops_elementwise_gpu.py::run_gemm_case:
NaN interior inside a guard band, every element against the fp64 reference under the arithmetic bound (K + 4) U32 mag and its
epilogue extensions, the guards bit for bit).  No tolerance of its own: every bound is opcheck's.

One factor varies at a time around a small base (no cross product; every operand has a few hundred rows at most):
    m      M in {1, 2, 16, bm - 1, bm, bm + 1, 2 bm + 1}: a tile with one live row, a full tile, one row past it - the row predicates of
           every loader and epilogue; every epilogue class the tile serves (an odd M gives the row-broadcast gate ONE half of M rows)
    n      N in {8, bn - 8, bn, bn + 8} (the gated pair: 64 and bn + 64; the head split: 128, 256, 384): the column predicates
    k      1 .. 9 K slices (conv tiles: 1 .. 9 channel chunks per tap): ring prologues and tails at nk < NS and every nk % NS
    split  K ranges at nk in {5, 9}, counted in the units the tile's mainloop divides (K slices; the 32-element chunks of the 256x256
           tiles, two per slice): uneven ranges (the smallest split that does not divide the units), one unit each, three more ranges
           than units (some ranges are empty).  The planner passes an explicit K split through; classify() pins that
    seg    conv k = 3 over B = 3 segments of L in {1, 2, 3, bm - 1, bm, bm + 1} rows, C in {64, 192}: the tap masks at q == 0 and
           q == segV - 1 with a segment boundary before, on and after a tile boundary, segments shorter than a wave tile
    vrows  virtual rows (segV != segS) on every tile (the head-split tiles under their head split), source rows the mapping skips are NaN
    sconv  the DAC encoder's strided conv (rstride > 1), the clips between NaN guard segments
    small  the small-M production plans through the automatic tile, the plan pinned as tests/test_gemm_plan_cpu.py pins it

Before a launch the planner (foley_debug_gemm_plan, no device needed) is asked about every combination; what it refuses is
asserted refused with its message (PLAN_REFUSALS), what the tile's launcher refuses after the plan likewise (LAUNCH_REFUSALS,
asserted on the device: the refusal comes before any kernel is launched).  Nothing is skipped; test_edge_coverage_and_refusals
counts both and asserts that every tile launches every sweep it is eligible for.

MI355X, largest err / bound per sweep (recorded under elementwise.gemm.edge.*): m 0.94, n 0.94, k 0.98, seg 0.93 (all four on a
16-bit head-split or gated output, where half an ulp of the store is most of the bound), vrows 0.96 on the head-split tiles for the
same reason and 0.009 on fp32 stores, split 0.22, small 0.73, sconv 0.007 (fp32 stores: the worst case of K additions is far
from a real sum).  Every case passed; no kernel was changed.
"""
import os
import re

import pytest

import test_ops_elementwise_gpu as ew
from foley_amd.host import runtime as rt
from test_gemm_plan_cpu import plan

gpu = pytest.mark.gpu      # per test: the coverage tests of this file run without a device

# tile id -> (bm, bn): gemm_plan.h kTiles (test_tile_table_matches_the_library reads the rows of the header)
TILE_DIMS = {
    1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (128, 64), 5: (128, 128), 6: (64, 64), 7: (128, 128), 8: (64, 128), 9: (256, 128),
    11: (128, 128), 13: (64, 64), 15: (128, 128), 19: (256, 128), 21: (128, 128), 22: (256, 64), 23: (256, 128), 24: (192, 128),
    25: (128, 128), 26: (96, 128), 27: (64, 128), 28: (192, 128), 29: (256, 128), 31: (256, 256), 32: (256, 256),
}
# K slices a mainloop keeps in flight (bf16 weights), maintained by hand from the launch tables: gemm_impl.h launch_typed (NS), gemm_conv3.hip
# launch_gemm_conv3, gemm_ws_impl.h launch_gemm_ws_t (NS) and launch_ws_conv3_* (NSB), gemm_wide_impl.h (NSB slices of 32).
# test_ring_depths_match_the_launch_tables reads the same numbers out of those sources, so a ring deepened in a kernel fails there
# until this table (and with it the K sweep's range) follows.  None is deeper than 8: the K sweep ends at 9.
RING_DEPTH = {1: 4, 2: 3, 3: 4, 4: 3, 5: 4, 6: 4, 7: 4, 8: 4, 9: 3, 11: 3, 13: 3, 15: 5, 19: 3, 21: 6, 22: 6, 23: 4, 24: 4, 25: 5, 26: 5,
              27: 6, 28: 4, 29: 3, 31: 6, 32: 5}
NK_SWEEP = list(range(1, max(9, max(RING_DEPTH.values()) + 1) + 1))
# the unit a K split divides (K elements): the mainloop's K slice - except the 256x256 tiles, whose BK = 32 mainloop splits K over
# 32-element chunks (gemm_wide_impl.h: nkc = C / BK), two per 64-element slice
SPLIT_UNIT = {31: 32, 32: 32}
CLASSES = ["store", "store_t", "gate", "gate_split", "silugate", "qkv"]
PLAN_EPI = {"store": "store", "store_t": "store_t", "gate": "gate", "gate_split": "gate", "silugate": "silugate", "qkv": "qkv"}
CONV_TILES = sorted(t for t, c in ew.TILE_CASES.items() if c[2])
VROWS = [(10, 8, 112), (7, 8, 16), (3, 40, 41), (5, 1, 3)]      # (segs, segV, segS): the production P = 8 over Ls = 112; M = 56 below every tile
SCONV_TILES16 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]                  # the 16-bit register-staged and direct-to-LDS tiles (0: automatic)
# foley_dac_encode takes waveforms of a multiple of the codec hop only ("waveform length must be a multiple of the codec hop"), so
# every strided conv sees Tin % stride == 0: the smallest Tin is the stride itself (ONE output row per clip: every tap row but
# those of the clip is padding), and no Tin that is not a multiple exists to be tested; 5 x stride is a second multiple.
SCONV_TIN = (1, 5)
# (sweep, tile) -> the message the planner refuses with
_WSCONV_MSG = "GEMM: tiles 21 / 22 / 23 / 24 need a bf16 channels-last conv k=3"
PLAN_REFUSALS = {("vrows", 21): _WSCONV_MSG, ("vrows", 22): _WSCONV_MSG, ("vrows", 23): _WSCONV_MSG, ("vrows", 24): _WSCONV_MSG}
# (sweep, tile) -> the message the tile's launcher refuses with after the planner accepted (gemm_conv3.hip launch_gemm_conv3;
# gemm_wide_impl.h: tile 31 is a conv k = 3 tile, tile 32 requires segV >= M)
_WIDE_MSG = "256x256 GEMM: operand addressing not supported by this tile"
_CONV3_MSG = "conv3: not a k=3 / pad 1 / dilation 1 channels-last conv"
LAUNCH_REFUSALS = {("vrows", 11): _CONV3_MSG, ("vrows", 13): _CONV3_MSG, ("vrows", 31): _WIDE_MSG, ("vrows", 32): _WIDE_MSG}
# launched / refused by the planner / refused by the launcher, as DESIGN.md states them
COUNTS = {"launched": 3004, "plan_refused": 32, "launch_refused": 40}


# ----------------------------------------------------------------------------- the cases (pure arithmetic on the tables: no device)
def _classes(tile):
    return [e for e in CLASSES if e in ew.TILE_CASES[tile][1]]


def _base(tile):
    """The epilogue of the N, K and mapped sweeps: the plain fp32 store, or the head split on the tiles that serve nothing else."""
    return "store" if "store" in ew.TILE_CASES[tile][1] else "qkv"


def _dts(tile, epi):
    """The tile's own dtypes: fp32 where served; fp16 next to bf16 for the base epilogue only."""
    return [d for d in ew.TILE_CASES[tile][0] if d != "f16" or epi == _base(tile)]


def _bk(dt):
    return 32 if dt == "f32" else 64


def _case(sweep, tile, dt, epi, M, N, K, tag, **o):
    c = dict(sweep=sweep, tile=tile, dt=dt, epi=epi, mnk=(M, N, K), name=f"edge.{sweep}.t{tile}.{tag}", **o)
    if ew.TILE_CASES[tile][2] and "conv" not in o and "vrows" not in o:      # a conv tile: ONE segment of M rows (unless the case maps its rows itself)
        c["conv"] = (1, M, K // 3)
    if epi == "qkv":      # B = 1, L = M, a non-zero token offset; N = 384: q, k and V^T of one head, else q alone of N / 128 heads
        c["qkv"] = (1, M, 1, 5, 3) if N == 384 else (1, M, N // 128, 5, 1)
    return c


def _n_of(tile, epi):
    """N of the M sweep: bn + 8, or the smallest legal N above bn (gated pair: a multiple of 64; head split: 384 = q, k and V^T)."""
    bn = TILE_DIMS[tile][1]
    return bn + 64 if epi == "silugate" else (384 if epi == "qkv" else bn + 8)


def _k_of(tile, dt, nk):
    """nk K slices; a conv tile: nk channel chunks per tap."""
    return (3 if ew.TILE_CASES[tile][2] else 1) * _bk(dt) * nk


def _split_units(tile, dt, nk):
    return nk * _bk(dt) // SPLIT_UNIT.get(tile, _bk(dt))


def split_ranges(units, ks):
    """Units per K range as every mainloop cuts them: range s is [units s / ks, units (s + 1) / ks) in integers."""
    return [units * (s + 1) // ks - units * s // ks for s in range(ks)]


def sweep_cases(sweep, tile):
    bm, bn = TILE_DIMS[tile]
    conv = ew.TILE_CASES[tile][2]
    base = _base(tile)
    out = []
    if sweep == "m":      # five K slices (conv tiles: two chunks per tap, six tap slices)
        for epi in _classes(tile):
            for dt in _dts(tile, epi):
                for M in sorted({1, 2, 16, bm - 1, bm, bm + 1, 2 * bm + 1}):
                    out.append(_case("m", tile, dt, epi, M, _n_of(tile, epi), _k_of(tile, dt, 2 if conv else 5), f"M{M}"))
    elif sweep == "n":
        for epi in [e for e in ("store", "gate", "silugate", "qkv") if e in _classes(tile) and (e != "qkv" or base == "qkv")]:
            ns = {"silugate": [64, bn + 64], "qkv": [128, 256, 384]}.get(epi, sorted({8, bn - 8, bn, bn + 8}))
            for dt in _dts(tile, epi):
                for N in ns:
                    out.append(_case("n", tile, dt, epi, bm + 1, N, _k_of(tile, dt, 2 if conv else 5), f"N{N}"))
    elif sweep == "k":
        for dt in _dts(tile, base):
            for nk in NK_SWEEP:
                out.append(_case("k", tile, dt, base, bm + 1, _n_of(tile, base), _k_of(tile, dt, nk), f"nk{nk}"))
    elif sweep == "split":
        if "gate_split" in _classes(tile):
            # deferred slabs exist for 16-bit operands only.  fp32 operands split K through fp32 atomics on x: ks additions, each rounded
            # relative to the running |x|, where gated_residual_bound models the ONE addition x0 + g y (its U32 = two unit round-offs
            # covers the two ranges of the m and seg sweeps; five ranges measured 1.29 of it on tiles 1 / 2 / 5 / 8, in an order that
            # changes from run to run) - that form is no case of this sweep
            for dt in [d for d in _dts(tile, "gate_split") if d != "f32"]:
                for nk in (5, 9):
                    units = _split_units(tile, dt, nk)      # what the tile's mainloop divides: nk slices, 2 nk chunks on the 256x256 tiles
                    uneven = next(k for k in range(2, units) if units % k)      # 2 for 5 and 9 slices; 3 and 4 for the 10 and 18 chunks of the 256x256 tiles
                    for ks in (uneven, units, units + 3):
                        out.append(_case("split", tile, dt, "gate_split", bm + 1, bn + 8, _k_of(tile, dt, nk), f"nk{nk}.ks{ks}", ksplit=ks,
                                         n_slabs=24, units=units))
    elif sweep == "seg":
        if conv:
            for epi in [e for e in ("store", "gate_split", "silugate") if e in _classes(tile)]:
                for dt in _dts(tile, epi):
                    for Cc in (64, 192):
                        for L in sorted({1, 2, 3, bm - 1, bm, bm + 1}):
                            out.append(_case("seg", tile, dt, epi, 3 * L, _n_of(tile, epi), 3 * Cc, f"L{L}.C{Cc}", conv=(3, L, Cc)))
    elif sweep == "vrows":
        for dt in ew.TILE_CASES[tile][0]:      # the plain store; on the head-split tiles, which serve nothing else, the head split (N = 384)
            for segs, segV, segS in VROWS:
                out.append(_case("vrows", tile, dt, base, segs * segV, 136 if base == "store" else 384, 256, f"{segs}x{segV}of{segS}", vrows=(segV, segS)))
    return out


def sconv_cases():
    out = []
    for dt, tiles in (("f32", ew.DAC_TILES), ("bf16", SCONV_TILES16), ("f16", SCONV_TILES16)):
        for tile in tiles:
            for st in (2, 3, 5, 8):
                for mult in SCONV_TIN:
                    Tin = mult * st
                    out.append(dict(sweep="sconv", tile=tile, dt=dt, epi="store", mnk=(3 * mult, 72, 2 * st * 64),
                                    name=f"edge.sconv.t{tile}.s{st}.T{Tin}", sconv=(3, Tin, 64, st)))
    return out


# name -> (epilogue, (M, N, K), options, (tile, K split, panel groups)): the rows of tests/test_gemm_plan_cpu.py CASES of the same names
SMALL_M = {
    **{f"{n}_{M}": v for M, t_cross in ((16, 2), (224, 27)) for n, v in {
        "gelu_fc1": ("gelu", (M, 6144, 1536), {}, (3, 1, 0)), "qkv": ("qkv", (M, 4608, 1536), {"H": 12, "nK": 3}, (27, 1, 0)),
        "cross_q": ("qkv", (M, 1536, 1536), {"H": 12, "nK": 1}, (t_cross, 1, 0)),
        "gate_proj": ("gate_split", (M, 1536, 1536), {}, (25, 6, 0)), "gate_fc2": ("gate_split_f32slabs", (M, 1536, 6144), {}, (25, 8, 0)),
        "store": ("store", (M, 1536, 1536), {}, (3, 1, 0))}.items()},
    "store_1": ("store", (1, 1536, 1536), {}, (3, 1, 0)), "store_2": ("store", (2, 1536, 1536), {}, (3, 1, 0)),
    "store_1_n13824": ("store", (1, 13824, 1536), {}, (25, 1, 0)), "store_2_n13824": ("store", (2, 13824, 1536), {}, (25, 1, 0)),
}
_PLAN_ROW = {"gate_proj_16": "gate_proj_16_h16", "gate_proj_224": "gate_proj_224_h16", "gate_fc2_16": "gate_fc2_16_f32slabs",
             "gate_fc2_224": "gate_fc2_224_f32slabs"}


def plan_of(c):
    """The planner's answer for a case, on descriptors with fake addresses: (tile, K split, panel groups) or the refusal's text."""
    o = dict(dt=c["dt"], epi=PLAN_EPI[c["epi"]], mnk=c["mnk"], tile=c["tile"])
    if c.get("conv"):
        o["conv"] = c["conv"][1]
    if c["epi"] == "gate":
        o["ksplit"] = 1
    if c["epi"] == "gate_split":
        o["ksplit"] = c.get("ksplit", 2)
        if c["dt"] != "f32":
            o.update(slabs="h", cap=c.get("n_slabs", 8))
    if c["epi"] == "qkv":
        o.update(nK=c["qkv"][4], L=c["qkv"][1])
    if c.get("vrows"):
        o["vrows"] = c["vrows"]
    if c.get("sconv"):
        o["sconv"] = (c["sconv"][1], c["sconv"][3])
    p = plan(o)
    return p if isinstance(p, str) else p[:3]


def classify(c):
    """('launch', plan) | ('plan_refused', message) | ('launch_refused', message); an unexpected refusal (or an expected one that
    does not come) is an assertion failure - nothing is skipped."""
    p, key = plan_of(c), (c["sweep"], c["tile"])
    if isinstance(p, str):
        assert key in PLAN_REFUSALS and PLAN_REFUSALS[key] in p, (c["name"], c["dt"], c["epi"], p)
        return "plan_refused", PLAN_REFUSALS[key]
    assert key not in PLAN_REFUSALS, (c["name"], "the planner was expected to refuse", p)
    assert c["tile"] == 0 or p[0] == c["tile"], (c["name"], p)
    # the K split: an explicit one is passed through as given - also where it exceeds the slices there are to divide (nk + 3: the planner
    # neither clamps to nk nor refuses; only the slab count caps it, and the cases bring 24 slabs) - and no other epilogue splits K
    assert p[1] == (c.get("ksplit", 2) if c["epi"] == "gate_split" else 1), (c["name"], "K split", p)
    if key in LAUNCH_REFUSALS:
        return "launch_refused", LAUNCH_REFUSALS[key]
    return "launch", p


SWEEPS = ["m", "n", "k", "split", "seg", "vrows"]


def _eligible(sweep, tile):
    return {"split": "gate_split" in _classes(tile), "seg": ew.TILE_CASES[tile][2]}.get(sweep, True)


# ----------------------------------------------------------------------------- coverage (no device)
def _csrc(name):
    with open(os.path.join(os.path.dirname(rt.__file__), "..", "csrc", name)) as f:
        return f.read()


def _exist():
    """The tile ids the library knows (as test_ops_elementwise_gpu.test_every_tile_has_a_case derives them from the planner)."""
    return {t for t in range(1, 48) if "unknown tile" not in str(plan(dict(epi="gate", mnk=(500, 1536, 1536), tile=t)))}


def test_tile_table_matches_the_library():
    """TILE_DIMS against the rows of kTiles in csrc/gemm_plan.h, and its id set against the planner's: a new tile id fails here (and in
    test_every_tile_has_a_case) until it has edge cases."""
    src = _csrc("gemm_plan.h")
    body = src[src.index("constexpr TileInfo kTiles["):]
    body = body[:body.index("};")]
    rows = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"/\*\s*(\d+)\s*\*/\s*\{\s*(\d+),\s*(\d+),\s*FAM_", body)}
    assert rows == TILE_DIMS, (rows, TILE_DIMS)
    assert set(TILE_DIMS) == _exist() == set(ew.TILE_CASES) == set(RING_DEPTH)
    assert max(RING_DEPTH.values()) <= 8 and NK_SWEEP == list(range(1, 10))
    assert set(CONV_TILES) == {11, 13, 21, 22, 23, 24, 31}


def test_ring_depths_match_the_launch_tables():
    """RING_DEPTH and SPLIT_UNIT against the kernels' sources: the template arguments of the launch tables where a table has one
    line per tile, the NSB expressions verbatim where a launcher computes the depth.  A deeper ring fails here, not silently."""
    got = {}
    impl = _csrc("gemm_impl.h")      # case N: ... launch_tile<T, BM, BN, WM, WN, NS[, true]>
    for m in re.finditer(r"case (\d+):[^\n]*?(?:\n[^\n]*?)?launch_tile<T, \d+, \d+, \d+, \d+, (\d+)", impl):
        got[int(m.group(1))] = int(m.group(2))
    ws = _csrc("gemm_ws_impl.h")
    for m in re.finditer(r"case (\d+): return launch_ws_tile<T, \d+, \d+, \d+, \d+, (\d+), \d+, 0>", ws):      # bf16 weights
        got[int(m.group(1))] = int(m.group(2))
    for m in re.finditer(r"if \(tile == (\d+)\) \{[^}]*?launch_ws_one<T, \d+, \d+, \d+, \d+, (\d+), \d+, EPI_QKV_SPLIT, 0>", ws):
        got[int(m.group(1))] = int(m.group(2))
    c3 = _csrc("gemm_conv3.hip")      # tile 11 / 13 are the launcher's tile == 1 / else branches, NS = 3 in every dtype
    assert set(re.findall(r"launch_c3_epi<\w+, \d+, \d+, \d+, \d+, (\d+)>", c3)) == {"3"}
    got[11] = got[13] = 3
    # tap-fused conv k = 3: 128x128 six weight slices, 256x128 / 192x128 four (bf16 weights); 256x64 (both kernels) six
    assert "constexpr int NSB = BM == 128 ? 6 : (WF ? 6 : 4), NAB = (NSB + 2 + 2) / 3;" in ws
    assert ws.count("constexpr int BM = 256, BN = 64, LW = 4, NSB = 6, NAB = 3;") == 1
    assert ws.count("constexpr int BM = 256, BN = 64, WM = 8, WN = 1, LW = 4, NSB = 6, NAB = 3;") == 1
    got.update({21: 6, 22: 6, 23: 4, 24: 4})
    wide = _csrc("gemm_wide_impl.h")      # slices of BK = 32: conv 6 (fp8 8), plain 5 (fp8 6)
    assert "constexpr int NSB = TAPS == 3 ? (WF ? 8 : 6) : (WF ? 6 : 5);" in wide
    assert "constexpr int BM = 256, BN = 256, BK = 32," in wide and "nkc = C / BK;" in wide
    got.update({31: 6, 32: 5})
    assert got == RING_DEPTH, {t: (got.get(t), RING_DEPTH.get(t)) for t in set(got) | set(RING_DEPTH) if got.get(t) != RING_DEPTH.get(t)}
    assert SPLIT_UNIT == {31: 32, 32: 32}


def test_edge_coverage_and_refusals():
    """Every (tile, dtype, epilogue, shape) of the sweeps through the planner: launched or refused with the expected message,
    counted; every tile launches at least one case of every sweep it is eligible for."""
    n = {"launch": 0, "plan_refused": 0, "launch_refused": 0}
    refused = set()
    for tile in sorted(TILE_DIMS):
        for sweep in SWEEPS:
            cases = sweep_cases(sweep, tile)
            assert bool(cases) == _eligible(sweep, tile), (sweep, tile)
            kinds = [classify(c)[0] for c in cases]
            for k in kinds:
                n[k] += 1
            if sweep != "vrows" and cases:
                assert "launch" in kinds, f"tile {tile} launches no case of the {sweep} sweep"
            if sweep == "vrows" and "launch" not in kinds:
                refused.add(tile)
        for nk in (5, 9):      # the split sweep reaches its three edges in the units the tile's own mainloop divides
            kinds = set()
            for c in sweep_cases("split", tile):
                if c["name"].split(".")[3] == f"nk{nk}":
                    r = split_ranges(c["units"], c["ksplit"])
                    assert sum(r) == c["units"] == c["mnk"][2] // (3 if ew.TILE_CASES[tile][2] else 1) // SPLIT_UNIT.get(tile, 64)
                    kinds |= {"uneven"} if len(set(r)) > 1 and min(r) > 0 else set()
                    kinds |= {"one_each"} if set(r) == {1} else set()
                    kinds |= {"empty"} if min(r) == 0 else set()
            assert kinds == ({"uneven", "one_each", "empty"} if _eligible("split", tile) else set()), (tile, nk, kinds)
    assert refused == {t for s, t in list(PLAN_REFUSALS) + list(LAUNCH_REFUSALS) if s == "vrows"}, refused
    for c in sconv_cases():
        n[classify(c)[0]] += 1
    assert {c["tile"] for c in sconv_cases() if c["dt"] == "f32"} == set(ew.DAC_TILES)
    small = len(SMALL_M) * 2
    print(f"edge sweeps: {n['launch']} launched + {small} small-M, {n['plan_refused']} refused by the planner, {n['launch_refused']} by a launcher")
    assert (n["launch"], n["plan_refused"], n["launch_refused"]) == (COUNTS["launched"], COUNTS["plan_refused"], COUNTS["launch_refused"]), n


def test_small_m_plans_are_the_cpu_table_rows():
    from test_gemm_plan_cpu import CASES
    for name, (epi, mnk, o, want) in SMALL_M.items():
        case, pinned = CASES[_PLAN_ROW.get(name, name)]
        assert case["mnk"] == mnk and pinned[:3] == want, (name, case, pinned)


# ----------------------------------------------------------------------------- the launches
def _run(dev, c):
    kind, what = classify(c)
    kw = {k: c[k] for k in ("conv", "qkv", "ksplit", "n_slabs", "vrows", "sconv") if c.get(k) is not None}
    args = (dev, c["name"], c["epi"], c["mnk"], ew.DTS[c["dt"]])
    if kind == "plan_refused":
        return
    if kind == "launch_refused":      # refused by the tile's launcher before any kernel is launched
        with pytest.raises(rt.FoleyRuntimeError, match=re.escape(what)):
            ew.run_gemm_case(*args, tile=c["tile"], **kw)
        return
    ew.run_gemm_case(*args, tile=c["tile"], want_plan=what if c["tile"] else None, **kw)


def _run_all(dev, cases):
    """Every case runs; the failures of all of them are reported together (a failing case does not hide its neighbours)."""
    bad = []
    for c in cases:
        try:
            _run(dev, c)
        except AssertionError as e:
            bad.append(f"{c['name']} [{c['epi']}, {c['dt']}]: {e}")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad)


def _sweep_params():
    """One test per (sweep, tile, epilogue): a few dozen small launches each."""
    return [pytest.param(s, t, e, id=f"{s}-t{t}-{e}") for s in SWEEPS for t in sorted(TILE_DIMS)
            for e in dict.fromkeys(c["epi"] for c in sweep_cases(s, t))]


@gpu
@pytest.mark.parametrize("sweep,tile,epi", _sweep_params())
def test_gemm_edge_sweep(dev, sweep, tile, epi):
    _run_all(dev, [c for c in sweep_cases(sweep, tile) if c["epi"] == epi])


@gpu
@pytest.mark.parametrize("dt", ew.ALL3)
def test_gemm_strided_conv_elementwise(dev, dt):
    """The strided conv of the DAC encoder (rstride > 1, taps = 2 stride, pad ceil(stride / 2)) against F.conv1d in fp64."""
    _run_all(dev, [c for c in sconv_cases() if c["dt"] == dt])


@gpu
@pytest.mark.parametrize("dt", ew.H16)
@pytest.mark.parametrize("name", list(SMALL_M))
def test_gemm_small_m_production_plans(dev, name, dt):
    """The bs = 1 loop's launches at M = 16 / 224 and the vector GEMMs at M = 1 / 2: the automatic tile must give the pinned plan and
    the whole output is checked."""
    epi, mnk, o, want = SMALL_M[name]
    kw = dict(want_plan=want, seed=300)
    if epi == "qkv":
        kw["qkv"] = (1, mnk[0], o["H"], 0, o["nK"])
    if epi.startswith("gate_split"):
        kw["ksplit"] = 0
    ew.run_gemm_case(dev, f"edge.small.{name}", epi, mnk, ew.DTS[dt], **kw)
