"""Every attention form of csrc/attention.hip per element at its query, key and split edges (the harness of
tests/test_ops_elementwise_gpu.py::test_attention_elementwise: the outputs are NaN interiors inside guard bands, EVERY element is
judged by opcheck.attention_ref_and_bound - the fp64 softmax from the operands as rounded, p_dtype the operand type for 16-bit
operands, the output term of the type actually stored - and the guards bit for bit; for 16-bit operands every V^T column at or
beyond Skv holds 1e4, so a pad key that receives any weight fails an element).  No tolerance of its own.

FORMS names what launch_attention can select: attn_kernel<64 / 96 / 128>, attn_bf16_kernel, attn_lds_kernel by where its merge
records lie and by the width of its V^T image, attn_bf16_wide_kernel<64 / 96 / 128>, attn_bf16_long_kernel,
attn_bf16_pair_kernel<4 / 5 / 6>.  The rule is restated in test_ops_elementwise_gpu._attn_form_of (with the launcher's img / mrg /
merge_off arithmetic) and every case asserts the form it was written for.  Of the four attn_lds_kernel variants
{merge_off == 0, != 0} x {lgCV 4, 5} THREE exist: lgCV 4 means a pitch <= 128, hence at most four key tiles, hence
img = 73 728 B and img + mrg = 123 904 B <= 160 KiB - merge_off != 0 always (test_form_census scans the launcher's whole staged
range for it).

One factor varies at a time around a small base per form (no cross product); 16-bit forms run bf16 and fp16, attn_kernel fp32:
    skv     forms without a lower limit: 1, 2, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96 keys (attn_bf16_kernel: waves that own no key
            tile; also 290 keys under a pitch of 320, where it serves ten tiles in its looped form; the wide kernel at 128: also 511);
            attn_lds_kernel 97 .. 256 (four to eight key tiles, five, six and seven among them); long / pair 512 .. 577 (a full last
            64-key tile, one key in its first half, a full first half with an empty second, one key in the second)
    pitch   ceil32(Skv), + 8, ceil64(Skv), the next multiple of 256 - where the form stays selected (long / pair at Skv 513: the
            clamp of the last 16-byte chunk at pitch - 8); a pitch below ceil32(Skv) or off the multiples of 8 is refused, the
            message and every bit of both outputs asserted
    sq      1, 31, 32, 33, QT - 1, QT, QT + 1, 2 QT + 1 queries (QT: queries per workgroup) wherever SOME B x H keeps the form
            selected (SQ_RUN pins the list); pair<NQ>: also one live query in the last workgroup, and a multiple of 32 NQ
    split   0, 1, 31, 32, 33, QT, Sq - 1, Sq: the side that receives no row is a guarded buffer whose bits must not change
    bdiv    kv_bdiv in {1, 2, B}, the shared K / V entries distinct
    out     16-bit operands -> fp32 stores (the FOLEY_ATTN16(T, float) instance of every 16-bit kernel); fp32 operands -> bf16 / fp16
    scores  opcheck.ATTN_SCORE_CLASSES: the maximum rises in every tile (and falls for every third query) / stays in the first tile /
            the last key holds half the weight / a middle tile lies 63 below the maximum
tests/test_opcheck_cpu.py holds the emulation of every form's arithmetic (32- / 64-key tiles, the four key runs, the two key
halves) to 1.0 of the bound on the operands of the scores, out and small-Skv cases: the inputs are fair without a GPU.  That
emulation is also what showed i.i.d. operands to be unfair at 2 .. 33 keys in 16 bits (1.31 of the bound at two keys, see FEW_KEYS):
those cases carry 'onoff' operands.

MI355X, 839 launched + 44 refused, every case inside its bound, no kernel changed; largest err / bound per sweep (recorded under
elementwise.attention.edge.<sweep>.<form>.<type>), bf16 / fp16 / fp32 operands:
    skv 0.79 / 0.66 / 0.008     pitch 0.73 / 0.56     sq 0.78 / 0.62 / 0.006     split 0.76 / 0.53 / 0.005     bdiv 0.79 / 0.62 / 0.006
    out 0.73 / 0.46 (fp32 stores of 16-bit operands), 0.93 (attn_kernel<64> storing bf16: the half ulp of the store is the bound)
    scores 0.82 (pair<5>, rise) / 0.67 / 0.02
The 16-bit maxima sit on attn_bf16_wide_kernel<128>, whose base has the most elements (5.6 M).  The file runs in 22 s, the slowest
test (skv, long kernel) 3.9 s.

Mutants (scratch builds, arithmetic and masks only, never committed; "earlier" = the 93 attention tests from before this file):
    pair kernel key mask < -> <=          every ragged pair case fails (V^T pad 1e4); Skv 512 / 544 / 576 and scores 'first' pass; earlier: fails
    long kernel never rescales            every long case but scores 'first' fails; earlier: the two per-element long cases fail, the norm gates pass
    pair merge with f_b = 0               every pair case fails; earlier: fails
    lds merge reads wave 2's O for wave 3 every lds case of all three variants fails; earlier: the Skv 250 cases fail
    long kernel FIRST-half key mask <=    skv (513, 543, 577) and pitch (Skv 513) fail; earlier: all 93 pass (their long case has 33 keys in the last tile)
    fp32 store packs element 2 twice      the out sweep of all eleven 16-bit forms fails; earlier: all 93 pass
"""
import functools
import re

import pytest
import torch

import opcheck as oc
from foley_amd.host import runtime as rt
from test_ops_elementwise_gpu import DTS, H16, _attn_form_of, _attn_kernel_of, _attn_lds_layout, record_parity

gpu = pytest.mark.gpu      # per test: the census tests of this file run without a device

_LDS = "attn_lds_kernel[merge_off {} 0, lgCV {}]"
LDS_BEHIND4, LDS_BEHIND5, LDS_OVER5, LDS_OVER4 = _LDS.format("!=", 4), _LDS.format("!=", 5), _LDS.format("==", 5), _LDS.format("==", 4)
# form -> (head dim, operand kinds, key tile KT, queries per workgroup QT)
FORMS = {
    "attn_kernel<64>": (64, ["f32"], 32, 32), "attn_kernel<96>": (96, ["f32"], 32, 32), "attn_kernel<128>": (128, ["f32"], 32, 32),
    "attn_bf16_kernel": (128, H16, 32, 32),
    LDS_BEHIND4: (128, H16, 32, 32), LDS_BEHIND5: (128, H16, 32, 32), LDS_OVER5: (128, H16, 32, 32),
    "attn_bf16_wide_kernel<64>": (64, H16, 32, 128), "attn_bf16_wide_kernel<96>": (96, H16, 32, 128), "attn_bf16_wide_kernel<128>": (128, H16, 32, 128),
    "attn_bf16_long_kernel": (128, H16, 64, 128),
    "attn_bf16_pair_kernel<4>": (128, H16, 64, 128), "attn_bf16_pair_kernel<5>": (128, H16, 64, 160), "attn_bf16_pair_kernel<6>": (128, H16, 64, 192),
}
UNREACHABLE = {LDS_OVER4}
FP32, LDS = [f for f in FORMS if f.startswith("attn_kernel")], [LDS_BEHIND4, LDS_BEHIND5, LDS_OVER5]
LONG = ["attn_bf16_long_kernel"] + [f"attn_bf16_pair_kernel<{n}>" for n in (4, 5, 6)]
SWEEPS = ["skv", "pitch", "sq", "split", "bdiv", "out", "scores"]


def c32(n):
    return (n + 31) // 32 * 32


# form -> the base problem (B, H, Sq, Skv) and its V^T pitch as a function of Skv.  Small grids (gw = ceil(Sq / 128) H B < 256) for the
# fp32, register-loaded and staged forms; B H = 128 x two 128-query tiles = 256 workgroups for the wide kernel at head dim 128;
# B H = 64 for long / pair: Sq 385 .. 480 -> pair<4>, 481 .. 512 -> pair<5>, 577 .. 640 -> pair<6>, >= 769 -> long
BASE = {f: dict(B=4, H=2, Sq=70, Skv=77) for f in FP32 + ["attn_bf16_kernel"]}
BASE.update({LDS_BEHIND4: dict(B=4, H=2, Sq=70, Skv=100), LDS_BEHIND5: dict(B=4, H=2, Sq=70, Skv=100), LDS_OVER5: dict(B=4, H=2, Sq=70, Skv=250),
             "attn_bf16_wide_kernel<64>": dict(B=4, H=2, Sq=170, Skv=77), "attn_bf16_wide_kernel<96>": dict(B=4, H=2, Sq=170, Skv=77),
             "attn_bf16_wide_kernel<128>": dict(B=8, H=16, Sq=170, Skv=77),
             "attn_bf16_long_kernel": dict(B=4, H=16, Sq=790, Skv=545), "attn_bf16_pair_kernel<4>": dict(B=4, H=16, Sq=430, Skv=545),
             "attn_bf16_pair_kernel<5>": dict(B=4, H=16, Sq=500, Skv=545), "attn_bf16_pair_kernel<6>": dict(B=4, H=16, Sq=600, Skv=545)})
PITCH_OF = {LDS_BEHIND5: lambda skv: 136}      # 16-byte chunks beyond the 16 of the narrow V^T image, over four key tiles
SKV_FREE = [1, 2, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96]
# The bound's u_p is half the unit round-off of P: an allowance for rows that average over many rounded probabilities.  With i.i.d.
# normal operands the forms' own arithmetic (tests/test_opcheck_cpu.py, P rounded once, nothing else) measures, err / bound: 2 keys
# 1.31 bf16 / 1.14 fp16; 16, 17, 32 keys 1.12, 1.05, 1.02 in bf16 on the 5.6 M elements of the wide kernel's base; 33 keys 0.96.  That
# is the arithmetic, not a kernel, so the 16-bit cases of 2 .. 33 keys carry opcheck's 'onoff' operands instead (same shapes, same
# key counts, the probabilities 1 or e^-12: nothing is lost in their rounding), which that emulation holds to 1.0.
FEW_KEYS = 33
SKV_LONG = [512, 513, 543, 544, 545, 575, 576, 577]
SKV = {**{f: SKV_FREE for f in FP32 + ["attn_bf16_wide_kernel<64>", "attn_bf16_wide_kernel<96>"]},
       "attn_bf16_kernel": SKV_FREE + [290], "attn_bf16_wide_kernel<128>": SKV_FREE + [511],
       LDS_BEHIND4: [97, 127, 128], LDS_BEHIND5: [97, 127, 128], LDS_OVER5: [129, 160, 161, 192, 193, 224, 255, 256],
       **{f: SKV_LONG for f in LONG}}
PITCH_SKV = {LDS_OVER5: 161, **{f: 513 for f in LONG}}      # Skv of the pitch sweep where the base's leaves no room (ceil32 = 256) or no clamp (ceil32 = ceil64)
# form -> the Sq the sq sweep runs, with the (B, H) that keeps the form selected (_find_bh; test_form_census asserts the table)
_SQ32, _SQ128 = [1, 31, 32, 33, 65], [1, 31, 32, 33, 127, 128, 129, 257]
SQ_RUN = {**{f: _SQ32 for f in FORMS if FORMS[f][3] == 32}, **{f: _SQ128 for f in FORMS if "wide" in f}, "attn_bf16_long_kernel": _SQ128,
          # pair<4> is selected only where its workgroup count IS gw = 256 and pair<5>, pair<6> have fewer: from 129 queries on (B H = 128);
          # pair<5>: from 161; pair<6> wins every tie, so it alone runs the small sizes (B H = 256 workgroups of one query block)
          "attn_bf16_pair_kernel<4>": [129, 1024], "attn_bf16_pair_kernel<5>": [161, 960], "attn_bf16_pair_kernel<6>": [1, 31, 32, 33, 191, 192, 193, 385]}
REFUSAL = "attention: V^T pitch must cover Skv rounded up to 32 (multiple of 8)"
COUNTS = {"launched": 839, "refused": 44}


def pitch_of(form, skv):
    return PITCH_OF.get(form, c32)(skv)


def form_of(c):
    hd, kinds, _, _ = FORMS[c["form"]]
    return _attn_form_of(c["B"], c["H"], c["Sq"], c["Skv"], hd, c["kind"] != "f32", c["pitch"])


def _find_bh(form, Sq, Skv, pitch):
    """(B, H) at which `form` is selected: the base's, else the smallest multiple of 16 as B x 16, else the smallest B H of all (H the
    largest of 8, 4, 2, 1 that divides it); None where no B H up to 512 selects it."""
    hd, kinds, _, _ = FORMS[form]
    for B, H in [(BASE[form]["B"], BASE[form]["H"])] + [(bh // 16, 16) for bh in range(16, 513, 16)] + \
            [(bh // next(h for h in (8, 4, 2, 1) if bh % h == 0), next(h for h in (8, 4, 2, 1) if bh % h == 0)) for bh in range(1, 513)]:
        if _attn_form_of(B, H, Sq, Skv, hd, kinds != ["f32"], pitch) == form:
            return B, H
    return None


@functools.lru_cache(maxsize=None)
def sq_runs(form):
    """[(Sq, B, H)] of the sq sweep: the issue's eight sizes, for a pair form also the first k QT + 1 and the first k QT (k <= 8) that
    select it (a last workgroup with ONE live query in one block and its other blocks empty; a last workgroup that is full)."""
    QT, b = FORMS[form][3], BASE[form]
    pitch = pitch_of(form, b["Skv"])
    want = sorted({1, 31, 32, 33, QT - 1, QT, QT + 1, 2 * QT + 1})
    out = [(s,) + _find_bh(form, s, b["Skv"], pitch) for s in want if _find_bh(form, s, b["Skv"], pitch)]
    if "pair" in form:
        for r in (1, 0):
            s = next((k * QT + r for k in range(1, 9) if _find_bh(form, k * QT + r, b["Skv"], pitch)), None)
            if s is not None and s not in [o[0] for o in out]:
                out.append((s,) + _find_bh(form, s, b["Skv"], pitch))
    return out


def _case(sweep, form, kind, tag, **o):
    c = dict(BASE[form], sweep=sweep, form=form, kind=kind, out=kind, ops="rand", div=1, seed=700 + SWEEPS.index(sweep))
    c.update(o)
    c.setdefault("pitch", pitch_of(form, c["Skv"]))
    c.setdefault("split", min(c["Sq"] - 1, 9) if c["Sq"] > 1 else 0)      # a split inside the first query tile unless the case sweeps it
    c["name"] = f"{sweep}.{tag}"
    return c


def sweep_cases(sweep, form):
    hd, kinds, KT, QT = FORMS[form]
    b, out = BASE[form], []
    for kind in kinds:
        if sweep == "skv":
            # 2 .. 33 keys in 16 bits: 'onoff' operands - i.i.d. ones are NOT fair there (FEW_KEYS below)
            out += [_case(sweep, form, kind, f"Skv{s}", Skv=s, ops="onoff" if kind != "f32" and 2 <= s <= FEW_KEYS else "rand") for s in SKV[form]]
        elif sweep == "pitch" and kind != "f32":      # fp32 operands: V is not transposed, there is no pitch
            skv = PITCH_SKV.get(form, b["Skv"])
            for p in dict.fromkeys([c32(skv), c32(skv) + 8, (skv + 63) // 64 * 64, (c32(skv) // 256 + 1) * 256]):
                c = _case(sweep, form, kind, f"Skv{skv}.p{p}", Skv=skv, pitch=p)
                out += [c] if form_of(c) == form else []      # a pitch that selects another form is that form's case, not this one's
        elif sweep == "sq":
            out += [_case(sweep, form, kind, f"Sq{s}.B{B}.H{H}", Sq=s, B=B, H=H) for s, B, H in sq_runs(form)]
        elif sweep == "split":
            out += [_case(sweep, form, kind, f"split{s}", split=s) for s in sorted({0, 1, 31, 32, 33, QT, b["Sq"] - 1, b["Sq"]})]
        elif sweep == "bdiv":
            out += [_case(sweep, form, kind, f"div{d}", div=d) for d in (1, 2, b["B"])]
        elif sweep == "out":
            out += [_case(sweep, form, kind, f"to_{o}", out=o) for o in (["bf16", "f16"] if kind == "f32" else ["f32"])]
        elif sweep == "scores":
            out += [_case(sweep, form, kind, cls, ops=cls) for cls in oc.ATTN_SCORE_CLASSES]
    return out


def refusal_cases():
    """Every 16-bit form's base under a pitch eight short of ceil32(Skv) and under one that is no multiple of 8."""
    out = []
    for form, (hd, kinds, _, _) in FORMS.items():
        for kind in [k for k in kinds if k != "f32"]:
            skv = BASE[form]["Skv"]
            out += [_case("pitch", form, kind, f"refused.p{p}", pitch=p) for p in (c32(skv) - 8, c32(skv) + 4)]
    return out


def _eligible(sweep, form):
    return sweep != "pitch" or FORMS[form][1] != ["f32"]


def operands(c):
    return oc.attn_edge_operands(c["ops"], c["B"], c["H"], c["Sq"], c["Skv"], FORMS[c["form"]][0], c["div"], c["seed"], c["kind"] == "f32")


# ----------------------------------------------------------------------------- census (no device)
def test_form_census():
    """Every selectable form runs every sweep it is eligible for, every case lands on the form it names, the launcher's LDS
    arithmetic leaves exactly three attn_lds_kernel variants, and the two selection flips sit where the sweeps put them."""
    n = 0
    for form in FORMS:
        for sweep in SWEEPS:
            cases = sweep_cases(sweep, form)
            assert bool(cases) == _eligible(sweep, form), (sweep, form)
            for c in cases:
                assert form_of(c) == form, (c["name"], form, form_of(c))
                assert form.startswith(_attn_kernel_of(c["B"], c["H"], c["Sq"], c["Skv"], FORMS[form][0], c["kind"] != "f32", c["pitch"]).split("<")[0])
                assert c["B"] % c["div"] == 0 and 0 <= c["split"] <= c["Sq"] and (c["kind"] == "f32" or (c["pitch"] >= c32(c["Skv"]) and c["pitch"] % 8 == 0))
            n += len(cases)
    # the staged range of launch_attention, exhaustively: four or more key tiles under a pitch of at most 256
    seen = set()
    for skv in range(97, 257):
        for pitch in range(c32(skv), 257, 8):
            f = _attn_form_of(4, 2, 70, skv, 128, True, pitch)
            assert f.startswith("attn_lds_kernel"), (skv, pitch, f)
            img, merge_off, lgcv = _attn_lds_layout(skv, pitch)
            assert (merge_off != 0) == (skv <= 128) and (lgcv == 4) == (pitch == 128) and max(img + 50176 if merge_off else img, 50176) <= 160 * 1024
            seen.add(f)
    assert seen == set(LDS) and not seen & UNREACHABLE
    assert _attn_form_of(4, 2, 70, 96, 128, True, 96) == "attn_bf16_kernel" and _attn_form_of(4, 2, 70, 97, 128, True, 128) == LDS_BEHIND4      # three key tiles | four
    assert _attn_form_of(4, 2, 70, 250, 128, True, 264) == "attn_bf16_kernel"                                                                  # a pitch beyond 256 is not staged
    for f in LONG:      # Skv 511 -> wide, 512 -> long / pair, on each form's own grid
        b = BASE[f]
        assert _attn_form_of(b["B"], b["H"], b["Sq"], 511, 128, True, 512) == "attn_bf16_wide_kernel<128>" and _attn_form_of(b["B"], b["H"], b["Sq"], 512, 128, True, 512) == f
    b = BASE["attn_bf16_wide_kernel<128>"]
    assert _attn_form_of(b["B"], b["H"], b["Sq"], 512, 128, True, 512) in LONG
    # the key edges the sweeps reach
    assert {s % 32 for s in SKV_FREE} >= {0, 1, 31} and {1, 2, 32, 33, 64, 65, 96} <= set(SKV_FREE)      # a full last tile, one key; one, two, three tiles and one key more
    assert {(s + 31) // 32 for f in LDS for s in SKV[f]} == {4, 5, 6, 7, 8}
    assert {s % 64 for s in SKV_LONG} == {0, 1, 31, 32, 33, 63}
    assert all(PITCH_SKV[f] % 64 and c32(PITCH_SKV[f]) < (PITCH_SKV[f] + 63) // 64 * 64 for f in LONG)      # the chunk clamp at pitch - 8 is taken
    assert any(136 <= c["pitch"] <= 256 and c["Skv"] <= 128 for c in sweep_cases("pitch", LDS_BEHIND5))
    assert any(c["pitch"] % 32 for f in FORMS for c in sweep_cases("pitch", f))
    # the fp32-output instance of every 16-bit kernel, the 16-bit stores of the fp32 kernel at every head dim
    o32 = {(c["form"], c["kind"]) for f in FORMS for c in sweep_cases("out", f) if c["out"] == "f32"}
    assert o32 == {(f, k) for f, v in FORMS.items() if v[1] != ["f32"] for k in H16}
    assert {(c["form"], c["out"]) for f in FP32 for c in sweep_cases("out", f)} == {(f, o) for f in FP32 for o in H16}
    # the sq sweep: what the rule lets each form run
    got = {f: [r[0] for r in sq_runs(f)] for f in FORMS}
    assert got == SQ_RUN, got
    for f in [f for f in FORMS if "pair" in f]:
        QT = FORMS[f][3]
        assert {s % QT for s in got[f]} >= {0, 1}, (f, got[f])
    r = refusal_cases()
    assert all(c["pitch"] < c32(c["Skv"]) or c["pitch"] % 8 for c in r)
    print(f"attention edge sweeps: {n} launched, {len(r)} refused")
    assert (n, len(r)) == (COUNTS["launched"], COUNTS["refused"]), (n, len(r))


def test_form_table_matches_the_launcher():
    """FORMS against attention.hip: the kernels it defines, the head dims and NQ it instantiates, the constants of its staging rule."""
    import os
    with open(os.path.join(os.path.dirname(rt.__file__), "..", "csrc", "attention.hip")) as f:
        src = f.read()
    kernels = set(re.findall(r"__global__ [^\n]*? void (attn_\w+)\(", src))
    assert kernels == {"attn_kernel", "attn_bf16_kernel", "attn_lds_kernel", "attn_bf16_wide_kernel", "attn_bf16_long_kernel", "attn_bf16_pair_kernel"}, kernels
    assert {f.split("<")[0].split("[")[0] for f in FORMS} == kernels
    assert set(re.findall(r"FOLEY_LAUNCH\(\(attn_kernel<O, (\d+)>\)", src)) == {"64", "96", "128"}
    assert set(re.findall(r"FOLEY_LAUNCH\(\(attn_bf16_wide_kernel<T, O, (\d+)>\)", src)) == {"64", "96", "128"}
    assert set(re.findall(r"FOLEY_LAUNCH\(\(attn_bf16_pair_kernel<T, O, (\d)>\)", src)) == {"4", "5", "6"}
    assert "mrg = 4 * 3 * 16 * 64 * 4 + 2 * 4 * 32 * 4;" in src and "(128L << ((a.vt_pitch > 128 ? 5 : 4) + 4))" in src
    assert "const int merge_off = staged && img + mrg <= 160 * 1024 ? (int)img : 0;" in src
    assert "staged = !wide && hd == 128 && nt >= 4 && a.vt_pitch <= 256 && img <= 160 * 1024;" in src
    assert REFUSAL in src


# ----------------------------------------------------------------------------- the launches
@functools.lru_cache(maxsize=4)
def _ref_e(ops_key, kind, dev):
    """fp64 reference and bound of one operand set and operand type, once: the cases of a sweep that share their operands (split,
    pitch, out) share it.  Computed by opcheck.attention_ref_and_bound from the operands on `dev` (fp64 matrix products of torch)."""
    q, k, v = oc.attn_edge_operands(*ops_key)
    dt = DTS[kind]
    ref, bound = oc.attention_ref_and_bound(q.to(dev), k.to(dev), v.to(dev), dt, p_dtype=dt if kind != "f32" else None)
    return ref, bound.e


def _ops_key(c):
    return (c["ops"], c["B"], c["H"], c["Sq"], c["Skv"], FORMS[c["form"]][0], c["div"], c["seed"], c["kind"] == "f32")


def _device_operands(c, dev):
    q, k, v = operands(c)
    dt = DTS[c["kind"]]
    if c["kind"] == "f32":
        return q.to(dev), k.to(dev), v.to(dev)
    vd = torch.full(v.shape[:2] + (v.shape[3], c["pitch"]), 1e4, dtype=dt)      # the pad holds LARGE finite values: a pad key with any weight fails an element
    vd[..., :c["Skv"]] = v.transpose(2, 3).to(dt)
    return q.to(dev, dt), k.to(dev, dt), vd.to(dev)


def _run(dev, c):
    """One launch under the checks; returns err / bound."""
    hd = FORMS[c["form"]][0]
    assert form_of(c) == c["form"], (c["name"], form_of(c))
    B, H, Sq, split, odt = c["B"], c["H"], c["Sq"], c["split"], DTS[c["out"]]
    ref, e = _ref_e(_ops_key(c), c["kind"], str(dev))
    q, k, vd = _device_operands(c, dev)
    # a side that receives no row: one NaN row per clip inside its guards, every bit of which must stay
    ga = oc.guarded((B, max(split, 1), H * hd), odt, dev, rows=(1, 1))
    gb = oc.guarded((B, max(Sq - split, 1), H * hd), odt, dev, rows=(1, 1))
    idle = [(g, g.ibuf.clone()) for g, rows in ((ga, split), (gb, Sq - split)) if rows == 0]
    rt.op_attention(q, k, vd, ga.view, gb.view, split, c["div"])
    what = f"attention edge {c['name']} ({c['form']}) {c['kind']} -> {c['out']}"
    r = 0.0
    for g, snap in idle:
        assert torch.equal(g.ibuf, snap), what + ": the output that receives no row was written"
    if split:
        r = max(r, oc.assert_elementwise(ga.view, ref[:, :split], oc.Bound(e[:, :split], odt), what + " outA"))
    if Sq - split:
        r = max(r, oc.assert_elementwise(gb.view, ref[:, split:], oc.Bound(e[:, split:], odt), what + " outB"))
    ga.check(what + " around outA")
    gb.check(what + " around outB")
    return r


def _slug(form):
    return re.sub(r"[^a-z0-9]+", "_", form.replace("!=", "behind").replace("==", "over")).strip("_")


def _params():
    return [pytest.param(s, f, id=f"{s}-{_slug(f)}") for s in SWEEPS for f in FORMS if _eligible(s, f)]


@gpu
@pytest.mark.parametrize("sweep,form", _params())
def test_attention_edge_sweep(dev, sweep, form):
    """Every case of one sweep of one form; the failures of all of them are reported together."""
    bad, worst = [], {}
    for c in sweep_cases(sweep, form):
        try:
            r = _run(dev, c)
            worst[c["kind"]] = max(worst.get(c["kind"], 0.0), r)
            print(f"{c['name']} {c['kind']} -> {c['out']}: err / bound {r:.3f}")
        except AssertionError as e:
            bad.append(f"{c['name']} [{c['kind']} -> {c['out']}]: {e}")
    for kind, r in worst.items():
        record_parity(f"elementwise.attention.edge.{sweep}.{_slug(form)}.{kind}", err_over_bound=r, kernel=form)
    assert not bad, f"{len(bad)} cases of {form} failed:\n" + "\n".join(bad)


@gpu
@pytest.mark.parametrize("form", [f for f in FORMS if FORMS[f][1] != ["f32"]], ids=_slug)
def test_attention_pitch_refusals(dev, form):
    """A V^T pitch that does not cover ceil32(Skv), or is no multiple of 8, is refused with the launcher's message before any kernel
    is launched: both outputs keep every bit."""
    for c in [c for c in refusal_cases() if c["form"] == form]:
        hd, odt = FORMS[form][0], DTS[c["out"]]
        q, k, vd = _device_operands(dict(c, pitch=c32(c["Skv"]) + 8), dev)
        vd = vd[..., :c["pitch"]].contiguous()
        ga = oc.guarded((c["B"], c["split"], c["H"] * hd), odt, dev, rows=(1, 1))
        gb = oc.guarded((c["B"], c["Sq"] - c["split"], c["H"] * hd), odt, dev, rows=(1, 1))
        snap = ga.ibuf.clone(), gb.ibuf.clone()
        with pytest.raises(rt.FoleyRuntimeError, match=re.escape(REFUSAL)):
            rt.op_attention(q, k, vd, ga.view, gb.view, c["split"], 1)
        assert torch.equal(ga.ibuf, snap[0]) and torch.equal(gb.ibuf, snap[1]), (c["name"], "an output was written by a refused launch")
