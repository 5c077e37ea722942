"""Which GEMM launches take write-through output stores (GemmPlan::wt_out), without a GPU.

The flag is the fifth word of foley_debug_gemm_plan_ex - foley_debug_gemm_plan's plan (same descriptors, same planner call; its
four words keep their meaning and are asserted equal here) with the fields added since.  Set: the single-clip regime, one round
of at most 256 workgroups on fewer than 1536 rows, 16-bit operands, deferred split-K slabs.  Unset: everything else - the 8-clip
batch (M = 4000), the 30 s clip (M = 3000, which the 256x256 K-range route also fits into one round), the fp32 parity mode,
launches without slabs (the other epilogues' outputs lost their A/B in the loop: DESIGN.md section 4, "Round 8").
"""
import ctypes as C

import pytest

from test_gemm_plan_cpu import _desc, _lib, plan


def plan_ex(case):
    o = dict(case)
    dt, epi = o.pop("dt", "bf16"), o.pop("epi")
    keep = []
    d0 = _desc(dt, epi, *o["mnk"], o, keep)
    d1 = _desc(dt, epi, *o["pair"], dict(o, **o.get("pair_opts", {})), keep) if "pair" in o else None
    out = (C.c_int32 * 8)()
    lib = _lib()
    lib.foley_debug_gemm_plan_ex.argtypes = lib.foley_debug_gemm_plan.argtypes
    lib.foley_debug_gemm_plan_ex.restype = C.c_int
    rc = lib.foley_debug_gemm_plan_ex(C.byref(d0), C.byref(d1) if d1 is not None else None, o.get("krot", 0), out)
    assert rc == 0, lib.foley_last_error().decode()
    return tuple(out)


D, MLP, HC = 1536, 6144, 4096
# id -> (case, flag)
CASES = {
    # bs = 1: the 126 gated-residual launches per iteration (proj / fc2 plain, linear1 / w2 as conv k = 3), bf16 and fp32 slabs
    "proj_500": (dict(epi="gate", mnk=(500, D, D), slabs="h"), 1),
    "fc2_500": (dict(epi="gate", mnk=(500, D, MLP), slabs="h"), 1),
    "fc2_500_f32slabs": (dict(epi="gate", mnk=(500, D, MLP), slabs="f32"), 1),
    "fc2_500_f16": (dict(epi="gate", dt="f16", mnk=(500, D, MLP), slabs="h"), 1),
    "lin1_500_conv": (dict(epi="gate", mnk=(500, D, 3 * D), conv=500, slabs="h"), 1),
    "w2_500_conv": (dict(epi="gate", mnk=(500, D, 3 * HC), conv=500, slabs="h"), 1),
    "proj_pair_500_80": (dict(epi="gate", mnk=(500, D, D), pair=(80, D, D), slabs="h"), 1),
    "fc2_pair_500_80": (dict(epi="gate", mnk=(500, D, MLP), pair=(80, D, MLP), slabs="h"), 1),
    "proj_1": (dict(epi="gate", mnk=(1, D, D), slabs="h"), 1),
    # no slabs / no K split: nothing this flag serves
    "proj_500_no_slabs": (dict(epi="gate", mnk=(500, D, D), ksplit=1), 0),
    "proj_500_one_range": (dict(epi="gate", mnk=(500, D, D), slabs="h", ksplit=1), 0),
    "store_500": (dict(epi="store", mnk=(500, D, D)), 0),
    # the 16-bit output rows and head-split destinations: measured, lost in the loop, not served
    "fc1_500_gelu": (dict(epi="gelu", mnk=(500, MLP, D)), 0),
    "qkv_500": (dict(epi="qkv", mnk=(500, 3 * D, D)), 0),
    "cross_q_500": (dict(epi="qkv", mnk=(500, D, D), nK=1, attn=True), 0),
    "w13_500_conv": (dict(epi="silugate", mnk=(500, 2 * HC, 3 * D), conv=500), 0),
    # bs = 8, 30 s, 20 s: today's stores
    "proj_4000": (dict(epi="gate", mnk=(4000, D, D), slabs="h"), 0),
    "fc2_4000": (dict(epi="gate", mnk=(4000, D, MLP), slabs="h"), 0),
    "w2_4000_conv": (dict(epi="gate", mnk=(4000, D, 3 * HC), conv=500, slabs="h"), 0),
    "proj_3000": (dict(epi="gate", mnk=(3000, D, D), slabs="h"), 0),
    "fc2_3000": (dict(epi="gate", mnk=(3000, D, MLP), slabs="h"), 0),
    "fc2_pair_3000_480": (dict(epi="gate", mnk=(3000, D, MLP), pair=(480, D, MLP), slabs="h"), 0),
    "fc2_2000": (dict(epi="gate", mnk=(2000, D, MLP), slabs="h"), 0),
    "proj_pair_1500_80": (dict(epi="gate", mnk=(1500, D, D), pair=(80, D, D), slabs="h"), 0),      # 1580 rows: the large-M side
    # fp32 parity mode: no K split, no flag
    "proj_500_f32": (dict(epi="gate", dt="f32", mnk=(500, D, D), slabs="f32"), 0),
    "fc2_500_f32": (dict(epi="gate", dt="f32", mnk=(500, D, MLP), slabs="f32"), 0),
}


@pytest.mark.parametrize("cid", list(CASES))
def test_write_through_flag(cid):
    case, want = CASES[cid]
    got = plan_ex(case)
    assert got[:4] == plan(case), (cid, got)      # the four-word entry reports the same plan
    assert got[4] == want, (cid, got)
    assert got[5:] == (0, 0, 0), (cid, got)
    if want:      # one round, and a K split whose slabs the flag is about
        assert got[1] > 1, (cid, got)


def test_flag_is_a_one_round_rule():
    """The same layer on either side of 256 workgroups: an explicit K split that overfills the round loses the flag."""
    base = dict(epi="gate", mnk=(500, D, MLP), slabs="h", cap=16, tile=25)      # 4 x 12 = 48 tiles of 128x128
    assert plan_ex(dict(base, ksplit=5))[4] == 1      # 240 workgroups
    assert plan_ex(dict(base, ksplit=6))[4] == 0      # 288
