"""GEMM tile planning without a GPU: the launcher's decisions (tile, K split, panel groups, K-origin rotation) for a table of
shapes, through the test-only entry foley_debug_gemm_plan (not in include/foley_hip.h, typed here with ctypes).

The entry builds GemmArgs from the descriptors exactly as foley_op_gemm / foley_debug_gemm_pair do and stops before the
dispatch; nothing touches the device, so the operand addresses below are fake (16-byte aligned unless a case says otherwise).
Every tile rule of launch_typed (csrc/gemm_impl.h) has a shape on each side of its threshold here, most of them the shapes its
measurement comments quote.  An expected value is either (tile, ksplit, n_groups, k_rot) or the substring of the error.
"""
import ctypes as C

import pytest

from foley_amd.host import runtime as rt

DT = {"f32": 0, "bf16": 1, "f16": 5}
EPI = {"store": 0, "store_t": 1, "silu": 2, "gelu": 3, "silugate": 4, "gate": 5, "dac": 6, "qkv": 7}


def _lib():
    lib = rt.load_library()
    lib.foley_debug_gemm_plan.argtypes = [C.POINTER(rt.GemmDescC), C.POINTER(rt.GemmDescC), C.c_int, C.POINTER(C.c_int32)]
    lib.foley_debug_gemm_plan.restype = C.c_int
    return lib


def _desc(dt, epi, M, N, K, o, keep):
    """Descriptor of one problem with fake device addresses (o: per-case options, see CASES)."""
    addr = iter(range(1 << 40, 1 << 41, 1 << 32))
    d = rt.GemmDescC()
    d.A, d.W, d.bias = next(addr), next(addr), next(addr)
    d.M, d.N, d.K = M, N, K
    if o.get("conv"):   # channels-last conv k=3 'same' over segments of o["conv"] rows
        d.taps, d.tapC, d.dil, d.tap0, d.lda = 3, K // 3, 1, -1, o.get("lda", K // 3)
        d.segV = d.segS = o["conv"]
    elif o.get("sconv"):   # strided conv k = 2 x stride over clips of Tin rows (runtime.gemm_desc sconv=): M = clips x (Tin // stride)
        Tin, st = o["sconv"]
        d.taps, d.tapC, d.dil, d.tap0, d.lda = 2 * st, K // (2 * st), 1, -((st + 1) // 2), K // (2 * st)
        d.segV, d.segS, d.rstride = Tin // st, Tin, st
    else:
        d.taps, d.tapC, d.dil, d.tap0, d.lda = 1, K, 1, 0, o.get("lda", K)
        d.segV = d.segS = M
    if o.get("vrows"):   # virtual rows: product row r reads source row (r // segV) x segS + r % segV
        d.segV, d.segS = o["vrows"]
    if o.get("misaligned_A"):
        d.A += 8
    d.out0 = next(addr) + (8 if o.get("scalar_out") else 0)
    d.osegV, d.out_row, d.out_seg = M, N, M * N
    if epi == "gate":
        d.rb.p, d.rb.ld, d.rb.mode = next(addr), N, 0
    d.dtype, d.epilogue, d.tile, d.ksplit = DT[dt], EPI[epi], o.get("tile", 0), o.get("ksplit", 0)
    if o.get("slabs"):
        d.partials, d.partial_slabs = next(addr), o.get("cap", 8)
        d.partial_dtype = DT[dt] if o["slabs"] == "h" else 0
    d.ldw, d.wfmt = o.get("ldw", 0), o.get("wfmt", 0)
    if epi == "qkv":
        nK = o.get("nK", 3)
        q = rt.QkvSplitDescC()
        q.L, q.nK = o.get("L", M), nK
        q.H = N // (nK * 128)
        for i in range(nK):
            q.dst[i] = next(addr)
        q.out_dtype, q.S_tot, q.eps = DT[dt], q.L, 1e-6
        if o.get("attn"):   # cross attention to <= 96 cached text keys in the epilogue
            q.attn_k, q.attn_vt, q.attn_out = next(addr), next(addr), next(addr)
            q.attn_skv, q.attn_pitch, q.attn_bdiv = 77, 96, 1
        keep.append(q)
        d.qkv = C.pointer(q)
    return d


def plan(case):
    """(tile, ksplit, n_groups, k_rot) the launcher picks for a case, or the error message."""
    o = dict(case)
    dt, epi = o.pop("dt", "bf16"), o.pop("epi")
    keep = []
    d0 = _desc(dt, epi, *o["mnk"], o, keep)
    d1 = None
    if "pair" in o:
        o1 = dict(o, **o.get("pair_opts", {}))
        d1 = _desc(dt, epi, *o["pair"], o1, keep)
    out = (C.c_int32 * 4)()
    lib = _lib()
    rc = lib.foley_debug_gemm_plan(C.byref(d0), C.byref(d1) if d1 is not None else None, o.get("krot", 0), out)
    if rc != 0:
        return lib.foley_last_error().decode()
    return tuple(out)


# id -> (case, expected).  mnk = (M, N, K) of the (first) problem; pair = (M, N, K) of the second problem of a two-problem
# launch (same options, overridden by pair_opts); conv = segment rows of a channels-last conv k=3 (K = 3 x channels);
# slabs = deferred split-K partials ("h": operand dtype, "f32") with cap slabs (default 8); krot = the caller's K-rotation
# opt-in; scalar_out = an output address that rules out the vector epilogue; lda / ldw = row pitches in elements.
# D = 1536 (mlp 6144, conv hidden 4096); M = 500 / 2000 / 3000 / 4000 = 5 s x 1 / 20 s / 30 s / 5 s x 8 clips of audio tokens.
CASES = {
    'store_1': (dict(epi='store', mnk=(1, 1536, 1536)), (3, 1, 0, 0)),
    'store_2': (dict(epi='store', mnk=(2, 1536, 1536)), (3, 1, 0, 0)),
    'store_1_n13824': (dict(epi='store', mnk=(1, 13824, 1536)), (25, 1, 0, 0)),
    'store_2_n13824': (dict(epi='store', mnk=(2, 13824, 1536)), (25, 1, 0, 0)),
    'gelu_fc1_16': (dict(epi='gelu', mnk=(16, 6144, 1536)), (3, 1, 0, 0)),
    'qkv_16': (dict(epi='qkv', mnk=(16, 4608, 1536)), (27, 1, 0, 0)),
    'cross_q_16': (dict(epi='qkv', mnk=(16, 1536, 1536), nK=1), (2, 1, 0, 0)),
    'gate_proj_16_h16': (dict(epi='gate', mnk=(16, 1536, 1536), slabs='h'), (25, 6, 0, 0)),
    'gate_fc2_16_f32slabs': (dict(epi='gate', mnk=(16, 1536, 6144), slabs='f32'), (25, 8, 0, 0)),
    'store_16': (dict(epi='store', mnk=(16, 1536, 1536)), (3, 1, 0, 0)),
    'gelu_fc1_224': (dict(epi='gelu', mnk=(224, 6144, 1536)), (3, 1, 0, 0)),
    'qkv_224': (dict(epi='qkv', mnk=(224, 4608, 1536)), (27, 1, 0, 0)),
    'cross_q_224': (dict(epi='qkv', mnk=(224, 1536, 1536), nK=1), (27, 1, 0, 0)),
    'gate_proj_224_h16': (dict(epi='gate', mnk=(224, 1536, 1536), slabs='h'), (25, 6, 0, 0)),
    'gate_fc2_224_f32slabs': (dict(epi='gate', mnk=(224, 1536, 6144), slabs='f32'), (25, 8, 0, 0)),
    'store_224': (dict(epi='store', mnk=(224, 1536, 1536)), (3, 1, 0, 0)),
    'gelu_fc1_500': (dict(epi='gelu', mnk=(500, 6144, 1536)), (25, 1, 0, 0)),
    'qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536)), (26, 1, 0, 0)),
    'cross_q_500': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1), (27, 1, 0, 0)),
    'gate_proj_500_h16': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h'), (25, 5, 0, 0)),
    'gate_fc2_500_f32slabs': (dict(epi='gate', mnk=(500, 1536, 6144), slabs='f32'), (25, 5, 0, 0)),
    'store_500': (dict(epi='store', mnk=(500, 1536, 1536)), (3, 1, 0, 0)),
    'gelu_fc1_1000': (dict(epi='gelu', mnk=(1000, 6144, 1536)), (29, 1, 0, 0)),
    'qkv_1000': (dict(epi='qkv', mnk=(1000, 4608, 1536)), (25, 1, 0, 0)),
    'cross_q_1000': (dict(epi='qkv', mnk=(1000, 1536, 1536), nK=1), (27, 1, 0, 0)),
    'gate_proj_1000_h16': (dict(epi='gate', mnk=(1000, 1536, 1536), slabs='h'), (25, 2, 0, 0)),
    'gate_fc2_1000_f32slabs': (dict(epi='gate', mnk=(1000, 1536, 6144), slabs='f32'), (25, 2, 0, 0)),
    'store_1000': (dict(epi='store', mnk=(1000, 1536, 1536)), (3, 1, 0, 0)),
    'gelu_fc1_2000': (dict(epi='gelu', mnk=(2000, 6144, 1536)), (32, 1, 0, 0)),
    'qkv_2000': (dict(epi='qkv', mnk=(2000, 4608, 1536)), (28, 1, 6, 0)),
    'cross_q_2000': (dict(epi='qkv', mnk=(2000, 1536, 1536), nK=1), (26, 1, 0, 0)),
    'gate_proj_2000_h16': (dict(epi='gate', mnk=(2000, 1536, 1536), slabs='h'), (32, 5, 0, 0)),
    'gate_fc2_2000_f32slabs': (dict(epi='gate', mnk=(2000, 1536, 6144), slabs='f32'), (32, 5, 0, 0)),
    'store_2000': (dict(epi='store', mnk=(2000, 1536, 1536)), (25, 1, 0, 0)),
    'gelu_fc1_3000': (dict(epi='gelu', mnk=(3000, 6144, 1536)), (29, 1, 6, 0)),
    'qkv_3000': (dict(epi='qkv', mnk=(3000, 4608, 1536)), (32, 1, 0, 0)),
    'cross_q_3000': (dict(epi='qkv', mnk=(3000, 1536, 1536), nK=1), (25, 1, 2, 0)),
    'gate_proj_3000_h16': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h'), (32, 3, 0, 0)),
    'gate_fc2_3000_f32slabs': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='f32'), (32, 3, 0, 0)),
    'store_3000': (dict(epi='store', mnk=(3000, 1536, 1536)), (3, 1, 0, 0)),
    'gelu_fc1_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536)), (29, 1, 6, 0)),
    'qkv_4000': (dict(epi='qkv', mnk=(4000, 4608, 1536)), (28, 1, 6, 0)),
    'cross_q_4000': (dict(epi='qkv', mnk=(4000, 1536, 1536), nK=1), (28, 1, 0, 0)),
    'gate_proj_4000_h16': (dict(epi='gate', mnk=(4000, 1536, 1536), slabs='h'), (19, 1, 0, 0)),
    'gate_fc2_4000_f32slabs': (dict(epi='gate', mnk=(4000, 1536, 6144), slabs='f32'), (19, 1, 0, 0)),
    'store_4000': (dict(epi='store', mnk=(4000, 1536, 1536)), (29, 1, 0, 0)),
    'gate_proj_1536_atomic': (dict(epi='gate', mnk=(1536, 1536, 1536)), (15, 2, 2, 0)),
    'gate_proj_500_atomic': (dict(epi='gate', mnk=(500, 1536, 1536)), (3, 2, 0, 0)),
    'gate_proj_500_ks1': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', ksplit=1), (3, 1, 0, 0)),
    'gate_proj_500_ks3': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='f32', ksplit=3), (25, 3, 0, 0)),
    'gate_proj_500_cap2': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', cap=2), (25, 2, 0, 0)),
    'gate_proj_4000_atomic': (dict(epi='gate', mnk=(4000, 1536, 1536)), (19, 1, 0, 0)),
    'gate_fc2_1500_h16': (dict(epi='gate', mnk=(1500, 1536, 6144), slabs='h'), (25, 1, 0, 0)),
    'gate_fc2_1536_h16': (dict(epi='gate', mnk=(1536, 1536, 6144), slabs='h'), (32, 7, 0, 0)),
    'gate_fc2_3000_scalar': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='h', scalar_out=1), (32, 3, 0, 0)),
    'gelu_fc1_4000_scalar': (dict(epi='gelu', mnk=(4000, 6144, 1536), scalar_out=1), (19, 1, 6, 0)),
    'gelu_fc1_500_scalar': (dict(epi='gelu', mnk=(500, 6144, 1536), scalar_out=1), (15, 1, 0, 0)),
    'qkv_500_scalar': (dict(epi='qkv', mnk=(500, 4608, 1536), scalar_out=1), (26, 1, 0, 0)),
    'cross_q_500_attn': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, attn=1), (27, 1, 0, 0)),
    'cross_q_4000_attn': (dict(epi='qkv', mnk=(4000, 1536, 1536), nK=1, attn=1), (28, 1, 0, 0)),
    'qkv_3840': (dict(epi='qkv', mnk=(3840, 4608, 1536)), (28, 1, 6, 0)),
    'qkv_512': (dict(epi='qkv', mnk=(512, 4608, 1536)), (25, 1, 0, 0)),
    'qkv_560': (dict(epi='qkv', mnk=(560, 4608, 1536)), (26, 1, 0, 0)),
    'mod_panel_224': (dict(epi='store', mnk=(224, 331776, 1536)), (32, 1, 0, 0)),
    'mod_panel_120': (dict(epi='store', mnk=(120, 331776, 1536)), (25, 1, 0, 0)),
    'mod_panel_16': (dict(epi='store', mnk=(16, 331776, 1536)), (25, 1, 0, 0)),
    'mod_panel_224_k4096_w2g': (dict(epi='store', mnk=(224, 331776, 4096)), (1, 1, 0, 0)),
    'vit_fc1_22000': (dict(epi='gelu', mnk=(22000, 3072, 768)), (29, 1, 3, 0)),
    'vit_fc1_22000_k2048': (dict(epi='gelu', mnk=(22000, 3072, 2048)), (32, 1, 2, 0)),
    'vit_fc2_22000': (dict(epi='store_t', mnk=(22000, 768, 3072)), (29, 1, 1, 0)),
    'embed_silu_2': (dict(epi='silu', mnk=(2, 1536, 256)), (3, 1, 0, 0)),
    'embed_store_t_154': (dict(epi='store_t', mnk=(154, 1536, 768)), (3, 1, 0, 0)),
    'narrow_n64_4000': (dict(epi='store', mnk=(4000, 64, 1536)), (3, 1, 0, 0)),
    'narrow_n64_500': (dict(epi='store', mnk=(500, 64, 1536)), (3, 1, 0, 0)),
    'narrow_n64_silugate': (dict(epi='silugate', mnk=(4000, 64, 1536)), (25, 1, 0, 0)),
    'silugate_plain_500': (dict(epi='silugate', mnk=(500, 8192, 1536)), (25, 1, 0, 0)),
    'silugate_plain_2000': (dict(epi='silugate', mnk=(2000, 8192, 1536)), (29, 1, 8, 0)),
    'gelu_1200_n1024': (dict(epi='gelu', mnk=(1200, 1024, 1536)), (3, 1, 0, 0)),
    'conv_w13_250': (dict(epi='silugate', mnk=(250, 8192, 4608), conv=250), (21, 1, 0, 0)),
    'conv_w2_250_h16': (dict(epi='gate', mnk=(250, 1536, 12288), conv=250, slabs='h'), (21, 8, 0, 0)),
    'conv_lin_250_store': (dict(epi='store', mnk=(250, 1536, 4608), conv=250), (21, 1, 0, 0)),
    'conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500), (22, 1, 0, 0)),
    'conv_w2_500_h16': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h'), (22, 5, 0, 0)),
    'conv_lin_500_store': (dict(epi='store', mnk=(500, 1536, 4608), conv=500), (21, 1, 0, 0)),
    'conv_w13_1000': (dict(epi='silugate', mnk=(1000, 8192, 4608), conv=1000), (23, 1, 0, 0)),
    'conv_w2_1000_h16': (dict(epi='gate', mnk=(1000, 1536, 12288), conv=1000, slabs='h'), (22, 2, 0, 0)),
    'conv_lin_1000_store': (dict(epi='store', mnk=(1000, 1536, 4608), conv=1000), (21, 1, 0, 0)),
    'conv_w13_2000': (dict(epi='silugate', mnk=(2000, 8192, 4608), conv=2000), (31, 1, 0, 0)),
    'conv_w2_2000_h16': (dict(epi='gate', mnk=(2000, 1536, 12288), conv=2000, slabs='h'), (31, 5, 0, 0)),
    'conv_lin_2000_store': (dict(epi='store', mnk=(2000, 1536, 4608), conv=2000), (21, 1, 0, 0)),
    'conv_w13_3000': (dict(epi='silugate', mnk=(3000, 8192, 4608), conv=3000), (23, 1, 8, 0)),
    'conv_w2_3000_h16': (dict(epi='gate', mnk=(3000, 1536, 12288), conv=3000, slabs='h'), (31, 3, 0, 0)),
    'conv_lin_3000_store': (dict(epi='store', mnk=(3000, 1536, 4608), conv=3000), (21, 1, 2, 0)),
    'conv_w13_4000': (dict(epi='silugate', mnk=(4000, 8192, 4608), conv=4000), (31, 1, 6, 0)),
    'conv_w2_4000_h16': (dict(epi='gate', mnk=(4000, 1536, 12288), conv=4000, slabs='h'), (24, 1, 0, 0)),
    'conv_lin_4000_store': (dict(epi='store', mnk=(4000, 1536, 4608), conv=4000), (24, 1, 0, 0)),
    'conv_w2_500_atomic': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500), (21, 4, 0, 0)),
    'conv_w2_4000_atomic': (dict(epi='gate', mnk=(4000, 1536, 12288), conv=4000), (24, 1, 0, 0)),
    'conv_w2_500_2clips': (dict(epi='gate', mnk=(1000, 1536, 12288), conv=500, slabs='h'), (22, 2, 0, 0)),
    'conv_w2_500_lda': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', lda=4160), (22, 5, 0, 0)),
    'conv_w13_4000_fp8': (dict(epi='silugate', mnk=(4000, 8192, 4608), conv=4000, wfmt=1), (31, 1, 6, 0)),
    'conv_w2_4000_fp8': (dict(epi='gate', mnk=(4000, 1536, 12288), conv=4000, slabs='h', wfmt=1), (23, 1, 0, 0)),
    'conv_w2_500_fp8': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', wfmt=1), (21, 5, 0, 0)),
    'conv_w2_3000_fp8': (dict(epi='gate', mnk=(3000, 1536, 12288), conv=3000, slabs='h', wfmt=2), (31, 3, 0, 0)),
    'conv_gelu_500': (dict(epi='gelu', mnk=(500, 1536, 4608), conv=500), (3, 1, 0, 0)),
    'conv_w2_f32_500': (dict(dt='f32', epi='gate', mnk=(500, 1536, 12288), conv=500), (13, 1, 0, 0)),
    'conv_w2_f32_4000': (dict(dt='f32', epi='gate', mnk=(4000, 1536, 12288), conv=4000), (11, 1, 0, 0)),
    'conv_w13_f32_500': (dict(dt='f32', epi='silugate', mnk=(500, 8192, 4608), conv=500), (11, 1, 0, 0)),
    'conv_lin_f32_100': (dict(dt='f32', epi='store', mnk=(100, 1536, 4608), conv=100), (13, 1, 0, 0)),
    'conv_w2_f16_3000': (dict(dt='f16', epi='gate', mnk=(3000, 1536, 12288), conv=3000, slabs='h'), (31, 3, 0, 0)),
    'fp8_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), wfmt=1), (15, 1, 0, 0)),
    'fp8_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), wfmt=1), (15, 1, 0, 0)),
    'fp8_gate_500': (dict(epi='gate', mnk=(500, 1536, 6144), slabs='h', wfmt=2), (15, 5, 0, 0)),
    'fp8_gelu_3000': (dict(epi='gelu', mnk=(3000, 6144, 1536), wfmt=1), (19, 1, 6, 0)),
    'fp8_qkv_3000': (dict(epi='qkv', mnk=(3000, 4608, 1536), wfmt=1), (32, 1, 0, 0)),
    'fp8_gate_3000': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='h', wfmt=2), (32, 3, 0, 0)),
    'fp8_gelu_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536), wfmt=1), (19, 1, 6, 0)),
    'fp8_qkv_4000': (dict(epi='qkv', mnk=(4000, 4608, 1536), wfmt=1), (19, 1, 5, 0)),
    'fp8_gate_4000': (dict(epi='gate', mnk=(4000, 1536, 6144), slabs='h', wfmt=2), (19, 1, 0, 0)),
    'fp8_mod_panel_224': (dict(epi='store', mnk=(224, 331776, 1536), wfmt=1), (32, 1, 0, 0)),
    'fp8_cross_500': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, attn=1, wfmt=1), (15, 1, 0, 0)),
    'fp8_silu_2': (dict(epi='silu', mnk=(2, 1536, 256), wfmt=1), (15, 1, 0, 0)),
    'f16_gelu_4000': (dict(dt='f16', epi='gelu', mnk=(4000, 6144, 1536)), (29, 1, 6, 0)),
    'f16_qkv_500': (dict(dt='f16', epi='qkv', mnk=(500, 4608, 1536)), (26, 1, 0, 0)),
    'f16_gate_3000': (dict(dt='f16', epi='gate', mnk=(3000, 1536, 6144), slabs='h'), (32, 3, 0, 0)),
    'f16_qkv_3000': (dict(dt='f16', epi='qkv', mnk=(3000, 4608, 1536)), (32, 1, 0, 0)),
    'f32_dac1_2000': (dict(dt='f32', epi='store', mnk=(2000, 1024, 7168)), (8, 1, 0, 0)),
    'f32_dac1_2000_k512': (dict(dt='f32', epi='store', mnk=(2000, 1024, 512)), (5, 1, 0, 0)),
    'f32_dac1_1000': (dict(dt='f32', epi='store', mnk=(1000, 1024, 7168)), (3, 1, 0, 0)),
    'f32_dac1_3000': (dict(dt='f32', epi='store', mnk=(3000, 1024, 7168)), (5, 1, 0, 0)),
    'f32_dac_epi_2000': (dict(dt='f32', epi='dac', mnk=(2000, 1024, 7168)), (8, 1, 0, 0)),
    'f32_gelu_500': (dict(dt='f32', epi='gelu', mnk=(500, 6144, 1536)), (5, 1, 0, 0)),
    'f32_gelu_4000': (dict(dt='f32', epi='gelu', mnk=(4000, 6144, 1536)), (5, 1, 0, 0)),
    'f32_qkv_500': (dict(dt='f32', epi='qkv', mnk=(500, 4608, 1536)), (8, 1, 0, 0)),
    'f32_qkv_4000': (dict(dt='f32', epi='qkv', mnk=(4000, 4608, 1536)), (5, 1, 0, 0)),
    'f32_gate_500': (dict(dt='f32', epi='gate', mnk=(500, 1536, 1536)), (3, 1, 0, 0)),
    'f32_gate_500_ks3': (dict(dt='f32', epi='gate', mnk=(500, 1536, 1536), ksplit=3), (3, 3, 0, 0)),
    'f32_silugate_500': (dict(dt='f32', epi='silugate', mnk=(500, 8192, 1536)), (5, 1, 0, 0)),
    'f32_store_100': (dict(dt='f32', epi='store', mnk=(100, 1536, 1536)), (3, 1, 0, 0)),
    'pair_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(80, 6144, 1536)), (25, 1, 0, 0)),
    'pair_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), pair=(80, 4608, 1536)), (26, 1, 0, 0)),
    'pair_cross_500': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, pair=(80, 1536, 1536)), (27, 1, 0, 0)),
    'pair_gate_500_h16': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', pair=(80, 1536, 1536)), (25, 4, 0, 0)),
    'pair_fc2_500_f32slabs': (dict(epi='gate', mnk=(500, 1536, 6144), slabs='f32', pair=(80, 1536, 6144)), (25, 4, 0, 0)),
    'pair_gelu_2000': (dict(epi='gelu', mnk=(2000, 6144, 1536), pair=(320, 6144, 1536)), (32, 1, 0, 0)),
    'pair_qkv_2000': (dict(epi='qkv', mnk=(2000, 4608, 1536), pair=(320, 4608, 1536)), (28, 1, 0, 0)),
    'pair_cross_2000': (dict(epi='qkv', mnk=(2000, 1536, 1536), nK=1, pair=(320, 1536, 1536)), (25, 1, 0, 0)),
    'pair_gate_2000_h16': (dict(epi='gate', mnk=(2000, 1536, 1536), slabs='h', pair=(320, 1536, 1536)), (25, 1, 0, 0)),
    'pair_fc2_2000_f32slabs': (dict(epi='gate', mnk=(2000, 1536, 6144), slabs='f32', pair=(320, 1536, 6144)), (25, 1, 0, 0)),
    'pair_gelu_3000': (dict(epi='gelu', mnk=(3000, 6144, 1536), pair=(480, 6144, 1536)), (29, 1, 0, 0)),
    'pair_qkv_3000': (dict(epi='qkv', mnk=(3000, 4608, 1536), pair=(480, 4608, 1536)), (32, 1, 0, 0)),
    'pair_cross_3000': (dict(epi='qkv', mnk=(3000, 1536, 1536), nK=1, pair=(480, 1536, 1536)), (28, 1, 0, 0)),
    'pair_gate_3000_h16': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h', pair=(480, 1536, 1536)), (32, 3, 0, 0)),
    'pair_fc2_3000_f32slabs': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='f32', pair=(480, 1536, 6144)), (32, 3, 0, 0)),
    'pair_gelu_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536), pair=(640, 6144, 1536)), (32, 1, 0, 0)),
    'pair_qkv_4000': (dict(epi='qkv', mnk=(4000, 4608, 1536), pair=(640, 4608, 1536)), (29, 1, 0, 0)),
    'pair_cross_4000': (dict(epi='qkv', mnk=(4000, 1536, 1536), nK=1, pair=(640, 1536, 1536)), (29, 1, 0, 0)),
    'pair_gate_4000_h16': (dict(epi='gate', mnk=(4000, 1536, 1536), slabs='h', pair=(640, 1536, 1536)), (19, 1, 0, 0)),
    'pair_fc2_4000_f32slabs': (dict(epi='gate', mnk=(4000, 1536, 6144), slabs='f32', pair=(640, 1536, 6144)), (19, 1, 0, 0)),
    'pair_qkv_3840': (dict(epi='qkv', mnk=(3840, 4608, 1536), pair=(192, 4608, 1536)), (28, 1, 0, 0)),
    'pair_qkv_500_mv97': (dict(epi='qkv', mnk=(500, 4608, 1536), pair=(97, 4608, 1536)), (25, 1, 0, 0)),
    'pair_cross_500_attn': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, attn=1, pair=(80, 1536, 1536)), (27, 1, 0, 0)),
    'pair_gate_500_g1_noslabs': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', pair=(80, 1536, 1536), pair_opts={'slabs': None}), (3, 1, 0, 0)),
    'pair_gate_3000_g1_noslabs': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h', pair=(480, 1536, 1536), pair_opts={'slabs': None}), (3, 1, 0, 0)),
    'pair_gate_3000_cap2': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h', pair=(480, 1536, 1536), pair_opts={'cap': 2}), (32, 2, 0, 0)),
    'pair_gate_500_atomic': (dict(epi='gate', mnk=(1536, 1536, 1536), pair=(256, 1536, 1536)), (15, 2, 0, 0)),
    'pair_gate_3000_conv1': (dict(epi='gate', mnk=(3000, 1536, 4608), slabs='h', conv=3000, pair=(480, 1536, 1536), pair_opts={'conv': None}), (3, 1, 0, 0)),
    'pair_gelu_4000_fp8': (dict(epi='gelu', mnk=(4000, 6144, 1536), wfmt=1, pair=(640, 6144, 1536)), (32, 1, 0, 0)),
    'pair_qkv_500_fp8': (dict(epi='qkv', mnk=(500, 4608, 1536), wfmt=1, pair=(80, 4608, 1536)), (15, 1, 0, 0)),
    'pair_gate_3000_fp8': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='h', wfmt=1, pair=(480, 1536, 6144)), (32, 3, 0, 0)),
    'pair_gate_f32_500': (dict(dt='f32', epi='gate', mnk=(500, 1536, 1536), pair=(80, 1536, 1536)), (3, 1, 0, 0)),
    'pair_qkv_f32_500': (dict(dt='f32', epi='qkv', mnk=(500, 4608, 1536), pair=(80, 4608, 1536)), (8, 1, 0, 0)),
    'pair_gelu_f16_4000': (dict(dt='f16', epi='gelu', mnk=(4000, 6144, 1536), pair=(640, 6144, 1536)), (32, 1, 0, 0)),
    'pair_mixed_fmt': (dict(epi='gelu', mnk=(500, 6144, 1536), wfmt=1, pair=(80, 6144, 1536), pair_opts={'wfmt': 0}), 'GEMM: the two problems of a launch must share the weight format'),
    'pair_gelu_500_mv1': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(1, 6144, 1536)), (25, 1, 0, 0)),
    'store_16_krot': (dict(epi='store', mnk=(16, 1536, 1536), krot=1), (3, 1, 0, 0)),
    'store_224_krot': (dict(epi='store', mnk=(224, 1536, 1536), krot=1), (3, 1, 0, 0)),
    'gelu_fc1_500_krot': (dict(epi='gelu', mnk=(500, 6144, 1536), krot=1), (25, 1, 0, 1)),
    'qkv_500_krot': (dict(epi='qkv', mnk=(500, 4608, 1536), krot=1), (26, 1, 0, 1)),
    'cross_q_500_krot': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, krot=1), (27, 1, 0, 1)),
    'gate_proj_500_h16_krot': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', krot=1), (25, 5, 0, 1)),
    'gate_fc2_500_f32slabs_krot': (dict(epi='gate', mnk=(500, 1536, 6144), slabs='f32', krot=1), (25, 5, 0, 1)),
    'store_500_krot': (dict(epi='store', mnk=(500, 1536, 1536), krot=1), (3, 1, 0, 0)),
    'gelu_fc1_2000_krot': (dict(epi='gelu', mnk=(2000, 6144, 1536), krot=1), (32, 1, 0, 0)),
    'qkv_2000_krot': (dict(epi='qkv', mnk=(2000, 4608, 1536), krot=1), (28, 1, 6, 0)),
    'gate_proj_2000_h16_krot': (dict(epi='gate', mnk=(2000, 1536, 1536), slabs='h', krot=1), (32, 5, 0, 0)),
    'gelu_fc1_4000_krot': (dict(epi='gelu', mnk=(4000, 6144, 1536), krot=1), (29, 1, 6, 0)),
    'gate_proj_500_ks3_krot': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='f32', ksplit=3, krot=1), (25, 3, 0, 1)),
    'gelu_fc1_500_scalar_krot': (dict(epi='gelu', mnk=(500, 6144, 1536), scalar_out=1, krot=1), (15, 1, 0, 1)),
    'qkv_500_scalar_krot': (dict(epi='qkv', mnk=(500, 4608, 1536), scalar_out=1, krot=1), (26, 1, 0, 1)),
    'cross_q_500_attn_krot': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, attn=1, krot=1), (27, 1, 0, 1)),
    'mod_panel_224_krot': (dict(epi='store', mnk=(224, 331776, 1536), krot=1), (32, 1, 0, 0)),
    'conv_w2_500_h16_krot': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', krot=1), (22, 5, 0, 0)),
    'fp8_gelu_500_krot': (dict(epi='gelu', mnk=(500, 6144, 1536), wfmt=1, krot=1), (15, 1, 0, 1)),
    'fp8_qkv_500_krot': (dict(epi='qkv', mnk=(500, 4608, 1536), wfmt=1, krot=1), (15, 1, 0, 1)),
    'f16_qkv_500_krot': (dict(dt='f16', epi='qkv', mnk=(500, 4608, 1536), krot=1), (26, 1, 0, 1)),
    'f32_gelu_500_krot': (dict(dt='f32', epi='gelu', mnk=(500, 6144, 1536), krot=1), (5, 1, 0, 0)),
    'pair_gelu_500_krot': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(80, 6144, 1536), krot=1), (25, 1, 0, 1)),
    'pair_qkv_500_krot': (dict(epi='qkv', mnk=(500, 4608, 1536), pair=(80, 4608, 1536), krot=1), (26, 1, 0, 1)),
    'pair_cross_500_krot': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, pair=(80, 1536, 1536), krot=1), (27, 1, 0, 1)),
    'pair_gate_500_h16_krot': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', pair=(80, 1536, 1536), krot=1), (25, 4, 0, 1)),
    'pair_gate_2000_h16_krot': (dict(epi='gate', mnk=(2000, 1536, 1536), slabs='h', pair=(320, 1536, 1536), krot=1), (25, 1, 0, 1)),
    'pair_qkv_500_mv97_krot': (dict(epi='qkv', mnk=(500, 4608, 1536), pair=(97, 4608, 1536), krot=1), (25, 1, 0, 1)),
    'pair_gelu_500_mv1_krot': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(1, 6144, 1536), krot=1), (25, 1, 0, 1)),
    'ldw_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), ldw=1600), (25, 1, 0, 0)),
    'ldw_gelu_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536), ldw=1600), (29, 1, 6, 0)),
    'ldw_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), ldw=1600), (26, 1, 0, 0)),
    'ldw_gate_3000': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h', ldw=1600), (32, 3, 0, 0)),
    'ldw_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', ldw=12352), (22, 5, 0, 0)),
    'ldw_fp8_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), ldw=1600, wfmt=1), (15, 1, 0, 0)),
    'ldw_gelu_500_scalar': (dict(epi='gelu', mnk=(500, 6144, 1536), ldw=1600, scalar_out=1), (15, 1, 0, 0)),
    'ldw_pair_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(80, 6144, 1536), pair_opts={'ldw': 1600}), (25, 1, 0, 0)),
    'ldw_f32_500': (dict(dt='f32', epi='gelu', mnk=(500, 6144, 1536), ldw=1600), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'ldw_tile1': (dict(epi='gelu', mnk=(500, 6144, 1536), ldw=1600, tile=1), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'ldw_narrow_n64': (dict(epi='store', mnk=(4000, 64, 1536), ldw=1600), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'big_gelu_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536), lda=524288), (1, 1, 0, 0)),
    'big_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), lda=4194304), (1, 1, 0, 0)),
    'big_qkv_4000': (dict(epi='qkv', mnk=(4000, 4608, 1536), lda=524288), (1, 1, 0, 0)),
    'big_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), lda=4194304), (1, 1, 0, 0)),
    'big_cross_500': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, lda=4194304), (2, 1, 0, 0)),
    'big_gate_3000': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='h', lda=524288), (3, 1, 0, 0)),
    'big_gate_500': (dict(epi='gate', mnk=(500, 1536, 6144), slabs='h', lda=4194304), (1, 5, 0, 0)),
    'big_store_n64': (dict(epi='store', mnk=(4000, 64, 1536), lda=524288), (3, 1, 0, 0)),
    'big_store_500_n1536': (dict(epi='store', mnk=(4000, 256, 1536), lda=524288), (3, 1, 0, 0)),
    'big_mod_panel_w': (dict(epi='store', mnk=(224, 331776, 4096)), (1, 1, 0, 0)),
    'big_mod_panel_w_ldw': (dict(epi='store', mnk=(224, 331776, 2048), ldw=4096), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'big_pair_gelu_4000': (dict(epi='gelu', mnk=(4000, 6144, 1536), pair=(640, 6144, 1536), pair_opts={'lda': 524288}), (32, 1, 0, 0)),
    'big_pair_gate_3000': (dict(epi='gate', mnk=(3000, 1536, 1536), slabs='h', pair=(480, 1536, 1536), pair_opts={'lda': 2097152}), (32, 3, 0, 0)),
    'big_fp8': (dict(epi='gelu', mnk=(4000, 6144, 1536), lda=524288, wfmt=1), 'GEMM: fp8-weight operands exceed the 2 GiB buffer-offset range'),
    'big_conv': (dict(epi='gate', mnk=(300000, 1536, 12288), conv=300000, slabs='h'), 'GEMM: conv3 operands exceed the 2 GiB buffer-offset range'),
    'big_f32_dac': (dict(dt='f32', epi='store', mnk=(2000, 1024, 7168), lda=524288), (2, 1, 0, 0)),
    'big_tile32': (dict(epi='gelu', mnk=(4000, 6144, 1536), lda=524288, tile=32), 'GEMM: the 256x256 tiles range every load against 32-bit buffer extents: operands exceed the 2 GiB buffer-offset range'),
    'big_tile21': (dict(epi='gate', mnk=(300000, 1536, 12288), conv=300000, tile=21), 'GEMM: conv3 operands exceed the 2 GiB buffer-offset range'),
    'big_tile6': (dict(epi='store', mnk=(4000, 64, 1536), lda=524288, tile=6), (3, 1, 0, 0)),
    'big_tile27': (dict(epi='qkv', mnk=(500, 1536, 1536), nK=1, lda=4194304, tile=27), (2, 1, 0, 0)),
    'big_tile8': (dict(epi='store', mnk=(4000, 256, 1536), lda=524288, tile=8), (2, 1, 0, 0)),
    'tile1_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=1), (1, 1, 0, 0)),
    'tile2_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=2), (2, 1, 0, 0)),
    'tile3_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=3), (3, 1, 0, 0)),
    'tile4_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=4), (4, 1, 0, 0)),
    'tile5_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=5), (5, 1, 0, 0)),
    'tile6_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=6), (6, 1, 0, 0)),
    'tile7_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=7), (7, 1, 0, 0)),
    'tile8_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=8), (8, 1, 0, 0)),
    'tile9_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=9), (9, 1, 0, 0)),
    'tile15_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=15), (15, 1, 0, 0)),
    'tile19_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=19), (19, 1, 0, 0)),
    'tile25_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=25), (25, 1, 0, 0)),
    'tile29_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=29), (29, 1, 0, 0)),
    'tile32_gelu_500': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=32), (32, 1, 0, 0)),
    'tile1_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=1), (1, 1, 0, 0)),
    'tile5_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=5), (5, 1, 0, 0)),
    'tile9_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=9), (9, 1, 0, 0)),
    'tile15_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=15), (15, 1, 0, 0)),
    'tile19_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=19), (19, 1, 0, 0)),
    'tile25_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=25), (25, 1, 0, 0)),
    'tile29_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=29), (29, 1, 0, 0)),
    'tile26_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=26), (26, 1, 0, 0)),
    'tile27_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=27), (27, 1, 0, 0)),
    'tile28_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=28), (28, 1, 0, 0)),
    'tile32_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=32), (32, 1, 0, 0)),
    'tile3_qkv_500': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=3), (26, 1, 0, 0)),
    'tile5_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=5), (5, 5, 0, 0)),
    'tile15_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=15), (15, 5, 0, 0)),
    'tile25_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=25), (25, 5, 0, 0)),
    'tile29_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=29), (29, 6, 0, 0)),
    'tile1_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=1), (1, 5, 0, 0)),
    'tile9_gate_500': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=9), (9, 6, 0, 0)),
    'tile11_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=11), (11, 5, 0, 0)),
    'tile11_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=11), (11, 1, 0, 0)),
    'tile13_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=13), (13, 4, 0, 0)),
    'tile13_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=13), (13, 1, 0, 0)),
    'tile21_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=21), (21, 5, 0, 0)),
    'tile21_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=21), (21, 1, 0, 0)),
    'tile22_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=22), (22, 5, 0, 0)),
    'tile22_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=22), (22, 1, 0, 0)),
    'tile23_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=23), (23, 8, 0, 0)),
    'tile23_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=23), (23, 1, 0, 0)),
    'tile24_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=24), (24, 7, 0, 0)),
    'tile24_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=24), 'GEMM: tile 24 (192x128 conv) serves bf16 weights, gated-residual / fp32-store epilogues'),
    'tile31_conv_w2_500': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=31), (31, 8, 0, 0)),
    'tile31_conv_w13_500': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=31), (31, 1, 0, 0)),
    'tile25_scalar': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=25, scalar_out=1), (15, 1, 0, 0)),
    'tile29_scalar': (dict(epi='gelu', mnk=(4000, 6144, 1536), tile=29, scalar_out=1), (19, 1, 6, 0)),
    'tile15_fp8': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=15, wfmt=1), (15, 1, 0, 0)),
    'tile19_fp8': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=19, wfmt=2), (19, 1, 0, 0)),
    'tile21_fp8': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=21, wfmt=1), (21, 5, 0, 0)),
    'tile5_f32_gate': (dict(dt='f32', epi='gate', mnk=(500, 1536, 1536), tile=5), (5, 1, 0, 0)),
    'tile8_f32': (dict(dt='f32', epi='store', mnk=(2000, 1024, 7168), tile=8), (8, 1, 0, 0)),
    'tile11_f32': (dict(dt='f32', epi='gate', mnk=(500, 1536, 12288), conv=500, tile=11), (11, 1, 0, 0)),
    'tile13_f32': (dict(dt='f32', epi='gate', mnk=(500, 1536, 12288), conv=500, tile=13), (13, 1, 0, 0)),
    'tile3_ks0': (dict(epi='gate', mnk=(500, 1536, 1536), tile=3), (3, 2, 0, 0)),
    'tile6_ks0': (dict(epi='gate', mnk=(500, 1536, 1536), tile=6), (6, 2, 0, 0)),
    'tile2_ks0': (dict(epi='gate', mnk=(500, 1536, 1536), tile=2), (2, 2, 0, 0)),
    'err_tile5_fp8': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=5, wfmt=1), 'GEMM: fp8 weights need tile 15, 19 or 21'),
    'err_tile25_fp8': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=25, wfmt=1), 'GEMM: fp8 weights need tile 15, 19 or 21'),
    'err_fp8_f32': (dict(dt='f32', epi='gelu', mnk=(500, 6144, 1536), wfmt=1), 'GEMM: fp8 weight storage needs bf16 operands'),
    'err_tile21_plain': (dict(epi='gate', mnk=(500, 1536, 1536), slabs='h', tile=21), 'GEMM: tiles 21 / 22 / 23 / 24 need a bf16 channels-last conv k=3'),
    'err_tile22_fp8': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=22, wfmt=1), 'GEMM: tile 22 serves bf16 weights'),
    'err_tile24_silugate': (dict(epi='silugate', mnk=(500, 8192, 4608), conv=500, tile=24), 'GEMM: tile 24 (192x128 conv) serves bf16 weights, gated-residual / fp32-store epilogues'),
    'err_tile24_fp8': (dict(epi='gate', mnk=(500, 1536, 12288), conv=500, slabs='h', tile=24, wfmt=1), 'GEMM: tile 24 (192x128 conv) serves bf16 weights, gated-residual / fp32-store epilogues'),
    'err_tile27_gelu': (dict(epi='gelu', mnk=(500, 6144, 1536), tile=27), 'GEMM: tile 27 (64x128) serves the fused head split with bf16 weights only'),
    'err_tile26_store': (dict(epi='store', mnk=(500, 6144, 1536), tile=26), 'GEMM: tile 27 (64x128) serves the fused head split with bf16 weights only'),
    'err_tile28_fp8': (dict(epi='qkv', mnk=(500, 4608, 1536), tile=28, wfmt=1), 'GEMM: fp8 weights need tile 15, 19 or 21'),
    'err_tile10_gate': (dict(epi='gate', mnk=(500, 1536, 1536), tile=10), 'GEMM: unknown tile'),
    'err_tile33_gate': (dict(epi='gate', mnk=(500, 1536, 1536), tile=33), 'GEMM: unknown tile'),
    'err_tile_neg_gate': (dict(epi='gate', mnk=(500, 1536, 1536), tile=-1), 'GEMM: unknown tile'),
    'err_misaligned': (dict(epi='gelu', mnk=(500, 6144, 1536), misaligned_A=1), 'GEMM: operands must be 16-byte aligned'),
    'err_k_slice': (dict(epi='gelu', mnk=(500, 6144, 1000)), 'GEMM: K / tap width / lda must be multiples of the 128-byte K-slice'),
    'err_pair_k_slice': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(80, 6144, 1000)), 'GEMM: K / tap width / lda must be multiples of the 128-byte K-slice'),
    'err_pair_misaligned': (dict(epi='gelu', mnk=(500, 6144, 1536), pair=(80, 6144, 1536), pair_opts={'misaligned_A': 1}), 'GEMM: operands must be 16-byte aligned'),
    'err_qkv_n': (dict(epi='qkv', mnk=(500, 4736, 1536), nK=3), 'fused head split: N must be nK*H*128 and M a multiple of L'),
    'err_qkv_l': (dict(epi='qkv', mnk=(500, 4608, 1536), L=300), 'fused head split: N must be nK*H*128 and M a multiple of L'),
    'err_ldw_f32': (dict(dt='f32', epi='store', mnk=(500, 1536, 1536), ldw=1600), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'err_ldw_tile5': (dict(epi='gelu', mnk=(500, 6144, 1536), ldw=1600, tile=5), 'GEMM: padded weight rows (ldw != K) need a wave-specialised tile'),
    'err_big_fp8': (dict(epi='gate', mnk=(3000, 1536, 6144), slabs='h', lda=524288, wfmt=1), 'GEMM: fp8-weight operands exceed the 2 GiB buffer-offset range'),
    'err_big_conv_tile23': (dict(epi='gate', mnk=(300000, 1536, 12288), conv=300000, tile=23), 'GEMM: conv3 operands exceed the 2 GiB buffer-offset range'),
    'err_big_tile31': (dict(epi='gate', mnk=(300000, 1536, 12288), conv=300000, tile=31), 'GEMM: the 256x256 tiles range every load against 32-bit buffer extents: operands exceed the 2 GiB buffer-offset range'),
}


@pytest.mark.parametrize("cid", list(CASES))
def test_gemm_plan(cid):
    case, want = CASES[cid]
    got = plan(case)
    if isinstance(want, str):
        assert isinstance(got, str) and want in got, (cid, got)
    else:
        assert got == want, (cid, got)


def test_plan_needs_no_device_and_checks_its_arguments():
    lib = _lib()
    out = (C.c_int32 * 4)()
    assert lib.foley_debug_gemm_plan(None, None, 0, out) != 0
    keep = []
    d0 = _desc("bf16", "gelu", 500, 6144, 1536, {}, keep)
    d1 = _desc("bf16", "store", 80, 6144, 1536, {}, keep)
    assert lib.foley_debug_gemm_plan(C.byref(d0), C.byref(d1), 0, out) != 0   # the two problems must share the epilogue
    assert "epilogue" in lib.foley_last_error().decode()
