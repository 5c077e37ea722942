"""Two-problem launches of the two-stream blocks at op level, K-origin rotation, and the LayerNorm at the DiT's width.

run_forward's triple-stream blocks launch the audio and the (much smaller) visual stream as ONE GEMM / LayerNorm
(launch_gemm_pair, launch_ln_mod_pair) and, for single-clip forwards, let the small-grid GEMMs rotate their K origin per M tile
(GemmArgs::krot_ok).  None of that is reachable through the C ABI, so the library carries test-only entries (foley_debug_gemm_pair,
foley_debug_gemm_krot, foley_debug_gemm_last, foley_debug_ln_mod_pair; not in include/foley_hip.h, typed here with ctypes).

Every pair is checked three ways: each problem against an fp64 CPU reference; the pair against two single launches forced to
the tile / K split the pair reported (bit for bit - pairs and singles differ only in workgroup order); and the reported tile
against PAIR_TILES below, which is derived from launch_typed's rules (gemm_impl.h), so that a change of a tile rule cannot
silently move a case off the tile family it was written for.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import opcheck as oc
from conftest import record_parity, rel_err
from foley_amd.host import runtime as rt, tables

pytestmark = pytest.mark.gpu

# ----------------------------------------------------------------------------- expected tiles
# case id -> (operands, epilogue, (M, N, K) of the audio problem, (Mv, Nv, Kv) of the visual problem, options, tile the launcher
# must report).  D = 1536, H = 12, mlp_hidden 6144 (xl: 1408 / 11 / 5632); (500, 80) = bs 1 at 5 s, (4000, 640) = bs 8,
# (3000, 480) = 30 s.  Derivations (gemm_impl.h launch_typed, "b128" = 128x128 tiles of the audio problem):
#   gelu 500+80      b128 192 -> tile 5 -> 16-bit: 25 (fp8: 15); fp32 (b128 > 160, no half tiles) 5
#   gelu 4000+640    256x128 grid 768 -> 9 -> 29 (fp8: 19); short-K rule: 4 rounds of 256x128 vs 2 of 256x256 -> 32
#   gelu 3000+480    9 -> 29; short-K rule: 3 rounds vs 2 x 1.64 -> stays 29
#   qkv  500+80      5 -> 25; head split: 96-row tiles 216 + 36 <= 256 -> 26 (fp8: 15); fp32: b128 144, 64x128 288 -> 8
#   qkv  4000+640    9 -> 29; 192-row tiles cost 4 rounds -> 29; short-K 3 rounds vs 2 x 1.64 -> 29 (fp8: 19)
#   qkv  3000+480    9 -> 29; short-K: 2 rounds of 256x128 vs ONE of 256x256 -> 32
#   qkv  3840+192    9 -> 29; 192-row tiles 756 (3 rounds x 320) < 612 (3 x 384) -> 28
#   cross 500+80     b128 48 -> 3, not a head-split tile -> 25 -> with the visual problem 60 <= 100 -> 27, fused attention
#   cross 4000+640   256x128 grid 192 + 36 -> 9 -> 29 (no fused attention); cross 3000+480: 168 -> 9, 192-row tiles -> 28
#   gate 500+80      deferred slabs, b128 48 -> 5 -> 25, K split 256 / 60 -> 4 (forced: as asked)
#   gate 4000+640    256x128 grid 192 -> 9 -> 19 (gated residual), K split 256 / 228 -> 1
#   gate 3000+480    b128 288 -> 3, mid-size route (pair 336 > 256) -> 256x256 with ksp 256 / 84 -> 3 K ranges -> 32
#   gate 1536+256    atomics (no slabs): b128 144 -> 5 -> 25, K split 2, scalar epilogue -> 15
#   gate g0 slabs    the visual problem has none: no deferred route, b128 48 -> 3, slab cap 1 -> K split 1
PAIR_TILES = {
    # fp32 operands (parity mode)
    "f32_gelu_5s": ("f32", "gelu", (500, 6144, 1536), (80, 6144, 1536), {}, 5),
    "f32_qkv_5s": ("f32", "qkv", (500, 4608, 1536), (80, 4608, 1536), {}, 8),
    "f32_qkv_small": ("f32", "qkv", (80, 768, 1536), (16, 768, 1536), {"H": 2}, 2),
    "f32_cross_5s": ("f32", "cross", (500, 1536, 1536), (80, 1536, 1536), {}, 5),
    "f32_gate_5s": ("f32", "gate", (500, 1536, 1536), (80, 1536, 1536), {}, 3),
    "f32_gate_atomic_ks3": ("f32", "gate", (500, 1536, 1536), (80, 1536, 1536), {"ksplit": 3}, 3),
    # 16-bit operands (bf16 and fp16)
    "gelu_5s": ("h", "gelu", (500, 6144, 1536), (80, 6144, 1536), {}, 25),
    "gelu_5s_mv1": ("h", "gelu", (500, 6144, 1536), (1, 6144, 1536), {}, 25),
    "gelu_5s_mv127": ("h", "gelu", (500, 6144, 1536), (127, 6144, 1536), {}, 25),
    "gelu_5s_mv129": ("h", "gelu", (500, 6144, 1536), (129, 6144, 1536), {}, 25),
    "gelu_xl": ("h", "gelu", (500, 5632, 1408), (80, 5632, 1408), {}, 25),
    "gelu_bs8": ("h", "gelu", (4000, 6144, 1536), (640, 6144, 1536), {}, 32),
    "gelu_30s": ("h", "gelu", (3000, 6144, 1536), (480, 6144, 1536), {}, 29),
    "gelu_mixed_nk": ("h", "gelu", (500, 6144, 1536), (80, 1536, 1024), {}, 25),
    "qkv_5s": ("h", "qkv", (500, 4608, 1536), (80, 4608, 1536), {}, 26),
    "qkv_5s_mv1": ("h", "qkv", (500, 4608, 1536), (1, 4608, 1536), {"Bc": 1}, 26),
    "qkv_5s_mv95": ("h", "qkv", (500, 4608, 1536), (95, 4608, 1536), {"Bc": 1}, 26),
    "qkv_5s_mv97": ("h", "qkv", (500, 4608, 1536), (97, 4608, 1536), {"Bc": 1}, 25),
    "qkv_xl": ("h", "qkv", (500, 4224, 1408), (80, 4224, 1408), {"H": 11}, 26),
    "qkv_bs8": ("h", "qkv", (4000, 4608, 1536), (640, 4608, 1536), {"Bc": 16}, 29),
    "qkv_30s": ("h", "qkv", (3000, 4608, 1536), (480, 4608, 1536), {}, 32),
    "qkv_3840": ("h", "qkv", (3840, 4608, 1536), (192, 4608, 1536), {}, 28),
    "cross_5s": ("h", "cross", (500, 1536, 1536), (80, 1536, 1536), {}, 27),
    "cross_bs8": ("h", "cross", (4000, 1536, 1536), (640, 1536, 1536), {"Bc": 16}, 29),
    "cross_30s": ("h", "cross", (3000, 1536, 1536), (480, 1536, 1536), {}, 28),
    "cross_xl": ("h", "cross", (500, 1408, 1408), (80, 1408, 1408), {"H": 11}, 27),
    "gate_5s_f32slabs": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "f32"}, 25),
    "gate_5s_h16slabs": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "h", "tok_gate": True}, 25),
    "gate_fc2_5s": ("h", "gate", (500, 1536, 6144), (80, 1536, 6144), {"slabs": "h"}, 25),
    "gate_5s_ks3": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "f32", "ksplit": 3}, 25),
    "gate_5s_ks7": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "h", "ksplit": 7}, 25),
    "gate_xl": ("h", "gate", (500, 1408, 1408), (80, 1408, 1408), {"slabs": "h"}, 25),
    "gate_bs8": ("h", "gate", (4000, 1536, 1536), (640, 1536, 1536), {"slabs": "h"}, 19),
    "gate_30s": ("h", "gate", (3000, 1536, 1536), (480, 1536, 1536), {"slabs": "h"}, 32),
    "gate_30s_fc2": ("h", "gate", (3000, 1536, 6144), (480, 1536, 6144), {"slabs": "f32"}, 32),
    "gate_atomic": ("h", "gate", (1536, 1536, 1536), (256, 1536, 1536), {}, 15),
    "gate_g0_slabs_only": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "h", "g1_slabs": False}, 3),
    "gate_g0_slabs_only_ks4": ("h", "gate", (500, 1536, 1536), (80, 1536, 1536), {"slabs": "h", "g1_slabs": False, "ksplit": 4}, 3),
    "gate_mixed_n": ("h", "gate", (500, 1536, 1536), (80, 768, 1536), {"slabs": "h"}, 25),
    "gate_mixed_short_k": ("h", "gate", (500, 1536, 6144), (80, 1536, 128), {"slabs": "f32"}, 25),
    "gate_mixed_short_k_wide": ("h", "gate", (3000, 1536, 1536), (480, 1536, 64), {"slabs": "h"}, 32),
    # fp8 e4m3fn weight storage under bf16 activations
    "fp8_gelu_5s": ("fp8", "gelu", (500, 6144, 1536), (80, 6144, 1536), {}, 15),
    "fp8_gelu_bs8": ("fp8", "gelu", (4000, 6144, 1536), (640, 6144, 1536), {}, 32),
    "fp8_qkv_5s": ("fp8", "qkv", (500, 4608, 1536), (80, 4608, 1536), {}, 15),
    "fp8_qkv_bs8": ("fp8", "qkv", (4000, 4608, 1536), (640, 4608, 1536), {"Bc": 16}, 19),
    "fp8_gate_bs8": ("fp8", "gate", (4000, 1536, 1536), (640, 1536, 1536), {"slabs": "h"}, 19),
}
# the tile families every operand kind must reach (32 by both routes: the short-K rule and the mid-size gated-residual route)
REQUIRED_TILES = {"f32": {5, 3, 2, 8}, "h": {15, 25, 27, 26, 28, 19, 29, 32}, "fp8": {15, 19, 32}}
SHORT_K_32 = ("gelu_bs8", "qkv_30s")
MID_SPLIT_32 = ("gate_30s", "gate_30s_fc2")

F32_TOL, BF16_TOL, F16_TOL = 2e-6, 6e-3, 8e-4                      # test_ops_gpu.py: per-dtype GEMM gates
QKV_TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3, torch.float16: 6e-4}   # test_gemm_fused_head_split
ATTN_TOL = {torch.float32: 1e-5, torch.bfloat16: 6e-3, torch.float16: 1e-3}  # test_gemm_cross_q_with_attention_epilogue
SLAB_TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3, torch.float16: 5e-4}  # test_gemm_deferred_split_k
RES_TOL = 1e-5                                                               # test_gemm_split_k: x + gate * y
# rotated vs unrotated K walk (same tile, same K split), relative Frobenius distance over the whole output: fp32 results differ by
# fp32 summation order only; 16-bit results additionally by the final rounding of the elements where that order flips it
ROT_BOUND = {torch.float32: 1e-6, torch.bfloat16: 5e-4, torch.float16: 2e-4}   # measured on MI355X: 2.7e-7, 1.6e-4, 5.3e-5

EPI = {"gelu": rt.EPI_GELU_T, "qkv": rt.EPI_QKV_SPLIT, "cross": rt.EPI_QKV_SPLIT, "gate": rt.EPI_GATE_RES,
       "store": rt.EPI_STORE_F32}


def _tol(dtype):
    return {torch.float32: F32_TOL, torch.bfloat16: BF16_TOL, torch.float16: F16_TOL}[dtype]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_g(seed)) * scale


def _sample_rows(M):
    """Every row below 3000; above, a few hundred spread over M including the first and the last 16 (test_gemm_bf16_past_2gib).
    The LayerNorm cases below sample with it; the GEMM pairs check every row (Problem)."""
    if M < 3000:
        return torch.arange(M)
    idx = torch.cat((torch.arange(16), torch.randint(16, M - 16, (224,), generator=_g(90)), torch.arange(M - 16, M)))
    return idx.unique()


# ----------------------------------------------------------------------------- test-only library entries
_typed = []


def _lib():
    lib = rt.load_library()
    if not _typed:
        rb = C.POINTER(rt.RowBcastC)
        lib.foley_debug_gemm_pair.argtypes = [C.POINTER(rt.GemmDescC), C.POINTER(rt.GemmDescC), C.c_void_p]
        lib.foley_debug_gemm_pair.restype = C.c_int
        lib.foley_debug_gemm_krot.argtypes = [C.c_int]
        lib.foley_debug_gemm_krot.restype = C.c_int
        lib.foley_debug_gemm_last.argtypes = [C.POINTER(C.c_int)] * 3
        lib.foley_debug_gemm_last.restype = None
        one = [C.c_void_p, C.c_int, rb, rb, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, rb]
        lib.foley_debug_ln_mod_pair.argtypes = one + one + [C.c_int, C.c_float, C.c_int, C.c_void_p]
        lib.foley_debug_ln_mod_pair.restype = C.c_int
        _typed.append(True)
    return lib


def gemm_pair(d0, d1) -> int:
    """One launch of both problems (launch_gemm_pair); returns the shared K split."""
    lib = _lib()
    rt._check(lib, lib.foley_debug_gemm_pair(C.byref(d0), C.byref(d1), rt._stream()), "foley_debug_gemm_pair")
    return int(d0._used.value)


def gemm_last():
    """(tile, K split, k_rot) of this thread's last dispatched GEMM."""
    t, k, r = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib().foley_debug_gemm_last(C.byref(t), C.byref(k), C.byref(r))
    return t.value, k.value, r.value


def gemm_krot(on: bool) -> int:
    return _lib().foley_debug_gemm_krot(1 if on else 0)


def ln_mod_pair(sets, D, eps, out_dtype_code):
    """sets: two dicts x, M, shift, scale, out, partials (None: nothing pending), k, bias, gate."""
    lib = _lib()
    args = []
    for s in sets:
        p = s.get("partials")
        args += [rt._ptr(s["x"]) if s["M"] > 0 else None, s["M"], C.byref(s["shift"]) if s.get("shift") else None,
                 C.byref(s["scale"]) if s.get("scale") else None, rt._ptr(s["out"]) if s["M"] > 0 else None,
                 rt._ptr(p) if p is not None else None, 0 if p is None or p.dtype == torch.float32 else rt.dt_of(p),
                 s.get("k", 0), rt._ptr(s["bias"]) if s.get("bias") is not None else None,
                 C.byref(s["gate"]) if p is not None else None]
    rt._check(lib, lib.foley_debug_ln_mod_pair(*args, D, eps, out_dtype_code, rt._stream()), "foley_debug_ln_mod_pair")


# ----------------------------------------------------------------------------- GEMM pair problems
class Problem:
    """One stream's GEMM: operands rounded through the compute dtype, fp64 reference of ALL rows, output buffers.  ew: the problem
    belongs to a large-grid case (M >= 3000 - the 256x256 tiles, the three-range split-K route) and is checked element by element
    as well (tests/opcheck.py); it then carries mag = |A| @ |W|^T + |bias| for the bound."""

    def __init__(self, dev, kind, epi, M, N, K, seed, opts, S=None, ew=False):
        self.dev, self.epi, self.M, self.N, self.K = dev, epi, M, N, K
        self.dt = {"f32": torch.float32, "h": opts["dt"], "fp8": torch.bfloat16}[kind]
        A = _rand((M, K), seed).to(self.dt)
        W = _rand((N, K), seed + 1, 1 / math.sqrt(K))
        W = W.to(torch.float8_e4m3fn) if kind == "fp8" else W.to(self.dt)
        b = _rand((N,), seed + 2, 0.1)
        self.rows = torch.arange(M)
        self.y = A.double() @ W.double().t() + b.double()                      # [M, N] fp64
        self.ew = ew
        if ew:
            self.mag0 = A.double().abs() @ W.double().abs().t()
            self.e_y = (K + 4) * oc.U32 * (self.mag0 + b.double().abs())
        self.Ad, self.Wd, self.bd = A.to(dev), W.to(dev), b.to(dev)
        self.seed = seed

    def fresh_gate(self, opts):
        M, N, dev = self.M, self.N, self.dev
        self.x0 = _rand((M, N), self.seed + 3)
        if opts.get("tok_gate"):   # per-(cfg, token) gate rows: rows [cfg = 2][clip][l], L tokens
            L = self.L
            self.gate = _rand((2 * L, N), self.seed + 4)
            self.g_full = self.gate.view(2, 1, L, N).expand(2, M // (2 * L), L, N).reshape(M, N)
            self.rb = rt.rowbcast(self.gate.to(dev), 1, rows_per_cfg=M // 2, L=L)
        else:
            self.gate = _rand((N,), self.seed + 4)
            self.g_full = self.gate.expand(M, N)
            self.rb = rt.rowbcast(self.gate.to(dev), 0)


def _nan(shape, dev, dtype):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _rope64(x, cos, sin):
    """x [n, H, 128] fp64, cos / sin [n, 64]: x * cos + rotate_half(x) * sin per pair (oracle apply_rope, in fp64)."""
    c2, s2 = cos.repeat_interleave(2, 1)[:, None], sin.repeat_interleave(2, 1)[:, None]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return x * c2 + torch.stack((-x1, x0), dim=-1).flatten(-2) * s2


def _rms64(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


class PairCase:
    """Builds both problems of a case, their (NaN-initialised) outputs, descriptors for a pair or single launches, and checks."""

    def __init__(self, dev, case, dt):
        kind, epi, s0, s1, opts, self.want_tile = PAIR_TILES[case]
        self.kind, self.epi, self.opts, self.dev = kind, epi, dict(opts, dt=dt), dev
        ew = s0[0] >= 3000
        self.p = [Problem(dev, kind, epi, *s0, 1000, self.opts, ew=ew), Problem(dev, kind, epi, *s1, 2000, self.opts, ew=ew)]
        self.ew_ratio = 0.0      # largest err / bound of the element-wise checks (recorded by test_gemm_pair)
        self.dt = self.p[0].dt
        P0, P1 = self.p
        if epi in ("qkv", "cross"):
            self.H = opts.get("H", 12)
            self.nK = 3 if epi == "qkv" else 1
            self.Bc = opts.get("Bc", 2)
            P0.L, P1.L = P0.M // self.Bc, P1.M // self.Bc
            assert P0.L * self.Bc == P0.M and P1.L * self.Bc == P1.M
            self.S = P0.L + P1.L
            P0.tok_off, P1.tok_off = P1.L, 0                      # visual tokens first, audio at Lv (run_forward split_args)
            self.Sp = (self.S + 31) // 32 * 32
            self.h16 = self.dt != torch.float32
            P = max(P0.L, 3 * P1.L) + 1
            self.cos, self.sin = tables.rope_table(P)
            for i, Pi in enumerate(self.p):
                Pi.gains = [1 + 0.1 * _rand((128,), Pi.seed + 5 + j) for j in range(2)]
                Pi.pos = (torch.arange(Pi.L) * (1 if i == 0 else 3)).to(torch.int32)
            if epi == "cross":
                self.clips = self.Bc // 2
                self.Skv, self.pitch = 77, 96
                self.tk = _rand((2, self.H, self.Skv, 128), 3001).to(self.dt)
                self.tv = _rand((2, self.H, self.Skv, 128), 3002).to(self.dt)
        if epi == "gate":
            for Pi in self.p:
                Pi.L = Pi.M // 2 if Pi.M % 2 == 0 else Pi.M
                Pi.fresh_gate(self.opts if Pi.M % 2 == 0 else {})

    # -- buffers -------------------------------------------------------------------------------------------------------------
    def buffers(self):
        """A fresh set of NaN-initialised outputs (shared Q / K / V for the head split) + the V^T pad contents."""
        dev, dt, P0, P1 = self.dev, self.dt, *self.p
        b = {}
        if self.epi == "gelu":
            b["out"] = [_nan((Pi.M, Pi.N), dev, dt) for Pi in self.p]
        elif self.epi in ("qkv", "cross"):
            Bc, H, S = self.Bc, self.H, self.S
            b["q"] = _nan((Bc, H, S, 128), dev, dt)
            if self.epi == "qkv":
                b["k"] = _nan((Bc, H, S, 128), dev, dt)
                if self.h16:
                    vt = _rand((Bc, H, 128, self.Sp), 3003).to(dt)
                    vt[..., :S] = float("nan")
                    b["v"] = vt.to(dev)
                else:
                    b["v"] = _nan((Bc, H, S, 128), dev, dt)
            else:
                b["att"] = [_nan((Pi.M, H * 128), dev, dt) for Pi in self.p]
                b["tk"] = self.tk.to(dev)
                if self.h16:
                    vt = torch.zeros(2, H, 128, self.pitch, dtype=dt)
                    vt[..., :self.Skv] = self.tv.transpose(2, 3)
                    b["tv"] = vt.to(dev)
                else:
                    b["tv"] = self.tv.to(dev)
        else:
            b["x"] = [Pi.x0.to(dev) for Pi in self.p]
            sl = self.opts.get("slabs")
            if sl:
                sdt = torch.float32 if sl == "f32" else dt
                b["slabs"] = [_nan((8, Pi.M, Pi.N), dev, sdt) for Pi in self.p]
                if self.opts.get("g1_slabs", True) is False:
                    b["slabs"][1] = None
        return b

    def descs(self, b, tile=0, ksplit=None):
        """Descriptors of both problems writing into the buffers b."""
        out = []
        for i, Pi in enumerate(self.p):
            kw = dict(epilogue=EPI[self.epi], tile=tile)
            if self.epi == "gelu":
                kw["out0"] = b["out"][i]
            elif self.epi in ("qkv", "cross"):
                g = [Pi.gains[0].to(self.dev), Pi.gains[1].to(self.dev), None][:self.nK]
                pos = Pi.pos.to(self.dev)
                dst = [b["q"], b["k"], b["v"]] if self.epi == "qkv" else [b["q"]]
                poss = [pos, pos, None] if self.epi == "qkv" else [pos]
                attn = (b["tk"], b["tv"], b["att"][i], self.clips) if self.epi == "cross" else None
                vtp = self.Sp if (self.epi == "qkv" and self.h16) else 0
                kw["qkv"] = rt.qkv_split_desc(Pi.L, self.H, g, poss, dst, self.S, Pi.tok_off, 1e-6, self.cos.to(self.dev),
                                              self.sin.to(self.dev), vt_pitch=vtp, attn=attn)
            else:
                kw.update(out0=b["x"][i], rb=Pi.rb, ksplit=self.opts.get("ksplit", 0) if ksplit is None else ksplit)
                if b.get("slabs") and b["slabs"][i] is not None:
                    kw["partials"] = b["slabs"][i]
            d = rt.gemm_desc(Pi.Ad, Pi.Wd, Pi.bd, **kw)
            d._q = kw.get("qkv")      # (d.qkv.contents is a new wrapper without the fused flag)
            out.append(d)
        return out

    # -- checks --------------------------------------------------------------------------------------------------------------
    def check_reference(self, b, ks, fused, record):
        dt, dev = self.dt, self.dev
        worst = 0.0
        if self.epi == "gelu":
            for i, Pi in enumerate(self.p):
                o = b["out"][i]
                assert bool(torch.isfinite(o).all()), f"problem {i}: unwritten or non-finite outputs"
                e = rel_err(o[Pi.rows.to(dev)].float(), F.gelu(Pi.y, approximate="tanh"))
                assert e < _tol(dt), (i, e)
                worst = max(worst, e)
                if Pi.ew:
                    a_act = oc.measure_a_act("gelu", Pi.y, dev)
                    record_parity(f"pair_gemm.a_act.gelu.M{Pi.M}.{str(dt)[6:]}", a_act=a_act)
                    self.ew_ratio = max(self.ew_ratio, oc.assert_elementwise(
                        o, oc.act64("gelu", Pi.y), oc.act_bound("gelu", Pi.e_y, a_act, dt), f"problem {i}: GELU output"))
        elif self.epi == "qkv":
            S = self.S
            for name in ("q", "k"):
                assert not bool(torch.isnan(b[name]).any()), f"{name}: token rows left unwritten"
            vt = b["v"]
            if self.h16:
                assert not bool(torch.isnan(vt[..., :S]).any()), "V^T: token columns left unwritten"
                assert torch.equal(vt[..., S:].cpu(), self.vt_pad), "V^T pad columns [S, Sp) were overwritten"
            else:
                assert not bool(torch.isnan(vt).any())
            for i, Pi in enumerate(self.p):
                r = Pi.rows
                bi, li = r // Pi.L, r % Pi.L
                y = Pi.y.view(len(r), 3, self.H, 128)
                cos, sin = self.cos[Pi.pos[li].long()].double(), self.sin[Pi.pos[li].long()].double()
                rq = _rope64(_rms64(y[:, 0], Pi.gains[0].double(), 1e-6), cos, sin)
                rk = _rope64(_rms64(y[:, 1], Pi.gains[1].double(), 1e-6), cos, sin)
                tok = (li + Pi.tok_off).to(dev)
                bd = bi.to(dev)
                gq = b["q"][bd, :, tok].float()                    # [n, H, 128]
                gk = b["k"][bd, :, tok].float()
                gv = vt[bd, :, :, tok].float() if self.h16 else vt[bd, :, tok].float()
                for got, ref in ((gq, rq), (gk, rk), (gv, y[:, 2])):
                    e = rel_err(got, ref)
                    assert e < QKV_TOL[dt], (i, e)
                    worst = max(worst, e)
                if Pi.ew:
                    ey = Pi.e_y.view(len(r), 3, self.H, 128)
                    for j, (got, ref) in enumerate(((gq, rq), (gk, rk), (gv, y[:, 2]))):
                        bound = oc.head_split_bound(ey[:, j], y[:, j], dt, Pi.gains[j] if j < 2 else None)
                        self.ew_ratio = max(self.ew_ratio, oc.assert_elementwise(got, ref, bound, f"problem {i}: head split {'qkv'[j]}"))
        elif self.epi == "cross":
            H, S = self.H, self.S
            if not fused:   # plain head split: q in dst[0], attention launched by the caller (run_forward's cross step)
                assert not bool(torch.isnan(b["q"]).any()), "q: token rows left unwritten"
                assert all(bool(torch.isnan(a).all()) for a in b["att"]), "attention rows written by a non-fused launch"
                vt = b["tv"]
                rt.op_attention(b["q"], b["tk"], vt, b["att"][1], b["att"][0], self.p[1].L, kv_bdiv=self.clips)
            else:
                assert bool(torch.isnan(b["q"]).all()), "fused launch wrote q"
            for i, Pi in enumerate(self.p):
                a = b["att"][i]
                assert bool(torch.isfinite(a).all()), f"problem {i}: attention rows left unwritten"
                r = Pi.rows
                bi, li = r // Pi.L, r % Pi.L
                y = Pi.y.view(len(r), H, 128)
                cos, sin = self.cos[Pi.pos[li].long()].double(), self.sin[Pi.pos[li].long()].double()
                rq = _rope64(_rms64(y, Pi.gains[0].double(), 1e-6), cos, sin).to(dt).double()   # rounded like the kernel's q
                sets = bi // self.clips
                k, v = self.tk.double()[sets], self.tv.double()[sets]    # [n, H, Skv, 128]
                s = torch.einsum("nhd,nhkd->nhk", rq, k) / math.sqrt(128)
                ref = torch.einsum("nhk,nhkd->nhd", torch.softmax(s, -1), v).reshape(len(r), H * 128)
                e = rel_err(a[r.to(dev)].float(), ref)
                assert e < ATTN_TOL[dt], (i, e)
                worst = max(worst, e)
                if fused:
                    # Every element as well, in the GENERAL form of opcheck.cross_attention_ref_and_bound: random operands, so the
                    # projection carries its real accumulation bound e_y and, at K ~ 1536, nearly every bf16 element of q is ambiguous
                    # in its on-chip rounding (the dyadic cases of test_ops_elementwise_gpu.py are the sharp ones).  The bound is then
                    # a few per cent of P @ |V| - weak, but rigorous, and enough to catch a row served from the wrong text set or a
                    # query that lost a key tile (errors of tens of per cent of P @ |V| on that row), which the norm gate above averages away.
                    mag = Pi.Ad.double().cpu().abs() @ Pi.Wd.float().double().cpu().abs().t() + Pi.bd.double().cpu().abs()
                    e_y = ((Pi.K + 4) * oc.U32 * mag).view(len(r), H, 128)
                    q64 = _rope64(_rms64(y, Pi.gains[0].double(), 1e-6), cos, sin)
                    e_q = oc.head_split_pre_bound(e_y, y, Pi.gains[0])
                    ref_e, bound, share = oc.cross_attention_ref_and_bound(q64, e_q, self.tk, self.tv, sets, dt)
                    self.ew_ratio = max(self.ew_ratio, oc.assert_elementwise(a, ref_e, bound, f"problem {i}: fused cross attention"))
                    self.amb_share = max(getattr(self, "amb_share", 0.0), share)
        else:
            sl = b.get("slabs")
            for i, Pi in enumerate(self.p):
                rows = Pi.rows.to(dev)
                x = b["x"][i]
                slabs = sl[i] if sl else None
                yv = Pi.y - Pi.bd.double().cpu()                     # raw product, bias not included
                if slabs is not None and ks > 1:
                    assert torch.equal(x.cpu(), Pi.x0), f"problem {i}: residual touched by a deferred split-K launch"
                    assert bool(torch.isfinite(slabs[:ks]).all()), f"problem {i}: slab elements left unwritten"
                    assert bool(torch.isnan(slabs[ks:]).all()), f"problem {i}: slabs beyond the K split written"
                    e = rel_err(slabs[:ks, rows].double().sum(0), yv)
                    assert e < SLAB_TOL[slabs.dtype], (i, e)
                    if Pi.ew:
                        bound = oc.slab_bound((Pi.K + 4) * oc.U32 * Pi.mag0, Pi.mag0, ks, slabs.dtype)
                        self.ew_ratio = max(self.ew_ratio, oc.assert_elementwise(slabs[:ks].double().sum(0), yv, bound, f"problem {i}: slab sum"))
                else:
                    if slabs is not None:
                        assert bool(torch.isnan(slabs).all()), f"problem {i}: slabs written without a K split"
                    ref = Pi.x0[Pi.rows].double() + Pi.y * Pi.g_full[Pi.rows].double()
                    e = rel_err(x[rows], ref)
                    assert e < RES_TOL, (i, e)
                    if Pi.ew:
                        bound = oc.gated_residual_bound(Pi.e_y, Pi.g_full, Pi.x0, Pi.y)
                        self.ew_ratio = max(self.ew_ratio, oc.assert_elementwise(x, ref, bound, f"problem {i}: gated residual"))
                    assert bool(torch.isfinite(x).all())
                worst = max(worst, e)
        record.append(worst)

    def outputs(self, b, fused=False):
        """Everything a launch may write, for bit comparisons (non-fused cross: the attention ran after the pair launch)."""
        if self.epi == "gelu":
            return list(b["out"])
        if self.epi == "qkv":
            return [b["q"], b["k"], b["v"]]
        if self.epi == "cross":
            return [b["q"]] + (list(b["att"]) if fused else [])
        return list(b["x"]) + [s for s in (b.get("slabs") or []) if s is not None]


def _bits_equal(a, b):
    """Bit equality that treats NaN payloads alike (unwritten outputs stay NaN in both)."""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


def _case_params():
    out = []
    for case, (kind, *_rest) in PAIR_TILES.items():
        dts = [torch.bfloat16, torch.float16] if kind == "h" else [torch.float32 if kind == "f32" else torch.bfloat16]
        out += [pytest.param(case, dt, id=f"{case}-{str(dt)[6:]}") for dt in dts]
    return out


def test_pair_table_covers_every_tile_family():
    """The coverage promise of PAIR_TILES: every tile id listed per operand kind has a case (each case asserts it is reached)."""
    for kind, need in REQUIRED_TILES.items():
        have = {v[-1] for v in PAIR_TILES.values() if v[0] == kind}
        assert need <= have, (kind, need - have)
    assert all(PAIR_TILES[c][-1] == 32 and PAIR_TILES[c][1] in ("gelu", "qkv") for c in SHORT_K_32)
    assert all(PAIR_TILES[c][-1] == 32 and PAIR_TILES[c][1] == "gate" for c in MID_SPLIT_32)


@pytest.mark.parametrize("case,dt", _case_params())
def test_gemm_pair(dev, case, dt):
    """One launch of the audio + visual problem: fp64 per problem, the tile of PAIR_TILES, and bit-identity with two single
    launches forced to the reported tile and K split (not for fp32 atomics with a K split: their summation order is free)."""
    pc = PairCase(dev, case, dt)
    assert gemm_krot(False) == 0
    b = pc.buffers()
    if pc.epi == "qkv" and pc.h16:
        pc.vt_pad = b["v"][..., pc.S:].cpu().clone()
    d = pc.descs(b)
    ks = gemm_pair(*d)
    tile, ks_rec, k_rot = gemm_last()
    assert (tile, ks_rec, k_rot) == (pc.want_tile, ks, 0), (tile, ks_rec, k_rot)
    fused = pc.epi == "cross" and d[0]._q.fused()
    if pc.epi == "cross":
        assert d[1]._q.fused() == fused
        assert fused == (pc.want_tile == 27 and pc.h16)
    if pc.epi == "gate":
        if "ksplit" in pc.opts and pc.opts.get("g1_slabs", True):
            assert ks == pc.opts["ksplit"]
        if pc.opts.get("slabs") and pc.opts.get("g1_slabs", True) is False:
            assert ks == 1, "a pair whose second problem has no slabs must not split K"
    worst = []
    pc.check_reference(b, ks, fused, worst)
    record_parity(f"pair_gemm.{case}.{str(dt)[6:]}", rel_err=worst[0], tile=tile, ksplit=ks)
    if pc.p[0].ew:
        record_parity(f"elementwise.pair_gemm.{case}.{str(dt)[6:]}", err_over_bound=pc.ew_ratio, tile=tile, ksplit=ks)
    if fused:
        record_parity(f"elementwise.pair_gemm.cross_attn.{case}.{str(dt)[6:]}", err_over_bound=pc.ew_ratio, ambiguous_share=pc.amb_share, tile=tile)

    if pc.epi == "gate" and ks > 1 and not pc.opts.get("slabs"):
        return          # fp32 atomics: bit-identity not defined
    b1 = pc.buffers()
    s0, s1 = pc.descs(b1, tile=tile, ksplit=ks)
    for i, s in enumerate((s0, s1)):
        rt._check(_lib(), _lib().foley_op_gemm(C.byref(s), rt._stream()), "foley_op_gemm")
        t_i, ks_i, kr_i = gemm_last()
        assert (t_i, kr_i) == (tile, 0) and (pc.epi != "gate" or ks_i == ks), (i, t_i, ks_i, kr_i)
        if pc.epi == "cross":
            assert s._q.fused() == fused
    for i, (x, y) in enumerate(zip(pc.outputs(b, fused), pc.outputs(b1, fused))):
        assert _bits_equal(x, y), f"output {i}: the pair launch differs from its single launches"


# ----------------------------------------------------------------------------- K-origin rotation
# (name, epilogue, M, N, K, forced tile (0 = auto), options): small grids of the wave-specialised tiles whose M-tile count does not
# divide the slice count (K = 1408 = 22 slices over 4 M tiles, K = 1536 = 24 over 5).  Gated residual: the walk wraps inside each
# K range [k_lo, k_hi) (22 slices in 3 ranges of 7 / 7 / 8, 4 M tiles).
ROT_CASES = [
    ("store_25", "store", 500, 1536, 1408, 25, {}),
    ("gelu_15", "gelu", 500, 1536, 1408, 15, {}),
    ("gelu_29", "gelu", 1000, 1024, 1408, 29, {}),
    ("store_19", "store", 1000, 768, 1408, 19, {}),
    ("qkv_27", "qkv", 250, 768, 1408, 27, {"H": 2}),
    ("qkv_26", "qkv", 450, 768, 1536, 26, {"H": 2}),
    ("qkv_28", "qkv", 700, 768, 1408, 28, {"H": 2}),
    ("gate_25_ks3", "gate", 500, 1536, 1408, 25, {"ksplit": 3, "slabs": "h"}),
    ("gate_25_ks3_f32slabs", "gate", 500, 1536, 1408, 25, {"ksplit": 3, "slabs": "f32"}),
]
BM = {15: 128, 25: 128, 26: 96, 27: 64, 28: 192, 19: 256, 29: 256}


def _single_rot_run(dev, epi, A, W, b, dt, M, N, tile, opts, H, krot):
    """One launch with the rotation hook set to krot; returns (outputs, (tile, ksplit, k_rot))."""
    out = {}
    kw = dict(epilogue=EPI[epi], tile=tile)
    if epi == "store":
        out["o"] = _nan((M, N), dev, torch.float32)
        kw["out0"] = out["o"]
    elif epi == "gelu":
        out["o"] = _nan((M, N), dev, dt)
        kw["out0"] = out["o"]
    elif epi == "qkv":
        L, Bc = M, 1
        pitch = (L + 31) // 32 * 32
        q, k = _nan((Bc, H, L, 128), dev, dt), _nan((Bc, H, L, 128), dev, dt)
        v = _nan((Bc, H, 128, pitch), dev, dt)
        cos, sin = tables.rope_table(L + 1)
        g = (1 + 0.1 * _rand((128,), 4001)).to(dev)
        pos = torch.arange(L, dtype=torch.int32, device=dev)
        kw["qkv"] = rt.qkv_split_desc(L, H, [g, g, None], [pos, pos, None], [q, k, v], L, 0, 1e-6, cos.to(dev), sin.to(dev),
                                      vt_pitch=pitch)
        out.update(q=q, k=k, v=v)
        out["ref_args"] = (g.cpu(), cos, sin)
    else:
        x0 = _rand((M, N), 4002)
        out["x"] = x0.to(dev)
        out["slabs"] = _nan((8, M, N), dev, torch.float32 if opts["slabs"] == "f32" else dt)
        kw.update(out0=out["x"], rb=rt.rowbcast(_rand((N,), 4003).to(dev), 0), ksplit=opts["ksplit"], partials=out["slabs"])
    prev = gemm_krot(krot)
    try:
        rt.op_gemm(A, W, b, **kw)
        rec = gemm_last()
    finally:
        gemm_krot(prev)
    return out, rec


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,epi,M,N,K,tile,opts", ROT_CASES, ids=[c[0] for c in ROT_CASES])
def test_k_origin_rotation_single(dev, name, epi, M, N, K, tile, opts, dt):
    """Rotated K walk (GemmArgs::krot_ok, as run_forward sets it for single-clip forwards): k_rot reported, fp64 within the gate of the
    unrotated launch, M tile 0 (rotation 0) bit-identical to the unrotated launch, and the whole result within ROT_BOUND of it."""
    H = opts.get("H", 1)
    A = _rand((M, K), 4010).to(dt)
    W = _rand((N, K), 4011, 1 / math.sqrt(K)).to(dt)
    b = _rand((N,), 4012, 0.1)
    Ad, Wd, bd = A.to(dev), W.to(dev), b.to(dev)
    rot, rec_r = _single_rot_run(dev, epi, Ad, Wd, bd, dt, M, N, tile, opts, H, True)
    base, rec_b = _single_rot_run(dev, epi, Ad, Wd, bd, dt, M, N, tile, opts, H, False)
    assert rec_r[0] == tile and rec_r[2] == 1, rec_r
    assert rec_b == (tile, rec_r[1], 0), rec_b
    assert gemm_krot(False) == 0                        # the hook was restored
    y = A.double() @ W.double().t() + b.double()
    bm = BM[tile]
    if epi in ("store", "gelu"):
        ref = y if epi == "store" else F.gelu(y, approximate="tanh")
        pairs = [(rot["o"], base["o"])]
        for o in (rot["o"], base["o"]):   # fp32 results of 16-bit operands: test_gemm_linear's 16-bit gate
            assert rel_err(o.float(), ref) < _tol(dt)
        tile0 = [(rot["o"][:bm], base["o"][:bm])]
        outdt = torch.float32 if epi == "store" else dt
    elif epi == "qkv":
        g, cos, sin = rot["ref_args"]
        yy = y.view(M, 3, H, 128)
        c, s = cos[:M].double(), sin[:M].double()
        rq = _rope64(_rms64(yy[:, 0], g.double(), 1e-6), c, s)
        rk = _rope64(_rms64(yy[:, 1], g.double(), 1e-6), c, s)
        for o in (rot, base):
            assert rel_err(o["q"][0].transpose(0, 1).float(), rq) < QKV_TOL[dt]
            assert rel_err(o["k"][0].transpose(0, 1).float(), rk) < QKV_TOL[dt]
            assert rel_err(o["v"][0, :, :, :M].permute(2, 0, 1).float(), yy[:, 2]) < QKV_TOL[dt]
        pairs = [(rot[n], base[n]) for n in ("q", "k")] + [(rot["v"][..., :M], base["v"][..., :M])]
        tile0 = [(rot[n][:, :, :bm], base[n][:, :, :bm]) for n in ("q", "k")] + [(rot["v"][..., :bm], base["v"][..., :bm])]
        outdt = dt
    else:
        ks = rec_r[1]
        assert ks == opts["ksplit"]
        for o in (rot, base):
            assert torch.equal(o["x"].cpu(), _rand((M, N), 4002)), "residual touched by a deferred split-K launch"
            assert rel_err(o["slabs"][:ks].double().sum(0), y - b.double()) < SLAB_TOL[o["slabs"].dtype]
        pairs = [(rot["slabs"][:ks], base["slabs"][:ks])]
        tile0 = [(rot["slabs"][:ks, :bm], base["slabs"][:ks, :bm])]
        outdt = rot["slabs"].dtype
    for r, u in tile0:
        assert torch.equal(r, u), "M tile 0 (rotation 0) differs from the unrotated walk"
    d = max(rel_err(r.float(), u.float()) for r, u in pairs)
    record_parity(f"krot.single.{name}.{str(dt)[6:]}", rel_err_rot_vs_unrot=d, bound=ROT_BOUND[outdt])
    assert d < ROT_BOUND[outdt], d
    assert d > 0.0, "k_rot reported, but the rotated walk summed in the unrotated order"


ROT_PAIRS = [("gelu_xl", 25), ("qkv_xl", 26), ("cross_xl", 27), ("gate_xl", 25)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case,tile", ROT_PAIRS, ids=[c[0] for c in ROT_PAIRS])
def test_k_origin_rotation_pair(dev, case, tile, dt):
    """The rotated walk in the two-stream pair launches (xl width: 22 K slices over 4 - 8 M tiles of the audio problem): fp64 per
    problem, and M tile 0 of both problems (rotation 0) bit-identical to the unrotated pair.  The visual problem's 80 rows are one
    M tile, except on the 64-row tile 27 where its second tile rotates too."""
    pc = PairCase(dev, case, dt)
    runs = {}
    for on in (True, False):
        b = pc.buffers()
        if pc.epi == "qkv":
            pc.vt_pad = b["v"][..., pc.S:].cpu().clone()
        d = pc.descs(b)
        prev = gemm_krot(on)
        try:
            ks = gemm_pair(*d)
            rec = gemm_last()
        finally:
            gemm_krot(prev)
        assert rec[0] == tile and rec[2] == (1 if on else 0), rec
        fused = pc.epi == "cross" and d[0]._q.fused()
        assert fused == (pc.epi == "cross")
        worst = []
        pc.check_reference(b, ks, fused, worst)
        runs[on] = (b, ks)
    (br, ks_r), (bu, ks_u) = runs[True], runs[False]
    assert ks_r == ks_u
    bm = BM[tile]
    P0, P1 = pc.p
    if pc.epi == "gelu":
        tile0 = [(br["out"][i][:bm], bu["out"][i][:bm]) for i in range(2)]
        pairs = [(br["out"][i], bu["out"][i]) for i in range(2)]
    elif pc.epi == "qkv":   # rows of M tile 0 are tokens [tok_off, tok_off + bm) of clip 0 (Bc = 2: clip 0 holds the first L rows)
        assert P1.M <= bm
        sl = slice(P0.tok_off, P0.tok_off + bm)
        tile0 = [(br[n][0, :, sl], bu[n][0, :, sl]) for n in ("q", "k")] + [(br["v"][0, ..., sl], bu["v"][0, ..., sl])]
        tile0 += [(br[n][:, :, :P0.tok_off], bu[n][:, :, :P0.tok_off]) for n in ("q", "k")]
        pairs = [(br[n], bu[n]) for n in ("q", "k")] + [(br["v"][..., :pc.S], bu["v"][..., :pc.S])]
    elif pc.epi == "cross":
        tile0 = [(br["att"][i][:bm], bu["att"][i][:bm]) for i in range(2)]
        pairs = [(br["att"][i], bu["att"][i]) for i in range(2)]
    else:
        tile0 = [(br["slabs"][i][:ks_r, :bm], bu["slabs"][i][:ks_r, :bm]) for i in range(2)]
        pairs = [(br["slabs"][i][:ks_r], bu["slabs"][i][:ks_r]) for i in range(2)]
    for i, (r, u) in enumerate(tile0):
        assert _bits_equal(r, u), f"{i}: unrotated rows differ between the rotated and the unrotated pair"
    outdt = pairs[0][0].dtype
    d = max(rel_err(r.float(), u.float()) for r, u in pairs)
    record_parity(f"krot.pair.{case}.{str(dt)[6:]}", rel_err_rot_vs_unrot=d, bound=ROT_BOUND[outdt])
    assert d < ROT_BOUND[outdt], d


# ----------------------------------------------------------------------------- LayerNorm (+ pending split-K) at the DiT's width
LN_TOL = {torch.float32: 1e-4, torch.bfloat16: 4e-3, torch.float16: 5e-4}   # vs fp64 from the same fp32 inputs, rows ~ 1e3 + N(0, 1)
# two kernel forms on the same rows (different reduction orders): fp32 round-off of |x| ~ 1e3 against a unit standard deviation
LN_FORM_BOUND = 2.0 ** -23 * 1e3


def _ln_inputs(dev, M, D, seed, odt, k, slab, tok):
    """x rows of 1e3 + N(0, 1) (a one-pass variance or a bad Chan combination fails here), shift / scale / gate rows (per (cfg,
    token) with tok, else vectors), k pending slabs.  Made on the device; the fp64 reference reads the sampled rows."""
    gd = torch.Generator(device=dev).manual_seed(seed)
    rows = _sample_rows(M) if M > 0 else torch.arange(0)
    s = {"M": M, "D": D, "rows": rows, "x0": 1e3 + torch.randn(M, D, device=dev, generator=gd)}
    if tok and M > 0 and M % 2 == 0:
        L = M // 2
        tab = torch.randn(2, L, 3 * D, device=dev, generator=gd) * 0.3
        s["op"] = [rt.rowbcast(tab[..., c * D:], 1, L, L, ld=3 * D) for c in range(3)]
        cfg, li = (rows // L).to(dev), (rows % L).to(dev)
        s["full"] = [tab[cfg, li, c * D:(c + 1) * D].double().cpu() for c in range(3)]
    else:
        vec = torch.randn(3, D, device=dev, generator=gd) * 0.3
        s["op"] = [rt.rowbcast(vec[c], 0) for c in range(3)]
        s["full"] = [vec[c].double().cpu().expand(len(rows), D) for c in range(3)]
    if k:
        sdt = torch.float32 if (slab == "f32" or odt == torch.float32) else odt   # 16-bit slabs carry the output type
        s["slabs"] = (torch.randn(k, M, D, device=dev, generator=gd) * 0.5).to(sdt)
        s["bias"] = torch.randn(D, device=dev, generator=gd) * 0.1
    return s


def _ln_ref(s, eps=1e-6):
    rd = s["rows"].to(s["x0"].device)
    x = s["x0"][rd].double().cpu()
    if "slabs" in s:
        x = x + s["full"][2] * (s["slabs"][:, rd].double().sum(0).cpu() + s["bias"].double().cpu())
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return x, (x - mu) / torch.sqrt(var + eps) * (1 + s["full"][1]) + s["full"][0]


def _ln_dev(s, odt):
    """Device arguments of one row set: a fresh copy of x and a NaN output."""
    a = {"M": s["M"], "x": s["x0"].clone(), "out": _nan((s["M"], s["D"]), s["x0"].device, odt), "shift": s["op"][0],
         "scale": s["op"][1]}
    if "slabs" in s:
        a.update(partials=s["slabs"], k=s["slabs"].shape[0], bias=s["bias"], gate=s["op"][2])
    return a


def _ln_check(s, a, odt, tag):
    if s["M"] == 0:
        return 0.0
    xr, ref = _ln_ref(s)
    rd = s["rows"].to(a["x"].device)
    assert bool(torch.isfinite(a["out"]).all()), f"{tag}: output rows left unwritten"
    if "slabs" in s:   # written back in place: x + gate * (sum + bias), to fp32 round-off
        x = a["x"][rd].double().cpu()
        assert bool(((x - xr).abs() <= 1e-5 + 5e-7 * xr.abs()).all()), f"{tag}: x written back wrong"
    else:
        assert torch.equal(a["x"], s["x0"]), f"{tag}: x changed without pending work"
    e = rel_err(a["out"][rd].float(), ref)
    assert e < LN_TOL[odt], (tag, e)
    return e


def _ln_single(a):
    if "partials" in a:
        rt.op_ln_mod_pending(a["x"], 1e-6, a["shift"], a["scale"], a["out"], a["partials"], a["k"], a["bias"], a["gate"])
    else:
        rt.op_ln_mod(a["x"], 1e-6, a["shift"], a["scale"], a["out"])


ODT = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("odt", ODT, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("M,D", [(500, 1536), (4096, 1536), (4097, 1536), (6000, 1536), (500, 1408)])
@pytest.mark.parametrize("k,slab", [(0, None), (1, "f32"), (2, "h"), (6, "f32"), (7, "h"), (8, "f32"), (8, "h")])
def test_ln_mod_width(dev, M, D, odt, k, slab):
    """LayerNorm(x + gate * (sum of k slabs + bias)) * (1 + scale) + shift at D = 1536: the two-wave kernel up to 4096 rows, the
    one-wave MAXV 6 kernel above (and always at D = 1408); k = 7 / 8 take a second batch of SB = 6 slabs.  Per-token operands
    for even k, vectors for odd k; 16-bit slabs ("h") in the output's type (fp32 for an fp32 output)."""
    s = _ln_inputs(dev, M, D, 5000 + k, odt, k, slab, tok=(k % 2 == 0))
    a = _ln_dev(s, odt)
    _ln_single(a)
    e = _ln_check(s, a, odt, "single")
    record_parity(f"ln_width.M{M}.D{D}.k{k}{slab or ''}.{str(odt)[6:]}", rel_err=e)


LN_PAIRS = [(500, 80), (3000, 480), (7, 1), (0, 80), (4000, 640)]


@pytest.mark.parametrize("odt", ODT, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("M0,M1", LN_PAIRS)
@pytest.mark.parametrize("pend", ["first", "second", "both", "none"])
def test_ln_mod_pair(dev, M0, M1, pend, odt):
    """launch_ln_mod_pair over the audio and visual row sets, pending slabs on either, both or neither: fp64 per set, and the pair
    bit-identical to its two single launches where they take the same kernel form (total rows <= 4096: the two-wave kernel).
    (4000, 640) totals 4640 rows - the one-wave kernel - while its singles take the two-wave one: fp32 round-off apart."""
    D = 1536
    ks = {"first": (3, 0), "second": (0, 7), "both": (2, 8), "none": (0, 0)}[pend]
    sets = [_ln_inputs(dev, M, D, 6000 + 10 * i, odt, ks[i], "h", tok=(i == 0)) for i, M in enumerate((M0, M1))]
    a = [_ln_dev(s, odt) for s in sets]
    ln_mod_pair(a, D, 1e-6, rt.dt_of(a[0]["out"]))
    worst = max(_ln_check(s, ai, odt, f"pair set {i}") for i, (s, ai) in enumerate(zip(sets, a)))
    record_parity(f"ln_pair.{M0}+{M1}.{pend}.{str(odt)[6:]}", rel_err=worst)
    singles = [_ln_dev(s, odt) for s in sets]
    for sg in singles:
        if sg["M"] > 0:
            _ln_single(sg)
    same_form = (M0 + M1 <= 4096) == all(M <= 4096 for M in (M0, M1))
    for i, (p, sg) in enumerate(zip(a, singles)):
        if sets[i]["M"] == 0:
            continue
        if same_form:
            assert torch.equal(p["out"], sg["out"]) and torch.equal(p["x"], sg["x"]), f"set {i}: pair != single launch"
        else:
            assert rel_err(p["x"], sg["x"]) < 1e-7
            e = rel_err(p["out"].float(), sg["out"].float())
            record_parity(f"ln_pair_vs_single_form.{M0}+{M1}.{pend}.{str(odt)[6:]}.set{i}", rel_err=e)
            assert e < (LN_FORM_BOUND if odt == torch.float32 else LN_TOL[odt]), e
