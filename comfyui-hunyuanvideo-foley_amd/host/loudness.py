"""Loudness and true-peak output stage on the HIP engine: the ITU-R BS.1770-4 meter, a static gain to a target loudness and a
look-ahead true-peak limiter.  The reference does none of this; the sampler hands back the raw DAC-VAE output.

Everything runs on libfoley_hip.so, on the waveform where the decode left it:
  * foley_op_loudness_energy   K-weighting (two biquads, fp64 state) and the energy of every 100 ms hop, chunk-parallel;
  * foley_op_loudness_gate     400 ms blocks, the -70 LUFS and the relative -10 LU gate, the integrated loudness;
  * foley_op_true_peak         the 4x oversampled peak envelope (the method of BS.1770 Annex 2) and its maximum;
  * foley_op_loudness_apply    y = G x, or the limiter: r = min(1, c / (G p)), sliding minimum, box mean, one multiply.
The K-weighting coefficients are the Recommendation's 48 kHz ones, so other rates are refused.  The oversampling taps are OURS
(a Kaiser-windowed sinc, below) - the method is the Annex's, its coefficient table is not reproduced here.  The chunk transition
matrix and the taps are built here in fp64.  There is no fallback: CPU tensors raise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import runtime as rt

Tensor = torch.Tensor

SAMPLE_RATE = 48000
HOP, CHUNK = 4800, 480                      # 100 ms hop; the kernels' chunk (a tenth of a hop)
MAX_LOOKAHEAD = 480                         # 10 ms
LIMITER_TILE = 1024                         # output samples per workgroup of the limiter (csrc/loudness.hip TP_TILE)
# ITU-R BS.1770-4 table 1 / table 2 (48 kHz), a0 = 1: (b0, b1, b2, a1, a2)
K_STAGES = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
            (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))


# ----------------------------------------------------------------------------- host-built tables
def state_matrix() -> Tensor:
    """One zero-input sample step of the cascade over the transposed-direct-form-II state (s1, s2 | t1, t2): [4, 4] fp64.
    y1 = s1; s1' = -a1 y1 + s2; s2' = -a2 y1; y2 = B0 y1 + t1; t1' = B1 y1 - A1 y2 + t2; t2' = B2 y1 - A2 y2."""
    (_b0, _b1, _b2, a1, a2), (B0, B1, B2, A1, A2) = K_STAGES
    return torch.tensor([[-a1, 1.0, 0.0, 0.0],
                         [-a2, 0.0, 0.0, 0.0],
                         [B1 - A1 * B0, 0.0, -A1, 1.0],
                         [B2 - A2 * B0, 0.0, -A2, 0.0]], dtype=torch.float64)


def chunk_transition(chunk: int = CHUNK) -> Tensor:
    """T = A^chunk: the state a chunk's initial state leaves at its end; by linearity end = T s0 + (end from zero state).
    The high-pass stage has a double pole at radius 0.995 next to z = 1: its state entries reach 44 and nearly cancel, and an
    fp64 matrix power loses five digits there.  The power is therefore taken in exact rational arithmetic over the fp64
    coefficients and rounded once."""
    from fractions import Fraction
    A = [[Fraction(v) for v in row] for row in state_matrix().tolist()]
    mul = lambda X, Y: [[sum(X[i][k] * Y[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    P = [[Fraction(int(i == j)) for j in range(4)] for i in range(4)]
    n = int(chunk)
    while n:
        if n & 1:
            P = mul(P, A)
        A = mul(A, A)
        n >>= 1
    return torch.tensor([[float(v) for v in row] for row in P], dtype=torch.float64)


def true_peak_prototype() -> Tensor:
    """h[k], k = -24 .. 24 (index k + 24): sinc(k / 4) * kaiser(49, beta 8), fp64."""
    k = torch.arange(-24, 25, dtype=torch.float64)
    return torch.sinc(k / 4.0) * torch.kaiser_window(49, periodic=False, beta=8.0, dtype=torch.float64)


def true_peak_taps() -> Tensor:
    """[3, 12] fp64: row r - 1, column j + 5 = h[r - 4 j] for j = -5 .. 6, every phase scaled to sum to 1 (phase 0 of the
    prototype is the identity and is not stored).  u[4 n + r] = sum_j x[n + j] * taps[r - 1, j + 5]."""
    h = true_peak_prototype()
    rows = []
    for r in (1, 2, 3):
        row = torch.stack([h[r - 4 * j + 24] for j in range(-5, 7)])
        rows.append(row / row.sum())
    return torch.stack(rows)


_T: Optional[Tensor] = None
_TAPS32: Optional[Tensor] = None


def _tables() -> Tuple[Tensor, Tensor]:
    global _T, _TAPS32
    if _T is None:
        _T, _TAPS32 = chunk_transition(), true_peak_taps().to(torch.float32)
    return _T, _TAPS32


# ----------------------------------------------------------------------------- public API
@dataclass
class LoudnessResult:
    """lufs [B] integrated loudness (fp64, -inf: silent), true_peak_dbtp / sample_peak_dbfs [B], silent [B] bool - CPU tensors
    from the one device-to-host read; block_lufs [B, nb] the 400 ms block loudnesses, left on the device; gain_db [B] the static
    gain normalize() applied (set on its `before` result only)."""
    lufs: Tensor
    true_peak_dbtp: Tensor
    sample_peak_dbfs: Tensor
    block_lufs: Tensor
    silent: Tensor
    gain_db: Optional[Tensor] = None


def _check_wave(waveform: Tensor, sample_rate: int) -> Tensor:
    if int(sample_rate) != SAMPLE_RATE:
        raise ValueError(f"the loudness stage runs at {SAMPLE_RATE} Hz (the BS.1770 coefficients are the 48 kHz ones); got {sample_rate}")
    wav = waveform.unsqueeze(1) if waveform.dim() == 2 else waveform
    if wav.dim() != 3:
        raise ValueError("waveform must be [B, C, N] or [B, N]")
    if wav.shape[1] > 2:
        raise ValueError(f"the loudness stage takes mono or stereo (channel weights 1.0); got {wav.shape[1]} channels")
    return wav


def _db(x: Tensor) -> Tensor:
    return 20.0 * torch.log10(x.to(torch.float64))


def _measure(wav: Tensor) -> LoudnessResult:
    if not wav.is_cuda:
        raise rt.FoleyRuntimeError("the loudness stage runs on the HIP engine: the waveform must be on the GPU")
    T, taps = _tables()
    wav = wav.to(torch.float32)
    if wav.stride(2) != 1:
        wav = wav.contiguous()
    e = rt.op_loudness_energy(wav, T)
    lufs, _gamma, blocks = rt.op_loudness_gate(e)
    tp, sp, _ = rt.op_true_peak(wav, taps)
    host = torch.stack((lufs, tp.to(torch.float64), sp.to(torch.float64))).cpu()          # the one device-to-host read
    return LoudnessResult(lufs=host[0], true_peak_dbtp=_db(host[1]), sample_peak_dbfs=_db(host[2]), block_lufs=blocks,
                          silent=torch.isinf(host[0]))


@torch.inference_mode()
def measure(waveform: Tensor, sample_rate: int) -> LoudnessResult:
    """Integrated loudness (LUFS, BS.1770-4 gating), true peak (dBTP, 4x oversampling) and sample peak (dBFS) of every clip of
    waveform [B, C, N] or [B, N] (C 1 or 2) at 48 kHz, on the device."""
    return _measure(_check_wave(waveform, sample_rate))


def lookahead_samples(lookahead_ms: float) -> int:
    W = int(round(48.0 * float(lookahead_ms)))
    if not 1 <= W <= MAX_LOOKAHEAD:
        raise ValueError(f"lookahead_ms gives {W} samples: the limiter looks 1 .. {MAX_LOOKAHEAD} samples ahead (up to 10 ms)")
    return W


def check_args(target_lufs: float, true_peak_dbtp: float = -1.0, limiter: bool = False, lookahead_ms: float = 5.0) -> int:
    """The refusals of normalize() that need no waveform; returns the look-ahead in samples."""
    if not float(target_lufs) <= 0.0:
        raise ValueError(f"target_lufs must be <= 0 LUFS, got {target_lufs}")
    if not float(true_peak_dbtp) <= 0.0:
        raise ValueError(f"true_peak_dbtp is a ceiling <= 0 dBTP, got {true_peak_dbtp}")
    return lookahead_samples(lookahead_ms)


def static_gain(lufs: Tensor, true_peak_dbtp_measured: Tensor, target_lufs: float, ceiling_dbtp: float, limiter: bool):
    """(gain_db [B] fp64, gain [B] fp32 linear with 0 for silent clips): target - L, in gain-only mode held under the ceiling."""
    g_db = float(target_lufs) - lufs.to(torch.float64)
    if not limiter:
        g_db = torch.minimum(g_db, float(ceiling_dbtp) - true_peak_dbtp_measured.to(torch.float64))
    silent = torch.isinf(lufs)
    g_db = torch.where(silent, torch.zeros_like(g_db), g_db)
    gain = torch.pow(10.0, g_db / 20.0).to(torch.float32)
    return g_db, torch.where(silent, torch.zeros_like(gain), gain)


@torch.inference_mode()
def normalize(audio_batch: dict, target_lufs: float = -16.0, true_peak_dbtp: float = -1.0, limiter: bool = False,
              lookahead_ms: float = 5.0):
    """Bring every clip of an AUDIO dict ({'waveform': [B, C, N] or [B, N] on the GPU, 'sample_rate': 48000}) to `target_lufs`,
    each on its own.  limiter=False: one static gain per clip, lowered where the true peak would pass the ceiling.
    limiter=True: the full gain, then a look-ahead limiter (lookahead_ms, at most 10) holds the peak envelope under the ceiling;
    the loudness it takes is not won back.  A silent clip (-inf LUFS) is returned unchanged.  Returns (AUDIO dict, before, after):
    the measurements before and after (re-measured); before.gain_db is the static gain applied."""
    W = check_args(target_lufs, true_peak_dbtp, limiter, lookahead_ms)
    waveform = audio_batch["waveform"]
    wav = _check_wave(waveform, audio_batch["sample_rate"])
    before = _measure(wav)
    g_db, gain = static_gain(before.lufs, before.true_peak_dbtp, target_lufs, true_peak_dbtp, limiter)
    before.gain_db = g_db
    wav32 = wav.to(torch.float32)
    if wav32.stride(2) != 1:
        wav32 = wav32.contiguous()
    y = rt.op_loudness_apply(wav32, gain.to(wav.device), limiter=bool(limiter), ceiling=10.0 ** (float(true_peak_dbtp) / 20.0),
                             lookahead=W, taps=_tables()[1] if limiter else None)
    after = _measure(y)
    out = y.view(waveform.shape) if waveform.dim() == 2 else y
    return {"waveform": out, "sample_rate": audio_batch["sample_rate"]}, before, after
