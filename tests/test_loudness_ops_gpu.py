"""The loudness kernels (csrc/loudness.hip) at op level against the fp64 restatement (tests/loudness_ref.py): K-weighted hop
energies, the gate, the true-peak envelope and the limiter, at the smallest shapes where they can go wrong."""
import math

import numpy as np
import pytest
import torch

from conftest import record_parity
from foley_amd.host import loudness as L, runtime as rt
import loudness_ref as LR

pytestmark = pytest.mark.gpu
FS = 48000
U32 = 2.0 ** -24
ABS_FLOOR = 10.0 ** ((-100.0 + 0.691) / 10.0) * 4800          # the energy of one hop of one channel at -100 LUFS

ENERGY_N = (479, 480, 481, 4799, 4800, 19199, 19200, 19201, 24037)
_CACHE = {}


def _program(B, C, N, seed, lo_db=-50.0):
    """White noise (sigma 0.1) + 50 Hz hum (0.2) + DC (0.05) - the hum and the DC load the slow poles - scaled per clip to
    between -50 and -6 dBFS: [B, C, N] fp32."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    x = 0.1 * rng.standard_normal((B, C, N)) + 0.2 * np.sin(2 * np.pi * 50 * n / FS) + 0.05
    scale = 10.0 ** (np.linspace(lo_db, -6.0, B) / 20.0) if B > 1 else np.array([10.0 ** (-20.0 / 20.0)])
    return (x * scale[:, None, None]).astype(np.float32)


def _energy_cases():
    """Every energy input with its sequential fp64 energies and the reordering floor: the largest relative distance, per hop,
    between the sequential filter and its chunked restatement (the kernel's chunk length and summation order), over all cases."""
    if "energy" not in _CACHE:
        T = L.chunk_transition().numpy()
        cases = {("mono", N): _program(1, 1, N, N) for N in ENERGY_N}
        cases[("pitched", 52923)] = _program(3, 2, 52923, 7)
        seq = {k: LR.hop_energies(x) for k, x in cases.items()}
        floor = 0.0
        for k, x in cases.items():
            if seq[k].size:
                floor = max(floor, float((np.abs(LR.hop_energies_chunked(x, T) - seq[k]) / seq[k]).max()))
        _CACHE["energy"] = (cases, seq, floor)
    return _CACHE["energy"]


def _dev_wave(x, dev, pitch=None):
    """[B, C, N] on the device; with `pitch` a view into a longer, NaN-filled buffer (row pitch > N)."""
    t = torch.from_numpy(x)
    if pitch is None:
        return t.to(dev)
    buf = torch.full((x.shape[0], x.shape[1], pitch), float("nan"), dtype=torch.float32)
    buf[..., :x.shape[2]] = t
    return buf.to(dev)[..., :x.shape[2]]


# ----------------------------------------------------------------------------- energies
@pytest.mark.parametrize("key", [("mono", N) for N in ENERGY_N] + [("pitched", 52923)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_hop_energies(dev, key):
    cases, seq, floor = _energy_cases()
    x, want = cases[key], seq[key]
    xd = _dev_wave(x, dev, pitch=53000 if key[0] == "pitched" else None)
    T = L.chunk_transition()
    e = rt.op_loudness_energy(xd, T)
    assert e.dtype == torch.float64 and tuple(e.shape) == want.shape == (x.shape[0], x.shape[1], x.shape[2] // 4800)
    e2 = rt.op_loudness_energy(xd, T)
    assert torch.equal(e, e2)                                                  # no atomics: the same bits
    if not want.size:
        return
    got = e.cpu().numpy()
    err = float((np.abs(got - want) / want).max())
    print(f"{key}: kernel vs sequential fp64 {err:.3e} relative per hop, reordering floor {floor:.3e}")
    record_parity(f"loudness_energy_{key[0]}_{key[1]}", err=err, d0=floor, ratio=err / floor)
    assert (np.abs(got - want) <= 4 * floor * want + ABS_FLOOR).all()


# ----------------------------------------------------------------------------- gate
def _tone_steps():
    """Mono, 1 kHz: 1 s at -80, 1 s at -40, 2 s at -20, 1 s at -40 dBFS."""
    n = np.arange(5 * FS)
    lev = np.repeat([-80.0, -40.0, -20.0, -20.0, -40.0], FS)
    return (10.0 ** (lev / 20.0) * np.sin(2 * np.pi * 1000 * n / FS)).astype(np.float32)[None, None]


def _gate_margin(res):
    l = res["block_lufs"]
    l = l[np.isfinite(l)]
    return float(min(np.abs(l + 70.0).min(), np.abs(l - res["gamma"]).min()))


def _lufs_tol(floor, value):
    """The energy gate carried through the logarithm: every z within (1 + eps) relative, so is a mean of them, and 10 log10 of it
    moves by 10 log10(1 + eps); the fp64 log and the few operations around it add some ulps of the value."""
    return 10.0 * math.log10(1.0 + 4 * floor) + 16 * 2.0 ** -52 * max(1.0, abs(value))


def test_gate_on_the_tone_steps(dev):
    _c, _s, floor = _energy_cases()
    x = _tone_steps()
    res = LR.gate(LR.hop_energies(x)[0])
    assert len(res["z"]) == 47 and res["n_abs"] == 40 and res["n_rel"] == 23 and abs(res["lufs"] - (-23.604)) < 5e-4
    assert _gate_margin(res) > 0.01                                            # no block sits where a rounding could flip it
    e = rt.op_loudness_energy(torch.from_numpy(x).to(dev), L.chunk_transition())
    lufs, gamma, blocks = rt.op_loudness_gate(e)
    lufs, gamma, blocks = float(lufs.cpu()[0]), float(gamma.cpu()[0]), blocks.cpu().numpy()[0]
    print(f"tone steps: L {lufs:.6f} (oracle {res['lufs']:.6f}), gamma {gamma:.6f} (oracle {res['gamma']:.6f}), margin {_gate_margin(res):.2f} LU")
    assert abs(lufs - res["lufs"]) <= _lufs_tol(floor, lufs) and abs(gamma - res["gamma"]) <= _lufs_tol(floor, gamma)
    loud = res["block_lufs"] > -70.0
    assert blocks.shape == (47,) and (np.abs(blocks - res["block_lufs"])[loud] <= _lufs_tol(floor, 70.0)).all()
    assert (blocks[~loud] < -70.0).all()
    record_parity("loudness_gate_tone_steps", err=abs(lufs - res["lufs"]), d0=_lufs_tol(floor, lufs), ratio=abs(lufs - res["lufs"]) / _lufs_tol(floor, lufs))


def test_gate_stereo_batch_through_measure(dev):
    _c, _s, floor = _energy_cases()
    x = _program(3, 2, 52923, 11, lo_db=-40.0)                                  # the quietest clip stays clear of the -70 gate
    m = L.measure(_dev_wave(x, dev, pitch=53000), FS)
    assert m.lufs.dtype == torch.float64 and m.block_lufs.is_cuda and tuple(m.block_lufs.shape) == (3, 8)
    seq = LR.hop_energies(x)
    for b in range(3):
        res = LR.gate(seq[b])
        assert _gate_margin(res) > 0.01
        assert abs(float(m.lufs[b]) - res["lufs"]) <= _lufs_tol(floor, res["lufs"])
    assert not m.silent.any()


def test_silent_and_too_short_clips(dev):
    m = L.measure(torch.zeros(2, 1, 24000, device=dev), FS)
    assert (m.lufs == -math.inf).all() and m.silent.all() and (m.true_peak_dbtp == -math.inf).all()
    x = _tone_steps()[..., :19199]
    m = L.measure(torch.from_numpy(x).to(dev), FS)                             # three hops: no block
    assert float(m.lufs[0]) == -math.inf and bool(m.silent[0]) and tuple(m.block_lufs.shape) == (1, 0)
    m = L.measure(torch.from_numpy(x[0]).to(dev), FS)                          # [B, N] is [B, 1, N]
    assert float(m.lufs[0]) == -math.inf and math.isfinite(float(m.true_peak_dbtp[0]))


# ----------------------------------------------------------------------------- true peak
def _fs4(N):
    n = np.arange(N)
    x = 0.5 * np.sin(2 * np.pi * 12000 * n / FS + np.pi / 4)
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(480) / 480)
    x[:480] *= ramp
    x[-480:] *= ramp[::-1]
    return x.astype(np.float32)[None]


def _noise(C, N, seed=3):
    return (0.3 * np.random.default_rng(seed).standard_normal((C, N))).astype(np.float32)


def _impulses(N):
    x = np.zeros((1, N), dtype=np.float32)
    x[0, 0] = x[0, N - 1] = 1.0
    return x


@pytest.mark.parametrize("name,x", [("fs4", _fs4(2500)), ("noise", _noise(1, 2500)), ("impulses", _impulses(2049)),
                                    ("stereo", _noise(2, 1025, seed=4)), ("short", _noise(2, 3, seed=5))], ids=lambda v: v if isinstance(v, str) else "")
def test_true_peak_envelope(dev, name, x):
    p, bound = LR.envelope(x)
    xd = _dev_wave(x[None], dev, pitch=x.shape[1] + 13 if name == "stereo" else None)
    tp, sp, env = rt.op_true_peak(xd, L.true_peak_taps().to(torch.float32), with_envelope=True)
    env_h = env.cpu().numpy()[0].astype(np.float64)
    err = np.abs(env_h - p)
    print(f"{name}: envelope error / bound max {float((err / np.maximum(bound, 1e-300)).max()):.3f}, true peak {LR.db(float(tp.cpu()[0])):.3f} dBTP")
    assert (err <= bound).all()
    assert float(tp.cpu()[0]) == float(env.max().cpu()) and float(sp.cpu()[0]) == float(np.abs(x).max())    # a maximum is exact
    tp2, _sp, _e = rt.op_true_peak(xd, L.true_peak_taps().to(torch.float32), with_sample_peak=False)
    assert _sp is None and _e is None and torch.equal(tp, tp2)
    if name == "fs4":
        assert -6.4 <= LR.db(float(tp.cpu()[0])) <= -5.8
    if name == "impulses":
        assert float(tp.cpu()[0]) == 1.0


# ----------------------------------------------------------------------------- limiter
CEIL = 10.0 ** (-1.0 / 20.0)
GAIN = float(np.float32(3.7))


def _limiter_input(N, C, seed):
    rng = np.random.default_rng(seed)
    x = (0.04 * rng.standard_normal((C, N))).astype(np.float32)
    for at in (0, N - 1, N // 2, N // 2 + min(5, N // 4)):                      # the ends, and two peaks closer than any W used
        x[0, at] = 0.9                                                         # the peaks sit in channel 0 only
    return x


@pytest.mark.parametrize("N,W,C", [(L.LIMITER_TILE - 1, 240, 1), (L.LIMITER_TILE, 240, 1), (L.LIMITER_TILE + 1, 240, 1),
                                   (L.LIMITER_TILE - 1, 7, 1), (L.LIMITER_TILE, 7, 1), (L.LIMITER_TILE + 1, 7, 2),
                                   (100, 240, 1), (2500, 240, 2), (2500, 480, 1)])
def test_limiter(dev, N, W, C):
    x = _limiter_input(N, C, seed=N + W)
    taps = L.true_peak_taps().to(torch.float32)
    xd = torch.from_numpy(np.stack([x, x])).to(dev)                           # clip 1 carries gain 0: passed through
    gain = torch.tensor([GAIN, 0.0], device=dev)
    y, g = rt.op_loudness_apply(xd, gain, limiter=True, ceiling=CEIL, lookahead=W, taps=taps, with_gain_curve=True)
    y_gain = rt.op_loudness_apply(xd, gain)
    assert torch.equal(y[1], xd[1]) and torch.equal(y_gain[1], xd[1]) and bool((g[1] == 1).all())
    assert torch.equal(y_gain[0].cpu(), torch.from_numpy(x) * torch.tensor(GAIN, dtype=torch.float32))       # fl32(G) * x, exactly
    g_h = g[0].cpu().numpy().astype(np.float64)
    # (a) against the oracle: r within [r_lo, r_hi] for an envelope within its bound (the device rounds r down: one more ulp), g is
    # monotone in r, and the fp32 box mean of W + 1 terms and its division err by at most (W + 2) * 2^-24 relative
    p, bound = LR.envelope(x)
    r_lo = LR.reduction(p + bound, GAIN, CEIL) * (1 - 2.0 ** -22)
    r_hi = LR.reduction(np.maximum(p - bound, 0.0), GAIN, CEIL)
    g_lo, g_hi = LR.gain_curve(r_lo, W), LR.gain_curve(r_hi, W)
    slack = (W + 2) * U32
    assert (g_h >= g_lo * (1 - slack)).all() and (g_h <= g_hi * (1 + slack)).all()
    g_ref, r_ref = LR.limiter_gain(p, GAIN, CEIL, W)
    print(f"N {N} W {W} C {C}: max |g - oracle| {float(np.abs(g_h - g_ref).max()):.3e}, min g {g_h.min():.4f}")
    assert (r_ref < 1).any()
    # (b) the three properties on the device's own envelope and gain
    _tp, _sp, env = rt.op_true_peak(xd[:1], taps, with_envelope=True)
    p_d = env[0].cpu().numpy().astype(np.float64)
    r_d = LR.reduction(p_d, GAIN, CEIL)
    assert (g_h <= r_d).all()
    assert (GAIN * g_h * p_d <= CEIL * (1 + 2.0 ** -50)).all()
    free = LR.untouched(r_d, W)
    assert (g_h[free] == 1.0).all() and (g_h < 1.0).any()
    # (c) where nothing was touched the output is the gain-only output, bit for bit; elsewhere y = (G g) x in fp32
    free_t = torch.from_numpy(free)
    assert torch.equal(y[0].cpu()[:, free_t], y_gain[0].cpu()[:, free_t])
    if W < N // 4:
        assert free.any() and not free.all()
    want = (torch.tensor(GAIN, dtype=torch.float32) * g[0].cpu())[None] * torch.from_numpy(x)
    assert torch.equal(y[0].cpu(), want)
    y2, g2 = rt.op_loudness_apply(xd, gain, limiter=True, ceiling=CEIL, lookahead=W, taps=taps, with_gain_curve=True)
    assert torch.equal(y, y2) and torch.equal(g, g2)


def test_normalize_gain_only_and_limiter(dev):
    """normalize() on two tones of different level: gain-only lands on the target (the oracle reads it on the output), the
    limiter's re-measured true peak is recorded next to the ceiling."""
    _c, _s, floor = _energy_cases()
    n = np.arange(2 * FS)
    x = np.stack([0.05 * np.sin(2 * np.pi * 440 * n / FS), 0.3 * np.sin(2 * np.pi * 997 * n / FS)]).astype(np.float32)[:, None]
    out, before, after = L.normalize({"waveform": torch.from_numpy(x).to(dev), "sample_rate": FS}, target_lufs=-20.0)
    for b in range(2):
        l0 = LR.integrated_loudness(x[b])
        assert abs(float(before.lufs[b]) - l0) <= _lufs_tol(floor, l0)
        assert abs(float(before.gain_db[b]) - (-20.0 - l0)) <= _lufs_tol(floor, l0)
        got = LR.integrated_loudness(out["waveform"][b].cpu().numpy())
        # the gain is rounded to fp32 once and every product once more: at most (1 + 2^-24)^2 on the amplitude
        assert abs(got - (-20.0)) <= 2 * _lufs_tol(floor, l0) + 40 * math.log10(1 + U32)
        assert abs(float(after.lufs[b]) - got) <= _lufs_tol(floor, got)
    hot = _limiter_input(24000, 1, seed=9)[None] * np.float32(0.5)
    out, before, after = L.normalize({"waveform": torch.from_numpy(hot).to(dev), "sample_rate": FS}, target_lufs=-14.0, limiter=True)
    tp_ref = LR.db(LR.true_peak(out["waveform"][0].cpu().numpy()))
    print(f"planted peaks: gain {float(before.gain_db[0]):.2f} dB, true peak before {float(before.true_peak_dbtp[0]):.3f}, after "
          f"{float(after.true_peak_dbtp[0]):.3f} dBTP (oracle on the output {tp_ref:.3f}) under -1.0; loudness after {float(after.lufs[0]):.3f}")
    record_parity("loudness_limiter_planted_peaks", true_peak_after_dbtp=float(after.true_peak_dbtp[0]), ceiling_dbtp=-1.0,
                  lufs_after=float(after.lufs[0]), gain_db=float(before.gain_db[0]))
    assert float(before.true_peak_dbtp[0]) + float(before.gain_db[0]) > -1.0                # the ceiling did bind
    # at the base rate G g p <= c holds, and y = fl32(fl32(G g) x) adds two roundings; between the samples the moving gain may
    # ripple past the ceiling (the true peak above is recorded, not gated)
    assert float(after.sample_peak_dbfs[0]) <= -1.0 + 20 * math.log10(1 + 4 * U32)
