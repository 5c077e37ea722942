"""The loudness stage without a GPU: the fp64 restatement (tests/loudness_ref.py) against the published anchors of ITU-R BS.1770
and EBU Tech 3341, the host tables of host/loudness.py against it, the limiter's properties, the ABI surface and the node's
keyword plumbing."""
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from foley_amd import nodes
from foley_amd.host import config as C, runtime as rt, sampler
import loudness_ref as LR
from abi_pin import assert_abi_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48000


def _loud():
    from foley_amd.host import loudness
    return loudness


def _sine(freq, dbfs, secs, phase=0.0):
    n = np.arange(int(round(secs * FS)), dtype=np.float64)
    return 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * n / FS + phase)


# ----------------------------------------------------------------------------- the oracle against the published anchors
def test_997_hz_full_scale_sine_reads_minus_3_01():
    """BS.1770's own anchor: a 0 dBFS 997 Hz sine in one channel reads -3.01 LKFS."""
    got = LR.integrated_loudness(_sine(997.0, 0.0, 5.0))
    print("997 Hz anchor:", got)
    assert abs(got - (-3.01)) < 0.005


def test_tech_3341_case_1():
    """Stereo 1 kHz sine, -23 dBFS, 20 s: -23.0 +/- 0.1 LUFS (the standard's tolerance)."""
    s = _sine(1000.0, -23.0, 20.0)
    got = LR.integrated_loudness(np.stack([s, s]))
    print("Tech 3341 case 1:", got)
    assert abs(got - (-23.0)) <= 0.1


def test_tech_3341_case_3_relative_gate():
    """Stereo 10 s at -36, 60 s at -23, 10 s at -36 dBFS: -23.0 +/- 0.1 LUFS - the quiet ends fall to the relative gate."""
    s = np.concatenate([_sine(1000.0, -36.0, 10.0), _sine(1000.0, -23.0, 60.0), _sine(1000.0, -36.0, 10.0)])
    res = LR.gate(LR.hop_energies(np.stack([s, s])))
    print("Tech 3341 case 3:", res["lufs"], res["n_rel"], "of", len(res["z"]))
    assert abs(res["lufs"] - (-23.0)) <= 0.1
    assert len(res["z"]) == 797 and res["n_abs"] == 797 and res["n_rel"] < 797


def test_short_and_silent_clips_read_minus_infinity():
    assert LR.integrated_loudness(np.zeros(FS)) == -math.inf
    assert LR.integrated_loudness(_sine(1000.0, -20.0, 19199 / FS)) == -math.inf          # nh = 3: no block


# ----------------------------------------------------------------------------- chunking and carry
def test_chunk_transition_is_the_homogeneous_response():
    L = _loud()
    assert L.K_STAGES[0] == tuple(LR.SOS[0][[0, 1, 2, 4, 5]]) and L.K_STAGES[1] == tuple(LR.SOS[1][[0, 1, 2, 4, 5]])
    T = L.chunk_transition().numpy()
    want = LR.homogeneous_transition(L.CHUNK)
    assert L.CHUNK == LR.CHUNK == 480 and T.dtype == np.float64
    # T is the exactly rounded power; the filter run in fp64 from the unit states carries 480 steps of rounding through a state
    # whose entries reach 44 and nearly cancel (the double pole next to z = 1): measured 3.1e-13 of the largest entry, gated at 1e-9
    err = np.abs(T - want).max() / np.abs(want).max()
    print("transition vs homogeneous response:", err)
    assert err <= 1e-9
    one = LR.homogeneous_transition(1)
    assert np.array_equal(L.state_matrix().numpy(), one)


def test_chunked_restatement_equals_the_sequential_filter():
    rng = np.random.default_rng(0)
    n = np.arange(24037)
    x = 0.1 * rng.standard_normal((2, n.size)) + 0.2 * np.sin(2 * np.pi * 50 * n / FS) + 0.05
    x = x.astype(np.float32)
    seq = LR.hop_energies(x)
    chk = LR.hop_energies_chunked(x, _loud().chunk_transition().numpy())
    rel = np.abs(chk - seq).max() / seq.max()
    print("chunked vs sequential, relative:", rel)
    assert seq.shape == (2, 5) and rel < 1e-11
    # the carried state itself, against scipy's carried zi: chunk by chunk
    from scipy.signal import sosfilt
    zi = np.zeros((2, 2))
    ys = []
    for k in range(0, 24000, 480):
        y, zi = sosfilt(LR.SOS, x[0, k:k + 480].astype(np.float64), zi=zi)
        ys.append(y)
    assert np.array_equal(np.concatenate(ys), LR.kweight(x[0, :24000]))


# ----------------------------------------------------------------------------- taps
def test_true_peak_taps():
    L = _loud()
    h = L.true_peak_prototype().numpy()
    assert h.shape == (49,) and np.array_equal(h, h[::-1]) and h[24] == 1.0
    assert np.abs(h - LR.prototype()).max() < 1e-15
    ph = LR.phase_taps()
    assert np.abs(ph[0] - np.eye(12)[5]).max() < 1e-15                                   # phase 0: the identity (sin(pi j) in fp64)
    taps = L.true_peak_taps().numpy()
    assert taps.shape == (3, 12) and np.abs(taps - ph[1:]).max() < 1e-15
    assert np.abs(taps.sum(1) - 1.0).max() < 1e-15
    assert np.allclose(taps[0], taps[2][::-1], atol=1e-16)                               # phases 1 and 3 mirror each other


def test_fs4_sine_reads_minus_6_dbtp():
    """Tech 3341's true-peak vector: fs/4 at 45 degrees, amplitude 0.5 - every sample is 0.354 (-9.03 dBFS), the peak 0.5."""
    x = _sine(12000.0, -6.0206, 0.1, phase=np.pi / 4)
    assert abs(LR.db(np.abs(x).max()) - (-9.03)) < 0.01
    # the vector is a steady tone: 10 ms raised-cosine ramps keep the cut edges (x is zero outside the clip) from ringing in the
    # interpolator - cut hard, the first samples overshoot and the clip reads -5.92
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(480) / 480)
    x[:480] *= ramp
    x[-480:] *= ramp[::-1]
    tp = LR.db(LR.true_peak(x[None]))
    print("fs/4 true peak:", tp)
    assert -6.0 - 0.4 <= tp <= -6.0 + 0.2


# ----------------------------------------------------------------------------- limiter
def _planted(N, seed=1):
    rng = np.random.default_rng(seed)
    x = (0.05 * rng.standard_normal(N)).astype(np.float32)
    for at in (0, N - 1, N // 2, N // 2 + min(100, N // 4)):
        x[at] = 0.9
    return x


@pytest.mark.parametrize("N,W", [(4000, 240), (4000, 7), (100, 240)])
def test_limiter_oracle_properties(N, W):
    x = _planted(N)
    p, _ = LR.envelope(x[None])
    G, c = 4.0, 10.0 ** (-1.0 / 20.0)
    g, r = LR.limiter_gain(p, G, c, W)
    assert g.shape == (N,) and (r < 1).any()
    assert (g <= r).all()
    assert (G * g * p <= c * (1 + 2.0 ** -50)).all()
    rp = np.concatenate([np.ones(W), r, np.ones(W)])
    free = np.lib.stride_tricks.sliding_window_view(rp, 2 * W + 1).min(-1) == 1.0        # r == 1 on [n - W, n + W]
    assert (g[free] == 1.0).all() and ((g < 1.0) | free).all()
    if W < N // 4:
        assert free.any()


# ----------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_work():
    L = _loud()
    cpu = torch.zeros(1, 1, 9600)
    with pytest.raises(ValueError, match="48000"):
        L.measure(cpu, 44100)
    with pytest.raises(ValueError, match="mono or stereo"):
        L.measure(torch.zeros(1, 3, 9600), FS)
    for kw, word in ((dict(target_lufs=1.0), "target_lufs"), (dict(true_peak_dbtp=0.5), "ceiling"),
                     (dict(limiter=True, lookahead_ms=0.0), "look"), (dict(limiter=True, lookahead_ms=10.5), "look")):
        with pytest.raises(ValueError, match=word):
            L.normalize({"waveform": cpu, "sample_rate": FS}, **kw)
    assert L.lookahead_samples(5.0) == 240 and L.lookahead_samples(10.0) == 480 and L.lookahead_samples(0.02) == 1
    with pytest.raises(rt.FoleyRuntimeError):                                             # no CPU fallback
        L.measure(cpu, FS)


def test_static_gain_rule():
    L = _loud()
    lufs = torch.tensor([-30.0, -20.0, -math.inf], dtype=torch.float64)
    tp = torch.tensor([-10.0, -2.0, -math.inf], dtype=torch.float64)
    g_db, gain = L.static_gain(lufs, tp, -16.0, -1.0, limiter=False)
    assert g_db.tolist() == [9.0, 1.0, 0.0] and gain[2] == 0.0                            # clip 0: the ceiling binds (9 < 14)
    assert gain[0] == torch.tensor(10.0 ** (9.0 / 20.0), dtype=torch.float64).to(torch.float32)
    g_db, gain = L.static_gain(lufs, tp, -16.0, -1.0, limiter=True)
    assert g_db.tolist() == [14.0, 4.0, 0.0]


# ----------------------------------------------------------------------------- ABI surface
NAMES = ("foley_op_loudness_energy", "foley_op_loudness_gate", "foley_op_true_peak", "foley_op_loudness_apply")


def test_abi_declares_the_loudness_entries():
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    lib = rt.load_library()
    for name in NAMES:
        assert name in rt.EXPORTED_SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr)
        assert getattr(lib, name) is not None
    assert_abi_version()
    for op in ("op_loudness_energy", "op_loudness_gate", "op_true_peak", "op_loudness_apply"):
        assert callable(getattr(rt, op))
    src = open(os.path.join(ROOT, "comfyui-hunyuanvideo-foley_amd", "csrc", "loudness.hip")).read()
    assert "getenv" not in src and "atomicAdd" not in src                                 # no environment, no float atomics
    assert "build/loudness.o" in open(os.path.join(ROOT, "comfyui-hunyuanvideo-foley_amd", "csrc", "Makefile")).read()


# ----------------------------------------------------------------------------- node plumbing
def _node(monkeypatch, duration=5.0, batch_size=2, **kw):
    model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
    model.get_empty_clip_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    model.get_empty_sync_sequence = lambda bs, len: torch.zeros(bs, len, 768)
    dac = types.SimpleNamespace(has_encoder=True, cfg=C.DAC48K, sample_rate=48000)
    seen = {"encoded": [], "normalize": []}
    wave = torch.arange(batch_size * int(round(duration * 50)) * 960, dtype=torch.float32).view(batch_size, 1, -1)

    def fake_sample(visual, text, secs, m, d, **k):
        seen.update(k)
        return wave, 48000

    def fake_encode(prompts, deps, dev, dt=None):
        seen["encoded"].append(list(prompts))
        return torch.zeros(len(prompts), 5, 768)

    def fake_normalize(audio_batch, target_lufs=-16.0, true_peak_dbtp=-1.0, limiter=False, lookahead_ms=5.0):
        seen["normalize"].append((audio_batch, target_lufs, true_peak_dbtp, limiter, lookahead_ms))
        z = torch.zeros(batch_size, dtype=torch.float64)
        res = _loud().LoudnessResult(z, z, z, z[:, None], z.bool(), gain_db=z)
        return {"waveform": audio_batch["waveform"] * 0.5, "sample_rate": 48000}, res, res

    monkeypatch.setattr(sampler, "denoise_process_with_generator", fake_sample)
    monkeypatch.setattr(nodes, "encode_text_feat", fake_encode)
    if "foley_amd.host.loudness" in sys.modules or kw.get("loudness_lufs") is not None:
        monkeypatch.setattr(_loud(), "normalize", fake_normalize)
    deps = {"dac_model": dac, "siglip2_model": None, "syncformer_model": None}
    out = nodes.HunyuanFoleySampler().generate_audio(model, deps, 16, duration, "p", "n", 4.5, 10, "euler", batch_size, 0, True, **kw)
    return out, seen, wave


def test_node_loudness_reaches_normalize_with_the_sampler_tensor(monkeypatch):
    (first, batch), seen, wave = _node(monkeypatch, loudness_lufs=-23.0, true_peak_dbtp=-2.0, peak_limiter=True)
    (audio_batch, target, ceiling, limiter, look), = seen["normalize"]
    assert audio_batch["waveform"] is wave and audio_batch["sample_rate"] == 48000        # the tensor the sampler returned, not a copy
    assert (target, ceiling, limiter, look) == (-23.0, -2.0, True, 5.0)
    assert torch.equal(batch["waveform"], wave * 0.5) and torch.equal(first["waveform"], wave[:1] * 0.5)
    (first, batch), seen, wave = _node(monkeypatch, loudness_lufs=-16.0)
    assert seen["normalize"][0][1:] == (-16.0, -1.0, False, 5.0)


def test_node_without_loudness_never_calls_the_module(monkeypatch):
    (first, batch), seen, wave = _node(monkeypatch)
    assert seen["normalize"] == [] and torch.equal(batch["waveform"], wave)
    (_f, batch2), seen, _w = _node(monkeypatch, loudness_lufs=None, true_peak_dbtp=-1.0, peak_limiter=False)
    assert seen["normalize"] == [] and torch.equal(batch2["waveform"], wave)


def test_node_loudness_refusals_come_before_the_encoders(monkeypatch):
    for kw, word in ((dict(loudness_lufs=3.0), "target_lufs"), (dict(loudness_lufs=-16.0, true_peak_dbtp=1.0), "ceiling")):
        with pytest.raises(ValueError, match=word):
            _out, seen, _w = _node(monkeypatch, **kw)
    _out, seen, _w = _node(monkeypatch, loudness_lufs=-16.0)
    assert seen["encoded"] == [["n", "p"]]
    calls = []
    monkeypatch.setattr(nodes, "encode_text_feat", lambda *a, **k: calls.append(1))
    with pytest.raises(ValueError, match="target_lufs"):
        model = types.SimpleNamespace(cfg=C.XXL, device=torch.device("cpu"), dtype=torch.float32, arena=None)
        nodes.HunyuanFoleySampler().generate_audio(model, {"dac_model": None}, 16, 5.0, "p", "n", 4.5, 10, "euler", 1, 0, True,
                                                   loudness_lufs=0.5)
    assert calls == []
