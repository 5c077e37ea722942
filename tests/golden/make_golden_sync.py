"""Generate the sync-score golden g19 by RUNNING THE REFERENCE'S Synchformer (build container only).

    python tests/golden/make_golden_sync.py

The reference's own `Synchformer` (models/synchformer/synchformer.py), its `encode_audio_with_sync` and `compare_v_a` run on the CPU
in fp32 with the synthesised weights of host/encoders.py::synchformer_sync_schema.  Two shims make the package import on this
image, nothing of its arithmetic is touched:
  * a stub `torchaudio` whose transforms.MelSpectrogram exists (synchformer.py uses it as an annotation only);
  * ASTModel.get_head_mask -> [None] * n (transformers 5 removed the method; head_mask is None throughout).
The `mel` callable handed to encode_audio_with_sync is torchaudio's MelSpectrogram definition computed by library code:
torch.stft (n_fft 1024, hop 160, win 400 periodic Hann, center, reflect) -> |X|^2 -> transformers.audio_utils.mel_filter_bank
(HTK, norm None, 0 - 8000 Hz) applied as MelScale does.  The 48 kHz -> 16 kHz resampling is the restated formula of torchaudio's
default (torchaudio is not installed), see `resample_formula`.

g19_sync.npz (fp32), for two B = 2 clips of 5 s and 8 s (click train + noise, host/synth.py::synth_click_audio):
  w16_{5,8}_head      the first 4096 samples of the 16 kHz signal (the full signal is recomputed from the formula by the tests)
  mel_5, mel_5_idx    the normalised log-mel [n, 128, 66] of segments (b, s) = mel_5_idx (the AST input)
  afeat_{5,8}_sel     [2, 3, 6, 768] audio features at segments afeat_{5,8}_idx (of 14 and 24)
  vfeat_{5,8}_head    the first 768 values of the visual features [1, S_v*8, 768]; the features themselves are not stored -
                      they are synth_tensor(VFEAT_KEY % sec, ...) with 14 and 24 segments, regenerated bit for bit by the tests
  starts_{5,8}        window starts;  logits_{5,8} [2, W, 21] compare_v_a of every window
"""
from __future__ import annotations

import importlib
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_harness  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

load_package()
from foley_amd.host import encoders as E, synth  # noqa: E402


VFEAT_KEY = "g19.vfeat%d"
VFEAT_SEGMENTS = {5: 14, 8: 24}


def resample_formula(x: torch.Tensor, orig: int = 48000, new: int = 16000) -> torch.Tensor:
    """torchaudio.functional.resample(x, orig, new) at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99),
    restated: the kernel of _get_sinc_resample_kernel in float64, zero padding (width, width + orig), stride-orig conv1d."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    lpw, base = 6, min(orig, new) * 0.99
    width = math.ceil(lpw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = (torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx) * base
    t = t.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    kernel = (torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * window * (base / orig)).to(x.dtype)
    n = x.shape[-1]
    y = F.conv1d(F.pad(x[:, None], (width, width + orig)), kernel, stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[..., :math.ceil(new * n / orig)]


def load_synchformer():
    ref_harness.load_reference()
    ref_harness._install_synchformer_stubs()
    if "torchaudio" not in sys.modules:
        ta = types.ModuleType("torchaudio")
        ta.__path__ = []
        tt = types.ModuleType("torchaudio.transforms")
        tt.MelSpectrogram = object
        ta.transforms = tt
        sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = ta, tt
    pkg_name = "hunyuanvideo_foley.models.synchformer"
    if pkg_name not in sys.modules:
        pkg = types.ModuleType(pkg_name)
        pkg.__path__ = [os.path.join(ref_harness.REFERENCE_ROOT, "hunyuanvideo_foley", "models", "synchformer")]
        sys.modules[pkg_name] = pkg
    sf = importlib.import_module(pkg_name + ".synchformer")
    ma = importlib.import_module(pkg_name + ".modeling_ast")
    ma.ASTModel.get_head_mask = lambda self, hm, n, *a, **k: [None] * n
    return sf, sf.Synchformer().eval()


def mel_callable():
    from transformers.audio_utils import mel_filter_bank
    fb = torch.from_numpy(mel_filter_bank(num_frequency_bins=513, num_mel_filters=128, min_frequency=0.0, max_frequency=8000.0,
                                          sampling_rate=16000, norm=None, mel_scale="htk")).float()         # [513, 128]
    win = torch.hann_window(400)

    def mel(x):
        spec = torch.stft(x.reshape(-1, x.shape[-1]), n_fft=1024, hop_length=160, win_length=400, window=win, center=True,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True).abs().pow(2.0)
        out = torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)                               # MelScale.forward
        return out.reshape(*x.shape[:-1], 128, out.shape[-1])
    return mel


def main():
    sf, model = load_synchformer()
    sd = synth.materialize(E.synchformer_sync_schema())
    own = model.state_dict()
    prefixes = E.SYNC_PREFIXES
    expect = {k for k in own if k.startswith(prefixes)}
    assert expect == set(sd), sorted(expect ^ set(sd))                                   # the schema = Synchformer's keys
    assert all(tuple(own[k].shape) == tuple(v.shape) for k, v in sd.items())
    missing = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if k.startswith(prefixes)]
    mel = mel_callable()
    captured = {}
    extract = model.extract_afeats

    def hook(x):
        captured["mel"] = x[:, :, 0].clone()
        return extract(x)
    model.extract_afeats = hook
    out = {}
    with torch.inference_mode():
        for sec, stride in ((5, None), (8, 5)):
            n_seg_v = VFEAT_SEGMENTS[sec]
            w48 = synth.synth_click_audio(2, sec * 48000, 48000)
            w16 = resample_formula(w48)
            afeat = sf.encode_audio_with_sync(model, w16, mel)                                # [2, S_a, 6, 768]
            vfeat = synth.synth_tensor(VFEAT_KEY % sec, (1, n_seg_v * 8, 768), 1.0)
            S = min(n_seg_v, afeat.shape[1])
            starts = sorted({0, S - 14} | (set(range(0, S - 14, stride)) if stride else set()))
            v = vfeat.expand(2, -1, -1).reshape(2, n_seg_v, 8, 768)
            logits = torch.stack([model.compare_v_a(v[:, s:s + 14], afeat[:, s:s + 14]) for s in starts], dim=1)
            out[f"w16_{sec}_head"] = w16[:, :4096]
            out[f"vfeat_{sec}_head"] = vfeat.reshape(-1)[:768]
            out[f"starts_{sec}"] = torch.tensor(starts, dtype=torch.int32)
            out[f"logits_{sec}"] = logits
            print(f"{sec} s: w16 {tuple(w16.shape)}, afeat {tuple(afeat.shape)}, windows {starts}, argmax {logits.argmax(-1).tolist()}")
            if sec == 5:
                idx = torch.tensor([[0, 0], [0, 13], [1, 6]], dtype=torch.int32)      # both edges of the reflect padding
                out["mel_5"] = captured["mel"][idx[:, 0].long(), idx[:, 1].long()]
                out["mel_5_idx"] = idx
            idx = torch.tensor([0, afeat.shape[1] // 2, afeat.shape[1] - 1], dtype=torch.int32)
            out[f"afeat_{sec}_sel"] = afeat[:, idx.long()]
            out[f"afeat_{sec}_idx"] = idx
    path = os.path.join(HERE, "g19_sync.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
