"""CPU-only: the receptive field of the full-width DAC decoder in latent frames.  The GPU test of a 60 s x 6 decode
(tests/test_model_gpu.py::test_dac_decode_60s_six_clips) compares latent WINDOWS against the oracle, each with a margin of
DAC_WINDOW_MARGIN frames cut off before comparing; that only holds if a window's interior does not see past the margin.
Established here on the oracle itself: the interior of a window with margin m equals the same frames decoded with margin 2m."""
import torch

from conftest import rel_err
from foley_amd.host import config as C, synth
from oracle import foley_oracle as O

DAC_WINDOW_MARGIN = 16      # latent frames; keep in step with tests/test_model_gpu.py


def test_dac_window_margin_covers_receptive_field():
    m, w, hop = DAC_WINDOW_MARGIN, 8, C.DAC48K.hop
    dsd = {k: v.double() for k, v in synth.synth_dac_state_dict(C.DAC48K).items()}   # fp64: round-off far below the gate
    z = torch.randn(1, 128, w + 4 * m, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    dec = lambda t: O.dac_decode(dsd, t.contiguous(), C.DAC48K.rates, C.DAC48K.dilations)
    with torch.inference_mode():
        wide = dec(z)                                                   # frames [2m, 2m + w) have margin 2m on both sides
        inner = dec(z[..., m:3 * m + w])                                # ... and margin m here
        assert rel_err(inner[..., m * hop:(m + w) * hop], wide[..., 2 * m * hop:(2 * m + w) * hop]) <= 1e-7
        # clip edges (the decoder's zero padding): a head / tail window needs the margin on its inner side only
        head = dec(z[..., :w + m])
        assert rel_err(head[..., :w * hop], wide[..., :w * hop]) <= 1e-7
        tail = dec(z[..., -(w + m):])
        assert rel_err(tail[..., -w * hop:], wide[..., -w * hop:]) <= 1e-7
        # and the margin is needed: with a quarter of it the interior differs well beyond round-off
        short = dec(z[..., 2 * m - m // 4:2 * m + w + m // 4])
        assert rel_err(short[..., (m // 4) * hop:(m // 4 + w) * hop], wide[..., 2 * m * hop:(2 * m + w) * hop]) > 1e-5
