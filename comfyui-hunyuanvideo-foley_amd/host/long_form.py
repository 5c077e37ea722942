"""Long clips as one batch of overlapping windows (pure CPU logic): where the windows start and how they are blended.

A long clip of Ltot latent frames is covered by n_win windows of La frames each, window k over the global frames
[starts[k], starts[k] + La).  Every window is one clip of the sampler's batch - its own slice of the video, RoPE positions 0..La -
and after every solver step the frames several windows cover are replaced in all of them by one weighted mean
(foley_set_windows), so the windows agree on their overlaps and the stitched latent decodes to one waveform.  Under a multistep
order (sampler.MultistepSpec) every window keeps the history of its own velocities; only the samples are blended.

Clip index of the batch: v * n_win + k for variation v (the node's batch_size) and window k.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence

import torch

# Latent frames of one decode (variations * Ltot) that has been run: 60 s x 6 clips at 50 Hz, the node's widget extremes.
MAX_DECODE_FRAMES = 18000


@dataclass
class WindowPlan:
    starts: List[int]          # [n_win] latent frames, ascending, starts[0] == 0
    La: int                    # frames per window
    weights: torch.Tensor      # [n_win, La] fp32: per global frame the covering windows' weights sum to 1

    @property
    def n_win(self) -> int:
        return len(self.starts)

    @property
    def Ltot(self) -> int:
        return self.starts[-1] + self.La

    def clip_index(self, variation: int, window: int) -> int:
        return variation * self.n_win + window

    def check_extent(self, variations: int) -> None:
        """Refuse a stitched decode larger than any that has been run (60 s x 6 clips)."""
        if variations * self.Ltot > MAX_DECODE_FRAMES:
            raise ValueError(f"{variations} variation(s) x {self.Ltot} latent frames = {variations * self.Ltot} frames in one "
                             f"decode; the limit is {MAX_DECODE_FRAMES} (60 s x 6 clips): lower batch_size or the duration")

    def coverage(self) -> torch.Tensor:
        """[Ltot] number of windows that cover each global frame."""
        n = torch.zeros(self.Ltot, dtype=torch.int64)
        for s in self.starts:
            n[s:s + self.La] += 1
        return n

    @classmethod
    def from_frames(cls, starts: Sequence[int], La: int) -> "WindowPlan":
        """Windows at arbitrary starts (latent frames).  Any depth of coverage is allowed; a gap between consecutive windows and
        starts that do not ascend from 0 are refused."""
        starts = [int(s) for s in starts]
        La = int(La)
        if La < 1 or not starts:
            raise ValueError("a window plan needs at least one window of at least one frame")
        if starts[0] != 0:
            raise ValueError(f"the first window starts at frame 0, got {starts[0]}")
        for a, b in zip(starts, starts[1:]):
            if b <= a:
                raise ValueError(f"window starts must ascend, got {starts}")
            if b > a + La:
                raise ValueError(f"gap between the windows at {a} and {b}: frames {a + La}..{b - 1} are in no window (La = {La})")
        return cls(starts, La, blend_weights(starts, La))


def blend_weights(starts: Sequence[int], La: int) -> torch.Tensor:
    """[n_win, La] fp32.  Each window gets a trapezoid - 1 in its interior, a linear ramp over its overlap with the previous window
    and one over its overlap with the next (none at the global start and end), evaluated at the frame centre l + 0.5 so that no
    covered frame has weight 0; where both ramps reach a frame their product is taken - and every global frame's weights are then
    divided by their sum.  Built in float64 and rounded once; a frame one window covers has exactly 1.0."""
    n = len(starts)
    Ltot = starts[-1] + La
    l = torch.arange(La, dtype=torch.float64)
    w = torch.ones(n, La, dtype=torch.float64)
    for k in range(n):
        if k > 0:
            ov = starts[k - 1] + La - starts[k]
            if ov > 0:
                w[k] *= torch.where(l < ov, (l + 0.5) / ov, torch.ones_like(l))
        if k < n - 1:
            ov = starts[k] + La - starts[k + 1]
            if ov > 0:
                w[k] *= torch.where(l >= La - ov, (La - l - 0.5) / ov, torch.ones_like(l))
    total = torch.zeros(Ltot, dtype=torch.float64)
    for k in range(n):
        total[starts[k]:starts[k] + La] += w[k]
    for k in range(n):
        w[k] /= total[starts[k]:starts[k] + La]
    return w.to(torch.float32).contiguous()


def plan_windows(total_s: float, window_s: float, overlap_s: float = 2.0, frame_rate: int = 50,
                 variations: int = 1) -> WindowPlan:
    """The windows of a `total_s` second clip: windows of `window_s` seconds that overlap their neighbours by at least `overlap_s`.

    `total_s` is cut down to whole seconds, and `window_s` must be a whole number of seconds >= 1: the starts fall on whole seconds
    because the 8 fps SigLIP2 frames, the 25 fps Synchformer frames and the 50 Hz latents only share a grid at 1 s.  `overlap_s` is
    any value in [0, window_s).  total_s <= window_s gives ONE window of the total length; otherwise
    n = ceil((T - O) / (W - O)) windows, window k starting at second floor(k * (T - W) / (n - 1) + 0.5) - spread evenly, the last
    one ending at T.  (With a fractional overlap_s the rounding of a start could cut an overlap below it; n is then raised until
    it does not - at most to starts one second apart, an overlap of window_s - 1, which is all an overlap_s above that gets.)  Uneven totals give frames three windows cover, e.g. (T, W, O) = (19, 10, 2): starts 0, 5, 9 s.

    `variations` (the node's batch_size): variations * Ltot above 18000 latent frames is refused - the largest decode that has
    been run."""
    if float(window_s) != int(window_s) or int(window_s) < 1:
        raise ValueError(f"window_s must be a whole number of seconds >= 1, got {window_s}")
    W, T, O = int(window_s), int(total_s), float(overlap_s)
    if T < 1:
        raise ValueError(f"total_s must be at least 1 s, got {total_s}")
    if not 0.0 <= O < W:
        raise ValueError(f"overlap_s must lie in [0, window_s), got {overlap_s}")
    fr = int(frame_rate)
    if T <= W:
        plan = WindowPlan.from_frames([0], T * fr)
    else:
        n_max = T - W + 1                       # starts one second apart: the deepest overlap whole-second starts can give
        n = min(max(2, math.ceil((T - O) / (W - O))), n_max)
        while True:
            secs = [int(math.floor(k * (T - W) / (n - 1) + 0.5)) for k in range(n)]
            if n == n_max or all(a + W - b >= O for a, b in zip(secs, secs[1:])):
                break
            n += 1
        plan = WindowPlan.from_frames([s * fr for s in secs], W * fr)
    plan.check_extent(int(variations))
    return plan
