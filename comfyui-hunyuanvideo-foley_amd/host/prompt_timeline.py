"""Timed prompts: a prompt timeline through a per-token cross-attention.  Pure Python - the semantics the library's timeline
kernel (csrc/attention_timeline.hip, foley_prepare_timeline) is driven by.

A timeline is a list of (start_s, end_s, prompt).  Time that no span covers takes the base prompt (the widget's); equal texts share
one text set; neighbouring segments with the same text merge.  Every query token of the two-stream blocks' cross-attention has a
time - audio frame l: (l + 0.5) / 50 s, SigLIP2 token j: (j + 0.5) / 8 s (the sync tokens never reach that attention) - and reads
the triple (set_a, set_b, alpha):

    out = (1 - alpha) * softmax(q K_a^T / sqrt(d)) V_a + alpha * softmax(q K_b^T / sqrt(d)) V_b

set_a is the set of the token's own segment.  A crossfade of c seconds gives the boundary tb between segments i and i + 1 a linear
ramp of half-width h = min(c / 2, len_i / 2, len_{i+1} / 2): inside (tb - h, tb + h) a token blends towards the neighbour's set,
alpha rising from 0 at the ramp's outer edge to 0.5 at tb on both sides - the two sides meet at 0.5 / 0.5.  c = 0: hard cuts.
Times are exact rationals of integers until the one division, alpha is computed in float64 and rounded to fp32 once.

The cap: MAX_SETS = 16 distinct text sets in a run, the negative prompt included.  Sixteen sets cost about 150 MB of cached
K / V^T at xxl: 18 blocks x 16 sets x 12 heads x (77 + 96) x 128 x 2 B = 153 MB (K rows [77, 128] and V^T rows [128, 96] in bf16).

The weights this project ships are synthetic: nothing here claims anything about how a timed prompt sounds."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

MAX_SETS = 16            # FOLEY_TIMELINE_MAX_SETS (include/foley_hip.h); the arithmetic is in the module docstring
AUDIO_RATE = 50          # latent frames per second
VISUAL_RATE = 8          # SigLIP2 tokens per second


class TimelineError(ValueError):
    pass


@dataclass(frozen=True)
class Segment:
    start_s: float
    end_s: float
    prompt: str
    set: int             # index into the timeline's distinct prompts
    h_lo: float          # half-width of the ramp at the segment's start (0: none - the clip's start, or a hard cut)
    h_hi: float          # ... and at its end


@dataclass(frozen=True)
class Timeline:
    """What the sampler takes as `timeline=`: the segments that cover [0, duration) and the distinct prompts, in the order
    text_feats["text_feat"] holds their features."""
    segments: Tuple[Segment, ...]
    prompts: Tuple[str, ...]

    def key(self):
        return (tuple((s.start_s, s.end_s, s.set, s.h_lo, s.h_hi) for s in self.segments), len(self.prompts))


def parse(timeline, base_prompt: str, duration_s: float, crossfade_s: float = 0.0, extra_sets: int = 1) -> Timeline:
    """[(start_s, end_s, prompt), ...] -> Timeline.  Refused with a message: malformed entries, negative times, end <= start,
    spans out of order or overlapping, a negative crossfade, more than MAX_SETS sets (`extra_sets` counts the negative prompt)."""
    duration_s, c = float(duration_s), float(crossfade_s)
    if not duration_s > 0.0:
        raise TimelineError(f"prompt_timeline: the clip's duration must be positive, got {duration_s}")
    if not c >= 0.0:
        raise TimelineError(f"prompt_crossfade_s must be >= 0, got {crossfade_s}")
    spans = []
    for i, e in enumerate(timeline or ()):
        if not isinstance(e, (tuple, list)) or len(e) != 3 or not isinstance(e[2], str):
            raise TimelineError(f"prompt_timeline[{i}] is not (start_s, end_s, prompt): {e!r}")
        try:
            t0, t1 = float(e[0]), float(e[1])
        except (TypeError, ValueError):
            raise TimelineError(f"prompt_timeline[{i}] is not (start_s, end_s, prompt): {e!r}") from None
        if not (t0 >= 0.0 and t1 >= 0.0):
            raise TimelineError(f"prompt_timeline[{i}]: negative time in ({t0}, {t1})")
        if not t1 > t0:
            raise TimelineError(f"prompt_timeline[{i}]: end {t1} <= start {t0}")
        spans.append((t0, t1, e[2]))
    if not spans:
        raise TimelineError("prompt_timeline is empty: pass None for a run without a timeline")
    spans.sort(key=lambda s: s[0])
    for a, b in zip(spans, spans[1:]):
        if b[0] < a[1]:
            raise TimelineError(f"prompt_timeline: spans ({a[0]}, {a[1]}) and ({b[0]}, {b[1]}) overlap")
    # cover [0, duration): spans cut at the clip's end, gaps take the base prompt, equal neighbours merge
    cover: List[List] = []

    def put(t0, t1, text):
        if t1 <= t0:
            return
        if cover and cover[-1][2] == text:
            cover[-1][1] = t1
        else:
            cover.append([t0, t1, text])

    t = 0.0
    for t0, t1, text in spans:
        if t0 >= duration_s:
            break
        put(t, t0, base_prompt)
        put(t0, min(t1, duration_s), text)
        t = min(t1, duration_s)
    put(t, duration_s, base_prompt)
    prompts: List[str] = []
    for seg in cover:
        if seg[2] not in prompts:
            prompts.append(seg[2])
    if len(prompts) + int(extra_sets) > MAX_SETS:
        raise TimelineError(f"prompt_timeline: {len(prompts)} distinct prompts + {int(extra_sets)} (negative prompt) exceed "
                            f"{MAX_SETS} text sets")
    lens = [s[1] - s[0] for s in cover]
    hs = [min(c / 2, lens[i] / 2, lens[i + 1] / 2) for i in range(len(cover) - 1)]      # ramp half-width per boundary
    segs = tuple(Segment(s[0], s[1], s[2], prompts.index(s[2]), hs[i - 1] if i > 0 else 0.0, hs[i] if i < len(hs) else 0.0)
                 for i, s in enumerate(cover))
    return Timeline(segs, tuple(prompts))


def token_times(Lv: int, La: int, start_frame: int = 0) -> List[float]:
    """Times of the cross-attention's query tokens, visual first: token j of a window that starts at latent frame `start_frame`
    sits at start / 50 + (j + 0.5) / 8 s, audio frame l at (start + l + 0.5) / 50 s - integer numerators, one division each, so
    two windows give the same float for the same global instant."""
    s = int(start_frame)
    return [(8 * s + 50 * j + 25) / 400.0 for j in range(Lv)] + [(2 * (s + l) + 1) / 100.0 for l in range(La)]


def _triple(segs: Sequence[Segment], t: float) -> Tuple[int, int, float]:
    i = len(segs) - 1
    for k, s in enumerate(segs):
        if t < s.end_s:
            i = k
            break
    s = segs[i]
    if i + 1 < len(segs) and s.h_hi > 0.0 and t > s.end_s - s.h_hi:
        return s.set, segs[i + 1].set, 0.5 * (t - (s.end_s - s.h_hi)) / s.h_hi
    if i > 0 and s.h_lo > 0.0 and t < s.start_s + s.h_lo:
        return s.set, segs[i - 1].set, 0.5 * ((s.start_s + s.h_lo) - t) / s.h_lo
    return s.set, s.set, 0.0


def token_table(segments: Sequence[Segment], Lv: int, La: int, start_frame: int = 0):
    """(set_a, set_b, alpha) of one clip's Lv + La query tokens: lists of int, int, float (float64; rounded to fp32 once where the
    table becomes a tensor).  start_frame: the clip is the window of a long clip that starts at that latent frame - the shift."""
    sa, sb, al = [], [], []
    for t in token_times(Lv, La, start_frame):
        a, b, x = _triple(segments, t)
        sa.append(a)
        sb.append(b)
        al.append(min(max(x, 0.0), 0.5))
    return sa, sb, al


def batch_table(tl: Timeline, Lv: int, La: int, ncfg: int, clips: int, starts: Optional[Sequence[int]] = None):
    """The table of one run, [ncfg * clips, Lv + La] as three flat lists (row b = h * clips + k).  With ncfg > 1 the sets are
    [negative ; prompts...]: every row of the halves below the last points every token at set 0 with alpha 0 (ncfg 3: halves 0
    and 1), the last half's rows carry the timeline with its set indices moved up by one.  starts (a windowed run: clip
    v * n_win + k is window k): row k's table is the timeline shifted by starts[k] latent frames."""
    off = 1 if ncfg > 1 else 0
    S = Lv + La
    n_win = len(starts) if starts else 1
    if clips % n_win:
        raise TimelineError(f"{clips} clips are not a multiple of {n_win} windows")
    per_win = [token_table(tl.segments, Lv, La, starts[k] if starts else 0) for k in range(n_win)]
    sa, sb, al = [], [], []
    for h in range(ncfg):
        for k in range(clips):
            if h < ncfg - 1:
                sa += [0] * S
                sb += [0] * S
                al += [0.0] * S
            else:
                a, b, x = per_win[k % n_win]
                sa += [v + off for v in a]
                sb += [v + off for v in b]
                al += x
    return sa, sb, al
