"""Step cache policy: which loop iterations reuse the blocks' residual instead of running them (what DiT samplers call TeaCache /
first-block cache).  Pure Python, no torch: the library runs the same machine between its graph replays (csrc/foley_rt.hip
StepCachePolicy); this module is its statement on the host - the spec users hand to the sampler, the argument checks, and the
reference the tests compare the library's decisions with.

Per model call of loop iteration i (multi-stage solvers count stages) the library measures how far the first block's modulated
audio input m moved since the previous iteration, rel = max over the batch rows of sum|m - m_prev| / sum|m_prev|.
    iteration 0, the last iteration and any iteration without a delta of this loop are always full;
    schedule mode   skips exactly the listed iterations;
    threshold mode  every iteration i >= 1 adds poly(rel) to an accumulator and is skipped while the accumulator is below the
                    threshold, inside `interval` and below `max_consecutive` skips in a row; a full iteration resets it.
Thresholds are NOT calibrated for any checkpoint: published TeaCache polynomial fits are model-specific and none exists for this
model, so `poly` defaults to the identity.  In threshold mode one decision serves the whole batch (the max over its rows): a clip's
result depends on what it is batched with, and on how denoise_process_multi shards the batch.  Schedule mode is batch- and
shard-independent.  There is no per-clip skipping inside a batch."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

MODE_OFF, MODE_SCHEDULE, MODE_THRESHOLD = 0, 1, 2


@dataclass(frozen=True)
class StepCacheSpec:
    """threshold        threshold mode: skip while the accumulated change stays below it (>= 0, finite)
    skip                schedule mode: the iteration indices of the FULL run to skip (an edit run uses those >= its first one)
    interval            (start, end) in fractions of the loop: only iterations with start <= i / n_iter < end may skip
    max_consecutive     longest run of skips (None: no cap)
    poly                polynomial applied to rel before it is accumulated, highest degree first as numpy.poly1d (None: identity)
    Exactly one of threshold / skip; interval, max_consecutive and poly belong to threshold mode."""
    threshold: Optional[float] = None
    skip: Optional[Tuple[int, ...]] = None
    interval: Optional[Tuple[float, float]] = None
    max_consecutive: Optional[int] = None
    poly: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        if self.skip is not None:
            object.__setattr__(self, "skip", tuple(int(i) for i in self.skip))
        if self.poly is not None:
            object.__setattr__(self, "poly", tuple(float(k) for k in self.poly))
        if self.interval is not None:
            object.__setattr__(self, "interval", (float(self.interval[0]), float(self.interval[1])))

    @property
    def mode(self) -> int:
        return MODE_SCHEDULE if self.skip is not None else MODE_THRESHOLD

    def check(self, n_iter: int) -> None:
        """Refuse what the library would refuse (and what only the host can see), for a FULL run of n_iter iterations."""
        if (self.threshold is None) == (self.skip is None):
            raise ValueError("step cache: give exactly one of a threshold (threshold mode) and a skip list (schedule mode)")
        if self.skip is not None:
            bad = [i for i in self.skip if not 0 <= i < n_iter]
            if bad:
                raise ValueError(f"step cache: skip indices {bad} lie outside [0, {n_iter})")
            if self.interval is not None or self.max_consecutive is not None or self.poly is not None:
                raise ValueError("step cache: interval, max_consecutive and poly belong to threshold mode")
        else:
            t = float(self.threshold)
            if not (math.isfinite(t) and t >= 0.0):
                raise ValueError(f"step cache: the threshold must be finite and >= 0, got {self.threshold}")
            if self.poly is not None and (len(self.poly) == 0 or not all(math.isfinite(k) for k in self.poly)):
                raise ValueError("step cache: poly needs at least one finite coefficient")
        if self.interval is not None and not 0.0 <= self.interval[0] <= self.interval[1]:
            raise ValueError(f"step cache: interval {self.interval} must satisfy 0 <= start <= end")
        if self.max_consecutive is not None and int(self.max_consecutive) < 1:
            raise ValueError("step cache: max_consecutive must be >= 1 (None: no cap)")

    def skip_rows(self, n_iter: int, i0: int = 0) -> List[int]:
        """Schedule mode: the 0 / 1 list of the run's iterations [i0, n_iter) - an edit run takes the suffix of the plain run's list,
        as it does of the guidance table."""
        rows = [0] * n_iter
        for i in self.skip or ():
            rows[i] = 1
        return rows[i0:]

    def interval_rows(self, n_iter: int, i0: int = 0) -> Optional[Tuple[int, int]]:
        """The iterations [lo, hi) of the run's suffix [i0, n_iter) on which start <= i / n_iter < end (tables.guidance_schedule's
        rule, on the full run's index), or None without an interval."""
        if self.interval is None:
            return None
        inside = [i for i in range(n_iter) if self.interval[0] <= i / n_iter < self.interval[1]]
        if not inside:
            return (0, 0)
        return (max(inside[0] - i0, 0), max(inside[-1] + 1 - i0, 0))


class StepCachePolicy:
    """The state machine of one loop of n_iter iterations.  decide(i, rel) -> True to skip iteration i; rel is the measured change
    (ignored at i = 0, where nothing was measured, and in schedule mode)."""

    def __init__(self, n_iter: int, mode: int, skip: Optional[Sequence[int]] = None, threshold: float = 0.0,
                 poly: Optional[Sequence[float]] = None, interval: Optional[Tuple[int, int]] = None, max_consecutive: int = 0):
        if mode == MODE_SCHEDULE and (skip is None or len(skip) != n_iter):
            raise ValueError("step cache: the skip list must have one entry per iteration")
        self.n, self.mode, self.skip = int(n_iter), mode, list(skip) if skip is not None else None
        self.threshold, self.poly = float(threshold), [float(k) for k in poly] if poly else []
        self.lo, self.hi = interval if interval is not None else (0, self.n)
        self.maxc = int(max_consecutive or 0)
        self.acc, self.run, self.have_delta, self.last_acc = 0.0, 0, False, 0.0

    @classmethod
    def from_spec(cls, spec: StepCacheSpec, n_iter: int, i0: int = 0) -> "StepCachePolicy":
        """For the suffix [i0, n_iter) of a run of n_iter iterations (i0 = 0: the plain run)."""
        spec.check(n_iter)
        n = n_iter - i0
        if spec.mode == MODE_SCHEDULE:
            return cls(n, MODE_SCHEDULE, skip=spec.skip_rows(n_iter, i0))
        return cls(n, MODE_THRESHOLD, threshold=spec.threshold, poly=spec.poly, interval=spec.interval_rows(n_iter, i0),
                   max_consecutive=spec.max_consecutive or 0)

    def decide(self, i: int, rel: float = -1.0) -> bool:
        forced = i == 0 or i == self.n - 1 or not self.have_delta
        if self.mode == MODE_SCHEDULE:
            skip = not forced and bool(self.skip[i])
        else:
            if i > 0:
                v = float(rel)
                if self.poly:
                    v = 0.0
                    for k in self.poly:
                        v = v * float(rel) + k
                self.acc += v
            self.last_acc = self.acc             # what this iteration's decision compared with the threshold
            skip = (not forced and self.acc < self.threshold and self.lo <= i < self.hi
                    and (self.maxc <= 0 or self.run < self.maxc))
        if skip:
            self.run += 1
        else:
            self.acc, self.run, self.have_delta = 0.0, 0, True
        return skip

    def pattern(self, rels: Sequence[float]) -> List[int]:
        """The decisions of a whole loop from a fixed rel sequence (only meaningful where rel does not depend on them)."""
        return [int(self.decide(i, rels[i])) for i in range(self.n)]
