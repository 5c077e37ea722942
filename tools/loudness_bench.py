"""Wall time of the loudness stage (host/loudness.py) on one GPU: measure(), normalize() with the static gain and normalize() with
the limiter, for a 5 s clip and for six 60 s clips (the node's widget extremes).  The three calls are interleaved per repetition
after a warm-up; each figure is the median of the synchronised wall times, with the spread (max - min).

    python tools/loudness_bench.py [--reps 3] [--shapes 5x1,60x6]

The input is band-limited noise with a few loud clicks at -14 dBFS or so, built on the device; normalising it to -16 LUFS under a
-1 dBTP ceiling makes the limiter work on the clicks.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from foley_amd.host import loudness  # noqa: E402


def program(B, secs, dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    n = int(secs * 48000)
    x = 0.02 * torch.randn(B, 1, n, generator=g)
    x[:, :, ::48000 // 3] = 0.7                       # three clicks a second
    return x.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="5x1,60x6")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {}
    for shape in a.shapes.split(","):
        secs, B = (int(v) for v in shape.split("x"))
        batch = {"waveform": program(B, secs, dev), "sample_rate": 48000}
        calls = {"measure": lambda: loudness.measure(batch["waveform"], 48000),
                 "normalize": lambda: loudness.normalize(batch, -16.0, -1.0),
                 "normalize+limiter": lambda: loudness.normalize(batch, -16.0, -1.0, limiter=True)}
        times = {k: [] for k in calls}
        last = {}
        for rep in range(a.reps + 1):                 # repetition 0 is the warm-up
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[k] = fn()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        _o, before, after = last["normalize+limiter"]
        out[shape] = {k: {"median_ms": 1e3 * statistics.median(v), "spread_ms": 1e3 * (max(v) - min(v))} for k, v in times.items()}
        out[shape]["limiter"] = {"lufs_before": before.lufs.tolist()[0], "gain_db": before.gain_db.tolist()[0],
                                 "true_peak_before_dbtp": before.true_peak_dbtp.tolist()[0],
                                 "true_peak_after_dbtp": after.true_peak_dbtp.tolist()[0], "lufs_after": after.lufs.tolist()[0]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
