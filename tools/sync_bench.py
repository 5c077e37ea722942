"""Time the sync scorer (host/sync_score.py::sync_scores) on synthesised weights: B = 6 clips at 5 s and at 8 s, fp16 operands,
48 kHz input (resampling included), device events around each call after warm-up.  Prints one JSON line per case.

    python tools/sync_bench.py [--reps 10] [--warmup 3]
    rocprofv3 --kernel-trace --stats -d <dir> -o sync -- python tools/sync_bench.py --reps 3     (the kernel table, a run of its own)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from foley_amd.host import encoders as E, sync_score as S, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=6)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    deps = {"sync_score_model": synth.materialize(E.synchformer_sync_schema())}
    for sec in (5.0, 8.0):
        wav = synth.synth_click_audio(args.batch, int(sec * 48000), 48000).unsqueeze(1).to(dev)
        s_v = (int(sec * 25) - 16) // 8 + 1
        feat = synth.synth_tensor("bench.vfeat", (1, s_v * 8, 768), 1.0).to(dev)
        for _ in range(args.warmup):
            S.sync_scores(deps, wav, 48000, syncformer_feat=feat)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = S.sync_scores(deps, wav, 48000, syncformer_feat=feat)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        print(json.dumps({"case": f"B{args.batch}_{sec:g}s_fp16", "windows": len(r.starts), "median_ms": times[len(times) // 2],
                          "min_ms": times[0], "max_ms": times[-1], "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
