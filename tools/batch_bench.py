"""Cost of per-clip conditioning: the 5 s / 50-step Euler / CFG 4.5 xxl (bf16) loop at bs=8 with every clip sharing its
conditioning (homogeneous), with 8 different prompts (text-to-audio), with 8 different synthetic videos, and the same 8 videos as
8 sequential bs=1 runs.  Variants are interleaved per repetition; each figure is the median wall time of a full sampling call
(noise upload, prepare, loop, DAC decode, synchronised), reported as audio-s/s.

    python tools/batch_bench.py [--reps 3] [--steps 50] [--duration 5]
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
from foley_amd.host import config as C, sampler, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--duration", type=float, default=5.0)
    ap.add_argument("--bs", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, bs, dur = C.XXL, a.bs, a.duration
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev, C.DAC48K)
    t2a = [synth.synth_conditioning(cfg, dur, t2a=True, sd=sd, seed=1 + 3 * k, device=dev) for k in range(bs)]
    v2a = [synth.synth_conditioning(cfg, dur, t2a=False, sd=sd, seed=1 + 3 * k, device=dev) for k in range(bs)]

    def feats(conds, shared_text=False):
        cat = lambda key: torch.cat([c[key] for c in conds])
        txt = {"text_feat": cat("text"), "uncond_text_feat": cat("uncond_text")}
        if shared_text:
            txt = {k: v[:1] for k, v in txt.items()}
        return {"siglip2_feat": cat("clip"), "syncformer_feat": cat("sync")}, txt

    runs = {
        "homogeneous_bs%d" % bs: [(feats(t2a[:1]), bs)],
        "t2a_%d_prompts" % bs: [(feats(t2a), bs)],
        "v2a_%d_videos" % bs: [(feats(v2a, shared_text=True), bs)],
        "v2a_%d_sequential_bs1" % bs: [(feats(v2a[k:k + 1]), 1) for k in range(bs)],
    }
    gen = torch.Generator("cpu")

    def once(parts):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (vis, txt), n in parts:
            sampler.denoise_process_with_generator(vis, txt, dur, model, dac, 4.5, a.steps, n, "euler", generator=gen.manual_seed(0))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for parts in runs.values():       # warm-up: captured graphs, table caches
        once(parts)
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, parts in runs.items():
            times[k].append(once(parts))
    out = {k: {"median_s": statistics.median(v), "audio_s_per_s": bs * dur / statistics.median(v), "runs_s": v}
           for k, v in times.items()}
    print(json.dumps({"workload": "xxl bf16, %g s, %d-step Euler, CFG 4.5, %d clips" % (dur, a.steps, bs), "results": out}))


if __name__ == "__main__":
    main()
