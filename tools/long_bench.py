"""Cost of coupling the windows of a long clip: xxl (bf16), a synthetic 34 s video, 50-step Euler, CFG 4.5, window_s = 10 with a 2 s
overlap - 4 windows at 0, 8, 16, 24 s - as ONE coupled batch (foley_set_windows), against the same four 10 s slices as an
uncoupled per-clip batch, as four sequential bs=1 runs, and against the plain single 34 s run.  Variants are interleaved per
repetition; each figure is the median wall time of a full sampling call (noise upload, prepare, loop, stitch, DAC decode,
synchronised).

    python tools/long_bench.py [--reps 3] [--steps 50] [--total 34] [--window 10] [--overlap 2] [--only windowed,uncoupled]
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
from foley_amd.host import config as C, long_form, sampler, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--total", type=float, default=34.0)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--overlap", type=float, default=2.0)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = C.XXL
    plan = long_form.plan_windows(a.total, a.window, a.overlap, cfg.frame_rate)
    n_win, W, T = plan.n_win, float(a.window), plan.Ltot / cfg.frame_rate
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev, C.DAC48K)
    wins = [synth.synth_conditioning(cfg, W, t2a=False, sd=sd, seed=1 + 3 * k, device=dev) for k in range(n_win)]
    whole = synth.synth_conditioning(cfg, T, t2a=False, sd=sd, seed=1, device=dev)

    def feats(conds):
        cat = lambda key: torch.cat([c[key] for c in conds])
        return ({"siglip2_feat": cat("clip"), "syncformer_feat": cat("sync")},
                {"text_feat": conds[0]["text"], "uncond_text_feat": conds[0]["uncond_text"]})       # one prompt for all windows

    gen = torch.Generator("cpu")

    def call(vis_txt, secs, n, windows=None):
        vis, txt = vis_txt
        sampler.denoise_process_with_generator(vis, txt, secs, model, dac, 4.5, a.steps, n, "euler", generator=gen.manual_seed(0),
                                               windows=windows)

    runs = {
        "windowed_%d_coupled" % n_win: lambda: call(feats(wins), T, 1, plan),
        "uncoupled_batch_%d" % n_win: lambda: call(feats(wins), W, n_win),
        "sequential_%d_bs1" % n_win: lambda: [call(feats(wins[k:k + 1]), W, 1) for k in range(n_win)],
        "plain_single_%gs" % T: lambda: call(feats([whole]), T, 1),
    }
    if a.only:
        runs = {k: f for k, f in runs.items() if any(k.startswith(o) for o in a.only.split(","))}

    def once(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for f in runs.values():       # warm-up: captured graphs, table caches
        once(f)
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            times[k].append(once(f))
    out = {k: {"median_s": statistics.median(v), "spread_s": max(v) - min(v), "runs_s": v} for k, v in times.items()}
    print(json.dumps({"workload": "xxl bf16, %g s as %d windows of %g s at %s, %d-step Euler, CFG 4.5"
                                  % (T, n_win, W, [s // cfg.frame_rate for s in plan.starts], a.steps), "results": out}))


if __name__ == "__main__":
    main()
