"""Cost of the guidance controls: xxl (bf16), a synthetic 5 s video, 50-step Euler, bs=1 and bs=8, as the plain two-half run
(CFG 4.5), the same with a guidance schedule (interval), with CFG rescale, with projected guidance (`apg`: momentum -0.5, eta 0;
`zero_star`: CFG-Zero* with one zero-velocity iteration), and as a three-half run (separate video and text scales: 1.5x the rows).  Variants are interleaved per repetition; each figure is the median wall time of a full sampling call
(noise upload, prepare, loop, DAC decode, synchronised).

    python tools/guidance_bench.py [--reps 3] [--steps 50] [--bs 1,8] [--only plain,rescale]
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
    ap.add_argument("--secs", type=float, default=5.0)
    ap.add_argument("--bs", default="1,8")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev, C.DAC48K)
    cond = synth.synth_conditioning(cfg, a.secs, t2a=False, sd=sd, seed=1, device=dev)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    gen = torch.Generator("cpu")
    Spec = sampler.GuidanceSpec

    models = {}                   # one context per run over the one packed arena: every run keeps its workspace and captured graph

    def call(bs, name, spec):
        if (bs, name) not in models:
            models[(bs, name)] = sampler.FoleyModel.from_arena(cfg, model.arena, torch.bfloat16, dev)
        sampler.denoise_process_with_generator(vis, txt, a.secs, models[(bs, name)], dac, 4.5, a.steps, bs, "euler",
                                               generator=gen.manual_seed(0), guidance=spec)

    Proj = sampler.ProjectionSpec
    variants = {"plain": None, "schedule": Spec(interval=(0.2, 0.7)), "rescale": Spec(rescale=0.7),
                "apg": Spec(projection=Proj("apg", 0.0, -0.5)), "zero_star": Spec(projection=Proj("cfg_zero_star", zero_init=1)),
                "three_halves": Spec(g_video=3.0)}
    runs = {"bs%d_%s" % (bs, k): (lambda bs=bs, k=k, sp=sp: call(bs, k, sp)) for bs in (int(b) for b in a.bs.split(",")) for k, sp in variants.items()}
    if a.only:
        runs = {k: f for k, f in runs.items() if any(o in k for o in a.only.split(","))}

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
    print(json.dumps({"workload": "xxl bf16, %g s video, %d-step Euler, CFG 4.5 (three halves: video 3.0 / text 4.5)" % (a.secs, a.steps),
                      "results": out}))


if __name__ == "__main__":
    main()
