"""Time a FlowEdit sampling call (host/audio_edit.py::FlowEditSpec) against the plain run of the same batch on synthesised xxl
weights, bf16, 5 s, one variation, euler: the FlowEdit loop (two batch clips: the source and the target branch) and the plain loop
of two clips with two prompts, ALTERNATED in one process after warm-up (device events around foley_sample, the plans prepared
beforehand, each on a context of its own so that neither re-prepares).  Only the step launch differs between the two.  Prints one
JSON line per case: the median and the spread (min, max) over --reps.

    python tools/flowedit_bench.py [--reps 7] [--warmup 2] [--steps 50]

For the step kernels' own times run it under a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o kt -- python tools/flowedit_bench.py --reps 2 --warmup 1
    python tools/prof_summary.py $(find <dir> -name "*.db" | head -1)
and read flowedit_step_kernel / solver_step_kernel in the table.
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
from foley_amd.host import audio_edit, config as C, sampler, synth, tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, La, steps, V = C.XXL, 250, args.steps, 1
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    other = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev, seed=17)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"source_text_feat": cond["text"], "text_feat": other["text"], "uncond_text_feat": cond["uncond_text"]}
    _v, pair_txt = sampler.flowedit_features(vis, txt, V)
    models = [sampler.FoleyModel(cfg, sd, torch.bfloat16, dev) for _ in range(2)]
    x0 = 0.5 * torch.randn(1, 128, La, generator=torch.Generator().manual_seed(1)).to(dev)
    noise = torch.randn(2 * V, 128, La, generator=torch.Generator().manual_seed(0)).to(dev)
    table = audio_edit.flowedit_noise(torch.Generator().manual_seed(2), steps, V, 128, La, torch.float32).to(dev)

    fe, plain = models
    fe.ctx.prepare(sampler.build_plan(fe, vis, pair_txt, La, 4.5, steps, 2 * V, "euler", edit_i0=0))
    fe.ctx.set_flowedit(x0, table, None, g_src=2.0, g_tar=4.5, sigma0=float(tables.sigma_grid(steps)[0]))
    plain.ctx.prepare(sampler.build_plan(plain, vis, pair_txt, La, 4.5, steps, 2 * V, "euler"))
    z, lat = x0.clone(), noise.clone()
    cases = {"flowedit_5s_v1_bf16": lambda: (z.copy_(x0), fe.ctx.sample(z, use_graph=True)),
             "plain_5s_x2_two_prompts_bf16": lambda: (lat.copy_(noise), plain.ctx.sample(lat, use_graph=True))}
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):                       # alternate: drift of the device's clocks falls on both alike
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name, t in times.items():
        t.sort()
        print(json.dumps({"case": name, "median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": len(t), "iterations": steps,
                          "median_ms_per_iter": t[len(t) // 2] / steps}), flush=True)


if __name__ == "__main__":
    main()
