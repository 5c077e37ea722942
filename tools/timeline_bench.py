"""Cost of a prompt timeline: bench.py's default workload shape - xxl (bf16), text-to-audio 5 s, 50-step Euler, CFG 4.5 - as a plain
run and under a three-segment timeline with 0.25 s ramps, at bs=1 and bs=8.  A timeline run loses the cross-attention fused into
its q projection's epilogue: 18 more launches per iteration on small grids.  The two variants are interleaved per repetition in
one process; each figure is the median wall time of a full sampling call (noise upload, prepare, loop, DAC decode, synchronised).

    python tools/timeline_bench.py [--reps 3] [--steps 50] [--bs 1,8] [--only timeline] [--profile]

--profile adds the per-op event profile of one eager forward (foley_profile_forward) for every variant: the cross-attention rows -
the timeline kernel against the plain path's q projection with its fused attention, or its separate attention launch.
The plain and the timeline runs use a context each (their workspaces differ in the cached text sets), so interleaving them
measures the runs, not the switch.

For the kernels alone, run it under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) with --only timeline and
--only plain, and compare the attn_tl16_kernel rows with the plain path's cross-attention.
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
from foley_amd.host import config as C, prompt_timeline, sampler, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--duration", type=float, default=5.0)
    ap.add_argument("--bs", default="1,8")
    ap.add_argument("--only", default="")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = C.XXL
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    model = {False: sampler.FoleyModel(cfg, sd, torch.bfloat16, dev), True: sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)}
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev), dev, C.DAC48K)
    conds = [synth.synth_conditioning(cfg, a.duration, t2a=True, sd=sd, seed=1 + 3 * k, device=dev) for k in range(3)]
    T = a.duration
    tl = prompt_timeline.parse([(0.0, 0.4 * T, "a"), (0.4 * T, 0.7 * T, "b")], "c", T, 0.25)
    vis = {"siglip2_feat": conds[0]["clip"], "syncformer_feat": conds[0]["sync"]}
    pad = lambda t: sampler.pad_or_trim_text(t, 77)
    unc = pad(conds[0]["uncond_text"])
    txt_plain = {"text_feat": pad(conds[0]["text"]), "uncond_text_feat": unc}
    txt_timed = {"text_feat": torch.cat([pad(c["text"]) for c in conds]), "uncond_text_feat": unc}
    gen = torch.Generator("cpu")

    def call(txt, n, timeline):
        sampler.denoise_process_with_generator(vis, txt, T, model[timeline is not None], dac, 4.5, a.steps, n, "euler",
                                               generator=gen.manual_seed(0), timeline=timeline)

    runs = {}
    for n in [int(b) for b in a.bs.split(",")]:
        runs["plain_bs%d" % n] = lambda n=n: call(txt_plain, n, None)
        runs["timeline_bs%d" % n] = lambda n=n: call(txt_timed, n, tl)
    if a.only:
        runs = {k: f for k, f in runs.items() if any(k.startswith(o) for o in a.only.split(","))}

    def once(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for f in runs.values():       # warm-up: captured graphs, table caches (alternating variants re-capture: part of what is measured)
        once(f)
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            times[k].append(once(f))
    out = {k: {"median_s": statistics.median(v), "spread_s": max(v) - min(v), "runs_s": v} for k, v in times.items()}
    for k in list(out):
        if k.startswith("timeline_") and "plain_" + k[len("timeline_"):] in out:
            out[k]["ratio_to_plain"] = out[k]["median_s"] / out["plain_" + k[len("timeline_"):]]["median_s"]
    prof = {}
    if a.profile:
        for k, f in runs.items():
            f()                   # leaves the variant's plan prepared on its context
            m = model[k.startswith("timeline")]
            pl = m.ctx.plan
            lat = torch.randn(pl["clips"], cfg.latent_dim, pl["La"], device=dev)
            rows, _bracket = m.ctx.profile_forward(lat, 0, 3)
            prof[k] = [{"label": r["label"], "kernel": r["kernel"][:60], "calls_per_forward": r["calls_per_forward"], "avg_us": round(r["avg_us"], 2)}
                       for r in rows if "cross" in r["label"]]
    print(json.dumps({"profile_cross_rows": prof, "workload": "xxl bf16, text-to-audio %g s, %d-step Euler, CFG 4.5; timeline: 3 segments, 0.25 s ramps, %d text sets"
                                  % (T, a.steps, len(tl.prompts) + 1), "results": out}))


if __name__ == "__main__":
    main()
