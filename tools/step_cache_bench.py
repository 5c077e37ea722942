"""Cost and gain of the step cache: xxl (bf16), a synthetic 5 s video, 50-step Euler, CFG 4.5, bs=1 and bs=8, as the plain run, armed
but idle (threshold 0: the head / body split, the probe and the per-iteration read-back, no skip), under the alternate schedule
(odd iterations skipped) and in threshold mode at the threshold that gives the same number of skips (found by bisection on the
run's own reported pattern - thresholds are not calibrated for any checkpoint).  Variants are interleaved per repetition; each
figure is the median wall time of a full sampling call (noise upload, prepare, loop, DAC decode, synchronised).

    python tools/step_cache_bench.py [--reps 3] [--steps 50] [--bs 1,8] [--only plain,idle]
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
    Spec = sampler.StepCacheSpec

    models = {}                   # one context per run over the one packed arena: every run keeps its workspace and captured graphs

    def call(bs, name, spec):
        if (bs, name) not in models:
            models[(bs, name)] = sampler.FoleyModel.from_arena(cfg, model.arena, torch.bfloat16, dev)
        m = models[(bs, name)]
        sampler.denoise_process_with_generator(vis, txt, a.secs, m, dac, 4.5, a.steps, bs, "euler", generator=gen.manual_seed(0),
                                               step_cache=spec)
        return m.ctx.plan.get("step_cache_report")

    alternate = Spec(skip=tuple(range(1, a.steps, 2)))
    target = len([i for i in alternate.skip if i != a.steps - 1])

    def threshold_for(bs):
        """Bisection on the reported number of skips (monotone in the threshold up to ties); the closest count wins."""
        lo, hi, best = 0.0, 4.0, (None, None)
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            k = sum(call(bs, "search", Spec(threshold=mid))["skipped"])
            if best[0] is None or abs(k - target) < abs(best[1] - target):
                best = (mid, k)
            if k == target:
                break
            lo, hi = (mid, hi) if k < target else (lo, mid)
        return best

    skips, runs = {}, {}
    for bs in (int(b) for b in a.bs.split(",")):
        variants = {"plain": None, "idle": Spec(threshold=0.0), "alternate": alternate}
        if not a.only or "threshold" in a.only:
            th, k = threshold_for(bs)
            variants["threshold"] = Spec(threshold=th)
            skips["bs%d_threshold" % bs] = {"threshold": th, "skipped": k}
            models.pop((bs, "search"), None)
        for name, sp in variants.items():
            runs["bs%d_%s" % (bs, name)] = (lambda bs=bs, name=name, sp=sp: call(bs, name, sp))
    if a.only:
        runs = {k: f for k, f in runs.items() if any(o in k for o in a.only.split(","))}

    def once(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rep

    for f in runs.values():       # warm-up: captured graphs, table caches
        once(f)
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            t, rep = once(f)
            times[k].append(t)
            if rep is not None:
                skips.setdefault(k, {})["skipped"] = sum(rep["skipped"])
    out = {k: {"median_s": statistics.median(v), "spread_s": max(v) - min(v), "runs_s": v, **skips.get(k, {})} for k, v in times.items()}
    print(json.dumps({"workload": "xxl bf16, %g s video, %d-step Euler, CFG 4.5; alternate schedule skips %d" % (a.secs, a.steps, target),
                      "results": out}))


if __name__ == "__main__":
    main()
