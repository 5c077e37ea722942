"""Time audio editing (host/audio_edit.py) on synthesised xxl weights, bf16, 5 s x 1 clip, CFG 4.5, euler: the sampling loop of a
plain run, of an edit run at strength 1 with a span mask and of a strength-0.5 run (device events around foley_sample, the plan
prepared beforehand), the solver step alone in its plain and blend forms at the run's shape, and the DAC encode alone at 5 s and
30 s.  Warm-up first; prints one JSON line per case (median / min / max over --reps).

    python tools/edit_bench.py [--reps 5] [--warmup 2] [--steps 50]
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
from foley_amd.host import audio_edit, config as C, runtime as rt, sampler, synth, tables  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, La, steps = C.XXL, 250, args.steps
    sd = synth.synth_dit_state_dict(cfg, device=dev)
    cond = synth.synth_conditioning(cfg, 5.0, t2a=True, sd=sd, device=dev)
    vis = {"siglip2_feat": cond["clip"], "syncformer_feat": cond["sync"]}
    txt = {"text_feat": cond["text"], "uncond_text_feat": cond["uncond_text"]}
    model = sampler.FoleyModel(cfg, sd, torch.bfloat16, dev)
    dac = sampler.FoleyDAC(synth.synth_dac_state_dict(C.DAC48K, device=dev, encoder=True), dev, C.DAC48K)
    model.attach_dac(dac)
    noise = torch.randn(1, 128, La, generator=torch.Generator().manual_seed(0)).to(dev)
    x0 = 0.5 * torch.randn(1, 128, La, generator=torch.Generator().manual_seed(1)).to(dev)
    mask = audio_edit.build_mask(La, [(2.0, 3.0)], 0.1).to(dev)

    def loop_case(name, strength, edit):
        if edit:
            k0, i0 = tables.edit_start(steps, "euler", strength)
            plan = sampler.build_plan(model, vis, txt, La, 4.5, steps, 1, "euler", edit_i0=i0)
            model.ctx.prepare(plan)
            model.ctx.set_edit(x0, noise, mask)
            start = rt.op_flow_mix(noise, x0, float(tables.sigma_grid(steps)[k0]))
        else:
            plan = sampler.build_plan(model, vis, txt, La, 4.5, steps, 1, "euler")
            model.ctx.prepare(plan)
            start = noise
        lat = torch.empty_like(noise)
        r = timed(lambda: (lat.copy_(start), model.ctx.sample(lat, use_graph=True)), args.reps, args.warmup)
        r.update(case=name, iterations=plan["n_iter"], median_ms_per_iter=r["median_ms"] / plan["n_iter"])
        print(json.dumps(r), flush=True)

    loop_case("plain_5s_x1_bf16", 1.0, False)
    loop_case("edit_s1.0_mask_5s_x1_bf16", 1.0, True)
    loop_case("edit_s0.5_mask_5s_x1_bf16", 0.5, True)

    # the solver step alone at the run's shape: [uncond ; cond] x 1 clip, rows in bf16, 1000 launches per timing
    coef = tables.edit_solver_table(tables.sigma_grid(1000), "euler", 1000).to(dev)
    pred = torch.randn(2 * La, 128, device=dev)
    x, rows = noise.clone(), torch.empty(2 * La, 128, dtype=torch.bfloat16, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)

    def steps_plain():
        step.zero_()
        for _ in range(1000):
            rt.op_solver_step(pred, x, None, None, 2, 4.5, coef, step, rows)

    def steps_blend():
        step.zero_()
        for _ in range(1000):
            rt.op_solver_step(pred, x, None, None, 2, 4.5, coef, step, rows, edit=(x0, noise, mask))

    for name, fn in (("solver_step_plain", steps_plain), ("solver_step_blend", steps_blend)):
        r = timed(fn, args.reps, args.warmup)
        r.update(case=name + "_5s_x1", us_per_step=r["median_ms"])      # 1000 steps per timing: ms -> us per step
        print(json.dumps(r), flush=True)

    for sec in (5.0, 30.0):
        wave = 0.1 * torch.randn(1, int(sec * 48000), generator=torch.Generator().manual_seed(2)).to(dev)
        r = timed(lambda: audio_edit.encode_source(wave, model, dac, int(sec * 50)), args.reps, args.warmup)
        r.update(case=f"encode_{sec:g}s_x1")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
