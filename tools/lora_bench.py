"""Merge time of a rank-16 / rank-128 LoRA adapter on every block matrix of xxl (synthetic weights), bf16 and e4m3fn arenas: the
median of five lora.ensure calls after a warm one, the restore and the merges of such a call timed apart, a device-to-device copy
of as many bytes as the pristine copies hold in the same process, and one tensor of each layout kind merged alone at rank 128.
Prints one JSON line per case and one with all of them.

    python tools/lora_bench.py
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package
load_package()
import torch
from foley_amd.host import config as C, lora, sampler, synth

dev = torch.device("cuda:0")
cfg = C.XXL
out = {}
sd = synth.synth_dit_state_dict(cfg, device=dev)
dsd = synth.synth_dac_state_dict(C.DAC_TINY, device=dev)
shapes = {k: v[0] for k, v in synth.dit_schema(cfg).items()}
mods = [m for m in lora.modules(cfg) if m.startswith(("triple_blocks.", "single_blocks."))]
print(len(mods), "block matrices", flush=True)
g = torch.Generator(device=dev).manual_seed(0)


def adapter(rank):
    a = {}
    for m in mods:
        s = shapes[m + ".weight"]
        a[m + ".lora_down.weight"] = (torch.randn((rank,) + tuple(s[1:]), device=dev, generator=g) * 0.02).bfloat16()
        a[m + ".lora_up.weight"] = (torch.randn((s[0], rank) + (1,) * (len(s) - 2), device=dev, generator=g) * 0.02).bfloat16()
    return a


def sync():
    torch.cuda.synchronize(dev)


for label, quant in (("bf16", "none"), ("bf16+e4m3fn", "fp8_e4m3fn")):
    model = sampler.FoleyModel.from_reference_state(cfg, sd, torch.bfloat16, dev, dsd, dac_cfg=C.DAC_TINY, quantization=quant)
    for rank in (16, 128):
        ad = adapter(rank)
        lora.ensure(model, [(ad, 0.5)])          # warm: takes the pristine copies
        sync()
        nbytes = model.ctx.lora_backup_bytes()
        plan = lora.plan_merge([(ad, 0.7)], cfg)
        t_ens, t_rest, t_merge = [], [], []
        for i in range(5):
            sync(); t0 = time.perf_counter()
            lora.ensure(model, [(ad, 0.6 + 0.01 * i)])
            sync(); t_ens.append(time.perf_counter() - t0)
        for i in range(5):
            sync(); t0 = time.perf_counter()
            model.ctx.lora_begin()
            sync(); t1 = time.perf_counter()
            for key, lst in plan.items():
                model.ctx.lora_merge(key, lst)
            model.ctx.lora_end()
            sync(); t2 = time.perf_counter()
            t_rest.append(t1 - t0); t_merge.append(t2 - t1)
        a_, b_ = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        t_copy = []
        for i in range(6):
            sync(); t0 = time.perf_counter()
            b_.copy_(a_)
            sync(); t_copy.append(time.perf_counter() - t0)
        del a_, b_
        med = lambda v: statistics.median(v) * 1e3
        rec = {"tensors": len(plan), "backup_GB": nbytes / 1e9, "ensure_ms": med(t_ens), "restore_ms": med(t_rest), "merge_ms": med(t_merge),
               "copy_ms": med(t_copy[1:]), "merge_GBps_rw": 2 * nbytes / statistics.median(t_merge) / 1e9,
               "copy_GBps_rw": 2 * nbytes / statistics.median(t_copy[1:]) / 1e9}
        out[f"{label} rank {rank}"] = rec
        print(label, rank, json.dumps(rec), flush=True)
        # per layout kind: one tensor of each, merge alone
        if rank == 128:
            for key in ("triple_blocks.0.audio_mlp.fc1.weight", "single_blocks.0.linear_qkv.weight", "single_blocks.0.linear1.weight",
                        "single_blocks.0.linear2.w1.weight", "single_blocks.0.linear2.w2.weight", "single_blocks.0.modulation.linear.weight"):
                ts = []
                for i in range(4):
                    model.ctx.lora_begin(); sync(); t0 = time.perf_counter()
                    model.ctx.lora_merge(key, plan[key]); sync(); ts.append(time.perf_counter() - t0)
                    model.ctx.lora_end()
                n = 1
                for v in shapes[key]:
                    n *= v
                es = 1 if (quant != "none") else 2
                print(f"   {label} {key}: {statistics.median(ts[1:]) * 1e3:.3f} ms, {2 * n * es / statistics.median(ts[1:]) / 1e9:.0f} GB/s r+w", flush=True)
        lora.ensure(model, None)
        del ad, plan
    model.ctx.close()
    del model
    torch.cuda.empty_cache()
print(json.dumps(out))
