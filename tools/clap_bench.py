"""Time the CLAP scorer (host/clap_score.py::clap_scores) on synthesised weights of the released architecture (HTSAT-base:
patch_embeds_hidden_size 128, depths 2 / 2 / 12 / 2, heads 4 / 8 / 16 / 32; RoBERTa-base text tower): B = 6 clips at 5 s (one
window each) and at 23 s (three windows each), fp16 operands, 48 kHz input, device events around each call after a warm-up,
median of the repetitions.  Prints one JSON line per case: the whole call (audio tower + text tower + cosine) and the audio
tower alone.

    python tools/clap_bench.py [--reps 5] [--warmup 2]
    rocprofv3 --kernel-trace --stats -d <dir> -o clap -- python tools/clap_bench.py --reps 3     (the kernel table, a run of its own)
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
from foley_amd.host import clap_score as CS, encoders_hip as EH, synth  # noqa: E402


class ByteTokenizer:
    """<s> bytes </s>, right-padded with <pad> = 1 (a stand-in for the Roberta tokenizer: the bench needs token ids, not words)."""

    def __call__(self, texts, padding=True, return_tensors="pt"):
        ids = [[0] + [3 + (b % 250) for b in t.encode()][:75] + [2] for t in texts]
        n = max(len(i) for i in ids)
        batch = {"input_ids": torch.tensor([i + [1] * (n - len(i)) for i in ids]),
                 "attention_mask": torch.tensor([[1] * len(i) + [0] * (n - len(i)) for i in ids])}

        class B(dict):
            def to(self, dev):
                return B({k: v.to(dev) for k, v in self.items()})
        return B(batch)


def build_deps():
    from transformers import ClapConfig, ClapFeatureExtractor, ClapModel
    torch.manual_seed(0)
    cfg = ClapConfig(audio_config=dict(patch_embeds_hidden_size=128, depths=[2, 2, 12, 2], num_attention_heads=[4, 8, 16, 32],
                                       hidden_size=1024, enable_fusion=False),
                     text_config=dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                                      vocab_size=50265, max_position_embeddings=514), projection_dim=512)
    model = ClapModel(cfg).eval()
    ex = ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad")
    return {"clap_score_model": (model.state_dict(), CS.config_dict(model.config, ex)), "clap_tokenizer": ByteTokenizer()}


def timed(fn, warmup, reps):
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
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=6)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    deps = build_deps()
    prompt = "footsteps on gravel, a door slams"
    for sec in (5.0, 23.0):
        wav = synth.synth_click_audio(args.batch, int(sec * 48000), 48000).unsqueeze(1).to(dev)
        last = {}
        total = timed(lambda: last.__setitem__("r", CS.clap_scores(deps, wav, 48000, prompt)), args.warmup, args.reps)
        sd, cfg = deps["clap_score_model"]
        E = EH._engine_for(sd, dev, torch.float16)
        w48 = CS.prepare_waveform(deps, wav, 48000)
        tower = timed(lambda: CS.audio_embeds_hip(sd, cfg, w48, E, CS._tables(deps, dev, cfg)), 1, args.reps)
        print(json.dumps({"case": f"B{args.batch}_{sec:g}s_fp16", "windows": len(last["r"].starts), "median_ms": total[len(total) // 2],
                          "min_ms": total[0], "max_ms": total[-1], "audio_tower_median_ms": tower[len(tower) // 2], "reps": args.reps}),
              flush=True)


if __name__ == "__main__":
    main()
