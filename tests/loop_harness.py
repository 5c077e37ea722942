"""What the GPU tests of the sampling loop share (test_guidance_gpu.py, test_multistep_gpu.py, test_step_cache_gpu.py,
test_edit_gpu.py, test_windows_gpu.py, test_cond_sets_gpu.py, test_timeline_gpu.py): the tiny model with its conditionings, the
run over denoise_process_with_generator, the reader of the library's run state, and the memo of reference loops (loop_ref.py),
which the CPU tests of the loop use too."""
import ctypes

import torch

import loop_ref as L
from foley_amd.host import config as C, runtime as rt, sampler, synth


def tiny_run(dev, n_conds):
    """(sd, dsd, model, dac, conds): C.TINY in fp32 with its C.DAC_TINY decoder, and n_conds 1 s conditionings of seeds 10 + 3 i."""
    sd = synth.synth_dit_state_dict(C.TINY)
    dsd = synth.synth_dac_state_dict(C.DAC_TINY)
    model = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    dac = sampler.FoleyDAC(dsd, dev, C.DAC_TINY)
    conds = [synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd, seed=10 + 3 * i) for i in range(n_conds)]
    return sd, dsd, model, dac, conds


def batched(conds):
    """The sampler's (visual, text) feature dicts with one row per conditioning."""
    cat = lambda k: torch.cat([c[k] for c in conds])
    return ({"siglip2_feat": cat("clip"), "syncformer_feat": cat("sync")},
            {"text_feat": cat("text"), "uncond_text_feat": cat("uncond_text")})


def noise(n=1, seed=5, L=50):
    return torch.randn(n, 128, L, generator=torch.Generator().manual_seed(seed))


def run(model, dac, conds, noise, solver, steps, scale, use_graph=False, **options):
    """(audio, sample rate, latents) of a 1 s run (per window, with windows=) on the given noise."""
    vis, txt = batched(conds)
    return sampler.denoise_process_with_generator(vis, txt, 1.0, model, dac, scale, steps, noise.shape[0], solver, noise=noise,
                                                  use_graph=use_graph, return_latents=True, **options)


def run_state(model):
    """(iterations captured so far, addresses of the workspace, the schedule table, the factors) - the library's test-only entry."""
    lib = rt.load_library()
    lib.foley_debug_run_state.argtypes, lib.foley_debug_run_state.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int
    out = (ctypes.c_uint64 * 4)()
    rt._check(lib, lib.foley_debug_run_state(model.ctx._h, out), "foley_debug_run_state")
    return tuple(out)


def captures(model):
    return int(run_state(model)[0])


_LOOPS = {}


def _key(v):
    if isinstance(v, torch.Tensor):
        return (tuple(v.shape), hash(v.contiguous().numpy().tobytes()))
    if isinstance(v, dict):
        return tuple((k, _key(v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return tuple(_key(e) for e in v)
    return (tuple(v.starts), v.La) if hasattr(v, "starts") else v


def ref_loop(sd, conds, noise, steps, scale, solver="euler", **options):
    """loop_ref.restated_loop on C.TINY under the given conditionings (one: shared; several: one row each), computed once per
    distinct argument set and shared among the tests of a session: Loop(x, windows, info)."""
    key = _key((sd["final_layer.linear.weight"], conds, noise, steps, scale, solver, options))
    if key not in _LOOPS:
        cat = lambda k: torch.cat([c[k] for c in conds])
        with torch.inference_mode():
            _LOOPS[key] = L.restated_loop(sd, C.TINY.heads, noise, cat("text"), cat("uncond_text"), cat("clip"), cat("sync"), steps, scale,
                                          solver, **options)
    return _LOOPS[key]
