"""The one restated loop (tests/loop_ref.py) where its options meet: the refusal of windows with an edit, and the combined runs
that the GPU tests compare the engine with (test_multistep_gpu.py, test_guidance_gpu.py) - each on those tests' inputs, finite,
of the run's shape, and moved by the option far more than the 1e-4 gate of the GPU comparison.  Each option alone is pinned in
its own CPU test file (edit, windows, guidance, multistep, step cache, timeline)."""
import pytest
import torch

from conftest import rel_err
from foley_amd.host import audio_edit, config as C, long_form, step_cache as S, synth
from loop_harness import ref_loop


@pytest.fixture(scope="module")
def tiny():
    sd = synth.synth_dit_state_dict(C.TINY)
    conds = [synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd, seed=10 + 3 * i) for i in range(2)]
    return sd, conds


def _loop(sd, conds, noise, scale, solver="euler", **kw):
    return ref_loop(sd, conds, noise, 10, scale, solver, **kw)


def test_windows_with_an_edit_are_refused(tiny):
    sd, conds = tiny
    plan = long_form.WindowPlan.from_frames([0, 30], 50)
    with pytest.raises(ValueError, match="edit"):
        _loop(sd, conds[:1], torch.zeros(1, 128, 80), 4.5, windows=plan, edit=(torch.zeros(1, 128, 50), None, 1.0))


GUID = dict(g_video=7.0, interval=(0.2, 0.7), rescale=0.7)          # test_guidance_gpu.py's "all three", at text scale 2


def _inputs(name, conds):
    """(conds, noise, shape, options, the same run without the option under test) of one combined GPU test."""
    plan = long_form.WindowPlan.from_frames([0, 30, 45], 50)
    three = [conds[0], conds[1], conds[0]]
    if name == "order 3, windows":
        wn = torch.randn(1, 128, plan.Ltot, generator=torch.Generator().manual_seed(9))
        return three, wn, (1, 128, 95), dict(scale=4.5, order=3, windows=plan, shift=C.TINY.flow_shift), dict(order=None)
    if name == "order 3, skip list":
        noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
        return conds[:1], noise, (1, 128, 50), dict(scale=4.5, order=3, cache=S.StepCacheSpec(skip=(3, 6)), shift=C.TINY.flow_shift), dict(cache=None)
    g = torch.Generator().manual_seed(9)
    noise, x0 = torch.randn(1, 128, 50, generator=g), 0.7 * torch.randn(1, 128, 50, generator=g)
    plain = dict(scale=4.5, g_video=None, interval=None, rescale=0.0)
    if name == "guidance, edit":
        edit = (x0, audio_edit.build_mask(50, [(0.3, 0.6)], 0.1), 0.6)
        return conds[:1], noise, (1, 128, 50), dict(scale=2.0, solver="heun-2", edit=edit, **GUID), plain
    wn = torch.randn(1, 128, plan.Ltot, generator=g)
    return three, wn, (1, 128, 95), dict(scale=2.0, windows=plan, **GUID), plain


@pytest.mark.parametrize("name", ["order 3, windows", "order 3, skip list", "guidance, edit", "guidance, windows"])
def test_combined_runs_are_finite_and_moved_by_their_option(tiny, name):
    sd, conds = tiny
    cs, noise, shape, options, without = _inputs(name, conds)
    got = _loop(sd, cs, noise, **options)
    base = _loop(sd, cs, noise, **dict(options, **without))
    d = rel_err(got.x, base.x)
    print("%s: %.2e from the run without the option" % (name, d))
    assert got.x.shape == shape and bool(torch.isfinite(got.x).all())
    assert d > 1e-2, (name, d)
    if name == "order 3, skip list":
        assert got.info["skipped"] == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
