"""The step cache without a GPU: the policy state machine of host/step_cache.py against hand-worked sequences, the spec and node
refusals, what build_plan hands to the library, the restated loop of tests/loop_ref.py under it against the plain one, the C surface."""
import os
import re

import pytest
import torch

import loop_ref as L
from abi_pin import assert_abi_version
from conftest import ROOT, rel_err
from foley_amd import nodes
from foley_amd.host import config as C, runtime as rt, sampler, step_cache as S, synth

Spec, Policy = S.StepCacheSpec, S.StepCachePolicy


# ----------------------------------------------------------------------------- the state machine, by hand
def test_schedule_mode_skips_the_listed_iterations_but_never_the_forced_ones():
    p = Policy.from_spec(Spec(skip=range(8)), 8)                       # everything listed: 0 and 7 stay full
    assert p.pattern([0.0] * 8) == [0, 1, 1, 1, 1, 1, 1, 0]
    p = Policy.from_spec(Spec(skip=(1, 3, 4)), 6)
    assert p.pattern([9.9] * 6) == [0, 1, 0, 1, 1, 0]                  # rel plays no part
    assert Policy.from_spec(Spec(skip=()), 5).pattern([0.0] * 5) == [0] * 5


def test_threshold_mode_accumulates_and_resets():
    """rel 0.1 per iteration, threshold 0.25: 0.1 skip, 0.2 skip, 0.3 full (reset), 0.1 skip, ... - runs of two skips."""
    p = Policy.from_spec(Spec(threshold=0.25), 9)
    seen = []
    for i in range(9):
        skip = p.decide(i, -1.0 if i == 0 else 0.1)
        seen.append((int(skip), round(p.last_acc, 6)))
    assert seen == [(0, 0.0), (1, 0.1), (1, 0.2), (0, 0.3), (1, 0.1), (1, 0.2), (0, 0.3), (1, 0.1), (0, 0.2)]   # the last one is full
    # a single large change forces a full iteration at once; an accumulator equal to the threshold is not below it
    assert Policy.from_spec(Spec(threshold=0.25), 6).pattern([-1, 0.1, 0.5, 0.25, 0.1, 0.1]) == [0, 1, 0, 0, 1, 0]
    # threshold 0 never skips: armed but idle
    assert Policy.from_spec(Spec(threshold=0.0), 6).pattern([-1] + [0.0] * 5) == [0] * 6


def test_interval_cap_and_polynomial():
    rel = [-1.0] + [0.01] * 9
    assert Policy.from_spec(Spec(threshold=1.0), 10).pattern(rel) == [0] + [1] * 8 + [0]
    # interval (0.3, 0.7) of 10 iterations: only 3..6 may skip; outside it the iterations are full and reset the accumulator
    assert Spec(threshold=1.0, interval=(0.3, 0.7)).interval_rows(10) == (3, 7)
    assert Policy.from_spec(Spec(threshold=1.0, interval=(0.3, 0.7)), 10).pattern(rel) == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    # at most two skips in a row
    assert Policy.from_spec(Spec(threshold=1.0, max_consecutive=2), 10).pattern(rel) == [0, 1, 1, 0, 1, 1, 0, 1, 1, 0]
    # poly highest degree first: 100 rel^2 + 0.5 at rel 0.1 adds 1.5 per iteration, threshold 2 -> skip, full, skip, full, ...
    p = Policy.from_spec(Spec(threshold=2.0, poly=(100.0, 0.0, 0.5)), 7)
    assert p.pattern([-1.0] + [0.1] * 6) == [0, 1, 0, 1, 0, 1, 0]
    assert Spec(threshold=1.0, interval=(0.0, 0.0)).interval_rows(10) == (0, 0)


def test_edit_runs_use_the_suffix_of_the_list_and_of_the_interval():
    spec = Spec(skip=(1, 4, 5, 7))
    assert spec.skip_rows(10) == [0, 1, 0, 0, 1, 1, 0, 1, 0, 0] and spec.skip_rows(10, 4) == [1, 1, 0, 1, 0, 0]
    # the suffix starts without a delta: its iteration 0 (the plain run's 4) is full although the list names it
    assert Policy.from_spec(spec, 10, 4).pattern([0.0] * 6) == [0, 1, 0, 1, 0, 0]
    th = Spec(threshold=1.0, interval=(0.3, 0.7))
    assert th.interval_rows(10, 4) == (0, 3) and th.interval_rows(10, 8) == (0, 0)
    assert Policy.from_spec(th, 10, 4).pattern([-1.0] + [0.01] * 5) == [0, 1, 1, 0, 0, 0]


# ----------------------------------------------------------------------------- refusals
def test_spec_refusals():
    for bad in (Spec(), Spec(threshold=0.1, skip=(1,)), Spec(threshold=-0.1), Spec(threshold=float("nan")), Spec(threshold=float("inf")),
                Spec(skip=(10,)), Spec(skip=(-1,)), Spec(skip=(1,), interval=(0.0, 1.0)), Spec(skip=(1,), max_consecutive=2),
                Spec(threshold=0.1, max_consecutive=0), Spec(threshold=0.1, interval=(0.5, 0.2)), Spec(threshold=0.1, poly=())):
        with pytest.raises(ValueError, match="step cache"):
            bad.check(10)
    Spec(threshold=0.0).check(10)
    Spec(skip=(0, 9)).check(10)
    with pytest.raises(ValueError, match="one entry per iteration"):
        Policy(10, S.MODE_SCHEDULE, skip=[0] * 9)


def test_node_refusals():
    node = nodes.HunyuanFoleySampler()
    args = (None, None, 16, 1.0, "p", "n", 4.5, 10, "euler", 1, 0, True)
    with pytest.raises(ValueError, match="cache_threshold and cache_skip together"):
        node.generate_audio(*args, cache_threshold=0.2, cache_skip=[1, 3])
    with pytest.raises(ValueError, match=r"outside \[0, 10\)"):
        node.generate_audio(*args, cache_skip=[3, 10])
    with pytest.raises(ValueError, match=r"outside \[0, 10\)"):
        node.generate_audio(*args, cache_skip=[-1])
    with pytest.raises(ValueError, match="finite and >= 0"):
        node.generate_audio(*args, cache_threshold=-1.0)
    with pytest.raises(ValueError, match="pass cache_threshold"):
        node.generate_audio(*args, cache_interval=(0.1, 0.9))
    # no new socket or widget: existing workflows load unchanged
    inputs = nodes.HunyuanFoleySampler.INPUT_TYPES()
    assert not any(k.startswith("cache_") for group in inputs.values() for k in group)


def test_node_logs_one_line_per_context(caplog):
    class _Ctx:
        def __init__(self, plan):
            self.plan = plan

    class _M:
        def __init__(self, plan):
            self.ctx = _Ctx(plan)
    with caplog.at_level("INFO", logger=nodes.log.name):
        nodes.log_step_cache([_M({"step_cache_report": {"rel": [-1.0, 0.1, 0.1, 0.1], "skipped": [0, 1, 1, 0]}}), _M({}), _M(None)])
    lines = [r.getMessage() for r in caplog.records if r.name == nodes.log.name]
    assert lines == ["step cache: skipped 2 of 4 iterations"]


# ----------------------------------------------------------------------------- the restated loop
@pytest.fixture(scope="module")
def tiny():
    sd = synth.synth_dit_state_dict(C.TINY)
    c = synth.synth_conditioning(C.TINY, 1.0, t2a=False, sd=sd, seed=10)
    noise = torch.randn(1, 128, 50, generator=torch.Generator().manual_seed(5))
    return sd, c, noise


def test_restated_loop_idle_is_the_plain_loop_and_skipping_moves_it(tiny):
    sd, c, noise = tiny
    a = (sd, C.TINY.heads, noise, c["text"], c["uncond_text"], c["clip"], c["sync"], 10, 4.5, "heun-2")
    with torch.inference_mode():
        plain = L.restated_loop(*a).x
        off = L.restated_loop(*a, cache=None).x
        idle, _, info = L.restated_loop(*a, cache=Spec(threshold=0.0))
        alt, _, ia = L.restated_loop(*a, cache=Spec(skip=range(1, 10, 2)))
    assert torch.equal(off, plain) and torch.equal(idle, plain)
    assert info["skipped"] == [0] * 10 and info["rel"][0] == -1.0 and all(0.05 < r < 0.3 for r in info["rel"][1:])
    assert ia["skipped"] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 0]
    assert 1e-2 < rel_err(alt, plain) < 5e-2


# ----------------------------------------------------------------------------- what the library is handed, the C surface
def test_build_plan_carries_the_library_arguments(tiny):
    class _M:                                               # build_plan reads the config, the device and the empty rows only
        cfg, device, dtype, quantization, _text_len_fixed = C.TINY, torch.device("cpu"), torch.float32, "none", None
        empty_clip_feat, empty_sync_feat = tiny[0]["empty_clip_feat"].view(1, -1), tiny[0]["empty_sync_feat"].view(1, -1)
        get_empty_clip_sequence = sampler.FoleyModel.get_empty_clip_sequence
        get_empty_sync_sequence = sampler.FoleyModel.get_empty_sync_sequence
    c = tiny[1]
    vis, txt = {"siglip2_feat": c["clip"], "syncformer_feat": c["sync"]}, {"text_feat": c["text"], "uncond_text_feat": c["uncond_text"]}
    m = _M()
    assert "step_cache" not in sampler.build_plan(m, vis, txt, 50, 4.5, 10, 1, "euler")
    pl = sampler.build_plan(m, vis, txt, 50, 4.5, 10, 1, "euler", step_cache=Spec(skip=(1, 3)))
    assert pl["step_cache"] == {"mode": 1, "skip": [0, 1, 0, 1, 0, 0, 0, 0, 0, 0]}
    pl = sampler.build_plan(m, vis, txt, 50, 4.5, 10, 1, "euler", edit_i0=2, step_cache=Spec(threshold=0.2, interval=(0.3, 0.7), max_consecutive=2))
    assert pl["step_cache"] == {"mode": 2, "threshold": 0.2, "poly": None, "interval": (1, 5), "max_consecutive": 2}
    with pytest.raises(ValueError, match="step cache"):
        sampler.build_plan(m, vis, txt, 50, 4.5, 10, 1, "euler", step_cache=Spec(skip=(10,)))


def test_new_symbols_declared_and_exported():
    """Fails without the feature: the built library exports the step cache's entries with the declared signatures."""
    hdr = open(os.path.join(ROOT, "include", "foley_hip.h")).read()
    lib = rt.load_library()
    for name in ("foley_set_step_cache", "foley_step_cache_report", "foley_op_cache_probe", "foley_op_cache_probe_work",
                 "foley_op_cache_delta", "foley_op_cache_apply"):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", hdr), name
        assert name in rt.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"int foley_set_step_cache\(foley_ctx\* ctx, int mode, const uint8_t\* skip, int n_skip, double threshold, "
                     r"const double\* poly,\s+int n_poly, const int32_t\* interval, int max_consecutive, void\* stream\);", hdr)
    assert re.search(r"int foley_step_cache_report\(foley_ctx\* ctx, float\* rel, int32_t\* skipped, int n\);", hdr)
    assert "#define FOLEY_STEP_CACHE_SCHEDULE 1" in hdr and "#define FOLEY_STEP_CACHE_THRESHOLD 2" in hdr
    assert S.MODE_SCHEDULE == 1 and S.MODE_THRESHOLD == 2
    assert_abi_version()
    # the probe's scratch: two floats per workgroup of four rows, per batch row
    assert lib.foley_op_cache_probe_work(1, 50) == 13 * 2 and lib.foley_op_cache_probe_work(6, 33) == 6 * 9 * 2
    assert lib.foley_op_cache_probe_work(0, 50) == 0
    # refusals that need no device: a null context
    assert lib.foley_set_step_cache(None, 1, None, 0, 0.0, None, 0, None, 0, None) != 0
    assert b"null context" in lib.foley_last_error()
