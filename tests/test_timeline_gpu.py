"""The prompt timeline on the HIP engine: the loop against the oracle restatement with timed text (tests/timeline_ref.py), a
one-span timeline against the plain run, the keying of the captured graph (on the timeline state, and across runs that differ in
several options at once), the refusals of foley_prepare_timeline, a bf16 run."""
import ctypes

import pytest
import torch

import loop_harness as H
import timeline_ref as TR
from conftest import rel_err
from foley_amd.host import audio_edit, config as C, long_form, prompt_timeline as PT, runtime as rt, sampler
from oracle import foley_oracle as O

pytestmark = pytest.mark.gpu

LA, STEPS, CFG = 50, 10, 4.5
PLAN = dict(starts=[0, 30, 45], La=50)             # the windows of test_windows_gpu: Ltot 95


@pytest.fixture(scope="module")
def tiny(dev):
    sd, dsd, model, dac, conds = H.tiny_run(dev, 3)
    texts = torch.cat([O.pad_or_trim_text(c["text"], 77) for c in conds])        # the features of prompts "a", "b", "c"
    unc = O.pad_or_trim_text(conds[0]["uncond_text"], 77)
    return sd, dsd, model, dac, conds[0], texts, unc


THREE = ([(0.0, 0.3, "a"), (0.3, 0.7, "b")], "c", 0.2)          # a | b | c (the base prompt) with 0.2 s ramps at 0.3 s and 0.7 s
_ROW = {"a": 0, "b": 1, "c": 2}


def _timeline(spans, base, crossfade, duration=1.0):
    return PT.parse(spans, base, duration, crossfade)


def _cond(cond, texts, unc, tl, plain=None):
    """The clip's conditioning with the timeline's prompts as its text rows (no timeline: the one prompt `plain`)."""
    rows = texts[[_ROW[p] for p in tl.prompts]] if tl is not None else texts[_ROW[plain]:_ROW[plain] + 1]
    return dict(cond, text=rows, uncond_text=unc)


def _run(model, dac, cond, texts, unc, tl, noise, solver="euler", use_graph=False, plain=None, edit=None, windows=None, dtype_model=None):
    return H.run(dtype_model or model, dac, [_cond(cond, texts, unc, tl, plain)], noise, solver, STEPS, CFG, use_graph, timeline=tl,
                 edit=edit, windows=windows)[2]


_ORACLE = {}


def _oracle(sd, cond, texts, unc, tl, noise, solver):
    key = (tl.key() if tl is not None else None, solver)
    if key not in _ORACLE:
        sets = torch.cat([unc, texts[[_ROW[p] for p in tl.prompts]]])
        flat = PT.batch_table(tl, cond["clip"].shape[1], LA, 2, noise.shape[0])
        with torch.inference_mode():
            _ORACLE[key] = TR.oracle_timeline_latents(sd, C.TINY.heads, noise, sets, flat, cond["clip"], cond["sync"], STEPS, CFG, solver)
    return _ORACLE[key]


@pytest.mark.parametrize("solver", ["euler", "heun-2"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_three_segment_timeline_matches_oracle(tiny, solver, use_graph):
    sd, _dsd, model, dac, cond, texts, unc = tiny
    tl = _timeline(*THREE)
    assert tl.prompts == ("a", "b", "c") and any(s.h_hi > 0 for s in tl.segments)
    noise = torch.randn(1, 128, LA, generator=torch.Generator().manual_seed(5))
    want = _oracle(sd, cond, texts, unc, tl, noise, solver)
    got = _run(model, dac, cond, texts, unc, tl, noise, solver, use_graph)
    e = rel_err(got, want)
    print("timeline %s graph=%d: %.2e" % (solver, use_graph, e))
    assert got.shape == (1, 128, LA) and e < 1e-4, (solver, use_graph, e)


def test_one_span_timeline_is_the_plain_run_of_that_prompt(tiny):
    sd, _dsd, model, dac, cond, texts, unc = tiny
    noise = torch.randn(2, 128, LA, generator=torch.Generator().manual_seed(6))
    with torch.inference_mode():
        want = O.sample_latents(sd, C.TINY.heads, noise, texts[1:2], unc, cond["clip"], cond["sync"], STEPS, CFG, "euler")
    tl = _timeline([(0.0, 1.0, "b")], "b", 0.25)
    assert len(tl.segments) == 1
    timed = _run(model, dac, cond, texts, unc, tl, noise)
    plain = _run(model, dac, cond, texts, unc, None, noise, plain="b")
    e_t, e_p = rel_err(timed, want), rel_err(plain, want)
    print("one span: timeline %.2e plain %.2e" % (e_t, e_p))
    assert e_t < 1e-4 and e_p < 1e-4


def test_two_prompt_timeline_differs_from_either_prompt(tiny):
    """An implementation that ignored the table would reproduce one of the single-prompt runs."""
    _sd, _dsd, model, dac, cond, texts, unc = tiny
    noise = torch.randn(1, 128, LA, generator=torch.Generator().manual_seed(7))
    two = _run(model, dac, cond, texts, unc, _timeline([(0.0, 0.5, "a")], "b", 0.0), noise)
    for p in ("a", "b"):
        one = _run(model, dac, cond, texts, unc, None, noise, plain=p)
        e = rel_err(two, one)
        print("two prompts vs %s alone: %.2e" % (p, e))
        assert e > 1e-3, (p, e)


def test_graph_keyed_on_the_timeline_state(tiny):
    """One context, use_graph=True: plain, timeline A, timeline B of the same shape (graph kept, tables rewritten), plain, edit
    with a timeline, windowed with a timeline.  Every run equals its eager run."""
    _sd, _dsd, model, dac, cond, texts, unc = tiny
    g = torch.Generator().manual_seed(8)
    tA, tB = _timeline(*THREE), _timeline([(0.0, 0.6, "b"), (0.6, 0.8, "a")], "c", 0.1)
    assert tA.prompts != tB.prompts and len(tA.prompts) == len(tB.prompts)
    wplan = long_form.WindowPlan.from_frames(**PLAN)
    tW = _timeline([(0.0, 0.5, "a"), (0.9, 1.4, "b")], "c", 0.2, duration=wplan.Ltot / 50.0)
    n1, nw = torch.randn(1, 128, LA, generator=g), torch.randn(1, 128, wplan.Ltot, generator=g)
    ed = audio_edit.EditSpec(0.7 * torch.randn(1, 128, LA, generator=g), 1.0, audio_edit.build_mask(LA, [(0.2, 0.5)], 0.1))
    seq = [("plain", None, n1, None, None), ("A", tA, n1, None, None), ("B", tB, n1, None, None), ("plain", None, n1, None, None),
           ("edit", tA, n1, ed, None), ("win", tW, nw, None, wplan)]
    want = {}
    for name, tl, noise, edit, win in seq:
        if name not in want:
            want[name] = _run(model, dac, cond, texts, unc, tl, noise, plain="c", edit=edit, windows=win).clone()
    assert want["win"].shape == (1, 128, wplan.Ltot)
    for a, b in (("plain", "A"), ("A", "B"), ("A", "edit")):
        assert rel_err(want[a], want[b]) > 1e-3, (a, b)
    caps = {}
    for name, tl, noise, edit, win in seq:
        c0 = H.captures(model)
        got = _run(model, dac, cond, texts, unc, tl, noise, use_graph=True, plain="c", edit=edit, windows=win)
        caps[name] = H.captures(model) - c0
        assert rel_err(got, want[name]) < 1e-6, name
    assert caps["A"] >= 1 and caps["B"] == 0 and caps["plain"] >= 1, caps      # plain <-> timeline re-captures, A -> B keeps the graph


def test_graph_keyed_across_different_options(tiny, dev):
    """One context, use_graph=True, two clips of 1 s, 10 euler steps: plain -> two windows under multistep order 2 -> an edit with
    a mask under a guidance schedule with rescale -> a step-cache skip list under three halves -> a timeline -> plain.  Every
    transition swaps one set of options for another (the keying tests of the features toggle one each).  Each run captures exactly
    once and carries the bits of the same call with use_graph=False on a context of its own: graph and eager issue the same
    launches with the same arguments.  The last plain run carries the bits of the first."""
    sd, _dsd, model, dac, cond, texts, unc = tiny
    g = torch.Generator().manual_seed(12)
    wplan = long_form.WindowPlan.from_frames([0, 30], LA)
    n2, nw = torch.randn(2, 128, LA, generator=g), torch.randn(1, 128, wplan.Ltot, generator=g)
    ed = audio_edit.EditSpec(0.7 * torch.randn(2, 128, LA, generator=g), 1.0, audio_edit.build_mask(LA, [(0.2, 0.5)], 0.1))
    Guid = sampler.GuidanceSpec
    seq = [("plain", {}),
           ("windows, order 2", dict(noise=nw, windows=wplan, multistep=sampler.MultistepSpec(2))),
           ("edit, schedule, rescale", dict(edit=ed, guidance=Guid(interval=(0.2, 0.7), rescale=0.7))),
           ("skip list, three halves", dict(scale=2.0, guidance=Guid(g_video=7.0), step_cache=sampler.StepCacheSpec(skip=(3, 6)))),
           ("timeline", dict(tl=_timeline(*THREE))),
           ("plain", {})]

    def call(m, use_graph, tl=None, scale=CFG, noise=n2, **kw):
        return H.run(m, dac, [_cond(cond, texts, unc, tl, "c")], noise, "euler", STEPS, scale, use_graph, timeline=tl, **kw)[2].clone()

    want = {}
    for name, kw in seq[:-1]:
        want[name] = call(sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY), False, **kw)
    assert want["windows, order 2"].shape == (1, 128, wplan.Ltot)
    names = list(want)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert want[a].shape != want[b].shape or rel_err(want[a], want[b]) > 1e-3, (a, b)
    one = sampler.FoleyModel(C.TINY, sd, torch.float32, dev, dac_cfg=C.DAC_TINY)
    got = []
    for name, kw in seq:
        c0 = H.captures(one)
        got.append(call(one, True, **kw))
        e = rel_err(got[-1], want[name])
        print("%s: graph vs eager %.2e, captures +%d" % (name, e, H.captures(one) - c0))
        assert H.captures(one) == c0 + 1, name
        assert torch.equal(got[-1], want[name]), (name, e)
    assert torch.equal(got[-1], got[0])


def test_prepare_timeline_refusals(tiny):
    _sd, _dsd, model, dac, cond, texts, unc = tiny
    tl = _timeline(*THREE)
    vis, txt = H.batched([_cond(cond, texts, unc, tl)])
    n = 2 *(cond["clip"].shape[1] + LA)

    def plan(**edits):
        p = dict(sampler.build_plan(model, vis, txt, LA, CFG, STEPS, 1, "euler", timeline=tl))
        sa, sb, al = (list(x) for x in p["timeline"])
        for k, (i, v) in edits.items():
            {"a": sa, "b": sb, "alpha": al}[k][i] = v
        p["timeline"] = (sa, sb, al)
        return p

    model.ctx.prepare(plan())
    for edits, word in ((dict(a=(3, 4)), "set index"), (dict(b=(n - 1, -1)), "set index"), (dict(alpha=(5, 1.0)), "alpha"),
                        (dict(alpha=(5, -0.25)), "alpha"), (dict(alpha=(5, float("nan"))), "alpha")):
        with pytest.raises(rt.FoleyRuntimeError, match=word):
            model.ctx.prepare(plan(**edits))
    p = plan()
    p["text"] = torch.zeros(17, p["Lt"], p["text"].shape[2], device=model.device)
    with pytest.raises(rt.FoleyRuntimeError, match=r"\[1, 16\]"):
        model.ctx.prepare(p)
    p = plan()
    p["timeline"] = tuple(x[:-1] for x in p["timeline"])
    with pytest.raises(rt.FoleyRuntimeError, match="entries"):
        model.ctx.prepare(p)
    # NULL tables and n_text = 0, straight at the C entry
    lib, pc = rt.load_library(), rt.FoleyPlanC()
    pc.ncfg, pc.clips, pc.La, pc.Lv, pc.Ls, pc.Lt, pc.n_iter = 2, 1, LA, 8, 16, 77, STEPS
    arr = (ctypes.c_int32 * n)()
    al = (ctypes.c_float * n)()
    for t, word in ((rt.TextTimelineC(4, None, arr, al), b"null table"), (rt.TextTimelineC(4, arr, arr, None), b"null table"),
                    (rt.TextTimelineC(0, arr, arr, al), b"[1, 16]")):
        assert lib.foley_prepare_timeline(model.ctx._h, ctypes.byref(pc), ctypes.byref(t), None) != 0
        assert word in lib.foley_last_error()
    assert lib.foley_prepare_timeline(model.ctx._h, ctypes.byref(pc), None, None) != 0
    # the context still serves a plain run afterwards
    noise = torch.randn(1, 128, LA, generator=torch.Generator().manual_seed(9))
    assert torch.isfinite(_run(model, dac, cond, texts, unc, None, noise, plain="a")).all()


def test_bf16_timeline_runs_end_to_end(tiny, dev):
    """A bf16 TINY run through the 16-bit timeline kernel; its distance from the fp32 run is printed, not gated."""
    sd, dsd, model, dac, cond, texts, unc = tiny
    m16 = sampler.FoleyModel(C.TINY, sd, torch.bfloat16, dev, dac_cfg=C.DAC_TINY)
    tl = _timeline(*THREE)
    noise = torch.randn(1, 128, LA, generator=torch.Generator().manual_seed(5))
    got = _run(model, dac, cond, texts, unc, tl, noise, dtype_model=m16)
    got_g = _run(model, dac, cond, texts, unc, tl, noise, use_graph=True, dtype_model=m16)
    ref = _run(model, dac, cond, texts, unc, tl, noise)
    print("bf16 timeline vs fp32: %.3e" % rel_err(got, ref))
    assert got.shape == (1, 128, LA) and bool(torch.isfinite(got).all()) and rel_err(got_g, got) < 1e-6
