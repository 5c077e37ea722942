"""The guidance combine of the three solver step kernels and the CFG-rescale statistics (rowops.hip) under per-element bounds
and guard bands (tests/opcheck.py, tests/guidance_ref.py).

The step forms run with a guidance descriptor - a schedule table whose row changes every iteration and, on every second
iteration, per-clip factors - for two and three halves, into guarded buffers; every element is held against the bound of the step
with the combine's extra roundings, the staged rows bit for bit against the device's own x in all ncfg copies.  With two halves, a
constant table and no factors the three forms must give the bits of the calls without a descriptor; under a varying table with
factors, for one to three halves, the edit form with nothing to keep and the windows form with one window must give the bits of
the plain form.  The factors are held
against fp64 under the any-order fp32 bound of the two centred sums; because that bound cannot see one lost element in smooth
data, a second family of inputs carries its variance in a handful of edge elements, each worth at least ten bounds."""
import pytest
import torch

import guidance_ref as G
import opcheck as oc
from conftest import record_parity
from foley_amd.host import long_form, runtime as rt, tables
from step_harness import ALL3, DTS, GUIDANCE, SOLVER_ITERS, STEP_SHAPES, StepState, _rand

pytestmark = pytest.mark.gpu

_WORST = {}


def _rec(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), float(ratio))
    record_parity(f"elementwise.guidance.{family}", err_over_bound=_WORST[family])


def _sched(n):
    """[n, 2] fp32, another (g_video, g_text) on every iteration."""
    return torch.tensor([[1.5 + 0.75 * i, 4.0 - 0.5 * i] for i in range(n)], dtype=torch.float32)


def _factors(clips, seed):
    return 0.5 + torch.rand(clips, generator=torch.Generator().manual_seed(seed))


def _guided_ref(pred, st, coef_row, sched_row, ncfg, scale):
    x, xs, da, _ = st.snapshot()
    clips, _, L = x.shape
    v, e_v = oc.combine_ref(pred, clips, L, ncfg, float(sched_row[0].double()), float(sched_row[1].double()), scale)
    return oc.step_ref_and_bounds(v, e_v, x, xs, da, coef_row)


class _Desc:
    """The schedule and the factors in guarded device buffers; desc(with_scale) builds the descriptor of one launch."""

    def __init__(self, dev, sched, clips, seed):
        self.gs = oc.guarded(tuple(sched.shape), torch.float32, dev, rows=(1, 1))
        self.gs.view.copy_(sched.to(dev))
        self.scale = _factors(clips, seed)
        self.gf = oc.guarded((clips, 1), torch.float32, dev, rows=(1, 1))
        self.gf.view.copy_(self.scale.view(-1, 1).to(dev))

    def desc(self, with_scale):
        return rt.guidance_desc(self.gs.view, self.gf.view.view(-1) if with_scale else None)

    def check(self, sched, what):
        oc.assert_bits_equal(self.gs.view, sched, what + " schedule untouched")
        oc.assert_bits_equal(self.gf.view, self.scale.view(-1, 1), what + " factors untouched")
        self.gs.check(what)
        self.gf.check(what)


# ----------------------------------------------------------------------------- the three step forms with a descriptor
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_guided_step_elementwise(dev, clips, C, L, solver, ncfg, dt):
    n = SOLVER_ITERS[solver]
    coef, sched = tables.solver_table(tables.sigma_grid(n), solver, n), _sched(n)
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 200)
    d = _Desc(dev, sched, clips, 201)
    cd = coef.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 202 + it)
        with_scale = it % 2 == 1
        r = _guided_ref(pred, st, coef[it], sched[it], ncfg, d.scale if with_scale else None)
        st.step(pred, cd, gd=d.desc(with_scale))
        what = f"guided step {solver} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it}"
        worst = max(worst, st.check(it, r, *r["x"], what))
        d.check(sched, what)
    _rec(f"solver_step.{solver}", worst)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_guided_step_edit_elementwise(dev, clips, C, L, solver, ncfg, dt):
    """Per-clip source latents and a fractional per-clip mask with exact 0 and 1 entries (the edit form's own variants are
    test_rowops_elementwise_gpu.py's)."""
    n = SOLVER_ITERS[solver]
    coef, sched = tables.edit_solver_table(tables.sigma_grid(n), solver, n), _sched(n)
    x0, noise = _rand((clips, C, L), 210, 0.7), _rand((clips, C, L), 211)
    mask = torch.rand(clips, L, generator=torch.Generator().manual_seed(212))
    mask[:, : L // 3] = 0.0
    mask[:, L // 3: L // 2] = 1.0
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 213)
    d = _Desc(dev, sched, clips, 214)
    cd, edit = coef.to(dev), (x0.to(dev), noise.to(dev), mask.to(dev))
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 215 + it)
        with_scale = it % 2 == 1
        r = _guided_ref(pred, st, coef[it], sched[it], ncfg, d.scale if with_scale else None)
        ref, bound = r["x"]
        if r["flags"] & oc.STEP_BLEND:
            ref, bound = oc.edit_blend_ref_and_bound(ref, bound.e, r["s_next"], x0, noise, mask)
        st.step(pred, cd, gd=d.desc(with_scale), edit=edit)
        what = f"guided step_edit {solver} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it}"
        worst = max(worst, st.check(it, r, ref, bound, what))
        d.check(sched, what)
    _rec(f"solver_step_edit.{solver}", worst)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("_clips,C,L", STEP_SHAPES)
def test_guided_step_windows_elementwise(dev, _clips, C, L, solver, ncfg, dt):
    """Two variations of three windows (a frame in all three where L >= 3, disjoint windows otherwise): every window is a clip
    with its own factor, applied before the blend."""
    n = SOLVER_ITERS[solver]
    coef, sched = tables.edit_solver_table(tables.sigma_grid(n), solver, n), _sched(n)
    starts = [0, L // 3, 2 * L // 3] if L >= 3 else [0, L, 2 * L]
    plan = long_form.WindowPlan.from_frames(starts, L)
    n_win, clips = plan.n_win, 2 * plan.n_win
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 220)
    d = _Desc(dev, sched, clips, 221)
    cd, sd, wd = coef.to(dev), torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 222 + it)
        with_scale = it % 2 == 1
        r = _guided_ref(pred, st, coef[it], sched[it], ncfg, d.scale if with_scale else None)
        ref, bound = r["x"]
        if r["flags"] & oc.STEP_BLEND:
            ref, e, _, _, _ = oc.windows_mean_ref_and_bound(ref, bound.e, n_win, starts, plan.weights)
            bound = oc.Bound(e)
        st.step(pred, cd, gd=d.desc(with_scale), windows=(sd, wd, plan.Ltot))
        what = f"guided step_windows {solver} C{C} L{L} starts {starts} ncfg {ncfg} {dt} it {it}"
        worst = max(worst, st.check(it, r, ref, bound, what))
        d.check(sched, what)
    _rec(f"solver_step_windows.{solver}", worst)


# ----------------------------------------------------------------------------- two halves, constant table, no factors: the old bits
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("form", ["plain", "edit", "windows"])
@pytest.mark.parametrize("clips,C,L", [(2, 128, 50), (2, 40, 65)])
def test_constant_schedule_keeps_the_bits(dev, clips, C, L, form, dt):
    solver, ncfg = "heun-2", 2
    n = SOLVER_ITERS[solver]
    coef = (tables.solver_table if form == "plain" else tables.edit_solver_table)(tables.sigma_grid(n), solver, n).to(dev)
    sched = torch.full((n, 2), GUIDANCE, dtype=torch.float32, device=dev)
    sched[:, 1] = -3.0                       # two halves read column 0 only
    starts = [0, L // 3]
    plan = long_form.WindowPlan.from_frames(starts, L)
    kw = {}
    if form == "edit":
        x0, noise, mask = _rand((1, C, L), 230, 0.7).to(dev), _rand((clips, C, L), 231).to(dev), torch.rand(L, generator=torch.Generator().manual_seed(232)).to(dev)
        kw = {"edit": (x0, noise, mask)}
    elif form == "windows":
        sd, wd = torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
        kw = {"windows": (sd, wd, plan.Ltot)}
    a, b = StepState(dev, clips, C, L, ncfg, DTS[dt], 233), StepState(dev, clips, C, L, ncfg, DTS[dt], 233)
    gd = rt.guidance_desc(sched, None)
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 234 + it).to(dev)
        a.step(pred, coef, **kw)                    # no guidance option at all
        b.step(pred, coef, gd=gd, **kw)
        for ga, gb, name in zip((a.gx, a.gs, a.ga, a.gr, a.ctr), (b.gx, b.gs, b.ga, b.gr, b.ctr), ("x", "x_saved", "d_acc", "rows_out", "counter")):
            oc.assert_bits_equal(gb.view, ga.view, f"{form} {dt} it {it} {name}: descriptor with a constant table vs none")
            gb.check(f"{form} {name}")
    # an explicit gd=None is the call without the option as well
    c = StepState(dev, clips, C, L, ncfg, DTS[dt], 233)
    for it in range(n):
        c.step(_rand((ncfg * clips * L, C), 234 + it).to(dev), coef, gd=None, **kw)
    oc.assert_bits_equal(c.gx.view, a.gx.view, f"{form} {dt}: null descriptor")


# ----------------------------------------------------------------------------- the forms agree with each other under any descriptor
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [1, 2, 3])
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("clips,C,L", [(2, 40, 65), (1, 128, 1)])
def test_forms_agree_under_a_descriptor(dev, clips, C, L, solver, ncfg, dt):
    """With a schedule that changes every iteration and per-clip factors, the edit entry without a mask and with an all-ones mask
    (one source clip), and the windows entry with the single window [0, L) of weight 1.0f, give the bits of the plain guided
    entry in x, x_saved, d_acc, the staged rows and the counter: a partial tile in both axes, and the one-frame clip.  All four
    read the table with the STEP_BLEND rows, which the plain form ignores."""
    n = SOLVER_ITERS[solver]
    coef, sched = tables.edit_solver_table(tables.sigma_grid(n), solver, n).to(dev), _sched(n)
    x0, noise = _rand((1, C, L), 240, 0.7).to(dev), _rand((clips, C, L), 241).to(dev)
    ones = torch.ones(L, dtype=torch.float32, device=dev)
    sd, wd = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, L, dtype=torch.float32, device=dev)
    forms = {"plain": {}, "edit, no mask": {"edit": (x0, noise, None)}, "edit, mask of ones": {"edit": (x0, noise, ones)},
             "one window": {"windows": (sd, wd, L)}}
    states = {f: StepState(dev, clips, C, L, ncfg, DTS[dt], 242) for f in forms}
    d = _Desc(dev, sched, clips, 243)
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 244 + it).to(dev)
        for f, kw in forms.items():
            states[f].step(pred, coef, gd=d.desc(it % 2 == 0), **kw)
        a = states["plain"]
        assert int(a.ctr.view.item()) == it + 1
        for f in list(forms)[1:]:
            b = states[f]
            for ga, gb, name in zip((a.gx, a.gs, a.ga, a.gr, a.ctr), (b.gx, b.gs, b.ga, b.gr, b.ctr), ("x", "x_saved", "d_acc", "rows_out", "counter")):
                oc.assert_bits_equal(gb.view, ga.view, f"{f} vs plain: {solver} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it} {name}")
                gb.check(f"{f} {name}")
        for g in (a.gx, a.gs, a.ga, a.gr, a.ctr):
            g.check("plain")
        d.check(sched, "forms")


# ----------------------------------------------------------------------------- the rescale factors
FACTOR_SHAPES = STEP_SHAPES + [(1, 128, 2100)]       # 66 workgroups per clip: the finishing wave's lanes hold two records each
PHI = 0.7


def _stats(dev, pred, clips, L, ncfg, sched, it, phi=PHI):
    """The device's factors [clips] (CPU) from guarded buffers."""
    g = oc.guarded((clips, 1), torch.float32, dev, rows=(1, 1))
    ctr = torch.tensor([it], dtype=torch.int32, device=dev)
    sd = sched.to(dev) if sched is not None else None
    rt.op_guidance_stats(pred.to(dev), clips, L, ncfg, GUIDANCE, sd, ctr, phi, out=g.view.view(-1))
    g.check("guidance_stats factors")
    assert int(ctr.item()) == it                                 # the statistics only read the counter
    return g.view.cpu().view(-1).clone()


@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("clips,C,L", FACTOR_SHAPES)
def test_factors_against_fp64(dev, clips, C, L, ncfg):
    sched = _sched(3)
    halves = [_rand((clips * L, C), 240 + h, 1.0 + 0.5 * h) + 0.3 * h for h in range(ncfg)]     # halves of different spread and mean
    pred = torch.cat(halves)
    for it, sc in ((2, sched), (0, None)):                       # a table row, and the scalar
        gv, gt = (float(sched[it, 0].double()), float(sched[it, 1].double())) if sc is not None else (oc.f32(GUIDANCE),) * 2
        f, bound = G.factor_ref(pred, clips, L, ncfg, gv, gt, PHI)
        got = _stats(dev, pred, clips, L, ncfg, sc, it)
        print(f"{clips}x{C}x{L} ncfg {ncfg}: f {f.tolist()} got {got.tolist()} bound {bound.tolist()}")
        _rec("factor", oc.assert_elementwise(got, f, bound, f"factors {clips}x{C}x{L} ncfg {ncfg} it {it}"))
        assert float((f - 1.0).abs().min()) > 0.1                                # the factors are not trivially 1


def _edge_elements(C, L):
    """(channel, frame) pairs on the edges a reduction can lose: the corners of the clip, the ends of a lane group (channels 63 /
    64), of a wave's rows (frames 7 / 8) and of a workgroup's (frames 31 / 32 / 33), the last frame and the last channel."""
    cand = [(0, 0), (C - 1, L - 1), (63, 31), (64, 32), (C - 1, 33), (0, L - 1), (C - 1, 0), (1, 7), (C - 2, 8)]
    out = []
    for c, l in cand:
        e = (min(c, C - 1), min(l, L - 1))
        if e not in out:
            out.append(e)
    return out


@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_factors_see_every_edge_element(dev, clips, C, L, ncfg):
    """Smooth data of spread 1e-3 plus, in every clip, spikes on the edge elements: 4 in the last half (the guided value then
    carries g times that) and, on every second one, -3 in the first half as well, so that the spikes differ in how much they add
    to the two sums.  Leaving any one of them out of the statistics moves the fp64 factor by at least ten bounds - so a kernel
    within the bound has read them all."""
    edges = _edge_elements(C, L)
    assert len(edges) >= 2
    pred = (1e-3 * _rand((ncfg * clips * L, C), 250)).view(ncfg, clips, L, C)
    for k, (c, l) in enumerate(edges):
        pred[ncfg - 1, :, l, c] = 4.0
        if ncfg == 3:
            pred[1, :, l, c] = 4.0                               # h1 and h2 agree there: the text term adds nothing
        if k % 2:
            pred[0, :, l, c] = -3.0
    pred = pred.reshape(ncfg * clips * L, C).contiguous()
    sched = torch.tensor([[2.5, 2.0]], dtype=torch.float32)
    f, bound = G.factor_ref(pred, clips, L, ncfg, 2.5, 2.0, PHI)
    for c, l in edges:
        keep = torch.ones(clips, C, L, dtype=torch.bool)
        keep[:, c, l] = False
        f_lost, _ = G.factor_ref(pred, clips, L, ncfg, 2.5, 2.0, PHI, keep=keep)
        moved = (f_lost - f).abs() / bound
        assert float(moved.min()) >= 10.0, (f"losing (channel {c}, frame {l}) moves the factor by {moved.tolist()} bounds", f.tolist())
    got = _stats(dev, pred, clips, L, ncfg, sched, 0)
    _rec("factor_edges", oc.assert_elementwise(got, f, bound, f"edge-carried factors {clips}x{C}x{L} ncfg {ncfg}"))


@pytest.mark.parametrize("ncfg", [2, 3])
def test_constant_pred_gives_exactly_one(dev, ncfg):
    for clips, C, L in STEP_SHAPES:
        pred = torch.full((ncfg * clips * L, C), 0.3)
        got = _stats(dev, pred, clips, L, ncfg, _sched(1), 0)
        oc.assert_bits_equal(got, torch.ones(clips), f"constant pred {clips}x{C}x{L} ncfg {ncfg}")
        halves = torch.cat([torch.full((clips * L, C), k) for k in (0.3, -1.25, 2.0)[:ncfg]])      # a constant per half: v is constant too
        oc.assert_bits_equal(_stats(dev, halves, clips, L, ncfg, _sched(1), 0), torch.ones(clips), f"constant halves {clips}x{C}x{L} ncfg {ncfg}")
    zero = _stats(dev, torch.zeros(ncfg * 2 * 50, 128), 2, 50, ncfg, None, 0)
    oc.assert_bits_equal(zero, torch.ones(2), "zero pred")


@pytest.mark.parametrize("clips,C,L", [(3, 128, 33), (1, 128, 2100)])
def test_factors_repeat_bit_for_bit(dev, clips, C, L):
    pred = _rand((3 * clips * L, C), 260)
    a = _stats(dev, pred, clips, L, 3, _sched(2), 1)
    b = _stats(dev, pred, clips, L, 3, _sched(2), 1)
    oc.assert_bits_equal(a, b, "two calls")
    assert bool((a != 1.0).all())


def test_phi_zero_and_one(dev):
    """phi 0 gives 1 whatever the data; phi 1 the bare ratio of the deviations."""
    clips, C, L = 2, 96, 31
    pred = torch.cat([_rand((clips * L, C), 270), 2.0 * _rand((clips * L, C), 271)])
    oc.assert_bits_equal(_stats(dev, pred, clips, L, 2, None, 0, phi=0.0), torch.ones(clips), "phi 0")
    f, bound = G.factor_ref(pred, clips, L, 2, oc.f32(GUIDANCE), oc.f32(GUIDANCE), 1.0)
    oc.assert_elementwise(_stats(dev, pred, clips, L, 2, None, 0, phi=1.0), f, bound, "phi 1")


def test_stats_refusals(dev):
    pred = torch.zeros(2 * 50, 128, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = rt.load_library()
    out, work = torch.zeros(1, device=dev), torch.zeros(4, device=dev)
    gd = rt.guidance_desc(None, out)
    import ctypes
    assert lib.foley_op_guidance_stats(ctypes.byref(gd), rt._ptr(pred), 1, 128, 50, 2, 4.5, rt._ptr(ctr), 0.5, rt._ptr(work), 4, rt._stream()) != 0
    assert b"work buffer" in lib.foley_last_error()
    wide = torch.zeros(2 * 4, 300, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="256 channels"):
        rt.op_guidance_stats(wide, 1, 4, 2, 4.5, None, ctr, 0.5)
