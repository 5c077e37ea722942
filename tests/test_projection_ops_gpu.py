"""Projected guidance at op level (rowops.hip: guidance_proj_stats_kernel, guidance_proj_coef_kernel and the projected
instantiations of the step forms) under per-clip and per-element bounds and guard bands (tests/opcheck.py, tests/projection_ref.py).

The coefficients and APG's plane are held against fp64 under the bound the kernels' documented summation chain gives (chain length
x 2^-24 x the sum of |products|, propagated to a_c and a_w to first order), at every shape at which launch 1 masks rows or
channels and once past launch 2's 64 lanes.  Because that bound cannot see one lost element in smooth data, a second family of
inputs carries its weight on edge elements, each worth at least four bounds.  The consequences that hold as bits are tested as
bits; the step's value is held against opcheck.step_ref_and_bounds fed the projected v and its bound."""
import pytest
import torch

import opcheck as oc
import projection_ref as P
from conftest import record_parity
from foley_amd.host import runtime as rt, tables
from step_harness import ALL3, DTS, GUIDANCE, StepState, _rand

pytestmark = pytest.mark.gpu

_WORST = {}
MODES = {"apg": P.APG, "zero_star": P.ZERO_STAR}


def _rec(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), float(ratio))
    record_parity(f"elementwise.projection.{family}", err_over_bound=_WORST[family])


class _Proj:
    """The rows, the coefficients and the plane of one run in guarded device buffers (the plane starts as NaN: a row with
    beta = 0 must not read it)."""

    def __init__(self, dev, mode, rows, clips, La, C):
        self.dev, self.mode, self.clips, self.La = dev, mode, clips, La
        self.rows = rows.clone()
        self.gr = oc.guarded(tuple(rows.shape), torch.float32, dev, rows=(1, 1))
        self.gr.view.copy_(rows.to(dev))
        self.gc = oc.guarded((clips, 2), torch.float32, dev, rows=(1, 1))
        self.gp = oc.guarded((clips * La, C), torch.float32, dev, rows=(2, 3)) if mode == P.APG else None

    def set_row(self, it, col, value):
        self.rows[it, col] = value
        self.gr.view.copy_(self.rows.to(self.dev))

    @property
    def desc(self):
        return rt.projection_desc(self.mode, self.gr.view, self.gc.view, self.gp.view if self.gp is not None else None)

    def plane(self):
        return self.gp.view.cpu().clone().view(self.clips, self.La, -1) if self.gp is not None else None

    def project(self, pred, it, guidance=GUIDANCE, sched=None):
        """The two launches at iteration `it` (the counter is only read); returns the coefficients [clips, 2] on the CPU."""
        ctr = torch.tensor([it], dtype=torch.int32, device=self.dev)
        rt.op_guidance_project(self.desc, pred.to(self.dev), self.clips, self.La, guidance, sched.to(self.dev) if sched is not None else None, ctr)
        assert int(ctr.item()) == it
        self.check("guidance_project")
        return self.gc.view.cpu().clone()

    def check(self, what):
        oc.assert_bits_equal(self.gr.view, self.rows, what + " rows untouched")
        for g in (self.gr, self.gc, self.gp):
            if g is not None:
                g.check(what)


def _sched(n):
    return torch.tensor([[1.5 + 0.75 * i, -7.0] for i in range(n)], dtype=torch.float32)      # two halves read column 0


def _halves(clips, La, C, seed):
    """[2 clips La, C]: halves of different spread and mean, correlated (c = 0.6 u + noise) and not parallel."""
    u = _rand((clips * La, C), seed, 0.8) + 0.2
    return torch.cat([u, 0.6 * u + _rand((clips * La, C), seed + 1, 0.7) - 0.1])


# ----------------------------------------------------------------------------- coefficients and plane against fp64
SHAPES = [(clips, C, La) for clips in (1, 3) for C in (64, 100, 128, 256) for La in (1, 31, 32, 33, 50)]
LONG = (1, 128, 2081)      # 66 workgroups per clip: two lanes of launch 2 hold two records each, the last workgroup one row


def _check_coef(p, pred, it, g, sched, what, m_prev=None):
    ref = P.coef_ref(pred, p.clips, p.La, g, p.rows[it].tolist(), p.mode, m_prev=m_prev)
    got = p.project(pred, it, guidance=g if sched is None else -99.0, sched=sched)
    print(f"{what}: coef {ref['coef'].tolist()} got {got.tolist()} bound {ref['bound'].tolist()}")
    worst = oc.assert_elementwise(got, ref["coef"], ref["bound"], what + " coefficients")
    if p.mode == P.APG:
        worst = max(worst, oc.assert_elementwise(p.plane(), ref["m"], ref["e_m"], what + " plane"))
    return ref, worst


def _apg_run(dev, clips, C, La, clip_case):
    """Three consecutive iterations, beta 0 then -0.5 twice, from a plane of NaN; R at half the smallest (every clip is clipped) or
    twice the largest (none is) fp64 |m| of the iteration; the scale from a table on the first case, the scalar on the second."""
    rows = tables.projection_rows(3, "apg", 0.25, -0.5, 0.0, 0)
    p = _Proj(dev, P.APG, rows, clips, La, C)
    sched = _sched(3) if clip_case == "half" else None
    worst = 0.0
    for it in range(3):
        pred = _halves(clips, La, C, 400 + 2 * it)
        g = float(sched[it, 0].double()) if sched is not None else oc.f32(GUIDANCE)
        prev = p.plane() if it else None
        norm = P.coef_ref(pred, clips, La, g, p.rows[it].tolist(), P.APG, m_prev=prev)["norm"]
        p.set_row(it, 2, 0.5 * float(norm.min()) if clip_case == "half" else 2.0 * float(norm.max()))
        ref, w = _check_coef(p, pred, it, g, sched, f"apg {clips}x{C}x{La} R {clip_case} it {it}", m_prev=prev)
        assert bool((ref["r"] < 0.6).all()) if clip_case == "half" else bool((ref["r"] == 1.0).all())
        assert float((ref["coef"][:, 0] - 1.0).abs().min()) > 0.02                          # not the trivial coefficient
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("clip_case", ["half", "twice"])
@pytest.mark.parametrize("clips,C,La", SHAPES)
def test_apg_coefficients_and_plane_against_fp64(dev, clips, C, La, clip_case):
    _rec("apg_coef", _apg_run(dev, clips, C, La, clip_case))


@pytest.mark.parametrize("clips,C,La", SHAPES + [LONG])
def test_zero_star_coefficients_against_fp64(dev, clips, C, La):
    rows = tables.projection_rows(3, "cfg_zero_star", zero_init=1)
    p = _Proj(dev, P.ZERO_STAR, rows, clips, La, C)
    sched = _sched(3)
    for it, sc in ((2, sched), (1, None), (0, sched)):           # a table row, the scalar, and a dead row
        pred = _halves(clips, La, C, 420 + it)
        g = float(sched[it, 0].double()) if sc is not None else oc.f32(GUIDANCE)
        ref, w = _check_coef(p, pred, it, g, sc, f"zero* {clips}x{C}x{La} it {it}")
        if it == 0:
            assert bool((p.gc.view == 0).all()), "zero* dead row: zero coefficients"
        else:
            assert float(ref["coef"][:, 1].abs().min()) > 1e-3
        _rec("zero_star_coef", w)


def test_apg_past_the_finishing_wave(dev):
    _rec("apg_coef", _apg_run(dev, *LONG, "half"))


# ----------------------------------------------------------------------------- the edge condition
def _edge_elements(C, La):
    """(channel, frame) pairs on the edges a reduction can lose: the corners of the clip - the last row and the last channel among
    them -, the ends of a lane group (channels 63 / 64), of a wave's rows (frames 7 / 8) and of a workgroup's (frames 31 / 32 / 33)."""
    cand = [(0, 0), (C - 1, La - 1), (63, 31), (64, 32), (C - 1, 33), (0, La - 1), (C - 1, 0), (1, 7), (C - 2, 8)]
    out = []
    for c, l in cand:
        e = (min(c, C - 1), min(l, La - 1))
        if e not in out:
            out.append(e)
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clips,C,La", [(2, 128, 50), (3, 100, 33), (2, 256, 34), (1, 64, 65), (2, 96, 31)])
def test_coefficients_see_every_edge_element(dev, clips, C, La, mode):
    """Smooth data of spread 1e-3 plus, in every clip, spikes on the edge elements - c = 4 with u = -3 or 2 in turn, so the spikes
    differ in what they add to each sum.  Leaving any one of them out moves an fp64 coefficient by at least 4 bounds (verified here
    on the CPU) - so a kernel within the bound has read them all.  APG runs with a clipping R, so both its coefficients depend on
    the data."""
    md = MODES[mode]
    edges = _edge_elements(C, La)
    assert len(edges) >= 2 and (C - 1, La - 1) in edges
    pred = (1e-3 * _rand((2 * clips * La, C), 430)).view(2, clips, La, C)
    for k, (c, l) in enumerate(edges):
        pred[1, :, l, c] = 4.0
        pred[0, :, l, c] = -3.0 if k % 2 else 2.0
    pred = pred.reshape(2 * clips * La, C).contiguous()
    g = 2.5
    rows = tables.projection_rows(1, md, 0.0, 0.0, 0.0, 0)
    if md == P.APG:
        rows[0, 2] = 0.5 * float(P.coef_ref(pred, clips, La, g, rows[0].tolist(), md)["norm"].min())
    ref = P.coef_ref(pred, clips, La, g, rows[0].tolist(), md)
    for c, l in edges:
        keep = torch.ones(clips, La, C, dtype=torch.bool)
        keep[:, l, c] = False
        lost = P.coef_ref(pred, clips, La, g, rows[0].tolist(), md, keep=keep)
        moved = ((lost["coef"] - ref["coef"]).abs() / ref["bound"].clamp_min(1e-300)).amax(1)
        assert float(moved.min()) >= 4.0, (f"losing (channel {c}, frame {l}) moves the coefficients by {moved.tolist()} bounds", ref["coef"].tolist())
    p = _Proj(dev, md, rows, clips, La, C)
    got = p.project(pred, 0, guidance=g)
    _rec("coef_edges", oc.assert_elementwise(got, ref["coef"], ref["bound"], f"edge-carried coefficients {mode} {clips}x{C}x{La}"))


# ----------------------------------------------------------------------------- what holds as bits
def _euler(n, dev, hist=False):
    sig = tables.sigma_grid(n)
    t = tables.solver_table(sig, "euler", n, multistep_order=2) if hist else tables.solver_table(sig, "euler", n)
    return t, t.to(dev)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clips,C,La", [(2, 128, 50), (3, 100, 33)])
def test_scale_one_gives_the_conditional_prediction_bit_for_bit(dev, clips, C, La, mode):
    """g == 1 (an iteration outside a guidance interval): a_c = 1 and a_w = 0 exactly and v == c, read from the ring slot the
    history step stores v to; APG's second iteration has momentum and a clipping R."""
    md = MODES[mode]
    rows = tables.projection_rows(2, md, 0.25, -0.5, 0.5, 0)
    p = _Proj(dev, md, rows, clips, La, C)
    _, cd = _euler(2, dev, hist=True)
    st = StepState(dev, clips, C, La, 2, torch.float32, 440, saved=False, slots=1)
    for it in range(2):
        pred = _halves(clips, La, C, 441 + it)
        coef = p.project(pred, it, guidance=1.0)
        oc.assert_bits_equal(coef, torch.tensor([[1.0, 0.0]] * clips), f"{mode} g = 1 it {it}: coefficients")
        st.step(pred, cd, guidance=1.0, proj=p.desc)
        c = pred.view(2, clips, La, C)[1].transpose(1, 2).contiguous()
        oc.assert_bits_equal(st.gh.view[0], c, f"{mode} g = 1 it {it}: v == c")
        p.check("g = 1")


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("mode", list(MODES))
def test_dead_row_leaves_x_and_the_staged_rows(dev, mode, dt):
    """live == 0: both coefficients are zeros (live times a finite number: the sign is the product's), v is a zero, and an euler
    row leaves x - and so the rows staged from it - as they were, bit for bit."""
    clips, C, La, md = 2, 100, 33, MODES[mode]
    rows = tables.projection_rows(2, md, 0.25, -0.5, 0.0, 1)
    p = _Proj(dev, md, rows, clips, La, C)
    _, cd = _euler(2, dev, hist=True)
    st = StepState(dev, clips, C, La, 2, DTS[dt], 450, saved=False, slots=1)
    x0 = st.gx.view.cpu().clone()
    pred = _halves(clips, La, C, 451)
    assert bool((p.project(pred, 0) == 0).all()), f"{mode} dead row: zero coefficients"
    st.step(pred, cd, proj=p.desc)
    oc.assert_bits_equal(st.gx.view, x0, f"{mode} {dt} dead row: x")
    oc.assert_bits_equal(st.gr.view, oc.rows_of(x0, 2, DTS[dt]), f"{mode} {dt} dead row: staged rows")
    assert bool((st.gh.view[0] == 0).all()) and int(st.ctr.view.item()) == 1
    for g in (st.gx, st.gr, st.gh, st.ctr):
        g.check("dead row")
    # the row after it is live: x moves
    pred = _halves(clips, La, C, 452)
    p.project(pred, 1)
    st.step(pred, cd, proj=p.desc)
    assert not torch.equal(st.gx.view.cpu(), x0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clips,C,La", [(3, 128, 33), LONG])
def test_projection_repeats_bit_for_bit(dev, clips, C, La, mode):
    md = MODES[mode]
    rows = tables.projection_rows(2, md, 0.25, -0.5, 1.0, 0)
    out = []
    for _ in range(2):
        p = _Proj(dev, md, rows, clips, La, C)
        coefs = [p.project(_halves(clips, La, C, 460 + it), it) for it in range(2)]
        out.append((torch.stack(coefs), p.plane()))
    oc.assert_bits_equal(out[0][0], out[1][0], f"{mode}: coefficients of two runs")
    if md == P.APG:
        oc.assert_bits_equal(out[0][1], out[1][1], "apg: planes of two runs")
    assert bool((out[0][0][..., 1] != 0).all())


def _forms(dev, clips, C, La):
    x0, noise = _rand((1, C, La), 470, 0.7).to(dev), _rand((clips, C, La), 471).to(dev)
    ones = torch.ones(La, dtype=torch.float32, device=dev)
    sd, wd = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, La, dtype=torch.float32, device=dev)
    return {"plain": {}, "edit, no mask": {"edit": (x0, noise, None)}, "edit, mask of ones": {"edit": (x0, noise, ones)},
            "one window": {"windows": (sd, wd, La)}}


_STATE = ("x", "x_saved", "d_acc", "rows_out", "counter")


def _same_bits(a, b, what):
    for ga, gb, name in zip((a.gx, a.gs, a.ga, a.gr, a.ctr), (b.gx, b.gs, b.ga, b.gr, b.ctr), _STATE):
        if ga is not None:
            oc.assert_bits_equal(gb.view, ga.view, f"{what} {name}")
            gb.check(f"{what} {name}")
    if a.gh is not None:
        oc.assert_bits_equal(b.gh.view, a.gh.view, f"{what} ring", nan_ok=True)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("form", ["plain", "edit, mask of ones", "one window"])
def test_null_projection_descriptor_is_the_plain_entry(dev, form, dt):
    """foley_op_solver_step_projected with a null second argument is foley_op_solver_step bit for bit, in every form."""
    clips, C, La, n = 2, 40, 65, 3
    coef = tables.edit_solver_table(tables.sigma_grid(n), "heun-2", n).to(dev)
    kw = _forms(dev, clips, C, La)[form]
    a, b = StepState(dev, clips, C, La, 2, DTS[dt], 472), StepState(dev, clips, C, La, 2, DTS[dt], 472)
    for it in range(n):
        pred = _halves(clips, La, C, 473 + it).to(dev)
        a.step(pred, coef, **kw)
        b.step(pred, coef, projected_entry=True, **kw)
        _same_bits(a, b, f"{form} {dt} it {it}: null projection descriptor")


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("solver,slots", [("euler", 0), ("heun-2", 0), ("euler", 1)])
@pytest.mark.parametrize("clips,C,La", [(2, 40, 65), (1, 128, 1)])
def test_forms_agree_under_a_projection(dev, clips, C, La, solver, slots, mode, dt):
    """Under a projection descriptor whose coefficients change every iteration the edit entry without a mask and with an all-ones
    mask and the windows entry with the single window [0, L) give the bits of the plain projected entry in x, x_saved, d_acc, the
    staged rows, the counter and the ring."""
    md, n = MODES[mode], 3
    sig = tables.sigma_grid(n)
    coef = tables.edit_solver_table(sig, solver, n, 0, **({"multistep_order": 2} if slots else {})).to(dev)
    rows = tables.projection_rows(n, md, 0.25, -0.5, 0.0, 0)
    p = _Proj(dev, md, rows, clips, La, C)
    forms = _forms(dev, clips, C, La)
    states = {f: StepState(dev, clips, C, La, 2, DTS[dt], 480, saved=solver != "euler", slots=slots) for f in forms}
    for it in range(n):
        pred = _halves(clips, La, C, 481 + it)
        p.project(pred, it)
        for f, kw in forms.items():
            states[f].step(pred, coef, proj=p.desc, **kw)
        assert int(states["plain"].ctr.view.item()) == it + 1
        for f in list(forms)[1:]:
            _same_bits(states["plain"], states[f], f"{f} vs plain: {mode} {solver} slots {slots} {clips}x{C}x{La} {dt} it {it}")
        p.check("forms")


# ----------------------------------------------------------------------------- the step's value against fp64
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("solver,slots", [("euler", 0), ("heun-2", 0), ("euler", 1)])
@pytest.mark.parametrize("clips,C,La", [(2, 128, 50), (3, 100, 33)])
def test_projected_step_elementwise(dev, clips, C, La, solver, slots, mode, dt):
    """The two launches, then the projected step: x, x_saved, d_acc, the ring and the staged rows of every iteration against
    opcheck.step_ref_and_bounds fed the fp64 v = a_c c + a_w w and its bound; APG with momentum and a clipping R."""
    md, n = MODES[mode], 3
    sig = tables.sigma_grid(n)
    coef = tables.solver_table(sig, solver, n, **({"multistep_order": 2} if slots else {}))
    cd = coef.to(dev)
    rows = tables.projection_rows(n, md, 0.25, -0.5, 0.0, 0)
    p = _Proj(dev, md, rows, clips, La, C)
    st = StepState(dev, clips, C, La, 2, DTS[dt], 490, saved=solver != "euler", slots=slots)
    sched = _sched(n)
    gd = rt.guidance_desc(sched.to(dev), None)
    worst = 0.0
    for it in range(n):
        pred = _halves(clips, La, C, 491 + it)
        g = float(sched[it, 0].double())
        prev = p.plane() if it else None
        if md == P.APG:
            p.set_row(it, 2, 0.5 * float(P.coef_ref(pred, clips, La, g, p.rows[it].tolist(), md, m_prev=prev)["norm"].min()))
        ref = P.coef_ref(pred, clips, La, g, p.rows[it].tolist(), md, m_prev=prev)
        p.project(pred, it, guidance=-99.0, sched=sched)
        v, e_v = P.projected_value(pred, clips, La, ref, md)
        x, xs, da, ring = st.snapshot()
        r = oc.step_ref_and_bounds(v, e_v, x, xs, da, coef[it], ring, it)
        st.step(pred, cd, guidance=-99.0, gd=gd, proj=p.desc)
        worst = max(worst, st.check(it, r, *r["x"], f"projected step {mode} {solver} slots {slots} {clips}x{C}x{La} {dt} it {it}", ring))
        p.check("projected step")
    _rec(f"solver_step.{mode}", worst)


# ----------------------------------------------------------------------------- refusals
def test_op_refusals(dev):
    import ctypes
    clips, C, La = 1, 128, 50
    lib = rt.load_library()
    pred, ctr = torch.zeros(2 * clips * La, C, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rows, coef, plane = torch.zeros(1, 4, device=dev), torch.zeros(clips, 2, device=dev), torch.zeros(clips * La, C, device=dev)
    work = torch.zeros(8, device=dev)
    d = rt.projection_desc(P.APG, rows, coef, plane)
    assert lib.foley_op_guidance_project(ctypes.byref(d), None, rt._ptr(pred), clips, C, La, 4.5, rt._ptr(ctr), rt._ptr(work), 3, rt._stream()) != 0
    assert b"work buffer" in lib.foley_last_error()
    with pytest.raises(rt.FoleyRuntimeError, match="unknown mode"):
        rt.op_guidance_project(rt.projection_desc(3, rows, coef, plane), pred, clips, La, 4.5, None, ctr)
    with pytest.raises(rt.FoleyRuntimeError, match="momentum plane"):
        rt.op_guidance_project(rt.projection_desc(P.APG, rows, coef, None), pred, clips, La, 4.5, None, ctr)
    with pytest.raises(rt.FoleyRuntimeError, match="256 channels"):
        rt.op_guidance_project(rt.projection_desc(P.ZERO_STAR, rows, coef), torch.zeros(2 * 4, 300, device=dev), 1, 4, 4.5, None, ctr)
    x = torch.zeros(clips, C, La, device=dev)
    scoef = tables.solver_table(tables.sigma_grid(2), "euler", 2).to(dev)
    with pytest.raises(rt.FoleyRuntimeError, match="two halves"):
        rt.op_solver_step(torch.zeros(3 * clips * La, C, device=dev), x, None, None, 3, 4.5, scoef, ctr, None, proj=rt.projection_desc(P.ZERO_STAR, rows, coef))
    with pytest.raises(rt.FoleyRuntimeError, match="no rescale factors"):
        rt.op_solver_step(pred, x, None, None, 2, 4.5, scoef, ctr, None, gd=rt.guidance_desc(None, torch.ones(clips, device=dev)),
                          proj=rt.projection_desc(P.ZERO_STAR, rows, coef))
    with pytest.raises(rt.FoleyRuntimeError, match="its plane"):
        rt.op_solver_step(pred, x, None, None, 2, 4.5, scoef, ctr, None, proj=rt.projection_desc(P.APG, rows, coef, None))
    assert int(ctr.item()) == 0
