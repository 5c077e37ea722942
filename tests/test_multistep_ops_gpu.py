"""The history instantiations of the solver step (foley_op_solver_step with a ring), element by element: every iteration of a
run of order + 1 iterations from a NaN-filled ring against opcheck.step_ref_and_bounds(..., ring, it) - x, the written slot, the
staged rows - with the untouched slot and all guard bands bit for bit; the plain, edit and windows forms, the guidance descriptor,
the zero-weight table against the step without a ring, the refusals."""
import pytest
import torch

import opcheck as oc
from conftest import record_parity
from foley_amd.host import long_form, runtime as rt, tables
from step_harness import DTS, GUIDANCE, StepState, _rand

pytestmark = pytest.mark.gpu

SHAPES = [(2, 128, 50), (3, 128, 33), (1, 128, 1), (2, 40, 65)]      # ragged 32-tiles over L and over C, the single frame
NAN = float("nan")
_WORST = {}


def _rec(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), float(ratio))
    record_parity(f"elementwise.rowops.solver_step_hist.{family}", err_over_bound=_WORST[family])


def _table(order, n, edit=False):
    """n rows of the order's table on a shifted (non-uniform) grid: the warm-up rows, the first full row and - order 3, n = 4 - the
    row that wraps the ring."""
    sig = tables.sigma_grid(n, 3.0)
    if edit:
        return tables.edit_solver_table(sig, "euler", n, 0, multistep_order=order)
    return tables.solver_table(sig, "euler", n, multistep_order=order)


def _hist_ref(pred, st, coef_row, it, gv=oc.f32(GUIDANCE), gt=oc.f32(GUIDANCE), scale=None):
    """(the fp64 step with the history terms from the state `st` holds now, the ring as it is before the step)."""
    x, xs, da, ring = st.snapshot()
    v, e_v = oc.combine_ref(pred, x.shape[0], x.shape[2], st.ncfg, gv, gt, scale)
    return oc.step_ref_and_bounds(v, e_v, x, xs, da, coef_row, ring, it), ring


def test_tables_carry_what_the_cases_claim():
    for order in (2, 3):
        t = _table(order, order + 1)
        assert t[0, 4] == 0 and bool((t[1:, 4] == tables.STEP_HIST).all())
        assert float(t[order - 1, 4 + order]) != 0.0 and bool((t[:order - 1, 4 + order] == 0).all())      # full history from row order - 1
    assert float(_table(3, 4)[1, 7]) == 0.0 and float(_table(3, 4)[3, 7]) != 0.0


# ----------------------------------------------------------------------------- plain form
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("ncfg", [1, 2])
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("clips,C,L", SHAPES)
def test_step_hist_elementwise(dev, clips, C, L, order, ncfg, dt):
    """order + 1 iterations from a ring of NaN: the warm-up rows must not read it (a NaN would reach x), iteration `order` uses the
    full history and - order 3 - reads v_{n-2} from the slot it then overwrites; the fourth iteration of order 3 wraps the ring."""
    n = order + 1
    coef = _table(order, n)
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 300, saved=ncfg == 2, slots=order - 1)
    cd = coef.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 301 + it)
        r, ring = _hist_ref(pred, st, coef[it], it)
        st.step(pred, cd)
        worst = max(worst, st.check(it, r, *r["x"], f"step_hist order {order} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it}", ring))
    _rec(f"order{order}", worst)


@pytest.mark.parametrize("order", [2, 3])
def test_step_hist_three_halves_with_descriptor(dev, order):
    """ncfg 3 with a schedule table and per-clip factors: the slot receives the guided value as the step used it, factor included."""
    clips, C, L, ncfg, n = 3, 128, 33, 3, order + 1
    coef = _table(order, n)
    sched = torch.tensor([[7.0, 2.0], [1.0, 1.0], [3.5, 4.5], [6.0, 1.5]])[:n].contiguous()
    scale = torch.tensor([0.8, 1.0, 1.15])
    sd, cs = sched.to(dev), scale.to(dev)
    gd = rt.guidance_desc(sd, cs)
    st = StepState(dev, clips, C, L, ncfg, torch.bfloat16, 320, saved=False, slots=order - 1)
    cd = coef.to(dev)
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 321 + it)
        r, ring = _hist_ref(pred, st, coef[it], it, float(sched[it, 0].double()), float(sched[it, 1].double()), scale)
        st.step(pred, cd, gd=gd)
        _rec(f"order{order}.guided", st.check(it, r, *r["x"], f"step_hist guided order {order} it {it}", ring))
    assert torch.equal(cs.cpu(), scale) and torch.equal(sd.cpu(), sched)


# ----------------------------------------------------------------------------- edit form
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("clips,C,L", SHAPES)
def test_step_hist_edit_elementwise(dev, clips, C, L, order, dt):
    """A fractional mask with exact 0 and 1 entries; every euler row is a blend row, so history rows blend too.  The slot keeps
    the velocity, not the blended sample."""
    n, ncfg = order + 1, 2
    coef = _table(order, n, edit=True)
    assert bool(((coef[:, 4].int() & tables.STEP_BLEND) != 0).all()) and int(coef[n - 1, 4]) == tables.STEP_BLEND | tables.STEP_HIST
    x0, noise = _rand((1, C, L), 331, 0.7), _rand((clips, C, L), 332)
    mask = torch.rand(clips, L, generator=torch.Generator().manual_seed(333))
    mask[:, : L // 3] = 0.0
    mask[:, L // 3: L // 2] = 1.0
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 334, saved=False, slots=order - 1)
    cd, ops = coef.to(dev), (x0.to(dev), noise.to(dev), mask.to(dev))
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 335 + it)
        r, ring = _hist_ref(pred, st, coef[it], it)
        ref, bound = oc.edit_blend_ref_and_bound(r["x"][0], r["x"][1].e, r["s_next"], x0, noise, mask)
        st.step(pred, cd, edit=ops)
        worst = max(worst, st.check(it, r, ref, bound, f"step_hist edit order {order} {clips}x{C}x{L} {dt} it {it}", ring))
    _rec(f"order{order}.edit", worst)


# ----------------------------------------------------------------------------- windows form
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("order", [2, 3])
def test_step_hist_windows_elementwise(dev, order, dt):
    """2 variations x 2 windows of 33 frames at starts (0, 20): frames 20 .. 32 are covered twice, a window edge lies inside a
    32-frame tile.  The last row is a plain row (flag cleared), the others blend; each window keeps the history of its own
    velocities either way."""
    C, L, starts, ncfg = 128, 33, [0, 20], 2
    plan = long_form.WindowPlan.from_frames(starts, L)
    n_win, clips, n = plan.n_win, 2 * plan.n_win, order + 1
    coef = _table(order, n, edit=True)
    coef[n - 1, 4] = float(int(coef[n - 1, 4]) & ~tables.STEP_BLEND)          # a history row without the blend
    coef[n - 1, 5] = 0.0
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 350, saved=False, slots=order - 1)
    cd, sd, wd = coef.to(dev), torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 351 + it)
        r, ring = _hist_ref(pred, st, coef[it], it)
        ref, bound = r["x"]
        blend = bool(r["flags"] & oc.STEP_BLEND)
        assert blend == (it < n - 1)
        if blend:
            ref, e, _, _, _ = oc.windows_mean_ref_and_bound(ref, bound.e, n_win, starts, plan.weights)
            bound = oc.Bound(e)
        st.step(pred, cd, windows=(sd, wd, plan.Ltot))
        what = f"step_hist windows order {order} {dt} it {it}"
        worst = max(worst, st.check(it, r, ref, bound, what, ring))
        if blend:                        # the two windows agree on the frames both cover, bit for bit
            xg = st.gx.view.cpu().view(2, n_win, C, L)
            oc.assert_bits_equal(xg[:, 0, :, 20:], xg[:, 1, :, :13], what + " windows agree")
    _rec(f"order{order}.windows", worst)


# ----------------------------------------------------------------------------- zero history weights: the Euler bits
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("dt", list(DTS))
def test_zero_history_weights_are_the_plain_step(dev, dt, flagged):
    """The plain euler table through the history kernel (two slots of NaN), also with STEP_HIST set on rows whose weights are
    zero: x and the staged rows carry the bits of the step without a ring, and the ring receives the velocities."""
    clips, C, L, ncfg, n = 3, 128, 33, 2, 3
    coef = tables.solver_table(tables.sigma_grid(n, 3.0), "euler", n)
    if flagged:
        coef[:, 4] = float(tables.STEP_HIST)
    cd = coef.to(dev)
    x0 = _rand((clips, C, L), 370)
    xa, xb = x0.to(dev), x0.to(dev)
    ra, rb = (torch.full((ncfg * clips * L, C), NAN, dtype=DTS[dt], device=dev) for _ in range(2))
    ca, cb = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    ring = torch.full((2, clips, C, L), NAN, device=dev)
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 371 + it).to(dev)
        rt.op_solver_step(pred, xa, None, None, ncfg, GUIDANCE, cd, ca, ra)
        rt.op_solver_step(pred, xb, None, None, ncfg, GUIDANCE, cd, cb, rb, hist=ring)
        oc.assert_bits_equal(xb, xa, f"zero weights {dt} it {it} x")
        oc.assert_bits_equal(rb, ra, f"zero weights {dt} it {it} rows")
    assert not bool(torch.isnan(ring).any()) and int(cb.item()) == n


# ----------------------------------------------------------------------------- refusals
def test_step_hist_refusals(dev):
    clips, C, L = 1, 40, 5
    x, pred = torch.zeros(clips, C, L, device=dev), torch.zeros(clips * L, C, device=dev)
    coef, ctr = _table(2, 3).to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ring = torch.zeros(3, clips, C, L, device=dev)
    for kw in (dict(slots=0), dict(slots=3)):
        with pytest.raises(rt.FoleyRuntimeError, match="slots"):
            rt.op_solver_step(pred, x, None, None, 1, 1.0, coef, ctr, None, hist=ring, **kw)
    with pytest.raises(rt.FoleyRuntimeError, match="ring"):
        rt.op_solver_step(pred, x, None, None, 1, 1.0, coef, ctr, None, hist=None, slots=1)
    with pytest.raises(rt.FoleyRuntimeError, match="exclude"):
        rt.op_solver_step(pred, x, None, None, 1, 1.0, coef, ctr, None, hist=ring[:1].contiguous(), edit=(x, x, None),
                          windows=(torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, L, device=dev), L))
    assert int(ctr.item()) == 0 and not bool(x.any())
