"""The history instantiations of the solver step (foley_op_solver_step_hist), element by element: every iteration of a run of
order + 1 iterations from a NaN-filled ring against tests/multistep_ref.py::step_ref_and_bounds - x, the written slot, the staged
rows - with the untouched slot and all guard bands bit for bit; the plain, edit and windows forms, the guidance descriptor, the
zero-weight table against foley_op_solver_step, the refusals."""
import pytest
import torch

import guidance_ref as G
import multistep_ref as M
import opcheck as oc
from conftest import record_parity
from foley_amd.host import long_form, runtime as rt, tables

pytestmark = pytest.mark.gpu

DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(2, 128, 50), (3, 128, 33), (1, 128, 1), (2, 40, 65)]      # ragged 32-tiles over L and over C, the single frame
GUIDANCE = 4.5
NAN = float("nan")
_WORST = {}


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


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


class _State:
    """Guarded device state of one run: x (and x_saved / d_acc when `saved`), the NaN-filled ring, the staged rows, the counter."""

    def __init__(self, dev, clips, C, L, ncfg, dtype, slots, seed, saved):
        f = lambda s: self._filled((clips, C, L), dev, _rand((clips, C, L), s))
        self.dev, self.ncfg, self.dtype, self.slots = dev, ncfg, dtype, slots
        self.gx = f(seed)
        self.gs, self.ga = (f(seed + 1), f(seed + 2)) if saved else (None, None)
        self.gh = oc.guarded((slots, clips, C, L), torch.float32, dev, rows=(1, 1))      # NaN inside, guard slabs around
        self.gr = oc.guarded((ncfg * clips * L, C), dtype, dev, rows=(2, 3))
        self.ctr = oc.guarded((1, 1), torch.int32, dev, rows=(1, 1), fill=0)

    @staticmethod
    def _filled(shape, dev, src):
        g = oc.guarded(shape, torch.float32, dev, rows=(1, 1))
        g.view.copy_(src.to(dev))
        return g

    def snapshot(self):
        c = lambda g: g.view.cpu().clone() if g is not None else None
        return c(self.gx), c(self.gs), c(self.ga), c(self.gh)

    def step(self, pred, coef_dev, **kw):
        v = lambda g: g.view if g is not None else None
        rt.op_solver_step_hist(self.gh.view, pred.to(self.dev), self.gx.view, v(self.gs), v(self.ga), self.ncfg, GUIDANCE, coef_dev,
                               self.ctr.view.view(1), self.gr.view, **kw)

    def check(self, it, r, x_ref, x_bound, ring_before, what):
        worst = oc.assert_elementwise(self.gx.view, x_ref, x_bound, what + " x")
        ring = self.gh.view.cpu()
        worst = max(worst, oc.assert_elementwise(ring[r["slot"]], *r["hist"], what + " written slot"))
        for s in range(self.slots):
            if s != r["slot"]:
                oc.assert_bits_equal(ring[s], ring_before[s], what + f" untouched slot {s}")
        if self.gs is not None:
            oc.assert_bits_equal(self.gs.view, r["x_saved"].float(), what + " x_saved")
            worst = max(worst, oc.assert_elementwise(self.ga.view, *r["d_acc"], what + " d_acc"))
        assert int(self.ctr.view.item()) == it + 1, what
        oc.assert_bits_equal(self.gr.view, oc.rows_of(self.gx.view, self.ncfg, self.dtype), what + " rows_out (every CFG copy)")
        self.gr.view.fill_(NAN)
        for g in (self.gx, self.gs, self.ga, self.gh, self.gr, self.ctr):
            if g is not None:
                g.check(what)
        return worst


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
    st = _State(dev, clips, C, L, ncfg, DTS[dt], order - 1, 300, saved=ncfg == 2)
    cd = coef.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 301 + it)
        x, xs, da, ring = st.snapshot()
        v, e_v = G.combine_ref(pred, clips, L, ncfg, oc.f32(GUIDANCE), oc.f32(GUIDANCE))
        r = M.step_ref_and_bounds(v, e_v, x, xs, da, coef[it], ring, it)
        st.step(pred, cd)
        worst = max(worst, st.check(it, r, *r["x"], ring, f"step_hist order {order} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it}"))
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
    st = _State(dev, clips, C, L, ncfg, torch.bfloat16, order - 1, 320, saved=False)
    cd = coef.to(dev)
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 321 + it)
        x, xs, da, ring = st.snapshot()
        v, e_v = G.combine_ref(pred, clips, L, ncfg, float(sched[it, 0].double()), float(sched[it, 1].double()), scale)
        r = M.step_ref_and_bounds(v, e_v, x, xs, da, coef[it], ring, it)
        st.step(pred, cd, gd=gd)
        _rec(f"order{order}.guided", st.check(it, r, *r["x"], ring, f"step_hist guided order {order} it {it}"))
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
    st = _State(dev, clips, C, L, ncfg, DTS[dt], order - 1, 334, saved=False)
    cd, ops = coef.to(dev), (x0.to(dev), noise.to(dev), mask.to(dev))
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 335 + it)
        x, xs, da, ring = st.snapshot()
        v, e_v = G.combine_ref(pred, clips, L, ncfg, oc.f32(GUIDANCE), oc.f32(GUIDANCE))
        r = M.step_ref_and_bounds(v, e_v, x, xs, da, coef[it], ring, it)
        ref, bound = oc.edit_blend_ref_and_bound(r["x"][0], r["x"][1].e, r["s_next"], x0, noise, mask)
        st.step(pred, cd, edit=ops)
        worst = max(worst, st.check(it, r, ref, bound, ring, f"step_hist edit order {order} {clips}x{C}x{L} {dt} it {it}"))
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
    st = _State(dev, clips, C, L, ncfg, DTS[dt], order - 1, 350, saved=False)
    cd, sd, wd = coef.to(dev), torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 351 + it)
        x, xs, da, ring = st.snapshot()
        v, e_v = G.combine_ref(pred, clips, L, ncfg, oc.f32(GUIDANCE), oc.f32(GUIDANCE))
        r = M.step_ref_and_bounds(v, e_v, x, xs, da, coef[it], ring, it)
        ref, bound = r["x"]
        blend = bool(r["flags"] & oc.STEP_BLEND)
        assert blend == (it < n - 1)
        if blend:
            ref, e, _, _, _ = oc.windows_mean_ref_and_bound(ref, bound.e, n_win, starts, plan.weights)
            bound = oc.Bound(e)
        st.step(pred, cd, windows=(sd, wd, plan.Ltot))
        what = f"step_hist windows order {order} {dt} it {it}"
        worst = max(worst, st.check(it, r, ref, bound, ring, what))
        if blend:                        # the two windows agree on the frames both cover, bit for bit
            xg = st.gx.view.cpu().view(2, n_win, C, L)
            oc.assert_bits_equal(xg[:, 0, :, 20:], xg[:, 1, :, :13], what + " windows agree")
    _rec(f"order{order}.windows", worst)


# ----------------------------------------------------------------------------- zero history weights: the Euler bits
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("dt", list(DTS))
def test_zero_history_weights_are_the_plain_step(dev, dt, flagged):
    """The plain euler table through the history kernel (two slots of NaN), also with STEP_HIST set on rows whose weights are
    zero: x and the staged rows carry the bits of foley_op_solver_step, and the ring receives the velocities."""
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
        rt.op_solver_step_hist(ring, pred, xb, None, None, ncfg, GUIDANCE, cd, cb, rb)
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
            rt.op_solver_step_hist(ring, pred, x, None, None, 1, 1.0, coef, ctr, None, **kw)
    with pytest.raises(rt.FoleyRuntimeError, match="ring"):
        rt.op_solver_step_hist(None, pred, x, None, None, 1, 1.0, coef, ctr, None, slots=1)
    with pytest.raises(rt.FoleyRuntimeError, match="exclude"):
        rt.op_solver_step_hist(ring[:1].contiguous(), pred, x, None, None, 1, 1.0, coef, ctr, None, edit=(x, x, None),
                               windows=(torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, L, device=dev), L))
    assert int(ctr.item()) == 0 and not bool(x.any())
