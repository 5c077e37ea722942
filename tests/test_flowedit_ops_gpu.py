"""The FlowEdit step and staging ops (foley_op_flowedit_step / foley_op_flowedit_stage) against the torch restatement of
tests/flowedit_ref.py: one iteration sequence on random predictions, as test_edit_gpu.test_blend_step_op does for the edit form."""
import pytest
import torch

import flowedit_ref as FR
import opcheck as oc
from conftest import rel_err
from foley_amd.host import runtime as rt, tables

pytestmark = pytest.mark.gpu

STEPS = 6
G_SRC, G_TAR = 2.0, 4.5
SHAPES = [(1, 128, 33), (3, 128, 75), (2, 40, 50)]      # frame and channel tile edges, several variations, a single channel tile pair
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (x_src per variation, mask kind, fresh noise): every value of each at least twice
OPERANDS = [(False, "none", False), (True, "binary", True), (False, "fractional", True), (True, "per_clip", False)]


def _mask(kind, V, L, g):
    if kind == "none":
        return None
    if kind == "binary":
        return (torch.rand(L, generator=g) > 0.5).float()
    if kind == "per_clip":
        return (torch.rand(V, L, generator=g) > 0.5).float()
    m = torch.rand(1, L, generator=g)                    # fractional, with exact 0 and 1 columns
    m[:, :5] = 0.0
    m[:, 5:10] = 1.0
    return m


def _state(dev, V, Cc, L, per_clip_src, mask_kind, fresh, rows_dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    x_src = torch.randn(V if per_clip_src else 1, Cc, L, generator=g)
    noise = torch.randn(STEPS if fresh else 1, V, Cc, L, generator=g)
    mask = _mask(mask_kind, V, L, g)
    z = oc.guarded((V, Cc, L), torch.float32, dev, rows=(1, 1))
    z.view.copy_(x_src.expand(V, -1, -1) + 0.3 * torch.randn(V, Cc, L, generator=g))
    rows = oc.guarded((4 * V * L, Cc), rows_dtype, dev, rows=(2, 3))
    return g, x_src, noise, mask, z, rows


def _check_rows(rows, z_dev, x_src, n, s, rows_dtype, what):
    z_src, z_tar = FR.ref_inputs(z_dev, x_src, n, s)
    want = FR.rows_of(z_src, z_tar, rows_dtype)
    got = rows.view.cpu()
    if rows_dtype == torch.float32:
        assert torch.equal(got, want), what
    else:
        assert rel_err(got.float(), want.float()) < 1e-2, what
    rows.check(what)
    rows.view.fill_(float("nan"))


@pytest.mark.parametrize("V,Cc,L", SHAPES)
@pytest.mark.parametrize("rows_dtype", DTYPES)
@pytest.mark.parametrize("per_clip_src,mask_kind,fresh", OPERANDS)
def test_flowedit_step_op(dev, V, Cc, L, rows_dtype, per_clip_src, mask_kind, fresh):
    g, x_src, noise, mask, z, rows = _state(dev, V, Cc, L, per_clip_src, mask_kind, fresh, rows_dtype)
    coef = tables.edit_solver_table(tables.sigma_grid(STEPS), "euler", STEPS)
    d = lambda t: None if t is None else t.to(dev)
    x_src_d, noise_d, mask_d, coef_d = d(x_src), d(noise), d(mask), d(coef)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    step_u = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in range(STEPS):
        pred = torch.randn(4 * V * L, Cc, generator=g)
        n_next = noise[min(it + 1, STEPS - 1)] if fresh else noise[0]
        before = z.view.cpu().clone()
        zu = before.to(dev)                                # the unmasked step on the same state
        step_u.fill_(it)
        rt.op_flowedit_step(pred.to(dev), zu, x_src_d, noise_d, None, coef_d, step_u, None, G_SRC, G_TAR)
        rt.op_flowedit_step(pred.to(dev), z.view, x_src_d, noise_d, mask_d, coef_d, step, rows.view, G_SRC, G_TAR)
        torch.cuda.synchronize()
        what = f"iteration {it}"
        assert int(step) == it + 1 and int(step_u) == it + 1, what
        z_ref, _zs, _zt = FR.ref_flowedit_step(pred, before, x_src, n_next, mask, coef[it], G_SRC, G_TAR)
        got = z.view.cpu()
        assert rel_err(got, z_ref) < 1e-6, what
        z.check(what)
        if mask is None:
            assert torch.equal(got, zu.cpu()), what
        else:
            mm = mask.view(-1, 1, L).expand(V, Cc, L)
            assert torch.equal(got[mm == 0], before[mm == 0]), what          # m = 0: the frame keeps its value bit for bit
            assert torch.equal(got[mm == 1], zu.cpu()[mm == 1]), what        # m = 1: the unmasked update bit for bit
        _check_rows(rows, got, x_src, n_next, coef[it, 5], rows_dtype, what)


@pytest.mark.parametrize("V,Cc,L", SHAPES)
@pytest.mark.parametrize("rows_dtype", DTYPES)
@pytest.mark.parametrize("per_clip_src,fresh", [(False, True), (True, False)])
def test_flowedit_stage_op(dev, V, Cc, L, rows_dtype, per_clip_src, fresh):
    _g, x_src, noise, _mask_, z, rows = _state(dev, V, Cc, L, per_clip_src, "none", fresh, rows_dtype, seed=13)
    x_src_d, noise_d = x_src.to(dev), noise.to(dev)
    r = STEPS - 2 if fresh else 0
    for sigma in (1.0, 0.73, 0.0):
        rt.op_flowedit_stage(z.view, x_src_d, noise_d, rows.view, sigma, r)
        torch.cuda.synchronize()
        if sigma == 0.0 and rows_dtype == torch.float32:
            # the source branch is x_src itself; the target branch is (z - x_src) + x_src: z to one rounding, z where z == x_src
            got = rows.view.cpu().view(2, 2 * V, L, Cc)
            xs = x_src.expand(V, -1, -1)
            assert torch.equal(got[0, :V], xs.permute(0, 2, 1)) and torch.equal(got[1, :V], xs.permute(0, 2, 1))
            assert rel_err(got[0, V:], z.view.cpu().permute(0, 2, 1)) < 1e-6
        _check_rows(rows, z.view.cpu(), x_src, noise[r], sigma, rows_dtype, f"sigma {sigma}")
    z.check("stage leaves z alone")
    # z == x_src: the target rows are the source rows bit for bit
    z.view.copy_(x_src_d.expand(V, -1, -1))
    rt.op_flowedit_stage(z.view, x_src_d, noise_d, rows.view, 0.73, r)
    got = rows.view.cpu().view(2, 2, V * L, Cc)
    assert torch.equal(got[:, 0], got[:, 1])
    assert not torch.isnan(got.float()).any()


def test_flowedit_op_refusals(dev):
    V, Cc, L = 3, 128, 40
    lib = rt.load_library()
    with pytest.raises(rt.FoleyRuntimeError, match="null descriptor"):
        rt._check(lib, lib.foley_op_flowedit_step(None, None), "foley_op_flowedit_step")
    with pytest.raises(rt.FoleyRuntimeError, match="null descriptor"):
        rt._check(lib, lib.foley_op_flowedit_stage(None, 0.5, 0, None), "foley_op_flowedit_stage")
    z = torch.zeros(V, Cc, L, device=dev)
    pred = torch.zeros(4 * V * L, Cc, device=dev)
    noise = torch.zeros(STEPS, V, Cc, L, device=dev)
    rows = torch.empty(4 * V * L, Cc, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    coef = tables.edit_solver_table(tables.sigma_grid(STEPS), "euler", STEPS).to(dev)
    with pytest.raises(rt.FoleyRuntimeError, match="src_clips"):
        rt.op_flowedit_step(pred, z, torch.zeros(2, Cc, L, device=dev), noise, None, coef, step, rows, G_SRC, G_TAR)
    with pytest.raises(rt.FoleyRuntimeError, match="mask_clips"):
        rt.op_flowedit_step(pred, z, z, noise, torch.ones(2, L, device=dev), coef, step, rows, G_SRC, G_TAR)
    with pytest.raises(rt.FoleyRuntimeError, match="noise_rows"):
        rt.op_flowedit_step(pred, z, z, noise[:2].contiguous(), None, coef, step, rows, G_SRC, G_TAR)
    with pytest.raises(rt.FoleyRuntimeError, match="src_clips"):
        rt.op_flowedit_stage(z, torch.zeros(2, Cc, L, device=dev), noise, rows, 0.5, 0)
    with pytest.raises(rt.FoleyRuntimeError, match="noise_row"):
        rt.op_flowedit_stage(z, z, noise, rows, 0.5, STEPS)
    plain = tables.solver_table(tables.sigma_grid(STEPS), "euler", STEPS).to(dev)          # no blend rows
    with pytest.raises(rt.FoleyRuntimeError, match="FOLEY_STEP_BLEND"):
        rt.op_flowedit_step(pred, z, z, noise, None, plain, step, rows, G_SRC, G_TAR)
    torch.cuda.synchronize()
    assert int(step) == 0                                  # a refused call launches nothing
