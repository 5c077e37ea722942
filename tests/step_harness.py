"""What the op-level tests of the solver step share: the shapes and seeds' generator, and the guarded device state of one run
with the checks every iteration gets (test_rowops_elementwise_gpu.py, test_guidance_ops_gpu.py, test_multistep_ops_gpu.py); the
torch restatement of one step that the edit and windows step tests compare with."""
import torch

import opcheck as oc
from foley_amd.host import runtime as rt, tables

DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ALL3 = list(DTS)
STEP_SHAPES = [(2, 128, 50), (3, 128, 33), (1, 128, 1), (2, 96, 31), (2, 40, 65)]      # ragged 32-tiles over L and over C, the single frame
SOLVER_ITERS = {"euler": 2, "heun-2": 3, "midpoint-2": 3, "kutta-4": 5}      # every row of each coefficient table, and its first repeat
GUIDANCE = 4.5


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _filled(shape, dtype, dev, src, rows=(1, 1)):
    """A guarded buffer whose interior starts as `src` (state a kernel updates in place)."""
    g = oc.guarded(shape, dtype, dev, rows=rows)
    g.view.copy_(src.to(dev))
    return g


def ref_step(pred, x, x_saved, d_acc, row, ncfg, g, x0=None, noise=None, mask=None):
    """torch restatement of one step on the kernel's state (test_edit_gpu.py, test_windows_gpu.py): (x, x_saved, d_acc).  With x0
    and noise (mask None: all ones) a row flagged STEP_BLEND ends in the edit blend; without them it is the plain step."""
    clips, Cc, L = x.shape
    w_new, w_acc, dt, w_store, flags, s = [float(v) for v in row[:6]]
    flags = int(flags)
    P = pred.view(ncfg, clips, L, Cc).permute(0, 1, 3, 2)
    v = P[0] + g * (P[1] - P[0]) if ncfg == 2 else P[0]
    acc = torch.zeros_like(x) if flags & tables.STEP_ACC_RESET else d_acc
    deriv = w_new * v + w_acc * acc if w_acc != 0 else w_new * v
    base = x_saved if flags & tables.STEP_USE_SAVED else x
    xs = x.clone() if flags & tables.STEP_SAVE_X else x_saved
    xn = base + deriv * dt
    if x0 is not None and flags & tables.STEP_BLEND:
        m = torch.ones(1, 1, L, device=x.device) if mask is None else mask.view(-1, 1, L)
        xn = m * xn + (1 - m) * (s * noise + (1 - s) * x0)
    return xn, xs, acc + w_store * v


class StepState:
    """x / x_saved / d_acc / rows_out of one run and - slots > 0 - a NaN-filled velocity ring, all guarded; the step counter."""

    def __init__(self, dev, clips, C, L, ncfg, dtype, seed, saved=True, rows=True, slots=0):
        self.dev, self.shape, self.ncfg, self.dtype = dev, (clips, C, L), ncfg, dtype
        self.gx = _filled((clips, C, L), torch.float32, dev, _rand((clips, C, L), seed))
        self.gs = _filled((clips, C, L), torch.float32, dev, _rand((clips, C, L), seed + 1)) if saved else None
        self.ga = _filled((clips, C, L), torch.float32, dev, _rand((clips, C, L), seed + 2)) if saved else None
        self.gh = oc.guarded((slots, clips, C, L), torch.float32, dev, rows=(1, 1)) if slots else None      # NaN inside, guard slabs around
        self.gr = oc.guarded((ncfg * clips * L, C), dtype, dev, rows=(2, 3)) if rows else None
        self.ctr = oc.guarded((1, 1), torch.int32, dev, rows=(1, 1), fill=0)

    @property
    def args(self):
        v = lambda g: g.view if g is not None else None
        return v(self.gx), v(self.gs), v(self.ga), v(self.gr)

    def snapshot(self):
        """(x, x_saved, d_acc, ring) on the CPU, None for what the run does not have."""
        c = lambda g: g.view.cpu().clone() if g is not None else None
        return c(self.gx), c(self.gs), c(self.ga), c(self.gh)

    def step(self, pred, coef_dev, guidance=GUIDANCE, **kw):
        """One rt.op_solver_step on this state (with its ring, when it has one); kw: gd / edit / windows / slots."""
        if self.gh is not None:
            kw["hist"] = self.gh.view
        rt.op_solver_step(pred.to(self.dev), *self.args[:3], self.ncfg, guidance, coef_dev, self.ctr.view.view(1), self.args[3], **kw)

    def check(self, it, r, x_ref, x_bound, what, ring_before=None):
        """After iteration `it`: x against (x_ref, x_bound), x_saved bit for bit, d_acc in its bound, the counter, the staged rows
        bit for bit from the device's own x in every CFG copy, the written ring slot in its bound and the others bit for bit as
        `ring_before` held them, all guards."""
        worst = oc.assert_elementwise(self.gx.view, x_ref, x_bound, what + " x")
        if self.gh is not None:
            ring = self.gh.view.cpu()
            worst = max(worst, oc.assert_elementwise(ring[r["slot"]], *r["hist"], what + " written slot"))
            for s in range(ring.shape[0]):
                if s != r["slot"]:
                    oc.assert_bits_equal(ring[s], ring_before[s], what + f" untouched slot {s}")
        if self.gs is not None:
            oc.assert_bits_equal(self.gs.view, r["x_saved"].float(), what + " x_saved")
            worst = max(worst, oc.assert_elementwise(self.ga.view, *r["d_acc"], what + " d_acc"))
        assert int(self.ctr.view.item()) == it + 1, what
        if self.gr is not None:
            oc.assert_bits_equal(self.gr.view, oc.rows_of(self.gx.view, self.ncfg, self.dtype), what + " rows_out (every CFG copy)")
            self.gr.view.fill_(float("nan"))
        for g in (self.gx, self.gs, self.ga, self.gh, self.gr, self.ctr):
            if g is not None:
                g.check(what)
        return worst
