"""The step cache's kernels at op level (csrc/rowops.hip: cache_probe_kernel + cache_rel_kernel, cache_axpy_kernel): the probe's m
per element against fp64 under opcheck.layernorm_ref_and_bound, its change measure, the exact zeros, repetition bit for bit,
guard bands around every output; delta / apply bit for bit against fp32 a - b / a + b.

Shapes: D = 256 (one float4 per lane), 1408 (xl: 22 x 64 floats, not a multiple of 256: the clamped loads and the column guard) and
1536 (xxl); La = 33 and 50 (neither a multiple of the four rows of a workgroup: a ragged last workgroup per batch row); Bc = 1, 2
and 6 batch rows (a workgroup never meets two); shift / scale as one vector (the two-stream blocks' modulation) and as Ls = 16 rows
per half up-sampled per token (the single blocks')."""
import pytest
import torch

import opcheck as oc
from opcheck import U32
from foley_amd.host import runtime as rt, tables

pytestmark = pytest.mark.gpu

LS = 16


def _rand(shape, seed, scale=1.0, offset=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + offset


def _operands(dev, D, La, Bc, mode, seed):
    """(a0 [Bc La, D], shift_full, scale_full, RowBcast shift, RowBcast scale): rows offset from 0 so that the centring matters."""
    ncfg = 1 if Bc == 1 else 2
    clips = Bc // ncfg
    a0 = _rand((Bc * La, D), seed, 1.0, 3.0)
    if mode == "vec":
        sh, sc = _rand((D,), seed + 1), _rand((D,), seed + 2, 0.3)
        full = lambda t: t.expand(Bc * La, D)
        rb = lambda t: rt.rowbcast(t.to(dev), 0)
    else:
        sh, sc = _rand((ncfg * LS, D), seed + 1), _rand((ncfg * LS, D), seed + 2, 0.3)
        idx = tables.nearest_exact_index(La, LS)
        full = lambda t: t.view(ncfg, LS, D)[:, idx].unsqueeze(1).expand(ncfg, clips, La, D).reshape(Bc * La, D)
        rb = lambda t: rt.rowbcast(t.to(dev), 2, rows_per_cfg=clips * La, L=La, Ls=LS)
    return a0, full(sh), full(sc), rb(sh), rb(sc)


def _bufs(dev, M, D, Bc, old):
    gm, gr = oc.guarded((M, D), torch.float32, dev), oc.guarded((Bc, 1), torch.float32, dev, rows=(1, 1))
    gm.view.copy_(old.to(dev))
    return gm, gr


def _rel64(m, old, Bc):
    num, den = (m.double() - old.double()).abs().view(Bc, -1).sum(1), old.double().abs().view(Bc, -1).sum(1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(den))


@pytest.mark.parametrize("Bc", [1, 2, 6])
@pytest.mark.parametrize("La", [33, 50])
@pytest.mark.parametrize("D", [256, 1408, 1536])
def test_probe(dev, D, La, Bc):
    M = Bc * La
    for mode in ("vec", "up"):
        what = "D %d La %d Bc %d %s" % (D, La, Bc, mode)
        eps = 1e-6 if mode == "vec" else 1e-5
        a0, sh_f, sc_f, rb_sh, rb_sc = _operands(dev, D, La, Bc, mode, 100 + D + La + Bc)
        old = _rand((M, D), 7, 1.2)
        gm, gr = _bufs(dev, M, D, Bc, old)
        a0d = a0.to(dev)
        rt.op_cache_probe(a0d, Bc, eps, rb_sh, rb_sc, gm.view, gr.view.view(-1))
        torch.cuda.synchronize()
        for g, n in ((gm, "m_prev"), (gr, "rel")):
            g.check(what + ": " + n)
        # m per element against fp64
        _x, m64, _bx, bound = oc.layernorm_ref_and_bound(a0, sh_f, sc_f, eps, torch.float32)
        m = gm.view.cpu()
        worst = oc.assert_elementwise(m, m64, bound, what + ": m")
        oc.assert_bits_equal(a0d, a0, what + ": a0 is only read")
        # the change measure from the m the kernel wrote (checked above) and the old values: two sums of La D non-negative fp32
        # terms in any order (each at most n unit round-offs of its sum), the differences' and the division's roundings
        rel, want = gr.view.view(-1).cpu().double(), _rel64(m, old, Bc)
        tol = (La * D + 8) * U32
        print("%s: m err / bound %.3f, rel %s, |rel - fp64| / rel max %.2e (gate %.2e)" % (
            what, worst, ["%.4f" % r for r in rel], float(((rel - want).abs() / want).max()), tol))
        assert bool(((rel - want).abs() <= tol * want).all()), (what, rel, want)
        assert float(want.min()) > 0.5                              # unrelated old values: a change of order 1
        # and from the fp64 m: each |m - old| term may also move by that element's bound on m
        den = old.double().abs().view(Bc, -1).sum(1)
        slack = bound.total(m64, m).expand_as(m64).reshape(Bc, -1).sum(1) / den
        want64 = _rel64(m64, old, Bc)
        assert bool(((rel - want64).abs() <= tol * want64 + slack).all()), (what, rel, want64, slack)
        # repeat from the same state: the same bits, in m and in rel
        gm2, gr2 = _bufs(dev, M, D, Bc, old)
        rt.op_cache_probe(a0d, Bc, eps, rb_sh, rb_sc, gm2.view, gr2.view.view(-1))
        oc.assert_bits_equal(gm2.view, m, what + ": m on repetition")
        oc.assert_bits_equal(gr2.view, gr.view.cpu(), what + ": rel on repetition")
        # no change: m_prev == m gives exactly 0.0f and leaves m as it is
        rt.op_cache_probe(a0d, Bc, eps, rb_sh, rb_sc, gm2.view, gr2.view.view(-1))
        oc.assert_bits_equal(gr2.view, torch.zeros(Bc, 1), what + ": rel without a change")
        oc.assert_bits_equal(gm2.view, m, what + ": m without a change")
        # zeros: an all-zero m_prev gives rel_b == 0.0f (not inf, not NaN), and m all the same
        gm3, gr3 = _bufs(dev, M, D, Bc, torch.zeros(M, D))
        rt.op_cache_probe(a0d, Bc, eps, rb_sh, rb_sc, gm3.view, gr3.view.view(-1))
        oc.assert_bits_equal(gr3.view, torch.zeros(Bc, 1), what + ": rel from zeros")
        oc.assert_bits_equal(gm3.view, m, what + ": m from zeros")
        for g in (gm2, gr2, gm3, gr3):
            g.check(what + ": guards of the repetitions")


def test_probe_rows_differ_per_batch_row(dev):
    """One batch row's old values equal its m, the others' do not: only that row reports 0 - a record never mixes two rows."""
    D, La, Bc = 256, 50, 6
    a0, sh_f, sc_f, rb_sh, rb_sc = _operands(dev, D, La, Bc, "up", 3)
    gm, gr = _bufs(dev, Bc * La, D, Bc, torch.zeros(Bc * La, D))
    rt.op_cache_probe(a0.to(dev), Bc, 1e-5, rb_sh, rb_sc, gm.view, gr.view.view(-1))
    m = gm.view.clone()
    old = m.clone()
    old[: 4 * La] *= 1.25                                              # rows 0..3 moved by a fifth, rows 4 and 5 did not
    gm.view.copy_(old)
    rt.op_cache_probe(a0.to(dev), Bc, 1e-5, rb_sh, rb_sc, gm.view, gr.view.view(-1))
    rel = gr.view.view(-1).cpu()
    assert bool((rel[4:] == 0).all()) and bool(((rel[:4] - 0.2).abs() < 1e-5).all()), rel
    gm.check(), gr.check()


def test_probe_refusals(dev):
    a0 = torch.zeros(50, 258, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="multiple of 4"):
        rt.op_cache_probe(a0, 1, 1e-6, None, None, torch.zeros_like(a0))
    a0 = torch.zeros(50, 4096, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="2048"):
        rt.op_cache_probe(a0, 1, 1e-6, None, None, torch.zeros_like(a0))


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 4096 + 3, 50 * 256, 4096 * 256 * 4 + 1029])
def test_delta_and_apply_bit_for_bit(dev, n, misalign):
    """n not a multiple of the vector width (the scalar tail), more elements than one pass of the grid covers (4096 workgroups x 256 lanes x 4 floats, and
    1029 more: the grid-stride loop), and operands off the 16-byte grid (misalign 1: the scalar path; 0: four guard rows of n floats keep the interior
    on it)."""
    a, b = _rand((n, 1), 11, 3.0), _rand((n, 1), 12, 3.0)
    ga = oc.guarded((n, 1), torch.float32, dev, rows=(4, 4), misalign=misalign)
    gb = oc.guarded((n, 1), torch.float32, dev, rows=(4, 4), misalign=misalign)
    ga.view.copy_(a.to(dev))
    gb.view.copy_(b.to(dev))
    rt.op_cache_delta(ga.view, gb.view)                                  # b <- a - b
    oc.assert_bits_equal(gb.view, a - b, "delta n %d" % n)
    oc.assert_bits_equal(ga.view, a, "delta leaves aN")
    rt.op_cache_apply(ga.view, gb.view)                                  # a <- a + (a - b)
    oc.assert_bits_equal(ga.view, a + (a - b), "apply n %d" % n)
    oc.assert_bits_equal(gb.view, a - b, "apply leaves delta")
    ga.check("delta / apply: audio"), gb.check("delta / apply: delta")
