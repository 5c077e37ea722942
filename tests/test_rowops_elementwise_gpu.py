"""The row, solver and DAC edge kernels of rowops.hip under per-element bounds and guard bands (tests/opcheck.py).

What a sample launches between the GEMM, LayerNorm and attention families: the stand-alone head split, latent_rows, the three
solver steps and the stitch, flow_mix, rows_add_act, add_periodic, gather_rows, cast, rows_periodic_check, dac_in / dac_out,
rows_to_planes.  Every output is launched into a NaN-filled interior between guard rows (pad columns where the layout has a
pitch: the transposed V), every element is held against a bound derived from the arithmetic - or compared bit for bit where the
kernel only moves data or performs one correctly rounded operation - and the guards are compared bit for bit.  The shapes are the
smallest that reach the edge in question (a ragged 32-token tile, a 64-sample seam, the 4096-workgroup cap of grid1d), not the
workload's.  Each family's largest err / bound goes to the parity records.
"""
import pytest
import torch

import opcheck as oc
from conftest import record_parity
from foley_amd.host import long_form, runtime as rt, tables
from step_harness import ALL3, DTS, GUIDANCE, SOLVER_ITERS, STEP_SHAPES, StepState, _rand

pytestmark = pytest.mark.gpu

CAP = 4096 * 256                 # work items one grid1d launch covers without striding (rowops.hip)
_WORST = {}


def _rec(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), float(ratio))
    record_parity(f"elementwise.rowops.{family}", err_over_bound=_WORST[family])


# ----------------------------------------------------------------------------- stand-alone head split
QKV_L, QKV_NK, QKV_H, QKV_OFF = [1, 16, 17, 33, 77], [1, 2, 3], [1, 3], [0, 5]
QKV_EPS = [1e-6, 1.1920928955078125e-07]


def _qkv_clips(L):
    return 1 + L % 3          # 2, 2, 3, 1, 3 clips: M H nQ then leaves 1, 2 and 3 items in a last wave (asserted below)


def _qkv_variant(L, nK, H, off):
    """(rotate, gains, eps, wide pitch) - rotated over the matrix so that each value meets each L and each nK."""
    i = (QKV_L.index(L) + nK + H + (1 if off else 0)) % 4
    return {"pos": i != 1, "gain": i != 2, "eps": QKV_EPS[i % 2], "wide": i == 3}


def test_qkv_cases_cover_the_ragged_waves_and_every_variant():
    """Role (1) of qkv_split_kernel gives a wave four items and a workgroup sixteen: the matrix must leave 1, 2 and 3 items in a
    last wave and fewer than 16 in a last workgroup; every (rotate, gain, eps, pitch) variant must occur at every L and nK."""
    left_wave, left_wg = set(), set()
    for L in QKV_L:
        for nK in QKV_NK:
            seen = set()
            for H in QKV_H:
                for off in QKV_OFF:
                    v = _qkv_variant(L, nK, H, off)
                    seen.add((v["pos"], v["gain"], v["eps"], v["wide"]))
                    for vtrans in (False, True):
                        items = _qkv_clips(L) * L * H * (nK - (1 if vtrans else 0))
                        left_wave.add(items % 4)
                        left_wg.add(items % 16)
            assert len(seen) == 4, (L, nK, seen)
    assert {1, 2, 3} <= left_wave and any(0 < r < 16 for r in left_wg)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("off", QKV_OFF)
@pytest.mark.parametrize("H", QKV_H)
@pytest.mark.parametrize("nK", QKV_NK)
@pytest.mark.parametrize("L", QKV_L)
def test_qkv_split_elementwise(dev, L, nK, H, off, dt):
    """Both V layouts of one point of the matrix.  nK = 2 is the text K / V call: gain (k, none), no rotation of V.  Token rows
    before tok_off and after tok_off + L, and the V^T columns outside the tokens, must keep the bits they held."""
    dtype = DTS[dt]
    B = _qkv_clips(L)
    var = _qkv_variant(L, nK, H, off)
    S = off + L + 3
    M = B * L
    qkv = _rand((M, nK * H * 128), 1000 + L + nK)
    y = qkv.view(B, L, nK, H, 128)
    gains = [1 + 0.1 * _rand((128,), 1100 + j) for j in range(2)]
    pos = (2 * torch.randperm(L, generator=torch.Generator().manual_seed(L))).to(torch.int32)      # non-monotonic
    cos, sin = tables.rope_table(2 * L + 1)
    qd, cd, sd = qkv.to(dev), cos.to(dev), sin.to(dev)
    worst = 0.0
    for vtrans in (False, True):
        nQ = nK - 1 if (vtrans or nK >= 2) else nK             # operands normalised / rotated; the last of nK >= 2 is V
        has_v = nK >= 2 or vtrans
        pitch = (S + 31) // 32 * 32 + (32 if var["wide"] else 0)
        gl = [(gains[j] if (var["gain"] or nK == 2) else None) for j in range(nQ)] + ([None] if has_v else [])
        pl = [(pos if var["pos"] else None) for j in range(nQ)] + ([None] if has_v else [])
        guards = []
        for j in range(nK):
            is_vt = vtrans and j == nK - 1
            g = oc.guarded((B, H, 128, pitch) if is_vt else (B, H, S, 128), dtype, dev, rows=(1, 1), fill=3.0)
            (g.view[..., off:off + L] if is_vt else g.view[:, :, off:off + L]).fill_(float("nan"))
            guards.append(g)
        dsts = [g.view for g in guards]
        rt.op_qkv_split(qd, L, H, [t.to(dev) if t is not None else None for t in gl], [t.to(dev) if t is not None else None for t in pl],
                        dsts, S, off, var["eps"], cd, sd, vt_pitch=pitch if vtrans else 0)
        what = f"qkv_split L{L} nK{nK} H{H} off{off} {dt} vtrans {vtrans} {var}"
        keep = torch.full((1,), 3.0, dtype=dtype)
        for j in range(nK):
            got = dsts[j].cpu()
            yj = y[:, :, j].reshape(M, H, 128)
            if vtrans and j == nK - 1:
                want = yj.view(B, L, H, 128).permute(0, 2, 3, 1).to(dtype)
                oc.assert_bits_equal(got[..., off:off + L], want, what + " V^T")
                out = torch.cat((got[..., :off], got[..., off + L:]), -1)
                oc.assert_bits_equal(out, keep.expand_as(out), what + " V^T columns outside the tokens")
                continue
            out = torch.cat((got[:, :, :off], got[:, :, off + L:]), 2)
            oc.assert_bits_equal(out, keep.expand_as(out), what + f" operand {j}: rows outside the tokens")
            if gl[j] is None and pl[j] is None:                  # V (or a bare copy): bit for bit
                oc.assert_bits_equal(got[:, :, off:off + L], yj.view(B, L, H, 128).transpose(1, 2).to(dtype), what + f" operand {j} copy")
                continue
            c, s = (cos[pos.long()].repeat(B, 1), sin[pos.long()].repeat(B, 1)) if pl[j] is not None else (None, None)
            ref, bound = oc.qkv_head_ref_and_bound(yj, gl[j], c, s, var["eps"], dtype)
            bound.e = bound.e.view(B, L, H, 128).transpose(1, 2)
            worst = max(worst, oc.assert_elementwise(got[:, :, off:off + L], ref.view(B, L, H, 128).transpose(1, 2), bound, what + f" operand {j}"))
        for g in guards:
            g.check(what)
    _rec(f"qkv_split.{dt}", worst)


# ----------------------------------------------------------------------------- latent rows
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [1, 2])
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_latent_rows_bits(dev, clips, C, L, ncfg, dt):
    x = _rand((clips, C, L), 60)
    g = oc.guarded((ncfg * clips * L, C), DTS[dt], dev, rows=(2, 3))
    rt.op_latent_rows(x.to(dev), ncfg, g.view)
    oc.assert_bits_equal(g.view, oc.rows_of(x, ncfg, DTS[dt]), f"latent_rows {clips}x{C}x{L} ncfg {ncfg} {dt}")
    g.check("latent_rows")


# ----------------------------------------------------------------------------- solver steps: one bound per iteration
def _step_ref(pred, st, coef_row):
    """The fp64 step from the state `st` holds now, two halves (or one) under the scalar GUIDANCE."""
    x, xs, da, _ = st.snapshot()
    return oc.solver_step_ref_and_bounds(pred, x, xs, da, coef_row, st.ncfg, GUIDANCE)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ncfg", [1, 2])
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_solver_step_elementwise(dev, clips, C, L, solver, ncfg, dt):
    """euler with ncfg 1 runs without x_saved / d_acc (null pointers); the multi-stage tables start from a NON-zero x_saved / d_acc so
    that a row which must reset or overwrite them is seen to do so."""
    n = SOLVER_ITERS[solver]
    coef = tables.solver_table(tables.sigma_grid(n), solver, n)
    st = StepState(dev, clips, C, L, ncfg, DTS[dt], 70, saved=not (solver == "euler" and ncfg == 1))
    cd = coef.to(dev)
    worst = 0.0
    for it in range(n):
        pred = _rand((ncfg * clips * L, C), 71 + it)
        r = _step_ref(pred, st, coef[it])
        st.step(pred, cd)
        worst = max(worst, st.check(it, r, *r["x"], f"solver_step {solver} {clips}x{C}x{L} ncfg {ncfg} {dt} it {it}"))
    _rec(f"solver_step.{solver}", worst)


def test_solver_step_without_rows_out(dev):
    clips, C, L, ncfg = 2, 96, 31, 2
    coef = tables.solver_table(tables.sigma_grid(3), "heun-2", 3)
    st = StepState(dev, clips, C, L, ncfg, torch.float32, 80, rows=False)
    for it in range(3):
        pred = _rand((ncfg * clips * L, C), 81 + it)
        r = _step_ref(pred, st, coef[it])
        st.step(pred, coef.to(dev))
        _rec("solver_step.heun-2", st.check(it, r, *r["x"], f"solver_step without rows_out it {it}"))


EDIT_VARIANTS = [(1, 0, "none", 2), (1, 1, "binary", 1), ("clips", "clips", "fractional", 2), ("clips", "clips", "binary", 1), ("clips", 1, "fractional", 2)]


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("clips,C,L", STEP_SHAPES)
def test_solver_step_edit_elementwise(dev, clips, C, L, solver, dt):
    """x0_clips / mask_clips in {1, clips}, masks absent, binary and fractional (with exact 0 and 1 entries), both CFG counts."""
    n = SOLVER_ITERS[solver]
    coef = tables.edit_solver_table(tables.sigma_grid(n), solver, n)
    cd = coef.to(dev)
    worst = 0.0
    for vi, (x0c, mc, kind, ncfg) in enumerate(EDIT_VARIANTS):
        x0c, mc = (clips if x0c == "clips" else x0c), (clips if mc == "clips" else mc)
        gen = torch.Generator().manual_seed(90 + vi)
        x0, noise = _rand((x0c, C, L), 91 + vi, 0.7), _rand((clips, C, L), 92 + vi)
        mask = None if kind == "none" else torch.rand(mc, L, generator=gen)
        if kind == "binary":
            mask = (mask > 0.5).float()
        elif kind == "fractional":
            mask[:, : L // 3] = 0.0
            mask[:, L // 3: L // 2] = 1.0
        st = StepState(dev, clips, C, L, ncfg, DTS[dt], 93 + vi, saved=not (solver == "euler" and vi % 2 == 1))
        edit = (x0.to(dev), noise.to(dev), (mask.to(dev) if mask is not None else None))
        for it in range(n):
            pred = _rand((ncfg * clips * L, C), 94 + it)
            r = _step_ref(pred, st, coef[it])
            ref, bound = r["x"]
            if r["flags"] & oc.STEP_BLEND:
                ref, bound = oc.edit_blend_ref_and_bound(ref, bound.e, r["s_next"], x0, noise, mask)
            st.step(pred, cd, edit=edit)
            worst = max(worst, st.check(it, r, ref, bound, f"solver_step_edit {solver} {clips}x{C}x{L} {dt} variant {vi} it {it}"))
    _rec(f"solver_step_edit.{solver}", worst)


def _win_plans(L):
    """Starts of 1, 2 and 3 windows of L frames: Ltot = L; Ltot = n_win L (disjoint); a window edge inside a 32-frame tile; one on a
    tile boundary (L >= 32); a frame covered by three windows (L >= 3)."""
    plans = [[0], [0, L], [0, max(1, 2 * L // 5)]]
    if L >= 32:
        plans.append([0, 32])
    if L >= 3:
        plans.append([0, L // 3, 2 * L // 3])
    else:
        plans.append([0, L, 2 * L])
    return plans


def test_window_plans_cover_what_they_claim():
    for _, _, L in STEP_SHAPES:
        plans = _win_plans(L)
        assert {len(p) for p in plans} == {1, 2, 3}
        assert any(p[-1] + L == len(p) * L and len(p) > 1 for p in plans) and [0] in plans
        if L >= 3:
            assert any(int(long_form.WindowPlan.from_frames(p, L).coverage().max()) == 3 for p in plans)
    assert [0, 32] in _win_plans(50) and any(p[1] % 32 for p in _win_plans(50) if len(p) == 2)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("solver", list(SOLVER_ITERS))
@pytest.mark.parametrize("_clips,C,L", STEP_SHAPES)
def test_solver_step_windows_elementwise(dev, _clips, C, L, solver, dt):
    """Two variations of every window plan of _win_plans.  Rows without the blend flag leave every window its own update; blend rows
    replace every frame in all its covering windows by the weighted mean (window order) - singly covered frames keep their bits."""
    n = SOLVER_ITERS[solver]
    coef = tables.edit_solver_table(tables.sigma_grid(n), solver, n)
    cd = coef.to(dev)
    worst = 0.0
    for pi, starts in enumerate(_win_plans(L)):
        plan = long_form.WindowPlan.from_frames(starts, L)
        n_win, ncfg = plan.n_win, 2 - pi % 2
        clips = 2 * n_win
        st = StepState(dev, clips, C, L, ncfg, DTS[dt], 120 + pi, saved=not (solver == "euler" and pi % 2 == 1))
        sd, wd = torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
        for it in range(n):
            pred = _rand((ncfg * clips * L, C), 121 + it)
            r = _step_ref(pred, st, coef[it])
            ref, bound = r["x"]
            blend = bool(r["flags"] & oc.STEP_BLEND)
            if blend:
                ref, e, _, _, _ = oc.windows_mean_ref_and_bound(ref, bound.e, n_win, starts, plan.weights)
                bound = oc.Bound(e)
            st.step(pred, cd, windows=(sd, wd, plan.Ltot))
            what = f"solver_step_windows {solver} C{C} L{L} starts {starts} {dt} it {it}"
            worst = max(worst, st.check(it, r, ref, bound, what))
            if blend and n_win > 1:      # the windows that cover a frame agree on it bit for bit
                xg = st.gx.view.cpu().view(2, n_win, C, L)
                for k in range(n_win):
                    for k2 in range(k + 1, n_win):
                        lo, hi = starts[k2], min(starts[k] + L, starts[k2] + L)
                        if lo < hi:
                            oc.assert_bits_equal(xg[:, k, :, lo - starts[k]:hi - starts[k]], xg[:, k2, :, :hi - starts[k2]], what + f" windows {k} / {k2} agree")
    _rec(f"solver_step_windows.{solver}", worst)


STITCH = {255: (100, [0, 60, 90, 155]), 256: (100, [0, 60, 90, 156]), 257: (100, [0, 60, 90, 157]), 600: (250, [0, 100, 200, 350])}


@pytest.mark.parametrize("Ltot", list(STITCH))
def test_windows_stitch_elementwise(dev, Ltot):
    """Ltot around the 256-frame workgroup and past two of them; frames in one, two and three windows.  Where the covering windows
    hold equal bits the value must come out as it is."""
    L, starts = STITCH[Ltot]
    plan = long_form.WindowPlan.from_frames(starts, L)
    assert plan.Ltot == Ltot and int(plan.coverage().max()) == 3
    V, C = 2, 5
    x = _rand((V * plan.n_win, C, L), 130)
    sd, wd = torch.tensor(starts, dtype=torch.int32, device=dev), plan.weights.to(dev)
    lib = rt.load_library()

    def stitch(xs):
        g = oc.guarded((V, C, Ltot), torch.float32, dev, rows=(1, 1))
        rt._check(lib, lib.foley_op_windows_stitch(rt._ptr(xs), V * plan.n_win, plan.n_win, C, L, Ltot, rt._ptr(sd), rt._ptr(wd), rt._ptr(g.view),
                                                   rt._stream()), "foley_op_windows_stitch")
        g.check(f"windows_stitch Ltot {Ltot}")
        return g.view.cpu()
    _, _, G, e_G, cov = oc.windows_mean_ref_and_bound(x.double(), None, plan.n_win, starts, plan.weights)
    got = stitch(x.to(dev))
    _rec("windows_stitch", oc.assert_elementwise(got, G, e_G, f"windows_stitch Ltot {Ltot}"))
    for k, s in enumerate(starts):                  # singly covered frames are copies
        m = cov[s:s + L] == 1
        oc.assert_bits_equal(got[:, :, s:s + L][..., m], x.view(V, plan.n_win, C, L)[:, k][..., m], f"windows_stitch Ltot {Ltot}: single coverage")
    Gx = _rand((V, C, Ltot), 131)
    xa = torch.stack([Gx[v, :, s:s + L] for v in range(V) for s in starts]).contiguous()
    oc.assert_bits_equal(stitch(xa.to(dev)), Gx, f"windows_stitch Ltot {Ltot}: windows that agree")


# ----------------------------------------------------------------------------- grid-stride tails (and one shape far below the cap)
@pytest.mark.parametrize("x0_clips", [1, 3])
@pytest.mark.parametrize("shape", [(3, 128, 2800), (3, 128, 77)], ids=["past_cap", "small"])
def test_flow_mix_elementwise(dev, shape, x0_clips):
    """[3, 128, 2800] is 1 075 200 elements: 26 624 past what 4096 workgroups of 256 reach without striding.  sigma = 1 returns the
    noise bits, sigma = 0 the x0 bits."""
    noise, x0 = _rand(shape, 140), _rand((x0_clips,) + shape[1:], 141, 0.7)
    assert (noise.numel() > CAP) == (shape[2] == 2800)
    nd, xd = noise.to(dev), x0.to(dev)
    for s in (0.73, 1.0, 0.0):
        g = oc.guarded(shape, torch.float32, dev, rows=(1, 1))
        rt.op_flow_mix(nd, xd, s, out=g.view)
        what = f"flow_mix {shape} x0_clips {x0_clips} sigma {s}"
        _rec("flow_mix", oc.assert_elementwise(g.view, *oc.flow_mix_ref_and_bound(noise, x0, s), what))
        if s == 1.0:
            oc.assert_bits_equal(g.view, noise, what)
        if s == 0.0:
            oc.assert_bits_equal(g.view, x0.expand(shape).contiguous(), what)
        g.check(what)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("with_a,with_v", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("R,D", [(700, 1536), (9, 1536)], ids=["past_cap", "small"])
def test_rows_add_act_elementwise(dev, R, D, with_a, with_v, dt):
    dtype = DTS[dt]
    assert (R * D > CAP) == (R == 700)
    a, v = (_rand((R, D), 150, 3.0) if with_a else None), (_rand((D,), 151) if with_v else None)
    ad, vd = (a.to(dev) if with_a else None), (v.to(dev) if with_v else None)
    for silu in (False, True):
        g = oc.guarded((R, D), dtype, dev, rows=(2, 3))
        rt.op_rows_add_act(ad, vd, g.view, silu)
        what = f"rows_add_act [{R}, {D}] a {with_a} v {with_v} silu {silu} {dt}"
        ref, bound = oc.rows_add_act_ref_and_bound(a, v, silu, dtype, dev)
        if bound is None or not (with_a or with_v):      # one correctly rounded addition (or act(0) = 0): bit for bit
            want = oc.sum32_cast(a, v, dtype).expand(R, D).contiguous() if (with_a or with_v) else torch.zeros(R, D, dtype=dtype)
            oc.assert_bits_equal(g.view, want, what)
        else:
            _rec(f"rows_add_act.{dt}", oc.assert_elementwise(g.view, ref.expand(R, D), bound, what))
        g.check(what)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("R", [1400, 13], ids=["past_cap", "small"])
def test_add_periodic_bits(dev, R, dt):
    D, period = 768, 8
    assert (R * D > CAP) == (R == 1400)
    x, pos = _rand((R, D), 160), _rand((period, D), 161)
    g = oc.guarded((R, D), DTS[dt], dev, rows=(2, 3))
    rt.op_add_periodic(x.to(dev), pos.to(dev), g.view)
    want = (x + pos.repeat((R + period - 1) // period, 1)[:R]).to(DTS[dt])
    oc.assert_bits_equal(g.view, want, f"add_periodic [{R}, {D}] {dt}")
    g.check("add_periodic")


@pytest.mark.parametrize("groups,n_idx,src_rows,D", [(3, 700, 900, 500), (2, 5, 9, 64)], ids=["past_cap", "small"])
def test_gather_rows_bits(dev, groups, n_idx, src_rows, D):
    """Repeated and descending indices, several groups, src_rows != n_idx."""
    assert (groups * n_idx * D > CAP) == (n_idx == 700)
    src = _rand((groups * src_rows, D), 170)
    idx = torch.flip(torch.arange(n_idx) // 2, (0,))
    idx[::7] = src_rows - 1 - (idx[::7] % 3)
    idx = idx.to(torch.int32)
    g = oc.guarded((groups * n_idx, D), torch.float32, dev, rows=(2, 3))
    rt.op_gather_rows(src.to(dev), idx.to(dev), groups, g.view)
    want = src.view(groups, src_rows, D)[:, idx.long()].reshape(groups * n_idx, D)
    oc.assert_bits_equal(g.view, want, f"gather_rows groups {groups} n_idx {n_idx} D {D}")
    g.check("gather_rows")


CAST_PAIRS = [("f32", "bf16"), ("bf16", "f32"), ("f32", "f16"), ("f16", "f32"), ("f32", "f32")]


@pytest.mark.parametrize("n", [CAP + 77, 77], ids=["past_cap", "small"])
@pytest.mark.parametrize("sd,dd", CAST_PAIRS)
def test_cast_bits(dev, sd, dd, n):
    """Against torch's CPU cast: ties, overflow to infinity, subnormals, signed zeros and infinities bit for bit; an expected NaN
    only has to be a NaN."""
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65504.0, 65520.0, 65519.9, 1e-8, 6e-8, -2.9e-8, 1e-40,
                            3.3895e38, 1.00390625, 1.01171875, 1.0009765625, 1.00048828125, -1.00146484375])
    src = torch.cat((special, _rand((n - special.numel(),), 180) * torch.logspace(-9, 5, n - special.numel()))).to(DTS[sd])
    src[-1] = float("nan")
    g = oc.guarded((n, 1), DTS[dd], dev, rows=(2, 3))
    rt.op_cast(src.to(dev), g.view)
    oc.assert_bits_equal(g.view.view(1, n), src.to(DTS[dd]).view(1, n), f"cast {sd} -> {dd} n {n}", nan_ok=True)
    g.check("cast")


def test_cast_refuses_unsupported_pairs(dev):
    for sd, dd in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                   (torch.int32, torch.float32), (torch.float32, torch.int32)):
        src, dst = torch.zeros(8, dtype=sd, device=dev), torch.full((8,), 3, dtype=dd, device=dev)
        with pytest.raises(rt.FoleyRuntimeError, match="unsupported dtype pair"):
            rt.op_cast(src, dst)
        assert bool((dst == 3).all())


@pytest.mark.parametrize("T", [66000, 50], ids=["past_cap", "small"])
def test_rows_to_planes_bits(dev, T):
    B, C = (1, 16) if T == 66000 else (3, 12)
    assert (B * T * C > CAP) == (T == 66000)
    rows = _rand((B * T, C), 190)
    g = oc.guarded((B, C, T), torch.float32, dev, rows=(1, 1))
    rt.op_rows_to_planes(rows.to(dev), B, g.view)
    oc.assert_bits_equal(g.view, rows.view(B, T, C).transpose(1, 2).contiguous(), f"rows_to_planes T {T}")
    g.check("rows_to_planes")


# ----------------------------------------------------------------------------- DAC edges
@pytest.mark.parametrize("C", [64, 96])
@pytest.mark.parametrize("T", [1, 3, 63, 64, 65, 300])
def test_dac_out_elementwise(dev, T, C):
    """Every output sample of both clips: the zero halo at the two ends of each clip, the halo that crosses a 64-sample workgroup
    seam, and the boundary between the clips of the batch (a halo that read the neighbouring clip would show at t < 3 and t >= T - 3)."""
    B = 2
    s, w, b = _rand((B, T, C), 200), _rand((7 * C,), 201, 0.1), _rand((1,), 202, 0.1)
    g = oc.guarded((B, T), torch.float32, dev, rows=(2, 3))
    rt.op_dac_out(s.to(dev), w.to(dev), b.to(dev), g.view)
    ref, bound, a_act = oc.dac_out_ref_and_bound(s, w, b, dev)
    r = oc.assert_elementwise(g.view, ref, bound, f"dac_out T{T} C{C}")
    g.check("dac_out")
    _rec("dac_out", r)
    record_parity(f"elementwise.rowops.dac_out.a_act.T{T}.C{C}", a_act=a_act)


@pytest.mark.parametrize("B,T", [(2, 1), (2, 3), (2, 63), (2, 64), (2, 65), (2, 300), (1, 66000)])
def test_dac_in_elementwise(dev, B, T):
    """alpha includes small values (1e-3 ...), where the snake's 1 / (alpha + 1e-9) factor is large.  [1, 66 000] is 1 056 000 work
    items (four channels each): past the 4096-workgroup cap."""
    C = 64
    assert (B * T * C // 4 > CAP) == (T == 66000)
    x, w, b = _rand((B, T), 210), _rand((7, C), 211, 0.4), _rand((C,), 212, 0.1)
    alpha = torch.cat((torch.tensor([1e-3, 1e-2, 0.05, 0.3]), 1 + 0.2 * _rand((C - 4,), 213).abs()))
    g0 = oc.guarded((B * T, C), torch.float32, dev, rows=(2, 3))
    g1 = oc.guarded((B * T, C), torch.float32, dev, rows=(2, 3))
    rt.op_dac_in(x.to(dev), w.to(dev), b.to(dev), alpha.to(dev), g0.view, g1.view)
    y64, s64, b0, b1, a_act = oc.dac_in_ref_and_bounds(x, w, b, alpha, dev)
    r0 = oc.assert_elementwise(g0.view, y64, b0, f"dac_in out0 B{B} T{T}")
    r1 = oc.assert_elementwise(g1.view, s64, b1, f"dac_in out1 (snake) B{B} T{T}")
    g0.check("dac_in out0")
    g1.check("dac_in out1")
    _rec("dac_in", max(r0, r1))


# ----------------------------------------------------------------------------- rows_periodic_check
def _periodic(groups, rows, D, seed):
    base = _rand((groups, 8, D), seed)
    base[0, 3, 5] = float("nan")              # equal NaN bit patterns count as periodic
    base[-1, 0, 7] = 0.0
    return base.repeat(1, (rows + 7) // 8, 1)[:, :rows].contiguous()


def _flags(dev, x, init=None):
    groups = x.shape[0]
    g = oc.guarded((groups, 1), torch.int32, dev, rows=(1, 1), fill=0)
    if init is not None:
        g.view.copy_(init.view(groups, 1).to(dev))
    rt.op_rows_periodic_check(x, 8, g.view.view(groups))
    g.check("rows_periodic_check flags")
    return g.view.view(groups).cpu()


@pytest.mark.parametrize("rows", [8, 9, 16, 358])
@pytest.mark.parametrize("groups", [1, 2, 32])
def test_rows_periodic_check(dev, groups, rows):
    """The compare is on BIT PATTERNS: + 0.0 against - 0.0 counts as different, equal NaN patterns as periodic.  Flags are OR-ed into
    what the buffer held.  rows = 8 (= the period): nothing is launched and the flags stay.  One differing bit in one group sets
    exactly that group's flag - at the first compared element, at the last, each group in turn; with 358 rows a group holds 537 600
    compared elements, so every group from the third on lies past index 1 048 576."""
    D = 1536
    x = _periodic(groups, rows, D, 220 + groups).to(dev)
    init = (torch.arange(groups, dtype=torch.int32) % 3) * 2                       # 0, 2, 4: bit 0 clear
    assert _flags(dev, x, init).tolist() == init.tolist(), "all periodic: every flag as it was"
    if rows <= 16:
        assert oc.periodic_flags(x, 8).tolist() == [0] * groups
    xi = x.view(torch.int32)
    spots = [(8, 0), (rows - 1, D - 1)] if rows > 8 else [(7, D - 1)]
    for g in range(groups):
        for (r, c) in spots:
            xi[g, r, c] ^= 1
            want = init.clone()
            if rows > 8:
                want[g] |= 1
            assert _flags(dev, x, init).tolist() == want.tolist(), (groups, rows, g, r, c)
            xi[g, r, c] ^= 1
    if rows > 8:
        if groups == 32 and rows == 358:
            assert 2 * (rows - 8) * D > CAP                                           # group 2 onwards: compared elements past the cap
        x[groups - 1, 8, 7] = -0.0                                                    # row 0 holds + 0.0 there
        want = [0] * groups
        want[groups - 1] = 1
        assert _flags(dev, x).tolist() == want, "+ 0.0 against - 0.0 differs"
        if rows <= 16:
            assert oc.periodic_flags(x, 8).tolist() == want


def test_rows_periodic_check_refuses_33_groups(dev):
    x = _periodic(33, 16, 64, 230).to(dev)
    flags = torch.zeros(33, dtype=torch.int32, device=dev)
    with pytest.raises(rt.FoleyRuntimeError, match="at most 32 groups"):
        rt.op_rows_periodic_check(x, 8, flags)
    assert flags.tolist() == [0] * 33
