"""Host-built schedule / index / trig tables for one sampling run (tiny, built once with torch CPU).

These are the step-invariant lookups the reference rebuilds inside its hot loop:
  * flow-match sigma grid + model timesteps (scheduling_flow_match_discrete.py:131-170),
  * per-iteration solver coefficients - the `step()` state machine for euler / heun-2 /
    midpoint-2 / kutta-4 (:262-373) flattened into a table the device kernel indexes,
  * sinusoidal timestep features (embed_layers.py:76-101),
  * RoPE cos/sin table (posemb_layers.py:117-172; one row per position, one column per pair),
  * token -> RoPE position maps incl. the interleaved audio/visual scheme (hifi_foley.py:35-60,
    236-251), and the nearest-exact up-sampling index of the sync features (hifi_foley.py:761).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

SOLVERS = ("euler", "heun-2", "midpoint-2", "kutta-4")
STEP_SAVE_X, STEP_USE_SAVED, STEP_ACC_RESET = 1, 2, 4
STEP_BLEND = 8          # edit runs only (foley_set_edit): blend towards the source after this row, sigma_{k+1} in column 5
STEP_HIST = 16          # multistep runs only (foley_set_multistep): the row adds history terms, weights in columns 6 and 7
SOLVER_STAGES = {"euler": 1, "heun-2": 2, "midpoint-2": 2, "kutta-4": 4}
MULTISTEP_ORDERS = (2, 3)


def sigma_grid(steps: int, shift: float = 1.0) -> torch.Tensor:
    s = torch.linspace(1, 0, steps + 1)
    if shift != 1.0:
        s = (shift * s) / (1 + (shift - 1) * s)
    return s


def model_timesteps(sigmas: torch.Tensor) -> torch.Tensor:
    return (sigmas[:-1] * 1000).to(torch.float32)


def multistep_weights(sigmas: torch.Tensor, n: int, order: int):
    """Variable-step Adams-Bashforth weights (c_0, c_1, c_2) of the step sigma_n -> sigma_{n+1} for the velocities v_n, v_{n-1},
    v_{n-2}: the integrals over [sigma_n, sigma_{n+1}] of the Lagrange basis polynomials on the nodes sigma_n, sigma_{n-1}
    (, sigma_{n-2}), divided by dt = sigma_{n+1} - sigma_n.  fp64 from the fp32 grid's values; the caller rounds to fp32 once.
    Order 1 is Euler, (1, 0, 0)."""
    if order <= 1:
        return 1.0, 0.0, 0.0
    s = [float(sigmas[n - j].double()) for j in range(order)]
    h = float(sigmas[n + 1].double()) - s[0]
    if order == 2:                                  # closed form: r = dt / (sigma_n - sigma_{n-1})
        r = h / (s[0] - s[1])
        return 1.0 + r / 2, -r / 2, 0.0
    a = [t - s[0] for t in s]                       # nodes relative to sigma_n (a[0] = 0); u runs over [0, h]
    out = []
    for j in range(3):
        p, q = (a[k] for k in range(3) if k != j)   # basis j = (u - p)(u - q) / ((a_j - p)(a_j - q))
        out.append((h * h / 3 - (p + q) * h / 2 + p * q) / ((a[j] - p) * (a[j] - q)))
    return tuple(out)


def solver_table(sigmas: torch.Tensor, solver: str, n_iter: int, multistep_order: Optional[int] = None,
                 start: int = 0) -> torch.Tensor:
    """[n_iter, 8] rows {w_new, w_acc, dt, w_store, flags, 0, c_1, c_2}.

    Per iteration the device computes  deriv = w_new*v + w_acc*acc ; x' = base + deriv*dt ;
    acc' = (reset ? 0 : acc) + w_store*v, with base = saved sample or current sample.
    Like the reference, every loop iteration is one solver *stage* and the sigma index only
    advances after the last stage of a step.

    multistep_order (2 or 3, euler only): Adams-Bashforth rows - c_0 in column 0, c_1 and c_2 (the weights of v_{n-1} and v_{n-2},
    multistep_weights) in columns 6 and 7, STEP_HIST on every row with a non-zero history weight; the device continues
    deriv = fma(c_1, v_{n-1}, deriv), fma(c_2, v_{n-2}, deriv).  Warm-up takes the order the history allows: row `start` (where a
    run that takes the suffix [start:] begins, without history) is the Euler row, the row after it carries the order-2 weights.
    Rows before `start` are those of a run from row 0.  None gives the one-step tables, value for value.
    """
    if solver not in SOLVERS:
        raise ValueError(f"Solver {solver} not supported. Supported solvers: {list(SOLVERS)}")
    if multistep_order is not None:
        if solver != "euler":
            raise ValueError(f"multistep_order needs the euler solver (one model call per sigma step), got {solver}: the "
                             "multi-stage solvers do not combine with a velocity history")
        if multistep_order not in MULTISTEP_ORDERS or isinstance(multistep_order, bool) or int(multistep_order) != multistep_order:
            raise ValueError(f"multistep_order must be one of {list(MULTISTEP_ORDERS)}, got {multistep_order}")
        if not 0 <= int(start) <= n_iter:
            raise ValueError(f"start must lie in [0, n_iter], got {start}")
    rows = torch.zeros(n_iter, 8, dtype=torch.float32)
    idx, stage, dt = 0, 0, None
    for i in range(n_iter):
        if stage == 0:
            dt = sigmas[idx + 1] - sigmas[idx]          # fp32, like the reference
        if solver == "euler":
            rows[i, :5] = torch.tensor([1.0, 0.0, float(dt), 0.0, 0.0])
            if multistep_order is not None:
                have = i - (int(start) if i >= int(start) else 0)      # velocities of this run before row i
                c = torch.tensor(multistep_weights(sigmas, idx, min(int(multistep_order), have + 1)), dtype=torch.float64).float()
                rows[i, 0], rows[i, 6], rows[i, 7] = c[0], c[1], c[2]
                if c[1] != 0 or c[2] != 0:
                    rows[i, 4] = float(STEP_HIST)
            idx += 1
            continue
        if solver in ("heun-2", "midpoint-2"):
            heun = solver == "heun-2"
            if stage == 0:
                rows[i, :5] = torch.tensor([1.0, 0.0, float(dt if heun else dt / 2), 0.5 if heun else 0.0,
                                            float(STEP_SAVE_X | STEP_ACC_RESET)])
                stage = 1
            else:
                rows[i, :5] = torch.tensor([0.5 if heun else 1.0, 1.0 if heun else 0.0, float(dt), 0.0,
                                            float(STEP_USE_SAVED)])
                stage, idx = 0, idx + 1
            continue
        # kutta-4
        if stage == 0:
            rows[i, :5] = torch.tensor([1.0, 0.0, float(dt / 2), 1.0 / 6.0, float(STEP_SAVE_X | STEP_ACC_RESET)])
        elif stage == 1:
            rows[i, :5] = torch.tensor([1.0, 0.0, float(dt / 2), 1.0 / 3.0, 0.0])
        elif stage == 2:
            rows[i, :5] = torch.tensor([1.0, 0.0, float(dt), 1.0 / 3.0, 0.0])
        else:
            rows[i, :5] = torch.tensor([1.0 / 6.0, 1.0, float(dt), 0.0, float(STEP_USE_SAVED)])
        stage = (stage + 1) % 4
        if stage == 0:
            idx += 1
    return rows


def guidance_schedule(n_iter: int, g_video: float, g_text: float, interval=None) -> torch.Tensor:
    """[n_iter, 2] fp32 rows {g_video, g_text} of the loop iterations (foley_set_guidance; a two-half run reads column 0).
    interval = (start, end), 0 <= start < end <= 1: the scales hold on the iterations with start <= i / n_iter < end, the others
    carry (1, 1) - the conditional prediction alone.  i counts loop iterations, so a multi-stage solver counts its stages, as
    the coefficient rows do; an edit run takes the rows [i0:] of the plain run's table."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError(f"n_iter must be >= 1, got {n_iter}")
    rows = torch.empty(n_iter, 2, dtype=torch.float32)
    rows[:, 0], rows[:, 1] = float(g_video), float(g_text)
    if interval is not None:
        start, end = (float(t) for t in interval)
        if not 0.0 <= start < end <= 1.0:
            raise ValueError(f"guidance interval must satisfy 0 <= start < end <= 1, got ({start}, {end})")
        for i in range(n_iter):
            if not start <= i / n_iter < end:
                rows[i] = 1.0
    return rows


PROJECTION_MODES = {"apg": 1, "cfg_zero_star": 2}      # FOLEY_GUIDANCE_APG, FOLEY_GUIDANCE_ZERO_STAR


def projection_rows(n_iter: int, mode, eta: float = 0.0, momentum: float = -0.5, norm_threshold: float = 0.0, zero_init: int = 0,
                    start: int = 0) -> torch.Tensor:
    """[n_iter - start, 4] fp32 rows {eta, beta, R, live} of the loop iterations [start, n_iter) (foley_set_projected_guidance),
    computed in fp64 and rounded once.  mode "apg" (or 1): eta scales the part of the guidance difference parallel to the
    conditional prediction, beta = `momentum` is the weight of the running average on every row but the first (row `start` has
    beta = 0: the run has no average yet, and the plane is not read), R = `norm_threshold` clips the norm of the averaged
    difference (0: no clip).  mode "cfg_zero_star" (or 2): eta, beta and R are 0.  live = 0 on the rows i < zero_init of the full
    run (a zero velocity), 1 elsewhere.  i counts loop iterations, so a multi-stage solver counts its stages, as every other table
    does; an edit run passes start = i0 and gets the rows [i0, n_iter)."""
    n_iter, start, zero_init = int(n_iter), int(start), int(zero_init)
    m = PROJECTION_MODES.get(mode, mode)
    if m not in PROJECTION_MODES.values():
        raise ValueError(f"projection mode must be one of {list(PROJECTION_MODES)}, got {mode!r}")
    if n_iter < 1 or not 0 <= start < n_iter:
        raise ValueError(f"projection rows need n_iter >= 1 and 0 <= start < n_iter, got n_iter {n_iter}, start {start}")
    if zero_init < 0:
        raise ValueError(f"zero_init must be >= 0, got {zero_init}")
    rows = torch.zeros(n_iter, 4, dtype=torch.float64)
    if m == PROJECTION_MODES["apg"]:
        rows[:, 0], rows[:, 1], rows[:, 2] = float(eta), float(momentum), float(norm_threshold)
        rows[start, 1] = 0.0
    rows[:, 3] = 1.0
    rows[:zero_init, 3] = 0.0
    return rows[start:].to(torch.float32).contiguous()


def edit_start(steps: int, solver: str, strength: float):
    """(k0, i0) of an edit run at `strength`: the run is the suffix [i0, steps) of the plain run's iterations, starting from the
    source noised to sigma_{k0}.  Counted in whole solver steps (the diffusers img2img rule): n_full = steps // stages,
    n_keep = min(int(n_full * strength), n_full), k0 = n_full - n_keep, i0 = k0 * stages.  n_keep = 0 is refused."""
    if solver not in SOLVERS:
        raise ValueError(f"Solver {solver} not supported. Supported solvers: {list(SOLVERS)}")
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must lie in (0, 1], got {strength}")
    stages = SOLVER_STAGES[solver]
    n_full = int(steps) // stages
    n_keep = min(int(n_full * strength), n_full)
    if n_keep < 1:
        raise ValueError(f"strength {strength} leaves no {solver} step of {steps} to run (n_full = {n_full}): raise the "
                         "strength or the step count")
    k0 = n_full - n_keep
    return k0, k0 * stages


def edit_solver_table(sigmas: torch.Tensor, solver: str, n_iter: int, i0: int = 0, multistep_order: Optional[int] = None) -> torch.Tensor:
    """Rows [i0:] of solver_table with STEP_BLEND and sigma_{k+1} (column 5) on every iteration that ends a solver step.
    multistep_order: the suffix has no history at i0, so the warm-up of its Adams-Bashforth rows begins there (start=i0)."""
    ms = {} if multistep_order is None else {"multistep_order": multistep_order, "start": i0}
    rows = solver_table(sigmas, solver, n_iter, **ms).clone()
    stages = SOLVER_STAGES[solver]
    for i in range(stages - 1, n_iter, stages):
        k = i // stages
        rows[i, 4] = float(int(rows[i, 4]) | STEP_BLEND)
        rows[i, 5] = sigmas[k + 1]
    return rows[i0:].contiguous()


def timestep_features(t: torch.Tensor, dim: int = 256, max_period: int = 10000) -> torch.Tensor:
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def rope_table(n_pos: int, dim: int = 128, theta: float = 10000.0):
    """cos/sin [n_pos, dim/2] for positions 0..n_pos-1 (pair k uses theta^(-2k/dim))."""
    pos = torch.linspace(0.0, float(n_pos), n_pos + 1, dtype=torch.float32)[:n_pos]
    idx = torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2]
    freqs = torch.pow(torch.tensor(theta, dtype=torch.float32).expand_as(idx), -(idx / torch.tensor(float(dim))))
    ang = torch.outer(pos, freqs)
    return ang.cos().contiguous(), ang.sin().contiguous()


def nearest_exact_index(out_len: int, in_len: int) -> torch.Tensor:
    """Source index of F.interpolate(x, size=out_len, mode='nearest-exact') (hifi_foley.py:44,58,761).
    ATen evaluates it in *float32*: scale = float(in)/float(out), idx = min(int(floor((i + 0.5f) * scale)),
    in-1) - a float64 evaluation picks the neighbouring row for ~5 % of the widget-reachable
    durations (1.1 s, 2.7 s, 30.1 s ...), so the float32 arithmetic is reproduced operation by operation."""
    scale = torch.tensor(float(in_len), dtype=torch.float32) / torch.tensor(float(out_len), dtype=torch.float32)
    i = torch.arange(out_len, dtype=torch.float32)
    return torch.clamp(torch.floor((i + 0.5) * scale).long(), max=in_len - 1)


def interleaved_positions(la: int, lv: int):
    """audio token i -> 2i ; visual token j -> 2*floor((j+0.5)*la/lv)+1."""
    down = nearest_exact_index(lv, la)
    up = nearest_exact_index(la, lv)
    if not torch.equal(up[down], torch.arange(lv)):
        raise ValueError(f"interleaved RoPE is not a pure re-indexing for La={la}, Lv={lv}")
    return 2 * torch.arange(la), 2 * down + 1


def build_tables(la: int, lv: int, ls: int, lt: int, steps: int, solver: str, shift: float,
                 time_freq_dim: int = 256, fp8_time: Optional[torch.dtype] = None,
                 edit_i0: Optional[int] = None, multistep_order: Optional[int] = None, start: int = 0) -> Dict[str, torch.Tensor]:
    """fp8_time: round the sinusoid timestep features through this fp8 type (fp8-wrapped model under
    autocast, embed_layers.py:134 - golden g8).  edit_i0 (edit runs): the per-iteration tables are the rows [edit_i0:] of the
    plain run's, the solver rows carry the blend (edit_solver_table).  multistep_order / start: Adams-Bashforth rows
    (solver_table); an edit run's warm-up begins at edit_i0."""
    sig = sigma_grid(steps, shift)
    ts = model_timesteps(sig)
    n_iter = steps
    pa, pv = interleaved_positions(la, lv)
    rope_len = max(2 * la, lt, lv) + 1
    cos, sin = rope_table(rope_len)
    out = {
        "sigmas": sig,
        "timesteps": ts,
        "t_feat": (timestep_features(ts, time_freq_dim) if fp8_time is None
                   else timestep_features(ts, time_freq_dim).to(fp8_time).to(torch.float32)).contiguous(),
        "solver_coef": solver_table(sig, solver, n_iter, multistep_order=multistep_order, start=start),
        "rope_cos": cos, "rope_sin": sin,
        "pos_audio_self": pa.to(torch.int32), "pos_visual_self": pv.to(torch.int32),
        "pos_linear": torch.arange(max(la, lv, lt), dtype=torch.int32),
        "sync_gather": nearest_exact_index(la, ls).to(torch.int32),
    }
    if edit_i0 is not None:
        out["t_feat"] = out["t_feat"][edit_i0:].contiguous()
        out["solver_coef"] = edit_solver_table(sig, solver, n_iter, edit_i0, multistep_order=multistep_order)
    return out
