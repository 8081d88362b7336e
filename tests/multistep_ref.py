"""The reference side of the multistep solvers ab2 / ab3 (docs/multistep.md): the CPU oracle's forwards combined by the rule of the route
in use and driven through the Adams-Bashforth recurrence with the weights of cfm.ab_weights.  No GPU.

    k_i     = the guided velocity of evaluation i, at the grid point t_i (one evaluation per step)
    single  : k = F + (F - N) c                          rows with c < 1e-5 take k = F
    dual    : k = (F + (F - T) a) + (T - N) c            rows with both below 1e-5 take k = F
    window  : c, a = lo[b] <= t_i[b] <= hi[b] ? the row's strengths : 0
    y_{i+1} = y_i + h (w0 k_i + w1 k_{i-1} + w2 k_{i-2}),   h = t_{i+1} - t_i, (w0, w1, w2) = ab_weights(grid of the row, i, order)

Every row has its own grid (a scalar route hands every row the same one), so h and the weights are (b,) vectors throughout.
"""
import numpy as np
import torch

import dual_guidance_ref as DG
import guidance_window_ref as GW
from f5_tts_mlx_amd.cfm import ab_weights, time_grid, time_grid_rows

ORDER = dict(ab2=2, ab3=3)
MISTAKES = ("uniform_weights", "stale_history", "no_startup")
UNIFORM = {1: (1.0, 0.0, 0.0), 2: (1.5, -0.5, 0.0), 3: (23 / 12, -16 / 12, 5 / 12)}

# ---- the shape of the engine-level tests: TINY, B = 3, ragged 23 / 37 / 31 (tests/guidance_window_ref.py), 6 grid points -----------------
B, N, NT, NREF, DURS = GW.B, GW.N, GW.NT, GW.NREF, GW.DURS
STEPS = 6                                                  # five steps: ab3 takes three third-order ones
SWAYS = [-1.0, None, -0.5]                                 # the per-row grids (tests/test_row_controls_gpu.py)
CFG = 2.0                                                  # f5_sample
CFG_ROWS = [2.0, 0.0, 1.3]                                 # f5_sample_rows: row 1 is unguided
DUAL_A, DUAL_C = GW.DUAL_A, GW.DUAL_C                      # f5_sample_dual
LO, HI = GW.LO, GW.HI                                      # f5_sample_window (single guidance, GW.CFG_ROWS)
inputs = GW.inputs


def grids_of(kind, batch=B, steps=STEPS):
    """(batch, steps) float32: "sway" = the sway -1 grid in every row, "rows" = one sway coefficient per row"""
    return np.tile(time_grid(steps, -1.0), (batch, 1)) if kind == "sway" else time_grid_rows(steps, SWAYS[:batch])


def weight_table(grids, order):
    """(steps - 1, b, 3) float32: what the engine stages"""
    grids = np.atleast_2d(np.asarray(grids, np.float32))
    return np.stack([np.stack([ab_weights(g, i, order) for g in grids]) for i in range(grids.shape[1] - 1)])


def amplification(grids, order):
    """A = max over steps and rows of sum_j |w_ij|: by how much one step amplifies an error of its k's, relative to Euler's 1"""
    return float(np.abs(weight_table(grids, order).astype(np.float64)).sum(axis=2).max())


def ab_sample(dit, cond, text, durations, y0, grids, method, strengths, audio=None, lo=None, hi=None, mistake=None):
    """-> (final mel with the conditioning spliced in, trajectory (steps, b, n, d)).  grids: (b, steps) float32, a row per batch row;
    strengths / audio / lo / hi: one value per row (audio = None: single guidance; lo = None: no window).  mistake (seeded, for the
    helper's own test): "uniform_weights" takes the classical coefficients of the step's order whatever the spacing, "stale_history"
    reads k_{i-2} where k_{i-1} belongs, "no_startup" takes step 0 as a second-order step on a history of zeros."""
    assert mistake is None or mistake in MISTAKES
    order = ORDER[method]
    aux = DG.aux_of(dit, cond, text, durations, y0)
    f32, dt = torch.float32, dit.dtype
    grids = np.atleast_2d(np.asarray(grids, np.float32))
    nb, steps = grids.shape
    tg = torch.from_numpy(grids)
    c_rows = torch.as_tensor(strengths, dtype=f32)
    a_rows = None if audio is None else torch.as_tensor(audio, dtype=f32)
    col = lambda v: torch.as_tensor(np.asarray(v), dtype=dt).reshape(-1, 1, 1)                  # noqa: E731

    def velocity(t_rows, x):
        c, a = c_rows, a_rows
        if lo is not None:
            inside = (torch.as_tensor(lo, dtype=f32) <= t_rows) & (t_rows <= torch.as_tensor(hi, dtype=f32))
            zero = torch.zeros_like(c_rows)
            c = torch.where(inside, c_rows, zero)
            a = None if a_rows is None else torch.where(inside, a_rows, zero)
        guided = ~(c < 1e-5) if a is None else (~(c < 1e-5) | ~(a < 1e-5))
        f, tt, n = DG.three_forwards(dit, aux, x, t_rows.to(dt))
        k = f + (f - n) * c.to(dt).reshape(-1, 1, 1) if a is None else DG.combine(f, tt, n, a, c)
        return torch.where(guided.reshape(-1, 1, 1), k, f)

    y = torch.as_tensor(y0).to(dt)
    states, ks = [y], []
    for i in range(steps - 1):
        ks = [velocity(tg[:, i], y)] + ks[:2]
        w = np.stack([ab_weights(g, i, order) for g in grids]).astype(np.float64)               # (b, 3)
        if mistake == "uniform_weights":
            w = np.stack([np.asarray(UNIFORM[int(np.count_nonzero(r))]) for r in w])
        hist = list(ks) + [torch.zeros_like(y)] * (3 - len(ks))
        if mistake == "stale_history" and len(ks) == 3:
            hist[1] = ks[2]
        if mistake == "no_startup" and i == 0:
            w = np.tile(np.asarray(UNIFORM[2]), (nb, 1))
        h = grids[:, i + 1].astype(np.float64) - grids[:, i].astype(np.float64)
        incr = col(w[:, 0]) * hist[0]
        for j in (1, 2):
            if np.any(w[:, j] != 0.0):
                incr = incr + col(w[:, j]) * hist[j]
        y = y + col(h) * incr
        states.append(y)
    traj = torch.stack(states)
    cond_p = torch.zeros_like(traj[-1])
    cond_p[:, :cond.shape[1]] = cond
    return torch.where(aux["cond_mask"][..., None], cond_p, traj[-1]), traj


# ---- the cases of the engine-level tests: route -> what ab_sample and Engine.sample take ---------------------------------------------------
ROUTES = {
    # name: (grid kind, strengths of the reference, audio, window, keyword arguments of Engine.sample)
    "scalar": ("sway", [CFG] * B, None, None, dict(cfg_strength=CFG)),
    "rows": ("rows", CFG_ROWS, None, None, dict(cfg_strength=CFG_ROWS)),
    "dual": ("rows", DUAL_C, DUAL_A, None, dict(cfg_strength=DUAL_C, audio_cfg_strength=DUAL_A)),
    "window": ("sway", GW.CFG_ROWS, None, (LO, HI), dict(cfg_strength=GW.CFG_ROWS,
                                                          cfg_interval=np.stack([np.asarray(LO, np.float32), np.asarray(HI, np.float32)], axis=1))),
}


def engine_grid(route):
    """the `t` argument of Engine.sample: the (steps,) grid of a scalar call, (b, steps) on a per-row route"""
    kind = ROUTES[route][0]
    return time_grid(STEPS, -1.0) if route == "scalar" else grids_of(kind)


def reference(dit, route, method, mistake=None, ins=None):
    cond, text, y0 = ins if ins is not None else inputs()
    kind, strengths, audio, window, _ = ROUTES[route]
    lo, hi = window if window else (None, None)
    return ab_sample(dit, cond, text, DURS, y0, grids_of(kind), method, strengths, audio=audio, lo=lo, hi=hi, mistake=mistake)
