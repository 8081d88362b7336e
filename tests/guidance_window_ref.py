"""The reference side of the guidance window (docs/guidance_window.md): the CPU oracle's conditioning states combined by the rules of
f5_sample_rows / f5_sample_dual, each row's strengths gated by its window on the time of the FUNCTION EVALUATION, driven through the
oracle's own solvers.  No GPU.

    in(b)  = lo[b] <= t_eval <= hi[b]                    both ends inclusive, in the fp32 the solver computes the time in
    c, a   = in(b) ? the row's strengths : 0
    single : k = F + (F - N) c                           rows with c < 1e-5 take k = F
    dual   : k = (F + (F - T) a) + (T - N) c             rows with both below 1e-5 take k = F

The record of a run -- which rows were guided at which evaluation -- is the expected wide / narrow pattern of the engine: an evaluation
is wide when any row was guided at it.
"""
import torch

import dual_guidance_ref as DG
from f5test import O

PER_STEP = dict(euler=1, midpoint=2, rk4=4)
MISTAKES = ("per_step", "half_open", "audio_ungated")


def eval_times(grid, method):
    """the fp32 times at which the solver evaluates the field for `grid`, in order (oracle odeint_*)"""
    out = []
    for i in range(len(grid) - 1):
        t0, dt = grid[i], grid[i + 1] - grid[i]
        out += {"euler": [t0], "midpoint": [t0, t0 + 0.5 * dt], "rk4": [t0, t0 + 0.5 * dt, t0 + 0.5 * dt, t0 + dt]}[method]
    return torch.stack(out) if out else torch.zeros(0)


def window_sample(dit, cond, text, durations, y0, steps, method, text_strength, lo, hi, audio=None, sway_sampling_coef=-1.0, mistake=None):
    """-> (final mel with the conditioning spliced in, trajectory (steps, b, n, d), record (nfe, b) bool: row b guided at evaluation j).
    text_strength / audio / lo / hi: one value per row; audio = None is single guidance.  mistake (seeded, for the helper's own test):
    "per_step" tests the window on the step's time where it belongs on the stage's, "half_open" takes the interval as [lo, hi),
    "audio_ungated" leaves the audio strength of dual guidance outside the gate."""
    assert mistake is None or mistake in MISTAKES
    aux = DG.aux_of(dit, cond, text, durations, y0)
    grid = O.time_grid(steps, sway_sampling_coef, dtype=torch.float32).to(dit.dtype)
    f32 = torch.float32
    lo_t, hi_t = torch.as_tensor(lo, dtype=f32), torch.as_tensor(hi, dtype=f32)
    c_rows = torch.as_tensor(text_strength, dtype=f32)
    a_rows = None if audio is None else torch.as_tensor(audio, dtype=f32)
    record = []

    def fn(t, x):
        t_gate = grid[len(record) // PER_STEP[method]] if mistake == "per_step" else t
        t_gate = torch.as_tensor(t_gate).to(f32)
        inside = (lo_t <= t_gate) & ((t_gate < hi_t) if mistake == "half_open" else (t_gate <= hi_t))
        zero = torch.zeros_like(c_rows)
        c = torch.where(inside, c_rows, zero)
        a = None if a_rows is None else (a_rows if mistake == "audio_ungated" else torch.where(inside, a_rows, zero))
        guided = ~(c < 1e-5) if a is None else (~(c < 1e-5) | ~(a < 1e-5))
        record.append(guided)
        f, tt, n = DG.three_forwards(dit, aux, x, t)
        if a is None:
            k = f + (f - n) * c.to(f.dtype).reshape(-1, 1, 1)
        else:
            k = DG.combine(f, tt, n, a, c)
        return torch.where(guided.reshape(-1, 1, 1), k, f)

    traj = DG.SOLVERS[method](fn, torch.as_tensor(y0).to(dit.dtype), grid)
    cond_mask = aux["cond_mask"][..., None]
    cond_p = torch.zeros_like(traj[-1])
    cond_p[:, :cond.shape[1]] = cond
    rec = torch.stack(record) if record else torch.zeros((0, len(c_rows)), dtype=torch.bool)
    return torch.where(cond_mask, cond_p, traj[-1]), traj, rec


def pattern_of(record):
    """wide (1) / narrow (0) per evaluation"""
    return record.any(dim=1).to(torch.uint8)


# ---- the shape both test files use (tests/test_row_controls_gpu.py): TINY, B = 3, ragged 23 / 37 / 31 --------------------------------------
B, N, NT, NREF = 3, 37, 10, 12
DURS = [23, 37, 31]
SOLVER_CASES = [("euler", 5), ("midpoint", 4), ("rk4", 3)]
# One window per row on the sway -1 grid t = 1 - cos(pi/2 i/(steps-1)).  Evaluation times: euler-5 0, .0761, .2929, .6173; midpoint-4 0,
# .0670, .1340, .3170, .5, .75; rk4-3 0, .1464 x2, .2929 x2, .6464 x2, 1.  Every bound is at least 1e-2 from every one of them; each
# solver gets a narrow evaluation (t = 0), wide ones, and wide ones in which some row is outside its window.
LO, HI = [0.05, 0.2, 0.6], [0.4, 0.55, 0.9]
CFG_ROWS = [2.0, 1.5, 2.5]                                 # single guidance
DUAL_A, DUAL_C = [3.0, 0.0, 1.0], [0.5, 2.0, 0.0]          # dual guidance: (audio, text) per row


def inputs():
    """the seeded batch of the row-controls / dual-guidance tests: (cond, text, y0)"""
    import numpy as np
    from f5test import TINY, randn, rng
    r = rng(77)
    cond = randn(r, B, NREF, TINY.mel_dim)
    text = torch.from_numpy(r.integers(0, TINY.text_num_embeds, (B, NT)).astype(np.int32))
    text[1, 8:], text[2, 6:] = -1, -1
    y0 = torch.zeros((B, N, TINY.mel_dim))
    for i, d in enumerate(DURS):
        y0[i, :d] = torch.from_numpy(r.standard_normal((TINY.mel_dim, d)).astype(np.float32).T)
    return cond, text, y0
