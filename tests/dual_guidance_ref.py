"""The reference side of dual guidance (docs/dual_guidance.md): the CPU oracle's three conditioning states combined by the rule and driven
through the oracle's own solvers.  No GPU.

    F = DiT(drop_audio_cond=False, drop_text=False)      audio kept, text kept
    T = DiT(drop_audio_cond=True,  drop_text=False)      audio dropped, text kept
    N = DiT(drop_audio_cond=True,  drop_text=True)       both dropped
    k = (F + (F - T) * a) + (T - N) * c                  a = the row's audio (speaker) strength, c = its text strength
"""
import torch

from f5test import O

SOLVERS = dict(euler=O.odeint_euler, midpoint=O.odeint_midpoint, rk4=O.odeint_rk4)


def aux_of(dit, cond, text, durations, y0):
    """step_cond, mask, text and the conditioning mask of the batch, as O.sample builds them (a one-point grid: no evaluation)"""
    _, _, aux = O.sample(dit, cond, text, torch.as_tensor(durations), y0=y0, steps=1, method="euler", cfg_strength=0.0, return_aux=True)
    return aux


def three_forwards(dit, aux, x, t):
    """(F, T, N) at time t (a scalar or one per row)"""
    return tuple(dit.forward(x, aux["step_cond"], aux["text"], t, drop_audio, drop_text, aux["mask"])
                 for drop_audio, drop_text in ((False, False), (True, False), (True, True)))


def combine(f, t, n, audio, text_strength):
    a = torch.as_tensor(audio, dtype=f.dtype).reshape(-1, 1, 1)
    c = torch.as_tensor(text_strength, dtype=f.dtype).reshape(-1, 1, 1)
    return (f + (f - t) * a) + (t - n) * c


def dual_sample(dit, cond, text, durations, y0, steps, method, audio, text_strength, sway_sampling_coef=-1.0, t_is=None):
    """-> (final mel with the conditioning spliced in, trajectory (steps, b, n, d)); audio / text_strength: one value per row.
    t_is: which forward stands in for T (a seeded mistake: "F", "N" or "audio_kept_text_dropped"); None = the rule."""
    aux = aux_of(dit, cond, text, durations, y0)

    def fn(t, x):
        f, tt, n = three_forwards(dit, aux, x, t)
        if t_is == "F":
            tt = f
        elif t_is == "N":
            tt = n
        elif t_is == "audio_kept_text_dropped":
            tt = dit.forward(x, aux["step_cond"], aux["text"], t, False, True, aux["mask"])
        return combine(f, tt, n, audio, text_strength)

    grid = O.time_grid(steps, sway_sampling_coef, dtype=torch.float32).to(dit.dtype)
    traj = SOLVERS[method](fn, torch.as_tensor(y0).to(dit.dtype), grid)
    cond_mask = aux["cond_mask"][..., None]
    cond_p = torch.zeros_like(traj[-1])
    cond_p[:, :cond.shape[1]] = cond
    return torch.where(cond_mask, cond_p, traj[-1]), traj
