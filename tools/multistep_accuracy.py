"""Accuracy of the solvers at equal numbers of function evaluations, on the CPU oracle (docs/multistep.md; the table there comes from
here).  No GPU:
python tools/multistep_accuracy.py [out.jsonl]

TINY config, synthetic_weights(seed=42), fp64, B = 2, ragged 29 / 40 frames, cfg 2.  Every figure is the mean |delta| of the final
state (frames below each row's duration) against rk4 on a 129-point grid of the same kind.  NFE = function evaluations of the guided
velocity: Euler, ab2 and ab3 take NFE + 1 grid points, midpoint NFE / 2 + 1.

The random-weight field is rough: no solver is in its asymptotic regime at these step counts and the 129-point rk4 solution is not
converged either, so the table can show which result lies closer to a finer solve of the same field and nothing about an order of
convergence -- and nothing about a trained checkpoint."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import f5_oracle as O  # noqa: E402
from f5_tts_mlx_amd import cfm  # noqa: E402
from f5_tts_mlx_amd.weights import TINY, synthetic_weights  # noqa: E402

B, NREF, NT, DURS, CFG = 2, 12, 10, [29, 40], 2.0
NFES = (8, 16, 32)
SOLVERS = dict(euler=(O.odeint_euler, 1), midpoint=(O.odeint_midpoint, 2), ab2=(cfm.odeint_ab2, 1), ab3=(cfm.odeint_ab3, 1))


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    r = np.random.default_rng(77)
    f64 = torch.float64
    cond = torch.from_numpy(r.standard_normal((B, NREF, TINY.mel_dim))).to(f64)
    text = torch.from_numpy(r.integers(0, TINY.text_num_embeds, (B, NT)).astype(np.int32))
    text[1, 7:] = -1
    y0 = torch.zeros((B, max(DURS), TINY.mel_dim), dtype=f64)
    for i, d in enumerate(DURS):
        y0[i, :d] = torch.from_numpy(r.standard_normal((TINY.mel_dim, d)).T)
    dit = O.DiTOracle(TINY, synthetic_weights(TINY, seed=42), dtype=f64)
    _, _, aux = O.sample(dit, cond, text, torch.tensor(DURS), y0=y0, steps=1, method="euler", cfg_strength=0.0, return_aux=True)
    live = torch.arange(max(DURS))[None, :] < torch.tensor(DURS)[:, None]

    def field(t, x):
        f = dit.forward(x, aux["step_cond"], aux["text"], t, False, False, aux["mask"])
        n = dit.forward(x, aux["step_cond"], aux["text"], t, True, True, aux["mask"])
        return f + (f - n) * CFG

    for sway in (-1.0, None):
        fine = O.odeint_rk4(field, y0, O.time_grid(129, sway, dtype=f64))[-1]
        for nfe in NFES:
            row = dict(grid="sway -1" if sway is not None else "linear", nfe=nfe)
            for name, (solve, per) in SOLVERS.items():
                y = solve(field, y0, O.time_grid(nfe // per + 1, sway, dtype=f64))[-1]
                row[name] = float((y - fine).abs()[live].mean())
            line = json.dumps({k: (float(f"{v:.3e}") if isinstance(v, float) else v) for k, v in row.items()})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")


if __name__ == "__main__":
    main()
