"""Digests of what every sampling route returns, for refactors of the host layer: run it once per build of the library (F5TTS_HIP_LIB
selects another build) or per tree, and compare the outputs line by line -- a host-side change must leave every line as it was.

Tiny configuration, seeded synthetic weights and inputs, the shapes of the row-control tests (B = 3, N = 37, ragged 23 / 37 / 31, nt = 9);
Euler at 5 points, midpoint at 4, rk4 at 3; precisions f16 and bf16x3 (one and two operand segments), and mxfp8 for the calls it does not
refuse (plain and edit).  Calls: plain guided and unguided, edit mask, rows, rows with mask, dual, window single (mixed wide / narrow
pattern), window dual -- each eager and as a hipGraph, run twice (the second graph call replays) -- and dit_forward scalar, per row and
dual.  One JSON line per call: SHA-256 of `out` and of the trajectory (of each branch for a forward), and whether the two runs agreed;
nothing else varies between runs.  Only public Engine methods are used.

    python tools/route_bits.py > route_bits.jsonl
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f5_tts_mlx_amd.cfm import time_grid, time_grid_rows  # noqa: E402
from f5_tts_mlx_amd.engine import Engine  # noqa: E402
from f5_tts_mlx_amd.weights import TINY, synthetic_weights  # noqa: E402

B, N, NT, NREF, DURS = 3, 37, 9, 12, [23, 37, 31]
SOLVERS = (("euler", 5), ("midpoint", 4), ("rk4", 3))
SWAY = [-1.0, None, -0.5]                                  # per-row time grids
CFG_ROWS = [2.0, 0.0, 1.3]                                 # row 1 unguided
DUAL_A, DUAL_C = [3.0, 0.0, 1.0], [0.5, 2.0, 0.0]          # (audio, text) strength per row
LO, HI = [0.05, 0.2, 0.6], [0.4, 0.55, 0.9]                # windows that leave some evaluations without a guided row
WINDOW = np.stack([LO, HI], 1)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def make_inputs(device):
    r = np.random.default_rng(77)
    mel = TINY.mel_dim
    cond = np.zeros((B, N, mel), np.float32)
    cond[:, :NREF] = r.standard_normal((B, NREF, mel)).astype(np.float32)
    text = r.integers(0, TINY.text_num_embeds, (B, NT)).astype(np.int32)
    text[1, 7:], text[2, 5:] = -1, -1
    y0 = np.zeros((B, N, mel), np.float32)
    for i, d in enumerate(DURS):
        y0[i, :d] = r.standard_normal((d, mel)).astype(np.float32)
    keep = np.zeros((B, N), bool)                          # edit mask: the reference frames, two of them dropped, and every fifth frame behind
    keep[:, :NREF] = True
    keep[:, 4:6] = False
    for i, d in enumerate(DURS):
        keep[i, NREF:d:5] = True
    dev = lambda a: torch.from_numpy(a).to(device).contiguous()  # noqa: E731
    return dev(text), dev(cond), [NREF] * B, list(DURS), dev(y0), dev(keep)


def sample_calls(steps, coef_rows):
    """name -> keyword arguments of Engine.sample that select the route (t included)"""
    t, grids = time_grid(steps, -1.0), time_grid_rows(steps, coef_rows)
    return {
        "plain_guided": dict(t=t, cfg_strength=2.0),
        "plain_unguided": dict(t=t, cfg_strength=0.0),
        "edit": dict(t=t, cfg_strength=2.0, mask=True),
        "rows": dict(t=grids, cfg_strength=CFG_ROWS),
        "rows_edit": dict(t=grids, cfg_strength=CFG_ROWS, mask=True),
        "dual": dict(t=grids, cfg_strength=DUAL_C, audio_cfg_strength=DUAL_A),
        "window": dict(t=grids, cfg_strength=[2.0, 1.5, 2.5], cfg_interval=WINDOW),
        "window_dual": dict(t=grids, cfg_strength=DUAL_C, audio_cfg_strength=DUAL_A, cfg_interval=WINDOW),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="write the lines here instead of standard output")
    args = ap.parse_args(argv)
    sink = open(args.out, "w") if args.out else sys.stdout
    weights = synthetic_weights(TINY, seed=42)
    text, cond, lens, durs, y0, keep = make_inputs(args.device)
    bad = 0

    def emit(rec, runs):
        nonlocal bad
        rec.update(runs[-1], reproducible=all(r == runs[0] for r in runs))
        bad += not rec["reproducible"]
        print(json.dumps(rec, sort_keys=True), file=sink, flush=True)

    for prec in ("f16", "bf16x3", "mxfp8"):
        eng = Engine(TINY, precision=prec, device=args.device)
        eng.load_weights(weights)
        for method, steps in SOLVERS:
            for name, kw in sample_calls(steps, SWAY).items():
                if prec == "mxfp8" and name not in ("plain_guided", "plain_unguided", "edit"):
                    continue
                kw = dict(kw)
                t = kw.pop("t")
                mask = keep if kw.pop("mask", False) else None
                for graph in (False, True):
                    runs = []
                    for _ in range(2):
                        out, traj = eng.sample(text, cond, lens, durs, y0, t, method=method, use_graph=graph, cond_keep=mask, **kw)
                        torch.cuda.synchronize()
                        runs.append(dict(out=sha(out), traj=sha(traj)))
                    emit(dict(call=name, precision=prec, method=method, steps=steps, graph=graph), runs)
        if prec != "mxfp8":
            forwards = {"forward_scalar": dict(t=0.35), "forward_rows": dict(t=[0.1, 0.5, 0.9]),
                        "forward_dual": dict(t=[0.1, 0.5, 0.9], audio_cfg_strength=1.0)}
            for name, kw in forwards.items():
                runs = []
                for _ in range(2):
                    preds = eng.dit_forward(y0, text, cond, lens, durs, cfg_strength=2.0, **kw)
                    torch.cuda.synchronize()
                    runs.append({k: sha(p) for k, p in zip(("pred", "null_pred", "text_pred"), preds)})
                emit(dict(call=name, precision=prec), runs)
        del eng
    if bad:
        print(f"route_bits: {bad} call(s) gave different digests on their two runs: not comparable by digest", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
