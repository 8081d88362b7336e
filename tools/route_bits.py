"""Digests of what every sampling route returns, for refactors of the host layer: run it once per build of the library (F5TTS_HIP_LIB
selects another build) or per tree, and compare the outputs line by line -- a host-side change must leave every line as it was.

Tiny configuration, seeded synthetic weights and inputs, the shapes of the row-control tests (B = 3, N = 37, ragged 23 / 37 / 31, nt = 9);
Euler at 5 points, midpoint at 4, rk4 at 3; precisions f16 and bf16x3 (one and two operand segments), and mxfp8 for the calls it does not
refuse (plain and edit).  Calls: plain guided and unguided, edit mask, rows, rows with mask, dual, window single (mixed wide / narrow
pattern), window dual -- each eager and as a hipGraph, run twice (the second graph call replays) -- and dit_forward scalar, per row and
dual.  One JSON line per call: SHA-256 of `out` and of the trajectory (of each branch for a forward), the call's status word (the first
word of the workspace), what f5_engine_ln_fold_active says of a plain call of the line's shape, and whether the two runs agreed; nothing
else varies between runs.  A call the library refuses is a line too: `refused` holds its return code and message, which is how the order
of the refusals of one call gets compared.

Then the option axis: every engine option away from its default (OPTION_AXIS; the last entry also forces the role-split GEMM kernel, so
that the LN fold runs at width 256), one engine each, on five of the sample calls (OPTION_CALLS; mxfp8: the plain ones) and the scalar forward in all three precisions, Euler
at 5 points.
--full adds the 335M configuration (f16, N = 937, Euler at 3 points, eager and graph): the default route at batch 1, ln_fold = 1 at batch 1
(single-round route, statistics form) and at batch 4 with fold_stats -1 and 1 (staged route, row-factor and statistics form).

Public Engine methods, plus the workspace's first word and the C entry point f5_engine_ln_fold_active, which have no Python wrapper.

    python tools/route_bits.py [--full] > route_bits.jsonl
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f5_tts_mlx_amd.cfm import time_grid, time_grid_rows  # noqa: E402
from f5_tts_mlx_amd.engine import Engine  # noqa: E402
from f5_tts_mlx_amd.weights import F5TTS_335M, TINY, synthetic_weights  # noqa: E402

B, N, NT, NREF, DURS = 3, 37, 9, 12, [23, 37, 31]
SOLVERS = (("euler", 5), ("midpoint", 4), ("rk4", 3))
SWAY = [-1.0, None, -0.5]                                  # per-row time grids
CFG_ROWS = [2.0, 0.0, 1.3]                                 # row 1 unguided
DUAL_A, DUAL_C = [3.0, 0.0, 1.0], [0.5, 2.0, 0.0]          # (audio, text) strength per row
LO, HI = [0.05, 0.2, 0.6], [0.4, 0.55, 0.9]                # windows that leave some evaluations without a guided row
WINDOW = np.stack([LO, HI], 1)
# (option, value, f5_debug_set_gemm_tile): at this size ln_fold = 1 is refused under the default routing, with one message per route
OPTION_AXIS = (("ln_fusion", 1, 0), ("qkv_transposed", 0, 0), ("q_premul", 0, 0), ("null_keeps_cond", 1, 0), ("isolate_rows", 1, 0),
               ("graph_split", 1, 0), ("sat_check", 0, 0), ("ln_fold", 0, 0), ("ln_fold", 1, 0), ("ln_fold", 1, 14))
OPTION_CALLS = ("plain_guided", "plain_unguided", "rows_edit", "dual", "window")
FULL_N, FULL_NT, FULL_NREF = 937, 64, 300
# (batch, {option: value}) of the --full section
FULL_AXIS = ((1, {}), (1, {"ln_fold": 1}), (4, {"ln_fold": 1, "fold_stats": -1}), (4, {"ln_fold": 1, "fold_stats": 1}))


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def make_inputs(device, cfg=TINY, durs=DURS, n=N, nt=NT, nref=NREF):
    r = np.random.default_rng(77)
    mel, b = cfg.mel_dim, len(durs)
    cond = np.zeros((b, n, mel), np.float32)
    cond[:, :nref] = r.standard_normal((b, nref, mel)).astype(np.float32)
    text = r.integers(0, cfg.text_num_embeds, (b, nt)).astype(np.int32)
    if b == B:
        text[1, 7:], text[2, 5:] = -1, -1
    y0 = np.zeros((b, n, mel), np.float32)
    for i, d in enumerate(durs):
        y0[i, :d] = r.standard_normal((d, mel)).astype(np.float32)
    keep = np.zeros((b, n), bool)                          # edit mask: the reference frames, two of them dropped, and every fifth frame behind
    keep[:, :nref] = True
    keep[:, 4:6] = False
    for i, d in enumerate(durs):
        keep[i, nref:d:5] = True
    dev = lambda a: torch.from_numpy(a).to(device).contiguous()  # noqa: E731
    return dev(text), dev(cond), [nref] * b, list(durs), dev(y0), dev(keep)


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


def status_word(eng) -> int:
    torch.cuda.synchronize()
    return int(eng._workspace[:4].view(torch.int32).item())


def fold_active(eng, inputs, steps, method, cfg):
    """f5_engine_ln_fold_active for the plain call of these shapes: 0 / 1 / 2, or the refusal"""
    text, cond, lens, durs, _, _ = inputs
    ws = eng.workspace(cond.shape[0], cond.shape[1], text.shape[1], steps, method)
    a, keep = eng._args(text, cond, lens, durs, None, np.zeros(steps, np.float32), steps, method, cfg, cond.shape[0] > 1, False, None, None, ws)
    active = C.c_int(-1)
    rc = eng.lib.f5_engine_ln_fold_active(eng._h, C.byref(a), C.byref(active))
    del keep
    return int(active.value) if rc == 0 else f"rc={rc}: {eng.lib.f5_last_error().decode('utf-8', 'replace')}"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="write the lines here instead of standard output")
    ap.add_argument("--full", action="store_true", help="add the section on the 335M configuration")
    args = ap.parse_args(argv)
    sink = open(args.out, "w") if args.out else sys.stdout
    weights = synthetic_weights(TINY, seed=42)
    inputs = make_inputs(args.device)
    bad = 0

    def emit(rec, eng, inp, steps, method, cfg, call):
        """runs `call` twice; the line holds the second run's digests, or the refusal"""
        nonlocal bad
        runs = []
        for _ in range(2):
            try:
                runs.append(dict(call(), status=status_word(eng)))
            except (RuntimeError, ValueError) as e:
                runs.append(dict(refused=str(e)))
        rec.update(runs[-1], reproducible=all(r == runs[0] for r in runs), ln_fold_active=fold_active(eng, inp, steps, method, cfg))
        bad += not rec["reproducible"]
        print(json.dumps(rec, sort_keys=True), file=sink, flush=True)

    def sample_line(rec, eng, inp, name, kw, method, steps, graph):
        text, cond, lens, durs, y0, keep = inp
        kw = dict(kw)
        t = kw.pop("t")
        mask = keep if kw.pop("mask", False) else None

        def call():
            out, traj = eng.sample(text, cond, lens, durs, y0, t, method=method, use_graph=graph, cond_keep=mask, **kw)
            return dict(out=sha(out), traj=sha(traj))

        cfg = kw["cfg_strength"] if np.ndim(kw["cfg_strength"]) == 0 else 2.0
        emit(dict(rec, call=name, method=method, steps=steps, graph=graph), eng, inp, steps, method, cfg, call)

    def forward_line(rec, eng, inp, name, kw):
        text, cond, lens, durs, y0, _ = inp

        def call():
            preds = eng.dit_forward(y0, text, cond, lens, durs, cfg_strength=2.0, **kw)
            return {k: sha(p) for k, p in zip(("pred", "null_pred", "text_pred"), preds)}

        emit(dict(rec, call=name), eng, inp, 2, "euler", 2.0, call)

    for prec in ("f16", "bf16x3", "mxfp8"):
        eng = Engine(TINY, precision=prec, device=args.device)
        eng.load_weights(weights)
        for method, steps in SOLVERS:
            for name, kw in sample_calls(steps, SWAY).items():
                if prec == "mxfp8" and name not in ("plain_guided", "plain_unguided", "edit"):
                    continue
                for graph in (False, True):
                    sample_line(dict(precision=prec), eng, inputs, name, kw, method, steps, graph)
        if prec != "mxfp8":
            forwards = {"forward_scalar": dict(t=0.35), "forward_rows": dict(t=[0.1, 0.5, 0.9]),
                        "forward_dual": dict(t=[0.1, 0.5, 0.9], audio_cfg_strength=1.0)}
            for name, kw in forwards.items():
                forward_line(dict(precision=prec), eng, inputs, name, kw)
        del eng

    # the option axis: range_check "off", so that no status word makes the engine change its own options between the lines
    calls = sample_calls(5, SWAY)
    for prec in ("f16", "bf16x3", "mxfp8"):
        for opt, val, tile in OPTION_AXIS:
            eng = Engine(TINY, precision=prec, device=args.device, range_check="off")
            eng.load_weights(weights)
            eng.set_option(opt, val)
            eng.lib.f5_debug_set_gemm_tile(tile)
            rec = dict(precision=prec, option=f"{opt}={val}", gemm_tile=tile)
            try:
                for name in OPTION_CALLS:
                    if prec == "mxfp8" and not name.startswith("plain"):
                        continue
                    for graph in (False, True):
                        sample_line(rec, eng, inputs, name, calls[name], "euler", 5, graph)
                forward_line(rec, eng, inputs, "forward_scalar", dict(t=0.35))
            finally:
                eng.lib.f5_debug_set_gemm_tile(0)
            del eng

    if args.full:
        eng = Engine(F5TTS_335M, precision="f16", device=args.device, range_check="off")
        eng.load_weights(synthetic_weights(F5TTS_335M, seed=42))
        t = time_grid(3, -1.0)
        for batch, opts in FULL_AXIS:
            inp = make_inputs(args.device, F5TTS_335M, [FULL_N - 40 * i for i in range(batch)], FULL_N, FULL_NT, FULL_NREF)
            for opt in ("ln_fold", "fold_stats"):
                eng.set_option(opt, opts.get(opt, -1))
            rec = dict(config="335M", precision="f16", batch=batch, option=" ".join(f"{k}={v}" for k, v in opts.items()) or "default")
            for graph in (False, True):
                sample_line(rec, eng, inp, "plain_guided", dict(t=t, cfg_strength=2.0), "euler", 3, graph)
        del eng
    if bad:
        print(f"route_bits: {bad} call(s) gave different digests on their two runs: not comparable by digest", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
