"""Cost of per-request sampling controls on one GPU (docs/row_controls.md; the figures there come from here):
python tools/row_controls_cost.py [out.jsonl]

335M shape, N = 937 frames, 32-point Euler, precision f16, hipGraph replay, synthetic weights and the inputs of bench.py.
  sample:  one sample() on the per-row route (every row its own guidance strength and sway coefficient) against one sample() on the
           scalar route, at batch 2 and batch 32; and, at batch 32, against what a caller without the route has to do: k separate scalar
           calls of 32 / k rows each, one per group of equal settings (k = 2, 4).
  loss:    F5TTS.__call__ at b = 8 with DiT.row_times (one batched forward) against the loop of batch-1 forwards.
Legs of a comparison alternate inside every repetition; each figure is a host clock around calls that end in a device synchronise,
median / min / max of RUNS repetitions after WARMUP (the first call of a shape captures its graph)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from f5_tts_mlx_amd.cfm import F5TTS  # noqa: E402
from f5_tts_mlx_amd.dit import DiT  # noqa: E402
from f5_tts_mlx_amd.weights import F5TTS_335M, synthetic_weights  # noqa: E402

RUNS, WARMUP = 5, 2
POINTS = 32
SWAYS = (-1.0, None, -0.5, -0.8)
CFGS = (2.0, 1.5, 2.5, 1.0)


def alternate(legs):
    """legs: {name: fn}; -> {name: sorted seconds}"""
    times = {k: [] for k in legs}
    for rep in range(WARMUP + RUNS):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(time.perf_counter() - t0)
    return {k: sorted(v) for k, v in times.items()}


def record(sink, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ts):
    return dict(median_ms=round(1e3 * ts[len(ts) // 2], 2), min_ms=round(1e3 * ts[0], 2), max_ms=round(1e3 * ts[-1], 2))


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    model = DiT.from_config(F5TTS_335M, precision="f16", device=dev)
    model.load_weights(synthetic_weights(F5TTS_335M, seed=42))
    f5 = F5TTS(transformer=model)
    N = bench.N_FRAMES
    model.engine.workspace(32, N, bench.NT, POINTS, "euler", rows=True)         # the largest plan first: no call re-allocates (and drops graphs)
    for B in (2, 32):
        cond, text, y0, _ = bench.synth_batch(B, first=0, device=dev)
        kw = dict(duration=N, steps=POINTS, method="euler", use_graph=True)
        cfg_rows = [CFGS[i % 4] for i in range(B)]
        sway_rows = [SWAYS[i % 4] for i in range(B)]
        legs = {"scalar": lambda: f5.sample(cond, text, y0=y0, cfg_strength=2.0, sway_sampling_coef=-1.0, **kw),
                "rows": lambda: f5.sample(cond, text, y0=y0, cfg_strength=cfg_rows, sway_sampling_coef=sway_rows, **kw)}
        if B == 32:
            for k in (2, 4):
                h = B // k

                def grouped(k=k, h=h):
                    for g in range(k):
                        s = slice(g * h, (g + 1) * h)
                        # (pad_to: the group keeps the batch's key-padding rule; the lengths are all N here)
                        f5.sample(cond[s], text[s], y0=y0[s], cfg_strength=CFGS[g], sway_sampling_coef=SWAYS[g], pad_to=N, **kw)

                legs[f"grouped_k{k}"] = grouped
        res = alternate(legs)
        base = res["scalar"][len(res["scalar"]) // 2]
        for name, ts in res.items():
            record(sink, what="sample", batch=B, frames=N, points=POINTS, precision="f16", leg=name, runs=RUNS,
                   vs_scalar=round(ts[len(ts) // 2] / base, 4), graphs_held=model.engine.graph_count(), **stats(ts))
        model.engine.synchronize()
        record(sink, what="status", batch=B, saturation_events=model.engine.saturation_events, range_events=model.engine.range_events)
    # the flow-matching loss: a different time per row
    b = 8
    cond, text, y0, _ = bench.synth_batch(b, first=0, device=dev)
    mel = torch.zeros((b, N, 100), device=dev)
    mel[:, :cond.shape[1]] = cond
    mel[:, cond.shape[1]:] = y0[:, cond.shape[1]:] * 0.5
    rand = dict(time=torch.linspace(0.05, 0.95, b), frac_lengths=torch.full((b,), 0.8), span_rand=torch.full((b,), 0.5),
                x0=y0.cpu(), rand_audio_drop=0.9, rand_cond_drop=0.9)
    vals = {}

    def loss(flag):
        model.row_times = flag
        vals[flag] = float(f5(mel, text.cpu(), rand=rand))

    res = alternate({"loop": lambda: loss(False), "row_times": lambda: loss(True)})
    base = res["loop"][len(res["loop"]) // 2]
    for name, ts in res.items():
        record(sink, what="loss_forward", batch=b, frames=N, precision="f16", leg=name, runs=RUNS, vs_loop=round(ts[len(ts) // 2] / base, 4),
               loss=vals[name == "row_times"], **stats(ts))


if __name__ == "__main__":
    main()
