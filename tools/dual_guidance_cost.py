"""Cost of dual guidance on one GPU (docs/dual_guidance.md; the figures there come from here):
python tools/dual_guidance_cost.py [out.jsonl]

335M shape, N = 937 frames, 32-point Euler, precision f16, hipGraph replay, synthetic weights and the inputs of bench.py.
One sample() on the dual route (three branches per evaluation; every row its own pair of strengths) against one sample() on the per-row
route (two branches; every row its own strength), at batch 2 and batch 32.  The legs alternate inside every repetition; each figure is a
host clock around a call that ends in a device synchronise, median / min / max of RUNS repetitions after WARMUP (the first call of a
shape captures its graph)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from f5_tts_mlx_amd.cfm import F5TTS  # noqa: E402
from f5_tts_mlx_amd.dit import DiT  # noqa: E402
from f5_tts_mlx_amd.weights import F5TTS_335M, synthetic_weights  # noqa: E402

RUNS, WARMUP = 5, 2
POINTS = 32
TEXT_CFGS = (2.0, 1.5, 2.5, 1.0)
AUDIO_CFGS = (3.0, 0.5, 1.0, 2.0)


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
    ws = model.engine.workspace(32, N, bench.NT, POINTS, "euler", rows="dual")     # the largest plan first: no call re-allocates (and drops graphs)
    record(sink, what="workspace", batch=32, plan="dual", bytes=int(ws.numel()))
    for B in (2, 32):
        cond, text, y0, _ = bench.synth_batch(B, first=0, device=dev)
        kw = dict(duration=N, steps=POINTS, method="euler", use_graph=True, y0=y0, sway_sampling_coef=-1.0)
        text_rows = [TEXT_CFGS[i % 4] for i in range(B)]
        audio_rows = [AUDIO_CFGS[i % 4] for i in range(B)]
        legs = {"rows": lambda: f5.sample(cond, text, cfg_strength=text_rows, **kw),
                "dual": lambda: f5.sample(cond, text, cfg_strength=text_rows, audio_cfg_strength=audio_rows, **kw)}
        res = alternate(legs)
        base = res["rows"][len(res["rows"]) // 2]
        for name, ts in res.items():
            record(sink, what="sample", batch=B, frames=N, points=POINTS, precision="f16", leg=name, runs=RUNS,
                   vs_rows=round(ts[len(ts) // 2] / base, 4), graphs_held=model.engine.graph_count(), **stats(ts))
        model.engine.synchronize()
        record(sink, what="status", batch=B, saturation_events=model.engine.saturation_events, range_events=model.engine.range_events)


if __name__ == "__main__":
    main()
