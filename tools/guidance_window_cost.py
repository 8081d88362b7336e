"""Cost of a guidance window on one GPU (docs/guidance_window.md; the figures there come from here):
python tools/guidance_window_cost.py [out.jsonl]

335M shape, N = 937 frames, precision f16, hipGraph replay, synthetic weights and the inputs of bench.py; 32-point Euler and 8-point
rk4, batch 2 and batch 32.  Legs, for single and for dual guidance: the per-row call guided everywhere (f5_sample_rows /
f5_sample_dual), the window call with the full window (the same launches: must cost the same), and windows [-1, hi] that cover about
half and about a quarter of the function evaluations -- the same window for every row, so the evaluations outside it run the
conditional branch alone.  `f` is the fraction of wide evaluations the engine reports (f5_debug_last_sample_pattern); `forwards` the
forward-count ratio the figure is to be read against, (1 + f) / 2 of the guided call's B N-row forwards for single guidance and
(1 + 2 f) / 3 for dual.  The legs alternate inside every repetition; each figure is a host clock around a call that ends in a device
synchronise, median / min / max of RUNS repetitions after WARMUP (the first call of a shape and pattern captures its graph)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from f5_tts_mlx_amd.cfm import F5TTS, time_grid  # noqa: E402
from f5_tts_mlx_amd.dit import DiT  # noqa: E402
from f5_tts_mlx_amd.weights import F5TTS_335M, synthetic_weights  # noqa: E402

RUNS, WARMUP = 5, 2
SOLVERS = (("euler", 32), ("rk4", 8))
TEXT_CFGS = (2.0, 1.5, 2.5, 1.0)
AUDIO_CFGS = (3.0, 0.5, 1.0, 2.0)
PER_STEP = dict(euler=1, midpoint=2, rk4=4)


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


def closing_bound(points, method, fraction):
    """hi of a window [-1, hi] that holds the first round(fraction * nfe) evaluation times of the sway -1 grid: midway between the last
    one inside and the first one outside (the engine's own fp32 times are within an ulp of these; the gap is orders wider)"""
    t = time_grid(points, -1.0).astype(np.float32)
    times = []
    for i in range(points - 1):
        t0, dt = t[i], t[i + 1] - t[i]
        times += {"euler": [t0], "midpoint": [t0, t0 + 0.5 * dt], "rk4": [t0, t0 + 0.5 * dt, t0 + 0.5 * dt, t0 + dt]}[method]
    k = int(round(fraction * len(times)))
    while times[k] == times[k - 1]:           # the two middle stages of rk4 share a time: keep them on one side
        k += 1
    return float(0.5 * (times[k - 1] + times[k]))


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    model = DiT.from_config(F5TTS_335M, precision="f16", device=dev)
    model.load_weights(synthetic_weights(F5TTS_335M, seed=42))
    eng = model.engine
    eng.set_graph_cache(16)                    # eight legs per shape: none evicts another
    f5 = F5TTS(transformer=model)
    N = bench.N_FRAMES
    ws = eng.workspace(32, N, bench.NT, 32, "euler", rows="window_dual")     # the largest plan first: no call re-allocates (and drops graphs)
    record(sink, what="workspace", batch=32, plan="window_dual", bytes=int(ws.numel()))
    for method, points in SOLVERS:
        nfe = (points - 1) * PER_STEP[method]
        windows = {"full": (-1.0, 2.0), "half": (-1.0, closing_bound(points, method, 0.5)), "quarter": (-1.0, closing_bound(points, method, 0.25))}
        for B in (2, 32):
            cond, text, y0, _ = bench.synth_batch(B, first=0, device=dev)
            kw = dict(duration=N, steps=points, method=method, use_graph=True, y0=y0, sway_sampling_coef=-1.0)
            text_rows = [TEXT_CFGS[i % 4] for i in range(B)]
            audio_rows = [AUDIO_CFGS[i % 4] for i in range(B)]
            legs, wide = {}, {}
            for guidance, extra in (("single", {}), ("dual", dict(audio_cfg_strength=audio_rows))):
                legs[guidance + "/rows"] = lambda extra=extra: f5.sample(cond, text, cfg_strength=text_rows, **extra, **kw)
                wide[guidance + "/rows"] = nfe
                for name, w in windows.items():
                    def leg(extra=extra, w=w, key=guidance + "/" + name):
                        f5.sample(cond, text, cfg_strength=text_rows, cfg_interval=w, **extra, **kw)
                        wide[key] = int(eng.last_sample_pattern().sum())
                    legs[guidance + "/" + name] = leg
            res = alternate(legs)
            for name, ts in res.items():
                guidance = name.split("/")[0]
                base = res[guidance + "/rows"]
                f = wide[name] / nfe
                record(sink, what="sample", batch=B, frames=N, method=method, points=points, nfe=nfe, precision="f16", guidance=guidance,
                       leg=name.split("/")[1], wide=wide[name], f=round(f, 4),
                       forwards=round((1 + f) / 2 if guidance == "single" else (1 + 2 * f) / 3, 4),
                       vs_rows=round(ts[len(ts) // 2] / base[len(base) // 2], 4), runs=RUNS, graphs_held=eng.graph_count(), **stats(ts))
            eng.synchronize()
            record(sink, what="status", batch=B, method=method, saturation_events=eng.saturation_events, range_events=eng.range_events)


if __name__ == "__main__":
    main()
