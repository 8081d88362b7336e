"""Cost of row isolation on one GPU (docs/isolate_rows.md; the figures there come from here):
python tools/isolate_rows_cost.py [out.jsonl]

335M shape, precision f16, hipGraph replay, synthetic weights and the inputs of bench.py (3 s reference, 281 frames) on a RAGGED batch:
every row generates a sentence of 4 ... 9 s behind its reference, the lengths spread evenly over the rows (656 ... 1124 frames, padded to
the longest), y0 zero past each duration.  32-point Euler and 8-point rk4, batch 32 and batch 8.  Two legs, sample(isolate_rows=True)
and the same call without the argument, alternating inside every repetition; each figure is a host clock around a call that ends in a
device synchronise, median / min / max of RUNS repetitions after WARMUP (the first call of a leg captures its graph).  `padding` is the
share of the B x N frames that lie past their row's duration: what the conv-pos early exit can skip at most."""
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

RUNS, WARMUP = 7, 2
SOLVERS = (("euler", 32), ("rk4", 8))
BATCHES = (32, 8)
REF_FRAMES = 281
FRAMES_PER_SEC = 93.75
SENTENCE_S = (4.0, 9.0)


def durations(B):
    secs = np.linspace(SENTENCE_S[0], SENTENCE_S[1], B)
    d = [REF_FRAMES + int(s * FRAMES_PER_SEC) for s in secs]
    return d[::2] + d[1::2][::-1]                  # long and short rows mixed over the batch, the longest not first


def record(sink, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(1e3 * ts[len(ts) // 2], 2), min_ms=round(1e3 * ts[0], 2), max_ms=round(1e3 * ts[-1], 2))


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    model = DiT.from_config(F5TTS_335M, precision="f16", device=dev)
    model.load_weights(synthetic_weights(F5TTS_335M, seed=42))
    eng = model.engine
    f5 = F5TTS(transformer=model)
    for B in BATCHES:
        durs = durations(B)
        N = max(durs)
        cond, text, _, _ = bench.synth_batch(B, first=0, device=dev)
        y0 = torch.zeros((B, N, 100), dtype=torch.float32)
        for i, d in enumerate(durs):
            y0[i, :d] = torch.from_numpy(np.random.default_rng(3456 + i).standard_normal((100, d)).astype(np.float32).T.copy())
        y0 = y0.to(dev)
        padding = 1.0 - sum(durs) / (B * N)
        for method, points in SOLVERS:
            kw = dict(duration=torch.tensor(durs), steps=points, method=method, use_graph=True, y0=y0, sway_sampling_coef=-1.0)
            legs = {"off": lambda: f5.sample(cond, text, **kw), "on": lambda: f5.sample(cond, text, isolate_rows=True, **kw)}
            times = {k: [] for k in legs}
            outs = {}
            for rep in range(WARMUP + RUNS):
                for name in (("off", "on") if rep % 2 == 0 else ("on", "off")):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[name], _ = legs[name]()
                    torch.cuda.synchronize()
                    if rep >= WARMUP:
                        times[name].append(time.perf_counter() - t0)
            moved = [float((outs["on"][i, REF_FRAMES:d] - outs["off"][i, REF_FRAMES:d]).abs().mean()) for i, d in enumerate(durs)]
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            for name in ("off", "on"):
                record(sink, what="sample", batch=B, frames=N, min_frames=min(durs), padding=round(padding, 4), method=method, points=points,
                       precision="f16", isolate_rows=name, vs_off=round(med[name] / med["off"], 4), runs=RUNS,
                       raw_ms=[round(1e3 * t, 2) for t in times[name]], **stats(times[name]))
            # how far the option moves a row: nothing for the longest (it has no padding), most for the shortest
            record(sink, what="effect", batch=B, method=method, points=points, mean_abs_change_longest=round(moved[durs.index(N)], 8),
                   mean_abs_change_shortest=round(moved[durs.index(min(durs))], 6))
            eng.synchronize()
            record(sink, what="status", batch=B, method=method, saturation_events=eng.saturation_events, range_events=eng.range_events,
                   graphs_held=eng.graph_count())


if __name__ == "__main__":
    main()
