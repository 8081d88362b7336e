"""Cost of the multistep solvers on one GPU (docs/multistep.md; the figures there come from here):
python tools/multistep_cost.py [out.jsonl]

335M shape, N = 937 frames, precision f16, hipGraph replay, synthetic weights and the inputs of bench.py, cfg 2, sway -1; 32 grid
points (31 function evaluations for each of the three), batch 1 and batch 32.  Legs: Euler, ab2, ab3, alternating inside every
repetition in one process; each figure is a host clock around a call that ends in a device synchronise, median / min / max of RUNS
repetitions after WARMUP (the first call of a shape and method captures its graph).  Expected from the code: equal cost within the
run-to-run spread -- an Adams-Bashforth stage reads one or two B N 100 fp32 buffers more than an Euler stage and writes one."""
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

RUNS, WARMUP, POINTS = 5, 2, 32
METHODS = ("euler", "ab2", "ab3")


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    model = DiT.from_config(F5TTS_335M, precision="f16", device=dev)
    model.load_weights(synthetic_weights(F5TTS_335M, seed=42))
    eng = model.engine
    f5 = F5TTS(transformer=model)
    N = bench.N_FRAMES
    eng.workspace(32, N, bench.NT, POINTS, "ab3")              # the largest plan first: no call re-allocates (and drops graphs)
    for B in (1, 32):
        cond, text, y0, _ = bench.synth_batch(B, first=0, device=dev)
        kw = dict(duration=N, steps=POINTS, use_graph=True, y0=y0, sway_sampling_coef=-1.0, cfg_strength=2.0)
        times = {m: [] for m in METHODS}
        for rep in range(WARMUP + RUNS):
            for m in METHODS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f5.sample(cond, text, method=m, **kw)
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times[m].append(time.perf_counter() - t0)
        base = sorted(times["euler"])[RUNS // 2]
        for m in METHODS:
            ts = sorted(times[m])
            line = json.dumps(dict(what="sample", batch=B, frames=N, method=m, points=POINTS, precision="f16", runs=RUNS,
                                   median_ms=round(1e3 * ts[RUNS // 2], 2), min_ms=round(1e3 * ts[0], 2), max_ms=round(1e3 * ts[-1], 2),
                                   vs_euler=round(ts[RUNS // 2] / base, 4)))
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
        eng.synchronize()
        print(json.dumps(dict(what="status", batch=B, saturation_events=eng.saturation_events, range_events=eng.range_events)), flush=True)


if __name__ == "__main__":
    main()
