"""Cost of audio.resample on one GPU: HIP events around the call, after warm-up, median of 20 runs, next to the bytes the launch has
to move (input + output + table).  The figures of docs/resample.md come from here:  python tools/resample_cost.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f5_tts_mlx_amd import audio as A  # noqa: E402

B, L, RUNS, WARMUP = 32, 240_000, 20, 5


def main():
    x = torch.randn((B, L), device="cuda")
    for orig, new in ((24_000, 16_000), (44_100, 24_000)):
        taps, first, o, n, T, width = A.resample_table(orig, new)
        for _ in range(WARMUP):
            out = A.resample(x, orig, new)
        torch.cuda.synchronize()
        ms = []
        for _ in range(RUNS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = A.resample(x, orig, new)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        ms.sort()
        med = (ms[RUNS // 2 - 1] + ms[RUNS // 2]) / 2
        nbytes = x.numel() * 4 + out.numel() * 4 + taps.nbytes + first.nbytes
        print(json.dumps(dict(orig=orig, new=new, o=o, n=n, T=T, batch=B, samples_in=L, samples_out=out.shape[1], bytes=nbytes,
                              median_ms=round(med, 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4),
                              gb_per_s=round(nbytes / med / 1e6, 1))))


if __name__ == "__main__":
    main()
