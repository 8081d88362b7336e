"""Cost of vocoding the sentences of one text on one GPU: the per-sentence loop of generate(batch_sentences=True) against one ragged
call (generate(..., vocode_batched=True)).  12 sentences of 12 distinct lengths between 150 and 900 frames, precision f16, HIP events
around each leg, 5 warm-up calls, median of 20.  The figures of docs/vocode_ragged.md come from here:
python tools/vocode_ragged_cost.py

Legs: "loop_graph" is what generate() runs today (Vocos default use_graph=True; 12 lengths through the handle's 8 graph slots, so every
sentence of every call captures and instantiates its graph again), "loop_eager" the same loop with use_graph=False (launch cost
without capture cost), "ragged_graph" / "ragged_eager" one decode(mel, lens=frames) on the padded batch."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f5_tts_mlx_amd.vocos import HOP, Vocos, synthetic_vocos_weights  # noqa: E402

FRAMES = [423, 150, 900, 287, 764, 218, 559, 832, 355, 627, 491, 696]     # 12 distinct lengths, 150 ... 900, in no order
RUNS, WARMUP = 20, 5


def timed(fn):
    for _ in range(WARMUP):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    return out, (ms[RUNS // 2 - 1] + ms[RUNS // 2]) / 2, ms[0], ms[-1]


def main():
    assert len(set(FRAMES)) == 12 and min(FRAMES) == 150 and max(FRAMES) == 900
    w = synthetic_vocos_weights(seed=7)
    B, N = len(FRAMES), max(FRAMES)
    g = torch.Generator(device="cuda").manual_seed(1)
    mel = torch.randn((B, N, 100), device="cuda", generator=g) * 2.0 - 1.0
    for b, f in enumerate(FRAMES):
        mel[b, f:] = float("nan")                                        # what the loop never sees must not matter to the ragged call
    results = {}
    for leg in ("loop_graph", "loop_eager", "ragged_graph", "ragged_eager"):
        voc = Vocos(w, precision="f16", device="cuda:0", use_graph=leg.endswith("graph"))   # one handle (one graph cache) per leg
        if leg.startswith("loop"):
            fn = lambda: torch.cat([voc(mel[i:i + 1, :FRAMES[i]]).reshape(-1) for i in range(B)], dim=0)      # noqa: E731
        else:
            def fn():
                waves = voc(mel, lens=FRAMES)
                return torch.cat([waves[i, :HOP * (FRAMES[i] - 1)] for i in range(B)], dim=0)
        out, med, lo, hi = timed(fn)
        results[leg] = out
        print(json.dumps(dict(leg=leg, sentences=B, frames_total=sum(FRAMES), frames_padded=B * N, graphs_held=voc.graph_count(),
                              median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3))), flush=True)
        del voc
    ref = results["loop_eager"]
    for leg, out in results.items():
        same = bool(torch.equal(out, ref))
        diff = float((out - ref).abs().mean() / ref.abs().mean())
        print(json.dumps(dict(leg=leg, finite=bool(torch.isfinite(out).all()), bit_equal_to_loop_eager=same, mean_rel_diff=diff)), flush=True)


if __name__ == "__main__":
    main()
