"""Cost of the row-isolated duration prediction on one GPU (docs/duration_rows.md; the figures there come from here):
python tools/duration_rows_cost.py [out.jsonl]

The predictor of the checkpoint (dim 512, depth 8, 8 heads, text_dim 512, ff_mult 2, 2 text blocks; synthetic weights), B = 32 references
of 300 ... 900 frames spread evenly over the rows and mixed over the batch, padded to the longest, each with a text of a tenth as many
tokens.  Two legs in one process, the native call `f5_predict_duration` and `f5_predict_duration_rows` on the same inputs, hipGraph
replay, alternating inside every repetition (the order swapped from one repetition to the next); each figure is a host clock around a call
that ends in a device synchronise, median / min / max of RUNS repetitions after WARMUP (the first call of a leg captures its graph).
`padding` is the share of the B x N positions at or past their row's length: what the ragged kernels can skip at most."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from f5_tts_mlx_amd.duration import DurationPredictor, DurationTransformer, row_lengths, synthetic_duration_weights  # noqa: E402

RUNS, WARMUP = 50, 10
B = 32
FRAMES = (300, 900)
PRECISIONS = ("f16", "bf16")
MODEL = dict(dim=512, depth=8, text_num_embeds=2545, text_dim=512, conv_layers=2, ff_mult=2)


def record(sink, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(1e3 * ts[len(ts) // 2], 3), min_ms=round(1e3 * ts[0], 3), max_ms=round(1e3 * ts[-1], 3))


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    lens = [int(v) for v in np.linspace(FRAMES[0], FRAMES[1], B)]
    lens = lens[::2] + lens[1::2][::-1]                      # long and short rows mixed over the batch, the longest not first
    tokens = [n // 10 for n in lens]
    n_in, nt = max(lens), max(tokens)
    r = np.random.default_rng(0)
    mel = torch.from_numpy((r.standard_normal((B, n_in, 100)) * 1.5 - 1.0).astype(np.float32))
    text = torch.from_numpy(r.integers(0, MODEL["text_num_embeds"], (B, nt)).astype(np.int32))
    for b in range(B):
        mel[b, lens[b]:] = 0.0
        text[b, tokens[b]:] = -1
    rows = row_lengths(text, n_in, lens)[2]
    padding = 1.0 - sum(rows) / (B * max(n_in, nt))
    mel_d, lens_t = mel.to(dev), torch.tensor(lens)
    weights = synthetic_duration_weights(seed=5, **MODEL)
    for precision in PRECISIONS:
        dp = DurationPredictor(DurationTransformer(dim=MODEL["dim"], depth=MODEL["depth"], heads=8, text_dim=512, ff_mult=2, conv_layers=2,
                                                   text_num_embeds=MODEL["text_num_embeds"], precision=precision, device=dev))
        dp.load_weights(weights)
        legs = {"plain": lambda: dp.predict_native(mel_d, text, lens=lens_t, use_graph=True),
                "rows": lambda: dp.predict_native(mel_d, text, lens=lens_t, use_graph=True, isolate_rows=True)}
        times = {k: [] for k in legs}
        outs = {}
        for rep in range(WARMUP + RUNS):
            for name in (("plain", "rows") if rep % 2 == 0 else ("rows", "plain")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = legs[name]()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times[name].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for name in ("plain", "rows"):
            record(sink, what="predict_native", call="f5_predict_duration" + ("_rows" if name == "rows" else ""), batch=B, n_in=n_in, nt=nt,
                   min_frames=min(lens), padding=round(padding, 4), precision=precision, vs_plain=round(med[name] / med["plain"], 4),
                   runs=RUNS, **stats(times[name]))
        sec = {k: v[0].cpu() for k, v in outs.items()}
        longest, shortest = lens.index(max(lens)), lens.index(min(lens))
        # how far the mode moves a row's frame count: nothing for the longest (it has no padding)
        record(sink, what="effect", precision=precision, frames_plain=[int(sec["plain"][i] * 93) for i in (longest, shortest)],
               frames_rows=[int(sec["rows"][i] * 93) for i in (longest, shortest)],
               max_rel_change=round(float(((sec["rows"] - sec["plain"]).abs() / sec["plain"]).max()), 4), status=dp.last_status,
               graphs_held=dp.transformer.lib.f5_duration_graph_count(dp.transformer._h))


if __name__ == "__main__":
    main()
