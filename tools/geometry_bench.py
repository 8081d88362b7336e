"""Timing of a geometry outside the 335M family on one GPU (docs/geometries.md; the figures there come from here):
python tools/geometry_bench.py [out.jsonl]

1. sample() for weights.REF_SMALL (dim 768, inner width 512, 16 conv-pos groups of 48 channels, text 384), precision f16, synthetic
   weights and the inputs of bench.py (3 s reference, 937 frames, 32-point Euler, CFG, hipGraph replay; the text ids taken modulo the
   model's vocabulary of 256), batch 1 and batch 32, with bench.py's own timing: `timed_samples`, a host clock around back-to-back calls
   that ends in a device synchronise.
2. The kernels its four block GEMMs resolve to at both batch sizes, as f5_debug_gemm_route names them (the routing function the
   launcher switches over; nothing is launched).
3. Conv-pos at op level, 2 x 937 tokens (batch 1: both branches), 31 taps, both output modes: the 48-channel kernel at C = 768 next to
   the 64-channel kernels at C = 1024 (f5_convpos_kernel<false,1>, and the ring kernel the automatic route picks there), bench.py's
   `_time_launches`: HIP events around a replayed graph of back-to-back launches."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from f5_tts_mlx_amd import engine as E  # noqa: E402
from f5_tts_mlx_amd.cfm import F5TTS  # noqa: E402
from f5_tts_mlx_amd.dit import DiT  # noqa: E402
from f5_tts_mlx_amd.weights import REF_SMALL, synthetic_weights  # noqa: E402

CALLS = {1: (10, 2), 32: (3, 1)}          # batch -> (timed calls, warm-up calls)
EPI_GELU_TANH, EPI_RESID_GATE, EPI_QKV_ROPE = 2, 4, 5


def record(sink, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def sync():
    torch.cuda.synchronize()


def block_gemm_kernels(lib, cfg, B, N):
    M, inner = 2 * B * N, cfg.inner_dim
    buf = C.create_string_buffer(64)
    out = {}
    for name, epi, n_out, seq_len, bits in (("qkv", EPI_QKV_ROPE, 3 * inner, N, 1), ("out_proj", EPI_RESID_GATE, cfg.dim, 0, 0),
                                             ("ff1", EPI_GELU_TANH, cfg.ff_dim, 0, 0), ("ff2", EPI_RESID_GATE, cfg.dim, 0, 0)):
        n = lib.f5_debug_gemm_route(epi, M, n_out, 1, seq_len, bits, 0, buf, 64, None)
        out[name] = buf.value.decode() if n >= 0 else "refused: " + lib.f5_last_error().decode()
    return out


def convpos_times(lib, dev, sink):
    B, N, taps = 2, bench.N_FRAMES, 31
    buf = C.create_string_buffer(64)
    g = torch.Generator(device=dev).manual_seed(7)
    for Cc, groups, tps, label in ((768, 16, 0, "48 channels per group"), (1024, 16, 1, "64 channels per group, selector 1"),
                                   (1024, 16, 0, "64 channels per group, automatic")):
        cpg = Cc // groups
        rows = lib.f5_op_conv_packed_rows(Cc, cpg)
        x = torch.randn((B * N, Cc), generator=g, device=dev).to(torch.float16)
        w = (torch.randn((rows, taps * 64), generator=g, device=dev) * (taps * cpg) ** -0.5).to(torch.float16)
        if cpg == 48:                                       # the weight store's zero padding: rows and columns 48..63 of every tile
            w4 = w.view(groups, 64, taps, 64)
            w4[:, 48:] = 0
            w4[:, :, :, 48:] = 0
        bias = torch.zeros(Cc, device=dev)
        out16 = torch.empty((B * N, Cc), dtype=torch.float16, device=dev)
        out32 = torch.zeros((B * N, Cc), dtype=torch.float32, device=dev)
        for mode in (0, 1):
            def run():
                s = E.stream_ptr(dev)
                E.check(lib.f5_op_convpos(E.ptr(x), E.ptr(None), E.ptr(w), E.ptr(None), E.ptr(bias), E.ptr(out16 if mode == 0 else None),
                                          E.ptr(None), E.ptr(out32 if mode == 1 else None), B, N, Cc, groups, taps, 1, mode, s))
            E.check(lib.f5_debug_set_convpos_tps(tps))
            try:
                with E.operand_type("f16"):
                    us = [1e3 * bench._time_launches(run, dev, 50) for _ in range(3)]
                    lib.f5_debug_last_convpos_kernel(buf, 64)
            finally:
                E.check(lib.f5_debug_set_convpos_tps(0))
            record(sink, what="convpos", shape=label, C=Cc, groups=groups, tokens=B * N, taps=taps, mode=mode, kernel=buf.value.decode(),
                   us_per_launch=[round(u, 2) for u in us])


def main():
    sink = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    lib = E.load_library()
    cfg = REF_SMALL
    model = DiT.from_config(cfg, precision="f16", device=dev)
    model.load_weights(synthetic_weights(cfg, seed=42))
    f5 = F5TTS(transformer=model)
    for B, (calls, warmup) in CALLS.items():
        cond, text, y0, _ = bench.synth_batch(B, first=0, device=dev)
        text = text % cfg.text_num_embeds
        kw = dict(duration=bench.N_FRAMES, steps=bench.ODE_POINTS, method="euler", cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, use_graph=True)
        runs = []
        for _ in range(3):
            elapsed, out, _ = bench.timed_samples(f5, cond, text, kw, calls, warmup, sync)
            runs.append(round(1e3 * elapsed / calls, 2))
        model.engine.synchronize()
        record(sink, what="sample", config="REF_SMALL", precision="f16", batch=B, frames=bench.N_FRAMES, method="euler", points=bench.ODE_POINTS,
               ms_per_sample=runs, mel_frames_per_s=round(B * bench.N_FRAMES / (min(runs) * 1e-3)), finite=bool(torch.isfinite(out).all()),
               saturation_events=model.engine.saturation_events, block_gemm_kernels=block_gemm_kernels(lib, cfg, B, bench.N_FRAMES))
    convpos_times(lib, dev, sink)


if __name__ == "__main__":
    main()
