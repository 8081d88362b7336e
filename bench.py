#!/usr/bin/env python
"""bench.py -- F5-TTS 335M flow-matching sampling throughput on MI355X (BASELINE.json metric).

A "step" = one `F5TTS.sample()` call (32-point Euler = 31 updates = 62 DiT forwards with CFG) over a
batch of synthetic 10 s utterances (N = 937 mel frames, SURVEY.md §8(d) inputs), inputs resident in
HBM, output = final mel on device.  value = mel frames produced per second, whole job.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--precision f16|bf16|bf16x3|mxfp8] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line (`ms_per_step` = one timed step).  `--dump-outputs DIR`
writes what the last timed step returned (`out`, `trajectory`) as DIR/<name>.npy, float32, at most 64 MB in all.  Everything else
-- parity against the committed golden, kernel rooflines and the measured MFMA peak, the sub-records (wave-to-wave, batch 32, bf16,
eager, configs[4]) and the CPU baseline -- runs only with `--full` (`--no-sub` / `--no-cpu-baseline` then drop parts of it).

Precision: the headline mode is "f16" (IEEE-half MFMA operands, fp32 everywhere else), the one-pass mode that meets the
1e-3 mel-L1 parity gate; a --full line carries `parity_l1`, the measured distance of the TIMED configuration's output from the fp32
oracle's committed answer for this very workload (tests/golden/full_b1_euler32.npz).  "bf16" (BASELINE's label) is reported
as a sub-record together with its parity figure, which is outside the gate.

Multi-GPU (utterances are independent): `--gpus N` with no launcher environment re-executes itself under
`torch.distributed.run --nproc-per-node N` (rendezvous on 127.0.0.1); under a launcher (WORLD_SIZE set) it is one rank.  One
process per GPU, weights generated on rank 0 and replicated with ONE RCCL broadcast of the weights arena, every rank samples
its own B utterances, no data-path collective ("scaling": "weak").  `--dry-run` runs the same launch / barrier / reduce /
report skeleton on CPU over gloo without touching the engine (what the CPU test suite exercises).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

# hipGraph replay: no per-node packet capture (f5_tts_mlx_amd/__init__.py explains; set here too, ahead of torch's first HIP call)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_FRAMES = 937            # int(10.0 * 93.75), generate.py:23,163
REF_SAMPLES = 72_000      # 3.0 s reference audio -> 281 mel frames
NT = 160
ODE_POINTS = 32
BF16_PEAK_TFLOPS = 2500.0  # dense bf16 / fp16 MFMA peak, MI355X_MICROARCH.md
FP8_PEAK_TFLOPS = 5000.0   # dense fp8 (MX) MFMA peak, MI355X_MICROARCH.md
PARITY_TOL = 1e-3
DUMP_BYTES = 64 << 20      # --dump-outputs: budget of all files together
GOLDEN = os.path.join(ROOT, "tests", "golden", "full_b1_euler32.npz")
DTYPE_TEXT = {
    "f16": "f16 (IEEE-half MFMA operands, fp32 accumulate / residual stream / LayerNorm / softmax state; meets the 1e-3 gate)",
    "bf16": "bf16 (bfloat16 MFMA operands; outside the 1e-3 parity gate, see parity_l1)",
    "bf16x3": "bf16x3 (split-bf16 operands, 3 MFMA passes, fp32-class)",
    "mxfp8": "mxfp8 (OCP e4m3 + E8M0 block scales for the four per-block GEMMs; attention and the rest bf16)",
}


def flops_forward(N: int, hoisted: bool) -> float:
    """Algorithmic flops of one DiT utterance-forward, SURVEY.md §8(d).  hoisted=True drops the work the engine
    runs once per sample instead of once per forward (text path, adaLN/time linears, cond/text input proj)."""
    blocks = 22 * (N * 2 * (4 * 1024 ** 2 + 2 * 1024 * 2048) + 4 * N ** 2 * 1024)
    conv = 2 * N * 2 * 31 * 64 * 1024
    out = N * 2 * 1024 * 100
    if hoisted:
        return blocks + conv + out + N * 2 * 128 * 1024
    ada = 22 * 2 * 1024 * 6144 + 2 * 1024 * 2048 + 2 * (256 * 1024 + 1024 ** 2)
    text = 4 * N * (2 * 2 * 512 * 1024 + 2 * 7 * 512)
    return blocks + conv + out + N * 2 * 712 * 1024 + ada + text


def synth_waves(B: int, first: int) -> np.ndarray:
    return np.stack([np.random.default_rng(1234 + i).standard_normal(REF_SAMPLES).astype(np.float32) * np.float32(0.1)
                     for i in range(first, first + B)])


def synth_batch(B: int, first: int, device):
    """SURVEY §8(d) inputs for utterances [first, first + B): reference mel (through the HIP mel front-end, one launch for the
    batch), text ids, injected noise; also returns the raw reference waves (device) for the wave -> wave timing."""
    from f5_tts_mlx_amd.audio import log_mel_spectrogram
    waves = torch.from_numpy(synth_waves(B, first)).to(device)
    cond = log_mel_spectrogram(waves)                                    # (B, 281, 100) on device
    text = torch.from_numpy(np.stack([np.random.default_rng(2345 + i).integers(0, 2545, NT).astype(np.int32)
                                      for i in range(first, first + B)])).to(device)
    y0 = torch.from_numpy(np.ascontiguousarray(np.stack(
        [np.random.default_rng(3456 + i).standard_normal((100, N_FRAMES)).astype(np.float32).T for i in range(first, first + B)]))).to(device)
    return cond, text, y0, waves


# ------------------------------------------------------------------------------------------------
# roofline: live HIP-event timing of the dominant kernels at the bench shape
# ------------------------------------------------------------------------------------------------
def _time_launches(run, dev, iters: int) -> float:
    """Average duration (ms) of `iters` back-to-back launches of `run`, replayed from a hipGraph (as the kernel runs inside
    sample(): no host launch gaps), timed with HIP events on the stream the graph is launched on."""
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(iters):
            run()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


class ClockPowerSampler:
    """rocm-smi polled from a thread while the GPU works (best effort: absent or unreadable rocm-smi -> no record).  Batch 32 runs at the
    board's power cap -- the clock, not the schedule, sets its time (profiles/r06/power_probe_real_vs_zero_operands.jsonl) -- so the line
    carries the clock and power its numbers were measured at.  Polling costs host CPU only."""

    def __init__(self):
        import shutil
        self.exe = shutil.which("rocm-smi")
        self.samples, self._stop, self._th = [], False, None

    def _poll(self):
        import re
        import subprocess
        while not self._stop:
            try:
                out = subprocess.run([self.exe, "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=5).stdout
                card = next(iter(json.loads(out).values()))
                sclk = next((v for k, v in card.items() if "sclk" in k.lower()), None)
                pw = next((v for k, v in card.items() if "power" in k.lower() and "(w)" in k.lower()), None)
                mhz = re.search(r"(\d+)\s*mhz", str(sclk), re.I)
                if mhz and pw is not None:
                    self.samples.append((int(mhz.group(1)), float(pw)))
            except Exception:   # noqa: BLE001
                pass
            time.sleep(0.2)

    def __enter__(self):
        if self.exe:
            import threading
            self._th = threading.Thread(target=self._poll, daemon=True)
            self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._th is not None:
            self._th.join(timeout=10)
        return False

    def summary(self):
        s = self.samples[1:] if len(self.samples) > 2 else self.samples       # (the first sample may predate the load)
        if not s:
            return None
        import statistics
        return dict(sclk_mhz_median=statistics.median(x[0] for x in s), power_w_median=statistics.median(x[1] for x in s), samples=len(s),
                    source="rocm-smi --showclocks --showpower, polled every 0.2 s while the timed calls ran")


def mfma_peak_measured(precision: str, dev) -> dict:
    """The MFMA rate this box delivers right now, measured ("print the measured MFMA micro-benchmark peak you
    divide by"): f5_op_mfma_peak = every wave of 1 024 workgroups streams v_mfma_f32_32x32x16 on register operands, no memory
    traffic -- once on lane-constant registers (what zero-filled benchmarks see) and once on workload-like operand registers that
    change from MFMA to MFMA (the delivered clock depends on how many operand bits toggle, MI355X_MICROARCH.md "DVFS give-back").
    `frac` in the roofline records keeps the data-sheet 2.5 PF denominator; `frac_of_measured` divides by the workload-like figure.
    Round 6: the loop now has eight INDEPENDENT accumulators (until round 5 every other MFMA waited for its predecessor and the figure
    was that chain's rate, ~1 340 TF, not the pipe's: ~1 650 TF on the same values) and runs ~0.4 s per figure, long enough for the
    clock to settle where the power management holds it (csrc/rowops.hip mfma_peak_kernel, profiles/r06/mfma_energy_probe.jsonl)."""
    import ctypes as C
    from f5_tts_mlx_amd import engine as E
    lib = E.load_library()
    opd = E.operand_dtype(precision)
    sink = torch.zeros(4, device=dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    ops = torch.randn(16 * 64 * 8, generator=g).to(dev).to(opd)
    out = {}
    with E.operand_type(precision):
        for key, operands in (("constant_operands", None), ("workload_like_operands", ops)):
            fl = C.c_double()
            run = lambda: E.check(lib.f5_op_mfma_peak(E.ptr(operands), 1024, 20000, E.ptr(sink), C.byref(fl), E.stream_ptr(dev)))   # noqa: E731
            best = None
            for _ in range(2):
                run()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(6):
                    run()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / 6
                best = ms if best is None else min(best, ms)
            out[key] = fl.value / (best * 1e-3) / 1e12
    return out


def _pmc_traffic(key: str, shape: str, precision: str):
    """HBM/fabric bytes per launch from the last committed rocprofv3 --pmc passes (profiles/pmc_traffic.json: FETCH_SIZE and
    WRITE_SIZE, separate passes, collected by tools/gpu_pmc_ops.sh), if there is an entry for this kernel, shape and precision."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        for e in pm.get("entries", []):
            if e.get("key") == key and e.get("shape") == shape and e.get("precision") == precision:
                return e["fetch_bytes_corrected_x2"] + e["write_bytes"]
    except Exception:
        pass
    return None


def kernel_rooflines(precision: str, dev, B: int, iters: int = 20, peak_meas: dict | None = None):
    """Live timing of the five kernels that make up a DiT block (>= 95 % of sample() time), each launched through its C-ABI op entry
    point at the bench shape M = 2*B*N rows (cond + null branch), from a hipGraph, HIP events around `iters` launches.
    `share` = launches per block x average time / block total; the entry with the largest share is the dominant kernel."""
    from f5_tts_mlx_amd import engine as E
    lib = E.load_library()
    peak_meas = peak_meas or mfma_peak_measured(precision, dev)
    M, D, FF, H = 2 * B * N_FRAMES, 1024, 2048, 16
    npad = (N_FRAMES + 63) // 64 * 64
    nseg = 3 if precision == "bf16x3" else 1
    opd = E.operand_dtype(precision)
    g = torch.Generator(device="cpu").manual_seed(0)
    # operand statistics of the real workload (activations ~N(0,1), weights ~N(0,1/fan_in)): data toggling sets the
    # DVFS clock, so a microbenchmark on hotter random data would not agree with the in-graph rocprof average
    mk = lambda std, *s: (torch.randn(*s, generator=g) * std).to(dev).to(opd)
    lo = (lambda t: t) if nseg == 3 else (lambda t: None)      # one-pass modes have no "lo" operands / outputs
    P, st = E.ptr, (lambda: E.stream_ptr(dev))
    x1, x1l, x2, x2l = mk(1.0, M, D), mk(0.004, M, D), mk(1.0, M, FF), mk(0.004, M, FF)
    wq, wql = mk(D ** -0.5, 3 * D, D), mk(1e-4, 3 * D, D)
    wo, wol = mk(D ** -0.5, D, D), mk(1e-4, D, D)
    w1, w1l = mk(D ** -0.5, FF, D), mk(1e-4, FF, D)
    w2, w2l = mk(FF ** -0.5, D, FF), mk(1e-4, D, FF)
    bq, b1, bd, gate = torch.zeros(3 * D, device=dev), torch.zeros(FF, device=dev), torch.zeros(D, device=dev), torch.full((D,), 0.5, device=dev)
    cos_t, sin_t = torch.ones(N_FRAMES, 32, device=dev), torch.zeros(N_FRAMES, 32, device=dev)
    qk = [torch.empty(M, 2 * D, dtype=opd, device=dev) for _ in range(2)]
    vt = [torch.zeros(2 * B * H, 64, npad, dtype=opd, device=dev) for _ in range(2)]
    ao = [torch.empty(M, D, dtype=opd, device=dev) for _ in range(2)]
    ffh = [torch.empty(M, FF, dtype=opd, device=dev) for _ in range(2)]
    xres = torch.zeros(M, D, device=dev)
    # LN fold (engine option "ln_fold", default -1 = on from 22 000 rows in the one-pass modes): sample() then runs the residual GEMMs with
    # the x (1 + s) operand / row-sum outputs and QKV / FF1 with the folded epilogue -- time (and count the bytes of) those launches
    folded = nseg == 1 and M >= 22000
    if folded:
        fscale = torch.zeros(D, device=dev)
        fstats = torch.zeros(D // 64, M, 2, device=dev)
        frowf = torch.ones(M, 2, device=dev)
        fh16 = torch.zeros(M, D, dtype=opd, device=dev)
        fshift = torch.zeros(M, device=dev)           # the row shift of the folded operand (the previous LayerNorm's mean)
        fc = {n: (torch.zeros(n, device=dev), torch.zeros(n, device=dev)) for n in (3 * D, FF)}

    class _fold:                                      # the op-level hooks are process-wide switches: set around ONE launch
        def __init__(self, kind, n=0):
            self.kind, self.n = kind, n

        def __enter__(self):
            if folded and self.kind == "producer":
                E.check(lib.f5_debug_set_op_fold_producer(P(fscale), P(fh16), P(fstats), P(fshift)))
            elif folded:
                E.check(lib.f5_debug_set_op_fold_consumer(P(frowf), P(fc[self.n][0]), P(fc[self.n][1])))

        def __exit__(self, *a):
            if folded and self.kind == "producer":
                E.check(lib.f5_debug_set_op_fold_producer(P(None), P(None), P(None), P(None)))
            elif folded:
                E.check(lib.f5_debug_set_op_fold_consumer(P(None), P(None), P(None)))

    def k_qkv():
        with _fold("consumer", 3 * D):
            _k_qkv()

    def k_out():
        with _fold("producer"):
            _k_out()

    def k_ff1():
        with _fold("consumer", FF):
            _k_ff1()

    def k_ff2():
        with _fold("producer"):
            _k_ff2()

    def _k_qkv():
        E.check(lib.f5_op_qkv_rope(P(x1), P(lo(x1l)), P(wq), P(lo(wql)), P(bq), P(cos_t), P(sin_t), P(qk[0]), P(lo(qk[1])), P(vt[0]),
                                   P(lo(vt[1])), 2 * B, N_FRAMES, npad, H, D, nseg, st()))

    def k_attn():
        import ctypes as C
        E.check(lib.f5_op_attention(P(qk[0]), P(lo(qk[1])), P(vt[0]), P(lo(vt[1])), P(ao[0]), P(lo(ao[1])), P(None), 2 * B, H, N_FRAMES,
                                    npad, D, C.c_float(0.125), int(nseg == 3), st()))

    def _k_out():
        E.check(lib.f5_op_gemm_resid_gate(P(x1), P(lo(x1l)), P(wo), P(lo(wol)), P(bd), P(gate), P(None), P(xres), M, D, D, D, D, D, nseg, st()))

    def _k_ff1():
        E.check(lib.f5_op_gemm(P(x1), P(lo(x1l)), P(w1), P(lo(w1l)), P(b1), P(None), P(ffh[0]), P(lo(ffh[1])), M, FF, D, D, D, FF, nseg, 2, st()))

    def _k_ff2():
        E.check(lib.f5_op_gemm_resid_gate(P(x2), P(lo(x2l)), P(w2), P(lo(w2l)), P(bd), P(gate), P(None), P(xres), M, D, FF, FF, FF, D, nseg, st()))

    fold_bytes = (2 * M * D + 8 * M * (D // 64)) if folded else 0      # producer: + the 16-bit (x - m)(1 + s) operand and the slice statistics
    specs = [
        ("qkv_gemm", "QKV projection GEMM + bias + RoPE + head split (f5_gemm*_kernel<EPI_QKV_ROPE>)", k_qkv, 2.0 * M * D * 3 * D,
         f"M={M} N={3 * D} K={D}", 2 * M * D + 2 * 3 * D * D + 2 * M * 3 * D),
        ("attention", "flash attention, 16 heads x 64 (f5_attn*_kernel)", k_attn, 4.0 * 2 * B * H * N_FRAMES * N_FRAMES * 64,
         f"B={2 * B} H={H} N={N_FRAMES} d=64", 2 * 3 * M * D + 2 * M * D),
        ("out_proj_gemm", "attention out-projection GEMM + gated fp32 residual update (f5_gemm*_kernel<EPI_RESID_GATE>, K=1024)", k_out,
         2.0 * M * D * D, f"M={M} N={D} K={D}", 2 * M * D + 2 * D * D + 8 * M * D + fold_bytes),
        ("ff1_gemm", "FF1 GEMM + bias + GELU-tanh (f5_gemm*_kernel<EPI_GELU_TANH>)", k_ff1, 2.0 * M * D * FF, f"M={M} N={FF} K={D}",
         2 * M * D + 2 * D * FF + 2 * M * FF),
        ("ff2_gemm", "FF2 GEMM + gated fp32 residual update (f5_gemm*_kernel<EPI_RESID_GATE>, K=2048)", k_ff2, 2.0 * M * FF * D,
         f"M={M} N={D} K={FF}", 2 * M * FF + 2 * D * FF + 8 * M * D + fold_bytes),
    ]
    out = []
    import ctypes as C
    # sample() folds softmax_scale * log2(e) into q in the QKV epilogue (single-segment operand modes); time the same kernels
    lib.f5_debug_set_op_q_premul(C.c_float(0.125 * 1.4426950408889634 if nseg == 1 else 0.0))
    # ... and hands the QKV projection the pair-major rotation tables (256x256 kernel: transposed q / k tiles)
    tt = [torch.empty(64 * N_FRAMES, device=dev) for _ in range(2)]
    E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), N_FRAMES, 64,
                                   C.c_float(0.125 * 1.4426950408889634 if nseg == 1 else 1.0), st()))
    E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0]), P(tt[1])))
    with E.operand_type(precision):
        k_qkv()                                        # q / k / V^T hold real values before attention is timed
        for key, name, fn, flops, shape, alg_bytes in specs:
            ms = _time_launches(fn, dev, iters)
            ach = flops / (ms * 1e-3) / 1e12
            out.append(dict(key=key, bound="mfma", kernel=name, shape=shape, avg_launch_ms=ms, achieved=ach, peak=BF16_PEAK_TFLOPS,
                            unit="TFLOP/s", frac=ach / BF16_PEAK_TFLOPS, peak_measured_tflops=peak_meas["workload_like_operands"],
                            peak_measured_constant_operands_tflops=peak_meas["constant_operands"],
                            frac_of_measured=ach / peak_meas["workload_like_operands"], traffic=_pmc_traffic(key, shape, precision),
                            traffic_unit="bytes/launch (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE)", algorithmic_bytes=alg_bytes,
                            algorithmic_flops=flops, ln_fold=bool(folded)))
    lib.f5_debug_set_op_q_premul(C.c_float(0.0))
    E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
    total = sum(k["avg_launch_ms"] for k in out)
    for k in out:
        k["share_of_block"] = k["avg_launch_ms"] / total
    # the residual-update GEMM template runs twice per block (out-proj + FF2): as ONE kernel symbol it is the dominant entry of the
    # rocprofv3 --stats CSV at batch 1; report the symbol-level share too
    sym = {"f5_gemm*_kernel<EPI_RESID_GATE>": sum(k["avg_launch_ms"] for k in out if k["key"] in ("out_proj_gemm", "ff2_gemm")) / total}
    for k in out:
        if k["key"] not in ("out_proj_gemm", "ff2_gemm"):
            sym[k["key"]] = k["share_of_block"]
    return out, sym


def gemm_roofline_f8(dev, B: int, iters: int = 20):
    """mxfp8 mode: the QKV projection runs on f5_gemm256f8_kernel (MX-fp8 operands, v_mfma_scale_f32_32x32x64_f8f6f4).  Timed
    here through f5_op_gemm_f8 with the plain bf16-output epilogue (same main loop and output bytes; the RoPE / head-split
    epilogue of the in-engine launch is not exported as an op), operands quantised from workload-like data."""
    from f5_tts_mlx_amd import engine as E
    lib = E.load_library()
    M, D = 2 * B * N_FRAMES, 1024
    g = torch.Generator(device="cpu").manual_seed(0)
    a = (torch.randn(M, D, generator=g)).to(dev)
    w = (torch.randn(3 * D, D, generator=g) * D ** -0.5).to(dev)
    a8, asc = torch.empty(M, D, dtype=torch.uint8, device=dev), torch.empty(M, D // 32, dtype=torch.uint8, device=dev)
    w8, wsc = torch.empty(3 * D, D, dtype=torch.uint8, device=dev), torch.empty(3 * D, D // 32, dtype=torch.uint8, device=dev)
    st = E.stream_ptr(dev)
    E.check(lib.f5_op_quantize_mx(E.ptr(a), D, E.ptr(a8), D, E.ptr(asc), M, D, st))
    E.check(lib.f5_op_quantize_mx(E.ptr(w), D, E.ptr(w8), D, E.ptr(wsc), 3 * D, D, st))
    bias = torch.zeros(3 * D, device=dev)
    out = torch.empty(M, 3 * D, dtype=torch.bfloat16, device=dev)

    def run():
        E.check(lib.f5_op_gemm_f8(E.ptr(a8), E.ptr(asc), E.ptr(w8), E.ptr(wsc), E.ptr(bias), E.ptr(None), E.ptr(None), E.ptr(None),
                                  E.ptr(out), E.ptr(None), E.ptr(None), M, 3 * D, D, D, D, 3 * D, 1, E.stream_ptr(dev)))
    ms = _time_launches(run, dev, iters)
    achieved = 2.0 * M * D * 3 * D / (ms * 1e-3) / 1e12
    return dict(key="qkv_gemm_f8", bound="mfma", kernel="QKV-shaped MX-fp8 GEMM + bias, bf16 out (f5_gemm256f8_kernel<EPI_BF16>)",
                shape=f"M={M} N={3 * D} K={D}", avg_launch_ms=ms, achieved=achieved, peak=FP8_PEAK_TFLOPS, unit="TFLOP/s",
                frac=achieved / FP8_PEAK_TFLOPS, traffic=None, traffic_unit="bytes/launch",
                algorithmic_bytes=M * D + 3 * D * D + (M + 3 * D) * D // 32 + 2 * M * 3 * D)


# ------------------------------------------------------------------------------------------------
# CPU baseline (the oracle; checker / baseline leg only)
# ------------------------------------------------------------------------------------------------
def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(weights, budget_s: float = 25.0):
    """The oracle (CPU restatement of the reference, kind="port") timed on the host cores on a bounded sample: full-size
    fp32 DiT forwards at N=937 (B=1), first a short sweep over thread counts (one forward each), then the best setting is
    timed again; extrapolated to the 62 forwards of a 32-point Euler solve.  ~10-30 s of CPU work in total."""
    from oracle import f5_oracle as O   # checker / baseline leg only
    from f5_tts_mlx_amd.weights import F5TTS_335M
    orc = O.DiTOracle(F5TTS_335M, weights)
    r = np.random.default_rng(0)
    x = torch.from_numpy(r.standard_normal((1, N_FRAMES, 100)).astype(np.float32))
    cond = torch.zeros((1, N_FRAMES, 100))
    cond[:, :281] = torch.from_numpy(r.standard_normal((1, 281, 100)).astype(np.float32))
    text = torch.from_numpy(r.integers(0, 2545, (1, NT)).astype(np.int32))
    ncpu = os.cpu_count() or 1
    cands = [c for c in (8, 16, 32, 64) if c <= ncpu] or [ncpu]   # BLAS at these sizes stops scaling (and collapses) beyond ~32 threads
    t_start = time.perf_counter()
    best, sweep = None, {}
    orc.forward(x[:, :256], cond[:, :256], text, torch.tensor(0.3), False, False, None)    # warm the allocator / thread pool
    for c in cands:
        torch.set_num_threads(c)
        t0 = time.perf_counter()
        orc.forward(x, cond, text, torch.tensor(0.3), False, False, None)
        sweep[c] = time.perf_counter() - t0
        if best is None or sweep[c] < sweep[best]:
            best = c
        if sweep[c] > 1.25 * sweep[best] or time.perf_counter() - t_start > budget_s:
            break
    torch.set_num_threads(best)
    n_rep, t0 = 0, time.perf_counter()
    while n_rep < 2 or (time.perf_counter() - t_start < budget_s and n_rep < 4):
        orc.forward(x, cond, text, torch.tensor(0.3), bool(n_rep % 2), bool(n_rep % 2), None)
        n_rep += 1
    dt = (time.perf_counter() - t0) / n_rep
    n_fwd = 2 * (ODE_POINTS - 1)
    return dict(value=N_FRAMES / (n_fwd * dt), unit="mel-frames/s", cores=best, kind="port",
                sample=f"{n_rep} full-size fp32 DiT forwards (B=1, N={N_FRAMES}) of the oracle on torch-CPU with {best} threads "
                       f"(sweep s/forward: {dict((k, round(v, 2)) for k, v in sweep.items())}), {dt:.2f} s each, "
                       f"extrapolated x{n_fwd} forwards per utterance",
                rtf=10.0 / (n_fwd * dt), host_cpus=ncpu, cpu_model=_cpu_model())


# ------------------------------------------------------------------------------------------------
# launch helpers
# ------------------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def relaunch_under_torchrun(ngpus: int) -> None:
    """`python bench.py --gpus N` with no launcher environment: become N ranks on this node (one per GPU) under
    torch.distributed.run, rendezvous on 127.0.0.1 (the container hostname may not resolve)."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ngpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    os.execve(sys.executable, cmd, env)


def parity_against_golden(out_utt0: torch.Tensor, args) -> dict | None:
    """mel L1 of utterance 0 of the timed configuration vs the fp32 oracle's committed answer for the same utterance and solver
    (tests/golden/make_fullsize_golden.py: 32-point Euler = configs[1] / [2], 16-point midpoint = configs[4])."""
    path = GOLDEN if (args.method == "euler" and args.ode_points == ODE_POINTS) else os.path.join(
        os.path.dirname(GOLDEN), f"full_b1_{args.method}{args.ode_points}.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    l1 = float(np.abs(out_utt0.detach().cpu().numpy().astype(np.float64) - g["out"].astype(np.float64)).mean())
    n_fwd = 2 * {"euler": 1, "midpoint": 2, "rk4": 4}[args.method] * (args.ode_points - 1)
    return dict(parity_l1=l1, parity_gate=PARITY_TOL, parity_ok=bool(l1 <= PARITY_TOL),
                parity_ref=f"fp32 CPU oracle, tests/golden/{os.path.basename(path)} (bench utterance 0, {n_fwd} forwards)")


def timed_samples(f5, cond, text, kw, steps, warmup, barrier):
    """-> (seconds of the `steps` timed calls, out and trajectory of the last call)"""
    out = traj = None
    for _ in range(warmup):
        out, traj = f5.sample(cond, text, **kw)
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out, traj = f5.sample(cond, text, **kw)
    barrier()
    return time.perf_counter() - t0, out, traj


def dump_outputs(dirname: str, arrays: dict) -> dict:
    """--dump-outputs: each array as DIR/<name>.npy in float32, in order, within DUMP_BYTES together.  An array larger than the budget
    left is written as a fixed sample of its flattened elements (indices drawn from default_rng(0), sorted) to DIR/<name>_sample.npy,
    so that two builds run with the same arguments write comparable files.  Returns {file name: shape written}."""
    os.makedirs(dirname, exist_ok=True)
    left, written = DUMP_BYTES, {}
    for name, t in arrays.items():
        t = torch.as_tensor(t).detach().to(torch.float32)
        cap = left // 4
        if t.numel() > cap:
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), cap))
            t, name = t.reshape(-1)[torch.from_numpy(idx).to(t.device)], name + "_sample"
        a = t.cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a)
        left -= a.nbytes
        written[name + ".npy"] = list(a.shape)
    return written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None,
                    help="utterances per GPU.  Default: 1 on one GPU (BASELINE configs[1]); 32 per GPU when --gpus > 1 "
                         "(BASELINE configs[3]: batch 256 sharded over 8 GPUs, weak scaling at 32 / GPU)")
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "bf16x3", "mxfp8"])
    ap.add_argument("--vocoder", action="store_true", help="put the Vocos vocoder (random-init) into the HEADLINE timed region")
    ap.add_argument("--config", default=None, choices=["c5"],
                    help="c5 = BASELINE configs[4]: MX-fp8 block GEMMs + Vocos, 16-point midpoint, batch 32")
    ap.add_argument("--method", default="euler")
    ap.add_argument("--ode-points", type=int, default=ODE_POINTS)
    ap.add_argument("--weights", default=os.environ.get("F5_WEIGHTS"),
                    help="directory of a REAL checkpoint (model_v1.safetensors + vocab.txt, as F5TTS.from_pretrained reads it; "
                         "default $F5_WEIGHTS): timed instead of the seeded synthetic weights (SURVEY.md section 8(d)).  The parity figure "
                         "against the committed golden applies to the synthetic weights only and is omitted then; "
                         "tools/real_checkpoint_parity.py measures the drift of a real checkpoint against the oracle")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-sub", action="store_true", help="skip the sub-records (batch 32, bf16, wave-to-wave RTF)")
    ap.add_argument("--dry-run", action="store_true", help="CPU / gloo: launch, barrier, reduce and report only (no engine)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, <= 64 MB in all; rank 0's shard)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: parity against the golden, kernel rooflines and the measured MFMA "
                         "peak, the sub-records (unless --no-sub) and the CPU baseline (unless --no-cpu-baseline)")
    args = ap.parse_args()
    batch_explicit = args.batch is not None
    if args.config == "c5":
        args.precision, args.vocoder, args.method, args.ode_points = "mxfp8", True, "midpoint", 16
        if not batch_explicit:
            args.batch = 32
    if args.batch is None:
        # the multi-GPU line is BASELINE configs[3] (32 utterances per GPU, weak scaling); the single-GPU line configs[1] (batch 1)
        args.batch = 32 if max(args.gpus, int(os.environ.get("WORLD_SIZE", "1"))) > 1 else 1

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args.gpus)                 # does not return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = world > 1
    dist = None
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dry_run:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    ranks_in_group = dist.get_world_size() if dist_on else 1       # asked of the communicator, not read from the environment
    B = args.batch

    def barrier():
        if not args.dry_run:
            torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        if not args.dry_run:
            torch.cuda.synchronize()

    def max_over_ranks(x: float) -> float:
        if not dist_on:
            return x
        tt = torch.tensor([x], dtype=torch.float64, device="cpu" if args.dry_run else f"cuda:{local}")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    if args.dry_run:
        # same skeleton, no GPU: a "step" is a small CPU matmul; proves the N-rank launch path and the report fields
        a = torch.randn(256, 256, generator=torch.Generator().manual_seed(0))
        for _ in range(args.warmup):
            a = torch.tanh(a @ a.T / 256)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            a = torch.tanh(a @ a.T / 256)
        barrier()
        mine = time.perf_counter() - t0
        elapsed = max_over_ranks(mine)
        fastest = -max_over_ranks(-mine)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, {"out": a})
        if rank == 0:
            ms = elapsed / args.steps * 1e3
            print(json.dumps({"metric": "mel_frames_per_sec", "value": world * B * N_FRAMES / (ms * 1e-3), "unit": "mel-frames/s",
                              "n_gpus": world, "gpus_arg": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
                              "rank_ms_min": fastest / args.steps * 1e3, "rank_ms_max": ms, "ranks_seen_by_rccl": ranks_in_group,
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "dry-run (CPU, gloo)",
                              "data": "dry run: no engine, no GPU", "config": {"workload": "dry-run launch skeleton", "global_batch": world * B,
                                                                              "seq_len": N_FRAMES, "parallelism": f"dp{world} (utterance sharding)"}}))
        if dist_on:
            dist.destroy_process_group()
        return

    from f5_tts_mlx_amd.cfm import F5TTS
    from f5_tts_mlx_amd.dit import DiT
    from f5_tts_mlx_amd.weights import F5TTS_335M, synthetic_weights
    device = torch.device(f"cuda:{local}")
    torch.cuda.set_device(device)

    def make_model(precision):
        m = DiT.from_config(F5TTS_335M, precision=precision, device=device)
        if os.environ.get("F5_BENCH_LN_FOLD") is not None:             # A/B runs under a profiler (tools/gpu_r6_prof_b1.sh); default: the engine's own
            m.engine.set_option("ln_fold", int(os.environ["F5_BENCH_LN_FOLD"]))
        return m

    weights = None
    t_w = time.perf_counter()
    real = args.weights is not None
    if real:
        # a real checkpoint: rank 0 goes through F5TTS.from_pretrained (cfm.py:404-520: upstream key renames, conv layouts, vocab), the
        # other ranks build the same empty model and receive the arena by the broadcast below
        if not os.path.isdir(args.weights):
            raise SystemExit(f"--weights / $F5_WEIGHTS: {args.weights!r} is not a directory")
        if rank == 0:
            model = F5TTS.from_pretrained(args.weights, precision=args.precision, device=str(device), vocoder_name_or_path=None).transformer
            from safetensors.numpy import load_file
            from f5_tts_mlx_amd.weights import convert_upstream_weights
            wf = load_file(os.path.join(args.weights, "model_v1.safetensors"))
            weights = {k: np.asarray(v, np.float32) for k, v in (convert_upstream_weights(wf) if any(k.startswith("ema_model.") for k in wf) else wf).items()}
        else:
            model = make_model(args.precision)
    else:
        model = make_model(args.precision)
        if rank == 0:
            weights = synthetic_weights(F5TTS_335M, seed=42)
            model.load_weights(weights)
    bcast_ms = None
    if dist_on:
        from f5_tts_mlx_amd.dist import broadcast_weights
        bcast_ms = broadcast_weights(model.engine, src=0)
    load_s = time.perf_counter() - t_w

    vocoder = None
    if args.vocoder or (args.full and not args.no_sub):
        from f5_tts_mlx_amd.vocos import Vocos, synthetic_vocos_weights
        vocoder = Vocos(synthetic_vocos_weights(seed=7), precision=args.precision if args.precision != "mxfp8" else "bf16", device=device)
    f5 = F5TTS(transformer=model, vocoder=vocoder.decode if args.vocoder else None)
    cond, text, y0, waves = synth_batch(B, first=rank * B, device=device)
    kw = dict(duration=N_FRAMES, steps=args.ode_points, method=args.method, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0,
              use_graph=not args.no_graph)

    elapsed, out, traj = timed_samples(f5, cond, text, kw, args.steps, args.warmup, barrier)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"out": out, "trajectory": traj})
    del traj
    rank_elapsed = elapsed
    elapsed = max_over_ranks(elapsed)
    rank_ms_min = -max_over_ranks(-rank_elapsed) / args.steps * 1e3        # the fastest rank (diagnosis of a scaling run: a slow GPU / link
    rank_ms_max = elapsed / args.steps * 1e3                               # shows as a spread, a collective problem as both high)
    model.engine.synchronize()                                             # resolves pending status checks (LN-fold operand range)
    assert torch.isfinite(out).all()

    if rank == 0:
        per = {"euler": 1, "midpoint": 2, "rk4": 4}[args.method]
        n_fwd = 2 * per * (args.ode_points - 1)
        fwd_exec, fwd_ref = flops_forward(N_FRAMES, hoisted=True), flops_forward(N_FRAMES, hoisted=False)

        def summarize(ms_per_step, nb, nworld=1):
            tf = nworld * nb * n_fwd * fwd_exec / 1e12 / (ms_per_step * 1e-3)
            return dict(ms_per_step=ms_per_step, value=nworld * nb * N_FRAMES / (ms_per_step * 1e-3), unit="mel-frames/s",
                        rtf_mel_only=nworld * nb * 10.0 / (ms_per_step * 1e-3), whole_path_tflops=tf,
                        whole_path_frac_of_bf16_peak=tf / (nworld * BF16_PEAK_TFLOPS))

        ms_per_step = elapsed / args.steps * 1e3
        head = summarize(ms_per_step, B, world)
        rec = {
            "metric": "mel_frames_per_sec", "value": head["value"], "unit": "mel-frames/s", "n_gpus": world, "gpus_arg": args.gpus,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE_TEXT[args.precision],
            "data": ("REAL checkpoint " + os.path.abspath(args.weights) + ", synthetic inputs (white-noise reference audio, random token ids)") if real
                    else "synthetic (seeded random-init 335M weights, white-noise reference audio, random token ids)",
            "config": {"workload": f"{'BASELINE configs[4]' if (args.config == 'c5' and B == 32 and world == 1) else ('BASELINE configs[3] (32 utterances / GPU, weak scaling)' if (world > 1 and B == 32) else ('BASELINE configs[1]' if (world == 1 and B == 1) else ('BASELINE configs[2]' if (world == 1 and B == 32) else 'custom batch')))}: "
                                   f"F5-TTS 335M, {args.ode_points}-point {args.method} (={n_fwd} DiT forwards, CFG), "
                                   f"batch {B}/GPU x 10 s (N=937) utterances, hipGraph={not args.no_graph}"
                                   + ("; f16 (IEEE half) MFMA operands IN PLACE OF BASELINE's bf16 -- same width and MFMA rate, three more "
                                      "significand bits; plain bf16 fails the 1e-3 parity gate, see sub.b1_bf16" if args.precision == "f16" else "")
                                   + ("; mxfp8 is a reduced-precision mode OUTSIDE the 1e-3 parity gate" if args.precision == "mxfp8" else "")
                                   + (", + Vocos vocoder (mel -> waveform) in the timed region" if args.vocoder else ""),
                       "global_batch": world * B, "seq_len": N_FRAMES, "parallelism": f"dp{world} (utterance sharding)"},
            "per_gpu_value": head["value"] / world,
            "executed_tflop_per_step": world * B * n_fwd * fwd_exec / 1e12, "reference_tflop_per_step": world * B * n_fwd * fwd_ref / 1e12,
            "whole_path_tflops": head["whole_path_tflops"], "whole_path_frac_of_bf16_peak": head["whole_path_frac_of_bf16_peak"],
            "rtf_mel_only": head["rtf_mel_only"],
            "weights_load_s": load_s, "weights_broadcast_ms": bcast_ms, "ranks_seen_by_rccl": ranks_in_group,
            "rank_ms_min": rank_ms_min, "rank_ms_max": rank_ms_max,
            "ln_fold_range_events": model.engine.range_events, "fp16_saturation_events": model.engine.saturation_events,
            "range_check": model.engine.range_check,
        }
        # --full: everything beyond the headline, measured after it
        if args.full:
            if args.precision == "mxfp8":
                kernels, sym = [gemm_roofline_f8(device, B)], {}
            else:
                kernels, sym = kernel_rooflines(args.precision, device, B)
            dominant = max(kernels, key=lambda k: k.get("share_of_block", 1.0))
            if sym and sym.get("f5_gemm*_kernel<EPI_RESID_GATE>", 0.0) >= max(sym.values(), default=0.0):
                # the residual-update GEMM symbol (out-proj + FF2 launches) leads the rocprof CSV: report its heavier instance
                dominant = max((k for k in kernels if k["key"] in ("out_proj_gemm", "ff2_gemm")), key=lambda k: k["share_of_block"])
            rec.update(roofline=dominant, roofline_kernels=kernels, roofline_symbol_shares=sym)
            if dominant.get("peak_measured_tflops"):
                # the measured MFMA micro-benchmark peak next to the data-sheet figure every `frac` divides by
                rec["peak_tflops_datasheet"] = BF16_PEAK_TFLOPS
                rec["peak_measured_tflops"] = dominant["peak_measured_tflops"]
                rec["peak_measured_constant_operands_tflops"] = dominant["peak_measured_constant_operands_tflops"]
                rec["whole_path_frac_of_measured_peak"] = head["whole_path_tflops"] / (world * dominant["peak_measured_tflops"])
            # utterance 0 against the fp32 oracle's golden of this solver (with a vocoder in the loop `out` is a waveform: compare the mel
            # of one extra un-vocoded call instead -- outside the timed region)
            if real:
                par = None
            elif args.vocoder:
                # the SAME batch without the vocoder (same kernels, same LN-fold decision as the timed call): utterance 0 of it
                o_mel, _ = F5TTS(transformer=model).sample(cond, text, **kw)
                torch.cuda.synchronize()
                par = parity_against_golden(o_mel[0], args)
                del o_mel
            else:
                par = parity_against_golden(out[0], args)
            if par:
                rec.update(par)
                if args.precision == "mxfp8":
                    rec["parity_note"] = ("mxfp8 is a reduced-precision mode outside the 1e-3 gate by design; parity_l1 is its measured distance from "
                                          "the fp32 oracle (the oracle with the same MX rounding: tests/golden/make_fullsize_golden.py --emulate mxfp8)")
        if world == 1 and B == 32:
            # the line itself is the batch-32 configuration: the same top-level scalars as the sub-record of the default run
            rec.update(b32_ms_per_step=ms_per_step, b32_value=head["value"], b32_whole_path_frac=head["whole_path_frac_of_bf16_peak"],
                       b32_frac_of_measured=rec.get("whole_path_frac_of_measured_peak"), b32_parity_l1=rec.get("parity_l1"))

        if args.full and world == 1 and not args.no_sub:
            sub = {}
            # (1) RTF as SURVEY §8(d) defines it: reference WAVE in -> mel front-end -> sample -> Vocos -> WAVE out
            f5w = F5TTS(transformer=model, vocoder=vocoder.decode)

            def wave_step():
                c = f5w._mel_spec(waves)                                   # HIP mel front-end, one launch for the batch
                return f5w.sample(c, text, **kw)[0]
            for _ in range(1):
                w_out = wave_step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                w_out = wave_step()
            barrier()
            ms_w = (time.perf_counter() - t0) / args.steps * 1e3
            assert torch.isfinite(w_out).all()
            rec["rtf"] = B * 10.0 / (ms_w * 1e-3)
            # the reference's own definition (generate.py:183-189): seconds of GENERATED audio (reference trimmed off) per second
            rec["rtf_generated_only"] = B * (N_FRAMES - REF_SAMPLES // 256) * 256 / 24000.0 / (ms_w * 1e-3)
            sub["wave_to_wave"] = dict(ms_per_step=ms_w, includes="mel front-end + sample + Vocos vocoder (random-init weights)",
                                       samples_out=int(w_out.numel()))
            # (2) BASELINE configs[2]: batch 32 in the same precision (the MFMA-roofline configuration)
            if B != 32:
                c32, t32, y32, _ = synth_batch(32, first=0, device=device)
                kw32 = dict(kw, y0=y32)
                n32 = 5
                with ClockPowerSampler() as smi32:
                    el, o32, _ = timed_samples(f5, c32, t32, kw32, n32, 1, barrier)
                s32 = summarize(el / n32 * 1e3, 32)
                s32["timed_iterations"] = n32
                if smi32.summary():
                    # the 2.5 PF datasheet peak assumes 2.4 GHz; under the power cap the chip sustains less: the same fraction against the
                    # dense peak AT THE CLOCK THE RUN WAS MEASURED AT
                    s32["clock_power"] = smi32.summary()
                    s32["whole_path_frac_of_peak_at_sustained_clock"] = s32["whole_path_tflops"] / (BF16_PEAK_TFLOPS * s32["clock_power"]["sclk_mhz_median"] / 2400.0)
                p32 = parity_against_golden(o32[0], args) if not real else None
                if p32:
                    s32.update(p32)
                del c32, t32, y32, o32
                torch.cuda.empty_cache()
                if args.precision != "mxfp8":
                    # the five block kernels at M = 59 968 (the shapes the MFMA-roofline target is quoted on), same live timing
                    k32, sym32 = kernel_rooflines(args.precision, device, 32, iters=10)
                    s32["roofline_kernels"] = k32
                    s32["roofline_symbol_shares"] = sym32
                    s32["whole_path_frac_of_measured_peak"] = s32["whole_path_tflops"] / k32[0]["peak_measured_tflops"]
                    torch.cuda.empty_cache()
                sub[f"b32_{args.precision}"] = s32
                # BASELINE configs[2] (the >= 50 % roofline target is quoted on it) as TOP-LEVEL scalars: the driver's `parsed` record keeps
                # scalars and drops nested sub-records
                rec.update(b32_ms_per_step=s32["ms_per_step"], b32_value=s32["value"], b32_whole_path_frac=s32["whole_path_frac_of_bf16_peak"],
                           b32_frac_of_measured=s32.get("whole_path_frac_of_measured_peak"), b32_parity_l1=s32.get("parity_l1"),
                           b32_precision=args.precision, b32_sclk_mhz=(s32.get("clock_power") or {}).get("sclk_mhz_median"),
                           b32_power_w=(s32.get("clock_power") or {}).get("power_w_median"),
                           b32_frac_at_sustained_clock=s32.get("whole_path_frac_of_peak_at_sustained_clock"))
            # (3) the north-star's nominal dtype next to the parity-valid one
            if args.precision != "bf16" and B == 1:
                mb = make_model("bf16")
                mb.load_weights(weights)
                el, ob, _ = timed_samples(F5TTS(transformer=mb), cond, text, kw, 3, 1, barrier)
                sb = summarize(el / 3 * 1e3, B)
                pb = parity_against_golden(ob[0], args) if not real else None
                if pb:
                    sb.update(pb)
                sub["b1_bf16"] = sb
                del mb
            # (4) what a first-seen shape costs under use_graph="auto" (the Python default: almost every generate() call): the same
            # kernels launched eagerly, ~5 000 launches per sample, host-bound
            # Measured as a PAIR: eager and graph legs in alternation, here, minutes after the headline (a headline-vs-this comparison across
            # the sub-records in between is a comparison of clock states: profiles/r06/graph_sync_probe.jsonl)
            if B == 1 and not args.no_graph:
                legs = {"eager": [], "graph": []}
                for _ in range(2):
                    for name, g in (("eager", False), ("graph", True)):
                        el, oe, _ = timed_samples(f5, cond, text, dict(kw, use_graph=g), 3, 1, barrier)
                        legs[name].append(el / 3 * 1e3)
                se = summarize(min(legs["eager"]), B)
                se["note"] = "eager launches (no hipGraph): the cost of a shape signature the first time it is seen"
                se["paired_graph_ms_per_step"] = min(legs["graph"])
                se["legs_ms"] = {k: [round(x, 3) for x in v] for k, v in legs.items()}
                sub["b1_eager"] = se
            # (5) BASELINE configs[4]: MX-fp8 block GEMMs + Vocos in the timed region, 16-point midpoint, batch 32 -- a reduced-precision mode
            # OUTSIDE the parity gate by design, reported with its distance from the fp32 oracle and against the 5 PF dense fp8 peak
            if B == 1 and args.precision == "f16" and not real:
                import argparse as _ap
                m8 = make_model("mxfp8")
                m8.load_weights(weights)
                c32, t32, y32, _ = synth_batch(32, first=0, device=device)
                kw8 = dict(duration=N_FRAMES, steps=16, method="midpoint", cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y32, use_graph=not args.no_graph)
                v8 = Vocos(synthetic_vocos_weights(seed=7), precision="bf16", device=device)
                n8 = 3
                el, o8, _ = timed_samples(F5TTS(transformer=m8, vocoder=v8.decode), c32, t32, kw8, n8, 1, barrier)
                ms8 = el / n8 * 1e3
                nf8 = 2 * 2 * 15
                tf8 = 32 * nf8 * fwd_exec / 1e12 / (ms8 * 1e-3)
                s8 = dict(ms_per_step=ms8, value=32 * N_FRAMES / (ms8 * 1e-3), unit="mel-frames/s", rtf=32 * 10.0 / (ms8 * 1e-3),
                          whole_path_tflops=tf8, whole_path_frac_of_fp8_peak=tf8 / FP8_PEAK_TFLOPS, timed_iterations=n8,
                          workload="BASELINE configs[4]: 32 utterances x 10 s, 16-point midpoint (60 forwards), MX-fp8 (e4m3 + E8M0 per 32) QKV / "
                                   "out-proj / FF1 / FF2 GEMMs, everything else bf16, Vocos vocoder (random-init) in the timed region",
                          samples_out=int(o8.numel()))
                om, _ = F5TTS(transformer=m8).sample(c32, t32, **kw8)         # the same batch without the vocoder: utterance 0 vs the golden
                torch.cuda.synchronize()
                p8 = parity_against_golden(om[0], _ap.Namespace(method="midpoint", ode_points=16))
                if p8:
                    s8.update(p8)
                    s8["parity_note"] = "reduced-precision mode outside the 1e-3 gate by design (the oracle with the same MX rounding predicts 2.1e-2)"
                s8["roofline"] = gemm_roofline_f8(device, 32, iters=10)
                sub["c5_mxfp8"] = s8
                rec.update(c5_ms_per_step=ms8, c5_value=s8["value"], c5_rtf=s8["rtf"], c5_whole_path_frac_of_fp8_peak=s8["whole_path_frac_of_fp8_peak"],
                           c5_parity_l1=s8.get("parity_l1"), c5_qkv_gemm_frac_of_fp8_peak=s8["roofline"]["frac"])
                del m8, v8, c32, t32, y32, o8, om
                torch.cuda.empty_cache()
            rec["sub"] = sub
        else:
            rec["rtf"] = None if not args.vocoder else head["rtf_mel_only"]
        if args.full and world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(weights)
        print(json.dumps(rec))
    if dist_on:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
