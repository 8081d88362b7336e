"""Op-level times (us per launch) of the five kernels of a DiT block at the bench shape, batch 1, for the library this process loads
(F5TTS_HIP_LIB=<another build> for an A/B of two libraries, one process each, in alternation): bench.kernel_rooflines -- every kernel
through its C-ABI op entry point, 50 launches replayed from a hipGraph -- repeated REPS times, one JSON line.

    python tools/block_ops_us.py [precision = f16] [REPS = 3]

Back-to-back launches of ONE kernel overlap at their ends, and a launch of 11 us scatters by +-0.5 us between repetitions (out-proj sits
at 10.8 or at 12 us, profiles/r07): take the median of a dozen, and settle a difference below 1 us with per-kernel averages of a
rocprofv3 --kernel-trace --stats run of bench.py instead."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    prec = sys.argv[1] if len(sys.argv) > 1 else "f16"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda:0")
    rows = []
    for _ in range(reps):
        out, _ = bench.kernel_rooflines(prec, dev, 1, iters=50, peak_meas=dict(workload_like_operands=1.0, constant_operands=1.0))
        rows.append({k["key"]: round(k["avg_launch_ms"] * 1e3, 2) for k in out})
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("F5TTS_HIP_LIB", "libf5tts_hip.so")), precision=prec, us=rows)))


if __name__ == "__main__":
    main()
