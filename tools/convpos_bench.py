#!/usr/bin/env python
"""Conv-pos at op level (f5_op_convpos, fp16 operands): microseconds per launch at one shape, warm and cold, per mode and selector.

    python tools/convpos_bench.py --label parent --tps 1 --modes 0,1 --reps 12              # one JSON line per (mode, cache state)
    F5TTS_HIP_LIB=/path/to/other/libf5tts_hip.so python tools/convpos_bench.py --label ...  # another build of the library

warm: `--launches` launches back to back between two events, the operands stay in the caches.
cold: 512 MiB are written to a scratch buffer before every launch, outside the timed events (the Infinity Cache holds 256 MiB), and
      every launch is timed on its own; a repetition is the mean of `--cold-launches` of them.  A single launch between events carries
      the events' own cost, the same for every build.

Probe builds (the anatomy of the kernels: parts removed by csrc/convpos.hip's CP_ABL bits, ring depth and taps per barrier of
f5_convpos_ring_kernel by CP_RING_NST / CP_RING_S / CP_RING_EPI) are made WITHOUT a GPU from the objects csrc/build.sh left:

    python tools/convpos_bench.py --build-probe /tmp/abl1.so --defs=-DCP_ABL=1

compiles csrc/convpos.hip for both operand types with the definitions and links it with the other objects of csrc/build/.
Probe builds with CP_ABL != 0 compute wrong results by design; they are timed, never tested.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "f5_tts_mlx_amd", "csrc")


def build_probe(out, defs):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = sorted(os.path.join(CSRC, "build", f) for f in os.listdir(os.path.join(CSRC, "build")) if f.endswith(".o") and not f.startswith("convpos_"))
    if not objs:
        sys.exit("run csrc/build.sh first: its objects are linked into the probe")
    with tempfile.TemporaryDirectory() as tmp:
        mine = []
        for v in (0, 1):
            o = os.path.join(tmp, f"convpos_h{v}.o")
            subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", f"-DF5_F16={v}", *defs,
                                   "-c", os.path.join(CSRC, "convpos.hip"), "-o", o])
            mine.append(o)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, *mine, "-o", out])
    print(f"built {out} with {' '.join(defs) or 'no definitions'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build-probe", metavar="OUT.so")
    ap.add_argument("--defs", action="append", default=[], help="-D... for --build-probe (repeatable)")
    ap.add_argument("--label", default="")
    ap.add_argument("--tps", type=int, default=0, help="f5_debug_set_convpos_tps: 0 auto, 1 / 2 / 4, 8 = ring kernel")
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--N", type=int, default=937)
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--taps", type=int, default=31)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--cold-launches", type=int, default=10)
    ap.add_argument("--no-cold", action="store_true")
    a = ap.parse_args()
    if a.build_probe:
        return build_probe(a.build_probe, a.defs)

    import ctypes as C

    import torch

    sys.path.insert(0, ROOT)
    from f5_tts_mlx_amd import engine as E

    lib = E.load_library()
    dev = torch.device("cuda:0")
    P, s = E.ptr, E.stream_ptr(dev)
    g = torch.Generator().manual_seed(0)
    rows = a.B * a.N
    x = torch.randn(rows, a.C, generator=g).to(torch.float16).to(dev)
    w = (torch.randn(a.C, a.taps * 64, generator=g) * (a.taps * 64) ** -0.5).to(torch.float16).to(dev)
    bias = (torch.randn(a.C, generator=g) * 0.1).to(dev)
    hi, lo = torch.empty_like(x), torch.empty_like(x)
    out = torch.zeros(rows, a.C, device=dev)
    scratch = None if a.no_cold else torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    E.check(lib.f5_op_set_operand_type(1))
    E.check(lib.f5_debug_set_convpos_tps(a.tps))
    name = C.create_string_buffer(64)

    def launch(mode):
        E.check(lib.f5_op_convpos(P(x), P(None), P(w), P(None), P(bias), P(hi if mode == 0 else None), P(lo if mode == 0 else None),
                                  P(out if mode else None), a.B, a.N, a.C, a.C // 64, a.taps, 1, mode, s))

    def timed(mode, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch(mode)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for mode in (int(m) for m in a.modes.split(",")):
        for _ in range(5):
            launch(mode)
        torch.cuda.synchronize()
        lib.f5_debug_last_convpos_kernel(name, 64)
        for cache in ("warm",) if a.no_cold else ("warm", "cold"):
            us = []
            for _ in range(a.reps):
                if cache == "warm":
                    us.append(timed(mode, a.launches))
                else:
                    one = []
                    for _ in range(a.cold_launches):
                        scratch.fill_(1)
                        one.append(timed(mode, 1))
                    us.append(sum(one) / len(one))
            print(json.dumps(dict(label=a.label, lib=os.environ.get("F5TTS_HIP_LIB", "default"), kernel=name.value.decode(), tps=a.tps, mode=mode,
                                  C=a.C, N=a.N, B=a.B, taps=a.taps, cache=cache, reps=a.reps, us_median=round(statistics.median(us), 2),
                                  us_min=round(min(us), 2), us_max=round(max(us), 2))), flush=True)
    lib.f5_debug_set_convpos_tps(0)
    lib.f5_op_set_operand_type(0)


if __name__ == "__main__":
    main()
