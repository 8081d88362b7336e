"""Records tests/golden/split_tail_parent.npz: the row digests of every case of tests/split_tail.py, computed by the library this
process loads.  The file stands for the bits of the split kernels BEFORE their tails were shared out among the wave groups, so it is
recorded with a build of that commit:

    git worktree add /tmp/parent <commit before>; bash /tmp/parent/f5_tts_mlx_amd/csrc/build.sh
    F5TTS_HIP_LIB=/tmp/parent/f5_tts_mlx_amd/csrc/libf5tts_hip.so python tools/record_split_tail.py [--out FILE]

Every launch is also held against the fp64 reference of its op matrix while it is recorded; a launch that misses is an error.  Needs
a GPU."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import split_tail as ST  # noqa: E402
from f5test import DEV, E, operand_mode, stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=ST.GOLDEN)
    a = ap.parse_args()
    lib = E.load_library()
    rec = ST.record(lib, E, DEV, stream(), operand_mode)
    np.savez(a.out, **rec)
    n = sum(v.size for v in rec.values())
    print(f"recorded {len(rec)} groups, {n} row digests ({8 * n} bytes) with {os.environ.get('F5TTS_HIP_LIB', 'the in-tree library')} -> {a.out}")


if __name__ == "__main__":
    main()
