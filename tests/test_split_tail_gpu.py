"""The tails of the in-workgroup split kernels (ring_ks2<1> of csrc/gemm.hip, f5_attn2s_kernel of csrc/attention.hip), bit for bit
against what the library computed before both wave groups finished the tile (tests/split_tail.py, tests/golden/split_tail_parent.npz,
recorded by tools/record_split_tail.py), and against the fp64 references of the two op matrices within their derived bounds.

ring_ks2<1>, f16 and bf16x3: RESID_GATE (keep bytes, ldo = N + 8), ADDROWS, F32 at N = 100; M in 1, 63, 64, 65, 130; N in 100, 128,
256; K in 64 (group 1 owns no K tile), 128, 192, 1024.  attn2s, f16 with two and four groups and bf16x3: N in 1, 31, 33, 64, 65, 130,
499; B H = 3; ldo > 64 H; null and ragged kv_len (groups without a tile).

Wall time on one MI355X: 3.7 s for the module (10 tests, 336 launches)."""
import numpy as np
import pytest

import split_tail as ST
from f5test import DEV, E, operand_mode, stream

pytestmark = pytest.mark.gpu

GROUPS = ST.all_groups()


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


@pytest.fixture(scope="module")
def golden():
    return ST.load_golden()


@pytest.mark.parametrize("key,kind,cases", GROUPS, ids=[g[0] for g in GROUPS])
def test_bits_of_the_parent_and_fp64_bounds(lib, golden, key, kind, cases):
    want_all = golden[key]
    at, failures, rows = 0, [], 0
    for c in cases:
        with operand_mode(c.op):
            _, name, want_name, bad, dg = ST.run(lib, E, kind, c, DEV, stream())
        want = want_all[at:at + dg.size].reshape(dg.shape)
        at += dg.size
        rows += dg.shape[1]
        if name != want_name:
            bad.append(f"ran {name}, not {want_name}")
        if want.shape != dg.shape or not np.array_equal(want, dg):
            off = np.argwhere(want != dg) if want.shape == dg.shape else []
            bad.append(f"{len(off)} output row(s) differ from the recording in some bit, first (output, row) = {tuple(off[0]) if len(off) else None}")
        if bad:
            failures.append((c.id, bad))
    print(f"[split tail] {key}: {len(cases)} launches, {rows} rows per output compared bitwise, {len(failures)} failed")
    assert at == want_all.size, (key, at, want_all.size)
    assert not failures, failures[:5]
