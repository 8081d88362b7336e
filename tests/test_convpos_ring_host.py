"""tests/convpos_ring_cases.py on the CPU: the cover holds every value it promises with every output form, and its statement of the
route (kernel_name) agrees with the launcher's own decision, asked through f5_debug_convpos_route (nothing is launched), over a
grid of shapes on both sides of every condition and under every selector."""
import ctypes as C
import itertools

import pytest

import convaudio_matrix as CM
import convpos_ring_cases as RC
from f5_tts_mlx_amd import engine as E


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def test_cover_holds_every_value_with_every_output_form():
    pairs = RC.twins()
    assert len(pairs) == len(RC.DATA) * len(RC.OUTS) and 2 * len(pairs) <= 64
    for ring, twin in pairs:
        assert (ring.tps, twin.tps, ring.nseg, twin.nseg) == (RC.RING, RC.TWIN, 1, 1)
        assert ring.datakey == twin.datakey and CM.convpos_group(ring) == CM.convpos_group(twin)      # same data, same outputs
        assert ring.var != "neighbours" or ring.B == 3
    for field, values in (("taps", RC.TAPS), ("N", RC.NS), ("B", RC.BS), ("C", RC.CS), ("var", RC.VARS)):
        for v, out in itertools.product(values, RC.OUTS):
            assert any(getattr(r, field) == v and (r.mode, r.lo) == out for r, _ in pairs), (field, v, out)
    # 8 and 16 groups under both numberings, one group on a 3-D grid of several tiles, with one element and with three
    seen = {(r.C, r.xcd) for r, _ in pairs}
    assert {(512, 0), (512, 1), (1024, 0), (1024, 1)} <= seen
    assert {(r.N > 128, r.B) for r, _ in pairs if r.C == 64} >= {(True, 1), (True, 3)}
    assert RC.case(RC.RACE, RC.RING, 0, 1).kw | dict(tps=0) == CM._cp(1024, 257, 3, 31, 1, 0, 1, 0, 1).kw


def test_names_the_issue_fixes():
    for (Cc, N, B, nseg, tps), want in RC.ROUTES:
        assert RC.kernel_name(Cc, N, B, nseg, tps, 1) == want
    # no case of the conv-pos matrix changes kernel: its own name function and this one agree on all of them
    for c in CM.cases("convpos"):
        assert RC.kernel_name(c.C, c.N, c.B, c.nseg, c.tps, c.xcd) == CM.convpos_kernel_name(c), c.id


def test_route_function_of_the_library_agrees(lib):
    buf = C.create_string_buffer(64)
    n = 0
    try:
        for tps, xcd in itertools.product((0, 1, 2, 4, 8), (1, 0)):
            E.check(lib.f5_debug_set_convpos_tps(tps))
            E.check(lib.f5_debug_set_convpos_xcd_map(xcd))
            for Cc, N, B, nseg in itertools.product((64, 128, 512, 1024, 2048), (1, 257, 511, 512, 513, 937, 1024, 1025, 2048, 2049),
                                                    (1, 2, 3, 4, 32), (1, 3)):
                E.check(lib.f5_debug_convpos_route(B, N, Cc // 64, nseg, buf, 64))
                assert buf.value.decode() == RC.kernel_name(Cc, N, B, nseg, tps, xcd), (Cc, N, B, nseg, tps, xcd)
                n += 1
    finally:
        lib.f5_debug_set_convpos_tps(0)
        lib.f5_debug_set_convpos_xcd_map(1)
    assert n == 5 * 2 * 5 * 10 * 5 * 2
    assert lib.f5_debug_convpos_route(0, 937, 16, 1, buf, 64) != 0 and lib.f5_debug_convpos_route(2, 937, 16, 2, buf, 64) != 0
    assert lib.f5_debug_set_convpos_tps(3) != 0 and lib.f5_debug_set_convpos_tps(16) != 0
