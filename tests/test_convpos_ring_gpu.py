"""f5_convpos_ring_kernel (csrc/convpos.hip: weight slabs and halo tile by LDS-DMA, a ring of slabs, swizzled 128-byte rows) against
its twin f5_convpos_kernel<false,1>: the same inputs under selector 8 and selector 1 must give the same bytes and the same range
status word, in both operand builds and all three output forms, and the ring run must pass the fp64 bound of
tests/convaudio_matrix.py with its guard bands intact.  Then a race screen (one shape twenty times, one digest) and the routes:
which shapes reach the ring kernel on their own and which keep the kernel they had.  Cases: tests/convpos_ring_cases.py.
"""
import ctypes as C
import hashlib

import pytest
import torch

import convaudio_matrix as CM
import convpos_ring_cases as RC
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def last_kernel(lib):
    buf = C.create_string_buffer(64)
    n = lib.f5_debug_last_convpos_kernel(buf, 64)
    assert n == len(buf.value)
    return buf.value.decode()


def run(lib, c, op16, io=None):
    """one conv-pos case through f5_op_convpos under its selectors -> (io, name of the kernel that ran); the caller holds the operand mode"""
    io = io or CM.build(c, op16, device=DEV)
    i, o = io.ins, {k: (None if v is None else v.t) for k, v in io.outs.items()}
    lo_in = c.nseg == 3
    E.check(lib.f5_debug_set_op_sat_flag(P(io.flag)))
    E.check(lib.f5_debug_set_convpos_tps(c.tps))
    E.check(lib.f5_debug_set_convpos_xcd_map(c.xcd))
    try:
        E.check(lib.f5_op_convpos(P(i["x_hi"]), P(i["x_lo"] if lo_in else None), P(i["w_hi"]), P(i["w_lo"] if lo_in else None), P(i["bias"]),
                                  P(o["hi"]), P(o["lo"]), P(o["out"]), c.B, c.N, c.C, c.C // 64, c.taps, c.nseg, c.mode, stream()))
    finally:
        E.check(lib.f5_debug_set_convpos_tps(0))
        E.check(lib.f5_debug_set_convpos_xcd_map(1))
        E.check(lib.f5_debug_set_op_sat_flag(None))
    torch.cuda.synchronize()
    return io, last_kernel(lib)


def digest(io):
    """the outputs WITH their guard bands, and the status word"""
    h = hashlib.sha1()
    for name in ("hi", "lo", "out"):
        if io.outs[name] is not None:
            h.update(io.outs[name].raw.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    h.update(io.flag.cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("op16", CM.OPS16)
def test_ring_kernel_gives_the_bits_of_its_twin(lib, op16):
    bad = []
    with operand_mode(op16):
        for ring, twin in RC.twins():
            io_r, name_r = run(lib, ring, op16)
            io_t, name_t = run(lib, twin, op16)
            want_r, want_t = (RC.kernel_name(c.C, c.N, c.B, 1, c.tps, c.xcd) for c in (ring, twin))
            if (name_r, name_t) != (want_r, want_t):
                bad.append(f"{ring.id} {op16}: ran {name_r!r} and {name_t!r}, the selectors ask for {want_r!r} and {want_t!r}")
            if digest(io_r) != digest(io_t):
                diff = [k for k in ("hi", "lo", "out") if io_r.outs[k] is not None and not torch.equal(CM.bits(io_r.outs[k].raw), CM.bits(io_t.outs[k].raw))]
                bad.append(f"{ring.id} {op16}: not the bytes of f5_convpos_kernel<false,1> in {diff or 'the status word'} "
                           f"(status {int(io_r.flag.cpu()[0])} against {int(io_t.flag.cpu()[0])})")
            bad += CM.check(io_r)
    print(f"[convpos ring] {op16}: {len(RC.twins())} pairs, worst |err| / bound "
          f"{max(v for k, v in CM.WORST.items() if k[1] == op16 and 'tps=8' in k[0]):.3f}")
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad[:25])


def test_twenty_launches_of_one_shape_give_one_digest(lib):
    """a slab read before it has landed, or overwritten before every wave has read it, shows as a launch that differs"""
    c = RC.case(RC.RACE, RC.RING, 0, 1)
    seen = {}
    with operand_mode("f16"):
        for k in range(RC.RACE_LAUNCHES):
            io, name = run(lib, c, "f16")
            assert name == "f5_convpos_ring_kernel+xcd"
            seen.setdefault(digest(io), []).append(k)
            if k == 0:
                assert not CM.check(io)
    assert len(seen) == 1, f"launches fall into {len(seen)} groups: {list(seen.values())}"


@pytest.mark.parametrize("shape,want", RC.ROUTES)
def test_route(lib, shape, want):
    Cc, N, B, nseg, tps = shape
    c = CM._cp(Cc, N, B, 31, nseg, tps, 1, 1, 0)
    with operand_mode("f16"):
        io, name = run(lib, c, "f16")
    assert name == want and RC.kernel_name(Cc, N, B, nseg, tps, 1) == want
    if name.startswith("f5_convpos_ring_kernel"):        # the shape the route exists for: the twin's bytes there too
        with operand_mode("f16"):
            io_t, name_t = run(lib, CM._cp(Cc, N, B, 31, nseg, RC.TWIN, 1, 1, 0), "f16")
        assert name_t == "f5_convpos_kernel<false,1>+xcd" and digest(io) == digest(io_t)
    if Cc * N * B <= 1024 * 257 * 3:                      # the fp64 reference of the long shapes is not worth its seconds here
        assert not CM.check(io)
