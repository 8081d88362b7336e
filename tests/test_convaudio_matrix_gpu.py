"""The conv-position kernel (csrc/convpos.hip), the mel front-end and ISTFT head (csrc/audio.hip) and the noise generator
(csrc/noise.hip) against fp64 (the host generator for the noise), by construction: the case generators, references and checkers of
tests/convaudio_matrix.py, run through the C ABI.  Every output lies between guard bands that must come back bit for bit, every input
is followed by NaN, conv-pos runs under both operand types and every case of it reads f5_debug_last_convpos_kernel and compares the
name with what its selectors should give (a selector of 4 taps per step with nseg 3 runs f5_convpos_kernel<true,2>).  Cases of conv-pos
that differ in the block numbering or the taps per step alone must agree bit for bit.

The harness itself is tested on the CPU by tests/test_convaudio_matrix_host.py, which shows each of its deliberately wrong emulations
flagged.

Wall time on one MI355X: this module 11.0 s (9 tests).  The two conv-pos items take 4.1 s each (285 cases under each operand type, 34
groups of them compared bit for bit: the block numbering and the taps per step turned out not to change a single bit, so the fallback
to the bound was not needed); mel 0.15 s (92 cases), ISTFT 0.08 s (41), noise 0.35 s (11), noise_bits 0.01 s (4 cases, 196 618 bit patterns).
Largest |err| / bound seen: conv-pos 0.95 (bf16) and 0.74 (fp16), mel 0.30, ISTFT 0.003; every noise value bit-equal to the host generator.
"""
import ctypes as C
import hashlib
import time

import pytest
import torch

import convaudio_matrix as CM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu

LAUNCHED = {t: {} for t in CM.OPS16}          # operand type -> kernel name -> launches, counted from the hook


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def last_convpos_kernel(lib):
    buf = C.create_string_buffer(64)
    n = lib.f5_debug_last_convpos_kernel(buf, 64)
    assert n == len(buf.value)
    return buf.value.decode()


def launch(lib, io):
    """one case through its entry point; returns the return code (the caller synchronises)"""
    c, i, s = io.case, io.ins, stream()
    o = {k: (None if v is None else v.t) for k, v in io.outs.items()}
    op = c.op
    if op == "convpos":
        lo_in = c.nseg == 3
        E.check(lib.f5_debug_set_convpos_tps(c.tps))
        E.check(lib.f5_debug_set_convpos_xcd_map(c.xcd))
        try:
            return lib.f5_op_convpos(P(i["x_hi"]), P(i["x_lo"] if lo_in else None), P(i["w_hi"]), P(i["w_lo"] if lo_in else None), P(i["bias"]),
                                     P(o["hi"]), P(o["lo"]), P(o["out"]), c.B, c.N, c.C, c.C // 64, c.taps, c.nseg, c.mode, s)
        finally:
            E.check(lib.f5_debug_set_convpos_tps(0))
            E.check(lib.f5_debug_set_convpos_xcd_map(1))
    if op == "mel":
        if c.B == 1:
            return lib.f5_mel_spectrogram(P(i["wave"]), C.c_int64(c.L), P(i["window"]), P(i["fb"]), 1024, c.hop, c.n_mels, P(o["out"]), s)
        return lib.f5_mel_spectrogram_batch(P(i["wave"]), c.B, C.c_int64(c.L), P(i["window"]), P(i["fb"]), 1024, c.hop, c.n_mels, P(o["out"]), s)
    if op == "istft":
        if c.entry == "plain":
            return lib.f5_op_istft(P(i["x"]), c.ldx, P(i["window"]), P(o["frames"]), P(o["wave"]), c.nframes, 1024, c.hop, s)
        return lib.f5_op_istft_batch(P(i["x"]), c.ldx, P(i["window"]), P(o["frames"]), P(o["wave"]), c.B, c.nframes, 1024, c.hop, s)
    if op == "noise":
        seeds = (C.c_uint64 * c.B)(*c.seeds)
        durs = (C.c_int32 * c.B)(*c.durs)
        scratch = torch.empty(3 * c.B, dtype=torch.int32, device=DEV)
        return lib.f5_noise_normal(seeds, c.B, durs, c.N, c.mel, P(o["y0"]), P(scratch), s)
    if op == "noise_bits":
        return lib.f5_op_noise_from_bits(P(i["bits"]), i["bits"].numel(), P(o["out"]), s)
    raise KeyError(op)


def run_case(lib, c, op16, same):
    """the caller holds the operand mode"""
    io = CM.build(c, op16, device=DEV)
    E.check(lib.f5_debug_set_op_sat_flag(P(io.flag)))
    try:
        rc = launch(lib, io)
    finally:
        E.check(lib.f5_debug_set_op_sat_flag(None))
    torch.cuda.synchronize()
    bad = []
    if c.op == "convpos":
        name = last_convpos_kernel(lib)
        LAUNCHED[op16][name] = LAUNCHED[op16].get(name, 0) + 1
        if name != CM.convpos_kernel_name(c):
            bad.append(f"{c.id} {op16}: ran {name!r}, the selectors ask for {CM.convpos_kernel_name(c)!r}")
    refuse = bool(c.kw.get("refuse"))
    if (rc != 0) != refuse:
        return bad + [f"{c.id} {op16}: " + (f"refused: {lib.f5_last_error().decode()}" if rc else "accepted, but must be refused")]
    bad += CM.check(io)
    if c.op == "convpos":
        out = io.outs["hi"] if c.mode == 0 else io.outs["out"]
        h = hashlib.sha1(out.t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
        if c.lo:
            h.update(io.outs["lo"].t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
        first = same.setdefault(CM.convpos_group(c), (c.id, h.digest()))
        if first[1] != h.digest():
            bad.append(f"{c.id} {op16}: not the bits of {first[0]}, which differs in the block numbering / taps per step alone")
    return bad


ALL = CM.cases()


@pytest.mark.parametrize("op,op16", [(op, t) for op in CM.OPS for t in CM.op_types(op)])
def test_matrix(lib, op, op16):
    failures, same = [], {}
    t0 = time.perf_counter()
    cs = [c for c in ALL if c.op == op]
    CM.pool_reset(op)
    with operand_mode(op16):
        assert lib.f5_op_get_operand_type() == (1 if op16 == "f16" else 0)
        for c in cs:
            failures += run_case(lib, c, op16, same)
    if op in CM.POOLED:
        failures += CM.pool_findings(op)
    worst = {k[0]: v for k, v in CM.WORST.items() if k[0].startswith(op + "[") and k[1] == op16}
    if op == "convpos":
        groups = {}
        for c in cs:
            groups.setdefault(CM.convpos_group(c), []).append(c)
        print(f"[convaudio matrix] convpos {op16}: {sum(len(v) > 1 for v in groups.values())} groups of cases compared bit for bit; worst |err| / bound "
              f"{max(worst.values()):.3f}")
    else:
        for k, v in worst.items():
            print(f"[convaudio matrix] worst |err| / bound {v:.4f}  {k}")
    print(f"[convaudio matrix] {op} {op16}: {len(cs)} cases, {time.perf_counter() - t0:.2f} s")
    assert not failures, f"{len(failures)} findings in {op} ({op16}):\n" + "\n".join(failures[:25])


@pytest.mark.parametrize("op16", CM.OPS16)
def test_every_convpos_instantiation_is_launched_under_both_numberings(lib, op16):
    """all 5 instantiations x {plain, +xcd}, counted from the names f5_debug_last_convpos_kernel reported while test_matrix ran; the
    hook reports "" after a launch that was refused"""
    if not LAUNCHED[op16]:                               # selected alone: run the cases that name the kernels
        with operand_mode(op16):
            seen = set()
            for c in (c for c in ALL if c.op == "convpos"):
                if CM.convpos_kernel_name(c) not in seen:
                    seen.add(CM.convpos_kernel_name(c))
                    assert not run_case(lib, c, op16, {})
    missing = [k for k in CM.CP_NAMES if not LAUNCHED[op16].get(k)]
    print(f"[convaudio matrix] convpos {op16} launches per kernel: {LAUNCHED[op16]}")
    assert not missing and set(LAUNCHED[op16]) == set(CM.CP_NAMES), (missing, LAUNCHED[op16])
    with operand_mode(op16):
        x = torch.zeros(64, dtype=torch.float32, device=DEV)
        assert lib.f5_op_convpos(P(x), P(None), P(x), P(None), P(x), P(x), P(None), P(None), 1, 1, 64, 1, 2, 1, 0, stream()) != 0      # even tap count
        assert last_convpos_kernel(lib) == ""


def test_tps4_with_nseg3_runs_the_two_slab_kernel(lib):
    """the mapping the header records: with nseg == 3 a selector of 2 or 4 taps per step runs f5_convpos_kernel<true,2>"""
    got = {}
    for tps in (1, 2, 4):
        c = next(c for c in ALL if c.op == "convpos" and c.nseg == 3 and c.tps == tps and c.C == 128)
        assert not run_case(lib, c, "bf16", {})
        got[tps] = last_convpos_kernel(lib)
    assert got == {1: "f5_convpos_kernel<true,1>", 2: "f5_convpos_kernel<true,2>", 4: "f5_convpos_kernel<true,2>"}, got
