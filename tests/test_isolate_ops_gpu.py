"""The two kernels with row lengths behind the isolate_rows option (docs/isolate_rows.md), through their op entry points:
f5_op_grn_ragged and f5_op_convpos_ragged.  Bitwise statements compare launches of the same shape (conv-pos) or the element alone at
its own length (GRN, whose chunking is aligned at token 0); the fp64 bounds are those of tests/rowops_matrix.py and
tests/convaudio_matrix.py, called, not copied."""
import ctypes as C

import numpy as np
import pytest
import torch

import convaudio_matrix as CM
import rowops_matrix as RM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


class sat_flag:
    """the per-op saturation report into a word of ours for the length of a block"""

    def __init__(self, lib):
        self.lib = lib
        self.word = torch.zeros(1, dtype=torch.int32, device=DEV)

    def __enter__(self):
        E.check(self.lib.f5_debug_set_op_sat_flag(P(self.word)))
        return self

    def __exit__(self, *exc):
        E.check(self.lib.f5_debug_set_op_sat_flag(None))

    def value(self):
        return int(self.word.cpu()[0])


def dev_lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def same_bits(a, b):
    return torch.equal(RM.bits(a), RM.bits(b))


# ---- GRN -------------------------------------------------------------------------------------------------------------------------
GRN_B, GRN_N = 4, 70
GRN_LENS = (70, 64, 33, 5)          # the full length, a chunk boundary (32-token chunks), one token past a boundary, less than one chunk


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("dim", [256, 1024])
def test_grn_ragged(lib, dim, op16):
    r = np.random.default_rng(1000 + dim)
    g = RM._randn(r, GRN_B, GRN_N, dim)
    gamma, beta = RM._randn(r, dim, scale=0.1), RM._randn(r, dim, scale=0.1)
    g_nan = g.clone()
    for b, n in enumerate(GRN_LENS):
        g_nan[b, n:] = NAN
    s = stream()
    with operand_mode(op16), sat_flag(lib) as flag:
        d_g, d_gamma, d_beta = RM.pad_in(g_nan, DEV), RM.pad_in(gamma, DEV), RM.pad_in(beta, DEV)
        hi = RM.Out((GRN_B * GRN_N, dim), RM.op_dtype(op16), DEV, guard=dim)
        lo = RM.Out((GRN_B * GRN_N, dim), RM.op_dtype(op16), DEV, guard=dim)
        scratch = RM.Out((RM.grn_scratch_floats(GRN_B, GRN_N, dim),), torch.float32, DEV)
        assert lib.f5_op_grn_scratch_floats(GRN_B, GRN_N, dim) == RM.grn_scratch_floats(GRN_B, GRN_N, dim)
        d_lens = dev_lens(GRN_LENS)
        E.check(lib.f5_op_grn_ragged(P(d_g), P(d_gamma), P(d_beta), P(scratch.t), P(hi.t), P(lo.t), GRN_B, GRN_N, dim, P(d_lens), s),
                "f5_op_grn_ragged")
        torch.cuda.synchronize()
        bad = hi.guard_violations("hi") + lo.guard_violations("lo") + scratch.guard_violations("scratch")
        got_hi, got_lo = hi.t.view(GRN_B, GRN_N, dim), lo.t.view(GRN_B, GRN_N, dim)
        for b, n in enumerate(GRN_LENS):
            # the element alone at seq_len = lens[b]: the same bits, both halves
            solo_g = RM.pad_in(g[b:b + 1, :n].contiguous(), DEV)
            s_hi = RM.Out((n, dim), RM.op_dtype(op16), DEV, guard=dim)
            s_lo = RM.Out((n, dim), RM.op_dtype(op16), DEV, guard=dim)
            s_scr = RM.Out((RM.grn_scratch_floats(1, n, dim),), torch.float32, DEV)
            E.check(lib.f5_op_grn(P(solo_g), P(d_gamma), P(d_beta), P(s_scr.t), P(s_hi.t), P(s_lo.t), 1, n, dim, s), "f5_op_grn")
            torch.cuda.synchronize()
            if not same_bits(got_hi[b, :n], s_hi.t):
                bad.append(f"row {b} (len {n}): hi differs from f5_op_grn on the row alone")
            if not same_bits(got_lo[b, :n], s_lo.t):
                bad.append(f"row {b} (len {n}): lo differs from f5_op_grn on the row alone")
            # exact zeros past the length
            if int((RM.bits(got_hi[b, n:]) != 0).sum()) or int((RM.bits(got_lo[b, n:]) != 0).sum()):
                bad.append(f"row {b} (len {n}): tokens past the length are not exact zeros")
            # the fp64 reference of the row alone, within the matrix's bound for GRN
            case = RM.Case("grn", dim=dim, N=n, B=1, zero=0, lo=1)
            bad += [f"row {b} (len {n}): {v}" for v in RM.chk_grn(case, op16, dict(g=g[b:b + 1, :n], gamma=gamma, beta=beta),
                                                                   dict(hi=got_hi[b, :n].cpu(), lo=got_lo[b, :n].cpu()))]
        if flag.value() != 0:
            bad.append(f"range flag {flag.value()}: the NaN padding reached a packer")
        # refusals: before any launch
        assert lib.f5_op_grn_ragged(P(d_g), P(d_gamma), P(d_beta), P(scratch.t), P(hi.t), P(lo.t), GRN_B, GRN_N, dim, None, s) != 0
        assert lib.f5_last_error() == b"grn_ragged: lens is null"
    assert not bad, "\n".join(bad)


# ---- conv-pos --------------------------------------------------------------------------------------------------------------------
def last_convpos_kernel(lib):
    buf = C.create_string_buffer(64)
    lib.f5_debug_last_convpos_kernel(buf, 64)
    return buf.value.decode()


def convpos_route(lib, B, N, groups, nseg):
    buf = C.create_string_buffer(64)
    lib.f5_debug_convpos_route(B, N, groups, nseg, buf, 64)
    return buf.value.decode()


CP_C, CP_B, CP_TAPS = 512, 5, 31
# family -> (seq_len, nseg, the name f5_debug_last_convpos_kernel must report).  512 channels are 8 groups, dealt to XCDs; the ring
# kernel is reached automatically from 512 tokens on while the grid is one round: 4 tiles x 8 groups x 5 elements = 160 workgroups
CP_FAMILIES = {
    "one_pass": (257, 1, "f5_convpos_kernel<false,1>+xcd"),
    "three_pass": (257, 3, "f5_convpos_kernel<true,1>+xcd"),
    "ring": (512, 1, "f5_convpos_ring_kernel+xcd"),
}


def cp_lens(N):
    """the full length, a tile boundary (128 tokens) + 1, the boundary, the boundary - 1, inside the first tile"""
    return (N, 129, 128, 127, 50)


def cp_launch(lib, c, x_hi, x_lo, w_hi, w_lo, bias, outs, lens):
    """lens: a device tensor, None = the new entry point with lens NULL, "plain" = f5_op_convpos"""
    lo_in = c.nseg == 3
    a = (P(x_hi), P(x_lo if lo_in else None), P(w_hi), P(w_lo if lo_in else None), P(bias), P(None if outs["hi"] is None else outs["hi"].t),
         P(None if outs["lo"] is None else outs["lo"].t), P(None if outs["out"] is None else outs["out"].t), c.B, c.N, c.C, c.C // 64, c.taps,
         c.nseg, c.mode)
    if isinstance(lens, str):
        return lib.f5_op_convpos(*a, stream())
    return lib.f5_op_convpos_ragged(*a, P(lens), stream())


def cp_outs(c, op16, spec, old_init):
    outs = {}
    for name in ("hi", "lo", "out"):
        sp = spec[name]
        outs[name] = None if sp is None else RM.Out(sp["shape"], sp["dtype"], DEV, sp["guard"], old_init if name == "out" else None)
    return outs


@pytest.mark.parametrize("op16", CM.OPS16)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("family", list(CP_FAMILIES))
def test_convpos_ragged(lib, family, mode, op16):
    N, nseg, kernel = CP_FAMILIES[family]
    lens = cp_lens(N)
    c = CM._cp(CP_C, N, CP_B, CP_TAPS, nseg, 0, 1, mode, 1 if mode == 0 else 0, var="isolate")
    ins, spec = CM.gen_convpos(c, op16, np.random.default_rng(c.seed(op16)))
    valid = torch.zeros(CP_B, N, dtype=torch.bool)
    for b, n in enumerate(lens):
        valid[b, :n] = True
    rows = valid.reshape(-1)
    # the input with zeros past the lengths (what the plain call is given), and with NaN there (what the ragged call is given)
    x = torch.where(valid[:, :, None], ins["x"], torch.zeros(()))
    x_hi, x_lo = CM.split(x.reshape(CP_B * N, CP_C), op16)
    ins = dict(ins, x=x, x_hi=x_hi, x_lo=x_lo)
    nan_hi, nan_lo = x_hi.clone(), x_lo.clone()
    nan_hi[~rows] = NAN
    nan_lo[~rows] = NAN
    # mode 1 accumulates: rows past the lengths start as the sentinel, which must still be there afterwards
    old = ins["old"].clone()
    RM.bits(old)[~rows] = RM.SENT32
    bad = []
    with operand_mode(op16), sat_flag(lib) as flag:
        if family == "ring":
            assert convpos_route(lib, CP_B, N, CP_C // 64, nseg) == kernel
            assert convpos_route(lib, CP_B, N - 1, CP_C // 64, nseg) != kernel          # the smallest seq_len of that route
        d = {k: RM.pad_in(v, DEV) for k, v in dict(x_hi=x_hi, x_lo=x_lo, nan_hi=nan_hi, nan_lo=nan_lo, w_hi=ins["w_hi"], w_lo=ins["w_lo"],
                                                  bias=ins["bias"]).items()}
        plain, ragged, null = (cp_outs(c, op16, spec, old) for _ in range(3))
        assert cp_launch(lib, c, d["x_hi"], d["x_lo"], d["w_hi"], d["w_lo"], d["bias"], plain, "plain") == 0, lib.f5_last_error()
        assert last_convpos_kernel(lib) == kernel
        d_lens = dev_lens(lens)
        assert cp_launch(lib, c, d["nan_hi"], d["nan_lo"], d["w_hi"], d["w_lo"], d["bias"], ragged, d_lens) == 0, lib.f5_last_error()
        assert last_convpos_kernel(lib) == kernel
        assert cp_launch(lib, c, d["x_hi"], d["x_lo"], d["w_hi"], d["w_lo"], d["bias"], null, None) == 0, lib.f5_last_error()
        assert last_convpos_kernel(lib) == kernel
        torch.cuda.synchronize()
        if flag.value() != 0:
            bad.append(f"range flag {flag.value()}: the NaN padding reached a packer")
    got = {}
    for name in ("hi", "lo", "out"):
        if plain[name] is None:
            got[name] = None
            continue
        bad += ragged[name].guard_violations(name) + null[name].guard_violations(name + " (lens NULL)")
        p, g, z = plain[name].t.cpu(), ragged[name].t.cpu(), null[name].t.cpu()
        if not same_bits(z, p):
            bad.append(f"{name}: lens = NULL through f5_op_convpos_ragged is not f5_op_convpos bit for bit")
        if not same_bits(g[rows], p[rows]):
            n_off = int((RM.bits(g[rows]) != RM.bits(p[rows])).sum())
            bad.append(f"{name}: {n_off} values of rows n < lens[b] differ from the plain call on the zeroed input")
        kept = RM.bits(g[~rows]) == RM._sentinel(g)
        if not bool(kept.all()):
            bad.append(f"{name}: {int((~kept).sum())} values of rows n >= lens[b] were written")
        got[name] = torch.where(rows[:, None], g, p)              # the ragged call's own rows; the plain call's where it wrote none
    # mode 1: a row past the lengths started from the NaN sentinel in both calls and has no `out - old` to compare
    bad += cp_check_rows(c, op16, ins, got, rows if mode == 1 else torch.ones_like(rows))
    assert not bad, "\n".join(bad)


def cp_check_rows(c, op16, ins, got, ref_rows):
    """tests/convaudio_matrix.py chk_convpos on the rows `ref_rows`; the others are handed over as the reference's own value"""
    if bool(ref_rows.all()):
        return CM.chk_convpos(c, op16, ins, got)
    pre, ref = CM._convpos_ref(c, op16, ins)
    old = ins["old"].clone()
    out = got["out"].clone()
    old[~ref_rows] = 0.0
    out[~ref_rows] = ref[~ref_rows].float()
    return CM.chk_convpos(c, op16, dict(ins, old=old), dict(got, out=out))
