"""The row / elementwise kernels of csrc/rowops.hip against fp64 (or an exact reference), by construction: the case generators,
references and checkers of tests/rowops_matrix.py, run through the f5_op_* entry points under both operand types.  Every output
lies between guard bands that must come back bit for bit, every input is followed by NaN, the 16-bit outputs are asked for with
and without the lo half, and the ops that carry the fp16 range tracker report to a status word that every case reads back.

The harness itself is tested on the CPU by tests/test_rowops_matrix_host.py, which shows each of its deliberately wrong emulations
flagged.

Wall time on one MI355X (same machine, one after the other): tests/test_ops_gpu.py, unchanged since the parent commit, 39.1 s (215
tests); this module 5.7 s (42 tests, 1 988 matrix cases under each operand type; the slowest item, GRN, 0.45 s).
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import rowops_matrix as RM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    """the references are thousands of tiny CPU tensors: the thread pool only gets in the way"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def F(v):
    return C.c_float(v)


def Z(v):
    return C.c_size_t(v)


def launch(lib, io):
    """one case through its entry point(s); returns the return code (the caller synchronises)"""
    c, i, s = io.case, io.ins, stream()
    o = {k: (None if v is None else v.t) for k, v in io.outs.items()}
    op = c.op
    if op == "ln_modulate":
        E.check(lib.f5_debug_set_op_ln_mean_out(P(o["mean"])))
        try:
            return lib.f5_op_ln_modulate(P(i["x"]), P(i["scale"]), P(i["shift"]), P(o["hi"]), P(o["lo"]), c.rows, c.dim, s)
        finally:
            E.check(lib.f5_debug_set_op_ln_mean_out(None))
    if op == "layernorm":
        return lib.f5_op_layernorm(P(i["x"]), P(i["w"]), P(i["b"]), P(o["f32"]), P(o["hi"]), P(o["lo"]), c.rows, c.dim, s)
    if op == "dwconv_ln":
        return lib.f5_op_dwconv_ln(P(i["x"]), P(i["dw_w"]), P(i["dw_b"]), P(i["ln_w"]), P(i["ln_b"]), P(o["hi"]), P(o["lo"]), c.B, c.N, c.dim, s)
    if op == "grn":
        assert lib.f5_op_grn_scratch_floats(c.B, c.N, c.dim) == RM.grn_scratch_floats(c.B, c.N, c.dim)
        return lib.f5_op_grn(P(i["g"]), P(i["gamma"]), P(i["beta"]), P(o["scratch"]), P(o["hi"]), P(o["lo"]), c.B, c.N, c.dim, s)
    if op == "text_embed":
        fn = lib.f5_op_text_embed if c.mask else lib.f5_op_text_embed_nomask
        return fn(P(i["text"]), c.nt, P(i["table"]), P(i["pos_table"]), c.max_pos, P(o["out"]), P(o["ids"]), P(o["keep"]), RM.TE_B, RM.TE_N,
                  c.dim, s)
    if op == "pack_bf16":
        return lib.f5_op_pack_bf16(P(i["src"]), P(i["rowkeep"]), P(o["hi"]), P(o["lo"]), c.rows, c.cols, c.ld, c.col0, s)
    if op == "im2col7":
        return lib.f5_op_im2col7(P(i["x"]), P(o["hi"]), P(o["lo"]), c.B, c.N, c.ch, s)
    if op == "pack_x":
        return lib.f5_op_pack_x(P(i["y"]), P(o["hi"]), P(o["lo"]), c.rows, c.mel, s)
    if op == "pack_cond_text":
        return lib.f5_op_pack_cond_text(P(i["cond"]), P(i["lens"]), P(i["text_emb"]), P(o["hi"]), P(o["lo"]), RM.PCT_B, RM.PCT_N, c.mel, c.dt,
                                        c.nkc, s)
    if op == "ode_stage":
        cfg, coef, div = RM.ode_scalars(c)
        # with cfg_ptr the by-value scale must not be read: hand over one that would be caught
        return lib.f5_op_ode_stage(P(i["pred"]), P(i["null_pred"]), F(-77.0 if c.cfgptr else cfg), P(i["cfg_dev"]), P(i["base"]), P(i["dt"]),
                                   F(coef), F(div), c.mode, P(o["kstore"]), P(i["k1"]), P(i["k2"]), P(i["k3"]), P(o["out"]), P(o["xin_hi"]),
                                   P(o["xin_lo"]), c.rows, c.mel, s)
    if op == "splice":
        return lib.f5_op_splice(P(i["cond"]), P(i["y"]), P(i["lens"]), P(o["out"]), c.B, c.N, c.mel, s)
    if op == "rowkeep":
        return lib.f5_op_rowkeep(P(i["dur"]), P(o["keep"]), c.B, c.N, s)
    if op == "copy_words":
        src = i["src"][c.src_off:]
        assert src.data_ptr() % 16 == 4 * c.src_off and o["dst"].data_ptr() % 16 == 4 * c.dst_off
        return lib.f5_op_copy_words(P(src), P(o["dst"]), Z(c.nwords), s)
    if op == "stage_words":
        words = np.ascontiguousarray(i["words"])
        return lib.f5_op_stage_words(words.ctypes.data_as(C.c_void_p), Z(c.nwords), P(o["dst"]), s)
    if op == "zero_vt_pad":
        return lib.f5_op_zero_vt_pad(P(o["vt"]), Z(c.rows), c.seq, c.npad, s)
    if op == "skinny_gemm":
        return lib.f5_op_skinny_gemm(P(i["a"]), P(i["w"]), P(i["bias"]), P(o["out"]), c.M, c.N, c.K, c.silu_in, c.silu_out, s)
    if op == "time_sinus":
        return lib.f5_op_time_sinus(P(i["t"]), P(o["out"]), len(RM.TIMES), c.dim, s)
    if op == "rope_tables":
        rc = lib.f5_op_rope_table(P(o["cos"]), P(o["sin"]), c.seq, RM.ROPE_DH, s)
        return rc or lib.f5_op_rope_table_g4(P(o["tq"]), P(o["tk"]), c.seq, RM.ROPE_DH, F(c.qscale), s)
    if op == "text_pos_table":
        return lib.f5_op_text_pos_table(P(o["table"]), c.max_pos, c.dim, s)
    if op == "duration_head":
        return lib.f5_op_duration_head(P(i["x"]), P(i["g"]), P(i["w"]), P(i["mask"]), P(o["out"]), c.B, c.N, c.dim, F(RM.DUR_EPS), s)
    raise KeyError(op)


def run_case(lib, c, op16):
    """the caller holds the operand mode"""
    io = RM.build(c, op16, device=DEV)
    E.check(lib.f5_debug_set_op_sat_flag(P(io.flag)))
    try:
        rc = launch(lib, io)
    finally:
        E.check(lib.f5_debug_set_op_sat_flag(None))
    if rc != 0:
        return [f"{c.id} {op16}: refused: {lib.f5_last_error().decode()}"]
    torch.cuda.synchronize()
    return RM.check(io)


ALL = RM.cases()


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("op", list(RM.OPS))
def test_matrix(lib, op, op16):
    failures = []
    t0 = time.perf_counter()
    cs = [c for c in ALL if c.op == op]
    with operand_mode(op16):
        assert lib.f5_op_get_operand_type() == (1 if op16 == "f16" else 0)
        for c in cs:
            failures += run_case(lib, c, op16)
    print(f"[rowops matrix] {op} {op16}: {len(cs)} cases, {time.perf_counter() - t0:.2f} s")
    assert not failures, f"{len(failures)} findings in {op} ({op16}):\n" + "\n".join(failures[:25])


def test_every_claimed_instantiation_is_launched():
    """NV 1-4 of the three LayerNorm kernels, both WITH_MEAN values and MBLK 1-4 of the skinny GEMM, counted from the shapes of the
    cases test_matrix runs (the same list under each operand type)"""
    counts = RM.instantiation_counts(ALL)
    assert set(RM.CLAIMED) <= set(counts)
    missing = [k for k in RM.CLAIMED if counts[k] == 0]
    assert not missing, missing
