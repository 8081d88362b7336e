"""The MX-fp8 path (csrc/gemm_f8.hip, its producers in csrc/rowops.hip) against fp64, by construction: every case of
tests/mxfp8_matrix.py through f5_op_gemm_f8, f5_op_qkv_rope_f8, f5_op_quantize_mx, f5_op_quantize_mx_bf16 and f5_op_ln_modulate_f8, operands as
raw e4m3 / E8M0 bytes between guard rows of NaN codes, sentinels around and inside every output, the identity and lattice classes held
to the exact value, gauss to the element-wise bound derived in the module's docstring, the quantisers to the oracle's bytes.

Then the requests the launchers must refuse: asserted through the return code and f5_last_error, nothing is launched for them.

The harness itself is tested on the CPU by tests/test_mxfp8_matrix_host.py, which shows that each of 20 kinds of subtly wrong kernel
would fail here.  tests/test_mxfp8_gpu.py keeps the model-level half of the coverage.
"""
import time

import pytest
import torch

import mxfp8_matrix as X
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def launch_gemm(lib, b, **twist):
    """one case through f5_op_gemm_f8; twist bends single arguments (the refusal tests).  Returns the return code."""
    c = b["case"]
    owned = X.owned_outputs(c)
    a = {"a8": X.ptr_tensor(b, "a8"), "as": X.ptr_tensor(b, "as"), "w8": X.ptr_tensor(b, "w8"), "ws": X.ptr_tensor(b, "ws"),
         "bias": b["bias"], "gate": b["gate"], "keep": b["keep"], "M": c.M, "N": c.N, "K": c.K, "lda8": c.lda8, "ldw8": c.ldw8, "ldo": c.ldo,
         "epi": X.EPI[c.epi.replace("_NOKEEP", "")]}
    for name in ("out_f32", "out_bf", "out8", "out8s"):
        a[name] = b[name].ptr_tensor() if name in owned else None
    a.update(twist)
    return lib.f5_op_gemm_f8(P(a["a8"]), P(a["as"]), P(a["w8"]), P(a["ws"]), P(a["bias"]), P(a["gate"]), P(a["keep"]), P(a["out_f32"]),
                             P(a["out_bf"]), P(a["out8"]), P(a["out8s"]), a["M"], a["N"], a["K"], a["lda8"], a["ldw8"], a["ldo"], a["epi"], stream())


def launch_qkv(lib, b, **twist):
    c = b["case"]
    a = {"a8": X.ptr_tensor(b, "a8"), "qk": b["qk"].ptr_tensor(), "vt": b["vt"].ptr_tensor(), "npad": c.npad, "heads": X.QKV_H, "lda8": c.lda8}
    a.update(twist)
    return lib.f5_op_qkv_rope_f8(P(a["a8"]), P(X.ptr_tensor(b, "as")), P(X.ptr_tensor(b, "w8")), P(X.ptr_tensor(b, "ws")), P(b["bias"]),
                                 P(b["cos"]), P(b["sin"]), P(a["qk"]), P(a["vt"]), c.B, c.seq, a["npad"], a["heads"], X.QKV_D, a["lda8"], c.ldw8,
                                 c.qpre, stream())


def launch_producer(lib, b, **twist):
    c = b["case"]
    a = {"x": b["x_dev"][X.GUARD:] if c.kind != "ln" else b["x_dev"], "q": b["q"].ptr_tensor(), "ldx": c.lda8, "ldq": c.ldw8, "cols": c.N}
    a.update(twist)
    if c.kind == "ln":
        return lib.f5_op_ln_modulate_f8(P(a["x"]), P(b["scale_dev"]), P(b["shift_dev"]), P(a["q"]), P(b["qs"].ptr_tensor()), c.M, a["cols"],
                                        X.LN_EPS, stream())
    fn = lib.f5_op_quantize_mx if c.kind == "quant" else lib.f5_op_quantize_mx_bf16
    return fn(P(a["x"]), a["ldx"], P(a["q"]), a["ldq"], P(b["qs"].ptr_tensor()), c.M, a["cols"], stream())


LAUNCH = {"gemm": launch_gemm, "qkv": launch_qkv, "quant": launch_producer, "quant16": launch_producer, "ln": launch_producer}


def run_case(lib, c, stats):
    b = X.make_buffers(c, device=DEV)
    ref = X.reference(b)
    rc = LAUNCH[c.kind](lib, b)
    if rc != 0:
        return [f"refused: {lib.f5_last_error().decode()}"]
    torch.cuda.synchronize()
    return X.check(b, ref, stats)


# ---- the matrix --------------------------------------------------------------------------------------------------------------
CASES = X.cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c.group, []).append(_c)


def _gid(g):
    return "-".join(s for s in g if s)


def _operand_types(group):
    """which process operand types a group runs under.  quantize_mx_bf16 follows the type; the bf16 epilogue of the MX-fp8 GEMM and the
    QKV projection of the mode must NOT (they exist in the bf16 build only): they run under both and are checked as bf16 both times"""
    if group[0] == "quant16":
        return (group[1],)
    return ("bf16", "f16") if group[0] == "qkv" or group[1] == "BF16" else ("bf16",)


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_matrix(lib, group):
    failures, stats, t0, n = [], {}, time.time(), 0
    before = lib.f5_op_get_operand_type()
    for op in _operand_types(group):
        with operand_mode(op):
            assert lib.f5_op_get_operand_type() == (1 if op == "f16" else 0)
            for c in GROUPS[group]:
                bad = run_case(lib, c, stats)
                n += 1
                if bad:
                    failures.append((c.id, op, bad))
    assert lib.f5_op_get_operand_type() == before                    # the operand type of the process is what it was
    print(f"[mxfp8 matrix] {_gid(group)}: {n} launches, {len(failures)} failed, {time.time() - t0:.2f} s; largest |err| / bound "
          f"{stats.get('worst', 0.0):.3f}")
    assert not failures, failures[:4]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _off(t, n):
    """the same storage n elements further on: a pointer that is off its alignment (never dereferenced: the launch is refused)"""
    return t.reshape(-1)[n:]


def _refusals():
    f32 = X.gemm_case("F32", "gauss", 31, 512, 256)
    bf = X.gemm_case("BF16", "gauss", 31, 512, 256)
    gelu = X.gemm_case("GELU_TANH", "gauss", 31, 512, 256)
    res = X.gemm_case("RESID_GATE", "gauss", 31, 512, 256)
    qkv = next(c for c in CASES if c.kind == "qkv")
    ln = next(c for c in CASES if c.kind == "ln" and c.N == 1024 and c.M == 3)
    qf = next(c for c in CASES if c.kind == "quant" and c.N == 64 and c.M == 3)
    q16 = next(c for c in CASES if c.kind == "quant16" and c.N == 64 and c.M == 3)
    yield "N_not_256", f32, lambda b: {"N": 384}, "gemm_f8"
    yield "K_not_128", f32, lambda b: {"K": 192}, "gemm_f8"
    yield "lda8_below_K", f32, lambda b: {"lda8": 240}, "gemm_f8"
    yield "lda8_not_16", f32, lambda b: {"lda8": 264}, "gemm_f8"
    yield "ldw8_not_16", f32, lambda b: {"ldw8": 264}, "gemm_f8"
    yield "a8_off_16_bytes", f32, lambda b: {"a8": _off(X.ptr_tensor(b, "a8"), 8)}, "16-byte"
    yield "w8_off_16_bytes", f32, lambda b: {"w8": _off(X.ptr_tensor(b, "w8"), 8)}, "16-byte"
    yield "a_scales_off_4_bytes", f32, lambda b: {"as": _off(X.ptr_tensor(b, "as"), 2)}, "4-byte"
    yield "w_scales_off_4_bytes", f32, lambda b: {"ws": _off(X.ptr_tensor(b, "ws"), 2)}, "4-byte"
    yield "f32_without_out", f32, lambda b: {"out_f32": None}, "gemm_f8(f32)"
    yield "f32_ldo_below_N", f32, lambda b: {"ldo": 256}, "gemm_f8(f32)"
    yield "bf16_ldo_not_8", bf, lambda b: {"ldo": 516}, "gemm_f8(bf16)"
    yield "bf16_out_off_16_bytes", bf, lambda b: {"out_bf": _off(b["out_bf"].ptr_tensor(), 4)}, "gemm_f8(bf16)"
    yield "bf16_without_out", bf, lambda b: {"out_bf": None}, "gemm_f8(bf16)"
    yield "gelu_without_out8s", gelu, lambda b: {"out8s": None}, "gemm_f8(gelu)"
    yield "gelu_ldo8_not_8", gelu, lambda b: {"ldo": 516}, "gemm_f8(gelu)"
    yield "gelu_out8_off_8_bytes", gelu, lambda b: {"out8": _off(b["out8"].ptr_tensor(), 4)}, "gemm_f8(gelu)"
    yield "resid_ldo_not_4", res, lambda b: {"ldo": 514}, "gemm_f8(resid)"
    yield "resid_out_off_16_bytes", res, lambda b: {"out_f32": _off(b["out_f32"].ptr_tensor(), 2)}, "gemm_f8(resid)"
    yield "resid_gate_off_16_bytes", res, lambda b: {"gate": _off(b["gate"], 1)}, "gemm_f8(resid)"
    yield "resid_without_gate", res, lambda b: {"gate": None}, "gemm_f8(resid)"
    yield "epilogue_5_through_gemm_f8", f32, lambda b: {"epi": 5}, "f5_op_gemm_f8"
    yield "qkv_heads_not_dmodel_64", qkv, lambda b: {"heads": 3}, "gemm_f8(qkv)"
    yield "qkv_npad_below_seq_len", qkv, lambda b: {"npad": 64}, "gemm_f8(qkv)"
    yield "qkv_qk_off_16_bytes", qkv, lambda b: {"qk": _off(b["qk"].ptr_tensor(), 4)}, "gemm_f8(qkv)"
    yield "qkv_without_vt", qkv, lambda b: {"vt": None}, "gemm_f8(qkv)"
    yield "qkv_lda8_not_16", qkv, lambda b: {"lda8": 264}, "gemm_f8"
    yield "ln_dim_1280", ln, lambda b: {"cols": 1280}, "ln_modulate_f8"
    yield "ln_dim_128", ln, lambda b: {"cols": 128}, "ln_modulate_f8"
    yield "ln_x_off_16_bytes", ln, lambda b: {"x": _off(b["x_dev"], 1)}, "ln_modulate_f8"
    yield "quantize_mx_cols_48", qf, lambda b: {"cols": 48}, "quantize_mx"
    yield "quantize_mx_ldx_below_cols", qf, lambda b: {"ldx": 32}, "quantize_mx"
    yield "quantize_mx_x_off_16_bytes", qf, lambda b: {"x": _off(b["x_dev"][X.GUARD:], 1)}, "quantize_mx"
    yield "quantize_mx_bf16_cols_48", q16, lambda b: {"cols": 48}, "quantize_mx_bf16"
    yield "quantize_mx_bf16_ldq_not_4", q16, lambda b: {"ldq": 66}, "quantize_mx_bf16"
    yield "quantize_mx_bf16_x_off_8_bytes", q16, lambda b: {"x": _off(b["x_dev"][X.GUARD:], 1)}, "quantize_mx_bf16"


@pytest.mark.parametrize("name,c,twist,where", list(_refusals()), ids=[r[0] for r in _refusals()])
def test_illegal_requests_are_refused_and_touch_nothing(lib, name, c, twist, where):
    """the buffers are made for the legal case and one argument is bent; the launcher answers before anything reaches the GPU"""
    b = X.make_buffers(c, device=DEV)
    with operand_mode(c.op if c.kind == "quant16" else "bf16"):
        rc = LAUNCH[c.kind](lib, b, **twist(b))
        msg = lib.f5_last_error().decode()
    torch.cuda.synchronize()
    print(f"[mxfp8 matrix] refusal {name}: rc={rc} error={msg!r}")
    assert rc != 0 and where in msg, (name, rc, msg)
    for k in ("out_f32", "out_bf", "out8", "out8s", "qk", "vt", "q", "qs"):
        if k in b:
            assert b[k].guard_damage(interior_too=True) == 0, (name, k)
