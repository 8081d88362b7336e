"""Cases, launchers and row digests for the tails of the two in-workgroup split kernels: ring_ks2<1> (csrc/gemm.hip, two wave groups
split the K tiles) and f5_attn2s_kernel (csrc/attention.hip, two or four wave groups split the KV tiles).

Both kernels end by summing the groups' partial results through LDS.  Who adds what, and which wave stores it, may change; the bits may
not: the sum of a GEMM element is acc_0 + acc_1 in group order, the attention merge keeps its expressions.  So the expected values here
are not computed but RECORDED: tools/record_split_tail.py runs every case below through the library of the commit BEFORE the tails were
shared out among the groups and writes tests/golden/split_tail_parent.npz; tests/test_split_tail_gpu.py compares bitwise against it, and
checks every launch against the fp64 references and bounds of tests/gemm_matrix.py / tests/attention_matrix.py as well, so that a bad
recording cannot hide.

What is recorded per case is one 64-bit digest per output row and output, sum over the columns of (bit pattern x an odd 64-bit weight
of the column) mod 2^64: two rows that differ in any bit have different digests unless 2^-64 luck intervenes, a mismatch still names the
row, and the whole table of 336 launches stays at a few hundred KB (the outputs themselves are about 15 MB).

Shared by the test and the recorder; needs no GPU to import."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

import attention_matrix as AM
import gemm_matrix as GM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_tail_parent.npz")

# ---- the GEMM cases: selector 10 forces ring_ks2<1> (64x128 block tile, wave tile 32x64 = two 32-column blocks, one per group) ---------
GEMM_PRECISIONS = {"f16": ("f16", 1), "bf16x3": ("bf16", 3)}         # name -> (operand type, nseg)
GEMM_MS = (1, 63, 64, 65, 130)          # one row; a row short of, exactly, and one row past the block tile; three row tiles, ragged
GEMM_NS = (100, 128, 256)               # a partial column tile (the last block, one of group 1's, is cut after 4 columns); one tile; two
GEMM_KS = (64, 128, 192, 1024)          # one K tile (group 1 owns none), one each, two and one (fewer than ring stages), the model's
GEMM_EPIS = ("RESID_GATE", "ADDROWS", "F32")     # the preloaded residual update (keep bytes, ldo > N), the staged-or-direct 16-bit pair, plain
GEMM_KERNEL = "ring_ks2<1>"


def gemm_cases(prec, epi):
    op, nseg = GEMM_PRECISIONS[prec]
    ns = (100,) if epi == "F32" else GEMM_NS              # final_proj's shape class: N = 100 only
    return [GM.make_case(op, 10, epi, nseg, M, N, K) for M in GEMM_MS for N in ns for K in GEMM_KS]


# ---- the attention cases -------------------------------------------------------------------------------------------------------------
# name -> (operand type, route of tests/attention_matrix.py, kernel): one-pass fp16 with two and four groups, bf16x3 with two (a forced
# split of four falls through to the same two-group kernel there: the launcher has no other)
ATTN_VARIANTS = {"f16-ks2": ("f16", "v2s_ks2", AM.V2S_KS2), "f16-ks4": ("f16", "v2s_ks4", AM.V2S_KS4),
                 "bf16x3-ks2": ("bf16", "v2s_hp", AM.V2S_HP), "bf16x3-ks4": ("bf16", "fall_ks4_hp", AM.V2S_HP)}
ATTN_NS = (1, 31, 33, 64, 65, 130, 499)      # one query; around half a tile and a tile; two query blocks; eight KV tiles, fill 51


def attn_cases(variant):
    """B H = 3 both ways: three heads of one sequence without kv_len, three sequences of one head with ragged kv_len -- the first keeps
    all N keys, the others stop after 1 ... N - 1 (tests/attention_matrix.py ragged), which leaves groups of those workgroups without a
    tile.  make_case never hands out the tight leading dimensions: ldo = 64 H + 4, + 8 or + 12."""
    op, route, _ = ATTN_VARIANTS[variant]
    out = []
    for i, N in enumerate(ATTN_NS):
        out.append(AM.make_case(op, route, 1, 3, N, 0, "gauss", i, qpre=i & 1))
        out.append(AM.make_case(op, route, 3, 1, N, 2, "gauss", i + 1, qpre=(i + 1) & 1))
    return out


# ---- digests ---------------------------------------------------------------------------------------------------------------------------
_GOLDEN_RATIO = 0x9E3779B97F4A7C15 - (1 << 64)      # the odd 64-bit constant of Fibonacci hashing, as a signed value


def _weights(n, device):
    w = (torch.arange(n, dtype=torch.int64, device=device) + 1) * _GOLDEN_RATIO     # int64 arithmetic wraps mod 2^64
    return (w ^ (w >> 29)) | 1


def row_digests(view):
    """[M][N] tensor of 16- or 32-bit elements -> [M] int64"""
    bits = view.contiguous().view(torch.int16 if view.element_size() == 2 else torch.int32).to(torch.int64)
    bits = bits & (0xFFFF if view.element_size() == 2 else 0xFFFFFFFF)
    return (bits * _weights(view.shape[1], view.device)[None, :]).sum(dim=1)


def digests(b, owned):
    """the owned outputs of a launch -> [len(owned)][M] int64 on the CPU"""
    return torch.stack([row_digests(b[name].view) for name in owned]).cpu().numpy()


# ---- launchers (the same calls as tests/test_gemm_matrix_gpu.py / tests/test_attention_matrix_gpu.py) -----------------------------------
def _last(fn):
    buf = C.create_string_buffer(64)
    fn(buf, 64)
    return buf.value.decode()


def run_gemm(lib, E, c, device, stream):
    """-> (buffers, kernel name); the caller holds the operand mode"""
    P = E.ptr
    b = GM.make_buffers(c, device=device)
    lo = (lambda t: t) if c.nseg == 3 else (lambda t: None)
    a_hi, a_lo, w_hi, w_lo = b["a"][0], lo(b["a"][1]), b["w"][0], lo(b["w"][1])
    of, oh, ol = b["out_f32"].ptr_tensor(), b["out_hi"].ptr_tensor(), b["out_lo"].ptr_tensor()
    E.check(lib.f5_debug_set_gemm_tile(c.sel))
    try:
        if c.epi == "RESID_GATE":
            rc = lib.f5_op_gemm_resid_gate(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(b["gate"]), P(b["keep"]), P(of), c.M, c.N, c.K,
                                           c.lda, c.ldw, c.ldo, c.nseg, stream)
        elif c.epi == "ADDROWS":
            rc = lib.f5_op_gemm_addrows(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["addrows"].ptr_tensor()), c.a_row_mod, P(of), P(oh),
                                        P(ol if c.nseg == 3 else None), c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.nseg, stream)
        else:
            rc = lib.f5_op_gemm(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(of), P(oh), P(ol if c.nseg == 3 else None), c.M, c.N, c.K,
                                c.lda, c.ldw, c.ldo, c.nseg, GM.EPI[c.epi], stream)
        name = _last(lib.f5_debug_last_gemm_kernel)
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))
    assert rc == 0, lib.f5_last_error().decode()
    torch.cuda.synchronize()
    return b, name


def run_attn(lib, E, c, device, stream):
    """-> (buffers, kernel name); the caller holds the operand mode"""
    P = E.ptr
    b = AM.make_buffers(c, device=device)
    hp, pipe, wide, kvsplit = c.knobs
    E.check(lib.f5_debug_set_attn_pipe(0))
    E.check(lib.f5_debug_set_attn_wide(wide))
    E.check(lib.f5_debug_set_attn_kvsplit(kvsplit))
    try:
        rc = lib.f5_op_attention_ex(P(AM.qk_ptr_tensor(b, 0)), P(AM.qk_ptr_tensor(b, 1) if hp else None), P(AM.vt_ptr_tensor(b, 0)),
                                    P(AM.vt_ptr_tensor(b, 1) if hp else None), P(b["out_hi"].ptr_tensor()), P(b["out_lo"].ptr_tensor()), P(b["kv"]),
                                    c.B, c.H, c.N, c.npad, c.D, C.c_float(AM.SCALE), hp, c.ldqk, c.ldo, c.qpre, pipe, P(None), P(None), c.ldo8,
                                    stream)
        name = _last(lib.f5_debug_last_attn_kernel)
    finally:
        E.check(lib.f5_debug_set_attn_wide(-1))
        E.check(lib.f5_debug_set_attn_kvsplit(-1))
    assert rc == 0, lib.f5_last_error().decode()
    torch.cuda.synchronize()
    return b, name


def all_groups():
    """(key, kind, cases) of every group of cases, in a fixed order"""
    out = [(f"gemm-{prec}-{epi}", "gemm", gemm_cases(prec, epi)) for prec in GEMM_PRECISIONS for epi in GEMM_EPIS]
    out += [(f"attn-{v}", "attn", attn_cases(v)) for v in ATTN_VARIANTS]
    return out


def run(lib, E, kind, c, device, stream):
    """one case -> (buffers, kernel name, the kernel the case must reach, findings of the fp64 check, digests)"""
    if kind == "gemm":
        b, name = run_gemm(lib, E, c, device, stream)
        return b, name, GEMM_KERNEL, GM.check(b), digests(b, GM.owned_outputs(c))
    b, name = run_attn(lib, E, c, device, stream)
    return b, name, c.kernel_name, AM.check(b), digests(b, AM.owned_outputs(c))


def record(lib, E, device, stream, operand_mode):
    """run every case through `lib` -> {group key: the digests of its cases, flattened and concatenated in case order}"""
    rec = {}
    for key, kind, cs in all_groups():
        parts = []
        for c in cs:
            with operand_mode(c.op):
                _, name, want, bad, dg = run(lib, E, kind, c, device, stream)
            assert name == want and not bad, (c.id, name, bad)
            parts.append(dg.reshape(-1))
        rec[key] = np.concatenate(parts)
    return rec


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
