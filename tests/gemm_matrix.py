"""The GEMM test matrix: case generator, buffers with guards and poison, fp64 reference, tolerances and checker.

Shared by tests/test_gemm_matrix_gpu.py (runs the cases through the C ABI) and tests/test_gemm_matrix_host.py (runs the checker
over a torch emulation of the kernels, right and deliberately wrong, on the CPU).  Nothing here needs a GPU or the library.

A case is (operand type, tile selector, epilogue, nseg, M, N, K) plus the leading dimensions it is launched with.  The shapes are
derived from the selector's block tile, the leading dimensions are never the tight ones, every output is a view into a larger
allocation whose surroundings must come back bit-identical, and the pad columns of the operands hold NaN.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace

import torch

# ---- epilogues (csrc/common.hpp F5Epi) and the entry point that reaches each ------------------------------------------------
EPI = {"F32": 0, "BF16": 1, "GELU_TANH": 2, "GELU_ERF": 3, "RESID_GATE": 4, "ADDROWS": 6, "RESID_KEEP": 7, "GELU_ERF_BF16": 8}
EPIS = tuple(EPI)
OUT16 = ("BF16", "GELU_TANH", "GELU_ERF_BF16")            # 16-bit output only
RS128_EPIS = ("F32", "BF16", "GELU_TANH", "RESID_GATE")   # gemm_rs128.hip implements these (and QKV_ROPE, not in this matrix)
WIDE_EPIS = ("BF16", "GELU_TANH")                         # the 128x256 ring tiles are instantiated for these (and QKV_ROPE)
OPS = ("bf16", "f16")
SELECTORS = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14)
ANY_N = (0, 1, 2, 3, 5, 6, 10, 11)
# block tile (BM, BN) of the kernel a selector forces; 0 (auto) ends on the 64x64 ring at small shapes
TILE = {0: (64, 64), 1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (256, 256), 5: (64, 128), 6: (64, 64), 8: (128, 192), 9: (128, 128),
        10: (64, 128), 11: (128, 128), 12: (128, 256), 13: (128, 256), 14: (128, 256)}
KS = (64, 128, 192, 1024)      # one K tile (fewer than ring stages; a split-K group that owns none), two, an odd count, the model's

GUARD = 64                     # guard rows in front of and behind every output
SENT32 = 0x7FC0BEEF            # fp32 sentinel: a NaN with a payload
SENT16 = 0x7FA5                # 16-bit sentinel: a NaN in bf16 and in fp16
W_TAIL = 3.0e4                 # weight rows N ... ceil128(N) - 1 (the kernels may read them): large, finite in both operand types


def cdiv(a, b):
    return -(-a // b)


def eps_op(op):
    """largest relative error of ONE round-to-nearest into the operand type: bf16 has 8 significand bits, fp16 11"""
    return 2.0 ** -8 if op == "bf16" else 2.0 ** -11


def op_dtype(op):
    return torch.bfloat16 if op == "bf16" else torch.float16


@dataclass(frozen=True)
class Case:
    op: str
    sel: int
    epi: str
    nseg: int
    M: int
    N: int
    K: int
    lda: int
    ldw: int
    ldo: int          # ldx / ldres / ldadd likewise
    ring: int = 1     # f5_debug_set_gemm_ring: 0 = the register-staged small tiles instead of the global_load_lds ring
    a_row_mod: int = 0
    note: str = ""

    @property
    def kernel(self):
        return expected_kernel(self.sel, self.epi, self.M, self.N, self.ring)

    @property
    def id(self):
        return (f"{self.op}-{self.kernel}-sel{self.sel}{'' if self.ring else '-noring'}-{self.epi}-nseg{self.nseg}-"
                f"M{self.M}-N{self.N}-K{self.K}")

    @property
    def group(self):
        return (self.op, self.kernel, self.sel, self.ring, self.epi, self.nseg)


def expected_kernel(sel, epi, M, N, ring=1, *, seq_len=0, g4=False, qkv_tile=0):
    """What f5_launch_gemm resolves a launch to (the base name, without the +variant suffixes); None = it refuses the launch.  The rule
    itself is csrc/gemm_route.hpp f5_gemm_route; this is its mirror, written out by hand so that the two can be compared point by
    point (tests/test_gemm_route_host.py) and the launcher checked against it (tests/test_gemm_matrix_gpu.py).  The keyword arguments matter for epi "QKV_ROPE" only
    (not an epilogue of this matrix): seq_len = rows per batch element, g4 = the group-major rotation tables are set, qkv_tile = the
    f5_debug_set_gemm_qkv_tile knob."""
    qkv = epi == "QKV_ROPE"
    t128, t64, t256 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 64) * cdiv(N, 128), cdiv(M, 256) * (N // 256)
    v2ok = N % 256 == 0 and M >= 256
    if sel == 4 or (sel == 0 and v2ok and t256 >= 512):
        return "gemm256" if v2ok else None
    if epi in RS128_EPIS or qkv:
        t128x256 = cdiv(M, 128) * (N // 256)
        if qkv and seq_len > 0:
            t128x256 = (M // seq_len) * cdiv(seq_len, 128) * (N // 256)       # the role-split QKV epilogue deals row tiles per batch element
        rows_ok = not qkv or (seq_len > 0 and M % seq_len == 0)
        qkv14 = qkv and sel == 0 and rows_ok and g4 and t128x256 <= 256 and (qkv_tile == 14 or (qkv_tile == 0 and t128x256 >= 176))
        mid = sel == 0 and t128 >= 384 and rows_ok
        if (sel == 14 or qkv14 or mid) and N % 256 == 0:
            return "rs128" if rows_ok else None          # selector 14 with a ragged M % seq_len: f5_launch_gemm_rs128 refuses it
        if sel == 14:
            sel = 0
    if qkv and sel == 0 and qkv_tile in (12, 13) and g4 and N % 256 == 0 and cdiv(M, 128) * (N // 256) <= 256:
        sel = qkv_tile
    if sel in (12, 13):
        if (epi in WIDE_EPIS or qkv) and N % 256 == 0:
            return "ring_wide<2,2,2,4>" if sel == 12 else "ring_wide<1,4,4,2>"
        sel = 0
    if sel in (10, 11):
        return "ring_ks2<1>" if sel == 10 else "ring_ks2<2>"
    if sel in (8, 9):
        if N % (192 if sel == 8 else 128) == 0:
            return "ring8<3>" if sel == 8 else "ring8<2>"
        sel = 0
    if sel == 0 and ring:
        if N % 128 == 0 and 176 <= t128 <= 256:
            return "ring8<2>"
        if 176 <= t64 <= 256:
            return "ring_ks2<1>"
    if sel in (0, 4):
        sel = 1 if t128 >= 384 else (2 if t64 >= 384 else 3)
    if qkv and sel == 3:
        sel = 2
    if qkv and sel == 6:
        sel = 5                   # the V^T / head mapping wants >= one whole head per tile column
    if sel == 5:
        return "ring<1,2>"
    if sel == 6:
        return "ring<1,1>"
    if sel == 1:
        return "cfg<2,2>"
    if ring:
        if sel == 2 and 512 < t64 <= 768:
            return "cfg<1,2>"
        return "ring<1,2>" if sel == 2 else "ring<1,1>"      # selector 14 with an epilogue gemm_rs128.hip lacks ends here too
    return "cfg<1,2>" if sel == 2 else "cfg<1,1>"


def leading_dims(epi, N, K):
    """Never the tight ones.  lda / ldw must be multiples of 8 (gemm.hpp); the 16-bit outputs are written as 16-byte chunks by the
    staged epilogues, so their rows must start on 16 bytes: ldo is a multiple of 8 wherever a 16-bit output exists (BF16, GELU_TANH,
    GELU_ERF_BF16, ADDROWS), N + 8 otherwise (every N of the matrix that has a whole column tile is a multiple of 4, which keeps the
    fp32 rows of the staged epilogues on 16 bytes as well; N = 1 has only partial tiles, which are written element by element)."""
    ldo = (cdiv(N, 8) * 8 + 8) if (epi in OUT16 or epi == "ADDROWS") else N + 8
    return K + 8, K + 16, ldo


def make_case(op, sel, epi, nseg, M, N, K, ring=1, note=""):
    lda, ldw, ldo = leading_dims(epi, N, K)
    return Case(op, sel, epi, nseg, M, N, K, lda, ldw, ldo, ring, (M + 1) // 2 if epi == "ADDROWS" else 0, note)


def shape_classes(sel):
    """(Ms, Ns) of a selector, from its block tile: row counts around one tile and a ragged several-tile one; the smallest N the
    kernel takes and a multi-tile one, plus N = 100 / 200 (partial column tiles) where it takes any N."""
    bm, bn = TILE[sel]
    ms = [1, bm - 1, bm, bm + 1, 3 * bm + 37]
    if sel == 4:
        ms = [m for m in ms if m >= 256]        # the 256x256 kernel needs M >= 256
    ns = [1, 2 * bn + 128 if bn < 128 else 3 * 128, 100, 200] if sel in ANY_N else [bn, 3 * bn if bn == 192 else 2 * bn]
    return ms, ns


def cases():
    """the whole matrix, in a fixed order"""
    out = []
    for op in OPS:
        for sel in SELECTORS:
            ms, ns = shape_classes(sel)
            for epi in EPIS:
                for nseg in (1, 3):
                    for M in ms:
                        for N in ns:
                            for K in KS:
                                out.append(make_case(op, sel, epi, nseg, M, N, K))
                    # the register-staged 64x128 / 64x64 kernels: selectors 2 / 3 run the ring kernels unless the ring is switched off
                    # (with it on, 64x128 is only chosen between 512 and 768 tiles, the batch-1 QKV projection)
                    if sel in (2, 3):
                        for M in ms:
                            for N in (100, 256):
                                for K in (64, 192):
                                    out.append(make_case(op, sel, epi, nseg, M, N, K, ring=0, note="ring off"))
                    if sel == 2:
                        out.append(make_case(op, sel, epi, nseg, 2100, 2048, 64, note="528 tiles of 64x128: the register-staged kernel"))
    return out


# ---- shape tables shared by the GPU matrix (tests/test_gemm_matrix_gpu.py) and the routing test on the CPU (tests/test_gemm_route_host.py)
# forced selectors the dispatcher does not honour for this (epilogue, N): (selector, epilogue, M, N)
FALLBACKS = [(8, "F32", 300, 256), (8, "RESID_KEEP", 300, 512), (9, "BF16", 300, 192), (12, "BF16", 300, 384), (13, "GELU_TANH", 300, 384),
             (12, "RESID_GATE", 300, 256), (13, "F32", 300, 512), (12, "ADDROWS", 300, 256), (14, "RESID_GATE", 300, 384), (14, "F32", 300, 100),
             (14, "ADDROWS", 300, 256), (14, "RESID_KEEP", 300, 512), (14, "GELU_ERF", 300, 256), (14, "GELU_ERF_BF16", 300, 256)]
# selector 4 (the 256x256 kernel) at shapes it cannot run: the launch is refused
SEL4_REFUSALS = [("sel4_M_below_256", make_case("bf16", 4, "F32", 1, 255, 256, 128)), ("sel4_N_not_256", make_case("bf16", 4, "F32", 1, 300, 384, 128)),
                 ("sel4_N_100_resid_gate", make_case("f16", 4, "RESID_GATE", 1, 300, 100, 128))]
# every GEMM launch of prepare / run_dit for the 335M configuration at 937 frames, M = 2 x B x 937 rows: (name, epilogue, N, K)
PRODUCTION = [("hoisted_proj", "F32", 1024, 128 + 512), ("text_pw1", "GELU_ERF", 1024, 512), ("text_pw2", "RESID_KEEP", 512, 1024),
              ("input_proj", "ADDROWS", 1024, 128), ("attn_out", "RESID_GATE", 1024, 1024), ("ff1", "GELU_TANH", 2048, 1024),
              ("ff2", "RESID_GATE", 1024, 2048), ("final_proj", "F32", 100, 1024)]
# what f5_gemm_route's comments (csrc/gemm_route.hpp) promise for the block GEMMs: batch 1 one round of 8-wave workgroups (128x128 for FF1, split-K 64x128 for
# the out-projection and FF2), the role-split 128x256 kernel at the mid sizes, the 256x256 kernel at batch 32
PROMISED = {1: {"attn_out": "ring_ks2<1>", "ff1": "ring8<2>", "ff2": "ring_ks2<1>", "input_proj": "ring_ks2<1>"},
            8: {"attn_out": "rs128", "ff1": "rs128", "ff2": "rs128", "final_proj": "ring_ks2<1>"},
            32: {"attn_out": "gemm256", "ff1": "gemm256", "ff2": "gemm256"}}


# ---- buffers ---------------------------------------------------------------------------------------------------------------
def _rand(gen, *shape, scale=1.0, device="cpu"):
    return torch.randn(*shape, generator=gen, device=device, dtype=torch.float32) * scale


def _round_op(x, op):
    return (x.clamp(-65504.0, 65504.0) if op == "f16" else x).to(op_dtype(op))


def _split(x, op):
    hi = _round_op(x, op)
    lo = (x - hi.float()).to(op_dtype(op))
    return hi, lo


def _operand(x, ld, rows, op, tail=None):
    """[rows][ld] operand pair holding x in its top-left corner: pad columns NaN, rows past x `tail` (large finite)"""
    r, k = x.shape
    hi, lo = _split(x, op)
    bufs = []
    for part in (hi, lo):
        b = torch.full((rows, ld), float("nan"), dtype=op_dtype(op), device=x.device)
        if rows > r:
            b[r:, :k] = tail
        b[:r, :k] = part
        bufs.append(b)
    return bufs


class Guarded:
    """an [M][N] output inside a [GUARD + M + GUARD][ld] allocation full of a sentinel bit pattern"""

    def __init__(self, M, N, ld, dtype, device, init=None):
        self.M, self.N, self.ld = M, N, ld
        self.ibits = torch.int32 if dtype == torch.float32 else torch.int16
        sent = SENT32 if dtype == torch.float32 else SENT16
        self.alloc = torch.full((2 * GUARD + M, ld), sent, dtype=self.ibits, device=device).view(dtype)
        if init is not None:
            self.view[:] = init
        self.before = self.alloc.clone()

    @property
    def view(self):
        return self.alloc[GUARD:GUARD + self.M, :self.N]

    def ptr_tensor(self):
        return self.alloc[GUARD:]            # data_ptr() of this is the address of view[0][0]

    def guard_damage(self, interior_too=False):
        """number of elements outside the [M][N] interior (or anywhere) whose bits changed"""
        diff = self.alloc.view(self.ibits) != self.before.view(self.ibits)
        if not interior_too:
            diff[GUARD:GUARD + self.M, :self.N] = False
        return int(diff.sum())


def make_buffers(c: Case, device="cpu", seed=None):
    """operands, epilogue inputs and guarded outputs of a case; deterministic in the case"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed if seed is not None else zlib.crc32(c.id.encode()))
    M, N, K, op = c.M, c.N, c.K, c.op
    a_rows = c.a_row_mod if c.a_row_mod > 0 else M
    b = {"case": c}
    b["a32"] = _rand(gen, a_rows, K, device=device)
    b["w32"] = _rand(gen, N, K, scale=K ** -0.5, device=device)
    b["a"] = _operand(b["a32"], c.lda, a_rows, op)
    b["w"] = _operand(b["w32"], c.ldw, cdiv(N, 128) * 128, op, tail=W_TAIL)
    b["bias"] = _rand(gen, N, scale=0.3, device=device) if c.epi != "ADDROWS" else None
    b["gate"] = _rand(gen, N, device=device) if c.epi == "RESID_GATE" else None
    keep = None
    if c.epi in ("RESID_GATE", "RESID_KEEP"):
        keep = (torch.rand(M, generator=gen, device=device) > 0.3).to(torch.uint8)
        keep[M - 1] = 1                 # the last row of a ragged tile is live ...
        if M >= 2:
            keep[0] = 0                 # ... and at least one row is masked
    b["keep"] = keep
    f32, o16 = torch.float32, op_dtype(op)
    x0 = _rand(gen, M, N, device=device) if c.epi == "RESID_GATE" else None
    b["x0"] = x0
    b["resid"] = Guarded(M, N, c.ldo, f32, device, init=_rand(gen, M, N, device=device)) if c.epi == "RESID_KEEP" else None
    b["addrows"] = Guarded(M, N, c.ldo, f32, device, init=_rand(gen, M, N, device=device)) if c.epi == "ADDROWS" else None
    b["out_f32"] = Guarded(M, N, c.ldo, f32, device, init=x0)
    b["out_hi"] = Guarded(M, N, c.ldo, o16, device)
    b["out_lo"] = Guarded(M, N, c.ldo, o16, device)
    return b


def owned_outputs(c: Case):
    """which of (out_f32, out_hi, out_lo) the epilogue writes"""
    if c.epi in OUT16:
        return ("out_hi", "out_lo") if c.nseg == 3 else ("out_hi",)
    if c.epi == "ADDROWS":
        return ("out_f32", "out_hi", "out_lo") if c.nseg == 3 else ("out_f32", "out_hi")
    return ("out_f32",)


# ---- reference -------------------------------------------------------------------------------------------------------------
def _gelu(pre, kind):
    return torch.nn.functional.gelu(pre, approximate="tanh") if kind == "tanh" else torch.nn.functional.gelu(pre)


def reference(b, rows=None):
    """fp64 of the same operation: from the operands rounded to the operand type (nseg 1) or the fp32 inputs (nseg 3).
    rows: optional index tensor -> only those rows (the production-shape table samples rows above 15 000)"""
    c = b["case"]
    idx = torch.arange(c.M, device=b["a32"].device) if rows is None else rows
    arow = idx % c.a_row_mod if c.a_row_mod > 0 else idx
    a = b["a32"][arow]
    a = (a if c.nseg == 3 else _round_op(a, c.op).float()).double()
    w = (b["w32"] if c.nseg == 3 else _round_op(b["w32"], c.op).float()).double()
    acc = a @ w.T
    pre = acc + b["bias"].double() if b["bias"] is not None else acc
    e = c.epi
    if e in ("F32", "BF16"):
        return pre
    if e == "GELU_TANH":
        return _gelu(pre, "tanh")
    if e in ("GELU_ERF", "GELU_ERF_BF16"):
        return _gelu(pre, "erf")
    if e == "RESID_GATE":
        return b["x0"][idx].double() + b["gate"].double() * (pre * b["keep"][idx].double()[:, None])
    if e == "ADDROWS":
        return acc + b["addrows"].view[idx].double()
    if e == "RESID_KEEP":
        return (b["resid"].view[idx].double() + pre) * b["keep"][idx].double()[:, None]
    raise ValueError(e)


# ---- tolerances: functions of the operand type, written once -----------------------------------------------------------------
def tol_f32(c: Case, refmax):
    """fp32 outputs: the project's bounds -- one-pass operands against the SAME rounded operands 2e-4 of the output scale (fp32
    accumulation order only), three-pass against the fp32 inputs 5e-5 (the dropped lo x lo term and the split's rounding)."""
    return (2e-4 if c.nseg == 1 else 5e-5) * max(1.0, refmax)


def tol_16(c: Case, ref):
    """16-bit outputs, element-wise.  nseg 1: |got - ref| <= eps_op |ref| + floor -- ONE round-to-nearest of a value that is right to
    fp32 accuracy (floor = tol_f32; never less than the half spacing 2^-25 of the fp16 subnormals) cannot exceed it; rounding twice,
    truncating, or rounding through bf16 in the fp16 build does.  nseg 3 (hi + lo pairs): the project's 1e-4 of the output scale behind
    an activation, 5e-5 plain."""
    refmax = float(ref.abs().max())
    if c.nseg == 3:
        return torch.full_like(ref, (5e-5 if c.epi in ("BF16", "ADDROWS") else 1e-4) * max(1.0, refmax))
    return eps_op(c.op) * ref.abs() + max(tol_f32(c, refmax), 2.0 ** -25)


# ---- checker ---------------------------------------------------------------------------------------------------------------
def check(b, ref=None, rows=None):
    """-> list of findings (empty = the launch did what the reference says and touched nothing else)"""
    c = b["case"]
    bad = []
    owned = owned_outputs(c)
    for name in ("out_f32", "out_hi", "out_lo", "resid", "addrows"):
        g = b[name]
        if g is None:
            continue
        n = g.guard_damage(interior_too=name not in owned)
        if n:
            bad.append(f"{name}: {n} element(s) outside what the epilogue owns changed")
    if ref is None:
        ref = reference(b, rows)
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    refmax = float(ref.abs().max())
    if not bool(torch.isfinite(ref).all()):
        bad.append("reference not finite")

    def cmp(name, got, tol):
        d = (got.double() - ref).abs()
        ok = d <= tol
        if not bool(ok.all()):
            nbad = int((~ok).sum())
            i = int((~ok).reshape(-1).nonzero()[0])
            r_, c_ = divmod(i, ref.shape[1])
            t = tol if isinstance(tol, float) else float(tol.reshape(-1)[i])
            bad.append(f"{name}: {nbad} element(s) off, first at ({r_}, {c_}): got {float(got.reshape(-1)[i])!r} ref "
                       f"{float(ref.reshape(-1)[i])!r} tol {t:.3e}; max |err| {float(torch.nan_to_num(d, nan=float('inf')).max()):.3e}")

    if "out_f32" in owned:
        cmp("out_f32", sel(b["out_f32"].view), tol_f32(c, refmax))
    if "out_hi" in owned:
        hi = sel(b["out_hi"].view).float()
        if c.nseg == 3:
            cmp("out_hi+out_lo", hi.double() + sel(b["out_lo"].view).double(), tol_16(c, ref))
        else:
            cmp("out_hi", hi, tol_16(c, ref))
        if c.epi == "ADDROWS":         # the 16-bit copy is the rounding of the fp32 value that was written
            want = _round_op(sel(b["out_f32"].view), c.op)
            if not torch.equal(want.view(torch.int16), sel(b["out_hi"].view).contiguous().view(torch.int16)):
                bad.append("out_hi is not the rounding of out_f32")
    return bad


# ---- torch emulation of the kernels (CPU): the checker's own test ------------------------------------------------------------
FAULTS = ("tile_transposed", "last_row_missing", "row_past_M", "col_past_N", "a_pad_read", "f16_through_bf16", "truncated",
          "keep_ignored", "a_row_mod_ignored", "bias_twice")


def fault_applies(fault, c: Case):
    return {"tile_transposed": c.M >= 32 and c.N >= 32, "f16_through_bf16": c.op == "f16" and c.epi in OUT16 and c.nseg == 1 and c.M * c.N >= 4096,
            # (fp16: a truncation error only beats eps_op |ref| + floor on elements of the size of the largest: it takes many elements)
            "truncated": c.epi in OUT16 and c.nseg == 1 and c.M * c.N >= (4096 if c.op == "bf16" else 32768),
            "keep_ignored": c.epi in ("RESID_GATE", "RESID_KEEP") and c.M >= 2,
            "a_row_mod_ignored": c.epi == "ADDROWS" and c.M >= 3, "bias_twice": c.epi == "RESID_KEEP",
            "last_row_missing": c.M % TILE[c.sel][0] != 0}.get(fault, True)


def _truncate(x, op):
    """fp32 -> operand type by dropping the low bits (round toward zero)"""
    if op == "bf16":
        return (x.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    r = x.to(torch.float16)
    over = r.float().abs() > x.abs()
    bits = r.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16)


def emulate(b, fault=None):
    """Write the outputs as a kernel would: operand-typed products accumulated exactly and rounded once to fp32, the epilogue in fp32,
    one rounding into the 16-bit outputs.  `fault` = one of FAULTS makes it subtly wrong."""
    c = b["case"]
    M, N, K = c.M, c.N, c.K
    kk = K + 1 if fault == "a_pad_read" else K
    A = [t[:, :kk].double() for t in b["a"]]
    W = [t[:N, :kk].double() for t in b["w"]]
    rows = torch.arange(M)
    if c.a_row_mod > 0:
        rows = rows.clamp(max=c.a_row_mod - 1) if fault == "a_row_mod_ignored" else rows % c.a_row_mod
    acc = A[0][rows] @ W[0].T
    if c.nseg == 3:
        acc = acc + A[1][rows] @ W[0].T + A[0][rows] @ W[1].T
    acc = acc.float()
    if fault == "tile_transposed":
        acc[:32, :32] = acc[:32, :32].T.clone()
    e = c.epi
    keep = None
    if b["keep"] is not None:
        keep = torch.ones(M, 1) if fault == "keep_ignored" else b["keep"].float()[:, None]
    pre = acc + b["bias"] if b["bias"] is not None else acc
    if fault == "bias_twice":
        pre = pre + b["bias"]
    if e in ("F32", "BF16"):
        v = pre
    elif e == "GELU_TANH":
        v = _gelu(pre.double(), "tanh").float()
    elif e in ("GELU_ERF", "GELU_ERF_BF16"):
        v = _gelu(pre.double(), "erf").float()
    elif e == "RESID_GATE":
        v = b["x0"] + b["gate"] * (pre * keep)
    elif e == "ADDROWS":
        v = acc + b["addrows"].view
    else:
        v = (b["resid"].view + pre) * keep
    nrow = M - 1 if fault == "last_row_missing" else M

    def store(g, val):
        g.alloc[GUARD:GUARD + nrow, :N] = val[:nrow]
        if fault == "row_past_M":
            g.alloc[GUARD + M, :N] = val[M - 1]
        if fault == "col_past_N":
            g.alloc[GUARD:GUARD + M, N] = val[:, N - 1]

    owned = owned_outputs(c)
    if "out_f32" in owned:
        store(b["out_f32"], v)
    if "out_hi" in owned:
        if fault == "f16_through_bf16":
            hi = v.to(torch.bfloat16).float().to(torch.float16)
        elif fault == "truncated":
            hi = _truncate(v.contiguous(), c.op)
        else:
            hi = _round_op(v, c.op)
        store(b["out_hi"], hi)
        if "out_lo" in owned:
            store(b["out_lo"], (v - hi.float()).to(op_dtype(c.op)))


def with_dims(c: Case, **kw):
    return replace(c, **kw)
