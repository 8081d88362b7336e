"""The attention test matrix (csrc/attention.hip): case generator, poisoned and guarded buffers, fp64 reference, derived element-wise
bound, checker, a Python transcription of the launcher's routing rule, and a torch emulation of the kernels with seeded mistakes.

Shared by tests/test_attention_matrix_gpu.py (runs the cases through f5_op_attention_ex and compares the kernel the launch reached,
f5_debug_last_attn_kernel, with the transcription) and tests/test_attention_matrix_host.py (runs the checker over the emulation, right
and deliberately wrong, on the CPU).  Nothing here needs a GPU or the library.

A case is (operand type, route, B, H, N, kv_len, npad, leading dimensions, value class, fp8 output or not).  q, k and v are handed over
already in the operand type; the route through f5_op_qkv_rope is the GEMM matrix's business.  kv_len >= 1 is the contract of the
kernels (a row with no key has no softmax); zero is not a request the engine makes and is left out.

Buffers.  K rows kv_len[b] ... N - 1 are scaled so that their logit exceeds every legitimate one of the launch by MASK_MARGIN (natural
units) for every query (q's first head dimension is kept positive for that), and the V^T columns of those keys hold +-1e4: a mask that
lets one through owns the row.  All of it is finite: masking is p = 0 times V.  V^T columns N ... npad - 1 are zero (attention.hpp), the
pad columns of qk are NaN, NaN rows sit in front of the first and behind the last row of qk (the kernels clamp tail reads to row
seq_len - 1 of the batch element), and every output lies pre-filled with a sentinel between guard rows and pad columns that must come
back bit-identical, while the interior must have lost the sentinel everywhere.

Bound (element-wise, from the reference alone).  With u = eps_op(type), p_j the fp64 softmax weights, ref = sum p_j v_j,
A = sum p_j |v_j|, u32 = 2^-24:
  one-pass   u A        P is rounded once to the operand type for the P V product (f5_pack2_bounded); the row sum is taken from the
                        unrounded fp32 P, so nothing cancels
           + u |ref|    the one rounding of the output
  bf16x3     2 u^2 A    P = hi + lo with the residual rounded (u^2), and the dropped lo x lo term of P V (u^2)
           + u^2 |ref|  the output pair hi + lo, residual rounded
  both     + sum_j p_j ds_ij |v_j| + |ref| sum_j p_j ds_ij      a logit error ds moves p_j by the factor e^ds, in the numerator and in the
                        row sum (the issue's 2 ds A, kept per key);  ds_ij = u32 (64 (S|.|_ij + max_j |s_ij|) + 4 |s_ij|) + EXP2 2^-23
                        [+ u^2 S|.|_ij for bf16x3: the dropped q_lo k_lo term], with S|.| = sum_d |q_d k_d| in logit units:
                        64 fp32 additions of exact products on top of -m_ref (the C operand of the first MFMA in v2f<true> / v2p),
                        the rounding of c2 = scale * log2(e) (two: the constant and the product), of the fused multiply-add
                        s c2 - m c2 and of m c2, and the hardware exp2
           + (kv + 3 ntile + 16) u32 (A + |ref|)                fp32: kv additions into O and into l, one multiply per tile and
                        accumulator for the rescale (alpha itself cancels between O and l), the split merge, 1 / l and O / l
  fp16     + 2^-25 sum_j |v_j| / L + 2^-25                      P (or its lo half) below the fp16 normal range 2^-14 is rounded to a
                        multiple of 2^-24; every kernel takes P against a reference point m <= max_j s_ij (the running maximum, or
                        the standing point of the kernels without a tile maximum, which only moves up), so in units of the final
                        row sum L = sum_j e^(s_j - max s) >= 1 the error per key is at most 2^-25 / L; and an output below 2^-14
There is no max(1, .) floor and no fitted factor.  One-pass launches of 4096 elements or more are also held to a systematic-error
allowance: the slope of (got - ref) against ref stays within u / 4 plus what may push every element the same way (check() has the
reasoning); a P that is truncated or rounded twice tilts the output by about u and stays inside the element-wise bound.

exp2.  __builtin_amdgcn_exp2f measured on an MI355X with tools/probes/math_ulp.hip (2^21 arguments in [-60, 15]) against fp64:
    function       measured (ULP)   granted (ULP)
    amdgcn_exp2f   0.769            3.076
Four times the measurement is granted, as tests/rowops_matrix.py does for its transcendentals.

MX-fp8 output (attn_store_f8).  Dequantised with the scale byte the kernel wrote, every value lies within the one-pass bound without
its output-rounding term plus one e4m3 rounding at that scale (2^-4 relative, 2^-10 of the scale below the normal range), and the
byte is the one f5_mx_scale_byte (oracle/mx_oracle.py mx_scale_bytes) gives for some block maximum in [amax - bound, amax + bound].
"""
from __future__ import annotations

import math
import os
import sys
import zlib
from dataclasses import dataclass

import torch

from gemm_matrix import cdiv, eps_op, op_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mx_oracle as MX  # noqa: E402

OPS = ("bf16", "f16")
VALUES = ("gauss", "peaked", "spikes", "large_v")
SCALE = 0.125
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
U32 = 2.0 ** -24
EXP2_ULP_MEASURED = 0.769
EXP2_ULP = 4 * EXP2_ULP_MEASURED
GUARD = 8                      # guard rows in front of and behind qk, V^T and every output
SENT16 = 0x7FA5                # a NaN in bf16 and in fp16
SENT8 = 0x7F                   # e4m3fn NaN: the kernels clamp to +-448 and never write it
SENT8S = 0xFF                  # E8M0 NaN: f5_mx_scale_byte stops at 254
MASK_MARGIN = 300.0            # logit excess of a masked key over every legitimate one (natural units); at least 100 after the fp16 cap
MASK_V = 1.0e4
LARGE_V = 3.0e4
FILLS = (1, 31, 32, 33, 63, 64)

# ---- kernels and routing -------------------------------------------------------------------------------------------------------
V2_HP, V2 = "f5_attn2_kernel<true,0>", "f5_attn2_kernel<false,0>"
V2F_PRE, V2F, V2P = "f5_attn2f_kernel<true>", "f5_attn2f_kernel<false>", "f5_attn2p_kernel"
V2S_HP, V2S_KS2, V2S_KS4 = "f5_attn2s_kernel<true,2,2>", "f5_attn2s_kernel<false,2,3,true>", "f5_attn2s_kernel<false,4,2,true>"
KERNELS = (V2_HP, V2, V2F_PRE, V2F, V2P, V2S_HP, V2S_KS2, V2S_KS4)
F8_KERNELS = (V2, V2F_PRE, V2F, V2P, V2S_KS2, V2S_KS4)        # attn_store_f8 sits in the six one-pass kernels
WIDE_KERNELS = (V2F_PRE, V2F, V2P)                            # 256 queries per workgroup, two query blocks per wave
NO_TILE_MAX = (V2F_PRE, V2F, V2P, V2S_KS2, V2S_KS4)           # exponentials against a standing reference point, exact fallback
SPLIT = {V2S_HP: 2, V2S_KS2: 2, V2S_KS4: 4}
# route name -> (hp, pipe, wide, kvsplit, q_prescaled or None = either); the first eight reach one kernel each by the knobs that select it
ROUTES = {"v2_hp": (1, -1, 0, 1, None), "v2": (0, -1, 0, 1, None), "v2f_pre": (0, 0, 1, 1, 1), "v2f": (0, 0, 1, 1, 0), "v2p": (0, 1, 1, 1, 1),
          "v2s_hp": (1, -1, 0, 2, None), "v2s_ks2": (0, -1, 0, 2, None), "v2s_ks4": (0, -1, 0, 4, None),
          # requests the launcher does not honour: they fall through silently
          "fall_ks4_hp": (1, -1, 0, 4, 0), "fall_pipe_plain_q": (0, 1, 1, 1, 0), "fall_wide_hp": (1, -1, 1, 1, 0), "fall_wide_ks2": (0, -1, 1, 2, 1),
          "auto": (0, -1, -1, -1, None), "auto_hp": (1, -1, -1, -1, 0), "auto_pipe": (0, 1, -1, -1, 1)}
FALL_THROUGHS = {"fall_ks4_hp": V2S_HP, "fall_pipe_plain_q": V2F, "fall_wide_hp": V2_HP, "fall_wide_ks2": V2S_KS2}


def expected_kernel(B, H, N, hp, q_prescaled, pipe=-1, wide=-1, kvsplit=-1, pipe_default=0):
    """f5_launch_attention's rule (csrc/attention.hip), transcribed by hand: which instantiation a legal launch reaches under the
    knobs f5_debug_set_attn_wide / _kvsplit / _pipe (pipe_default).  The GPU test compares it with the hook on every launch."""
    ks = kvsplit
    if ks < 0:
        wgs, ntile = cdiv(N, 128) * B * H, cdiv(N, 64)
        ks = 4 if (wgs <= 160 and ntile >= 8) else (2 if (wgs <= 320 and ntile >= 4) else 1)
    if not hp and ks <= 1 and (wide >= 1 or (wide < 0 and cdiv(N, 256) * B * H >= 512)):
        if (pipe_default if pipe < 0 else pipe) and q_prescaled:
            return V2P
        return V2F_PRE if q_prescaled else V2F
    if ks > 1:
        return V2S_HP if hp else (V2S_KS4 if ks >= 4 else V2S_KS2)
    return V2_HP if hp else V2


# (route, B, H, N, q_prescaled, expected kernel, note): the automatic rule on either side of each threshold.  Workgroups = ceil(N / 128) B H.
# 161 = 7 x 23 needs seven query blocks: the one case of the matrix above N = 704 that is not a wide kernel's (N = 769, 13 tiles); below
# it the far side is the next reachable count (164 / 165 with four / five query blocks).  321 = 3 x 107 cannot occur at exactly 4 tiles
# (two query blocks): 322 is launched there and 321 at 5 tiles; the transcription is asserted at all the exact points in
# tests/test_attention_matrix_host.py.
AUTO = (("auto", 512, 1, 64, 1, V2F_PRE, "512 wide workgroups"), ("auto", 511, 1, 64, 1, V2, "511 wide workgroups"),
        ("auto", 256, 2, 33, 0, V2F, "512 wide workgroups, plain q"), ("auto_pipe", 512, 1, 64, 1, V2P, "512 wide workgroups, pipe"),
        ("auto", 73, 7, 50, 0, V2, "511 wide workgroups, plain q"),
        ("auto", 40, 1, 449, 0, V2S_KS4, "160 workgroups, 8 tiles"), ("auto", 41, 1, 449, 1, V2S_KS2, "164 workgroups, 8 tiles"),
        ("auto", 20, 2, 448, 1, V2S_KS2, "160 workgroups, 7 tiles"), ("auto", 32, 1, 513, 1, V2S_KS4, "160 workgroups, 9 tiles"),
        ("auto", 11, 3, 513, 0, V2S_KS2, "165 workgroups, 9 tiles"), ("auto", 23, 1, 769, 0, V2S_KS2, "161 workgroups, 13 tiles"),
        ("auto", 160, 1, 193, 0, V2S_KS2, "320 workgroups, 4 tiles"), ("auto", 161, 1, 193, 1, V2, "322 workgroups, 4 tiles"),
        ("auto", 80, 2, 192, 0, V2, "320 workgroups, 3 tiles"), ("auto", 106, 1, 257, 1, V2S_KS2, "318 workgroups, 5 tiles"),
        ("auto", 107, 1, 257, 0, V2, "321 workgroups, 5 tiles"),
        ("auto_hp", 40, 1, 449, 0, V2S_HP, "160 workgroups, 8 tiles, bf16x3"), ("auto_hp", 107, 1, 257, 0, V2_HP, "321 workgroups, bf16x3"))
# the 335M model (16 heads, N = 937, batch doubled for guidance, q pre-multiplied, pipe default 0): batch -> kernel, from the rule's
# own comments: one split-KV round at batch 1, the 128-query kernel until 512 wide workgroups exist, then the large-grid kernel
PRODUCTION = {1: V2S_KS2, 2: V2, 3: V2, 4: V2F_PRE, 8: V2F_PRE, 16: V2F_PRE, 32: V2F_PRE}


@dataclass(frozen=True)
class Case:
    op: str
    route: str
    B: int
    H: int
    N: int
    kv: tuple | None
    npad: int
    ldqk: int
    ldo: int
    ldo8: int
    values: str
    qpre: int
    f8: bool = False
    spikes: tuple = ()
    note: str = ""

    @property
    def knobs(self):
        hp, pipe, wide, kvsplit, _ = ROUTES[self.route]
        return hp, pipe, wide, kvsplit

    @property
    def hp(self):
        return ROUTES[self.route][0]

    @property
    def D(self):
        return self.H * 64

    @property
    def kernel(self):
        hp, pipe, wide, kvsplit = self.knobs
        return expected_kernel(self.B, self.H, self.N, hp, self.qpre, pipe, wide, kvsplit)

    @property
    def kernel_name(self):
        return self.kernel + ("+f8" if self.f8 else "")

    @property
    def kvs(self):
        return tuple(self.kv) if self.kv is not None else (self.N,) * self.B

    @property
    def id(self):
        kv = "none" if self.kv is None else "_".join(map(str, self.kv)) if self.B <= 4 else f"all{self.kv[0]}"
        return (f"{self.op}-{self.route}-{self.values}{'-f8' if self.f8 else ''}-B{self.B}-H{self.H}-N{self.N}-kv{kv}-npad{self.npad}-"
                f"q{self.qpre}-ld{self.ldqk}_{self.ldo}")

    @property
    def group(self):
        return (self.op, self.kernel, self.values, self.f8)


def ceil64(n):
    return cdiv(n, 64) * 64


def seq_lengths():
    """Tile counts 1 ... 11 (ring depths 2 and 3 wrap several times; each tail length of v2p's four-tile loop twice; split groups
    that own no tile, exactly one, and unequal counts for 2 and 4 groups) with last-tile fills of 1, 31, 32, 33, 63 and 64 keys: all six
    fills at one to three tiles, two per tile count above.  N mod 128 (mod 256 for the wide kernels) then ends the queries in the first
    wave (fill 1 on an odd tile count), in the last one (fills 33 ... 64 on an even one), in the second query block of a wide wave, and
    leaves waves entirely past the sequence."""
    ns = []
    for t in range(1, 12):
        for i, f in enumerate(FILLS):
            if t <= 3 or (t + i) % 3 == 0:
                ns.append(64 * (t - 1) + f)
    return ns


BH = ((1, 1), (1, 3), (3, 1), (2, 4), (3, 3), (1, 17), (2, 2))     # B H = 1, 3, 3, 8, 9, 17, 4: the turned-away tail of the XCD numbering, two rounds


def spike_shapes(ks):
    """(B, H, N, kv_len, spikes) of the spike class for a kernel that splits the KV range over ks groups (1 = no split).  Every spike is a
    live key of every batch element (position < min kv_len).  The kernels without a tile maximum leave the standing reference point
    only behind a spike in a LATER tile of a group, that is a key >= 64 ks: the first six shapes put one there -- on the last key of a
    partial tile (tiles ks, ks + 1 and 2 ks), in the second and third tile of group 0, in neighbouring tiles, under ragged lengths, and
    with groups that stay at their only tile while group 0's reference point moves.  Then a spike in the first tile (the reference
    point stays far above everything that follows) and the lists of tests/test_ops_gpu.py."""
    a, b2 = 64 * ks, 128 * ks
    return [(1, 2, a + 20, 0, ((a + 19, 400.0),)),                                   # ks + 1 tiles: groups 1 ... stay at their first tile
            (2, 2, a + 97, 1, ((a + 96, 400.0),)),                                   # last key of the partial tile ks + 1
            (1, 3, b2 + 65, 1, ((a + 3, 100.0), (b2 + 5, 200.0))),                   # second and third tile of group 0
            (2, 4, b2 + 31, (b2 + 31, b2 + 30), ((a, 50.0), (a + 65, 90.0), (b2 + 20, 20.0))),
            (1, 1, b2 + 31, 0, ((b2 + 30, 400.0),)),                                 # last key of the partial tile 2 ks
            (3, 2, a + 129, (a + 129, a + 128, a + 65), ((a + 10, 60.0),)),
            (1, 2, b2 + 63, 0, ((3, 100.0),)),
            (1, 2, 300, 0, ((70, 30.0), (200, 60.0))), (1, 2, 400, 1, ((40, 40.0), (100, 80.0), (130, 160.0), (290, 300.0))),
            (1, 2, 700, 0, ((64, 50.0), (65, 90.0), (640, 20.0))), (3, 3, 200, (200, 130, 71), ((70, 30.0),))]


def ragged(N, B, start):
    """kv_len of a launch: lengths from {1, 32, 33, 63, 64, 65, N - 64, N - 1, N} (those that lie in 1 ... N), mixed inside the launch;
    with several batch elements the first one keeps the whole sequence, so that the launch runs the tile count N stands for"""
    pool = sorted({x for x in (1, 32, 33, 63, 64, 65, N - 64, N - 1, N) if 1 <= x <= N})
    if B == 1:
        pool = [x for x in pool if x < N] or [N]
    kv = [pool[(start + 2 * i) % len(pool)] for i in range(B)]
    if B >= 2:
        kv[0] = N
    return tuple(kv)


def make_case(op, route, B, H, N, kvmode, values, idx=0, f8=False, qpre=None, note="", spikes=()):
    """kvmode: 0 = null kv_len, 1 = all N, 2 / 3 = ragged, a tuple = those lengths"""
    want_q = ROUTES[route][4]
    q = want_q if want_q is not None else (idx & 1 if qpre is None else qpre)
    D = H * 64
    kv = kvmode if isinstance(kvmode, tuple) else (None if kvmode == 0 else ((N,) * B if kvmode == 1 else ragged(N, B, idx + kvmode)))
    assert (values == "spikes") == bool(spikes) and all(p < min(kv or (N,)) for p, _ in spikes)
    return Case(op, route, B, H, N, kv, ceil64(N) + 64 * (idx % 2), 2 * D + 8 * (1 + idx % 3), D + 4 * (1 + idx % 3), D + 4 * (1 + (idx + 1) % 3),
                values, q, f8, spikes, note)


def _shapes(values, wide):
    """(B, H, N, kvmode) of a value class (the spike class: spike_shapes)"""
    ns = seq_lengths()
    out = []
    if values == "gauss":
        for i, N in enumerate(ns):
            B, H = BH[i % len(BH)]
            out.append((B, H, N, i % 4))
        for N in (65, 193, 449, 703):                       # every B H at two, four, eight and eleven tiles
            for j, (B, H) in enumerate(BH):
                out.append((B, H, N, 2 + j % 2))
        for t in range(2, 12):                              # every tile count next to batch elements that run fewer tiles in the same launch
            out.append((3, 1 + t % 2, 64 * (t - 1) + FILLS[t % 6], 2))
        if wide:
            out.append((2, 2, 1100, 2))                     # 18 tiles, five 256-query blocks
    else:
        step = {"peaked": 0, "large_v": 2}[values]
        for i, N in enumerate(ns[step::3]):
            B, H = BH[(i + step) % len(BH)]
            out.append((B, H, N, (i + step) % 4))
        out += [(3, 2, 200, 2), (2, 4, 300, 3)]
    return out


def cases():
    """the whole matrix, in a fixed order"""
    out = []
    for op in OPS:
        for route in list(ROUTES)[:8]:
            kernel = expected_kernel(1, 1, 64, ROUTES[route][0], ROUTES[route][4] or 0, *ROUTES[route][1:4])
            for values in VALUES:
                if values == "spikes":
                    for idx, (B, H, N, kvmode, spikes) in enumerate(spike_shapes(SPLIT.get(kernel, 1))):
                        out.append(make_case(op, route, B, H, N, kvmode, values, idx, spikes=spikes))
                    continue
                for idx, (B, H, N, kvmode) in enumerate(_shapes(values, kernel in WIDE_KERNELS)):
                    out.append(make_case(op, route, B, H, N, kvmode, values, idx))
            if kernel in F8_KERNELS:
                for values in ("gauss", "peaked"):
                    for idx, (B, H, N, kvmode) in enumerate(_shapes("large_v", False)):       # the 13-shape list
                        out.append(make_case(op, route, B, H, N, kvmode, values, idx + 1, f8=True))
                out.append(make_case(op, route, 1, 3, 130, 2, "large_v", 2, f8=True))
        for route in FALL_THROUGHS:
            for idx, (B, H, N, kvmode) in enumerate(((1, 2, 130, 0), (3, 2, 577, 2))):
                out.append(make_case(op, route, B, H, N, kvmode, "gauss", idx, note="fall-through"))
        for route, B, H, N, q, _, note in AUTO:
            out.append(make_case(op, route, B, H, N, 0, "gauss", B, qpre=q, note=note))
    return out


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def _round_op(x, op):
    return (x.clamp(-65504.0, 65504.0) if op == "f16" else x).to(op_dtype(op))


def _split(x, op):
    hi = _round_op(x, op)
    return hi, _round_op(x - hi.float(), op)


class Guarded:
    """an [M][N] output inside a [GUARD + M + GUARD][ld] allocation full of a sentinel bit pattern"""

    def __init__(self, M, N, ld, bits, sent, device):
        self.M, self.N, self.ld, self.sent = M, N, ld, sent
        self.alloc = torch.full((2 * GUARD + M, ld), sent, dtype=bits, device=device)
        self.before = self.alloc.clone()

    @property
    def view(self):
        return self.alloc[GUARD:GUARD + self.M, :self.N]

    def ptr_tensor(self):
        return self.alloc[GUARD:]

    def flat(self):
        """the elements from view[0][0] on, as the kernel addresses them"""
        return self.alloc.view(-1)[GUARD * self.ld:]

    def guard_damage(self, interior_too=False):
        diff = self.alloc != self.before
        if not interior_too:
            diff[GUARD:GUARD + self.M, :self.N] = False
        return int(diff.sum())

    def unwritten(self):
        return int((self.view == self.sent).sum())


def make_buffers(c: Case, device="cpu"):
    """operands and guarded outputs of a case; deterministic in the case"""
    gen = torch.Generator(device=device)
    gen.manual_seed(zlib.crc32(c.id.encode()))
    B, H, N, D, op = c.B, c.H, c.N, c.D, c.op
    dt = op_dtype(op)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, device=device, dtype=torch.float32)
    q, k, v = rnd(B, N, H, 64), rnd(B, N, H, 64), rnd(B, N, H, 64)
    q[..., 0] = q[..., 0].abs() + 0.5                 # every query has a positive first component: the masked keys point along it
    if c.values == "peaked":
        q *= 4.0                                      # logits with a standard deviation of 4: a handful of keys carry the weight
    if c.values == "large_v":
        v = (torch.rand(B, N, H, 64, generator=gen, device=device) * 2.0 - 1.0) * LARGE_V
    for pos, factor in c.spikes:
        k[:, pos] *= factor
    f = LN2 if c.qpre else SCALE                       # logit (natural units) = f * (q . k) on the values the kernel is handed
    if c.qpre:
        q = q * (SCALE * LOG2E)
    parts = 2 if c.hp else 1
    qs, ks = (_split(q, op), _split(k, op)) if c.hp else ((_round_op(q, op),), (_round_op(k, op),))
    qj, kj = sum(t.double() for t in qs), sum(t.double() for t in ks)
    kvs = c.kvs
    # the largest legitimate logit of the launch -> masked K rows g e_0 with f * min(q_0) * g >= that + MASK_MARGIN
    smax = 0.0
    for b in range(B):
        s = torch.einsum("nhd,mhd->hnm", qj[b], kj[b, :kvs[b]])
        smax = max(smax, float(s.abs().max()) * f)
    g = min((smax + MASK_MARGIN) / (f * float(qj[..., 0].min())), 6.0e4)
    ks = [t.clone() for t in ks]
    for b in range(B):
        for i, t in enumerate(ks):
            t[b, kvs[b]:] = 0.0
            if i == 0:
                t[b, kvs[b]:, :, 0] = g
    vs = _split(v, op) if c.hp else (_round_op(v, op),)
    rows = B * N
    qk, vt = [], []
    for i in range(parts):
        buf = torch.full((2 * GUARD + rows, c.ldqk), float("nan"), dtype=dt, device=device)
        buf[GUARD:GUARD + rows, :D] = qs[i].reshape(rows, D)
        buf[GUARD:GUARD + rows, D:2 * D] = ks[i].reshape(rows, D)
        qk.append(buf)
        w = torch.full((2 * GUARD + B * H * 64, c.npad), float("nan"), dtype=dt, device=device)
        body = torch.zeros((B, H, 64, c.npad), dtype=dt, device=device)
        body[..., :N] = vs[i].permute(0, 2, 3, 1)
        for b in range(B):
            if kvs[b] < N:
                sign = torch.where(torch.arange(64, device=device) % 2 == 0, 1.0, -1.0)[None, :, None]
                body[b, :, :, kvs[b]:N] = (MASK_V * sign).to(dt) if i == 0 else 0.0
        w[GUARD:GUARD + B * H * 64] = body.reshape(B * H * 64, c.npad)
        vt.append(w)
    i16 = torch.int16
    return {"case": c, "f": f, "mask_excess": f * float(qj[..., 0].min()) * g - smax, "qk": qk, "vt": vt,
            "kv": None if c.kv is None else torch.tensor(c.kv, dtype=torch.int32, device=device),
            "out_hi": Guarded(rows, D, c.ldo, i16, SENT16, device),
            "out_lo": Guarded(rows, D, c.ldo, i16, SENT16, device),
            "out8": Guarded(rows, D, c.ldo8, torch.uint8, SENT8, device),
            "out8s": Guarded(rows, D // 32, D // 32, torch.uint8, SENT8S, device)}


def qk_ptr_tensor(b, i):
    return b["qk"][i][GUARD:]


def vt_ptr_tensor(b, i):
    return b["vt"][i][GUARD:]


def owned_outputs(c: Case):
    return ("out8", "out8s") if c.f8 else (("out_hi", "out_lo") if c.hp else ("out_hi",))


def _operands(b):
    """q, k [B][N][H][64] and v^T [B][H][64][N] in fp64, hi + lo joined: the exact values the kernel was handed"""
    c = b["case"]
    rows, D = c.B * c.N, c.D
    qk = sum(t[GUARD:GUARD + rows, :2 * D].double() for t in b["qk"])
    vt = sum(t[GUARD:GUARD + c.B * c.H * 64].double() for t in b["vt"]).reshape(c.B, c.H, 64, c.npad)
    return qk[:, :D].reshape(c.B, c.N, c.H, 64), qk[:, D:].reshape(c.B, c.N, c.H, 64), vt


# ---- reference and bound -----------------------------------------------------------------------------------------------------------
def reference(b):
    """-> (ref, bound, bound without the output rounding, drift): the first three fp64 [B*N][D] -- softmax(q k^T scale + mask) v from the
    values the kernel was handed, and the element-wise bound of the module docstring; drift = what the terms that need not average out
    (logit error, fp32 accumulation) may contribute to a systematic relative error.  Batch elements of equal kv_len are taken together."""
    c = b["case"]
    q, k, vt = _operands(b)
    u = eps_op(c.op)
    ref = torch.empty((c.B, c.N, c.H, 64), dtype=torch.float64, device=q.device)
    bound, bound0 = torch.empty_like(ref), torch.empty_like(ref)
    drift = 0.0
    for kv in sorted(set(c.kvs)):
        bs = [i for i, x in enumerate(c.kvs) if x == kv]
        qq, kk = q[bs].permute(0, 2, 1, 3), k[bs, :kv].permute(0, 2, 1, 3)          # [b][H][N][64], [b][H][kv][64]
        vv = vt[bs][..., :kv].transpose(-1, -2)                                   # [b][H][kv][64]
        s = (qq @ kk.transpose(-1, -2)) * b["f"]
        sabs = (qq.abs() @ kk.abs().transpose(-1, -2)) * b["f"]
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        L = p.sum(-1, keepdim=True)
        p /= L
        r, A = p @ vv, p @ vv.abs()
        ds = U32 * (64.0 * (sabs + s.abs().amax(-1, keepdim=True)) + 4.0 * s.abs()) + EXP2_ULP * 2.0 ** -23
        if c.hp:
            ds += u * u * sabs
        pd = p * ds
        score = pd @ vv.abs() + pd.sum(-1, keepdim=True) * r.abs()
        floor = (kv + 3 * cdiv(kv, 64) + 16) * U32 * (A + r.abs())
        sub = (2.0 ** -25 * vv.abs().sum(-2, keepdim=True) / L + 2.0 ** -25) if c.op == "f16" else 0.0
        b0 = (2 * u * u if c.hp else u) * A + score + floor + sub
        for t, val in ((ref, r), (bound0, b0), (bound, b0 + (u * u if c.hp else u) * r.abs())):
            t[bs] = val.permute(0, 2, 1, 3)
        # what may push every element the same way: the constant c2 and the roundings of s c2 - m c2 (4 u32 |s|), a bias of the exp2
        # instruction, and the fp32 accumulations of O and l should the matrix core not round to nearest.  The 64 additions of a score
        # are independent roundings of either sign: they are in the element-wise bound at their worst case, not in a mean.
        drift = max(drift, 2.0 * (4.0 * U32 * float(s.abs().max()) + EXP2_ULP * 2.0 ** -23) + 2.0 * (kv + 3 * cdiv(kv, 64) + 16) * U32)
    n = c.B * c.N
    return ref.reshape(n, c.D), bound.reshape(n, c.D), bound0.reshape(n, c.D), drift


def fallback_events(b):
    """number of (query row, KV tile) pairs of the launch whose fp64 scores trip the 2^14 row-sum limit of the kernels without a tile
    maximum in a NON-first tile of a split group (one group when the kernel does not split): the standing reference point is the
    maximum of the group's first tile and moves to a tile's maximum whenever that tile's row sum against it exceeds 2^14.  Tile
    granularity; v2p's reference point is the maximum of the first 32 keys only, so it trips no later."""
    c = b["case"]
    ks = SPLIT.get(c.kernel, 1)
    q, k, _ = _operands(b)
    n = 0
    for bi, kv in enumerate(c.kvs):
        s = torch.einsum("nhd,mhd->hnm", q[bi], k[bi, :kv]) * (b["f"] / LN2)          # exp2 units
        for g in range(ks):
            m = None
            for t in range(g, cdiv(kv, 64), ks):
                st = s[..., t * 64:t * 64 + 64]
                if m is None:
                    m = st.amax(-1)
                    continue
                trip = torch.exp2(st - m[..., None]).sum(-1) > 16384.0
                n += int(trip.sum())
                m = torch.where(trip, torch.maximum(m, st.amax(-1)), m)
    return n


def _scale_byte(amax):
    """f5_mx_scale_byte of a block maximum, through the MX reference (a block that holds the maximum 32 times)"""
    return MX.mx_scale_bytes(amax.to(torch.float32)[..., None].expand(*amax.shape, 32)).to(torch.int32).reshape(amax.shape)


# ---- checker ---------------------------------------------------------------------------------------------------------------------
def check(b, ref3=None):
    """-> list of findings (empty = the launch computed what the reference says, inside the bound, and touched nothing else)"""
    c = b["case"]
    bad = []
    owned = owned_outputs(c)
    for name in ("out_hi", "out_lo", "out8", "out8s"):
        n = b[name].guard_damage(interior_too=name not in owned)
        if n:
            bad.append(f"{name}: {n} element(s) outside what the kernel owns changed")
        if name in owned and b[name].unwritten():
            bad.append(f"{name}: {b[name].unwritten()} interior element(s) still hold the sentinel")
    ref, bound, bound0, drift = ref3 if ref3 is not None else reference(b)
    if not bool(torch.isfinite(ref).all() and torch.isfinite(bound).all()):
        bad.append("reference or bound not finite")
    dt = op_dtype(c.op)

    def cmp(name, got, tol):
        if not bool(torch.isfinite(got).all()):
            bad.append(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite element(s)")
        d = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
        ok = d <= tol
        b["worst"] = float((d / tol).max())                 # reported by the GPU test: how much of the bound the kernel used
        if not bool(ok.all()):
            i = int((~ok).reshape(-1).nonzero()[0])
            bad.append(f"{name}: {int((~ok).sum())} element(s) off, first at {divmod(i, c.D)}: got {float(got.reshape(-1)[i])!r} ref "
                       f"{float(ref.reshape(-1)[i])!r} tol {float(tol.reshape(-1)[i]):.3e}; max err / tol {float((d / tol).max()):.3f}")

    if c.f8:
        e8 = b["out8s"].view.to(torch.int32)                                   # [rows][D / 32]
        S = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), (e8 - 127).double()).repeat_interleave(32, dim=1)
        got = b["out8"].view.contiguous().view(torch.float8_e4m3fn).float().double() * S
        cmp("out8 * 2^(out8s - 127)", got, bound0 + torch.maximum(2.0 ** -4 * (ref.abs() + bound0), 2.0 ** -10 * S))
        blk = lambda t: t.reshape(t.shape[0], c.D // 32, 32).amax(-1)          # noqa: E731
        lo, hi = _scale_byte(blk((ref.abs() - bound0).clamp(min=0.0))), _scale_byte(blk(ref.abs() + bound0))
        off = (e8 < lo) | (e8 > hi)
        if bool(off.any()):
            i = int(off.reshape(-1).nonzero()[0])
            bad.append(f"out8s: {int(off.sum())} scale byte(s) outside [{int(lo.reshape(-1)[i])}, {int(hi.reshape(-1)[i])}], first "
                       f"{int(e8.reshape(-1)[i])} at {divmod(i, c.D // 32)}")
    else:
        got = b["out_hi"].view.contiguous().view(dt).double()
        if c.hp:
            got = got + b["out_lo"].view.contiguous().view(dt).double()
        cmp("out_hi + out_lo" if c.hp else "out_hi", got, bound)
        # Systematic error (one-pass kernels).  Round-to-nearest errors of P and of the output have no preferred sign: over n elements
        # the slope of (got - ref) against ref is their mean, at most u / sqrt(3 n) in standard deviation (under 0.01 u from 4096 elements
        # on), plus what does not average out (drift).  A P that is truncated, or rounded a second time toward zero, loses u of every
        # inexact weight on average and tilts the whole output by about -u: u / 4 separates the two.
        if not c.hp and ref.numel() >= 4096:
            slope = float(((got - ref) * ref).sum() / (ref * ref).sum())
            b["slope"] = abs(slope) / (eps_op(c.op) / 4 + drift)
            if not abs(slope) <= eps_op(c.op) / 4 + drift:
                bad.append(f"out_hi: systematic relative error {slope:.3e}, allowed {eps_op(c.op) / 4 + drift:.3e}")
    return bad


# ---- torch emulation of the kernels (CPU): the checker's own test ---------------------------------------------------------------
FAULTS = ("mask_plus1", "mask_minus1", "mask_seq_len", "mask_npad", "mask_other_batch", "dropped_tile", "tail_key_counted",
          "rescale_skipped", "tile_weight", "p_truncated", "p_via_bf16", "rowsum_base", "v_swap", "head_q", "head_k", "head_out",
          "ldo_dmodel", "ldqk_dmodel", "split_partial_dropped", "split_no_rescale", "p_lo_dropped", "q_lo_dropped", "row_past_seq",
          "pad_col_written", "untouched", "f8_scale_plus1", "f8_amax_one_lane")


def fault_applies(fault, c: Case):
    """does the mistake change the arithmetic (or a store) of this case at all?"""
    kvs, nt = c.kvs, [cdiv(x, 64) for x in c.kvs]
    split = SPLIT.get(c.kernel, 1)
    small = c.values == "peaked" or (c.values == "gauss" and c.N <= 130)          # a single key's share of the weight beats the bound
    many = max(kvs) >= 8                                                          # (one key alone has weight 1 whatever the arithmetic)
    late_spike = any(64 * split <= p < max(kvs) for p, _ in c.spikes)
    return {"mask_plus1": any(x % 64 for x in kvs), "mask_seq_len": any(x < c.N for x in kvs), "mask_npad": any(x < ceil64(x) for x in kvs),
            "mask_other_batch": any(min(kvs[(i + 1) % c.B], 64 * nt[i]) != kvs[i] for i in range(c.B)),
            "dropped_tile": max(nt) >= 2 and c.values in ("gauss", "large_v"), "tail_key_counted": any(x == c.N and x % 64 for x in kvs) and small,
            # the kernels with a tile maximum rescale whenever the maximum moves; the others only behind a score 2^14 above the reference point
            "rescale_skipped": max(nt) >= 2 * split and (c.values in ("peaked", "spikes") if c.kernel not in NO_TILE_MAX else late_spike),
            "tile_weight": max(nt) >= 2 and (c.values == "peaked" or (c.values == "gauss" and (c.op == "f16" or bool(c.hp)))),
            # a truncation tilts the output by about -u where most weights are inexact: not where one key has nearly all of it (p = 1 is exact)
            "p_truncated": not c.hp and not c.f8 and c.B * c.N * c.D >= 4096 and c.values in ("gauss", "large_v") and min(kvs) >= 8,
            "p_via_bf16": c.op == "f16" and not c.hp and not c.f8 and c.values in ("gauss", "peaked") and many,
            "rowsum_base": many, "v_swap": min(kvs) >= 2 and small, "head_q": c.H >= 2, "head_k": c.H >= 2, "head_out": c.H >= 2,
            "ldo_dmodel": c.B * c.N >= 2, "ldqk_dmodel": c.B * c.N >= 2,
            "split_partial_dropped": split > 1 and max(nt) >= 2 and c.values in ("gauss", "large_v"),
            "split_no_rescale": split > 1 and max(nt) >= 2 and c.values in ("peaked", "spikes"),
            "p_lo_dropped": bool(c.hp) and c.values in ("gauss", "peaked") and many,
            "q_lo_dropped": bool(c.hp) and c.values in ("gauss", "peaked") and many,
            "f8_scale_plus1": c.f8, "f8_amax_one_lane": c.f8}.get(fault, True)


def _truncate(x, op):
    """fp32 -> operand type by dropping the low bits (round toward zero)"""
    if op == "bf16":
        return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    r = x.to(torch.float16)
    over = r.float().abs() > x.abs()
    bits = r.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16)


def _mm32(a, bmat):
    """an MFMA chain: exact products, fp32 accumulator (emulated as one rounding of the fp64 sum)"""
    return (a.double() @ bmat.double()).float()


def emulate(b, fault=None):
    """Write the outputs as the kernel of the case would: 64-key tiles read from the buffers the kernel reads (tail rows clamped to
    seq_len - 1), fp32 scores, the running maximum or the standing reference point with its 2^14 fallback, P rounded to the operand
    type for P V, the row sum from the unrounded P, the split groups merged flash-decoding style, one rounding of the output (a hi + lo
    pair for bf16x3, MX-fp8 blocks for the fp8 output).  `fault` = one of FAULTS makes it subtly wrong."""
    c = b["case"]
    B, H, N, D, op = c.B, c.H, c.N, c.D, c.op
    dt = op_dtype(op)
    kern, KS = c.kernel, SPLIT.get(c.kernel, 1)
    c2 = 1.0 if c.qpre else float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    parts = 2 if c.hp else 1
    ldqk = 2 * D if fault == "ldqk_dmodel" else c.ldqk
    qkf = [t.view(-1)[GUARD * c.ldqk:] for t in b["qk"]]
    hs = torch.arange(H)

    def rows_of(i, r0, nrows, col0, hsel):
        """[H][nrows][64] of part i: rows r0 ..., head columns col0 + 64 hsel"""
        idx = (r0 + torch.arange(nrows))[None, :, None] * ldqk + col0 + (hsel * 64)[:, None, None] + torch.arange(64)[None, None, :]
        return qkf[i][idx].float()

    results = []
    for bi in range(B):
        kv = c.kvs[bi]
        thr = {"mask_plus1": kv + 1, "mask_minus1": kv - 1, "mask_seq_len": N, "mask_npad": c.npad, "mask_other_batch": c.kvs[(bi + 1) % B],
               "tail_key_counted": ceil64(kv) if kv == N else kv}.get(fault, kv)
        ntile = cdiv(kv, 64)
        hq = (hs + 1) % H if fault == "head_q" else hs
        hk = (hs + 1) % H if fault == "head_k" else hs
        qp = [rows_of(i, bi * N, N, 0, hq) for i in range(parts)]
        if fault == "q_lo_dropped":
            qp[1] = torch.zeros_like(qp[1])
        keys = torch.arange(ntile * 64).clamp(max=N - 1)
        kp = [qkf[i][((bi * N + keys)[None, :, None] * ldqk + D + (hk * 64)[:, None, None] + torch.arange(64)[None, None, :])].float()
              for i in range(parts)]
        vp = [t[GUARD + bi * H * 64:GUARD + (bi + 1) * H * 64].reshape(H, 64, c.npad).float() for t in b["vt"]]
        if fault == "v_swap":
            vp = [t.clone() for t in vp]
            for t in vp:
                t[..., [0, 1]] = t[..., [1, 0]]
        state = []
        for g in range(KS):
            m = torch.full((H, N, 1), float("-inf"))
            l = torch.zeros((H, N, 1))
            o = torch.zeros((H, N, 64))
            first = True
            for t in range(g, ntile, KS):
                if fault == "dropped_tile" and ntile >= 2 and t == (ntile - 1) // 2:
                    continue
                sl = slice(t * 64, t * 64 + 64)
                kt = [x[:, sl].transpose(-1, -2) for x in kp]
                s = qp[0].double() @ kt[0].double()
                if c.hp:
                    s = s + qp[0].double() @ kt[1].double() + qp[1].double() @ kt[0].double()
                s = s.float()
                s = s.masked_fill((torch.arange(t * 64, t * 64 + 64) >= thr)[None, None, :], float("-inf"))
                tmax = s.amax(-1, keepdim=True)
                if kern in NO_TILE_MAX and not first:
                    psum = torch.exp2(s * c2 - m * c2).sum(-1, keepdim=True)
                    m_new = torch.where(psum <= 16384.0, m, torch.maximum(m, tmax))      # (NaN compares false: the exact path)
                else:
                    m_new = torch.maximum(m, tmax)
                alpha = torch.exp2((m - m_new) * c2)
                alpha = torch.where(m_new == float("-inf"), torch.ones_like(alpha), alpha)
                if not (fault == "rescale_skipped" and not first):
                    l, o = l * alpha, o * alpha
                m = m_new
                targ = s * c2 - m * c2
                p = torch.exp2(targ)
                if fault == "tile_weight" and t == 0:
                    p = p * (1.0 + 2.0 ** -5)
                l = l + (torch.exp(targ) if fault == "rowsum_base" else p).sum(-1, keepdim=True)
                if fault == "p_truncated":
                    ph = _truncate(p, op)
                elif fault == "p_via_bf16":
                    ph = p.to(torch.bfloat16).float().to(torch.float16)
                else:
                    ph = p.to(dt)
                vt_t = [x[..., sl].transpose(-1, -2) for x in vp]
                acc = ph.double() @ vt_t[0].double()
                if c.hp:
                    pl = torch.zeros_like(ph) if fault == "p_lo_dropped" else (p - ph.float()).to(dt)
                    acc = acc + ph.double() @ vt_t[1].double() + pl.double() @ vt_t[0].double()
                o = (o.double() + acc).float()
                first = False
            state.append((m, l, o))
        m, l, o = state[0]
        if KS > 1:
            if fault == "split_partial_dropped":
                state = [state[0]] + state[2:]
            m_all = torch.stack([x[0] for x in state]).amax(0)
            l, o = torch.zeros_like(l), torch.zeros_like(o)
            for mg, lg, og in state:
                ag = torch.ones_like(mg) if fault == "split_no_rescale" else torch.nan_to_num(torch.exp2((mg - m_all) * c2), nan=0.0)
                l, o = l + lg * ag, o + og * ag
        results.append((o * (1.0 / l)).permute(1, 0, 2))         # [N][H][64]
    val = torch.stack(results)                                   # [B][N][H][64]
    if fault == "head_out":
        val = val[:, :, (hs + 1) % H]
    val = val.reshape(B * N, D)
    ldo = D if fault == "ldo_dmodel" else None
    nrow = B * N

    def store(g, x):
        ld = ldo if ldo is not None and g.N == D else g.ld
        idx = torch.arange(nrow)[:, None] * ld + torch.arange(g.N)[None, :]
        if fault == "untouched":
            idx = idx[:-1]
            x = x[:-1]
        g.flat()[idx] = x
        if fault == "row_past_seq":
            g.flat()[nrow * g.ld:nrow * g.ld + g.N] = x[-1]
        if fault == "pad_col_written":
            g.flat()[torch.arange(nrow) * g.ld + g.N] = x[:, -1]

    if c.f8:
        xb = val.reshape(nrow, D // 32, 32)
        if fault == "f8_amax_one_lane":
            half = (torch.arange(32) % 8 < 4)
            e0, e1 = _scale_byte(xb[..., half].abs().amax(-1)), _scale_byte(xb[..., ~half].abs().amax(-1))
            e_el = torch.where(half[None, None, :], e0[..., None], e1[..., None])
            e8 = e0
        else:
            e8 = _scale_byte(xb.abs().amax(-1)) + (1 if fault == "f8_scale_plus1" else 0)
            e_el = e8[..., None].expand(-1, -1, 32)
        inv = torch.pow(torch.tensor(2.0, dtype=torch.float64), (127 - e_el).double()).float()
        q8 = (xb * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).reshape(nrow, D)
        store(b["out8"], q8)
        store(b["out8s"], e8.to(torch.uint8))
    else:
        hi = _round_op(val, op)
        store(b["out_hi"], hi.view(torch.int16))
        if c.hp:
            store(b["out_lo"], _round_op(val - hi.float(), op).view(torch.int16))
