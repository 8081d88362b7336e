"""The conv-pos / audio / noise kernel test matrix (csrc/convpos.hip, csrc/audio.hip mel front-end and ISTFT head, csrc/noise.hip): case
generators, guarded buffers, fp64 references, checkers.  The layout is that of tests/rowops_matrix.py, whose Case / Out / pad_in /
build / check / host_backend and shared checkers do the work here too (the table of ops is swapped in for the call).

Shared by tests/test_convaudio_matrix_gpu.py (runs the cases through the C ABI) and tests/test_convaudio_matrix_host.py (runs the
checkers over an emulation of the kernels, right and deliberately wrong, on the CPU).  Nothing here needs a GPU or the library.

Ops: convpos (16-bit operands: both operand types), mel, istft, noise, noise_bits (fp32 only: one operand type is enough).

Tolerances.  u = 2^-24.  Every bound is counted from the kernel's expression, next to its checker.  The library functions are allowed
four times the largest error measured on an MI355X against fp64 (tools/probes/math_ulp.hip: 2^21 samples per function over the
arguments these kernels produce, the twiddle grid exactly).  "abs" figures are absolute errors in units of u, what a sine or cosine
near one of its zeros is judged by:
    function                                          measured          granted
    sincosf, twiddle grid +-6.2831853f i / 1024       0.883 u abs       3.532 u abs     (1.121 ULP)
    sincosf, phases in +-100                          1.155 u abs       4.620 u abs     (1.532 ULP)
    logf on [1e-5, 1e14]                              2.319 ULP         9.276 ULP       (2.296 on [1e-5, 1e6])
    __builtin_amdgcn_rcpf on [2, 1e30]                0.882 ULP         3.528 ULP
    expf (tests/rowops_matrix.py)                     0.845 ULP         3.380 ULP
    __builtin_amdgcn_exp2f (tests/attention_matrix.py) 0.769 ULP        3.076 ULP
One ULP is at most 2 u relative.
"""
from __future__ import annotations

import contextlib
import math
import os
import sys
import zlib

import numpy as np
import torch

import rowops_matrix as RM
from rowops_matrix import (GUARD, OPS16, OUTLIER, SAT, SENT32, U, Case, Out, bits, cdiv, chk_exact, chk_f32, chk_pair,  # noqa: F401
                           eps_op, floor_op, op_dtype, pad_in, split, to_op)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TW_ABS, PH_ABS = 4 * 0.883, 4 * 1.155                 # sincosf, absolute, in units of u
ULP_LOG, ULP_RCP, ULP_EXP, ULP_EXP2 = 4 * 2.319, 4 * 0.882, 4 * 0.845, 4 * 0.769
NFFT, NBIN = 1024, 513
LOG_FLOOR = float(np.float32(1e-5))                   # the kernel's 1e-5f

# pooled figures of the ops whose rule is a share over all their values (noise, noise_bits): op -> [bit-equal, total]
POOL = {}
# worst observed |err| / bound of the latest check of each case (printed by the tests)
WORST = {}


class DCase(Case):
    """a case whose DATA depend on some of its keywords only (`data`): cases that differ in a selector alone get the same inputs, so
    that their outputs can be compared bit for bit and the fp64 reference is computed once"""

    def __init__(self, op, data, **kw):
        super().__init__(op, **kw)
        self.__dict__["data"] = tuple(data)

    @property
    def datakey(self):
        return self.op + "[" + ",".join(f"{k}={self.kw[k]}" for k in self.data) + "]"

    def seed(self, op16):
        return zlib.crc32((self.datakey + op16).encode())


def _randn(r, *shape, scale=1.0):
    return torch.from_numpy((r.standard_normal(shape) * scale).astype(np.float32))


def _hann(n=NFFT, periodic=True):
    k = torch.arange(n, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * k / (n if periodic else n - 1))).float()


# ================================================================================================================================
# conv-pos: grouped Conv1d(C, C, taps, groups = C / 64, pad = taps / 2) + Mish on channels-last input
# ================================================================================================================================
CP_C = (64, 128, 512, 1024)
CP_N = (1, 2, 15, 16, 31, 127, 128, 129, 257)
CP_TAPS = (1, 3, 5, 29, 31)
CP_DATA = ("C", "N", "B", "taps", "var")
CP_OUTS = ((0, 1), (0, 0), (1, 0))                    # (mode, lo)
MISH_PUSH = (10.0, -10.0, 30.0, 31.0, 100.0, -100.0)  # bias of channel co: MISH_PUSH[co % 6]


def _cp(C, N, B, taps, nseg, tps, xcd, mode, lo, var="normal"):
    kw = dict(C=C, N=N, B=B, taps=taps, var=var, nseg=nseg, tps=tps, xcd=xcd, mode=mode, lo=lo)
    if var == "outlier":
        kw["outlier"] = 1
    return DCase("convpos", CP_DATA, **kw)


def cases_convpos():
    cs = []
    combos = [(nseg, tps, xcd, out) for out in CP_OUTS for xcd in (1, 0) for tps in (0, 1, 2, 4) for nseg in (1, 3)]
    i = 0
    # every channel count x token count at batch 1, three selector combinations each (the 48 combinations go round)
    for C in CP_C:
        for N in CP_N:
            for _ in range(3):
                nseg, tps, xcd, (mode, lo) = combos[i % len(combos)]
                i += 7                                # 7 and 48 are coprime: every combination comes up
                cs.append(_cp(C, N, 1, 31, nseg, tps, xcd, mode, lo))
    # B > 1 under both numberings, every tps: the groups whose members must agree bit for bit
    for k, (C, N, B, taps) in enumerate(((512, 1, 3, 1), (512, 129, 2, 31), (1024, 16, 2, 5), (1024, 257, 3, 31))):
        for nseg in (1, 3):
            for (mode, lo) in (CP_OUTS if k == 0 else (CP_OUTS[(k + nseg) % 3],)):
                for tps in (0, 1, 2, 4):
                    for xcd in (0, 1):
                        cs.append(_cp(C, N, B, taps, nseg, tps, xcd, mode, lo))
    # tap counts: with 2 or 4 taps per step the last step of 1, 3, 5, 29 (and 31) taps is partial
    for taps in (1, 3, 5, 29):
        for nseg in (1, 3):
            for tps in (1, 2, 4):
                cs.append(_cp(128, 31, 2, taps, nseg, tps, 1, 0, 1))
                cs.append(_cp(512, 130, 1, taps, nseg, tps, tps & 1, 1, 0))
    # a batch element between neighbours 1e3 times larger: rows shorter than the halo (zero padding on both sides at once) and longer
    for C in (128, 512, 1024):
        for N in (2, 16, 129):
            for nseg in (1, 3):
                cs.append(_cp(C, N, 3, 31, nseg, (1, 2, 4)[(N + nseg) % 3], (C // 128 + N) & 1, int(nseg == 3), int(nseg == 1), "neighbours"))
    # pre-activations pushed to +-10, 30, 31, +-100: the clamp of f5_mish
    for nseg, tps, (mode, lo) in ((1, 1, (0, 1)), (1, 4, (1, 0)), (3, 2, (0, 1)), (3, 1, (1, 0)), (1, 2, (0, 0))):
        cs.append(_cp(64, 31, 1, 3, nseg, tps, 1, mode, lo, "mish"))
        cs.append(_cp(512, 129, 2, 31, nseg, tps, 1, mode, lo, "mish"))
    # an outlier weight row: beyond the fp16 range the hi half is +-65504 exactly, the lo half finite, and the flag is raised
    for nseg, tps, lo in ((1, 0, 1), (1, 2, 0), (3, 1, 1), (3, 4, 0), (1, 4, 1)):
        cs.append(_cp(128, 129, 1, 31, nseg, tps, 1, 0, lo, "outlier"))
    return cs


def convpos_kernel_name(c):
    """what f5_debug_last_convpos_kernel must report for a case (csrc/convpos.hip f5_launch_convpos)"""
    t = c.tps or 1
    name = f"f5_convpos_kernel<true,{min(t, 2)}>" if c.nseg == 3 else f"f5_convpos_kernel<false,{t}>"
    return name + ("+xcd" if (c.C // 64) % 8 == 0 and c.xcd else "")


CP_NAMES = tuple(f"f5_convpos_kernel<{hp},{t}>{x}" for hp, t in (("false", 1), ("false", 2), ("false", 4), ("true", 1), ("true", 2))
                 for x in ("", "+xcd"))


def convpos_group(c):
    """cases that must give the same bits: same data, nseg and outputs; the block numbering and the taps per step do not change the
    order in which an element is accumulated (taps ascending, 4 K steps of 16 per tap, hi x hi, lo x hi, hi x lo)"""
    return (c.datakey, c.nseg, c.mode, c.lo)


def gen_convpos(c, op16, r):
    x = _randn(r, c.B, c.N, c.C)
    w = _randn(r, c.C, c.taps, 64, scale=(c.taps * 64) ** -0.5)             # [co][tap][ci]: the kernel's layout
    bias = _randn(r, c.C, scale=0.1)
    old = _randn(r, c.B * c.N, c.C)
    if c.var == "neighbours":
        x[0] *= 1.0e3
        x[2] *= 1.0e3
    elif c.var == "mish":
        bias = bias + torch.tensor(MISH_PUSH, dtype=torch.float32)[torch.arange(c.C) % 6]
    elif c.var == "outlier":
        w[33] *= OUTLIER
    x_hi, x_lo = split(x.reshape(c.B * c.N, c.C), op16)
    w_hi, w_lo = split(w.reshape(c.C, c.taps * 64), op16)
    ins = dict(x=x, w=w, bias=bias, old=old, x_hi=x_hi, x_lo=x_lo, w_hi=w_hi, w_lo=w_lo)
    g = 128 * c.C                                                           # a whole tile of rows behind the last one
    s16 = dict(shape=(c.B * c.N, c.C), dtype=op_dtype(op16), guard=g)
    if c.mode == 0:
        return ins, dict(hi=dict(s16), lo=dict(s16) if c.lo else None, out=None)
    return ins, dict(hi=None, lo=None, out=dict(shape=(c.B * c.N, c.C), dtype=torch.float32, guard=g, init=old))


def _conv(x, w, B, N, C, taps, across_batch=False, shift=0, tap_weight=None):
    """out[b][n][co] = sum_{tap, ci} x[b][n + tap - pad - shift][group(co) * 64 + ci] * w[co][tap][ci], zero outside [0, N), in the
    precision of x and w: one matrix product per group over the unfolded windows"""
    pad = taps // 2
    x = x.reshape(B, N, C)
    if across_batch:
        x, B, N = x.reshape(1, B * N, C), 1, B * N
    xp = torch.zeros((B, N + taps - 1 + 2, C), dtype=x.dtype)
    xp[:, pad + shift:pad + shift + N] = x
    win = xp.unfold(1, taps, 1)[:, :N]                                      # [B][N][C][taps]
    w = w.reshape(C, taps, 64)
    if tap_weight is not None:
        w = w * tap_weight.to(w.dtype).reshape(1, taps, 1)
    out = torch.empty((B * N, C), dtype=x.dtype)
    for g in range(C // 64):
        a = win[:, :, g * 64:(g + 1) * 64].permute(0, 1, 3, 2).reshape(B * N, taps * 64)
        out[:, g * 64:(g + 1) * 64] = a @ w[g * 64:(g + 1) * 64].reshape(64, taps * 64).T
    return out


def _mish(y):
    return y * torch.tanh(torch.nn.functional.softplus(y))


def _mish32(x, clamp=True):
    """common.hpp f5_mish in fp32: x n / (n + 2), n = w (w + 2), w = exp(min(x, 30))"""
    w = torch.exp(x.clamp(max=30.0) if clamp else x)
    n = w * (w + 2.0)
    return x * n / (n + 2.0)


def _tps_eff(c):
    t = c.tps or 1
    return min(t, 2) if c.nseg == 3 else t


def emu_convpos(c, op16, ins, bug):
    B, N, C, taps = c.B, c.N, c.C, c.taps
    if c.nseg == 3 and bug != "lo_terms_dropped":
        x, w = ins["x"], ins["w"]                           # hi + lo carries fp32 operands up to the dropped lo x lo term
    else:
        x, w = ins["x_hi"].float(), ins["w_hi"].float()
    partial = taps % _tps_eff(c) != 0                       # the last pipeline step holds fewer taps than slabs
    tw = None
    if partial and bug in ("last_tap_dropped", "clamped_slab_used"):
        tw = torch.ones(taps)
        tw[taps - 1] = 0.0 if bug == "last_tap_dropped" else 2.0
    acc = _conv(x, w, B, N, C, taps, across_batch=(bug == "conv_across_batch"), shift=int(bug == "pad_off_by_one"), tap_weight=tw)
    bias = ins["bias"]
    if bug == "bias_of_group_0":
        bias = bias[:64].repeat(C // 64)
    v = _mish32(acc + bias, clamp=(bug != "mish_unclamped"))
    unwritten = torch.zeros(B * N, dtype=torch.bool)
    if bug == "group_of_wrong_xcd" and (C // 64) % 8 == 0 and c.xcd and B > 1:
        # the 1-D decode with nx in place of nx * B: every block takes itself for one of batch element 0 (of a group that may not
        # exist), the rows of the other batch elements are never written
        unwritten[N:] = True
    if bug == "one_group_as_1d" and C == 64 and B == 1:
        # a (token tiles, 1, 1) grid taken for the 1-D numbering: block i computes group i of token tile 0, the other tiles are never
        # written (what csrc/convpos.hip did at C = 64, B = 1, N > 128 until this matrix ran)
        unwritten[128:] = True
    if c.mode == 1:
        out = v if bug == "mode1_overwrites" else ins["old"] + v
        out[unwritten] = ins["old"][unwritten]
        return dict(out=out, flag=0)
    hi, lo = RM._emu_pack(v, op16, bug)
    hi, lo = hi.clone(), lo.clone()
    bits(hi)[unwritten] = RM.SENT16
    bits(lo)[unwritten] = RM.SENT16
    return dict(hi=hi, lo=lo, flag=RM._flag_of(v, op16))


_CP_REF = {}


def _convpos_ref(c, op16, ins):
    """fp64 conv + bias and Mish of it: from the operands rounded to the operand type (nseg 1) or from the fp32 inputs (nseg 3), as
    tests/gemm_matrix.py reference().  Computed once per (data, operand type, nseg)."""
    key = (c.datakey, op16, c.nseg)
    if key not in _CP_REF:
        if len(_CP_REF) >= 6:
            _CP_REF.clear()
        if c.nseg == 3:
            x, w = ins["x"].double(), ins["w"].double()
        else:
            x, w = ins["x_hi"].double(), ins["w_hi"].double()
        pre = _conv(x, w, c.B, c.N, c.C, c.taps) + ins["bias"].double()
        _CP_REF[key] = (pre, _mish(pre))
    return _CP_REF[key]


def chk_convpos(c, op16, ins, got):
    """The op is a K = 64 taps GEMM with fp32 accumulation behind an activation whose slope is at most 1.09, so the bounds are those of
    tests/gemm_matrix.py tol_f32 / tol_16, not new numbers -- with one difference that only tightens them: the output scale
    max(1, max |ref|) is taken per batch element (each is a GEMM of its own; a neighbour 1e3 times larger must not buy room), and the
    channel of the outlier weight row answers for itself.
        mode 1 (out += v):       2e-4 (nseg 1) / 5e-5 (nseg 3) of the scale, on out - out_before, plus u |out| for the rounding of the sum
        mode 0, nseg 1:          |hi - ref| <= eps_op |ref| + floor, floor = the mode 1 bound (chk_pair)
        mode 0, nseg 3:          1e-4 of the scale (chk_pair's B)
    plus the Mish term: with p the pre-activation, w = exp2(1.4427 min(p, 30)) carries 2 |p| u from the two roundings of its argument
    and the granted exp2 figure; n = w (w + 2) doubles that and adds 2 u; n / (n + 2) is no more sensitive than n; then the granted rcp
    figure, one addition and two products: (4 |p| + 4 ULP_EXP2 + 2 ULP_RCP + 7) u |ref|, |p| taken at most 30 where p > 0.  Dropping
    the factor beyond the clamp costs 2 / (n + 2) < 1e-25.  It matters only where the bounds above are smaller than it."""
    pre, ref = _convpos_ref(c, op16, ins)
    a = ref.abs().reshape(c.B, c.N, c.C)
    other = torch.ones(c.C, dtype=torch.bool)
    if c.var == "outlier":
        other[33] = False
    scale = torch.ones_like(a)
    scale[:, :, other] = a[:, :, other].amax(dim=(1, 2), keepdim=True).clamp_min(1.0).expand(-1, c.N, int(other.sum()))
    if c.var == "outlier":
        scale[:, :, 33] = a[:, :, 33].amax(dim=1, keepdim=True).clamp_min(1.0)
    scale = scale.reshape(c.B * c.N, c.C)
    pm = torch.where(pre > 0, pre.clamp(max=30.0), pre.abs())
    mish = (4 * pm + 4 * ULP_EXP2 + 2 * ULP_RCP + 7) * U * ref.abs() + 1e-25 * ref.abs()
    bad = []
    if c.mode == 1:
        out = got["out"]
        tol = (2e-4 if c.nseg == 1 else 5e-5) * scale + mish + U * out.double().abs().nan_to_num(0.0)
        bad += chk_f32("out - out_before", out.double() - ins["old"].double(), ref, tol)
        _worst(c, op16, out.double() - ins["old"].double(), ref, tol)
        return bad
    B_ = (2e-4 if c.nseg == 1 else 1e-4) * scale + mish
    bad += chk_pair("out", got["hi"], got["lo"], ref, B_, op16)
    _worst(c, op16, got["hi"].double() + (got["lo"].double() if (got["lo"] is not None and c.nseg == 3) else 0.0), ref,
           B_ + (eps_op(op16) * ref.abs() if c.nseg == 1 or got["lo"] is None else 0.0) + floor_op(op16), finite_only=True)
    return bad


def _worst(c, op16, got, ref, bound, finite_only=False):
    r = ((got.double() - ref.double()).abs() / torch.as_tensor(bound, dtype=torch.float64).clamp_min(1e-300))
    if finite_only:
        r = r[torch.isfinite(r) & (ref.double().abs() < SAT)]
    WORST[(c.id, op16)] = float(r.nan_to_num(float("inf")).max()) if r.numel() else 0.0


# ================================================================================================================================
# the 1024-point radix-2 FFT of csrc/audio.hip, shared by the mel and ISTFT bounds
# ================================================================================================================================
# Higham, Accuracy and Stability of Numerical Algorithms, theorem 24.2 (radix 2, n = 2^t): ||dX||_2 <= (t eta / (1 - t eta)) ||X||_2,
# eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4 u / (1 - 4 u), mu = the absolute error of the twiddle factors.  The kernels take
# cos and sin of the fp32 angle 6.2831853f * i / 1024: the granted sincosf figure on exactly that grid, plus two roundings of an angle
# below pi (the constant 6.2831853f against 2 pi, and the product with i; the division by 1024 is exact): mu = (TW_ABS + 2 pi) u.
_MU = (TW_ABS + 2 * math.pi) * U
_G4 = 4 * U / (1 - 4 * U)
_ETA = _MU + _G4 * (math.sqrt(2.0) + _MU)
FFT_REL = 10 * _ETA / (1 - 10 * _ETA)


# ================================================================================================================================
# mel front-end
# ================================================================================================================================
MEL_SIGS = ("silence", "dc", "impulse0", "impulse_last", "tone", "noise1e-6", "noise0.1", "noise1e4")


def mel_lengths(hop):
    return (hop - 1, hop, 3 * hop + 17, 1024 + 1)


def cases_mel():
    cs = []
    i = 0
    for hop in (256, 100):
        for L in mel_lengths(hop):
            for n_mels in (1, 100, 257):
                for B in (1, 3):
                    # two signals per shape, going round; the shapes without a frame need one only
                    for _ in range(1 if L < hop else 2):
                        cs.append(Case("mel", L=L, hop=hop, n_mels=n_mels, B=B, sig=MEL_SIGS[i % len(MEL_SIGS)]))
                        i += 3
    for sig in MEL_SIGS:                                  # every signal at the production table size
        cs.append(Case("mel", L=5 * 256 + 3, hop=256, n_mels=100, B=3, sig=sig))
    return cs


def mel_filterbank(n_mels):
    """the tests' own table: n_mels triangles with centres spread evenly over the 513 bins, at least two bins wide on either side"""
    k = torch.arange(NBIN, dtype=torch.float64)
    ctr = (torch.arange(n_mels, dtype=torch.float64) + 1) * (NBIN - 1) / (n_mels + 1)
    half = max(2.0, 2.0 * (NBIN - 1) / (n_mels + 1))
    return (1.0 - (k[None, :] - ctr[:, None]).abs() / half).clamp_min(0.0).float()


def gen_mel(c, op16, r):
    L, B = c.L, c.B
    t = torch.arange(L, dtype=torch.float64)
    if c.sig == "silence":
        w = torch.zeros(B, L)
    elif c.sig == "dc":
        w = torch.full((B, L), 0.25)
    elif c.sig == "impulse0":
        w = torch.zeros(B, L)
        w[:, 0] = 1.0
    elif c.sig == "impulse_last":
        w = torch.zeros(B, L)
        w[:, L - 1] = 1.0
    elif c.sig == "tone":
        w = (0.5 * torch.sin(2 * math.pi * 37 * t / NFFT)).float().repeat(B, 1)           # the centre of bin 37
    else:
        w = _randn(r, B, L, scale=float(c.sig[5:]))
    w = w * (1.0e3 ** torch.arange(B, dtype=torch.float32)).reshape(B, 1)                 # rows of the batch differ in scale by 1e3
    frames = L // c.hop
    # no frame: no launch, and one row of n_mels per batch element to show that nothing was written
    spec = dict(out=dict(shape=(B, max(frames, 1), c.n_mels), dtype=torch.float32, guard=2 * c.n_mels))
    return dict(wave=w, window=_hann(), fb=mel_filterbank(c.n_mels)), spec


def _mel_frames(wave, window, hop, nframes, centre=True, stride=None):
    """[B][nframes][1024] fp64: zero-padded ("constant") centred frames times the window"""
    B, L = wave.shape
    flat = wave.double().reshape(-1)
    out = torch.zeros((B, nframes, NFFT), dtype=torch.float64)
    for b in range(B):
        base = b * (L if stride is None else stride)
        row = torch.cat([flat[base:base + L], torch.full((max(0, L - (flat.numel() - base)),), float("nan"), dtype=torch.float64)])
        p = torch.cat([torch.zeros(NFFT // 2, dtype=torch.float64), row, torch.zeros(NFFT, dtype=torch.float64)])
        for f in range(nframes):
            s = f * hop + (0 if centre else NFFT // 2)
            out[b, f] = p[s:s + NFFT]
    return out * window.double()


def emu_mel(c, op16, ins, bug):
    frames = c.L // c.hop
    if frames == 0:
        return dict(out=None)
    window = _hann(periodic=False) if bug == "symmetric_window" else ins["window"]
    stride = frames * c.hop if bug == "batch_stride_wrong" else None
    xw = _mel_frames(ins["wave"], window, c.hop, frames, centre=(bug != "no_centre_pad"), stride=stride)
    mag = torch.fft.rfft(xw, dim=-1).abs()
    acc = mag @ ins["fb"].double().T
    out = torch.log(acc if bug == "no_log_floor" else acc.clamp_min(LOG_FLOOR)).float()
    if bug == "mel_loop_stops_at_256":
        bits(out)[:, :, 256:] = SENT32
    return dict(out=out)                                    # last_frame_kept writes behind the output: host_backend


def chk_mel(c, op16, ins, got):
    """Reference: fp64 framing, the fp32 window table, rfft, the fp32 filterbank table, log(max(., 1e-5f)).  Per frame, with xw the
    windowed frame and X its transform (||X||_2 = 32 ||xw||_2 over all 1024 bins):
        windowing       one rounding per sample: ||d xw||_2 <= u ||xw||_2, which the transform hands on as 32 u ||xw||_2
        FFT             ||dX||_2 <= FFT_REL ||X||_2 (above)                              => E = (FFT_REL + u) 32 ||xw||_2
        magnitude       a a, b b, their sum and the square root: three roundings of mag, plus |dX_k|
        filterbank      |d acc_m| <= sum_k |dX_k| f_mk + (3 + 514) u sum_k mag_k f_mk <= E ||f_m||_2 (1 + 3 u) + 517 u acc_m   (Cauchy-Schwarz;
                        514 u: 513 products and additions in any order)
    The output must lie in [log(max(acc - d, 1e-5f)), log(max(acc + d, 1e-5f))], widened by the granted logf figure."""
    out = got["out"]
    frames = c.L // c.hop
    if frames == 0:
        untouched = bits(out.contiguous()) == SENT32
        return [] if bool(untouched.all()) else [f"out: {int((~untouched).sum())} elements written although L < hop"]
    xw = _mel_frames(ins["wave"], ins["window"], c.hop, frames)
    fb = ins["fb"].double()
    acc = torch.fft.rfft(xw, dim=-1).abs() @ fb.T
    E = (FFT_REL + U) * 32.0 * xw.norm(dim=-1, keepdim=True)
    d = E * fb.norm(dim=-1) * (1 + 3 * U) + 517 * U * acc
    lo, hi = torch.log((acc - d).clamp_min(LOG_FLOOR)), torch.log((acc + d).clamp_min(LOG_FLOOR))
    lo, hi = lo - ULP_LOG * 2 * U * lo.abs(), hi + ULP_LOG * 2 * U * hi.abs()
    g = out.double()
    bad = []
    miss = ~((g >= lo) & (g <= hi))
    mid = torch.log(acc.clamp_min(LOG_FLOOR))
    ratio = ((g - mid).abs() / torch.maximum(hi - mid, mid - lo)).nan_to_num(float("inf"))
    WORST[(c.id, op16)] = float(ratio.max())
    if miss.any():
        i = int(miss.reshape(-1).nonzero()[0])
        bad.append(f"out: {int(miss.sum())} elements outside the interval (worst {float(ratio.max()):.2f} x), first at {i}: got "
                   f"{g.reshape(-1)[i].item()!r} want [{lo.reshape(-1)[i].item()!r}, {hi.reshape(-1)[i].item()!r}]")
    if c.sig == "silence" and not bool((bits(out.contiguous()) == bits(out.contiguous()).reshape(-1)[0]).all()):
        bad.append("out: silence does not give one and the same logf(1e-5f) everywhere")
    return bad


# ================================================================================================================================
# ISTFT head
# ================================================================================================================================
IST_FRAMES = (1, 2, 3, 4, 5, 6, 37)
IST_LDX = (1026, 1032, 1280)
IST_VARS = ("plain", "extreme")


def cases_istft():
    cs = []
    i = 0
    for nf in IST_FRAMES:
        for B, entry in ((1, "plain"), (1, "batch"), (3, "batch")):
            for hop in (256, 128, 512):
                if hop != 256 and (nf + B + i) % 3:       # a third of the other hops
                    i += 1
                    continue
                cs.append(Case("istft", nframes=nf, B=B, entry=entry, hop=hop, ldx=IST_LDX[i % 3], var=IST_VARS[(i // 3) % 2]))
                i += 1
    for ldx in IST_LDX:                                   # every row stride with both inputs at a size with edges and interior
        for var in IST_VARS:
            cs.append(Case("istft", nframes=6, B=3, entry="batch", hop=256, ldx=ldx, var=var))
    return list({c.id: c for c in cs}.values())           # one of these is in the round above already


def gen_istft(c, op16, r):
    rows = c.B * c.nframes
    x = _randn(r, rows, c.ldx)                            # the columns behind 1026 are read by nobody
    mag = _randn(r, rows, NBIN, scale=1.5)
    mag = mag - 2.0 * torch.arange(c.B, dtype=torch.float32).repeat_interleave(c.nframes).reshape(rows, 1)      # rows of the batch differ in scale
    ph = torch.from_numpy(r.uniform(-math.pi, math.pi, (rows, NBIN)).astype(np.float32))
    if c.var == "extreme":
        mag[:, 5::17] = 9.0                               # beyond the clip at 100
        mag[:, 7::19] = 89.0                              # expf overflows into the clip
        mag[:, 11::13] = -100.0
        ph = torch.from_numpy(r.uniform(-100.0, 100.0, (rows, NBIN)).astype(np.float32))
        ph[:, 3], ph[:, 4] = 100.0, -100.0
    # the "imaginary" part of DC and Nyquist must be ignored: sizeable bins with phases that have one
    mag[:, 0], mag[:, NBIN - 1] = 3.0, 3.5
    ph[:, 0], ph[:, NBIN - 1] = 1.0, -2.0
    x[:, :NBIN], x[:, NBIN:2 * NBIN] = mag, ph
    out_len = c.hop * (c.nframes - 1)
    spec = dict(wave=dict(shape=(c.B, out_len if out_len else c.hop), dtype=torch.float32, guard=2 * c.hop),
                frames=dict(shape=(rows, NFFT), dtype=torch.float32, guard=NFFT))
    return dict(x=x, window=_hann()), spec


def _ist_spec(x, clip=True, ldx=None):
    """rows of x -> complex128 [rows][513]; ldx: the row stride a kernel that ignores the real one would use"""
    if ldx is not None:
        flat = torch.cat([x.reshape(-1), torch.full((ldx,), float("nan"))])
        x = torch.stack([flat[i * ldx:i * ldx + 2 * NBIN] for i in range(x.shape[0])])
    m = torch.exp(x[:, :NBIN].double())
    if clip:
        m = m.clamp(max=100.0)
    p = x[:, NBIN:2 * NBIN].double()
    return torch.complex(m * torch.cos(p), m * torch.sin(p))


def _ist_ola(fr, w, B, nf, hop, bug=None):
    """overlap-add of [B * nf][1024] windowed frames, the window-square envelope and the trim of 512 at both ends, in fp64"""
    out_len = hop * (nf - 1)
    total = NFFT + hop * (nf - 1)
    w2 = w * w
    wave = torch.zeros((B, out_len), dtype=torch.float64)
    interior = sum(float(w2[o]) for o in range(NFFT // 2 % hop, NFFT, hop))
    for b in range(B):
        # ola_reads_next_row: the last-frame clamp is missing, the sum runs on into the frames of the next row (NaN behind the last)
        extra = NFFT // hop if bug == "ola_reads_next_row" else 0
        y, env = torch.zeros(total + extra * hop, dtype=torch.float64), torch.zeros(total + extra * hop, dtype=torch.float64)
        for f in range(nf + extra):
            row = b * nf + f
            y[f * hop:f * hop + NFFT] += fr[row] if row < fr.shape[0] else float("nan")
            env[f * hop:f * hop + NFFT] += w2
        if bug == "envelope_of_full_overlap":
            env = torch.full_like(env, interior)
        s0 = NFFT // 2 + (hop if bug == "trim_off_by_hop" else 0)
        wave[b] = (y / env)[s0:s0 + out_len]
    return wave


def emu_istft(c, op16, ins, bug):
    x, w = ins["x"], ins["window"].double()
    S = _ist_spec(x, clip=(bug != "no_clip"), ldx=(2 * NBIN if bug == "ldx_ignored" else None))
    if bug == "conj_sign":
        S = S.conj()
    leak = S[:, 0].imag[:, None] + S[:, NBIN - 1].imag[:, None] * (1.0 - 2.0 * (torch.arange(NFFT) % 2))
    S = S.clone()
    S[:, 0], S[:, NBIN - 1] = S[:, 0].real + 0j, S[:, NBIN - 1].real + 0j
    t = torch.fft.irfft(S, n=NFFT, dim=-1)
    if bug == "nyquist_imag_kept":                        # as a packed real transform that does not zero them would: into the samples
        t = t + leak / NFFT
    fr = t * w
    out = dict(frames=fr.float())
    if c.nframes > 1:
        out["wave"] = _ist_ola(fr, w, c.B, c.nframes, c.hop, bug).float()
    return out


def chk_istft(c, op16, ins, got):
    """Reference: fp64 torch.istft of min(exp(mag), 100) e^{i phase} (hann, centred), and for the frame scratch irfft times the window.
    Per frame, with S the Hermitian-extended spectrum (1024 bins) and t = 1024 irfft(S) (||t||_2 = 32 ||S||_2):
        spectrum    expf: 2 ULP_EXP u relative on the magnitude (the clipped ones are exact); sincosf: PH_ABS u absolute on each of cos and
                    sin; one product each: |dS_k| <= (2 ULP_EXP + sqrt(2) PH_ABS + 1) u |S_k| = REL_S |S_k|, handed on as 32 REL_S ||S||_2
                    (a magnitude below the normal range, exp(-100), may be flushed: 1e-37 absolute covers it)
        FFT         ||dt||_2 <= FFT_REL ||t||_2; only this 2-norm is known, so it stands for every sample: E = (FFT_REL + REL_S) 32 ||S||_2
        frame       fr_i = t_i (1 / 1024) window_i: two roundings: |d fr_i| <= E window_i / 1024 (1 + 2 u) + 2 u |fr_i|
        overlap-add at most A = n_fft / hop + 1 terms, A u of the absolute sum; the fp32 envelope: a product and an addition per term,
                    (A + 1) u relative; one correctly rounded division:
                    |d wave| <= [sum_f E_f window / 1024 (1 + 4 u) + (2 A + 4) u sum_f |fr|] / env"""
    x, w = ins["x"], ins["window"].double()
    S = _ist_spec(x)
    S[:, 0], S[:, NBIN - 1] = S[:, 0].real + 0j, S[:, NBIN - 1].real + 0j
    fr = torch.fft.irfft(S, n=NFFT, dim=-1) * w
    REL_S = (2 * ULP_EXP + math.sqrt(2.0) * PH_ABS + 1) * U
    full2 = 2 * (S.abs() ** 2).sum(-1) - S[:, 0].abs() ** 2 - S[:, NBIN - 1].abs() ** 2
    E = (FFT_REL + REL_S) * 32.0 * full2.sqrt().reshape(-1, 1) + 32.0 * 32.0 * 1e-37
    dfr = E * w / NFFT * (1 + 2 * U) + 2 * U * fr.abs()
    bad = chk_f32("frames", got["frames"], fr, dfr)
    worst = float(((got["frames"].double() - fr).abs() / dfr.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    wave = got["wave"]
    if c.nframes == 1:
        untouched = bits(wave.contiguous()) == SENT32
        if not bool(untouched.all()):
            bad.append(f"wave: {int((~untouched).sum())} elements written although one frame gives no sample")
    else:
        ref = torch.istft(S.reshape(c.B, c.nframes, NBIN).transpose(1, 2), NFFT, hop_length=c.hop, window=w, center=True)
        A = NFFT // c.hop + 1
        B1 = _ist_ola(E * w / NFFT, w, c.B, c.nframes, c.hop) * (1 + 4 * U)           # the same overlap-add of the frame bounds
        B2 = _ist_ola(fr.abs(), w, c.B, c.nframes, c.hop) * (2 * A + 4) * U
        bad += chk_f32("wave", wave, ref, B1 + B2)
        worst = max(worst, float(((wave.double() - ref).abs() / (B1 + B2).clamp_min(1e-300)).nan_to_num(float("inf")).max()))
    WORST[(c.id, op16)] = worst
    return bad


# ================================================================================================================================
# noise: f5_noise_normal against f5_tts_mlx_amd/rng.py, and the float path alone on chosen bit patterns
# ================================================================================================================================
def _rng():
    from f5_tts_mlx_amd import rng
    return rng


def cases_noise():
    def k(name, N, mel, durs, seeds=None, refuse=0):
        B = len(durs)
        return Case("noise", name=name, B=B, N=N, mel=mel, durs=tuple(durs), seeds=tuple(seeds or [3 + 1000003 * b for b in range(B)]),
                    refuse=refuse)
    return [
        k("no_padding", 37, 100, [37]),
        k("dur1_small", 40, 100, [1]),                                    # N * mel = 4000 < 4096
        k("dur1_large", 93, 100, [1, 1]),                                 # N * mel = 9300 > 4096: the strided zero fill
        k("odd_count", 9, 7, [5, 1, 9], [5, 6, 7]),                       # odd mel * dur: the last counter pair is half used
        k("seven_values", 4, 7, [1], [0]),
        k("longest_and_shortest", 257, 100, [257, 1, 129], [2 ** 40 + 7, 123456789, 2 ** 63 - 1]),
        k("same_seed", 50, 100, [50, 20, 50], [3, 3, 3]),
        k("B256", 3, 2, [1 + (b % 3) for b in range(256)], list(range(256))),
        k("B257_refused", 3, 2, [1] * 257, refuse=1),
        k("dur0_refused", 8, 4, [3, 0], refuse=1),
        k("dur_beyond_N_refused", 8, 4, [3, 9], refuse=1),
    ]


def gen_noise(c, op16, r):
    n = min(c.B, 256) * c.N * c.mel                       # B = 257 is refused before anything is written
    return dict(seeds=list(c.seeds), durs=list(c.durs)), dict(y0=dict(shape=(n,), dtype=torch.float32, guard=c.N * c.mel))


def _noise_threads(c):
    """the threads per batch element f5_noise_normal launches (csrc/noise.hip)"""
    half = (max(c.durs) * c.mel + 1) // 2
    threads = max(half, 4096)
    if threads > c.N * c.mel:
        threads = max(c.N * c.mel, half)
    return cdiv(threads, 256) * 256


def emu_noise(c, op16, ins, bug):
    if c.refuse:
        return dict(y0=None)
    rng = _rng()
    y = torch.zeros((c.B, c.N, c.mel))
    for b, (sd, d) in enumerate(zip(c.seeds, c.durs)):
        if bug == "seed_halves_swapped":
            sd = ((sd & 0xFFFFFFFF) << 32) | (sd >> 32)
        if bug == "dur_of_wrong_batch":
            d = c.durs[0]
        z = rng.mlx_like_normal(sd, (c.mel, d))
        z = z.reshape(d, c.mel) if bug == "frame_major_draw" else z.T
        if bug == "odd_pair_dropped" and (c.mel * d) % 2:
            i = (c.mel * d + 1) // 2 - 1                                   # value index of the first output of the half-used pair
            z = z.copy()
            z[i % d, i // d] = np.float32(np.nan)
        y[b, :d] = torch.from_numpy(np.ascontiguousarray(z))
        if bug == "pad_not_zero":                                          # one pad element per thread, no stride
            pad = y[b, d:].reshape(-1)
            bits(pad)[_noise_threads(c):] = SENT32
    return dict(y0=y.reshape(-1))


def _chk_normal(name, op, g, ref):
    """every value within one fp32 spacing of rng.py; the bit-equal count goes into the op's pool"""
    g64, r64 = g.astype(np.float64), ref.astype(np.float64)
    ok = np.abs(g64 - r64) <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    p = POOL.setdefault(op, [0, 0])
    p[0] += int(np.sum(g == ref))
    p[1] += g.size
    if not ok.all():
        i = int(np.flatnonzero(~ok.reshape(-1))[0])
        return [f"{name}: {int((~ok).sum())} values more than one fp32 spacing from the host generator, first at {i}: got "
                f"{g.reshape(-1)[i]!r} want {ref.reshape(-1)[i]!r}"]
    return []


def pool_reset(op):
    POOL[op] = [0, 0]


def pool_findings(op):
    """the rule of tests/test_model_gpu.py test_device_noise_matches_the_host_generator, pooled over all values of the op's cases (a
    draw of 7 values cannot have a share of 0.999 of its own unless all are equal)"""
    eq, n = POOL.get(op, [0, 0])
    share = eq / max(n, 1)
    print(f"[convaudio matrix] {op}: bit-equal share {share:.6f} of {n} values")
    return [] if share >= 0.999 else [f"{op}: only {share:.6f} of {n} values are bit-equal to the host generator (0.999 asked)"]


def chk_noise(c, op16, ins, got):
    y = got["y0"]
    if c.refuse:
        untouched = bits(y.contiguous()) == SENT32
        return [] if bool(untouched.all()) else [f"y0: {int((~untouched).sum())} elements written by a call that must be refused"]
    rng = _rng()
    y = y.reshape(c.B, c.N, c.mel).numpy()
    bad = []
    for b, (sd, d) in enumerate(zip(c.seeds, c.durs)):
        pad = y[b, d:]
        if not np.all(pad.view(np.uint32) == 0):
            bad.append(f"y0[{b}]: {int(np.sum(pad.view(np.uint32) != 0))} pad elements are not +0.0")
        bad += _chk_normal(f"y0[{b}]", "noise", y[b, :d], rng.mlx_like_normal(sd, (c.mel, d)).T)
    return bad


NB_NAMED = (0, 1, 127, 128, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF)
# what rng.py gives there (the lowest 127 patterns and the highest 256 sit on the clamps of the uniform mapping)
NB_NAMED_WANT = (-5.4199829, -5.4199829, -5.2947040, -5.2947040, 7.4703344e-08, 7.4703344e-08, 5.4199829, 5.4199829, 5.4199829, 5.4199829)


def cases_noise_bits():
    return [Case("noise_bits", which=w) for w in ("named", "lowest", "highest", "stride")]


def noise_bit_patterns(which):
    n = 1 << 16
    if which == "named":
        return np.array(NB_NAMED, dtype=np.uint32)
    if which == "lowest":
        return np.arange(n, dtype=np.uint32)
    if which == "highest":
        return (np.arange(n, dtype=np.uint64) + np.uint64(2 ** 32 - n)).astype(np.uint32)
    step = (2 ** 32 - 2 * n) // n                        # 65534: an even stride, so an odd term goes with it
    return (np.uint64(n) + np.arange(n, dtype=np.uint64) * np.uint64(step) + (np.arange(n, dtype=np.uint64) % np.uint64(7))).astype(np.uint32)


def gen_noise_bits(c, op16, r):
    b = noise_bit_patterns(c.which)
    return dict(bits=torch.from_numpy(b.view(np.int32).copy())), dict(out=dict(shape=(b.size,), dtype=torch.float32))


def emu_noise_bits(c, op16, ins, bug):
    b = ins["bits"].numpy().view(np.uint32)
    if bug is None:
        return dict(out=torch.from_numpy(_rng().bits_to_normal(b)))
    from scipy.special import erfinv
    u = b.astype(np.float32) / np.float32(0xFFFFFFFF)
    lo = np.nextafter(np.float32(-1.0), np.float32(0.0))
    if bug != "no_upper_clamp":
        u = np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0)))
    if bug == "fma_in_uniform":
        # (1 - lo) u + lo in one rounding, on the unrounded factor 2 - 2^-24.  With the factor as fp32 forms it, 1 - lo = 2.0f, the
        # product is exact and a fused multiply-add gives the same bits as the two steps: only the folded factor can go wrong.
        u = ((1.0 - np.float64(lo)) * u.astype(np.float64) + np.float64(lo)).astype(np.float32)
    else:
        u = (np.float32(1.0) - lo) * u + lo
    with np.errstate(all="ignore"):
        return dict(out=torch.from_numpy((np.float32(np.sqrt(2.0)) * erfinv(u.astype(np.float64))).astype(np.float32)))


def chk_noise_bits(c, op16, ins, got):
    g = got["out"].numpy()
    b = ins["bits"].numpy().view(np.uint32)
    bad = []
    if not np.isfinite(g).all():
        i = int(np.flatnonzero(~np.isfinite(g))[0])
        bad.append(f"out: {int((~np.isfinite(g)).sum())} values are not finite, first at bits {int(b[i]):#010x}: {g[i]!r}")
    bad += _chk_normal("out", "noise_bits", g, _rng().bits_to_normal(b))
    if c.which == "named":
        want = np.array(NB_NAMED_WANT, dtype=np.float32)
        off = np.abs(g.astype(np.float64) - want.astype(np.float64)) > np.spacing(np.abs(want)).astype(np.float64)
        if off.any():
            bad.append(f"out: named patterns {[hex(int(v)) for v in b[off]]} give {g[off].tolist()}, not {want[off].tolist()}")
    return bad


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _op(name, tracked=False, packs=False, op16=False):
    g = globals()
    return dict(cases=g["cases_" + name], gen=g["gen_" + name], emu=g["emu_" + name], chk=g["chk_" + name], tracked=tracked, exact=False,
                packs=packs, op16=op16)


OPS = {
    "convpos": _op("convpos", tracked=True, packs=True, op16=True),
    "mel": _op("mel"),
    "istft": _op("istft"),
    "noise": _op("noise"),
    "noise_bits": _op("noise_bits"),
}
POOLED = ("noise", "noise_bits")


def op_types(op):
    """the operand types an op is run under: both where it has 16-bit operands"""
    return OPS16 if OPS[op]["op16"] else OPS16[:1]


def cases(op=None):
    if op is not None:
        return OPS[op]["cases"]()
    return [c for o in OPS for c in OPS[o]["cases"]()]


@contextlib.contextmanager
def _table():
    """rowops_matrix's build / check / host_backend look their op up in its table OPS: ours for the length of a call"""
    old, RM.OPS = RM.OPS, OPS
    try:
        yield
    finally:
        RM.OPS = old


def build(c, op16, device="cpu"):
    with _table():
        return RM.build(c, op16, device)


def check(io):
    with _table():
        return RM.check(io)


def host_backend(bug=None):
    """rowops_matrix.host_backend, plus the two mistakes that write behind an output instead of into it"""
    inner = RM.host_backend(None if bug in ("tail_rows_written", "last_frame_kept") else bug)

    def run(io):
        c = io.case
        with _table():
            inner(io)
        if bug == "tail_rows_written" and c.op == "convpos":
            o = io.outs["hi"] if c.mode == 0 else io.outs["out"]
            rows = cdiv(c.N, 128) * 128 - c.N             # rows >= seq_len of the last tile of the last batch element
            bits(o.raw)[o.g0 + o.n:o.g0 + o.n + rows * c.C] = 0
        if bug == "last_frame_kept" and c.op == "mel":
            o = io.outs["out"]
            frames = c.L // c.hop
            at = o.g0 + (o.n if frames else 0)            # frame L / hop of the last batch element
            bits(o.raw)[at:at + c.n_mels] = 0
    return run
