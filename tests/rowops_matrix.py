"""The row / elementwise kernel test matrix (csrc/rowops.hip): case generators, guarded buffers, fp64 (or exact) references, checkers.

Shared by tests/test_rowops_matrix_gpu.py (runs the cases through the C ABI) and tests/test_rowops_matrix_host.py (runs the checkers
over a torch emulation of the kernels, right and deliberately wrong, on the CPU).  Nothing here needs a GPU or the library.

Every op of the table OPS has
    cases()                    -> list of Case
    gen(c, op16, r)            -> (inputs, output specs): CPU tensors, and for every output its shape / dtype / guard size
    emu(c, op16, ins, bug)     -> the outputs as a plain fp32 torch emulation of the kernel (bug names a deliberate mistake)
    chk(c, op16, ins, got)     -> list of violations of the fp64 / exact reference
build() places the inputs in front of NaN (poison for integers) and every output between guard bands filled with a sentinel bit
pattern (the payload is pre-filled with it too: an element the kernel should have written and did not is a mismatch); check() adds
the guard comparison and the fp16 range flag to the op's own checker.

Tolerances.  u = 2^-24 is the unit roundoff of fp32.  An op that had a relative bound in tests/test_ops_gpu.py keeps it (of
max(1, max |ref|), as there).  The others get a bound counted from the kernel's expression (written next to each checker).  The
library functions are allowed four times the largest error measured on an MI355X against fp64 over the arguments these kernels
produce (2^21 samples per function plus the exact grids of the tables; the margin is for arguments the sample missed):
    function   measured (ULP)   granted (ULP)
    rsqrtf     0.863            3.452
    expf       0.845            3.380
    log1pf     0.557            2.228
    sinf       1.572            6.288
    cosf       1.564            6.256
    powf       1.269            5.076
sqrtf and the fp32 division came out correctly rounded (0.500) and count as one rounding each.
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

OPS16 = ("bf16", "f16")
U = 2.0 ** -24
ULP_RSQRT, ULP_EXP, ULP_LOG1P, ULP_SIN, ULP_COS, ULP_POW = 4 * 0.863, 4 * 0.845, 4 * 0.557, 4 * 1.572, 4 * 1.564, 4 * 1.269
SAT = 65504.0
OUTLIER = 3.0e5              # beyond 2 x 65504: the residual of the clamped hi half leaves the fp16 range as well
SENT32 = 0x7FC0BEEF          # 4-byte sentinel: an fp32 NaN with a payload
SENT16 = 0x7FA5              # 2-byte sentinel: a NaN in bf16 and in fp16
SENT8 = 0xA5
GUARD = 64
LN_EPS = 1e-6


def cdiv(a, b):
    return -(-a // b)


def eps_op(op16):
    """unit roundoff of the operand type: bf16 has 8 significand bits, fp16 11 (tests/test_ops_gpu.py eps_op)"""
    return 2.0 ** -8 if op16 == "bf16" else 2.0 ** -11


def floor_op(op16):
    """absolute rounding error where the operand type is subnormal: fp16 spaces 2^-24 below 2^-14; bf16 has fp32's exponent range"""
    return 2.0 ** -25 if op16 == "f16" else 0.0


def op_dtype(op16):
    return torch.bfloat16 if op16 == "bf16" else torch.float16


def to_op(x, op16):
    """fp32 -> operand type, round to nearest even; fp16 saturates at +-65504"""
    return (x.clamp(-SAT, SAT) if op16 == "f16" else x).to(op_dtype(op16))


def split(x, op16):
    """fp32 -> (hi, lo): what f5test.split_bf16 computes under the operand mode (csrc/op16.hpp f5_split)"""
    hi = to_op(x, op16)
    lo = to_op(x - hi.to(torch.float32), op16)
    return hi, lo


def bits(t):
    if t.element_size() == 2:
        return t.view(torch.int16)
    if t.element_size() == 4:
        return t.view(torch.int32)
    return t.view(torch.uint8)


def _sentinel(t):
    n = t.element_size()
    if n == 2:
        return SENT16
    return SENT32 if n == 4 else SENT8


class Case:
    def __init__(self, op, **kw):
        self.op, self.kw = op, kw

    def __getattr__(self, k):
        try:
            return self.__dict__["kw"][k]
        except KeyError:
            raise AttributeError(k) from None

    @property
    def id(self):
        return self.op + "[" + ",".join(f"{k}={v}" for k, v in self.kw.items()) + "]"

    def seed(self, op16):
        return zlib.crc32((self.id + op16).encode())

    def __repr__(self):
        return self.id


class Out:
    """an output of `shape` between two guard bands of at least `guard` elements; everything starts as the sentinel"""

    def __init__(self, shape, dtype, device, guard=GUARD, init=None, offset=0):
        self.n = int(np.prod(shape))
        g = cdiv(max(GUARD, guard), 16) * 16            # keeps the payload on 16 bytes whatever the element size
        self.g0 = g + offset
        self.raw = torch.empty(self.g0 + self.n + g, dtype=dtype, device=device)
        bits(self.raw).fill_(_sentinel(self.raw))
        self.t = self.raw[self.g0:self.g0 + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def guard_violations(self, name):
        b, s = bits(self.raw), _sentinel(self.raw)
        bad = []
        for which, band in (("front", b[:self.g0]), ("back", b[self.g0 + self.n:])):
            hit = (band != s).nonzero()
            if hit.numel():
                bad.append(f"{name}: {which} guard band overwritten ({hit.numel()} elements, first at {int(hit[0])})")
        return bad


def pad_in(t, device):
    """an input followed by 64 elements of NaN (floats) or of a value that is wrong everywhere (integers)"""
    if t is None:
        return None
    flat = torch.empty(t.numel() + 64, dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1)
    flat[t.numel():] = float("nan") if t.is_floating_point() else 1
    flat = flat.to(device)
    return flat[:t.numel()].view(t.shape)


class IO:
    pass


def build(c, op16, device="cpu"):
    r = np.random.default_rng(c.seed(op16))
    ins, spec = OPS[c.op]["gen"](c, op16, r)
    io = IO()
    io.case, io.op16, io.device = c, op16, device
    io.ins_cpu = ins
    io.ins = {k: (pad_in(v, device) if isinstance(v, torch.Tensor) else v) for k, v in ins.items()}
    io.outs = {}
    for name, s in spec.items():
        io.outs[name] = None if s is None else Out(s["shape"], s["dtype"], device, s.get("guard", GUARD), s.get("init"), s.get("offset", 0))
    io.flag = torch.zeros(1, dtype=torch.int32, device=device) if OPS[c.op].get("tracked") else None
    return io


def check(io):
    """-> list of violations: guard bands, the fp16 range flag, then the op's own reference"""
    c, op16 = io.case, io.op16
    bad = []
    for name, o in io.outs.items():
        if o is not None:
            bad += o.guard_violations(name)
    if io.flag is not None:
        want = 4 if (op16 == "f16" and c.kw.get("outlier")) else 0
        got = int(io.flag.cpu()[0])
        if got != want:
            bad.append(f"range flag {got}, expected {want}")
    got = {k: (None if o is None else o.t.detach().cpu()) for k, o in io.outs.items()}
    bad += OPS[c.op]["chk"](c, op16, io.ins_cpu, got)
    return [f"{c.id} {op16}: {b}" for b in bad]


def host_backend(bug=None):
    """runs the torch emulation into the buffers of an IO; `bug` is a mistake of the emulation or one of the generic ones"""

    def run(io):
        c, op16 = io.case, io.op16
        res = OPS[c.op]["emu"](c, op16, io.ins_cpu, None if bug in GENERIC_BUGS else bug)
        flag = res.pop("flag", 0)
        for name, t in res.items():
            if io.outs.get(name) is not None and t is not None:
                io.outs[name].t.copy_(t)
        if io.flag is not None:
            io.flag.fill_(0 if bug == "no_flag" else flag)
        first = next(o for o in io.outs.values() if o is not None and o.n > 0)
        if bug == "guard_front":
            bits(first.raw)[first.g0 - 1] = 0
        elif bug == "guard_back":
            bits(first.raw)[first.g0 + first.n] = 0
        elif bug == "one_off":
            # one element of the first output moved: by one bit where the op is exact, far outside the bound where it is computed
            flat = first.t.reshape(-1)
            i = flat.numel() // 2
            if OPS[c.op].get("exact") or not flat.is_floating_point():
                bits(flat)[i] ^= 1
            else:
                flat[i] = flat[i] * 1.05 + 0.05
    return run


GENERIC_BUGS = ("guard_front", "guard_back", "one_off", "no_flag")


# ---- shared checkers -----------------------------------------------------------------------------------------------------------
def _first(mask):
    i = int(mask.reshape(-1).nonzero()[0])
    return i


def chk_exact(name, got, want):
    if got is None:
        return []
    if got.shape != want.shape:
        return [f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"]
    ne = bits(got.contiguous()) != bits(want.contiguous())
    if ne.any():
        i = _first(ne)
        return [f"{name}: {int(ne.sum())} elements differ bit for bit, first at {i}: got {got.reshape(-1)[i].item()!r} want {want.reshape(-1)[i].item()!r}"]
    return []


def chk_f32(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound: number or tensor); NaN fails"""
    if got is None:
        return []
    err = (got.double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    bad = ~(err <= bound)
    if bad.any():
        i = _first(bad)
        worst = float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
        return [f"{name}: {int(bad.sum())} elements outside the bound (worst {worst:.2f} x), first at {i}: got {got.reshape(-1)[i].item()!r} "
                f"ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item():.3e}"]
    return []


def chk_pair(name, hi, lo, ref, B, op16):
    """(hi, lo) of a computed value v, v any fp32 within B of ref: |hi - v| <= eps |v| and |hi + lo - v| <= eps^2 |v| (plus the
    subnormal floor of the type).  Under fp16 a v beyond +-65504 must give hi = +-65504 exactly and a finite lo."""
    bad = []
    e, fl = eps_op(op16), floor_op(op16)
    ref = ref.double()
    B = torch.as_tensor(B, dtype=torch.float64).expand_as(ref)
    a = ref.abs()
    over = (a - B > SAT) if op16 == "f16" else torch.zeros_like(a, dtype=torch.bool)
    edge = ((a + B >= SAT) & ~over) if op16 == "f16" else torch.zeros_like(over)       # may or may not saturate: only finiteness
    plain = ~(over | edge)
    if hi is not None:
        h = hi.double()
        if not torch.isfinite(h).all():
            bad.append(f"{name}_hi: {int((~torch.isfinite(h)).sum())} values are not finite")
        if over.any() and not torch.equal(h[over], torch.sign(ref[over]) * SAT):
            bad.append(f"{name}_hi: a value beyond the fp16 range is not clamped to +-65504")
        bad += chk_f32(f"{name}_hi", hi[plain], ref[plain], e * (a + B)[plain] + B[plain] + fl)
    if lo is not None:
        l = lo.double()
        if not torch.isfinite(l).all():
            bad.append(f"{name}_lo: {int((~torch.isfinite(l)).sum())} values are not finite")
        if hi is not None:
            bad += chk_f32(f"{name}_hi+lo", (hi.double() + l)[plain], ref[plain], B[plain] + e * e * (a + B)[plain] + fl)
        else:                                      # alone, lo is only known to be a rounding residual
            bad += chk_f32(f"{name}_lo", lo[plain], torch.zeros_like(ref[plain]), e * (a + B)[plain] * (1 + e) + fl)
    return bad


def chk_split(name, hi, lo, v, op16):
    """(hi, lo) of a KNOWN fp32 value: bit for bit the split of f5test.split_bf16"""
    wh, wl = split(v, op16)
    return chk_exact(f"{name}_hi", hi, wh) + chk_exact(f"{name}_lo", lo, wl)


def _randn(r, *shape, scale=1.0):
    return torch.from_numpy((r.standard_normal(shape) * scale).astype(np.float32))


def _pair_spec(shape, op16, lo, guard, init=None):
    s = dict(shape=shape, dtype=op_dtype(op16), guard=guard, init=init)
    return {"hi": dict(s), "lo": dict(s) if lo else None}


def _emu_pack(v, op16, bug):
    """the packers of op16.hpp on an fp32 tensor, with the mistakes a packer can make"""
    if bug == "hi_truncated":
        step = v.abs().clamp_min(1e-30).log2().floor().exp2() * (2 * eps_op(op16))
        hi = (torch.trunc(v / step) * step).to(op_dtype(op16))
        return hi, to_op(v - hi.float(), op16)
    if bug == "f16_inf" and op16 == "f16":
        hi = v.to(torch.float16)
        return hi, (v - hi.float()).to(torch.float16)
    return split(v, op16)


def _flag_of(v, op16):
    return 4 if (op16 == "f16" and bool((v.abs() > SAT).any())) else 0


# ---- LayerNorm family ----------------------------------------------------------------------------------------------------------
LN_DIMS = (256, 512, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 9)


def _stress_rows(r, dim):
    """mean 1000 with unit spread; a constant row (variance 0); a single 1e4 spike; between two ordinary rows"""
    x = _randn(r, 5, dim)
    x[1] += 1000.0
    x[2] = 3.25
    x[3] = _randn(r, dim, scale=0.1)
    x[3, dim // 3] = 1.0e4
    return x


def _ln64(x, eps=LN_EPS):
    xd = x.double()
    m = xd.mean(-1, keepdim=True)
    v = ((xd - m) ** 2).mean(-1, keepdim=True)
    return (xd - m) / torch.sqrt(v + eps), m.squeeze(-1), 1.0 / torch.sqrt(v + eps)


def _wave_sum32(lanes):
    """f5_wave_sum (csrc/common.hpp) on [rows][64] fp32 partials: a butterfly over lane distances 32, 16, 8, 4, 2, 1"""
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ off]
    return lanes[:, :1]


def _row_stats32(flat, about_0=False):
    """(mean, variance) of fp32 rows in the kernels' own order: lane l owns columns i * 256 + 4 l ... + 3 of each 256-column chunk i, adds
    (a + b) + (c + d) per chunk, the wave tree finishes, and the sum meets the rounded constant 1 / dim"""
    rows, dim = flat.shape
    v = flat.reshape(rows, dim // 256, 64, 4)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(dim), dtype=torch.float32)
    s = torch.zeros((rows, 64))
    for i in range(dim // 256):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    m = _wave_sum32(s) * inv
    sq = torch.zeros((rows, 64))
    for i in range(dim // 256):
        for e in range(4):
            d = v[:, i, :, e] - (0.0 if about_0 else m)
            sq = sq + d * d
    return m, _wave_sum32(sq) * inv


def _ln32(x, bug=None, eps=LN_EPS):
    """fp32 emulation of the row statistics (two passes and the summation order of the kernels)"""
    dim = x.shape[-1]
    flat = x.reshape(-1, dim)
    if bug == "nv3_as_4" and dim == 768:
        # the wave reads 1024 columns of a 768-wide row: the statistics take in the head of the next row (NaN behind the last)
        src = torch.cat([flat.reshape(-1), torch.full((256,), float("nan"))])
        wide = torch.stack([src[i * 768:i * 768 + 1024] for i in range(flat.shape[0])])
        m, var = _row_stats32(wide)
    else:
        m, var = _row_stats32(flat, about_0=(bug == "var_about_0"))
    rstd = 1.0 / torch.sqrt(var + (0.0 if bug == "no_eps" else eps))
    return ((flat - m) * rstd).reshape(x.shape), m.reshape(x.shape[:-1])


def _ln_bound(rel, ref):
    """the project's bound: rel of max(1, max |ref|) (tests/test_ops_gpu.py), the stress rows included.  An element that was pushed out
    of the fp16 range on purpose (|ref| > 1e5) does not set the scale of the others: it answers for rel of its own magnitude."""
    a = ref.abs()
    big = a > 1.0e5
    rest = float(a[~big].max()) if bool((~big).any()) else 0.0
    return torch.where(big, rel * a, torch.full_like(a, rel * max(1.0, rest)))


def _ln_centring(c, mean, rstd, gain):
    """What the stress cases, and only they, get on top of the project's bound.  On an MI355X two of them miss it as it stands:
        ln_modulate dim 512, mean-1000 row (bf16 seed):  |err| 1.44e-4 against 1.06e-4 (1.36 x)
        ln_modulate dim 768, constant row (fp16 seed):   |err| 2.38e-4 against 2.12e-4 (1.12 x)
    and an emulation of the kernels' summation order gives the first figure bit for bit, so it is the arithmetic and not a defect:
    x - mean carries the absolute error of the mean, which rstd (1000 on the constant row) and the affine gain hand on.  That error
    is one rounding at the size of the mean for the last addition of its sum and one for the product with the rounded 1 / dim (the
    compiler contracts the product into the subtraction, which on the constant row leaves the rounding of 1 / 768 itself):
    2 u |mean| rstd |gain|, per element.  The error of the mean behind the first figure is 1.06 u |mean|."""
    if not c.kw.get("stress"):
        return 0.0
    return 2 * U * mean.double().abs().reshape(-1, 1) * rstd.reshape(-1, 1) * gain.double().abs().reshape(1, -1)


def cases_ln_modulate():
    cs = [Case("ln_modulate", dim=d, rows=n, mean=m, lo=lo) for d in LN_DIMS for n in LN_ROWS for m in (0, 1) for lo in (1, 0)]
    cs += [Case("ln_modulate", dim=d, rows=5, mean=m, lo=1, stress=1) for d in LN_DIMS for m in (0, 1)]
    cs += [Case("ln_modulate", dim=256, rows=5, mean=0, lo=lo, outlier=1) for lo in (1, 0)]
    return cs


def gen_ln_modulate(c, op16, r):
    x = _stress_rows(r, c.dim) if c.kw.get("stress") else _randn(r, c.rows, c.dim) * 3 + 0.5
    sc, sh = _randn(r, c.dim, scale=0.5), _randn(r, c.dim, scale=0.5)
    if c.kw.get("outlier"):
        sh[7] = OUTLIER
    spec = _pair_spec((c.rows, c.dim), op16, c.lo, 4 * c.dim)
    spec["mean"] = dict(shape=(c.rows,), dtype=torch.float32) if c.mean else None
    return dict(x=x, scale=sc, shift=sh), spec


def emu_ln_modulate(c, op16, ins, bug):
    xn, m = _ln32(ins["x"], bug)
    y = xn * (1.0 + ins["scale"]) + ins["shift"]
    hi, lo = _emu_pack(y, op16, bug)
    return dict(hi=hi, lo=lo, mean=m, flag=_flag_of(y, op16))


def chk_ln_modulate(c, op16, ins, got):
    xn, m, rstd = _ln64(ins["x"])
    ref = xn * (1 + ins["scale"].double()) + ins["shift"].double()
    bad = chk_pair("out", got["hi"], got["lo"], ref, _ln_bound(2e-5, ref) + _ln_centring(c, m, rstd, 1 + ins["scale"]), op16)
    # the row mean: NV * 4 additions per lane, 6 levels of the wave tree, the product with 1 / dim (itself rounded): n = 4 NV + 8 roundings
    n = 4 * (c.dim // 256) + 8
    bad += chk_f32("mean", got.get("mean"), m, n * U * ins["x"].double().abs().mean(-1))
    return bad


def _subsets():
    return [(f, h, l) for f in (1, 0) for h in (1, 0) for l in (1, 0) if f or h or l]


def cases_layernorm():
    cs = [Case("layernorm", dim=d, rows=n, f32=f, hi=h, lo=l) for d in LN_DIMS for n in LN_ROWS for f, h, l in _subsets()]
    cs += [Case("layernorm", dim=d, rows=5, f32=1, hi=1, lo=1, stress=1) for d in LN_DIMS]
    cs += [Case("layernorm", dim=256, rows=5, f32=f, hi=1, lo=1, outlier=1) for f in (1, 0)]
    return cs


def gen_layernorm(c, op16, r):
    x = _stress_rows(r, c.dim) if c.kw.get("stress") else _randn(r, c.rows, c.dim) * 3 + 0.5
    w, b = 1 + _randn(r, c.dim, scale=0.1), _randn(r, c.dim, scale=0.1)
    if c.kw.get("outlier"):
        b[7] = OUTLIER
    spec = _pair_spec((c.rows, c.dim), op16, 1, 4 * c.dim)
    if not c.hi:
        spec["hi"] = None
    if not c.lo:
        spec["lo"] = None
    spec["f32"] = dict(shape=(c.rows, c.dim), dtype=torch.float32, guard=4 * c.dim) if c.f32 else None
    return dict(x=x, w=w, b=b), spec


def emu_layernorm(c, op16, ins, bug):
    y = _ln32(ins["x"], bug)[0] * ins["w"] + ins["b"]
    hi, lo = _emu_pack(y, op16, bug)
    return dict(f32=y, hi=hi, lo=lo)


def chk_layernorm(c, op16, ins, got):
    xn, m, rstd = _ln64(ins["x"])
    ref = xn * ins["w"].double() + ins["b"].double()
    B = _ln_bound(2e-5, ref) + _ln_centring(c, m, rstd, ins["w"])      # ln_modulate's bound: the arithmetic is the same
    bad = chk_f32("f32", got["f32"], ref, B)
    if got["f32"] is not None:                    # the value the kernel packed is known: the pair is its split, bit for bit
        return bad + chk_split("out", got["hi"], got["lo"], got["f32"], op16)
    return bad + chk_pair("out", got["hi"], got["lo"], ref, B, op16)


DW_BN = ((1, 1), (1, 2), (1, 3), (3, 4), (2, 7), (3, 37))


def cases_dwconv_ln():
    cs = [Case("dwconv_ln", dim=d, B=1, N=n, lo=lo) for d in LN_DIMS for n in LN_ROWS for lo in (1, 0)]
    cs += [Case("dwconv_ln", dim=d, B=b, N=n, lo=lo) for d in LN_DIMS for b, n in DW_BN if not (b == 1 and n in LN_ROWS) for lo in (1, 0)]
    cs += [Case("dwconv_ln", dim=d, B=5, N=1, lo=1, stress=1) for d in LN_DIMS]
    cs += [Case("dwconv_ln", dim=256, B=2, N=5, lo=lo, outlier=1) for lo in (1, 0)]
    return cs


def gen_dwconv_ln(c, op16, r):
    d = c.dim
    x = _randn(r, c.B, c.N, d)
    dw_w, dw_b = _randn(r, d, 7, scale=0.4), _randn(r, d, scale=0.1)
    ln_w, ln_b = 1 + _randn(r, d, scale=0.1), _randn(r, d, scale=0.1)
    if c.kw.get("stress"):        # five sequences of one token: the centre tap alone, weight 1, no bias -> the conv hands the stress rows on
        x = _stress_rows(r, d).reshape(5, 1, d)
        dw_w[:, 3] = 1.0
        dw_b.zero_()
    if c.kw.get("outlier"):
        ln_b[7] = OUTLIER
    return dict(x=x, dw_w=dw_w, dw_b=dw_b, ln_w=ln_w, ln_b=ln_b), _pair_spec((c.B * c.N, d), op16, c.lo, 4 * d)


def _dwconv(x, w, b, bug=None):
    """depthwise k = 7, pad 3, zero padding per batch element; x [B][N][dim], w [dim][7]"""
    B, N, d = x.shape
    shift = 2 if bug == "conv_pad_off_by_one" else 3
    src = x.reshape(1, B * N, d) if bug == "conv_across_batch" else x
    n = src.shape[1]
    y = b.expand(src.shape).clone()
    for t in range(7):
        lo, hi = max(0, shift - t), min(n, n + shift - t)          # output positions whose tap t lands inside the sequence
        if hi > lo:
            y[:, lo:hi] += src[:, lo + t - shift:hi + t - shift] * w[:, t]
    return y.reshape(B, N, d)


def emu_dwconv_ln(c, op16, ins, bug):
    y = _dwconv(ins["x"], ins["dw_w"], ins["dw_b"], bug)
    z = (_ln32(y, bug)[0] * ins["ln_w"] + ins["ln_b"]).reshape(c.B * c.N, c.dim)
    hi, lo = _emu_pack(z, op16, bug)
    return dict(hi=hi, lo=lo, flag=_flag_of(z, op16))


def chk_dwconv_ln(c, op16, ins, got):
    y = _dwconv(ins["x"].double(), ins["dw_w"].double(), ins["dw_b"].double())
    xn, m, rstd = _ln64(y)
    ref = (xn * ins["ln_w"].double() + ins["ln_b"].double()).reshape(c.B * c.N, c.dim)
    return chk_pair("out", got["hi"], got["lo"], ref, _ln_bound(3e-5, ref) + _ln_centring(c, m, rstd, ins["ln_w"]), op16)


# ---- GRN -----------------------------------------------------------------------------------------------------------------------
def grn_scratch_floats(B, N, dim):
    return B * cdiv(N, 32) * dim + B * dim


def cases_grn():
    cs = []
    for d in (4, 100, 256, 260, 1536):
        for n in (1, 31, 32, 33, 64, 65):
            for b, zero in ((1, 0), (3, 0), (3, 1)):
                cs += [Case("grn", dim=d, N=n, B=b, zero=zero, lo=lo) for lo in (1, 0)]
    cs += [Case("grn", dim=256, N=33, B=3, zero=0, lo=lo, outlier=1) for lo in (1, 0)]
    return cs


def gen_grn(c, op16, r):
    g, gamma, beta = _randn(r, c.B, c.N, c.dim), _randn(r, c.dim, scale=0.1), _randn(r, c.dim, scale=0.1)
    if c.zero:
        g[1] = 0.0                 # Gx = 0 everywhere: only the 1e-6 of the denominator keeps Nx finite
    if c.kw.get("outlier"):
        beta[c.dim // 2] = OUTLIER
    spec = _pair_spec((c.B * c.N, c.dim), op16, c.lo, c.dim)
    spec["scratch"] = dict(shape=(grn_scratch_floats(c.B, c.N, c.dim),), dtype=torch.float32)
    return dict(g=g, gamma=gamma, beta=beta), spec


def emu_grn(c, op16, ins, bug):
    g = ins["g"]
    src = g[:, :(c.N // 32) * 32] if bug == "grn_drops_last_chunk" else g
    gx = torch.sqrt((src * src).sum(1, keepdim=True))
    count = cdiv(c.dim, 256) * 256 if bug == "grn_wrong_count" else c.dim
    nx = gx / (gx.sum(-1, keepdim=True) / count + 1e-6)
    y = (ins["gamma"] * (g * nx) + ins["beta"] + g).reshape(c.B * c.N, c.dim)
    hi, lo = _emu_pack(y, op16, bug)
    return dict(hi=hi, lo=lo, flag=_flag_of(y, op16))


def chk_grn(c, op16, ins, got):
    g = ins["g"].double()
    gx = torch.linalg.vector_norm(g, ord=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(-1, keepdim=True) + 1e-6)
    ref = (ins["gamma"].double() * (g * nx) + ins["beta"].double() + g).reshape(c.B * c.N, c.dim)
    return chk_pair("out", got["hi"], got["lo"], ref, _ln_bound(2e-5, ref), op16)


# ---- text embedding (exact) ----------------------------------------------------------------------------------------------------
TE_B, TE_N, TE_V = 3, 12, 20


def cases_text_embed():
    return [Case("text_embed", nt=TE_N + dn, max_pos=TE_N + dp, dim=d, pos=p, mask=m)
            for dn in (-4, 0, 3) for dp in (5, 0, -3) for d in (4, 128, 516) for p in (1, 0) for m in (1, 0)]


def gen_text_embed(c, op16, r):
    text = torch.from_numpy(r.integers(1, TE_V, (TE_B, c.nt)).astype(np.int32))
    text[0, 3] = 0                      # a real token with id 0 (1 after the shift)
    text[1, c.nt // 2:] = -1            # filler tail
    text[2, :] = -1                     # a row that is all filler
    table = _randn(r, TE_V + 1, c.dim)
    pos = _randn(r, c.max_pos, c.dim) if c.pos else None
    shape = (2, TE_B, TE_N)
    return dict(text=text, table=table, pos_table=pos), dict(out=dict(shape=shape + (c.dim,), dtype=torch.float32, guard=c.dim),
                                                             ids=dict(shape=shape, dtype=torch.int32), keep=dict(shape=shape, dtype=torch.uint8))


def _text_embed(c, ins, bug=None):
    text, table, pos = ins["text"], ins["table"], ins["pos_table"]
    ids = torch.zeros((TE_B, TE_N), dtype=torch.int64)
    m = min(c.nt, TE_N)
    ids[:, :m] = text[:, :m].to(torch.int64) + 1
    ids2 = torch.stack([ids, torch.zeros_like(ids)])                   # branch 1: the text is dropped
    keep = (ids != 0) if (c.mask or bug == "keep_ignores_nomask") else torch.ones_like(ids, dtype=torch.bool)
    keep2 = torch.stack([keep, keep])                                  # taken BEFORE the drop: the same for both branches
    if bug == "keep_after_drop":
        keep2 = (ids2 != 0) if c.mask else torch.ones_like(ids2, dtype=torch.bool)
    v = table[ids2]
    if pos is not None:
        n = torch.arange(TE_N)
        if bug == "pos_not_clamped":
            padded = torch.cat([pos, torch.full((TE_N, c.dim), float("nan"))])
            v = v + padded[n]
        else:
            v = v + pos[n.clamp_max(c.max_pos - 1)]
    out = torch.where(keep2[..., None], v, torch.zeros_like(v))
    return dict(out=out, ids=ids2.to(torch.int32), keep=keep2.to(torch.uint8))


def emu_text_embed(c, op16, ins, bug):
    return _text_embed(c, ins, bug)


def chk_text_embed(c, op16, ins, got):
    want = _text_embed(c, ins)
    return [b for k in ("ids", "keep", "out") for b in chk_exact(k, got[k], want[k])]


# ---- packers (exact) -----------------------------------------------------------------------------------------------------------
def cases_pack_bf16():
    shapes = ((1, 1, 1, 0), (5, 7, 16, 3), (9, 33, 40, 4), (4, 64, 64, 0), (300, 101, 128, 20))
    cs = [Case("pack_bf16", rows=a, cols=b, ld=l, col0=o, rowkeep=k, lo=lo) for a, b, l, o in shapes for k in (0, 1) for lo in (1, 0)]
    return cs + [Case("pack_bf16", rows=5, cols=7, ld=16, col0=3, rowkeep=0, lo=1, outlier=1)]


def gen_pack_bf16(c, op16, r):
    src = _randn(r, c.rows, c.cols)
    if c.kw.get("outlier"):
        src[2, 3], src[4, 0] = OUTLIER, -OUTLIER
    keep = torch.from_numpy((r.random(c.rows) < 0.6).astype(np.uint8)) if c.rowkeep else None
    return dict(src=src, rowkeep=keep), _pair_spec((c.rows, c.ld), op16, c.lo, c.ld)


def _embed_cols(c, t, op16, bug=None):
    """the packed columns inside an untouched (sentinel) [rows][ld] matrix"""
    full = torch.empty((c.rows, c.ld), dtype=op_dtype(op16))
    bits(full).fill_(SENT16)
    if bug == "ld_ignored":                    # rows written c.cols apart instead of c.ld
        flat = full.reshape(-1)
        for r_ in range(c.rows):
            flat[r_ * c.cols + c.col0:r_ * c.cols + c.col0 + c.cols] = t[r_]
        return full
    col0 = 0 if bug == "col0_ignored" else c.col0
    full[:, col0:col0 + c.cols] = t
    return full


def emu_pack_bf16(c, op16, ins, bug):
    v = ins["src"].clone()
    if ins["rowkeep"] is not None:
        v[ins["rowkeep"] == 0] = 0.0
    hi, lo = _emu_pack(v, op16, bug)
    return dict(hi=_embed_cols(c, hi, op16, bug), lo=_embed_cols(c, lo, op16, bug))


def chk_pack_bf16(c, op16, ins, got):
    want = emu_pack_bf16(c, op16, ins, None)
    return chk_exact("hi", got["hi"], want["hi"]) + chk_exact("lo", got["lo"], want["lo"])


def cases_im2col7():
    cs = [Case("im2col7", ch=ch, N=n, B=b, lo=lo) for ch in (1, 100, 128) for n in (1, 3, 4, 10) for b in (1, 3) for lo in (1, 0)]
    return cs + [Case("im2col7", ch=100, N=4, B=3, lo=1, outlier=1)]


def gen_im2col7(c, op16, r):
    x = _randn(r, c.B, c.N, c.ch)
    if c.kw.get("outlier"):
        x[1, 2, 5], x[2, 0, 0] = OUTLIER, -OUTLIER
    return dict(x=x), _pair_spec((c.B * c.N, 7 * 128), op16, c.lo, 7 * 128)


def emu_im2col7(c, op16, ins, bug):
    x = ins["x"]
    v = torch.zeros((c.B, c.N, 7, 128))
    if bug == "pad_not_zero":
        v[..., c.ch:] = 1.0
    for t in range(7):
        lo, hi = max(0, 3 - t), min(c.N, c.N + 3 - t)
        if hi > lo:
            v[:, lo:hi, t, :c.ch] = x[:, lo + t - 3:hi + t - 3]
    hi_, lo_ = _emu_pack(v.reshape(c.B * c.N, 7 * 128), op16, bug)
    return dict(hi=hi_, lo=lo_)


def chk_im2col7(c, op16, ins, got):
    want = emu_im2col7(c, op16, ins, None)
    return chk_exact("hi", got["hi"], want["hi"]) + chk_exact("lo", got["lo"], want["lo"])


def cases_pack_x():
    cs = [Case("pack_x", mel=m, rows=n, lo=lo) for m in (1, 100, 128) for n in (1, 77) for lo in (1, 0)]
    return cs + [Case("pack_x", mel=100, rows=77, lo=lo, outlier=1) for lo in (1, 0)]


def gen_pack_x(c, op16, r):
    y = _randn(r, c.rows, c.mel)
    if c.kw.get("outlier"):
        y[c.rows // 2, c.mel // 2], y[0, 0] = OUTLIER, -OUTLIER
    return dict(y=y), _pair_spec((c.rows, 128), op16, c.lo, 128)


def emu_pack_x(c, op16, ins, bug):
    v = torch.full((c.rows, 128), 1.0 if bug == "pad_not_zero" else 0.0)
    v[:, :c.mel] = ins["y"]
    hi, lo = _emu_pack(v, op16, bug)
    return dict(hi=hi, lo=lo, flag=_flag_of(v, op16))


def chk_pack_x(c, op16, ins, got):
    want = emu_pack_x(c, op16, ins, None)
    return chk_exact("hi", got["hi"], want["hi"]) + chk_exact("lo", got["lo"], want["lo"])


PCT_B, PCT_N = 3, 5


def cases_pack_cond_text():
    cs = [Case("pack_cond_text", mel=m, dt=d, nkc=k, lo=lo) for m in (1, 100, 128) for d in (4, 512) for k in (0, 1) for lo in (1, 0)]
    return cs + [Case("pack_cond_text", mel=100, dt=4, nkc=1, lo=lo, outlier=1) for lo in (1, 0)]


def gen_pack_cond_text(c, op16, r):
    cond, te = _randn(r, PCT_B, PCT_N, c.mel), _randn(r, 2, PCT_B, PCT_N, c.dt)
    lens = torch.tensor([0, 1, PCT_N], dtype=torch.int32)          # nothing, one frame, everything kept
    if c.kw.get("outlier"):
        cond[2, 1, c.mel // 2], te[1, 0, 3, 1] = OUTLIER, -OUTLIER
    return dict(cond=cond, lens=lens, text_emb=te), _pair_spec((2, PCT_B, PCT_N, 128 + c.dt), op16, c.lo, 128 + c.dt)


def emu_pack_cond_text(c, op16, ins, bug):
    cond, lens, te = ins["cond"], ins["lens"].to(torch.int64), ins["text_emb"]
    n = torch.arange(PCT_N)
    inside = (n[None] <= lens[:, None]) if bug == "cond_mask_le" else (n[None] < lens[:, None])        # [B][N]
    v = torch.zeros((2, PCT_B, PCT_N, 128 + c.dt))
    v[..., 128:] = te
    masked = torch.where(inside[..., None], cond, torch.zeros_like(cond))
    v[0, ..., :c.mel] = masked
    if c.nkc and bug != "null_keeps_cond_ignored":
        v[1, ..., :c.mel] = masked
    hi, lo = _emu_pack(v, op16, bug)
    return dict(hi=hi, lo=lo, flag=_flag_of(v, op16))


def chk_pack_cond_text(c, op16, ins, got):
    want = emu_pack_cond_text(c, op16, ins, None)
    return chk_exact("hi", got["hi"], want["hi"]) + chk_exact("lo", got["lo"], want["lo"])


# ---- ODE stage -----------------------------------------------------------------------------------------------------------------
ODE_DT = 0.0506


def cases_ode_stage():
    cs = [Case("ode_stage", mode=mo, null=nu, cfgptr=cp, kstore=ks, hi=h, lo=l, rows=n, mel=m)
          for mo in (0, 1) for nu in (1, 0) for cp in (0, 1) for ks in (0, 1) for h in (1, 0) for l in (1, 0) for n in (1, 77) for m in (100, 128)]
    return cs + [Case("ode_stage", mode=mo, null=1, cfgptr=0, kstore=1, hi=1, lo=l, rows=77, mel=100, outlier=1) for mo in (0, 1) for l in (1, 0)]


def ode_scalars(c):
    """(cfg, coef, divisor): Euler / midpoint stages use coef * dt, the RK4 final dt / 6"""
    return 2.0, (1.0 if c.mode else 0.5), (6.0 if c.mode else 1.0)


def gen_ode_stage(c, op16, r):
    shape = (c.rows, c.mel)
    ins = dict(pred=_randn(r, *shape), null_pred=_randn(r, *shape) if c.null else None, base=_randn(r, *shape),
               dt=torch.tensor([ODE_DT]), cfg_dev=torch.tensor([ode_scalars(c)[0]]) if c.cfgptr else None)
    for k in ("k1", "k2", "k3"):
        ins[k] = _randn(r, *shape) if c.mode else None
    if c.kw.get("outlier"):
        ins["base"][c.rows // 2, 3], ins["base"][0, 0] = OUTLIER, -OUTLIER
    spec = dict(out=dict(shape=shape, dtype=torch.float32, guard=c.mel), kstore=dict(shape=shape, dtype=torch.float32, guard=c.mel) if c.kstore else None)
    pair = _pair_spec((c.rows, 128), op16, c.lo, 128)
    spec["xin_hi"], spec["xin_lo"] = (pair["hi"] if c.hi else None), pair["lo"]
    return ins, spec


def emu_ode_stage(c, op16, ins, bug):
    cfg, coef, div = ode_scalars(c)
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    pr = ins["pred"]
    k = pr
    if c.null:
        d = pr - ins["null_pred"]
        k = pr + (-d if bug == "cfg_wrong_sign" else d) * f(cfg)
    a = (f(coef) * ins["dt"][0]) / f(div)
    upd = k
    if c.mode:
        w = 1.0 if bug == "rk4_weights_1111" else 2.0
        upd = ((ins["k1"] + w * ins["k2"]) + w * ins["k3"]) + k
    o = ins["base"] + a * upd
    res = dict(out=o, kstore=k.clone())
    if c.hi:                    # without xin_hi the kernel writes neither half
        v = torch.zeros((c.rows, 128))
        v[:, :c.mel] = o
        res["xin_hi"], res["xin_lo"] = _emu_pack(v, op16, bug)
        res["flag"] = _flag_of(v, op16)
    return res


def chk_ode_stage(c, op16, ins, got):
    cfg, coef, div = ode_scalars(c)
    D = lambda t: t.double()
    pr, base = D(ins["pred"]), D(ins["base"])
    k, kmag, nk = pr, pr.abs(), 0
    if c.null:              # k = pr + (pr - null) * cfg: a subtraction, a product, an addition
        nu = D(ins["null_pred"])
        k, kmag, nk = pr + (pr - nu) * cfg, pr.abs() + (pr.abs() + nu.abs()) * abs(cfg), 3
    a = coef * float(np.float32(ODE_DT)) / div              # (coef * dt) / divisor: a product and a division
    upd, umag, nu_ = k, kmag, 0
    if c.mode:              # ((k1 + 2 k2) + 2 k3) + k: the doublings are exact, three additions
        upd = D(ins["k1"]) + 2 * D(ins["k2"]) + 2 * D(ins["k3"]) + k
        umag, nu_ = D(ins["k1"]).abs() + 2 * D(ins["k2"]).abs() + 2 * D(ins["k3"]).abs() + kmag, 3
    ref = base + a * upd    # base + a * upd: a product and an addition
    n = nk + 2 + nu_ + 2
    bad = chk_f32("kstore", got["kstore"], k, max(nk, 1) * U * kmag)
    bad += chk_f32("out", got["out"], ref, n * U * (base.abs() + abs(a) * umag))
    if c.hi:                # the packed value is the fp32 `out` the kernel stored: the pair is its split, bit for bit; pad columns are +0
        v = torch.zeros((c.rows, 128))
        v[:, :c.mel] = got["out"]
        bad += chk_split("xin", got["xin_hi"], got["xin_lo"], v, op16)
    elif got["xin_lo"] is not None:
        untouched = torch.empty((c.rows, 128), dtype=op_dtype(op16))
        bits(untouched).fill_(SENT16)
        bad += chk_exact("xin_lo (no xin_hi: nothing may be written)", got["xin_lo"], untouched)
    return bad


# ---- masks, splice, copies (exact) ---------------------------------------------------------------------------------------------
def _lens_sets(B, N):
    return [(0, 1, N)] if B == 3 else [(v,) for v in sorted({0, 1, N})]


def cases_splice():
    return [Case("splice", B=b, N=n, lens=l, mel=100) for b in (1, 3) for n in (1, 5, 300) for l in _lens_sets(b, n)]


def gen_splice(c, op16, r):
    shape = (c.B, c.N, c.mel)
    return (dict(cond=_randn(r, *shape), y=_randn(r, *shape), lens=torch.tensor(c.lens, dtype=torch.int32)),
            dict(out=dict(shape=shape, dtype=torch.float32, guard=c.mel)))


def emu_splice(c, op16, ins, bug):
    lens = ins["lens"].to(torch.int64)
    if bug == "lens_of_wrong_batch":
        lens = lens.roll(1)
    inside = torch.arange(c.N)[None] < lens[:, None]
    return dict(out=torch.where(inside[..., None], ins["cond"], ins["y"]))


def chk_splice(c, op16, ins, got):
    return chk_exact("out", got["out"], emu_splice(c, op16, ins, None)["out"])


def cases_rowkeep():
    return [Case("rowkeep", B=b, N=n, lens=l) for b in (1, 3) for n in (1, 5, 300) for l in _lens_sets(b, n)]


def gen_rowkeep(c, op16, r):
    return dict(dur=torch.tensor(c.lens, dtype=torch.int32)), dict(keep=dict(shape=(c.B, c.N), dtype=torch.uint8))


def emu_rowkeep(c, op16, ins, bug):
    dur = ins["dur"].to(torch.int64)
    if bug == "lens_of_wrong_batch":
        dur = dur.roll(1)
    return dict(keep=(torch.arange(c.N)[None] < dur[:, None]).to(torch.uint8))


def chk_rowkeep(c, op16, ins, got):
    return chk_exact("keep", got["keep"], emu_rowkeep(c, op16, ins, None)["keep"])


COPY_BIG = 4 * 256 * 4096 + 7        # one word group per thread of the 4096-block cap, and a tail: the grid-stride loop takes a second trip


def cases_copy_words():
    return [Case("copy_words", nwords=n, src_off=s, dst_off=d) for n in (1, 3, 4, 5, 1023, COPY_BIG) for s, d in ((0, 0), (1, 0), (0, 1), (1, 1))]


def gen_copy_words(c, op16, r):
    src = torch.from_numpy(r.integers(-2 ** 31, 2 ** 31, c.nwords + c.src_off, dtype=np.int64).astype(np.int32))
    return dict(src=src), dict(dst=dict(shape=(c.nwords,), dtype=torch.int32, offset=c.dst_off))


def emu_copy_words(c, op16, ins, bug):
    want = ins["src"][c.src_off:].clone()
    if bug == "copy_loses_tail":
        bits(want)[(c.nwords // 4) * 4:] = SENT32
    return dict(dst=want)


def chk_copy_words(c, op16, ins, got):
    return chk_exact("dst", got["dst"], ins["src"][c.src_off:])


def cases_stage_words():
    return [Case("stage_words", nwords=n) for n in (1, 959, 960, 961, 2000)]


def gen_stage_words(c, op16, r):
    return dict(words=r.integers(0, 2 ** 32, c.nwords, dtype=np.uint64).astype(np.uint32)), dict(dst=dict(shape=(c.nwords,), dtype=torch.int32))


def emu_stage_words(c, op16, ins, bug):
    want = torch.from_numpy(ins["words"].view(np.int32).copy())
    if bug == "copy_loses_tail":
        bits(want)[(c.nwords // 960) * 960:] = SENT32
    return dict(dst=want)


def chk_stage_words(c, op16, ins, got):
    return chk_exact("dst", got["dst"], torch.from_numpy(ins["words"].view(np.int32).copy()))


def cases_zero_vt_pad():
    return [Case("zero_vt_pad", seq=s, npad=p, rows=n) for s, p in ((1, 64), (63, 64), (64, 64), (65, 128)) for n in (1, 48)]


def gen_zero_vt_pad(c, op16, r):
    vt = to_op(_randn(r, c.rows, c.npad), op16)
    return dict(vt0=vt), dict(vt=dict(shape=(c.rows, c.npad), dtype=op_dtype(op16), guard=c.npad, init=vt))


def emu_zero_vt_pad(c, op16, ins, bug):
    vt = ins["vt0"].clone()
    vt[:, c.seq + (1 if bug == "pad_off_by_one" else 0):] = 0.0
    return dict(vt=vt)


def chk_zero_vt_pad(c, op16, ins, got):
    return chk_exact("vt", got["vt"], emu_zero_vt_pad(c, op16, ins, None)["vt"])


# ---- fp32 helpers of the time / position path ----------------------------------------------------------------------------------
SK_M = (1, 32, 33, 70, 128, 129, 257)          # 70: the only row count of the list that ends on three accumulator blocks


def skinny_mblks(M):
    """the MBLK instantiations a launch of M rows runs (128 rows per pass over W)"""
    return [cdiv(min(128, M - m0), 32) for m0 in range(0, M, 128)]


def cases_skinny_gemm():
    return [Case("skinny_gemm", M=m, N=n, K=k, silu_in=si, silu_out=so, bias=b)
            for m in SK_M for n in (1, 31, 32, 33, 129) for k in (8, 16, 264) for si in (0, 1) for so in (0, 1) for b in (1, 0)]


def gen_skinny_gemm(c, op16, r):
    return (dict(a=_randn(r, c.M, c.K), w=_randn(r, c.N, c.K, scale=c.K ** -0.5), bias=_randn(r, c.N, scale=0.1) if c.bias else None),
            dict(out=dict(shape=(c.M, c.N), dtype=torch.float32, guard=c.N)))


def _skinny(c, a, w, bias, bug=None):
    silu = torch.nn.functional.silu
    if bug == "skinny_drops_bias":
        bias = None
    if bug == "skinny_k_tail":                 # a K loop in steps of 16 that drops the last 8
        a, w = a[:, :(c.K // 16) * 16], w[:, :(c.K // 16) * 16]
    if bug == "skinny_row_clamp":              # three accumulator blocks where four are needed: rows 96 ... 127 of a pass repeat row 95
        m = torch.arange(c.M)
        a = a[torch.where(m % 128 >= 96, m - m % 128 + 95, m)]
    y = (silu(a) if c.silu_in else a) @ w.T
    if bias is not None:
        y = y + bias
    return silu(y) if c.silu_out else y


def emu_skinny_gemm(c, op16, ins, bug):
    return dict(out=_skinny(c, ins["a"], ins["w"], ins["bias"], bug))


def chk_skinny_gemm(c, op16, ins, got):
    ref = _skinny(c, ins["a"].double(), ins["w"].double(), None if ins["bias"] is None else ins["bias"].double())
    return chk_f32("out", got["out"], ref, _ln_bound(1e-5, ref))


TIMES = (0.0, 0.0012834, 0.3, 0.5, 0.77, 0.94935, 1.0)


def cases_time_sinus():
    return [Case("time_sinus", dim=d) for d in (4, 254, 256, 1024)]


def gen_time_sinus(c, op16, r):
    return dict(t=torch.tensor(TIMES)), dict(out=dict(shape=(len(TIMES), c.dim), dtype=torch.float32, guard=c.dim))


def _time_sinus(c, t):
    half = c.dim // 2
    e = torch.exp(torch.arange(half, dtype=t.dtype) * -(math.log(10000.0) / (half - 1)))
    arg = (1000 * t[:, None]) * e[None]
    return torch.cat([arg.sin(), arg.cos()], -1)


def emu_time_sinus(c, op16, ins, bug):
    out = _time_sinus(c, ins["t"])
    if bug == "halves_swapped":                # [cos | sin] instead of [sin | cos]
        out = torch.cat([out[:, c.dim // 2:], out[:, :c.dim // 2]], -1)
    return dict(out=out)


def chk_time_sinus(c, op16, ins, got):
    return chk_f32("out", got["out"], _time_sinus(c, ins["t"].double()), 2e-4)      # argument up to 1000 rad in fp32


ROPE_DH = 64
QSCALES = (1.0, ROPE_DH ** -0.5 * math.log2(math.e))


def _angles64(n_pos, dim):
    """(angle [n_pos][dim / 2], 2 j / dim) in fp64"""
    x = torch.arange(0, dim, 2, dtype=torch.float64) / dim
    return torch.arange(n_pos, dtype=torch.float64)[:, None] * (10000.0 ** -x)[None], x


def _angle_bound(n_pos, dim, ulp_fn):
    """|cosf / sinf(a_fp32) - cos / sin(a)|: the argument rounding, position * 2^-23, plus the allowance of the function itself on a
    result of magnitude <= 1"""
    pos = torch.arange(n_pos, dtype=torch.float64)[:, None]
    return (pos * 2.0 ** -23 + ulp_fn * U).expand(n_pos, dim // 2)


def _angles32(n_pos, dim):
    inv = 1.0 / torch.pow(torch.tensor(10000.0), torch.arange(0, dim, 2, dtype=torch.float32) / dim)
    return torch.arange(n_pos, dtype=torch.float32)[:, None] * inv[None]


def g4_permute(cos_t, sin_t):
    """[seq][dh / 2] tables -> group-major [dh / 4][seq][4] = (cos_2g, cos_2g+1, sin_2g, sin_2g+1)"""
    seq, half = cos_t.shape
    c, s = cos_t.reshape(seq, half // 2, 2), sin_t.reshape(seq, half // 2, 2)
    return torch.cat([c, s], -1).permute(1, 0, 2).contiguous()


def cases_rope_tables():
    return [Case("rope_tables", seq=s, qscale=q) for s in (1, 63, 64, 65, 300) for q in QSCALES]


def gen_rope_tables(c, op16, r):
    half = ROPE_DH // 2
    t = dict(shape=(c.seq, half), dtype=torch.float32, guard=half)
    g = dict(shape=(ROPE_DH // 4, c.seq, 4), dtype=torch.float32)
    return dict(), dict(cos=dict(t), sin=dict(t), tq=dict(g), tk=dict(g))


def emu_rope_tables(c, op16, ins, bug):
    a = _angles32(c.seq, ROPE_DH)
    cos_t, sin_t = a.cos(), a.sin()
    tk = g4_permute(cos_t, sin_t)
    if bug == "g4_interleaved":                # (cos_2g, sin_2g, cos_2g+1, sin_2g+1) instead of the two cosines first
        tk = tk[..., [0, 2, 1, 3]].contiguous()
    tq = tk if bug == "q_table_unscaled" else tk * torch.tensor(c.qscale, dtype=torch.float32)
    return dict(cos=cos_t, sin=sin_t, tk=tk, tq=tq)


def chk_rope_tables(c, op16, ins, got):
    a, _ = _angles64(c.seq, ROPE_DH)
    bad = chk_f32("cos", got["cos"], a.cos(), _angle_bound(c.seq, ROPE_DH, ULP_COS))
    bad += chk_f32("sin", got["sin"], a.sin(), _angle_bound(c.seq, ROPE_DH, ULP_SIN))
    # the group-major twins: the same fp32 expression, so the k table is the permuted plain table bit for bit and the q table its fp32
    # product with qscale (at qscale 1 the k table itself)
    tk = g4_permute(got["cos"], got["sin"])
    bad += chk_exact("tk", got["tk"], tk)
    bad += chk_exact("tq", got["tq"], tk * torch.tensor(c.qscale, dtype=torch.float32))
    return bad


def cases_text_pos_table():
    return [Case("text_pos_table", max_pos=s, dim=d) for s in (1, 63, 64, 65, 300) for d in (128, 516)] + [Case("text_pos_table", max_pos=4096, dim=128)]


def gen_text_pos_table(c, op16, r):
    return dict(), dict(table=dict(shape=(c.max_pos, c.dim), dtype=torch.float32, guard=c.dim))


def emu_text_pos_table(c, op16, ins, bug):
    a = _angles32(c.max_pos, c.dim)
    return dict(table=torch.cat([a.sin(), a.cos()] if bug == "halves_swapped" else [a.cos(), a.sin()], -1))


def chk_text_pos_table(c, op16, ins, got):
    a, _ = _angles64(c.max_pos, c.dim)
    ref = torch.cat([a.cos(), a.sin()], -1)
    bound = torch.cat([_angle_bound(c.max_pos, c.dim, ULP_COS), _angle_bound(c.max_pos, c.dim, ULP_SIN)], -1)
    return chk_f32("table", got["table"], ref, bound.clamp_max(4e-4))      # and the project's 4e-4 at 4096 positions stays a cap


# ---- duration head -------------------------------------------------------------------------------------------------------------
DUR_EPS = 1e-5


def cases_duration_head():
    return [Case("duration_head", dim=d, N=n, B=b, mask=m) for d in (64, 100, 512) for n in (1, 3, 4, 5, 90) for b in (1, 3)
            for m in ("full", "ragged", "zero")]


def gen_duration_head(c, op16, r):
    x, g, w = _randn(r, c.B, c.N, c.dim), 1 + _randn(r, c.dim, scale=0.1), _randn(r, c.dim, scale=c.dim ** -0.5)
    mask = torch.ones((c.B, c.N), dtype=torch.uint8)
    if c.mask == "zero":
        mask.zero_()
    elif c.mask == "ragged":
        for b in range(c.B):
            mask[b, max(0, c.N - 1 - 2 * b) // (b + 1):] = 0
        mask[0, 0] = 1
    return dict(x=x, g=g, w=w, mask=mask), dict(out=dict(shape=(c.B,), dtype=torch.float32))


def _duration_head(c, x, g, w, mask, bug=None):
    rstd = 1.0 / torch.sqrt((x * x).mean(-1) + DUR_EPS)                 # [B][N]
    dot = (x * g * w).sum(-1)
    m = mask.to(x.dtype)
    cnt = m.sum(-1).clamp_min(1.0)
    if bug == "mean_over_all_rows":
        cnt = torch.full_like(cnt, c.N)
    mean = (dot * rstd * m).sum(-1) / cnt
    return torch.nn.functional.softplus(mean, threshold=20.0), rstd


def emu_duration_head(c, op16, ins, bug):
    return dict(out=_duration_head(c, ins["x"], ins["g"], ins["w"], ins["mask"], bug)[0])


def chk_duration_head(c, op16, ins, got):
    x, g, w, mask = ins["x"].double(), ins["g"].double(), ins["w"].double(), ins["mask"]
    ref, rstd = _duration_head(c, x, g, w, mask)
    # roundings in front of the softplus, relative to the ABSOLUTE sum A = sum_n mask rstd sum_d |x g w| / count:
    #   dot: two products per term, L = ceil(dim / 64) additions per lane, 6 levels of the wave tree        -> L + 8
    #   rstd: the sum of squares (one product, L + 6 additions), / dim, + eps, rsqrtf; a square root halves
    #         the relative error of its argument                                                             -> (L + 9) / 2 + 2 ULP_RSQRT
    #   dot * rstd, ceil(N / 4) additions per wave, 3 across the waves, the division by the count            -> ceil(N / 4) + 5
    L = cdiv(c.dim, 64)
    n = (L + 8) + (L + 9) / 2 + 2 * ULP_RSQRT + cdiv(c.N, 4) + 5
    m = mask.double()
    A = ((x * g * w).abs().sum(-1) * rstd * m).sum(-1) / m.sum(-1).clamp_min(1.0)
    # softplus is 1-Lipschitz; log1pf(expf(mean)): a relative error d of expf moves log1p(y) by y d / (1 + y) <= log1p(y) d
    bound = n * U * A + (ULP_EXP + ULP_LOG1P) * 2 * U * ref.abs()
    return chk_f32("out", got["out"], ref, bound)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _op(name, tracked=False, exact=False, packs=False):
    g = globals()
    return dict(cases=g["cases_" + name], gen=g["gen_" + name], emu=g["emu_" + name], chk=g["chk_" + name], tracked=tracked, exact=exact,
                packs=packs)


OPS = {
    "ln_modulate": _op("ln_modulate", tracked=True, packs=True),
    "layernorm": _op("layernorm", packs=True),
    "dwconv_ln": _op("dwconv_ln", tracked=True, packs=True),
    "grn": _op("grn", tracked=True, packs=True),
    "text_embed": _op("text_embed", exact=True),
    "pack_bf16": _op("pack_bf16", exact=True, packs=True),
    "im2col7": _op("im2col7", exact=True, packs=True),
    "pack_x": _op("pack_x", tracked=True, exact=True, packs=True),
    "pack_cond_text": _op("pack_cond_text", tracked=True, exact=True, packs=True),
    "ode_stage": _op("ode_stage", tracked=True, packs=True),
    "splice": _op("splice", exact=True),
    "rowkeep": _op("rowkeep", exact=True),
    "copy_words": _op("copy_words", exact=True),
    "stage_words": _op("stage_words", exact=True),
    "zero_vt_pad": _op("zero_vt_pad", exact=True),
    "skinny_gemm": _op("skinny_gemm"),
    "time_sinus": _op("time_sinus"),
    "rope_tables": _op("rope_tables"),
    "text_pos_table": _op("text_pos_table"),
    "duration_head": _op("duration_head"),
}
PACKS_WITH_LO = tuple(op for op in OPS if OPS[op]["packs"])
# text_embed covers f5_op_text_embed (mask = 1) and f5_op_text_embed_nomask (mask = 0); rope_tables covers f5_op_rope_table and
# f5_op_rope_table_g4


def cases(op=None):
    if op is not None:
        return OPS[op]["cases"]()
    return [c for o in OPS for c in OPS[o]["cases"]()]


def instantiations(c):
    """the template instantiations of csrc/rowops.hip a case launches, from its shape alone"""
    if c.op == "ln_modulate":
        return [f"ln_modulate_kernel<{c.dim // 256},{'true' if c.mean else 'false'}>"]
    if c.op in ("layernorm", "dwconv_ln"):
        return [f"{c.op}_kernel<{c.dim // 256}>"]
    if c.op == "skinny_gemm":
        return [f"skinny_gemm_mfma_kernel<{m}>" for m in skinny_mblks(c.M)]
    return []


CLAIMED = ([f"ln_modulate_kernel<{nv},{m}>" for nv in (1, 2, 3, 4) for m in ("true", "false")]
           + [f"{k}_kernel<{nv}>" for k in ("layernorm", "dwconv_ln") for nv in (1, 2, 3, 4)]
           + [f"skinny_gemm_mfma_kernel<{m}>" for m in (1, 2, 3, 4)])


def instantiation_counts(cs=None):
    counts = {k: 0 for k in CLAIMED}
    for c in (cases() if cs is None else cs):
        for k in instantiations(c):
            counts[k] = counts.get(k, 0) + 1
    return counts
