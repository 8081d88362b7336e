"""The kernels behind the DiT geometries outside the 335M family (docs/geometries.md), op by op through the C ABI:

  * conv-pos with 48 channels per group (f5_convpos_kernel<., ., 48>) against the fp64 reference and the derived bounds of
    tests/convaudio_matrix.py (chk_convpos's bounds, restated for a group width of 48 because the matrix's own generator and reference
    are written for 64), outputs between guard bands, inputs followed by NaN;
  * dwconv_ln / dwconv_ln_ragged at the widths that are no multiple of 256, through tests/rowops_matrix.py's generator and checker;
  * the GEMM shapes of the narrow configuration through tests/gemm_matrix.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import convaudio_matrix as CM
import convpos_ring_cases as RC
import gemm_matrix as GM
import rowops_matrix as RM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu

CPG, GROUPS, CH = 48, 16, 768


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def last_convpos_kernel(lib):
    buf = C.create_string_buffer(64)
    lib.f5_debug_last_convpos_kernel(buf, 64)
    return buf.value.decode()


# ---- conv-pos, 48 channels per group ------------------------------------------------------------------------------------------------
def _pack48(lib, w):
    """(C, taps, 48) fp32 -> the weight store's [C / 48 * 64][taps][64]"""
    Cc, taps, _ = w.shape
    out = np.zeros((lib.f5_op_conv_packed_rows(Cc, CPG), taps, 64), np.float32)
    wn = np.ascontiguousarray(w.numpy())
    assert lib.f5_op_pack_conv_groups(wn.ctypes.data_as(C.c_void_p), Cc, taps, CPG, out.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(out)


def _conv48(x, w, B, N, taps, lens=None):
    """out[b][n][co] = sum_{tap, ci} x[b][n + tap - pad][group(co) * 48 + ci] * w[co][tap][ci], zero outside [0, len_b): convaudio_matrix._conv
    for groups of 48, in the precision of x and w"""
    pad = taps // 2
    x = x.reshape(B, N, CH).clone()
    if lens is not None:
        for b, ln in enumerate(lens):
            x[b, ln:] = 0
    xp = torch.zeros((B, N + taps - 1, CH), dtype=x.dtype)
    xp[:, pad:pad + N] = x
    win = xp.unfold(1, taps, 1)                                             # [B][N][C][taps]
    out = torch.empty((B * N, CH), dtype=x.dtype)
    for g in range(GROUPS):
        a = win[:, :, g * CPG:(g + 1) * CPG].permute(0, 1, 3, 2).reshape(B * N, taps * CPG)
        out[:, g * CPG:(g + 1) * CPG] = a @ w[g * CPG:(g + 1) * CPG].reshape(CPG, taps * CPG).T
    return out


_DATA = {}


def _data(lib, B, N, taps, op16):
    """inputs, packed operands and the fp64 references of a shape, made once and shared by the cases that differ in nseg / mode alone"""
    key = (B, N, taps, op16)
    if key not in _DATA:
        if len(_DATA) >= 4:
            _DATA.clear()
        r = np.random.default_rng(1000 * N + 10 * taps + B + (7 if op16 == "f16" else 0))
        x = CM._randn(r, B, N, CH)
        w = CM._randn(r, CH, taps, CPG, scale=(taps * CPG) ** -0.5)
        bias = CM._randn(r, CH, scale=0.1)
        old = CM._randn(r, B * N, CH)
        x_hi, x_lo = CM.split(x.reshape(B * N, CH), op16)
        wp = _pack48(lib, w)
        w_hi, w_lo = CM.split(wp.reshape(-1, taps * 64), op16)
        # the operand the kernel multiplies, back in the tensor's own layout, for the one-pass reference
        w_hi_t = w_hi.float().reshape(GROUPS, 64, taps, 64)[:, :CPG, :, :CPG].reshape(CH, taps, CPG)
        ref = {}
        for nseg in (1, 3):
            xs, ws = (x.double(), w.double()) if nseg == 3 else (x_hi.double().reshape(B, N, CH), w_hi_t.double())
            pre = _conv48(xs, ws, B, N, taps) + bias.double()
            ref[nseg] = (pre, CM._mish(pre))
        _DATA[key] = dict(x=x, w=w, bias=bias, old=old, x_hi=x_hi, x_lo=x_lo, w_hi=w_hi, w_lo=w_lo, w_hi_t=w_hi_t, ref=ref)
    return _DATA[key]


def _bounds(pre, ref, B, N, nseg, mode, out=None):
    """tests/convaudio_matrix.py chk_convpos: the GEMM bound on the per-element output scale plus the Mish term"""
    a = ref.abs().reshape(B, N, CH)
    scale = a.amax(dim=(1, 2), keepdim=True).clamp_min(1.0).expand(-1, N, CH).reshape(B * N, CH)
    pm = torch.where(pre > 0, pre.clamp(max=30.0), pre.abs())
    mish = (4 * pm + 4 * CM.ULP_EXP2 + 2 * CM.ULP_RCP + 7) * CM.U * ref.abs() + 1e-25 * ref.abs()
    if mode == 1:
        return (2e-4 if nseg == 1 else 5e-5) * scale + mish + CM.U * out.double().abs().nan_to_num(0.0)
    return (2e-4 if nseg == 1 else 1e-4) * scale + mish


def _launch(lib, d, B, N, taps, nseg, mode, lo, op16, lens=None):
    """-> (outputs dict of RM.Out, flag); the caller holds the operand mode"""
    dev = {k: RM.pad_in(d[k], DEV) for k in ("x_hi", "x_lo", "w_hi", "w_lo", "bias")}
    g = 128 * CH
    hi = lo_ = out = None
    if mode == 0:
        hi = RM.Out((B * N, CH), CM.op_dtype(op16), DEV, guard=g)
        lo_ = RM.Out((B * N, CH), CM.op_dtype(op16), DEV, guard=g) if lo else None
    else:
        out = RM.Out((B * N, CH), torch.float32, DEV, guard=g, init=d["old"])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    E.check(lib.f5_debug_set_op_sat_flag(P(flag)))
    try:
        three = nseg == 3
        args = (P(dev["x_hi"]), P(dev["x_lo"] if three else None), P(dev["w_hi"]), P(dev["w_lo"] if three else None), P(dev["bias"]),
                P(hi.t if hi else None), P(lo_.t if lo_ else None), P(out.t if out else None), B, N, CH, GROUPS, taps, nseg, mode)
        if lens is None:
            rc = lib.f5_op_convpos(*args, stream())
        else:
            lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
            rc = lib.f5_op_convpos_ragged(*args, P(lens_dev), stream())
    finally:
        E.check(lib.f5_debug_set_op_sat_flag(None))
    torch.cuda.synchronize()
    assert rc == 0, lib.f5_last_error().decode()
    return dict(hi=hi, lo=lo_, out=out), int(flag.cpu()[0])


def _check(d, outs, flag, B, N, nseg, mode, op16):
    bad = []
    for name, o in outs.items():
        if o is not None:
            bad += o.guard_violations(name)
    if flag != 0:
        bad.append(f"range flag {flag}")
    pre, ref = d["ref"][nseg]
    if mode == 1:
        got = outs["out"].t.cpu()
        bad += CM.chk_f32("out - out_before", got.double() - d["old"].double(), ref, _bounds(pre, ref, B, N, nseg, 1, got))
    else:
        bad += CM.chk_pair("out", outs["hi"].t.cpu(), None if outs["lo"] is None else outs["lo"].t.cpu(), ref, _bounds(pre, ref, B, N, nseg, 0), op16)
    return bad


# (nseg, mode, lo): both operand passes and both output modes, the lo half with and without
VARIANTS = ((1, 0, 1), (1, 1, 0), (3, 0, 1), (3, 1, 0), (1, 0, 0))


@pytest.mark.parametrize("op16", CM.OPS16)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("taps", [31, 7])
def test_convpos_48_against_fp64(lib, taps, B, op16):
    failures = []
    with operand_mode(op16):
        for N in (1, 127, 128, 129, 300):
            d = _data(lib, B, N, taps, op16)
            for nseg, mode, lo in VARIANTS:
                outs, flag = _launch(lib, d, B, N, taps, nseg, mode, lo, op16)
                name = last_convpos_kernel(lib)
                want = f"f5_convpos_kernel<{'true' if nseg == 3 else 'false'},1,48>+xcd"
                bad = _check(d, outs, flag, B, N, nseg, mode, op16)
                if name != want:
                    bad.append(f"ran {name!r}, not {want!r}")
                failures += [f"N={N} nseg={nseg} mode={mode} lo={lo}: {b}" for b in bad]
    assert not failures, failures[:10]


@pytest.mark.parametrize("op16", CM.OPS16)
@pytest.mark.parametrize("tps", [2, 4])
def test_convpos_48_taps_per_step_give_the_same_bits(lib, tps, op16):
    """the taps per pipeline step do not change the order in which an element is accumulated (convaudio_matrix.convpos_group)"""
    B, N, taps = 2, 129, 31
    with operand_mode(op16):
        d = _data(lib, B, N, taps, op16)
        for nseg in (1, 3):
            first, _ = _launch(lib, d, B, N, taps, nseg, 0, 1, op16)
            E.check(lib.f5_debug_set_convpos_tps(tps))
            try:
                second, flag = _launch(lib, d, B, N, taps, nseg, 0, 1, op16)
                name = last_convpos_kernel(lib)
            finally:
                E.check(lib.f5_debug_set_convpos_tps(0))
            assert name == (f"f5_convpos_kernel<true,2,48>+xcd" if nseg == 3 else f"f5_convpos_kernel<false,{tps},48>+xcd")
            assert not _check(d, second, flag, B, N, nseg, 0, op16)
            for k in ("hi", "lo"):
                assert torch.equal(RM.bits(first[k].t), RM.bits(second[k].t)), (nseg, k)


@pytest.mark.parametrize("op16", CM.OPS16)
@pytest.mark.parametrize("nseg,mode", [(1, 0), (3, 1)])
def test_convpos_48_ragged_keeps_the_padding_out(lib, nseg, mode, op16):
    """lengths that leave one whole 128-token tile and one part of a tile in the padding, NaN behind every length: the valid rows are
    finite and within the bound of the conv of the row alone, the padding rows are never written"""
    B, N, taps = 2, 300, 31
    lens = [170, 300]                                          # element 0: rows 170..255 are part of tile 1, tile 2 lies in the padding whole
    with operand_mode(op16):
        d = dict(_data(lib, B, N, taps, op16))
        x = d["x"].clone()
        pre = _conv48((x.double() if nseg == 3 else d["x_hi"].double().reshape(B, N, CH)),
                      (d["w"].double() if nseg == 3 else d["w_hi_t"].double()), B, N, taps, lens=lens) + d["bias"].double()
        d["ref"] = {nseg: (pre, CM._mish(pre))}
        for k in ("x_hi", "x_lo"):
            t = d[k].clone().reshape(B, N, CH)
            t[0, lens[0]:] = float("nan")
            d[k] = t.reshape(B * N, CH)
        outs, flag = _launch(lib, d, B, N, taps, nseg, mode, 1, op16, lens=lens)
    assert last_convpos_kernel(lib) == f"f5_convpos_kernel<{'true' if nseg == 3 else 'false'},1,48>+xcd"
    valid = torch.zeros(B, N, dtype=torch.bool)
    for b, ln in enumerate(lens):
        valid[b, :ln] = True
    valid = valid.reshape(-1)
    bad = []
    for name, o in outs.items():
        if o is None:
            continue
        bad += o.guard_violations(name)
        got = o.t.cpu()
        assert torch.isfinite(got[valid].float()).all(), name
        if mode == 1:                                          # the padding rows keep `old`, bit for bit
            assert torch.equal(RM.bits(got[~valid]), RM.bits(d["old"][~valid])), name
        else:
            assert bool((RM.bits(got[~valid]) == RM.SENT16).all()), name
    pre, ref = d["ref"][nseg]
    if mode == 1:
        got = outs["out"].t.cpu()
        bad += CM.chk_f32("out - out_before", (got.double() - d["old"].double())[valid], ref[valid], _bounds(pre, ref, B, N, nseg, 1, got)[valid])
    else:
        bad += CM.chk_pair("out", outs["hi"].t.cpu()[valid], outs["lo"].t.cpu()[valid], ref[valid], _bounds(pre, ref, B, N, nseg, 0)[valid], op16)
    assert not bad and flag == 0, (bad[:5], flag)


def test_convpos_48_neighbouring_columns_belong_to_different_groups(lib):
    """columns g * 48 + 47 and g * 48 + 48 come from different groups' inputs and weights: with one group's input channels set to zero
    the first is bias alone and the second is not (a kernel that stored 64 columns per group would write group g's padding there)"""
    B, N, taps, g = 1, 129, 7, 5
    with operand_mode("bf16"):
        d = dict(_data(lib, B, N, taps, "bf16"))
        x = d["x"].clone()
        x[:, :, g * CPG:(g + 1) * CPG] = 0
        d["x_hi"], d["x_lo"] = CM.split(x.reshape(B * N, CH), "bf16")
        pre = _conv48(d["x_hi"].double().reshape(B, N, CH), d["w_hi_t"].double(), B, N, taps) + d["bias"].double()
        d["ref"] = {1: (pre, CM._mish(pre))}
        outs, flag = _launch(lib, d, B, N, taps, 1, 0, 0, "bf16")
        assert not _check(d, outs, flag, B, N, 1, 0, "bf16")
    got = outs["hi"].t.cpu().float()
    lone = CM._mish(d["bias"].double())
    for col in range(g * CPG, (g + 1) * CPG):
        assert float((got[:, col].double() - lone[col]).abs().max()) <= 2.0 ** -8 * abs(float(lone[col])) + 1e-6, col
    for col in (g * CPG - 1, (g + 1) * CPG):                      # the neighbours on either side carry their own group's conv
        assert float(got[:, col].double().std()) > 0.05, col


def test_kernel_choice_for_narrow_and_full_groups(lib):
    """48 and 32 channels per group never run the ring kernel; 64 channels run what they ran before, at the shapes and under the
    selectors tests/convpos_ring_cases.py fixes"""
    z = torch.zeros(4 << 20, dtype=torch.bfloat16, device=DEV)                 # operands of any of the shapes below, all zero
    o = torch.empty(4 << 20, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(1024, dtype=torch.float32, device=DEV)

    def ran(B, N, Cc, groups, nseg=1):
        lo = P(z) if nseg == 3 else P(None)
        E.check(lib.f5_op_convpos(P(z), lo, P(z), lo, P(b), P(o), P(None), P(None), B, N, Cc, groups, 31, nseg, 0, stream()))
        torch.cuda.synchronize()
        return last_convpos_kernel(lib)

    with operand_mode("bf16"):
        assert ran(2, 937, 768, 16) == "f5_convpos_kernel<false,1,48>+xcd"     # one round of 256 workgroups: the ring's shape, not its width
        assert ran(2, 937, 768, 16, 3) == "f5_convpos_kernel<true,1,48>+xcd"
        assert ran(2, 937, 1024, 32) == "f5_convpos_kernel<false,1>+xcd"       # 16 super groups of two 32-channel groups
        for (Cc, N, B, nseg, tps), name in RC.ROUTES:
            E.check(lib.f5_debug_set_convpos_tps(tps))
            try:
                assert ran(B, N, Cc, Cc // 64, nseg) == name == RC.kernel_name(Cc, N, B, nseg, tps), (Cc, N, B, nseg, tps)
            finally:
                E.check(lib.f5_debug_set_convpos_tps(0))
        E.check(lib.f5_debug_set_convpos_tps(RC.RING))                         # the ring selector does not reach narrow groups either
        try:
            assert ran(1, 300, 768, 16) == "f5_convpos_kernel<false,1,48>+xcd" and ran(1, 300, 1024, 32) == "f5_convpos_kernel<false,1>+xcd"
            assert ran(1, 300, 1024, 16) == "f5_convpos_ring_kernel+xcd"
        finally:
            E.check(lib.f5_debug_set_convpos_tps(0))


# ---- dwconv_ln at widths that are no multiple of 256 ----------------------------------------------------------------------------------
DW_WIDTHS = (128, 384, 640)


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("dim", DW_WIDTHS)
def test_dwconv_ln_on_the_128_column_granule(lib, dim, op16):
    """rows 1, 5 and 67 (one wave, two blocks with a part block, 17 blocks), through the matrix's generator, guards and checker"""
    failures = []
    with operand_mode(op16):
        for B, N in ((1, 1), (1, 5), (1, 67), (3, 37)):
            for lo in (1, 0):
                c = RM.Case("dwconv_ln", dim=dim, B=B, N=N, lo=lo)
                io = RM.build(c, op16, device=DEV)
                E.check(lib.f5_debug_set_op_sat_flag(P(io.flag)))
                try:
                    i, o = io.ins, io.outs
                    rc = lib.f5_op_dwconv_ln(P(i["x"]), P(i["dw_w"]), P(i["dw_b"]), P(i["ln_w"]), P(i["ln_b"]), P(o["hi"].t),
                                             P(o["lo"].t if o["lo"] else None), c.B, c.N, c.dim, stream())
                finally:
                    E.check(lib.f5_debug_set_op_sat_flag(None))
                torch.cuda.synchronize()
                assert rc == 0, lib.f5_last_error().decode()
                failures += RM.check(io)
    assert not failures, failures[:10]


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("dim", DW_WIDTHS)
def test_dwconv_ln_ragged_on_the_128_column_granule(lib, dim, op16):
    """lengths 0, 1 and full: a valid token gets the bits of f5_op_dwconv_ln on its row alone (checked against the matrix's reference
    through that launch), a token behind its length is zeros, NaN in the padding stays out"""
    B, N = 3, 67
    lens = [0, 1, N]
    r = np.random.default_rng(dim)
    x = RM._randn(r, B, N, dim)
    par = [RM._randn(r, dim, 7, scale=0.4), RM._randn(r, dim, scale=0.1), 1 + RM._randn(r, dim, scale=0.1), RM._randn(r, dim, scale=0.1)]
    xn = x.clone()
    for b, ln in enumerate(lens):
        xn[b, ln:] = float("nan")
    dt = RM.op_dtype(op16)
    with operand_mode(op16):
        dev = [t.to(DEV) for t in par]
        hi, lo = RM.Out((B * N, dim), dt, DEV, guard=4 * dim), RM.Out((B * N, dim), dt, DEV, guard=4 * dim)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
        E.check(lib.f5_op_dwconv_ln_ragged(P(xn.to(DEV)), P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(hi.t), P(lo.t), B, N, dim, P(lens_dev),
                                           stream()))
        torch.cuda.synchronize()
        assert not hi.guard_violations("hi") and not lo.guard_violations("lo")
        h, l = hi.t.view(B, N, dim), lo.t.view(B, N, dim)
        for b, ln in enumerate(lens):
            assert not RM.bits(h[b, ln:]).any() and not RM.bits(l[b, ln:]).any(), b
            if ln == 0:
                continue
            # the row alone through the unragged launch, itself checked against fp64 by the matrix's checker
            c = RM.Case("dwconv_ln", dim=dim, B=1, N=ln, lo=1)
            h1, l1 = torch.empty((ln, dim), dtype=dt, device=DEV), torch.empty((ln, dim), dtype=dt, device=DEV)
            xb = x[b:b + 1, :ln].contiguous().to(DEV)
            E.check(lib.f5_op_dwconv_ln(P(xb), P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(h1), P(l1), 1, ln, dim, stream()))
            torch.cuda.synchronize()
            assert torch.equal(RM.bits(h[b, :ln]), RM.bits(h1)) and torch.equal(RM.bits(l[b, :ln]), RM.bits(l1)), b
            ins = dict(x=x[b:b + 1, :ln], dw_w=par[0], dw_b=par[1], ln_w=par[2], ln_b=par[3])
            assert not RM.chk_dwconv_ln(c, op16, ins, dict(hi=h1.cpu(), lo=l1.cpu())), b


# ---- the GEMM shapes of the narrow configuration --------------------------------------------------------------------------------------
# (name, epilogue, N, K): dim 768, inner width 512, ff 1536, text 384 / 768, mel 100 padded to 128.  The fused QKV projection
# (EPI_QKV_ROPE, N = 1536, K = 768) is no epilogue of tests/gemm_matrix.py: test_qkv_rope_1536x768 below runs it through f5_op_qkv_rope_k with the
# bounds tests/test_ops_gpu.py applies to the square projection
NARROW_GEMMS = (("out_proj", "RESID_GATE", 768, 512), ("ff1", "GELU_TANH", 1536, 768), ("ff2", "RESID_GATE", 768, 1536),
                ("text_pw1", "GELU_ERF", 768, 384), ("text_pw2", "RESID_KEEP", 384, 768), ("hoisted_proj", "F32", 768, 512),
                ("input_proj", "ADDROWS", 768, 128), ("out_mel", "F32", 100, 768))


@pytest.mark.parametrize("op", GM.OPS)
@pytest.mark.parametrize("M", [1, 64, 257, 600])
def test_gemm_shapes_of_the_narrow_configuration(lib, op, M):
    buf = C.create_string_buffer(64)
    failures = []
    for nseg in (1, 3):
        for name, epi, N, K in NARROW_GEMMS:
            c = GM.make_case(op, 0, epi, nseg, M, N, K, note=name)
            with operand_mode(op):
                b = GM.make_buffers(c, device=DEV)
                lo = (lambda t: t) if nseg == 3 else (lambda t: None)
                a_hi, a_lo, w_hi, w_lo = b["a"][0], lo(b["a"][1]), b["w"][0], lo(b["w"][1])
                of, oh, ol = b["out_f32"].ptr_tensor(), b["out_hi"].ptr_tensor(), b["out_lo"].ptr_tensor()
                s = stream()
                if epi == "RESID_GATE":
                    rc = lib.f5_op_gemm_resid_gate(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(b["gate"]), P(b["keep"]), P(of), c.M, c.N,
                                                   c.K, c.lda, c.ldw, c.ldo, c.nseg, s)
                elif epi == "RESID_KEEP":
                    rc = lib.f5_op_gemm_resid_keep(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(b["resid"].ptr_tensor()), P(b["keep"]),
                                                   P(of), c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.nseg, s)
                elif epi == "ADDROWS":
                    rc = lib.f5_op_gemm_addrows(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["addrows"].ptr_tensor()), c.a_row_mod, P(of), P(oh),
                                                P(ol if nseg == 3 else None), c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.nseg, s)
                else:
                    rc = lib.f5_op_gemm(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(of), P(oh), P(ol if nseg == 3 else None), c.M, c.N,
                                        c.K, c.lda, c.ldw, c.ldo, c.nseg, GM.EPI[epi], s)
                torch.cuda.synchronize()
            if rc != 0:
                failures.append((name, nseg, "refused: " + lib.f5_last_error().decode()))
                continue
            lib.f5_debug_last_gemm_kernel(buf, 64)
            bad = GM.check(b)
            if buf.value.decode() != c.kernel:
                bad.append(f"ran {buf.value.decode()}, the dispatcher's source says {c.kernel}")
            if bad:
                failures.append((name, nseg, bad[:3]))
    assert not failures, failures[:8]


# ---- the fused QKV projection with an inner width that is not the model width ------------------------------------------------------------
@pytest.mark.parametrize("op", GM.OPS)
@pytest.mark.parametrize("M", [1, 64, 257, 600])
def test_qkv_rope_1536x768(lib, op, M):
    """N = 3 x 512, K = 768, 8 heads, one sequence of M tokens, straight and transposed q / k tiles: q, k and V^T against fp64 with the
    bounds tests/test_ops_gpu.py _attention_case applies to the square projection (5e-5 of the output scale with three operand passes,
    2e-2 x 2^-8 -- scaled to the operand type -- with one, plus N 2^-22 for the fp32 rotation angle)"""
    import test_ops_gpu as T
    from f5test import O, bf16r, join, op_dtype, randn, rng, split_bf16
    H, inner, K, N = 8, 512, 768, M
    npad = (N + 63) // 64 * 64
    r = rng(M)
    x, w, bias = randn(r, N, K), randn(r, 3 * inner, K, scale=K ** -0.5), randn(r, 3 * inner, scale=0.1)
    freqs = O.rotary_freqs(64, N).double()
    with operand_mode(op):
        x_hi, x_lo = split_bf16(x.to(DEV))
        w_hi, w_lo = split_bf16(w.to(DEV))
        cos_t, sin_t = torch.empty((N, 32), device=DEV), torch.empty((N, 32), device=DEV)
        E.check(lib.f5_op_rope_table(P(cos_t), P(sin_t), N, 64, stream()))
        tt = [torch.empty(64 * N, device=DEV) for _ in range(2)]
        E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), N, 64, C.c_float(1.0), stream()))
        bias_d = bias.to(DEV)
        for nseg in (1, 3):
            xx, ww = (x.double(), w.double()) if nseg == 3 else (bf16r(x).double(), bf16r(w).double())
            q, k, v = [t.reshape(1, N, H, 64).transpose(1, 2) for t in (xx @ ww.T + bias.double()).chunk(3, dim=-1)]
            q, k = O.apply_rotary_pos_emb(q, freqs), O.apply_rotary_pos_emb(k, freqs)
            for tr in (False, True):
                qk = [torch.zeros((N, 2 * inner), dtype=op_dtype(), device=DEV) for _ in range(2)]
                vt = [torch.zeros((H, 64, npad), dtype=op_dtype(), device=DEV) for _ in range(2)]
                E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0] if tr else None), P(tt[1] if tr else None)))
                try:
                    E.check(lib.f5_op_qkv_rope_k(P(x_hi), P(x_lo), P(w_hi), P(w_lo), P(bias_d), P(cos_t), P(sin_t), P(qk[0]), P(qk[1]), P(vt[0]),
                                                 P(vt[1]), 1, N, npad, H, inner, K, nseg, stream()), "qkv_rope_k")
                finally:
                    E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
                torch.cuda.synchronize()
                both = join(qk[0], qk[1] if nseg == 3 else None).cpu()
                got_q = both[:, :inner].reshape(1, N, H, 64).transpose(1, 2)
                got_k = both[:, inner:].reshape(1, N, H, 64).transpose(1, 2)
                got_v = join(vt[0], vt[1] if nseg == 3 else None).cpu().reshape(1, H, 64, npad)[..., :N].transpose(-1, -2)
                tol_in = 5e-5 if nseg == 3 else T.tol16(2e-2)
                for nm, g, rf in (("q", got_q, q), ("k", got_k, k), ("v", got_v, v)):
                    mx = float((g.double() - rf).abs().max())
                    rot = 0.0 if nm == "v" else 2.0 * N * 2.0 ** -23
                    assert mx <= (tol_in + rot) * max(1.0, float(rf.abs().max())), (nm, nseg, tr, mx)
                if npad > N:
                    assert float(join(vt[0], vt[1]).cpu()[..., N:].abs().max()) == 0.0
