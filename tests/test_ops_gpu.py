"""Per-kernel parity: HIP op (through the C ABI) vs the oracle / plain torch fp32 on the same inputs.

Tolerances: fp32 kernels 1e-5 relative; bf16 MFMA kernels are compared (a) against the SAME operands
rounded to bf16 with fp32 accumulation (kernel-bug detector, ~1e-3 of the output scale from summation
order only) and (b) in bf16x3 mode against full fp32 (<= 5e-5 of the output scale).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f5test import DEV, E, O, P, bf16r, join, op_dtype, randn, report, rng, split_bf16, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def sync():
    torch.cuda.synchronize()


def last_gemm_kernel(lib):
    """name of the kernel the most recent GEMM launch resolved to (f5_debug_last_gemm_kernel)"""
    buf = C.create_string_buffer(64)
    lib.f5_debug_last_gemm_kernel(buf, 64)
    return buf.value.decode()


# ---- tolerances of 16-bit results as functions of the operand type the test runs with (bf16, or fp16 under f5test.operand_mode) ----
def eps_op():
    """largest relative error of one round-to-nearest into the operand type: 2^-8 (bf16: 8 significand bits) or 2^-11 (fp16: 11)"""
    return 2.0 ** -8 if op_dtype() == torch.bfloat16 else 2.0 ** -11


F32_FLOOR = 2e-4       # the project's bound of an fp32 GEMM result against the same rounded operands, relative to the output scale


def tol16(bf16_tol, floor=F32_FLOOR):
    """A bound on a 16-bit result that was written for bf16 as `bf16_tol` (a multiple of 2^-8): exactly that value under bf16; under fp16
    the same multiple of 2^-11, plus the part that does not shrink with the operand type (fp32 accumulation: `floor`)."""
    if op_dtype() == torch.bfloat16:
        return bf16_tol
    return bf16_tol * (2.0 ** -11 / 2.0 ** -8) + floor


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
def _gemm(lib, a, w, bias, epi, nseg, N=None):
    M, K = a.shape
    N = N or w.shape[0]
    a_hi, a_lo = split_bf16(a.to(DEV))
    wpad = torch.zeros(((w.shape[0] + 127) // 128 * 128, K))
    wpad[: w.shape[0]] = w
    w_hi, w_lo = split_bf16(wpad.to(DEV))
    out_f = torch.full((M, N), float("nan"), device=DEV)
    out_hi = torch.zeros((M, N), dtype=op_dtype(), device=DEV)
    out_lo = torch.zeros((M, N), dtype=op_dtype(), device=DEV)
    b = bias.to(DEV) if bias is not None else None
    E.check(lib.f5_op_gemm(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b), P(out_f), P(out_hi), P(out_lo), M, N, K, K, K, N, nseg, epi,
                           stream()), "f5_op_gemm")
    sync()
    return out_f.cpu(), out_hi.cpu(), out_lo.cpu()


@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (300, 256, 128), (937, 100, 256), (1874, 1024, 1024), (129, 384, 2048)])
def test_gemm_f32_out(lib, M, N, K):
    r = rng(M + N + K)
    a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
    ref32 = a.double() @ w.double().T + bias.double()
    refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
    out, _, _ = _gemm(lib, a, w, bias, 0, 1)
    mx, mean, ref = report(f"gemm bf16 {M}x{N}x{K} vs bf16-rounded operands", out, refbf)
    assert mx <= 2e-4 * max(1.0, float(refbf.abs().max()))
    out3, _, _ = _gemm(lib, a, w, bias, 0, 3)
    mx, mean, ref = report(f"gemm bf16x3 {M}x{N}x{K} vs fp64", out3, ref32)
    assert mx <= 5e-5 * max(1.0, float(ref32.abs().max()))


def test_gemm_asymmetric_identity(lib):
    """A = I with an asymmetric W detects a transposed / permuted C write (CDNA guide rule 16)."""
    K = 128
    a = torch.eye(K)
    w = torch.arange(256 * K, dtype=torch.float32).reshape(256, K) % 251
    out, _, _ = _gemm(lib, a, w, None, 0, 1)
    assert torch.equal(out, w.T.contiguous()[:K]), "C tile layout is wrong"


@pytest.mark.parametrize("epi", [1, 2, 3])
def test_gemm_epilogues(lib, epi):
    r = rng(epi)
    M, N, K = 257, 384, 256
    a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
    pre = a.double() @ w.double().T + bias.double()
    if epi == 1:
        ref = pre
    elif epi == 2:
        ref = F.gelu(pre, approximate="tanh")
    else:
        ref = F.gelu(pre)
    out_f, out_hi, out_lo = _gemm(lib, a, w, bias, epi, 3)
    got = out_f if epi == 3 else join(out_hi, out_lo)
    mx, _, _ = report(f"gemm epilogue {epi} (bf16x3)", got, ref)
    assert mx <= 1e-4
    if epi != 3:  # hi part alone is the bf16 rounding of the value
        mxh, _, _ = report(f"gemm epilogue {epi} hi-part", out_hi.float(), ref)
        assert mxh <= eps_op() * float(ref.abs().max()) + 1e-4


# ------------------------------------------------------------------------------------------------
# QKV + RoPE + attention
# ------------------------------------------------------------------------------------------------
QPRE = 0.125 * 1.4426950408889634     # softmax scale * log2(e): what the engine folds into q (F5GemmArgs::q_premul)


def _attention_case(lib, B, H, N, kv_len, nseg, seed=0, premul=False, tr_tables=False):
    """premul: the op-level twin of the engine's default -- q leaves the QKV epilogue multiplied by scale * log2(e) and the
    attention kernels take their scores in exp2 units (single-segment operands only)."""
    if premul:
        assert nseg == 1
        E.check(lib.f5_debug_set_op_q_premul(C.c_float(QPRE)))
    try:
        _attention_case_body(lib, B, H, N, kv_len, nseg, seed, premul, tr_tables)
    finally:
        E.check(lib.f5_debug_set_op_q_premul(C.c_float(0.0)))


def _attention_case_body(lib, B, H, N, kv_len, nseg, seed, premul, tr_tables=False):
    D = H * 64
    r = rng(seed)
    x = randn(r, B * N, D)
    w = randn(r, 3 * D, D, scale=D ** -0.5)
    bias = randn(r, 3 * D, scale=0.1)
    npad = (N + 63) // 64 * 64
    x_hi, x_lo = split_bf16(x.to(DEV))
    w_hi, w_lo = split_bf16(w.to(DEV))
    cos_t = torch.empty((N, 32), device=DEV)
    sin_t = torch.empty((N, 32), device=DEV)
    E.check(lib.f5_op_rope_table(P(cos_t), P(sin_t), N, 64, stream()))
    qk = [torch.zeros((B * N, 2 * D), dtype=op_dtype(), device=DEV) for _ in range(2)]
    vt = [torch.zeros((B * H, 64, npad), dtype=op_dtype(), device=DEV) for _ in range(2)]
    bias_d = bias.to(DEV)
    tt = None
    if tr_tables:
        # group-major rotation tables [16][N][4] = (cos, cos, sin, sin) of two neighbouring pairs (the q table carrying the q factor):
        # the staged kernels then accumulate the q / k tiles transposed, as sample() does; the k table holds the token-major values
        tt = [torch.empty(64 * N, device=DEV) for _ in range(2)]
        E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), N, 64, C.c_float(QPRE if premul else 1.0), stream()))
        g4 = tt[1].view(16, N, 4)
        assert torch.equal(g4[:, :, 0:2].permute(1, 0, 2).reshape(N, 32), cos_t) and torch.equal(g4[:, :, 2:4].permute(1, 0, 2).reshape(N, 32), sin_t)
        E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0]), P(tt[1])))
    try:
        E.check(lib.f5_op_qkv_rope(P(x_hi), P(x_lo), P(w_hi), P(w_lo), P(bias_d), P(cos_t), P(sin_t), P(qk[0]), P(qk[1]),
                                   P(vt[0]), P(vt[1]), B, N, npad, H, D, nseg, stream()), "qkv_rope")
        sync()
        if tr_tables:       # the straight tiles must give the same 16-bit values (same expressions; report if contraction differs)
            qk2 = [torch.zeros_like(qk[0]) for _ in range(2)]
            vt2 = [torch.zeros_like(vt[0]) for _ in range(2)]
            E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
            E.check(lib.f5_op_qkv_rope(P(x_hi), P(x_lo), P(w_hi), P(w_lo), P(bias_d), P(cos_t), P(sin_t), P(qk2[0]), P(qk2[1]),
                                       P(vt2[0]), P(vt2[1]), B, N, npad, H, D, nseg, stream()), "qkv_rope")
            sync()
            dq = float((qk[0].float() - qk2[0].float()).abs().max())
            print(f"[qkv transposed vs straight tiles] B{B} H{H} N{N} nseg={nseg} premul={premul}: max |dq| = {dq:.3e}, "
                  f"identical = {torch.equal(qk[0], qk2[0])}")
            assert dq <= eps_op() * float(qk2[0].float().abs().max()) and torch.equal(vt[0], vt2[0])
    finally:
        E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
    out = [torch.zeros((B * N, D), dtype=op_dtype(), device=DEV) for _ in range(2)]
    kv = torch.tensor(kv_len, dtype=torch.int32, device=DEV) if kv_len is not None else None
    E.check(lib.f5_op_attention(P(qk[0]), P(qk[1]), P(vt[0]), P(vt[1]), P(out[0]), P(out[1]), P(kv), B, H, N, npad, D,
                                C.c_float(0.125), int(nseg == 3), stream()), "attention")
    sync()
    # --- reference (oracle functions) in fp64
    xx = x.double() if nseg == 3 else bf16r(x).double()
    ww = w.double() if nseg == 3 else bf16r(w).double()
    qkv = xx @ ww.T + bias.double()
    q, k, v = [t.reshape(B, N, H, 64).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
    freqs = O.rotary_freqs(64, N).double()
    q, k = O.apply_rotary_pos_emb(q, freqs), O.apply_rotary_pos_emb(k, freqs)
    # rope table parity
    report("rope cos table", cos_t.cpu(), freqs.cos()[:, 0::2])
    assert float((cos_t.cpu().double() - freqs.cos()[:, 0::2]).abs().max()) < 1e-5 * max(1, N / 100)
    # q/k/v written by the epilogue
    got_q = join(qk[0], qk[1] if nseg == 3 else None).cpu()[:, :D].reshape(B, N, H, 64).transpose(1, 2)
    if premul:
        got_q = got_q / QPRE
    got_k = join(qk[0], qk[1] if nseg == 3 else None).cpu()[:, D:].reshape(B, N, H, 64).transpose(1, 2)
    got_v = join(vt[0], vt[1] if nseg == 3 else None).cpu().reshape(B, H, 64, npad)[..., :N].transpose(-1, -2)
    tol_in = 5e-5 if nseg == 3 else tol16(2e-2)
    for nm, g, rf in (("q", got_q, q), ("k", got_k, k), ("v", got_v, v)):
        mx, _, _ = report(f"qkv_rope {nm} nseg={nseg} B{B} H{H} N{N}", g, rf)
        # rotary angle = position * inv_freq in fp32: a 1-ulp difference in inv_freq (device powf vs torch pow) is
        # amplified by the position, hence the N * 2^-23 term for q and k
        rot = 0.0 if nm == "v" else 2.0 * N * 2.0 ** -23
        assert mx <= (tol_in + rot) * max(1.0, float(rf.abs().max())), nm
    assert float(join(vt[0], vt[1]).cpu().reshape(B, H, 64, npad)[..., N:].abs().max() if npad > N else 0.0) == 0.0
    # attention proper, from the operands the kernel actually saw
    qq, kk, vv = got_q.double(), got_k.double(), got_v.double()
    s = (qq @ kk.transpose(-1, -2)) * 0.125
    if kv_len is not None:
        keep = torch.arange(N)[None, :] < torch.tensor(kv_len)[:, None]
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(B * N, D)
    got = join(out[0], out[1] if nseg == 3 else None).cpu()
    mx, mean, _ = report(f"attention nseg={nseg} B{B} H{H} N{N} kv={kv_len}", got, ref)
    tol = 5e-5 if nseg == 3 else tol16(1.5e-2)
    assert mx <= tol * max(1.0, float(ref.abs().max()))
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 499, 937])
@pytest.mark.parametrize("nseg", [1, 3])
def test_attention_shapes(lib, N, nseg):
    _attention_case(lib, 1, 2, N, None, nseg, seed=N)


@pytest.mark.parametrize("nseg", [1, 3])
def test_attention_ragged_mask(lib, nseg):
    _attention_case(lib, 3, 2, 200, [200, 130, 1], nseg, seed=7)


def test_attention_softmax_spike(lib, hp=1, premul=False, N=300, spikes=((70, 30.0), (200, 60.0))):
    """force large running-max jumps across KV tiles (online-softmax rescale path)."""
    B, H, D = 1, 2, 128
    r = rng(3)
    q = randn(r, B * N, D)
    k = randn(r, B * N, D)
    for pos, factor in spikes:
        k[pos] *= factor
    v = randn(r, B * N, D)
    npad = (N + 63) // 64 * 64
    if premul:
        E.check(lib.f5_debug_set_op_q_premul(C.c_float(QPRE)))
        q_dev = bf16r(q) * QPRE          # what the QKV epilogue would have written (exact here: the test rounds q first)
        qk = torch.cat([q_dev, k], dim=1)
    else:
        qk = torch.cat([q, k], dim=1)
    qk_hi, qk_lo = split_bf16(qk.to(DEV))
    vt_full = torch.zeros((B * H, 64, npad))
    vt_full[..., :N] = v.reshape(N, H, 64).permute(1, 2, 0)
    vt_hi, vt_lo = split_bf16(vt_full.to(DEV))
    out = [torch.zeros((B * N, D), dtype=op_dtype(), device=DEV) for _ in range(2)]
    lo = (lambda t: t) if hp else (lambda t: None)
    try:
        E.check(lib.f5_op_attention(P(qk_hi), P(lo(qk_lo)), P(vt_hi), P(lo(vt_lo)), P(out[0]), P(lo(out[1])), P(None), B, H, N, npad, D,
                                    C.c_float(0.125), hp, stream()))
        sync()
    finally:
        E.check(lib.f5_debug_set_op_q_premul(C.c_float(0.0)))
    rr = (lambda t: t) if hp else bf16r                      # one-pass kernels: the reference sees the rounded operands
    qq = (bf16r(bf16r(q) * QPRE) / QPRE if premul else rr(q)).double().reshape(N, H, 64).transpose(0, 1)
    kk = rr(k).double().reshape(N, H, 64).transpose(0, 1)
    vv = rr(v).double().reshape(N, H, 64).transpose(0, 1)
    ref = (torch.softmax(qq @ kk.transpose(-1, -2) * 0.125, dim=-1) @ vv).transpose(0, 1).reshape(N, D)
    got = join(out[0], out[1] if hp else None).cpu()
    mx, mean, _ = report(f"attention spike hp={hp}", got, ref)
    assert torch.isfinite(got).all()
    # logits reach |s| ~ 500 here; split-bf16 products carry ~2^-17 relative error, i.e. ~4e-3 absolute on such a logit,
    # which moves near-tied softmax weights by a few 1e-3.  The test is about the rescale path: no NaN, tiny mean error.
    if hp:
        assert mean <= 2e-5 and mx <= 5e-3 * max(1.0, float(ref.abs().max()))
    else:                                                    # P and the output are rounded to the 16-bit operand type
        assert mean <= tol16(3e-3) and mx <= tol16(3e-2) * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------
# conv position embedding
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,taps", [(1, 50, 128, 31), (2, 130, 256, 31), (1, 937, 1024, 31), (2, 200, 128, 5)])
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("tps", [0, 1, 2, 4])
def test_convpos(lib, B, N, C, taps, nseg, tps):
    """tps: weight slabs (taps) per pipeline step of the kernel -- 0 = the launcher's choice, 1 / 2 / 4 forced (31 and 5 taps are
    not multiples of 2 or 4: the last step is partial).  With nseg == 3 the launcher maps a selector of 2 or 4 to
    f5_convpos_kernel<true,2> (there is no <true,4>): the tps=4, nseg=3 items run the same kernel as tps=2;
    tests/test_convaudio_matrix_gpu.py asserts the mapping through f5_debug_last_convpos_kernel."""
    E.check(lib.f5_debug_set_convpos_tps(tps))
    try:
        _convpos_case(lib, B, N, C, taps, nseg)
    finally:
        E.check(lib.f5_debug_set_convpos_tps(0))


def _convpos_case(lib, B, N, C, taps, nseg):
    r = rng(N + C)
    G = C // 64
    x = randn(r, B, N, C)
    w = randn(r, C, taps, 64, scale=(taps * 64) ** -0.5)     # reference layout (out, k, in/groups)
    bias = randn(r, C, scale=0.1)
    x_hi, x_lo = split_bf16(x.reshape(B * N, C).to(DEV))
    w_hi, w_lo = split_bf16(w.reshape(C, taps * 64).to(DEV))
    out = [torch.zeros((B * N, C), dtype=op_dtype(), device=DEV) for _ in range(2)]
    acc = randn(r, B * N, C).to(DEV)
    acc0 = acc.clone()
    bias_d = bias.to(DEV)
    E.check(lib.f5_op_convpos(P(x_hi), P(x_lo), P(w_hi), P(w_lo), P(bias_d), P(out[0]), P(out[1]), P(None), B, N, C, G,
                              taps, nseg, 0, stream()), "convpos mode0")
    E.check(lib.f5_op_convpos(P(x_hi), P(x_lo), P(w_hi), P(w_lo), P(bias_d), P(None), P(None), P(acc), B, N, C, G, taps,
                              nseg, 1, stream()), "convpos mode1")
    sync()
    xx = x.double() if nseg == 3 else bf16r(x).double()
    ww = w.double() if nseg == 3 else bf16r(w).double()
    y = F.conv1d(xx.transpose(1, 2), ww.permute(0, 2, 1), bias.double(), padding=taps // 2, groups=G).transpose(1, 2)
    ref = (y * torch.tanh(F.softplus(y))).reshape(B * N, C)
    got = join(out[0], out[1] if nseg == 3 else None).cpu()
    mx, _, _ = report(f"convpos nseg={nseg} B{B} N{N} C{C}", got, ref)
    tol = 5e-5 if nseg == 3 else tol16(1e-2)
    assert mx <= tol * max(1.0, float(ref.abs().max()))
    mx2, _, _ = report("convpos accumulate mode", (acc - acc0).cpu(), ref)
    assert mx2 <= (5e-5 if nseg == 3 else 2e-3) * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------
# row kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(1, 256), (5, 512), (937, 1024)])
def test_ln_modulate(lib, rows, dim):
    r = rng(rows)
    x, sc, sh = randn(r, rows, dim) * 3 + 0.5, randn(r, dim, scale=0.5), randn(r, dim, scale=0.5)
    hi = torch.zeros((rows, dim), dtype=op_dtype(), device=DEV)
    lo = torch.zeros_like(hi)
    xd, scd, shd = x.to(DEV), sc.to(DEV), sh.to(DEV)      # keep the device copies alive across the call
    E.check(lib.f5_op_ln_modulate(P(xd), P(scd), P(shd), P(hi), P(lo), rows, dim, stream()))
    sync()
    ref = O.DiTOracle.layer_norm(x.double()) * (1 + sc.double()) + sh.double()
    mx, _, _ = report(f"ln_modulate {rows}x{dim}", join(hi, lo).cpu(), ref)
    assert mx <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((hi.float().cpu() - ref).abs().max()) <= eps_op() * float(ref.abs().max()) + 1e-5


@pytest.mark.parametrize("B,N,dim", [(1, 5, 256), (2, 100, 512)])
def test_dwconv_ln(lib, B, N, dim):
    r = rng(N)
    x = randn(r, B, N, dim)
    dw_w, dw_b = randn(r, dim, 7, 1, scale=0.4), randn(r, dim, scale=0.1)
    ln_w, ln_b = 1 + randn(r, dim, scale=0.1), randn(r, dim, scale=0.1)
    hi = torch.zeros((B * N, dim), dtype=op_dtype(), device=DEV)
    lo = torch.zeros_like(hi)
    dev = [t.to(DEV) for t in (x, dw_w.reshape(dim, 7).contiguous(), dw_b, ln_w, ln_b)]
    E.check(lib.f5_op_dwconv_ln(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), P(hi), P(lo), B, N, dim, stream()))
    sync()
    y = F.conv1d(x.double().transpose(1, 2), dw_w.double().permute(0, 2, 1), dw_b.double(), padding=3, groups=dim).transpose(1, 2)
    ref = O.DiTOracle.layer_norm(y, ln_w.double(), ln_b.double()).reshape(B * N, dim)
    mx, _, _ = report(f"dwconv_ln B{B} N{N} d{dim}", join(hi, lo).cpu(), ref)
    assert mx <= 3e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("B,N,dim", [(1, 31, 256), (3, 100, 1024)])
def test_grn(lib, B, N, dim):
    r = rng(dim)
    g, gamma, beta = randn(r, B, N, dim), randn(r, dim, scale=0.1), randn(r, dim, scale=0.1)
    scratch = torch.zeros(lib.f5_op_grn_scratch_floats(B, N, dim), device=DEV)
    hi = torch.zeros((B * N, dim), dtype=op_dtype(), device=DEV)
    lo = torch.zeros_like(hi)
    dev = [t.to(DEV) for t in (g, gamma, beta)]
    E.check(lib.f5_op_grn(P(dev[0]), P(dev[1]), P(dev[2]), P(scratch), P(hi), P(lo), B, N, dim, stream()))
    sync()
    gd = g.double()
    gx = torch.linalg.vector_norm(gd, ord=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    ref = (gamma.double() * (gd * nx) + beta.double() + gd).reshape(B * N, dim)
    mx, _, _ = report(f"grn B{B} N{N} d{dim}", join(hi, lo).cpu(), ref)
    assert mx <= 2e-5 * max(1.0, float(ref.abs().max()))


def test_text_embed_bit_exact_index_path(lib):
    r = rng(11)
    B, N, nt, dim, V = 3, 40, 12, 128, 50
    text = torch.from_numpy(r.integers(0, V, (B, nt)).astype(np.int32))
    text[1, 9:] = -1
    text[2, 0:] = -1
    text[0, 3] = 0                                   # a real token with id 0 (-> 1 after the +1 shift)
    table = randn(r, V + 1, dim)
    pos = torch.empty((4096, dim), device=DEV)
    E.check(lib.f5_op_text_pos_table(P(pos), 4096, dim, stream()))
    out = torch.zeros((2, B, N, dim), device=DEV)
    ids = torch.full((2, B, N), -7, dtype=torch.int32, device=DEV)
    keep = torch.full((2, B, N), 9, dtype=torch.uint8, device=DEV)
    text_d, table_d = text.to(DEV), table.to(DEV)
    E.check(lib.f5_op_text_embed(P(text_d), nt, P(table_d), P(pos), 4096, P(out), P(ids), P(keep), B, N, dim, stream()))
    sync()
    ref_pos = O.precompute_freqs_cis(dim, 4096)
    mxp, _, _ = report("text pos table", pos.cpu(), ref_pos)
    assert mxp <= 4e-4                                # fp32 angle up to 4095 rad: sin/cos argument rounding
    cfg = type("C", (), dict(text_dim=dim, text_max_pos=4096, conv_layers=0))()
    orc = O.DiTOracle.__new__(O.DiTOracle)
    orc.cfg, orc.dtype, orc.emu = cfg, torch.float32, False
    orc.w = {"transformer.text_embed.text_embed.weight": table}
    for br, drop in ((0, False), (1, True)):
        emb, ref_ids = orc.text_embed(text, N, drop)
        assert torch.equal(ids[br].cpu().to(torch.int64), ref_ids), "token index path must be bit exact"
        shifted = torch.nn.functional.pad(text.to(torch.int64) + 1, (0, N - nt))
        assert torch.equal(keep[br].cpu().bool(), shifted != 0)
        want = (emb + ref_pos[:N][None]) * (shifted != 0)[..., None]
        got = out[br].cpu()
        # same table on both sides: use the device table for an exact comparison
        want_dev = (table[ref_ids] + pos.cpu()[:N][None]) * (shifted != 0)[..., None]
        assert torch.equal(got, want_dev)
        assert float((got - want).abs().max()) <= 4e-4


def test_time_tables(lib):
    r = rng(5)
    n, F_, D = 7, 256, 512
    t = torch.tensor([0.0, 0.0012834, 0.3, 0.5, 0.77, 0.94935, 1.0])
    sin_out = torch.empty((n, F_), device=DEV)
    t_d = t.to(DEV)
    E.check(lib.f5_op_time_sinus(P(t_d), P(sin_out), n, F_, stream()))
    half = F_ // 2
    emb = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))
    arg = (1000 * t[:, None]) * emb[None, :]
    ref = torch.cat([arg.double().sin(), arg.double().cos()], dim=-1)
    sync()
    mx, _, _ = report("time sinus", sin_out.cpu(), ref)
    assert mx <= 2e-4                                   # argument up to 1000 rad in fp32
    a, w, b = randn(r, n, F_), randn(r, D, F_, scale=F_ ** -0.5), randn(r, D, scale=0.1)
    out = torch.empty((n, D), device=DEV)
    a_d, w_d, b_d = a.to(DEV), w.to(DEV), b.to(DEV)
    for si, so in ((0, 0), (1, 0), (0, 1)):
        E.check(lib.f5_op_skinny_gemm(P(a_d), P(w_d), P(b_d), P(out), n, D, F_, si, so, stream()))
        sync()
        aa = F.silu(a.double()) if si else a.double()
        ref = aa @ w.double().T + b.double()
        ref = F.silu(ref) if so else ref
        mx, _, _ = report(f"skinny gemm silu_in={si} silu_out={so}", out.cpu(), ref)
        assert mx <= 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("M,N,K", [(1, 96, 64), (33, 70, 256), (124, 1000, 1024), (200, 257, 128)])
def test_skinny_gemm_shapes(lib, M, N, K):
    """fp32 MFMA skinny GEMM at ragged row/column counts (row chunks of 128, partial 32-column groups)."""
    r = rng(77)
    a, w, b = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
    a_d, w_d, b_d = a.to(DEV), w.to(DEV), b.to(DEV)
    out = torch.full((M, N), float("nan"), device=DEV)
    E.check(lib.f5_op_skinny_gemm(P(a_d), P(w_d), P(b_d), P(out), M, N, K, 1, 0, stream()))
    sync()
    ref = F.silu(a.double()) @ w.double().T + b.double()
    mx, _, _ = report(f"skinny gemm {M}x{N}x{K}", out.cpu(), ref)
    assert mx <= 1e-5 * max(1.0, float(ref.abs().max()))


def test_cfg_axpy(lib):
    r = rng(9)
    rows, mel = 77, 100
    pred, null, base = randn(r, rows, mel), randn(r, rows, mel), randn(r, rows, mel)
    dt = torch.tensor([0.0506], device=DEV)
    out = torch.empty((rows, mel), device=DEV)
    xin = [torch.full((rows, 128), 5.0, dtype=op_dtype(), device=DEV) for _ in range(2)]
    pred_d, null_d, base_d = pred.to(DEV), null.to(DEV), base.to(DEV)
    E.check(lib.f5_op_cfg_axpy(P(pred_d), P(null_d), C.c_float(2.0), P(base_d), P(dt), C.c_float(0.5), C.c_float(1.0), P(out),
                               P(xin[0]), P(xin[1]), rows, mel, stream()))
    sync()
    k = pred + (pred - null) * 2.0
    ref = base + (np.float32(0.5) * np.float32(0.0506)) * k
    assert float((out.cpu() - ref).abs().max()) <= 1e-6
    assert float(join(xin[0], xin[1]).cpu()[:, :mel].sub(out.cpu()).abs().max()) <= 2.0 ** -16 * float(out.abs().max())
    assert float(xin[0].float().cpu()[:, mel:].abs().max()) == 0.0


def test_mel_fixture(lib):
    """log-mel of the reference's WAV fixture vs the oracle (and its Appendix-C known-answer stats)."""
    import scipy.io.wavfile as wf
    from f5_tts_mlx_amd.audio import log_mel_spectrogram
    from f5_tts_mlx_amd.engine import library_path
    sr, a = wf.read(str(library_path().parent.parent / "assets" / "test_en_1_ref_short.wav"))
    audio = (a.astype(np.float64) / 32768.0).astype(np.float32)
    got = log_mel_spectrogram(torch.from_numpy(audio)).cpu()
    ref = torch.from_numpy(O.log_mel_spectrogram(audio, dtype=np.float64))
    assert got.shape == (1, 499, 100)
    mx, mean, _ = report("mel fixture", got, ref)
    assert mean <= 1e-5 and mx <= 2e-3
    assert abs(float(got.mean()) - (-1.26651)) < 1e-4 and abs(float(got.max()) - 4.46371) < 1e-4


# ------------------------------------------------------------------------------------------------
# 256x256 global_load_lds GEMM (v2) forced through the debug hook
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def force_v2(lib):
    E.check(lib.f5_debug_set_gemm_tile(4))
    yield
    E.check(lib.f5_debug_set_gemm_tile(0))


def test_gemm_v2_band_major_tile_numbering(lib, force_v2):
    """the 256x256 kernel numbers its tiles in bands of 4 column tiles when N has more than 4 of them (QKV: 12, FF1: 8); the
    numbering must not change a bit of the result (ragged M, 2 and 3 bands, also a band width that does not divide tiles_n)"""
    for (M, N, K) in ((700, 2048, 128), (1100, 3072, 64), (300, 1536, 192)):
        r = rng(M + N + K)
        a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
        outs = []
        for nband in (0, 4, 2, 5):
            E.check(lib.f5_debug_set_gemm_nband(nband))
            try:
                outs.append(_gemm(lib, a, w, bias, 0, 1)[0])
            finally:
                E.check(lib.f5_debug_set_gemm_nband(4))
        refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
        mx, _, _ = report(f"gemm256 band-major {M}x{N}x{K}", outs[1], refbf)
        assert mx <= 2e-4 * max(1.0, float(refbf.abs().max()))
        for o in outs[1:]:
            assert torch.equal(o, outs[0])


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 512, 128), (1000, 256, 192), (1874, 1024, 1024), (700, 768, 2048)])
def test_gemm_v2_f32_out(lib, force_v2, M, N, K):
    r = rng(M + N + K + 1)
    a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
    refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
    out, _, _ = _gemm(lib, a, w, bias, 0, 1)
    mx, _, _ = report(f"gemm256 bf16 {M}x{N}x{K} vs bf16-rounded operands", out, refbf)
    assert mx <= 2e-4 * max(1.0, float(refbf.abs().max()))
    ref32 = a.double() @ w.double().T + bias.double()
    out3, _, _ = _gemm(lib, a, w, bias, 0, 3)
    mx, _, _ = report(f"gemm256 bf16x3 {M}x{N}x{K} vs fp64", out3, ref32)
    assert mx <= 5e-5 * max(1.0, float(ref32.abs().max()))


def test_gemm_v2_identity_and_repeat(lib, force_v2):
    K = 256
    a = torch.eye(K)[:256]
    w = (torch.arange(512 * K, dtype=torch.float32).reshape(512, K) % 251) - 100
    for _ in range(3):   # repeated launches: the LDS ring / counted waits must not leave stale state
        out, _, _ = _gemm(lib, a, w, None, 0, 1)
        assert torch.equal(out, w.T.contiguous()[:256]), "v2 C tile layout / staging is wrong"


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("epi", [1, 2, 8])
def test_gemm_v2_16bit_epilogues_transposed_tile(lib, force_v2, epi, nseg):
    """16-bit row-major outputs of the 256x256 kernel (plain, GELU-tanh = FF1, GELU-erf): the tile is accumulated transposed
    (MFMA operands swapped) and staged with one 8-byte LDS write per 4 features.  Must match the fp64 reference on asymmetric
    data (a transposed or permuted tile cannot pass) and equal, bit for bit, the straight-order path (gemm flag 16384), with
    ragged M, bias, one- and three-segment operands."""
    for (M, N, K) in ((700, 512, 256), (1000, 768, 128), (256, 256, 64)):
        r = rng(M + N + K + epi)
        a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.3)
        pre = (a.double() if nseg == 3 else bf16r(a).double()) @ (w.double() if nseg == 3 else bf16r(w).double()).T + bias.double()
        ref = pre if epi == 1 else (F.gelu(pre, approximate="tanh") if epi == 2 else F.gelu(pre))
        outs = {}
        for flags in (0, 16384):
            E.check(lib.f5_debug_set_gemm_flags(flags))
            try:
                _, hi, lo = _gemm(lib, a, w, bias, epi, nseg)
            finally:
                E.check(lib.f5_debug_set_gemm_flags(0))
            outs[flags] = (hi.clone(), lo.clone() if lo is not None else None)
        got = join(outs[0][0], outs[0][1] if nseg == 3 else None)
        mx, _, _ = report(f"gemm256 16-bit epilogue {epi} nseg={nseg} {M}x{N}x{K}", got, ref)
        # one rounding of a value that is right to fp32 accuracy; the part that does not scale with the operand type is 1e-3 as it
        # always was under bf16, the fp32 bound of the GEMM under fp16
        fixed = 1e-3 if op_dtype() == torch.bfloat16 else F32_FLOOR * max(1.0, float(ref.abs().max()))
        assert mx <= (1e-4 if nseg == 3 else eps_op() * float(ref.abs().max()) + fixed)
        assert torch.equal(outs[0][0].view(torch.int16), outs[16384][0].view(torch.int16)), "transposed and straight tiles differ"
        if nseg == 3:
            assert torch.equal(outs[0][1].view(torch.int16), outs[16384][1].view(torch.int16))


@pytest.mark.parametrize("nseg", [1, 3])
def test_qkv_transposed_tiles_256_kernel(lib, force_v2, nseg):
    """QKV projection on the 256x256 kernel with the q / k column tiles accumulated transposed (rotation pairs in-lane,
    pair-major tables, 8-byte staging writes) and the V tiles straight: element-wise against the fp64 projection + rotation,
    against the straight-tile kernel, and through the attention that consumes it; one- and three-segment operands, q plain or
    carrying scale * log2(e), ragged batches whose rows straddle 32-token blocks, dmodel 256 and 1024."""
    for premul in ((False, True) if nseg == 1 else (False,)):
        _attention_case(lib, 2, 4, 300, [300, 211], nseg, seed=21, premul=premul, tr_tables=True)
        _attention_case(lib, 3, 4, 203, [203, 130, 1], nseg, seed=22, premul=premul, tr_tables=True)
    _attention_case(lib, 1, 16, 937, None, nseg, seed=24, premul=nseg == 1, tr_tables=True)


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("tile", [9, 12, 13, "knob12", "knob13"])
def test_qkv_transposed_wave_tiles_ring8(lib, tile, nseg):
    """the same on the 8-wave ring kernels (128x128 and 128x256 block tiles, 32x64 / 64x64 / 32x128 wave tiles): forced by the
    tile override, and chosen by the QKV-only knob at the batch-1 shape (M = 1874: one round of 128x256 tiles)"""
    knob = isinstance(tile, str)
    if knob:
        E.check(lib.f5_debug_set_gemm_qkv_tile(int(tile[-2:])))
    else:
        E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for premul in ((False, True) if nseg == 1 else (False,)):
            _attention_case(lib, 2, 4, 300, [300, 211], nseg, seed=31, premul=premul, tr_tables=True)
            _attention_case(lib, 3, 4, 203, [203, 130, 1], nseg, seed=32, premul=premul, tr_tables=True)
        _attention_case(lib, 2, 16, 937, [937, 800], nseg, seed=34, premul=nseg == 1, tr_tables=True)
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))
        E.check(lib.f5_debug_set_gemm_qkv_tile(0))


@pytest.mark.parametrize("tile", [4, 12, 13, 14])
def test_transposed_qkv_tiles_race_screen(lib, tile):
    """Round 2 saw a transposed-tile QKV epilogue WITHOUT LDS staging return a few hundred wrong elements on lanes 48-63, differently
    on every launch, on 4-wave kernels only (cause not found; that experiment never shipped and is not in the product library).  The
    SHIPPED transposed tiles (staged through LDS, 8-wave kernels: the 256x256 kernel and the 128x256 ring tiles) are screened here the
    way a race shows: 40 launches per shape -- row tails, ragged batches, batch-1 and multi-round grids -- each compared bit for bit
    with the straight-tile epilogue (gemm flag 16384) of the same kernel."""
    import ctypes as C
    D, H = 1024, 16
    r = rng(99 + tile)
    w = randn(r, 3 * D, D, scale=D ** -0.5)
    bias = randn(r, 3 * D, scale=0.1).to(DEV)
    w_hi, _ = split_bf16(w.to(DEV))
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for B, n in ((2, 937), (1, 2100), (3, 431), (5, 1000)):
            M = B * n
            npad = (n + 63) // 64 * 64
            a_hi, _ = split_bf16(randn(r, M, D).to(DEV))
            cos_t, sin_t = torch.empty(n, 32, device=DEV), torch.empty(n, 32, device=DEV)
            E.check(lib.f5_op_rope_table(P(cos_t), P(sin_t), n, 64, stream()))          # token-major (straight tiles) ...
            tt = [torch.empty(64 * n, device=DEV) for _ in range(2)]
            E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), n, 64, C.c_float(1.0), stream()))   # ... and pair-major twins

            def run(flags):
                E.check(lib.f5_debug_set_gemm_flags(flags))
                E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0]), P(tt[1])))
                qk = torch.zeros(M, 2 * D, dtype=op_dtype(), device=DEV)
                vt = torch.zeros(B * H, 64, npad, dtype=op_dtype(), device=DEV)
                E.check(lib.f5_op_qkv_rope(P(a_hi), P(None), P(w_hi), P(None), P(bias), P(cos_t), P(sin_t), P(qk), P(None), P(vt), P(None),
                                           B, n, npad, H, D, 1, stream()), "qkv_rope")
                sync()
                return qk, vt
            try:
                ref_qk, ref_vt = run(16384)                                # straight tiles
                assert float(ref_qk.float().abs().mean()) > 0.1
                for i in range(40):
                    qk, vt = run(0)                                         # transposed q / k tiles
                    assert torch.equal(qk, ref_qk) and torch.equal(vt, ref_vt), (tile, B, n, i, int((qk != ref_qk).sum()))
            finally:
                E.check(lib.f5_debug_set_gemm_flags(0))
                E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("nseg", [1, 3])
def test_attention_path_with_v2_qkv(lib, force_v2, nseg):
    _attention_case(lib, 2, 4, 300, [300, 211], nseg, seed=21)     # D = 256: QKV GEMM runs on the 256x256 kernel


def test_attention_wide_workgroups(lib, mode=1):
    """256-query workgroups, two query blocks per wave (the large-grid bf16 kernel), forced on small problems: ragged key
    lengths, sequence tails inside the second query block, one-tile sequences"""
    E.check(lib.f5_debug_set_attn_wide(mode))
    E.check(lib.f5_debug_set_attn_kvsplit(1))
    try:
        _attention_case(lib, 1, 2, 50, None, 1, seed=1)
        _attention_case(lib, 2, 2, 333, [333, 100], 1, seed=5)
        _attention_case(lib, 3, 2, 200, [200, 130, 1], 1, seed=7)
        _attention_case(lib, 1, 2, 937, None, 1, seed=8)
        _attention_case(lib, 2, 4, 300, [300, 211], 1, seed=21)
    finally:
        E.check(lib.f5_debug_set_attn_wide(-1))
        E.check(lib.f5_debug_set_attn_kvsplit(-1))


@pytest.mark.parametrize("premul", [False, True])
@pytest.mark.parametrize("path", ["wide", "split2", "split4", "auto"])
def test_attention_without_tile_maximum(lib, path, premul):
    """The default large-grid kernel (f5_attn2f_kernel) and the default split-KV kernels never compute a tile maximum after
    a sequence's first tile: they exponentiate against the standing reference point and fall back to the exact path when a row
    sum says a score was more than 2^14 above it.  Plain and ragged shapes must match the fp64 softmax like the old kernels,
    with q plain or pre-multiplied by scale * log2(e); spikes placed in later tiles (x30 / x60 / x400 on one key: logits in the
    hundreds, i.e. inf in the fast path) must come out finite and right, also when the spike is the last key of a partial tile
    or sits in the first tile (the reference point then stays far above everything that follows)."""
    if path == "wide":
        E.check(lib.f5_debug_set_attn_wide(1))
        E.check(lib.f5_debug_set_attn_kvsplit(1))
    elif path != "auto":
        E.check(lib.f5_debug_set_attn_kvsplit(int(path[-1])))
    try:
        _attention_case(lib, 1, 2, 50, None, 1, seed=1, premul=premul)
        _attention_case(lib, 3, 2, 200, [200, 130, 1], 1, seed=7, premul=premul)
        _attention_case(lib, 2, 4, 300, [300, 211], 1, seed=21, premul=premul)
        _attention_case(lib, 1, 2, 937, None, 1, seed=8, premul=premul)
        for N, spikes in ((300, ((70, 30.0), (200, 60.0))), (937, ((936, 400.0),)), (500, ((3, 100.0),)), (700, ((64, 50.0), (65, 90.0), (640, 20.0)))):
            test_attention_softmax_spike(lib, hp=0, premul=premul, N=N, spikes=spikes)
    finally:
        E.check(lib.f5_debug_set_attn_wide(-1))
        E.check(lib.f5_debug_set_attn_kvsplit(-1))


def _with_pipelined_attention(lib, fn):
    """run fn with the in-wave software-pipelined large-grid kernel (f5_attn2p_kernel) forced on, whatever the grid size"""
    E.check(lib.f5_debug_set_attn_wide(1))
    E.check(lib.f5_debug_set_attn_kvsplit(1))
    E.check(lib.f5_debug_set_attn_pipe(1))
    try:
        fn()
    finally:
        E.check(lib.f5_debug_set_attn_pipe(0))
        E.check(lib.f5_debug_set_attn_wide(-1))
        E.check(lib.f5_debug_set_attn_kvsplit(-1))


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 96, 130, 192, 257, 320, 499, 937, 1100])
def test_attention_pipelined_v2p_shapes(lib, N):
    """f5_attn2p_kernel (attention.hip v2p: half-tile software pipeline inside the wave, one wave per SIMD, asm MFMAs with the
    register class in the constraint): every tile count 1 ... 18 incl. each tail length of the four-tile loop (T - 1 = 4 g + 1 ... 4),
    partial last tiles that end in the first / second key block, one-block sequences, waves entirely past the sequence; q is
    pre-multiplied (the only mode the kernel serves)."""
    _with_pipelined_attention(lib, lambda: _attention_case(lib, 1, 2, N, None, 1, seed=N, premul=True))


def test_attention_pipelined_v2p_ragged_and_spikes(lib):
    """ragged key lengths (a different tile count per batch element inside one launch, kv_len < seq_len), the 16-head shape, and
    spikes that force the slow path (reference point moves mid-sequence: later tiles, the last key of a partial tile, the first
    tile -- the reference point then stays far above everything that follows -- and neighbouring tiles in a row)"""
    def run():
        _attention_case(lib, 3, 2, 200, [200, 130, 1], 1, seed=7, premul=True)
        _attention_case(lib, 2, 4, 300, [300, 211], 1, seed=21, premul=True)
        _attention_case(lib, 6, 16, 1100, [1100, 1099, 513, 512, 64, 7], 1, seed=9, premul=True)
        _attention_case(lib, 4, 2, 700, [700, 33, 32, 97], 1, seed=10, premul=True)
        for N, spikes in ((300, ((70, 30.0), (200, 60.0))), (937, ((936, 400.0),)), (500, ((3, 100.0),)), (700, ((64, 50.0), (65, 90.0), (640, 20.0))),
                          (400, ((40, 40.0), (100, 80.0), (130, 160.0), (290, 300.0)))):
            test_attention_softmax_spike(lib, hp=0, premul=True, N=N, spikes=spikes)
    _with_pipelined_attention(lib, run)


def test_attention_pipelined_v2p_large_grid_matches_v2f(lib):
    """the bench shape family (16 heads, N = 937, ragged): v2p against the fp64 reference and against v2f on the same operands
    (same arithmetic up to the order of the row-sum additions and the reference point: a few 16-bit ulps)"""
    _with_pipelined_attention(lib, lambda: _attention_case(lib, 8, 16, 937, [937, 936, 900, 641, 640, 500, 65, 937], 1, seed=12, premul=True))


@pytest.mark.parametrize("ks", [1, 2, 4])
def test_attention_kv_split(lib, ks):
    """in-workgroup KV split (small-batch kernel): every split factor gives the one-pass result, including groups that
    own no tile (N < 64*ks), ragged key lengths and the online-softmax merge across groups"""
    E.check(lib.f5_debug_set_attn_kvsplit(ks))
    try:
        _attention_case(lib, 1, 2, 50, None, 1, seed=1)            # one KV tile: groups 1.. are empty
        _attention_case(lib, 2, 2, 333, [333, 100], 1, seed=5)
        _attention_case(lib, 3, 2, 200, [200, 130, 1], 3, seed=7)
        _attention_case(lib, 1, 2, 937, None, 1, seed=8)
        _attention_case(lib, 1, 2, 937, None, 3, seed=9)
    finally:
        E.check(lib.f5_debug_set_attn_kvsplit(-1))


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 14])
@pytest.mark.parametrize("nseg", [1, 3])
def test_gemm_resid_gate(lib, tile, nseg):
    """x += gate * ((A W^T + b) * keep[row])  (dit.py:172-173, 319, 323) on both GEMM kernels."""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        r = rng(31 + tile)
        M, N, K = 700, (384 if tile == 8 else 512), 256
        a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
        gate, x0 = randn(r, N), randn(r, M, N)
        keep = torch.from_numpy((r.random(M) > 0.3).astype(np.uint8))
        a_hi, a_lo = split_bf16(a.to(DEV))
        w_hi, w_lo = split_bf16(w.to(DEV))
        bias_d, gate_d, keep_d, x = bias.to(DEV), gate.to(DEV), keep.to(DEV), x0.to(DEV).clone()
        E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(bias_d), P(gate_d), P(keep_d), P(x), M, N, K, K, K,
                                          N, nseg, stream()), "gemm_resid_gate")
        sync()
        aa = a.double() if nseg == 3 else bf16r(a).double()
        ww = w.double() if nseg == 3 else bf16r(w).double()
        ref = x0.double() + gate.double() * ((aa @ ww.T + bias.double()) * keep.double()[:, None])
        mx, _, _ = report(f"gemm resid_gate tile={tile} nseg={nseg}", x.cpu(), ref)
        assert mx <= (5e-5 if nseg == 3 else 2e-4) * max(1.0, float(ref.abs().max()))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("tile", [0, 14])
def test_gemm_rs128_several_rounds_all_epilogues(lib, tile):
    """VERDICT r3 weak #1, op level: the role-split 128 x 256 kernel (gemm_rs128.hip) with more tiles than CUs -- what the `mid`
    dispatch rule (tile 0 = auto at these shapes) runs for every block GEMM of batch 2 ... 16, forced as tile 14 as well.
    M = 4 x 937 x 2 = 7 496 rows: 59 row tiles x {4, 8, 12} column tiles = 236 ... 708 workgroups (1 - 3 rounds), ragged last row tile,
    RESID_GATE with masked rows, GELU-tanh 16-bit output, QKV + RoPE + transposed V (per-element row tiles), each against fp64."""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        r = rng(900 + tile)
        Bq, Nq, D, FF = 8, 937, 1024, 2048
        M = Bq * Nq
        a = randn(r, M, D)
        a_hi, a_lo = split_bf16(a.to(DEV))
        aa = bf16r(a).double()
        # --- out-proj-shaped RESID_GATE, 30 % of the rows masked
        w, bias, gate, x0 = randn(r, D, D, scale=D ** -0.5), randn(r, D, scale=0.1), randn(r, D), randn(r, M, D)
        keep = torch.from_numpy((r.random(M) > 0.3).astype(np.uint8))
        w_hi, _ = split_bf16(w.to(DEV))
        x, bias_d, gate_d, keep_d = x0.to(DEV).clone(), bias.to(DEV), gate.to(DEV), keep.to(DEV)     # (kept alive until the sync)
        E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(None), P(w_hi), P(None), P(bias_d), P(gate_d), P(keep_d), P(x), M, D, D,
                                          D, D, D, 1, stream()), "gemm_resid_gate")
        sync()
        ref = x0.double() + gate.double() * ((aa @ bf16r(w).double().T + bias.double()) * keep.double()[:, None])
        mx, _, _ = report(f"rs128 rounds resid_gate tile={tile} M={M}", x.cpu(), ref)
        assert mx <= 2e-4 * max(1.0, float(ref.abs().max()))
        # --- FF1-shaped GELU-tanh, 16-bit output
        w1, b1 = randn(r, FF, D, scale=D ** -0.5), randn(r, FF, scale=0.1)
        w1_hi, _ = split_bf16(w1.to(DEV))
        out16 = torch.zeros((M, FF), dtype=op_dtype(), device=DEV)
        b1_d = b1.to(DEV)
        E.check(lib.f5_op_gemm(P(a_hi), P(None), P(w1_hi), P(None), P(b1_d), P(None), P(out16), P(None), M, FF, D, D, D, FF, 1, 2, stream()), "gemm gelu")
        sync()
        refg = torch.nn.functional.gelu(aa @ bf16r(w1).double().T + b1.double(), approximate="tanh")
        mx, _, _ = report(f"rs128 rounds gelu tile={tile} M={M}", out16.float().cpu(), refg)
        assert mx <= tol16(1.5e-2) * max(1.0, float(refg.abs().max()))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))
    # --- QKV + RoPE + V^T through the same dispatch (attention on top checks q / k / V^T end to end); premul + pair-major tables as sample()
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        _attention_case(lib, 8, 16, 937, [937, 900, 800, 700, 600, 937, 500, 937], 1, seed=77, premul=True, tr_tables=True)
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


# (row mean / sigma, massive-activation channels, drift of the mean since the previous LayerNorm / sigma): the first row is ordinary data,
# the others are what a trained checkpoint may hold -- VERDICT r4 "next" #2
FOLD_STRESS = [(0.5, False, 0.2), (10.0, False, 0.3), (100.0, True, 1.0), (1.0, True, 0.0)]


@pytest.mark.parametrize("tile", [4, 14, "small"])
@pytest.mark.parametrize("stress", range(len(FOLD_STRESS)))
def test_ln_modulate_folded_into_the_gemms_around_it(lib, tile, stress):
    """LN fold (csrc/gemm.hpp fold_*; dit.py:319-321 and :323 -> :270 -> :136): the residual GEMM leaves (x - m)(1 + s) as 16-bit operands
    (m = the row's mean at the previous LayerNorm) plus per-row slice statistics, a tiny kernel merges them into rstd and
    rstd (mean - m), the QKV / FF1 GEMM finishes the LN in its epilogue:
        (LN(x)(1 + s) + b) W^T + bias = rstd (((x - m)(1 + s)) W^T) - rstd (mean - m) c1 + c2,   c1 = W (1 + s),  c2 = W b + bias.
    Both staged kernels (tile 4 = 256x256, 14 = role-split 128x256), ragged last row tile, masked rows.  Checked piece by piece:
    x bit-identical to the plain launch, x16 the exact rounding of (x - m)(1 + s), the slice statistics, the row factors and the
    constants against fp64, and the consumer outputs against an fp64 evaluation of the folded formula on the SAME operands (sharp: one
    16-bit rounding) as well as against the exact LN-modulate + GEMM NEXT TO the unfolded path (ln_modulate kernel + plain GEMM) on the
    same inputs: row means of 0.5 / 10 / 100 sigma, four channels at 1e3 sigma -- the folded error must stay within 2x the unfolded one
    whatever the mean is (the round-4 formulation, m = 0, is 10x / 100x worse at 10 / 100 sigma: profiles/r05/ln_fold_numerics_study.jsonl)."""
    # tile "small" (round 6): the batch-1-sized route -- automatic dispatch at M = 2 x 937 rows: the producer is the 64 x 128 split-K ring
    # kernel, the consumers the 8-wave 128 x 128 ring kernel (FF1) and one round of role-split 128 x 256 tiles (QKV), both in the
    # STATISTICS form (they merge the slice statistics themselves; there is no row-factor form on that route)
    small = tile == "small"
    mu_sig, outliers, drift = FOLD_STRESS[stress]
    r = rng(4100 + (1 if small else tile) + 17 * stress)
    Bq, Nq, H, D, FF = (2 if small else 8), 937, 16, 1024, 2048
    if small:
        tile = 0
    M = Bq * Nq
    eps_op = 2.0 ** -8 if op_dtype() == torch.bfloat16 else 2.0 ** -11
    a = randn(r, M, D)
    wo, bo, gate, x0 = randn(r, D, D, scale=D ** -0.5), randn(r, D, scale=0.1), randn(r, D), randn(r, M, D)
    if outliers:
        x0[:, 5:9] *= 1.0e3                                               # massive-activation channels
    x0 += 0.3 * randn(r, 1, D)                                             # column offsets
    sig0 = x0.std(-1, unbiased=False, keepdim=True)
    x0 += mu_sig * sig0 * torch.where(randn(r, M, 1) < 0, -1.0, 1.0)      # row means of mu_sig sigma, either sign
    keep = torch.from_numpy((r.random(M) > 0.3).astype(np.uint8))
    sv = torch.stack([randn(r, D, scale=0.3), randn(r, D, scale=0.3)])     # two modulation vectors: the second one is used (strides)
    bv = torch.stack([randn(r, D, scale=0.3), randn(r, D, scale=0.3)])
    a_hi, _ = split_bf16(a.to(DEV))
    wo_hi, _ = split_bf16(wo.to(DEV))
    bo_d, gate_d, keep_d, sv_d, bv_d = bo.to(DEV), gate.to(DEV), keep.to(DEV), sv.to(DEV), bv.to(DEV)
    x_plain, x = x0.to(DEV).clone(), x0.to(DEV).clone()
    x16 = torch.zeros((M, D), dtype=op_dtype(), device=DEV)
    stats = torch.full((D // 64, M, 2), float("nan"), device=DEV)             # slice-major
    s1, b1 = sv[1], bv[1]
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(None), P(wo_hi), P(None), P(bo_d), P(gate_d), P(keep_d), P(x_plain), M, D, D, D, D, D, 1,
                                          stream()), "resid_gate plain")
        sync()
        # the shift a forward would hold: the row's mean at the previous LayerNorm = the new mean minus what this update moved it by
        xnew = x_plain.cpu()
        m_prev = (xnew.double().mean(-1) - drift * xnew.double().std(-1, unbiased=False) * torch.where(randn(r, M) < 0, -1.0, 1.0).double()).float()
        shift_d = m_prev.to(DEV).clone()
        shift0_d = shift_d.clone()                                            # (f5_op_fold_rows below replaces shift_d by the rows' means)
        E.check(lib.f5_debug_set_op_fold_producer(P(sv_d[1]), P(x16), P(stats), P(shift_d)))
        try:
            E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(None), P(wo_hi), P(None), P(bo_d), P(gate_d), P(keep_d), P(x), M, D, D, D, D, D, 1,
                                              stream()), "resid_gate fold producer")
            # (tests/test_gemm_matrix_gpu.py leaves the fold variants of the batch-1-sized kernels to this test: say which one ran)
            assert last_gemm_kernel(lib) == {4: "gemm256", 14: "rs128"}.get(tile, "ring_ks2<1>+fold_producer")
        finally:
            E.check(lib.f5_debug_set_op_fold_producer(P(None), P(None), P(None), P(None)))
        sync()
        if stress == 0:
            # the operand-range flag: (x - m)(1 + s) is the one fp16 operand without a natural bound -- a value beyond +-65 504 must raise
            # bit 0 of the flag word (fp16 build only; bf16 has the range), ordinary data must leave it alone
            flag = torch.zeros(4, dtype=torch.int32, device=DEV)
            xbig = (x0 * 3.0e4).to(DEV).clone()
            for xin, want in ((x0.to(DEV).clone(), 0), (xbig, 1 if op_dtype() == torch.float16 else 0)):
                flag.zero_()
                E.check(lib.f5_debug_set_op_fold_overflow_flag(P(flag)))
                try:
                    x16_tmp, stats_tmp = torch.zeros_like(x16), torch.zeros_like(stats)
                    E.check(lib.f5_debug_set_op_fold_producer(P(sv_d[1]), P(x16_tmp), P(stats_tmp), P(None)))
                    E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(None), P(wo_hi), P(None), P(bo_d), P(gate_d), P(keep_d), P(xin), M, D, D, D, D, D, 1,
                                                      stream()), "resid_gate fold producer (range flag)")
                    sync()
                finally:
                    E.check(lib.f5_debug_set_op_fold_producer(P(None), P(None), P(None), P(None)))
                    E.check(lib.f5_debug_set_op_fold_overflow_flag(P(None)))
                assert flag.cpu().tolist() == [want, 0, 0, 0], (flag.cpu().tolist(), want)
        assert torch.equal(x, x_plain), "the fold producer changed the residual stream"
        xc = x.cpu()
        dsh = xc - m_prev[:, None]                                           # fp32, as the kernel subtracts
        want16 = (dsh * (1.0 + s1)).to(op_dtype())
        assert torch.equal(x16.cpu(), want16), "x16 is not the rounding of (x - m)(1 + s)"
        ds = dsh.double().reshape(M, D // 64, 64)
        st = stats.cpu().double().permute(1, 0, 2)
        assert float((st[..., 0] - ds.sum(-1)).abs().max()) <= 1e-5 * float(ds.abs().sum(-1).max())
        m2_ref = ((ds - ds.mean(-1, keepdim=True)) ** 2).sum(-1)
        assert float((st[..., 1] - m2_ref).abs().max()) <= 2e-5 * float(m2_ref.max())
        rowf = torch.full((M + 8, 2), float("nan"), device=DEV)
        E.check(lib.f5_op_fold_rows(P(stats), D // 64, M, P(rowf), P(shift_d), stream()), "fold_rows")
        sync()
        x64 = xc.double()
        mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
        rstd = (var + 1e-6).rsqrt()
        mean_d = mean - m_prev.double()[:, None]
        rf = rowf.cpu().double()
        assert bool(torch.isnan(rf[M:]).all())
        assert float((rf[:M, 0:1] / rstd - 1.0).abs().max()) <= 2e-5, "rstd"
        assert float((rf[:M, 1:2] - rstd * mean_d).abs().max()) <= 2e-5 * float((rstd * mean_d).abs().max() + 1.0)
        # fold_rows leaves the row's mean behind: the next producer's shift
        assert float((shift_d.cpu().double()[:, None] - mean).abs().max()) <= 2e-6 * float(mean.abs().max() + var.sqrt().max())
        # the generic slice count (the 16-slice case above is the unrolled instantiation): the first 8 slices as a 512-wide row, no shift
        rowf8 = torch.zeros((M, 2), device=DEV)
        E.check(lib.f5_op_fold_rows(P(stats), 8, M, P(rowf8), P(None), stream()), "fold_rows (8 slices)")
        sync()
        d8 = dsh.double()[:, :512]
        m8, v8 = d8.mean(-1, keepdim=True), d8.var(-1, unbiased=False, keepdim=True)
        r8 = (v8 + 1e-6).rsqrt()
        assert float((rowf8.cpu().double()[:, 0:1] / r8 - 1.0).abs().max()) <= 2e-5
        assert float((rowf8.cpu().double()[:, 1:2] - r8 * m8).abs().max()) <= 2e-5 * float((r8 * m8).abs().max() + 1.0)
        # --- constants, for both consumers
        w1, bias1 = randn(r, FF, D, scale=D ** -0.5), randn(r, FF, scale=0.1)
        wq, biasq = randn(r, 3 * D, D, scale=D ** -0.5), randn(r, 3 * D, scale=0.1)
        w1_hi, _ = split_bf16(w1.to(DEV))
        wq_hi, _ = split_bf16(wq.to(DEV))
        bias1_d, biasq_d = bias1.to(DEV), biasq.to(DEV)
        consts = {}
        for nm, w_hi, wf, bias_d, bias, Nn in (("ff1", w1_hi, w1, bias1_d, bias1, FF), ("qkv", wq_hi, wq, biasq_d, biasq, 3 * D)):
            c1 = torch.full((2, Nn + 64), float("nan"), device=DEV)
            c2 = torch.full((2, Nn + 64), float("nan"), device=DEV)
            E.check(lib.f5_op_fold_consts(P(w_hi), D, P(bias_d), P(sv_d), P(bv_d), C.c_size_t(D), 2, P(c1), P(c2), C.c_size_t(Nn + 64), Nn, D,
                                          stream()), "fold_consts")
            sync()
            w64 = bf16r(wf).double()
            for v in range(2):
                r1, r2 = w64 @ (1.0 + sv[v].double()), w64 @ bv[v].double() + bias.double()
                assert float((c1[v, :Nn].cpu().double() - r1).abs().max()) <= 2e-5 * float(r1.abs().max()), nm
                assert float((c2[v, :Nn].cpu().double() - r2).abs().max()) <= 2e-5 * max(1.0, float(r2.abs().max())), nm
            assert bool(torch.isnan(c1[:, Nn:]).all()) and bool(torch.isnan(c2[:, Nn:]).all())
            consts[nm] = (c1, c2, w64)
        # --- the folded formula in fp64 on the operands the consumers see, the exact LN-modulate + projection, and the UNFOLDED path
        h_exact = (x64 - mean) * rstd * (1.0 + s1.double()) + b1.double()
        h16 = torch.zeros((M, D), dtype=op_dtype(), device=DEV)
        E.check(lib.f5_op_ln_modulate(P(x), P(sv_d[1]), P(bv_d[1]), P(h16), P(None), M, D, stream()), "ln_modulate (unfolded path)")
        sync()

        def folded(nm, bias):
            c1, c2, w64 = consts[nm]
            return rstd * (want16.double() @ w64.T) - rstd * mean_d * c1[1, :w64.shape[0]].cpu().double() + c2[1, :w64.shape[0]].cpu().double()

        def rel_l1(got, ref):
            return float((got.double() - ref).abs().mean()) / float(ref.pow(2).mean().sqrt())

        def max_err(got, ref):
            return float((got.double() - ref).abs().max())

        # FF1 + GELU-tanh
        out16 = torch.zeros((M, FF), dtype=op_dtype(), device=DEV)
        out16_unf = torch.zeros((M, FF), dtype=op_dtype(), device=DEV)
        c1, c2, w64 = consts["ff1"]
        E.check(lib.f5_op_gemm(P(h16), P(None), P(w1_hi), P(None), P(bias1_d), P(None), P(out16_unf), P(None), M, FF, D, D, D, FF, 1, 2, stream()),
                "gemm gelu unfolded")
        mean_small = torch.full((M,), float("nan"), device=DEV)
        E.check(lib.f5_debug_set_op_fold_consumer(P(None) if small else P(rowf), P(c1[1]), P(c2[1])))
        if small:
            E.check(lib.f5_debug_set_op_fold_stats(P(stats), M, P(shift0_d), P(mean_small)))
        try:
            E.check(lib.f5_op_gemm(P(x16), P(None), P(w1_hi), P(None), P(None), P(None), P(out16), P(None), M, FF, D, D, D, FF, 1, 2, stream()),
                    "gemm gelu folded")
            sync()
            if small:
                assert torch.equal(mean_small, shift_d), "the rows' means left behind by the small FF1 consumer differ from fold_rows'"
            sharp = F.gelu(folded("ff1", bias1), approximate="tanh")
            exact = F.gelu(h_exact @ w64.T + bias1.double(), approximate="tanh")
            mx, _, _ = report(f"LN fold FF1 tile={tile} stress={FOLD_STRESS[stress]}: vs the folded formula in fp64", out16.float().cpu(), sharp)
            assert mx <= 2.5 * eps_op * max(1.0, float(sharp.abs().max()))
            e_fold, e_unf = rel_l1(out16.float().cpu(), exact), rel_l1(out16_unf.float().cpu(), exact)
            print(f"[ln_fold stress] tile={tile} |mu|/sigma={mu_sig} outliers={outliers} drift={drift}: FF1 mean|err|/rms folded {e_fold:.3e} "
                  f"unfolded {e_unf:.3e} ratio {e_fold / e_unf:.2f}")
            assert e_fold <= 2.0 * e_unf + 1e-6, (e_fold, e_unf)
            # a LOCALISED fault (one wrong row factor, one slice) hides in a mean -- the worst element of the folded path must
            # stay within a small factor of the worst element of the unfolded path against the same exact value
            m_fold, m_unf = max_err(out16.float().cpu(), exact), max_err(out16_unf.float().cpu(), exact)
            print(f"[ln_fold stress] tile={tile} FF1 max|err| folded {m_fold:.3e} unfolded {m_unf:.3e} ratio {m_fold / m_unf:.2f}")
            assert m_fold <= 4.0 * m_unf + 1e-6, (m_fold, m_unf)
            # --- the STATISTICS form of the consumer (round 6): no f5_op_fold_rows in between -- the kernel merges the producer's slice
            # statistics into its rows' factors before its K loop, in the arithmetic order of f5_fold_rows_kernel: the SAME bits, and the
            # workgroups of column tile 0 leave the rows' means behind (what fold_rows wrote into shift_d)
            out16_s = torch.zeros((M, FF), dtype=op_dtype(), device=DEV)
            mean_s = torch.full((M + 8,), float("nan"), device=DEV)
            E.check(lib.f5_debug_set_op_fold_consumer(P(None), P(c1[1]), P(c2[1])))
            E.check(lib.f5_debug_set_op_fold_stats(P(stats), M, P(shift0_d), P(mean_s)))
            try:
                E.check(lib.f5_op_gemm(P(x16), P(None), P(w1_hi), P(None), P(None), P(None), P(out16_s), P(None), M, FF, D, D, D, FF, 1, 2, stream()),
                        "gemm gelu folded, statistics form")
                assert last_gemm_kernel(lib) == {4: "gemm256+fold_stats", 14: "rs128+fold_stats"}.get(tile, "ring8<2>+fold_consumer")
                sync()
            finally:
                E.check(lib.f5_debug_set_op_fold_stats(P(None), 0, P(None), P(None)))
            assert torch.equal(out16_s, out16), "FF1: the statistics form differs from fold_rows + row factors"
            assert torch.equal(mean_s[:M], shift_d) and bool(torch.isnan(mean_s[M:]).all()), "the rows' means left behind differ from fold_rows'"
            E.check(lib.f5_debug_set_op_fold_consumer(P(None) if small else P(rowf), P(c1[1]), P(c2[1])))
            # --- QKV + RoPE + V^T, transposed q / k tiles, q pre-multiplied (as sample() runs it)
            npad = (Nq + 63) // 64 * 64
            cos_t, sin_t = torch.empty((Nq, 32), device=DEV), torch.empty((Nq, 32), device=DEV)
            E.check(lib.f5_op_rope_table(P(cos_t), P(sin_t), Nq, 64, stream()))
            tt = [torch.empty(64 * Nq, device=DEV) for _ in range(2)]
            E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), Nq, 64, C.c_float(QPRE), stream()))
            qk = torch.zeros((M, 2 * D), dtype=op_dtype(), device=DEV)
            vt = torch.zeros((Bq * H, 64, npad), dtype=op_dtype(), device=DEV)
            qk_unf, vt_unf = torch.zeros_like(qk), torch.zeros_like(vt)
            c1, c2, w64 = consts["qkv"]
            E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0]), P(tt[1])))
            E.check(lib.f5_debug_set_op_q_premul(C.c_float(QPRE)))
            try:
                E.check(lib.f5_debug_set_op_fold_consumer(P(None), P(None), P(None)))
                E.check(lib.f5_op_qkv_rope(P(h16), P(None), P(wq_hi), P(None), P(biasq_d), P(cos_t), P(sin_t), P(qk_unf), P(None), P(vt_unf), P(None),
                                           Bq, Nq, npad, H, D, 1, stream()), "qkv_rope unfolded")
                E.check(lib.f5_debug_set_op_fold_consumer(P(None) if small else P(rowf), P(c1[1]), P(c2[1])))
                if small:
                    E.check(lib.f5_debug_set_op_fold_stats(P(stats), M, P(shift0_d), P(mean_small)))
                E.check(lib.f5_op_qkv_rope(P(x16), P(None), P(wq_hi), P(None), P(None), P(cos_t), P(sin_t), P(qk), P(None), P(vt), P(None),
                                           Bq, Nq, npad, H, D, 1, stream()), "qkv_rope folded")
                sync()
                qk_s, vt_s = torch.zeros_like(qk), torch.zeros_like(vt)            # the statistics form: q / k (transposed tiles) and V (straight)
                mean_q = torch.full((M,), float("nan"), device=DEV)
                E.check(lib.f5_debug_set_op_fold_consumer(P(None), P(c1[1]), P(c2[1])))
                E.check(lib.f5_debug_set_op_fold_stats(P(stats), M, P(shift0_d), P(mean_q)))
                try:
                    E.check(lib.f5_op_qkv_rope(P(x16), P(None), P(wq_hi), P(None), P(None), P(cos_t), P(sin_t), P(qk_s), P(None), P(vt_s), P(None),
                                               Bq, Nq, npad, H, D, 1, stream()), "qkv_rope folded, statistics form")
                    sync()
                finally:
                    E.check(lib.f5_debug_set_op_fold_stats(P(None), 0, P(None), P(None)))
                assert torch.equal(qk_s, qk) and torch.equal(vt_s, vt), "QKV: the statistics form differs from fold_rows + row factors"
                assert torch.equal(mean_q, shift_d)
            finally:
                E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
                E.check(lib.f5_debug_set_op_q_premul(C.c_float(0.0)))
        finally:
            E.check(lib.f5_debug_set_op_fold_consumer(P(None), P(None), P(None)))
        freqs = O.rotary_freqs(64, Nq).double()

        def unpack(qk_, vt_):
            gq = qk_.float().cpu()[:, :D].reshape(Bq, Nq, H, 64).transpose(1, 2) / QPRE
            gk = qk_.float().cpu()[:, D:].reshape(Bq, Nq, H, 64).transpose(1, 2)
            gv = vt_.float().cpu().reshape(Bq, H, 64, npad)[..., :Nq].transpose(-1, -2)
            return gq, gk, gv

        got, got_unf = unpack(qk, vt), unpack(qk_unf, vt_unf)
        for label, qkv in (("folded formula", folded("qkv", biasq)), ("exact LN", h_exact @ w64.T + biasq.double())):
            q, k, v = [t.reshape(Bq, Nq, H, 64).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
            q, k = O.apply_rotary_pos_emb(q, freqs), O.apply_rotary_pos_emb(k, freqs)
            for nm, g, gu, rf_ in (("q", got[0], got_unf[0], q), ("k", got[1], got_unf[1], k), ("v", got[2], got_unf[2], v)):
                if label == "folded formula":
                    mx, _, _ = report(f"LN fold QKV tile={tile} {nm} vs {label}", g, rf_)
                    rot = 0.0 if nm == "v" else 2.0 * Nq * 2.0 ** -23
                    assert mx <= (2.5 * eps_op + rot) * max(1.0, float(rf_.abs().max())), (nm, label)
                else:
                    e_fold, e_unf = rel_l1(g, rf_), rel_l1(gu, rf_)
                    print(f"[ln_fold stress] tile={tile} |mu|/sigma={mu_sig}: {nm} mean|err|/rms folded {e_fold:.3e} unfolded {e_unf:.3e} "
                          f"ratio {e_fold / e_unf:.2f}")
                    assert e_fold <= 2.0 * e_unf + 1e-6, (nm, e_fold, e_unf)
                    m_fold, m_unf = max_err(g, rf_), max_err(gu, rf_)
                    print(f"[ln_fold stress] tile={tile} {nm} max|err| folded {m_fold:.3e} unfolded {m_unf:.3e} ratio {m_fold / m_unf:.2f}")
                    assert m_fold <= 4.0 * m_unf + 1e-6, (nm, m_fold, m_unf)
        assert float(vt.float().cpu().reshape(Bq, H, 64, npad)[..., Nq:].abs().max()) == 0.0
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


def test_ln_fold_fields_fail_loudly_on_small_tile_launches(lib):
    """The fold fields are only implemented by the staged epilogues: a launch that would run a small-tile kernel must refuse them."""
    r = rng(5)
    M, D = 937, 1024
    a_hi, _ = split_bf16(randn(r, M, D).to(DEV))
    w_hi, _ = split_bf16(randn(r, D, D, scale=D ** -0.5).to(DEV))
    gate, sc = randn(r, D).to(DEV), randn(r, D).to(DEV)
    x = randn(r, M, D).to(DEV)
    x16 = torch.zeros((M, D), dtype=op_dtype(), device=DEV)
    stats = torch.zeros((D // 64, M, 2), device=DEV)
    E.check(lib.f5_debug_set_op_fold_producer(P(sc), P(x16), P(stats), P(None)))
    try:
        rc = lib.f5_op_gemm_resid_gate(P(a_hi), P(None), P(w_hi), P(None), P(None), P(gate), P(None), P(x), M, D, D, D, D, D, 1, stream())
    finally:
        E.check(lib.f5_debug_set_op_fold_producer(P(None), P(None), P(None), P(None)))
    sync()
    assert rc != 0 and "LN fold" in lib.f5_last_error().decode()


@pytest.mark.parametrize("tile", [0, 1, 2, 4, 5])
@pytest.mark.parametrize("nseg", [1, 3])
def test_gemm_addrows(lib, tile, nseg):
    """EPI_ADDROWS: out = A[row % a_row_mod] W^T + addrows[row]  (+ the 16-bit copy) -- the per-step half of the split input
    projection (dit.py:250), K = 128 (mel 100 zero padded), both CFG branches reading the same x rows."""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        r = rng(77 + tile)
        M1, N, K = 350, 512, 128
        M = 2 * M1
        a, w = randn(r, M1, K), randn(r, N, K, scale=K ** -0.5)
        a[:, 100:] = 0.0
        add = randn(r, M, N)
        a_hi, a_lo = split_bf16(a.to(DEV))
        w_hi, w_lo = split_bf16(w.to(DEV))
        add_d = add.to(DEV)
        out = torch.full((M, N), float("nan"), device=DEV)
        hi = torch.zeros((M, N), dtype=op_dtype(), device=DEV)
        lo = torch.zeros_like(hi)
        E.check(lib.f5_op_gemm_addrows(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(add_d), M1, P(out), P(hi), P(lo), M, N, K, K, K, N, nseg,
                                       stream()), "gemm_addrows")
        sync()
        aa = a.double() if nseg == 3 else bf16r(a).double()
        ww = w.double() if nseg == 3 else bf16r(w).double()
        ref = torch.cat([aa, aa]) @ ww.T + add.double()
        mx, _, _ = report(f"gemm addrows tile={tile} nseg={nseg}", out.cpu(), ref)
        assert mx <= (5e-5 if nseg == 3 else 2e-4) * max(1.0, float(ref.abs().max()))
        assert torch.equal(hi.cpu(), bf16r(out.cpu()).to(op_dtype()))            # the 16-bit copy is the rounding of the fp32 value
        if nseg == 3:
            assert float((join(hi, lo).cpu().double() - out.cpu().double()).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 5, 6, 9, 10, 11])
def test_gemm_resid_gate_fused_ln_is_bit_identical(lib, tile, nseg):
    """LN-modulate fused behind the residual GEMM (the last-arriving workgroup of a row block runs it, dit.py:319-321 in one
    launch): x and h must equal, bit for bit, f5_op_gemm_resid_gate followed by f5_op_ln_modulate -- for every small-tile kernel
    configuration, with row masking, ragged M, all four LN widths, and on a second launch (the counters re-arm themselves)."""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for (M, N, K) in ((1874, 1024, 1024), (1874, 1024, 2048), (937, 1024, 1024), (333, 512, 192), (70, 256, 64), (129, 768, 128)):
            if tile == 9 and N % 128:
                continue
            r = rng(M + N + K + tile + nseg)
            a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
            gate, scale, shift = randn(r, N, scale=0.5), randn(r, N, scale=0.3), randn(r, N, scale=0.3)
            x0 = randn(r, M, N, scale=2.0)
            keep = (torch.from_numpy(r.random(M)) > 0.2).to(torch.uint8)
            a_hi, a_lo = split_bf16(a.to(DEV))
            w_hi, w_lo = split_bf16(w.to(DEV))
            lo = (lambda t: t) if nseg == 3 else (lambda t: None)
            dv = lambda t: t.to(DEV).contiguous()
            bias_d, gate_d, scale_d, shift_d, keep_d = dv(bias), dv(gate), dv(scale), dv(shift), dv(keep)
            # reference: two launches
            x_ref = dv(x0)
            h_ref = torch.zeros((M, N), dtype=op_dtype(), device=DEV)
            h_ref_lo = torch.zeros_like(h_ref)
            E.check(lib.f5_op_gemm_resid_gate(P(a_hi), P(lo(a_lo)), P(w_hi), P(lo(w_lo)), P(bias_d), P(gate_d), P(keep_d), P(x_ref), M, N, K,
                                              K, K, N, nseg, stream()), "gemm_resid_gate")
            E.check(lib.f5_op_ln_modulate(P(x_ref), P(scale_d), P(shift_d), P(h_ref), P(lo(h_ref_lo)), M, N, stream()), "ln_modulate")
            sync()
            counters = torch.zeros((M + 63) // 64 + 8, dtype=torch.int32, device=DEV)
            for rep in range(2):
                x = dv(x0)
                h = torch.full((M, N), 7.0, dtype=op_dtype(), device=DEV)
                h_lo = torch.full_like(h, 7.0)
                E.check(lib.f5_op_gemm_resid_gate_ln(P(a_hi), P(lo(a_lo)), P(w_hi), P(lo(w_lo)), P(bias_d), P(gate_d), P(keep_d), P(x),
                                                     P(scale_d), P(shift_d), P(h), P(lo(h_lo)), P(counters), M, N, K, K, K, nseg, stream()),
                        "gemm_resid_gate_ln")
                sync()
                assert torch.equal(x, x_ref), f"x differs (tile {tile}, {M}x{N}x{K}, launch {rep})"
                assert torch.equal(h.view(torch.int16), h_ref.view(torch.int16)), f"h differs (tile {tile}, {M}x{N}x{K}, launch {rep})"
                if nseg == 3:
                    assert torch.equal(h_lo.view(torch.int16), h_ref_lo.view(torch.int16))
                assert int(counters.abs().sum()) == 0, "row-block counters must re-arm"
        # a shape that runs the 256x256 kernel has no fused tail: the call must fail loudly, not skip the LN
        if tile == 0:
            M, N, K = 40000, 1024, 64
            z16 = torch.zeros((M, K), dtype=op_dtype(), device=DEV)
            w16 = torch.zeros((N, K), dtype=op_dtype(), device=DEV)
            v = torch.zeros(N, device=DEV)
            x = torch.zeros((M, N), device=DEV)
            h = torch.zeros((M, N), dtype=op_dtype(), device=DEV)
            cnt = torch.zeros(1024, dtype=torch.int32, device=DEV)
            rc = lib.f5_op_gemm_resid_gate_ln(P(z16), P(None), P(w16), P(None), P(v), P(v), P(None), P(x), P(v), P(v), P(h), P(None), P(cnt),
                                              M, N, K, K, K, 1, stream())
            assert rc != 0 and b"fused LN" in lib.f5_last_error()
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("tile", [1, 2, 3, 5, 6])
def test_gemm_all_small_tile_kernels(lib, tile):
    """every block-tile variant (register-staged 128x128 / 64x128 / 64x64 and the global_load_lds ring 64x128 / 64x64)"""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for (M, N, K) in ((1, 128, 64), (333, 384, 192), (1874, 1024, 1024), (130, 100, 2048)):
            r = rng(M + N + K + tile)
            a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
            refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
            out, _, _ = _gemm(lib, a, w, bias, 0, 1)
            mx, _, _ = report(f"gemm tile={tile} {M}x{N}x{K}", out, refbf)
            assert mx <= 2e-4 * max(1.0, float(refbf.abs().max()))
            out3, _, _ = _gemm(lib, a, w, bias, 0, 3)
            ref32 = a.double() @ w.double().T + bias.double()
            assert float((out3.double() - ref32).abs().max()) <= 5e-5 * max(1.0, float(ref32.abs().max()))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("tile", [8, 9, 10, 11])
def test_gemm_ring8_kernels(lib, tile):
    """8-wave ring kernels (128x192 / 128x128 block tiles; 64x128 / 128x128 with the K tiles split over two wave groups
    and summed through LDS), one workgroup per CU at batch 1: plain, bf16x3, the fused
    epilogues and the QKV + RoPE + head-split epilogue whose 96-column wave tiles straddle head boundaries"""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for (M, N, K) in ((1, 384, 64), (333, 384, 192), (1874, 768, 1024), (130, 1152, 2048)):
            r = rng(M + N + K + tile)
            a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
            refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
            out, _, _ = _gemm(lib, a, w, bias, 0, 1)
            mx, _, _ = report(f"gemm tile={tile} {M}x{N}x{K}", out, refbf)
            assert mx <= 2e-4 * max(1.0, float(refbf.abs().max()))
            out3, _, _ = _gemm(lib, a, w, bias, 0, 3)
            ref32 = a.double() @ w.double().T + bias.double()
            assert float((out3.double() - ref32).abs().max()) <= 5e-5 * max(1.0, float(ref32.abs().max()))
            _, hi, lo = _gemm(lib, a, w, bias, 2, 3)
            refg = F.gelu(ref32, approximate="tanh")
            assert float((join(hi, lo).double() - refg).abs().max()) <= 1e-4 * max(1.0, float(refg.abs().max()))
        _attention_case(lib, 2, 4, 300, [300, 211], 1, seed=21)     # D = 256, N = 768 = 4 x 192 = 6 x 128
        _attention_case(lib, 1, 6, 130, None, 3, seed=22)           # D = 384, N = 1152
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("tile", [0, 5, 9, 10])
def test_gemm_ring_band_major_numbering_same_bits(lib, tile):
    """Ring kernels, tile numbering (f5_debug_set_gemm_order): band-major (3; the auto choice for one-round launches whose A operand fits
    an L2 -- batch-1 out-projection / FF1 / FF2) only permutes which workgroup computes which tile: the results must be bit-identical to
    m-fastest (2) and n-fastest (1), on the batch-1 shapes, a ragged one and one whose column tiles do not split into bands."""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for (M, N, K) in ((1874, 1024, 1024), (1874, 2048, 1024), (1874, 1024, 2048), (999, 1536, 256), (700, 768, 128)):
            r = rng(M + N + K)
            a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
            outs = {}
            for order in (1, 2, 3, 0):
                E.check(lib.f5_debug_set_gemm_order(order))
                outs[order] = _gemm(lib, a, w, bias, 0, 1)[0].clone()
            ref = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
            assert float((outs[3].double() - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max()))
            for order in (1, 2, 0):
                assert torch.equal(outs[order], outs[3]), (tile, M, N, K, order)
    finally:
        E.check(lib.f5_debug_set_gemm_order(0))
        E.check(lib.f5_debug_set_gemm_tile(0))


@pytest.mark.parametrize("tile", [12, 13])
def test_gemm_wide_ring_kernels(lib, tile):
    """128x256 ring tiles (8 waves of 64x64, 8 waves of 32x128): plain, bf16x3, GELU epilogue and the
    QKV + RoPE + head-split epilogue (staged, one or two heads per wave tile)"""
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        for (M, N, K) in ((1, 256, 64), (333, 512, 192), (1874, 768, 1024), (130, 1280, 2048)):
            r = rng(M + N + K + tile)
            a, w, bias = randn(r, M, K), randn(r, N, K, scale=K ** -0.5), randn(r, N, scale=0.1)
            refbf = (bf16r(a).double() @ bf16r(w).double().T) + bias.double()
            out, hi1, _ = _gemm(lib, a, w, bias, 1, 1)
            mx, _, _ = report(f"gemm tile={tile} {M}x{N}x{K}", hi1.float(), refbf)
            assert mx <= tol16(1e-2) * max(1.0, float(refbf.abs().max()))
            _, hi, lo = _gemm(lib, a, w, bias, 1, 3)
            ref32 = a.double() @ w.double().T + bias.double()
            assert float((join(hi, lo).double() - ref32).abs().max()) <= 5e-5 * max(1.0, float(ref32.abs().max()))
            _, hi, lo = _gemm(lib, a, w, bias, 2, 3)
            refg = F.gelu(ref32, approximate="tanh")
            assert float((join(hi, lo).double() - refg).abs().max()) <= 1e-4 * max(1.0, float(refg.abs().max()))
        _attention_case(lib, 2, 4, 300, [300, 211], 1, seed=21)     # D = 256, N = 768 = 3 x 256
        _attention_case(lib, 1, 8, 130, None, 3, seed=22)           # D = 512, N = 1536
        _attention_case(lib, 2, 16, 937, None, 1, seed=23)          # the batch-1 shape: M = 1874, N = 3072
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))

