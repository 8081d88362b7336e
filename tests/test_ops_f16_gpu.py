"""Per-kernel parity of the fp16-operand build of the kernels (engine precision "f16", namespace f5hf in csrc/op16.hpp).

The op tests of test_ops_gpu.py are written against "the operand type": here a fixture switches both the test helpers
(f5test.operand_mode: buffers and reference rounding become torch.float16) and the library's f5_op_* entry points to fp16
and re-runs them with the parameter lists of the bf16 tests -- every MFMA kernel family (small-tile, ring, 8-wave ring, split-K ring,
wide ring, 256x256 and role-split 128x256 GEMMs with each fused epilogue; the attention kernels incl. ragged masks, the KV split and
the online-softmax rescale path; the conv position embedding) and the 16-bit producers (LN-modulate, depthwise conv + LN, GRN).
The fp16 kernels are separately compiled code (the f5_sat clamp, sat_flag, other MFMA and convert instructions), and the bounds of
the shared test bodies follow the operand type (test_ops_gpu.eps_op / tol16): an fp16 kernel that loses three significand bits fails.
"""
import numpy as np
import pytest
import torch

import test_ops_gpu as T
from f5test import DEV, E, P, bf16r, op_dtype, operand_mode, randn, report, rng, split_bf16, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


@pytest.fixture(autouse=True)
def f16_operands():
    with operand_mode("f16"):
        assert op_dtype() == torch.float16
        yield
    assert op_dtype() == torch.bfloat16


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (937, 100, 256), (1874, 1024, 1024)])
def test_gemm_f32_out_f16(lib, M, N, K):
    T.test_gemm_f32_out(lib, M, N, K)


def test_gemm_asymmetric_identity_f16(lib):
    T.test_gemm_asymmetric_identity(lib)


@pytest.mark.parametrize("epi", [1, 2, 3])
def test_gemm_epilogues_f16(lib, epi):
    T.test_gemm_epilogues(lib, epi)


@pytest.mark.parametrize("N", [1, 63, 65, 499, 937])
def test_attention_shapes_f16(lib, N):
    T._attention_case(lib, 1, 2, N, None, 1, seed=N)


def test_attention_ragged_mask_f16(lib):
    T._attention_case(lib, 3, 2, 200, [200, 130, 1], 1, seed=7)


def test_attention_large_grid_f16(lib):
    """>= 1024 workgroups: the 256-query kernel with two query blocks per wave"""
    T._attention_case(lib, 8, 16, 937, None, 1, seed=11)


def test_attention_softmax_spike_f16(lib):
    T.test_attention_softmax_spike(lib)
    T.test_attention_softmax_spike(lib, hp=0)


@pytest.mark.parametrize("N", [1, 33, 64, 65, 130, 257, 320, 499, 937])
def test_attention_pipelined_v2p_shapes_f16(lib, N):
    T.test_attention_pipelined_v2p_shapes(lib, N)


def test_attention_pipelined_v2p_ragged_and_spikes_f16(lib):
    T.test_attention_pipelined_v2p_ragged_and_spikes(lib)


def test_attention_pipelined_v2p_large_grid_f16(lib):
    T.test_attention_pipelined_v2p_large_grid_matches_v2f(lib)


@pytest.mark.parametrize("tile", [4, 13, 14])
def test_transposed_qkv_tiles_race_screen_f16(lib, tile):
    T.test_transposed_qkv_tiles_race_screen(lib, tile)


@pytest.mark.parametrize("tps", [0, 1, 2])
@pytest.mark.parametrize("B,N,C", [(2, 130, 256), (1, 937, 1024)])
def test_convpos_f16(lib, B, N, C, tps):
    T.test_convpos(lib, B, N, C, 31, 1, tps)


@pytest.mark.parametrize("rows,dim", [(5, 512), (937, 1024)])
def test_ln_modulate_f16(lib, rows, dim):
    T.test_ln_modulate(lib, rows, dim)


def test_dwconv_ln_f16(lib):
    T.test_dwconv_ln(lib, 2, 100, 512)


@pytest.mark.parametrize("tile", [0, 2, 10])
def test_gemm_resid_gate_fused_ln_f16(lib, tile):
    T.test_gemm_resid_gate_fused_ln_is_bit_identical(lib, tile, 1)


@pytest.mark.parametrize("tile", [0, 4, 8, 10])
def test_gemm_resid_gate_f16(lib, tile):
    T.test_gemm_resid_gate(lib, tile, 1)


@pytest.mark.parametrize("tile", [1, 2, 3, 5, 6])
def test_gemm_small_tile_kernels_f16(lib, tile):
    T.test_gemm_all_small_tile_kernels(lib, tile)


def test_fp16_producers_saturate(lib):
    """|x| > 65504 must come out as +-65504, not inf (csrc/op16.hpp f5_sat): LN-modulate with a huge scale."""
    rows, dim = 4, 256
    r = rng(5)
    x = randn(r, rows, dim)
    sc = torch.full((dim,), 1.0e6)
    sh = torch.zeros(dim)
    hi = torch.zeros((rows, dim), dtype=torch.float16, device=DEV)
    xd, scd, shd = x.to(DEV), sc.to(DEV), sh.to(DEV)
    E.check(lib.f5_op_ln_modulate(P(xd), P(scd), P(shd), P(hi), P(None), rows, dim, stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(hi).all() and float(hi.abs().max()) == 65504.0


@pytest.mark.parametrize("tile", [0, 14])
def test_gemm_rs128_several_rounds_all_epilogues_f16(lib, tile):
    T.test_gemm_rs128_several_rounds_all_epilogues(lib, tile)


@pytest.mark.parametrize("tile", [4, 14, "small"])
@pytest.mark.parametrize("stress", range(len(T.FOLD_STRESS)))
def test_ln_modulate_folded_into_the_gemms_around_it_f16(lib, tile, stress):
    T.test_ln_modulate_folded_into_the_gemms_around_it(lib, tile, stress)


force_v2 = T.force_v2


@pytest.mark.parametrize("tile", [8, 9, 10, 11])
def test_gemm_ring8_kernels_f16(lib, tile):
    T.test_gemm_ring8_kernels(lib, tile)


@pytest.mark.parametrize("tile", [12, 13])
def test_gemm_wide_ring_kernels_f16(lib, tile):
    T.test_gemm_wide_ring_kernels(lib, tile)


@pytest.mark.parametrize("tile", [0, 1, 2, 4, 5])
@pytest.mark.parametrize("nseg", [1, 3])
def test_gemm_addrows_f16(lib, tile, nseg):
    T.test_gemm_addrows(lib, tile, nseg)


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 512, 128), (1000, 256, 192), (1874, 1024, 1024), (700, 768, 2048)])
def test_gemm_v2_f32_out_f16(lib, force_v2, M, N, K):
    T.test_gemm_v2_f32_out(lib, None, M, N, K)


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("epi", [1, 2, 8])
def test_gemm_v2_16bit_epilogues_transposed_tile_f16(lib, force_v2, epi, nseg):
    """incl. the only op-level run of EPI_GELU_ERF_BF16 (the Vocos epilogue) on this kernel"""
    T.test_gemm_v2_16bit_epilogues_transposed_tile(lib, None, epi, nseg)


def test_gemm_v2_band_major_tile_numbering_f16(lib, force_v2):
    T.test_gemm_v2_band_major_tile_numbering(lib, None)


@pytest.mark.parametrize("tile", [0, 5, 9, 10])
def test_gemm_ring_band_major_numbering_same_bits_f16(lib, tile):
    T.test_gemm_ring_band_major_numbering_same_bits(lib, tile)


@pytest.mark.parametrize("nseg", [1, 3])
def test_qkv_transposed_tiles_256_kernel_f16(lib, force_v2, nseg):
    T.test_qkv_transposed_tiles_256_kernel(lib, None, nseg)


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("tile", [9, 12, 13, "knob12", "knob13"])
def test_qkv_transposed_wave_tiles_ring8_f16(lib, tile, nseg):
    T.test_qkv_transposed_wave_tiles_ring8(lib, tile, nseg)


@pytest.mark.parametrize("nseg", [1, 3])
def test_attention_path_with_v2_qkv_f16(lib, force_v2, nseg):
    T.test_attention_path_with_v2_qkv(lib, None, nseg)


@pytest.mark.parametrize("ks", [1, 2, 4])
def test_attention_kv_split_f16(lib, ks):
    T.test_attention_kv_split(lib, ks)


@pytest.mark.parametrize("premul", [False, True])
@pytest.mark.parametrize("path", ["wide", "split2", "split4", "auto"])
def test_attention_without_tile_maximum_f16(lib, path, premul):
    T.test_attention_without_tile_maximum(lib, path, premul)


def test_attention_wide_workgroups_f16(lib):
    T.test_attention_wide_workgroups(lib)


@pytest.mark.parametrize("B,N,dim", [(1, 31, 256), (3, 100, 1024)])
def test_grn_f16(lib, B, N, dim):
    T.test_grn(lib, B, N, dim)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("tile", [0, 4, 14])
def test_fp16_range_detector_on_every_packer(lib, tile):
    """VERDICT r5 weak #1 / "next" #2: f5_sat clamps silently, so every producer of a 16-bit MFMA operand also REPORTS a value beyond
    +-65 504 (op16.hpp f5_sat_commit -> F5_STATUS_SATURATED = 4 in the word f5_debug_set_op_sat_flag points to; in a sample() call that
    word is the status word of the workspace).  Each packer is run on ordinary data (the flag must stay 0) and with ONE outlier that
    lands beyond the range (the flag must come back 4, the output finite): LN-modulate, the 16-bit GEMM epilogues -- plain, GELU --,
    QKV behind the rotation (q, k and the transposed V tiles separately), conv-pos, on the small-tile (0 = auto at these sizes), the
    256 x 256 (4) and the role-split 128 x 256 (14) kernels."""
    import ctypes as C
    r = rng(321 + tile)
    flag = _flag()

    def run(what, fn, expect):
        flag.zero_()
        E.check(lib.f5_debug_set_op_sat_flag(P(flag)))
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            E.check(lib.f5_debug_set_op_sat_flag(P(None)))
        got = int(flag.item())
        assert got == expect, (what, got, expect)
        for o in out:
            assert torch.isfinite(o.float()).all(), what
        return out

    # ---- LN-modulate (h: the A operand of QKV / FF1 wherever the LN fold is off, i.e. always at batch 1)
    rows, dim = 300, 1024
    x = randn(r, rows, dim).to(DEV)
    sh = randn(r, dim, scale=0.1).to(DEV)
    for big in (False, True):
        sc = randn(r, dim, scale=0.1)
        if big:
            sc[517] = 1.0e6                                   # one massive modulation channel
        scd = sc.to(DEV)
        hi = torch.zeros((rows, dim), dtype=torch.float16, device=DEV)
        run(f"ln_modulate big={big}", lambda: (E.check(lib.f5_op_ln_modulate(P(x), P(scd), P(sh), P(hi), P(None), rows, dim, stream())), hi)[1:],
            4 if big else 0)

    # ---- 16-bit GEMM epilogues + QKV: M rows so that the forced large kernels have whole tiles, one weight row scaled up
    E.check(lib.f5_debug_set_gemm_tile(tile))
    try:
        B, n, D, FF, H = (8, 937, 1024, 2048, 16) if tile else (2, 300, 1024, 2048, 16)
        M = B * n
        npad = (n + 63) // 64 * 64
        a_hi, _ = split_bf16(randn(r, M, D).to(DEV))
        for epi in (1, 2):
            for big in (False, True):
                w1 = randn(r, FF, D, scale=D ** -0.5)
                if big:
                    w1[1234] *= 1.0e5                          # one output channel: |acc| ~ 1e5 > 65 504 (positive half survives the GELU)
                w1_hi, _ = split_bf16(w1.to(DEV))
                b1 = randn(r, FF, scale=0.1).to(DEV)
                out16 = torch.zeros((M, FF), dtype=torch.float16, device=DEV)
                run(f"gemm epi={epi} big={big} tile={tile}",
                    lambda: (E.check(lib.f5_op_gemm(P(a_hi), P(None), P(w1_hi), P(None), P(b1), P(None), P(out16), P(None), M, FF, D, D, D, FF, 1, epi,
                                                    stream()), "gemm"), out16)[1:], 4 if big else 0)
                if big:
                    assert float(out16.float().abs().max()) == 65504.0
        cos_t, sin_t = torch.empty(n, 32, device=DEV), torch.empty(n, 32, device=DEV)
        E.check(lib.f5_op_rope_table(P(cos_t), P(sin_t), n, 64, stream()))
        tt = [torch.empty(64 * n, device=DEV) for _ in range(2)]
        E.check(lib.f5_op_rope_table_g4(P(tt[0]), P(tt[1]), n, 64, C.c_float(1.0), stream()))
        E.check(lib.f5_debug_set_op_rope_tables_g4(P(tt[0]), P(tt[1])))
        try:
            for which, row in (("clean", None), ("q", 100), ("k", D + 77), ("v", 2 * D + 515)):
                w = randn(r, 3 * D, D, scale=D ** -0.5)
                if row is not None:
                    w[row] *= 1.0e5
                w_hi, _ = split_bf16(w.to(DEV))
                bias = randn(r, 3 * D, scale=0.1).to(DEV)
                qk = torch.zeros(M, 2 * D, dtype=torch.float16, device=DEV)
                vt = torch.zeros(B * H, 64, npad, dtype=torch.float16, device=DEV)
                run(f"qkv {which} tile={tile}",
                    lambda: (E.check(lib.f5_op_qkv_rope(P(a_hi), P(None), P(w_hi), P(None), P(bias), P(cos_t), P(sin_t), P(qk), P(None), P(vt), P(None),
                                                        B, n, npad, H, D, 1, stream()), "qkv_rope"), qk, vt)[1:], 0 if row is None else 4)
        finally:
            E.check(lib.f5_debug_set_op_rope_tables_g4(P(None), P(None)))
    finally:
        E.check(lib.f5_debug_set_gemm_tile(0))

    # ---- conv-pos (mode 0: the 16-bit intermediate between the two convolutions)
    if tile == 0:
        Bc, Nc, Cc, G, taps = 1, 200, 256, 4, 31
        for big in (False, True):
            xw = randn(r, Bc * Nc, Cc)
            ww = randn(r, Cc, taps * 64, scale=(taps * 64) ** -0.5)
            if big:
                ww[33] *= 3.0e5
            x_hi, _ = split_bf16(xw.to(DEV))
            w_hi, _ = split_bf16(ww.to(DEV))
            bias_d = randn(r, Cc, scale=0.1).to(DEV)
            out = torch.zeros(Bc * Nc, Cc, dtype=torch.float16, device=DEV)
            run(f"convpos big={big}",
                lambda: (E.check(lib.f5_op_convpos(P(x_hi), P(None), P(w_hi), P(None), P(bias_d), P(out), P(None), P(None), Bc, Nc, Cc, G, taps, 1, 0,
                                                   stream()), "convpos"), out)[1:], 4 if big else 0)
