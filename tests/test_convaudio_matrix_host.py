"""The conv-pos / audio / noise test matrix tested on the CPU: a correct emulation of every op passes every checker of
tests/convaudio_matrix.py (under both operand types where the op has 16-bit operands), and each deliberately wrong emulation -- the
mistakes these kernels can make without crashing -- is flagged by at least one case of the op it belongs to.  What
tests/test_convaudio_matrix_gpu.py asserts about the kernels is only worth what this module shows about the harness."""
import zlib

import numpy as np
import pytest

import convaudio_matrix as CM

CASES = {op: CM.cases(op) for op in CM.OPS}

# mistake -> the ops whose emulation can make it
WRONG = {
    "conv_across_batch": ["convpos"],                         # zero padding at the ends of the batch only
    "pad_off_by_one": ["convpos"],
    "last_tap_dropped": ["convpos"],                          # the partial last pipeline step loses its tap
    "clamped_slab_used": ["convpos"],                         # tap taps - 1 counted twice
    "group_of_wrong_xcd": ["convpos"],                        # 1-D block decode with nx in place of nx * B
    "one_group_as_1d": ["convpos"],                           # one group, one batch element: the 3-D grid decoded as the 1-D one
    "tail_rows_written": ["convpos"],                         # rows >= seq_len of the last tile stored
    "mode1_overwrites": ["convpos"],
    "bias_of_group_0": ["convpos"],
    "lo_terms_dropped": ["convpos"],                          # nseg 3 run on the hi halves alone
    "mish_unclamped": ["convpos"],                            # NaN beyond 88
    "no_centre_pad": ["mel"],
    "symmetric_window": ["mel"],
    "last_frame_kept": ["mel"],
    "no_log_floor": ["mel"],
    "batch_stride_wrong": ["mel"],                            # rows frames * hop apart instead of L
    "mel_loop_stops_at_256": ["mel"],
    "nyquist_imag_kept": ["istft"],
    "no_clip": ["istft"],
    "conj_sign": ["istft"],
    "envelope_of_full_overlap": ["istft"],                    # edges divided by the interior envelope
    "trim_off_by_hop": ["istft"],
    "ola_reads_next_row": ["istft"],
    "ldx_ignored": ["istft"],
    "frame_major_draw": ["noise"],
    "odd_pair_dropped": ["noise"],
    "pad_not_zero": ["noise"],                                # the zero fill without its stride
    "seed_halves_swapped": ["noise"],
    "dur_of_wrong_batch": ["noise"],
    "no_upper_clamp": ["noise_bits"],                         # inf at 0xFFFFFFFF
    "fma_in_uniform": ["noise_bits"],
    "guard_front": list(CM.OPS),
    "guard_back": list(CM.OPS),
    "one_off": list(CM.OPS),
    "hi_truncated": ["convpos"],                              # mode 0: hi truncated instead of rounded
    "f16_inf": ["convpos"],                                   # fp16 overflow to inf instead of the clamp
    "no_flag": ["convpos"],                                   # a saturation that does not raise the flag
}
F16_ONLY = ("f16_inf", "no_flag")


def findings(c, op16, bug=None):
    io = CM.build(c, op16)
    CM.host_backend(bug)(io)
    return CM.check(io)


@pytest.mark.parametrize("op,op16", [(op, t) for op in CM.OPS for t in CM.op_types(op)])
def test_correct_emulation_passes_every_checker(op, op16):
    CM.pool_reset(op)
    bad = [b for c in CASES[op] for b in findings(c, op16)]
    if op in CM.POOLED:
        bad += CM.pool_findings(op)
    assert not bad, "\n".join(bad[:20])
    if op != "convpos":
        print(f"[convaudio harness] {op}: worst |err| / bound per case:", {k[0]: round(v, 4) for k, v in CM.WORST.items() if k[0].startswith(op + "[")})


def _probe_cases(op, bug):
    """the cases made for a mistake, and the small ones, come first (the probe stops at the first case that notices)"""
    cs = CASES[op]
    if op == "convpos":
        made_for = {"mish_unclamped": "mish", "f16_inf": "outlier", "no_flag": "outlier", "conv_across_batch": "neighbours"}.get(bug)
        cs = sorted(cs, key=lambda c: (c.var != made_for, c.B * c.N * c.C * c.taps))
    return cs


@pytest.mark.parametrize("bug,op", [(b, op) for b, ops in WRONG.items() for op in ops])
def test_wrong_emulation_is_flagged(bug, op):
    flagged = {}
    types = [t for t in CM.op_types(op) if not (bug in F16_ONLY and t != "f16")]
    for op16 in types:
        CM.pool_reset(op)
        flagged[op16] = next((c.id for c in _probe_cases(op, bug) if findings(c, op16, bug)), None)      # the first case that notices
        if flagged[op16] is None and op in CM.POOLED and CM.pool_findings(op):
            flagged[op16] = "the pooled bit-equal share"
    print(f"[convaudio harness] {bug} in {op}: flagged by {flagged}")
    assert flagged and all(flagged.values()), flagged


def test_every_wrong_kernel_of_the_list_is_probed():
    assert len(WRONG) == 37
    assert sum(len(ops) for ops in WRONG.values()) == 31 + 3 * len(CM.OPS) + 3
    for op in CM.OPS:
        assert any(op in ops for ops in WRONG.values()), op


def test_axes_of_the_convpos_cases():
    cs = CASES["convpos"]
    assert len({c.id for c in cs}) == len(cs) and 200 <= len(cs) <= 400, len(cs)
    assert {c.C for c in cs} == set(CM.CP_C) and {c.N for c in cs} >= set(CM.CP_N) and {c.taps for c in cs} == set(CM.CP_TAPS)
    assert max(c.B * c.N * c.C for c in cs) <= 3 * 257 * 1024
    for name, vals in (("B", {1, 2, 3}), ("nseg", {1, 3}), ("tps", {0, 1, 2, 4}), ("xcd", {0, 1}), ("mode", {0, 1})):
        assert {c.kw[name] for c in cs} == vals, name
    assert {c.lo for c in cs if c.mode == 0} == {0, 1}
    # every channel count meets every token count; B > 1 at C = 512 and 1024 under both numberings
    assert {(c.C, c.N) for c in cs} >= {(C, N) for C in CM.CP_C for N in CM.CP_N}
    for C in (512, 1024):
        assert {(c.xcd, c.B > 1) for c in cs if c.C == C} >= {(0, True), (1, True)}, C
    # every instantiation under both numberings, from the names the hook is to report; the tps = 4, nseg = 3 selector runs <true,2>
    assert {CM.convpos_kernel_name(c) for c in cs} == set(CM.CP_NAMES)
    assert {CM.convpos_kernel_name(c) for c in cs if c.tps == 4 and c.nseg == 3} == {"f5_convpos_kernel<true,2>", "f5_convpos_kernel<true,2>+xcd"}
    # partial last steps at every tap count, one tap included
    assert {(c.taps, c.tps) for c in cs} >= {(t, s) for t in (1, 3, 5, 29, 31) for s in (2, 4)}
    assert {c.var for c in cs} == {"normal", "neighbours", "mish", "outlier"}
    # the groups whose members must agree bit for bit compare both numberings and all selectors somewhere
    groups = {}
    for c in cs:
        groups.setdefault(CM.convpos_group(c), set()).add((c.tps, c.xcd))
    assert sum(len(v) == 8 for v in groups.values()) >= 8


def test_axes_of_the_audio_and_noise_cases():
    mel = CASES["mel"]
    assert {c.hop for c in mel} == {256, 100} and {c.n_mels for c in mel} == {1, 100, 257} and {c.B for c in mel} == {1, 3}
    for hop in (256, 100):
        assert {c.L for c in mel if c.hop == hop} >= {hop - 1, hop, 3 * hop + 17, 1025}
    assert {c.sig for c in mel} == set(CM.MEL_SIGS)
    ist = CASES["istft"]
    assert {c.nframes for c in ist} == {1, 2, 3, 4, 5, 6, 37} and {c.B for c in ist} == {1, 3} and {c.ldx for c in ist} == {1026, 1032, 1280}
    assert {c.hop for c in ist} == {128, 256, 512} and {c.entry for c in ist} == {"plain", "batch"} and {c.var for c in ist} == set(CM.IST_VARS)
    assert {(c.nframes, c.var) for c in ist} >= {(n, v) for n in (1, 2, 37) for v in CM.IST_VARS}
    noise = {c.name: c for c in CASES["noise"]}
    assert noise["dur1_small"].N * noise["dur1_small"].mel < 4096 < noise["dur1_large"].N * noise["dur1_large"].mel
    assert noise["B256"].B == 256 and noise["B257_refused"].B == 257 and sum(c.refuse for c in noise.values()) == 3
    assert any((c.mel * d) % 2 for c in noise.values() for d in c.durs)
    b = np.concatenate([CM.noise_bit_patterns(c.which) for c in CASES["noise_bits"]])
    assert set(CM.NB_NAMED) <= set(b.tolist()) and len(set(b.tolist())) >= 3 * 65536
    assert set(range(65536)) <= set(b.tolist()) and set(range(2 ** 32 - 65536, 2 ** 32)) <= set(b.tolist())
    for op in CM.OPS:
        assert len({c.id for c in CASES[op]}) == len(CASES[op]), op
    print("[convaudio harness] cases per op:", {op: len(CASES[op]) for op in CM.OPS})


def test_the_fft_bound_has_room_for_the_kernel_and_none_for_a_wrong_bin():
    """the derived relative bound of the 1024-point transform: about 1e-5, against 3e-7 of an fp32 emulation of the same radix-2
    algorithm and O(1) of a wrong bin"""
    assert 5e-6 < CM.FFT_REL < 2e-5


def test_mlx_like_normal_keeps_its_bits():
    """rng.bits_to_normal was factored out of rng.mlx_like_normal: the draws are those of the commit before (first values and a
    checksum of a (7, 13) draw, computed there)"""
    from f5_tts_mlx_amd.rng import mlx_like_normal
    pinned = {0: ([1062559246, 1051663194, 1068609603, 3198077039], 1459647026),
              3: ([1056348988, 3212369652, 1057674348, 3208952488], 3572482877),
              2 ** 40 + 7: ([1052762784, 1070874196, 3219311339, 1069831193], 3410870542),
              2 ** 63 - 1: ([3211150568, 3204978095, 3197809734, 1073948789], 2673578003)}
    for seed, (head, crc) in pinned.items():
        a = mlx_like_normal(seed, (7, 13))
        assert a.dtype == np.float32 and a.shape == (7, 13)
        assert a.reshape(-1)[:4].view(np.uint32).tolist() == head and zlib.crc32(a.tobytes()) == crc, seed
