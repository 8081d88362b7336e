"""The row-op test matrix tested on the CPU: a correct torch emulation of every op passes every checker of tests/rowops_matrix.py under
both operand types, and each deliberately wrong emulation -- the mistakes a row kernel can make without crashing -- is flagged by at
least one case of every op it applies to.  What tests/test_rowops_matrix_gpu.py asserts about the kernels is only worth what this
module shows about the harness."""
import pytest
import torch

import rowops_matrix as RM

CASES = {op: RM.cases(op) for op in RM.OPS}
PACKERS = [op for op in RM.OPS if RM.OPS[op]["packs"]]
TRACKED = [op for op in RM.OPS if RM.OPS[op]["tracked"]]
LN_OPS = ["ln_modulate", "layernorm", "dwconv_ln"]

# mistake -> the ops whose emulation can make it
WRONG = {
    "conv_across_batch": ["dwconv_ln"],                       # depthwise conv that reads across the batch boundary
    "conv_pad_off_by_one": ["dwconv_ln"],
    "no_eps": LN_OPS,                                         # variance without eps: the constant row
    "var_about_0": LN_OPS,                                    # variance taken about 0: the mean-1000 row
    "nv3_as_4": LN_OPS,                                       # NV = 3 treated as 4
    "grn_drops_last_chunk": ["grn"],
    "grn_wrong_count": ["grn"],                               # Gx averaged over the 256-padded channel count
    "keep_after_drop": ["text_embed"],
    "keep_ignores_nomask": ["text_embed"],                    # mask_padding = 0 ignored
    "pos_not_clamped": ["text_embed"],
    "pad_not_zero": ["pack_x", "im2col7"],
    "cond_mask_le": ["pack_cond_text"],
    "null_keeps_cond_ignored": ["pack_cond_text"],
    "rk4_weights_1111": ["ode_stage"],
    "cfg_wrong_sign": ["ode_stage"],
    "lens_of_wrong_batch": ["splice", "rowkeep"],
    "copy_loses_tail": ["copy_words", "stage_words"],
    "mean_over_all_rows": ["duration_head"],                  # masked mean divided by the sequence length
    "skinny_drops_bias": ["skinny_gemm"],
    "skinny_k_tail": ["skinny_gemm"],                         # K loop in steps of 16: K = 8 and 264 lose their last 8
    "skinny_row_clamp": ["skinny_gemm"],                      # MBLK one short: rows 96 ... 127 of a pass repeat row 95
    "halves_swapped": ["time_sinus", "text_pos_table"],       # [cos | sin] for [sin | cos] and the other way round
    "g4_interleaved": ["rope_tables"],                        # wrong order inside a group of the group-major table
    "q_table_unscaled": ["rope_tables"],
    "pad_off_by_one": ["zero_vt_pad"],                        # the first pad column keeps its old value
    "col0_ignored": ["pack_bf16"],
    "ld_ignored": ["pack_bf16"],
    "guard_front": list(RM.OPS),                              # one element written into a guard band
    "guard_back": list(RM.OPS),
    "one_off": list(RM.OPS),                                  # one output element wrong (one bit where the op is exact)
    "hi_truncated": PACKERS,                                  # hi truncated instead of rounded
    "f16_inf": PACKERS,                                       # fp16 overflow to inf instead of the clamp
    "no_flag": TRACKED,                                       # a saturation that does not raise the flag
}
F16_ONLY = ("f16_inf", "no_flag")


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    """thousands of tiny tensors: the thread pool only gets in the way"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def findings(c, op16, bug=None):
    io = RM.build(c, op16)
    RM.host_backend(bug)(io)
    return RM.check(io)


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("op", list(RM.OPS))
def test_correct_emulation_passes_every_checker(op, op16):
    bad = [b for c in CASES[op] for b in findings(c, op16)]
    assert not bad, "\n".join(bad[:20])


def _probe_cases(op, bug):
    """every case of the small ops; of the 16 MB copy only what a mistake of the copy itself needs"""
    cs = CASES[op]
    if op == "copy_words" and bug != "copy_loses_tail":
        cs = [c for c in cs if c.nwords < RM.COPY_BIG]
    # the cases made for a mistake come first (the probe stops at the first case that notices)
    return sorted(cs, key=lambda c: not (c.kw.get("outlier") or c.kw.get("stress") or c.kw.get("dim") == 768))


@pytest.mark.parametrize("bug,op", [(b, op) for b, ops in WRONG.items() for op in ops])
def test_wrong_emulation_is_flagged(bug, op):
    flagged = {}
    for op16 in (("f16",) if bug in F16_ONLY else RM.OPS16):
        flagged[op16] = next((c.id for c in _probe_cases(op, bug) if findings(c, op16, bug)), None)      # the first case that notices
    print(f"[rowops harness] {bug} in {op}: flagged by {flagged}")
    assert all(flagged.values()), flagged


def test_every_wrong_kernel_of_the_list_is_probed():
    assert len(WRONG) == 33
    for op in RM.OPS:
        assert any(op in ops for ops in WRONG.values()), op


def test_reference_packer_is_the_suite_packer():
    """rowops_matrix.split (which must not import the library) is f5test.split_bf16 under either operand mode: the two copies of the
    packer reference stay in step, and under fp16 both halves stay finite"""
    import f5test
    x = torch.cat([torch.randn(4096) * 3, torch.tensor([0.0, 1e-7, 65504.0, 65519.9, 65520.0, 1e5, -1e5, 3e5, -3e5, 1e-30])])
    for op16 in RM.OPS16:
        with f5test.operand_mode(op16):
            hi, lo = f5test.split_bf16(x)
        wh, wl = RM.split(x, op16)
        assert torch.equal(RM.bits(hi), RM.bits(wh)) and torch.equal(RM.bits(lo), RM.bits(wl)), op16
        if op16 == "f16":
            assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()


def test_generators_reach_every_op_and_instantiation():
    for op in RM.OPS:
        assert len(CASES[op]) > 0, op
        assert len({c.id for c in CASES[op]}) == len(CASES[op]), f"{op}: duplicate case ids"
    counts = RM.instantiation_counts()
    assert set(RM.CLAIMED) <= set(counts)
    assert all(counts[k] > 0 for k in RM.CLAIMED), {k: v for k, v in counts.items() if v == 0}
    print("[rowops harness] cases per op:", {op: len(CASES[op]) for op in RM.OPS}, "per instantiation:", counts)


def test_axes_of_the_matrix():
    """the shapes at which the kernels take another path are in the lists"""
    sk = CASES["skinny_gemm"]
    assert {m for c in sk for m in RM.skinny_mblks(c.M)} == {1, 2, 3, 4}
    assert {c.M for c in sk} >= {1, 32, 33, 128, 129, 257} and {c.N for c in sk} >= {1, 31, 32, 33, 129} and {c.K for c in sk} == {8, 16, 264}
    assert {c.dim for c in CASES["grn"]} >= {4, 100, 260, 1536} and {c.N for c in CASES["grn"]} >= {32, 33, 64, 65}
    assert {c.nwords for c in CASES["copy_words"]} >= {1, 3, 4, 5, 1023, 4 * 256 * 4096 + 7}
    assert {c.nwords for c in CASES["stage_words"]} == {1, 959, 960, 961, 2000}
    assert {(c.B, c.N) for c in CASES["dwconv_ln"]} >= {(1, 1), (1, 2), (1, 3), (3, 4), (2, 7), (3, 37)}
    assert len({(c.f32, c.hi, c.lo) for c in CASES["layernorm"]}) == 7
    for op in RM.PACKS_WITH_LO:
        assert {c.lo for c in CASES[op]} == {0, 1}, op
