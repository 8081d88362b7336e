"""The GEMM matrix harness tested on the CPU: the generator (count, ABI constraints of csrc/gemm.hpp, no duplicates), and the checker
(guards, poison, tolerances) over a torch emulation of GEMM + epilogue -- a right one must pass, and ten deliberately wrong ones must
each be flagged.  That is what shows that tests/test_gemm_matrix_gpu.py would fail on a subtly wrong kernel; no GPU is involved."""
import collections

import pytest
import torch

import gemm_matrix as GM

CASES = GM.cases()


def test_generator_count_and_uniqueness():
    per_sel = {s: len(GM.shape_classes(s)[0]) * len(GM.shape_classes(s)[1]) * len(GM.KS) for s in GM.SELECTORS}
    assert [per_sel[s] for s in GM.SELECTORS] == [80, 80, 80, 80, 24, 80, 80, 40, 40, 80, 80, 40, 40, 40]
    extra = 2 * 5 * 2 * 2 + 1                       # ring off: selectors 2 and 3, 5 M x 2 N x 2 K; the 528-tile shape of selector 2
    want = len(GM.OPS) * len(GM.EPIS) * 2 * (sum(per_sel.values()) + extra)
    assert len(CASES) == want == 28960
    assert len(set(CASES)) == len(CASES) and len({c.id for c in CASES}) == len(CASES)
    # nothing dropped: every operand type x selector x epilogue x nseg is there, with every K
    combos = collections.Counter((c.op, c.sel, c.epi, c.nseg) for c in CASES)
    assert len(combos) == 2 * 14 * 8 * 2
    assert {c.K for c in CASES} == set(GM.KS)


def test_every_case_obeys_the_abi():
    for c in CASES:
        assert c.M >= 1 and c.N >= 1 and c.K % 64 == 0 and c.nseg in (1, 3)
        assert c.lda % 8 == 0 and c.ldw % 8 == 0 and c.lda > c.K and c.ldw > c.K and c.ldo > c.N       # never the tight ones
        if c.epi in GM.OUT16 or c.epi == "ADDROWS":
            assert c.ldo % 8 == 0                   # 16-byte rows for the staged 16-bit stores
        if c.N >= 64:
            assert (c.ldo * 4) % 16 == 0
        assert (c.a_row_mod > 0) == (c.epi == "ADDROWS") and c.a_row_mod <= c.M
        k = c.kernel
        assert k is not None, c.id                  # every case of the matrix is a legal request
        if c.sel == 4:
            assert c.M >= 256 and c.N % 256 == 0 and k == "gemm256"
        if c.sel in (12, 13, 14):
            assert c.N % 256 == 0
        if c.sel in (1, 5, 6, 10, 11):
            assert k == {1: "cfg<2,2>", 5: "ring<1,2>", 6: "ring<1,1>", 10: "ring_ks2<1>", 11: "ring_ks2<2>"}[c.sel]
        # operands far below the 2 GiB the kernels' 32-bit byte offsets allow
        assert max(c.M, 1) * c.lda < 2 ** 24 and (c.N + 256) * c.ldw < 2 ** 24


def test_known_silent_fallbacks_are_named():
    """a forced selector that the dispatcher does not honour is recorded under the kernel it actually reaches"""
    assert GM.expected_kernel(14, "ADDROWS", 300, 256) == "ring<1,1>"
    assert GM.expected_kernel(14, "RESID_GATE", 300, 256) == "rs128"
    assert GM.expected_kernel(12, "RESID_GATE", 300, 256) == "ring<1,1>"
    assert GM.expected_kernel(12, "BF16", 300, 256) == "ring_wide<2,2,2,4>"
    assert GM.expected_kernel(8, "F32", 300, 256) == "ring<1,1>" and GM.expected_kernel(8, "F32", 300, 384) == "ring8<3>"
    assert GM.expected_kernel(4, "F32", 100, 256) is None and GM.expected_kernel(4, "F32", 300, 100) is None
    # the auto rule at the production shapes f5_gemm_route's comments name (M = 2 x 937 per batch element)
    assert GM.expected_kernel(0, "GELU_TANH", 1874, 2048) == "ring8<2>"
    assert GM.expected_kernel(0, "RESID_GATE", 1874, 1024) == "ring_ks2<1>"
    assert GM.expected_kernel(0, "ADDROWS", 1874, 1024) == "ring_ks2<1>"
    assert GM.expected_kernel(0, "F32", 14992, 100) == "ring_ks2<1>"
    assert GM.expected_kernel(0, "RESID_GATE", 14992, 1024) == "rs128"
    assert GM.expected_kernel(0, "RESID_GATE", 59968, 1024) == "gemm256"
    assert GM.expected_kernel(2, "F32", 2100, 2048) == "cfg<1,2>"


SLICE = CASES[::23]


def test_checker_passes_a_right_emulation():
    assert len(SLICE) > 1200
    seen = set()
    for c in SLICE:
        b = GM.make_buffers(c)
        GM.emulate(b)
        bad = GM.check(b)
        assert not bad, (c.id, bad)
        seen.add((c.op, c.epi, c.nseg))
    assert len(seen) == 2 * 8 * 2


def test_untouched_buffers_are_flagged():
    """a launch that writes nothing leaves the sentinel in the interior: not a pass"""
    for c in SLICE[::97]:
        b = GM.make_buffers(c)
        if c.epi == "RESID_GATE" and not bool(b["keep"].any()):
            continue                                # every row masked: x stays as it is, rightly
        assert GM.check(b), c.id


@pytest.mark.parametrize("fault", GM.FAULTS)
def test_checker_flags_a_wrong_emulation(fault):
    hit = collections.Counter()
    for c in CASES[::7]:
        key = (c.op, c.epi, c.nseg)
        if hit[key] >= 3 or c.K > 192 or not GM.fault_applies(fault, c):
            continue
        b = GM.make_buffers(c)
        GM.emulate(b, fault)
        bad = GM.check(b)
        assert bad, f"{fault} went unnoticed in {c.id}"
        hit[key] += 1
    # the fault was tried in every operand type it can occur in
    ops = {k[0] for k in hit}
    assert ops == ({"f16"} if fault == "f16_through_bf16" else {"bf16", "f16"}) and sum(hit.values()) >= 6, hit


def test_one_rounding_meets_the_16_bit_bound_and_two_do_not():
    """eps_op is the bound of ONE round-to-nearest: values rounded once meet it without any floor; values rounded through a coarser
    type first, or truncated, do not"""
    g = torch.Generator().manual_seed(1)
    v = (torch.randn(200000, generator=g, dtype=torch.float64) * 3).float()
    for op in GM.OPS:
        once = GM._round_op(v, op).double()
        assert bool(((once - v.double()).abs() <= GM.eps_op(op) * v.double().abs() + 2.0 ** -25).all())      # (fp16 subnormals: spacing 2^-24)
        trunc = GM._truncate(v.clone(), op).double()
        assert bool(((trunc - v.double()).abs() > GM.eps_op(op) * v.double().abs()).any())
    twice = v.to(torch.bfloat16).float().to(torch.float16).double()
    assert bool(((twice - v.double()).abs() > GM.eps_op("f16") * v.double().abs()).any())
