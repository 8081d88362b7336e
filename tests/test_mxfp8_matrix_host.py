"""tests/mxfp8_matrix.py on the CPU: the case set covers what it claims, every case lies inside what the launchers enforce, the checker
passes a correct emulation of the kernels and flags every seeded mistake.  Needs no GPU and no library."""
import pytest
import torch

import mxfp8_matrix as X

CASES = X.cases()
SLICE = X.host_slice(CASES)
GEMM = [c for c in CASES if c.kind == "gemm"]


def test_case_count_and_ids():
    assert len(CASES) == 276 and len(GEMM) == 150, (len(CASES), len(GEMM))
    assert len({c.id for c in CASES}) == len(CASES)
    assert sum(c.kind == "qkv" for c in CASES) == 16 and sum(c.kind == "ln" for c in CASES) == 20
    assert sum(c.kind == "quant" for c in CASES) == 30 and sum(c.kind == "quant16" for c in CASES) == 60


def test_gemm_coverage():
    assert {c.M for c in GEMM} == set(X.MS) and {c.N for c in GEMM} == set(X.NS) and {c.K for c in GEMM} == set(X.KS)
    assert {c.T for c in GEMM} == {1, 2, 3, 4, 5}
    for T in range(1, 6):
        at = [c for c in GEMM if c.T == T]
        assert any(c.M < 256 for c in at), T
        assert any(c.M > 256 and c.M % 256 for c in at), T                       # a partial last row tile behind a full one
        assert {c.epi for c in at} == set(X.GEMM_EPIS), T                        # every epilogue at every K-tile count
        for values in X.VALUES:
            assert {c.epi for c in at if c.values == values} == set(X.epis_of(values)), (T, values)
    assert set(X.TILE_COUNTS) <= {c.ntiles for c in GEMM}
    # the XCD remap: fewer than 8 tiles, a multiple of 8, and q >= 1 with r != 0
    assert any(c.ntiles < 8 for c in GEMM) and any(c.ntiles % 8 == 0 for c in GEMM) and any(c.ntiles > 8 and c.ntiles % 8 for c in GEMM)
    for c in GEMM:
        assert (c.lda8, c.ldw8) == (c.K + 16, c.K + 32) and c.ldo > c.N


def test_qkv_coverage():
    q = [c for c in CASES if c.kind == "qkv"]
    assert {c.B for c in q} == {1, 2} and all(c.N == 3 * X.QKV_D and c.K == X.QKV_D and X.QKV_H * 64 == X.QKV_D for c in q)
    for c in q:
        assert c.npad in (X.ceil64(c.seq), X.ceil64(c.seq) + 64) and c.M == c.B * c.seq
        if c.B == 2:
            assert c.seq % 32 != 0 and c.seq % 4 != 0            # the seam inside a 32-row block (and inside a 4-row register group)
    for B in (1, 2):
        assert {(c.npad - X.ceil64(c.seq), c.qpre != 0) for c in q if c.B == B} == {(0, False), (0, True), (64, False), (64, True)}


def test_cases_lie_inside_what_the_launchers_enforce():
    """shapes, leading dimensions and the byte offset of every pointer behind its allocation (torch allocations start on 64 bytes or more)"""
    for c in CASES:
        if c.kind in ("gemm", "qkv"):
            assert c.M >= 1 and c.N % 256 == 0 and c.K % 128 == 0
            assert c.lda8 % 16 == 0 and c.ldw8 % 16 == 0 and c.lda8 >= c.K and c.ldw8 >= c.K
            assert (X.GUARD * c.lda8) % 16 == 0 and (X.GUARD * c.ldw8) % 16 == 0 and (X.GUARD * (c.K // 32)) % 4 == 0
        if c.kind == "gemm":
            assert c.ldo >= c.N
            if c.epi == "BF16":
                assert c.ldo % 8 == 0 and (X.GUARD * c.ldo * 2) % 16 == 0
            if c.epi == "GELU_TANH":
                assert c.ldo % 8 == 0 and (X.GUARD * c.ldo) % 8 == 0
            if c.epi.startswith("RESID") or c.epi == "F32":
                assert c.ldo % 4 == 0 and (X.GUARD * c.ldo * 4) % 16 == 0
        if c.kind == "qkv":
            assert c.ldo == 2 * X.QKV_D and c.npad >= c.seq and c.npad % 64 == 0 and c.M % c.seq == 0 and (c.B == 1 or c.seq >= 4)
        if c.kind in ("quant", "quant16"):
            assert c.N % 32 == 0 and c.lda8 % 4 == 0 and c.ldw8 % 4 == 0 and c.lda8 > c.N and c.ldw8 > c.N
            assert (X.GUARD * c.lda8 * (4 if c.kind == "quant" else 2)) % 16 == 0 and (X.GUARD * c.ldw8) % 4 == 0
        if c.kind == "ln":
            assert c.N in (256, 512, 768, 1024)


def test_buffers_are_poisoned_and_guarded():
    c = X.gemm_case("GELU_TANH", "gauss", 31, 256, 128)
    b = X.make_buffers(c)
    assert bool((b["a8"][:X.GUARD] == 0x7F).all() and (b["a8"][X.GUARD + c.M:] == 0x7F).all() and (b["a8"][:, c.K:] == 0x7F).all())
    assert bool((b["as"][:X.GUARD] == 0xFF).all() and (b["as"][X.GUARD + c.M:] == 0xFF).all())
    assert b["w8"].shape[0] == c.N + 2 * X.GUARD and bool((b["w8"][:, c.K:] == 0x7F).all())
    assert bool(torch.isnan(b["bias"][c.N:]).all())
    assert b["out8"].unwritten() == c.M * c.N and b["out8s"].unwritten() == c.M * c.N // 32
    assert bool(torch.isnan(b["out_bf"].alloc.float()).all()) and bool(torch.isnan(b["out_f32"].alloc).all())
    r = X.make_buffers(X.gemm_case("RESID_GATE", "gauss", 31, 256, 128))
    assert bool(torch.isfinite(r["out_f32"].alloc).all()) and float(r["out_f32"].alloc[0, 0]) == 14591765.0


def test_dequant_is_the_oracles():
    """the byte table of the matrix (it also decodes on the GPU) against oracle/mx_oracle.py, over every code and a spread of scales"""
    q = torch.arange(256, dtype=torch.uint8).repeat(8, 1)
    q = q[(q & 0x7F) != 0x7F].reshape(8, -1)[:, :224]                          # the NaN codes are poison, not values
    e = (torch.arange(8 * 7).reshape(8, 7) * 4 + 3).to(torch.uint8)
    assert torch.equal(X.dequant(q, e), X.mx_dequantize(q, e))
    assert bool(torch.isnan(X.e4m3_value(torch.tensor([0x7F, 0xFF], dtype=torch.uint8))).all())


def test_identity_names_every_k():
    for c in GEMM:
        if c.values != "identity":
            continue
        k = X.identity_k(c.M, c.K)
        if c.M >= 128:
            assert set((k % 128).tolist()) == set(range(128)) and set((k // 128).tolist()) == set(range(c.T)), c.id
    for K in X.KS:                                                             # the columns of W, as vectors over j, are pairwise distinct
        b = X.make_buffers(X.gemm_case("F32", "identity", 1, 256, K))
        W = X.dequant(X.operand(b, "w8"), X.operand(b, "ws"))
        assert len({tuple(col) for col in W.T.tolist()}) == K


@pytest.mark.parametrize("values", ["identity", "lattice"])
def test_exact_references_are_exactly_representable(values):
    """computing them in fp32 equals fp64, under a permutation of K as well"""
    for c in SLICE:
        if c.kind != "gemm" or c.values != values:
            continue
        b = X.make_buffers(c)
        A, W = X.dequant(X.operand(b, "a8"), X.operand(b, "as")), X.dequant(X.operand(b, "w8"), X.operand(b, "ws"))
        ref = X.reference(b)["pre"]
        bias = b["bias"][:c.N] if b["bias"] is not None else 0.0
        perm = torch.randperm(c.K, generator=torch.Generator().manual_seed(1))
        assert torch.equal((A.float() @ W.float().T + bias).double(), ref), c.id
        assert torch.equal((A.float()[:, perm] @ W.float()[:, perm].T + bias).double(), ref), c.id
        if c.epi.startswith("RESID"):
            keep = b["keep"].double()[:, None] if b["keep"] is not None else 1.0
            want = b["x0"].double() + b["gate"][:c.N].double() * (ref * keep)
            assert torch.equal(want.float().double(), want), c.id


def test_lattice_notices_two_swapped_scale_bytes():
    c = X.gemm_case("F32", "lattice", 300, 256, 640)
    b = X.make_buffers(c)
    ref = X.reference(b)["pre"]
    s = X.operand(b, "as")
    row = next(r for r in range(c.M) if int(s[r, 4]) != int(s[r, 5]))
    s[row, 4], s[row, 5] = int(s[row, 5]), int(s[row, 4])
    assert int((X.reference(b)["pre"][row] != ref[row]).sum()) >= 200


def test_quantiser_inputs_hold_every_decision():
    for kind, op in (("quant", "bf16"), ("quant16", "bf16"), ("quant16", "f16")):
        mine = [c for c in CASES if c.kind == kind and c.op == op]
        assert {c.M for c in mine} == set(X.Q_ROWS) and {c.N for c in mine} == set(X.Q_COLS)
        union = set()
        for c in mine:
            x = X.make_buffers(c)["x"]
            assert bool(torch.isfinite(x.float()).all())
            f = X.quant_features(x)
            union |= f
            if (c.M, c.N) == (37, 1024):
                assert f >= set(X.features_of(op if kind == "quant16" else "f32")), (c.id, set(X.QUANT_FEATURES) - f)
        assert union >= set(X.features_of(op if kind == "quant16" else "f32")), (kind, op, set(X.QUANT_FEATURES) - union)


def test_slice_holds_every_combination():
    have = {(c.kind, c.epi, c.values, c.T) for c in SLICE}
    assert have >= {(c.kind, c.epi, c.values, c.T) for c in CASES}
    assert {(c.kind, c.op, c.N) for c in SLICE if c.kind in ("quant", "quant16", "ln")} == \
        {(c.kind, c.op, c.N) for c in CASES if c.kind in ("quant", "quant16", "ln")}


def test_correct_emulation_passes():
    """also the proof that the arithmetic of the reference model alone stays inside the bounds on these inputs"""
    extra = [c for c in CASES if c.kind == "qkv"] + [c for c in CASES if c.kind in ("quant", "quant16", "ln") and c.M == 37]
    for c in SLICE + extra:
        b = X.make_buffers(c)
        X.emulate(b)
        assert X.check(b) == [], c.id


@pytest.mark.parametrize("fault", X.FAULTS)
def test_every_seeded_mistake_is_flagged(fault):
    pool = [c for c in SLICE + [c for c in CASES if c.kind == "qkv"] if X.fault_applies(fault, c)]
    assert pool, fault
    # the mistakes of the operand mapping must be named by both exact classes, not only by a bound; the others by any case (the cheapest first)
    mapping = fault in ("scale_next_block", "opsel_swapped", "chunk_swapped", "last_ktile_dropped")
    need = {"-identity-", "-lattice-"} if mapping else {""}
    pool.sort(key=lambda c: (c.values == "gauss", c.M * c.N * c.K))
    flagged, tried = [], 0
    for c in pool:
        if not any(n in c.id for n in need):
            continue
        b = X.make_buffers(c)
        X.emulate(b, fault)
        tried += 1
        if X.check(b):
            flagged.append(c.id)
            need = {n for n in need if n not in c.id}
        if not need:
            break
    print(f"[mxfp8 matrix] {fault}: flagged on {len(flagged)} of the {tried} cases tried ({len(pool)} apply)")
    assert not need and flagged, (fault, need)


def test_fault_table_is_complete():
    want = {"scale_next_block", "scale_plus1", "opsel_swapped", "chunk_swapped", "stale_scales_odd_tile", "last_ktile_dropped",
            "single_ktile_uninit", "a_clamp_missing", "row_past_M", "col_tile_shifted", "keep_ignored", "gate_col_shift", "gelu_amax_8cols",
            "out8s_uses_ld", "e4m3_truncated", "saturation_missing", "quant_idle_lane_amax", "ln_mean_of_first_256", "rope_partner_sign",
            "seam_row_wrong_batch"}
    assert want <= set(X.FAULTS)
