"""The attention matrix's own test, on the CPU (tests/attention_matrix.py; the GPU side is tests/test_attention_matrix_gpu.py):

  * the generator: the exact case count, no duplicates, every case inside the ABI f5_launch_attention enforces, every (kernel, operand
    type) pair and every fp8-capable kernel present;
  * the transcription of the launcher's rule: the named fall-throughs, both sides of every automatic threshold, the 335M shapes;
  * the checker over a torch emulation that performs the kernel's roundings: the right emulation passes a slice that covers every
    (kernel, operand type, value class) -- which is also the check that the inputs are well chosen: the reference arithmetic alone
    stays inside the derived bound on them -- and every seeded mistake of AM.FAULTS is flagged, in both operand types wherever it
    can occur.
"""
import pytest

import attention_matrix as AM

CASES = AM.cases()
N_CASES = 2142


def _slice():
    """per (operand type, kernel, value class, fp8) up to four small cases: the first two in generator order, the one with the most
    KV tiles, and the first with several batch elements and heads"""
    pools = {}
    for c in CASES:
        if c.N <= 330 and c.B * c.H <= 9:
            pools.setdefault(c.group, []).append(c)
    out = {}
    for g, pool in pools.items():
        pick = pool[:2] + [max(pool, key=lambda c: max(c.kvs))] + [c for c in pool if c.B >= 2 and c.H >= 2][:1]
        out[g] = list(dict.fromkeys(pick))
    return out


SLICE = _slice()


def test_generator_counts_and_abi():
    assert len(CASES) == N_CASES
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        hp, pipe, wide, kvsplit = c.knobs
        assert c.B > 0 and c.H > 0 and c.N > 0
        assert c.npad % 64 == 0 and c.npad >= c.N and c.npad in (AM.ceil64(c.N), AM.ceil64(c.N) + 64)
        assert c.ldqk % 8 == 0 and c.ldqk > 2 * c.D and c.ldo % 4 == 0 and c.ldo > c.D and c.ldo8 % 4 == 0 and c.ldo8 > c.D
        assert not (c.f8 and hp) and c.values in AM.VALUES and c.op in AM.OPS
        assert c.kv is None or (len(c.kv) == c.B and all(1 <= x <= c.N for x in c.kv))
        assert wide in (-1, 0, 1) and kvsplit in (-1, 1, 2, 4) and pipe in (-1, 0, 1)
        assert c.N <= 704 or (c.N == 1100 and c.kernel in AM.WIDE_KERNELS) or (c.N == 769 and c.route == "auto" and c.B * c.H == 23)
    for op in AM.OPS:
        for k in AM.KERNELS:
            mine = [c for c in CASES if c.op == op and c.kernel == k and not c.f8]
            assert {c.values for c in mine} == set(AM.VALUES), (op, k)
            assert {AM.cdiv(c.N, 64) for c in mine} >= set(range(1, 12)), (op, k)
            assert {(c.N - 1) % 64 + 1 for c in mine} >= set(AM.FILLS), (op, k)
            # the kernels loop over ceil(kv_len / 64) tiles, not ceil(N / 64): the same coverage on the longest kv_len of each launch,
            # in the Gaussian class alone, and every tile count also with batch elements that run fewer tiles in the same launch
            gauss = [c for c in mine if c.values == "gauss"]
            assert {AM.cdiv(max(c.kvs), 64) for c in gauss} >= set(range(1, 12)), (op, k)
            assert {(max(c.kvs) - 1) % 64 + 1 for c in gauss} >= set(AM.FILLS), (op, k)
            assert {AM.cdiv(max(c.kvs), 64) for c in gauss if AM.cdiv(min(c.kvs), 64) < AM.cdiv(max(c.kvs), 64)} >= set(range(2, 12)), (op, k)
            for t in range(1, 12):
                assert sum(AM.cdiv(max(c.kvs), 64) == t for c in mine) >= 3, (op, k, t)
            assert {c.B * c.H for c in mine} >= {1, 3, 8, 9, 17} and {c.H for c in mine} >= {1, 2, 3} and max(c.B for c in mine) >= 3
            assert any(c.kv is None for c in mine) and any(c.kv is not None and len(set(c.kv)) > 1 for c in mine)
            assert {c.npad - AM.ceil64(c.N) for c in mine} == {0, 64}
            assert (sum(c.N == 1100 for c in mine) == 1) == (k in AM.WIDE_KERNELS)
        for k in AM.F8_KERNELS:
            assert any(c.op == op and c.kernel == k and c.f8 for c in CASES), (op, k)
    assert {(c.op, c.kernel) for c in CASES} == {(op, k) for op in AM.OPS for k in AM.KERNELS}
    assert set(SLICE) == {c.group for c in CASES}, "the CPU slice misses a (type, kernel, value class)"


def test_transcription_of_the_launcher_rule():
    ek = AM.expected_kernel
    # the eight kernels by their knobs, and the silent fall-throughs
    for route, want in (("v2_hp", AM.V2_HP), ("v2", AM.V2), ("v2f_pre", AM.V2F_PRE), ("v2f", AM.V2F), ("v2p", AM.V2P), ("v2s_hp", AM.V2S_HP),
                        ("v2s_ks2", AM.V2S_KS2), ("v2s_ks4", AM.V2S_KS4), *AM.FALL_THROUGHS.items()):
        hp, pipe, wide, kvsplit, q = AM.ROUTES[route]
        for B, H, N in ((1, 1, 1), (3, 2, 200), (2, 16, 937), (64, 16, 937)):
            assert ek(B, H, N, hp, q or 0, pipe, wide, kvsplit) == want, (route, B, H, N)
    assert ek(1, 2, 300, 1, 0, kvsplit=4) == AM.V2S_HP                 # a forced split of 4 with hp runs the two-group kernel
    assert ek(1, 2, 300, 0, 0, pipe=1, wide=1, kvsplit=1) == AM.V2F    # pipe without a pre-scaled q
    assert ek(1, 2, 300, 0, 1, pipe=-1, wide=1, kvsplit=1, pipe_default=1) == AM.V2P
    assert ek(1, 2, 300, 1, 0, wide=1, kvsplit=1) == AM.V2_HP          # wide with hp is ignored
    # wide: >= 512 workgroups of 256 queries (and no split: more than 320 workgroups of 128)
    assert ek(512, 1, 64, 0, 1) == AM.V2F_PRE and ek(511, 1, 64, 0, 1) == AM.V2 and ek(512, 1, 64, 0, 0) == AM.V2F
    assert ek(128, 2, 257, 0, 1) == AM.V2F_PRE and ek(128, 2, 256, 0, 1) == AM.V2      # ceil(N / 256) counts
    assert ek(512, 1, 64, 1, 0) == AM.V2_HP
    # split: <= 160 workgroups of 128 queries with >= 8 tiles -> 4 groups; <= 320 with >= 4 -> 2 (N = 449 ... 512: 4 query blocks, 8 tiles)
    assert ek(40, 1, 449, 0, 0) == AM.V2S_KS4 and ek(41, 1, 449, 0, 0) == AM.V2S_KS2 and ek(40, 1, 448, 0, 0) == AM.V2S_KS2
    assert ek(23, 1, 832, 0, 0) == AM.V2S_KS2 and ek(160, 1, 65, 0, 0) == AM.V2        # 161 workgroups at 13 tiles; 160 at two tiles
    assert ek(160, 1, 193, 0, 0) == AM.V2S_KS2 and ek(161, 1, 193, 0, 0) == AM.V2 and ek(160, 1, 192, 0, 0) == AM.V2
    assert ek(107, 1, 257, 0, 0) == AM.V2 and ek(106, 1, 257, 0, 0) == AM.V2S_KS2 and ek(80, 1, 449, 0, 0) == AM.V2S_KS2
    assert ek(81, 1, 449, 0, 0) == AM.V2 and ek(40, 1, 449, 1, 0) == AM.V2S_HP and ek(80, 1, 449, 1, 0) == AM.V2S_HP
    for route, B, H, N, q, want, note in AM.AUTO:
        hp, pipe, wide, kvsplit, _ = AM.ROUTES[route]
        assert (wide, kvsplit) == (-1, -1) and ek(B, H, N, hp, q, pipe) == want, note
    for c in CASES:
        if c.route in AM.FALL_THROUGHS:
            assert c.kernel == AM.FALL_THROUGHS[c.route]
    # the 335M model: 16 heads, N = 937, batch doubled for guidance, q pre-multiplied
    for batch in range(1, 33):
        want = AM.V2S_KS2 if batch == 1 else (AM.V2 if batch <= 3 else AM.V2F_PRE)
        assert ek(2 * batch, 16, 937, 0, 1) == want, batch
        assert AM.PRODUCTION.get(batch, want) == want


@pytest.mark.parametrize("group", list(SLICE), ids=lambda g: f"{g[0]}-{g[1]}-{g[2]}{'-f8' if g[3] else ''}")
def test_right_emulation_passes(group):
    for c in SLICE[group]:
        b = AM.make_buffers(c)
        assert b["mask_excess"] >= 100.0, (c.id, b["mask_excess"])
        assert AM.check(b) != [], "untouched outputs must be flagged"
        AM.emulate(b)
        bad = AM.check(b)
        assert not bad, (c.id, bad)


@pytest.mark.parametrize("op", AM.OPS)
@pytest.mark.parametrize("kernel", AM.NO_TILE_MAX)
def test_spikes_drive_the_exact_fallback(kernel, op):
    """every kernel without a tile maximum gets spike cases whose fp64 scores trip its 2^14 row-sum limit in a later tile of a group:
    each of the six shapes of AM.spike_shapes made for that (live spikes at keys >= 64 ks), and the launch where other groups stay at
    their only tile meanwhile"""
    mine = [c for c in CASES if c.op == op and c.kernel == kernel and c.values == "spikes"]
    ks = AM.SPLIT.get(kernel, 1)
    assert len(mine) == len(AM.spike_shapes(ks))
    for c in mine:
        assert all(p < min(c.kvs) for p, _ in c.spikes), c.id
    events = [AM.fallback_events(AM.make_buffers(c)) for c in mine[:6]]
    print(f"[attention matrix] {op} {kernel}: (row, tile) pairs past the 2^14 limit in a later tile: {events}")
    assert all(n > 0 for n in events), (kernel, op, events)
    assert AM.cdiv(mine[0].N, 64) == ks + 1 and max(p for p, _ in mine[0].spikes) >= 64 * ks


@pytest.mark.parametrize("op", AM.OPS)
@pytest.mark.parametrize("kernel", AM.KERNELS)
def test_skipped_rescale_is_flagged_on_every_kernel(kernel, op):
    """the running maximum of the kernels with a tile maximum, the exact fallback of the others (the four-group kernel included)"""
    mine = [c for c in CASES if c.op == op and c.kernel == kernel and c.values == "spikes" and AM.fault_applies("rescale_skipped", c)][:2]
    assert len(mine) == 2
    for c in mine:
        b = AM.make_buffers(c)
        ref3 = AM.reference(b)
        AM.emulate(b, "rescale_skipped")
        assert AM.check(b, ref3), f"rescale_skipped went unnoticed on {c.id}"


@pytest.mark.parametrize("op", AM.OPS)
@pytest.mark.parametrize("fault", AM.FAULTS)
def test_seeded_mistakes_are_flagged(fault, op):
    if fault == "p_via_bf16" and op == "bf16":
        return                                                # cannot occur: P already is bf16
    pool = [c for g in SLICE.values() for c in g if c.op == op and AM.fault_applies(fault, c)]
    picked, seen = [], set()
    for c in pool:                                            # up to four cases, of different kernels first
        if c.kernel not in seen or len(pool) <= 4:
            seen.add(c.kernel)
            picked.append(c)
    picked = picked[:4]
    assert picked, f"no case of the slice lets {fault} change anything"
    for c in picked:
        b = AM.make_buffers(c)
        ref3 = AM.reference(b)
        AM.emulate(b, fault)
        assert AM.check(b, ref3), f"{fault} went unnoticed on {c.id}"
