"""csrc/gemm_route.hpp f5_gemm_route -- the one function behind the GEMM launcher and the engine's questions about it -- asked through
f5_debug_gemm_route on the CPU (nothing is launched), against two independent statements of the same rule:

  * gemm_matrix.expected_kernel, the Python mirror of the dispatcher that tests/test_gemm_matrix_gpu.py confirms launch by launch on
    the GPU (where run_case also ties this query to the name the real launch reports);
  * the three predicates the engine plans with (runs-staged, fold-small, resid-LN-fusable), restated below from the C++ bodies they had
    while they were separate functions next to the launcher.
"""
import contextlib
import ctypes as C
import math
import random

import pytest

import gemm_matrix as GM
from f5_tts_mlx_amd import engine as E

EPI_ID = dict(GM.EPI, QKV_ROPE=5)
G4, LN_TAIL, PRODUCER, STATS, ROWF = 1, 2, 4, 8, 16           # variant_bits of f5_debug_gemm_route
STAGED, FOLD_SMALL, LN_FUSABLE = 1, 2, 4                      # its facts
FOLD_EPIS = ("RESID_GATE", "QKV_ROPE", "GELU_TANH")
NS = (1, 100, 128, 192, 200, 256, 384, 512, 768, 1024, 2048, 3072)
QKV_TILES = (0, 1, 12, 13, 14)


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


@contextlib.contextmanager
def knobs(lib, sel=0, ring=1, qkv_tile=0):
    try:
        E.check(lib.f5_debug_set_gemm_tile(sel))
        E.check(lib.f5_debug_set_gemm_ring(ring))
        E.check(lib.f5_debug_set_gemm_qkv_tile(qkv_tile))
        yield
    finally:
        lib.f5_debug_set_gemm_tile(0)
        lib.f5_debug_set_gemm_ring(1)
        lib.f5_debug_set_gemm_qkv_tile(0)


_BUF = C.create_string_buffer(64)
_FACTS = C.c_int(0)


def route(lib, epi, M, N, nseg=1, seq_len=0, bits=0, flags=0):
    """-> (name or None when refused, facts)"""
    _FACTS.value = -1
    n = lib.f5_debug_gemm_route(EPI_ID[epi], M, N, nseg, seq_len, bits, flags, _BUF, 64, C.byref(_FACTS))
    assert _FACTS.value >= 0
    if n < 0:
        return None, _FACTS.value
    name = _BUF.value.decode()
    assert n == len(name) and name
    return name, _FACTS.value


def named(base, epi, bits):
    """the name of a launch on kernel `base`: the variant suffixes the launchers append"""
    if base in ("gemm256", "rs128"):
        s = base + ("+qk_tr" if epi == "QKV_ROPE" and bits & G4 else "")
        if epi in ("QKV_ROPE", "GELU_TANH"):
            s += "+fold_stats" if bits & STATS else ("+fold_rowf" if bits & ROWF else "")
        return s
    return base + ("+fold_producer" if bits & PRODUCER else ("+fold_consumer" if bits & STATS else ""))


# ---- the three predicates as the C++ sources stated them (sel / ring / qkv_tile = the knobs; ldo == N is the caller's to check) -----
def was_resid_ln_fusable(sel, M, N):
    t256 = GM.cdiv(M, 256) * (N // 256)
    big = sel == 4 or (sel == 0 and N % 256 == 0 and M >= 256 and t256 >= 512)
    return not big and N % 256 == 0 and 256 <= N <= 1024 and M <= 64 * 65536


def was_runs_staged(sel, epi, M, N, seq_len, ln_tail):
    if epi not in FOLD_EPIS or ln_tail or N % 256 != 0:
        return False
    t256, t128 = GM.cdiv(M, 256) * (N // 256), GM.cdiv(M, 128) * GM.cdiv(N, 128)
    if sel == 4 or (sel == 0 and M >= 256 and t256 >= 512):
        return M >= 256
    rows_ok = epi != "QKV_ROPE" or (seq_len > 0 and M % seq_len == 0)
    return rows_ok and (sel == 14 or (sel == 0 and t128 >= 384))


def was_fold_small(sel, ring, qkv_tile, epi, M, N, nseg, seq_len, qkv_tr, ln_tail, flags):
    if sel != 0 or not ring or ln_tail or nseg != 1 or N % 256 != 0 or M < 1:
        return False
    t256, t128, t64 = GM.cdiv(M, 256) * (N // 256), GM.cdiv(M, 128) * GM.cdiv(N, 128), GM.cdiv(M, 64) * GM.cdiv(N, 128)
    if (M >= 256 and t256 >= 512) or t128 >= 384:
        return False                                  # the staged multi-round kernels take these
    if epi == "QKV_ROPE":
        if not qkv_tr or seq_len <= 0 or M % seq_len != 0 or qkv_tile != 0:
            return False
        return 176 <= (M // seq_len) * GM.cdiv(seq_len, 128) * (N // 256) <= 256
    if epi == "GELU_TANH":
        return 176 <= t128 <= 256
    if epi == "RESID_GATE":
        return not 176 <= t128 <= 256 and 176 <= t64 <= 256 and (flags & (8 | 256)) == 0
    return False


def check_point(lib, sel, ring, qkv_tile, epi, M, N, nseg=1, seq_len=0, bits=0, flags=0):
    """one query (the knobs are set by the caller): the kernel against the mirror, the facts against the predicates, the invariants"""
    want = GM.expected_kernel(sel, epi, M, N, ring, seq_len=seq_len, g4=bool(bits & G4), qkv_tile=qkv_tile)
    got, facts = route(lib, epi, M, N, nseg, seq_len, bits, flags)
    where = (sel, ring, qkv_tile, epi, M, N, nseg, seq_len, bits, flags)
    ln_tail = bool(bits & LN_TAIL)
    if not ln_tail:                                   # (the mirror knows no fused LN tail)
        assert got == (None if want is None else named(want, epi, bits)), (where, got, want)
    elif got is not None:                             # an accepted LN tail runs a small-tile kernel
        assert epi == "RESID_GATE" and facts & LN_FUSABLE and got not in ("gemm256", "rs128"), (where, got)
    assert bool(facts & LN_FUSABLE) == was_resid_ln_fusable(sel, M, N), (where, facts)
    assert bool(facts & STAGED) == was_runs_staged(sel, epi, M, N, seq_len, ln_tail), (where, facts)
    assert bool(facts & FOLD_SMALL) == was_fold_small(sel, ring, qkv_tile, epi, M, N, nseg, seq_len, bool(bits & G4), ln_tail, flags), (where, facts)
    if facts & STAGED:
        assert got in ("gemm256", "rs128", "gemm256+qk_tr", "rs128+qk_tr"), (where, got)
    if facts & FOLD_SMALL:
        assert got == {"RESID_GATE": "ring_ks2<1>", "GELU_TANH": "ring8<2>", "QKV_ROPE": "rs128+qk_tr"}[epi], (where, got)
    return got, facts


def check_fold_requests(lib, epi, M, N, nseg, seq_len, bits, flags, base, facts):
    """each LN-fold role on top of an accepted launch: the staged kernels and the single-round launch of that role take it, under the
    name the launchers give the variant; every other route refuses it"""
    for role in (PRODUCER, STATS, ROWF):
        got, facts2 = route(lib, epi, M, N, nseg, seq_len, bits | role, flags)
        assert facts2 == facts                        # the request changes no fact
        small_ok = facts & FOLD_SMALL and ((role == PRODUCER and epi == "RESID_GATE") or (role == STATS and epi == "GELU_TANH"))
        if base.split("+")[0] in ("gemm256", "rs128") or small_ok:
            assert got == named(base.split("+")[0], epi, bits | role), (epi, M, N, bits, role, got)
        else:
            assert got is None and "LN fold" in lib.f5_last_error().decode(), (epi, M, N, bits, role, got)


def test_matrix_fallbacks_refusals_and_production_shapes(lib):
    seen = set()
    for c in GM.cases():
        key = (c.sel, c.ring, c.epi, c.M, c.N)
        if key in seen:
            continue
        seen.add(key)
        with knobs(lib, c.sel, c.ring):
            got, _ = check_point(lib, c.sel, c.ring, 0, c.epi, c.M, c.N, c.nseg)
        assert got == c.kernel
    for sel, epi, M, N in GM.FALLBACKS:
        with knobs(lib, sel):
            got, _ = check_point(lib, sel, 1, 0, epi, M, N)
        assert got is not None and got == GM.expected_kernel(sel, epi, M, N)
    refusals = [c for _name, c in GM.SEL4_REFUSALS]
    assert len(refusals) == 3
    for c in refusals:
        with knobs(lib, c.sel):
            got, _ = check_point(lib, c.sel, 1, 0, c.epi, c.M, c.N)
            assert got is None and "256x256" in lib.f5_last_error().decode()
    with knobs(lib):
        for B in (1, 2, 4, 8, 16, 32):
            for name, epi, N, _K in GM.PRODUCTION:
                got, _ = check_point(lib, 0, 1, 0, epi, 2 * B * 937, N)
                assert got == GM.PROMISED.get(B, {}).get(name, got), (B, name, got)


def test_random_sweep_against_the_mirror_and_the_predicates(lib):
    rnd = random.Random(20240)
    points = folds = staged = small = 0
    for sel in GM.SELECTORS:
        for ring in (0, 1):
            with knobs(lib, sel, ring):
                for epi in GM.EPIS:
                    for i in range(120):
                        # 100 points log-uniform in 1 ... 70 000, 20 more where the single-round kernels live (about 1 000 ... 2 200 rows)
                        M = int(round(math.exp(rnd.uniform(0.0, math.log(70000.0))))) if i < 100 else rnd.randint(1000, 2200)
                        N = rnd.choice(NS)
                        nseg, flags = rnd.choice((1, 1, 3)), rnd.choice((0, 0, 8, 256))
                        got, facts = check_point(lib, sel, ring, 0, epi, M, N, nseg, flags=flags)
                        check_point(lib, sel, ring, 0, epi, M, N, nseg, bits=LN_TAIL, flags=flags)
                        points += 1
                        staged += bool(facts & STAGED)
                        small += bool(facts & FOLD_SMALL)
                        if got is not None:
                            check_fold_requests(lib, epi, M, N, nseg, 0, 0, flags, got, facts)
                            folds += 1
    # the single-round LN-fold launches of the out-projection / FF2 (producer) and FF1 (consumer), densely: every third row count
    # around the 176 ... 256-tile windows, with the operand modes and flags that switch the fold off
    with knobs(lib):
        for M in range(900, 2400, 3):
            for epi, N in (("RESID_GATE", 1024), ("GELU_TANH", 2048), ("RESID_GATE", 2048), ("GELU_TANH", 1024)):
                for nseg, flags in ((1, 0), (3, 0), (1, 8), (1, 256)):
                    got, facts = check_point(lib, 0, 1, 0, epi, M, N, nseg, flags=flags)
                    small += bool(facts & FOLD_SMALL)
                    check_fold_requests(lib, epi, M, N, nseg, 0, 0, flags, got, facts)
    print(f"[route] {points} points, {folds} with fold requests, {staged} staged, {small} fold-small")
    assert points >= 20000 and folds >= 15000 and staged > 100 and small > 100


def test_qkv_routing(lib):
    points = small = 0
    for sel in GM.SELECTORS:
        for ring in (0, 1):
            for qkv_tile in QKV_TILES:
                with knobs(lib, sel, ring, qkv_tile):
                    for seq_len in (431, 937, 1000):
                        for B in range(1, 33):
                            for M in (B * seq_len, B * seq_len + 5):          # whole sequences, and a ragged M % seq_len
                                for N in (3072, 384):
                                    for bits in (0, G4):
                                        got, facts = check_point(lib, sel, ring, qkv_tile, "QKV_ROPE", M, N, 1, seq_len, bits)
                                        points += 1
                                        small += bool(facts & FOLD_SMALL)
                                        if got is not None and B in (1, 2, 3, 8, 32) and N == 3072:
                                            check_fold_requests(lib, "QKV_ROPE", M, N, 1, seq_len, bits, 0, got, facts)
    assert points >= 20000 and small > 0
    with knobs(lib):
        # what the dispatcher's comments state: M = 2 x 937 with group-major tables is one round of 192 role-split tiles, without them
        # 720 register-staged 64x128 tiles; M = 3 x 431 (144 role-split tiles) stays on the small tiles
        assert route(lib, "QKV_ROPE", 2 * 937, 3072, 1, 937, G4)[0] == "rs128+qk_tr"
        assert 2 * GM.cdiv(937, 128) * (3072 // 256) == 192
        assert route(lib, "QKV_ROPE", 2 * 937, 3072, 1, 937, 0)[0] == "cfg<1,2>"
        assert GM.cdiv(2 * 937, 64) * (3072 // 128) == 720
        got, facts = route(lib, "QKV_ROPE", 3 * 431, 3072, 1, 431, G4)
        assert got == "ring<1,2>" and not facts & (STAGED | FOLD_SMALL)
    # the two launches where the predicates and the launcher used to differ: the single-round QKV launch runs on rs128 yet is not
    # "staged" (the fold reaches it as a fold-small launch), and selector 14 with a ragged M % seq_len is refused, not staged
    with knobs(lib):
        assert route(lib, "QKV_ROPE", 2 * 937, 3072, 1, 937, G4) == ("rs128+qk_tr", FOLD_SMALL)
    with knobs(lib, 14):
        assert route(lib, "QKV_ROPE", 2 * 937 + 5, 3072, 1, 937, G4) == (None, 0)
        assert "multiple of seq_len" in lib.f5_last_error().decode()
        assert route(lib, "QKV_ROPE", 2 * 937, 3072, 1, 937, G4) == ("rs128+qk_tr", STAGED)


def test_names_of_the_variants(lib):
    """the strings tests/test_ops_gpu.py asserts after its folded launches (M = 2 x 937 rows of the 335M shape), and the +qk_tr forms"""
    M = 2 * 937
    with knobs(lib):
        assert route(lib, "RESID_GATE", M, 1024, bits=PRODUCER)[0] == "ring_ks2<1>+fold_producer"
        assert route(lib, "GELU_TANH", M, 2048, bits=STATS)[0] == "ring8<2>+fold_consumer"
        assert route(lib, "QKV_ROPE", M, 3072, 1, 937, G4 | STATS)[0] == "rs128+qk_tr+fold_stats"
        assert route(lib, "QKV_ROPE", 32 * M, 3072, 1, 937, G4)[0] == "gemm256+qk_tr"
        assert route(lib, "QKV_ROPE", 32 * M, 3072, 1, 937, G4 | ROWF)[0] == "gemm256+qk_tr+fold_rowf"
        assert route(lib, "QKV_ROPE", 32 * M, 3072, 1, 937, 0)[0] == "gemm256"
        assert route(lib, "GELU_TANH", M, 2048, bits=ROWF)[0] is None                  # the single-round kernels: statistics form only
        assert route(lib, "RESID_GATE", M, 1024, bits=PRODUCER, flags=256)[0] is None  # ... and the preloaded residual epilogue
    for sel, k in ((4, "gemm256"), (14, "rs128")):
        with knobs(lib, sel):
            assert route(lib, "RESID_GATE", M, 1024, bits=PRODUCER)[0] == k
            assert route(lib, "GELU_TANH", M, 2048, bits=STATS)[0] == k + "+fold_stats"
            assert route(lib, "GELU_TANH", M, 2048, bits=ROWF)[0] == k + "+fold_rowf"
            assert route(lib, "QKV_ROPE", M, 3072, 1, 937, G4 | STATS)[0] == k + "+qk_tr+fold_stats"
    assert route(lib, "F32", 300, 256) == ("ring<1,1>", LN_FUSABLE)                    # the knobs are back at their defaults
