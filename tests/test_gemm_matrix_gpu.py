"""The GEMM family against fp64, by construction: every tile selector x epilogue x operand type x nseg of csrc/gemm.hip's dispatcher,
at shapes derived from the selector's block tile (tests/gemm_matrix.py), with leading dimensions that are never the tight ones, NaN in
the operands' pad columns, guard bands around every output, tolerances that follow from the operand type, and the name of the kernel
each launch resolved to (f5_debug_last_gemm_kernel) checked against what the dispatcher's source says and against the routing function
asked without a launch (f5_debug_gemm_route, tests/test_gemm_route_host.py).

Then: the coverage of (kernel, epilogue, operand type, nseg) instantiations, requests the launchers must refuse, and every GEMM launch of
prepare / run_dit of the 335M configuration at N = 937, batch 1 ... 32.

The harness itself (generator, checker, tolerances) is tested on the CPU by tests/test_gemm_matrix_host.py, which shows that each of
ten kinds of subtly wrong kernel would fail here.

Wall time on one MI355X (same machine, one after the other): tests/test_ops_gpu.py at the parent commit 42.3 s (215 tests), this module
22.6 s (595 tests, 28 960 matrix cases: operands, fp64 references and guard comparisons all stay on the device).
"""
import ctypes as C

import pytest
import torch

import gemm_matrix as GM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def last_kernel(lib):
    buf = C.create_string_buffer(64)
    n = lib.f5_debug_last_gemm_kernel(buf, 64)
    name = buf.value.decode()
    assert n == len(name)
    return name


def routed_kernel(lib, c):
    """what the routing function (csrc/gemm_route.hpp) says about the case, asked without a launch; "" = it would refuse"""
    buf = C.create_string_buffer(64)
    n = lib.f5_debug_gemm_route(GM.EPI[c.epi], c.M, c.N, c.nseg, 0, 0, 0, buf, 64, None)
    return buf.value.decode() if n >= 0 else ""


def launch(lib, b):
    """one case through the entry point of its epilogue; returns the return code (the caller synchronises)"""
    c = b["case"]
    lo = (lambda t: t) if c.nseg == 3 else (lambda t: None)
    a_hi, a_lo, w_hi, w_lo = b["a"][0], lo(b["a"][1]), b["w"][0], lo(b["w"][1])
    of, oh, ol = b["out_f32"].ptr_tensor(), b["out_hi"].ptr_tensor(), b["out_lo"].ptr_tensor()
    s = stream()
    if c.epi == "RESID_GATE":
        return lib.f5_op_gemm_resid_gate(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(b["gate"]), P(b["keep"]), P(of), c.M, c.N, c.K,
                                         c.lda, c.ldw, c.ldo, c.nseg, s)
    if c.epi == "RESID_KEEP":
        return lib.f5_op_gemm_resid_keep(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(b["resid"].ptr_tensor()), P(b["keep"]), P(of),
                                         c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.nseg, s)
    if c.epi == "ADDROWS":
        return lib.f5_op_gemm_addrows(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["addrows"].ptr_tensor()), c.a_row_mod, P(of), P(oh), P(ol if c.nseg == 3 else None),
                                      c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.nseg, s)
    # outputs the epilogue does not own are handed over all the same (guarded): they must come back untouched
    return lib.f5_op_gemm(P(a_hi), P(a_lo), P(w_hi), P(w_lo), P(b["bias"]), P(of), P(oh), P(ol if c.nseg == 3 else None), c.M, c.N, c.K,
                          c.lda, c.ldw, c.ldo, c.nseg, GM.EPI[c.epi], s)


class selector:
    def __init__(self, lib, sel, ring=1):
        self.lib, self.sel, self.ring = lib, sel, ring

    def __enter__(self):
        E.check(self.lib.f5_debug_set_gemm_tile(self.sel))
        E.check(self.lib.f5_debug_set_gemm_ring(self.ring))

    def __exit__(self, *exc):
        E.check(self.lib.f5_debug_set_gemm_tile(0))
        E.check(self.lib.f5_debug_set_gemm_ring(1))


def run_case(lib, c, rows=None):
    """-> (kernel reached, findings).  The caller holds the operand mode and the selector of the case."""
    b = GM.make_buffers(c, device=DEV)
    rc = launch(lib, b)
    if rc != 0:
        return None, [f"refused: {lib.f5_last_error().decode()}"]
    name = last_kernel(lib)
    torch.cuda.synchronize()
    bad = GM.check(b, rows=rows)
    if name != c.kernel:
        bad.append(f"ran {name}, the dispatcher's source says {c.kernel}")
    routed = routed_kernel(lib, c)
    if name != routed:
        bad.append(f"ran {name}, f5_debug_gemm_route says {routed!r}")
    return name, bad


# ---- the matrix --------------------------------------------------------------------------------------------------------------
CASES = GM.cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c.group, []).append(_c)
REACHED = set()          # (kernel, epilogue, operand type, nseg) over the whole module


def _gid(g):
    op, kernel, sel, ring, epi, nseg = g
    return f"{op}-{kernel}-sel{sel}{'' if ring else '-noring'}-{epi}-nseg{nseg}"


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_matrix(lib, group):
    op, kernel, sel, ring, epi, nseg = group
    failures = []
    with operand_mode(op), selector(lib, sel, ring):
        assert lib.f5_op_get_operand_type() == (1 if op == "f16" else 0)
        for c in GROUPS[group]:
            name, bad = run_case(lib, c)
            if name is not None:
                REACHED.add((name, epi, op, nseg))
            if bad:
                failures.append((c.id, bad))
    print(f"[matrix] {_gid(group)}: {len(GROUPS[group])} shapes, {len(failures)} failed")
    assert not failures, failures[:5]


# Every instantiation launch_epi (csrc/gemm.hip) / f5_launch_gemm256 / f5_launch_gemm_rs128 can produce for the eight epilogues of this matrix, written
# out from the sources: the nine small-tile / ring launchers are instantiated for every epilogue, gemm256.hip switches over all of
# them, gemm_rs128.hip over four, the 128x256 ring tiles are only instantiated for two (and for EPI_QKV_ROPE, which stays with
# test_ops_gpu._attention_case, like the +qk_tr variants of gemm256 / rs128).
EXPECTED = {(k, e) for k in ("cfg<2,2>", "cfg<1,2>", "cfg<1,1>", "ring<1,2>", "ring<1,1>", "ring8<3>", "ring8<2>", "ring_ks2<1>", "ring_ks2<2>", "gemm256")
            for e in GM.EPIS}
EXPECTED |= {("rs128", e) for e in GM.RS128_EPIS}
EXPECTED |= {(k, e) for k in ("ring_wide<2,2,2,4>", "ring_wide<1,4,4,2>") for e in GM.WIDE_EPIS}
# The fold variants need the LN-fold hooks around the launch, not a shape: ring_ks2<1>+fold_producer (RESID_GATE) and
# ring8<2>+fold_consumer (GELU_TANH) are reached, one-pass operands, both operand types, by
# test_ops_gpu.py::test_ln_modulate_folded_into_the_gemms_around_it[*-small] (and its _f16 twin), which asserts these names after
# its launches; gemm256 / rs128 +fold_rowf / +fold_stats by its [4] / [14] cases.
FOLD_VARIANTS_TESTED_ELSEWHERE = (("ring_ks2<1>+fold_producer", "RESID_GATE"), ("ring8<2>+fold_consumer", "GELU_TANH"))


def test_matrix_reaches_every_instantiation():
    """runs after test_matrix (same module, definition order): the whole matrix must have run in this process"""
    want = {(k, e, op, nseg) for (k, e) in EXPECTED for op in GM.OPS for nseg in (1, 3)}
    by_generator = {(c.kernel, c.epi, c.op, c.nseg) for c in CASES}
    assert want <= by_generator, sorted(want - by_generator)
    missing = sorted(want - REACHED)
    extra = sorted(k for k in REACHED if (k[0], k[1]) not in EXPECTED)
    print(f"[matrix] {len(REACHED)} (kernel, epilogue, operand type, nseg) instantiations reached, {len(want)} expected")
    assert not missing and not extra, (missing, extra)


# ---- forced selectors the dispatcher does not honour: recorded under the kernel actually reached ------------------------------
FALLBACKS = GM.FALLBACKS


@pytest.mark.parametrize("op", GM.OPS)
@pytest.mark.parametrize("sel,epi,M,N", FALLBACKS, ids=lambda v: str(v))
def test_fallbacks_compute_the_same_thing(lib, op, sel, epi, M, N):
    for nseg in (1, 3):
        c = GM.make_case(op, sel, epi, nseg, M, N, 192, note="fallback")
        with operand_mode(op), selector(lib, sel):
            name, bad = run_case(lib, c)
        print(f"[matrix] fallback sel={sel} {epi} N={N} {op} nseg={nseg}: ran {name}")
        assert not bad, (c.id, bad)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    base = dict(op="bf16", epi="F32", nseg=1)
    for name, c in GM.SEL4_REFUSALS:
        yield name, c, {}
    yield "lda_not_8", GM.make_case(sel=0, M=100, N=256, K=128, **base), {"lda": 128 + 4}
    yield "ldw_not_8", GM.make_case(sel=5, M=100, N=256, K=128, **base), {"ldw": 128 + 12}
    yield "K_not_64", GM.make_case(sel=0, M=100, N=256, K=128, **base), {"K": 96}
    yield "K_not_64_f16_addrows", GM.make_case("f16", 10, "ADDROWS", 1, 100, 256, 128), {"K": 32}
    yield "nseg3_without_lo", GM.make_case("bf16", 0, "BF16", 3, 100, 256, 128), {"drop_lo": True}
    yield "nseg3_without_lo_resid_keep", GM.make_case("f16", 6, "RESID_KEEP", 3, 100, 256, 128), {"drop_lo": True}
    yield "nseg_2", GM.make_case(sel=0, M=100, N=256, K=128, **base), {"nseg": 2}


@pytest.mark.parametrize("name,c,twist", list(_refusal_cases()), ids=[r[0] for r in _refusal_cases()])
def test_illegal_requests_are_refused_and_touch_nothing(lib, name, c, twist):
    """the buffers are made for the legal case; the request is then bent (a smaller K, a leading dimension that is not a multiple of
    8 ...), so that even a launcher that lets it through stays inside the allocations"""
    b = GM.make_buffers(c, device=DEV)
    twist = dict(twist)
    if twist.pop("drop_lo", False):
        b["a"][1] = None
        b["w"][1] = None
        b["case"] = c
        launch_case = c
    else:
        launch_case = GM.with_dims(c, **twist)
    b["case"] = launch_case
    with operand_mode(c.op), selector(lib, c.sel):
        if b["a"][1] is None:           # nseg 3 with null lo operands
            s = stream()
            of, oh, ol = b["out_f32"].ptr_tensor(), b["out_hi"].ptr_tensor(), b["out_lo"].ptr_tensor()
            if c.epi == "RESID_KEEP":
                rc = lib.f5_op_gemm_resid_keep(P(b["a"][0]), P(None), P(b["w"][0]), P(None), P(b["bias"]), P(b["resid"].ptr_tensor()), P(b["keep"]),
                                               P(of), c.M, c.N, c.K, c.lda, c.ldw, c.ldo, 3, s)
            else:
                rc = lib.f5_op_gemm(P(b["a"][0]), P(None), P(b["w"][0]), P(None), P(b["bias"]), P(of), P(oh), P(ol), c.M, c.N, c.K, c.lda, c.ldw,
                                    c.ldo, 3, GM.EPI[c.epi], s)
        else:
            rc = launch(lib, b)
        msg = lib.f5_last_error().decode()
        reached = last_kernel(lib)
    torch.cuda.synchronize()
    print(f"[matrix] refusal {name}: rc={rc} kernel={reached!r} error={msg!r}")
    assert rc != 0 and msg.strip() and reached == "", (name, rc, msg, reached)
    for k in ("out_f32", "out_hi", "out_lo", "resid", "addrows"):
        if b[k] is not None:
            assert b[k].guard_damage(interior_too=True) == 0, (name, k)


# ---- production shapes -------------------------------------------------------------------------------------------------------------
# every GEMM launch of prepare / run_dit (csrc/engine.hip) for the 335M configuration (dim 1024, ff 2048, text 512 / 1024, mel 100 padded
# to 128) at 937 frames: M = nb x B x 937 rows with nb = 2 (conditional + null branch); (name, epilogue, N, K)
PRODUCTION, PROMISED = GM.PRODUCTION, GM.PROMISED


def sample_rows(M, seed):
    """all rows up to 15 000; above, the first and last three, both rows on each side of every multiple of 256, 256 random ones"""
    if M <= 15000:
        return None
    rows = {0, 1, 2, M - 3, M - 2, M - 1}
    for m in range(256, M, 256):
        rows.update((m - 2, m - 1, m, m + 1))
    g = torch.Generator().manual_seed(seed)
    rows.update(torch.randint(0, M, (256,), generator=g).tolist())
    return torch.tensor(sorted(r for r in rows if 0 <= r < M), device=DEV)


@pytest.mark.parametrize("op", GM.OPS)
@pytest.mark.parametrize("B", [1, 2, 4, 8, 16, 32])
def test_production_shapes(lib, op, B):
    M = 2 * B * 937
    failures = []
    for name, epi, N, K in PRODUCTION:
        c = GM.make_case(op, 0, epi, 1, M, N, K, note=name)
        if epi == "ADDROWS":
            c = GM.with_dims(c, a_row_mod=M // 2)          # both branches read the same x rows
        rows = sample_rows(M, B)
        with operand_mode(op), selector(lib, 0):
            kernel, bad = run_case(lib, c, rows=rows)
        print(f"[parity] production B={B} {op} {name} {epi} M={M} N={N} K={K}: {kernel}"
              f"{'' if rows is None else f' ({len(rows)} rows compared)'}{' FAILED' if bad else ''}")
        if bad:
            failures.append((name, bad))
        want = PROMISED.get(B, {}).get(name)
        if want is not None and kernel != want:
            failures.append((name, f"f5_gemm_route's comments promise {want} at batch {B}, ran {kernel}"))
        torch.cuda.empty_cache()
    assert not failures, failures
