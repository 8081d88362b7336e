"""csrc/attention.hip against fp64, by construction: all eight kernel instantiations of each operand build (and the MX-fp8 output of the
six that have it) through f5_op_attention_ex, at sequence lengths derived from the kernels' structure, never with the tight leading
dimensions, masked keys that would own the row if one were let through, NaN around the operands, guard bands and sentinels around and
inside every output, an element-wise bound derived from the count of roundings (tests/attention_matrix.py), and the kernel each launch
reached (f5_debug_last_attn_kernel) compared with a Python transcription of the launcher's rule.

Then: every instantiation reached, the requests the launcher must refuse, and the production shapes by name.

The harness itself is tested on the CPU by tests/test_attention_matrix_host.py, which shows that each of 27 kinds of subtly wrong
kernel would fail here.

Wall time on one MI355X: 8.6 s for the module (123 tests, 2 142 matrix cases: operands, fp64 references and guard comparisons stay on
the device).  The one-pass kernels use 0.36 ... 0.93 of the element-wise bound and at most 0.15 of the systematic-error allowance; the
bf16x3 kernels use 0.01 ... 0.16 of theirs, where the worst-case fp32 accumulation terms outweigh the u^2 ones (each test prints its figures).
"""
import ctypes as C

import pytest
import torch

import attention_matrix as AM
from f5test import DEV, E, P, operand_mode, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def last_kernel(lib):
    buf = C.create_string_buffer(64)
    n = lib.f5_debug_last_attn_kernel(buf, 64)
    name = buf.value.decode()
    assert n == len(name)
    return name


class knobs:
    """f5_debug_set_attn_wide / _kvsplit for one launch; the automatic rule is back afterwards whatever happens.  The process default
    of pipe is pinned to 0 (the library's own default, which the transcription assumes) for the launch and left at 0."""

    def __init__(self, lib, wide, kvsplit):
        self.lib, self.wide, self.kvsplit = lib, wide, kvsplit

    def __enter__(self):
        E.check(self.lib.f5_debug_set_attn_pipe(0))
        E.check(self.lib.f5_debug_set_attn_wide(self.wide))
        E.check(self.lib.f5_debug_set_attn_kvsplit(self.kvsplit))

    def __exit__(self, *exc):
        E.check(self.lib.f5_debug_set_attn_pipe(0))
        E.check(self.lib.f5_debug_set_attn_wide(-1))
        E.check(self.lib.f5_debug_set_attn_kvsplit(-1))


def launch(lib, b, **twist):
    """one case through f5_op_attention_ex; twist bends single arguments (the refusal tests).  Returns the return code."""
    c = b["case"]
    hp, pipe, _, _ = c.knobs
    a = {"qk_hi": AM.qk_ptr_tensor(b, 0), "qk_lo": AM.qk_ptr_tensor(b, 1) if hp else None, "vt_hi": AM.vt_ptr_tensor(b, 0),
         "vt_lo": AM.vt_ptr_tensor(b, 1) if hp else None, "out_hi": b["out_hi"].ptr_tensor(), "out_lo": b["out_lo"].ptr_tensor(),
         "out8": b["out8"].ptr_tensor() if c.f8 else None, "out8s": b["out8s"].ptr_tensor() if c.f8 else None,
         "npad": c.npad, "ldqk": c.ldqk, "ldo": c.ldo, "ldo8": c.ldo8, "hp": hp}
    a.update(twist)
    return lib.f5_op_attention_ex(P(a["qk_hi"]), P(a["qk_lo"]), P(a["vt_hi"]), P(a["vt_lo"]), P(a["out_hi"]), P(a["out_lo"]), P(b["kv"]), c.B, c.H,
                                  c.N, a["npad"], c.D, C.c_float(AM.SCALE), a["hp"], a["ldqk"], a["ldo"], c.qpre, pipe, P(a["out8"]), P(a["out8s"]),
                                  a["ldo8"], stream())


def run_case(lib, c):
    """-> (kernel reached, findings).  The caller holds the operand mode."""
    b = AM.make_buffers(c, device=DEV)
    ref3 = AM.reference(b)
    _, _, wide, kvsplit = c.knobs
    with knobs(lib, wide, kvsplit):
        rc = launch(lib, b)
        name = last_kernel(lib)
    if rc != 0:
        return None, [f"refused: {lib.f5_last_error().decode()}"]
    torch.cuda.synchronize()
    bad = AM.check(b, ref3)
    if not b["mask_excess"] >= 100.0:          # the operands are drawn on the device: the margin of the masked keys is checked on every launch
        bad.append(f"masked keys exceed the legitimate logits by {b['mask_excess']:.1f} only")
    if name != c.kernel_name:
        bad.append(f"ran {name}, the transcription of the launcher's rule says {c.kernel_name}")
    USED["err"], USED["slope"] = max(USED["err"], b.get("worst", 0.0)), max(USED["slope"], b.get("slope", 0.0))
    return name, bad


# ---- the matrix --------------------------------------------------------------------------------------------------------------
CASES = AM.cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c.group, []).append(_c)
REACHED = set()          # (kernel name incl. +f8, operand type) over the whole module
USED = {"err": 0.0, "slope": 0.0}    # largest share of the element-wise bound / of the systematic-error allowance a launch used (printed)


def _gid(g):
    op, kernel, values, f8 = g
    return f"{op}-{kernel}-{values}{'-f8' if f8 else ''}"


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_matrix(lib, group):
    op = group[0]
    failures = []
    USED.update(err=0.0, slope=0.0)
    with operand_mode(op):
        assert lib.f5_op_get_operand_type() == (1 if op == "f16" else 0)
        for c in GROUPS[group]:
            name, bad = run_case(lib, c)
            if name is not None:
                REACHED.add((name, op))
            if bad:
                failures.append((c.id, bad))
    print(f"[attention matrix] {_gid(group)}: {len(GROUPS[group])} cases, {len(failures)} failed; largest |err| / bound {USED['err']:.3f}, "
          f"systematic error / allowance {USED['slope']:.3f}")
    assert not failures, failures[:5]


def test_matrix_reaches_every_instantiation():
    """All 16 (kernel, operand type) instantiations and all fp8 variants.  Reads the set test_matrix fills: it needs the whole module
    run in definition order in one process (as tests/test_gemm_matrix_gpu.py does) and fails under -k selection or reordering."""
    want = {(k, op) for op in AM.OPS for k in AM.KERNELS} | {(k + "+f8", op) for op in AM.OPS for k in AM.F8_KERNELS}
    assert want <= {(c.kernel_name, c.op) for c in CASES}
    print(f"[attention matrix] {len(REACHED)} (kernel, operand type) instantiations reached, {len(want)} expected")
    assert REACHED == want, (sorted(want - REACHED), sorted(REACHED - want))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refusals():
    hp = AM.make_case("bf16", "v2_hp", 2, 2, 130, 2, "gauss", 1)
    one = AM.make_case("f16", "v2", 2, 2, 130, 2, "gauss", 1)
    f8 = AM.make_case("bf16", "v2s_ks2", 2, 2, 130, 2, "gauss", 1, f8=True)
    yield "npad_not_64", one, lambda b: {"npad": one.npad + 32}
    yield "npad_below_seq_len", one, lambda b: {"npad": 128}
    yield "ldqk_not_8", one, lambda b: {"ldqk": one.ldqk + 4}
    yield "ldo_not_4", one, lambda b: {"ldo": one.ldo + 2}
    yield "hp_without_qk_lo", hp, lambda b: {"qk_lo": None}
    yield "hp_without_vt_lo", hp, lambda b: {"vt_lo": None}
    yield "hp_without_out_lo", hp, lambda b: {"out_lo": None}
    yield "hp_split_without_lo", AM.make_case("f16", "v2s_hp", 2, 2, 130, 2, "gauss", 1), lambda b: {"qk_lo": None}
    yield "out8_with_hp", hp, lambda b: {"out8": b["out8"].ptr_tensor(), "out8s": b["out8s"].ptr_tensor()}
    yield "out8_without_scales", f8, lambda b: {"out8s": None}
    yield "ldo8_not_4", f8, lambda b: {"ldo8": f8.ldo8 + 2}
    yield "null_q", one, lambda b: {"qk_hi": None}
    yield "null_v", one, lambda b: {"vt_hi": None}
    yield "null_out", one, lambda b: {"out_hi": None}


@pytest.mark.parametrize("name,c,twist", list(_refusals()), ids=[r[0] for r in _refusals()])
def test_illegal_requests_are_refused_and_touch_nothing(lib, name, c, twist):
    """the buffers are made for the legal case and one argument is bent, so that even a launcher that lets it through stays inside
    the allocations"""
    b = AM.make_buffers(c, device=DEV)
    _, _, wide, kvsplit = c.knobs
    with operand_mode(c.op), knobs(lib, wide, kvsplit):
        rc = launch(lib, b, **twist(b))
        msg = lib.f5_last_error().decode()
        reached = last_kernel(lib)
    torch.cuda.synchronize()
    print(f"[attention matrix] refusal {name}: rc={rc} kernel={reached!r} error={msg!r}")
    assert rc != 0 and msg.strip() and reached == "", (name, rc, msg, reached)
    for k in ("out_hi", "out_lo", "out8", "out8s"):
        assert b[k].guard_damage(interior_too=True) == 0, (name, k)


# ---- production shapes: the kernel name only --------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", AM.OPS)
@pytest.mark.parametrize("batch", [1, 2, 8, 32])
def test_production_shapes_reach_the_promised_kernel(lib, op, batch):
    """the 335M model (16 heads, N = 937, batch doubled for guidance, q pre-multiplied, kv_len set) under the automatic rule"""
    B, H, N, D = 2 * batch, 16, 937, 1024
    npad = AM.ceil64(N)
    dt = AM.op_dtype(op)
    qk = (torch.randn(B * N, 2 * D, device=DEV) * 0.2).to(dt)
    vt = torch.zeros(B * H, 64, npad, device=DEV, dtype=dt)
    vt[..., :N] = torch.randn(B * H, 64, N, device=DEV).to(dt)
    out = torch.zeros(B * N, D, device=DEV, dtype=dt)
    kv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    with operand_mode(op), knobs(lib, -1, -1):
        rc = lib.f5_op_attention_ex(P(qk), P(None), P(vt), P(None), P(out), P(None), P(kv), B, H, N, npad, D, C.c_float(AM.SCALE), 0, 2 * D, D, 1,
                                    -1, P(None), P(None), 0, stream())
        name = last_kernel(lib)
    torch.cuda.synchronize()
    print(f"[attention matrix] production batch {batch} {op}: {name}")
    assert rc == 0 and name == AM.PRODUCTION[batch] == AM.expected_kernel(B, H, N, 0, 1), (rc, name)
    assert bool(torch.isfinite(out.float()).all())
