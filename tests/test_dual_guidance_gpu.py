"""Dual guidance on the GPU (docs/dual_guidance.md): separate speaker and text CFG strengths per batch row,
k = (F + (F - T) a) + (T - N) c.

Op level: f5_op_ode_stage_dual (rows_per_vec = 37, nvec = 3, both operand types, guarded buffers, NaN on every side a selection must keep
out) and f5_op_pack_cond_text_dual with its keep twin against the two-branch kernels.  Engine level (TINY, B = 3, ragged 23 / 37 / 31):
the three predictions of f5_dit_forward_dual against the oracle's three forwards, f5_sample_dual against the reference helper
(tests/dual_guidance_ref.py) row by row, a == c against the rows route, row independence, graphs, editing, refusals and F5TTS.sample."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import dual_guidance_ref as DG
import rowops_matrix as RM
from f5test import DEV, E, O, P, TINY, operand_mode, report, rng, randn, stream, synthetic_weights
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths, time_grid, time_grid_rows
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-3                  # the project's mel-L1 gate
RPV, NVEC = 37, 3                  # rows per vector, vectors (tests/test_row_controls_gpu.py)
M = 2 * NVEC * RPV                 # two copies of the vectors: rows 111 .. 221 read the vectors of rows 0 .. 110
U = 2.0 ** -24                     # unit roundoff of fp32


def F(v):
    return C.c_float(v)


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _blocks():
    return [(r0, (r0 // RPV) % NVEC) for r0 in range(0, M, RPV)]


def _beq(a, b):
    return torch.equal(RM.bits(a.contiguous()).cpu(), RM.bits(b.contiguous()).cpu())


# ---- 1. ode_stage_dual -------------------------------------------------------------------------------------------------------------------
AUD, TXT = [3.0, 0.0, 1.5], [0.5, 0.0, 0.0]      # vector 1 is unguided (T and N are NaN there), vector 2 has c = 0 (N is NaN there)


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("mode", [0, 1])
def test_ode_stage_dual(lib, mode, op16):
    """kstore against an fp64 evaluation of the rule from the fp32 inputs.  The kernel computes d1 = fl(F - T), k1 = fma(d1, a, F),
    d2 = fl(T - N), k = fma(d2, c, k1): four roundings, each at most U = 2^-24 relative to its own result; the first and third reach k
    multiplied by |a| and |c|.  To first order |k - exact| <= U (|F - T| |a| + |k1| + |T - N| |c| + |k|); the factor 1 + 2^-20 covers the
    second-order terms.  A vector with c < 1e-5 stops at k1 (two roundings), an unguided one is F itself."""
    mel = 100
    r = rng(500 + mode)
    dts = [0.0506, 0.11, 0.0231]
    pred, base, tpred, npred = (randn(r, M, mel) for _ in range(4))
    for r0, v in _blocks():
        if v == 1:
            tpred[r0:r0 + RPV] = float("nan")
        if v in (1, 2):
            npred[r0:r0 + RPV] = float("nan")
    ks = [randn(r, M, mel) for _ in range(3)]
    d = {k: RM.pad_in(t, DEV) for k, t in dict(pred=pred, base=base, tp=tpred, np=npred, k1=ks[0], k2=ks[1], k3=ks[2]).items()}
    a_d, c_d, dt_d = (RM.pad_in(torch.tensor(x), DEV) for x in (AUD, TXT, dts))
    coef, div = (1.0, 6.0) if mode else (0.5, 1.0)
    kpt = [d["k1"], d["k2"], d["k3"]] if mode else [None] * 3
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        out, kst = RM.Out((M, mel), torch.float32, DEV, guard=mel), RM.Out((M, mel), torch.float32, DEV, guard=mel)
        hi, lo = RM.Out((M, 128), dt16, DEV, guard=128), RM.Out((M, 128), dt16, DEV, guard=128)
        E.check(lib.f5_op_ode_stage_dual(P(d["pred"]), P(d["tp"]), P(d["np"]), P(a_d), P(c_d), P(d["base"]), P(dt_d), RPV, NVEC, F(coef), F(div),
                                         mode, P(kst.t), P(kpt[0]), P(kpt[1]), P(kpt[2]), P(out.t), P(hi.t), P(lo.t), M, mel, stream()),
                "f5_op_ode_stage_dual")
        torch.cuda.synchronize()
        bad = out.guard_violations("out") + kst.guard_violations("kstore") + hi.guard_violations("xin_hi") + lo.guard_violations("xin_lo")
        assert not bad, bad
        k_got = kst.t.cpu()
        assert torch.isfinite(out.t).all() and torch.isfinite(k_got).all()
        worst = 0.0
        for r0, v in _blocks():
            sl = slice(r0, r0 + RPV)
            f64, t64, n64 = pred[sl].double(), tpred[sl].double(), npred[sl].double()
            a, c = float(np.float32(AUD[v])), float(np.float32(TXT[v]))
            if a < 1e-5 and c < 1e-5:
                assert _beq(k_got[sl], pred[sl]), (r0, v)                    # k = F by selection, NaN in T and N or not
            else:
                k1 = f64 + (f64 - t64) * a
                ref, bound = k1, U * ((f64 - t64).abs() * abs(a) + k1.abs())
                if c >= 1e-5:
                    ref = k1 + (t64 - n64) * c
                    bound = bound + U * ((t64 - n64).abs() * abs(c) + ref.abs())
                err = (k_got[sl].double() - ref).abs()
                bound = bound * (1 + 2.0 ** -20)
                assert bool((err <= bound).all()), (r0, v, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                assert not torch.equal(k_got[sl], pred[sl])
            # everything behind k: the scalar kernel fed this kstore as pred, without a null, bit for bit
            w_out, w_k = torch.empty((RPV, mel), device=DEV), torch.empty((RPV, mel), device=DEV)
            w_hi, w_lo = torch.empty((RPV, 128), dtype=dt16, device=DEV), torch.empty((RPV, 128), dtype=dt16, device=DEV)
            kk = [None if k is None else k[sl] for k in kpt]
            E.check(lib.f5_op_ode_stage(P(kst.t[sl]), P(None), F(0.0), P(None), P(d["base"][sl]), P(dt_d[v:]), F(coef), F(div), mode, P(w_k),
                                        P(kk[0]), P(kk[1]), P(kk[2]), P(w_out), P(w_hi), P(w_lo), RPV, mel, stream()), "f5_op_ode_stage")
            torch.cuda.synchronize()
            assert _beq(out.t[sl], w_out) and _beq(kst.t[sl], w_k), (r0, v)
            assert _beq(hi.t[sl], w_hi) and _beq(lo.t[sl], w_lo), (r0, v)
        print(f"ode_stage_dual [{op16}, mode {mode}]: worst |k - fp64| / bound = {worst:.3f}")
        # null side pointers: no text_pred is k = F, no null_pred leaves the (T - N) term out
        k2 = RM.Out((M, mel), torch.float32, DEV, guard=mel)
        o2 = RM.Out((M, mel), torch.float32, DEV, guard=mel)
        E.check(lib.f5_op_ode_stage_dual(P(d["pred"]), P(None), P(d["np"]), P(a_d), P(c_d), P(d["base"]), P(dt_d), RPV, NVEC, F(coef), F(div),
                                         mode, P(k2.t), P(kpt[0]), P(kpt[1]), P(kpt[2]), P(o2.t), P(None), P(None), M, mel, stream()), "no T")
        torch.cuda.synchronize()
        assert _beq(k2.t, d["pred"]) and not k2.guard_violations("k") and not o2.guard_violations("out")


def test_ode_stage_dual_refusals_launch_nothing(lib):
    r = rng(501)
    p_d = randn(r, M, 100).to(DEV)
    c_d = torch.ones(NVEC, device=DEV)
    out = RM.Out((M, 100), torch.float32, DEV)
    ok = dict(pred=p_d, base=p_d, out=out.t, aud=c_d, txt=c_d, dt=c_d, rpv=RPV, nvec=NVEC, mel=100)
    cases = [(dict(pred=None), "pred is null"), (dict(base=None), "base is null"), (dict(out=None), "out is null"),
             (dict(aud=None), "null audio_cfg_rows / text_cfg_rows"), (dict(txt=None), "null audio_cfg_rows / text_cfg_rows"),
             (dict(dt=None), "dt_rows is null"), (dict(rpv=0), "rows_per_vec must be >= 1"), (dict(nvec=0), "nvec must be >= 1"),
             (dict(mel=129), "mel_dim must be <= 128")]
    seen = set()
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.f5_op_ode_stage_dual(P(a["pred"]), P(p_d), P(p_d), P(a["aud"]), P(a["txt"]), P(a["base"]), P(a["dt"]), a["rpv"], a["nvec"], F(1.0),
                                      F(1.0), 0, P(None), P(None), P(None), P(None), P(a["out"]), P(None), P(None), M, a["mel"], stream())
        err = lib.f5_last_error().decode()
        assert rc != 0 and msg in err, (change, rc, err)
        seen.add(re.sub(r"\d+", "#", err))
    assert len(seen) == len(cases) - 1                       # each refusal its own message (the two strength vectors share theirs)
    torch.cuda.synchronize()
    assert bool((RM.bits(out.t) == RM.SENT32).all())


# ---- 2. pack_cond_text_dual ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("keep_form", [0, 1])
def test_pack_cond_text_dual(lib, keep_form, op16):
    B, N, mel, DT = 3, 37, 100, 256
    ld = 128 + DT
    r = rng(510 + keep_form)
    cond, te = randn(r, B, N, mel, scale=3.0), randn(r, 2, B, N, DT)
    if keep_form:
        keep = torch.from_numpy((r.random((B, N)) < 0.6).astype(np.uint8))
        keep[0, 0], keep[1, :], keep[2, N - 1] = 0, 0, 1
    else:
        lens = torch.tensor([12, 0, 37], dtype=torch.int32)
        keep = (torch.arange(N)[None, :] < lens[:, None]).to(torch.uint8)
    cond_nan = torch.where(keep[..., None] != 0, cond, torch.full_like(cond, float("nan")))      # NaN in EVERY dropped frame
    d_cond, d_te = RM.pad_in(cond_nan, DEV), RM.pad_in(te, DEV)
    d_sel = RM.pad_in(keep, DEV) if keep_form else RM.pad_in(lens, DEV)
    dt16 = RM.op_dtype(op16)
    dual = lib.f5_op_pack_cond_text_dual_keep if keep_form else lib.f5_op_pack_cond_text_dual
    two = lib.f5_op_pack_cond_text_keep if keep_form else lib.f5_op_pack_cond_text
    with operand_mode(op16):
        for want_lo in (True, False):
            hi, lo = RM.Out((3, B, N, ld), dt16, DEV, guard=ld), RM.Out((3, B, N, ld), dt16, DEV, guard=ld)
            E.check(dual(P(d_cond), P(d_sel), P(d_te), P(hi.t), P(lo.t if want_lo else None), B, N, mel, DT, stream()), "pack_cond_text_dual")
            w_hi, w_lo = RM.Out((2, B, N, ld), dt16, DEV, guard=ld), RM.Out((2, B, N, ld), dt16, DEV, guard=ld)
            E.check(two(P(d_cond), P(d_sel), P(d_te), P(w_hi.t), P(w_lo.t), B, N, mel, DT, 0, stream()), "pack_cond_text")
            torch.cuda.synchronize()
            bad = hi.guard_violations("hi") + lo.guard_violations("lo")
            assert not bad, bad
            pairs = [(hi.t, w_hi.t)] + ([(lo.t, w_lo.t)] if want_lo else [])
            for got, want in pairs:
                assert torch.isfinite(got.float()).all()
                assert _beq(got[:2], want)                                     # F, N: the two-branch kernel, bit for bit
                assert bool((RM.bits(got[2, :, :, :128]) == 0).all())          # T: zero cond columns ...
                assert _beq(got[2, :, :, 128:], got[0, :, :, 128:])            # ... and branch 0's text columns
                assert not _beq(got[1, :, :, 128:], got[0, :, :, 128:])
            assert bool((RM.bits(hi.t[0, :, :, :mel]) != 0).any())             # branch 0 does carry the kept conditioning
            if not want_lo:
                assert bool((RM.bits(lo.t) == RM.SENT16).all())
    out = RM.Out((3, B, N, ld), torch.bfloat16, DEV)
    for args, msg in (((P(None), P(d_sel), P(d_te), P(out.t), P(None), B, N, mel, DT), "null pointer"),
                      ((P(d_cond), P(None), P(d_te), P(out.t), P(None), B, N, mel, DT), "keep is null" if keep_form else "lens is null"),
                      ((P(d_cond), P(d_sel), P(d_te), P(out.t), P(None), B, N, 129, DT), "mel_dim must be <= 128"),
                      ((P(d_cond), P(d_sel), P(d_te), P(out.t), P(None), 0, N, mel, DT), "bad sizes")):
        rc = dual(*args, stream())
        assert rc != 0 and msg in lib.f5_last_error().decode(), (msg, lib.f5_last_error().decode())
    torch.cuda.synchronize()
    assert bool((RM.bits(out.t) == RM.SENT16).all())


# ---- engine level -------------------------------------------------------------------------------------------------------------------------
B, N, NT, NREF = 3, 37, 10, 12
DURS = [23, 37, 31]
A_ROWS, C_ROWS = [3.0, 0.0, 0.0], [0.5, 0.0, 2.0]          # (a, c) per row: both, neither, text alone


@pytest.fixture(scope="module")
def tiny_weights():
    return synthetic_weights(TINY, seed=42)


@pytest.fixture(scope="module")
def models(tiny_weights):
    out = {}
    for prec in ("bf16x3", "f16"):
        m = DiT.from_config(TINY, precision=prec, device=DEV)
        m.load_weights(tiny_weights)
        out[prec] = m
    return out


@pytest.fixture(scope="module")
def inputs():
    r = rng(77)
    cond = randn(r, B, NREF, TINY.mel_dim)
    text = torch.from_numpy(r.integers(0, TINY.text_num_embeds, (B, NT)).astype(np.int32))
    text[1, 8:], text[2, 6:] = -1, -1
    y0 = torch.zeros((B, N, TINY.mel_dim))
    for i, d in enumerate(DURS):
        y0[i, :d] = torch.from_numpy(r.standard_normal((TINY.mel_dim, d)).astype(np.float32).T)
    return cond, text, y0


@pytest.fixture(scope="module")
def oracle(tiny_weights):
    return O.DiTOracle(TINY, tiny_weights)


def _engine_args(inputs):
    """what F5TTS.sample hands the engine for `inputs`"""
    cond, text, y0 = inputs
    text_c, lens, dur, nmax = prepare_lengths(text, NREF, B, torch.tensor(DURS), None, 4096, "euler")
    assert nmax == N and dur.tolist() == DURS
    cond_p = torch.zeros((B, N, TINY.mel_dim), device=DEV)
    cond_p[:, :NREF] = cond.to(DEV)
    return text_c.to(DEV).contiguous(), cond_p, lens.tolist(), dur.tolist(), y0.to(DEV).contiguous()


_ref = {}


def _reference(oracle, inputs, method, steps, audio, text_strength):
    """the helper's result for these strengths, computed once"""
    key = (method, steps, tuple(audio), tuple(text_strength))
    if key not in _ref:
        cond, text, y0 = inputs
        _ref[key] = DG.dual_sample(oracle, cond, text, DURS, y0, steps, method, audio, text_strength)
    return _ref[key]


# ---- 3. dit_forward_dual --------------------------------------------------------------------------------------------------------------------
def test_dit_forward_dual_against_the_three_oracle_forwards(models, tiny_weights, oracle, inputs):
    """bounds: those of the f5_dit_forward tests for the same precision (tests/test_model_gpu.py, tests/test_row_controls_gpu.py): bf16x3
    2e-4, f16 1e-3 against the fp32 oracle and 3e-4 against the fp16-emulating one, each times max(1, mean |reference|)"""
    cond, text, y0 = inputs
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    times = [0.1, 0.5, 0.9]
    aux = DG.aux_of(oracle, cond, text, DURS, y0)
    want = dict(fp32=DG.three_forwards(oracle, aux, y0, torch.tensor(times)))
    want["f16emu"] = DG.three_forwards(O.DiTOracle(TINY, tiny_weights, emulate_f16=True), aux, y0, torch.tensor(times))
    for prec, bounds in (("bf16x3", dict(fp32=2e-4)), ("f16", dict(fp32=1e-3, f16emu=3e-4))):
        eng = models[prec].engine
        pred, null, tpred = eng.dit_forward(y0_d, text_d, cond_p, lens, durs, times, use_mask=True, audio_cfg_strength=1.0)
        torch.cuda.synchronize()
        assert eng.saturation_events == 0
        for ref_name, tol in bounds.items():
            for nm, got, ref in zip(("F", "T", "N"), (pred, tpred, null), want[ref_name]):
                assert torch.isfinite(got).all()
                _, mean, refm = report(f"dit_forward_dual[{prec}] {nm} vs oracle[{ref_name}]", got.cpu(), ref)
                assert mean <= tol * max(1.0, refm), (prec, nm, ref_name)
        # the three states are three different predictions; F / N against the two-branch forward: both are within the bound of the same
        # oracle result, so within twice the bound of each other
        assert not torch.equal(pred, tpred) and not torch.equal(tpred, null)
        p2, n2 = eng.dit_forward(y0_d, text_d, cond_p, lens, durs, times, cfg_strength=2.0, use_mask=True)
        for nm, got, ref in (("F", pred, p2), ("N", null, n2)):
            _, mean, refm = report(f"dit_forward_dual[{prec}] {nm} vs f5_dit_forward_rows", got.cpu(), ref.cpu())
            assert mean <= 2 * bounds["fp32"] * max(1.0, refm)


# ---- 4. sample with per-row strengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps", [("euler", 5), ("midpoint", 4), ("rk4", 3)])
def test_sample_dual_against_the_reference_helper(models, oracle, inputs, method, steps):
    """Measured on one MI355X (bf16x3, mean |delta| of row b, final mel / trajectory): see docs/dual_guidance.md."""
    cond, text, y0 = inputs
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    want, want_t = _reference(oracle, inputs, method, steps, A_ROWS, C_ROWS)
    # the comparison cannot pass by indifference: with the strengths swapped the helper itself lands far from its own result
    swap, _ = _reference(oracle, inputs, method, steps, C_ROWS, A_ROWS)
    for b in (0, 2):                                                         # (row 1 is (0, 0): nothing to swap)
        far = float((swap[b, lens[b]:DURS[b]] - want[b, lens[b]:DURS[b]]).abs().mean())
        print(f"helper, strengths swapped [{method}] row {b}: mean |delta| = {far:.3f}")
        assert far > 100 * MEL_L1_TOL, (method, b, far)
    eng = models["bf16x3"].engine
    out, traj = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(steps, -1.0), method=method, cfg_strength=C_ROWS, use_mask=True,
                           use_graph=False, audio_cfg_strength=A_ROWS)
    torch.cuda.synchronize()
    assert traj.shape == (steps, B, N, TINY.mel_dim) and torch.isfinite(out).all()
    for b in range(B):
        _, l1, _ = report(f"dual vs helper [{method}] row {b} final mel", out[b].cpu(), want[b])
        _, l1t, _ = report(f"dual vs helper [{method}] row {b} trajectory", traj[:, b].cpu(), want_t[:, b])
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (method, b)
        assert torch.equal(out[b, :lens[b]].cpu(), cond_p[b, :lens[b]].cpu())      # kept frames are cond, bit for bit
    assert not torch.equal(out[0], out[1])


# ---- 5. a == c ------------------------------------------------------------------------------------------------------------------------------
def test_equal_strengths_agree_with_the_rows_route(models, inputs):
    """a == c per row is algebraically the single rule F + (F - N) c: within the gate of f5_sample_rows, not bit for bit"""
    eng = models["bf16x3"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    cfgs = [2.0, 0.0, 1.3]
    for method, steps in (("euler", 5), ("rk4", 3)):
        kw = dict(method=method, cfg_strength=cfgs, use_mask=True, use_graph=False)
        want, want_t = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), **kw)]
        got, got_t = eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), audio_cfg_strength=cfgs, **kw)
        torch.cuda.synchronize()
        _, l1, _ = report(f"dual a == c vs f5_sample_rows [{method}] final mel", got.cpu(), want.cpu())
        _, l1t, _ = report(f"dual a == c vs f5_sample_rows [{method}] trajectory", got_t.cpu(), want_t.cpu())
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, method
        assert torch.equal(got[1], want[1])                  # the unguided row takes k = F on both routes
    # no row guided: the dual route runs F alone (nb = 1 on the three-branch plan), as the rows route does
    kw = dict(method="midpoint", cfg_strength=[0.0] * B, use_mask=True, use_graph=False)
    want, want_t = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), **kw)]
    got, got_t = eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), audio_cfg_strength=0.0, **kw)
    torch.cuda.synchronize()
    _, l1, _ = report("dual, no row guided, vs f5_sample_rows [midpoint] final mel", got.cpu(), want.cpu())
    _, l1t, _ = report("dual, no row guided, vs f5_sample_rows [midpoint] trajectory", got_t.cpu(), want_t.cpu())
    assert torch.isfinite(got).all() and l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL


# ---- 6. row independence ----------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent(models, inputs):
    eng = models["f16"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    grids = time_grid_rows(4, [-1.0, None, -0.5])
    res = []
    for aud, txt in ((A_ROWS, C_ROWS), ([A_ROWS[0], 1.7, A_ROWS[2]], [C_ROWS[0], 0.4, C_ROWS[2]])):
        out, traj = eng.sample(text, cond_p, lens, durs, y0, grids, method="midpoint", cfg_strength=txt, use_mask=True, use_graph=False,
                               audio_cfg_strength=aud)
        torch.cuda.synchronize()
        res.append((out.clone(), traj.clone()))
    (oa, ta), (ob, tb) = res
    assert eng.saturation_events == 0
    for b in (0, 2):
        assert torch.equal(oa[b], ob[b]) and torch.equal(ta[:, b], tb[:, b]), b
    assert not torch.equal(oa[1], ob[1]) and not torch.equal(ta[1:, 1], tb[1:, 1])
    assert torch.equal(ta[0], y0) and torch.equal(tb[0], y0)


# ---- 7. graphs --------------------------------------------------------------------------------------------------------------------------------
def test_one_graph_serves_every_pair_of_strengths(models, inputs):
    eng = models["f16"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 4
    t = time_grid(steps, -1.0)
    sets = {"a": (A_ROWS, C_ROWS), "b": ([0.7, 2.5, 1.0], [1.1, 0.3, 0.0])}
    kw = dict(method="euler", use_mask=True)
    eager = {k: [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, t, cfg_strength=c, audio_cfg_strength=a, use_graph=False, **kw)]
             for k, (a, c) in sets.items()}
    rows = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, t, cfg_strength=C_ROWS, use_graph=False, **kw)]
    torch.cuda.synchronize()
    assert not torch.equal(eager["a"][0], eager["b"][0]) and not torch.equal(eager["a"][0], rows[0])
    c0 = eng.graph_count()

    def run(key):
        a, c = sets[key]
        out, traj = eng.sample(text, cond_p, lens, durs, y0, t, cfg_strength=c, audio_cfg_strength=a, use_graph=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, eager[key][0]) and torch.equal(traj, eager[key][1]), key          # replay equals eager, bitwise

    run("a")
    assert eng.graph_count() == c0 + 1
    run("b")
    assert eng.graph_count() == c0 + 1                                   # other strengths, the same graph
    out, traj = eng.sample(text, cond_p, lens, durs, y0, t, cfg_strength=C_ROWS, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert eng.graph_count() == c0 + 2                                   # the rows route of the same shape: its own entry, its own bits
    assert torch.equal(out, rows[0]) and torch.equal(traj, rows[1])
    run("a")
    assert eng.graph_count() == c0 + 2                                   # ... which did not evict the dual graph


# ---- 8. editing -------------------------------------------------------------------------------------------------------------------------------
def test_prefix_keep_mask_equals_no_mask(models, inputs):
    eng = models["f16"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    keep = (torch.arange(N, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None])
    for method, steps in (("euler", 4), ("rk4", 3)):
        kw = dict(method=method, cfg_strength=C_ROWS, audio_cfg_strength=A_ROWS, use_mask=True, use_graph=False)
        want, want_t = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), **kw)]
        got, got_t = eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), cond_keep=keep, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(got_t, want_t), method
    # ... and a mask that keeps other frames is another result
    keep2 = keep.clone()
    keep2[:, 0] = False
    other, _ = eng.sample(text, cond_p, lens, durs, y0, time_grid(3, -1.0), cond_keep=keep2, **kw)
    assert not torch.equal(other, want)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_sample_dual_refusals_launch_nothing(models, inputs):
    eng = models["bf16x3"].engine
    lib = eng.lib
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 3
    ws = eng.workspace(B, N, NT, steps, "euler", rows="dual")
    out = torch.full_like(cond_p, -12345.0)
    a, keep = eng._args(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), steps, "euler", 2.0, True, False, out, None, ws)
    tr = time_grid_rows(steps, [-1.0, None, -0.5])
    ar, cr = np.asarray(A_ROWS, np.float32), np.asarray(C_ROWS, np.float32)
    tr_nan, ar_nan, cr_inf = tr.copy(), ar.copy(), cr.copy()
    tr_nan[1, 2], ar_nan[0], cr_inf[2] = np.nan, np.nan, np.inf
    rows_b, dual_b = C.c_size_t(), C.c_size_t()
    E.check(lib.f5_workspace_bytes_rows(eng._h, B, N, NT, steps, 0, C.byref(rows_b)))
    E.check(lib.f5_workspace_bytes_dual(eng._h, B, N, NT, steps, 0, C.byref(dual_b)))
    assert dual_b.value > rows_b.value and ws.numel() >= dual_b.value
    graphs = eng.graph_count()

    def refused(dc, msg):
        rc = lib.f5_sample_dual(eng._h, C.byref(a), None if dc is None else C.byref(dc), stream())
        err = lib.f5_last_error().decode()
        assert rc != 0 and msg in err, (msg, rc, err)

    D = E.F5DualControls
    refused(None, "controls is null")
    refused(D(0, cr.ctypes.data, ar.ctypes.data, 0), "controls.t_rows is null")
    refused(D(tr.ctypes.data, 0, ar.ctypes.data, 0), "controls.text_cfg_rows is null")
    refused(D(tr.ctypes.data, cr.ctypes.data, 0, 0), "controls.audio_cfg_rows is null")
    refused(D(tr_nan.ctypes.data, cr.ctypes.data, ar.ctypes.data, 0), "t_rows[1][2] is not finite")
    refused(D(tr.ctypes.data, cr_inf.ctypes.data, ar.ctypes.data, 0), "text_cfg_rows[2] is not finite")
    refused(D(tr.ctypes.data, cr.ctypes.data, ar_nan.ctypes.data, 0), "audio_cfg_rows[0] is not finite")
    ok = D(tr.ctypes.data, cr.ctypes.data, ar.ctypes.data, 0)
    a.workspace_bytes = rows_b.value                                      # the rows plan is too short for three branches
    refused(ok, "f5_workspace_bytes_dual")
    a.workspace_bytes = ws.numel()
    a.method = 7
    refused(ok, "Unknown method")                                         # ... and everything f5_sample refuses
    a.method = 0
    for name, value, back, msg in (("null_keeps_cond", 1, 0, "null_keeps_cond = 1"), ("ln_fold", 1, -1, "ln_fold = 1")):
        eng.set_option(name, value)
        try:
            refused(ok, msg)
            with pytest.raises(RuntimeError, match="f5_dit_forward_dual.*" + msg):
                eng.dit_forward(y0, text, cond_p, lens, durs, 0.5, audio_cfg_strength=1.0)
        finally:
            eng.set_option(name, back)
    with pytest.raises(RuntimeError, match="f5_sample_dual.*audio_cfg_rows\\[1\\] is not finite"):
        eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), method="euler", cfg_strength=2.0, use_graph=False, out=out,
                   audio_cfg_strength=[1.0, float("nan"), 0.0])
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all()) and eng.graph_count() == graphs
    del keep


def test_mxfp8_engine_refuses_dual_guidance(tiny_weights, inputs):
    eng = E.Engine(TINY, precision="mxfp8", device=DEV)
    eng.load_weights(tiny_weights)
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    out = torch.full_like(cond_p, -12345.0)
    traj = torch.full((4, B, N, TINY.mel_dim), -12345.0, device=DEV)
    with pytest.raises(RuntimeError, match="f5_sample_dual.*mxfp8"):
        eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), method="euler", cfg_strength=C_ROWS, use_mask=True, use_graph=False,
                   out=out, trajectory=traj, audio_cfg_strength=A_ROWS)
    with pytest.raises(RuntimeError, match="f5_dit_forward_dual.*mxfp8"):
        eng.dit_forward(y0, text, cond_p, lens, durs, 0.5, audio_cfg_strength=1.0)
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all()) and bool((traj == -12345.0).all())        # nothing was launched


def test_split_halves_get_their_rows_of_both_strengths(tiny_weights, inputs):
    """Engine._sample_split: each half batch gets its rows of the pair; utterances do not interact, so the bits are the unsplit call's"""
    m = DiT.from_config(TINY, precision="f16", device=DEV)
    m.load_weights(tiny_weights)
    eng = m.engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    kw = dict(method="euler", cfg_strength=C_ROWS, audio_cfg_strength=A_ROWS, use_mask=True)
    want = {g: [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), use_graph=g, **kw)] for g in (False, True)}
    eng.split_batch = 2
    n0 = eng.split_events
    for rep in range(2):                               # the first call of a shape runs the halves one after the other, then concurrently
        for g, (wo, wt) in want.items():
            out, traj = eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), use_graph=g, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out, wo) and torch.equal(traj, wt), (rep, g)
    assert eng.split_events == n0 + 4 and eng.saturation_events == 0


# ---- 10. F5TTS.sample ---------------------------------------------------------------------------------------------------------------------------
def test_f5tts_sample_equals_the_engine_call(models, inputs):
    cond, text, y0 = inputs
    eng = models["bf16x3"].engine
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    f5 = F5TTS(transformer=models["bf16x3"])
    kw = dict(duration=torch.tensor(DURS), steps=4, method="midpoint", y0=y0, use_graph=False, sway_sampling_coef=-1.0)
    got, got_t = [x.clone() for x in f5.sample(cond, text, cfg_strength=C_ROWS, audio_cfg_strength=A_ROWS, **kw)]
    want, want_t = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(4, -1.0), method="midpoint", cfg_strength=C_ROWS, use_mask=True,
                              use_graph=False, audio_cfg_strength=A_ROWS)
    assert torch.equal(got, want) and torch.equal(got_t, want_t)
    # a scalar strength takes the dual route too, and is the per-row call with that value in every row
    got, _ = [x.clone() for x in f5.sample(cond, text, cfg_strength=0.5, audio_cfg_strength=3.0, **kw)]
    want, _ = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(4, -1.0), method="midpoint", cfg_strength=[0.5] * B, use_mask=True,
                         use_graph=False, audio_cfg_strength=[3.0] * B)
    assert torch.equal(got, want)
    # without the argument: the call it was
    got, _ = [x.clone() for x in f5.sample(cond, text, cfg_strength=2.0, **kw)]
    want, _ = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(4, -1.0), method="midpoint", cfg_strength=2.0, use_mask=True, use_graph=False)
    assert torch.equal(got, want)
