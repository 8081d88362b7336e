"""Per-request sampling controls on the GPU (docs/row_controls.md): time grid and guidance strength indexed by batch row.

Op level: f5_op_ode_stage_rows and f5_op_resid_gate_ln_rows against the kernels they generalise, block of rows by block of rows and bit
for bit, at shapes whose row blocks align with no wave or workgroup multiple (rows_per_vec = 37, nvec = 3, M = 2 * 3 * 37: both branch
copies), both operand types, guarded buffers, NaN planted wherever a selection must keep it out.  Engine level (TINY, B = 3, ragged
23 / 37 / 31): the reference's (b,) time through DiT(row_times=True) as one forward, row independence, one hipGraph for all control
values, f5_sample_rows against the scalar route and the CPU oracle row by row, uniform controls, the sequence arguments of
F5TTS.sample and the refusal of the MX-fp8 mode."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import rowops_matrix as RM
from f5test import DEV, E, O, P, TINY, DiTConfig, operand_mode, report, rng, randn, stream, synthetic_weights
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths, time_grid, time_grid_rows
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-3                  # the project's mel-L1 gate (tests/test_reference_golden_gpu.py)
RPV, NVEC = 37, 3                  # rows per vector, vectors: a row block is no multiple of a wave's 4 rows per workgroup
M = 2 * NVEC * RPV                 # both branch copies: rows 111 .. 221 read the vectors of rows 0 .. 110
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def F(v):
    return C.c_float(v)


def Z(v):
    return C.c_size_t(v)


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _blocks():
    """(first row, vector) of every block of RPV rows"""
    return [(r0, (r0 // RPV) % NVEC) for r0 in range(0, M, RPV)]


def _beq(a, b):
    return torch.equal(RM.bits(a.contiguous()).cpu(), RM.bits(b.contiguous()).cpu())


# ---- 1. ode_stage_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("with_null", [1, 0])
@pytest.mark.parametrize("mode", [0, 1])
def test_ode_stage_rows_equals_the_scalar_kernel_block_by_block(lib, mode, with_null, op16):
    mel = 100
    r = rng(100 + 10 * mode + with_null)
    cfgs, dts = [2.0, 0.0, 1.3], [0.0506, 0.11, 0.0231]        # vector 1 is unguided: its null_pred is NaN and must reach nothing
    pred, base, null = randn(r, M, mel), randn(r, M, mel), randn(r, M, mel)
    for r0, v in _blocks():
        if v == 1:
            null[r0:r0 + RPV] = float("nan")
    ks = [randn(r, M, mel) for _ in range(3)]
    d = {k: RM.pad_in(t, DEV) for k, t in dict(pred=pred, base=base, null=null, k1=ks[0], k2=ks[1], k3=ks[2]).items()}
    cfg_d, dt_d = RM.pad_in(torch.tensor(cfgs), DEV), RM.pad_in(torch.tensor(dts), DEV)
    coef, div = (1.0, 6.0) if mode else (0.5, 1.0)
    kpt = [d["k1"], d["k2"], d["k3"]] if mode else [None] * 3
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        out, kst = RM.Out((M, mel), torch.float32, DEV, guard=mel), RM.Out((M, mel), torch.float32, DEV, guard=mel)
        hi, lo = RM.Out((M, 128), dt16, DEV, guard=128), RM.Out((M, 128), dt16, DEV, guard=128)
        E.check(lib.f5_op_ode_stage_rows(P(d["pred"]), P(d["null"] if with_null else None), P(cfg_d), P(d["base"]), P(dt_d), RPV, NVEC, F(coef),
                                         F(div), mode, P(kst.t), P(kpt[0]), P(kpt[1]), P(kpt[2]), P(out.t), P(hi.t), P(lo.t), M, mel, stream()),
                "f5_op_ode_stage_rows")
        torch.cuda.synchronize()
        bad = out.guard_violations("out") + kst.guard_violations("kstore") + hi.guard_violations("xin_hi") + lo.guard_violations("xin_lo")
        assert not bad, bad
        assert torch.isfinite(out.t).all() and torch.isfinite(kst.t).all()
        for r0, v in _blocks():
            sl = slice(r0, r0 + RPV)
            w_out, w_k = torch.empty((RPV, mel), device=DEV), torch.empty((RPV, mel), device=DEV)
            w_hi, w_lo = torch.empty((RPV, 128), dtype=dt16, device=DEV), torch.empty((RPV, 128), dtype=dt16, device=DEV)
            guided = with_null and cfgs[v] >= 1e-5
            nul = d["null"][sl] if guided else None
            kk = [None if k is None else k[sl] for k in kpt]
            E.check(lib.f5_op_ode_stage(P(d["pred"][sl]), P(nul), F(cfgs[v]), P(None), P(d["base"][sl]), P(dt_d[v:]), F(coef), F(div), mode,
                                        P(w_k), P(kk[0]), P(kk[1]), P(kk[2]), P(w_out), P(w_hi), P(w_lo), RPV, mel, stream()), "f5_op_ode_stage")
            torch.cuda.synchronize()
            tag = (r0, v)
            assert _beq(out.t[sl], w_out) and _beq(kst.t[sl], w_k), tag
            assert _beq(hi.t[sl], w_hi) and _beq(lo.t[sl], w_lo), tag
        if with_null:                                   # the guided blocks did use their null_pred
            assert not torch.equal(kst.t[:RPV].cpu(), pred[:RPV])
            assert torch.equal(kst.t[RPV:2 * RPV].cpu(), pred[RPV:2 * RPV])


# ---- 2. / 3. resid_gate_ln_rows -------------------------------------------------------------------------------------------------------
def _vectors(r, D, stride):
    """[NVEC][stride] with NaN between the vectors: a read past a vector's D columns would bring it along"""
    v = torch.full((NVEC, stride), float("nan"))
    v[:, :D] = randn(r, NVEC, D, scale=0.5)
    return v


def _ln_ref_block(lib, x_block, scale_vec, shift_vec, D, dt16, want_lo=True):
    w_hi = torch.empty((x_block.shape[0], D), dtype=dt16, device=DEV)
    w_lo = torch.empty((x_block.shape[0], D), dtype=dt16, device=DEV) if want_lo else None
    E.check(lib.f5_op_ln_modulate(P(x_block), P(scale_vec), P(shift_vec), P(w_hi), P(w_lo), x_block.shape[0], D, stream()), "f5_op_ln_modulate")
    torch.cuda.synchronize()
    return w_hi, w_lo


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("D", [256, 1024])
def test_ln_rows_without_y_equals_ln_modulate_block_by_block(lib, D, op16):
    r = rng(200 + D)
    stride = D + 8
    x = randn(r, M, D, scale=1.5) + randn(r, M, 1)
    scale, shift = _vectors(r, D, stride), _vectors(r, D, stride)
    x_d, sc_d, sh_d = RM.pad_in(x, DEV), RM.pad_in(scale, DEV), RM.pad_in(shift, DEV)
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        for want_lo in (True, False):
            hi, lo = RM.Out((M, D), dt16, DEV, guard=D), RM.Out((M, D), dt16, DEV, guard=D)
            x_run = RM.Out((M, D), torch.float32, DEV, guard=D, init=x_d)
            E.check(lib.f5_op_resid_gate_ln_rows(P(None), P(x_run.t), P(None), P(None), P(sc_d), P(sh_d), P(hi.t), P(lo.t if want_lo else None), M, D,
                                                 RPV, NVEC, Z(stride), stream()), "f5_op_resid_gate_ln_rows")
            torch.cuda.synchronize()
            bad = hi.guard_violations("hi") + lo.guard_violations("lo") + x_run.guard_violations("x")
            assert not bad, bad
            assert _beq(x_run.t, x_d)                                       # without y the residual stream is only read
            if not want_lo:
                assert bool((RM.bits(lo.t) == RM.SENT16).all())
            for r0, v in _blocks():
                sl = slice(r0, r0 + RPV)
                w_hi, w_lo = _ln_ref_block(lib, x_d[sl], sc_d[v, :D].contiguous(), sh_d[v, :D].contiguous(), D, dt16, want_lo)
                assert _beq(hi.t[sl], w_hi), (r0, v, want_lo)
                if want_lo:
                    assert _beq(lo.t[sl], w_lo), (r0, v)


@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("D", [256, 1024])
def test_resid_gate_ln_rows_with_y(lib, D, op16):
    r = rng(300 + D)
    stride = D + 8
    x, y = randn(r, M, D, scale=1.5), randn(r, M, D)
    gate, scale, shift = _vectors(r, D, stride), _vectors(r, D, stride), _vectors(r, D, stride)
    keep = torch.from_numpy((r.random(M) < 0.7).astype(np.uint8))
    keep[0], keep[M - 1], keep[RPV] = 0, 0, 1
    y_nan = torch.where(keep[:, None] != 0, y, torch.full_like(y, float("nan")))      # NaN in EVERY dropped row
    x_d, g_d, sc_d, sh_d, k_d = (RM.pad_in(t, DEV) for t in (x, gate, scale, shift, keep))
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        for use_keep, with_ln in ((True, True), (False, True), (True, False)):
            y_d = RM.pad_in(y_nan if use_keep else y, DEV)
            kmask = keep if use_keep else torch.ones(M, dtype=torch.uint8)
            hi, lo = RM.Out((M, D), dt16, DEV, guard=D), RM.Out((M, D), dt16, DEV, guard=D)
            x_run = RM.Out((M, D), torch.float32, DEV, guard=D, init=x_d)
            E.check(lib.f5_op_resid_gate_ln_rows(P(y_d), P(x_run.t), P(g_d), P(k_d if use_keep else None), P(sc_d if with_ln else None),
                                                 P(sh_d if with_ln else None), P(hi.t), P(lo.t), M, D, RPV, NVEC, Z(stride), stream()),
                    "f5_op_resid_gate_ln_rows")
            torch.cuda.synchronize()
            tag = (use_keep, with_ln)
            bad = hi.guard_violations("hi") + lo.guard_violations("lo") + x_run.guard_violations("x")
            assert not bad, bad
            x_new = x_run.t.cpu()
            assert torch.isfinite(x_new).all(), tag
            # x_new against fp64 x + gate * t: one fused multiply-add, within 1 ulp of the exact value
            vec = torch.tensor([v for _, v in _blocks() for _ in range(RPV)])
            g_rows = gate[vec, :D].double()
            t_rows = torch.where(kmask[:, None] != 0, y, torch.zeros_like(y)).double()
            ref = x.double() + g_rows * t_rows
            ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))
            err = (x_new.double() - ref).abs()
            assert bool((err <= ulp).all()), (tag, float((err / ulp).max()))
            dropped = kmask == 0
            assert _beq(x_new[dropped], x[dropped]), tag                       # a dropped row keeps x exactly, NaN in its y or not
            assert not torch.equal(x_new[~dropped], x[~dropped])
            if not with_ln:                                                      # no LN output: nothing is written
                assert bool((RM.bits(hi.t) == RM.SENT16).all()) and bool((RM.bits(lo.t) == RM.SENT16).all())
                continue
            for r0, v in _blocks():                                              # the LN of the x_new the kernel wrote, bit for bit
                sl = slice(r0, r0 + RPV)
                w_hi, w_lo = _ln_ref_block(lib, x_run.t[sl], sc_d[v, :D].contiguous(), sh_d[v, :D].contiguous(), D, dt16)
                assert _beq(hi.t[sl], w_hi) and _beq(lo.t[sl], w_lo), (tag, r0, v)


def test_host_refusals_launch_nothing(lib):
    D, stride = 256, 256
    r = rng(400)
    x, y = randn(r, M, D), randn(r, M, D)
    vec = randn(r, NVEC, stride)
    x_d, y_d, v_d = x.to(DEV), y.to(DEV), vec.to(DEV)
    hi, lo = RM.Out((M, D), torch.bfloat16, DEV), RM.Out((M, D), torch.bfloat16, DEV)
    x_run = RM.Out((M, D), torch.float32, DEV, init=x_d)
    ok = dict(y=y_d, x=x_run.t, gate=v_d, keep=None, scale=v_d, shift=v_d, rows=M, dim=D, rpv=RPV, nvec=NVEC, stride=stride)
    cases = [(dict(x=None), "x is null"), (dict(y=None, scale=None, shift=None), "y and ln_scale are both null"),
             (dict(rpv=0), "rows_per_vec must be >= 1"), (dict(nvec=0), "nvec must be >= 1"), (dict(stride=D - 4), "vec_stride 252 is smaller than dim"),
             (dict(dim=320), "dim must be 256/512/768/1024"), (dict(dim=1280), "dim must be 256/512/768/1024")]
    seen = set()
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.f5_op_resid_gate_ln_rows(P(a["y"]), P(a["x"]), P(a["gate"]), P(a["keep"]), P(a["scale"]), P(a["shift"]), P(hi.t), P(lo.t), a["rows"],
                                          a["dim"], a["rpv"], a["nvec"], Z(a["stride"]), stream())
        err = lib.f5_last_error().decode()
        assert rc != 0 and msg in err, (change, rc, err)
        seen.add(re.sub(r"\d+", "#", err))
    assert len(seen) == len(cases) - 1                       # each refusal its own message (the two bad dims share theirs)
    torch.cuda.synchronize()
    assert _beq(x_run.t, x_d) and not x_run.guard_violations("x")
    assert bool((RM.bits(hi.t) == RM.SENT16).all()) and bool((RM.bits(lo.t) == RM.SENT16).all())
    # the stage kernel: null vectors and a non-positive block size
    out = RM.Out((M, 100), torch.float32, DEV)
    p_d = randn(r, M, 100).to(DEV)
    c_d = torch.ones(NVEC, device=DEV)
    for cfgp, dtp, rpv, msg in ((None, c_d, RPV, "null cfg_rows / dt_rows"), (c_d, None, RPV, "null cfg_rows / dt_rows"),
                                (c_d, c_d, 0, "rows_per_vec and nvec must be >= 1")):
        rc = lib.f5_op_ode_stage_rows(P(p_d), P(None), P(cfgp), P(p_d), P(dtp), rpv, NVEC, F(1.0), F(1.0), 0, P(None), P(None), P(None), P(None),
                                      P(out.t), P(None), P(None), M, 100, stream())
        assert rc != 0 and msg in lib.f5_last_error().decode(), (msg, lib.f5_last_error().decode())
    torch.cuda.synchronize()
    assert bool((RM.bits(out.t) == RM.SENT32).all())


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
B, N, NT, NREF = 3, 37, 10, 12
DURS = [23, 37, 31]
CFGS = [2.0, 0.0, 1.3]
SWAYS = [-1.0, None, -0.5]


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


def _engine_args(inputs):
    """what F5TTS.sample hands the engine for `inputs`"""
    cond, text, y0 = inputs
    text_c, lens, dur, nmax = prepare_lengths(text, NREF, B, torch.tensor(DURS), None, 4096, "euler")
    assert nmax == N and dur.tolist() == DURS
    cond_p = torch.zeros((B, N, TINY.mel_dim), device=DEV)
    cond_p[:, :NREF] = cond.to(DEV)
    return text_c.to(DEV).contiguous(), cond_p, lens.tolist(), dur.tolist(), y0.to(DEV).contiguous()


def _golden_model(prec):
    g = np.load(os.path.join(GOLDEN, "ref_dit_forward.npz"))
    cfg = DiTConfig(**json.loads(str(g["cfg"])))
    m = DiT.from_config(cfg, precision=prec, device=DEV)
    m.load_weights(synthetic_weights(cfg, seed=int(g["weights_seed"])))
    m.row_times = True
    return g, m


def _count_forwards(m):
    calls = []
    inner = m.engine.dit_forward

    def counted(*a, **k):
        calls.append(np.ndim(a[5] if len(a) > 5 else k["t"]))
        return inner(*a, **k)

    m.engine.dit_forward = counted
    return calls


def test_reference_forward_with_row_times_is_one_forward():
    for prec, tol in (("bf16x3", 2e-4), ("bf16", 3e-2)):
        g, m = _golden_model(prec)
        x, cond, text, time, mask = (torch.from_numpy(g[k]) for k in ("x", "cond", "text", "time", "mask"))
        assert time.ndim == 1 and time.numel() == x.shape[0] > 1                # a (b,) time: the per-row route under row_times
        calls = _count_forwards(m)
        for tag, (drop, mk) in dict(cond=(False, None), null=(True, None), cond_masked=(False, mask), null_masked=(True, mask)).items():
            calls.clear()
            got = m(x=x, cond=cond, text=text, time=time, drop_audio_cond=drop, drop_text=drop, mask=mk)
            assert calls == [1], (prec, tag, calls)                              # ONE engine forward, with a per-row time
            _, mean, refm = report(f"dit[{prec}] row_times {tag} vs reference code", got.cpu(), torch.from_numpy(g["out_" + tag]))
            assert mean <= tol * max(1.0, refm), (prec, tag)
        if prec == "bf16x3":
            # differing times: the one forward against the loop of batch-1 forwards; each is within 2e-4 of the reference, so 4e-4 apart
            t2 = torch.tensor([0.2, 0.8])
            calls.clear()
            rows = m(x=x, cond=cond, text=text, time=t2, drop_audio_cond=False, drop_text=False, mask=mask)
            assert calls == [1]
            m.row_times = False
            calls.clear()
            loop = m(x=x, cond=cond, text=text, time=t2, drop_audio_cond=False, drop_text=False, mask=mask)
            m.row_times = True
            assert calls == [0, 0]
            _, mean, refm = report("dit[bf16x3] row_times vs the loop, differing times", rows.cpu(), loop.cpu())
            assert mean <= 4e-4 * max(1.0, refm) and not torch.equal(rows[0], rows[1])
            gl = np.load(os.path.join(GOLDEN, "ref_cfm_loss.npz"))
            tts = F5TTS(m)
            for name, (ra, rc) in dict(keep=(0.9, 0.9), drop_audio=(0.1, 0.9), drop_both=(0.9, 0.1)).items():
                rand = dict(x0=torch.from_numpy(gl["x0"]), time=torch.from_numpy(gl["time"]), frac_lengths=torch.from_numpy(gl["frac_lengths"]),
                            span_rand=torch.from_numpy(gl["span_rand"]), rand_audio_drop=ra, rand_cond_drop=rc)
                calls.clear()
                got = float(tts(torch.from_numpy(gl["mel"]), torch.from_numpy(gl["text"]), lens=torch.from_numpy(gl["lens"]), rand=rand))
                want = float(gl["loss_" + name])
                print(f"cfm loss, row_times [{name}]: engine {got:.6f} reference code {want:.6f} ({len(calls)} forward)")
                assert calls == [1] and abs(got - want) <= 2e-4 * want


def test_rows_are_independent(models, inputs):
    eng = models["f16"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 4
    grids_a = time_grid_rows(steps, SWAYS)
    grids_b = grids_a.copy()
    grids_b[1] = time_grid(steps, 0.4)
    cfg_a, cfg_b = list(CFGS), [CFGS[0], 1.7, CFGS[2]]
    res = []
    for grids, cfg in ((grids_a, cfg_a), (grids_b, cfg_b)):
        out, traj = eng.sample(text, cond_p, lens, durs, y0, grids, method="midpoint", cfg_strength=cfg, use_mask=True, use_graph=False)
        torch.cuda.synchronize()
        res.append((out.clone(), traj.clone()))
    (oa, ta), (ob, tb) = res
    assert eng.saturation_events == 0
    for b in (0, 2):
        assert torch.equal(oa[b], ob[b]) and torch.equal(ta[:, b], tb[:, b]), b
    assert not torch.equal(oa[1], ob[1]) and not torch.equal(ta[1:, 1], tb[1:, 1])
    assert torch.equal(ta[0], y0) and torch.equal(tb[0], y0)


def test_one_graph_serves_every_set_of_values(models, inputs):
    eng = models["f16"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 4
    sets = {"a": (time_grid_rows(steps, SWAYS), list(CFGS)), "b": (time_grid_rows(steps, [0.3, -1.0, None]), [0.7, 2.5, 1.0])}
    kw = dict(method="euler", use_mask=True)
    eager = {}
    for k, (g, c) in sets.items():
        eager[k] = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, g, cfg_strength=c, use_graph=False, **kw)]
    plain = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), cfg_strength=2.0, use_graph=False, **kw)]
    torch.cuda.synchronize()
    assert not torch.equal(eager["a"][0], eager["b"][0])
    c0 = eng.graph_count()
    out, traj = eng.sample(text, cond_p, lens, durs, y0, sets["a"][0], cfg_strength=sets["a"][1], use_graph=True, **kw)
    torch.cuda.synchronize()
    assert eng.graph_count() == c0 + 1 and torch.equal(out, eager["a"][0]) and torch.equal(traj, eager["a"][1])
    out, traj = eng.sample(text, cond_p, lens, durs, y0, sets["b"][0], cfg_strength=sets["b"][1], use_graph=True, **kw)
    torch.cuda.synchronize()
    assert eng.graph_count() == c0 + 1                                   # other values, the same graph
    assert torch.equal(out, eager["b"][0]) and torch.equal(traj, eager["b"][1])
    out, traj = eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), cfg_strength=2.0, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert eng.graph_count() == c0 + 2                                   # f5_sample of the same shape: its own entry, its own bits
    assert torch.equal(out, plain[0]) and torch.equal(traj, plain[1])
    out, traj = eng.sample(text, cond_p, lens, durs, y0, sets["a"][0], cfg_strength=sets["a"][1], use_graph=True, **kw)
    torch.cuda.synchronize()
    assert eng.graph_count() == c0 + 2                                   # ... which did not evict the rows route's graph
    assert torch.equal(out, eager["a"][0]) and torch.equal(traj, eager["a"][1])


_oracle = {}


def _oracle_row(weights, inputs, method, steps, b):
    """the CPU oracle's sample() of the batch with row b's controls as scalars (computed once per key)"""
    key = (method, steps, b)
    if key not in _oracle:
        cond, text, y0 = inputs
        dit = _oracle.setdefault("dit", O.DiTOracle(TINY, weights))
        _oracle[key] = O.sample(dit, cond, text, torch.tensor(DURS), y0=y0, steps=steps, method=method, cfg_strength=CFGS[b],
                                sway_sampling_coef=SWAYS[b])
    return _oracle[key]


@pytest.mark.parametrize("method,steps", [("euler", 5), ("midpoint", 4), ("rk4", 3)])
def test_rows_against_the_scalar_route_and_the_oracle(models, tiny_weights, inputs, method, steps):
    """Measured on one MI355X (bf16x3, mean |delta| of row b, final mel / trajectory): see docs/row_controls.md."""
    cond, text, y0 = inputs
    f5 = F5TTS(transformer=models["bf16x3"])
    kw = dict(duration=torch.tensor(DURS), steps=steps, method=method, y0=y0, use_graph=False)
    out, traj = [x.clone() for x in f5.sample(cond, text, cfg_strength=CFGS, sway_sampling_coef=SWAYS, **kw)]
    assert traj.shape == (steps, B, N, TINY.mel_dim) and torch.isfinite(out).all()
    lens = _engine_args(inputs)[2]
    for b in range(B):
        so, st = f5.sample(cond, text, cfg_strength=CFGS[b], sway_sampling_coef=SWAYS[b], **kw)
        _, l1, _ = report(f"rows vs scalar route [{method}] row {b} final mel", out[b].cpu(), so[b].cpu())
        _, l1t, _ = report(f"rows vs scalar route [{method}] row {b} trajectory", traj[:, b].cpu(), st[:, b].cpu())
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (method, b)
        oo, ot = _oracle_row(tiny_weights, inputs, method, steps, b)
        _, l1, _ = report(f"rows vs oracle [{method}] row {b} final mel", out[b].cpu(), oo[b])
        _, l1t, _ = report(f"rows vs oracle [{method}] row {b} trajectory", traj[:, b].cpu(), ot[:, b])
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (method, b)
        assert torch.equal(out[b, :lens[b]].cpu(), cond[b, :lens[b]])            # kept frames are cond, bit for bit
    assert not torch.equal(out[0], out[1])


def test_uniform_controls_agree_with_the_scalar_route(models, inputs):
    """all rows equal, passed as a (B, steps) grid: the rows route within the gate of f5_sample (not bit-exact: the gated projections run
    another epilogue)"""
    eng = models["bf16x3"].engine
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    for method, steps in (("euler", 5), ("rk4", 3)):
        t = time_grid(steps, -1.0)
        kw = dict(method=method, cfg_strength=2.0, use_mask=True, use_graph=False)
        want, want_t = [x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, t, **kw)]
        got, got_t = eng.sample(text, cond_p, lens, durs, y0, np.tile(t, (B, 1)), **kw)
        _, l1, _ = report(f"uniform rows vs f5_sample [{method}] final mel", got.cpu(), want.cpu())
        _, l1t, _ = report(f"uniform rows vs f5_sample [{method}] trajectory", got_t.cpu(), want_t.cpu())
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, method
        # a per-row cfg alone selects the route as well
        got2, _ = eng.sample(text, cond_p, lens, durs, y0, t, **dict(kw, cfg_strength=[2.0] * B))
        assert torch.equal(got2, got)


def test_f5tts_sample_sequence_seed_and_speed(models, inputs):
    cond, text, y0 = inputs
    seconds, speeds, seeds = [0.30, 0.40, 0.35], [1.0, 2.0, 0.5], [7, 8, 9]
    dp = lambda c, t, lens=None: torch.tensor(seconds, device=DEV)                  # noqa: E731
    f5 = F5TTS(transformer=models["bf16x3"], duration_predictor=dp)
    want_d = (torch.tensor(seconds) * 93 / torch.tensor(speeds)).to(torch.int32).tolist()
    assert want_d == [27, 18, 65]
    out, traj = f5.sample(cond, text, steps=3, method="euler", seed=seeds, speed=speeds, use_graph=False)
    assert f5.last_durations == want_d and out.shape == (B, max(want_d), TINY.mel_dim)
    assert torch.equal(traj[0], E.noise_normal(seeds, want_d, max(want_d), TINY.mel_dim, DEV))
    assert not torch.equal(traj[0, 0, :18], traj[0, 1, :18])                       # different seeds, different noise
    # an all-scalar call returns the bits of Engine.sample called the way it always was
    eng = models["bf16x3"].engine
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    got, got_t = [x.clone() for x in F5TTS(transformer=models["bf16x3"]).sample(
        cond, text, duration=torch.tensor(DURS), steps=5, method="euler", cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0, use_graph=False)]
    want, want_t = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(5, -1.0), method="euler", cfg_strength=2.0, use_mask=True,
                              use_graph=False)
    assert torch.equal(got, want) and torch.equal(got_t, want_t)


def test_sample_rows_refusals_launch_nothing(models, inputs):
    eng = models["bf16x3"].engine
    lib = eng.lib
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 3
    ws = eng.workspace(B, N, NT, steps, "euler", rows=True)
    out = torch.full_like(cond_p, -12345.0)
    a, keep = eng._args(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), steps, "euler", 2.0, True, False, out, None, ws)
    tr, cr = time_grid_rows(steps, SWAYS), np.asarray(CFGS, np.float32)
    tr_nan, cr_inf = tr.copy(), cr.copy()
    tr_nan[1, 2], cr_inf[2] = np.nan, np.inf
    small = C.c_size_t()
    E.check(lib.f5_workspace_bytes(eng._h, B, N, NT, steps, 0, C.byref(small)))
    big = C.c_size_t()
    E.check(lib.f5_workspace_bytes_rows(eng._h, B, N, NT, steps, 0, C.byref(big)))
    # the rows plan holds the (evaluation, row) tables on top of f5_sample's plan
    assert big.value >= small.value + (steps - 1) * B * (6 * TINY.depth + 2) * TINY.dim * 4

    def refused(rc_struct, msg):
        rc = lib.f5_sample_rows(eng._h, C.byref(a), None if rc_struct is None else C.byref(rc_struct), stream())
        err = lib.f5_last_error().decode()
        assert rc != 0 and msg in err, (msg, rc, err)

    refused(None, "controls is null")
    refused(E.F5RowControls(0, cr.ctypes.data, 0), "controls.t_rows is null")
    refused(E.F5RowControls(tr.ctypes.data, 0, 0), "controls.cfg_rows is null")
    refused(E.F5RowControls(tr_nan.ctypes.data, cr.ctypes.data, 0), "t_rows[1][2] is not finite")
    refused(E.F5RowControls(tr.ctypes.data, cr_inf.ctypes.data, 0), "cfg_rows[2] is not finite")
    a.workspace_bytes = small.value
    refused(E.F5RowControls(tr.ctypes.data, cr.ctypes.data, 0), "f5_workspace_bytes_rows")
    a.workspace_bytes = ws.numel()
    a.method = 7
    refused(E.F5RowControls(tr.ctypes.data, cr.ctypes.data, 0), "Unknown method")       # ... and everything f5_sample refuses
    a.method = 0
    eng.set_option("ln_fold", 1)
    try:
        refused(E.F5RowControls(tr.ctypes.data, cr.ctypes.data, 0), "ln_fold = 1")
    finally:
        eng.set_option("ln_fold", -1)
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all())
    del keep


def test_mxfp8_engine_refuses_the_rows_route(tiny_weights, inputs):
    eng = E.Engine(TINY, precision="mxfp8", device=DEV)
    eng.load_weights(tiny_weights)
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    out = torch.full_like(cond_p, -12345.0)
    traj = torch.full((4, B, N, TINY.mel_dim), -12345.0, device=DEV)
    with pytest.raises(RuntimeError, match="f5_sample_rows.*mxfp8"):
        eng.sample(text, cond_p, lens, durs, y0, time_grid_rows(4, SWAYS), method="euler", cfg_strength=CFGS, use_mask=True, use_graph=False,
                   out=out, trajectory=traj)
    with pytest.raises(RuntimeError, match="f5_dit_forward_rows.*mxfp8"):
        eng.dit_forward(y0, text, cond_p, lens, durs, [0.1, 0.5, 0.9], cfg_strength=0.0)
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all()) and bool((traj == -12345.0).all())        # nothing was launched
    # the scalar route of the same engine is what it was
    got, _ = eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), method="euler", cfg_strength=2.0, use_mask=True, use_graph=False)
    assert torch.isfinite(got).all()
