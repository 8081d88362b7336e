"""Multistep solvers ab2 / ab3 on the GPU (docs/multistep.md): Adams-Bashforth of order 2 / 3 on the call's time grid, one DiT evaluation
per step.

Op level: mode 2 of the three stage kernels (f5_op_ode_stage_ab) at rows_per_vec = 37, nvec = 3, M = 2 * 3 * 37 (the shapes of
tests/test_row_controls_gpu.py), both operand types, guarded buffers: against an fp64 evaluation, the per-row and dual kernels against
the scalar kernel block of rows by block of rows and bit for bit, NaN planted in every history buffer that no weight names.  Engine
level (TINY, B = 3, ragged 23 / 37 / 31, 6 grid points): step 0 is the Euler step bit for bit, graph replay and graph_split equal the
eager call, the final mel against the CPU restatement (tests/multistep_ref.py) on all four routes, and the Python layers."""
import numpy as np
import pytest
import torch

import multistep_ref as MS
import rowops_matrix as RM
from f5test import DEV, E, O, P, TINY, operand_mode, report, rng, randn, stream, synthetic_weights
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths, time_grid
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of fp32
MEL_L1_TOL = 1e-3                  # the project's mel-L1 gate: bf16x3 outright, f16 times A
BF16_TOL = 3e-2                    # what tests/test_row_controls_gpu.py holds bf16 to (of max(1, mean |ref|)): times A
RPV, NVEC, MEL = 37, 3, 100
M = 2 * NVEC * RPV
B, N, NT, NREF, DURS, STEPS = MS.B, MS.N, MS.NT, MS.NREF, MS.DURS, MS.STEPS
METHODS = ("ab2", "ab3")
ROUTES = tuple(MS.ROUTES)


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _blocks():
    """(first row, vector) of every block of RPV rows"""
    return [(r0, (r0 // RPV) % NVEC) for r0 in range(0, M, RPV)]


def _beq(a, b):
    return torch.equal(RM.bits(a.contiguous()).cpu(), RM.bits(b.contiguous()).cpu())


class _Outs:
    def __init__(self, rows, dt16):
        self.out, self.kst = RM.Out((rows, MEL), torch.float32, DEV, guard=MEL), RM.Out((rows, MEL), torch.float32, DEV, guard=MEL)
        self.hi, self.lo = RM.Out((rows, 128), dt16, DEV, guard=128), RM.Out((rows, 128), dt16, DEV, guard=128)

    def violations(self):
        return (self.out.guard_violations("out") + self.kst.guard_violations("kstore") + self.hi.guard_violations("xin_hi")
                + self.lo.guard_violations("xin_lo"))


def _stage_ab(lib, route, o, rows, pred, null, cfg, base, dt, abw, k1, k2, text=None, audio=None, rpv=1, nvec=1):
    E.check(lib.f5_op_ode_stage_ab(route, P(pred), P(text), P(null), P(audio), P(cfg), P(base), P(dt), P(abw), rpv, nvec, P(o.kst.t), P(k1), P(k2),
                                   P(o.out.t), P(o.hi.t), P(o.lo.t), rows, MEL, stream()), "f5_op_ode_stage_ab")
    torch.cuda.synchronize()
    bad = o.violations()
    assert not bad, bad


# ---- op level ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op16", RM.OPS16)
@pytest.mark.parametrize("terms", [3, 2, 1])
def test_mode2_against_fp64(lib, terms, op16):
    """out = fma(dt, fma(w2, k2, fma(w1, k1, w0 k)), base) on the k the kernel stored.  Bound: the product w0 k and the two fmas round
    once each, each result below S = |w0 k| + |w1 k1| + |w2 k2| in magnitude up to a factor 1 + 2u, so the increment is within 3 u S of
    its exact value; the last fma rounds once more, u |out| <= u (|base| + |dt| S).  In all u (4 |dt| S + |base|), with 2^-20 of it for
    the second-order terms.  k itself, pred + (pred - null) cfg in two or three roundings, is held to 3 u (|pred| + |pred - null| |cfg|).
    terms: 3 = both history buffers, 2 = k2's pointer null, 1 = both null -- the weights of the absent ones are left non-zero, so that a
    null pointer must be skipped by selection."""
    r = rng(300 + terms)
    cfg, dt = 2.0, 0.0506
    w = np.float32([2.4306, -2.1479, 0.7173])
    pred, base, null, k1, k2 = (randn(r, M, MEL) for _ in range(5))
    d = {k: RM.pad_in(t, DEV) for k, t in dict(pred=pred, base=base, null=null, k1=k1, k2=k2).items()}
    cfg_d, dt_d, w_d = (RM.pad_in(torch.tensor(v, dtype=torch.float32).reshape(-1), DEV) for v in (cfg, dt, w))
    with operand_mode(op16):
        o = _Outs(M, RM.op_dtype(op16))
        _stage_ab(lib, 0, o, M, d["pred"], d["null"], cfg_d, d["base"], dt_d, w_d, d["k1"] if terms >= 2 else None, d["k2"] if terms == 3 else None)
    k = o.kst.t.cpu().double()
    k_ref = pred.double() + (pred.double() - null.double()) * cfg
    assert not RM.chk_f32("kstore", o.kst.t.cpu(), k_ref, 3 * U * (pred.double().abs() + (pred.double() - null.double()).abs() * cfg))
    w64, dt64 = w.astype(np.float64), float(np.float32(dt))
    terms64 = [w64[0] * k] + ([w64[1] * k1.double()] if terms >= 2 else []) + ([w64[2] * k2.double()] if terms == 3 else [])
    S = sum(t.abs() for t in terms64)
    ref = base.double() + dt64 * sum(terms64)
    bound = U * (4 * abs(dt64) * S + base.double().abs()) * (1 + 2.0 ** -20)
    bad = RM.chk_f32("out", o.out.t.cpu(), ref, bound)
    assert not bad, bad
    padded = torch.zeros((M, 128))
    padded[:, :MEL] = o.out.t.cpu()
    bad = RM.chk_split("xin", o.hi.t.cpu(), o.lo.t.cpu(), padded, op16)         # the next operand is packed as in mode 0
    assert not bad, bad
    if terms < 3:                                                                # ... and the term did count where it is present
        assert float((o.out.t.cpu().double() - (ref + dt64 * w64[2] * k2.double())).abs().max()) > 1e-3


def _row_case(seed):
    """per-vector weights: vector 0 third order, vector 1 second (w2 absent), vector 2 first (w1 and w2 absent); the history of every
    absent weight is NaN in that vector's blocks"""
    r = rng(seed)
    dts = [0.0506, 0.11, 0.0231]
    ws = np.float32([[2.4306, -2.1479, 0.7173], [1.7301, -0.7301, 0.0], [1.0, 0.0, 0.0]])
    pred, base, null, text, k1, k2 = (randn(r, M, MEL) for _ in range(6))
    for r0, v in _blocks():
        if v >= 1:
            k2[r0:r0 + RPV] = float("nan")
        if v == 2:
            k1[r0:r0 + RPV] = float("nan")
    d = {k: RM.pad_in(t, DEV) for k, t in dict(pred=pred, base=base, null=null, text=text, k1=k1, k2=k2).items()}
    d["dt"], d["w"] = RM.pad_in(torch.tensor(dts), DEV), RM.pad_in(torch.from_numpy(ws.reshape(-1)), DEV)
    return d, pred


def _check_blocks(lib, o, d, dt16, scalar_of):
    """every block of the per-row launch `o` against the scalar kernel on that block with the block's (null, cfg) from scalar_of(v)"""
    assert torch.isfinite(o.out.t).all() and torch.isfinite(o.kst.t).all()       # no planted NaN reached anything
    for r0, v in _blocks():
        sl = slice(r0, r0 + RPV)
        null, cfg = scalar_of(v, sl)
        w = _Outs(RPV, dt16)
        _stage_ab(lib, 0, w, RPV, d["pred"][sl], null, cfg, d["base"][sl], d["dt"][v:], d["w"][3 * v:], d["k1"][sl], d["k2"][sl])
        assert _beq(o.out.t[sl], w.out.t) and _beq(o.kst.t[sl], w.kst.t), (r0, v)
        assert _beq(o.hi.t[sl], w.hi.t) and _beq(o.lo.t[sl], w.lo.t), (r0, v)


@pytest.mark.parametrize("op16", RM.OPS16)
def test_mode2_rows_equals_the_scalar_kernel_block_by_block(lib, op16):
    cfgs = [2.0, 0.0, 1.3]                                       # vector 1 is unguided: its null_pred is NaN as well
    d, pred = _row_case(410)
    for r0, v in _blocks():
        if v == 1:
            d["null"][r0:r0 + RPV] = float("nan")
    cfg_d = RM.pad_in(torch.tensor(cfgs), DEV)
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        o = _Outs(M, dt16)
        _stage_ab(lib, 1, o, M, d["pred"], d["null"], cfg_d, d["base"], d["dt"], d["w"], d["k1"], d["k2"], rpv=RPV, nvec=NVEC)
        _check_blocks(lib, o, d, dt16, lambda v, sl: (d["null"][sl] if cfgs[v] >= 1e-5 else None, cfg_d[v:]))
    assert not torch.equal(o.kst.t[:RPV].cpu(), pred[:RPV]) and torch.equal(o.kst.t[RPV:2 * RPV].cpu(), pred[RPV:2 * RPV])


@pytest.mark.parametrize("op16", RM.OPS16)
def test_mode2_dual_equals_the_scalar_kernel_block_by_block(lib, op16):
    """text strength 0 in every vector: k = F + (F - T) a is the scalar kernel's rule with T as its second prediction (vector 1 has both
    strengths 0: k = F, and T is NaN there); N is NaN everywhere, since no row's text strength loads it"""
    audio, texts = [3.0, 0.0, 1.5], [0.0, 0.0, 0.0]
    d, pred = _row_case(420)
    d["null"][:] = float("nan")
    for r0, v in _blocks():
        if v == 1:
            d["text"][r0:r0 + RPV] = float("nan")
    a_d, c_d = RM.pad_in(torch.tensor(audio), DEV), RM.pad_in(torch.tensor(texts), DEV)
    dt16 = RM.op_dtype(op16)
    with operand_mode(op16):
        o = _Outs(M, dt16)
        _stage_ab(lib, 2, o, M, d["pred"], d["null"], c_d, d["base"], d["dt"], d["w"], d["k1"], d["k2"], text=d["text"], audio=a_d, rpv=RPV,
                  nvec=NVEC)
        _check_blocks(lib, o, d, dt16, lambda v, sl: (d["text"][sl] if audio[v] >= 1e-5 else None, a_d[v:]))
    assert not torch.equal(o.kst.t[:RPV].cpu(), pred[:RPV]) and torch.equal(o.kst.t[RPV:2 * RPV].cpu(), pred[RPV:2 * RPV])


def test_mode2_refusals_launch_nothing(lib):
    x = torch.zeros((4, MEL), device=DEV)
    s = torch.ones(4, device=DEV)
    out = RM.Out((4, MEL), torch.float32, DEV, guard=MEL)

    def call(route=0, abw=s, kst=x, k1=None, cfg=s):
        rc = lib.f5_op_ode_stage_ab(route, P(x), P(None), P(None), P(None), P(cfg), P(x), P(s), P(abw), 4, 1, P(kst), P(k1), P(None), P(out.t), P(None),
                                    P(None), 4, MEL, stream())
        return rc, lib.f5_last_error().decode()

    for kw, msg in ((dict(route=3), "route must be 0, 1 or 2"), (dict(abw=None), "mode 2 needs abw and kstore"),
                    (dict(kst=None), "mode 2 needs abw and kstore"), (dict(k1=x), "kstore is one of the history buffers"),
                    (dict(route=1, cfg=None), "null cfg_rows")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((RM.bits(out.t) == RM.SENT32).all())


# ---- engine level --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_weights():
    return synthetic_weights(TINY, seed=42)


@pytest.fixture(scope="module")
def models(tiny_weights):
    out = {}
    for prec in ("bf16x3", "f16", "bf16", "mxfp8"):
        m = DiT.from_config(TINY, precision=prec, device=DEV)
        m.load_weights(tiny_weights)
        out[prec] = m
    return out


@pytest.fixture(scope="module")
def graph_engine(tiny_weights):
    """an f16 engine of its own with room for the two graphs of each of the eight cases"""
    m = DiT.from_config(TINY, precision="f16", device=DEV)
    m.load_weights(tiny_weights)
    m.engine.set_graph_cache(32)
    # the largest plan of the eight cases first: a graph is captured against the workspace's address, and a call that had to grow the
    # workspace would drop every graph captured before it at its next capture
    m.engine.workspace(B, N, NT, STEPS, "ab3", rows="window_dual")
    return m.engine


@pytest.fixture(scope="module")
def inputs():
    return MS.inputs()


@pytest.fixture(scope="module")
def oracle(tiny_weights):
    return O.DiTOracle(TINY, tiny_weights)


def _engine_args(inputs, rows=slice(0, B)):
    """what F5TTS.sample hands the engine for the rows `rows` of `inputs`"""
    cond, text, y0 = (x[rows] for x in inputs)
    durs = DURS[rows]
    text_c, lens, dur, nmax = prepare_lengths(text, NREF, len(durs), torch.tensor(durs), None, 4096, "ab2")
    assert dur.tolist() == durs
    cond_p = torch.zeros((len(durs), nmax, TINY.mel_dim), device=DEV)
    cond_p[:, :NREF] = cond.to(DEV)
    return text_c.to(DEV).contiguous(), cond_p, lens.tolist(), dur.tolist(), y0[:, :nmax].to(DEV).contiguous()


def _sample(eng, inputs, route, method, **kw):
    """Engine.sample on the shared batch through `route` -> clones of (out, trajectory)"""
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    kw.setdefault("use_graph", False)
    out, traj = eng.sample(text, cond_p, lens, durs, y0, MS.engine_grid(route), method=method, use_mask=True, **MS.ROUTES[route][4], **kw)
    torch.cuda.synchronize()
    return out.clone(), traj.clone()


_ref = {}


def _reference(oracle, inputs, route, method):
    """the CPU restatement's (final mel, trajectory), computed once per route and method"""
    if (route, method) not in _ref:
        _ref[route, method] = MS.reference(oracle, route, method, ins=inputs)
    return _ref[route, method]


def _solo(eng, inputs, method, **kw):
    """row 1 alone (37 frames: the full length), B = 1 without a mask, scalar route"""
    text, cond_p, lens, durs, y0 = _engine_args(inputs, slice(1, 2))
    kw.setdefault("use_graph", False)
    out, traj = eng.sample(text, cond_p, lens, durs, y0, time_grid(STEPS, -1.0), method=method, cfg_strength=MS.CFG, use_mask=False, **kw)
    torch.cuda.synchronize()
    return out.clone(), traj.clone()


@pytest.mark.parametrize("route", ROUTES)
def test_step_0_is_the_euler_step(models, inputs, route):
    eng = models["f16"].engine
    _, et = _sample(eng, inputs, route, "euler")
    trajs = {}
    for method in METHODS:
        _, trajs[method] = _sample(eng, inputs, route, method)
        assert torch.equal(trajs[method][:2], et[:2]), (route, method)                    # y0 and the first step, bit for bit
        assert not torch.equal(trajs[method][2], et[2]), (route, method)
    assert torch.equal(trajs["ab2"][:3], trajs["ab3"][:3]) and not torch.equal(trajs["ab2"][3], trajs["ab3"][3])    # step 1 is second order
    assert eng.saturation_events == 0


def test_step_0_is_the_euler_step_mxfp8_and_batch_1(models, inputs):
    eng = models["mxfp8"].engine                                                          # the scalar route runs the mode like any method
    _, et = _sample(eng, inputs, "scalar", "euler")
    for method in METHODS:
        out, traj = _sample(eng, inputs, "scalar", method)
        assert torch.isfinite(out).all() and torch.equal(traj[:2], et[:2]) and not torch.equal(traj[2], et[2]), method
    with pytest.raises(RuntimeError, match="f5_sample_rows.*mxfp8"):                      # ... and keeps its refusals
        _sample(eng, inputs, "rows", "ab2")
    eng = models["f16"].engine
    _, et = _solo(eng, inputs, "euler")
    for method in METHODS:
        _, traj = _solo(eng, inputs, method)
        assert torch.equal(traj[:2], et[:2]) and not torch.equal(traj[2], et[2]), method


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("route", ROUTES)
def test_graph_replay_and_graph_split_equal_eager(graph_engine, inputs, route, method):
    eng = graph_engine
    want, want_t = _sample(eng, inputs, route, method)
    c0 = eng.graph_count()
    for rep in range(2):                                                                  # capture, then replay
        out, traj = _sample(eng, inputs, route, method, use_graph=True)
        assert torch.equal(out, want) and torch.equal(traj, want_t), (route, method, rep)
    assert eng.graph_count() == c0 + 1
    # one graph per ODE step: the history lives in the workspace and outlasts a segment
    eng.set_option("graph_split", 1)
    try:
        for rep in range(2):
            out, traj = _sample(eng, inputs, route, method, use_graph=True)
            assert torch.equal(out, want) and torch.equal(traj, want_t), (route, method, "split", rep)
    finally:
        eng.set_option("graph_split", 0)
    assert eng.graph_count() == c0 + 2
    if route == "rows":
        # other grids and strengths on the same graph: the weights are staged values, not frozen ones
        from f5_tts_mlx_amd.cfm import time_grid_rows
        text, cond_p, lens, durs, y0 = _engine_args(inputs)
        g2, c2 = time_grid_rows(STEPS, [0.3, -1.0, None]), [0.7, 2.5, 1.0]
        res = []
        for graph in (False, True):
            res.append([x.clone() for x in eng.sample(text, cond_p, lens, durs, y0, g2, method=method, cfg_strength=c2, use_mask=True, use_graph=graph)])
        torch.cuda.synchronize()
        assert eng.graph_count() == c0 + 2 and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert not torch.equal(res[0][0], want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("route", ROUTES)
def test_final_mel_against_the_cpu_restatement(models, oracle, inputs, route, method):
    """Mean |delta| of row b's final mel against tests/multistep_ref.py.  A = max_i sum_j |w_ij| of the grid in use is the factor by which
    one step amplifies an error of its k's, relative to Euler's 1: bf16x3 meets the 1e-3 gate outright, f16 is held to 1e-3 A and bf16 to
    3e-2 max(1, mean |ref|) A.  Measured on one MI355X: see docs/multistep.md."""
    want, want_t = _reference(oracle, inputs, route, method)
    A = MS.amplification(MS.grids_of(MS.ROUTES[route][0]), MS.ORDER[method])
    print(f"multistep [{route}, {method}]: A = {A:.4f}")
    lens = _engine_args(inputs)[2]
    fails = []
    for prec, tol in (("bf16x3", MEL_L1_TOL), ("f16", MEL_L1_TOL * A), ("bf16", BF16_TOL * A)):
        out, traj = _sample(models[prec].engine, inputs, route, method)
        assert traj.shape == (STEPS, B, N, TINY.mel_dim) and torch.isfinite(out).all()
        for b in range(B):
            _, l1, refm = report(f"multistep [{route}, {method}, {prec}] row {b} final mel", out[b].cpu(), want[b])
            _, l1t, _ = report(f"multistep [{route}, {method}, {prec}] row {b} trajectory", traj[:, b].cpu(), want_t[:, b])
            bound = tol * (max(1.0, refm) if prec == "bf16" else 1.0)
            if not l1 <= bound:
                fails.append((prec, b, l1, bound))
            assert torch.equal(out[b, :lens[b]].cpu(), inputs[0][b, :lens[b]])              # kept frames are cond, bit for bit
    assert not fails, fails
    # not by indifference: the Euler call on the same inputs is far from the restatement
    eul, _ = _sample(models["bf16x3"].engine, inputs, route, "euler")
    far = float((eul.cpu() - want).abs().mean())
    print(f"multistep [{route}, {method}]: euler vs the restatement: mean |delta| = {far:.4f}")
    assert far > 10 * MEL_L1_TOL


@pytest.mark.parametrize("method", METHODS)
def test_batch_1_without_a_mask_against_the_cpu_restatement(models, oracle, inputs, method):
    cond, text, y0 = (x[1:2] for x in inputs)
    grid = MS.grids_of("sway", batch=1)
    want, _ = MS.ab_sample(oracle, cond, text, DURS[1:2], y0, grid, method, [MS.CFG])
    out, _ = _solo(models["bf16x3"].engine, inputs, method)
    _, l1, _ = report(f"multistep [B = 1, {method}, bf16x3] final mel", out[0].cpu(), want[0])
    assert l1 <= MEL_L1_TOL


def test_repeated_grid_point_in_one_row(models, oracle, inputs):
    """row 1's grid repeats a point: the step behind it drops to first order, the one after to second (decided per step and row on the
    host); the other rows keep their third-order steps"""
    cond, text, y0 = inputs
    grids = MS.grids_of("rows").copy()
    grids[1] = np.float32([0.0, 0.1, 0.1, 0.3, 0.55, 1.0])
    orders = [[int(np.count_nonzero(w)) for w in step] for step in MS.weight_table(grids, 3)]
    assert [o[1] for o in orders] == [1, 1, 1, 2, 3] and [o[0] for o in orders] == [1, 2, 3, 3, 3]     # (row 1, step 1: h = 0, w1 = +0)
    want, _ = MS.ab_sample(oracle, cond, text, DURS, y0, grids, "ab3", MS.CFG_ROWS)
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    out, traj = models["bf16x3"].engine.sample(text_d, cond_p, lens, durs, y0_d, grids, method="ab3", cfg_strength=MS.CFG_ROWS, use_mask=True,
                                               use_graph=False)
    assert torch.isfinite(traj).all() and torch.equal(traj[1, 1], traj[2, 1])             # the step of length 0 moves nothing
    for b in range(B):
        _, l1, _ = report(f"multistep [repeated point, ab3, bf16x3] row {b} final mel", out[b].cpu(), want[b])
        assert l1 <= MEL_L1_TOL, b


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------------
def test_f5tts_sample_equals_the_engine_call(models, inputs):
    cond, text, y0 = inputs
    f5 = F5TTS(transformer=models["bf16x3"])
    got, got_t = [x.clone() for x in f5.sample(cond, text, duration=torch.tensor(DURS), steps=STEPS, method="ab3", y0=y0, use_graph=False,
                                               cfg_strength=MS.CFG_ROWS, sway_sampling_coef=MS.SWAYS)]
    want, want_t = _sample(models["bf16x3"].engine, inputs, "rows", "ab3")
    assert torch.equal(got, want) and torch.equal(got_t, want_t)
    got, _ = [x.clone() for x in f5.sample(cond, text, duration=torch.tensor(DURS), steps=STEPS, method="ab2", y0=y0, use_graph=False,
                                           cfg_strength=MS.CFG, sway_sampling_coef=-1.0)]
    want, _ = _sample(models["bf16x3"].engine, inputs, "scalar", "ab2")
    assert torch.equal(got, want)
    assert G.parse_args(["--text", "x", "--method", "ab2"]).method == "ab2"
