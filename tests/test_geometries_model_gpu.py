"""DiT geometries outside the 335M family (docs/geometries.md) at model level: a 768-wide model with attention inner width 512, 16
conv-pos groups of 48 channels and 384-wide text (NARROW), the inner width alone, and the upstream "Small" shape in miniature, against
the CPU oracle.  Bounds: those tests/test_model_gpu.py applies to TINY for the same calls -- dit_forward: bf16x3 2e-4, f16 1e-3 against
the fp32 oracle and 3e-4 against the fp16-emulating one, each times max(1, mean |reference|); sample: the 1e-3 mel-L1 gate -- and, on the
per-row routes, the gate of tests/test_dual_guidance_gpu.py / tests/test_guidance_window_gpu.py with their reference helpers.
"""
import numpy as np
import pytest
import torch

import dual_guidance_ref as DG
import guidance_window_ref as GW
from f5test import DEV, O, DiTConfig, report, synth_inputs, synthetic_weights
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths, time_grid
from f5_tts_mlx_amd.dit import DiT
from test_model_gpu import MEL_L1_TOL, _pad_cond

pytestmark = pytest.mark.gpu

NARROW = DiTConfig(dim=768, depth=2, heads=8, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=384, conv_layers=2, conv_pos_groups=16)
INNER_ONLY = DiTConfig(dim=512, depth=2, heads=4, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=256, conv_layers=2, conv_pos_groups=8)
UPSTREAM_SMALL_MINI = DiTConfig(dim=768, depth=2, heads=12, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=512, conv_layers=2,
                                conv_pos_groups=16)
FWD_BOUNDS = {"bf16x3": dict(fp32=2e-4), "f16": dict(fp32=1e-3, f16emu=3e-4)}       # tests/test_model_gpu.py


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(NARROW, seed=42)


@pytest.fixture(scope="module")
def models(weights):
    out = {}
    for prec in ("bf16x3", "f16"):
        m = DiT.from_config(NARROW, precision=prec, device=DEV)
        m.load_weights(weights)
        out[prec] = m
    return out


@pytest.fixture(scope="module")
def oracles(weights):
    return dict(fp32=O.DiTOracle(NARROW, weights), f16emu=O.DiTOracle(NARROW, weights, emulate_f16=True))


def _forward_case(cfg, model, orcs, B, N, ragged, bounds):
    cond, text, durations, y0 = synth_inputs(cfg, B, N, nt=24, n_ref=30, seed=B * 100 + N, ragged=ragged)
    step_cond = _pad_cond(cond, N)
    mask = O.lens_to_mask(torch.tensor(durations), N) if B > 1 else None
    t = 0.37
    pred, null = model.engine.dit_forward(y0.to(DEV), text.to(DEV), step_cond.to(DEV).contiguous(), [N] * B, durations, t, use_mask=B > 1)
    torch.cuda.synchronize()
    assert model.engine.saturation_events == 0
    for rname, tol in bounds.items():
        for nm, got, drop in (("pred", pred, False), ("null", null, True)):
            want = orcs[rname].forward(y0, step_cond, text, torch.tensor(t), drop, drop, mask)
            assert torch.isfinite(got).all()
            _, mean, refm = report(f"dit_forward[{model.precision}, dim {cfg.dim} inner {cfg.inner_dim}] {nm} vs oracle[{rname}] B{B} N{N}", got.cpu(), want)
            assert mean <= tol * max(1.0, refm), (model.precision, nm, rname)


@pytest.mark.parametrize("prec", ["f16", "bf16x3"])
@pytest.mark.parametrize("B,N,ragged", [(1, 150, False), (2, 200, True)])
def test_dit_forward_narrow(models, oracles, B, N, ragged, prec):
    _forward_case(NARROW, models[prec], oracles, B, N, ragged, FWD_BOUNDS[prec])


_SAMPLE_REF = {}


def _sample_inputs():
    return synth_inputs(NARROW, 2, 96, nt=20, n_ref=33, seed=19, ragged=True)


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_sample_narrow(models, oracles, method):
    """5-point solve, batch 2 with ragged durations, every solver; f16 and bf16x3 inside the gate on the final mel and the trajectory"""
    cond, text, durations, y0 = _sample_inputs()
    kw = dict(steps=5, method=method, cfg_strength=2.0, sway_sampling_coef=-1.0)
    dur_t = torch.tensor(durations)
    want, want_t, aux = O.sample(oracles["fp32"], cond, text, dur_t, y0=y0, return_aux=True, **kw)
    for prec in ("bf16x3", "f16"):
        out, traj = F5TTS(transformer=models[prec]).sample(cond, text, duration=dur_t, y0=y0, **kw)
        torch.cuda.synchronize()
        assert out.shape == (2, 96, NARROW.mel_dim) and traj.shape == (5, 2, 96, NARROW.mel_dim) and torch.isfinite(out).all()
        _, l1, _ = report(f"sample[{prec}, narrow] {method} final mel vs oracle[fp32]", out.cpu(), want)
        _, l1t, _ = report(f"sample[{prec}, narrow] {method} trajectory vs oracle[fp32]", traj.cpu(), want_t)
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (prec, method)
        cm = aux["cond_mask"]
        assert torch.equal(out.cpu()[cm], torch.nn.functional.pad(cond, (0, 0, 0, 96 - cond.shape[1]))[cm])


@pytest.mark.parametrize("prec", ["f16", "bf16x3"])
def test_graph_replay_equals_eager_narrow(models, prec):
    cond, text, durations, y0 = _sample_inputs()
    f5 = F5TTS(transformer=models[prec])
    kw = dict(duration=torch.tensor(durations), steps=5, method="midpoint", y0=y0)
    a, ta = [x.clone() for x in f5.sample(cond, text, use_graph=False, **kw)]
    b, tb = [x.clone() for x in f5.sample(cond, text, use_graph=True, **kw)]
    c, tc = f5.sample(cond, text, use_graph=True, **kw)          # replay of the cached graph
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ta, tb) and torch.equal(b, c) and torch.equal(tb, tc)


# ---- the per-row routes: the shared batch and helpers of the TINY tests (same vocabulary and mel width) --------------------------------
B, N, NREF = 3, 37, 12
DURS = GW.DURS


def _engine_args(inputs):
    cond, text, y0 = inputs
    text_c, lens, dur, nmax = prepare_lengths(text, NREF, B, torch.tensor(DURS), None, 4096, "euler")
    assert nmax == N and dur.tolist() == DURS
    cond_p = torch.zeros((B, N, NARROW.mel_dim), device=DEV)
    cond_p[:, :NREF] = cond.to(DEV)
    return text_c.to(DEV).contiguous(), cond_p, lens.tolist(), dur.tolist(), y0.to(DEV).contiguous()


def _rows_within_gate(tag, out, traj, want, want_t):
    for b in range(B):
        _, l1, _ = report(f"{tag} row {b} final mel", out[b].cpu(), want[b])
        _, l1t, _ = report(f"{tag} row {b} trajectory", traj[:, b].cpu(), want_t[:, b])
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (tag, b)


def test_per_row_controls_narrow(models, oracles):
    """one guidance strength per row (f5_sample_rows): the helper's single-guidance rule k = F + (F - N) c[b] with the window open throughout"""
    inputs = GW.inputs()
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    want, want_t, _ = GW.window_sample(oracles["fp32"], inputs[0], inputs[1], DURS, inputs[2], 4, "midpoint", GW.CFG_ROWS, [-1.0] * B, [2.0] * B)
    for prec in ("bf16x3", "f16"):
        out, traj = models[prec].engine.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), method="midpoint", cfg_strength=GW.CFG_ROWS,
                                               use_mask=True, use_graph=False)
        torch.cuda.synchronize()
        _rows_within_gate(f"rows [narrow, {prec}, midpoint]", out, traj, want, want_t)


def test_dual_guidance_narrow(models, oracles):
    inputs = GW.inputs()
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    a_rows, c_rows = [3.0, 0.0, 0.0], [0.5, 0.0, 2.0]                      # tests/test_dual_guidance_gpu.py: both, neither, text alone
    want, want_t = DG.dual_sample(oracles["fp32"], inputs[0], inputs[1], DURS, inputs[2], 5, "euler", a_rows, c_rows)
    for prec in ("bf16x3", "f16"):
        out, traj = models[prec].engine.sample(text, cond_p, lens, durs, y0, time_grid(5, -1.0), method="euler", cfg_strength=c_rows,
                                               use_mask=True, use_graph=False, audio_cfg_strength=a_rows)
        torch.cuda.synchronize()
        _rows_within_gate(f"dual [narrow, {prec}, euler]", out, traj, want, want_t)
        for b in range(B):
            assert torch.equal(out[b, :lens[b]].cpu(), cond_p[b, :lens[b]].cpu())


def test_guidance_window_narrow(models, oracles):
    inputs = GW.inputs()
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    want, want_t, rec = GW.window_sample(oracles["fp32"], inputs[0], inputs[1], DURS, inputs[2], 3, "rk4", GW.CFG_ROWS, GW.LO, GW.HI)
    wide = rec.any(dim=1)
    assert bool(wide.any()) and bool((~wide).any())                         # both kinds of evaluation run
    window = np.stack([np.asarray(GW.LO, np.float32), np.asarray(GW.HI, np.float32)], axis=1)
    for prec in ("bf16x3", "f16"):
        out, traj = models[prec].engine.sample(text, cond_p, lens, durs, y0, time_grid(3, -1.0), method="rk4", cfg_strength=GW.CFG_ROWS,
                                               use_mask=True, use_graph=False, cfg_interval=window)
        torch.cuda.synchronize()
        _rows_within_gate(f"window [narrow, {prec}, rk4]", out, traj, want, want_t)


def test_cond_keep_narrow(models, oracles):
    """speech editing: the conditioning kept by a mask.  The reference is built as tests/test_edit_gpu.py builds it: step_cond =
    where(keep, cond, 0), the oracle's two forwards, its solver on the time grid, the final where"""
    Bn, Nn, n_ref = 2, 96, 60
    cond, text, durations, y0 = synth_inputs(NARROW, Bn, Nn, nt=20, n_ref=n_ref, seed=19, ragged=True)
    keep = torch.ones((Bn, n_ref), dtype=torch.bool)
    keep[:, 20:35] = False
    keep[1, :10] = False
    keep[1, 50:] = False
    dit = oracles["fp32"]
    kw = dict(steps=4, method="rk4", cfg_strength=2.0, sway_sampling_coef=-1.0)
    _, _, aux = O.sample(dit, cond, text, torch.tensor(durations), y0=y0, return_aux=True, **kw)
    cond_p = torch.nn.functional.pad(cond, (0, 0, 0, Nn - n_ref))
    km = (torch.nn.functional.pad(keep, (0, Nn - n_ref), value=False) & aux["cond_mask"])[..., None]
    step_cond = torch.where(km, cond_p, torch.zeros_like(cond_p))

    def fn(t, x):
        pred = dit.forward(x, step_cond, aux["text"], t, False, False, aux["mask"])
        null = dit.forward(x, step_cond, aux["text"], t, True, True, aux["mask"])
        return pred + (pred - null) * 2.0

    want_t = O.odeint_rk4(fn, y0, O.time_grid(4, -1.0))
    want = torch.where(km, cond_p, want_t[-1])
    for prec in ("bf16x3", "f16"):
        out, traj = F5TTS(transformer=models[prec]).sample(cond, text, duration=torch.tensor(durations), y0=y0, edit_mask=keep, **kw)
        torch.cuda.synchronize()
        _, l1, _ = report(f"edit[{prec}, narrow] final mel vs oracle", out.cpu(), want)
        _, l1t, _ = report(f"edit[{prec}, narrow] trajectory vs oracle", traj.cpu(), want_t)
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, prec
        assert torch.equal(out.cpu()[km[..., 0]], cond_p[km[..., 0]])


@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
def test_isolate_rows_narrow(weights, oracles, prec):
    """isolate_rows: a row of a ragged batch equals its solo sample() -- each row against the oracle's sample of that row alone at its
    own length: inside the gate with the option on, and the two padded rows outside it with the option off (the criterion of
    tests/test_isolate_rows_gpu.py, on its durations), so the option is seen to act on this geometry"""
    durs = [128, 37, 70]
    Bn, Nn, n_ref = 3, 128, 16
    r = np.random.default_rng(5)
    cond = torch.from_numpy(r.standard_normal((Bn, n_ref, NARROW.mel_dim)).astype(np.float32))
    text = torch.from_numpy(r.integers(0, NARROW.text_num_embeds, (Bn, 12)).astype(np.int32))
    y0 = torch.zeros((Bn, Nn, NARROW.mel_dim))
    for b, d in enumerate(durs):
        y0[b, :d] = torch.from_numpy(r.standard_normal((NARROW.mel_dim, d)).astype(np.float32).T)
    kw = dict(steps=4, method="rk4", cfg_strength=2.0, sway_sampling_coef=-1.0)
    solo = [O.sample(oracles["fp32"], cond[b:b + 1], text[b:b + 1], torch.tensor([d]), y0=y0[b:b + 1, :d], **kw)[0][0] for b, d in enumerate(durs)]
    m = DiT.from_config(NARROW, precision=prec, device=DEV)
    m.load_weights(weights)
    dist = {}
    for option in (True, False):
        out, _ = F5TTS(transformer=m).sample(cond, text, duration=torch.tensor(durs), y0=y0, isolate_rows=option, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        dist[option] = [float((out[b, n_ref:d].cpu() - solo[b][n_ref:d]).abs().mean()) for b, d in enumerate(durs)]
    print(f"[isolate, narrow, {prec}] rows vs solo oracle: option on {dist[True]}, off {dist[False]} (gate {MEL_L1_TOL:g})")
    assert max(dist[True]) <= MEL_L1_TOL, dist[True]
    assert dist[False][1] > MEL_L1_TOL and dist[False][2] > MEL_L1_TOL, dist[False]


def test_forced_ln_fold_is_refused_on_a_narrow_geometry(models):
    """the fold's automatic choice never takes a geometry outside the old family (the calls above ran with ln_fold = -1), and a forced
    ln_fold = 1 is refused by the call with the fold's own message, before anything is launched"""
    cond, text, durations, y0 = _sample_inputs()
    eng = models["f16"].engine
    f5 = F5TTS(transformer=models["f16"])
    kw = dict(duration=torch.tensor(durations), steps=3, method="euler", y0=y0, use_graph=False)
    want, _ = [x.clone() for x in f5.sample(cond, text, **kw)]
    eng.set_option("ln_fold", 1)
    try:
        with pytest.raises(RuntimeError, match=r"ln_fold = 1: this shape / precision cannot run the folded LN.*heads \* dim_head == dim"):
            f5.sample(cond, text, **kw)
    finally:
        eng.set_option("ln_fold", -1)
    got, _ = f5.sample(cond, text, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, want)                                   # the handle is as it was


# ---- the relaxations one at a time ----------------------------------------------------------------------------------------------------
def test_inner_width_alone():
    """dim 512 with 4 heads: inner width 256 under 64-channel conv-pos groups and 256-wide text; one forward and one 5-point Euler sample"""
    cfg = INNER_ONLY
    w = synthetic_weights(cfg, seed=42)
    orcs = dict(fp32=O.DiTOracle(cfg, w), f16emu=O.DiTOracle(cfg, w, emulate_f16=True))
    for prec in ("f16", "bf16x3"):
        m = DiT.from_config(cfg, precision=prec, device=DEV)
        m.load_weights(w)
        _forward_case(cfg, m, orcs, 2, 150, True, FWD_BOUNDS[prec])
        cond, text, durations, y0 = synth_inputs(cfg, 2, 96, nt=20, n_ref=33, seed=19, ragged=True)
        kw = dict(steps=5, method="euler", cfg_strength=2.0, sway_sampling_coef=-1.0)
        want, want_t = O.sample(orcs["fp32"], cond, text, torch.tensor(durations), y0=y0, **kw)
        out, traj = F5TTS(transformer=m).sample(cond, text, duration=torch.tensor(durations), y0=y0, **kw)
        torch.cuda.synchronize()
        _, l1, _ = report(f"sample[{prec}, inner only] euler final mel vs oracle[fp32]", out.cpu(), want)
        _, l1t, _ = report(f"sample[{prec}, inner only] euler trajectory vs oracle[fp32]", traj.cpu(), want_t)
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, prec


def test_upstream_small_in_miniature():
    """dim 768, 12 heads, text 512: inside the old family but for the 48-channel conv-pos groups"""
    cfg = UPSTREAM_SMALL_MINI
    w = synthetic_weights(cfg, seed=42)
    orcs = dict(fp32=O.DiTOracle(cfg, w), f16emu=O.DiTOracle(cfg, w, emulate_f16=True))
    for prec in ("f16", "bf16x3"):
        m = DiT.from_config(cfg, precision=prec, device=DEV)
        m.load_weights(w)
        _forward_case(cfg, m, orcs, 2, 200, True, FWD_BOUNDS[prec])
