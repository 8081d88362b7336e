"""Guidance window on the GPU (docs/guidance_window.md): a row is guided only at function evaluations whose time lies in its [lo, hi];
an evaluation in which no row is guided runs the conditional branch alone.

TINY, B = 3, ragged 23 / 37 / 31 (the shapes of tests/test_row_controls_gpu.py); Euler 5 points, midpoint 4, rk4 3.  f5_sample_window
against the reference helper (tests/guidance_window_ref.py) with single and with dual guidance, the wide / narrow pattern against the
helper's record, the full and the empty window against the calls they must equal bit for bit, prefixes of a trajectory, row
independence, graphs (one per pattern, whatever the values), refusals, and the Python layers down from generate_many."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import guidance_window_ref as GW
from f5test import DEV, E, O, TINY, report, stream, synthetic_weights
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths, time_grid
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-3                  # the project's mel-L1 gate
B, N, NT, NREF, DURS = GW.B, GW.N, GW.NT, GW.NREF, GW.DURS
FULL = (-1.0, 2.0)
EMPTY = (0.01, 0.05)               # between the first two evaluation times of every solver case: contains none
GUIDANCE = {"single": (None, GW.CFG_ROWS), "dual": (GW.DUAL_A, GW.DUAL_C)}
PER = GW.PER_STEP


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
    return GW.inputs()


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


def _reference(oracle, inputs, method, steps, which):
    """the helper's (final mel, trajectory, record) for the windows GW.LO / GW.HI, computed once per solver and kind of guidance"""
    key = (method, steps, which)
    if key not in _ref:
        cond, text, y0 = inputs
        audio, strengths = GUIDANCE[which]
        _ref[key] = GW.window_sample(oracle, cond, text, DURS, y0, steps, method, strengths, GW.LO, GW.HI, audio=audio)
    return _ref[key]


def _sample(eng, inputs, method, steps, which="single", window=None, strengths=None, audio="same", **kw):
    """Engine.sample on the shared batch -> clones of (out, trajectory); window = None: the call without cfg_interval"""
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    a, c = GUIDANCE[which]
    a = a if audio == "same" else audio
    kw.setdefault("use_graph", False)
    out, traj = eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), method=method, cfg_strength=c if strengths is None else strengths,
                           use_mask=True, audio_cfg_strength=a, cfg_interval=window, **kw)
    torch.cuda.synchronize()
    return out.clone(), traj.clone()


def _pairs(lo=GW.LO, hi=GW.HI):
    return np.stack([np.asarray(lo, np.float32), np.asarray(hi, np.float32)], axis=1)


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["single", "dual"])
@pytest.mark.parametrize("method,steps", GW.SOLVER_CASES)
def test_sample_window_against_the_reference_helper(models, oracle, inputs, method, steps, which):
    """Measured on one MI355X (bf16x3, mean |delta| of row b, final mel / trajectory): see docs/guidance_window.md."""
    want, want_t, rec = _reference(oracle, inputs, method, steps, which)
    # every bound at least 1e-3 from every evaluation time of its row: the comparison does not hang on the rounding of a time
    times = GW.eval_times(O.time_grid(steps, -1.0), method)
    for b in range(B):
        gap = float(torch.cat([(times - GW.LO[b]).abs(), (times - GW.HI[b]).abs()]).min())
        assert gap >= 1e-3, (method, b, gap)
    # the pattern exercises all three kinds of evaluation
    wide = rec.any(dim=1)
    assert bool(wide.any()) and bool((~wide).any()) and bool((wide & ~rec.all(dim=1)).any()), (method, rec.tolist())
    eng = models["bf16x3"].engine
    out, traj = _sample(eng, inputs, method, steps, which, _pairs())
    assert traj.shape == (steps, B, N, TINY.mel_dim) and torch.isfinite(out).all()
    lens = _engine_args(inputs)[2]
    for b in range(B):
        _, l1, _ = report(f"window [{which}, {method}] row {b} final mel", out[b].cpu(), want[b])
        _, l1t, _ = report(f"window [{which}, {method}] row {b} trajectory", traj[:, b].cpu(), want_t[:, b])
        assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL, (which, method, b)
        assert torch.equal(out[b, :lens[b]].cpu(), inputs[0][b, :lens[b]])            # kept frames are cond, bit for bit
    # not by indifference: the call guided throughout is far from the helper's windowed result
    full, _ = _sample(eng, inputs, method, steps, which, FULL)
    far = float((full.cpu() - want).abs().mean())
    print(f"window [{which}, {method}]: guided throughout vs the helper's window: mean |delta| = {far:.3f}")
    assert far > 10 * MEL_L1_TOL


# ---- 2. pattern ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps", GW.SOLVER_CASES)
def test_pattern_equals_the_helpers_record(models, oracle, inputs, method, steps):
    eng = models["f16"].engine
    for which in ("single", "dual"):
        rec = _reference(oracle, inputs, method, steps, which)[2]
        _sample(eng, inputs, method, steps, which, _pairs())
        got = eng.last_sample_pattern()
        assert got.dtype == np.uint8 and got.tolist() == GW.pattern_of(rec).tolist(), (method, which)
        # the hook honours its capacity: the count in full, the flags up to `cap`
        nfe, buf = C.c_int(), np.full(16, 7, np.uint8)
        E.check(eng.lib.f5_debug_last_sample_pattern(eng._h, C.byref(nfe), C.c_void_p(buf.ctypes.data), 2))
        assert nfe.value == len(rec) and buf[:2].tolist() == got[:2].tolist() and bool((buf[2:] == 7).all())


# ---- 3. full window -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["single", "dual"])
@pytest.mark.parametrize("method,steps", GW.SOLVER_CASES)
def test_full_window_is_the_call_without_one(models, inputs, method, steps, which):
    eng = models["f16"].engine
    want, want_t = _sample(eng, inputs, method, steps, which)                        # f5_sample_rows / f5_sample_dual
    got, got_t = _sample(eng, inputs, method, steps, which, FULL)
    assert torch.equal(got, want) and torch.equal(got_t, want_t)
    assert eng.last_sample_pattern().tolist() == [1] * ((steps - 1) * PER[method])
    assert eng.saturation_events == 0


# ---- 4. never guided ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps", GW.SOLVER_CASES)
def test_empty_window_is_the_unguided_call(models, inputs, method, steps):
    eng = models["f16"].engine
    times = GW.eval_times(O.time_grid(steps, -1.0), method)
    assert not bool(((times >= EMPTY[0]) & (times <= EMPTY[1])).any())
    want, want_t = _sample(eng, inputs, method, steps, "single", strengths=[0.0] * B)      # f5_sample_rows, one branch
    got, got_t = _sample(eng, inputs, method, steps, "single", EMPTY)
    assert torch.equal(got, want) and torch.equal(got_t, want_t)
    assert eng.last_sample_pattern().tolist() == [0] * ((steps - 1) * PER[method])
    guided, _ = _sample(eng, inputs, method, steps, "single")
    assert not torch.equal(guided, want)
    # dual guidance: the three-branch plan run on its first branch alone, as f5_sample_dual does with both strengths 0
    want, want_t = _sample(eng, inputs, method, steps, "dual", strengths=[0.0] * B, audio=[0.0] * B)
    got, got_t = _sample(eng, inputs, method, steps, "dual", EMPTY)
    assert torch.equal(got, want) and torch.equal(got_t, want_t)
    assert eng.last_sample_pattern().tolist() == [0] * ((steps - 1) * PER[method])


# ---- 5. prefixes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps,edge", [("euler", 5, 0.2), ("midpoint", 4, 0.2), ("rk4", 3, 0.5)])
def test_trajectory_prefixes(models, inputs, method, steps, edge):
    """A window that closes at `edge`: every evaluation before the first narrow one is the full-window call's, so the trajectory points
    of the steps that end before it are too.  One that opens there: the same against the unguided call."""
    eng = models["f16"].engine
    times = GW.eval_times(O.time_grid(steps, -1.0), method)
    assert float((times - edge).abs().min()) >= 1e-3
    for window, strengths, first_other in (((-1.0, edge), None, 0), ((edge, 2.0), [0.0] * B, 1)):
        # the full-window call with the rows' strengths, and f5_sample_rows with every strength 0
        base, base_t = _sample(eng, inputs, method, steps, "single", FULL if strengths is None else None, strengths=strengths)
        got, got_t = _sample(eng, inputs, method, steps, "single", window)
        pat = eng.last_sample_pattern().tolist()
        j = pat.index(first_other)                                # the first evaluation that differs in kind from the base call's
        assert 0 < j < len(pat) and pat == [1 - first_other] * j + [first_other] * (len(pat) - j), (window, pat)
        same = j // PER[method] + 1                               # trajectory points 0 .. same-1 come from evaluations before j
        assert same >= 2 and torch.equal(got_t[:same], base_t[:same]), (window, same)
        assert not torch.equal(got_t[same], base_t[same]) and not torch.equal(got, base)


# ---- 6. rows are independent ------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent(models, inputs):
    eng = models["f16"].engine
    res, pats = [], []
    # row 1: another window (other evaluations are inside it) and other strengths; rows 0 and 2 keep theirs, and so does the pattern
    for lo1, hi1, c1, a1 in ((GW.LO[1], GW.HI[1], GW.DUAL_C[1], GW.DUAL_A[1]), (0.05, 0.55, 0.7, 1.9)):
        lo, hi = [GW.LO[0], lo1, GW.LO[2]], [GW.HI[0], hi1, GW.HI[2]]
        res.append(_sample(eng, inputs, "midpoint", 4, "dual", _pairs(lo, hi), strengths=[GW.DUAL_C[0], c1, GW.DUAL_C[2]],
                           audio=[GW.DUAL_A[0], a1, GW.DUAL_A[2]]))
        pats.append(eng.last_sample_pattern().tolist())
    (oa, ta), (ob, tb) = res
    assert pats[0] == pats[1] and 0 in pats[0] and 1 in pats[0]                  # the same launches ran
    assert eng.saturation_events == 0
    for b in (0, 2):
        assert torch.equal(oa[b], ob[b]) and torch.equal(ta[:, b], tb[:, b]), b
    assert not torch.equal(oa[1], ob[1]) and not torch.equal(ta[1:, 1], tb[1:, 1])
    assert torch.equal(ta[0], _engine_args(inputs)[4]) and torch.equal(tb[0], ta[0])


# ---- 7. graphs --------------------------------------------------------------------------------------------------------------------------------
def test_one_graph_per_pattern_whatever_the_values(models, inputs):
    eng = models["f16"].engine
    method, steps = "rk4", 3
    sets = {"a": dict(window=_pairs(), strengths=GW.CFG_ROWS),
            "b": dict(window=_pairs([0.06, 0.25, 0.62], [0.45, 0.5, 0.95]), strengths=[0.7, 2.5, 1.0]),       # other values, the same pattern
            "c": dict(window=_pairs([0.05, 0.2, 0.6], [0.4, 0.55, 1.5]), strengths=GW.CFG_ROWS)}              # row 2 reaches t = 1: another pattern
    eager, pats = {}, {}
    for k, kw in sets.items():
        eager[k] = _sample(eng, inputs, method, steps, "single", **kw)
        pats[k] = eng.last_sample_pattern().tolist()
    assert pats["a"] == pats["b"] != pats["c"] and not torch.equal(eager["a"][0], eager["b"][0])
    rows = _sample(eng, inputs, method, steps, "single")
    c0 = eng.graph_count()

    def run(key):
        out, traj = _sample(eng, inputs, method, steps, "single", use_graph=True, **sets[key])
        assert torch.equal(out, eager[key][0]) and torch.equal(traj, eager[key][1]), key          # replay equals eager, bitwise
        assert eng.last_sample_pattern().tolist() == pats[key]

    run("a")
    assert eng.graph_count() == c0 + 1
    run("b")
    assert eng.graph_count() == c0 + 1                                   # other strengths and bounds, the same pattern: the same graph
    run("c")
    assert eng.graph_count() == c0 + 2                                   # another pattern: its own graph
    run("a")
    run("c")
    assert eng.graph_count() == c0 + 2                                   # ... and both replay correctly afterwards
    out, traj = _sample(eng, inputs, method, steps, "single", use_graph=True)
    assert eng.graph_count() == c0 + 3                                   # the rows route of the same shape keeps its own entry and bits
    assert torch.equal(out, rows[0]) and torch.equal(traj, rows[1])
    # one graph per ODE step (engine option graph_split): the same kernels, the same bits
    eng.set_option("graph_split", 1)
    try:
        run("a")
        run("a")
    finally:
        eng.set_option("graph_split", 0)
    assert eng.graph_count() == c0 + 4


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_sample_window_refusals_launch_nothing(models, inputs):
    from f5_tts_mlx_amd.cfm import time_grid_rows
    eng = models["bf16x3"].engine
    lib = eng.lib
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    steps = 3
    ws = eng.workspace(B, N, NT, steps, "euler", rows="window_dual")
    out = torch.full_like(cond_p, -12345.0)
    traj = torch.full((steps, B, N, TINY.mel_dim), -12345.0, device=DEV)
    a, keep = eng._args(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), steps, "euler", 2.0, True, False, out, traj, ws)
    tr = time_grid_rows(steps, [-1.0, None, -0.5])
    f32 = lambda v: np.asarray(v, np.float32)                             # noqa: E731
    ar, cr, lo, hi = f32(GW.DUAL_A), f32(GW.DUAL_C), f32(GW.LO), f32(GW.HI)
    sizes = {}
    for name, fn, extra in (("rows", "f5_workspace_bytes_rows", ()), ("dual", "f5_workspace_bytes_dual", ()),
                            ("win", "f5_workspace_bytes_window", (0,)), ("win_dual", "f5_workspace_bytes_window", (1,))):
        v = C.c_size_t()
        E.check(getattr(lib, fn)(eng._h, B, N, NT, steps, 0, *extra, C.byref(v)))
        sizes[name] = v.value
    assert sizes["win"] > sizes["rows"] and sizes["win_dual"] > sizes["dual"] and ws.numel() >= sizes["win_dual"]
    graphs = eng.graph_count()
    seen = set()

    def refused(wc, msg, named=True):
        rc = lib.f5_sample_window(eng._h, C.byref(a), None if wc is None else C.byref(wc), stream())
        err = lib.f5_last_error().decode()
        assert rc != 0 and msg in err and (not named or "f5_sample_window" in err), (msg, rc, err)
        seen.add(re.sub(r"\d+", "#", err))

    def W(t=tr, c=cr, au=ar, lo_=lo, hi_=hi):
        return E.F5WindowControls(*(0 if x is None else x.ctypes.data for x in (t, c, au, lo_, hi_)), 0)

    def poked(x, i, v):
        y = x.copy()
        y.reshape(-1)[i] = v
        return y

    bad = [poked(tr, 5, np.nan), poked(cr, 2, np.inf), poked(ar, 0, np.nan), poked(lo, 1, -np.inf), poked(hi, 2, np.nan), poked(lo, 0, 0.5)]
    refused(None, "controls is null")
    refused(W(t=None), "controls.t_rows is null")
    refused(W(c=None), "controls.text_cfg_rows is null")
    refused(W(lo_=None), "controls.lo_rows is null")
    refused(W(hi_=None), "controls.hi_rows is null")
    refused(W(t=bad[0]), "t_rows[1][2] is not finite")
    refused(W(c=bad[1]), "text_cfg_rows[2] is not finite")
    refused(W(au=bad[2]), "audio_cfg_rows[0] is not finite")
    refused(W(lo_=bad[3]), "lo_rows[1] is not finite")
    refused(W(hi_=bad[4]), "hi_rows[2] is not finite")
    refused(W(lo_=bad[5]), "lo_rows[0] = 0.5 is above hi_rows[0] = 0.4")
    ok, ok_single = W(), W(au=None)
    a.workspace_bytes = sizes["dual"]                                     # the dual plan has no room for the tables ...
    refused(ok, "f5_workspace_bytes_window")
    a.workspace_bytes = sizes["rows"]                                     # ... nor has the rows plan for single guidance
    refused(ok_single, "f5_workspace_bytes_window")
    assert len(seen) == 12                                                # each refusal its own message (the two workspace ones share theirs)
    a.workspace_bytes = ws.numel()
    a.method = 7
    refused(ok, "Unknown method", named=False)                            # ... and everything f5_sample refuses
    a.method = 0
    eng.set_option("ln_fold", 1)
    try:
        refused(ok, "ln_fold = 1")
        refused(ok_single, "ln_fold = 1")
    finally:
        eng.set_option("ln_fold", -1)
    eng.set_option("null_keeps_cond", 1)
    try:
        refused(ok, "null_keeps_cond = 1")                                # dual guidance only: single guidance keeps f5_sample_rows' rule
    finally:
        eng.set_option("null_keeps_cond", 0)
    with pytest.raises(RuntimeError, match="f5_sample_window.*hi_rows\\[1\\] is not finite"):
        eng.sample(text, cond_p, lens, durs, y0, time_grid(steps, -1.0), method="euler", cfg_strength=2.0, use_graph=False, out=out,
                   trajectory=traj, cfg_interval=[(0.0, 1.0), (0.0, float("inf")), (0.0, 1.0)])
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all()) and bool((traj == -12345.0).all()) and eng.graph_count() == graphs
    del keep


def test_mxfp8_engine_refuses_the_window(tiny_weights, inputs):
    eng = E.Engine(TINY, precision="mxfp8", device=DEV)
    eng.load_weights(tiny_weights)
    text, cond_p, lens, durs, y0 = _engine_args(inputs)
    out = torch.full_like(cond_p, -12345.0)
    traj = torch.full((4, B, N, TINY.mel_dim), -12345.0, device=DEV)
    for audio in (None, GW.DUAL_A):
        with pytest.raises(RuntimeError, match="f5_sample_window.*mxfp8"):
            eng.sample(text, cond_p, lens, durs, y0, time_grid(4, -1.0), method="euler", cfg_strength=GW.CFG_ROWS, use_mask=True, use_graph=False,
                       out=out, trajectory=traj, audio_cfg_strength=audio, cfg_interval=_pairs())
    torch.cuda.synchronize()
    assert bool((out == -12345.0).all()) and bool((traj == -12345.0).all())        # nothing was launched


# ---- 9. the Python layers -------------------------------------------------------------------------------------------------------------------
def test_f5tts_sample_equals_the_engine_call(models, inputs):
    cond, text, y0 = inputs
    eng = models["bf16x3"].engine
    f5 = F5TTS(transformer=models["bf16x3"])
    kw = dict(duration=torch.tensor(DURS), steps=4, method="midpoint", y0=y0, use_graph=False, sway_sampling_coef=-1.0)
    pairs = [tuple(p) for p in _pairs().tolist()]
    got, got_t = [x.clone() for x in f5.sample(cond, text, cfg_strength=GW.DUAL_C, audio_cfg_strength=GW.DUAL_A, cfg_interval=pairs, **kw)]
    pat = eng.last_sample_pattern().tolist()
    want, want_t = _sample(eng, inputs, "midpoint", 4, "dual", _pairs())
    assert torch.equal(got, want) and torch.equal(got_t, want_t) and 0 in pat and 1 in pat
    # one pair for the whole batch is that pair in every row, with single guidance and a scalar strength as well
    got, _ = [x.clone() for x in f5.sample(cond, text, cfg_strength=2.0, cfg_interval=(0.1, 0.4), **kw)]
    want, _ = _sample(eng, inputs, "midpoint", 4, "single", _pairs([0.1] * B, [0.4] * B), strengths=[2.0] * B)
    assert torch.equal(got, want)
    # without the argument: the call it was
    got, _ = [x.clone() for x in f5.sample(cond, text, cfg_strength=2.0, **kw)]
    text_d, cond_p, lens, durs, y0_d = _engine_args(inputs)
    want, _ = eng.sample(text_d, cond_p, lens, durs, y0_d, time_grid(4, -1.0), method="midpoint", cfg_strength=2.0, use_mask=True, use_graph=False)
    assert torch.equal(got, want)


def test_split_halves_get_their_rows_of_the_window(tiny_weights, inputs):
    """Engine._sample_split: each half batch gets its rows of the windows; utterances do not interact, so the bits are the unsplit call's"""
    m = DiT.from_config(TINY, precision="f16", device=DEV)
    m.load_weights(tiny_weights)
    eng = m.engine
    want = {(w, g): _sample(eng, inputs, "euler", 5, w, _pairs(), use_graph=g) for w in ("single", "dual") for g in (False, True)}
    eng.split_batch = 2
    n0 = eng.split_events
    for rep in range(2):                               # the first call of a set of controls runs the halves one after the other
        for (w, g), (wo, wt) in want.items():
            out, traj = _sample(eng, inputs, "euler", 5, w, _pairs(), use_graph=g)
            assert torch.equal(out, wo) and torch.equal(traj, wt), (rep, w, g)
    assert eng.split_events == n0 + 8 and eng.saturation_events == 0
    # rows 0 - 1 ran on this handle, row 2 on the sibling: each saw the pattern of its own rows
    rec = (torch.tensor(GW.LO)[None] <= GW.eval_times(O.time_grid(5, -1.0), "euler")[:, None]) & \
          (GW.eval_times(O.time_grid(5, -1.0), "euler")[:, None] <= torch.tensor(GW.HI)[None])
    assert eng.last_sample_pattern().tolist() == rec[:, :2].any(dim=1).int().tolist()
    assert eng._sibling.last_sample_pattern().tolist() == rec[:, 2:].any(dim=1).int().tolist()


def test_generate_many_and_requests_file_reach_the_window_call(models, monkeypatch, tmp_path):
    """a `controls` entry and the "cfg_interval" key of a --requests line end in the same f5_sample_window call: the same waves, bit for
    bit, and a pattern with narrow evaluations; without the key the call is guided throughout and gives other waves"""
    vocab = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}
    idx = torch.arange(256, device=DEV) % 100

    def voc(mel, lens=None):
        return mel[:, :, idx].reshape(mel.shape[0], -1)

    eng = models["bf16x3"].engine
    f5 = F5TTS(transformer=models["bf16x3"], vocab_char_map=vocab, vocoder=voc)
    src, sr = G.read_wav(G.pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav"))
    ref = str(tmp_path / "ref.wav")
    G.write_wav(ref, np.asarray(src, np.float32)[24_000:24_000 + 30 * 256 + 9], 24_000)
    reqs = [("Hello there.", ref, "some call me nature."), ("Short one", ref, "others call me.")]
    kw = dict(steps=5, method="euler", seed=5, estimate_duration=True, f5tts=f5)
    by_controls = [w.clone() for w in G.generate_many(reqs, controls=[dict(cfg_interval=[0.05, 0.4]), dict(cfg_interval=(0.2, 0.55))], **kw)]
    pat = eng.last_sample_pattern().tolist()
    assert pat == [0, 1, 1, 0]                         # euler-5 evaluates at 0, .0761, .2929, .6173
    plain = G.generate_many(reqs, **kw)
    assert not torch.equal(plain[0], by_controls[0])
    f = tmp_path / "reqs.jsonl"
    outs = [str(tmp_path / f"out{i}.wav") for i in range(2)]
    f.write_text("".join(json.dumps(dict(text=t, ref_audio=p, ref_text=rt, output=o, cfg_interval=w)) + "\n"
                         for (t, p, rt), o, w in zip(reqs, outs, ([0.05, 0.4], [0.2, 0.55]))))
    monkeypatch.setattr(G.F5TTS, "from_pretrained", classmethod(lambda cls, *a, **k: f5))
    G.main(["--requests", str(f), "--steps", "5", "--method", "euler", "--seed", "5", "--estimate-duration", "1"])
    assert eng.last_sample_pattern().tolist() == pat
    for o, want in zip(outs, by_controls):
        got, _ = G.read_wav(o)
        assert np.array_equal(np.asarray(got, np.float32), want.cpu().numpy())
