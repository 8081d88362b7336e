"""Guidance window, host side (docs/guidance_window.md): the workspace plan, the struct, the refusals that need no device, the new control
on its way from generate_many / a --requests file / the command line to F5TTS.sample, Engine's control normalisation, and the reference
helper's own power to tell the rule from three seeded mistakes.  No GPU."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

import guidance_window_ref as GW
import test_multivoice_host as MV
import test_row_controls_host as RH
from f5test import O, ROOT, TINY, DiTConfig, synthetic_weights
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import time_grid, time_grid_rows

FMAX = float(np.finfo(np.float32).max)


def _handle(lib, cfg, prec):
    h = C.c_void_p()
    cc = E.to_c_config(cfg)
    assert lib.f5_engine_create(C.byref(cc), E.PRECISIONS[prec], C.byref(h)) == 0, lib.f5_last_error()
    return h


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,prec,B,N,nt,steps,method", [("tiny", "bf16x3", 3, 37, 9, 5, "euler"), ("tiny", "f16", 2, 80, 16, 3, "rk4"),
                                                              ("full", "f16", 2, 937, 120, 32, "euler"), ("tiny", "f16", 3, 37, 9, 1, "midpoint")])
def test_workspace_plan_is_the_rows_or_dual_plan_plus_the_tables(cfgname, prec, B, N, nt, steps, method):
    lib = E.load_library()
    h = _handle(lib, TINY if cfgname == "tiny" else DiTConfig(), prec)
    try:
        def size(fn, *extra):
            v = C.c_size_t()
            assert getattr(lib, fn)(h, B, N, nt, steps, E.METHODS[method], *extra, C.byref(v)) == 0, lib.f5_last_error()
            return v.value

        rows, dual = size("f5_workspace_bytes_rows"), size("f5_workspace_bytes_dual")
        nfe = max((steps - 1) * GW.PER_STEP[method], 1)
        pad = lambda n: (n + 255) // 256 * 256                       # noqa: E731  (the plan's allocation granule)
        assert size("f5_workspace_bytes_window", 0) == rows + pad(nfe * B * 4)              # one [nfe][B] table behind the rows plan
        assert size("f5_workspace_bytes_window", 1) == dual + pad(2 * nfe * B * 4)          # two behind the dual plan
        v = C.c_size_t()
        assert lib.f5_workspace_bytes_window(h, 0, N, nt, steps, 0, 0, C.byref(v)) != 0 and b"bad sizes" in lib.f5_last_error()
        assert lib.f5_workspace_bytes_window(h, B, N, nt, steps, 9, 0, C.byref(v)) != 0 and b"Unknown method" in lib.f5_last_error()
        assert lib.f5_workspace_bytes_window(h, B, N, nt, steps, 0, 1, None) != 0 and b"null argument" in lib.f5_last_error()
    finally:
        lib.f5_engine_destroy(h)


def test_sample_window_refuses_null_controls_without_a_device():
    lib = E.load_library()
    h = _handle(lib, TINY, "f16")
    try:
        a = E.F5SampleArgs()
        p = np.ones(4, np.float32).ctypes.data
        W = E.F5WindowControls
        seen = set()
        for wc, msg in ((None, "controls is null"), (W(0, p, p, p, p, 0), "controls.t_rows is null"),
                        (W(p, 0, p, p, p, 0), "controls.text_cfg_rows is null"), (W(p, p, 0, 0, p, 0), "controls.lo_rows is null"),
                        (W(p, p, 0, p, 0, 0), "controls.hi_rows is null"),
                        (W(p, p, 0, p, p, 0), "weights are not finalized")):     # audio_cfg_rows may be null: single guidance
            rc = lib.f5_sample_window(h, C.byref(a), None if wc is None else C.byref(wc), C.c_void_p(0))
            err = lib.f5_last_error().decode()
            assert rc != 0 and msg in err and (msg.startswith("weights") or err.startswith("f5_sample_window: ")), (msg, err)
            seen.add(err)
        assert len(seen) == 6 and lib.f5_engine_graph_count(h) == 0
        nfe = C.c_int(-1)
        assert lib.f5_debug_last_sample_pattern(h, C.byref(nfe), None, 0) == 0 and nfe.value == 0      # no window call yet
        assert lib.f5_debug_last_sample_pattern(h, None, None, 0) != 0
    finally:
        lib.f5_engine_destroy(h)


def test_window_controls_struct_matches_the_header(tmp_path):
    fields = ("t_rows", "text_cfg_rows", "audio_cfg_rows", "lo_rows", "hi_rows", "cond_keep_dev")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "f5tts_hip.h"\nint main(void){printf("%zu %zu %zu'
                   + " %zu" * len(fields) + '\\n", sizeof(f5_window_controls), sizeof(f5_row_controls), sizeof(f5_dual_controls), '
                   + ", ".join(f"offsetof(f5_window_controls, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", ROOT + "/include", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = E.F5WindowControls
    assert [n for n, _ in W._fields_] == list(fields)
    assert got == [C.sizeof(W), C.sizeof(E.F5RowControls), C.sizeof(E.F5DualControls)] + [getattr(W, f).offset for f in fields]


# ---- Engine's control normalisation ---------------------------------------------------------------------------------------------------
def test_engine_row_controls_with_cfg_interval():
    t = time_grid(5, -1.0)
    c = E.Controls.of(t, 2.0, 3, None, None)                                   # None: today's call
    assert c.steps == 5 and c.plan is False and c.struct()[1] is None
    c = E.Controls.of(t, 2.0, 3, cfg_interval=(0.25, 0.5))                     # one pair selects the route and is broadcast, with t and cfg
    assert c.steps == 5 and c.lo is not None and c.audio is None and c.plan == "window"
    tr, cr, lo, hi = c.t, c.cfg, c.lo, c.hi
    assert tr.shape == (3, 5) and all(np.array_equal(r, t) for r in tr) and cr.tolist() == [2.0] * 3
    assert lo.tolist() == [0.25] * 3 and hi.tolist() == [0.5] * 3
    assert all(x.dtype == np.float32 and x.flags["C_CONTIGUOUS"] for x in (tr, cr, lo, hi))
    grids = time_grid_rows(5, [-1.0, None, -0.5])
    pairs = [[0.0, 0.5], [0.25, 0.75], [-1.0, 2.0]]
    c = E.Controls.of(grids, [0.5, 0.0, 2.0], 3, [3.0, 0.0, 0.0], pairs)       # per-row forms of everything, dual guidance
    assert c.audio is not None and c.plan == "window_dual" and np.array_equal(c.t, grids)
    assert c.cfg.tolist() == [0.5, 0.0, 2.0] and c.audio.tolist() == [3.0, 0.0, 0.0]
    assert c.lo.tolist() == [0.0, 0.25, -1.0] and c.hi.tolist() == [0.5, 0.75, 2.0]
    # rows without a window keep their plans
    assert E.Controls.of(t, [1.0, 2.0, 3.0], 3).plan is True and E.Controls.of(t, 2.0, 3, 1.0).plan == "dual"
    for bad in ([0.1, 0.2, 0.3], [[0.1, 0.2]] * 2, 0.5, [[0.1, 0.2, 0.3]] * 3):
        with pytest.raises(ValueError, match=r"cfg_interval: expected \(lo, hi\) or 3 pairs of shape \(3, 2\)"):
            E.Controls.of(t, 2.0, 3, cfg_interval=bad)
    with pytest.raises(ValueError, match="expected 3 values"):
        E.Controls.of(t, [1.0, 2.0], 3, cfg_interval=(0.0, 1.0))
    with pytest.raises(ValueError, match="audio_cfg_strength: expected 3 values"):
        E.Controls.of(t, 2.0, 3, [1.0, 2.0], (0.0, 1.0))
    # the halves of a split call get their rows
    assert E.Controls.of(t, 2.0, 3, None, None).slice(1, 3).lo is None
    half = E.Controls.of(t, 2.0, 3, cfg_interval=(0.1, 0.2)).slice(1, 3)
    assert half.lo.tolist() == [np.float32(0.1)] * 2 and half.hi.tolist() == [np.float32(0.2)] * 2
    half = E.Controls.of(t, 2.0, 3, cfg_interval=pairs).slice(1, 3)
    assert np.array_equal(np.stack([half.lo, half.hi], 1), np.asarray(pairs[1:], np.float32))


# ---- generate / generate_many / requests file / command line ---------------------------------------------------------------------------
def _voc(mel, lens):
    return mel[:, :-1, 0].repeat_interleave(256, dim=1)


D = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, speed=1.0)


def test_request_controls_with_the_interval_key():
    assert G.request_controls(None, 2, [0, 0, 1], D) == D and set(G.CONTROL_KEYS) == set(D)          # the tuple keeps its four keys
    got = G.request_controls([dict(cfg_interval=[0.25, 0.5]), dict(cfg_strength=0.5)], 2, [0, 0, 1], D)
    assert got == dict(D, cfg_strength=[2.0, 2.0, 0.5], cfg_interval=[(0.25, 0.5), (0.25, 0.5), (-FMAX, FMAX)])
    assert G.WHOLE_INTERVAL == (-FMAX, FMAX) and all(isinstance(v, float) for pair in got["cfg_interval"] for v in pair)
    # a call-level pair is the default of the rows that do not override it, and always becomes one pair per row
    got = G.request_controls([None, dict(cfg_interval=(0, 1))], 2, [0, 0, 1], dict(D, cfg_interval=[0.1, 0.6]))
    assert got["cfg_interval"] == [(0.1, 0.6), (0.1, 0.6), (0.0, 1.0)] and got["cfg_strength"] == 2.0
    assert G.request_controls(None, 2, [0, 0, 1], dict(D, cfg_interval=(0.1, 0.6)))["cfg_interval"] == [(0.1, 0.6)] * 3
    # beside the audio key
    got = G.request_controls([dict(cfg_interval=[0.5, 0.5], audio_cfg_strength=3.0), None], 2, [0, 1], D)
    assert got["cfg_interval"] == [(0.5, 0.5), (-FMAX, FMAX)] and got["audio_cfg_strength"] == [3.0, 2.0]


BAD_PAIRS = [([0.5, 0.25], "must have lo <= hi"), ([0.1, float("nan")], "must be a finite number"), ([float("-inf"), 0.5], "must be a finite number"),
             ([0.1], r"must be a pair \(lo, hi\)"), ([0.1, 0.2, 0.3], r"must be a pair \(lo, hi\)"), (0.5, r"must be a pair \(lo, hi\)"),
             ("ab", r"must be a pair \(lo, hi\)"), (["0.1", 0.5], "must be a finite number"), ([True, 0.5], "must be a finite number"),
             (None, r"must be a pair \(lo, hi\)"), ([1e39, 2e39], "must be a pair of finite fp32 numbers")]


def test_interval_validation_names_the_request(monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached the device front end")

    monkeypatch.setattr(G._audio, "prepare_references", never)
    f5 = MV._Stub(lambda mel: mel)
    reqs = [("Hello.", None, None), ("Bye.", None, None)]
    for bad, msg in BAD_PAIRS:
        with pytest.raises(ValueError, match="request 1: cfg_interval " + msg):
            G.generate_many(reqs, f5tts=f5, controls=[None, dict(cfg_interval=bad)])
        with pytest.raises(ValueError, match="request 1: cfg_interval " + msg):
            G.request_controls([None, dict(cfg_interval=bad)], 2, [0, 1], D)
        if bad is not None:                                      # (None as an argument means: no window)
            with pytest.raises(ValueError, match="^cfg_interval " + msg):
                G.generate_many(reqs, f5tts=f5, cfg_interval=bad)
            with pytest.raises(ValueError, match="request 0: cfg_interval " + msg):
                G.generate("Hello.", f5tts=f5, cfg_interval=bad)
    with pytest.raises(ValueError, match=r"request 0: unknown control\(s\) \['cfg_window'\]"):
        G.generate_many(reqs, f5tts=f5, controls=[dict(cfg_window=[0.0, 1.0]), None])
    assert not f5.calls


def test_generate_many_interval_reaches_sample_per_row(monkeypatch, tmp_path):
    # request 0 has two rows, request 1 one (test_row_controls_host)
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=[dict(cfg_interval=[0.25, 0.5], cfg_strength=0.5), None])
    kw = f5.calls[0]["kw"]
    assert kw["cfg_strength"] == [0.5, 0.5, 2.0] and kw["cfg_interval"] == [(0.25, 0.5), (0.25, 0.5), G.WHOLE_INTERVAL]
    assert "audio_cfg_strength" not in kw
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=[None, dict(cfg_interval=(0.5, 1.0))], cfg_interval=(0.0, 0.25))
    assert f5.calls[0]["kw"]["cfg_interval"] == [(0.0, 0.25), (0.0, 0.25), (0.5, 1.0)]
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, cfg_interval=[0.0, 0.25], audio_cfg_strength=1.5)
    assert f5.calls[0]["kw"]["cfg_interval"] == [(0.0, 0.25)] * 3 and f5.calls[0]["kw"]["audio_cfg_strength"] == [1.5] * 3
    # a call that does not use the key passes no new keyword
    for controls in (None, [None, dict(seed=5)], [dict(cfg_strength=1.0), {}], [dict(audio_cfg_strength=1.0), None]):
        out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=controls)
        assert "cfg_interval" not in f5.calls[0]["kw"], controls


def test_requests_file_and_command_line(monkeypatch, tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello.", cfg=0.5, cfg_interval=[0.25, 0.5])) + "\n" + json.dumps(dict(text="Bye.")) + "\n"
                 + json.dumps(dict(text="Again.", cfg_interval=[0, 1], audio_cfg=0.0)) + "\n")
    assert G.read_request_controls(str(f)) == [dict(cfg_strength=0.5, cfg_interval=(0.25, 0.5)), None,
                                               dict(audio_cfg_strength=0.0, cfg_interval=(0.0, 1.0))]
    assert [r["text"] for r in G.read_requests(str(f))] == ["Hello.", "Bye.", "Again."]        # the key is accepted, not "unknown"
    for bad, msg in BAD_PAIRS:
        if isinstance(bad, list) and any(isinstance(v, float) and not np.isfinite(v) for v in bad):
            continue                                                     # (no JSON spelling)
        b = tmp_path / "bad.jsonl"
        b.write_text('{"text": "ok"}\n' + json.dumps(dict(text="x", cfg_interval=bad)) + "\n")
        with pytest.raises(ValueError, match='bad.jsonl:2: "cfg_interval" ' + msg):
            G.read_request_controls(str(b))
    assert G.parse_args(["--text", "x"]).cfg_interval is None
    assert G.parse_args(["--text", "x", "--cfg-interval", "0.25", "0.75"]).cfg_interval == [0.25, 0.75]
    with pytest.raises(SystemExit):
        G.parse_args(["--text", "x", "--cfg-interval", "0.25"])
    seen = {}

    def fake_many(reqs, **kw):
        seen.update(kw=kw)
        return [torch.zeros(4)] * len(reqs)

    def fake_generate(text, **kw):
        seen.update(kw=kw)

    monkeypatch.setattr(G, "generate_many", fake_many)
    monkeypatch.setattr(G, "generate", fake_generate)
    G.main(["--requests", str(f), "--cfg-interval", "0.1", "0.9"])
    assert seen["kw"]["cfg_interval"] == (0.1, 0.9) and seen["kw"]["controls"][0] == dict(cfg_strength=0.5, cfg_interval=(0.25, 0.5))
    G.main(["--requests", str(f)])
    assert "cfg_interval" not in seen["kw"]
    G.main(["--text", "Hi.", "--cfg-interval", "0", "0.5"])
    assert seen["kw"]["cfg_interval"] == (0.0, 0.5) and seen["kw"]["cfg_strength"] == 2.0
    G.main(["--text", "Hi."])
    assert "cfg_interval" not in seen["kw"]


def test_f5tts_sample_passes_the_interval_on(monkeypatch):
    B = 3
    cond, text = torch.zeros((B, 6, 100)), torch.zeros((B, 4), dtype=torch.int32)
    f5, eng, _ = RH._f5(monkeypatch)
    pairs = [(0.0, 0.5), (0.25, 0.75), (-1.0, 2.0)]
    f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_strength=[0.5, 0.0, 2.0], cfg_interval=pairs, seed=1)
    kw = eng.calls[0]["kw"]
    assert kw["cfg_interval"].shape == (3, 2) and kw["cfg_interval"].tolist() == [list(p) for p in pairs] and "audio_cfg_strength" not in kw
    eng.calls.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_interval=(0.25, 0.5), audio_cfg_strength=1.0, seed=1)
    kw = eng.calls[0]["kw"]
    assert kw["cfg_interval"].tolist() == [0.25, 0.5] and kw["audio_cfg_strength"] == 1.0 and kw["cfg_strength"] == 2.0
    eng.calls.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", seed=1)
    assert "cfg_interval" not in eng.calls[0]["kw"]                             # None: the call it was
    for bad in ([0.1, 0.2, 0.3], [[0.1, 0.2]] * 2):
        with pytest.raises(ValueError, match=r"cfg_interval: expected \(lo, hi\) or 3 pairs"):
            f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_interval=bad)


# ---- the reference helper tells the rule from the seeded mistakes ----------------------------------------------------------------------
def test_reference_helper_discriminates():
    """The shape, strengths and windows of the GPU tests.  Each seeded mistake moves the helper's final mel (mean |delta| over the whole
    (B, N, mel) output, kept and padded frames included) by more than 1e-2, ten times the 1e-3 gate the engine is held to, so a
    comparison against this helper cannot pass by indifference.  Measured: per_step 0.066 - 0.148 (midpoint, rk4; Euler has one stage per
    step, so there the mistake is none), half_open 0.015 - 0.051, audio_ungated 0.063 - 0.075."""
    cond, text, y0 = GW.inputs()
    dit = O.DiTOracle(TINY, synthetic_weights(TINY, seed=42))
    for method, steps in GW.SOLVER_CASES:
        times = GW.eval_times(O.time_grid(steps, -1.0), method)
        for audio, strengths in ((None, GW.CFG_ROWS), (GW.DUAL_A, GW.DUAL_C)):
            kw = dict(steps=steps, method=method, text_strength=strengths, audio=audio)
            good, _, rec = GW.window_sample(dit, cond, text, GW.DURS, y0, lo=GW.LO, hi=GW.HI, **kw)
            assert rec.shape == (len(times), GW.B)
            # the record is the rule evaluated on the solver's own evaluation times
            inside = (torch.tensor(GW.LO)[None] <= times[:, None]) & (times[:, None] <= torch.tensor(GW.HI)[None])
            assert torch.equal(rec, inside)                                        # (every row has a strength >= 1e-5)

            def dist(mistake, hi=GW.HI, base=good):
                bad = GW.window_sample(dit, cond, text, GW.DURS, y0, lo=GW.LO, hi=hi, mistake=mistake, **kw)[0]
                d = float((bad - base).abs().mean())
                print(f"helper [{method}, {'dual' if audio else 'single'}] {mistake}: mean |delta| = {d:.4f}")
                return d

            if method != "euler":
                assert dist("per_step") > 1e-2, (method, "per_step")
            # a bound placed ON an evaluation time of row 0 (an fp32 value the solver itself produced): inclusive keeps it, half-open drops it
            hi_on = [float(times[3 if method == "rk4" else 2])] + GW.HI[1:]
            on, _, rec_on = GW.window_sample(dit, cond, text, GW.DURS, y0, lo=GW.LO, hi=hi_on, **kw)
            assert bool(rec_on[3 if method == "rk4" else 2, 0])
            assert dist("half_open", hi_on, on) > 1e-2, (method, "half_open")
            if audio is not None:
                assert dist("audio_ungated") > 1e-2, (method, "audio_ungated")
    # without a window that bites it is the helper of dual guidance, bit for bit
    import dual_guidance_ref as DG
    whole, whole_t, rec = GW.window_sample(dit, cond, text, GW.DURS, y0, 3, "rk4", GW.DUAL_C, [-1.0] * 3, [2.0] * 3, audio=GW.DUAL_A)
    want, want_t = DG.dual_sample(dit, cond, text, GW.DURS, y0, 3, "rk4", GW.DUAL_A, GW.DUAL_C)
    assert bool(rec.all()) and torch.equal(whole, want) and torch.equal(whole_t, want_t)
