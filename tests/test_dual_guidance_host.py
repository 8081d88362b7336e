"""Dual guidance, host side (docs/dual_guidance.md): the workspace plans, the refusals that need no device, the new control key on its
way from generate_many / a --requests file / the command line to F5TTS.sample, Engine's control normalisation, and the reference
helper's own power to tell the strengths apart.  No GPU."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

import dual_guidance_ref as DG
import test_multivoice_host as MV
import test_row_controls_host as RH
from f5test import O, ROOT, TINY, DiTConfig, randn, rng, synthetic_weights
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import time_grid, time_grid_rows

# (config, precision, B, N, nt, steps, method) -> f5_workspace_bytes, f5_workspace_bytes_rows of the commit before dual guidance,
# taken from a build of that commit: the two-branch plans must not move; and f5_workspace_bytes_dual of the commit before the planners
# became one, taken from a build of that one: nor must the three-branch plan
PARENT_BYTES = {
    ("tiny", "bf16x3", 3, 37, 9, 5, "euler"): (5344000, 5553152, 7101696),
    ("tiny", "f16", 2, 80, 16, 3, "rk4"): (5211136, 5489920, 6790912),
    ("full", "f16", 2, 937, 120, 32, "euler"): (195817984, 230419456, 283557376),
    ("full", "mxfp8", 4, 500, 64, 4, "midpoint"): (187952128, 201346304, 258054656),
}


def _handle(lib, cfg, prec):
    h = C.c_void_p()
    cc = E.to_c_config(cfg)
    assert lib.f5_engine_create(C.byref(cc), E.PRECISIONS[prec], C.byref(h)) == 0, lib.f5_last_error()
    return h


def _bytes(lib, fn, h, B, N, nt, steps, method):
    v = C.c_size_t()
    assert getattr(lib, fn)(h, B, N, nt, steps, E.METHODS[method], C.byref(v)) == 0, lib.f5_last_error()
    return v.value


@pytest.mark.parametrize("key", list(PARENT_BYTES), ids=lambda k: "-".join(str(x) for x in k))
def test_workspace_plans(key):
    lib = E.load_library()
    cfgname, prec, B, N, nt, steps, method = key
    cfg = TINY if cfgname == "tiny" else DiTConfig()
    h = _handle(lib, cfg, prec)
    try:
        plain, rows, dual = (_bytes(lib, fn, h, B, N, nt, steps, method)
                             for fn in ("f5_workspace_bytes", "f5_workspace_bytes_rows", "f5_workspace_bytes_dual"))
        assert (plain, rows, dual) == PARENT_BYTES[key]
        # the third branch: at least x (fp32) and the fp32 hoisted projection and velocity of B N more rows, on top of the rows plan
        assert dual >= rows + B * N * (2 * cfg.dim + cfg.mel_dim) * 4
        v = C.c_size_t()
        assert lib.f5_workspace_bytes_dual(h, 0, N, nt, steps, 0, C.byref(v)) != 0 and b"bad sizes" in lib.f5_last_error()
        assert lib.f5_workspace_bytes_dual(h, B, N, nt, steps, 9, C.byref(v)) != 0 and b"Unknown method" in lib.f5_last_error()
        assert lib.f5_workspace_bytes_dual(h, B, N, nt, steps, 0, None) != 0 and b"null argument" in lib.f5_last_error()
    finally:
        lib.f5_engine_destroy(h)


def test_sample_dual_refuses_null_controls_without_a_device():
    lib = E.load_library()
    h = _handle(lib, TINY, "f16")
    try:
        a = E.F5SampleArgs()
        one = np.ones(4, np.float32)
        p = one.ctypes.data
        seen = set()
        for dc, msg in ((None, "controls is null"), (E.F5DualControls(0, p, p, 0), "controls.t_rows is null"),
                        (E.F5DualControls(p, 0, p, 0), "controls.text_cfg_rows is null"),
                        (E.F5DualControls(p, p, 0, 0), "controls.audio_cfg_rows is null"),
                        (E.F5DualControls(p, p, p, 0), "weights are not finalized")):
            rc = lib.f5_sample_dual(h, C.byref(a), None if dc is None else C.byref(dc), C.c_void_p(0))
            err = lib.f5_last_error().decode()
            assert rc != 0 and msg in err, (msg, err)
            seen.add(err)
        assert len(seen) == 5 and lib.f5_engine_graph_count(h) == 0
    finally:
        lib.f5_engine_destroy(h)


def test_dual_controls_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "f5tts_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(f5_dual_controls), offsetof(f5_dual_controls, t_rows), offsetof(f5_dual_controls, text_cfg_rows),'
                   'offsetof(f5_dual_controls, audio_cfg_rows), offsetof(f5_dual_controls, cond_keep_dev), sizeof(f5_row_controls));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", ROOT + "/include", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = E.F5DualControls
    assert got == [C.sizeof(D), D.t_rows.offset, D.text_cfg_rows.offset, D.audio_cfg_rows.offset, D.cond_keep_dev.offset,
                   C.sizeof(E.F5RowControls)]


# ---- Engine's control normalisation ---------------------------------------------------------------------------------------------------
def test_engine_row_controls_with_audio_strength():
    t = time_grid(5, -1.0)
    c = E.Controls.of(t, 2.0, 3, None)                                         # None: today's call
    assert c.steps == 5 and c.plan is False and c.struct()[1] is None
    c = E.Controls.of(t, 2.0, 3, 1.5)                                          # a scalar selects the route all the same
    assert c.steps == 5 and c.audio is not None and c.lo is None and c.plan == "dual"
    tr, cr, ar = rows = (c.t, c.cfg, c.audio)
    assert tr.shape == (3, 5) and all(np.array_equal(r, t) for r in tr) and cr.tolist() == [2.0] * 3 and ar.tolist() == [1.5] * 3
    assert all(x.dtype == np.float32 and x.flags["C_CONTIGUOUS"] for x in rows)
    grids = time_grid_rows(5, [-1.0, None, -0.5])
    c = E.Controls.of(grids, [0.5, 0.0, 2.0], 3, [3.0, 0.0, 0.0])
    assert np.array_equal(c.t, grids) and c.cfg.tolist() == [0.5, 0.0, 2.0] and c.audio.tolist() == [3.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="audio_cfg_strength: expected 3 values"):
        E.Controls.of(t, 2.0, 3, [1.0, 2.0])
    assert E.Controls.of(t, 2.0, 3).plan is False and E.Controls.of(t, [1.0, 2.0, 3.0], 3).plan is True
    # the halves of a split call get their rows
    assert E.Controls.of(t, 2.0, 3, None).slice(1, 3).audio is None and E.Controls.of(t, 2.0, 3, 1.5).slice(1, 3).audio.tolist() == [1.5, 1.5]
    assert E.Controls.of(t, 2.0, 3, [3.0, 0.0, 0.5]).slice(1, 3).audio.tolist() == [0.0, 0.5]


# ---- generate / generate_many / requests file / command line ---------------------------------------------------------------------------
def _voc(mel, lens):
    return mel[:, :-1, 0].repeat_interleave(256, dim=1)


def test_generate_many_audio_control_reaches_sample_per_row(monkeypatch, tmp_path):
    # request 0 has two rows, request 1 one (test_row_controls_host)
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=[dict(audio_cfg_strength=3.0, cfg_strength=0.5), None], cfg_strength=2.0)
    kw = f5.calls[0]["kw"]
    assert kw["cfg_strength"] == [0.5, 0.5, 2.0]
    assert kw["audio_cfg_strength"] == [3.0, 3.0, 2.0]            # a request that does not set it: its own cfg_strength (the single-knob rule)
    # a call-level value is the default of the rows that do not override it
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=[None, dict(audio_cfg_strength=0.0)], audio_cfg_strength=1.25)
    kw = f5.calls[0]["kw"]
    assert kw["audio_cfg_strength"] == [1.25, 1.25, 0.0] and kw["cfg_strength"] == 2.0
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, audio_cfg_strength=1.25)
    assert f5.calls[0]["kw"]["audio_cfg_strength"] == [1.25, 1.25, 1.25]
    # a call that does not use the key passes no new keyword
    for controls in (None, [None, dict(seed=5)], [dict(cfg_strength=1.0), {}]):
        out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, _voc, controls=controls)
        assert "audio_cfg_strength" not in f5.calls[0]["kw"], controls


def test_request_controls_with_the_audio_key():
    d = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, speed=1.0)
    assert G.request_controls(None, 2, [0, 0, 1], d) == d and set(G.CONTROL_KEYS) == set(d)
    got = G.request_controls([dict(audio_cfg_strength=3), dict(cfg_strength=0.5)], 2, [0, 0, 1], d)
    assert got == dict(d, cfg_strength=[2.0, 2.0, 0.5], audio_cfg_strength=[3.0, 3.0, 0.5])
    assert all(isinstance(v, float) for v in got["audio_cfg_strength"])
    got = G.request_controls(None, 2, [0, 0, 1], dict(d, audio_cfg_strength=1.5))
    assert got["audio_cfg_strength"] == [1.5, 1.5, 1.5]


def test_audio_control_validation_names_the_request(monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached the device front end")

    monkeypatch.setattr(G._audio, "prepare_references", never)
    f5 = MV._Stub(lambda mel: mel)
    reqs = [("Hello.", None, None), ("Bye.", None, None)]
    for bad in (float("nan"), float("inf"), "2", None, True, [1.0]):
        with pytest.raises(ValueError, match="request 1: audio_cfg_strength must be a finite number"):
            G.generate_many(reqs, f5tts=f5, controls=[None, dict(audio_cfg_strength=bad)])
    with pytest.raises(ValueError, match=r"request 0: unknown control\(s\) \['audio_cfg'\]"):
        G.generate_many(reqs, f5tts=f5, controls=[dict(audio_cfg=1.0), None])
    with pytest.raises(ValueError, match="^audio_cfg_strength must be a finite number"):
        G.generate_many(reqs, f5tts=f5, audio_cfg_strength=float("nan"))
    assert not f5.calls


def test_requests_file_and_command_line(monkeypatch, tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello.", cfg=0.5, audio_cfg=3)) + "\n" + json.dumps(dict(text="Bye.")) + "\n"
                 + json.dumps(dict(text="Again.", audio_cfg=0.0)) + "\n")
    assert G.read_request_controls(str(f)) == [dict(cfg_strength=0.5, audio_cfg_strength=3), None, dict(audio_cfg_strength=0.0)]
    assert [r["text"] for r in G.read_requests(str(f))] == ["Hello.", "Bye.", "Again."]        # the key is accepted, not "unknown"
    bad = tmp_path / "bad.jsonl"
    bad.write_text('{"text": "ok"}\n{"text": "x", "audio_cfg": "3"}\n')
    with pytest.raises(ValueError, match='bad.jsonl:2.*"audio_cfg" must be a number'):
        G.read_request_controls(str(bad))
    assert G.parse_args(["--text", "x"]).audio_cfg is None
    assert G.parse_args(["--text", "x", "--audio-cfg", "1.5", "--cfg", "0.5"]).audio_cfg == 1.5
    seen = {}

    def fake_many(reqs, **kw):
        seen.update(kw=kw)
        return [torch.zeros(4)] * len(reqs)

    def fake_generate(text, **kw):
        seen.update(kw=kw)

    monkeypatch.setattr(G, "generate_many", fake_many)
    monkeypatch.setattr(G, "generate", fake_generate)
    G.main(["--requests", str(f), "--audio-cfg", "2.5"])
    assert seen["kw"]["audio_cfg_strength"] == 2.5 and seen["kw"]["controls"][0] == dict(cfg_strength=0.5, audio_cfg_strength=3)
    G.main(["--requests", str(f)])
    assert "audio_cfg_strength" not in seen["kw"]
    G.main(["--text", "Hi.", "--audio-cfg", "0.75"])
    assert seen["kw"]["audio_cfg_strength"] == 0.75 and seen["kw"]["cfg_strength"] == 2.0
    G.main(["--text", "Hi."])
    assert "audio_cfg_strength" not in seen["kw"]


def test_f5tts_sample_passes_the_audio_strength_on(monkeypatch):
    B = 3
    cond, text = torch.zeros((B, 6, 100)), torch.zeros((B, 4), dtype=torch.int32)
    f5, eng, _ = RH._f5(monkeypatch)
    f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_strength=[0.5, 0.0, 2.0], audio_cfg_strength=[3.0, 0.0, 0.0], seed=1)
    kw = eng.calls[0]["kw"]
    assert kw["audio_cfg_strength"] == [3.0, 0.0, 0.0] and kw["cfg_strength"] == [0.5, 0.0, 2.0]
    eng.calls.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", audio_cfg_strength=1, seed=1)
    kw = eng.calls[0]["kw"]
    assert kw["audio_cfg_strength"] == 1.0 and isinstance(kw["audio_cfg_strength"], float) and kw["cfg_strength"] == 2.0
    eng.calls.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", seed=1)
    assert "audio_cfg_strength" not in eng.calls[0]["kw"]                       # None: the call it was
    with pytest.raises(ValueError, match="audio_cfg_strength: expected a scalar or 3 values"):
        f5.sample(cond, text, duration=20, steps=5, method="euler", audio_cfg_strength=[1.0, 2.0])


# ---- the reference helper tells the strengths apart ------------------------------------------------------------------------------------
def test_reference_helper_discriminates():
    """The shape of the GPU tests (TINY, B = 3, ragged 23 / 37 / 31): a == c is the two-branch rule of the oracle's own sample() within
    fp32 rounding, and the seeded mistakes -- strengths swapped, T replaced by F, by N, by (audio kept, text dropped) -- each move the result
    by more than 100 x the 1e-3 gate, so a comparison against this helper cannot pass by indifference."""
    B, N, NT, NREF, DURS = 3, 37, 10, 12, [23, 37, 31]
    r = rng(77)
    cond = randn(r, B, NREF, TINY.mel_dim)
    text = torch.from_numpy(r.integers(0, TINY.text_num_embeds, (B, NT)).astype(np.int32))
    text[1, 8:], text[2, 6:] = -1, -1
    y0 = torch.zeros((B, N, TINY.mel_dim))
    for i, d in enumerate(DURS):
        y0[i, :d] = torch.from_numpy(r.standard_normal((TINY.mel_dim, d)).astype(np.float32).T)
    dit = O.DiTOracle(TINY, synthetic_weights(TINY, seed=42))
    valid = O.lens_to_mask(torch.tensor(DURS), N)
    a, c = [3.0] * B, [0.5] * B
    kw = dict(steps=3, method="rk4")
    good, _ = DG.dual_sample(dit, cond, text, DURS, y0, audio=a, text_strength=c, **kw)

    def dist(x):
        return float((x - good).abs()[valid].mean())

    assert dist(DG.dual_sample(dit, cond, text, DURS, y0, audio=c, text_strength=a, **kw)[0]) > 0.1
    for wrong in ("F", "N", "audio_kept_text_dropped"):
        assert dist(DG.dual_sample(dit, cond, text, DURS, y0, audio=a, text_strength=c, t_is=wrong, **kw)[0]) > 0.1, wrong
    same, _ = DG.dual_sample(dit, cond, text, DURS, y0, audio=c, text_strength=c, **kw)
    want, _ = O.sample(dit, cond, text, torch.tensor(DURS), y0=y0, cfg_strength=0.5, sway_sampling_coef=-1.0, **kw)
    d = float((same - want).abs()[valid].mean())
    print(f"a == c against the oracle's two-branch rule, rk4-3: mean |delta| = {d:.2e}")
    assert d <= 1e-5
