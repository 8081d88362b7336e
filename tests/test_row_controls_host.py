"""Per-request sampling controls, host side (docs/row_controls.md): generate_many(controls=...) validation and the mapping from
request to batch rows, read_request_controls, the per-row time grid, Engine's control normalisation and the sequence arguments of
F5TTS.sample on a stand-in engine.  No GPU."""
import json

import numpy as np
import pytest
import torch

import test_multivoice_host as MV
from f5_tts_mlx_amd import cfm as CFM
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS, per_row, time_grid, time_grid_rows


# ---- generate_many(controls=...) ---------------------------------------------------------------------------------------------------
def test_generate_many_controls_errors_before_anything_runs(monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached the device front end")

    monkeypatch.setattr(G._audio, "prepare_references", never)
    f5 = MV._Stub(lambda mel: mel)
    reqs = [("Hello.", None, None), ("Bye.", None, None)]
    with pytest.raises(ValueError, match=r"controls: expected one entry per request \(2\), got 1"):
        G.generate_many(reqs, f5tts=f5, controls=[None])
    with pytest.raises(ValueError, match=r"request 1: unknown control\(s\) \['cfg'\]"):
        G.generate_many(reqs, f5tts=f5, controls=[dict(seed=1), dict(cfg=2.0)])
    with pytest.raises(ValueError, match="request 0: controls entry must be None or a dict"):
        G.generate_many(reqs, f5tts=f5, controls=[3.0, None])
    assert not f5.calls


def test_generate_many_controls_map_requests_to_rows(monkeypatch, tmp_path):
    def voc(mel, lens):
        return mel[:, :-1, 0].repeat_interleave(256, dim=1)

    # request 0 has two rows ("Fine" carries no end mark and is dropped), request 1 one
    controls = [dict(cfg_strength=0.0, seed=11, speed=2.0), dict(sway_sampling_coef=None, cfg_strength=1.5)]
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, voc, controls=controls, cfg_strength=2.0, sway_sampling_coef=-1.0)
    (call,) = f5.calls
    kw = call["kw"]
    assert kw["cfg_strength"] == [0.0, 0.0, 1.5]
    assert kw["sway_sampling_coef"] == [-1.0, -1.0, None]             # request 0 keeps the call-level coefficient, request 1 goes linear
    assert kw["seed"] == [11, 11, 3]                                  # (_run_many calls with seed=3)
    assert kw["speed"] == [2.0, 2.0, 1.0]
    # the heuristic duration of a request uses ITS speed
    d0 = int(G.estimated_duration(np.zeros(5 * 256 + 5), G.DEFAULT_REF_TEXT, "Hello there. How are you? Fine", 2.0) * G.FRAMES_PER_SEC)
    d1 = int(G.estimated_duration(np.zeros(2 * 256), "the other voice.", "no punctuation here", 1.0) * G.FRAMES_PER_SEC)
    assert call["duration"].tolist() == [d0, d0, d1]
    # a control no request overrides stays the call-level scalar; entries that are None or empty change nothing
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, voc, controls=[None, dict(seed=5)])
    kw = f5.calls[0]["kw"]
    assert kw["seed"] == [3, 3, 5] and kw["cfg_strength"] == 2.0 and kw["sway_sampling_coef"] == -1.0 and kw["speed"] == 1.0
    out, f5, _, _ = MV._run_many(monkeypatch, tmp_path, voc, controls=[None, {}])
    kw = f5.calls[0]["kw"]
    assert kw["seed"] == 3 and kw["cfg_strength"] == 2.0 and kw["sway_sampling_coef"] == -1.0 and kw["speed"] == 1.0


def test_request_controls_function():
    d = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, speed=1.0)
    assert G.request_controls(None, 2, [0, 0, 1], d) == d
    got = G.request_controls([dict(speed=0.5), None], 2, [0, 0, 1], d)
    assert got == dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, speed=[0.5, 0.5, 1.0])
    assert set(G.CONTROL_KEYS) == set(d)


def test_read_request_controls(tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello.", cfg=1.5, sway_coef=None, seed=7, speed=1.25, output="a.wav")) + "\n\n"
                 + json.dumps(dict(text="Bye.")) + "\n" + json.dumps(dict(text="Again.", speed=2)) + "\n")
    assert G.read_request_controls(str(f)) == [dict(cfg_strength=1.5, sway_sampling_coef=None, seed=7, speed=1.25), None, dict(speed=2)]
    # read_requests hands back what it did before: the same four keys, the control keys accepted and left to read_request_controls
    assert G.read_requests(str(f)) == [dict(text="Hello.", ref_audio=None, ref_text=None, output="a.wav"),
                                       dict(text="Bye.", ref_audio=None, ref_text=None, output=None),
                                       dict(text="Again.", ref_audio=None, ref_text=None, output=None)]
    for line, what in (('{"text": "x", "seed": 1.5}', '"seed" must be an integer'), ('{"text": "x", "cfg": "2"}', '"cfg" must be a number'),
                       ('{"text": "x", "speed": null}', '"speed" must be a number'), ('{"text": ', "not a JSON object")):
        bad = tmp_path / "bad.jsonl"
        bad.write_text('{"text": "ok"}\n' + line + "\n")
        with pytest.raises(ValueError, match="bad.jsonl:2.*" + what):
            G.read_request_controls(str(bad))


def test_main_passes_request_controls_on(monkeypatch, tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello.", cfg=0.5)) + "\n" + json.dumps(dict(text="Bye.")) + "\n")
    seen = {}

    def fake_many(reqs, **kw):
        seen.update(reqs=reqs, kw=kw)
        return [torch.zeros(4), torch.zeros(4)]

    monkeypatch.setattr(G, "generate_many", fake_many)
    G.main(["--requests", str(f), "--cfg", "2.5"])
    assert seen["kw"]["controls"] == [dict(cfg_strength=0.5), None] and seen["kw"]["cfg_strength"] == 2.5
    f.write_text(json.dumps(dict(text="Hello.")) + "\n")
    G.main(["--requests", str(f)])
    assert seen["kw"]["controls"] is None                             # a file without control keys is the call it was


# ---- per-row grids and control normalisation -----------------------------------------------------------------------------------------
def test_time_grid_rows_is_time_grid_row_by_row():
    coefs = [-1.0, None, -0.5, 0.3, 0.0]
    for steps in (1, 2, 5, 32):
        g = time_grid_rows(steps, coefs)
        assert g.shape == (len(coefs), steps) and g.dtype == np.float32 and g.flags["C_CONTIGUOUS"]
        for i, c in enumerate(coefs):
            assert np.array_equal(g[i], time_grid(steps, c)), (steps, c)


def test_per_row():
    assert per_row(2.0, 3, "x") == (False, [2.0, 2.0, 2.0])
    assert per_row(None, 2, "x") == (False, [None, None])
    assert per_row([1, None, 3], 3, "x") == (True, [1, None, 3])
    assert per_row(np.array([1.0, 2.0]), 2, "x") == (True, [1.0, 2.0])
    assert per_row(torch.tensor([1, 2]), 2, "x") == (True, [1, 2])
    with pytest.raises(ValueError, match="speed: expected a scalar or 3 values"):
        per_row([1.0, 2.0], 3, "speed")


def test_engine_row_controls_normalisation():
    t = time_grid(5, -1.0)
    c = E.Controls.of(t, 2.0, 3)                                      # all-scalar: the old route
    assert c.steps == 5 and c.plan is False and c.struct()[1] is None
    c = E.Controls.of(t, [2.0, 0.0, 1.3], 3)                          # per-row cfg broadcasts the grid
    steps, tr, cr = c.steps, c.t, c.cfg
    assert steps == 5 and tr.shape == (3, 5) and tr.dtype == np.float32 and tr.flags["C_CONTIGUOUS"] and all(np.array_equal(r, t) for r in tr)
    assert cr.dtype == np.float32 and cr.tolist() == [2.0, 0.0, np.float32(1.3)]
    grids = time_grid_rows(5, [-1.0, None, -0.5])
    c = E.Controls.of(grids, 2.0, 3)                                  # per-row grid broadcasts cfg
    steps, tr, cr = c.steps, c.t, c.cfg
    assert steps == 5 and np.array_equal(tr, grids) and cr.tolist() == [2.0, 2.0, 2.0] and cr.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="expected 3 rows, got 2"):
        E.Controls.of(grids[:2], 2.0, 3)
    with pytest.raises(ValueError, match="expected 3 values"):
        E.Controls.of(t, [1.0, 2.0], 3)
    with pytest.raises(ValueError, match=r"t must be \(steps,\) or \(B, steps\)"):
        E.Controls.of(np.zeros((2, 2, 2), np.float32), 2.0, 2)
    # the halves of a split call get their rows
    half = E.Controls.of(grids, [2.0, 0.0, 1.3], 3).slice(1, 3)
    assert np.array_equal(half.t, grids[1:3]) and half.cfg.tolist() == [0.0, np.float32(1.3)]
    half = E.Controls.of(t, 2.0, 3).slice(1, 3)
    assert np.array_equal(half.t, t) and half.cfg == 2.0 and half.plan is False


FIELDS = ("t", "cfg", "audio", "lo", "hi")


def same_controls(a, b):
    """Field by field: both None, or equal fp32 C-contiguous arrays of one shape."""
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y), f
            assert x.flags["C_CONTIGUOUS"] and y.flags["C_CONTIGUOUS"], f
    assert a.plan == b.plan and a.steps == b.steps and a.guided == b.guided and a.key_bytes() == b.key_bytes()


def sliced_input(v, b0, b1, per_row_ndim):
    """Rows [b0, b1) of one sample() argument: a per-row form (ndim == per_row_ndim) is sliced, None and a shared one pass through."""
    return v if v is None or np.ndim(v) != per_row_ndim else np.asarray(v)[b0:b1]


@pytest.mark.parametrize("b0,b1", [(0, 2), (2, 3)])
def test_controls_slice_is_controls_of_the_sliced_inputs(b0, b1):
    B = 3
    ts = (time_grid(5, -1.0), time_grid_rows(5, [-1.0, None, -0.5]))
    cfgs = (2.0, [2.0, 0.0, 1.3])
    audios = (None, 1.5, [3.0, 0.0, 0.5])
    windows = (None, (0.25, 0.5), [[0.0, 0.5], [0.25, 0.75], [-1.0, 2.0]])
    for t in ts:
        for cfg in cfgs:
            for audio in audios:
                for win in windows:
                    got = E.Controls.of(t, cfg, B, audio, win).slice(b0, b1)
                    want = E.Controls.of(sliced_input(t, b0, b1, 2), sliced_input(cfg, b0, b1, 1), b1 - b0, sliced_input(audio, b0, b1, 1),
                                         sliced_input(win, b0, b1, 2))
                    same_controls(got, want)


def test_controls_struct_names_the_entry_point_of_each_plan():
    t, grids, B = time_grid(5, -1.0), time_grid_rows(5, [-1.0, None, -0.5]), 3
    mask = torch.ones((B, 7), dtype=torch.uint8)
    pairs = [[0.0, 0.5], [0.25, 0.75], [-1.0, 2.0]]
    cases = [(E.Controls.of(t, 2.0, B), False, None, None),
             (E.Controls.of(grids, 2.0, B), True, "f5_sample_rows", E.F5RowControls),
             (E.Controls.of(t, 2.0, B, [3.0, 0.0, 0.5]), "dual", "f5_sample_dual", E.F5DualControls),
             (E.Controls.of(t, [2.0, 0.0, 1.3], B, None, pairs), "window", "f5_sample_window", E.F5WindowControls),
             (E.Controls.of(grids, 2.0, B, 1.5, (0.25, 0.5)), "window_dual", "f5_sample_window", E.F5WindowControls)]
    for c, plan, name, ctype in cases:
        assert c.plan == plan and (plan is not False or c.plan is False)
        if ctype is None:                                             # the two calls without a controls struct: the mask is an argument
            assert c.struct() == ("f5_sample", None) and c.struct(mask) == ("f5_sample_edit", None)
            continue
        for m in (None, mask):
            got_name, cs = c.struct(m)
            assert got_name == name and type(cs) is ctype
            assert cs.cond_keep_dev == (None if m is None else m.data_ptr())       # (ctypes reads a void pointer of 0 back as None)
            assert cs.t_rows == c.t.ctypes.data
            assert (cs.cfg_rows if ctype is E.F5RowControls else cs.text_cfg_rows) == c.cfg.ctypes.data
            if ctype is not E.F5RowControls:
                assert cs.audio_cfg_rows == (None if c.audio is None else c.audio.ctypes.data)
            if ctype is E.F5WindowControls:
                assert cs.lo_rows == c.lo.ctypes.data and cs.hi_rows == c.hi.ctypes.data


# ---- F5TTS.sample on a stand-in engine -----------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self):
        self.calls = []

    def sample(self, text, cond, lens, durations, y0, t, **kw):
        self.calls.append(dict(text=text, cond=cond, lens=lens, durations=durations, y0=y0, t=t, kw=kw))
        return cond.clone(), y0[None].clone()


class _Transformer:
    device = torch.device("cpu")
    dim = 256

    def __init__(self):
        self.engine = _Engine()


class _Mel:
    n_mels, sample_rate, hop_length = 100, 24_000, 256


def _f5(monkeypatch, seconds=None):
    seeds_seen = []

    def fake_noise(seeds, durs, N, mel, device):
        seeds_seen.append((list(seeds), list(durs)))
        return torch.zeros((len(durs), N, mel))

    monkeypatch.setattr(CFM, "noise_normal", fake_noise)
    dp = None
    if seconds is not None:
        dp = lambda cond, text, lens=None: torch.tensor(seconds, dtype=torch.float32)      # noqa: E731
    tr = _Transformer()
    return F5TTS(transformer=tr, mel_spec_module=_Mel(), duration_predictor=dp), tr.engine, seeds_seen


def test_f5tts_sample_sequence_arguments(monkeypatch):
    B, n_ref = 3, 6
    cond = torch.zeros((B, n_ref, 100))
    text = torch.zeros((B, 4), dtype=torch.int32)
    f5, eng, seeds = _f5(monkeypatch, seconds=[0.5, 0.5, 0.5])
    f5.sample(cond, text, steps=5, method="euler", cfg_strength=[2.0, 0.0, 1.3], sway_sampling_coef=[-1.0, None, -0.5], seed=[7, 8, 9],
              speed=[1.0, 2.0, 0.5])
    (call,) = eng.calls
    assert np.array_equal(call["t"], time_grid_rows(5, [-1.0, None, -0.5]))
    assert call["kw"]["cfg_strength"] == [2.0, 0.0, 1.3]
    # speed per row on the predicted seconds: int32(0.5 s * 93 frames/s / speed) (cfm.py:253-262)
    want = [int(np.float32(0.5) * np.float32(93) / np.float32(s)) for s in (1.0, 2.0, 0.5)]
    assert f5.last_durations == want == [46, 23, 93] and call["durations"] == want
    assert seeds == [([7, 8, 9], want)]
    # one control as a sequence: the others stay what they were (a shared grid stays (steps,), a shared cfg a float)
    eng.calls.clear(), seeds.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_strength=[2.0, 0.0, 1.3], seed=4)
    assert eng.calls[0]["t"].shape == (5,) and eng.calls[0]["kw"]["cfg_strength"] == [2.0, 0.0, 1.3] and seeds == [([4, 4, 4], [20, 20, 20])]
    eng.calls.clear(), seeds.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", sway_sampling_coef=[None, None, -1.0], seed=[1, None, 3])
    assert eng.calls[0]["t"].shape == (3, 5) and eng.calls[0]["kw"]["cfg_strength"] == 2.0
    assert seeds[0][0][0] == 1 and seeds[0][0][2] == 3 and isinstance(seeds[0][0][1], int)       # None = fresh entropy for that row
    # all scalars: today's call, argument for argument
    eng.calls.clear(), seeds.clear()
    f5.sample(cond, text, duration=20, steps=5, method="euler", cfg_strength=2, sway_sampling_coef=-1.0, seed=4, speed=1.0)
    c = eng.calls[0]
    assert np.array_equal(c["t"], time_grid(5, -1.0)) and c["t"].ndim == 1 and c["kw"]["cfg_strength"] == 2.0
    assert isinstance(c["kw"]["cfg_strength"], float) and seeds == [([4, 4, 4], [20, 20, 20])]
    # a sequence of the wrong length is refused before the engine is reached
    eng.calls.clear()
    for kw in (dict(cfg_strength=[1.0, 2.0]), dict(sway_sampling_coef=[None]), dict(seed=[1, 2, 3, 4]), dict(speed=[1.0, 1.0])):
        with pytest.raises(ValueError, match="expected a scalar or 3 values"):
            f5.sample(cond, text, duration=20, steps=5, method="euler", **kw)
    assert not eng.calls


def test_dit_row_times_attribute_defaults_to_the_loop():
    from f5_tts_mlx_amd.dit import DiT
    from f5_tts_mlx_amd.weights import TINY
    assert DiT.from_config(TINY, device="cuda:0").row_times is False
    assert DiT(dim=256, row_times=True).row_times is True
