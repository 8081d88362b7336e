"""The duration predictor behind one C-ABI call (csrc/duration.hip, `f5_predict_duration`) against the Python-sequenced path it
restates (`DurationPredictor._run_ops`, native=False) and the fp64 oracle.  Every native call runs on a workspace that is 4 KiB longer
than `f5_duration_workspace_bytes` asks for; the tail carries a byte pattern that must survive the call."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from f5test import DEV, TINY, report, synthetic_weights
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.dit import DiT
from f5_tts_mlx_amd.duration import DurationPredictor, DurationTransformer, synthetic_duration_weights
from oracle import duration_oracle as DO

pytestmark = pytest.mark.gpu

MODELS = {          # dim 512: 32-channel conv-pos groups (super-group expansion in the native loader); dim 1024: 64-channel groups
    512: dict(dim=512, depth=3, heads=8),
    1024: dict(dim=1024, depth=1, heads=16),
}
CASES = {           # name: (dim, B, n_in, nt, lens)
    "b1_npad_gt_n": (512, 1, 90, 30, None),
    "b2_text_longer_ragged": (512, 2, 64, 80, [80, 53]),
    "b3_tile_edge_short_row": (512, 3, 130, 40, [130, 64, 9]),
    "dim1024": (1024, 2, 72, 20, [72, 40]),
}
PRECISIONS = ("bf16x3", "bf16", "f16")
GUARD, PATTERN = 4096, 0xA5


@functools.lru_cache(maxsize=None)
def weights(dim):
    m = MODELS[dim]
    return synthetic_duration_weights(seed=5, dim=dim, depth=m["depth"], text_num_embeds=70, text_dim=512, conv_layers=2, ff_mult=2)


@functools.lru_cache(maxsize=None)
def predictor(dim, precision):
    m = MODELS[dim]
    tr = DurationTransformer(dim=dim, depth=m["depth"], heads=m["heads"], text_dim=512, ff_mult=2, conv_layers=2, text_num_embeds=70,
                             precision=precision, device=DEV)
    dp = DurationPredictor(tr)
    dp.load_weights(weights(dim))
    return dp


def make_inputs(B, n_in, nt, seed):
    r = np.random.default_rng(seed)
    mel = torch.from_numpy((r.standard_normal((B, n_in, 100)) * 1.5 - 1.0).astype(np.float32))
    text = torch.from_numpy(r.integers(0, 70, (B, nt)).astype(np.int32))
    text[-1, nt - 5:] = -1
    return mel, text


@functools.lru_cache(maxsize=None)
def inputs(case):
    dim, B, n_in, nt, lens = CASES[case]
    mel, text = make_inputs(B, n_in, nt, seed=B + n_in)
    return mel, text, (None if lens is None else torch.tensor(lens))


_GUARDED = {}


def guarded_workspace(dp, B, n_in, nt):
    """The same workspace for the same predictor and shape (what a graph replay needs), 4 KiB longer than asked, tail patterned."""
    key = (id(dp), B, n_in, nt)
    if key not in _GUARDED:
        T = dp.transformer
        n = C.c_size_t()
        E.check(T.lib.f5_duration_workspace_bytes(T._h, B, n_in, nt, C.byref(n)))
        full = E._aligned_bytes(n.value + GUARD, T.device)
        full[n.value:] = PATTERN
        _GUARDED[key] = (full, n.value)
    return _GUARDED[key]


def run_native(dp, mel, text, lens=None, use_graph=False, **kw):
    full, n = guarded_workspace(dp, mel.shape[0], mel.shape[1], text.shape[1])
    sec, frames = dp.predict_native(mel, text, lens=lens, use_graph=use_graph, workspace=full[:n], **kw)
    torch.cuda.synchronize()
    assert bool((full[n:] == PATTERN).all()), "a launch wrote past f5_duration_workspace_bytes"
    return sec.cpu(), frames.cpu()


@functools.lru_cache(maxsize=None)
def sequenced(case, precision):
    """The Python-sequenced path (native=False), run twice: (result, reproduces itself bit for bit)."""
    mel, text, lens = inputs(case)
    dp = predictor(CASES[case][0], precision)
    a = dp(mel, text, lens=lens, native=False).cpu()
    b = dp(mel, text, lens=lens, native=False).cpu()
    return a, bool(torch.equal(a, b))


@functools.lru_cache(maxsize=None)
def native_eager(case, precision):
    mel, text, lens = inputs(case)
    return run_native(predictor(CASES[case][0], precision), mel, text, lens, use_graph=False)[0]


@functools.lru_cache(maxsize=None)
def oracle(case, emulate_bf16):
    dim, B, n_in, nt, _ = CASES[case]
    mel, text, lens = inputs(case)
    m = MODELS[dim]
    return DO.predict(weights(dim), mel, text, lens=lens, dim=dim, depth=m["depth"], heads=m["heads"], dtype=torch.float64,
                      emulate_bf16=emulate_bf16)


# the project's own bounds (test_duration_predictor_parity): relative to max(1, mean |ref|)
ORACLE_TOL = {"bf16x3": (2e-4, False), "bf16": (5e-3, True)}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_native_equals_the_python_sequenced_path(case, precision):
    """1. Same kernels, same order, same arguments: the seconds are the same BITS as `_run_ops` gives.  (Where `_run_ops` does not
    reproduce itself, both paths are held to the oracle bounds instead.)"""
    want, reproducible = sequenced(case, precision)
    got = native_eager(case, precision)
    print(f"[duration native] {case} [{precision}] sequenced={want.tolist()} native={got.tolist()} sequenced reproducible={reproducible}")
    assert got.shape == want.shape == (CASES[case][1],) and torch.isfinite(got).all() and (got > 0).all()
    if reproducible:
        assert torch.equal(got, want), (got - want).abs().max()
    else:
        assert precision in ORACLE_TOL, "the Python-sequenced path is not bit-reproducible and this precision has no oracle bound"
        tol, emu = ORACLE_TOL[precision]
        ref = oracle(case, emu)
        for name, val in (("sequenced", want), ("native", got)):
            mx, _, refm = report(f"duration {name} [{precision}] {case}", val, ref)
            assert mx <= tol * max(1.0, refm)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_native_meets_the_oracle_bounds(case, precision):
    """2. bf16x3 within 2e-4 of the fp64 oracle, bf16 within 5e-3 of the oracle that rounds its operands to bf16; f16 has no bound of its
    own in the project: it is held to the Python-sequenced path (test 1) and its distance to the fp64 oracle is printed."""
    got = native_eager(case, precision)
    if precision == "f16":
        report(f"duration native [f16] {case} vs oracle[fp64] (reported, no bound)", got, oracle(case, False))
        return
    tol, emu = ORACLE_TOL[precision]
    mx, _, refm = report(f"duration native [{precision}] {case}", got, oracle(case, emu))
    assert mx <= tol * max(1.0, refm)


def test_graph_capture_replay_and_cache_bound():
    """3. One graph per (B, n_in, nt, workspace); a replay serves new mel / text / lens of the same shape; at most 8 graphs."""
    dp = predictor(512, "bf16")
    lib, h = dp.transformer.lib, dp.transformer._h
    base = lib.f5_duration_graph_count(h)
    mel_a, text_a = make_inputs(2, 64, 80, seed=101)
    mel_b, text_b = make_inputs(2, 64, 80, seed=202)
    lens_a, lens_b = torch.tensor([80, 53]), torch.tensor([61, 80])
    a = run_native(dp, mel_a, text_a, lens_a, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 1
    b = run_native(dp, mel_b, text_b, lens_b, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 1
    b_eager = run_native(dp, mel_b, text_b, lens_b, use_graph=False)[0]
    a_eager = run_native(dp, mel_a, text_a, lens_a, use_graph=False)[0]
    assert torch.equal(b, b_eager) and torch.equal(a, a_eager) and not torch.equal(a, b)
    mel_c, text_c = make_inputs(1, 90, 30, seed=303)
    c = run_native(dp, mel_c, text_c, None, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 2
    assert torch.equal(c, run_native(dp, mel_c, text_c, None, use_graph=False)[0])
    # a fresh handle, nine distinct shapes: the least recently used graph leaves
    tr = DurationTransformer(dim=512, depth=1, heads=8, text_dim=512, ff_mult=2, conv_layers=2, text_num_embeds=70, precision="bf16", device=DEV)
    fresh = DurationPredictor(tr)
    fresh.load_weights(synthetic_duration_weights(seed=6, dim=512, depth=1, text_num_embeds=70, text_dim=512, conv_layers=2, ff_mult=2))
    assert tr.lib.f5_duration_graph_count(tr._h) == 0
    for i in range(9):
        mel, text = make_inputs(1, 8 + 3 * i, 6, seed=i)
        out = run_native(fresh, mel, text, None, use_graph=True)[0]
        assert torch.isfinite(out).all()
        assert tr.lib.f5_duration_graph_count(tr._h) == min(i + 1, 8)


@pytest.fixture(scope="module")
def tiny_f5():
    model = DiT.from_config(TINY, precision="bf16", device=DEV)
    model.load_weights(synthetic_weights(TINY, seed=2))
    return model


@pytest.mark.parametrize("speed", [1.0, 0.7, 1.3])
def test_frames_are_torchs_arithmetic(speed, tiny_f5):
    """4. frames = (int32)(seconds * 93 / speed): one fp32 product, one fp32 TRUE division, truncation -- the bits torch's elementwise
    fp32 multiply and divide give (computed on the host copy of the returned seconds: a correctly rounded division per element)."""
    dp = predictor(512, "bf16x3")
    mel, text, lens = inputs("b3_tile_edge_short_row")
    sec, frames = run_native(dp, mel, text, lens, frame_rate=93.0, speed=speed)
    assert frames.dtype == torch.int32 and frames.shape == (3,)
    want = (sec * 93 / speed).to(torch.int32)
    print(f"[duration frames] speed={speed} seconds={sec.tolist()} frames={frames.tolist()}")
    assert torch.equal(frames, want)
    # F5TTS.predict_duration: signature and result of the Python-sequenced predictor it used before
    f5 = F5TTS(transformer=tiny_f5, duration_predictor=dp)
    d = f5.predict_duration(mel, text, speed=speed)
    before = (dp(mel, text, native=False) * 93 / speed).to(torch.int32)
    assert d.dtype == torch.int32 and d.shape == (3,) and torch.equal(d.cpu(), before.cpu())


def test_native_leaves_the_process_operand_type_alone():
    """5. The handle carries its own operand type: an f16 predictor under a bf16 process-wide switch gives test 1's f16 result."""
    lib = E.load_library()
    saved = lib.f5_op_get_operand_type()
    try:
        E.check(lib.f5_op_set_operand_type(0))
        mel, text, lens = inputs("b2_text_longer_ragged")
        got = run_native(predictor(512, "f16"), mel, text, lens, use_graph=False)[0]
        assert lib.f5_op_get_operand_type() == 0
    finally:
        E.check(lib.f5_op_set_operand_type(saved))
    assert torch.equal(got, native_eager("b2_text_longer_ragged", "f16"))
    want, reproducible = sequenced("b2_text_longer_ragged", "f16")
    if reproducible:
        assert torch.equal(got, want)


@pytest.mark.parametrize("use_graph", [False, True])
def test_status_word_reports_an_fp16_clamp(use_graph):
    """6. 1.0e6 in the mel is beyond 65 504 at the first packer; the word is re-zeroed by every call, also under graph replay."""
    tr = DurationTransformer(dim=512, depth=3, heads=8, text_dim=512, ff_mult=2, conv_layers=2, text_num_embeds=70, precision="f16", device=DEV)
    dp = DurationPredictor(tr)           # its own instance: the warning is issued once per instance
    dp.load_weights(weights(512))
    mel, text, _ = inputs("b1_npad_gt_n")
    hot = mel.clone()
    hot[0, 5, 3] = 1.0e6
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ordinary = run_native(dp, mel, text, None, use_graph=use_graph)[0]
        assert dp.last_status & E.STATUS_SATURATED == 0
        for _ in range(2):
            out = run_native(dp, hot, text, None, use_graph=use_graph)[0]
            assert dp.last_status & E.STATUS_SATURATED
            assert torch.isfinite(out).all()
        again = run_native(dp, mel, text, None, use_graph=use_graph)[0]
        assert dp.last_status & E.STATUS_SATURATED == 0
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert torch.equal(again, ordinary) and torch.equal(ordinary, native_eager("b1_npad_gt_n", "f16"))


def test_sample_asks_the_native_predictor(tiny_f5):
    """7. F5TTS.sample(duration=None) -> predict_duration -> the predictor (cfm.py:307-308), frames at 93 per second (:260); with the
    instance switched to the native call the frames are the ones the Python-sequenced path gives."""
    dp = predictor(512, "bf16")
    mel, _, _ = inputs("b1_npad_gt_n")
    r = np.random.default_rng(9)
    text_small = torch.from_numpy(r.integers(0, TINY.text_num_embeds, (1, 12)).astype(np.int32))
    f5 = F5TTS(transformer=tiny_f5, duration_predictor=dp)
    saved = dp.native
    try:
        dp.native = False
        d_seq = f5.predict_duration(mel[:1], text_small, speed=1.0)
        dp.native = True
        graphs = dp.transformer.lib.f5_duration_graph_count(dp.transformer._h)
        d = f5.predict_duration(mel[:1], text_small, speed=1.0)
        assert dp.transformer.lib.f5_duration_graph_count(dp.transformer._h) == graphs + 1        # it was the native call
        assert d.dtype == torch.int32 and d.shape == (1,) and torch.equal(d.cpu(), d_seq.cpu())
        out, _ = f5.sample(mel[:1], text_small, duration=None, steps=2, method="euler", seed=0)
        assert out.shape[1] == max(int(d[0]), mel.shape[1] + 1)
    finally:
        dp.native = saved
