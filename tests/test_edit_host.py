"""Speech editing on the CPU: the frame layout of an edited utterance (edit.edit_layout, pure host arithmetic), the cross-fade table,
the seconds -> frames rule, the new C-ABI symbols and every refusal f5_op_wave_patch / the keep-mask ops / f5_sample_edit make before
a launch (none of them touches a device), and the Python keyword plumbing.  tests/test_edit_gpu.py runs the kernels."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from f5test import E, ROOT, TINY
from f5_tts_mlx_amd import edit as ED

HOP = ED.HOP_LENGTH


def _check_invariants(n_src, spans, src_idx, segs, guard=2):
    """what every layout must satisfy, whatever the spans"""
    N = len(src_idx)
    assert src_idx.dtype == np.int32 and segs.dtype == np.int32 and segs.shape[1] == 3
    assert N == n_src + sum(n - (e - s) for s, e, n in spans)                  # only the spans change the length
    assert src_idx[-1] == -1                                                   # duration >= lens + 1
    kept = src_idx[src_idx >= 0]
    assert (np.diff(kept) > 0).all() and (kept < n_src).all()                  # kept frames stay in order, none twice
    for s, e, _ in spans:                                                      # nothing of a span or its guards is kept
        assert not ((kept >= max(0, s - guard)) & (kept < min(n_src, e + guard))).any()
    # the sample table is hop x the frame table, clipped to the vocoded length, contiguous from 0, empty segments dropped
    L = HOP * (N - 1)
    want = [(d0 * HOP, min(d1 * HOP, L), -1 if s0 < 0 else s0 * HOP) for d0, d1, s0 in ED.frame_segments(src_idx)]
    want = [t for t in want if t[1] > t[0]]
    assert segs.tolist() == [list(t) for t in want]
    at = 0
    for k, (d0, d1, s0) in enumerate(segs.tolist()):
        assert d0 == at and d1 > d0
        at = d1
        if s0 >= 0:                                                            # a kept segment holds its fades (256 samples each) ...
            nf = (k > 0 and segs[k - 1][2] < 0) + (k + 1 < len(segs) and segs[k + 1][2] < 0)
            assert d1 - d0 >= nf * 256 and s0 + (d1 - d0) <= n_src * HOP       # ... and reads inside the recording
        else:
            assert k == 0 or segs[k - 1][2] >= 0                               # regenerated neighbours have been merged
    assert at == L or (len(segs) == 0 and L == 0)


def test_layout_no_spans_is_the_identity_but_for_the_last_frame():
    idx, segs = ED.edit_layout(20, [])
    assert idx.tolist() == list(range(19)) + [-1]
    assert segs.tolist() == [[0, 19 * HOP, 0]]                                 # (the last frame's own samples lie past hop (N - 1))
    _check_invariants(20, [], idx, segs)
    idx, segs = ED.edit_layout(1, [])
    assert idx.tolist() == [-1] and segs.shape == (0, 3)


@pytest.mark.parametrize("spans,want", [
    # one span, same length: frames 8 .. 11 replaced, guards 6, 7 and 12, 13 regenerated in place
    ([(8, 12, 4)], list(range(6)) + [-1] * 8 + list(range(14, 29)) + [-1]),
    # growing and shrinking
    ([(8, 12, 7)], list(range(6)) + [-1] * 11 + list(range(14, 29)) + [-1]),
    ([(8, 12, 1)], list(range(6)) + [-1] * 5 + list(range(14, 29)) + [-1]),
    # two spans far apart
    ([(5, 7, 3), (18, 20, 1)], list(range(3)) + [-1] * 7 + list(range(9, 16)) + [-1] * 5 + list(range(22, 29)) + [-1]),
    # adjacent spans (the second starts where the first ends): one regenerated stretch of 2 + 3 + 2 + 2 frames
    ([(8, 10, 3), (10, 12, 2)], list(range(6)) + [-1] * 9 + list(range(14, 29)) + [-1]),
    # spans whose guards meet: frames 12, 13 (guard of the first) and 14, 15 (guard of the second) are regenerated, count kept
    ([(8, 12, 4), (16, 18, 2)], list(range(6)) + [-1] * 14 + list(range(20, 29)) + [-1]),
    # one kept frame between the guards (frame 14): too short for two fades, merged
    ([(8, 12, 4), (17, 19, 2)], list(range(6)) + [-1] * 15 + list(range(21, 29)) + [-1]),
    # two kept frames between the guards stay
    ([(8, 12, 4), (18, 20, 2)], list(range(6)) + [-1] * 8 + [14, 15] + [-1] * 6 + list(range(22, 29)) + [-1]),
    # a span touching frame 0 (left guard clipped) and one touching the end (right guard clipped)
    ([(0, 3, 5)], [-1] * 7 + list(range(5, 29)) + [-1]),
    ([(1, 3, 2)], [-1] * 5 + list(range(5, 29)) + [-1]),
    ([(27, 30, 6)], list(range(25)) + [-1] * 8),
    ([(26, 28, 2)], list(range(24)) + [-1] * 6),
    # the whole recording
    ([(0, 30, 12)], [-1] * 12),
])
def test_layout_cases(spans, want):
    idx, segs = ED.edit_layout(30, spans)
    assert idx.tolist() == want
    _check_invariants(30, spans, idx, segs)


def test_layout_guard_argument_and_random_spans():
    idx, _ = ED.edit_layout(30, [(8, 12, 4)], guard_frames=0)
    assert idx.tolist() == list(range(8)) + [-1] * 4 + list(range(12, 29)) + [-1]
    idx, _ = ED.edit_layout(30, [(8, 12, 4)], guard_frames=5)
    assert idx.tolist() == list(range(3)) + [-1] * 14 + list(range(17, 29)) + [-1]
    assert ED.GUARD_FRAMES == ED.N_FFT // (2 * HOP) == 2
    r = np.random.default_rng(3)
    for _ in range(200):
        n_src = int(r.integers(1, 60))
        cuts = np.sort(r.choice(np.arange(n_src + 1), size=min(n_src + 1, 2 * int(r.integers(0, 4))), replace=False))
        spans = [(int(cuts[i]), int(cuts[i + 1]), int(r.integers(1, 9))) for i in range(0, len(cuts) - 1, 2)]
        idx, segs = ED.edit_layout(n_src, spans)
        _check_invariants(n_src, spans, idx, segs)


@pytest.mark.parametrize("spans,word", [
    ([(10, 14, 2), (5, 7, 2)], "sorted and disjoint"), ([(5, 10, 2), (9, 12, 2)], "sorted and disjoint"),
    ([(5, 5, 2)], "empty or outside"), ([(7, 5, 2)], "empty or outside"), ([(-1, 5, 2)], "empty or outside"), ([(25, 31, 2)], "empty or outside"),
    ([(5, 8, 0)], "must be >= 1 frame"),
])
def test_layout_refuses(spans, word):
    with pytest.raises(ValueError, match=word):
        ED.edit_layout(30, spans)


def test_spans_to_frames():
    # floor(start x 93.75), ceil(end x 93.75); new length max(1, round(seconds x 93.75)), default the span's own
    assert ED.spans_to_frames([(1.20, 1.85, None)], 400) == [(112, 174, 62)]
    assert ED.spans_to_frames([(1.20, 1.85, 0.9), (2.0, 2.5)], 400) == [(112, 174, 84), (187, 235, 48)]
    assert ED.spans_to_frames([(0.0, 0.001, 0.0001)], 400) == [(0, 1, 1)]
    assert ED.spans_to_frames([(3.0, 9.0, None)], 400) == [(281, 400, 119)]                 # clipped to the recording
    with pytest.raises(ValueError, match="start < end"):
        ED.spans_to_frames([(2.0, 1.0, None)], 400)
    assert ED.FRAMES_PER_SEC == 93.75


@pytest.mark.parametrize("F", [1, 2, 7, 256, 1000])
def test_fade_table(F):
    t = ED.fade_table(F)
    i = np.arange(F, dtype=np.float64)
    want = 0.5 * (1.0 - np.cos(np.pi * (i + 0.5) / F))
    assert t.dtype == np.float32 and t.shape == (F,) and np.array_equal(t, want.astype(np.float32))     # fp64, rounded once
    assert ((t > 0) & (t < 1)).all() and (np.diff(t) > 0).all()
    # symmetric to one rounding: the fp64 values sum to 1 exactly up to fp64 rounding, each fp32 value is within half an ulp (<= 2^-25,
    # values below 1) of its own
    assert np.abs(want + want[::-1] - 1.0).max() <= 4 * np.finfo(np.float64).eps
    assert np.abs(t.astype(np.float64) + t[::-1].astype(np.float64) - 1.0).max() <= 2.0 ** -24
    assert not t.flags.writeable


def test_fade_table_empty_and_negative():
    assert ED.fade_table(0).shape == (0,)
    with pytest.raises(ValueError):
        ED.fade_table(-1)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("f5_sample_edit", "f5_op_pack_cond_text_keep", "f5_op_splice_keep", "f5_op_gather_frames", "f5_op_wave_patch")


def test_symbols_exported_and_declared():
    lib = E.load_library()
    header = open(os.path.join(ROOT, "include", "f5tts_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    assert "cfm.py:198-224" in header and "cfm.py:395-397" in header            # the reference lines the new calls generalise


def _patch(lib, **kw):
    a = dict(gen=64, src=64, segs=[[0, 600, 0], [600, 1000, -1], [1000, 2000, 300]], fade=64, out=64, B=1, L=2048, Ls=4096, S=None, F=256)
    a.update(kw)
    segs = a["segs"]
    S = a["S"] if a["S"] is not None else (len(segs) // a["B"] if segs is not None and a["B"] > 0 else 1)
    arr = None if segs is None else (C.c_int32 * (3 * len(segs)))(*[v for t in segs for v in t])
    p = C.c_void_p
    rc = lib.f5_op_wave_patch(p(a["gen"]), p(a["src"]), arr, p(a["fade"]), p(a["out"]), a["B"], a["L"], a["Ls"], S, a["F"], p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(gen=0), "null pointer"), (dict(src=0), "null pointer"), (dict(segs=None), "null pointer"), (dict(out=0), "null pointer"),
    (dict(fade=0), "null pointer"),
    (dict(B=0, S=3), "batch 0 outside"), (dict(B=-1, S=3), "batch -1 outside"),
    (dict(S=0), "S = 0 segments per row outside 1..64"), (dict(S=65), "S = 65 segments per row outside 1..64"),
    (dict(F=-1), "negative fade length F = -1"),
    (dict(segs=[[0, 600, 0], [700, 1000, -1], [1000, 2000, 300]]), "row 0 segment 1 is [700, 1000) where 600 was expected"),   # a gap
    (dict(segs=[[0, 600, 0], [500, 1000, -1], [1000, 2000, 300]]), "row 0 segment 1 is [500, 1000) where 600 was expected"),   # an overlap
    (dict(segs=[[600, 1000, -1], [0, 600, 0], [1000, 2000, 300]]), "row 0 segment 0 is [600, 1000) where 0 was expected"),     # unsorted
    (dict(segs=[[0, 600, 0], [600, 500, -1], [500, 2000, 300]]), "sorted and contiguous"),                                    # end < begin
    (dict(segs=[[0, 600, 0], [600, 1000, -1], [1000, 2049, 300]]), "ends at 2049, beyond the row length L = 2048"),
    (dict(segs=[[0, 600, 0], [600, 1000, -1], [1000, 2000, 3100]]), "reads source samples [3100, 4100), outside [0, 4096]"),
    (dict(segs=[[0, 255, 0], [255, 1000, -1], [1000, 2000, 300]]), "kept segment 0 is 255 samples long, shorter than its 1 fade(s) of F = 256"),
    (dict(segs=[[0, 600, -1], [600, 1111, 0], [1111, 2000, -1]]), "kept segment 1 is 511 samples long, shorter than its 2 fade(s) of F = 256"),
    (dict(B=2, F=0, segs=[[0, 600, 0], [600, 1000, -1], [1000, 2000, 300], [0, 10, -1], [10, 20, 0], [21, 30, -1]]), "row 1 segment 2 is [21, 30) where 20"),
])
def test_wave_patch_refusals_need_no_gpu(kw, word):
    rc, msg = _patch(E.load_library(), **kw)
    assert rc != 0 and msg.startswith("wave_patch:") and word in msg, (rc, msg)


def test_wave_patch_accepts_what_it_should_without_a_launch():
    """L = 0 is a successful call with no launch (so it runs here); the minimum lengths are accepted up to the launch, which a host
    without a device cannot make -- the GPU tests run those"""
    rc, msg = _patch(E.load_library(), L=0, segs=[[0, 0, -1]], F=0, fade=0)
    assert rc == 0, msg


def _keep_ops(lib, name, **kw):
    p = C.c_void_p
    if name == "pack_cond_text_keep":
        a = dict(cond=64, keep=64, te=64, hi=64, lo=0, B=2, N=5, mel=100, dt=256)
        a.update(kw)
        rc = lib.f5_op_pack_cond_text_keep(p(a["cond"]), p(a["keep"]), p(a["te"]), p(a["hi"]), p(a["lo"]), a["B"], a["N"], a["mel"], a["dt"], 0, p(0))
    elif name == "splice_keep":
        a = dict(cond=64, y=64, keep=64, out=64, B=2, N=5, mel=100)
        a.update(kw)
        rc = lib.f5_op_splice_keep(p(a["cond"]), p(a["y"]), p(a["keep"]), p(a["out"]), a["B"], a["N"], a["mel"], p(0))
    else:
        a = dict(src=64, idx=64, cond=64, keep=64, B=2, n_src=7, N=5, mel=100)
        a.update(kw)
        rc = lib.f5_op_gather_frames(p(a["src"]), p(a["idx"]), p(a["cond"]), p(a["keep"]), a["B"], a["n_src"], a["N"], a["mel"], p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("name,kw,word", [
    ("pack_cond_text_keep", dict(cond=0), "null pointer"), ("pack_cond_text_keep", dict(keep=0), "null pointer"),
    ("pack_cond_text_keep", dict(te=0), "null pointer"), ("pack_cond_text_keep", dict(hi=0), "null pointer"),
    ("pack_cond_text_keep", dict(B=0), "bad sizes"), ("pack_cond_text_keep", dict(mel=129), "mel_dim must be <= 128"),
    ("splice_keep", dict(cond=0), "null pointer"), ("splice_keep", dict(y=0), "null pointer"), ("splice_keep", dict(keep=0), "null pointer"),
    ("splice_keep", dict(out=0), "null pointer"), ("splice_keep", dict(N=0), "bad sizes"),
    ("gather_frames", dict(src=0), "null pointer"), ("gather_frames", dict(idx=0), "null pointer"), ("gather_frames", dict(cond=0), "null pointer"),
    ("gather_frames", dict(keep=0), "null pointer"), ("gather_frames", dict(n_src=0), "bad sizes"), ("gather_frames", dict(mel=0), "bad sizes"),
])
def test_keep_op_refusals_need_no_gpu(name, kw, word):
    rc, msg = _keep_ops(E.load_library(), name, **kw)
    assert rc != 0 and msg.startswith(name + ":") and word in msg, (rc, msg)


@pytest.fixture(scope="module")
def engine_handle():
    """an engine handle without an arena: creating one plans sizes and touches no device"""
    lib = E.load_library()
    h = C.c_void_p()
    cfg = E.to_c_config(TINY)
    assert lib.f5_engine_create(C.byref(cfg), E.PRECISIONS["f16"], C.byref(h)) == 0
    yield h
    lib.f5_engine_destroy(h)


def test_sample_edit_refuses_a_null_mask_and_what_sample_refuses(engine_handle):
    """a null mask is refused first, with its own message; with a mask the call goes through f5_sample's own checks -- a null handle /
    argument block, and on a handle without weights the message f5_sample stops at.  None of it launches anything."""
    lib = E.load_library()
    a = E.F5SampleArgs()
    a.B, a.N, a.nt, a.steps = 1, 8, 4, 2
    assert lib.f5_sample_edit(engine_handle, C.byref(a), C.c_void_p(0), C.c_void_p(0)) != 0
    assert lib.f5_last_error() == b"f5_sample_edit: cond_keep is null"
    for h, args in ((None, C.byref(a)), (engine_handle, None)):
        assert lib.f5_sample_edit(h, args, C.c_void_p(64), C.c_void_p(0)) != 0
        assert lib.f5_last_error() == b"null argument"
    assert lib.f5_sample(engine_handle, C.byref(a), C.c_void_p(0)) != 0
    want = lib.f5_last_error()
    assert lib.f5_sample_edit(engine_handle, C.byref(a), C.c_void_p(64), C.c_void_p(0)) != 0
    assert lib.f5_last_error() == want == b"weights are not finalized"
    assert lib.f5_engine_graph_count(engine_handle) == 0


def test_workspace_bytes_answers_for_both_calls(engine_handle):
    """one size serves f5_sample and f5_sample_edit (the mask's B x N bytes are planned last, by the same function that places them);
    it stays a multiple of the 256-byte slot.  The layouts of f5_sample_args and f5_config are pinned by tests/test_host.py."""
    lib = E.load_library()
    n = {}
    for B, N in ((1, 96), (2, 96), (3, 1000)):
        v = C.c_size_t()
        assert lib.f5_workspace_bytes(engine_handle, B, N, 20, 8, 0, C.byref(v)) == 0
        n[(B, N)] = v.value
        assert v.value % 256 == 0
    assert n[(2, 96)] > n[(1, 96)]


# ---- Python plumbing -------------------------------------------------------------------------------------------------------------
def test_python_keywords_and_command_line(capsys):
    from f5_tts_mlx_amd.cfm import F5TTS
    assert inspect.signature(E.Engine.sample).parameters["cond_keep"].default is None
    assert inspect.signature(E.Engine._sample_split).parameters["cond_keep"].default is None
    assert inspect.signature(F5TTS.sample).parameters["edit_mask"].default is None
    sig = inspect.signature(ED.edit_speech)
    assert list(sig.parameters)[:4] == ["source_wav", "target_text", "spans_seconds", "f5tts"]
    assert sig.parameters["patch_wave"].default is True and sig.parameters["fade_samples"].default == 256
    assert sig.parameters["resample_source"].default is False
    assert inspect.signature(ED.edit_layout).parameters["guard_frames"].default == 2
    with pytest.raises(SystemExit) as e:
        ED.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--source", "--text", "--span", "--output"):
        assert flag in out
    assert ED._parse_span("1.20-1.85") == (1.20, 1.85, None) and ED._parse_span("1.20-1.85:0.9") == (1.20, 1.85, 0.9)
    assert os.path.exists(os.path.join(ROOT, "docs", "edit.md"))


def test_check_keep_validates_on_the_host():
    """Engine._check_keep needs no engine: a mask on the wrong device / of the wrong type is refused before the library is called"""
    eng = object.__new__(E.Engine)
    cond = torch.zeros((2, 5, 100))
    assert E.Engine._check_keep(eng, None, cond) is None
    with pytest.raises(TypeError, match="bool or uint8 CUDA tensor"):
        E.Engine._check_keep(eng, torch.ones((2, 5), dtype=torch.bool), cond)
    with pytest.raises(TypeError, match="bool or uint8 CUDA tensor"):
        E.Engine._check_keep(eng, [[1] * 5] * 2, cond)
    eng.__dict__.clear()
