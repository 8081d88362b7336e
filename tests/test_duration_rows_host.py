"""Row-isolated duration prediction, host side (docs/duration_rows.md): the leak of the shared inputs on the fp64 oracle, the definition of
the mode (`duration_rows_ref.predict_isolated`) pinned against the per-row solo oracle with every rule shown to be needed, the row-length
arithmetic, the refusals of the C call and of the Python layers, and the new calls' place in the header.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import duration_rows_ref as R
from f5test import ROOT
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.duration import DurationPredictor, F5DurationArgs, F5DurationConfig, row_lengths

LEAK_MIN = 2e-2        # every row but the longest moves by at least this next to its batch-mates (measured: 2.13e-2 ... 0.42)
SAME_TOL = 1e-12       # the longest row has no padding: fp64 noise of another batch size (measured: 0 ... 1.1e-16)
SOLO_TOL = 1e-10       # the restatement against the row alone, fp64 (measured: 0 ... 2.0e-16)
RULE_MIN = 1e-6        # a rule left out is visible beyond this (measured: the worst row of every case at least 3.3e-3)


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_inputs_leak(case):
    """1. On the padded batch every row but the longest is at least 2e-2 from its solo value, relative to max(1, mean |solo|); the
    longest row is within 1e-12.  In frames (x 93): mel_longer 108, 108, 88 alone and 108, 110, 113 in the batch."""
    d = R.rel(R.padded(case), R.solo(case))
    print(f"[duration rows] {case} solo frames {R.frames(R.solo(case))[0]} in the batch {R.frames(R.padded(case))[0]} distance {d}")
    assert d[0] <= SAME_TOL, d
    assert min(d[1:]) >= LEAK_MIN, d


def isolated(case, without=""):
    dim, _, _, _, tokens = R.CASES[case]
    mel, text, lens = R.inputs(case)
    return R.predict_isolated(R.weights(dim), mel, text, lens, torch.tensor(tokens), without=without, **R.model_kw(case))


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_restatement_equals_every_row_alone(case):
    """2a. The padded-batch predictor with the four rules is the per-row solo oracle."""
    d = R.rel(isolated(case), R.solo(case))
    print(f"[duration rows] {case} predict_isolated vs solo {d}")
    assert max(d) <= SOLO_TOL, d


@pytest.mark.parametrize("rule", R.RULES)
def test_each_rule_is_needed(rule):
    """2b. With one rule switched off some row of some case leaves 1e-6 (and the longest row of every case stays)."""
    worst = 0.0
    for case in R.CASES:
        d = R.rel(isolated(case, without=rule), R.solo(case))
        print(f"[duration rows] {case} without {rule}: {d}")
        assert d[0] <= SOLO_TOL, (case, d)
        worst = max(worst, max(d[1:]))
    assert worst > RULE_MIN, worst


# ---- row-length arithmetic ---------------------------------------------------------------------------------------------------------
def test_row_lengths_of_the_cases():
    for case, (_, n_in, nt, lens, tokens) in R.CASES.items():
        _, text, _ = R.inputs(case)
        got = row_lengths(text, n_in, list(lens))
        assert got == (list(lens), list(tokens), [max(a, b) for a, b in zip(lens, tokens)]), case
        assert got[2][0] == max(n_in, nt)


def test_row_length_arithmetic():
    text = torch.tensor([[5, 6, -1, 7, -1, -1], [-1, -1, -1, -1, -1, -1], [0, 0, 0, 0, 0, 0], [3, -1, -1, -1, -1, -1]], dtype=torch.int32)
    # one past the LAST id >= 0 (a -1 inside a row is a filler position of that row); no id at all = 0; id 0 is a token
    assert row_lengths(text, 9, [4, 9, 2, 4]) == ([4, 9, 2, 4], [4, 0, 6, 1], [4, 9, 6, 4])
    assert row_lengths(text, 5) == ([5] * 4, [4, 0, 6, 1], [5, 5, 6, 5])          # lens = None: every row has n_in frames
    for lens, word in (([4, 9, 2, 0], "row 3: lens = 0"), ([4, 10, 2, 4], "row 1: lens = 10"), ([4, 9, 2, 3], "row 3: its length"),
                       ([4, 3, 2, 4], "row 1: its length")):
        with pytest.raises(ValueError, match=word):
            row_lengths(text, 9, lens)
    assert row_lengths(text, 9, [3, 9, 2, 4])[2] == [4, 9, 6, 4]                  # three frames and four tokens: a row of four
    with pytest.raises(ValueError, match="expected 4 values"):
        row_lengths(text, 9, [4, 4])


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
CFG_335M = dict(dim=512, depth=8, heads=8, dim_head=64, ff_dim=1024, mel_dim=100, text_num_embeds=2545, text_dim=512, conv_layers=2,
                conv_pos_kernel=31, conv_pos_groups=16, text_max_pos=4096)


@pytest.fixture()
def handle():
    """a predictor handle without an arena (creating one plans sizes and touches no device)"""
    lib = E.load_library()
    lib.f5_duration_destroy.restype = None
    h = C.c_void_p()
    cfg = F5DurationConfig(**CFG_335M)
    assert lib.f5_duration_create(C.byref(cfg), E.PRECISIONS["f16"], C.byref(h)) == 0, lib.f5_last_error()
    yield lib, h
    lib.f5_duration_destroy(h)


def test_workspace_bytes_rows_is_the_plain_plan_plus_the_lengths(handle):
    lib, h = handle
    for B, n_in, nt in ((1, 4, 1), (3, 130, 40), (2, 64, 80), (32, 900, 200), (65, 100, 60)):
        plain, rows = C.c_size_t(), C.c_size_t()
        assert lib.f5_duration_workspace_bytes(h, B, n_in, nt, C.byref(plain)) == 0
        assert lib.f5_duration_workspace_bytes_rows(h, B, n_in, nt, C.byref(rows)) == 0
        assert rows.value == plain.value + (B * 4 + 255) // 256 * 256, (B, n_in, nt)
    v = C.c_size_t()
    assert lib.f5_duration_workspace_bytes_rows(h, 1, 3, 2, C.byref(v)) != 0 and b"N = max(n_in, nt) >= 4" in lib.f5_last_error()
    assert lib.f5_duration_workspace_bytes_rows(h, 1, 4097, 10, C.byref(v)) != 0 and b"text_max_pos" in lib.f5_last_error()
    assert lib.f5_duration_workspace_bytes_rows(h, 2, 64, 64, None) != 0 and b"null argument" in lib.f5_last_error()


def test_the_rows_call_refuses_before_any_launch_naming_the_row(handle):
    """Every length check comes before the first thing the call would need a device for: on a handle without weights a call with good
    lengths gets as far as "weights are not finalized", every bad one is refused with the row in the message."""
    lib, h = handle
    B, n_in, nt = 3, 20, 12
    fake = 4096                                    # never dereferenced: the call is refused before it stages anything

    def call(lens, text_lens, n_in=n_in, nt=nt):
        c_lens = None if lens is None else (C.c_int32 * B)(*lens)
        a = F5DurationArgs(B, n_in, nt, fake, fake, None if c_lens is None else C.cast(c_lens, C.c_void_p), 93.0, 1.0, fake, None, fake, 1 << 40, 0)
        rc = lib.f5_predict_duration_rows(h, C.byref(a), None if text_lens is None else (C.c_int32 * B)(*text_lens), None)
        return rc, lib.f5_last_error().decode()

    good = b"duration predictor weights are not finalized".decode()
    for lens, tl in (([20, 7, 1], [12, 3, 4]), (None, [0, 12, 5]), ([4, 1, 1], [0, 4, 12])):
        rc, msg = call(lens, tl)
        assert rc != 0 and msg == good, (lens, tl, msg)
    for lens, tl, word in (([20, 7, 1], [12, 13, 4], "row 1: text_lens = 13 is outside [0, nt = 12]"),
                           ([20, 7, 1], [-1, 3, 4], "row 0: text_lens = -1 is outside [0, nt = 12]"),
                           ([20, 7, 0], [12, 3, 4], "row 2: lens = 0 is outside [1, n_in = 20]"),
                           ([21, 7, 1], [12, 3, 4], "row 0: lens = 21 is outside [1, n_in = 20]"),
                           ([20, 3, 1], [12, 2, 4], "row 1: its length max(lens, text_lens) = 3 is below 4"),
                           ([20, 7, 1], [12, 3, 0], "row 2: its length max(lens, text_lens) = 1 is below 4")):
        rc, msg = call(lens, tl)
        assert rc != 0 and word in msg and msg.startswith("duration predictor: "), (lens, tl, msg)
    rc, msg = call(None, [1, 1, 1], n_in=3, nt=4)          # lens = NULL is every lens[b] = n_in, not N: 3 frames and one token
    assert rc != 0 and "row 0: its length max(lens, text_lens) = 3 is below 4" in msg, msg
    rc, msg = call([20, 7, 1], None)
    assert rc != 0 and msg == "f5_predict_duration_rows: null argument"
    assert lib.f5_predict_duration_rows(h, None, (C.c_int32 * B)(1, 1, 1), None) != 0
    rc, msg = call([2, 2, 2], [2, 2, 2], n_in=2, nt=2)      # the shape is refused as f5_predict_duration refuses it
    assert rc != 0 and "N = max(n_in, nt) >= 4" in msg
    assert lib.f5_duration_graph_count(h) == 0


def test_header_declares_the_calls_and_keeps_the_args_struct(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "f5tts_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int f5_predict_duration_rows(f5_duration* d, const f5_duration_args* args, const int32_t* text_lens , void* stream);" in flat
    assert "int f5_duration_workspace_bytes_rows(f5_duration* d, int B, int n_in, int nt, size_t* bytes);" in flat
    assert "int f5_predict_duration(f5_duration* d, const f5_duration_args* args, void* stream);" in flat
    assert "int f5_duration_workspace_bytes(f5_duration* d, int B, int n_in, int nt, size_t* bytes);" in flat
    lib = E.load_library()
    assert hasattr(lib, "f5_predict_duration_rows") and hasattr(lib, "f5_duration_workspace_bytes_rows")
    # f5_duration_args is the struct it was: 13 fields, the layout the plain call has always read
    fields = ("B", "n_in", "nt", "mel", "text", "lens", "frame_rate", "speed", "seconds", "frames", "workspace", "workspace_bytes", "use_graph")
    assert [n for n, _ in F5DurationArgs._fields_] == list(fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "f5tts_hip.h"\n'
                   # a second declaration with another type is a compile error: the prototypes are these
                   'int f5_predict_duration_rows(f5_duration*, const f5_duration_args*, const int32_t*, void*);\n'
                   'int f5_duration_workspace_bytes_rows(f5_duration*, int, int, int, size_t*);\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(f5_duration_args), '
                   + ", ".join(f"offsetof(f5_duration_args, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(F5DurationArgs)] + [getattr(F5DurationArgs, f).offset for f in fields]


# ---- Python layers -----------------------------------------------------------------------------------------------------------------
def test_the_flag_is_an_argument_of_every_layer():
    for fn in (DurationPredictor.__call__, DurationPredictor.predict_native, F5TTS.predict_duration, F5TTS.sample):
        assert inspect.signature(fn).parameters["isolate_rows"].default is False, fn


class _Recorder:
    """stands in for a DurationPredictor: records how it was called"""

    def __init__(self):
        self.calls = []

    def __call__(self, cond, text, **kw):
        self.calls.append(kw)
        return torch.tensor([1.0, 2.0])


@pytest.mark.parametrize("bad", [1, 0, "yes", None, [True]])
def test_the_flag_must_be_a_bool(bad):
    f5 = F5TTS.__new__(F5TTS)
    f5._duration_predictor = _Recorder()
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        f5.predict_duration(torch.zeros(2, 8, 100), torch.zeros(2, 4, dtype=torch.int32), isolate_rows=bad)
    assert f5._duration_predictor.calls == []
    dp = DurationPredictor.__new__(DurationPredictor)
    dp.native = False
    dp.transformer = type("T", (), dict(precision="bf16", w=None))()
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        dp(torch.zeros(2, 8, 100), torch.zeros(2, 4, dtype=torch.int32), isolate_rows=bad)


def test_predict_duration_passes_the_flag_on_and_nothing_new_without_it():
    f5 = F5TTS.__new__(F5TTS)
    f5._duration_predictor = rec = _Recorder()
    f5._mel_spec = type("M", (), dict(sample_rate=24_000, hop_length=256))()
    cond, text = torch.zeros(2, 8, 100), torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.tensor([8, 5])
    assert f5.predict_duration(cond, text).tolist() == [93, 186]
    f5.predict_duration(cond, text, lens=lens)
    f5.predict_duration(cond, text, isolate_rows=False)
    assert rec.calls == [{}, dict(lens=lens), {}]                      # unset: the predictor gets the call it always got
    f5.predict_duration(cond, text, lens=lens, isolate_rows=True)
    f5.predict_duration(cond, text, isolate_rows=True)
    assert rec.calls[3:] == [dict(lens=lens, isolate_rows=True), dict(isolate_rows=True)]
