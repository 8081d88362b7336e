"""Sentence joins on the CPU: the new C-ABI symbol and every refusal it makes before a launch (none touches a device), the restated
validation of tests/wave_join_ref.py against the library's, audio.join_layout against a brute force that places every sample, the
edge-trim rule on synthetic energy tables, the harness of tests/test_wave_join_gpu.py itself (the emulation passes the checker, every
seeded mistake is flagged), the wiring of generate() / generate_many() with the model replaced by recording stubs, and the argument,
command-line and request-file validation."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import wave_join_ref as WJ
from f5test import E, ROOT
from f5_tts_mlx_amd import audio as A
from f5_tts_mlx_amd import generate as G

BLOCK = 240


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbol_exported_declared_and_typed():
    lib = E.load_library()
    header = open(os.path.join(ROOT, "include", "f5tts_hip.h")).read()
    assert hasattr(lib, "f5_wave_join") and "int f5_wave_join(" in header
    assert "(float)(2 i + 1) / (float)(2 F)" in header and "fmaf(w(i, F), b - a, a)" in header     # the bit-level rules are the contract
    assert lib.f5_wave_join.argtypes is not None and len(lib.f5_wave_join.argtypes) == 9


GOOD = [[0, 0, 10, 1000, 0, 100], [900, 1, 0, 500, 100, 20], [1450, 0, 0, 50, 20, 0]]      # a cross-fade of 100, then a gap of 50


def _join(lib, **kw):
    a = dict(src=64, segs=GOOD, out=64, R=2, Ls=2048, Q=1, S=None, Lout=1500)
    a.update(kw)
    segs = a["segs"]
    S = a["S"] if a["S"] is not None else (len(segs) // a["Q"] if segs is not None and a["Q"] > 0 else 1)
    arr = None if segs is None else (C.c_int32 * (6 * len(segs)))(*[v for t in segs for v in t])
    p = C.c_void_p
    rc = lib.f5_wave_join(p(a["src"]), a["R"], a["Ls"], arr, a["Q"], S, p(a["out"]), a["Lout"], p(0))
    return rc, lib.f5_last_error().decode()


def _with(k, **fields):
    """GOOD with fields of segment k replaced"""
    names = ("dst_begin", "src_row", "src_begin", "len", "fade_in", "fade_out")
    segs = [list(t) for t in GOOD]
    for name, v in fields.items():
        segs[k][names.index(name)] = v
    return segs


REFUSALS = [
    (dict(src=0), "null pointer"), (dict(segs=None), "null pointer"), (dict(out=0), "null pointer"),
    (dict(R=0), "R = 0 source rows outside 1..65535"), (dict(R=65536), "R = 65536 source rows outside 1..65535"),
    (dict(Q=0, S=3), "Q = 0 output rows outside 1..65535"), (dict(Q=65536, S=3), "Q = 65536 output rows outside 1..65535"),
    (dict(S=0), "S = 0 segments per row outside 1..64"), (dict(S=65), "S = 65 segments per row outside 1..64"),
    (dict(Ls=-1), "Ls = -1 outside 0..2^31 - 1"), (dict(Ls=2 ** 31), "Ls = 2147483648 outside 0..2^31 - 1"),
    (dict(Lout=-1), "Lout = -1 outside 0..2^31 - 1"), (dict(Lout=2 ** 31), "Lout = 2147483648 outside 0..2^31 - 1"),
    (dict(segs=_with(1, dst_begin=-1)), "negative field"), (dict(segs=_with(0, src_row=-1)), "negative field"),
    (dict(segs=_with(2, src_begin=-5)), "negative field"), (dict(segs=_with(2, len=-1)), "negative field"),
    (dict(segs=_with(0, fade_in=-1)), "negative field"), (dict(segs=_with(2, fade_out=-1)), "negative field"),
    (dict(segs=_with(1, src_row=2)), "row 0 segment 1 names source row 2, but R = 2"),
    (dict(segs=_with(0, src_begin=1049)), "row 0 segment 0 reads source samples [1049, 2049), outside [0, 2048]"),
    (dict(segs=_with(2, fade_in=30, fade_out=21)), "row 0 segment 2 is 50 samples long, shorter than its fades of 30 + 21"),
    (dict(segs=[[0, 0, 0, 2 ** 23 + 2, 0, 2 ** 22 + 1]], Ls=2 ** 24, Lout=2 ** 24), "fade longer than 2^22"),
    (dict(segs=[[0, 0, 0, 2 ** 23 + 2, 2 ** 22 + 1, 0]], Ls=2 ** 24, Lout=2 ** 24), "fade longer than 2^22"),
    (dict(segs=[GOOD[1], GOOD[0], GOOD[2]]), "row 0 segment 1 begins at 0, before segment 0 at 900: the table must be sorted by dst_begin"),
    (dict(Lout=1499), "row 0 segment 2 ends at 1500, beyond the row length Lout = 1499"),
    (dict(segs=_with(1, dst_begin=901)), "segments 0 and 1 overlap by 99 samples, which is not a pure cross-fade"),       # shorter than F
    (dict(segs=_with(1, dst_begin=899)), "segments 0 and 1 overlap by 101 samples"),                                      # longer than F
    (dict(segs=_with(1, fade_in=99)), "not a pure cross-fade (fade_out 100, fade_in 99)"),
    (dict(segs=_with(0, fade_out=99)), "not a pure cross-fade (fade_out 99, fade_in 100)"),
    (dict(segs=_with(2, dst_begin=1399, fade_in=0)), "segments 1 and 2 overlap by 1 samples"),                            # no fade at all
    # three segments on one sample: the third would have to reach back over the second's fade-in
    (dict(segs=[[0, 0, 0, 200, 0, 100], [100, 1, 0, 200, 100, 100], [150, 0, 0, 200, 100, 0]]), "segments 1 and 2 overlap by 150 samples"),
    # the second row of two is the bad one; an empty entry between two segments takes no part in the order
    (dict(Q=2, segs=GOOD + [[0, 0, 0, 100, 0, 0], [0, 0, 0, 0, 0, 0], [99, 1, 0, 10, 0, 0]]), "row 1 segments 0 and 2 overlap by 1 samples"),
]


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_wave_join_refusals_need_no_gpu(kw, word):
    rc, msg = _join(E.load_library(), **kw)
    assert rc != 0 and msg.startswith("wave_join:") and word in msg, (rc, msg)


def test_wave_join_length_zero_is_a_call_without_a_launch():
    """Lout = 0 with empty entries only succeeds without a launch (so it runs here); a segment of any length is then beyond the row"""
    lib = E.load_library()
    rc, msg = _join(lib, Lout=0, segs=[[0, 1, 7, 0, 0, 0]] * 3)
    assert rc == 0, msg
    rc, msg = _join(lib, Lout=0, Ls=0, segs=[[0, 0, 0, 0, 0, 0]])
    assert rc == 0, msg
    rc, msg = _join(lib, Lout=0)
    assert rc != 0 and "beyond the row length Lout = 0" in msg


def test_restated_validation_agrees_with_the_library():
    """every table the library refuses is refused by wave_join_ref.validate for the same reason, and GOOD by neither (the library then
    goes on to its launch, which this test must not reach: GOOD is only put to the restatement).  This is what lets the layout tests
    below put join_layout's tables to the restatement alone."""
    lib = E.load_library()
    n = 0
    for kw, _ in REFUSALS:
        if "segs" not in kw or kw["segs"] is None:
            continue
        a = dict(R=2, Ls=2048, Lout=1500)
        a.update({k: v for k, v in kw.items() if k in a})
        Q = kw.get("Q", 1)
        word = WJ.validate(np.asarray(kw["segs"]).reshape(Q, -1, 6), a["R"], a["Ls"], a["Lout"])
        rc, msg = _join(lib, **kw)
        assert word is not None and rc != 0 and word in msg, (kw, word, msg)
        n += 1
    assert n >= 15
    assert WJ.validate(np.asarray(GOOD)[None], 2, 2048, 1500) is None
    assert WJ.validate(np.asarray(GOOD)[None], 2, 2048, 1499) == "beyond the row length"


# ---- join_layout ----------------------------------------------------------------------------------------------------------------------
def _check_layout(begin, length, row_req, fade, gap):
    table, out_lens, Lout = A.join_layout(begin, length, row_req, fade=fade, gap=gap)
    Q = max(row_req) + 1
    fq = fade if isinstance(fade, list) else [fade] * Q
    gq = gap if isinstance(gap, list) else [gap] * Q
    entries, want_lens, cover = WJ.brute_layout(begin, length, row_req, fq, gq)
    assert table.dtype == np.int32 and table.shape[0] == Q and table.shape[2] == 6
    assert out_lens == want_lens and Lout == max(want_lens)
    seen = set()
    for q in range(Q):
        rows = [r for r in range(len(row_req)) if row_req[r] == q]
        for k, r in enumerate(rows):
            assert table[q, k].tolist() == [entries[r][0], r, begin[r], length[r], entries[r][1], entries[r][2]], (q, k)
            seen.add(r)
        assert not table[q, len(rows):].any()                              # shorter requests pad with empty entries
        if rows:
            assert table[q, 0, 0] == 0 and table[q, 0, 4] == 0 and table[q, len(rows) - 1, 5] == 0     # outer edges: no fade
        assert cover[q].max(initial=0) <= 2                                # no sample is reached by three sentences
        if gq[q] > 0:
            assert cover[q].max(initial=0) <= 1                            # a pause: nothing overlaps
    assert seen == set(range(len(row_req)))
    # the library's own rules, restated (test_restated_validation_agrees_with_the_library): the table is one f5_wave_join accepts
    Ls = max(b + n for b, n in zip(begin, length))
    assert WJ.validate(table, len(row_req), Ls, Lout) is None
    assert Lout == 0 or WJ.validate(table, len(row_req), Ls, Lout - 1) == "beyond the row length"
    return table, out_lens


@pytest.mark.parametrize("gap", [0, 5, 1000])
@pytest.mark.parametrize("fade", [0, 1, 7, 240, 10 ** 6])
def test_join_layout_against_the_brute_force(fade, gap):
    """hand-made: sentences of 1, 2 and 3 samples between long ones, a fade larger than every sentence, a request with one sentence,
    Q = 1; then seeded random batches"""
    _check_layout([10, 0, 3, 7, 0, 5], [1000, 1, 2, 3, 900, 50], [0] * 6, fade, gap)                       # Q = 1
    table, lens = _check_layout([10, 0, 3], [1000, 2, 600], [0, 0, 0], fade, gap)
    assert table[0, 1, 4] == min(fade, 1) and table[0, 1, 5] == min(fade, 1)                               # 2 // 2 = 1 on either side
    _check_layout([5], [77], [0], fade, gap)                                                              # one sentence: one segment
    _check_layout([5, 6, 7, 8], [300, 77, 500, 1], [0, 1, 1, 2], fade, gap)                                # single-sentence requests among others
    _check_layout([0, 0, 0], [100, 0, 100], [0, 0, 0], fade, gap)                                          # an empty sentence in the middle
    r = np.random.default_rng(1000 * gap + fade % 997)
    for _ in range(12):
        Q = int(r.integers(1, 5))
        counts = r.integers(1, 6, Q)
        row_req = [q for q in range(Q) for _ in range(counts[q])]
        length = [int(v) for v in r.choice([1, 2, 3, 5, 40, 481, 2000], len(row_req))]
        begin = [int(v) for v in r.integers(0, 300, len(row_req))]
        _check_layout(begin, length, row_req, fade, gap)


def test_join_layout_per_request_settings_and_refusals():
    table, lens = _check_layout([0, 0, 0, 0], [100, 100, 100, 100], [0, 0, 1, 1], [10, 30], [0, 7])
    assert table[0, 1].tolist() == [90, 1, 0, 100, 10, 0] and table[1, 1].tolist() == [107, 3, 0, 100, 30, 0] and lens == [190, 207]
    # fade 0, no gap: the segments abut, which is torch.cat
    table, lens = _check_layout([3, 4], [50, 60], [0, 0], 0, 0)
    assert table[0].tolist() == [[0, 0, 3, 50, 0, 0], [50, 1, 4, 60, 0, 0]] and lens == [110]
    with pytest.raises(ValueError, match="one value or one per request"):
        A.join_layout([0, 0], [5, 5], [0, 1], fade=[1, 2, 3], gap=0)
    with pytest.raises(ValueError, match="must not be negative"):
        A.join_layout([0], [5], [0], fade=-1, gap=0)
    with pytest.raises(ValueError, match="row 1"):
        A.join_layout([0, 0], [5, -5], [0, 0], fade=0, gap=0)
    with pytest.raises(ValueError, match="65 sentences exceeds the 64 segments"):
        A.join_layout([0] * 65, [5] * 65, [0] * 65, fade=0, gap=0)
    assert A.join_layout([0] * 64, [5] * 64, [0] * 64, fade=2, gap=0)[1] == [64 * 5 - 63 * 2]


# ---- the edge trim --------------------------------------------------------------------------------------------------------------------
def _table(levels_db, lens, block=BLOCK):
    """energy table of one row whose block k has the level levels_db[k] (None: exactly zero energy)"""
    e = np.zeros(len(levels_db))
    for k, db in enumerate(levels_db):
        n_k = min((k + 1) * block, lens) - k * block
        e[k] = 0.0 if db is None else n_k * 10.0 ** (db / 10.0)
    return e[None]


@pytest.mark.parametrize("levels,begin,length,keep,want", [
    # the reference (two loud blocks) ends on a block boundary; the loud block is the FIRST block after it: nothing is cut in front
    ([-5, -5, -10, -60, -60, -60], 2 * BLOCK, 4 * BLOCK, 0, (2 * BLOCK, BLOCK)),
    ([-5, -5, -10, -60, -60, -60], 2 * BLOCK, 4 * BLOCK, 1, (2 * BLOCK, 2 * BLOCK)),      # the margin does not reach into the reference
    # the loud reference is never a candidate: the window is the generated part's own loud block
    ([-5, -5, -60, -60, -10, -60], 2 * BLOCK, 4 * BLOCK, 0, (4 * BLOCK, BLOCK)),
    ([-5, -5, -60, -60, -10, -60], 2 * BLOCK, 4 * BLOCK, 1, (3 * BLOCK, 3 * BLOCK)),
    # no loud block after the reference: the whole range is kept, no exception -- also with exactly zero energy
    ([-5, -5, -60, -60, -60, -60], 2 * BLOCK, 4 * BLOCK, 2, (2 * BLOCK, 4 * BLOCK)),
    ([-5, -5, None, None], 2 * BLOCK, 2 * BLOCK, 0, (2 * BLOCK, 2 * BLOCK)),
    # the reference ends mid-block: block 1 holds reference samples and is no candidate even though it is loud; block 3 is
    ([-5, -5, -60, -10, -60, -60], BLOCK + 100, 4 * BLOCK + 40, 0, (3 * BLOCK, BLOCK)),
    # ... and with a margin that reaches back beyond the reference's end the window is clipped to begin
    ([-5, -5, -60, -10, -60, -60], BLOCK + 100, 4 * BLOCK + 40, 5, (BLOCK + 100, 4 * BLOCK + 40)),
    # ... and only block 1 loud: no candidate is, so everything is kept
    ([-5, -5, -60, -60, -60, -60], BLOCK + 100, 4 * BLOCK + 40, 0, (BLOCK + 100, 4 * BLOCK + 40)),
    # a last partial block of 17 samples that is loud: the window ends at the row's end, not at the block's
    ([-5, -60, -60, -10], BLOCK, 2 * BLOCK + 17, 0, (3 * BLOCK, 17)),
    # the threshold is exclusive, as in silence_window
    ([-5, -42, -41.9, -42], BLOCK, 3 * BLOCK, 0, (2 * BLOCK, BLOCK)),
    # a sentence shorter than the rest of the reference's last block: no candidate block at all
    ([-5, -5], BLOCK + 100, 30, 0, (BLOCK + 100, 30)),
    ([-5, -5], BLOCK, 0, 0, (BLOCK, 0)),
])
def test_sentence_windows_on_hand_made_tables(levels, begin, length, keep, want):
    got = A.sentence_windows(_table(levels, begin + length), [begin], [length], BLOCK, -42.0, keep)
    assert got == ([want[0]], [want[1]])


def test_sentence_windows_rows_are_independent():
    e = np.concatenate([_table([-5, -60, -10, -60], 4 * BLOCK), _table([-5, -60, -60, -60], 4 * BLOCK)])
    assert A.sentence_windows(e, [BLOCK, BLOCK], [3 * BLOCK, 3 * BLOCK], BLOCK, -42.0, 0) == ([2 * BLOCK, BLOCK], [BLOCK, 3 * BLOCK])
    with pytest.raises(ValueError, match="row 0: .* need 5 blocks"):
        A.sentence_windows(e, [BLOCK, BLOCK], [3 * BLOCK + 1, 3 * BLOCK], BLOCK, -42.0, 0)


# ---- the harness of the GPU tests: the emulation passes, every seeded mistake is flagged ---------------------------------------------------
def test_checker_passes_the_emulation_and_flags_the_seeded_mistakes():
    src, table, Lout, out_lens = WJ.gpu_case()
    val, kind, _, bound = WJ.reference(src, table, Lout)
    assert all((kind == k).any() for k in (WJ.ZERO, WJ.COPY, WJ.FADE, WJ.OVERLAP)) and len(set(out_lens)) == 3
    assert set(table[:, :, 4].ravel().tolist()) | set(table[:, :, 5].ravel().tolist()) == {0, 1, 7, 256}
    assert not np.isnan(val).any() and float(bound[kind == WJ.OVERLAP].max()) < 4 * WJ.U        # |a|, |b| stay below 2
    assert WJ.check(WJ.emulate(src, table, Lout), src, table, Lout) == []
    for bug in WJ.BUGS:
        found = WJ.check(WJ.emulate(src, table, Lout, bug), src, table, Lout)
        assert found, bug
        if bug == "mask_instead_of_select":
            assert any("NaN" in m for m in found)                          # 0 * NaN from the padding of src
    # an output the kernel left untouched (the NaN prefill of the GPU test) is flagged too
    assert WJ.check(np.full((3, Lout), np.nan, np.float32), src, table, Lout)


def test_weight_is_symmetric_and_exact_where_it_must_be():
    """w(F - 1 - i, F) + w(i, F) = 1 up to one rounding each; the operands of the division are exact in fp32 up to F = 2^22"""
    for F in (1, 7, 256, 1 << 22):
        i = np.unique(np.concatenate([np.arange(min(F, 300)), np.arange(max(F - 300, 0), F)]))
        w, v = WJ.weight32(i, F).astype(np.float64), WJ.weight32(F - 1 - i, F).astype(np.float64)
        assert np.abs(w + v - 1.0).max() <= 2 * WJ.U and (w > 0).all() and (w < 1).all()
        assert np.array_equal(np.float32(2 * i + 1).astype(np.int64), 2 * i + 1) and int(np.float32(2 * F)) == 2 * F


# ---- wiring: generate_many and generate with stubs -----------------------------------------------------------------------------------------
class _Stub:
    """stands for F5TTS (tests/test_multivoice_host.py): mel whose value names row and frame"""

    class transformer:
        device = torch.device("cpu")

    def __init__(self, vocoder):
        self._vocoder = vocoder
        self.calls = []

    def sample(self, cond, text, duration=None, *, lens=None, **kw):
        self.calls.append(dict(text=text, duration=duration, lens=lens, kw=kw))
        if self._vocoder is not None:                                        # generate()'s loop: a wave, reference part first
            n = cond.shape[1] + 1000 + 10 * len(self.calls)
            return (1000.0 * len(self.calls) + torch.arange(n, dtype=torch.float32))[None], None
        durs = [int(d) for d in duration.tolist()]
        self.last_durations = durs
        R, N = len(durs), max(durs)
        return (1000.0 * torch.arange(R)[:, None, None] + torch.arange(N)[None, :, None]).expand(R, N, 100).contiguous(), None


def _voc(mel, lens):
    return mel[:, :-1, 0].repeat_interleave(256, dim=1)


SAMPLES = (5 * 256 + 5, 4 * 256 + 9)
REQS = [("Hello there. How are you? Fine", None, None),
        ("no punctuation here at all just a long run of words without any end mark to speak of", None, None)]


def _counted(monkeypatch):
    """prepare_references stubbed; join_rows and the library's f5_wave_join replaced by counters -> the list of join_rows calls"""
    def prep(waves, rates, **kw):
        frames = [n // 256 for n in SAMPLES[:len(waves)]]
        mel = torch.stack([torch.full((max(frames), 100), float(i + 1)) for i in range(len(waves))])
        return A.References(mel, frames, list(SAMPLES[:len(waves)]), [0] * len(waves), np.ones(len(waves), np.float32))

    calls = []

    def join_rows(decoded, begin, length, row_req, **kw):
        calls.append(dict(decoded=decoded, begin=list(begin), length=list(length), row_req=list(row_req), kw=kw))
        Q = max(row_req) + 1
        return torch.full((Q, 7), 5.0), [3 + q for q in range(Q)]

    def never(*a):
        raise AssertionError("f5_wave_join reached")

    monkeypatch.setattr(G._audio, "prepare_references", prep)
    monkeypatch.setattr(G._audio, "join_rows", join_rows)
    monkeypatch.setattr(E.load_library(), "f5_wave_join", never)
    return calls


def test_generate_many_unset_is_the_present_path_and_set_goes_through_join_rows(monkeypatch):
    calls = _counted(monkeypatch)
    kw = dict(steps=4, method="euler", seed=3, estimate_duration=True)
    plain = G.generate_many(REQS, f5tts=_Stub(_voc), **kw)
    assert calls == []                                                       # neither join_rows nor f5_wave_join
    f5 = _Stub(_voc)
    G.generate_many(REQS, f5tts=f5, **kw)
    d = f5.last_durations
    n0, n1 = 256 * (d[0] - 1) - SAMPLES[0], 256 * (d[2] - 1) - SAMPLES[1]
    assert plain[0].shape == (2 * n0,) and plain[1].shape == (n1,) and plain[0][0] == 5.0 and plain[0][n0] == 1005.0     # torch.cat, as it was
    got = G.generate_many(REQS, f5tts=_Stub(_voc), cross_fade_ms=10, trim_sentence_db=-42, **kw)
    (c,) = calls
    assert c["begin"] == [SAMPLES[0], SAMPLES[0], SAMPLES[1]] and c["length"] == [n0, n0, n1] and c["row_req"] == [0, 0, 1]
    assert c["kw"] == dict(cross_fade_ms=10.0, pause_ms=0, trim_db=-42.0) and c["decoded"].shape == (3, 256 * (max(d) - 1))
    assert [tuple(w.shape) for w in got] == [(3,), (4,)] and got[0][0] == 5.0          # sliced to join_rows' lengths
    # per request: a list with one value per request goes through as it is
    G.generate_many(REQS, f5tts=_Stub(_voc), sentence_pause_ms=[250, None], **kw)
    assert calls[1]["kw"] == dict(cross_fade_ms=0, pause_ms=[250.0, None], trim_db=None)
    # a vocoder without `lens`: each row decoded by itself, the rows copied into one padded buffer
    G.generate_many(REQS, f5tts=_Stub(lambda mel: mel[0, :, 0].repeat_interleave(256)), cross_fade_ms=0, **kw)
    c = calls[2]
    assert c["decoded"].shape == (3, 256 * max(d)) and c["length"] == [256 * d[0] - SAMPLES[0]] * 2 + [256 * d[2] - SAMPLES[1]]
    assert d[1] < d[2] and c["decoded"][1, 256 * d[1]:].abs().max() == 0 and c["decoded"][1, 256 * d[1] - 1] == 1000.0 + d[1] - 1


def test_generate_loop_unset_is_the_present_path_and_set_goes_through_join_rows(monkeypatch):
    calls = _counted(monkeypatch)
    text = "Hello there. How are you?"
    plain = G.generate(text, f5tts=_Stub(_voc), steps=4, method="euler", seed=1)
    assert calls == []
    n_ref = plain.shape[0] - 0                                               # (the stub's waves: reference + 1010 and + 1020 samples)
    assert plain.shape == (1010 + 1020,) and plain[1010] == 2000.0 + plain[0] - 1000.0
    ref = int(plain[0] - 1000.0)                                             # the reference's samples, cut off the front of each
    got = G.generate(text, f5tts=_Stub(_voc), steps=4, method="euler", seed=1, sentence_pause_ms=100)
    (c,) = calls
    assert c["begin"] == [ref, ref] and c["length"] == [1010, 1020] and c["row_req"] == [0, 0]
    assert c["kw"] == dict(cross_fade_ms=0, pause_ms=100.0, trim_db=None)
    assert c["decoded"].shape == (2, ref + 1020) and c["decoded"][0, ref + 1010:].abs().max() == 0 and c["decoded"][1, 0] == 2000.0
    assert got.shape == (3,)
    # one sentence: only a trim sends it through the join, as a single row
    G.generate("Hello there.", f5tts=_Stub(_voc), steps=4, method="euler", seed=1, cross_fade_ms=10, sentence_pause_ms=5)
    assert len(calls) == 1
    G.generate("Hello there.", f5tts=_Stub(_voc), steps=4, method="euler", seed=1, trim_sentence_db=-42)
    assert len(calls) == 2 and calls[1]["row_req"] == [0] and calls[1]["begin"] == [ref] and calls[1]["kw"]["trim_db"] == -42.0
    assert n_ref == 2030


# ---- validation, command line, request files ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(cross_fade_ms=-1), "cross_fade_ms must not be negative"), (dict(cross_fade_ms=float("nan")), "cross_fade_ms must be a finite number"),
    (dict(cross_fade_ms="10"), "cross_fade_ms must be a finite number"), (dict(cross_fade_ms=True), "cross_fade_ms must be a finite number"),
    (dict(sentence_pause_ms=-0.5), "sentence_pause_ms must not be negative"), (dict(sentence_pause_ms=float("inf")), "sentence_pause_ms must be a finite"),
    (dict(trim_sentence_db=0), "trim_sentence_db must be below 0 dB"), (dict(trim_sentence_db=3.0), "trim_sentence_db must be below 0 dB"),
    (dict(trim_sentence_db=float("-inf")), "trim_sentence_db must be a finite number"),
])
def test_arguments_are_validated_before_anything_runs(monkeypatch, kw, word):
    def never(*a, **k):
        raise AssertionError("reached the model")

    monkeypatch.setattr(G._audio, "prepare_references", never)
    monkeypatch.setattr(G, "read_wav", never)
    with pytest.raises(ValueError, match=word):
        G.generate_many(REQS, f5tts=_Stub(_voc), **kw)
    with pytest.raises(ValueError, match=word):
        G.generate("Hello there. How are you?", f5tts=_Stub(_voc), **kw)
    (name, v), = kw.items()
    with pytest.raises(ValueError, match="request 1: " + word):
        G.generate_many(REQS, f5tts=_Stub(_voc), **{name: [None, v]})


def test_per_request_lists_and_signatures(monkeypatch):
    with pytest.raises(ValueError, match=r"cross_fade_ms: expected one value or one per request \(2\), got 3"):
        G.generate_many(REQS, f5tts=_Stub(_voc), cross_fade_ms=[1, 2, 3])
    assert G.join_options(None, None, None) is None and G.join_options([None, None], None, None, 2) is None
    assert G.join_options(0, None, None) == dict(cross_fade_ms=0, pause_ms=0, trim_db=None)          # 0 is set: the join runs, and equals cat
    for fn in (G.generate, G.generate_many):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None for k in G.JOIN_KEYS)
    p = inspect.signature(A.join_rows).parameters
    assert (p["cross_fade_ms"].default, p["pause_ms"].default, p["trim_db"].default, p["keep_ms"].default) == (0, 0, None, 50)
    assert all(p[k].kind == p[k].KEYWORD_ONLY for k in ("cross_fade_ms", "pause_ms", "trim_db", "keep_ms"))
    p = inspect.signature(A.join_layout).parameters
    assert p["fade"].kind == p["fade"].KEYWORD_ONLY and p["gap"].kind == p["gap"].KEYWORD_ONLY
    for doc in ("sentence_joins.md", "multi_voice.md"):
        assert os.path.exists(os.path.join(ROOT, "docs", doc))
    assert "cross-fades between sentences" not in open(os.path.join(ROOT, "docs", "multi_voice.md")).read()


def test_command_line_and_request_files(tmp_path, monkeypatch):
    ns = G.parse_args(["--text", "x", "--cross-fade-ms", "10", "--sentence-pause-ms", "250", "--trim-sentence-db", "-42"])
    assert (ns.cross_fade_ms, ns.sentence_pause_ms, ns.trim_sentence_db) == (10.0, 250.0, -42.0)
    ns = G.parse_args(["--text", "x"])
    assert (ns.cross_fade_ms, ns.sentence_pause_ms, ns.trim_sentence_db) == (None, None, None)
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello. You.", cross_fade_ms=12, trim_db=-40)) + "\n\n" + json.dumps(dict(text="Bye.")) + "\n"
                 + json.dumps(dict(text="So. Long.", pause_ms=300.5, cfg=1.5)) + "\n")
    assert [r["text"] for r in G.read_requests(str(f))] == ["Hello. You.", "Bye.", "So. Long."]              # the keys are known
    assert G.read_request_joins(str(f)) == dict(cross_fade_ms=[12.0, None, None], sentence_pause_ms=[None, None, 300.5],
                                                trim_sentence_db=[-40.0, None, None])
    plain = tmp_path / "plain.jsonl"
    plain.write_text(json.dumps(dict(text="Hello.")) + "\n")
    assert G.read_request_joins(str(plain)) == {}
    for line, word in ((dict(text="a", trim_db=1), r'bad.jsonl:2: "trim_db": trim_sentence_db must be below 0'),
                       (dict(text="a", pause_ms=-1), r'bad.jsonl:2: "pause_ms": sentence_pause_ms must not be negative'),
                       (dict(text="a", cross_fade_ms="x"), r'bad.jsonl:2: "cross_fade_ms": cross_fade_ms must be a finite number')):
        bad = tmp_path / "bad.jsonl"
        bad.write_text('{"text": "ok"}\n' + json.dumps(line) + "\n")
        with pytest.raises(ValueError, match=word):
            G.read_request_joins(str(bad))
    # main(): a line's own value goes before the flag's; a file without the keys and no flag hands generate_many nothing new
    seen = []
    monkeypatch.setattr(G, "generate_many", lambda reqs, **kw: seen.append(kw) or [torch.zeros(1)] * len(reqs))
    G.main(["--requests", str(f), "--cross-fade-ms", "5"])
    G.main(["--requests", str(plain)])
    assert seen[0]["cross_fade_ms"] == [12.0, 5.0, 5.0] and seen[0]["sentence_pause_ms"] == [None, None, 300.5]
    assert seen[0]["trim_sentence_db"] == [-40.0, None, None]
    assert not set(G.JOIN_KEYS) & set(seen[1])
