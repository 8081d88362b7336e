"""Many voices in one call, on the CPU: the silence window and the gain rule (audio.silence_window / reference_gain, host fp64), the row
bookkeeping of generate.generate_many with the model, the vocoder and the device front end replaced by recording stubs, the command
line, the two new C-ABI symbols and every refusal they make before a launch (none touches a device), and the harness of
tests/test_multivoice_gpu.py itself: the emulation of both kernels passes the checkers, every seeded mistake is flagged."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import convaudio_matrix as CM
import multivoice_ref as MV
from f5test import E, ROOT
from f5_tts_mlx_amd import audio as A
from f5_tts_mlx_amd import generate as G

BLOCK = 240


# ---- silence_window ------------------------------------------------------------------------------------------------------------------
def _table(levels_db, lens, block=BLOCK):
    """energy table of one row whose block k has the level levels_db[k] (None: exactly zero energy)"""
    e = np.zeros(len(levels_db))
    for k, db in enumerate(levels_db):
        n_k = min((k + 1) * block, lens) - k * block
        e[k] = 0.0 if db is None else n_k * 10.0 ** (db / 10.0)
    return e[None]


@pytest.mark.parametrize("levels,lens,keep,want", [
    # loud blocks at the very ends: nothing to cut, whatever the margin
    ([-10, -60, -60, -10], 4 * BLOCK, 0, (0, 4 * BLOCK)), ([-10, -60, -60, -10], 4 * BLOCK, 3, (0, 4 * BLOCK)),
    # a single loud block, no margin / one block of margin / a margin larger than what is there on either side
    ([-60, -60, -10, -60, -60, -60], 6 * BLOCK, 0, (2 * BLOCK, BLOCK)), ([-60, -60, -10, -60, -60, -60], 6 * BLOCK, 1, (BLOCK, 3 * BLOCK)),
    ([-60, -60, -10, -60, -60, -60], 6 * BLOCK, 2, (0, 5 * BLOCK)), ([-60, -60, -10, -60, -60, -60], 6 * BLOCK, 9, (0, 6 * BLOCK)),
    # exactly zero energy is -inf, not an error
    ([None, -10, None], 3 * BLOCK, 0, (BLOCK, BLOCK)),
    # a last partial block of 17 samples: loud -> the length ends at lens, not at the block's end; silent -> cut with the rest
    ([-60, -10, -60, -10], 3 * BLOCK + 17, 0, (BLOCK, 2 * BLOCK + 17)), ([-60, -10, -60, -60], 3 * BLOCK + 17, 1, (0, 3 * BLOCK)),
    ([-60, -10, -60, -60], 3 * BLOCK + 17, 2, (0, 3 * BLOCK + 17)),
    # the threshold is exclusive: a block AT the threshold is not loud
    ([-42, -41.9, -42], 3 * BLOCK, 0, (BLOCK, BLOCK)),
])
def test_silence_window_on_hand_made_tables(levels, lens, keep, want):
    begin, length = A.silence_window(_table(levels, lens), [lens], BLOCK, -42.0, keep)
    assert (begin, length) == ([want[0]], [want[1]])


def test_silence_window_rows_are_independent_and_silent_rows_raise():
    e = np.concatenate([_table([-60, -10, -60], 3 * BLOCK), _table([-10, -60, -60], 3 * BLOCK)])
    assert A.silence_window(e, [3 * BLOCK, 2 * BLOCK + 5], BLOCK, -42.0, 0) == ([BLOCK, 0], [BLOCK, BLOCK])
    with pytest.raises(ValueError, match="row 1"):
        A.silence_window(np.concatenate([_table([-10], BLOCK), _table([-60], BLOCK)]), [BLOCK, BLOCK], BLOCK, -42.0, 5)
    with pytest.raises(ValueError, match="row 0"):
        A.silence_window(_table([None, None], 2 * BLOCK), [2 * BLOCK], BLOCK, -42.0, 5)
    with pytest.raises(ValueError, match="row 0"):
        A.silence_window(_table([-10, -10], 2 * BLOCK), [0], BLOCK, -42.0, 5)          # a row without samples has no block


def _bundled():
    audio, sr = G.read_wav(os.path.join(os.path.dirname(G.__file__), "assets", "test_en_1_ref_short.wav"))
    assert sr == 24_000
    return np.asarray(audio, np.float64).astype(np.float32)


def _energy64(x, block=BLOCK):
    """fp64 block energies of fp32 samples"""
    nb = -(-len(x) // block)
    return np.array([[float((x[k * block:(k + 1) * block].astype(np.float64) ** 2).sum()) for k in range(nb)]])


def test_silence_window_on_the_bundled_recording():
    """-42 dB, 5 blocks of margin: the levels recomputed here in fp64 put the first loud block at 7 and the last at 499 of 533, hence
    begin = 2 x 240 and end = 505 x 240"""
    x = _bundled()
    e = _energy64(x)
    nb = e.shape[1]
    n_k = np.minimum((np.arange(nb) + 1) * BLOCK, len(x)) - np.arange(nb) * BLOCK
    with np.errstate(divide="ignore"):
        loud = np.nonzero(10 * np.log10(e[0] / n_k) > -42.0)[0]
    first, last = int(loud[0]), int(loud[-1])
    assert (first, last, len(x) // BLOCK, nb) == (7, 499, 533, 534)     # 533 whole blocks and a partial one
    begin, length = A.silence_window(e, [len(x)], BLOCK, -42.0, 5)
    assert begin == [max(0, first - 5) * BLOCK] == [2 * BLOCK]
    assert begin[0] + length[0] == min(min(nb, last + 6) * BLOCK, len(x)) == 505 * BLOCK


# ---- reference_gain ------------------------------------------------------------------------------------------------------------------
def test_reference_gain():
    r = np.random.default_rng(1)
    loud = (r.standard_normal(5 * BLOCK + 7) * 0.3).astype(np.float32)
    quiet = (loud * np.float32(0.05)).astype(np.float32)
    for x, scaled in ((loud, False), (quiet, True)):
        e = _energy64(x)
        g = A.reference_gain(e, [0], [len(x)], BLOCK)
        total = 0.0
        for v in e[0].tolist():
            total += v
        rms = np.sqrt(total / len(x))
        assert g.dtype == np.float32 and g.shape == (1,)
        assert (rms < 0.1) == scaled
        assert g[0] == (np.float32(0.1 / rms) if scaled else np.float32(1.0))
    # a window: only the kept blocks count, over the kept length
    e = _energy64(quiet)
    g = A.reference_gain(e, [BLOCK], [2 * BLOCK], BLOCK, target_rms=0.2)
    assert g[0] == np.float32(0.2 / np.sqrt((e[0, 1] + e[0, 2]) / (2 * BLOCK)))
    # exactly at the target: not below it, so 1.0
    assert A.reference_gain(np.array([[BLOCK * 0.01]]), [0], [BLOCK], BLOCK)[0] == np.float32(1.0)
    with pytest.raises(ValueError, match="row 1.*rms 0"):
        A.reference_gain(np.array([[1.0, 1.0], [0.0, 0.0]]), [0, 0], [2 * BLOCK, 2 * BLOCK], BLOCK)
    with pytest.raises(ValueError, match="whole number of blocks"):
        A.reference_gain(e, [7], [BLOCK], BLOCK)


# ---- generate_many: row bookkeeping ---------------------------------------------------------------------------------------------------
class _Stub:
    """stands for F5TTS: records the sample() call, hands back mel whose value names row and frame"""

    class transformer:
        device = torch.device("cpu")

    def __init__(self, vocoder):
        self._vocoder = vocoder
        self.calls = []

    def sample(self, cond, text, duration=None, *, lens=None, **kw):
        assert self._vocoder is None                                     # detached for the call
        self.calls.append(dict(cond=cond, text=text, duration=duration, lens=lens, kw=kw))
        durs = [int(d) for d in duration.tolist()]
        self.last_durations = durs
        R, N = len(durs), max(durs)
        mel = (1000.0 * torch.arange(R)[:, None, None] + torch.arange(N)[None, :, None]).expand(R, N, 100).contiguous()
        return mel, None


def _refs(samples):
    frames = [n // 256 for n in samples]
    mel = torch.stack([torch.full((max(frames), 100), float(i + 1)) for i in range(len(samples))])
    return A.References(mel, frames, list(samples), [0] * len(samples), np.ones(len(samples), np.float32))


def _run_many(monkeypatch, tmp_path, vocoder, reqs=None, samples=(5 * 256 + 5, 2 * 256), **kw):
    seen = {}

    def prep(waves, rates, **pkw):
        seen.update(waves=waves, rates=rates, kw=pkw)
        return _refs(samples[:len(waves)])

    monkeypatch.setattr(G._audio, "prepare_references", prep)
    wav = str(tmp_path / "ref16k.wav")
    G.write_wav(wav, np.zeros(1600, np.float32), 16_000)
    if reqs is None:
        reqs = [("Hello there. How are you? Fine", None, None), ("no punctuation here", wav, "the other voice.")]
    f5 = _Stub(vocoder)
    out = G.generate_many(reqs, steps=4, method="euler", seed=3, estimate_duration=True, f5tts=f5, **kw)
    return out, f5, seen, wav


def test_generate_many_rows_trims_and_order(monkeypatch, tmp_path):
    def voc(mel, lens):                                                  # takes lens: ONE call on the padded batch; 256 samples per frame
        voc.calls.append((tuple(mel.shape), list(lens)))
        return mel[:, :-1, 0].repeat_interleave(256, dim=1)

    voc.calls = []
    out, f5, seen, wav = _run_many(monkeypatch, tmp_path, voc, trim_silence_db=-42.0)
    # the references: one per request, the bundled one for None, with their own rates; the options go through
    assert len(seen["waves"]) == 2 and seen["rates"] == [24_000, 16_000] and seen["kw"]["trim_silence_db"] == -42.0
    assert seen["waves"][0].shape[0] == len(_bundled()) and seen["waves"][1].shape[0] == 1600
    # sentences -> rows: two sentences of request 0 ("Fine" has no end mark and is dropped by split_sentences, as in generate()), the
    # whole text of request 1, which has no sentence punctuation
    (call,) = f5.calls
    assert call["text"] == G.convert_char_to_pinyin([G.DEFAULT_REF_TEXT + " Hello there.", G.DEFAULT_REF_TEXT + " How are you?",
                                                     "the other voice. no punctuation here"])
    assert call["cond"][:, 0, 0].tolist() == [1.0, 1.0, 2.0] and call["lens"].tolist() == [5, 5, 2]
    assert call["kw"]["seed"] == 3 and call["kw"]["steps"] == 4 and call["kw"]["method"] == "euler"
    # durations: the heuristic on the request's WHOLE text and its kept samples, the same for both rows of request 0
    d0 = int(G.estimated_duration(np.zeros(5 * 256 + 5), G.DEFAULT_REF_TEXT, "Hello there. How are you? Fine", 1.0) * G.FRAMES_PER_SEC)
    d1 = int(G.estimated_duration(np.zeros(2 * 256), "the other voice.", "no punctuation here", 1.0) * G.FRAMES_PER_SEC)
    assert call["duration"].tolist() == [d0, d0, d1] and d0 != d1
    # one decode call with the frame counts; each row trimmed by ITS reference's kept samples and cut at its own frames; order kept
    assert voc.calls == [((3, max(d0, d1), 100), [d0, d0, d1])]
    assert len(out) == 2
    n0, n1 = 256 * (d0 - 1) - (5 * 256 + 5), 256 * (d1 - 1) - 2 * 256
    assert out[0].shape == (2 * n0,) and out[1].shape == (n1,)
    assert out[0][0] == 5.0 and out[0][n0 - 1] == d0 - 2 and out[0][n0] == 1005.0 and out[0][-1] == 1000.0 + d0 - 2
    assert out[1][0] == 2002.0 and out[1][-1] == 2000.0 + d1 - 2
    assert f5._vocoder is voc                                            # put back


def test_generate_many_vocoder_without_lens_is_called_per_row(monkeypatch, tmp_path):
    calls = []

    def voc(mel):
        calls.append(tuple(mel.shape))
        return mel[0, :, 0].repeat_interleave(256)

    out, f5, _, _ = _run_many(monkeypatch, tmp_path, voc)
    d = f5.last_durations
    assert calls == [(1, d[0], 100), (1, d[1], 100), (1, d[2], 100)]       # each row on its own frames
    assert out[0].shape == (2 * (256 * d[0] - (5 * 256 + 5)),) and out[1].shape == (256 * d[2] - 2 * 256,)
    assert out[0][0] == 5.0 and out[1][0] == 2002.0


def test_generate_many_errors_raise_before_anything_runs(monkeypatch, tmp_path):
    def never(*a, **k):
        raise AssertionError("reached the device front end")

    monkeypatch.setattr(G._audio, "prepare_references", never)
    f5 = _Stub(lambda mel: mel)
    with pytest.raises(ValueError, match="at least one request"):
        G.generate_many([], f5tts=f5)
    with pytest.raises(ValueError, match="request 1: no text"):
        G.generate_many([("Hello.", None, None), ("   ", None, None)], f5tts=f5)
    wav = str(tmp_path / "odd.wav")
    G.write_wav(wav, np.zeros(100, np.float32), 192_000)                # 8:1 down: beyond what a tile of the resampler can stage
    with pytest.raises(ValueError, match="request 1: reference at 192000 Hz: resample: ratio"):
        G.generate_many([("Hello.", None, None), ("Hello.", wav, "text.")], f5tts=f5)
    with pytest.raises(ValueError, match="request 0: a reference recording needs its transcript"):
        G.generate_many([("Hello.", wav, None)], f5tts=f5)
    with pytest.raises(ValueError, match="request 0: expected"):
        G.generate_many([("Hello.", None)], f5tts=f5)
    assert not f5.calls
    # a row the front end refuses is reported as its request
    def refuse(*a, **k):
        raise ValueError("row 1: no block of 240 samples is louder than -42.0 dB: nothing to keep")

    monkeypatch.setattr(G._audio, "prepare_references", refuse)
    with pytest.raises(ValueError, match="^request 1: no block"):
        G.generate_many([("Hello.", None, None), ("Hello.", None, None)], f5tts=f5, trim_silence_db=-42.0)
    with pytest.raises(RuntimeError, match="needs a model with a vocoder"):
        G.generate_many([("Hello.", None, None)], f5tts=_Stub(None))


def test_check_resample_ratio_needs_no_gpu():
    for sr in (8000, 16_000, 22_050, 24_000, 44_100, 48_000):
        A.check_resample_ratio(sr, 24_000)
    with pytest.raises(ValueError, match="resample: ratio"):
        A.check_resample_ratio(192_000, 24_000)


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps(dict(text="Hello.", ref_audio="a.wav", ref_text="a text.", output="a_out.wav")) + "\n\n"
                 + json.dumps(dict(text="Bye.")) + "\n")
    ns = G.parse_args(["--requests", str(f), "--trim-silence", "-42", "--steps", "4"])
    assert ns.requests == str(f) and ns.trim_silence == -42.0 and ns.steps == 4 and ns.text is None and ns.output is None
    assert G.read_requests(str(f)) == [dict(text="Hello.", ref_audio="a.wav", ref_text="a text.", output="a_out.wav"),
                                       dict(text="Bye.", ref_audio=None, ref_text=None, output=None)]
    for extra in (["--text", "x"], ["--output", "x.wav"]):
        with pytest.raises(SystemExit) as e:
            G.parse_args(["--requests", str(f)] + extra)
        assert e.value.code == 2 and f"--requests excludes {extra[0]}" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        G.parse_args(["--trim-silence", "-42"])
    assert e.value.code == 2
    ns = G.parse_args(["--text", "x", "--output", "y.wav"])              # the plain call is what it was
    assert ns.requests is None and ns.trim_silence is None and ns.text == "x"
    bad = tmp_path / "bad.jsonl"
    bad.write_text('{"text": "ok"}\n{"speech": "no"}\n')
    with pytest.raises(ValueError, match="bad.jsonl:2"):
        G.read_requests(str(bad))
    sig = inspect.signature(G.generate_many)
    assert sig.parameters["trim_silence_db"].default is None and sig.parameters["output_sample_rate"].default is None
    assert all(p.kind == p.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "requests")
    assert os.path.exists(os.path.join(ROOT, "docs", "multi_voice.md"))


def test_python_keywords():
    from f5_tts_mlx_amd.cfm import F5TTS
    assert inspect.signature(F5TTS.sample).parameters["wave_lens"].default is None
    assert inspect.signature(F5TTS.predict_duration).parameters["lens"].default is None
    assert inspect.signature(A.MelSpec.__call__).parameters["lens"].default is None
    assert inspect.signature(A.block_energy).parameters["block"].default == 240 == A.ENERGY_BLOCK
    p = inspect.signature(A.prepare_references).parameters
    assert p["trim_silence_db"].default is None and p["keep_ms"].default == 50 and p["target_rms"].default == 0.1
    assert "-42" in A.prepare_references.__doc__


def test_predict_duration_hands_lens_on_only_when_given():
    from f5_tts_mlx_amd.cfm import F5TTS
    seen = []

    def predictor(cond, text, **kw):
        seen.append(kw)
        return torch.tensor([1.0, 2.0])

    f5 = object.__new__(F5TTS)
    f5._duration_predictor, f5._mel_spec = predictor, A.MelSpec()
    assert f5.predict_duration(None, None).tolist() == [93, 186]
    f5.predict_duration(None, None, 1.0, lens=[3, 4])
    assert seen == [{}, {"lens": [3, 4]}]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    lib = E.load_library()
    header = open(os.path.join(ROOT, "include", "f5tts_hip.h")).read()
    for name in ("f5_wave_block_energy", "f5_mel_spectrogram_ragged"):
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    assert "shfl_xor(v, d) for d = 32, 16, 8, 4, 2, 1" in header          # the summation order is part of the contract


def _energy(lib, **kw):
    a = dict(wave=64, B=2, L=1000, lens=64, block=240, energy=64, nblk=5)
    a.update(kw)
    p = C.c_void_p
    rc = lib.f5_wave_block_energy(p(a["wave"]), a["B"], a["L"], p(a["lens"]), a["block"], p(a["energy"]), a["nblk"], p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(wave=0), "null pointer"), (dict(lens=0), "null pointer"), (dict(energy=0), "null pointer"),
    (dict(B=0), "B = 0 outside 1..65535"), (dict(B=65536), "B = 65536 outside 1..65535"),
    (dict(block=0), "block = 0 outside 1..4096"), (dict(block=4097), "block = 4097 outside 1..4096"),
    (dict(L=-1, nblk=0), "L = -1 outside 0..2^31 - 1"), (dict(L=2 ** 31, nblk=8947849), "L = 2147483648 outside 0..2^31 - 1"),
    (dict(nblk=4), "nblk = 4, but ceil(L / block) = 5"), (dict(nblk=6), "nblk = 6, but ceil(L / block) = 5"),
    (dict(L=960, nblk=5), "nblk = 5, but ceil(L / block) = 4"), (dict(L=0, nblk=1), "nblk = 1, but ceil(L / block) = 0"),
])
def test_block_energy_refusals_need_no_gpu(kw, word):
    rc, msg = _energy(E.load_library(), **kw)
    assert rc != 0 and msg.startswith("block_energy:") and word in msg, (rc, msg)


def test_block_energy_length_zero_is_a_call_without_a_launch():
    rc, msg = _energy(E.load_library(), L=0, nblk=0)
    assert rc == 0, msg


def _ragged(lib, **kw):
    a = dict(wave=64, B=2, L=1000, begin=64, lens=64, gain=0, window=64, fb=64, n_fft=1024, hop=256, n_mels=100, out=64, N=3)
    a.update(kw)
    p = C.c_void_p
    rc = lib.f5_mel_spectrogram_ragged(p(a["wave"]), a["B"], a["L"], p(a["begin"]), p(a["lens"]), p(a["gain"]), p(a["window"]), p(a["fb"]),
                                       a["n_fft"], a["hop"], a["n_mels"], p(a["out"]), a["N"], p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(wave=0), "null pointer"), (dict(begin=0), "null pointer"), (dict(lens=0), "null pointer"), (dict(window=0), "null pointer"),
    (dict(fb=0), "null pointer"), (dict(out=0), "null pointer"),
    (dict(n_fft=512), "only n_fft = 1024 is supported (got 512)"),
    (dict(hop=0), "bad hop / n_mels / batch"), (dict(n_mels=0), "bad hop / n_mels / batch"), (dict(B=0), "bad hop / n_mels / batch"),
    (dict(B=65536), "bad hop / n_mels / batch"),
    (dict(N=0), "N = 0 frames per row must be >= 1"), (dict(N=-3), "N = -3 frames per row must be >= 1"),
    (dict(L=-1), "L = -1 outside 0..2^31 - 1"), (dict(L=2 ** 31), "L = 2147483648 outside 0..2^31 - 1"),
    (dict(gain=64, N=0), "N = 0 frames"),                                  # a gain table changes nothing about the checks
])
def test_mel_ragged_refusals_need_no_gpu(kw, word):
    rc, msg = _ragged(E.load_library(), **kw)
    assert rc != 0 and msg.startswith("mel_ragged:") and word in msg, (rc, msg)


def test_python_wrappers_validate_on_the_host():
    """what the kernels cannot check without the lengths on the host is checked in Python, before the library is called"""
    w = torch.zeros((2, 1000))
    for kw, word in ((dict(lens=[1000, 1001]), r"row 1: samples \[0, 1001\)"), (dict(lens=[10, 10], begin=[0, 995]), "row 1"),
                     (dict(lens=[10, -1]), "row 1"), (dict(lens=[10]), "one entry per row")):
        with pytest.raises(ValueError, match=word):
            A.log_mel_spectrogram_ragged(w, device="cpu", **kw)
    with pytest.raises(ValueError, match=r"lens\[1\] = 1001 outside"):
        A.block_energy(w, [0, 1001], device="cpu")
    with pytest.raises(ValueError, match="at least one recording"):
        A.prepare_references([])
    with pytest.raises(ValueError, match="one int or one per recording"):
        A.prepare_references([np.zeros(10), np.zeros(10)], [24_000])


# ---- the harness of the GPU tests: the emulation passes, every seeded mistake is flagged ------------------------------------------------
@pytest.mark.parametrize("block,L", [(7, 3 * 7 + 17), (240, 241), (64, 64 * 3 + 17)])
@pytest.mark.parametrize("pad", [float("nan"), 3.0])
def test_energy_checker_passes_the_emulation_and_flags_the_seeded_mistakes(block, L, pad):
    lens = MV.energy_lens(L, block)
    assert lens[0] == L and lens[1] == 0 and 0 < lens[2] < L and lens[2] % block
    w = MV.energy_wave(np.random.default_rng(block), 3, L, lens, pad=pad)
    assert not MV.chk_block_energy(w, lens, block, MV.emu_block_energy(w, lens, block))
    for bug in MV.ENERGY_BUGS:
        assert MV.chk_block_energy(w, lens, block, MV.emu_block_energy(w, lens, block, bug)), (bug, pad)
    # the two mistakes are different ones: with finite padding the partly filled block alone is wrong in the second
    if pad == 3.0:
        a, b = (MV.emu_block_energy(w, lens, block, bug) for bug in MV.ENERGY_BUGS)
        assert not torch.equal(a, b)


# (the order of two roundings shows in some of 100 bands, not reliably in the single value per frame of n_mels = 1: gains go with 100)
@pytest.mark.parametrize("hop,n_mels,gain", [(256, 100, MV.MEL_GAINS), (100, 100, MV.MEL_GAINS), (100, 1, None), (256, 100, None)])
@pytest.mark.parametrize("pad", [float("nan"), 0.25])
def test_mel_checkers_pass_the_emulation_and_flag_the_seeded_mistakes(hop, n_mels, gain, pad):
    rows = MV.mel_rows(hop)
    w = MV.mel_wave(np.random.default_rng(hop + n_mels), rows, pad=pad)
    window, fb = CM._hann(), CM.mel_filterbank(n_mels)
    frames = [n // hop for _, n in rows]
    assert frames[3] == 1 and (frames[2] == 0 or hop != 256)             # one frame exactly; no frame at all (at the production hop)
    plain = [MV.emu_mel_plain(MV.scaled_slice(w, b, b0, n, gain), window, fb, hop) if n >= hop else None for b, (b0, n) in enumerate(rows)]
    for N in (max(frames), max(frames) + 2):
        got = MV.emu_mel_ragged(w, rows, gain, window, fb, hop, N)
        assert not MV.chk_mel_ragged(got, plain, rows, hop, N)
        assert not MV.chk_mel_interval(got, w, rows, gain, window, fb, hop)
        for bug in MV.MEL_BUGS:
            if bug == "gain_after_window" and gain is None:
                continue                                                     # no gain, no order to get wrong
            wrong = MV.emu_mel_ragged(w, rows, gain, window, fb, hop, N, bug)
            assert MV.chk_mel_ragged(wrong, plain, rows, hop, N), (bug, N, pad)
    # reading past the slice and ignoring begin are caught by the fp64 interval too (they are no rounding matter)
    for bug in ("reads_past_lens", "begin_ignored"):
        wrong = MV.emu_mel_ragged(w, rows, gain, window, fb, hop, max(frames), bug)
        assert MV.chk_mel_interval(wrong, w, rows, gain, window, fb, hop), (bug, pad)
