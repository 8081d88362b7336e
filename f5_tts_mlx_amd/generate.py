"""Text-to-speech entry point (reference: f5_tts_mlx/generate.py).

`generate(...)` keeps the reference's keyword arguments, defaults and control flow (single vs per-sentence generation,
seconds -> frames with 93.75 frames/s, RMS normalisation that only scales UP, reference trimmed by SAMPLES).  Differences:
WAV I/O uses scipy (soundfile is not installed), playback (`AudioPlayer`, PortAudio) is out of scope, and the function
returns the waveform (the reference returns None).  Without `output_path` nothing is played; the wave is just returned.

`generate_many(requests, ...)` (no reference counterpart; docs/multi_voice.md) runs many requests, each with its own reference
recording, as ONE ragged `sample()` batch.
"""
from __future__ import annotations

import argparse
import datetime
import inspect
import pkgutil
import re
import sys
from typing import Literal, Optional

import numpy as np
import torch

from . import audio as _audio
from .cfm import F5TTS
from .engine import check_isolate_rows
from .utils import convert_char_to_pinyin

SAMPLE_RATE = 24_000
HOP_LENGTH = 256
FRAMES_PER_SEC = SAMPLE_RATE / HOP_LENGTH
TARGET_RMS = 0.1
DEFAULT_REF_TEXT = "Some call me nature, others call me mother nature."   # generate.py:143


def split_sentences(text):
    """generate.py:30-36."""
    sentence_endings = re.compile(r"([.!?;:])")
    sentences = sentence_endings.split(text)
    sentences = [sentences[i] + sentences[i + 1] for i in range(0, len(sentences) - 1, 2)]
    return [sentence.strip() for sentence in sentences if sentence.strip()]


def estimated_duration(ref_audio, ref_text: str, gen_text: str, speed: float = 1.0):
    """generate.py:104-111 (quirk kept: the 'pause punctuation' pattern is a literal sequence, not a class)."""
    ref_audio_len = ref_audio.shape[0] // HOP_LENGTH
    zh_pause_punc = r"。，、；：？！"
    ref_text_len = len(ref_text.encode("utf-8")) + 3 * len(re.findall(zh_pause_punc, ref_text))
    gen_text_len = len(gen_text.encode("utf-8")) + 3 * len(re.findall(zh_pause_punc, gen_text))
    duration_in_frames = ref_audio_len + int(ref_audio_len / ref_text_len * gen_text_len / speed)
    print(f"Got estimated duration: {duration_in_frames / FRAMES_PER_SEC}")
    return duration_in_frames / FRAMES_PER_SEC


def read_wav(path_or_bytes):
    """float64 samples in [-1, 1) + sample rate (what `soundfile.read` returns for PCM16/float WAVs)."""
    import io
    import scipy.io.wavfile as wf
    src = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    sr, a = wf.read(src)
    if a.dtype == np.int16:
        a = a.astype(np.float64) / 32768.0
    elif a.dtype == np.int32:
        a = a.astype(np.float64) / 2147483648.0
    elif a.dtype == np.uint8:
        a = (a.astype(np.float64) - 128.0) / 128.0
    else:
        a = a.astype(np.float64)
    if a.ndim > 1:
        a = a[:, 0]
    return a, sr


def write_wav(path, wave: np.ndarray, sample_rate: int = SAMPLE_RATE) -> None:
    import scipy.io.wavfile as wf
    wf.write(path, sample_rate, np.asarray(wave, dtype=np.float32))


def _takes_lens(vocoder) -> bool:
    """does this vocoder's call accept `lens` (Vocos.decode does; a plain mel -> wave callable does not)?"""
    try:
        return "lens" in inspect.signature(vocoder).parameters
    except (TypeError, ValueError):
        return False


JOIN_KEYS = ("cross_fade_ms", "sentence_pause_ms", "trim_sentence_db")


def _join_value(v, name: str, what: str = ""):
    """one sentence-join setting: None, or a finite number that is not negative (the two durations) or is below 0 (the trim level);
    ValueError naming the argument (and, through `what`, the request)"""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{what}{name} must be a finite number, got {v!r}")
    if name == "trim_sentence_db":
        if not v < 0:
            raise ValueError(f"{what}{name} must be below 0 dB, got {v!r}")
    elif v < 0:
        raise ValueError(f"{what}{name} must not be negative, got {v!r}")
    return float(v)


def join_options(cross_fade_ms, sentence_pause_ms, trim_sentence_db, n_requests: Optional[int] = None):
    """The three sentence-join arguments of generate() / generate_many() (docs/sentence_joins.md) -> None when none of them is set: the
    call is then the call it was, and nothing of the join is reached.  Otherwise the keyword arguments of audio.join_rows.  With
    n_requests (generate_many) each argument may also be a list with one value per request (None = not set for that request)."""
    given = dict(zip(JOIN_KEYS, (cross_fade_ms, sentence_pause_ms, trim_sentence_db)))
    out = {}
    for name, v in given.items():
        if n_requests is not None and isinstance(v, (list, tuple)):
            if len(v) != n_requests:
                raise ValueError(f"{name}: expected one value or one per request ({n_requests}), got {len(v)}")
            out[name] = [_join_value(x, name, f"request {i}: ") for i, x in enumerate(v)]
            if all(x is None for x in out[name]):
                out[name] = None
        else:
            out[name] = _join_value(v, name)
    if all(v is None for v in out.values()):
        return None
    return dict(cross_fade_ms=out["cross_fade_ms"] or 0, pause_ms=out["sentence_pause_ms"] or 0, trim_db=out["trim_sentence_db"])


def _padded_rows(rows):
    """1-D waves of different lengths -> one zero-padded [R, longest] buffer"""
    buf = torch.zeros((len(rows), max(max(int(r.shape[0]) for r in rows), 1)), dtype=torch.float32, device=rows[0].device)
    for i, r in enumerate(rows):
        buf[i, :r.shape[0]] = r
    return buf


def generate(
    generation_text: str,
    duration: Optional[float] = None,
    estimate_duration: bool = False,
    model_name: str = "lucasnewman/f5-tts-mlx",
    ref_audio_path: Optional[str] = None,
    ref_audio_text: Optional[str] = None,
    steps: int = 8,
    method: Literal["euler", "midpoint", "rk4", "ab2", "ab3"] = "rk4",
    cfg_strength: float = 2.0,
    sway_sampling_coef: float = -1.0,
    speed: float = 1.0,  # used when duration is None as part of the duration heuristic
    seed: Optional[int] = None,
    quantization_bits: Optional[int] = None,
    output_path: Optional[str] = None,
    f5tts: Optional[F5TTS] = None,          # extension: reuse an already loaded model
    batch_sentences: bool = False,          # extension: all sentences as ONE ragged sample() batch instead of the reference's loop
    resample_ref: bool = False,             # extension: accept a reference recording at any sample rate
    output_sample_rate: Optional[int] = None,   # extension: hand back (and write) the wave at this rate instead of 24 kHz
    vocode_batched: bool = False,           # extension: with batch_sentences, ONE ragged vocoder call instead of one per sentence
    audio_cfg_strength: Optional[float] = None,   # extension (dual guidance, docs/dual_guidance.md): speaker strength; `cfg_strength` is
                                            # then the text strength.  None = the single-knob call: sample() gets no new keyword
    cfg_interval=None,                      # extension (guidance window, docs/guidance_window.md): (lo, hi) -- guidance only at function
                                            # evaluations whose time lies in [lo, hi]; None = guided throughout, no new keyword to sample()
    cross_fade_ms: Optional[float] = None,  # extension (sentence joins, docs/sentence_joins.md): linear cross-fade between sentences
    sentence_pause_ms: Optional[float] = None,   # extension: silence between sentences; the sentences then fade to and from it
    trim_sentence_db: Optional[float] = None,    # extension: cut leading / trailing near-silence below this level off every sentence
    isolate_rows: bool = False,             # extension (docs/isolate_rows.md): with batch_sentences, a sentence's frames no longer depend
                                            # on the other sentences of the batch.  False = the call as it was: no new keyword to sample()
):
    """generate.py:113-245.  `batch_sentences=True` (opt-in, no reference counterpart; SURVEY.md section 8(f)2 names it as the point of
    owning the app loop): the sentences of a multi-sentence text are sampled as one ragged batch -- one `sample()` call, one set of
    launches at M = 2 x (sum of frames) instead of one set per sentence.  It is NOT bit-compatible with the loop: in a batch the
    key-padding mask exists (cfm.py:333-336), and by default GRN (convnext_v2.py:16) and the conv position embedding (dit.py:251) see
    the padding up to the longest sentence, exactly as the reference's own `sample()` behaves for a batch.  `isolate_rows=True`
    (docs/isolate_rows.md) takes the padding out of both: every sentence then runs the arithmetic of its own solo `sample()` and
    lands within the parity gate of it, whatever shares the batch -- still not the loop's bits, since a sentence alone runs at another
    length on other kernels.  What the call equals is `sample()` of that
    batch (tests/test_model_gpu.py::test_generate_batch_sentences), each element vocoded on its own frames (the padded tail of a
    shorter sentence never reaches the vocoder).  `vocode_batched=True` (opt-in, only together with `batch_sentences`) makes that one
    `decode(mel, lens=frames)` call on the padded batch instead of one call per sentence: the vocoder's three launches that mix time
    steps stop at each sentence's own length, so the samples are those of the loop -- bit for bit while the padded batch stays on the
    GEMM kernels its sentences reach alone (up to 896 rows), beyond that to GEMM rounding order (docs/vocode_ragged.md).  A vocoder
    whose call takes no `lens` argument keeps the loop.

    Sample rates (both opt-in, no reference counterpart: the reference refuses a reference recording that is not 24 kHz and always
    writes 24 kHz).  `resample_ref=True` converts a reference recording of another rate to 24 kHz on the model's device before the
    RMS step; `output_sample_rate` converts the final wave -- after the reference trim and the concatenation of all sentences -- once,
    and that wave is what is returned and written.  The converter (audio.resample) is a Hann-windowed sinc polyphase filter with
    6 zero crossings and a roll-off of 0.99: the design of torchaudio's default `resample`, which the PyTorch F5-TTS front end
    applies to its reference audio.  It is a short filter and its stop band is modest: docs/resample.md records the figures (a
    14 kHz tone at 48 kHz comes through the conversion to 24 kHz about 22 dB down, a 10 kHz tone at 24 kHz -> 16 kHz about 45 dB).

    Sentence joins (opt-in, docs/sentence_joins.md): `cross_fade_ms`, `sentence_pause_ms` and `trim_sentence_db` (all None: the code
    above, unchanged, and nothing of the join is called).  With any of them set the decoded sentences, reference part included, go as
    rows of one padded buffer to audio.join_rows: an optional edge trim per sentence (-42 is the customary level), then one
    f5_wave_join launch that lays them out with linear cross-fades (no pause) or fades to and from a pause.  A single-sentence text
    goes through it only for the trim.  ValueError before any launch for a negative or non-finite value and a trim level not below 0."""
    join = None                                                       # all three unset: nothing of the join is called
    if cross_fade_ms is not None or sentence_pause_ms is not None or trim_sentence_db is not None:
        join = join_options(cross_fade_ms, sentence_pause_ms, trim_sentence_db)
    window_kw = {} if cfg_interval is None else dict(cfg_interval=_interval(cfg_interval, "request 0: cfg_interval"))
    if isolate_rows is not False:
        check_isolate_rows(isolate_rows, "")                          # (a bool; the model's precision is looked at once there is a model)
    if output_sample_rate is not None:
        output_sample_rate = _audio._rate(output_sample_rate, "output_sample_rate")
    if f5tts is None:
        f5tts = F5TTS.from_pretrained(model_name, quantization_bits=quantization_bits)
    iso_kw = {}
    if isolate_rows is not False:
        iso_kw["isolate_rows"] = check_isolate_rows(isolate_rows, f5tts.transformer.engine.precision)
    if getattr(f5tts, "_vocoder", None) is None:
        # sample() would hand back mel frames; trimming them by audio samples and writing a WAV would produce garbage
        raise RuntimeError("generate() needs a model with a vocoder (F5TTS(..., vocoder=...) / from_pretrained with Vocos)")

    if ref_audio_path is None:
        data = pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav")   # generate.py:133-143
        audio, sr = read_wav(data)
        ref_audio_text = DEFAULT_REF_TEXT
    else:
        audio, sr = read_wav(ref_audio_path)
        if sr != SAMPLE_RATE and not resample_ref:
            raise ValueError("Reference audio must have a sample rate of 24kHz")

    audio = torch.from_numpy(np.asarray(audio)).to(torch.float32)
    if sr != SAMPLE_RATE:
        # filtered on the model's device; back on the host the rest of the function treats it like a 24 kHz file's samples
        audio = _audio.resample(audio, int(sr), SAMPLE_RATE, device=f5tts.transformer.device)[0].cpu()
    ref_audio_duration = audio.shape[0] / SAMPLE_RATE
    print(f"Got reference audio with duration: {ref_audio_duration:.2f} seconds")

    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < TARGET_RMS:
        audio = audio * TARGET_RMS / rms

    sentences = split_sentences(generation_text)
    is_single_generation = len(sentences) <= 1 or duration is not None
    dual_kw = {} if audio_cfg_strength is None else dict(audio_cfg_strength=_strength(audio_cfg_strength, "audio_cfg_strength"))
    dual_kw.update(window_kw)

    def run(text_for_model, dur, whole=False):
        wave, _ = f5tts.sample(audio[None], text=text_for_model, duration=dur, steps=steps, method=method, speed=speed,
                               cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed, **dual_kw)
        wave = wave.reshape(-1) if wave.ndim > 1 and wave.shape[0] == 1 else wave
        return wave if whole else wave[audio.shape[0]:]               # trim the reference by SAMPLES (generate.py:183)

    def joined(rows, ends):
        """decoded rows [R, L] (reference part included; row r ends at ends[r]) -> the one wave of this call"""
        n_ref = audio.shape[0]
        waves, out_lens = _audio.join_rows(rows, [min(n_ref, e) for e in ends], [max(e - n_ref, 0) for e in ends], [0] * len(ends), **join)
        return waves[0, :out_lens[0]]

    start_date = datetime.datetime.now()
    if is_single_generation:
        if duration is not None:
            duration = int(duration * FRAMES_PER_SEC)
        elif estimate_duration:
            duration = int(estimated_duration(audio, ref_audio_text, generation_text, speed) * FRAMES_PER_SEC)
        text = convert_char_to_pinyin([ref_audio_text + " " + generation_text])
        if join is not None and join["trim_db"] is not None:          # one sentence: a one-segment layout, for the trim alone
            wave = run(text, duration, whole=True)
            wave = joined(wave[None], [wave.shape[0]])
        else:
            wave = run(text, duration)
    elif batch_sentences:
        # every sentence gets the reference mel as conditioning and its own duration; sample() pads to the longest (cfm.py:319-321)
        texts = convert_char_to_pinyin([ref_audio_text + " " + t for t in sentences])
        cond = f5tts._mel_spec(audio[None].to(f5tts.transformer.device)).repeat(len(sentences), 1, 1)
        # (the whole text for every sentence, like the loop's first sentence; the loop's carried-over `duration` -- frames x 93.75
        # again from the second sentence on, generate.py:203-208 -- is a quirk of the loop and is not reproduced here)
        if estimate_duration:
            durs = torch.full((len(sentences),), int(estimated_duration(audio, ref_audio_text, generation_text, speed) * FRAMES_PER_SEC))
        else:
            durs = None                                               # duration predictor, per element (cfm.py:307-308)
        # mel frames out of sample() (vocoder detached for the call), then every sentence is vocoded ON ITS OWN FRAMES: frames past a
        # shorter sentence's duration hold unconstrained ODE state, and a vocoder with a receptive field (Vocos: a k = 7 ConvNeXt stack)
        # would leak them into the last ~0.25 s of that sentence before the trim
        voc = f5tts._vocoder
        try:
            f5tts._vocoder = None
            mel, _ = f5tts.sample(cond, text=texts, duration=durs, steps=steps, method=method, speed=speed, cfg_strength=cfg_strength,
                                  sway_sampling_coef=sway_sampling_coef, seed=seed, **dual_kw, **iso_kw)
        finally:
            f5tts._vocoder = voc
        frames = f5tts.last_durations                                 # per-element frame counts after the clamps of cfm.py:317-318
        if vocode_batched and _takes_lens(voc):
            waves = voc(mel, lens=frames)                             # (sentences, 256 * (N - 1)), row i zero past its own frames
            if join is not None:
                wave = joined(waves, [HOP_LENGTH * (int(f) - 1) for f in frames])
            else:
                wave = torch.cat([waves[i, audio.shape[0]:HOP_LENGTH * (int(frames[i]) - 1)] for i in range(len(sentences))], dim=0)
        elif join is not None:
            rows = [voc(mel[i:i + 1, :int(frames[i])]).reshape(-1) for i in range(len(sentences))]
            wave = joined(_padded_rows(rows), [int(r.shape[0]) for r in rows])
        else:
            wave = torch.cat([voc(mel[i:i + 1, :int(frames[i])]).reshape(-1)[audio.shape[0]:] for i in range(len(sentences))], dim=0)
    else:
        output = []
        for sentence_text in sentences:
            if duration is not None:
                duration = int(duration * FRAMES_PER_SEC)
            elif estimate_duration:                                   # quirk kept: uses the WHOLE text (generate.py:208)
                duration = int(estimated_duration(audio, ref_audio_text, generation_text, speed) * FRAMES_PER_SEC)
            text = convert_char_to_pinyin([ref_audio_text + " " + sentence_text])
            output.append(run(text, duration, whole=join is not None))
        if join is not None:
            wave = joined(_padded_rows(output), [int(r.shape[0]) for r in output])
        else:
            wave = torch.cat(output, dim=0)

    if wave.is_cuda:
        torch.cuda.synchronize()
    generated_duration = wave.shape[0] / SAMPLE_RATE
    print(f"Generated {generated_duration:.2f}s of audio in {datetime.datetime.now() - start_date}.")

    out_rate = SAMPLE_RATE
    if output_sample_rate is not None and output_sample_rate != SAMPLE_RATE:
        wave = _audio.resample(wave, SAMPLE_RATE, output_sample_rate)[0]
        out_rate = output_sample_rate

    if output_path is not None:
        write_wav(output_path, wave.detach().cpu().numpy(), out_rate)
    return wave


def _load_reference(ref_audio_path, ref_audio_text, which: str):
    """-> (fp32 samples, rate, transcript); None = the bundled sample and its text, as in generate()"""
    if ref_audio_path is None:
        audio, sr = read_wav(pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav"))
        return torch.from_numpy(np.asarray(audio)).to(torch.float32), int(sr), DEFAULT_REF_TEXT
    if not ref_audio_text:
        raise ValueError(f"{which}: a reference recording needs its transcript (ref_audio_text)")
    audio, sr = read_wav(ref_audio_path)
    return torch.from_numpy(np.asarray(audio)).to(torch.float32), int(sr), ref_audio_text


CONTROL_KEYS = ("cfg_strength", "sway_sampling_coef", "seed", "speed")
# dual guidance (docs/dual_guidance.md): accepted beside CONTROL_KEYS; it reaches sample() only when the call or a request sets it
AUDIO_CFG_KEY = "audio_cfg_strength"


# guidance window (docs/guidance_window.md): accepted beside CONTROL_KEYS like AUDIO_CFG_KEY; a (lo, hi) pair
CFG_INTERVAL_KEY = "cfg_interval"
# the window of a row whose request sets none in a call where another request does: every finite time, i.e. guided throughout
WHOLE_INTERVAL = (-float(np.finfo(np.float32).max), float(np.finfo(np.float32).max))


def _interval(v, what: str):
    """a guidance window as a (lo, hi) tuple of finite floats with lo <= hi, or ValueError naming `what`"""
    if isinstance(v, (str, bytes)) or not isinstance(v, (list, tuple, np.ndarray)) or len(v) != 2:
        raise ValueError(f"{what} must be a pair (lo, hi), got {v!r}")
    lo, hi = (_strength(x, what) for x in v)
    if max(abs(lo), abs(hi)) > WHOLE_INTERVAL[1]:                      # (the C call compares in fp32)
        raise ValueError(f"{what} must be a pair of finite fp32 numbers, got {v!r}")
    if lo > hi:
        raise ValueError(f"{what} must have lo <= hi, got {v!r}")
    return (lo, hi)


def _strength(v, what: str) -> float:
    """a guidance strength as a finite float, or ValueError naming `what`"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{what} must be a finite number, got {v!r}")
    return float(v)


def request_controls(controls, n_requests: int, row_req, defaults: dict) -> dict:
    """Per-request sampling controls -> the keyword arguments of F5TTS.sample.  controls: None, or a list with one entry per request, each
    None or a dict with any of CONTROL_KEYS; an entry overrides the call-level value (`defaults`) for all rows of its request.  row_req:
    the request of every batch row.  A control no request overrides stays the call-level scalar, so a call without overrides is the call
    it was before; an overridden one becomes a list with one value per row.  ValueError naming the request: a list of the wrong length,
    an entry that is neither None nor a dict, an unknown key.
    "audio_cfg_strength" (dual guidance) is accepted beside CONTROL_KEYS.  The key appears in the result only when `defaults` carries it
    (the call-level value) or a request sets it, and then always as one value per row: a row whose request does not set it gets the
    call-level value, or -- where there is none -- its own cfg_strength, which is algebraically the single-knob rule for that row.
    "cfg_interval" (guidance window) likewise: a (lo, hi) pair of finite numbers with lo <= hi, in the result only when `defaults` or a
    request carries it, then one pair per row; a row without one gets the call-level pair or, where there is none, WHOLE_INTERVAL."""
    out = dict(defaults)
    if CFG_INTERVAL_KEY in out:
        out[CFG_INTERVAL_KEY] = _interval(out[CFG_INTERVAL_KEY], CFG_INTERVAL_KEY)
    if controls is None:
        if AUDIO_CFG_KEY in out:
            out[AUDIO_CFG_KEY] = [_strength(out[AUDIO_CFG_KEY], AUDIO_CFG_KEY)] * len(row_req)
        if CFG_INTERVAL_KEY in out:
            out[CFG_INTERVAL_KEY] = [out[CFG_INTERVAL_KEY]] * len(row_req)
        return out
    controls = list(controls)
    if len(controls) != n_requests:
        raise ValueError(f"controls: expected one entry per request ({n_requests}), got {len(controls)}")
    for i, c in enumerate(controls):
        if c is None:
            continue
        if not isinstance(c, dict):
            raise ValueError(f"request {i}: controls entry must be None or a dict, got {type(c).__name__}")
        unknown = sorted(set(c) - set(CONTROL_KEYS) - {AUDIO_CFG_KEY, CFG_INTERVAL_KEY})
        if unknown:
            raise ValueError(f"request {i}: unknown control(s) {unknown}; expected any of {list(CONTROL_KEYS) + [AUDIO_CFG_KEY, CFG_INTERVAL_KEY]}")
        if AUDIO_CFG_KEY in c:
            _strength(c[AUDIO_CFG_KEY], f"request {i}: {AUDIO_CFG_KEY}")
        if CFG_INTERVAL_KEY in c:
            _interval(c[CFG_INTERVAL_KEY], f"request {i}: {CFG_INTERVAL_KEY}")
    for key in CONTROL_KEYS:
        if any(c is not None and key in c for c in controls):
            out[key] = [controls[i][key] if controls[i] is not None and key in controls[i] else defaults[key] for i in row_req]
    if AUDIO_CFG_KEY in defaults or any(c is not None and AUDIO_CFG_KEY in c for c in controls):
        cfg = out["cfg_strength"]
        rows = []
        for r, i in enumerate(row_req):
            if controls[i] is not None and AUDIO_CFG_KEY in controls[i]:
                rows.append(float(controls[i][AUDIO_CFG_KEY]))
            elif AUDIO_CFG_KEY in defaults:
                rows.append(_strength(defaults[AUDIO_CFG_KEY], AUDIO_CFG_KEY))
            else:
                rows.append(float(cfg[r] if isinstance(cfg, list) else cfg))
        out[AUDIO_CFG_KEY] = rows
    if CFG_INTERVAL_KEY in defaults or any(c is not None and CFG_INTERVAL_KEY in c for c in controls):
        out[CFG_INTERVAL_KEY] = [_interval(controls[i][CFG_INTERVAL_KEY], f"request {i}: {CFG_INTERVAL_KEY}")
                                 if controls[i] is not None and CFG_INTERVAL_KEY in controls[i] else out.get(CFG_INTERVAL_KEY, WHOLE_INTERVAL)
                                 for i in row_req]
    return out


def generate_many(
    requests,
    *,
    steps: int = 8,
    method: Literal["euler", "midpoint", "rk4", "ab2", "ab3"] = "rk4",
    cfg_strength: float = 2.0,
    sway_sampling_coef: float = -1.0,
    speed: float = 1.0,
    seed: Optional[int] = None,
    estimate_duration: bool = False,
    f5tts: Optional[F5TTS] = None,
    model_name: str = "lucasnewman/f5-tts-mlx",
    quantization_bits: Optional[int] = None,
    trim_silence_db: Optional[float] = None,
    output_sample_rate: Optional[int] = None,
    controls=None,
    audio_cfg_strength: Optional[float] = None,
    cfg_interval=None,
    cross_fade_ms=None,
    sentence_pause_ms=None,
    trim_sentence_db=None,
    isolate_rows: bool = False,
):
    """Many voices in one call (no reference counterpart; docs/multi_voice.md).  requests: a list of (generation_text, ref_audio_path or
    None, ref_audio_text); None = the bundled sample and its text.  -> a list of waves, one per request, in order.

    Every sentence of every request (split_sentences; a text without sentence punctuation is one sentence) is one row of ONE ragged
    `sample()` batch.  A row's conditioning is its request's reference, prepared by audio.prepare_references (any sample rate, level
    scaled up to 0.1 rms, and with `trim_silence_db` -- default None: nothing is cut; -42 is the customary figure -- leading and trailing
    silence removed); its text is ref_text + " " + sentence.  Its duration is, with `estimate_duration`, the heuristic on the request's
    WHOLE text and its reference's kept samples (the quirk batch_sentences keeps), otherwise the duration predictor's, which gets
    the rows' frame counts.  The batch is vocoded on each row's own frames -- one decode(mel, lens=frames) call when the vocoder
    takes `lens`, else one call per row --, each row is trimmed by its own reference's kept sample count and the rows of a request
    are concatenated.  Every row gets the same `seed` (the reference re-seeds per element).

    controls (docs/row_controls.md): None, or a list with one entry per request, each None or a dict with any of "cfg_strength",
    "sway_sampling_coef", "seed", "speed"; an entry overrides the call-level value for all rows of that request, and requests with
    different settings still share the one batch (the engine indexes time grid and guidance strength by batch row).
    audio_cfg_strength (docs/dual_guidance.md), as an argument or as a key of a controls entry: dual guidance -- the speaker strength,
    with cfg_strength as the text strength.  sample() gets the keyword (one value per row) only when the call or some request sets it; a
    row whose request does not set it, in a call that does not either, gets its own cfg_strength (the single-knob rule for that row).
    cfg_interval (docs/guidance_window.md), as an argument or as a key of a controls entry: a (lo, hi) pair -- the rows of the request are
    guided only at function evaluations whose time lies in [lo, hi], and an evaluation in which no row of the batch is guided runs the
    conditional branch alone.  sample() gets the keyword (one pair per row) only when the call or some request sets it; a row without
    one is then guided throughout.

    cross_fade_ms, sentence_pause_ms, trim_sentence_db (docs/sentence_joins.md; all None: the assembly above, unchanged): each one value
    for the call or a list with one per request (None = not set for that request).  With any of them set the decoded rows go to
    audio.join_rows -- an optional edge trim per sentence, then ONE f5_wave_join launch for all requests: linear cross-fades between
    the sentences of a request, or fades to and from a pause -- and `output_sample_rate` becomes ONE resample call on the padded
    result, each request sliced to its own length: the bits of resampling each request by itself, since the filter treats everything
    outside a wave as zero and the padding is exactly zero.

    isolate_rows (docs/isolate_rows.md; False: the call as it was, sample() gets no new keyword): True = a row of the batch reads nothing
    from its own padding, so a request's audio no longer depends on which requests share the call: every row lands within the parity
    gate of its solo sample() for the durations it was given.  One value for the call and NOT a key of a controls entry: it is an engine
    option, part of the hipGraph key, and one graph serves each value.  Durations from the duration predictor are covered: sample()
    then asks for the row-isolated prediction, in which a request's frame count does not depend on its batch-mates either
    (docs/duration_rows.md).

    It equals prepare_references -> sample(mel, text, durations, lens=frames) -> the decode -> the same slices, bit for bit; it does
    NOT equal a loop of generate() calls bit for bit (the batch has a key-padding mask, the gain is fp64 arithmetic on fp32 block sums
    instead of torch's fp32 mean, and by default GRN and the conv position embedding see the padding; with isolate_rows they do not, and
    what remains is the rounding order of other kernel routes, not the batch-mates).
    ValueError before any launch, naming the request: an empty list, a request without text, a reference recording without a
    transcript, a reference at a rate the resampler refuses, a `controls` list of the wrong length or with an unknown key, a join
    setting that is negative or not finite, a trim level not below 0, a cfg_interval that is not two finite numbers with lo <= hi, an
    isolate_rows that is not a bool or is True on an mxfp8 model."""
    requests = list(requests)
    if not requests:
        raise ValueError("generate_many needs at least one request")
    if isolate_rows is not False:
        check_isolate_rows(isolate_rows, "" if f5tts is None else f5tts.transformer.engine.precision)
    join = None                                                       # all three unset: nothing of the join is called
    if cross_fade_ms is not None or sentence_pause_ms is not None or trim_sentence_db is not None:
        join = join_options(cross_fade_ms, sentence_pause_ms, trim_sentence_db, len(requests))
    call_level = dict(cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed, speed=speed)
    if audio_cfg_strength is not None:
        call_level[AUDIO_CFG_KEY] = _strength(audio_cfg_strength, AUDIO_CFG_KEY)
    if cfg_interval is not None:
        call_level[CFG_INTERVAL_KEY] = _interval(cfg_interval, CFG_INTERVAL_KEY)
    request_controls(controls, len(requests), [], call_level)          # validation only: the rows are not known yet
    if output_sample_rate is not None:
        output_sample_rate = _audio._rate(output_sample_rate, "output_sample_rate")
        _audio.check_resample_ratio(SAMPLE_RATE, output_sample_rate)
    waves, rates, ref_texts, sentences = [], [], [], []
    for i, req in enumerate(requests):
        if len(req) != 3:
            raise ValueError(f"request {i}: expected (generation_text, ref_audio_path, ref_audio_text), got {len(req)} items")
        text, path, ref_text = req
        if not isinstance(text, str) or not text.strip():
            raise ValueError(f"request {i}: no text to generate")
        audio, sr, ref_text = _load_reference(path, ref_text, f"request {i}")
        try:
            _audio.check_resample_ratio(sr, SAMPLE_RATE)
        except ValueError as exc:
            raise ValueError(f"request {i}: reference at {sr} Hz: {exc}") from None
        waves.append(audio)
        rates.append(sr)
        ref_texts.append(ref_text)
        sentences.append(split_sentences(text) or [text.strip()])

    if f5tts is None:
        f5tts = F5TTS.from_pretrained(model_name, quantization_bits=quantization_bits)
    iso_kw = {}
    if isolate_rows is not False:
        iso_kw["isolate_rows"] = check_isolate_rows(isolate_rows, f5tts.transformer.engine.precision)
    voc = getattr(f5tts, "_vocoder", None)
    if voc is None:
        raise RuntimeError("generate_many() needs a model with a vocoder (F5TTS(..., vocoder=...) / from_pretrained with Vocos)")

    try:
        refs = _audio.prepare_references(waves, rates, trim_silence_db=trim_silence_db, target_rms=TARGET_RMS,
                                         device=f5tts.transformer.device)
    except ValueError as exc:                                         # one reference per request: its rows are the requests
        msg = str(exc)
        raise ValueError("request " + msg[4:] if msg.startswith("row ") else msg) from None

    row_req = [i for i, ss in enumerate(sentences) for _ in ss]      # request of every row
    texts = convert_char_to_pinyin([ref_texts[i] + " " + s for i, ss in enumerate(sentences) for s in ss])
    cond = refs.mel[torch.tensor(row_req, device=refs.mel.device)]
    lens = torch.tensor([refs.frames[i] for i in row_req], dtype=torch.int64)
    ctl = request_controls(controls, len(requests), row_req, call_level)
    req_speed = [speed if controls is None or controls[i] is None else controls[i].get("speed", speed) for i in range(len(requests))]
    durs = None                                                       # duration predictor, per row, with lens (cfm.py:307-308)
    if estimate_duration:
        per_req = [int(estimated_duration(np.broadcast_to(np.float32(0), (refs.samples[i],)), ref_texts[i], requests[i][0], req_speed[i])
                       * FRAMES_PER_SEC) for i in range(len(requests))]
        durs = torch.tensor([per_req[i] for i in row_req], dtype=torch.int64)

    start_date = datetime.datetime.now()
    try:                                                              # mel frames out of sample(): each row is vocoded on its own frames
        f5tts._vocoder = None
        mel, _ = f5tts.sample(cond, text=texts, duration=durs, lens=lens, steps=steps, method=method, speed=ctl["speed"],
                              cfg_strength=ctl["cfg_strength"], sway_sampling_coef=ctl["sway_sampling_coef"], seed=ctl["seed"],
                              **{k: ctl[k] for k in (AUDIO_CFG_KEY, CFG_INTERVAL_KEY) if k in ctl}, **iso_kw)
    finally:
        f5tts._vocoder = voc
    frames = f5tts.last_durations                                     # per-row frame counts after the clamps of cfm.py:317-318
    if join is not None:
        if _takes_lens(voc):
            decoded = voc(mel, lens=frames)
            ends = [HOP_LENGTH * (int(f) - 1) for f in frames]
        else:
            rows = [voc(mel[r:r + 1, :int(frames[r])]).reshape(-1) for r in range(len(row_req))]
            decoded, ends = _padded_rows(rows), [int(r.shape[0]) for r in rows]
        n_ref = [refs.samples[i] for i in row_req]
        joined, out_lens = _audio.join_rows(decoded, [min(b, e) for b, e in zip(n_ref, ends)], [max(e - b, 0) for b, e in zip(n_ref, ends)],
                                            row_req, **join)
        out = _audio.resample_rows(joined, out_lens, SAMPLE_RATE, output_sample_rate or SAMPLE_RATE)
    else:
        if _takes_lens(voc):
            decoded = voc(mel, lens=frames)                           # (rows, 256 * (N - 1)), row r zero past its own frames
            rows = [decoded[r, refs.samples[i]:HOP_LENGTH * (int(frames[r]) - 1)] for r, i in enumerate(row_req)]
        else:
            rows = [voc(mel[r:r + 1, :int(frames[r])]).reshape(-1)[refs.samples[i]:] for r, i in enumerate(row_req)]
        out = []
        for i in range(len(requests)):
            wave = torch.cat([rows[r] for r, q in enumerate(row_req) if q == i], dim=0)
            if output_sample_rate is not None and output_sample_rate != SAMPLE_RATE:
                wave = _audio.resample(wave, SAMPLE_RATE, output_sample_rate)[0]
            out.append(wave)
    if out[0].is_cuda:
        torch.cuda.synchronize()
    total = sum(w.shape[0] for w in out) / (output_sample_rate or SAMPLE_RATE)
    print(f"Generated {total:.2f}s of audio for {len(requests)} requests ({len(row_req)} rows) in {datetime.datetime.now() - start_date}.")
    return out


def read_requests(path):
    """A --requests file: one JSON object per line with "text", and optionally "ref_audio", "ref_text" and "output" (blank lines are
    skipped) -> a list of dicts with exactly these four keys (None where a line leaves one out)."""
    import json
    reqs = []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                obj = json.loads(line)
            except json.JSONDecodeError as exc:
                raise ValueError(f"{path}:{no}: not a JSON object ({exc.msg})") from None
            if not isinstance(obj, dict) or not isinstance(obj.get("text"), str):
                raise ValueError(f'{path}:{no}: expected an object with a "text" string')
            unknown = set(obj) - {"text", "ref_audio", "ref_text", "output"} - {"cfg", "sway_coef", "seed", "speed", "audio_cfg", "cfg_interval"} - set(JOIN_FILE_KEYS)
            if unknown:
                raise ValueError(f"{path}:{no}: unknown key(s) {sorted(unknown)}")
            reqs.append({k: obj.get(k) for k in ("text", "ref_audio", "ref_text", "output")})
    return reqs


JOIN_FILE_KEYS = {"cross_fade_ms": "cross_fade_ms", "pause_ms": "sentence_pause_ms", "trim_db": "trim_sentence_db"}


def read_request_joins(path):
    """The optional per-request sentence-join settings of a --requests file: the keys "cross_fade_ms", "pause_ms" and "trim_db" of every
    line (same lines as read_requests, which ignores them) -> a dict for generate_many(**...) with, for every setting some line sets, a
    list with one value per request (None where a line leaves it out); empty when no line sets any.  ValueError naming file and line for
    a value join_options would refuse."""
    import json
    cols = {name: [] for name in JOIN_FILE_KEYS.values()}
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                obj = json.loads(line)
            except json.JSONDecodeError as exc:
                raise ValueError(f"{path}:{no}: not a JSON object ({exc.msg})") from None
            if not isinstance(obj, dict):
                raise ValueError(f"{path}:{no}: expected an object")
            for key, name in JOIN_FILE_KEYS.items():
                try:
                    cols[name].append(_join_value(obj.get(key), name))
                except ValueError as exc:
                    raise ValueError(f'{path}:{no}: "{key}": {exc}') from None
    return {name: v for name, v in cols.items() if any(x is not None for x in v)}


def read_request_controls(path):
    """The optional per-request sampling controls of a --requests file: the keys "cfg", "sway_coef", "seed", "speed", "audio_cfg" and
    "cfg_interval" ([lo, hi], kept under the same name) of every line (same lines as read_requests, which ignores them) -> a list with one entry per request for generate_many(controls=...):
    a dict with the controls the line sets ("cfg_strength", "sway_sampling_coef", "seed", "speed", "audio_cfg_strength"), or None when
    it sets none."""
    import json
    names = {"cfg": "cfg_strength", "sway_coef": "sway_sampling_coef", "seed": "seed", "speed": "speed", "audio_cfg": AUDIO_CFG_KEY}
    out = []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                obj = json.loads(line)
            except json.JSONDecodeError as exc:
                raise ValueError(f"{path}:{no}: not a JSON object ({exc.msg})") from None
            if not isinstance(obj, dict):
                raise ValueError(f"{path}:{no}: expected an object")
            c = {}
            for key, name in names.items():
                if key not in obj:
                    continue
                v = obj[key]
                ok = (isinstance(v, int) and not isinstance(v, bool)) if key == "seed" else (
                    (isinstance(v, (int, float)) and not isinstance(v, bool)) or (key == "sway_coef" and v is None))
                if not ok:
                    raise ValueError(f'{path}:{no}: "{key}" must be {"an integer" if key == "seed" else "a number"}, got {v!r}')
                c[name] = v
            if CFG_INTERVAL_KEY in obj:
                try:
                    c[CFG_INTERVAL_KEY] = _interval(obj[CFG_INTERVAL_KEY], f'"{CFG_INTERVAL_KEY}"')
                except ValueError as exc:
                    raise ValueError(f"{path}:{no}: {exc}") from None
            out.append(c or None)
    return out


# command line: the reference's flags and defaults (generate.py:248-362), table driven
_CLI = (
    ("--model", str, "lucasnewman/f5-tts-mlx", "checkpoint: hub name or local directory"),
    ("--text", str, None, "what to say; read from stdin when omitted"),
    ("--duration", float, None, "total length (reference + generated) in seconds"),
    ("--estimate-duration", bool, False, "derive the length from the reference audio and the text sizes"),
    ("--ref-audio", str, None, "24 kHz mono WAV to clone (default: the bundled sample)"),
    ("--ref-text", str, None, "transcript of --ref-audio"),
    ("--output", str, None, "WAV file to write"),
    ("--steps", int, 8, "ODE grid points (steps - 1 solver updates)"),
    ("--cfg", float, 2.0, "classifier-free guidance strength (with --audio-cfg: the text strength)"),
    ("--audio-cfg", float, None, "dual guidance: speaker strength (full against text-only prediction); --cfg is then the text strength"),
    ("--sway-coef", float, -1.0, "sway-sampling coefficient of the time grid"),
    ("--speed", float, 1.0, "speaking-rate factor used by the duration heuristics"),
    ("--seed", int, None, "noise seed"),
)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(
        description="F5-TTS text to speech on MI355X (same flags as f5_tts_mlx.generate)",
        epilog="Text front-end: single-byte (ASCII / Latin) text is tokenised exactly like the reference; Chinese text needs "
               "jieba and pypinyin (utils.py:139-173), which this package uses when they are importable and otherwise refuses "
               "with an error rather than guessing.")
    for flag, kind, dflt, doc in _CLI:
        ap.add_argument(flag, type=kind, default=dflt, help=doc)
    ap.add_argument("--method", default="rk4", choices=("euler", "midpoint", "rk4", "ab2", "ab3"),
                    help="ODE solver (ab2 / ab3: Adams-Bashforth, one evaluation per step, docs/multistep.md)")
    ap.add_argument("--q", type=int, default=None, choices=(4, 8), help="load the MLX 4/8-bit checkpoint (model_v1_{4,8}b.safetensors).  The group-quantised weights are EXPANDED to fp32 on load and run "
                         "through the same 16-bit MFMA kernels as the full checkpoint: unlike in the reference this saves neither memory nor time here")
    ap.add_argument("--resample-ref", action="store_true", help="accept a --ref-audio of any sample rate: it is converted to 24 kHz on the GPU")
    ap.add_argument("--output-rate", type=int, default=None, help="sample rate of the result in Hz (default: 24000, the model's own rate)")
    ap.add_argument("--batch-sentences", action="store_true", help="sample all sentences of the text as one ragged batch instead of one after the other")
    ap.add_argument("--vocode-batched", action="store_true", help="with --batch-sentences: vocode the batch in one ragged call instead of one call per sentence")
    ap.add_argument("--requests", default=None, metavar="FILE.jsonl",
                    help="many voices in one batch: one JSON object per line with text, ref_audio, ref_text and output (ref_audio / ref_text "
                         "left out: the bundled sample); excludes --text and --output")
    ap.add_argument("--trim-silence", type=float, default=None, metavar="DB",
                    help="with --requests: cut leading and trailing silence below DB dB off every reference (-42 is customary; default: cut nothing)")
    ap.add_argument("--cfg-interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="guidance window: guide only at function evaluations whose time lies in [LO, HI] (default: throughout)")
    ap.add_argument("--isolate-rows", action="store_true",
                    help="with --requests or --batch-sentences: a row of the batch reads nothing from its own padding, so its audio does not depend on "
                         "what shares the batch (docs/isolate_rows.md)")
    ap.add_argument("--cross-fade-ms", type=float, default=None, metavar="MS",
                    help="linear cross-fade of MS milliseconds between the sentences of a text (default: plain concatenation)")
    ap.add_argument("--sentence-pause-ms", type=float, default=None, metavar="MS",
                    help="MS milliseconds of silence between sentences; with --cross-fade-ms the sentences fade to and from it")
    ap.add_argument("--trim-sentence-db", type=float, default=None, metavar="DB",
                    help="cut leading and trailing near-silence below DB dB off every generated sentence (-42 is customary)")
    ns = ap.parse_args(argv)
    if ns.requests is not None:
        for flag, value in (("--text", ns.text), ("--output", ns.output), ("--ref-audio", ns.ref_audio), ("--ref-text", ns.ref_text),
                            ("--duration", ns.duration)):
            if value is not None:
                ap.error(f"--requests excludes {flag}: every line of the file carries its own")
    elif ns.trim_silence is not None:
        ap.error("--trim-silence needs --requests")
    return ns


def main(argv=None):
    ns = parse_args(argv)
    if ns.requests is not None:
        reqs = read_requests(ns.requests)
        controls = read_request_controls(ns.requests)
        joins = dict(cross_fade_ms=ns.cross_fade_ms, sentence_pause_ms=ns.sentence_pause_ms, trim_sentence_db=ns.trim_sentence_db)
        for name, per_req in read_request_joins(ns.requests).items():  # a line's own value goes before the flag's
            joins[name] = [joins[name] if v is None else v for v in per_req]
        joins = {k: v for k, v in joins.items() if v is not None}
        waves = generate_many([(r["text"], r["ref_audio"], r["ref_text"]) for r in reqs], steps=ns.steps, method=ns.method,
                              cfg_strength=ns.cfg, sway_sampling_coef=ns.sway_coef, speed=ns.speed, seed=ns.seed,
                              estimate_duration=ns.estimate_duration, model_name=ns.model, quantization_bits=ns.q,
                              trim_silence_db=ns.trim_silence, output_sample_rate=ns.output_rate,
                              controls=controls if any(c is not None for c in controls) else None,
                              **({} if ns.audio_cfg is None else dict(audio_cfg_strength=ns.audio_cfg)),
                              **({} if ns.cfg_interval is None else dict(cfg_interval=tuple(ns.cfg_interval))),
                              **(dict(isolate_rows=True) if ns.isolate_rows else {}), **joins)
        for r, wave in zip(reqs, waves):
            if r["output"] is not None:
                write_wav(r["output"], wave.detach().cpu().numpy(), ns.output_rate or SAMPLE_RATE)
        return

    text = ns.text
    if text is None:
        if sys.stdin.isatty():
            print("Please enter the text to generate:")
            text = input("> ").strip()
        else:
            text = sys.stdin.read().strip()                            # generate.py:330-335 strips both

    generate(text, duration=ns.duration, estimate_duration=ns.estimate_duration, model_name=ns.model, ref_audio_path=ns.ref_audio,
             ref_audio_text=ns.ref_text, steps=ns.steps, method=ns.method, cfg_strength=ns.cfg, sway_sampling_coef=ns.sway_coef,
             speed=ns.speed, seed=ns.seed, quantization_bits=ns.q, output_path=ns.output, resample_ref=ns.resample_ref,
             output_sample_rate=ns.output_rate, batch_sentences=ns.batch_sentences, vocode_batched=ns.vocode_batched,
             **({} if ns.audio_cfg is None else dict(audio_cfg_strength=ns.audio_cfg)),
             **({} if ns.cfg_interval is None else dict(cfg_interval=tuple(ns.cfg_interval))),
             **(dict(isolate_rows=True) if ns.isolate_rows else {}),
             **{k: v for k, v in (("cross_fade_ms", ns.cross_fade_ms), ("sentence_pause_ms", ns.sentence_pause_ms),
                                  ("trim_sentence_db", ns.trim_sentence_db)) if v is not None})


if __name__ == "__main__":
    main()
