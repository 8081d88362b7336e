"""Speech editing: regenerate chosen spans of a recording and keep the rest (no counterpart in the MLX reference; the PyTorch
F5-TTS front end calls it speech editing).

The DiT is an infilling model: its training forward zeroes an interior span of the conditioning mel and predicts that span
(`F5TTS.__call__`, cfm.py:198-224).  `F5TTS.sample(..., edit_mask=...)` exposes that at sampling time; this module adds what makes it
usable from a WAV file:

  edit_layout   pure host arithmetic: which source frame each frame of the edited utterance comes from (-1 = regenerate) and the
                sample-domain segment table of the result
  gather_frames one launch that lays the edited conditioning mel out on the device (f5_op_gather_frames)
  fade_table    the raised-cosine cross-fade, fp64 rounded once
  wave_patch    puts the original samples back outside the edited spans (f5_op_wave_patch)
  edit_speech   the application-level call; `python -m f5_tts_mlx_amd.edit` is its command line

docs/edit.md states the contract and what is unmeasured.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio as _audio
from . import engine as _eng

SAMPLE_RATE = 24_000
HOP_LENGTH = 256
N_FFT = 1024
FRAMES_PER_SEC = SAMPLE_RATE / HOP_LENGTH              # 93.75
TARGET_RMS = 0.1                                       # generate.py's RMS normalisation (scales up only)
GUARD_FRAMES = N_FFT // (2 * HOP_LENGTH)               # 2: the frames whose 1024-sample window reaches into the replaced audio
MIN_KEEP_FRAMES = 2                                    # a kept stretch between two regenerated ones holds two fades of <= hop samples
MAX_SEGMENTS = 64                                      # f5_op_wave_patch: segments per row


def frame_segments(src_idx: np.ndarray) -> List[Tuple[int, int, int]]:
    """The runs of a src_idx map as (dst_begin, dst_end, src_begin) in frames: a kept run is a stretch of consecutive source frames,
    src_begin = -1 is a regenerated run.  Sorted and contiguous from 0."""
    src_idx = np.asarray(src_idx)
    segs: List[Tuple[int, int, int]] = []
    n, i = len(src_idx), 0
    while i < n:
        j = i + 1
        if src_idx[i] < 0:
            while j < n and src_idx[j] < 0:
                j += 1
            segs.append((i, j, -1))
        else:
            while j < n and src_idx[j] == src_idx[j - 1] + 1:
                j += 1
            segs.append((i, j, int(src_idx[i])))
        i = j
    return segs


def edit_layout(n_src_frames: int, spans: Sequence[Tuple[int, int, int]], guard_frames: int = GUARD_FRAMES):
    """Lay an edited utterance out in frames.  `spans` = [(start_frame, end_frame, new_len_frames), ...] on the SOURCE's frame axis:
    frames [start, end) are replaced by new_len regenerated frames.  Spans must be sorted and disjoint (touching is allowed), inside
    [0, n_src_frames], non-empty, with new_len >= 1; anything else raises ValueError.

    Returns (src_idx, segments):
      src_idx   int32 [N]: the source frame of every frame of the edited utterance, -1 = regenerate here (f5_op_gather_frames' map)
      segments  int32 [S][3]: (dst_begin, dst_end, src_begin) in SAMPLES of the vocoded result, hop x (N - 1) samples long --
                hop x the runs of src_idx (frame_segments), clipped to that length, empty ones dropped; src_begin = -1 for a
                regenerated segment (f5_op_wave_patch's table)

    Rules.  Every span is widened by `guard_frames` source frames on both sides, clipped at the edges; the widened frames are
    regenerated too but keep their count (n_fft / (2 hop) = 2: the frames whose analysis window reaches into the replaced audio).  A
    kept stretch shorter than MIN_KEEP_FRAMES = 2 between two regenerated ones is regenerated as well, count kept (it could not hold its
    two cross-fades).  The final frame is always regenerated: sample() needs duration >= lens + 1 (cfm.py:317)."""
    n_src = int(n_src_frames)
    guard = int(guard_frames)
    if n_src < 1:
        raise ValueError(f"n_src_frames must be >= 1 (got {n_src_frames})")
    if guard < 0:
        raise ValueError("guard_frames must be >= 0")
    spans = [(int(s), int(e), int(n)) for s, e, n in spans]
    regen = np.zeros(n_src, dtype=bool)                  # source frames that are regenerated in place (the guards)
    prev_end = 0
    for i, (s, e, n) in enumerate(spans):
        if not (0 <= s < e <= n_src):
            raise ValueError(f"span {i} = [{s}, {e}) is empty or outside [0, {n_src}]")
        if n < 1:
            raise ValueError(f"span {i}: new length {n} must be >= 1 frame")
        if s < prev_end:
            raise ValueError(f"span {i} = [{s}, {e}) starts before the previous span ends ({prev_end}): spans must be sorted and disjoint")
        prev_end = e
        regen[max(0, s - guard):s] = True
        regen[e:min(n_src, e + guard)] = True
    idx: List[int] = []
    pos = 0
    for s, e, n in spans:
        idx.extend(-1 if regen[f] else f for f in range(pos, s))
        idx.extend([-1] * n)
        pos = e
    idx.extend(-1 if regen[f] else f for f in range(pos, n_src))
    src_idx = np.asarray(idx, dtype=np.int32)
    src_idx[-1] = -1                                     # the final frame: duration >= lens + 1
    runs = frame_segments(src_idx)
    for k, (d0, d1, s0) in enumerate(runs):              # a kept stretch too short for two fades joins its regenerated neighbours
        if s0 >= 0 and 0 < k < len(runs) - 1 and d1 - d0 < MIN_KEEP_FRAMES:
            src_idx[d0:d1] = -1
    N = len(src_idx)
    L = HOP_LENGTH * (N - 1)
    segs = [(d0 * HOP_LENGTH, min(d1 * HOP_LENGTH, L), -1 if s0 < 0 else s0 * HOP_LENGTH) for d0, d1, s0 in frame_segments(src_idx)]
    segs = [t for t in segs if t[1] > t[0]]
    segments = np.asarray(segs, dtype=np.int32).reshape(-1, 3)
    return src_idx, segments


@lru_cache(maxsize=None)
def fade_table(F: int) -> np.ndarray:
    """fade[i] = 0.5 (1 - cos(pi (i + 0.5) / F)), i = 0 .. F - 1, in fp64 and rounded once to fp32 (audio.resample_table's convention):
    the weight of the ORIGINAL sample i samples into a kept segment from a seam.  fade[i] + fade[F - 1 - i] = 1 before rounding."""
    F = int(F)
    if F < 0:
        raise ValueError(f"fade length must be >= 0 (got {F})")
    i = np.arange(F, dtype=np.float64)
    t = (0.5 * (1.0 - np.cos(np.pi * (i + 0.5) / max(F, 1)))).astype(np.float32)
    t.setflags(write=False)                              # cached: handed out to every caller
    return t


def gather_frames(src: torch.Tensor, src_idx) -> Tuple[torch.Tensor, torch.Tensor]:
    """src (B, n_src, mel) fp32 CUDA, src_idx int32 (B, N) (tensor or array; -1 = regenerate) -> (cond (B, N, mel) fp32, keep (B, N)
    uint8) in one launch: f5_op_gather_frames."""
    lib = _eng.load_library()
    assert src.is_cuda and src.dtype == torch.float32 and src.ndim == 3
    src = src.contiguous()
    idx = torch.as_tensor(np.asarray(src_idx.cpu() if torch.is_tensor(src_idx) else src_idx), dtype=torch.int32)
    if idx.ndim == 1:
        idx = idx[None]
    B, n_src, mel = src.shape
    if idx.shape[0] != B:
        raise ValueError(f"src_idx has {idx.shape[0]} rows, src {B}")
    idx = idx.to(src.device).contiguous()
    N = idx.shape[1]
    cond = torch.empty((B, N, mel), dtype=torch.float32, device=src.device)
    keep = torch.empty((B, N), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        _eng.check(lib.f5_op_gather_frames(_eng.ptr(src), _eng.ptr(idx), _eng.ptr(cond), _eng.ptr(keep), B, n_src, N, mel,
                                           _eng.stream_ptr(src.device)), "f5_op_gather_frames")
    return cond, keep


_dev_fades = {}


def wave_patch(gen: torch.Tensor, src: torch.Tensor, segments, fade_samples: int = 256) -> torch.Tensor:
    """gen (B, L) fp32 CUDA (the vocoded edit), src (B, Ls) fp32 CUDA (the source at the model's rate and scale), segments int32
    (B, S, 3) or (S, 3) host table (edit_layout) -> (B, L): f5_op_wave_patch.  The library refuses a bad table (ValueError here)."""
    lib = _eng.load_library()
    assert gen.is_cuda and src.is_cuda and gen.dtype == src.dtype == torch.float32 and gen.ndim == src.ndim == 2
    gen, src = gen.contiguous(), src.contiguous()
    segs = np.ascontiguousarray(np.asarray(segments, dtype=np.int32))
    if segs.ndim == 2:
        segs = segs[None]
    B, L = gen.shape
    if segs.ndim != 3 or segs.shape[0] != B or segs.shape[2] != 3 or src.shape[0] != B:
        raise ValueError(f"segments must be (B, S, 3) with B = {B}, got {segs.shape}; src has {src.shape[0]} rows")
    F = int(fade_samples)
    key = (str(gen.device), F)
    if F > 0 and key not in _dev_fades:
        _dev_fades[key] = torch.from_numpy(fade_table(F).copy()).to(gen.device)
    fade = _dev_fades.get(key) if F > 0 else None
    out = torch.empty_like(gen)
    with torch.cuda.device(gen.device):
        rc = lib.f5_op_wave_patch(_eng.ptr(gen), _eng.ptr(src), segs.ctypes.data_as(C.c_void_p), _eng.ptr(fade), _eng.ptr(out), B,
                                  C.c_int64(L), C.c_int64(src.shape[1]), int(segs.shape[1]), F, _eng.stream_ptr(gen.device))
    if rc != 0 and lib.f5_last_error().startswith(b"wave_patch:"):
        raise ValueError(lib.f5_last_error().decode("utf-8", "replace"))
    _eng.check(rc, "f5_op_wave_patch")
    return out


def spans_to_frames(spans_seconds, n_src_frames: int) -> List[Tuple[int, int, int]]:
    """[(start_s, end_s, new_duration_s or None), ...] -> [(start_frame, end_frame, new_len_frames), ...]: floor(start x 93.75),
    ceil(end x 93.75) (clipped to the recording), new length max(1, round(seconds x 93.75)), the span's own length by default."""
    out = []
    for sp in spans_seconds:
        start, end = float(sp[0]), float(sp[1])
        new = sp[2] if len(sp) > 2 else None
        if not (0.0 <= start < end):
            raise ValueError(f"span {sp!r}: need 0 <= start < end (seconds)")
        s = min(int(math.floor(start * FRAMES_PER_SEC)), int(n_src_frames))
        e = min(int(math.ceil(end * FRAMES_PER_SEC)), int(n_src_frames))
        n = e - s if new is None else max(1, int(round(float(new) * FRAMES_PER_SEC)))
        out.append((s, e, n))
    return out


def edit_speech(source_wav, target_text: str, spans_seconds, f5tts, *, patch_wave: bool = True, fade_samples: int = 256,
                resample_source: bool = False, steps: int = 8, method: str = "rk4", cfg_strength: float = 2.0,
                sway_sampling_coef: float = -1.0, seed: Optional[int] = None, output_path: Optional[str] = None) -> torch.Tensor:
    """Regenerate `spans_seconds` = [(start, end, new_duration_or_None), ...] of the recording `source_wav` (path or WAV bytes) so that
    the whole says `target_text`, and keep the rest of the recording.  Returns the edited wave (1-D, 24 kHz, on the model's device) and
    writes it to `output_path` when given.

    The recording is read, converted to 24 kHz when `resample_source` allows it (audio.resample), RMS-scaled as generate() does (up
    only) and turned into mel frames; edit_layout + gather_frames build the conditioning of the edited utterance; one
    `f5tts.sample(..., duration=N, lens=N - 1, edit_mask=keep)` call with the vocoder attached regenerates the spans (and the guard
    frames around them); `patch_wave` puts the recording's own samples back outside them with raised-cosine cross-fades of
    `fade_samples` samples at the seams (wave_patch); an RMS gain that was applied is undone at the end."""
    from .generate import read_wav, write_wav
    from .utils import convert_char_to_pinyin
    if getattr(f5tts, "_vocoder", None) is None:
        raise RuntimeError("edit_speech() needs a model with a vocoder (F5TTS(..., vocoder=...) / from_pretrained with Vocos)")
    device = f5tts.transformer.device
    audio, sr = read_wav(source_wav)
    if sr != SAMPLE_RATE and not resample_source:
        raise ValueError("Source audio must have a sample rate of 24kHz (pass resample_source=True to convert it)")
    audio = torch.from_numpy(np.asarray(audio)).to(torch.float32)
    if sr != SAMPLE_RATE:
        audio = _audio.resample(audio, int(sr), SAMPLE_RATE, device=device)[0].cpu()
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    gain = None
    if rms < TARGET_RMS:
        gain = TARGET_RMS / rms
        audio = audio * gain
    audio = audio.to(device)

    mel = f5tts._mel_spec(audio[None])                                   # (1, n_src, mel)
    n_src = int(mel.shape[1])
    src_idx, segments = edit_layout(n_src, spans_to_frames(spans_seconds, n_src))
    N = len(src_idx)
    if len(segments) > MAX_SEGMENTS:
        raise ValueError(f"{len(segments)} segments: at most {MAX_SEGMENTS} (about {MAX_SEGMENTS // 2} spans) per call")
    cond, keep = gather_frames(mel, src_idx[None])
    text = convert_char_to_pinyin([target_text])
    wave, _ = f5tts.sample(cond, text=text, duration=N, lens=torch.tensor([N - 1]), edit_mask=keep.to(torch.bool), steps=steps,
                           method=method, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
    wave = wave.reshape(1, -1)
    if wave.shape[1] != HOP_LENGTH * (N - 1):
        raise ValueError(f"the target text needs {wave.shape[1] // HOP_LENGTH + 1} frames, the edited recording has {N}: "
                         "lengthen a replaced span")
    if patch_wave:
        wave = wave_patch(wave, audio[None], segments, fade_samples)
    wave = wave[0]
    if gain is not None:
        wave = wave / gain.to(device)
    if output_path is not None:
        write_wav(output_path, wave.detach().cpu().numpy(), SAMPLE_RATE)
    return wave


def _parse_span(s: str):
    """'1.20-1.85' or '1.20-1.85:0.9' -> (1.20, 1.85, None or 0.9)"""
    body, _, new = s.partition(":")
    start, sep, end = body.partition("-")
    if not sep:
        raise argparse.ArgumentTypeError(f"span {s!r}: expected START-END[:NEW_DURATION] in seconds")
    try:
        return float(start), float(end), (float(new) if new else None)
    except ValueError:
        raise argparse.ArgumentTypeError(f"span {s!r}: expected START-END[:NEW_DURATION] in seconds")


def main(argv=None):
    ap = argparse.ArgumentParser(description="F5-TTS speech editing on MI355X: regenerate spans of a recording, keep the rest")
    ap.add_argument("--model", default="lucasnewman/f5-tts-mlx", help="checkpoint: hub name or local directory")
    ap.add_argument("--source", required=True, help="24 kHz mono WAV to edit")
    ap.add_argument("--text", required=True, help="transcript of the WHOLE edited recording")
    ap.add_argument("--span", type=_parse_span, action="append", required=True, metavar="START-END[:NEW]",
                    help="seconds of the source to regenerate, optionally with the new duration of that stretch; repeatable, in order")
    ap.add_argument("--output", required=True, help="WAV file to write")
    ap.add_argument("--steps", type=int, default=8, help="ODE grid points")
    ap.add_argument("--method", default="rk4", choices=("euler", "midpoint", "rk4", "ab2", "ab3"), help="ODE solver")
    ap.add_argument("--cfg", type=float, default=2.0, help="classifier-free guidance strength")
    ap.add_argument("--sway-coef", type=float, default=-1.0, help="sway-sampling coefficient of the time grid")
    ap.add_argument("--seed", type=int, default=None, help="noise seed")
    ap.add_argument("--fade-samples", type=int, default=256, help="cross-fade length at the seams, in samples (<= 256)")
    ap.add_argument("--no-patch", action="store_true", help="return the vocoded result as it is: do not put the source's samples back")
    ap.add_argument("--resample-source", action="store_true", help="accept a --source of any sample rate: it is converted to 24 kHz on the GPU")
    ns = ap.parse_args(argv)
    from .cfm import F5TTS
    f5tts = F5TTS.from_pretrained(ns.model)
    edit_speech(ns.source, ns.text, ns.span, f5tts, patch_wave=not ns.no_patch, fade_samples=ns.fade_samples,
                resample_source=ns.resample_source, steps=ns.steps, method=ns.method, cfg_strength=ns.cfg,
                sway_sampling_coef=ns.sway_coef, seed=ns.seed, output_path=ns.output)


if __name__ == "__main__":
    main()
