"""Mel front-end (reference: f5_tts_mlx/audio.py) on the HIP engine.

`mel_filters` / `hanning` build small constant tables on the host exactly as the reference does
(float32 arithmetic, HTK scale, no norm); the STFT + filterbank + log run in one HIP kernel
(`f5_mel_spectrogram`, csrc/audio.hip).

`resample` changes the sample rate (no reference counterpart: the reference refuses anything but 24 kHz): the polyphase table is
built on the host in fp64 (`resample_table`), the filter runs in one HIP kernel (`f5_resample_batch`, csrc/audio.hip).

`join_rows` is the back half of a ragged batch (no reference counterpart; docs/sentence_joins.md): the decoded sentences of every
request are laid out with an optional edge trim, pauses and linear cross-fades by host integer arithmetic (`join_layout`,
`sentence_windows`) and ONE HIP launch (`f5_wave_join`, csrc/audio.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

from . import engine as _eng


@lru_cache(maxsize=None)
def mel_filters(sample_rate: int, n_fft: int, n_mels: int, f_min: float = 0, f_max: Optional[float] = None,
                norm: Optional[str] = None, mel_scale: str = "htk") -> np.ndarray:
    """audio.py:12-98.  Returns (n_mels, n_fft // 2 + 1) float32 (torch-compatible filterbank)."""
    if mel_scale != "htk":
        raise NotImplementedError("only the HTK mel scale is used on the sampling path (audio.py:188)")

    def hz_to_mel(freq):
        return 2595.0 * math.log10(1.0 + freq / 700.0)

    f_max = f_max or sample_rate / 2
    n_freqs = n_fft // 2 + 1
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs, dtype=np.float32)
    m_pts = np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2, dtype=np.float32)
    f_pts = (np.float32(700.0) * (np.float32(10.0) ** (m_pts / np.float32(2595.0)) - np.float32(1.0))).astype(np.float32)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down_slopes = (-slopes[:, :-2]) / f_diff[:-1]
    up_slopes = slopes[:, 2:] / f_diff[1:]
    filterbank = np.maximum(np.float32(0), np.minimum(down_slopes, up_slopes))
    if norm == "slaney":
        enorm = 2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])
        filterbank = filterbank * enorm[None, :]
    return np.ascontiguousarray(filterbank.T.astype(np.float32))


@lru_cache(maxsize=None)
def hanning(size: int) -> np.ndarray:
    """audio.py:101-112 — periodic Hann window."""
    return np.hanning(size + 1)[:-1].astype(np.float32)


_dev_tables = {}


def _tables(device: torch.device, sample_rate: int, n_fft: int, n_mels: int):
    key = (str(device), sample_rate, n_fft, n_mels)
    if key not in _dev_tables:
        _dev_tables[key] = (torch.from_numpy(hanning(n_fft)).to(device),
                            torch.from_numpy(mel_filters(sample_rate, n_fft, n_mels)).to(device))
    return _dev_tables[key]


def log_mel_spectrogram(audio: torch.Tensor, sample_rate: int = 24_000, n_mels: int = 100, n_fft: int = 1024,
                        hop_length: int = 256, padding: int = 0, device=None) -> torch.Tensor:
    """audio.py:162-210.  audio: [t] or [b, t] (device tensor or anything torch.as_tensor accepts).
    Returns (b, frames, n_mels) float32 on the GPU — the layout the reference code produces."""
    lib = _eng.load_library()
    audio = torch.as_tensor(audio)
    if device is not None:
        audio = audio.to(device)
    elif not audio.is_cuda:
        audio = audio.to("cuda")                                       # host input and no device given: current GPU
    audio = audio.to(torch.float32)
    if audio.ndim == 1:
        audio = audio[None]
    if padding > 0:
        audio = torch.nn.functional.pad(audio, (0, padding))
    audio = audio.contiguous()
    window, fb = _tables(audio.device, sample_rate, n_fft, n_mels)
    b, L = audio.shape
    frames = L // hop_length
    out = torch.empty((b, frames, n_mels), dtype=torch.float32, device=audio.device)
    # one launch for the whole batch (the reference loops over it in Python, audio.py:195), on the current stream of the device
    # that holds the audio, with that device current (a launch on another device's stream would be a device mismatch)
    with torch.cuda.device(audio.device):
        stream = _eng.stream_ptr(audio.device)
        _eng.check(lib.f5_mel_spectrogram_batch(_eng.ptr(audio), b, C.c_int64(L), _eng.ptr(window), _eng.ptr(fb), n_fft, hop_length,
                                                n_mels, _eng.ptr(out), stream), "f5_mel_spectrogram_batch")
    return out


RESAMPLE_LPW = 6                     # zero crossings of the sinc kept on each side
RESAMPLE_ROLLOFF = 0.99              # cut-off as a fraction of the lower Nyquist frequency


def _rate(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value <= 0:
        raise ValueError(f"{name} must be a positive integer number of Hz (got {value!r})")
    return int(value)


def resample_taps64(orig: int, new: int):
    """The whole filter before rounding: (h fp64 [n][2 * width + o], o, n, width, base), as include/f5tts_hip.h states it --
    h[i][k] = sinc(pi t) cos^2(pi t / (2 lpw)) base / o, t = (-i / n + (k - width) / o) base, exactly 0 where |t| >= lpw."""
    orig, new = _rate(orig, "orig_sr"), _rate(new, "new_sr")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * RESAMPLE_ROLLOFF
    width = math.ceil(RESAMPLE_LPW * o / base)
    i = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(2 * width + o, dtype=np.float64)[None, :]
    t = (-i / n + (k - width) / o) * base
    inside = np.abs(t) < RESAMPLE_LPW
    a = np.where(t == 0.0, 1.0, np.pi * t)                           # sinc(0) = 1 without a 0 / 0
    sinc = np.where(t == 0.0, 1.0, np.sin(a) / a)
    h = sinc * np.cos(np.pi * t / (2 * RESAMPLE_LPW)) ** 2 * base / o
    return np.where(inside, h, 0.0), o, n, width, base


@lru_cache(maxsize=None)
def resample_table(orig: int, new: int):
    """-> (taps fp32 [T][n], first int32 [n], o, n, T, width): the compact table f5_resample_batch takes.  first[i] is the first
    non-zero tap of phase i, T the longest non-zero run of a phase, taps[t][i] = h[i][first[i] + t] (zero past the end of a run)."""
    h64, o, n, width, _ = resample_taps64(orig, new)
    h = h64.astype(np.float32)                                       # the one rounding
    nz = h != 0
    first = nz.argmax(axis=1).astype(np.int32)
    last = h.shape[1] - 1 - nz[:, ::-1].argmax(axis=1)
    T = int((last - first + 1).max())
    padded = np.concatenate([h, np.zeros((n, T), np.float32)], axis=1)
    taps = np.ascontiguousarray(padded[np.arange(n)[None, :], first[None, :] + np.arange(T)[:, None]])
    for a in (taps, first):
        a.setflags(write=False)                                      # cached: handed out to every caller
    return taps, first, o, n, T, width


_dev_resample = {}


def _resample_tables(device: torch.device, orig: int, new: int):
    key = (str(device), orig, new)
    if key not in _dev_resample:
        taps, first = resample_table(orig, new)[:2]
        _dev_resample[key] = (torch.from_numpy(taps.copy()).to(device), torch.from_numpy(first.copy()).to(device))
    return _dev_resample[key]


def resample(audio: torch.Tensor, orig_sr: int, new_sr: int, device=None) -> torch.Tensor:
    """audio: [t] or [b, t] at orig_sr Hz (device tensor or anything torch.as_tensor accepts) -> (b, ceil(t * new_sr / orig_sr)) float32
    on the GPU at new_sr Hz.  Hann-windowed sinc polyphase filter (include/f5tts_hip.h f5_resample_batch; figures: docs/resample.md).
    Equal rates hand the input back and an empty input an empty result, both without a launch.  ValueError for rates that are not
    positive integers and for a ratio the kernel refuses."""
    orig_sr, new_sr = _rate(orig_sr, "orig_sr"), _rate(new_sr, "new_sr")
    lib = _eng.load_library()
    audio = torch.as_tensor(audio)
    if device is not None:
        audio = audio.to(device)
    elif not audio.is_cuda:
        audio = audio.to("cuda")                                       # host input and no device given: current GPU
    audio = audio.to(torch.float32)
    if audio.ndim == 1:
        audio = audio[None]
    if orig_sr == new_sr:
        return audio
    audio = audio.contiguous()
    _, _, o, n, T, width = resample_table(orig_sr, new_sr)
    b, L = audio.shape
    L_out = -((-n * L) // o)
    out = torch.empty((b, L_out), dtype=torch.float32, device=audio.device)
    if L == 0:
        return out
    taps, first = _resample_tables(audio.device, orig_sr, new_sr)
    # one launch for the whole batch, on the current stream of the device that holds the audio (as log_mel_spectrogram)
    with torch.cuda.device(audio.device):
        stream = _eng.stream_ptr(audio.device)
        rc = lib.f5_resample_batch(_eng.ptr(audio), b, C.c_int64(L), _eng.ptr(taps), _eng.ptr(first), o, n, T, width, _eng.ptr(out),
                                   C.c_int64(L_out), stream)
    if rc != 0 and lib.f5_last_error().startswith(b"resample: ratio"):
        raise ValueError(lib.f5_last_error().decode("utf-8", "replace"))
    _eng.check(rc, "f5_resample_batch")
    return out


# ---- many recordings in one call (no reference counterpart: the reference's sample() takes a raw wave for batch 1 only) -----------
ENERGY_BLOCK = 240                   # samples per energy block of prepare_references: 10 ms at 24 kHz


def _padded_batch(waves, device):
    """[b, t] (or [t]) fp32, contiguous, on `device` (None: where it is, or the current GPU for host input)"""
    waves = torch.as_tensor(waves)
    if device is not None:
        waves = waves.to(device)
    elif not waves.is_cuda:
        waves = waves.to("cuda")
    waves = waves.to(torch.float32)
    if waves.ndim == 1:
        waves = waves[None]
    if waves.ndim != 2:
        raise ValueError(f"a padded batch of waveforms is [b, t], got {tuple(waves.shape)}")
    return waves.contiguous()


def _host_ints(values, B: int, name: str) -> list:
    out = [int(v) for v in (values.tolist() if isinstance(values, (torch.Tensor, np.ndarray)) else values)]
    if len(out) != B:
        raise ValueError(f"{name} must have one entry per row ({B}), got {len(out)}")
    return out


def block_energy(waves: torch.Tensor, lens, block: int = ENERGY_BLOCK, device=None) -> torch.Tensor:
    """waves [b, t] padded, lens (b,) sample counts -> (b, ceil(t / block)) fp32 on the GPU: energy[b][k] = sum of the squares of row
    b's samples in block k that lie below lens[b] (f5_wave_block_energy in include/f5tts_hip.h states the summation order; the padding
    is never read).  One launch, no synchronisation when `lens` is already an int32 tensor on the device."""
    lib = _eng.load_library()
    waves = _padded_batch(waves, device)
    B, L = waves.shape
    if isinstance(lens, torch.Tensor) and lens.is_cuda and lens.dtype == torch.int32 and lens.shape == (B,):
        lens_dev = lens.contiguous()
    else:
        host = _host_ints(lens, B, "lens")
        for b, n in enumerate(host):
            if not 0 <= n <= L:
                raise ValueError(f"lens[{b}] = {n} outside 0..{L}")
        lens_dev = torch.tensor(host, dtype=torch.int32).to(waves.device)
    block = int(block)
    nblk = -(-L // block) if block > 0 else 0
    energy = torch.empty((B, nblk), dtype=torch.float32, device=waves.device)
    with torch.cuda.device(waves.device):
        rc = lib.f5_wave_block_energy(_eng.ptr(waves), B, L, _eng.ptr(lens_dev), block, _eng.ptr(energy), nblk, _eng.stream_ptr(waves.device))
    if rc != 0 and lib.f5_last_error().startswith(b"block_energy: block"):
        raise ValueError(lib.f5_last_error().decode("utf-8", "replace"))
    _eng.check(rc, "f5_wave_block_energy")
    return energy


def log_mel_spectrogram_ragged(waves: torch.Tensor, lens, begin=None, gain=None, sample_rate: int = 24_000, n_mels: int = 100,
                               n_fft: int = 1024, hop_length: int = 256, device=None) -> torch.Tensor:
    """waves [b, t] padded; row i is the recording waves[i, begin[i] : begin[i] + lens[i]] (begin: zeros when None), scaled by gain[i]
    (fp32; None: not scaled at all).  -> (b, N, n_mels) fp32 on the GPU, N = the largest lens[i] // hop_length: the frames of row i
    are the bits log_mel_spectrogram gives for a contiguous copy of gain[i] * slice, the frames past its own count exactly 0 -- the
    zero padding sample() gives the conditioning.  One launch (f5_mel_spectrogram_ragged).  `lens` and `begin`
    are host values (lists, arrays or CPU tensors): N comes from them, and they are checked against the row here."""
    lib = _eng.load_library()
    waves = _padded_batch(waves, device)
    B, L = waves.shape
    lens_h = _host_ints(lens, B, "lens")
    begin_h = [0] * B if begin is None else _host_ints(begin, B, "begin")
    for b in range(B):
        if begin_h[b] < 0 or lens_h[b] < 0 or begin_h[b] + lens_h[b] > L:
            raise ValueError(f"row {b}: samples [{begin_h[b]}, {begin_h[b] + lens_h[b]}) lie outside the row of {L}")
    N = max(n // hop_length for n in lens_h)                          # so that every row's frames fit: the kernel cannot check that
    out = torch.empty((B, N, n_mels), dtype=torch.float32, device=waves.device)
    if N == 0:
        return out
    window, fb = _tables(waves.device, sample_rate, n_fft, n_mels)
    table = torch.tensor([begin_h, lens_h], dtype=torch.int32).to(waves.device)
    gain_dev = None
    if gain is not None:
        gain_dev = torch.as_tensor(np.asarray(gain.cpu() if isinstance(gain, torch.Tensor) else gain, dtype=np.float32)).reshape(-1).to(waves.device)
        if gain_dev.numel() != B:
            raise ValueError(f"gain must have one entry per row ({B}), got {gain_dev.numel()}")
    with torch.cuda.device(waves.device):
        _eng.check(lib.f5_mel_spectrogram_ragged(_eng.ptr(waves), B, L, _eng.ptr(table[0]), _eng.ptr(table[1]), _eng.ptr(gain_dev),
                                                 _eng.ptr(window), _eng.ptr(fb), n_fft, hop_length, n_mels, _eng.ptr(out), N,
                                                 _eng.stream_ptr(waves.device)), "f5_mel_spectrogram_ragged")
    return out


def silence_window(energy, lens, block: int, threshold_db: float, keep_blocks: int):
    """The part of each recording between its first and its last loud block, `keep_blocks` blocks of margin on either side: host
    arithmetic in fp64 on the table block_energy made, no GPU.  energy (b, nblk), lens (b,) sample counts -> (begin, length), two
    lists of sample counts.  The level of block k is 10 log10(E_k / n_k), n_k = the samples of the row in that block (-inf for
    E_k = 0); a block is loud when its level is above threshold_db.  begin = max(0, first_loud - keep_blocks) block, end =
    min(row's block count, last_loud + 1 + keep_blocks) block, length = min(end, lens) - begin.  The kept samples are the recording's
    own: no synthetic silence is added.  ValueError for a row without a loud block."""
    e = np.asarray(energy.cpu() if isinstance(energy, torch.Tensor) else energy, dtype=np.float64)
    if e.ndim == 1:
        e = e[None]
    B = e.shape[0]
    lens = _host_ints(lens, B, "lens")
    block, keep_blocks = int(block), int(keep_blocks)
    if block < 1 or keep_blocks < 0:
        raise ValueError(f"block must be >= 1 and keep_blocks >= 0 (got {block}, {keep_blocks})")
    begin, length = [], []
    for b in range(B):
        nb = -(-lens[b] // block)
        if nb > e.shape[1]:
            raise ValueError(f"row {b}: {lens[b]} samples need {nb} blocks of {block}, the table has {e.shape[1]}")
        k = np.arange(nb)
        n_k = np.minimum((k + 1) * block, lens[b]) - k * block
        with np.errstate(divide="ignore"):
            level = 10.0 * np.log10(e[b, :nb] / n_k)
        loud = np.nonzero(level > threshold_db)[0]
        if loud.size == 0:
            raise ValueError(f"row {b}: no block of {block} samples is louder than {threshold_db} dB: nothing to keep")
        b_blk = max(0, int(loud[0]) - keep_blocks)
        e_blk = min(nb, int(loud[-1]) + 1 + keep_blocks)
        begin.append(b_blk * block)
        length.append(min(e_blk * block, lens[b]) - b_blk * block)
    return begin, length


def reference_gain(energy, begin, length, block: int, target_rms: float = 0.1) -> np.ndarray:
    """The level rule of generate() (generate.py:154-156: a quiet reference is scaled UP to target_rms, a loud one is left alone) on
    the block energies: host fp64.  Mean square of row b = the energies of its kept blocks, added in increasing k, over length[b];
    gain = float32(target_rms / rms) when rms < target_rms, else 1.0.  -> (b,) float32.  `begin` must be whole blocks and
    begin + length end on a block boundary or at the row's end, which is what silence_window returns (and begin = 0, length = lens).
    ValueError for rms = 0 (generate() would divide by it)."""
    e = np.asarray(energy.cpu() if isinstance(energy, torch.Tensor) else energy, dtype=np.float64)
    if e.ndim == 1:
        e = e[None]
    B = e.shape[0]
    begin, length = _host_ints(begin, B, "begin"), _host_ints(length, B, "length")
    block = int(block)
    gain = np.ones(B, dtype=np.float32)
    for b in range(B):
        if begin[b] % block:
            raise ValueError(f"row {b}: begin = {begin[b]} is not a whole number of blocks of {block}")
        k0, k1 = begin[b] // block, -(-(begin[b] + length[b]) // block)
        if length[b] <= 0 or k1 > e.shape[1]:
            raise ValueError(f"row {b}: samples [{begin[b]}, {begin[b] + length[b]}) are empty or beyond the energy table")
        total = 0.0
        for v in e[b, k0:k1].tolist():                                 # increasing k, one fp64 addition each
            total += v
        rms = math.sqrt(total / length[b])
        if rms == 0.0:
            raise ValueError(f"row {b}: the kept samples are all zero (rms 0): no level to normalise")
        if rms < target_rms:
            gain[b] = np.float32(target_rms / rms)
    return gain


class References:
    """What prepare_references hands back.  mel (b, N, n_mels) fp32 on the device, row i zero past frames[i]; frames: mel frames per
    row; samples: kept samples per row at 24 kHz (what a generated wave is trimmed by); begin: first kept sample per row; gain:
    float32 (b,) level factors."""

    def __init__(self, mel, frames, samples, begin, gain):
        self.mel, self.frames, self.samples, self.begin, self.gain = mel, frames, samples, begin, gain


def prepare_references(waves, sample_rates=24_000, *, trim_silence_db: Optional[float] = None, keep_ms: float = 50, target_rms: float = 0.1,
                       device=None) -> References:
    """Reference recordings of different lengths, sample rates and levels -> the conditioning of a ragged sample() batch.
    waves: a list of 1-D arrays / tensors; sample_rates: one int or one per row.  A row at another rate than 24 kHz goes through
    `resample` by itself (its table depends on the rate); the rows are written into one padded buffer; ONE block_energy launch
    (blocks of 240 samples = 10 ms) and ONE device-to-host copy of its table -- the only synchronisation -- give the host what the
    silence window and the gain are computed from; ONE ragged mel launch follows.
    trim_silence_db (default None: nothing is cut): leading and trailing silence below this level is cut (silence_window), keeping
    keep_ms of margin on either side; -42 is the customary figure for edge trimming in the PyTorch F5-TTS front end.  The gain
    (reference_gain: only scales up, to target_rms) is computed always, over the kept samples.
    ValueError names the row: a ratio the resampler refuses, a row without a loud block, an all-zero row, a row that keeps fewer
    than one frame of 256 samples."""
    SR, hop_length = 24_000, 256
    waves = list(waves)
    B = len(waves)
    if B == 0:
        raise ValueError("prepare_references needs at least one recording")
    rates = [sample_rates] * B if isinstance(sample_rates, (int, np.integer)) and not isinstance(sample_rates, bool) else list(sample_rates)
    if len(rates) != B:
        raise ValueError(f"sample_rates must be one int or one per recording ({B}), got {len(rates)}")
    rates = [_rate(r, f"sample rate of row {i}") for i, r in enumerate(rates)]
    rows = []
    for i, w in enumerate(waves):
        w = torch.as_tensor(w)
        if w.ndim != 1:
            raise ValueError(f"row {i}: a recording is 1-D (mono), got {tuple(w.shape)}")
        if rates[i] != SR:
            try:
                w = resample(w, rates[i], SR, device=device)[0]
            except ValueError as exc:
                raise ValueError(f"row {i}: {exc}") from None
        rows.append(_padded_batch(w, device)[0])
    dev = rows[0].device
    lens = [int(r.shape[0]) for r in rows]
    buf = torch.zeros((B, max(max(lens), 1)), dtype=torch.float32, device=dev)
    for i, r in enumerate(rows):
        buf[i, :lens[i]] = r.to(dev)
    energy = block_energy(buf, lens, ENERGY_BLOCK).cpu().numpy()       # the one synchronisation
    if trim_silence_db is not None:
        begin, length = silence_window(energy, lens, ENERGY_BLOCK, float(trim_silence_db), int(round(keep_ms * SR / 1000.0 / ENERGY_BLOCK)))
    else:
        begin, length = [0] * B, list(lens)
    for i in range(B):
        if length[i] < hop_length:
            raise ValueError(f"row {i}: {length[i]} samples are kept, fewer than one frame of {hop_length}")
    gain = reference_gain(energy, begin, length, ENERGY_BLOCK, target_rms)
    mel = log_mel_spectrogram_ragged(buf, length, begin, gain, sample_rate=SR, hop_length=hop_length)
    return References(mel, [n // hop_length for n in length], length, begin, gain)


# ---- sentence joins (no reference counterpart; docs/sentence_joins.md): the back half of generate() / generate_many() ---------------
JOIN_SEG_MAX = 64                    # f5_wave_join: segments per output row
JOIN_SAMPLE_RATE = 24_000            # the model's rate: what the millisecond arguments of join_rows are counted in


def _per_request(value, Q: int, name: str) -> list:
    """one value for every request, or one per request -> a list of Q"""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != Q:
            raise ValueError(f"{name} must be one value or one per request ({Q}), got {len(value)}")
        return list(value)
    return [value] * Q


def join_layout(begin, length, row_req, *, fade, gap):
    """Where the sentences of every request go: pure integer arithmetic, no GPU.  Row r of the decoded batch holds a sentence at samples
    [begin[r], begin[r] + length[r]) and belongs to request row_req[r]; `fade` and `gap` are sample counts, one for all requests or one
    per request.  Per request, in row order, the first segment sits at 0.  For consecutive sentences a and b:
    F = min(fade, len_a // 2, len_b // 2) -- a very short sentence shortens its own fades and does not raise --, fade_out[a] =
    fade_in[b] = F; with gap == 0 they overlap by F, dst_begin[b] = dst_end[a] - F (a cross-fade), with gap > 0 they do not,
    dst_begin[b] = dst_end[a] + gap (a fade to silence, the pause, a fade from silence).  The first sentence's head and the last one's
    tail are not faded.  -> (table int32 [Q][S][6] for f5_wave_join, out_lens: samples per request, Lout = the longest); Q = the largest
    request number + 1, S = the most sentences of a request, shorter requests pad with empty entries."""
    R = len(row_req)
    begin, length = _host_ints(begin, R, "begin"), _host_ints(length, R, "length")
    row_req = [int(q) for q in row_req]
    if R == 0 or min(row_req) < 0:
        raise ValueError("join_layout needs at least one row, and request numbers from 0")
    Q = max(row_req) + 1
    fade = [int(f) for f in _per_request(fade, Q, "fade")]
    gap = [int(g) for g in _per_request(gap, Q, "gap")]
    for r in range(R):
        if begin[r] < 0 or length[r] < 0:
            raise ValueError(f"row {r}: begin = {begin[r]} and length = {length[r]} must not be negative")
    if min(fade) < 0 or min(gap) < 0:
        raise ValueError(f"fade and gap must not be negative (got {fade}, {gap})")
    rows = [[r for r in range(R) if row_req[r] == q] for q in range(Q)]
    S = max(len(rs) for rs in rows)
    if S > JOIN_SEG_MAX:
        raise ValueError(f"a request of {S} sentences exceeds the {JOIN_SEG_MAX} segments of a row of f5_wave_join")
    table = np.zeros((Q, S, 6), dtype=np.int64)
    out_lens = []
    for q, rs in enumerate(rows):
        at = 0                                                         # where the previous sentence ended
        for k, r in enumerate(rs):
            F = 0
            if k > 0:
                F = min(fade[q], length[rs[k - 1]] // 2, length[r] // 2)
                table[q, k - 1, 5] = F
                at = at - F if gap[q] == 0 else at + gap[q]
            table[q, k] = (at, r, begin[r], length[r], F, 0)
            at += length[r]
        out_lens.append(at)
    if table.max(initial=0) > 2 ** 31 - 1:
        raise ValueError("the joined waves exceed 2^31 - 1 samples")
    return table.astype(np.int32), out_lens, max(out_lens)


def sentence_windows(energy, begin, length, block: int, threshold_db: float, keep_blocks: int):
    """Edge trim of generated sentences: silence_window's rule on the part of each decoded row that follows its reference.  energy
    (r, nblk): the block energies of the rows with lens = begin + length, blocks aligned at sample 0.  Only whole blocks that start at
    or after begin[r] are candidates -- the reference part never is, and neither is the block begin[r] falls into.  The kept window is
    [max(begin, (first_loud - keep_blocks) block), min(begin + length, (last_loud + 1 + keep_blocks) block)).  A row with no loud
    block keeps its whole range: a silent sentence must not abort a finished batch.  Host fp64, no GPU -> (begin, length)."""
    e = np.asarray(energy.cpu() if isinstance(energy, torch.Tensor) else energy, dtype=np.float64)
    if e.ndim == 1:
        e = e[None]
    R = e.shape[0]
    begin, length = _host_ints(begin, R, "begin"), _host_ints(length, R, "length")
    block, keep_blocks = int(block), int(keep_blocks)
    if block < 1 or keep_blocks < 0:
        raise ValueError(f"block must be >= 1 and keep_blocks >= 0 (got {block}, {keep_blocks})")
    out_b, out_n = [], []
    for r in range(R):
        end = begin[r] + length[r]
        k0, nb = -(-begin[r] // block), -(-end // block)
        if nb > e.shape[1]:
            raise ValueError(f"row {r}: {end} samples need {nb} blocks of {block}, the table has {e.shape[1]}")
        k = np.arange(k0, max(nb, k0))
        n_k = np.minimum((k + 1) * block, end) - k * block
        with np.errstate(divide="ignore", invalid="ignore"):
            level = 10.0 * np.log10(e[r, k0:max(nb, k0)] / n_k)
        loud = k[np.nonzero(level > threshold_db)[0]]
        lo, hi = begin[r], end
        if loud.size:
            lo = max(lo, (int(loud[0]) - keep_blocks) * block)
            hi = min(hi, (int(loud[-1]) + 1 + keep_blocks) * block)
        out_b.append(lo)
        out_n.append(hi - lo)
    return out_b, out_n


def _ms_to_samples(ms) -> int:
    return int(round(float(ms) * JOIN_SAMPLE_RATE / 1000.0))


def wave_join(src: torch.Tensor, table, Lout: int) -> torch.Tensor:
    """src [R, Ls] fp32 on the GPU, table int32 (Q, S, 6) on the host (join_layout) -> (Q, Lout): f5_wave_join, one call, no
    synchronisation.  The library refuses a bad table (ValueError here)."""
    lib = _eng.load_library()
    src = _padded_batch(src, None)
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    if table.ndim != 3 or table.shape[2] != 6:
        raise ValueError(f"a join table is (Q, S, 6), got {table.shape}")
    Q, S = table.shape[:2]
    R, Ls = src.shape
    out = torch.empty((Q, int(Lout)), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        rc = lib.f5_wave_join(_eng.ptr(src), R, C.c_int64(Ls), table.ctypes.data_as(C.c_void_p), Q, S, _eng.ptr(out), C.c_int64(int(Lout)),
                              _eng.stream_ptr(src.device))
    if rc != 0 and lib.f5_last_error().startswith(b"wave_join:"):
        raise ValueError(lib.f5_last_error().decode("utf-8", "replace"))
    _eng.check(rc, "f5_wave_join")
    return out


def join_rows(decoded, begin, length, row_req, *, cross_fade_ms=0, pause_ms=0, trim_db=None, keep_ms: float = 50):
    """The decoded rows of a ragged batch -> one wave per request.  decoded [R, Ls] on the GPU; row r holds a sentence of request
    row_req[r] at samples [begin[r], begin[r] + length[r]) (begin = its reference's samples).  cross_fade_ms, pause_ms and trim_db are
    one value for all requests or one per request (None = 0 / no trim for that request).
    With a trim_db: ONE block_energy launch on the decoded rows (blocks of 240 samples aligned at 0, lens = begin + length) and ONE
    copy of its table to the host -- the only synchronisation --, then sentence_windows cuts leading and trailing near-silence below
    trim_db off every sentence of the requests that ask for it, keeping keep_ms of margin.  Without one: no energy launch and no
    synchronisation.  Then join_layout (host integers) and ONE f5_wave_join launch.
    -> (waves (Q, Lout) fp32, exactly 0.0 past each request's length; out_lens).  With cross_fade_ms = 0, no pause and no trim row q
    is torch.cat of its sentences' slices, bit for bit."""
    decoded = _padded_batch(decoded, None)
    R = decoded.shape[0]
    begin, length = _host_ints(begin, R, "begin"), _host_ints(length, R, "length")
    row_req = [int(q) for q in row_req]
    if len(row_req) != R:
        raise ValueError(f"row_req must have one entry per row ({R}), got {len(row_req)}")
    for r in range(R):
        if begin[r] < 0 or length[r] < 0 or begin[r] + length[r] > decoded.shape[1]:
            raise ValueError(f"row {r}: samples [{begin[r]}, {begin[r] + length[r]}) lie outside the row of {decoded.shape[1]}")
    Q = max(row_req) + 1
    fade = [_ms_to_samples(v or 0) for v in _per_request(cross_fade_ms, Q, "cross_fade_ms")]
    gap = [_ms_to_samples(v or 0) for v in _per_request(pause_ms, Q, "pause_ms")]
    trim = _per_request(trim_db, Q, "trim_db")
    if any(t is not None for t in trim):
        lens = [b + n for b, n in zip(begin, length)]
        energy = block_energy(decoded, lens, ENERGY_BLOCK).cpu().numpy()   # the one synchronisation
        keep = int(round(keep_ms * JOIN_SAMPLE_RATE / 1000.0 / ENERGY_BLOCK))
        for q in range(Q):
            if trim[q] is None:
                continue
            rs = [r for r in range(R) if row_req[r] == q]
            b, n = sentence_windows(energy[rs], [begin[r] for r in rs], [length[r] for r in rs], ENERGY_BLOCK, float(trim[q]), keep)
            for i, r in enumerate(rs):
                begin[r], length[r] = b[i], n[i]
    table, out_lens, Lout = join_layout(begin, length, row_req, fade=fade, gap=gap)
    return wave_join(decoded, table, Lout), out_lens


def resample_rows(waves: torch.Tensor, lens, orig_sr: int, new_sr: int) -> list:
    """waves (Q, L) padded with EXACT zeros past lens[q] -> a list of Q waves at new_sr, from ONE f5_resample_batch call on the padded
    batch, each sliced to ceil(n lens[q] / o).  The bits of resample() on each waves[q, :lens[q]] by itself: the filter treats
    everything outside [0, L) as zero, the padding is zero, and an output sample's taps and their order depend on its index alone."""
    orig_sr, new_sr = _rate(orig_sr, "orig_sr"), _rate(new_sr, "new_sr")
    lens = _host_ints(lens, waves.shape[0], "lens")
    if orig_sr == new_sr:
        return [waves[q, :lens[q]] for q in range(len(lens))]
    _, _, o, n, _, _ = resample_table(orig_sr, new_sr)
    out = resample(waves, orig_sr, new_sr)
    return [out[q, :-((-n * lens[q]) // o)] for q in range(len(lens))]


def check_resample_ratio(orig_sr: int, new_sr: int) -> None:
    """ValueError when `resample` would refuse the pair of rates, without a launch and without a device: the library's own rule, asked
    through a call of length 0 (which checks everything and reads nothing)."""
    orig_sr, new_sr = _rate(orig_sr, "orig_sr"), _rate(new_sr, "new_sr")
    if orig_sr == new_sr:
        return
    lib = _eng.load_library()
    taps, first, o, n, T, width = resample_table(orig_sr, new_sr)
    p = C.c_void_p(taps.ctypes.data)                                   # any non-null address: nothing is read at length 0
    rc = lib.f5_resample_batch(p, 1, C.c_int64(0), p, C.c_void_p(first.ctypes.data), o, n, T, width, p, C.c_int64(0), C.c_void_p(0))
    if rc != 0:
        raise ValueError(lib.f5_last_error().decode("utf-8", "replace"))


class MelSpec:
    """audio.py:213-230.  Extension: `lens` (sample counts per row of a padded [b, t] batch) gives the ragged mel, each row on its own
    samples and zero past its own frames (log_mel_spectrogram_ragged); without it the call is the reference's."""

    def __init__(self, sample_rate=24_000, n_fft=1024, hop_length=256, n_mels=100, device=None):
        self.device = device                # where host audio is moved to (the owning model's device); None = current GPU
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.n_mels = n_mels

    def __call__(self, audio, lens=None, **kwargs) -> torch.Tensor:
        if lens is not None:
            return log_mel_spectrogram_ragged(audio, lens, sample_rate=self.sample_rate, n_mels=self.n_mels, n_fft=self.n_fft,
                                              hop_length=self.hop_length, device=self.device)
        return log_mel_spectrogram(audio, sample_rate=self.sample_rate, n_mels=self.n_mels, n_fft=self.n_fft,
                                   hop_length=self.hop_length, device=self.device)
