"""The ragged reference front end (csrc/audio.hip block_energy_kernel / mel_ragged_kernel behind f5_wave_block_energy and
f5_mel_spectrogram_ragged): case data, an emulation of both kernels on the CPU (right, and wrong on request), and the checkers.

Shared by tests/test_multivoice_gpu.py (runs the checkers over the kernels' results) and tests/test_multivoice_host.py (runs them over
the emulation and shows every seeded mistake flagged).  Nothing here needs a GPU or the library.

Bounds.  Block energy: all terms are non-negative and each of the at most `block` accumulation steps rounds once, so in ANY order
|E^ - E| <= 1.01 block 2^-24 E against the fp64 sum of the same fp32 samples.  Ragged mel: bit equality with the plain mel of a
contiguous copy of gain x slice, exact zeros past a row's frames, and tests/convaudio_matrix.py's interval (chk_mel) on the valid frames.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import convaudio_matrix as CM
from rowops_matrix import Case, bits

U = 2.0 ** -24
NFFT = 1024
ENERGY_BUGS = ("reads_past_lens", "partial_block_whole")
MEL_BUGS = ("reads_past_lens", "begin_ignored", "floor_past_frames", "gain_after_window")


# ---- block energy -----------------------------------------------------------------------------------------------------------------
def energy_lens(L, block):
    """the rows of a case: the whole row, an empty one, one that ends in the middle of a block (clipped to the row)"""
    return [L, 0, min(L, max(1, (L // block) * block - block // 2 if L > block else L // 2))]


def energy_wave(r, B, L, lens, pad=float("nan")):
    """fp32 rows with `pad` (NaN by default; a finite one at the row's level) at and past lens[b]; the levels of the rows differ by 1e2"""
    w = torch.from_numpy(r.standard_normal((B, L)).astype(np.float32)) * (1.0e2 ** torch.arange(B, dtype=torch.float32)).reshape(B, 1)
    for b in range(B):
        w[b, lens[b]:] = pad * 1.0e2 ** b
    return w


def emu_block_energy(wave, lens, block, bug=None):
    """the kernel's sum in its own order: lane l adds the squares of samples l, l + 64, ... of a block, an xor butterfly joins the lanes
    (fp32 throughout; the fused multiply-add is restated as the fp64 expression rounded once, exact but for double rounding)"""
    B, L = wave.shape
    nblk = -(-L // block)
    out = np.zeros((B, nblk), np.float32)
    w = wave.numpy()
    for b in range(B):
        n = L if bug == "reads_past_lens" else min(max(int(lens[b]), 0), L)
        for k in range(nblk):
            s0, s1 = k * block, min((k + 1) * block, n)
            if bug == "partial_block_whole" and s0 < n:
                s1 = min((k + 1) * block, L)
            lane = np.zeros(64, np.float32)
            for s in range(s0, max(s0, s1)):
                x = np.float64(w[b, s])
                lane[(s - s0) % 64] = np.float32(x * x + np.float64(lane[(s - s0) % 64]))
            d = 32
            while d >= 1:
                lane = (lane + lane[np.arange(64) ^ d]).astype(np.float32)
                d >>= 1
            out[b, k] = lane[0]
    return torch.from_numpy(out)


def chk_block_energy(wave, lens, block, got):
    """got [B][nblk] against fp64 sums of the same fp32 samples below lens[b]; blocks past lens exactly +0.0"""
    B, L = wave.shape
    nblk = -(-L // block)
    bad = []
    if tuple(got.shape) != (B, nblk):
        return [f"shape {tuple(got.shape)}, expected {(B, nblk)}"]
    w = wave.double()
    for b in range(B):
        n = int(lens[b])
        for k in range(nblk):
            s0, s1 = k * block, min((k + 1) * block, n)
            g = got[b, k]
            if s1 <= s0:
                if int(bits(g.reshape(1))[0]) != 0:
                    bad.append(f"row {b} block {k}: past lens, got {float(g)!r} instead of exactly 0")
                continue
            E = float((w[b, s0:s1] ** 2).sum())
            if not abs(float(g) - E) <= 1.01 * block * U * E:                      # (NaN fails)
                bad.append(f"row {b} block {k}: got {float(g)!r}, want {E!r} within {1.01 * block * U * E:.3e}")
    return bad


# ---- ragged mel -------------------------------------------------------------------------------------------------------------------
MEL_L = 5 * 256 + 3


def mel_rows(hop, L=MEL_L):
    """(begin, len) per row: the whole row, a slice in the middle, a slice at the end too short for a frame, one of exactly one frame"""
    return [(0, L), (17, 1025), (L - 255, 255), (0, hop)]


def mel_wave(r, rows, L=MEL_L, pad=float("nan")):
    """fp32 [B][L]: seeded noise inside each row's slice, `pad` everywhere outside it"""
    w = torch.full((len(rows), L), pad, dtype=torch.float32)
    for b, (b0, n) in enumerate(rows):
        w[b, b0:b0 + n] = torch.from_numpy((r.standard_normal(n) * 0.1 * (b + 1)).astype(np.float32))
    return w


MEL_GAINS = (1.0, 1.7, 0.3, 2.0)                           # 1.0, two that are no power of two, one that is


def scaled_slice(wave, b, begin, n, gain):
    """the contiguous copy the plain mel is run on: slice x gain, ONE fp32 rounding (no product without a gain)"""
    x = wave[b, begin:begin + n].clone()
    return x if gain is None else (x * torch.tensor(gain[b], dtype=torch.float32))


def _emu_mel_of_windowed(xw, fb):
    """[frames][1024] fp32 windowed frames -> [frames][n_mels] fp32, the rest of the frame body in fp64"""
    acc = torch.fft.rfft(xw.double(), dim=-1).abs() @ fb.double().T
    return torch.log(acc.clamp_min(CM.LOG_FLOOR)).float()


def _frames_of(x, hop, nframes):
    """[nframes][1024] fp32: zero-padded centred frames of the fp32 recording x"""
    p = torch.cat([torch.zeros(NFFT // 2), x, torch.zeros(NFFT)])
    return torch.stack([p[f * hop:f * hop + NFFT] for f in range(nframes)]) if nframes else torch.zeros((0, NFFT))


def emu_mel_plain(x, window, fb, hop):
    """the plain mel of one contiguous fp32 recording: fp32 x * window (one rounding), then fp64"""
    return _emu_mel_of_windowed(_frames_of(x, hop, x.numel() // hop) * window, fb)


def emu_mel_ragged(wave, rows, gain, window, fb, hop, N, bug=None):
    B, L = wave.shape
    out = torch.zeros((B, N, fb.shape[0]), dtype=torch.float32)
    if bug == "floor_past_frames":
        out[:] = math.log(CM.LOG_FLOOR)
    for b, (b0, n) in enumerate(rows):
        F = n // hop
        if F == 0:
            continue
        begin = 0 if bug == "begin_ignored" else b0
        x = wave[b, begin:(L if bug == "reads_past_lens" else begin + n)]
        g = None if gain is None else torch.tensor(gain[b], dtype=torch.float32)
        if bug == "gain_after_window" and g is not None:
            xw = (_frames_of(x, hop, F) * window) * g                               # two roundings in the other order
        else:
            xw = _frames_of(x if g is None else x * g, hop, F) * window
        out[b, :F] = _emu_mel_of_windowed(xw, fb)
    return out


def chk_mel_ragged(got, plain, rows, hop, N):
    """got [B][N][n_mels] against `plain`, the plain mel of each row's scaled contiguous copy ([F_b][n_mels], or None without a frame):
    the same bits on the valid frames, exactly +0.0 past them"""
    bad = []
    if got.shape[0] != len(rows) or got.shape[1] != N:
        return [f"shape {tuple(got.shape)}, expected ({len(rows)}, {N}, .)"]
    for b, (_, n) in enumerate(rows):
        F = n // hop
        if F and not torch.equal(bits(got[b, :F].contiguous()), bits(plain[b].contiguous())):
            diff = bits(got[b, :F].contiguous()) != bits(plain[b].contiguous())
            bad.append(f"row {b}: {int(diff.sum())} of {diff.numel()} values are not the bits of the plain mel of its slice")
        if bits(got[b, F:].contiguous()).any():
            bad.append(f"row {b}: {int((bits(got[b, F:].contiguous()) != 0).sum())} values past its {F} frames are not exactly 0")
    return bad


def chk_mel_interval(got, wave, rows, gain, window, fb, hop):
    """the fp64 interval of convaudio_matrix.chk_mel on every row's valid frames (the row as a one-element batch of that checker)"""
    bad = []
    for b, (b0, n) in enumerate(rows):
        F = n // hop
        if F == 0:
            continue
        x = scaled_slice(wave, b, b0, n, gain)[None]
        c = Case("mel", L=n, hop=hop, n_mels=int(fb.shape[0]), B=1, sig="noise", row=b)
        bad += [f"row {b}: {m}" for m in CM.chk_mel(c, "bf16", dict(wave=x, window=window, fb=fb), dict(out=got[b:b + 1, :F].contiguous()))]
    return bad
