"""The resampler test matrix (csrc/audio.hip resample_kernel behind f5_resample_batch): the filter restated in fp64, case generator,
guarded buffers, derived bound, checker.

Shared by tests/test_resample_gpu.py (runs the cases through the C ABI) and tests/test_resample_host.py (runs the checker over a
numpy fp32 emulation of the kernel, right and deliberately wrong, and holds the filter itself to its figures, on the CPU).  Nothing
here needs a GPU or the library, and nothing here imports f5_tts_mlx_amd: the filter below is written from its definition, with
`math` scalar functions per coefficient and a loop over the output samples, so that audio.resample_table (numpy, vectorised) has an
independent statement to be held against.

The filter.  g = gcd(orig, new), o = orig / g, n = new / g, lpw = 6, rolloff = 0.99, base = min(o, n) rolloff,
width = ceil(lpw o / base).  Phase i = 0 .. n - 1, tap k = 0 .. 2 width + o - 1:
    t = (-i / n + (k - width) / o) base;   h[i][k] = 0 where |t| >= lpw, else sinc(pi t) cos^2(pi t / (2 lpw)) base / o
in fp64, rounded once to fp32.  out[j n + i] = sum_k h[i][k] x[j o + k - width], x = 0 outside [0, L), L_out = ceil(n L / o).

The bound.  The reference sums the fp32-ROUNDED table widened back to fp64, so the rounding of the coefficients cancels and what
is left is the kernel's own arithmetic: T_i non-zero products accumulated in fp32, in any order, fused or not -- the classical bound
of a T_i-term dot product, gamma = T_i u / (1 - T_i u) with u = 2^-24, times sum_k |h[i][k] x[.]|.  (The fp64 sum of the reference
errs by at most T_i 2^-53 of the same sum, which is added.)  Nothing in it is measured.  A sum of magnitudes of zero leaves a bound
of zero: such an output must be exactly zero.  The signals keep |x| >= 2^-20 where they are not zero, so no product underflows.
"""
from __future__ import annotations

import math
import zlib
from functools import lru_cache

import numpy as np
import torch

LPW = 6
ROLLOFF = 0.99
U = 2.0 ** -24
GUARD = 64
SENT32 = 0x7FC0BEEF          # an fp32 NaN with a payload: guard bands and the not yet written output
TILE = 1024                  # outputs per workgroup of resample_kernel: a power of two, so the 256 m edges below cover it
ROW_GAIN = (1.0, -0.5, 2.0)  # rows of a batch differ (exactly: powers of two), so a row answered with another row's result shows
SIGNALS = ("noise", "impulse_first", "impulse_last", "ones")
BATCHES = (1, 3)

PAIRS = ((16_000, 24_000), (8_000, 24_000), (48_000, 24_000), (32_000, 24_000), (44_100, 24_000), (22_050, 24_000),
         (11_025, 24_000), (24_000, 16_000), (24_000, 48_000), (24_000, 44_100), (24_000, 22_050))


def cdiv(a, b):
    return -(-a // b)


# ---- the filter, from its definition -------------------------------------------------------------------------------------------
class Table:
    """h64 [n][K] the coefficients before rounding, h32 after; k0[i] / k1[i] the first non-zero tap of phase i and one past the last
    (of the ROUNDED table: what the kernel is handed), Ti[i] the number of non-zero taps"""


@lru_cache(maxsize=None)
def table(orig: int, new: int) -> Table:
    g = math.gcd(orig, new)
    tb = Table()
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LPW * o / base)
    K = 2 * width + o
    rows = []
    for i in range(n):
        row = []
        for k in range(K):
            t = (-i / n + (k - width) / o) * base
            if abs(t) >= LPW:
                row.append(0.0)
                continue
            a = math.pi * t
            sinc = 1.0 if t == 0.0 else math.sin(a) / a
            c = math.cos(math.pi * t / (2 * LPW))
            row.append(sinc * (c * c) * base / o)
        rows.append(row)
    tb.orig, tb.new, tb.o, tb.n, tb.base, tb.width, tb.K = orig, new, o, n, base, width, K
    tb.h64 = np.array(rows, dtype=np.float64)
    tb.h32 = tb.h64.astype(np.float32)
    tb.k0, tb.k1, tb.Ti = [], [], []
    for i in range(n):
        nz = [k for k in range(K) if tb.h32[i, k] != 0.0]
        tb.k0.append(nz[0])
        tb.k1.append(nz[-1] + 1)
        tb.Ti.append(len(nz))
    tb.T = max(b - a for a, b in zip(tb.k0, tb.k1))
    return tb


def compact(tb: Table):
    """-> (taps fp32 [T][n], first int32 [n], T): the form the kernel takes, built from the table above"""
    taps = np.zeros((tb.T, tb.n), dtype=np.float32)
    for i in range(tb.n):
        run = tb.h32[i, tb.k0[i]:tb.k1[i]]
        taps[:len(run), i] = run
    return taps, np.array(tb.k0, dtype=np.int32), tb.T


def out_len(tb: Table, L: int) -> int:
    return cdiv(tb.n * L, tb.o)


def apply64(tb: Table, h: np.ndarray, x: np.ndarray):
    """x fp64 [B][L] through the filter h [n][K] (fp64): -> (out [B][L_out], sum of the magnitudes of the products [B][L_out]);
    one output sample after the other"""
    B, L = x.shape
    Lo = out_len(tb, L)
    out, mag = np.zeros((B, Lo)), np.zeros((B, Lo))
    ax, ah = np.abs(x), np.abs(h)
    o, n, w = tb.o, tb.n, tb.width
    for p in range(Lo):
        j, i = divmod(p, n)
        ka, kb = tb.k0[i], tb.k1[i]
        a, b = j * o + ka - w, j * o + kb - w           # samples [a, b) meet taps [ka, kb)
        if a < 0:
            ka, a = ka - a, 0
        if b > L:
            kb, b = kb - (b - L), L
        if b > a:
            out[:, p] = x[:, a:b] @ h[i, ka:kb]
            mag[:, p] = ax[:, a:b] @ ah[i, ka:kb]
    return out, mag


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def lengths(tb: Table):
    """every L from 1 to 40 (L < width, L around a small o), o - 1, o, o + 1, and the L that put L_out at 256 m - 1, 256 m, 256 m + 1
    for m = 1 .. 9 -- every L that does where several do, the nearest reachable L_out on each side where none does"""
    Ls = set(range(1, 41)) | {tb.o - 1, tb.o, tb.o + 1}
    for m in range(1, 10):
        for v in (256 * m - 1, 256 * m, 256 * m + 1):
            L0 = v * tb.o // tb.n
            cand = range(max(1, L0 - 3), L0 + 4)
            exact = [L for L in cand if out_len(tb, L) == v]
            if exact:
                Ls.update(exact)
            else:
                Ls.add(max(L for L in cand if out_len(tb, L) < v))
                Ls.add(min(L for L in cand if out_len(tb, L) > v))
    return sorted(L for L in Ls if L >= 1)


class Case:
    def __init__(self, orig, new, L, B, signal):
        self.orig, self.new, self.L, self.B, self.signal = orig, new, L, B, signal

    @property
    def tb(self):
        return table(self.orig, self.new)

    @property
    def L_out(self):
        return out_len(self.tb, self.L)

    @property
    def id(self):
        return f"resample[{self.orig}->{self.new},L={self.L},B={self.B},{self.signal}]"

    def __repr__(self):
        return self.id


def cases(pair=None):
    cs = []
    for orig, new in ((pair,) if pair else PAIRS):
        for L in lengths(table(orig, new)):
            cs += [Case(orig, new, L, B, s) for B in BATCHES for s in SIGNALS]
    return cs


def signal(c: Case) -> np.ndarray:
    """fp32 [B][L]; non-zero samples keep |x| >= 2^-20"""
    if c.signal == "noise":
        r = np.random.default_rng(zlib.crc32(c.id.encode()))
        x = r.standard_normal((c.B, c.L))
        x = np.where(np.abs(x) < 2.0 ** -20, 2.0 ** -20, x)
    else:
        x = np.zeros((c.B, c.L))
        if c.signal == "impulse_first":
            x[:, 0] = 1.0
        elif c.signal == "impulse_last":
            x[:, c.L - 1] = 1.0
        else:
            x[:] = 1.0
        x *= np.array(ROW_GAIN[:c.B])[:, None]
    return x.astype(np.float32)


_refs = {}


def reference(c: Case):
    """(ref, mag) fp64 [B][L_out] of the case, computed once and never written to again"""
    if c.id not in _refs:
        ref, mag = apply64(c.tb, c.tb.h32.astype(np.float64), signal(c).astype(np.float64))
        ref.setflags(write=False)
        mag.setflags(write=False)
        _refs[c.id] = (ref, mag)
    return _refs[c.id]


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------
class IO:
    """x [B][L] (rows contiguous) between 64 NaN floats on each side; out [B][L_out] between 64 sentinel words on each side, the
    payload pre-filled with the sentinel too (a NaN: an output the kernel did not write, or one that took in a guard, shows)"""

    def __init__(self, c: Case, device="cpu"):
        self.case = c
        x = torch.from_numpy(signal(c))
        raw = torch.full((GUARD + x.numel() + GUARD,), float("nan"), dtype=torch.float32)
        raw[GUARD:GUARD + x.numel()] = x.reshape(-1)
        self.x_raw = raw.to(device)
        self.x = self.x_raw[GUARD:GUARD + x.numel()].view(c.B, c.L)
        n_out = c.B * c.L_out
        self.out_raw = torch.empty(GUARD + n_out + GUARD, dtype=torch.float32, device=device)
        self.out_raw.view(torch.int32).fill_(SENT32)
        self.out = self.out_raw[GUARD:GUARD + n_out].view(c.B, c.L_out)

    def result(self) -> np.ndarray:
        """the whole output allocation, guards included, as fp32 on the host"""
        return self.out_raw.detach().cpu().numpy().copy()


def check(c: Case, raw: np.ndarray):
    """(case, the output allocation with its guards) -> list of complaints"""
    tb, B, Lo = c.tb, c.B, c.L_out
    if raw.shape != (2 * GUARD + B * Lo,):
        return [f"{c.id}: output allocation of {raw.shape} words, expected {2 * GUARD + B * Lo}"]
    bad = []
    bits = raw.view(np.uint32)
    for which, band, at in (("front", bits[:GUARD], 0), ("back", bits[GUARD + B * Lo:], GUARD + B * Lo)):
        hit = np.nonzero(band != SENT32)[0]
        if hit.size:
            bad.append(f"{c.id}: {which} guard overwritten ({hit.size} words, first at {at + int(hit[0]) - GUARD} relative to the output)")
    got = raw[GUARD:GUARD + B * Lo].reshape(B, Lo).astype(np.float64)
    nan = np.isnan(got)
    if nan.any():
        b, p = (int(v[0]) for v in np.nonzero(nan))
        bad.append(f"{c.id}: {int(nan.sum())} outputs are NaN (not written, or a read outside [0, L)), first at row {b} sample {p}")
    ref, mag = reference(c)
    Ti = np.array(tb.Ti, dtype=np.float64)[np.arange(Lo) % tb.n]
    bound = (Ti * U / (1.0 - Ti * U) + Ti * 2.0 ** -53) * mag
    err = np.abs(got - ref)
    out = ~(err <= bound) & ~nan
    if out.any():
        b, p = (int(v[0]) for v in np.nonzero(out))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.nanmax(np.where(out, err / bound, 0.0)))
        bad.append(f"{c.id}: {int(out.sum())} outputs outside the bound (worst {worst:.3g} x), first at row {b} sample {p} (phase {p % tb.n}): "
                   f"got {got[b, p]!r} ref {ref[b, p]!r} bound {bound[b, p]:.3e}")
    return bad


# ---- numpy fp32 emulation of the kernel, right and wrong -------------------------------------------------------------------------
TABLE_BUGS = ("phase_advanced", "last_tap_dropped")
RESULT_BUGS = ("shifted_by_one", "row1_is_row0", "guard_word")
BUGS = TABLE_BUGS + RESULT_BUGS


def emulate(c: Case, taps, first, T, order="forward", bug=None) -> np.ndarray:
    """the sum in fp32, tap after tap in `order`, over the compact table -> the output allocation with its guards.  `bug`: a table
    advanced by one phase, the last non-zero tap of every phase dropped, the output shifted by one sample, batch row 1 answered with
    row 0's result, one guard word changed"""
    tb, B, L, Lo = c.tb, c.B, c.L, c.L_out
    taps, first = np.asarray(taps, dtype=np.float32), np.asarray(first, dtype=np.int64)
    if bug == "last_tap_dropped":
        taps = taps.copy()
        for i in range(tb.n):
            taps[np.nonzero(taps[:, i])[0][-1], i] = 0.0
    p = np.arange(Lo)
    j, i = p // tb.n, p % tb.n
    if bug == "phase_advanced":
        i = (i + 1) % tb.n
    xp = np.zeros((B, tb.width + (Lo // tb.n + 1) * tb.o + tb.K + T), dtype=np.float32)
    xp[:, tb.width:tb.width + L] = signal(c)
    at = j * tb.o + first[i]                                     # x[j o + k - width] sits at xp[j o + k]
    acc = np.zeros((B, Lo), dtype=np.float32)
    for t in (range(T) if order == "forward" else range(T - 1, -1, -1)):
        acc = acc + taps[t, i][None, :] * xp[:, at + t]
    if bug == "shifted_by_one":
        acc = np.concatenate([np.zeros((B, 1), np.float32), acc[:, :-1]], axis=1)
    if bug == "row1_is_row0" and B > 1:
        acc[1] = acc[0]
    raw = np.empty(2 * GUARD + B * Lo, dtype=np.float32)
    raw.view(np.uint32)[:] = SENT32
    raw[GUARD:GUARD + B * Lo] = acc.reshape(-1)
    if bug == "guard_word":
        raw.view(np.uint32)[GUARD + B * Lo] ^= 1
    return raw
