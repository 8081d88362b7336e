"""Sentence joins restated in numpy (tests/test_wave_join_host.py, tests/test_wave_join_gpu.py): what f5_wave_join must write, sample by
sample, as an fp64 value and a kind; the library's table validation; a brute-force join_layout that places the sentences sample by
sample; an fp32 emulation of the kernel that can make the mistakes the checker has to catch."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                       # unit roundoff of fp32
ZERO, COPY, FADE, OVERLAP = 0, 1, 2, 3
FADE_MAX = 1 << 22
BUGS = ("fade_out_from_wrong_end", "overlap_shifted_by_one", "weight_i_over_F", "mask_instead_of_select")


def weight32(i, F):
    """w(i, F) = (float)(2 i + 1) / (float)(2 F): one IEEE fp32 division of two exactly representable integers"""
    return np.float32(2 * np.asarray(i) + 1) / np.float32(2 * np.asarray(F))


def validate(table, R, Ls, Lout):
    """the refusals of f5_wave_join that concern the table, in the library's order -> None, or the key word of the refusal"""
    table = np.asarray(table, dtype=np.int64)
    for q in range(table.shape[0]):
        prev = None
        for k in range(table.shape[1]):
            d0, row, s0, n, fi, fo = table[q, k].tolist()
            if min(d0, row, s0, n, fi, fo) < 0:
                return "negative field"
            if row >= R:
                return "names source row"
            if s0 + n > Ls:
                return "reads source samples"
            if fi > FADE_MAX or fo > FADE_MAX:
                return "fade longer than 2^22"
            if fi + fo > n:
                return "shorter than its fades"
            if n == 0:
                continue
            if d0 + n > Lout:
                return "beyond the row length"
            if prev is not None:
                p0, p1, pfo = prev
                if d0 < p0:
                    return "sorted by dst_begin"
                if d0 < p1 and not (p1 - d0 == pfo and p1 - d0 == fi):
                    return "not a pure cross-fade"
            prev = (d0, d0 + n, fo)
    return None


def reference(src, table, Lout):
    """-> (val fp64 [Q][Lout], kind int8, exact fp32, bound fp64).  kind ZERO: +0.0; COPY: the source's bits; FADE: exact =
    float32(w) * float32(x), one fp32 multiplication (restated exactly); OVERLAP: val = a + w (b - a) in fp64 with the real w, and
    bound = u w |b - a| (1 + u) + u |val| (the difference and the fma round once each: tests/test_edit_gpu.py) + u w |b - a| (the one
    rounding of w itself).  The table must be valid."""
    table = np.asarray(table, dtype=np.int64)
    Q = table.shape[0]
    val, kind = np.zeros((Q, Lout)), np.zeros((Q, Lout), dtype=np.int8)
    exact, bound = np.zeros((Q, Lout), dtype=np.float32), np.zeros((Q, Lout))
    for q in range(Q):
        segs = [t for t in table[q].tolist() if t[3] > 0]
        for m, (d0, row, s0, n, fi, fo) in enumerate(segs):
            x = src[row, s0:s0 + n]
            i = np.arange(n)
            head = max(0, segs[m - 1][0] + segs[m - 1][3] - d0) if m > 0 else 0         # samples shared with the segment before
            tail = max(0, d0 + n - segs[m + 1][0]) if m + 1 < len(segs) else 0          # ... with the one after
            lone = slice(head, n - tail)
            e, kd = x.copy(), np.full(n, COPY, dtype=np.int8)
            if fi:
                e[:fi], kd[:fi] = weight32(i[:fi], fi) * x[:fi], FADE
            if fo:
                e[n - fo:], kd[n - fo:] = weight32(n - 1 - i[n - fo:], fo) * x[n - fo:], FADE
            out = slice(d0 + head, d0 + n - tail)
            exact[q, out], kind[q, out], val[q, out] = e[lone], kd[lone], e[lone].astype(np.float64)
            if head:                                                                     # this segment fades in over the one before
                pd0, prow, ps0, pn = segs[m - 1][:4]
                a = src[prow, ps0 + (d0 - pd0):ps0 + pn].astype(np.float64)
                b = x[:head].astype(np.float64)
                w = (2.0 * i[:head] + 1.0) / (2.0 * head)
                o = slice(d0, d0 + head)
                val[q, o], kind[q, o] = a + w * (b - a), OVERLAP
                bound[q, o] = U * w * np.abs(b - a) * (1 + U) + U * np.abs(val[q, o]) + U * w * np.abs(b - a)
    return val, kind, exact, bound


def check(got, src, table, Lout):
    """a result of f5_wave_join against the reference -> list of violations (empty: passed)"""
    got = np.asarray(got, dtype=np.float32)
    val, kind, exact, bound = reference(src, table, Lout)
    bad = []
    if got.shape != val.shape:
        return [f"shape {got.shape}, expected {val.shape}"]
    if np.isnan(got).any():
        bad.append(f"{int(np.isnan(got).sum())} NaN in the output")
    z = kind == ZERO
    if (got[z].view(np.int32) != 0).any():
        bad.append(f"{int((got[z].view(np.int32) != 0).sum())} samples no segment covers are not +0.0")
    for k, name in ((COPY, "copied"), (FADE, "single-fade")):
        m = kind == k
        wrong = got[m].view(np.int32) != exact[m].view(np.int32)
        if wrong.any():
            q, s = np.argwhere(m)[np.nonzero(wrong)[0][0]]
            bad.append(f"{int(wrong.sum())} {name} samples differ in their bits, first at [{q}][{s}]: {got[q, s]!r} for {exact[q, s]!r}")
    m = kind == OVERLAP
    with np.errstate(invalid="ignore"):
        over = ~(np.abs(got.astype(np.float64) - val) <= bound) & m
    if over.any():
        q, s = np.argwhere(over)[0]
        bad.append(f"{int(over.sum())} overlap samples beyond the bound, first at [{q}][{s}]: {got[q, s]!r} for {val[q, s]!r} +- {bound[q, s]:.3e}")
    return bad


def emulate(src, table, Lout, bug=None):
    """the kernel in fp32 numpy, sample by sample (fmaf through fp64: the product of two fp32 is exact there, and the one rounding of
    the sum to fp64 before the rounding to fp32 cannot be told from a single rounding at the bound the checker uses); `bug`: one of
    BUGS"""
    table = np.asarray(table, dtype=np.int64)
    Q, S = table.shape[:2]
    out = np.full((Q, Lout), np.nan, dtype=np.float32)

    def w(i, F):
        return np.float32(i) / np.float32(F) if bug == "weight_i_over_F" else weight32(i, F)

    for q in range(Q):
        for s in range(Lout):
            hits = [k for k in range(S) if 0 <= s - table[q, k, 0] < table[q, k, 3]]
            if not hits:
                if bug == "mask_instead_of_select":                       # loads through the row's first segment anyway, times 0
                    d0, row, s0 = table[q, 0, :3].tolist()
                    out[q, s] = np.float32(0.0) * src[row, min(max(s0 + s - d0, 0), src.shape[1] - 1)]
                else:
                    out[q, s] = 0.0
                continue
            d0, row, s0, n, fi, fo = table[q, hits[0]].tolist()
            ia = s - d0
            xa = src[row, s0 + ia]
            if len(hits) == 1:
                if ia < fi:
                    out[q, s] = w(ia, fi) * xa
                elif n - 1 - ia < fo:
                    out[q, s] = w(ia - (n - fo) if bug == "fade_out_from_wrong_end" else n - 1 - ia, fo) * xa
                else:
                    out[q, s] = xa
                continue
            e0, erow, es0, en, efi, _ = table[q, hits[1]].tolist()
            ib = s - e0
            xb = src[erow, es0 + ib]
            if bug == "overlap_shifted_by_one":                           # the weight of the sample after
                ib += 1
            out[q, s] = np.float32(float(w(ib, efi)) * float(np.float32(xb - xa)) + float(xa))
    return out


def brute_layout(begin, length, row_req, fade, gap):
    """join_layout by placing every sample: -> (entries {row: (dst_begin, fade_in, fade_out)}, out_lens, cover: per request the number
    of sentences that reach each output sample).  fade / gap: one value per request."""
    Q = max(row_req) + 1
    entries, out_lens, cover = {}, [], []
    for q in range(Q):
        rows = [r for r in range(len(row_req)) if row_req[r] == q]
        placed = {}                                                        # output position -> how many samples landed there
        cursor = 0
        for k, r in enumerate(rows):
            F = 0
            if k > 0:
                a = rows[k - 1]
                while F < fade[q] and 2 * (F + 1) <= length[a] and 2 * (F + 1) <= length[r]:
                    F += 1
                cursor = cursor - F if gap[q] == 0 else cursor + gap[q]
                entries[a] = entries[a][:2] + (F,)
            entries[r] = (cursor, F, 0)
            for _ in range(length[r]):
                placed[cursor] = placed.get(cursor, 0) + 1
                cursor += 1
        out_lens.append(cursor)
        c = np.zeros(max(cursor, 0), dtype=np.int64)
        for pos, cnt in placed.items():
            c[pos] = cnt
        cover.append(c)
    return entries, out_lens, cover


def gpu_case(seed=0):
    """The case of the GPU test: R = 6 rows of Ls = 2100, Q = 3 requests, S = 4 -> (src with NaN wherever the table does not read,
    table, Lout, out_lens).  Request 0: four segments -- a leading fade of 7 from silence at dst 5; a cross-fade of 256; a segment of
    EXACTLY fade_in + fade_out = 256 + 7 samples; a gap of 3 samples, smaller than the fades of 7 on either side of it; a join that
    abuts without fades (0).  Request 1: one segment and three empty entries.  Request 2: three segments and one empty entry in the
    MIDDLE, a gap of 300, larger than its fades of 7, and a cross-fade of 1.  The longest output is 4 096 + 41; the three lengths
    differ."""
    r = np.random.default_rng(seed)
    R, Ls = 6, 2100
    t = np.zeros((3, 4, 6), dtype=np.int32)
    # (dst_begin, src_row, src_begin, len, fade_in, fade_out)
    t[0, 0] = (5, 0, 100, 2000, 7, 256)
    t[0, 1] = (5 + 2000 - 256, 1, 0, 263, 256, 7)
    t[0, 2] = (t[0, 1, 0] + 263 + 3, 2, 50, 2050, 7, 0)
    at = t[0, 2, 0] + 2050
    t[0, 3] = (at, 3, 1, 4096 + 41 - at, 0, 0)
    t[1, 0] = (0, 4, 33, 1500, 0, 0)
    t[2, 0] = (0, 5, 0, 900, 0, 7)
    t[2, 1] = (0, 0, 0, 0, 0, 0)
    t[2, 2] = (900 + 300, 5, 900, 600, 7, 1)
    t[2, 3] = (900 + 300 + 600 - 1, 3, 1500, 600, 1, 0)
    out_lens = [int((t[q, :, 0] + t[q, :, 3]).max()) for q in range(3)]
    Lout = max(out_lens)
    assert Lout == 4096 + 41 and t[0, 3, 3] > 0 and validate(t, R, Ls, Lout) is None
    vals = (r.standard_normal((R, Ls)) * 0.3).astype(np.float32)
    src = np.full((R, Ls), np.nan, dtype=np.float32)
    for d0, row, s0, n, _, _ in t.reshape(-1, 6).tolist():
        src[row, s0:s0 + n] = vals[row, s0:s0 + n]
    assert np.isnan(src).any()
    return src, t, Lout, out_lens
