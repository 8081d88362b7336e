"""The resampler on the CPU: audio.resample_table against the independent statement of the filter in tests/resample_matrix.py, the
checker of that matrix against a numpy fp32 emulation of the kernel (right, in both summation orders, and wrong in each way a
resampling kernel can be wrong without crashing), the filter itself held to its figures, the refusals of f5_resample_batch (all of
them come before any launch) and the opt-in wiring of generate().  What tests/test_resample_gpu.py asserts about the kernel is only
worth what this module shows about the harness."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_matrix as RM
from f5test import E
from f5_tts_mlx_amd import audio as A

PAIR_IDS = [f"{a}-{b}" for a, b in RM.PAIRS]


# ---- the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RM.PAIRS, ids=PAIR_IDS)
def test_table_matches_the_restated_filter(pair):
    tb = RM.table(*pair)
    h64, o, n, width, base = A.resample_taps64(*pair)
    g = math.gcd(*pair)
    assert (o, n) == (pair[0] // g, pair[1] // g) == (tb.o, tb.n) and width == tb.width and base == tb.base
    assert h64.shape == tb.h64.shape == (n, 2 * width + o)
    # fp64 sin / cos on arguments up to 6 pi err by about 2e-15: a margin of a few hundred
    tol = 1e-12 * base / o
    diff = float(np.abs(h64 - tb.h64).max())
    print(f"[resample table] {pair}: o:n = {o}:{n} width {width} T {tb.T}, largest difference before rounding {diff:.3e} (cap {tol:.3e})")
    assert diff <= tol
    # clamped taps are exactly zero, in both
    t = np.array([[(-i / n + (k - width) / o) * base for k in range(tb.K)] for i in range(n)])
    assert (h64[np.abs(t) >= RM.LPW] == 0.0).all() and (tb.h64[np.abs(t) >= RM.LPW] == 0.0).all()
    # after rounding: bit-equal, except where the fp64 value lies within tol of an fp32 rounding boundary
    taps, first, o2, n2, T, width2 = A.resample_table(*pair)
    assert (o2, n2, width2) == (o, n, width) and taps.dtype == np.float32 and first.dtype == np.int32
    assert taps.shape == (T, n) and first.shape == (n,)
    want_taps, want_first, want_T = RM.compact(tb)
    assert T == want_T and (first == want_first).all()
    ne = taps.view(np.uint32) != want_taps.view(np.uint32)
    for tt, i in zip(*np.nonzero(ne)):
        v = tb.h64[i, first[i] + tt]
        lo, hi = sorted((float(taps[tt, i]), float(want_taps[tt, i])))
        assert np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi) and abs(v - (lo + hi) / 2) <= tol, (tt, i, v, lo, hi)
    # first / T agree with the non-zero runs of the rounded table
    h32 = h64.astype(np.float32)
    for i in range(n):
        nz = np.nonzero(h32[i])[0]
        assert first[i] == nz[0] and nz[-1] - nz[0] + 1 <= T
        run = h32[i, nz[0]:nz[-1] + 1]
        assert (taps[:len(run), i] == run).all() and (taps[len(run):, i] == 0.0).all()
    assert T == max(np.nonzero(h32[i])[0][-1] - np.nonzero(h32[i])[0][0] + 1 for i in range(n))
    assert T <= 2 * width + 1 and taps.nbytes + first.nbytes < 20 * 1024


def test_table_sizes_of_the_issue():
    assert A.resample_table(48_000, 24_000)[4] == 25                       # the longest run of all pairs
    assert max(A.resample_table(*p)[4] for p in RM.PAIRS) == 25
    taps, first, o, n, T, width = A.resample_table(11_025, 24_000)
    assert (o, n, T, 2 * width + o) == (147, 320, 13, 161)
    assert A.resample_table(24_000, 16_000) is A.resample_table(24_000, 16_000)          # cached


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def _host_cases(pair):
    """every length up to o + 1 and 40, and the tile edges 255 ... 257 and 1023 ... 1025 (or their neighbours), of one pair"""
    return [c for c in RM.cases(pair) if c.L_out <= 130 or 250 <= c.L_out <= 262 or 1018 <= c.L_out <= 1030]


@pytest.mark.parametrize("pair", RM.PAIRS, ids=PAIR_IDS)
def test_checker_accepts_the_emulation_in_both_orders(pair):
    taps, first, T = RM.compact(RM.table(*pair))
    cs = _host_cases(pair)
    assert {c.B for c in cs} == {1, 3} and {c.signal for c in cs} == set(RM.SIGNALS) and max(c.L_out for c in cs) > RM.TILE
    bad = [b for c in cs for order in ("forward", "reverse") for b in RM.check(c, RM.emulate(c, taps, first, T, order))]
    assert not bad, "\n".join(bad[:20])


def test_checker_accepts_the_emulation_over_the_package_table():
    for pair in ((44_100, 24_000), (24_000, 16_000)):
        taps, first, _, _, T, _ = A.resample_table(*pair)
        bad = [b for c in _host_cases(pair)[::7] for b in RM.check(c, RM.emulate(c, taps, first, T))]
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("bug", RM.BUGS)
@pytest.mark.parametrize("pair", RM.PAIRS, ids=PAIR_IDS)
def test_checker_flags_every_seeded_mistake(pair, bug):
    tb = RM.table(*pair)
    if bug == "phase_advanced" and tb.n == 1:
        return                                                            # one phase: nothing to advance
    taps, first, T = RM.compact(tb)
    cs = [c for c in _host_cases(pair) if c.L_out >= 2 and (bug != "row1_is_row0" or c.B == 3)]
    flagged = [c.id for c in cs if RM.check(c, RM.emulate(c, taps, first, T, bug=bug))]
    print(f"[resample harness] {bug} at {pair}: flagged by {len(flagged)} of {len(cs)} cases")
    assert flagged
    if bug in RM.RESULT_BUGS:                                             # these leave no case unflagged ...
        quiet = [c.id for c in cs if c.id not in flagged]
        if bug == "shifted_by_one":                                       # ... but a shift of an output that is the same everywhere
            quiet = [q for q in quiet if "noise" in q]
        assert not quiet, quiet[:10]


def test_case_generator_covers_what_it_claims():
    for pair in RM.PAIRS:
        tb = RM.table(*pair)
        Ls = RM.lengths(tb)
        assert set(range(1, 41)) <= set(Ls) and {tb.o, tb.o + 1} <= set(Ls) and (tb.o == 1 or tb.o - 1 in Ls)
        outs = sorted({RM.out_len(tb, L) for L in Ls})
        reach = {RM.out_len(tb, L) for L in range(1, 2400 * tb.o // tb.n + 8)}
        for m in range(1, 10):
            for v in (256 * m - 1, 256 * m, 256 * m + 1):
                if v in outs:
                    continue
                below, above = max(x for x in outs if x < v), min(x for x in outs if x > v)
                # nothing reachable lies between the neighbours and the target
                assert not any(below < r < above for r in reach), (pair, v, below, above)
        ids = [c.id for c in RM.cases(pair)]
        assert len(ids) == len(set(ids)) == len(Ls) * len(RM.BATCHES) * len(RM.SIGNALS)
    x = RM.signal(RM.Case(16_000, 24_000, 4001, 3, "noise"))
    assert np.abs(x[x != 0]).min() >= 2.0 ** -20 and x.dtype == np.float32
    assert RM.TILE & (RM.TILE - 1) == 0 and RM.TILE <= 2048               # a power-of-two tile: the 256 m edges are its edges


# ---- the filter is a resampler -------------------------------------------------------------------------------------------------
def _through(pair, freq, L=4000):
    """a unit sine of `freq` Hz through the fp64 filter: (output without 200 samples at each end, the analytic sine at those times)"""
    tb = RM.table(*pair)
    x = np.sin(2 * math.pi * freq * np.arange(L) / pair[0])[None]
    y = RM.apply64(tb, tb.h64, x)[0][0]
    p = np.arange(y.shape[0])
    return y[200:-200], np.sin(2 * math.pi * freq * p / pair[1])[200:-200]


@pytest.mark.parametrize("pair,freq,measured", [((16_000, 24_000), 1000, 5.5e-4), ((44_100, 24_000), 3000, 1.4e-4), ((24_000, 16_000), 3000, 5.2e-4)])
def test_pass_band_sine_comes_through(pair, freq, measured):
    y, want = _through(pair, freq)
    dev = float(np.abs(y - want).max())
    print(f"[resample filter] {freq} Hz, {pair[0]} -> {pair[1]}: max deviation from the analytic sine {dev:.3e} (recorded {measured:.1e}, cap 1e-3)")
    assert dev <= 1e-3


@pytest.mark.parametrize("pair,freq,measured", [((24_000, 16_000), 10_000, 0.0038), ((48_000, 24_000), 14_000, 0.054)])
def test_stop_band_tone_is_attenuated(pair, freq, measured):
    y, _ = _through(pair, freq)
    rms = float(np.sqrt(np.mean(y * y)))
    print(f"[resample filter] {freq} Hz, {pair[0]} -> {pair[1]} (above the new Nyquist): output rms {rms:.4f} (recorded {measured}, cap 0.1)")
    assert rms <= 0.1


def test_dc_gain_of_every_phase():
    lo, hi = 2.0, 0.0
    for pair in RM.PAIRS:
        gain = RM.table(*pair).h64.sum(axis=1)
        lo, hi = min(lo, float(gain.min())), max(hi, float(gain.max()))
    print(f"[resample filter] DC gain over every phase of every pair: {lo:.5f} ... {hi:.5f}")
    assert abs(lo - 1) <= 1e-3 and abs(hi - 1) <= 1e-3


# ---- the C ABI refuses before it launches --------------------------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(wave=64, B=1, L=100, taps=64, first=64, o=2, n=3, T=15, width=7, out=64, L_out=150, stream=0)
    a.update(kw)
    rc = lib.f5_resample_batch(C.c_void_p(a["wave"]), a["B"], C.c_int64(a["L"]), C.c_void_p(a["taps"]), C.c_void_p(a["first"]), a["o"],
                               a["n"], a["T"], a["width"], C.c_void_p(a["out"]), C.c_int64(a["L_out"]), C.c_void_p(a["stream"]))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(wave=0), "null pointer"), (dict(taps=0), "null pointer"), (dict(first=0), "null pointer"), (dict(out=0), "null pointer"),
    (dict(o=0), "must be >= 1"), (dict(n=0), "must be >= 1"), (dict(T=0), "must be >= 1"), (dict(width=0), "must be >= 1"),
    (dict(n=-3), "must be >= 1"),
    (dict(o=4, n=6, L_out=150), "not coprime"),
    (dict(L=-1, L_out=0), "negative length"),
    (dict(L_out=149), "ceil(n * L / o) = 150"), (dict(L=101, L_out=151), "ceil(n * L / o) = 152"),
    (dict(B=0), "outside 1..65535"), (dict(B=65536), "outside 1..65535"),
    (dict(o=8, n=1, T=97, width=49, L=100, L_out=13), "ratio 8:1 too large"),
    (dict(o=48_000, n=1, T=25, width=12, L=48_000, L_out=1), "too large"),
    (dict(T=18), "exceeds"),
])
def test_abi_refusals_need_no_gpu(kw, word):
    rc, msg = _call(E.load_library(), **kw)
    assert rc != 0 and msg.startswith("resample:") and word in msg, (rc, msg)


def test_abi_limit_admits_every_pair_and_an_empty_input_is_no_launch():
    lib = E.load_library()
    for pair in RM.PAIRS + ((48_000, 8_000), (44_100, 8_000), (48_000, 16_000)):
        _, _, o, n, T, width = A.resample_table(*pair)
        rc, msg = _call(lib, o=o, n=n, T=T, width=width, L=0, L_out=0)           # every check passes; L = 0 returns before the launch
        assert rc == 0, (pair, msg)
        # the limit stated in include/f5tts_hip.h
        assert (1023 // n + 1) * o + 2 * width + o + T - 1 <= 8192
    _, _, o, n, T, width = A.resample_table(8, 1)
    assert (1023 // n + 1) * o + 2 * width + o + T - 1 > 8192


# ---- Python wiring -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(0, 24_000), (24_000, 0), (-16_000, 24_000), (24_000, -1), (16_000.0, 24_000), (24_000, 22_050.5),
                                      (True, 24_000), ("16000", 24_000)])
def test_resample_refuses_bad_rates(orig, new):
    with pytest.raises(ValueError, match="positive integer"):
        A.resample(np.zeros(8, np.float32), orig, new)


class _OnlyAVocoder:
    _vocoder = staticmethod(lambda mel: mel)


def test_generate_default_still_refuses_a_16k_reference(tmp_path):
    from f5_tts_mlx_amd import generate as G
    path = tmp_path / "ref16k.wav"
    G.write_wav(str(path), np.sin(np.arange(16_000) * 0.05).astype(np.float32), 16_000)
    assert G.read_wav(str(path))[1] == 16_000
    with pytest.raises(ValueError, match="Reference audio must have a sample rate of 24kHz"):
        G.generate("Hello.", ref_audio_path=str(path), ref_audio_text="hi", f5tts=_OnlyAVocoder())
    with pytest.raises(ValueError, match="output_sample_rate"):
        G.generate("Hello.", f5tts=_OnlyAVocoder(), output_sample_rate=0)


def test_cli_lists_the_new_flags(capsys):
    from f5_tts_mlx_amd import generate as G
    with pytest.raises(SystemExit) as e:
        G.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--resample-ref" in text and "--output-rate" in text
    import inspect
    sig = inspect.signature(G.generate)
    assert sig.parameters["resample_ref"].default is False and sig.parameters["output_sample_rate"].default is None
    assert "torchaudio" in G.generate.__doc__ and "docs/resample.md" in G.generate.__doc__
