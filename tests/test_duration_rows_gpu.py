"""Row-isolated duration prediction on the GPU (docs/duration_rows.md): `f5_predict_duration_rows` against the fp64 oracle's prediction of
every row ALONE, against the Python-sequenced path it restates, under a change of the batch-mates, under graph replay, where nothing is
padded, in frames, and through `F5TTS.sample`.  Inputs and references: tests/duration_rows_ref.py.  Every native call runs on a workspace
4 KiB longer than the size call asks for; the tail carries a byte pattern that must survive the call.  Every bitwise statement compares
launches of one shape."""
import ctypes as C
import functools

import pytest
import torch

import duration_rows_ref as R
from f5test import DEV, TINY, synthetic_weights
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd.cfm import F5TTS, prepare_lengths
from f5_tts_mlx_amd.dit import DiT
from f5_tts_mlx_amd.duration import DurationPredictor, DurationTransformer

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "bf16", "f16")
# the project's bounds for this model (tests/test_duration_native_gpu.py ORACLE_TOL): (bound relative to max(1, mean |ref|), the oracle
# rounds its operands to bf16); f16 has none
ORACLE_TOL = {"bf16x3": (2e-4, False), "bf16": (5e-3, True)}
GUARD, PATTERN = 4096, 0xA5


@functools.lru_cache(maxsize=None)
def predictor(dim, precision):
    m = R.MODELS[dim]
    tr = DurationTransformer(dim=dim, depth=m["depth"], heads=m["heads"], text_dim=512, ff_mult=2, conv_layers=2, text_num_embeds=70,
                             precision=precision, device=DEV)
    dp = DurationPredictor(tr)
    dp.load_weights(R.weights(dim))
    return dp


_GUARDED = {}


def guarded_workspace(dp, B, n_in, nt, rows):
    """The same workspace for the same predictor, shape and entry point (what a graph replay needs), 4 KiB longer than asked."""
    key = (id(dp), B, n_in, nt, rows)
    if key not in _GUARDED:
        T = dp.transformer
        n = C.c_size_t()
        size = T.lib.f5_duration_workspace_bytes_rows if rows else T.lib.f5_duration_workspace_bytes
        E.check(size(T._h, B, n_in, nt, C.byref(n)))
        full = E._aligned_bytes(n.value + GUARD, T.device)
        full[n.value:] = PATTERN
        _GUARDED[key] = (full, n.value)
    return _GUARDED[key]


def run_native(dp, mel, text, lens, rows=True, use_graph=False, workspace_rows=None, **kw):
    """one native call -> (seconds, frames) on the host; rows: f5_predict_duration_rows, else the plain call (workspace_rows: the plain
    call on the larger workspace of the other entry point)"""
    full, n = guarded_workspace(dp, mel.shape[0], mel.shape[1], text.shape[1], rows if workspace_rows is None else workspace_rows)
    iso = dict(isolate_rows=True) if rows else {}
    sec, frames = dp.predict_native(mel, text, lens=lens, use_graph=use_graph, workspace=full[:n], **iso, **kw)
    torch.cuda.synchronize()
    assert bool((full[n:] == PATTERN).all()), "a launch wrote past the workspace size the call asks for"
    return sec.cpu(), frames.cpu()


@functools.lru_cache(maxsize=None)
def native_rows(case, precision):
    """(result, reproduces itself bit for bit) of the eager isolated call"""
    mel, text, lens = R.inputs(case)
    dp = predictor(R.CASES[case][0], precision)
    a = run_native(dp, mel, text, lens)[0]
    return a, bool(torch.equal(a, run_native(dp, mel, text, lens)[0]))


@functools.lru_cache(maxsize=None)
def native_plain(case, precision):
    mel, text, lens = R.inputs(case)
    dp = predictor(R.CASES[case][0], precision)
    a = run_native(dp, mel, text, lens, rows=False)[0]
    return a, bool(torch.equal(a, run_native(dp, mel, text, lens, rows=False)[0]))


@functools.lru_cache(maxsize=None)
def sequenced_rows(case, precision):
    """The Python-sequenced path with the flag, run twice: (result, reproduces itself bit for bit)."""
    mel, text, lens = R.inputs(case)
    dp = predictor(R.CASES[case][0], precision)
    a = dp(mel, text, lens=lens, native=False, isolate_rows=True).cpu()
    b = dp(mel, text, lens=lens, native=False, isolate_rows=True).cpu()
    return a, bool(torch.equal(a, b))


def within_bounds(name, got, case, precision, rows=slice(None)):
    """every row (of `rows`) within the precision's bound of the oracle's prediction of that row alone"""
    tol, emu = ORACLE_TOL[precision]
    d = R.rel(got, R.solo(case, emu))[rows]
    print(f"[duration rows] {name} [{precision}] {case}: per-row distance to the solo oracle {['%.2e' % v for v in d]} (bound {tol:g})")
    assert max(d) <= tol, (name, d)


def same_or_bounded(name, got, want, reproducible, case, precision, rows=slice(None)):
    """the project's rule for two launch sequences of one shape: the same bits where the yardstick reproduces itself, else both within
    the bounds (rows: the rows of the case compared, default all; got and want are whole batches of the case)"""
    if reproducible:
        assert torch.equal(got[rows], want[rows]), (name, (got - want).abs().max())
    else:
        assert precision in ORACLE_TOL, f"{name}: the call is not bit-reproducible and {precision} has no oracle bound"
        within_bounds(name, got, case, precision, rows)
        within_bounds(name + " (yardstick)", want, case, precision, rows)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_every_row_meets_its_solo_oracle_and_the_plain_call_does_not(case, precision):
    """4. bf16x3 within 2e-4 of the fp64 oracle of the row alone, bf16 within 5e-3 of the oracle that rounds its operands to bf16.  f16
    has no bound in the project: it is held to the sequenced path (test 5) and its distance is printed.  The plain call on the same
    inputs misses the bound on every row but the longest: the inputs discriminate, and the parent commit fails here."""
    got, _ = native_rows(case, precision)
    assert got.shape == (len(R.CASES[case][3]),) and torch.isfinite(got).all() and (got > 0).all()
    if precision == "f16":
        print(f"[duration rows] native [f16] {case}: per-row distance to the fp64 solo oracle {R.rel(got, R.solo(case))} (reported, no bound)")
        return
    within_bounds("native", got, case, precision)
    tol, emu = ORACLE_TOL[precision]
    d = R.rel(native_plain(case, precision)[0], R.solo(case, emu))
    print(f"[duration rows] plain call [{precision}] {case}: per-row distance to the solo oracle {['%.2e' % v for v in d]}")
    assert d[0] <= tol and min(d[1:]) > tol, d


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_native_equals_the_python_sequenced_path(case, precision):
    """5. The same kernels in the same order with the same arguments: the same bits where the sequenced path reproduces itself."""
    want, reproducible = sequenced_rows(case, precision)
    got, _ = native_rows(case, precision)
    print(f"[duration rows] {case} [{precision}] sequenced={want.tolist()} native={got.tolist()} sequenced reproducible={reproducible}")
    assert torch.isfinite(want).all()
    same_or_bounded("native vs sequenced", got, want, reproducible, case, precision)


def other_batch_mates(case, b, seed):
    """the inputs of the case with every row but b replaced: new mel, new text ids within the same token counts, NaN in their mel past
    their lens"""
    _, n_in, nt, lens, tokens = R.CASES[case]
    mel, text, _ = R.inputs(case)
    new_mel, new_text = R.make_inputs(len(lens), n_in, nt, tokens, seed=seed)
    for o in range(len(lens)):
        new_mel[o, lens[o]:] = float("nan")
    new_mel[b], new_text[b] = mel[b], text[b]
    return new_mel, new_text


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_a_row_does_not_depend_on_its_batch_mates(case, precision):
    """6. At a fixed shape: other content in the other rows (and NaN in their mel past lens) leaves row b's bits where the call
    reproduces itself, else within the bounds; NaN in a row's own mel at n >= lens[b] changes nothing."""
    dp = predictor(R.CASES[case][0], precision)
    lens = R.inputs(case)[2]
    base, reproducible = native_rows(case, precision)
    for b in range(len(lens)):
        mel, text = other_batch_mates(case, b, seed=1000 + b)
        out = run_native(dp, mel, text, lens)[0]
        assert torch.isfinite(out).all(), out
        assert not torch.equal(out, base)                    # the other rows did change
        same_or_bounded(f"row {b} next to other batch-mates", out, base, reproducible, case, precision, rows=slice(b, b + 1))
    mel, text, _ = R.inputs(case)
    own = mel.clone()
    for b, n in enumerate(lens.tolist()):
        own[b, n:] = float("nan")
    out = run_native(dp, own, text, lens)[0]
    same_or_bounded("NaN in every row's own mel past lens", out, base, reproducible, case, precision)


def test_graph_replay_keys_and_the_plain_call_untouched():
    """7. Replay equals eager bitwise; a replay serves new lens and text_lens of the same shape; the isolated and the plain call of one
    shape hold two graphs (also on one workspace); the plain call's bits are the same before and after an isolated call."""
    dp = predictor(512, "bf16")
    lib, h = dp.transformer.lib, dp.transformer._h
    mel_a, text_a, lens_a = R.inputs("text_longer")
    tokens_b = (55, 80, 12)
    mel_b, text_b = R.make_inputs(3, 64, 80, tokens_b, seed=77)
    lens_b = torch.tensor([40, 64, 33])
    base = lib.f5_duration_graph_count(h)
    plain_before = run_native(dp, mel_a, text_a, lens_a, rows=False, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 1
    a = run_native(dp, mel_a, text_a, lens_a, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 2                      # keyed apart from the plain call's
    b = run_native(dp, mel_b, text_b, lens_b, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 2                      # the lengths are staged outside the captured part
    a_again = run_native(dp, mel_a, text_a, lens_a, use_graph=True)[0]
    a_eager = run_native(dp, mel_a, text_a, lens_a, use_graph=False)[0]
    b_eager = run_native(dp, mel_b, text_b, lens_b, use_graph=False)[0]
    assert lib.f5_duration_graph_count(h) == base + 2
    assert torch.equal(a, a_eager) and torch.equal(a_again, a_eager) and torch.equal(b, b_eager) and not torch.equal(a, b)
    plain_after = run_native(dp, mel_a, text_a, lens_a, rows=False, use_graph=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 2 and torch.equal(plain_after, plain_before)
    assert torch.equal(plain_before, run_native(dp, mel_a, text_a, lens_a, rows=False, use_graph=False)[0])
    assert not torch.equal(plain_before[1:], a[1:])                        # two results, not one
    # the plain call on the isolated call's own workspace: the same buffer, another key -> another graph, the plain bits
    on_rows_ws = run_native(dp, mel_a, text_a, lens_a, rows=False, use_graph=True, workspace_rows=True)[0]
    assert lib.f5_duration_graph_count(h) == base + 3 and torch.equal(on_rows_ws, plain_before)
    assert torch.equal(run_native(dp, mel_a, text_a, lens_a, use_graph=True)[0], a_eager)
    assert lib.f5_duration_graph_count(h) == base + 3


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_padded_nothing_changed(precision):
    """8. A row with L[b] = N, a batch of one, and lens = None with full-length text: the flag changes no bits (where the plain call
    does not reproduce itself, both stay within the bounds of the oracle)."""
    for case in R.CASES:                                     # a row with L[b] = N: row 0 of every case
        plain, reproducible = native_plain(case, precision)
        same_or_bounded(f"{case}: the longest row, flag on / off", native_rows(case, precision)[0], plain, reproducible, case, precision,
                        rows=slice(0, 1))

    def unpadded(name, dim, mel, text, lens, oracle):
        """plain twice, isolated, sequenced isolated on inputs without padding; oracle(emulate_bf16) is only asked without bit equality"""
        dp = predictor(dim, precision)
        p0, p1, iso = (run_native(dp, mel, text, lens, rows=r)[0] for r in (False, False, True))
        seq = dp(mel, text, lens=lens, native=False, isolate_rows=True).cpu()
        print(f"[duration rows] {name} [{precision}]: plain {p0.tolist()} isolated {iso.tolist()} sequenced {seq.tolist()}")
        if torch.equal(p0, p1):
            assert torch.equal(iso, p0) and torch.equal(seq, p0)
            return
        assert precision in ORACLE_TOL, f"{name}: the plain call is not bit-reproducible and {precision} has no oracle bound"
        tol, emu = ORACLE_TOL[precision]
        ref = oracle(emu)
        for got in (p0, iso, seq):
            assert max(R.rel(got, ref)) <= tol, (name, got, ref)

    for case in ("mel_longer", "text_longer", "dim1024"):    # a batch of one: row 0 at the full shape (tokens = nt, lens = n_in)
        mel, text, lens = R.inputs(case)
        unpadded(f"batch of one, {case}", R.CASES[case][0], mel[:1], text[:1], lens[:1], lambda emu, case=case: R.solo(case, emu)[:1])
    mel, text = R.make_inputs(2, 72, 20, (20, 20), seed=5)   # lens = None, text without padding, the mel the longer side: every L[b] = N
    unpadded("lens = None, full text", 512, mel, text, None,
             lambda emu: R.DO.predict(R.weights(512), mel, text, dtype=torch.float64, emulate_bf16=emu, **R.MODELS[512]))


@pytest.mark.parametrize("case", ["mel_longer", "dim1024"])
def test_frames_are_the_rows_own(case):
    """9. bf16x3.  The oracle's solo seconds x 93 lie 0.1 ... 0.9 from an integer (measured 0.63, 0.73, 0.31 and 0.58, 0.20; the 2e-4
    bound is worth 0.02 frames), so the frames are the oracle's int(seconds x 93): 108, 108, 88 and 31, 28 alone.  The plain call gives
    108, 110, 113 and 31, 25."""
    want, frac = R.frames(R.solo(case))
    assert all(0.1 <= f <= 0.9 for f in frac), frac
    assert want == {"mel_longer": [108, 108, 88], "dim1024": [31, 28]}[case]
    dp = predictor(R.CASES[case][0], "bf16x3")
    mel, text, lens = R.inputs(case)
    sec, frames = run_native(dp, mel, text, lens, frame_rate=93.0, speed=1.0)
    plain = run_native(dp, mel, text, lens, rows=False, frame_rate=93.0, speed=1.0)[1]
    print(f"[duration rows] frames [{case}] isolated {frames.tolist()} plain {plain.tolist()} oracle alone {want}")
    assert frames.dtype == torch.int32 and frames.tolist() == want
    assert torch.equal(frames, (sec * 93 / 1.0).to(torch.int32))
    assert plain.tolist() == {"mel_longer": [108, 110, 113], "dim1024": [31, 25]}[case]


@pytest.fixture(scope="module")
def tiny_f5():
    model = DiT.from_config(TINY, precision="bf16", device=DEV)
    model.load_weights(synthetic_weights(TINY, seed=2))
    return model


@pytest.mark.parametrize("native", [False, True])
def test_sample_asks_for_the_isolated_prediction(native, tiny_f5):
    """10. F5TTS.sample(duration=None, isolate_rows=True): last_durations are the isolated prediction after the clamps of
    prepare_lengths; without the flag the call asks the predictor what it always asked and nothing new is keyed or allocated."""
    dp = predictor(512, "bf16x3")
    mel, text, lens = R.inputs("mel_longer")
    text = torch.where(text >= 0, text % TINY.text_num_embeds, text)          # ids the tiny DiT's table has, the same token counts
    f5 = F5TTS(transformer=tiny_f5, duration_predictor=dp)
    lib, h = dp.transformer.lib, dp.transformer._h
    kw = dict(steps=2, method="euler", seed=3)
    saved = dp.native
    try:
        dp.native = native
        frames_iso = f5.predict_duration(mel, text, lens=lens, isolate_rows=True).cpu()
        frames_plain = f5.predict_duration(mel, text, lens=lens).cpu()
        alone = torch.stack([f5.predict_duration(mel[b:b + 1, :n], text[b:b + 1, :t], lens=torch.tensor([n]))[0].cpu()
                             for b, (n, t) in enumerate(zip(R.CASES["mel_longer"][3], R.CASES["mel_longer"][4]))])
        print(f"[duration rows] sample native={native}: frames isolated {frames_iso.tolist()} plain {frames_plain.tolist()} alone {alone.tolist()}")
        assert frames_iso.dtype == torch.int32 and abs(int(frames_iso[0]) - int(frames_plain[0])) <= 1      # the longest row
        assert (frames_iso[1:] - frames_plain[1:]).abs().min() >= 2                                  # the inputs discriminate
        assert (frames_iso - alone).abs().max() <= 1               # another shape, other kernel routes: the same frame up to a boundary
        want = prepare_lengths(text, mel.shape[1], 3, frames_iso, lens, 4096, "euler")[2].tolist()
        want_plain = prepare_lengths(text, mel.shape[1], 3, frames_plain, lens, 4096, "euler")[2].tolist()
        assert want != want_plain
        graphs, spaces = lib.f5_duration_graph_count(h), set(dp._workspaces)
        out_plain, _ = f5.sample(mel, text, duration=None, lens=lens, **kw)
        assert f5.last_durations == want_plain and out_plain.shape[1] == max(want_plain)
        assert lib.f5_duration_graph_count(h) == graphs and set(dp._workspaces) == spaces       # the call of before: nothing new
        again, _ = f5.sample(mel, text, duration=torch.tensor(want_plain), lens=lens, **kw)
        assert torch.equal(out_plain, again)
        out, _ = f5.sample(mel, text, duration=None, lens=lens, isolate_rows=True, **kw)
        assert f5.last_durations == want and out.shape[1] == max(want) and torch.isfinite(out).all()
        given, _ = f5.sample(mel, text, duration=torch.tensor(want), lens=lens, isolate_rows=True, **kw)
        assert torch.equal(out, given)
        assert lib.f5_duration_graph_count(h) == graphs
    finally:
        dp.native = saved
