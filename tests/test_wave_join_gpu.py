"""Sentence joins on the GPU: f5_wave_join through the C ABI against the numpy restatement of tests/wave_join_ref.py -- the output
prefilled with NaN between guard bands, NaN in every source sample the table does not name; copies and single fades bit for bit,
overlaps within the derived bound --, the chunked launch, audio.join_rows against torch.cat and against the trim done by hand, the
batched resample of the padded result, and generate_many / generate on the tiny model with a synthetic Vocos against the same pipeline
done by hand.  tests/test_wave_join_host.py shows the checker used here flagging each seeded mistake.  Every test of this file needs
entry points that did not exist before the feature."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wave_join_ref as WJ
from f5test import DEV, E, P, TINY, stream, synthetic_weights
from rowops_matrix import Out, bits, pad_in
from f5_tts_mlx_amd import audio as A
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

VOCAB = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _call(lib, src_dev, R, Ls, table, Lout):
    """one call through the C ABI into an output prefilled with NaN between guard bands -> (result on the host, guard findings)"""
    table = np.ascontiguousarray(table, dtype=np.int32)
    Q, S = table.shape[:2]
    out = Out((Q, Lout), torch.float32, DEV, guard=512)
    out.t.fill_(float("nan"))
    rc = lib.f5_wave_join(P(src_dev), R, C.c_int64(Ls), table.ctypes.data_as(C.c_void_p), Q, S, P(out.t), C.c_int64(Lout), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.f5_last_error()
    return out.t.cpu().numpy(), out.guard_violations("out")


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def test_wave_join_against_the_reference(lib):
    """wave_join_ref.gpu_case: R = 6 rows of 2100, Q = 3, S = 4; fades of 0, 1, 7 and 256 in one table, a segment of exactly
    fade_in + fade_out, a gap smaller and one larger than its fades, a leading fade from silence, an empty entry at the end and one in
    the middle, three different output lengths with the longest 4 096 + 41.  Copies and single fades: int32 bit patterns; uncovered
    samples: +0.0; overlaps: |out - ref| <= u w |b - a| (1 + u) + u |ref| + u w |b - a|; no NaN; guards intact."""
    src, table, Lout, out_lens = WJ.gpu_case()
    dev = pad_in(torch.from_numpy(src), DEV)
    got, guards = _call(lib, dev, src.shape[0], src.shape[1], table, Lout)
    val, kind, _, bound = WJ.reference(src, table, Lout)
    m = kind == WJ.OVERLAP
    err = np.abs(got.astype(np.float64) - val)[m]
    print(f"[wave_join] {int(m.sum())} overlap samples: max |out - ref| / bound = {float((err / bound[m]).max()):.3f}; "
          f"kinds zero/copy/fade/overlap = {[int((kind == k).sum()) for k in range(4)]}")
    bad = guards + WJ.check(got, src, table, Lout)
    assert not bad, "\n".join(bad)
    for q, n in enumerate(out_lens):                                       # the zero tails differ in length
        assert not got[q, n:].view(np.int32).any() and (n == Lout or got[q, n:].size > 0)
    # the Python wrapper is the same call; a table the library refuses is a ValueError
    assert np.array_equal(A.wave_join(dev, table, Lout).cpu().numpy().view(np.int32), got.view(np.int32))
    wrong = table.copy()
    wrong[0, 1, 0] += 1
    with pytest.raises(ValueError, match="not a pure cross-fade"):
        A.wave_join(dev, wrong, Lout)


def test_wave_join_chunked_launch_equals_one_request_per_call(lib):
    """Q = 45 requests of up to S = 8 sentences: 48 table words per row, 20 rows per launch, so three launches (20, 20, 5); every
    request must get ITS segments: the bits of the same request joined alone"""
    r = np.random.default_rng(45)
    Q, Ls = 45, 96
    counts = [8 if q in (0, 19, 20, 44) else int(r.integers(1, 9)) for q in range(Q)]
    row_req = [q for q in range(Q) for _ in range(counts[q])]
    R = len(row_req)
    begin = [int(v) for v in r.integers(0, 30, R)]
    length = [int(v) for v in r.integers(1, 60, R)]
    fade = [int(v) for v in r.integers(0, 9, Q)]
    gap = [int(v) if q % 3 else 0 for q, v in enumerate(r.integers(1, 12, Q))]
    table, out_lens, Lout = A.join_layout(begin, length, row_req, fade=fade, gap=gap)
    assert table.shape == (Q, 8, 6) and Q * 8 * 6 > 2 * 960
    src = np.full((R, Ls), np.nan, dtype=np.float32)
    for i in range(R):
        src[i, begin[i]:begin[i] + length[i]] = r.standard_normal(length[i]).astype(np.float32)
    dev = pad_in(torch.from_numpy(src), DEV)
    got, guards = _call(lib, dev, R, Ls, table, Lout)
    bad = guards + WJ.check(got, src, table, Lout)
    assert not bad, "\n".join(bad)
    for q in range(Q):
        alone, guards = _call(lib, dev, R, Ls, table[q:q + 1], Lout)
        assert not guards and np.array_equal(alone.view(np.int32), got[q:q + 1].view(np.int32)), q


# ---- join_rows ------------------------------------------------------------------------------------------------------------------------
def _decoded(seed, R=5, Ls=6200):
    """rows whose sentence (after a 'reference' of begin[r] samples) is loud in the middle and near silent (-80 dB) at its edges"""
    r = np.random.default_rng(seed)
    begin = [240 * 2, 240 * 2 + 100, 700, 0, 333][:R]
    length = [5400, 4900, 5300, 4000, 5000][:R]
    x = np.full((R, Ls), np.nan, dtype=np.float32)
    for i in range(R):
        x[i, :begin[i]] = (r.standard_normal(begin[i]) * 0.3).astype(np.float32)                # the reference part: loud
        s = r.standard_normal(length[i]) * 1e-4
        lo, hi = 1500 + 97 * i, length[i] - 1700 - 31 * i
        s[lo:hi] = r.standard_normal(hi - lo) * 0.1
        x[i, begin[i]:begin[i] + length[i]] = s.astype(np.float32)
    return x, begin, length


def test_join_rows_without_fade_pause_and_trim_is_torch_cat():
    x, begin, length = _decoded(1)
    dev = pad_in(torch.from_numpy(x), DEV)
    row_req = [0, 0, 1, 2, 2]
    got, out_lens = A.join_rows(dev, begin, length, row_req, cross_fade_ms=0, pause_ms=0, trim_db=None)
    torch.cuda.synchronize()
    assert got.shape == (3, max(out_lens)) and len(set(out_lens)) == 3
    for q in range(3):
        want = torch.cat([dev[r, begin[r]:begin[r] + length[r]] for r in range(5) if row_req[r] == q])
        assert out_lens[q] == want.shape[0] and torch.equal(bits(got[q, :out_lens[q]]), bits(want)), q
        assert not bits(got[q, out_lens[q]:]).any()


def test_join_rows_trim_fades_and_pauses_by_hand():
    """join_rows = block_energy -> sentence_windows -> join_layout -> f5_wave_join, with per-request settings; the trimmed windows
    are the ones the loud middles dictate, and the result passes the reference's checker"""
    x, begin, length = _decoded(2)
    dev = pad_in(torch.from_numpy(x), DEV)
    row_req = [0, 0, 1, 2, 2]
    got, out_lens = A.join_rows(dev, begin, length, row_req, cross_fade_ms=[10, 0, 2.5], pause_ms=[0, 0, 100], trim_db=[-42, None, -42])
    torch.cuda.synchronize()
    lens = [b + n for b, n in zip(begin, length)]
    energy = A.block_energy(dev, lens, 240).cpu().numpy()
    b2, n2 = A.sentence_windows(energy, begin, length, 240, -42.0, 5)
    for r in range(5):
        lo, hi = begin[r] + 1500 + 97 * r, begin[r] + length[r] - 1700 - 31 * r                    # the loud middle
        assert begin[r] <= b2[r] <= lo and hi <= b2[r] + n2[r] <= begin[r] + length[r]
        assert lo - b2[r] <= 5 * 240 + 239 and b2[r] + n2[r] - hi <= 5 * 240 + 239               # 5 blocks of margin and block rounding
        assert b2[r] > begin[r] and b2[r] + n2[r] < begin[r] + length[r]                         # both edges lose something
    b2[2], n2[2] = begin[2], length[2]                                                           # request 1 asked for no trim
    table, want_lens, Lout = A.join_layout(b2, n2, row_req, fade=[240, 0, 60], gap=[0, 0, 2400])
    assert out_lens == want_lens and got.shape == (3, Lout)
    assert table[0, 1, 4] == 240 and table[2, 1, 4] == 60 and table[2, 1, 0] == n2[3] + 2400
    bad = WJ.check(got.cpu().numpy(), x, table, Lout)
    assert not bad, "\n".join(bad)
    # without a trim there is no energy launch: the rows' whole ranges are joined
    got2, lens2 = A.join_rows(dev, begin, length, row_req, cross_fade_ms=10)
    assert lens2 == [length[0] + length[1] - 240, length[2], length[3] + length[4] - 240]


def test_batched_resample_of_the_padded_result():
    """three requests of different lengths, 24 kHz -> 16 kHz: ONE resample call on the zero-padded [Q, Lout] batch, sliced to
    ceil(n len / o), has the bits of audio.resample on every request by itself"""
    x, begin, length = _decoded(3)
    dev = pad_in(torch.from_numpy(x), DEV)
    joined, out_lens = A.join_rows(dev, begin, length, [0, 0, 1, 2, 2], cross_fade_ms=10)
    assert len(set(out_lens)) == 3 and out_lens[1] % 3 and joined.shape[1] == max(out_lens)
    got = A.resample_rows(joined, out_lens, 24_000, 16_000)
    torch.cuda.synchronize()
    for q in range(3):
        want = A.resample(joined[q, :out_lens[q]].contiguous(), 24_000, 16_000)[0]
        assert want.shape[0] == -(-2 * out_lens[q] // 3) and got[q].shape == want.shape
        assert torch.equal(bits(got[q].contiguous()), bits(want)), q
    same = A.resample_rows(joined, out_lens, 24_000, 24_000)                 # equal rates: the slices themselves
    assert all(torch.equal(same[q], joined[q, :out_lens[q]]) for q in range(3))


# ---- end to end on the tiny model -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_x3():
    m = DiT.from_config(TINY, precision="bf16x3", device=DEV)
    m.load_weights(synthetic_weights(TINY, seed=42))
    return m


@pytest.fixture(scope="module")
def vocos():
    from f5_tts_mlx_amd.vocos import Vocos, synthetic_vocos_weights
    return Vocos(synthetic_vocos_weights(seed=7), precision="f16", device=DEV, use_graph=False)


def _bundled():
    audio, sr = G.read_wav(os.path.join(os.path.dirname(G.__file__), "assets", "test_en_1_ref_short.wav"))
    assert sr == 24_000
    return np.asarray(audio, np.float64).astype(np.float32)


def _requests(tmp_path):
    """two short references (tests/test_multivoice_gpu.py): 40 frames of the bundled recording; a burst of noise given at 16 kHz.
    The first request has three sentences, the second one"""
    src = _bundled()
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b16k.wav")
    G.write_wav(a, src[24_000:24_000 + 40 * 256 + 77], 24_000)
    r = np.random.default_rng(28)
    x = r.standard_normal(6400) * 1e-4
    x[1600:4800] = r.standard_normal(3200) * 0.05
    G.write_wav(b, x.astype(np.float32), 16_000)
    return [("Hello there. This one is a longer sentence, is it not? Short.", a, "some call me nature."), ("Short one", b, "others call me.")]


def _decode_by_hand(f5, voc, reqs, seed):
    """prepare_references -> sample(mel, text, durations, lens = frames) -> ONE ragged decode -> (decoded rows, reference samples per
    row, the end of every row, the request of every row)"""
    loaded = [G.read_wav(p) for _, p, _ in reqs]
    refs = A.prepare_references([torch.from_numpy(a).to(torch.float32) for a, _ in loaded], [int(sr) for _, sr in loaded], device=DEV)
    sentences = [G.split_sentences(t) or [t.strip()] for t, _, _ in reqs]
    row_req = [i for i, ss in enumerate(sentences) for _ in ss]
    texts = G.convert_char_to_pinyin([reqs[i][2] + " " + s for i, ss in enumerate(sentences) for s in ss])
    est = [int(G.estimated_duration(np.zeros(refs.samples[i]), reqs[i][2], reqs[i][0], 1.0) * G.FRAMES_PER_SEC) for i in range(len(reqs))]
    mel, _ = f5.sample(refs.mel[torch.tensor(row_req, device=DEV)], text=texts, duration=torch.tensor([est[i] for i in row_req]),
                       lens=torch.tensor([refs.frames[i] for i in row_req]), steps=4, method="euler", seed=seed)
    frames = list(f5.last_durations)
    return voc(mel, lens=frames), [refs.samples[i] for i in row_req], [256 * (f - 1) for f in frames], row_req


def test_generate_many_joined_equals_the_pipeline_by_hand(tmp_path, tiny_x3, vocos):
    """generate_many(cross_fade_ms=10, trim_sentence_db=-42) = prepare_references -> sample -> decode -> join_rows, bit for bit; the
    same call without the new arguments = the torch.cat of the slices it has always been; with output_sample_rate the joined call
    is the batched resample of the same result"""
    reqs = _requests(tmp_path)
    kw = dict(steps=4, method="euler", seed=5, estimate_duration=True)
    f5 = F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB, vocoder=vocos.decode)
    got = G.generate_many(reqs, f5tts=f5, cross_fade_ms=10, trim_sentence_db=-42, **kw)
    plain = G.generate_many(reqs, f5tts=f5, **kw)
    at16k = G.generate_many(reqs, f5tts=f5, cross_fade_ms=10, trim_sentence_db=-42, output_sample_rate=16_000, **kw)
    decoded, n_ref, ends, row_req = _decode_by_hand(F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB), vocos.decode, reqs, 5)
    assert row_req == [0, 0, 0, 1]
    begin, length = n_ref, [e - b for e, b in zip(ends, n_ref)]
    assert min(length) > 480
    want, want_lens = A.join_rows(decoded, begin, length, row_req, cross_fade_ms=10, pause_ms=0, trim_db=-42)
    cat = [torch.cat([decoded[r, begin[r]:ends[r]] for r in range(4) if row_req[r] == q]) for q in range(2)]
    torch.cuda.synchronize()
    for q in range(2):
        assert got[q].shape == (want_lens[q],) and got[q].numel() > 0 and torch.isfinite(got[q]).all()
        assert torch.equal(bits(got[q].contiguous()), bits(want[q, :want_lens[q]].contiguous())), q
        assert plain[q].shape == cat[q].shape and torch.equal(bits(plain[q]), bits(cat[q])), q
        r16 = A.resample(got[q].contiguous(), 24_000, 16_000)[0]
        assert at16k[q].shape == r16.shape and torch.equal(bits(at16k[q].contiguous()), bits(r16)), q
    assert got[0].shape[0] < plain[0].shape[0]                              # two cross-fades (and whatever the trim found) shorter
    print(f"[sentence_joins] request lengths plain {[int(w.shape[0]) for w in plain]}, joined {want_lens}")


def test_generate_cross_fade_is_shorter_by_the_overlaps(tmp_path, tiny_x3, vocos):
    """generate(batch_sentences=True, vocode_batched=True, cross_fade_ms=10) against the plain call: shorter by the sum of the overlaps
    join_layout computes from the sentences' lengths, the same bits up to the first fade and after the last one; the per-sentence decode
    path (vocode_batched=False), which copies its rows into a padded buffer first, gives the same wave"""
    wav = str(tmp_path / "ref12.wav")
    G.write_wav(wav, _bundled()[24_000:24_000 + 12 * 256], 24_000)
    f5 = F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB, vocoder=vocos.decode)
    text = "Hello there. This one is a longer sentence, is it not? Short."
    kw = dict(ref_audio_path=wav, ref_audio_text="some call me nature.", steps=4, method="euler", seed=5, estimate_duration=True, f5tts=f5,
              batch_sentences=True)
    plain = G.generate(text, vocode_batched=True, **kw)
    frames = list(f5.last_durations)
    got = G.generate(text, vocode_batched=True, cross_fade_ms=10, **kw)
    rows = G.generate(text, vocode_batched=False, cross_fade_ms=10, **kw)
    torch.cuda.synchronize()
    n_ref = 12 * 256
    length = [256 * (f - 1) - n_ref for f in frames]
    table, out_lens, _ = A.join_layout([n_ref] * 3, length, [0, 0, 0], fade=240, gap=0)
    overlaps = int(table[0, :, 4].sum())
    assert overlaps == 2 * 240 and sum(length) == plain.shape[0]
    assert got.shape[0] == plain.shape[0] - overlaps == out_lens[0]
    head, tail = length[0] - 240, length[2] - 240
    assert torch.equal(bits(got[:head].contiguous()), bits(plain[:head].contiguous()))
    assert torch.equal(bits(got[-tail:].contiguous()), bits(plain[-tail:].contiguous()))
    assert not torch.equal(got[head:head + 240], plain[head:head + 240]) and torch.isfinite(got).all()
    if 3 * max(frames) <= 896:                                              # the padded batch stays on the GEMM kernels its rows reach alone
        assert torch.equal(bits(rows.contiguous()), bits(got.contiguous()))
    else:
        assert rows.shape == got.shape
    # one sentence: the trim alone sends it through the join, and only cuts
    one = G.generate("Hello there.", ref_audio_path=wav, ref_audio_text="some call me nature.", steps=4, method="euler", seed=5,
                     estimate_duration=True, f5tts=f5)
    cut = G.generate("Hello there.", ref_audio_path=wav, ref_audio_text="some call me nature.", steps=4, method="euler", seed=5,
                     estimate_duration=True, f5tts=f5, trim_sentence_db=-42)
    assert 0 < cut.shape[0] <= one.shape[0]
    one_l = one.cpu().tolist()
    first = cut[0].item()
    assert first in one_l and torch.equal(cut, one[one_l.index(first):one_l.index(first) + cut.shape[0]])
