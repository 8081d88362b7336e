"""Many voices in one call, on the GPU: the two kernels of the ragged reference front end through the C ABI (csrc/audio.hip
block_energy_kernel, mel_ragged_kernel) with the data and checkers of tests/multivoice_ref.py -- every output between guard bands, every
input followed by NaN, NaN wherever a row must not be read --, then audio.prepare_references, F5TTS.sample with a raw-wave batch and
generate.generate_many on the tiny model against the same pipeline done by hand and against the oracle's batched sample().
tests/test_multivoice_host.py shows the checkers used here flagging each seeded mistake.  Every test of this file needs entry points
that did not exist before the feature."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import convaudio_matrix as CM
import multivoice_ref as MV
from f5test import DEV, E, O, P, TINY, stream, synthetic_weights
from rowops_matrix import Out, bits, pad_in
from f5_tts_mlx_amd import audio as A
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-3                                        # the bar of tests/test_model_gpu.py::test_generate_batch_sentences
VOCAB = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _i32(values):
    return pad_in(torch.tensor(list(values), dtype=torch.int32), DEV)


# ---- f5_wave_block_energy -----------------------------------------------------------------------------------------------------------
def _energy(lib, wave_dev, B, L, lens, block):
    """one call through the C ABI into a guarded buffer -> (rc, energy on the host, guard findings)"""
    nblk = -(-L // block)
    out, lens_dev = Out((B, nblk), torch.float32, DEV), _i32(lens)
    rc = lib.f5_wave_block_energy(P(wave_dev), B, L, P(lens_dev), block, P(out.t), nblk, stream())
    torch.cuda.synchronize()
    return rc, out.t.cpu(), out.guard_violations("energy")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("block", [1, 7, 240, 4096])
def test_block_energy(lib, block, B):
    """against fp64 sums of the same fp32 samples, |E^ - E| <= 1.01 block 2^-24 E (multivoice_ref: a bound for any order, nothing
    measured); blocks past lens exactly 0; NaN at and past lens[b] of every row; row b of a batch = the call on row b alone, bit for bit"""
    bad = []
    for L in (1, block - 1, block, block + 1, 3 * block + 17):
        if L == 0:                                                        # (block 1) a successful call without a launch: nothing written
            out = Out((B, 1), torch.float32, DEV)
            nan, zeros = pad_in(torch.full((B, 1), float("nan")), DEV), _i32([0] * B)
            assert lib.f5_wave_block_energy(P(nan), B, 0, P(zeros), block, P(out.t), 0, stream()) == 0, lib.f5_last_error()
            torch.cuda.synchronize()
            assert bool((bits(out.raw) == bits(out.raw)[0]).all())
            continue
        lens = MV.energy_lens(L, block)
        w = MV.energy_wave(np.random.default_rng(1000 * block + L), 3, L, lens)
        dev = pad_in(w, DEV)
        alone = []
        for b in range(3):                                                # each row by itself: B = 1 with lens = L, 0 and mid-block
            rc, got, guards = _energy(lib, dev[b], 1, L, lens[b:b + 1], block)
            assert rc == 0, lib.f5_last_error()
            bad += [f"block {block} L {L} row {b} alone: {m}" for m in guards + MV.chk_block_energy(w[b:b + 1], lens[b:b + 1], block, got)]
            alone.append(got)
        if B == 3:
            rc, got, guards = _energy(lib, dev, 3, L, lens, block)
            assert rc == 0, lib.f5_last_error()
            bad += [f"block {block} L {L} batch: {m}" for m in guards + MV.chk_block_energy(w, lens, block, got)]
            for b in range(3):
                if not torch.equal(bits(got[b]), bits(alone[b][0])):
                    bad.append(f"block {block} L {L}: row {b} of the batch has not the bits of the call on that row alone")
    assert not bad, "\n".join(bad[:20])


def test_block_energy_wrapper_and_clamped_lens(lib):
    """audio.block_energy = the C call; a lens outside 0 .. L is clamped in the kernel: wrong by definition, but inside the buffers"""
    L, block = 3 * 240 + 17, 240
    lens = MV.energy_lens(L, block)
    w = MV.energy_wave(np.random.default_rng(7), 3, L, lens)
    dev = pad_in(w, DEV)
    got = A.block_energy(dev, lens, block)
    torch.cuda.synchronize()
    assert got.shape == (3, 4) and not MV.chk_block_energy(w, lens, block, got.cpu())
    assert torch.equal(A.block_energy(dev, torch.tensor(lens, dtype=torch.int32, device=DEV)), got)
    finite = pad_in(torch.nan_to_num(w, nan=0.5), DEV)
    rc, clamped, guards = _energy(lib, finite, 3, L, [L + 1000, -5, 2 ** 31 - 1], block)
    rc2, want, _ = _energy(lib, finite, 3, L, [L, 0, L], block)
    assert rc == 0 and rc2 == 0 and not guards and torch.equal(bits(clamped), bits(want))


# ---- f5_mel_spectrogram_ragged --------------------------------------------------------------------------------------------------------
ROWSETS = ((0, 1, 2, 3), (0, 1, 2), (1, 2, 3))           # all four rows of multivoice_ref.mel_rows, and batches of three of them


def _plain_mel(lib, x, window, fb, hop, n_mels):
    """f5_mel_spectrogram on one contiguous recording"""
    F = x.numel() // hop
    out = torch.empty((F, n_mels), dtype=torch.float32, device=DEV)
    x_dev = pad_in(x, DEV)
    E.check(lib.f5_mel_spectrogram(P(x_dev), C.c_int64(x.numel()), P(window), P(fb), 1024, hop, n_mels, P(out), stream()), "f5_mel_spectrogram")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("gain", [None, MV.MEL_GAINS], ids=["nogain", "gain"])
@pytest.mark.parametrize("n_mels", [1, 100])
@pytest.mark.parametrize("hop", [256, 100])
def test_mel_ragged(lib, hop, n_mels, gain):
    """rows (0, L), (17, 1025), (L - 255, 255) and (0, hop) of a [.][5 x 256 + 3] buffer that is NaN outside the slices: the bits of
    f5_mel_spectrogram on contiguous pre-scaled copies, exact zeros past each row's frames, guards intact, and the fp64 interval of
    tests/convaudio_matrix.py on the valid frames; N = the largest frame count and that plus 2"""
    rows_all = MV.mel_rows(hop)
    w_all = MV.mel_wave(np.random.default_rng(hop + n_mels), rows_all)
    window_h, fb_h = CM._hann(), CM.mel_filterbank(n_mels)
    window, fb = pad_in(window_h, DEV), pad_in(fb_h, DEV)
    plain_all = [_plain_mel(lib, MV.scaled_slice(w_all, b, b0, n, gain), window, fb, hop, n_mels) if n >= hop else None
                 for b, (b0, n) in enumerate(rows_all)]
    bad = []
    for pick in ROWSETS:
        rows, w, plain = [rows_all[i] for i in pick], w_all[list(pick)].contiguous(), [plain_all[i] for i in pick]
        g = None if gain is None else [gain[i] for i in pick]
        B, L = w.shape
        dev = pad_in(w, DEV)
        frames = [n // hop for _, n in rows]
        for N in (max(frames), max(frames) + 2):
            out = Out((B, N, n_mels), torch.float32, DEV, guard=2 * n_mels)
            begin_dev, lens_dev = _i32(b0 for b0, _ in rows), _i32(n for _, n in rows)
            gain_dev = None if g is None else pad_in(torch.tensor(g, dtype=torch.float32), DEV)
            rc = lib.f5_mel_spectrogram_ragged(P(dev), B, L, P(begin_dev), P(lens_dev), P(gain_dev), P(window), P(fb), 1024, hop, n_mels,
                                               P(out.t), N, stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.f5_last_error()
            got = out.t.cpu()
            found = out.guard_violations("out") + MV.chk_mel_ragged(got, plain, rows, hop, N) + MV.chk_mel_interval(got, w, rows, g, window_h, fb_h, hop)
            bad += [f"rows {pick} N {N}: {m}" for m in found]
    assert not bad, "\n".join(bad[:20])


def test_mel_ragged_wrapper_melspec_and_clamped_slices(lib):
    """audio.log_mel_spectrogram_ragged / MelSpec(audio, lens=...) with the production tables = log_mel_spectrogram of each slice; a
    begin / lens outside the row is clamped in the kernel: wrong by definition, but inside the buffers"""
    r = np.random.default_rng(11)
    L = 7 * 256 + 40
    w = torch.from_numpy((r.standard_normal((3, L)) * 0.1).astype(np.float32))
    lens, begin = [L, 3 * 256 + 9, 255], [0, 300, 5]
    for b in range(3):
        w[b, :begin[b]] = float("nan")
        w[b, begin[b] + lens[b]:] = float("nan")
    dev = pad_in(w, DEV)
    got = A.log_mel_spectrogram_ragged(dev, lens, begin)
    assert got.shape == (3, 7, 100)
    for b in range(3):
        F = lens[b] // 256
        if F:
            assert torch.equal(bits(got[b, :F]), bits(A.log_mel_spectrogram(dev[b, begin[b]:begin[b] + lens[b]].contiguous())[0]))
        assert not bits(got[b, F:]).any()
    w0 = torch.nan_to_num(w, nan=0.0)
    w0[1, :lens[1]] = w[1, begin[1]:begin[1] + lens[1]]
    spec = A.MelSpec(device=DEV)
    m = spec(w0, lens=lens)                                                                     # host input goes to the MelSpec's device
    assert torch.equal(m, A.log_mel_spectrogram_ragged(pad_in(w0, DEV), lens)) and torch.equal(bits(m[:2]), bits(got[:2]))
    assert torch.equal(spec(w0[:1]), A.log_mel_spectrogram(w0[:1].to(DEV)))                     # without lens: what it was
    assert A.log_mel_spectrogram_ragged(dev, [10, 20, 255], begin).shape == (3, 0, 100)          # no frame anywhere: no launch
    # clamping: (begin, lens) = (-7, L + 50) is the whole row, (L + 9, 300) and (5, -1) are empty
    finite = pad_in(torch.nan_to_num(w, nan=0.25), DEV)
    window, fb = A._tables(torch.device(DEV), 24_000, 1024, 100)
    outs = []
    for bg, ln in (([-7, L + 9, 5], [L + 50, 300, -1]), ([0, L, 5], [L, 0, 0])):
        out, begin_dev, lens_dev = Out((3, 7, 100), torch.float32, DEV, guard=200), _i32(bg), _i32(ln)
        E.check(lib.f5_mel_spectrogram_ragged(P(finite), 3, L, P(begin_dev), P(lens_dev), P(None), P(window), P(fb), 1024, 256, 100, P(out.t), 7,
                                              stream()), "f5_mel_spectrogram_ragged")
        torch.cuda.synchronize()
        assert not out.guard_violations("out")
        outs.append(out.t.cpu())
    assert torch.equal(bits(outs[0]), bits(outs[1])) and not bits(outs[0][1:]).any()


# ---- prepare_references -----------------------------------------------------------------------------------------------------------------
def _bundled():
    audio, sr = G.read_wav(os.path.join(os.path.dirname(G.__file__), "assets", "test_en_1_ref_short.wav"))
    assert sr == 24_000
    return torch.from_numpy(np.asarray(audio)).to(torch.float32)


def _burst16k():
    """one second at 16 kHz: a burst of noise between a quarter of a second of near silence (-80 dB) on either side"""
    r = np.random.default_rng(16)
    x = r.standard_normal(16_000) * 1e-4
    x[4000:12_000] = r.standard_normal(8000) * 0.05
    return torch.from_numpy(x.astype(np.float32))


def _host_rules(energy, lens, trim_db, keep_blocks, block=240, target=0.1):
    """the window and gain rules restated: fp64 on the block energies"""
    begin, length, gain = [], [], []
    for b, n in enumerate(lens):
        nb = -(-n // block)
        e = energy[b, :nb].astype(np.float64)
        b_blk, e_blk = 0, nb
        if trim_db is not None:
            n_k = np.array([min((k + 1) * block, n) - k * block for k in range(nb)], np.float64)
            loud = [k for k in range(nb) if e[k] > 0 and 10.0 * np.log10(e[k] / n_k[k]) > trim_db]
            b_blk, e_blk = max(0, loud[0] - keep_blocks), min(nb, loud[-1] + 1 + keep_blocks)
        begin.append(b_blk * block)
        length.append(min(e_blk * block, n) - b_blk * block)
        total = 0.0
        for k in range(b_blk, e_blk):
            total += float(e[k])
        rms = np.sqrt(total / length[-1])
        gain.append(np.float32(target / rms) if rms < target else np.float32(1.0))
    return begin, length, gain


@pytest.mark.parametrize("trim_db", [None, -42.0], ids=["whole", "trimmed"])
def test_prepare_references(trim_db):
    """the bundled recording, the same at a quarter of its level (the gain path runs) and a burst with silent edges given at 16 kHz:
    frames, samples, begin and gain are the host rules on the block energies, the mel is the per-row path done by hand -- resample,
    slice, multiply by the same fp32 gain, plain mel -- bit for bit, zero past each row's frames"""
    src = _bundled()
    waves, rates = [src, src * 0.25, _burst16k()], [24_000, 24_000, 16_000]
    refs = A.prepare_references(waves, rates, trim_silence_db=trim_db, device=DEV)
    rows = [waves[0].to(DEV), waves[1].to(DEV), A.resample(waves[2], 16_000, 24_000, device=DEV)[0]]
    lens = [int(r.shape[0]) for r in rows]
    assert lens[2] == 24_000
    buf = torch.zeros((3, max(lens)), device=DEV)
    for i, r in enumerate(rows):
        buf[i, :lens[i]] = r
    energy = A.block_energy(buf, lens, 240).cpu().numpy()
    begin, length, gain = _host_rules(energy, lens, trim_db, 5)
    assert refs.begin == begin and refs.samples == length and refs.frames == [n // 256 for n in length]
    assert refs.gain.dtype == np.float32 and refs.gain.tolist() == [float(g) for g in gain]
    assert refs.gain[1] > 1.0 and refs.mel.shape == (3, max(refs.frames), 100)
    if trim_db is None:
        assert begin == [0, 0, 0] and length == lens
    else:
        assert begin[0] == 2 * 240 and begin[0] + length[0] == 505 * 240                        # (tests/test_multivoice_host.py)
        assert 0 < begin[2] <= 6000 - 5 * 240 + 240 and 18_000 + 5 * 240 - 240 <= begin[2] + length[2] < 24_000
    for i in range(3):
        x = rows[i][begin[i]:begin[i] + length[i]] * torch.tensor(gain[i], dtype=torch.float32, device=DEV)
        want = A.log_mel_spectrogram(x.contiguous())[0]
        F = refs.frames[i]
        assert want.shape[0] == F
        assert torch.equal(bits(refs.mel[i, :F]), bits(want)), i
        assert not bits(refs.mel[i, F:]).any(), i


def test_prepare_references_refuses():
    with pytest.raises(ValueError, match="row 1: no block"):
        A.prepare_references([_bundled()[:4800], torch.zeros(4800)], trim_silence_db=-42.0, device=DEV)
    with pytest.raises(ValueError, match="row 1.*rms 0"):
        A.prepare_references([_bundled()[:4800], torch.zeros(4800)], device=DEV)
    with pytest.raises(ValueError, match="row 0: 200 samples are kept, fewer than one frame"):
        A.prepare_references([_bundled()[24_000:24_200]], device=DEV)
    with pytest.raises(ValueError, match="row 1: resample: ratio"):
        A.prepare_references([_bundled()[:4800], torch.zeros(4800)], [24_000, 192_000], device=DEV)


# ---- sample() and generate_many on the tiny model -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_weights():
    return synthetic_weights(TINY, seed=42)


@pytest.fixture(scope="module")
def tiny_x3(tiny_weights):
    m = DiT.from_config(TINY, precision="bf16x3", device=DEV)
    m.load_weights(tiny_weights)
    return m


def test_sample_takes_a_raw_wave_batch_with_wave_lens(tiny_x3):
    """sample(cond=(b, nw), wave_lens=...) = sample() on the ragged mel with lens = the rows' frame counts (no gain, no trim);
    b > 1 without wave_lens still asserts"""
    src = _bundled()
    n = [30 * 256 + 100, 18 * 256]
    w = torch.full((2, n[0]), float("nan"))
    w[0], w[1, :n[1]] = src[24_000:24_000 + n[0]], src[48_000:48_000 + n[1]]
    f5 = F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB)
    kw = dict(text=["some call me nature. hello there.", "others call me. hi."], duration=torch.tensor([70, 50]), steps=4, method="euler", seed=5)
    got, _ = f5.sample(w, wave_lens=n, **kw)
    assert f5.last_durations == [70, 50]
    mel = A.log_mel_spectrogram_ragged(w, n, device=DEV)
    assert mel.shape == (2, 30, 100)
    want, _ = f5.sample(mel, lens=torch.tensor([30, 18]), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(want))
    with pytest.raises(AssertionError, match="batch 1"):
        f5.sample(torch.nan_to_num(w), **kw)


def _two_voices(tmp_path):
    """two short references and the requests: 40 frames of the bundled recording at 24 kHz; a burst of noise at rms 0.05 (the gain
    path runs) between a tenth of a second of near silence on either side, given at 16 kHz (28 frames once trimmed)"""
    src = _bundled().numpy()
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b16k.wav")
    G.write_wav(a, src[24_000:24_000 + 40 * 256 + 77], 24_000)
    r = np.random.default_rng(28)
    x = r.standard_normal(6400) * 1e-4
    x[1600:4800] = r.standard_normal(3200) * 0.05
    G.write_wav(b, x.astype(np.float32), 16_000)
    return [("Hello there. This one is a longer sentence, is it not?", a, "some call me nature."), ("Short one", b, "others call me.")]


def _by_hand(f5, voc, reqs, trim_db, seed):
    """prepare_references -> sample(mel, text, durations, lens = frames) -> decode each row on its own frames -> the same slices"""
    loaded = [G.read_wav(p) for _, p, _ in reqs]
    refs = A.prepare_references([torch.from_numpy(a).to(torch.float32) for a, _ in loaded], [int(sr) for _, sr in loaded],
                                trim_silence_db=trim_db, device=DEV)
    sentences = [G.split_sentences(t) or [t.strip()] for t, _, _ in reqs]
    row_req = [i for i, ss in enumerate(sentences) for _ in ss]
    texts = G.convert_char_to_pinyin([reqs[i][2] + " " + s for i, ss in enumerate(sentences) for s in ss])
    est = [int(G.estimated_duration(np.zeros(refs.samples[i]), reqs[i][2], reqs[i][0], 1.0) * G.FRAMES_PER_SEC) for i in range(len(reqs))]
    durs = torch.tensor([est[i] for i in row_req])
    lens = torch.tensor([refs.frames[i] for i in row_req])
    cond = refs.mel[torch.tensor(row_req, device=DEV)]
    mel, _ = f5.sample(cond, text=texts, duration=durs, lens=lens, steps=4, method="euler", seed=seed)
    frames = list(f5.last_durations)
    rows = [voc(mel[r:r + 1, :frames[r]]).reshape(-1)[refs.samples[i]:] for r, i in enumerate(row_req)]
    waves = [torch.cat([rows[r] for r, q in enumerate(row_req) if q == i]) for i in range(len(reqs))]
    return waves, dict(refs=refs, row_req=row_req, texts=texts, durs=durs, lens=lens, cond=cond, frames=frames, mel=mel)


def test_generate_many_fake_vocoder_by_hand_and_oracle(tmp_path, tiny_weights, tiny_x3):
    """two requests with different references, two sentences in the first: with the fake frame-synchronous vocoder of
    test_generate_batch_sentences the result is the hand-built pipeline bit for bit, and within MEL_L1_TOL of the fp32 oracle's batched
    sample() on the same prepared mel"""
    from f5_tts_mlx_amd.rng import mlx_like_normal
    from f5_tts_mlx_amd.utils import list_str_to_idx
    idx = torch.arange(256, device=DEV) % 100
    voc = lambda mel: mel[:, :, idx].reshape(mel.shape[0], -1) if mel.shape[0] > 1 else mel[0][:, idx].reshape(-1)   # noqa: E731
    reqs = _two_voices(tmp_path)
    got = G.generate_many(reqs, steps=4, method="euler", seed=5, estimate_duration=True, trim_silence_db=-42.0,
                          f5tts=F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB, vocoder=voc))
    want, h = _by_hand(F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB), voc, reqs, -42.0, 5)
    torch.cuda.synchronize()
    assert h["row_req"] == [0, 0, 1] and len(got) == 2
    assert h["refs"].gain[1] > 1.0 and len(set(h["refs"].frames)) == 2
    for i in range(2):
        assert got[i].shape == want[i].shape and got[i].numel() > 0 and torch.equal(bits(got[i]), bits(want[i])), i
    # the oracle on the same prepared mel, lens and clamped durations, with the noise sample() draws for seed 5
    durs, N = h["frames"], max(h["frames"])
    y0 = torch.zeros((3, N, 100))
    for r, d in enumerate(durs):
        y0[r, :d] = torch.from_numpy(mlx_like_normal(5, (100, d)).T.copy())
    ref, _ = O.sample(O.DiTOracle(TINY, tiny_weights), h["cond"].cpu(), list_str_to_idx(h["texts"], VOCAB), torch.tensor(durs), lens=h["lens"],
                      y0=y0, steps=4, method="euler")
    refs = h["refs"]
    for i in range(2):
        o = torch.cat([ref[r][:, idx.cpu()].reshape(-1)[refs.samples[i]:durs[r] * 256] for r, q in enumerate(h["row_req"]) if q == i])
        assert o.shape == got[i].shape
        l1 = float((got[i].cpu() - o).abs().mean())
        print(f"[generate_many] request {i}: vs the oracle's batched sample() {l1:.3e} (bar {MEL_L1_TOL:g})")
        assert l1 <= MEL_L1_TOL, (i, l1)


def test_generate_many_vocos_ragged_decode_equals_per_row(tmp_path, tiny_x3):
    """with a seeded random-weight Vocos, whose decode takes `lens`, generate_many makes ONE ragged decode call: the bits of decoding
    each row on its own frames"""
    from f5_tts_mlx_amd.vocos import Vocos, synthetic_vocos_weights
    voc = Vocos(synthetic_vocos_weights(seed=7), precision="f16", device=DEV, use_graph=False)
    assert G._takes_lens(voc.decode)
    reqs = _two_voices(tmp_path)
    got = G.generate_many(reqs, steps=4, method="euler", seed=5, estimate_duration=True,
                          f5tts=F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB, vocoder=voc.decode))
    want, h = _by_hand(F5TTS(transformer=tiny_x3, vocab_char_map=VOCAB), voc.decode, reqs, None, 5)
    torch.cuda.synchronize()
    assert 3 * max(h["frames"]) <= 896                                   # the padded batch stays on the GEMM kernels its rows reach alone
    for i in range(2):
        assert got[i].shape == want[i].shape and got[i].numel() > 0 and torch.isfinite(got[i]).all()
        assert torch.equal(bits(got[i]), bits(want[i])), i
