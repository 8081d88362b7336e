"""The resampling kernel (csrc/audio.hip resample_kernel) through f5_resample_batch against the fp64 statement of the filter: every
case of tests/resample_matrix.py -- eleven rate pairs, lengths from 1 sample to past nine 256-output boundaries, batches of 1 and 3,
noise / impulses / ones -- between guard bands, under the bound that matrix derives; then the properties of the launch (batch =
single launches, any stream, the two calls that launch nothing) and the wiring of generate().  tests/test_resample_host.py shows on
the CPU that the checker used here flags the mistakes a resampling kernel can make.

Wall time on one MI355X: 12.7 s for the module (24 tests, 6 432 matrix cases; the slowest item, 48 kHz -> 24 kHz, 1.2 s, most of it the
fp64 reference).
"""
import ctypes as C
import dataclasses
import math
import time

import numpy as np
import pytest
import torch

import resample_matrix as RM
from f5test import DEV, E, P, TINY, stream, synthetic_weights
from f5_tts_mlx_amd import audio as A

pytestmark = pytest.mark.gpu

PAIR_IDS = [f"{a}-{b}" for a, b in RM.PAIRS]


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def dev_table(pair):
    """the compact table of the matrix (not the package's) on the device"""
    taps, first, T = RM.compact(RM.table(*pair))
    return torch.from_numpy(taps).to(DEV), torch.from_numpy(first).to(DEV), T


def launch(lib, tb, x, taps, first, T, out, s=None):
    B, L = x.shape
    return lib.f5_resample_batch(P(x), B, C.c_int64(L), P(taps), P(first), tb.o, tb.n, T, tb.width, P(out), C.c_int64(out.shape[1]),
                                 stream() if s is None else s)


@pytest.mark.parametrize("pair", RM.PAIRS, ids=PAIR_IDS)
def test_matrix(lib, pair):
    tb = RM.table(*pair)
    taps, first, T = dev_table(pair)
    cs = RM.cases(pair)
    failures, t0 = [], time.perf_counter()
    for c in cs:
        io = RM.IO(c, device=DEV)
        rc = launch(lib, tb, io.x, taps, first, T, io.out)
        if rc != 0:
            failures.append(f"{c.id}: refused: {lib.f5_last_error().decode()}")
            continue
        torch.cuda.synchronize()
        failures += RM.check(c, io.result())
    print(f"[resample matrix] {pair[0]} -> {pair[1]} ({tb.o}:{tb.n}, T = {T}): {len(cs)} cases, {time.perf_counter() - t0:.2f} s")
    assert not failures, f"{len(failures)} findings:\n" + "\n".join(failures[:25])


def _edge_cases(pair):
    """noise at the lengths around the first and second tile boundary, and the shortest"""
    return [c for c in RM.cases(pair) if c.signal == "noise" and c.B == 3 and (c.L <= 3 or 1018 <= c.L_out <= 1030 or 2040 <= c.L_out <= 2056)]


@pytest.mark.parametrize("pair", RM.PAIRS, ids=PAIR_IDS)
def test_batch_equals_single_launches_on_any_stream(lib, pair):
    tb = RM.table(*pair)
    taps, first, T = dev_table(pair)
    side = torch.cuda.Stream(device=DEV)
    cs = _edge_cases(pair)
    assert len(cs) >= 6
    for c in cs:
        x = torch.from_numpy(RM.signal(c)).to(DEV)
        batch = torch.full((c.B, c.L_out), float("nan"), device=DEV)
        E.check(launch(lib, tb, x, taps, first, T, batch), "f5_resample_batch")
        for b in range(c.B):
            one = torch.full((1, c.L_out), float("nan"), device=DEV)
            E.check(launch(lib, tb, x[b:b + 1], taps, first, T, one), "f5_resample_batch")
            assert torch.equal(one[0].view(torch.int32), batch[b].view(torch.int32)), (c.id, b)
        torch.cuda.synchronize()                                            # x and the tables are ready before the other stream reads them
        other = torch.full((c.B, c.L_out), float("nan"), device=DEV)
        with torch.cuda.stream(side):
            E.check(launch(lib, tb, x, taps, first, T, other, s=C.c_void_p(side.cuda_stream)), "f5_resample_batch")
        side.synchronize()
        assert torch.equal(other.view(torch.int32), batch.view(torch.int32)), c.id


def test_python_entry_matches_the_matrix_and_the_calls_without_a_launch():
    c = RM.Case(44_100, 24_000, 3765, 3, "noise")
    x = RM.signal(c)
    got = A.resample(x, 44_100, 24_000, device=DEV)                           # host input, the package's own table
    assert got.shape == (3, c.L_out) and got.dtype == torch.float32 and got.is_cuda
    raw = np.empty(2 * RM.GUARD + got.numel(), np.float32)
    raw.view(np.uint32)[:] = RM.SENT32
    raw[RM.GUARD:-RM.GUARD] = got.cpu().numpy().reshape(-1)
    assert not RM.check(c, raw)
    one = A.resample(torch.from_numpy(x[1]).to(DEV), 44_100, 24_000)          # [t] on the device, no device argument
    assert one.shape == (1, c.L_out) and torch.equal(one[0], got[1])
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = A.resample(torch.from_numpy(x).to(DEV), 44_100, 24_000)
    side.synchronize()
    assert torch.equal(other, got)
    # equal rates: the same values, nothing launched; no samples: an empty result
    xd = torch.from_numpy(x).to(DEV)
    same = A.resample(xd, 24_000, 24_000)
    assert same.data_ptr() == xd.data_ptr() and torch.equal(same, xd)
    assert torch.equal(A.resample(x[0], 16_000, 16_000, device=DEV), xd[0:1])
    empty = A.resample(torch.zeros((2, 0)), 16_000, 24_000, device=DEV)
    assert empty.shape == (2, 0) and empty.dtype == torch.float32 and empty.is_cuda
    assert A.resample(np.zeros(0, np.float32), 48_000, 24_000).shape == (1, 0)
    with pytest.raises(ValueError, match="ratio 8:1 too large"):
        A.resample(xd, 8, 1)
    with pytest.raises(ValueError, match="positive integer"):
        A.resample(xd, 0, 24_000)


@pytest.fixture(scope="module")
def f5():
    """the model of tests/test_model_gpu.py::test_generate_end_to_end"""
    from f5_tts_mlx_amd.cfm import F5TTS
    from f5_tts_mlx_amd.dit import DiT
    from f5_tts_mlx_amd.vocos import Vocos, synthetic_vocos_weights
    vocab = {v: i for i, v in enumerate(open(str(E.library_path().parent.parent / "assets" / "vocab.txt")).read().split("\n"))}
    cfg = dataclasses.replace(TINY, text_num_embeds=len(vocab) - 1)
    model = DiT.from_config(cfg, precision="bf16", device=DEV)
    model.load_weights(synthetic_weights(cfg, seed=1))
    voc = Vocos(synthetic_vocos_weights(seed=7), device=DEV)
    return F5TTS(transformer=model, vocab_char_map=vocab, vocoder=voc.decode)


def test_generate_resamples_the_reference_and_the_result(f5, tmp_path):
    import pkgutil
    from f5_tts_mlx_amd import generate as G
    ref24, sr = G.read_wav(pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav"))
    assert sr == 24_000
    ref16 = A.resample(torch.from_numpy(ref24).to(torch.float32), 24_000, 16_000, device=DEV)[0]
    assert ref16.shape[0] == math.ceil(2 * ref24.shape[0] / 3)
    p16, p24 = tmp_path / "ref16k.wav", tmp_path / "ref24k.wav"
    G.write_wav(str(p16), ref16.cpu().numpy(), 16_000)
    back24 = A.resample(ref16, 16_000, 24_000)[0]
    G.write_wav(str(p24), back24.cpu().numpy(), 24_000)
    kw = dict(ref_audio_text=G.DEFAULT_REF_TEXT, duration=7.0, steps=3, method="euler", seed=0, f5tts=f5)
    # (a) a 16 kHz reference with resample_ref = the 24 kHz file that holds the resampled samples, without
    with pytest.raises(ValueError, match="24kHz"):
        G.generate("Hello world.", ref_audio_path=str(p16), **kw)
    a = G.generate("Hello world.", ref_audio_path=str(p16), resample_ref=True, **kw)
    plain = G.generate("Hello world.", ref_audio_path=str(p24), **kw)
    assert a.ndim == 1 and a.shape[0] > 0 and torch.isfinite(a).all()
    assert torch.equal(a, plain)
    # (b) the result at 16 kHz: one resampling of the plain result, returned and written
    out_path = tmp_path / "gen16k.wav"
    b = G.generate("Hello world.", ref_audio_path=str(p24), output_sample_rate=16_000, output_path=str(out_path), **kw)
    assert torch.equal(b, A.resample(plain, 24_000, 16_000)[0])
    assert b.shape[0] == math.ceil(2 * plain.shape[0] / 3) and torch.isfinite(b).all()
    data, sr = G.read_wav(str(out_path))
    assert sr == 16_000 and data.shape[0] == b.shape[0] and np.array_equal(data.astype(np.float32), b.cpu().numpy())
    # 24 000 asked for explicitly is the plain call
    assert torch.equal(G.generate("Hello world.", ref_audio_path=str(p24), output_sample_rate=24_000, **kw), plain)
