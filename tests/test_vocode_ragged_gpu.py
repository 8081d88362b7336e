"""Ragged vocoding on the GPU.  Every row of a padded batch, decoded with `lens`, must be what the existing kernels give for that
row's slice alone -- the same floating-point operations in the same order, so the comparison is `torch.equal`, for each of the three
ragged ops and for the whole decode -- and nothing the padding holds (zeros, NaN, 1e30) may change a bit of the output.

B = 5, N = 41, lens = [41, 40, 38, 2, 17]: a full row, one frame short, exactly one conv halo (3 frames) short, the minimum, and a
mid-length row; B * N = 205 rows is no multiple of the 4 rows per workgroup of the row kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

from f5test import DEV, E, P, TINY, operand_mode, op_dtype, stream, synthetic_weights
from f5_tts_mlx_amd.vocos import HOP, Vocos, synthetic_vocos_weights

pytestmark = pytest.mark.gpu

B, N, LENS = 5, 41, [41, 40, 38, 2, 17]
FILLS = (0.0, float("nan"), 1e30)
# the bounds of test_vocos_decode_parity (mean |error| over the mean magnitude of the oracle's wave), used only where a batch and its
# rows do not reach the same GEMM kernels
ORACLE_TOL = {"bf16x3": 2e-4, "bf16": 2e-3, "f16": 5e-4}
VOCOS_GEMMS = ((0, 512), (8, 1536), (4, 512), (0, 1026))      # (epilogue, N) of the embed, pwconv1, pwconv2 and head GEMMs


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


@pytest.fixture(scope="module")
def lens_dev():
    return torch.tensor(LENS, dtype=torch.int32, device=DEV)


def padded(valid: torch.Tensor, fill: float) -> torch.Tensor:
    """`valid` [B][N][...] with everything past each row's length replaced by `fill`"""
    x = valid.clone()
    for b, ln in enumerate(LENS):
        x[b, ln:] = fill
    return x.to(DEV).contiguous()


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def last_gemm(lib) -> str:
    buf = C.create_string_buffer(64)
    lib.f5_debug_last_gemm_kernel(buf, 64)
    return buf.value.decode()


def gemm_routes(lib, prec: str, M: int):
    """the kernels the four GEMM shapes of the vocoder reach at M rows (the routing function the launcher switches over; no launch)"""
    out = []
    with E.operand_type(prec):
        for epi, n in VOCOS_GEMMS:
            buf = C.create_string_buffer(64)
            assert lib.f5_debug_gemm_route(epi, M, n, 3 if prec == "bf16x3" else 1, 0, 0, 0, buf, 64, None) >= 0
            out.append(buf.value.decode())
    return out


# ---- each ragged op, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_im2col7_ragged(lib, lens_dev, prec):
    r = np.random.default_rng(3)
    valid = torch.from_numpy(r.standard_normal((B, N, 100)).astype(np.float32))
    with operand_mode(prec):
        outs = []
        for fill in FILLS:
            x = padded(valid, fill)
            hi = torch.full((B * N, 7 * 128), 7.0, dtype=op_dtype(), device=DEV)
            lo = torch.full_like(hi, 7.0)
            E.check(lib.f5_op_im2col7_ragged(P(x), P(hi), P(lo), B, N, 100, P(lens_dev), stream()))
            outs.append((hi.view(B, N, -1), lo.view(B, N, -1)))
        hi, lo = outs[0]
        for b, ln in enumerate(LENS):
            xb = valid[b, :ln].to(DEV).contiguous()
            h1 = torch.empty((ln, 7 * 128), dtype=op_dtype(), device=DEV)
            l1 = torch.empty_like(h1)
            E.check(lib.f5_op_im2col7(P(xb), P(h1), P(l1), 1, ln, 100, stream()))
            torch.cuda.synchronize()
            assert torch.equal(bits(hi[b, :ln]), bits(h1)) and torch.equal(bits(lo[b, :ln]), bits(l1)), (b, ln)
            assert not bits(hi[b, ln:]).any() and not bits(lo[b, ln:]).any(), (b, ln)
        for h2, l2 in outs[1:]:
            assert torch.equal(bits(h2), bits(hi)) and torch.equal(bits(l2), bits(lo))


@pytest.mark.parametrize("dim", [512, 1024])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_dwconv_ln_ragged(lib, lens_dev, prec, dim):
    r = np.random.default_rng(dim)
    valid = torch.from_numpy(r.standard_normal((B, N, dim)).astype(np.float32))
    par = [torch.from_numpy(a.astype(np.float32)).to(DEV) for a in (r.standard_normal((dim, 7)) * 0.4, r.standard_normal(dim) * 0.1,
                                                                    1 + 0.1 * r.standard_normal(dim), r.standard_normal(dim) * 0.1)]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with operand_mode(prec):
        outs = []
        try:
            E.check(lib.f5_debug_set_op_sat_flag(P(flag)))
            for fill in FILLS:
                x = padded(valid, fill)
                hi = torch.full((B * N, dim), 7.0, dtype=op_dtype(), device=DEV)
                lo = torch.full_like(hi, 7.0)
                E.check(lib.f5_op_dwconv_ln_ragged(P(x), P(par[0]), P(par[1]), P(par[2]), P(par[3]), P(hi), P(lo), B, N, dim, P(lens_dev),
                                                   stream()))
                outs.append((hi.view(B, N, -1), lo.view(B, N, -1)))
            torch.cuda.synchronize()
            assert int(flag.item()) == 0, "a padding row took part in the saturation report"
        finally:
            E.check(lib.f5_debug_set_op_sat_flag(None))
        hi, lo = outs[0]
        for b, ln in enumerate(LENS):
            xb = valid[b, :ln].to(DEV).contiguous()
            h1 = torch.empty((ln, dim), dtype=op_dtype(), device=DEV)
            l1 = torch.empty_like(h1)
            E.check(lib.f5_op_dwconv_ln(P(xb), P(par[0]), P(par[1]), P(par[2]), P(par[3]), P(h1), P(l1), 1, ln, dim, stream()))
            torch.cuda.synchronize()
            assert torch.equal(bits(hi[b, :ln]), bits(h1)) and torch.equal(bits(lo[b, :ln]), bits(l1)), (b, ln)
            assert not bits(hi[b, ln:]).any() and not bits(lo[b, ln:]).any(), (b, ln)
        for h2, l2 in outs[1:]:
            assert torch.equal(bits(h2), bits(hi)) and torch.equal(bits(l2), bits(lo))


def test_istft_ragged(lib, lens_dev):
    r = np.random.default_rng(5)
    valid = torch.from_numpy(r.standard_normal((B, N, 1026)).astype(np.float32))
    valid[:, :, :513] *= 1.5
    valid[0, 3, 7] = 9.0                                                       # the exp clip at 1e2
    win = torch.hann_window(1024, device=DEV)
    outs = []
    for fill in FILLS:
        y = padded(valid, fill)
        frames = torch.empty((B * N, 1024), device=DEV)
        wave = torch.full((B, HOP * (N - 1)), 7.0, device=DEV)
        E.check(lib.f5_op_istft_ragged(P(y), 1026, P(win), P(frames), P(wave), B, N, 1024, HOP, P(lens_dev), stream()))
        outs.append(wave)
    wave = outs[0]
    for b, ln in enumerate(LENS):
        yb = valid[b, :ln].to(DEV).contiguous()
        fr1 = torch.empty((ln, 1024), device=DEV)
        one = torch.empty(HOP * (ln - 1), device=DEV)
        E.check(lib.f5_op_istft(P(yb), 1026, P(win), P(fr1), P(one), ln, 1024, HOP, stream()))
        torch.cuda.synchronize()
        assert torch.equal(bits(wave[b, :HOP * (ln - 1)]), bits(one)), (b, ln)
        assert not bits(wave[b, HOP * (ln - 1):]).any(), (b, ln)               # exactly +0.0f
    for w2 in outs[1:]:
        assert torch.equal(bits(w2), bits(wave))


# ---- the whole decode ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vweights():
    return synthetic_vocos_weights(seed=7)


@pytest.fixture(scope="module")
def mel_valid():
    r = np.random.default_rng(41)
    return torch.from_numpy((r.standard_normal((B, N, 100)) * 2.0 - 1.0).astype(np.float32))


def _row_check(lib, prec, got_row, mel_row, voc, weights, exact, what):
    """one row of a ragged decode against the plain decode of its slice: bit for bit where both reach the same GEMM kernels, else both
    held to the oracle of the slice at the bound of test_vocos_decode_parity"""
    one = voc.decode(mel_row[None])
    torch.cuda.synchronize()
    assert one.ndim == 1 and one.shape == got_row.shape
    if exact:
        assert torch.equal(bits(got_row), bits(one)), what
        return
    from oracle import vocos_oracle as VO
    kw = dict(emulate_bf16=True) if prec == "bf16" else dict(emulate_f16=True) if prec == "f16" else {}
    want = VO.decode(weights, mel_row[None].cpu(), dtype=torch.float64, **kw)[0]
    refm = float(want.abs().mean())
    for name, w in (("ragged", got_row), ("plain", one)):
        mean = float((w.cpu().double() - want).abs().mean())
        print(f"[vocode_ragged] {what} [{prec}] {name} vs oracle: mean_abs={mean:.3e} ref_mean_abs={refm:.3e}")
        assert mean <= ORACLE_TOL[prec] * max(1e-3, refm) + 1e-6, (what, name)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16", "f16"])
def test_decode_ragged_equals_each_row_alone(lib, vweights, mel_valid, prec):
    voc = Vocos(vweights, precision=prec, device=DEV, use_graph=False)          # eager: the kernel-name hook sees the launches
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs, sat = [], []
    try:
        E.check(lib.f5_debug_set_op_sat_flag(P(flag)))                          # the word the fp16 packers report saturation to
        for fill in FILLS:
            flag.zero_()
            outs.append(voc.decode(padded(mel_valid, fill), lens=LENS))
            torch.cuda.synchronize()
            sat.append(int(flag.item()) & 4)
    finally:
        E.check(lib.f5_debug_set_op_sat_flag(None))
    batch_kernel = last_gemm(lib)
    got = outs[0]
    assert got.shape == (B, HOP * (N - 1)) and torch.isfinite(got).all()
    routes = gemm_routes(lib, prec, B * N)
    for b, ln in enumerate(LENS):
        mel_row = mel_valid[b, :ln].to(DEV)
        exact = gemm_routes(lib, prec, ln) == routes
        _row_check(lib, prec, got[b, :HOP * (ln - 1)], mel_row, voc, vweights, exact, f"row {b} (len {ln})")
        row_kernel = last_gemm(lib)
        assert (row_kernel == batch_kernel) or not exact, (row_kernel, batch_kernel)    # what ran agrees with what the routing said
        print(f"[vocode_ragged] decode [{prec}] row {b} len {ln}: {'exact' if exact else 'oracle-bound'} branch "
              f"(head GEMM {batch_kernel} / {row_kernel})")
        assert not bits(got[b, HOP * (ln - 1):]).any(), (b, ln)
    if prec == "f16":
        assert all(gemm_routes(lib, prec, ln) == routes for ln in LENS), "N was chosen so that f16 takes the exact branch"
    for o in outs[1:]:
        assert torch.equal(bits(o), bits(got))                                  # NaN / 1e30 padding: the bits of the zero fill
    assert sat[1] <= sat[0] and sat[2] <= sat[0], sat                           # no saturation report that the zero fill does not give


def test_decode_ragged_b1_and_tensor_lens(vweights, mel_valid):
    """with `lens` the result is always 2-D, also for one row; an integer tensor serves as `lens`"""
    voc = Vocos(vweights, precision="f16", device=DEV, use_graph=False)
    one = voc.decode(mel_valid[4:5].to(DEV), lens=torch.tensor([17]))
    plain = voc.decode(mel_valid[4:5, :17].to(DEV))
    torch.cuda.synchronize()
    assert one.shape == (1, HOP * (N - 1)) and plain.ndim == 1
    assert torch.equal(bits(one[0, :HOP * 16]), bits(plain)) and not bits(one[0, HOP * 16:]).any()
    with pytest.raises(ValueError, match=r"lens\[0\] = 42 outside"):
        voc.decode(mel_valid[4:5].to(DEV), lens=[42])


# ---- graph behaviour -----------------------------------------------------------------------------------------------------------
def test_graph_serves_new_lengths_and_keeps_the_plain_graph_apart(vweights, mel_valid):
    vg = Vocos(vweights, precision="f16", device=DEV, use_graph=True)
    ve = Vocos(vweights, precision="f16", device=DEV, use_graph=False)
    mel = padded(mel_valid, float("nan"))
    lens2 = [2, 41, 17, 38, 40]
    mel2 = mel_valid.clone()
    for b, ln in enumerate(lens2):
        mel2[b, ln:] = float("nan")
    mel2 = mel2.to(DEV)
    assert vg.graph_count() == 0
    a = vg.decode(mel, lens=LENS)
    assert vg.graph_count() == 1
    b2 = vg.decode(mel2, lens=lens2)                                             # the same (B, N): a replay, with new lengths
    assert vg.graph_count() == 1
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(ve.decode(mel, lens=LENS))) and torch.equal(bits(b2), bits(ve.decode(mel2, lens=lens2)))
    assert torch.isfinite(a).all() and torch.isfinite(b2).all()
    full = mel_valid.to(DEV)
    p = vg.decode(full)                                                          # the plain call of the same (B, N): its own graph
    assert vg.graph_count() == 2
    a2 = vg.decode(mel, lens=LENS)
    p2 = vg.decode(full)
    assert vg.graph_count() == 2
    torch.cuda.synchronize()
    assert torch.equal(bits(p), bits(ve.decode(full))) and torch.equal(bits(p2), bits(p)) and torch.equal(bits(a2), bits(a))
    assert ve.graph_count() == 0


def test_graph_cache_drops_a_dead_workspace_and_stays_bounded(vweights):
    """The two rules of the vocoder's graph cache: a graph captured against a workspace the caller has since replaced is dropped before
    the next capture, and at most 8 graphs are kept.  B = 1 and a few frames: every decode is a handful of small launches."""
    vg = Vocos(vweights, precision="f16", device=DEV, use_graph=True)
    ve = Vocos(vweights, precision="f16", device=DEV, use_graph=False)
    r = np.random.default_rng(16)
    mel = torch.from_numpy((r.standard_normal((1, 16, 100)) * 2.0 - 1.0).astype(np.float32)).to(DEV)

    def same(n):
        got = vg.decode(mel[:, :n].contiguous())
        want = ve.decode(mel[:, :n].contiguous())
        torch.cuda.synchronize()
        return got.shape == (HOP * (n - 1),) and torch.equal(bits(got), bits(want))

    assert vg.graph_count() == 0
    assert same(8) and vg.graph_count() == 1
    first = vg._workspace                          # kept alive: the larger workspace is then certain to lie at another address
    assert same(16) and vg.graph_count() == 1      # N = 16 needs a larger workspace: the graph of N = 8 went with the old one
    assert vg._workspace.data_ptr() != first.data_ptr()
    second = vg._workspace.data_ptr()
    assert same(12) and vg.graph_count() == 2      # fits the same workspace: a second graph beside the first
    for i, n in enumerate((4, 5, 6, 7, 9, 10, 11)):
        assert same(n), n
        assert vg.graph_count() == min(3 + i, 8), (n, vg.graph_count())
    assert vg._workspace.data_ptr() == second and vg.graph_count() == 8      # nine shapes on one workspace, eight graphs
    assert same(16) and same(11) and vg.graph_count() == 8                    # evicted and kept entries both still decode right
    assert ve.graph_count() == 0


# ---- generate ------------------------------------------------------------------------------------------------------------------
def test_generate_vocode_batched(tmp_path, lib, vweights):
    """generate(batch_sentences=True, vocode_batched=True) against vocode_batched=False on the text of test_generate_batch_sentences,
    tiny model, a real Vocos on synthetic weights.  The reference recording is cut to 12 frames so that the sentences get different
    frame counts (the longest sentence's text outgrows the estimated duration) and the whole batch stays at the GEMM kernels its
    rows reach alone: the two waves are then the same bits.  Where the routing differs the two are held to each other at the bound
    of test_vocos_decode_parity for the precision (each is within that bound of the oracle; asking it of their difference asks more)."""
    import os
    from f5_tts_mlx_amd import generate as G
    from f5_tts_mlx_amd.cfm import F5TTS
    from f5_tts_mlx_amd.dit import DiT
    prec = "f16"
    model = DiT.from_config(TINY, precision="bf16x3", device=DEV)
    model.load_weights(synthetic_weights(TINY, seed=42))
    vocab = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}
    voc = Vocos(vweights, precision=prec, device=DEV, use_graph=False)
    f5 = F5TTS(transformer=model, vocab_char_map=vocab, vocoder=voc.decode)
    src, sr = G.read_wav(os.path.join(os.path.dirname(G.__file__), "assets", "test_en_1_ref_short.wav"))
    wav = str(tmp_path / "ref12.wav")
    G.write_wav(wav, src[24_000:24_000 + 12 * 256].astype(np.float32), sr)
    text = "Hello there. This one is a longer sentence, is it not? Short."
    kw = dict(ref_audio_path=wav, ref_audio_text="some call me nature.", steps=4, method="euler", seed=5, estimate_duration=True, f5tts=f5,
              batch_sentences=True)
    loop = G.generate(text, vocode_batched=False, **kw)
    frames = list(f5.last_durations)
    got = G.generate(text, vocode_batched=True, **kw)
    torch.cuda.synchronize()
    assert list(f5.last_durations) == frames and len(set(frames)) > 1, frames   # a ragged batch
    assert got.shape == loop.shape == (sum(256 * (f - 1) - 12 * 256 for f in frames),)
    routes = gemm_routes(lib, prec, len(frames) * max(frames))
    exact = all(gemm_routes(lib, prec, f) == routes for f in frames)
    print(f"[vocode_ragged] generate: frames {frames}, {'exact' if exact else 'bounded'} branch")
    if exact:
        assert torch.equal(bits(got), bits(loop))
    else:
        refm = float(loop.abs().mean())
        assert float((got - loop).abs().mean()) <= ORACLE_TOL[prec] * max(1e-3, refm) + 1e-6
    # a vocoder that takes no `lens` keeps the loop: the flag changes nothing
    idx = torch.arange(256, device=DEV) % 100
    fake = lambda mel: mel[:, :, idx].reshape(mel.shape[0], -1) if mel.shape[0] > 1 else mel[0][:, idx].reshape(-1)   # noqa: E731
    f5 = F5TTS(transformer=model, vocab_char_map=vocab, vocoder=fake)
    kw["f5tts"] = f5
    a, b = G.generate(text, vocode_batched=False, **kw), G.generate(text, vocode_batched=True, **kw)
    assert torch.equal(a, b)
