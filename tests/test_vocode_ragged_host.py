"""Ragged vocoding on the CPU: the refusals of f5_vocode_ragged and of the three ragged ops (all of them come before any launch), the
host-side validation of `Vocos.decode(mel, lens=...)`, the opt-in wiring of generate(), and a numpy fp64 statement of what "row b ends
at lens[b]" means for the three places where Vocos mixes time steps -- held against the same functions run on each row's slice alone,
and shown to fail for the two mistakes a ragged kernel is most likely to make.  tests/test_vocode_ragged_gpu.py asserts the same
property of the kernels, bit for bit."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from f5test import E
from f5_tts_mlx_amd import vocos as V

B, N, LENS = 5, 41, [41, 40, 38, 2, 17]          # the shapes of the GPU tests


# ---- the C ABI refuses before it launches --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    """a vocoder handle that was never given an arena: creating one plans sizes and touches no device"""
    lib = E.load_library()
    h = C.c_void_p()
    cfg = V.VocosConfig(V.N_MELS, V.DIM, V.INTER, V.LAYERS, V.N_FFT, V.HOP)
    assert lib.f5_vocoder_create(C.byref(cfg), E.PRECISIONS["f16"], C.byref(h)) == 0
    yield h
    lib.f5_vocoder_destroy(h)


def _vocode(lib, h, **kw):
    a = dict(v=h, mel=64, lens=[3, 4], B=2, N=4, wave=64, ws=256, ws_bytes=1 << 40, graph=0)
    a.update(kw)
    lens = None if a["lens"] is None else (C.c_int32 * len(a["lens"]))(*a["lens"])          # read on the HOST: a real array
    rc = lib.f5_vocode_ragged(a["v"], C.c_void_p(a["mel"]), lens, a["B"], a["N"], C.c_void_p(a["wave"]), C.c_void_p(a["ws"]),
                              C.c_size_t(a["ws_bytes"]), a["graph"], C.c_void_p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(v=None), "handle is null"), (dict(mel=0), "mel is null"), (dict(lens=None), "lens is null"), (dict(wave=0), "wave is null"),
    (dict(ws=0), "workspace is null"),
    (dict(B=0, lens=[3]), "B must be >= 1"), (dict(B=-2, lens=[3]), "B must be >= 1"),
    (dict(N=1, B=1, lens=[1]), "N must be >= 2"),
    (dict(B=1, N=4, lens=[1]), "lens[0] = 1 outside 2..N = 4"), (dict(B=1, N=4, lens=[5]), "lens[0] = 5 outside 2..N = 4"),
    (dict(lens=[4, 0]), "lens[1] = 0 outside"), (dict(lens=[4, -7]), "lens[1] = -7 outside"),
    (dict(), "not finalized"),                                             # every argument in range, but no weights
])
def test_vocode_ragged_refusals_need_no_gpu(handle, kw, word):
    rc, msg = _vocode(E.load_library(), handle, **kw)
    assert rc != 0 and msg.startswith("f5_vocode_ragged:") and word in msg, (rc, msg)


def _op(lib, name, **kw):
    p = C.c_void_p
    if name == "im2col7":
        a = dict(x=64, hi=64, lo=64, nbatch=2, seq_len=5, channels=100, lens=64)
        a.update(kw)
        rc = lib.f5_op_im2col7_ragged(p(a["x"]), p(a["hi"]), p(a["lo"]), a["nbatch"], a["seq_len"], a["channels"], p(a["lens"]), p(0))
    elif name == "dwconv_ln":
        a = dict(x=64, dw_w=64, dw_b=64, ln_w=64, ln_b=64, hi=64, lo=64, nbatch=2, seq_len=5, dim=512, lens=64)
        a.update(kw)
        rc = lib.f5_op_dwconv_ln_ragged(p(a["x"]), p(a["dw_w"]), p(a["dw_b"]), p(a["ln_w"]), p(a["ln_b"]), p(a["hi"]), p(a["lo"]),
                                        a["nbatch"], a["seq_len"], a["dim"], p(a["lens"]), p(0))
    else:
        a = dict(x=64, ldx=1026, window=64, frames=64, wave=64, B=2, nframes=5, n_fft=1024, hop=256, lens=64)
        a.update(kw)
        rc = lib.f5_op_istft_ragged(p(a["x"]), a["ldx"], p(a["window"]), p(a["frames"]), p(a["wave"]), a["B"], a["nframes"], a["n_fft"],
                                    a["hop"], p(a["lens"]), p(0))
    return rc, lib.f5_last_error().decode()


@pytest.mark.parametrize("name,kw,word", [
    ("im2col7", dict(x=0), "x is null"), ("im2col7", dict(hi=0), "out_hi is null"), ("im2col7", dict(lens=0), "lens is null"),
    ("im2col7", dict(nbatch=0), "nbatch must be >= 1"), ("im2col7", dict(seq_len=1), "seq_len must be >= 2"),
    ("im2col7", dict(channels=129), "channels must be in [1, 128]"),
    ("dwconv_ln", dict(x=0), "x is null"), ("dwconv_ln", dict(dw_w=0), "dw_w / dw_b is null"), ("dwconv_ln", dict(ln_b=0), "ln_w / ln_b is null"),
    ("dwconv_ln", dict(hi=0), "out_hi is null"), ("dwconv_ln", dict(lens=0), "lens is null"),
    ("dwconv_ln", dict(nbatch=0), "nbatch must be >= 1"), ("dwconv_ln", dict(seq_len=1), "seq_len must be >= 2"),
    ("dwconv_ln", dict(dim=500), "dim must be 256/512/768/1024"),
    ("istft", dict(x=0), "x is null"), ("istft", dict(window=0), "window is null"), ("istft", dict(frames=0), "frames_scratch is null"),
    ("istft", dict(wave=0), "wave is null"), ("istft", dict(lens=0), "lens is null"), ("istft", dict(B=0), "B = 0 outside 1..65535"),
    ("istft", dict(nframes=1), "nframes must be >= 2"), ("istft", dict(n_fft=512), "only n_fft = 1024"),
    ("istft", dict(hop=0), "must divide n_fft"), ("istft", dict(ldx=1025), "ldx = 1025 below n_fft + 2"),
])
def test_ragged_op_refusals_need_no_gpu(name, kw, word):
    rc, msg = _op(E.load_library(), name, **kw)
    assert rc != 0 and msg.startswith(name + "_ragged:") and word in msg, (rc, msg)


def test_workspace_plan_covers_the_staged_lengths(handle):
    """f5_vocoder_workspace_bytes serves both calls: it grew by the staged lens and nothing else moved"""
    lib = E.load_library()
    n = C.c_size_t()
    assert lib.f5_vocoder_workspace_bytes(handle, B, N, C.byref(n)) == 0
    rows = B * N
    al = lambda x: (x + 255) & ~255                                               # noqa: E731
    plain = sum(al(x) for x in (rows * 100 * 4, rows * 512 * 4, rows * 512 * 4, rows * 1026 * 4, rows * 1024 * 4, B * 256 * (N - 1) * 4,
                                rows * 7 * 128 * 2, rows * 512 * 2, rows * 1536 * 2))
    assert n.value == plain + al(B * 4)
    assert lib.f5_vocoder_graph_count(handle) == 0


def test_load_tensor_checks_name_shape_and_arena(handle):
    lib = E.load_library()
    buf = (C.c_float * (V.INTER * V.DIM))()

    def load(name, *shape):
        rc = lib.f5_vocoder_load_tensor(handle, name, buf, len(shape), (C.c_int64 * len(shape))(*shape))
        return rc, lib.f5_last_error()

    no_arena = b"f5_vocoder_set_weights_arena must be called first"
    pw1 = b"backbone.convnext.3.pwconv1.weight"
    assert load(pw1, V.INTER, V.DIM) == (2, no_arena)                                   # right name and shape, no arena yet
    assert load(b"backbone.convnext.99.pwconv1.weight", V.INTER, V.DIM) == (2, b"unknown vocoder tensor name 'backbone.convnext.99.pwconv1.weight'")
    assert load(pw1, V.INTER, V.DIM, 1) == (2, b"tensor '" + pw1 + b"': unexpected shape")               # wrong rank
    assert load(pw1, V.INTER, V.DIM // 2) == (2, b"tensor '" + pw1 + b"': unexpected shape")            # wrong dimension
    assert load(pw1, V.DIM, V.INTER) == (2, b"tensor '" + pw1 + b"': unexpected shape")                 # transposed: the same count
    # the shapes the loader tolerates pass its shape check (and stop at the arena)
    dw, gamma = b"backbone.convnext.0.dwconv.weight", b"backbone.convnext.0.gamma"
    assert load(dw, V.DIM, 1, 7) == (2, no_arena) and load(dw, V.DIM, 7, 1) == (2, no_arena)
    assert load(dw, V.DIM, 7) == (2, b"tensor '" + dw + b"': unexpected shape")
    assert load(gamma, V.DIM) == (2, no_arena) and load(gamma, 1, 1, V.DIM) == (2, no_arena)
    assert load(gamma, 1, V.DIM + 1) == (2, b"tensor '" + gamma + b"': unexpected shape")
    # the embed conv weight has its own layout check
    emb = b"backbone.embed.weight"
    assert load(emb, V.DIM, V.N_MELS, 7) == (2, no_arena) and load(emb, V.DIM, 7, V.N_MELS) == (2, no_arena)
    assert load(emb, V.DIM, V.N_MELS) == (2, b"tensor '" + emb + b"': expected (dim, n_mels, 7) or (dim, 7, n_mels)")
    assert load(emb, V.DIM, 7, V.N_MELS + 1) == (2, b"tensor '" + emb + b"': expected (dim, n_mels, 7) or (dim, 7, n_mels)")
    assert lib.f5_vocoder_finalize(handle, None) != 0 and lib.f5_last_error() == b"vocoder arena not set"


# ---- Vocos.decode validates lens on the host -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [LENS, tuple(LENS), torch.tensor(LENS), torch.tensor(LENS, dtype=torch.int32), np.array(LENS),
                                  [np.int64(v) for v in LENS]])
def test_validate_lens_accepts(lens):
    out = V.validate_lens(lens, B, N)
    assert out == LENS and all(type(v) is int for v in out)


@pytest.mark.parametrize("lens,word", [
    ([41, 40, 38, 1, 17], r"lens\[3\] = 1 outside 2\.\.41"), ([42, 40, 38, 2, 17], r"lens\[0\] = 42 outside 2\.\.41"),
    ([41, 40, 38, 2, -17], r"lens\[4\] = -17 outside"), ([41, 40, 38, 2], "4 entries for a batch of 5"),
    ([41, 40, 38, 2, 17, 3], "6 entries for a batch of 5"), ([41, 40, 38, 2, 17.0], r"lens\[4\] = 17.0 is not an integer"),
    ([41, 40, True, 2, 17], r"lens\[2\] = True is not an integer"), (torch.tensor([41., 40., 38., 2., 17.]), "must hold integers"),
    (np.array(LENS, np.float32), "must hold integers"), (torch.tensor([LENS]), "must be 1-D"), (17, "must be a sequence"),
    ("41 40", "must be a sequence"),
])
def test_validate_lens_refuses(lens, word):
    with pytest.raises(ValueError, match=word):
        V.validate_lens(lens, B, N)


def test_decode_validates_before_any_library_call():
    """constructing a Vocos needs a GPU; `decode` on an object that has no library and no handle shows that a bad `lens` raises before
    either is touched"""
    v = object.__new__(V.Vocos)
    with pytest.raises(ValueError, match=r"lens\[1\] = 9 outside 2\.\.8"):
        V.Vocos.decode(v, torch.zeros((2, 8, 100)), lens=[8, 9])
    v.__dict__.clear()                                                            # nothing for __del__ to destroy
    assert list(inspect.signature(V.Vocos.decode).parameters) == ["self", "mel", "lens"]
    assert inspect.signature(V.Vocos.decode).parameters["lens"].default is None


# ---- what "row b ends at lens[b]" means, in numpy fp64 -------------------------------------------------------------------------
def im2col7(x, lens=None, bug=None):
    """x [B][N][C] -> [B][N][7][C]: tap t of output frame n is frame n + t - 3 of the same row when that lies inside the row's own
    length, else zero; an output frame past the length is zero.  The value is selected, never multiplied by a mask."""
    nb, n, ch = x.shape
    out = np.zeros((nb, n, 7, ch))
    for b in range(nb):
        ln = n if lens is None else lens[b]
        tap_end = n if bug == "tap_mask_uses_seq_len" else ln
        for f in range(ln):
            for t in range(7):
                nn = f + t - 3
                if 0 <= nn < tap_end:
                    out[b, f, t] = x[b, nn]
    return out


def dwconv7(x, w, bias, lens=None, bug=None):
    """x [B][N][D], w [D][7]: y[b][n] = bias + sum over t = 0 .. 6 of x[b][n + t - 3] w[:, t], taps outside the row's length left out;
    frames past the length are zero"""
    nb, n, d = x.shape
    out = np.zeros((nb, n, d))
    for b in range(nb):
        ln = n if lens is None else lens[b]
        tap_end = n if bug == "tap_mask_uses_seq_len" else ln
        for f in range(ln):
            y = bias.copy()
            for t in range(7):
                nn = f + t - 3
                if 0 <= nn < tap_end:
                    y = y + x[b, nn] * w[:, t]
            out[b, f] = y
    return out


def overlap_add(frames, window, hop, lens=None, bug=None):
    """frames [B][N][n_fft] (already windowed) -> wave [B][hop (N - 1)]: sample s of a row with nf frames is the sum of the frames that
    cover position s + n_fft / 2, over the sum of their squared window values -- frames and envelope both stop at nf; s >= hop (nf - 1)
    is zero"""
    nb, n, n_fft = frames.shape
    out = np.zeros((nb, hop * (n - 1)))
    for b in range(nb):
        nf = n if lens is None else lens[b]
        env_frames = n if bug == "envelope_uses_N" else nf
        for s in range(hop * (nf - 1)):
            pos = s + n_fft // 2
            acc = sum(frames[b, f, pos - f * hop] for f in range(nf) if 0 <= pos - f * hop < n_fft)
            env = sum(window[pos - f * hop] ** 2 for f in range(env_frames) if 0 <= pos - f * hop < n_fft)
            out[b, s] = acc / env
    return out


@pytest.fixture(scope="module")
def data():
    r = np.random.default_rng(11)
    d = dict(x=r.standard_normal((B, N, 6)), w=r.standard_normal((6, 7)), bias=r.standard_normal(6), fr=r.standard_normal((B, N, 16)),
             win=0.5 - 0.5 * np.cos(2 * np.pi * np.arange(16) / 16))
    for b, ln in enumerate(LENS):                                                  # the padding holds what must never be read
        d["x"][b, ln:] = np.nan
        d["fr"][b, ln:] = np.nan
    return d


def _rowwise(fn_batch, fn_row, width):
    """first mismatch between a batch result and the per-row results, or None: the valid part equal, the rest exactly zero"""
    got = fn_batch()
    for b, ln in enumerate(LENS):
        want = fn_row(b, ln)
        k = width(ln)
        if not np.array_equal(got[b, :k], want):
            return f"row {b} (len {ln}): valid part differs"
        if not (got[b, k:] == 0).all():
            return f"row {b} (len {ln}): tail not zero"
    return None


def _checks(d, bug=None):
    return dict(
        im2col7=_rowwise(lambda: im2col7(d["x"], LENS, bug), lambda b, ln: im2col7(d["x"][b:b + 1, :ln])[0], lambda ln: ln),
        dwconv7=_rowwise(lambda: dwconv7(d["x"], d["w"], d["bias"], LENS, bug), lambda b, ln: dwconv7(d["x"][b:b + 1, :ln], d["w"], d["bias"])[0],
                         lambda ln: ln),
        overlap_add=_rowwise(lambda: overlap_add(d["fr"], d["win"], 4, LENS, bug), lambda b, ln: overlap_add(d["fr"][b:b + 1, :ln], d["win"], 4)[0],
                             lambda ln: 4 * (ln - 1)))


def test_ragged_semantics_equal_each_row_alone(data):
    bad = {k: v for k, v in _checks(data).items() if v}
    assert not bad, bad
    # and nothing of the NaN padding came through
    assert np.isfinite(im2col7(data["x"], LENS)).all() and np.isfinite(dwconv7(data["x"], data["w"], data["bias"], LENS)).all()
    assert np.isfinite(overlap_add(data["fr"], data["win"], 4, LENS)).all()


@pytest.mark.parametrize("bug,hits", [("tap_mask_uses_seq_len", ("im2col7", "dwconv7")), ("envelope_uses_N", ("overlap_add",))])
def test_seeded_mistakes_are_seen(data, bug, hits):
    res = _checks(data, bug)
    print(f"[vocode_ragged harness] {bug}: {res}")
    for k in hits:
        assert res[k] is not None and "valid part differs" in res[k], (k, res[k])
    # with finite padding too: the mistake is a wrong VALUE, not only a NaN
    d = {k: np.nan_to_num(v, nan=0.75) for k, v in data.items()}
    res = _checks(d, bug)
    for k in hits:
        assert res[k] is not None, (k, res)


# ---- Python wiring -------------------------------------------------------------------------------------------------------------
def test_generate_has_the_new_keyword_and_flag(capsys):
    from f5_tts_mlx_amd import generate as G
    sig = inspect.signature(G.generate)
    assert sig.parameters["vocode_batched"].default is False
    assert "docs/vocode_ragged.md" in G.generate.__doc__
    with pytest.raises(SystemExit) as e:
        G.main(["--help"])
    assert e.value.code == 0
    assert "--vocode-batched" in capsys.readouterr().out
    # a plain mel -> wave callable keeps the per-sentence loop; Vocos.decode takes the ragged call
    assert not G._takes_lens(lambda mel: mel) and G._takes_lens(V.Vocos.decode) and G._takes_lens(lambda mel, lens=None: mel)
