"""Row-isolated batches on the GPU (docs/isolate_rows.md): F5TTS.sample(..., isolate_rows=True) on the tiny model against the CPU
oracle's SOLO sample of every row, through the plain, the per-row and the dual-guidance route, with and without the text mask; the
option in the hipGraph key; a batch of one; and the wiring of generate_many.  The inputs are those of tests/isolate_oracle.py, whose
solo references are computed once and shared."""
import numpy as np
import pytest
import torch

import isolate_oracle as IO
from f5test import DEV
from rowops_matrix import bits
from f5_tts_mlx_amd import audio as A
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.dit import DiT
from test_model_gpu import MEL_L1_TOL

pytestmark = pytest.mark.gpu

VOCAB = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}
_MODELS = {}


def model(precision: str, text_mask_padding: bool = True):
    key = (precision, text_mask_padding)
    if key not in _MODELS:
        m = DiT.from_config(IO.config(text_mask_padding), precision=precision, device=DEV)
        m.load_weights(IO.weights())
        _MODELS[key] = m
    return _MODELS[key]


def sample(m, rows=slice(None), **kw):
    """F5TTS.sample on the rows `rows` of the shared batch (all of them: padded to 128 frames)"""
    cond, text, durs, y0 = IO.inputs()
    durs = durs[rows]
    n = max(durs)
    out, _ = F5TTS(transformer=m).sample(cond[rows], text[rows], duration=torch.tensor(durs), y0=y0[rows, :n].contiguous(),
                                         **dict(IO.SOLVER, **kw))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


def distances(out, text_mask_padding=True):
    solo = IO.solo_reference(text_mask_padding)
    return [IO.row_distance(out, solo, b) for b in range(3)]


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
def test_isolated_rows_equal_their_solo_oracle_sample(precision):
    """option on: every row within the parity gate of the oracle's solo sample of that row -- the check that fails without the feature;
    option off, same call: the short rows are beyond it, which guards the inputs"""
    m = model(precision)
    on = distances(sample(m, isolate_rows=True))
    assert m.engine.get_option("isolate_rows") == 1
    off_out = sample(m)
    off = distances(off_out)
    assert m.engine.get_option("isolate_rows") == 0            # one value per call: the call without the argument runs as it always did
    print(f"[isolate] {precision}: rows vs solo oracle, option on {on}, off {off} (gate {MEL_L1_TOL:g})")
    assert max(on) <= MEL_L1_TOL, on
    assert off[1] > MEL_L1_TOL and off[2] > MEL_L1_TOL, off
    # the longest row has no padding: the row lengths change nothing for it, bit for bit, at this launch shape
    assert torch.equal(bits(sample(m, isolate_rows=True)[0]), bits(off_out[0]))


@pytest.mark.parametrize("route", ["rows", "dual"])
def test_isolated_rows_on_the_per_row_routes(route):
    """a strength per row selects f5_sample_rows; an audio strength f5_sample_dual, whose third branch makes the conv-pos length table
    3 B entries long.  Equal strengths make both the single-knob rule, so the solo references stay the same."""
    m = model("bf16x3")
    kw = dict(cfg_strength=[2.0, 2.0, 2.0]) if route == "rows" else dict(cfg_strength=2.0, audio_cfg_strength=2.0)
    on, off = distances(sample(m, isolate_rows=True, **kw)), distances(sample(m, **kw))
    print(f"[isolate] {route}: rows vs solo oracle, option on {on}, off {off} (gate {MEL_L1_TOL:g})")
    assert max(on) <= MEL_L1_TOL, on
    assert off[1] > MEL_L1_TOL and off[2] > MEL_L1_TOL, off


def test_isolated_rows_without_the_text_mask():
    """text_mask_padding = False: the text path's padding is not zeroed between the blocks, so the depthwise conv's length matters too"""
    m = model("bf16x3", text_mask_padding=False)
    on, off = distances(sample(m, isolate_rows=True), False), distances(sample(m), False)
    print(f"[isolate] no text mask: rows vs solo oracle, option on {on}, off {off} (gate {MEL_L1_TOL:g})")
    assert max(on) <= MEL_L1_TOL, on
    assert off[1] > MEL_L1_TOL and off[2] > MEL_L1_TOL, off


def test_option_is_part_of_the_graph_key():
    """captured graphs, one shape, option on / off / on / on: each run returns its own mode's result (the eager one, bit for bit) and
    the option costs exactly one more graph"""
    m = DiT.from_config(IO.config(), precision="bf16x3", device=DEV)       # an engine of its own: no graph of another test in its cache
    m.load_weights(IO.weights())
    eager = {v: sample(m, use_graph=False, **({"isolate_rows": True} if v else {})) for v in (True, False)}
    assert not torch.equal(bits(eager[True]), bits(eager[False]))
    n0 = m.engine.graph_count()
    assert n0 == 0
    runs = [(v, sample(m, use_graph=True, **({"isolate_rows": True} if v else {}))) for v in (True, False, True, True)]
    for i, (v, out) in enumerate(runs):
        assert torch.equal(bits(out), bits(eager[v])), f"run {i} (option {'on' if v else 'off'}) is not its mode's result"
    assert torch.equal(bits(runs[2][1]), bits(runs[3][1]))
    assert m.engine.graph_count() == n0 + 2


def test_a_batch_of_one_launches_what_it_launches_today():
    """no mask, no padding: the option is inactive and the result is the same bits"""
    m = model("bf16x3")
    assert torch.equal(bits(sample(m, rows=slice(1, 2), isolate_rows=True)), bits(sample(m, rows=slice(1, 2))))


def test_arguments_are_checked_before_any_launch():
    m = model("bf16x3")
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        sample(m, isolate_rows=1)
    m8 = DiT.from_config(IO.config(), precision="mxfp8", device=DEV)
    m8.load_weights(IO.weights())
    with pytest.raises(ValueError, match="not supported on an mxfp8 model"):
        sample(m8, isolate_rows=True)
    assert m8.engine.get_option("isolate_rows") == 0
    # the C call refuses the combination by itself, with its own message
    m8.engine.set_option("isolate_rows", 1)
    with pytest.raises(RuntimeError, match="f5_sample: engine option isolate_rows = 1 is not supported in precision mxfp8"):
        sample(m8)
    m8.engine.set_option("isolate_rows", 0)


# ---- generate_many ---------------------------------------------------------------------------------------------------------------
def _requests(tmp_path):
    """two requests of different length: two references, three rows, three durations"""
    import pkgutil
    data, _ = G.read_wav(pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav"))
    src = np.asarray(data, dtype=np.float32)
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    G.write_wav(a, src[24_000:24_000 + 40 * 256 + 77], 24_000)
    G.write_wav(b, src[48_000:48_000 + 28 * 256], 24_000)
    return [("Hello there. This one is a longer sentence, is it not?", a, "some call me nature."), ("Short one", b, "others call me.")]


def _by_hand(f5, voc, reqs, seed, **sample_kw):
    """prepare_references -> sample(mel, text, durations, lens = frames) -> decode each row on its own frames -> the same slices"""
    loaded = [G.read_wav(p) for _, p, _ in reqs]
    refs = A.prepare_references([torch.from_numpy(np.asarray(a)).to(torch.float32) for a, _ in loaded], [int(sr) for _, sr in loaded],
                                trim_silence_db=None, target_rms=G.TARGET_RMS, device=DEV)
    sentences = [G.split_sentences(t) or [t.strip()] for t, _, _ in reqs]
    row_req = [i for i, ss in enumerate(sentences) for _ in ss]
    texts = G.convert_char_to_pinyin([reqs[i][2] + " " + s for i, ss in enumerate(sentences) for s in ss])
    est = [int(G.estimated_duration(np.zeros(refs.samples[i]), reqs[i][2], reqs[i][0], 1.0) * G.FRAMES_PER_SEC) for i in range(len(reqs))]
    mel, _ = f5.sample(refs.mel[torch.tensor(row_req, device=DEV)], text=texts, duration=torch.tensor([est[i] for i in row_req]),
                       lens=torch.tensor([refs.frames[i] for i in row_req]), steps=4, method="euler", seed=seed, **sample_kw)
    frames = list(f5.last_durations)
    rows = [voc(mel[r:r + 1, :frames[r]]).reshape(-1)[refs.samples[i]:] for r, i in enumerate(row_req)]
    return [torch.cat([rows[r] for r, q in enumerate(row_req) if q == i]) for i in range(len(reqs))], frames


def test_generate_many_passes_the_option_on(tmp_path):
    """generate_many(isolate_rows=True) is prepare_references -> sample(isolate_rows=True) -> decode -> join done by hand, bit for bit;
    without the argument it is the present path, bit for bit, and the option is left off"""
    m = model("bf16x3")
    idx = torch.arange(256, device=DEV) % 100
    voc = lambda mel: mel[:, :, idx].reshape(mel.shape[0], -1) if mel.shape[0] > 1 else mel[0][:, idx].reshape(-1)   # noqa: E731
    reqs = _requests(tmp_path)
    kw = dict(steps=4, method="euler", seed=5, estimate_duration=True)
    got_on = G.generate_many(reqs, f5tts=F5TTS(transformer=m, vocab_char_map=VOCAB, vocoder=voc), isolate_rows=True, **kw)
    assert m.engine.get_option("isolate_rows") == 1
    want_on, frames = _by_hand(F5TTS(transformer=m, vocab_char_map=VOCAB), voc, reqs, 5, isolate_rows=True)
    got_off = G.generate_many(reqs, f5tts=F5TTS(transformer=m, vocab_char_map=VOCAB, vocoder=voc), **kw)
    assert m.engine.get_option("isolate_rows") == 0
    want_off, _ = _by_hand(F5TTS(transformer=m, vocab_char_map=VOCAB), voc, reqs, 5)
    torch.cuda.synchronize()
    assert len(set(frames)) > 1                                # a ragged batch: some row has padding
    for i in range(2):
        assert got_on[i].numel() > 0 and torch.equal(bits(got_on[i]), bits(want_on[i])), i
        assert torch.equal(bits(got_off[i]), bits(want_off[i])), i
    assert any(not torch.equal(bits(a), bits(b)) for a, b in zip(got_on, got_off))
