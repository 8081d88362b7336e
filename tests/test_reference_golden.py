"""The oracle against golden vectors produced by the REFERENCE's own Python source (tests/golden/ref_*.npz).

The vectors come from `tests/golden/make_reference_golden.py`: the reference modules imported unmodified from /root/reference,
executed over `oracle/mlx_shim.py` (numpy emulation of the mlx primitives; MLX itself is not installable here).  They pin the
oracle's restatement of the reference's code path; what stays unpinned is MLX's own arithmetic.

The checks that once ran the reference live (text front-end, random small configurations, from_pretrained) compare against answers
the generator recorded from it (`--only-recorded`): ref_text_front_end.json, ref_sample_fuzz.npz, ref_from_pretrained.json.
"""
import json
import os

import numpy as np
import pytest
import torch

from f5test import O, ROOT, DiTConfig, synthetic_weights

GOLDEN = os.path.join(ROOT, "tests", "golden")
FWD_TOL = 2e-5        # fp32 oracle vs fp32-numpy reference, |out| ~ 0.8: max abs
TRAJ_TOL = 1e-4       # after up to 12 chained forwards with CFG 2.0


def load(name):
    g = np.load(os.path.join(GOLDEN, name))
    cfg = DiTConfig(**json.loads(str(g["cfg"]))) if "cfg" in g.files else None
    return g, cfg


@pytest.fixture(scope="module")
def ref_model():
    g, cfg = load("ref_dit_forward.npz")
    return cfg, O.DiTOracle(cfg, synthetic_weights(cfg, seed=int(g["weights_seed"])), dtype=torch.float32)


def test_dit_forward_matches_reference_code(ref_model):
    """dit.py:362-401 — cond / null branches, key mask, scalar time broadcast"""
    cfg, dit = ref_model
    g, _ = load("ref_dit_forward.npz")
    x, cond, text, time, mask = (torch.from_numpy(g[k]) for k in ("x", "cond", "text", "time", "mask"))
    for tag, (da, dt, m) in dict(cond=(False, False, None), null=(True, True, None), cond_masked=(False, False, mask),
                                 null_masked=(True, True, mask)).items():
        out = dit.forward(x, cond, text, time, da, dt, m)
        assert float((out - torch.from_numpy(g["out_" + tag])).abs().max()) < FWD_TOL, tag
    out = dit.forward(x[:1], cond[:1], text[:1], torch.tensor(0.7), False, False, None)
    assert float((out - torch.from_numpy(g["out_scalar_time"])).abs().max()) < FWD_TOL
    # the masked and unmasked goldens differ where it matters (row 1 is the ragged one), so the mask path is exercised
    assert float(np.abs(g["out_cond"][1] - g["out_cond_masked"][1]).max()) > 1e-3
    assert float(np.abs(g["out_cond"][0] - g["out_cond_masked"][0]).max()) < 1e-5


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_sample_matches_reference_code(ref_model, method):
    """cfm.py:264-402 — ragged batch of 2: lens/duration arithmetic, cond mask, attention mask, CFG, sway grid, solver"""
    cfg, dit = ref_model
    g, _ = load("ref_sample.npz")
    durations = torch.from_numpy(g["durations"])
    nmax = int(durations.max())
    y0 = torch.zeros((2, nmax, cfg.mel_dim))
    for i, z in enumerate((g["z0"], g["z1"])):                  # the reference draws (channels, dur) per element (cfm.py:369-374)
        y0[i, :z.shape[1]] = torch.from_numpy(z.T)
    out, traj = O.sample(dit, torch.from_numpy(g["cond"]), torch.from_numpy(g["text"]), durations, lens=torch.from_numpy(g["lens"]),
                         steps=int(g[f"steps_{method}"]), method=method, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0)
    ref_traj = torch.from_numpy(g[f"traj_{method}"])
    assert traj.shape == ref_traj.shape
    assert torch.equal(traj[0], ref_traj[0])
    assert float((traj - ref_traj).abs().max()) < TRAJ_TOL
    assert float((out - torch.from_numpy(g[f"out_{method}"])).abs().max()) < TRAJ_TOL


def test_sample_batch1_no_cfg_matches_reference_code(ref_model):
    """batch 1: no attention mask (cfm.py:333-336), int duration, cfg_strength 0 early return (:351), no sway"""
    cfg, dit = ref_model
    g, _ = load("ref_sample.npz")
    y0 = torch.from_numpy(g["z0"].T.copy())[None]
    out, traj = O.sample(dit, torch.from_numpy(g["cond"][:1]), torch.from_numpy(g["text"][:1]), int(g["durations"][0]), steps=4,
                         method="euler", cfg_strength=0.0, sway_sampling_coef=None, y0=y0)
    assert float((traj - torch.from_numpy(g["traj_b1_nocfg"])).abs().max()) < TRAJ_TOL
    assert float((out - torch.from_numpy(g["out_b1_nocfg"])).abs().max()) < TRAJ_TOL


def test_cfm_loss_matches_reference_code(ref_model):
    """cfm.py:169-251 with the reference's draw order (frac_lengths, span rand, x0, time, audio drop, cond drop)"""
    cfg, dit = ref_model
    g, _ = load("ref_cfm_loss.npz")
    kw = dict(lens=torch.from_numpy(g["lens"]), x0=torch.from_numpy(g["x0"]), time=torch.from_numpy(g["time"]),
              frac_lengths=torch.from_numpy(g["frac_lengths"]), span_rand=torch.from_numpy(g["span_rand"]))
    for name, (ra, rc) in dict(keep=(0.9, 0.9), drop_audio=(0.1, 0.9), drop_both=(0.9, 0.1)).items():
        loss = float(O.cfm_loss(dit, torch.from_numpy(g["mel"]), torch.from_numpy(g["text"]), rand_audio_drop=ra, rand_cond_drop=rc, **kw))
        assert abs(loss - float(g["loss_" + name])) < 2e-5 * float(g["loss_" + name]), name
    assert len({float(g["loss_" + n]) for n in ("keep", "drop_audio", "drop_both")}) == 3


def test_host_pieces_match_reference_code():
    """utils.py masks / tokenisers (bit-exact), rope.py tables, time embedding, sway grid, audio.py mel front-end"""
    g, _ = load("ref_host.npz")
    lens = torch.from_numpy(g["lens"])
    assert np.array_equal(O.lens_to_mask(lens).numpy(), g["lens_mask"])
    assert np.array_equal(O.lens_to_mask(lens, 12).numpy(), g["lens_mask_len12"])
    fm = O.mask_from_frac_lengths(torch.tensor([20, 31, 8], dtype=torch.int32), torch.tensor([0.7, 0.85, 1.0]),
                                  torch.tensor([0.5, 0.1, 0.99]), 32)
    assert np.array_equal(fm.numpy(), g["frac_mask"])
    assert np.array_equal(O.list_str_to_tensor(["hello", "héllo wörld", ""]).numpy(), g["utf8"])
    vocab, tok_in = json.loads(str(g["vocab"])), json.loads(str(g["tok_in"]))
    assert np.array_equal(O.list_str_to_idx(tok_in, vocab).numpy(), g["tok_idx"])
    assert np.allclose(O.precompute_freqs_cis(512, 64).numpy(), g["freqs_cis"], atol=2e-5)   # fp32 angles up to 63 rad: 1 ulp of the argument
    assert np.array_equal(O.get_pos_embed_indices(torch.tensor([0, 3]), 10, max_pos=12).numpy(), g["pos_idx"])
    freqs = O.rotary_freqs(64, 24)
    assert np.allclose(freqs.numpy(), g["rope_freqs"].reshape(freqs.shape), atol=2e-6)
    rope_out = O.apply_rotary_pos_emb(torch.from_numpy(g["rope_in"]), freqs)
    assert np.allclose(rope_out.numpy(), g["rope_out"], atol=5e-6)
    for key, coef in (("sway_none", None), ("sway_m1", -1.0), ("sway_p05", 0.5)):
        assert np.allclose(O.time_grid(9, coef).numpy(), g[key], atol=3e-7), key
    assert np.allclose(O.hanning(1024), g["hanning"], atol=1e-7)
    assert np.allclose(O.mel_filters(24000, 1024, 100), g["mel_filters"], atol=2e-6)
    mel = O.log_mel_spectrogram(g["audio"])
    ref = g["mel"]                                              # reference layout (1, frames, mels), audio.py:196-198
    assert mel.shape == ref.shape
    assert float(np.abs(mel - ref).mean()) < 1e-5 and float(np.abs(mel - ref).max()) < 5e-4


def test_time_embedding_matches_reference_code(ref_model):
    """dit.py:56-66: sinusoidal features (scale 1000) ahead of the time MLP"""
    cfg, dit = ref_model
    g, _ = load("ref_host.npz")
    t = torch.from_numpy(g["time_in"])
    half = 128
    emb = 1000.0 * t[:, None] * torch.exp(torch.arange(half, dtype=torch.float32) * -(np.log(10000.0) / (half - 1)))[None]
    sinus = torch.cat([emb.sin(), emb.cos()], dim=-1)
    assert np.allclose(sinus.numpy(), g["time_sinus"], atol=2e-4)          # arguments up to 1000 rad in fp32
    out = dit.time_embed(t)
    assert out.shape == (3, cfg.dim) and torch.isfinite(out).all()


def test_package_host_functions_match_reference_code():
    """the product's host-side mirrors (f5_tts_mlx_amd.utils, no GPU needed): index paths bit-exact vs utils.py's outputs"""
    from f5_tts_mlx_amd import utils as U
    g, _ = load("ref_host.npz")
    lens = torch.from_numpy(g["lens"])
    assert np.array_equal(U.lens_to_mask(lens).numpy(), g["lens_mask"])
    assert np.array_equal(U.lens_to_mask(lens, 12).numpy(), g["lens_mask_len12"])
    fm = U.mask_from_frac_lengths(torch.tensor([20, 31, 8], dtype=torch.int32), torch.tensor([0.7, 0.85, 1.0]), max_length=32,
                                  rand=torch.tensor([0.5, 0.1, 0.99]))
    assert np.array_equal(fm.numpy(), g["frac_mask"])
    assert np.array_equal(U.list_str_to_tensor(["hello", "héllo wörld", ""]).numpy(), g["utf8"])
    assert np.array_equal(U.list_str_to_idx(json.loads(str(g["tok_in"])), json.loads(str(g["vocab"]))).numpy(), g["tok_idx"])


def test_duration_predictor_matches_reference_code():
    """duration.py:192-251 (return_loss=False): text longer than the mel (pad branch :218-220), ragged lens, masked mean, softplus"""
    from oracle import duration_oracle as DO
    from f5_tts_mlx_amd.duration import synthetic_duration_weights
    g = np.load(os.path.join(GOLDEN, "ref_duration.npz"))
    kw = json.loads(str(g["cfg"]))
    w = synthetic_duration_weights(seed=int(g["weights_seed"]), **kw)
    for tag in ("b1", "b2_long_text"):
        got = DO.predict(w, torch.from_numpy(g[f"{tag}_mel"]), torch.from_numpy(g[f"{tag}_text"]), lens=torch.from_numpy(g[f"{tag}_lens"]),
                         depth=kw["depth"], dtype=torch.float32)
        want = torch.from_numpy(g[f"{tag}_seconds"])
        assert got.shape == want.shape and float((got - want).abs().max()) < 2e-5 * float(want.abs().max()), tag


def test_sample_duration_clamps_match_reference_code(ref_model):
    """cfm.py:301-303,317-319: lens = max(#text tokens, lens) (more tokens than reference frames: the conditioning region runs over
    zero padding), duration raised to lens + 1, clipped to max_duration"""
    cfg, dit = ref_model
    g, _ = load("ref_sample_clamps.npz")
    nmax = int(g["max_duration"])
    y0 = torch.zeros((2, nmax, cfg.mel_dim))
    for i, z in enumerate((g["z0"], g["z1"])):
        y0[i, :z.shape[1]] = torch.from_numpy(z.T)
    out, traj, aux = O.sample(dit, torch.from_numpy(g["cond"]), torch.from_numpy(g["text"]), torch.from_numpy(g["durations"]),
                              lens=torch.from_numpy(g["lens"]), steps=3, method="euler", y0=y0, max_duration=nmax, return_aux=True)
    assert aux["duration"].tolist() == g["final_durations"].tolist() and aux["lens"].tolist() == [14, 11]
    assert float((traj - torch.from_numpy(g["traj"])).abs().max()) < TRAJ_TOL
    assert float((out - torch.from_numpy(g["out"])).abs().max()) < TRAJ_TOL


def test_text_front_end_matches_reference_code_live():
    """convert_char_to_pinyin / split_sentences / estimated_duration of the package vs the reference's own functions, as recorded from
    them over the shim (tests/golden/ref_text_front_end.json; jieba's segmentation of single-byte text is the package's emulation on
    both sides)"""
    from f5_tts_mlx_amd import generate as G
    from f5_tts_mlx_amd import utils as U
    g = json.load(open(os.path.join(GOLDEN, "ref_text_front_end.json"), encoding="utf-8"))
    assert len(g["texts"]) == len(g["pinyin"]) == len(g["sentences"]) == 9 and len(g["durations"]) == 2
    for t, pinyin, sentences in zip(g["texts"], g["pinyin"], g["sentences"]):
        assert U.convert_char_to_pinyin([t]) == pinyin, t
        assert G.split_sentences(t) == sentences, t
    audio = np.zeros(127987, np.float32)
    for ref_text, gen_text, speed, want in g["durations"]:
        assert G.estimated_duration(audio, ref_text, gen_text, speed) == want, (ref_text, gen_text)


def test_oracle_vs_reference_code_live_fuzz():
    """The reference's DiT / sample, run over the shim on several random small configurations (widths, depths, heads, text-conv depth
    incl. 0, batch, lengths, ragged masks, solvers, CFG on/off; tests/golden/ref_sample_fuzz.npz holds each case's inputs and the
    reference's trajectory) against the oracle on the same weights and inputs.  Complements ref_sample.npz, which is one configuration."""
    g = np.load(os.path.join(GOLDEN, "ref_sample_fuzz.npz"))
    worst = 0.0
    for case in range(int(g["cases"])):
        c = lambda k: g[f"case{case}_{k}"]   # noqa: E731
        cfg = DiTConfig(**json.loads(str(c("cfg"))))
        orc = O.DiTOracle(cfg, synthetic_weights(cfg, seed=int(c("weights_seed"))), dtype=torch.float32)
        sway = None if np.isnan(float(c("sway"))) else float(c("sway"))
        _, o_traj = O.sample(orc, torch.from_numpy(c("cond")), torch.from_numpy(c("text")), torch.from_numpy(c("durations")),
                             lens=torch.from_numpy(c("lens")), steps=3, method=str(c("method")), cfg_strength=float(c("cfg_strength")),
                             sway_sampling_coef=sway, y0=torch.from_numpy(c("y0")))
        ref = torch.from_numpy(c("traj"))
        assert ref.shape == o_traj.shape, (case, ref.shape, o_traj.shape)
        err = float((o_traj - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        worst = max(worst, err)
        assert err < 2e-4, (case, err, cfg)
    print("worst", worst)


# ------------------------------------------------------------------------------------------------
# checkpoint conversion / quantisation predicate pinned against the reference's own from_pretrained (cfm.py:404-520)
# ------------------------------------------------------------------------------------------------
_UPSTREAM_RENAMES = (                      # MLX-tree name fragment -> upstream (PyTorch F5-TTS) fragment, SURVEY Appendix B
    (".to_out.layers.", ".to_out."), (".text_blocks.layers.", ".text_blocks."), (".ff.ff.layers.0.layers.0.", ".ff.ff.0.0."),
    (".ff.ff.layers.2.", ".ff.ff.2."), (".time_mlp.layers.", ".time_mlp."), (".conv1d.layers.", ".conv1d."))


def _upstream_checkpoint(weights):
    """An upstream-style (PyTorch F5-TTS) state dict holding `weights` (MLX-tree names / layouts): `ema_model.` prefix, PyTorch
    module numbering, conv weights (out, in/groups, k), plus the non-parameter entries a real checkpoint carries."""
    out = {}
    for k, v in weights.items():
        for mlx_frag, up_frag in _UPSTREAM_RENAMES:
            if mlx_frag in k:
                k = k.replace(mlx_frag, up_frag)
                break
        if k.endswith(".dwconv.weight") or ".conv1d." in k and k.endswith(".weight"):
            v = np.ascontiguousarray(np.swapaxes(v, 1, 2))
        out["ema_model." + k] = v
    out["ema_model.mel_spec.mel_stft.spectrogram.window"] = np.zeros(1024, np.float32)
    out["ema_model.mel_spec.mel_stft.mel_scale.fb"] = np.zeros((513, 100), np.float32)
    out["initted"] = np.ones((), np.float32)
    out["step"] = np.array(1200000, np.int64)
    return out


def array_digest(a) -> str:
    """sha256 of an array's dtype, shape and bytes: how tests/golden/ref_from_pretrained.json records the reference's parameters"""
    import hashlib
    a = np.ascontiguousarray(np.asarray(a))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def upstream_checkpoint_dir(dirname, depth, seed):
    """A synthetic UPSTREAM-named 335M checkpoint directory cut to `depth` blocks (what tests/golden/make_reference_golden.py handed
    the reference's from_pretrained): vocab.txt, model_v1.safetensors (`synthetic_weights(seed)` through _upstream_checkpoint) and
    model_v1_8b.safetensors, the MLX 8-bit file written with the package's rule."""
    import dataclasses
    from safetensors.numpy import save_file
    from f5_tts_mlx_amd.weights import F5TTS_335M, quantize_mlx_affine
    vocab_text = open(os.path.join(ROOT, "f5_tts_mlx_amd", "assets", "vocab.txt")).read()
    cfg = dataclasses.replace(F5TTS_335M, text_num_embeds=len(vocab_text.split("\n")) - 1, depth=depth)
    w = synthetic_weights(cfg, seed=seed)
    w["transformer.rotary_embed.inv_freq"] = (1.0 / (10000 ** (np.arange(0, 64, 2, dtype=np.float32) / 64))).astype(np.float32)
    with open(os.path.join(dirname, "vocab.txt"), "w") as f:
        f.write(vocab_text)
    save_file(_upstream_checkpoint(w), os.path.join(dirname, "model_v1.safetensors"))
    q = {}
    for k, v in w.items():          # the package's rule for an MLX 8-bit file: Linear weights whose input width is a multiple of 64
        if k.endswith(".weight") and v.ndim == 2 and v.shape[1] % 64 == 0 and "text_embed.text_embed" not in k:
            pk, sc, bi = quantize_mlx_affine(v, 8)
            q[k], q[k[:-7] + ".scales"], q[k[:-7] + ".biases"] = pk, sc, bi
        else:
            q[k] = v
    save_file(q, os.path.join(dirname, "model_v1_8b.safetensors"))


def test_checkpoint_conversion_matches_reference_from_pretrained_live(tmp_path):
    """The reference's own `F5TTS.from_pretrained` (unmodified, over the mlx emulation; hub access and the third-party vocoder
    stubbed) loaded a synthetic UPSTREAM-named 335M checkpoint directory (upstream_checkpoint_dir, 2 blocks): its key renames / axis
    swaps (cfm.py:477-508) and the strict load into the reference's module tree define the truth, recorded as digests of every
    parameter in tests/golden/ref_from_pretrained.json; `weights.convert_upstream_weights` must yield the same names and arrays bit
    for bit.  Then the 8-bit path: `nn.quantize` with the reference's predicate (cfm.py:510-515) decided which Linears expect packed
    weights; the file written with the package's rule must hold exactly those modules and exactly the arrays the reference's strict
    load ended up with.  The resulting name -> shape map is compared with the committed tests/golden/ref_checkpoint_keymap.json."""
    from safetensors.numpy import load_file
    from f5_tts_mlx_amd.weights import convert_upstream_weights, dequantize_mlx_checkpoint
    rec = json.load(open(os.path.join(GOLDEN, "ref_from_pretrained.json")))
    depth = rec["depth"]
    upstream_checkpoint_dir(str(tmp_path), depth, rec["weights_seed"])
    # ---- full precision, convert_weights=True (the default): cfm.py:477-508
    ours = convert_upstream_weights(load_file(str(tmp_path / "model_v1.safetensors")))
    got = {k: array_digest(v) for k, v in ours.items()}
    assert set(got) == set(rec["params"]), (sorted(set(rec["params"]) - set(got))[:5], sorted(set(got) - set(rec["params"]))[:5])
    assert [k for k in got if got[k] != rec["params"][k]] == []
    # ---- 8-bit file: nn.quantize's predicate decides which modules expect (weight uint32, scales, biases); cfm.py:510-515
    qfile = load_file(str(tmp_path / "model_v1_8b.safetensors"))
    assert sorted(k[:-7] for k in qfile if k.endswith(".scales")) == rec["quantized"]
    assert {k: array_digest(v) for k, v in qfile.items()} == rec["params_8bit"]
    deq = dequantize_mlx_checkpoint(qfile, 8)
    assert set(deq) == set(ours) and all(deq[k].shape == ours[k].shape for k in ours)
    want = json.load(open(os.path.join(GOLDEN, "ref_checkpoint_keymap.json")))      # written from a full-depth (22 blocks) run
    keep = lambda k: ".transformer_blocks." not in k or int(k.split(".transformer_blocks.")[1].split(".")[0]) < depth   # noqa: E731
    want = dict(keymap={k: v for k, v in want["keymap"].items() if keep(k)}, quantized=[k for k in want["quantized"] if keep(k)])
    assert dict(keymap={k: list(v.shape) for k, v in sorted(ours.items())}, quantized=rec["quantized"]) == want


def test_checkpoint_conversion_matches_committed_reference_keymap():
    """Without the reference checkout (GPU box): `convert_upstream_weights` maps an upstream-named state dict onto exactly the
    parameter names / shapes the reference's from_pretrained produced (tests/golden/ref_checkpoint_keymap.json, written by the
    live test above), and the package's 8-bit rule selects exactly the modules the reference's `nn.quantize` predicate did."""
    import dataclasses
    from f5_tts_mlx_amd.weights import F5TTS_335M, convert_upstream_weights, param_specs
    want = json.load(open(os.path.join(GOLDEN, "ref_checkpoint_keymap.json")))
    nvocab = want["keymap"]["transformer.text_embed.text_embed.weight"][0]
    cfg = dataclasses.replace(F5TTS_335M, text_num_embeds=nvocab - 1)
    shapes = {n: tuple(s) for n, s, _ in param_specs(cfg)}
    shapes["transformer.rotary_embed.inv_freq"] = (32,)
    up = _upstream_checkpoint({k: np.zeros(s, np.float32) for k, s in shapes.items()})     # zero-filled: names / layouts only
    ours = convert_upstream_weights(up)
    assert {k: list(v.shape) for k, v in sorted(ours.items())} == want["keymap"]
    rule = sorted(k[:-7] for k, s in shapes.items() if k.endswith(".weight") and len(s) == 2 and s[1] % 64 == 0
                  and "text_embed.text_embed" not in k)
    assert rule == want["quantized"]
    assert "transformer.input_embed.proj" not in rule and "transformer.proj_out" in rule          # 712 % 64 != 0; 1024 % 64 == 0
