"""DiT geometries beyond the 335M family (docs/geometries.md), the host side: the parameter inventory of configurations whose attention
inner width differs from the model width, the weight store's packing of narrow conv-pos groups, and what f5_engine_create accepts and
refuses.  No GPU: the library's host functions only.
"""
import ctypes as C
import dataclasses
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from f5test import E, ROOT, TINY, F5TTS_335M, DiTConfig, synthetic_weights
from f5_tts_mlx_amd import weights as W
from f5_tts_mlx_amd.weights import param_specs

# the smallest configuration with all three properties: inner width 512 under a 768-wide model, 16 conv-pos groups of 48 channels,
# 384-wide text
NARROW = DiTConfig(dim=768, depth=2, heads=8, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=384, conv_layers=2, conv_pos_groups=16)


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


# computed at the commit before the inner width entered param_specs: sha256 of repr(param_specs), parameter count, five tensors of
# synthetic_weights(cfg, seed=42)
_T = "transformer."
PARENT = {
    "TINY": (TINY, "9686852346818609", 63, 3813476, {
        _T + "time_embed.time_mlp.layers.0.weight": "acda21bd0aa7200c",
        _T + "input_embed.conv_pos_embed.conv1d.layers.2.weight": "958454bc940f6046",
        _T + "transformer_blocks.0.attn.to_k.weight": "aca36ce402e76e2e",
        _T + "transformer_blocks.1.attn.to_out.layers.0.weight": "07ffb8a2a2dcdb1f",
        _T + "proj_out.bias": "b77f6c029f7ca07d"}),
    "F5TTS_335M": (F5TTS_335M, "3201d4eec66f9844", 363, 337096804, {
        _T + "time_embed.time_mlp.layers.0.weight": "691143c5e6f6c268",
        _T + "input_embed.conv_pos_embed.conv1d.layers.2.weight": "48fdcbe8db307bde",
        _T + "transformer_blocks.0.attn.to_k.weight": "868004c79c2bac7e",
        _T + "transformer_blocks.1.attn.to_out.layers.0.weight": "245e267a17d56d70",
        _T + "proj_out.bias": "b19bd777e2c26797"}),
}


@pytest.mark.parametrize("name", list(PARENT))
def test_weights_of_the_existing_configurations_are_unchanged(name):
    """the goldens depend on the seeded draws: for heads * dim_head == dim the shapes, their order and every draw stay what they were"""
    cfg, specs_sha, nspecs, nparams, tensors = PARENT[name]
    specs = param_specs(cfg)
    assert hashlib.sha256(repr(specs).encode()).hexdigest()[:16] == specs_sha and len(specs) == nspecs and W.num_params(cfg) == nparams
    w = synthetic_weights(cfg, seed=42)
    assert {k: _sha(w[k]) for k in tensors} == tensors


def _expected_shapes(cfg):
    """the reference constructor's parameter shapes, written out from dit.py (Attention: dim -> heads * dim_head -> dim, dit.py:117-125;
    ConvPositionEmbedding: groups = 16 whatever the width, dit.py:30; TextEmbedding: text_dim, ConvNeXt blocks text_dim -> 2 text_dim)"""
    D, I, Dt = cfg.dim, cfg.heads * cfg.dim_head, cfg.text_dim
    want = {
        _T + "transformer_blocks.0.attn.to_q.weight": (I, D), _T + "transformer_blocks.0.attn.to_q.bias": (I,),
        _T + "transformer_blocks.0.attn.to_k.weight": (I, D), _T + "transformer_blocks.0.attn.to_v.weight": (I, D),
        _T + "transformer_blocks.0.attn.to_v.bias": (I,),
        _T + "transformer_blocks.0.attn.to_out.layers.0.weight": (D, I), _T + "transformer_blocks.0.attn.to_out.layers.0.bias": (D,),
        _T + "transformer_blocks.0.ff.ff.layers.0.layers.0.weight": (D * cfg.ff_mult, D),
        _T + "input_embed.conv_pos_embed.conv1d.layers.0.weight": (D, 31, D // 16),
        _T + "input_embed.conv_pos_embed.conv1d.layers.2.weight": (D, 31, D // 16),
        _T + "input_embed.proj.weight": (D, 2 * cfg.mel_dim + Dt),
        _T + "text_embed.text_embed.weight": (cfg.text_num_embeds + 1, Dt),
        _T + "text_embed.text_blocks.layers.0.dwconv.weight": (Dt, 7, 1),
        _T + "text_embed.text_blocks.layers.0.pwconv1.weight": (2 * Dt, Dt),
        _T + "text_embed.text_blocks.layers.0.pwconv2.weight": (Dt, 2 * Dt),
    }
    return want


# Runs in an interpreter of its own: the numpy emulation of mlx registers stand-ins (mlx, einx, jieba, ...) in sys.modules, which no
# other test of the session may find.  argv: repository root, reference checkout, then one JSON object of DiT(...) arguments per
# configuration; prints one JSON object {parameter name: shape} per configuration.
_REF_SHAPES_PROGRAM = """
import json, sys
root, ref_dir = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, ref_dir]
from oracle import mlx_shim
mlx_shim.install()
from f5_tts_mlx import dit as ref_dit

def flatten(tree, prefix=""):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from flatten(v, prefix + str(k) + ".")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from flatten(v, prefix + str(i) + ".")
    elif hasattr(tree, "shape"):
        yield prefix[:-1], [int(d) for d in tree.shape]

for arg in sys.argv[3:]:
    print(json.dumps(dict(flatten(ref_dit.DiT(**json.loads(arg)).parameters()))))
"""
_REF_CONFIGS = {"NARROW": NARROW, "REF_SMALL": W.REF_SMALL}


@pytest.fixture(scope="module")
def reference_shapes():
    """{configuration name: {parameter name: shape}} of the reference's own DiT(...) at depth 2, built over the numpy emulation of mlx in
    ONE child interpreter for both configurations; None where the reference checkout is absent"""
    ref_dir = os.environ.get("F5_REFERENCE_DIR", "/root/reference")
    if not os.path.isdir(os.path.join(ref_dir, "f5_tts_mlx")):
        return None
    args = []
    for cfg in _REF_CONFIGS.values():
        args.append(json.dumps(dict(dim=cfg.dim, depth=2, heads=cfg.heads, dim_head=cfg.dim_head, ff_mult=cfg.ff_mult, mel_dim=cfg.mel_dim,
                                    text_num_embeds=cfg.text_num_embeds, text_dim=cfg.text_dim, conv_layers=cfg.conv_layers)))
    r = subprocess.run([sys.executable, "-c", _REF_SHAPES_PROGRAM, ROOT, ref_dir] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == len(_REF_CONFIGS), r.stdout[-2000:]
    return {name: {"transformer." + k: tuple(s) for k, s in json.loads(l).items()} for name, l in zip(_REF_CONFIGS, lines)}


@pytest.mark.parametrize("name", list(_REF_CONFIGS))
def test_weight_shapes_match_the_reference_constructor(reference_shapes, name):
    cfg = _REF_CONFIGS[name]
    got = {n: tuple(s) for n, s, _ in param_specs(cfg)}
    for n, s in _expected_shapes(cfg).items():
        assert got[n] == s, (n, got[n], s)
    assert cfg.conv_pos_groups == 16 and cfg.dim // cfg.conv_pos_groups == 48 and cfg.inner_dim == 512 and cfg.text_dim == 384
    # where the reference checkout is present: its own DiT(...) must hold exactly the tensors of the inventory
    if reference_shapes is None:
        return
    ref = dict(reference_shapes[name])
    ref.pop("transformer.rotary_embed.inv_freq", None)
    ours = {n: tuple(s) for n, s, _ in param_specs(dataclasses.replace(cfg, depth=2))}
    assert ref == ours, (sorted(set(ref) ^ set(ours))[:6], [(k, ref[k], ours[k]) for k in ref if k in ours and ref[k] != ours[k]][:6])


def test_synthetic_weights_pass_the_inventory_check():
    W.check_weights(NARROW, synthetic_weights(NARROW, seed=5))


# ---- conv-pos packing --------------------------------------------------------------------------------------------------------------
def _pack(lib, w, cpg):
    Cc, taps, gin = w.shape
    assert gin == cpg
    rows = lib.f5_op_conv_packed_rows(Cc, cpg)
    out = np.full((rows, taps, 64), np.nan, np.float32)
    assert lib.f5_op_pack_conv_groups(w.ctypes.data_as(C.c_void_p), Cc, taps, cpg, out.ctypes.data_as(C.c_void_p)) == 0, lib.f5_last_error()
    return out


def test_conv_pos_packing_48_round_trips(lib):
    """a 48-channel group in a 64-row, 64-column tile of its own, zeros outside the 48 x 48 block of every tap"""
    r = np.random.default_rng(48)
    Cc, taps = 768, 31
    w = r.standard_normal((Cc, taps, 48)).astype(np.float32)
    m = _pack(lib, w, 48)
    assert m.shape == (16 * 64, taps, 64)
    t = m.reshape(16, 64, taps, 64)
    assert np.array_equal(t[:, :48, :, :48].reshape(Cc, taps, 48), w)                  # the way back: the 48 x 48 blocks are the tensor
    assert not t[:, 48:].any() and not t[:, :, :, 48:].any()                           # exact zeros (no NaN left from the fill)


def test_conv_pos_packing_32_is_what_the_duration_predictor_did(lib):
    """the block-diagonal super groups, restated from the loop the duration predictor's loader ran before the packing moved into the
    weight store: output channel o keeps its 32 input channels in the half of the 64 columns that holds its group"""
    r = np.random.default_rng(32)
    D, kc = 512, 31
    w = r.standard_normal((D, kc, 32)).astype(np.float32)
    want = np.zeros((D, kc, 64), np.float32)
    for o in range(D):
        off = ((o // 32) % 2) * 32
        want[o, :, off:off + 32] = w[o]
    assert np.array_equal(_pack(lib, w, 32), want)


def test_conv_pos_packing_64_is_the_tensor_and_other_widths_are_refused(lib):
    w = np.random.default_rng(64).standard_normal((128, 5, 64)).astype(np.float32)
    assert np.array_equal(_pack(lib, w, 64), w)
    assert lib.f5_op_conv_packed_rows(768, 40) == -1 and lib.f5_op_conv_packed_rows(100, 48) == -1
    buf = np.zeros(16, np.float32)
    assert lib.f5_op_pack_conv_groups(buf.ctypes.data_as(C.c_void_p), 640, 1, 40, buf.ctypes.data_as(C.c_void_p)) != 0
    assert b"channels per group" in lib.f5_last_error()


def test_loader_of_a_narrow_engine_takes_the_reference_shapes(lib):
    """the loader of NARROW takes the reference shapes (inner x dim, dim x inner, (dim, 31, 48)) and refuses the square ones, and the arena
    has room for the zero-padded conv tiles.  Where to_q / to_k / to_v land in the fused matrix (inner rows apart) needs a device: the
    model tests of tests/test_geometries_model_gpu.py check it through every forward"""
    h = C.c_void_p()
    cfg = E.to_c_config(NARROW)
    assert lib.f5_engine_create(C.byref(cfg), E.PRECISIONS["f16"], C.byref(h)) == 0, lib.f5_last_error()
    try:
        buf = (C.c_float * 4)()

        def load(name, *shape):
            rc = lib.f5_load_tensor(h, name.encode(), buf, len(shape), (C.c_int64 * len(shape))(*shape))
            return rc, lib.f5_last_error().decode()

        blk = "transformer.transformer_blocks.1.attn."
        no_arena = "f5_set_weights_arena must be called first"                              # name and shape passed: stops at the arena
        assert load(blk + "to_q.weight", 512, 768) == (2, no_arena) and load(blk + "to_v.bias", 512) == (2, no_arena)
        assert load(blk + "to_out.layers.0.weight", 768, 512) == (2, no_arena)
        assert load("transformer.input_embed.conv_pos_embed.conv1d.layers.0.weight", 768, 31, 48) == (2, no_arena)
        assert load("transformer.text_embed.text_blocks.layers.0.pwconv1.weight", 768, 384) == (2, no_arena)
        for name, shape in ((blk + "to_q.weight", (768, 768)), (blk + "to_out.layers.0.weight", (768, 768)),
                            ("transformer.input_embed.conv_pos_embed.conv1d.layers.0.weight", (768, 31, 64))):
            rc, msg = load(name, *shape)
            assert rc != 0 and "expected" in msg, (name, msg)
        # the arena: everything param_specs lists in 16 bits or fp32, plus the zero padding of the conv tiles (768 -> 1024 rows, 48 -> 64 columns)
        n = C.c_size_t()
        assert lib.f5_weights_bytes(h, C.byref(n)) == 0
        conv_packed = 2 * (16 * 64) * 31 * 64 * 2
        assert n.value > conv_packed + 2 * NARROW.depth * (3 * 512 * 768 + 768 * 512)
    finally:
        lib.f5_engine_destroy(h)


# ---- what f5_engine_create accepts and refuses --------------------------------------------------------------------------------------
def _create(lib, cfg, precision="f16"):
    h = C.c_void_p()
    c = E.to_c_config(cfg)
    rc = lib.f5_engine_create(C.byref(c), E.PRECISIONS[precision], C.byref(h))
    msg = lib.f5_last_error().decode()
    if rc == 0:
        lib.f5_engine_destroy(h)
    return rc, msg


UPSTREAM_SMALL_MINI = DiTConfig(dim=768, depth=2, heads=12, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=512, conv_layers=2,
                                conv_pos_groups=16)
INNER_ONLY = DiTConfig(dim=512, depth=2, heads=4, dim_head=64, ff_mult=2, text_num_embeds=64, text_dim=256, conv_layers=2, conv_pos_groups=8)


@pytest.mark.parametrize("cfg", [NARROW, W.REF_SMALL, UPSTREAM_SMALL_MINI, INNER_ONLY, DiTConfig(dim=1024, depth=2, heads=8),
                                 DiTConfig(dim=512, depth=1, heads=8, conv_pos_groups=16, text_dim=128)],
                         ids=["NARROW", "REF_SMALL", "upstream_small", "inner_only", "dim1024_heads8", "groups_of_32_text_128"])
@pytest.mark.parametrize("precision", ["f16", "bf16", "bf16x3"])
def test_engine_create_accepts_the_new_geometries(lib, cfg, precision):
    rc, msg = _create(lib, cfg, precision)
    assert rc == 0, msg


@pytest.mark.parametrize("change,precision,word", [
    (dict(heads=5), "f16", "heads * dim_head must be a multiple of 256 (got 5 * 64 = 320)"),
    (dict(heads=20), "f16", "heads * dim_head must be <= 1024 (got 20 * 64 = 1280)"),
    (dict(dim=640), "f16", "dim / conv_pos_groups must be 32, 48 or 64 channels per group (got 640 / 16)"),      # 40 channels per group
    (dict(text_dim=200), "f16", "text_dim must be a multiple of 128 and <= 1024 (got 200)"),
    (dict(), "mxfp8", "mxfp8 needs heads * dim_head == dim, 64-channel conv-pos groups and text_dim % 256 == 0"),
], ids=["inner_320", "inner_1280", "40_channels_per_group", "text_200", "mxfp8_narrow"])
def test_engine_create_refuses_each_new_bound_with_its_own_message(lib, change, precision, word):
    rc, msg = _create(lib, dataclasses.replace(NARROW, **change), precision)
    assert rc != 0 and word in msg, (rc, msg)


def test_group_widths_next_to_the_accepted_ones(lib):
    """768 / 24 = 32 channels passes, 768 / 8 = 96 does not; 32-channel groups come in pairs"""
    assert _create(lib, dataclasses.replace(NARROW, conv_pos_groups=24))[0] == 0
    rc, msg = _create(lib, dataclasses.replace(NARROW, conv_pos_groups=8))
    assert rc != 0 and "32, 48 or 64 channels per group (got 768 / 8)" in msg, msg


def test_mxfp8_inside_the_family_is_untouched(lib):
    assert _create(lib, TINY, "mxfp8")[0] == 0
    for change in (dict(heads=8, dim=1024, depth=1), dict(text_dim=384, depth=1), dict(dim=768, heads=12, conv_pos_groups=16, depth=1)):
        rc, msg = _create(lib, dataclasses.replace(F5TTS_335M, **change), "mxfp8")
        assert rc != 0 and msg.startswith("mxfp8 needs heads * dim_head == dim"), (change, msg)


def test_convpos_route_of_narrow_groups_is_never_the_ring_kernel(lib):
    def route(B, N, groups, cpg, nseg=1):
        buf = C.create_string_buffer(64)
        assert lib.f5_debug_convpos_route_groups(B, N, groups, cpg, nseg, buf, 64) == 0, lib.f5_last_error()
        return buf.value.decode()

    def route64(B, N, groups, nseg=1):
        buf = C.create_string_buffer(64)
        assert lib.f5_debug_convpos_route(B, N, groups, nseg, buf, 64) == 0
        return buf.value.decode()

    assert route64(2, 937, 16) == "f5_convpos_ring_kernel+xcd" == route(2, 937, 16, 64)         # the 335M batch-1 launch: as it was
    assert route(2, 937, 16, 48) == "f5_convpos_kernel<false,1,48>+xcd"
    assert route(2, 937, 16, 48, 3) == "f5_convpos_kernel<true,1,48>+xcd"
    assert route(2, 937, 32, 32) == "f5_convpos_kernel<false,1>+xcd"                           # 16 super groups on the 64-channel kernel
    assert route(2, 937, 12, 48) == "f5_convpos_kernel<false,1,48>"                            # 12 groups: the 3-D grid
    assert lib.f5_debug_set_convpos_tps(8) == 0
    try:
        assert route(1, 100, 16, 64) == "f5_convpos_ring_kernel+xcd"
        assert route(1, 100, 16, 48) == "f5_convpos_kernel<false,1,48>+xcd" and route(1, 100, 16, 32) == "f5_convpos_kernel<false,1>+xcd"
    finally:
        assert lib.f5_debug_set_convpos_tps(0) == 0
