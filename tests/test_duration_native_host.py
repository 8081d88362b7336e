"""The duration predictor's C ABI (csrc/duration.hip) without a device: `f5_duration_create` only plans, like `f5_vocoder_create`."""
import ctypes as C
import os
import subprocess

import pytest

from f5test import ROOT
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd.duration import F5DurationArgs, F5DurationConfig

# the predictor F5TTS.from_pretrained builds (cfm.py:429-438): dim 512, depth 8, heads 8, text_dim 512, ff_mult 2, conv_layers 2
CFG_335M = dict(dim=512, depth=8, heads=8, dim_head=64, ff_dim=1024, mel_dim=100, text_num_embeds=2545, text_dim=512, conv_layers=2,
                conv_pos_kernel=31, conv_pos_groups=16, text_max_pos=4096)


def _cfg(**over):
    return F5DurationConfig(**dict(CFG_335M, **over))


def _create(lib, precision=E.PRECISIONS["f16"], **over):
    h = C.c_void_p()
    cfg = _cfg(**over)
    return lib.f5_duration_create(C.byref(cfg), precision, C.byref(h)), h


@pytest.fixture()
def handle():
    lib = E.load_library()
    lib.f5_duration_destroy.restype = None
    rc, h = _create(lib)
    assert rc == 0, lib.f5_last_error()
    yield lib, h
    lib.f5_duration_destroy(h)


def test_create_plans_the_335m_predictor_without_a_device(handle):
    lib, h = handle
    n = C.c_size_t()
    assert lib.f5_duration_weights_bytes(h, C.byref(n)) == 0
    # at least one 16-bit copy of the block matrices (4 dim^2 + 2 dim ff per block) plus the fp32 embedding table
    assert n.value > 8 * (4 * 512 * 512 + 2 * 512 * 1024) * 2 + 2546 * 512 * 4
    rc, h3 = _create(lib, precision=E.PRECISIONS["bf16x3"])
    n3 = C.c_size_t()
    assert rc == 0 and lib.f5_duration_weights_bytes(h3, C.byref(n3)) == 0 and n3.value > n.value      # hi + lo
    lib.f5_duration_destroy(h3)
    assert lib.f5_duration_graph_count(h) == 0


@pytest.mark.parametrize("over,precision,word", [
    (dict(dim_head=32, heads=16), 3, b"dim_head"),
    (dict(conv_pos_groups=4), 3, b"conv_pos_groups"),          # 128-channel groups
    (dict(conv_pos_groups=32), 3, b"conv_pos_groups"),         # 16-channel groups
    (dict(mel_dim=129), 3, b"mel_dim"),
    (dict(text_dim=384), 3, b"text_dim"),
    (dict(conv_layers=0), 3, b"conv_layers"),
    (dict(), E.PRECISIONS["mxfp8"], b"precision"),
])
def test_create_refuses_what_the_kernels_cannot_run(over, precision, word):
    lib = E.load_library()
    rc, h = _create(lib, precision=precision, **over)
    assert rc != 0 and not h.value
    assert word in lib.f5_last_error(), lib.f5_last_error()


def test_load_tensor_checks_name_shape_and_arena(handle):
    lib, h = handle
    buf = (C.c_float * (512 * 512))()
    ok_name = b"transformer.transformer_blocks.0.attn.to_q.weight"
    shp = (C.c_int64 * 2)(512, 512)
    assert lib.f5_duration_load_tensor(h, ok_name, buf, 2, shp) != 0                   # right name and shape, no arena yet
    assert b"f5_duration_set_weights_arena" in lib.f5_last_error()
    assert lib.f5_duration_load_tensor(h, b"duration_predictor." + ok_name, buf, 2, shp) != 0     # the prefixed name is the same tensor
    assert b"f5_duration_set_weights_arena" in lib.f5_last_error()
    assert lib.f5_duration_load_tensor(h, b"transformer.time_embed.time_mlp.layers.0.weight", buf, 2, shp) != 0
    assert b"unknown" in lib.f5_last_error() and b"time_embed" in lib.f5_last_error()
    bad = (C.c_int64 * 2)(512, 256)
    assert lib.f5_duration_load_tensor(h, ok_name, buf, 2, bad) != 0
    assert b"to_q.weight" in lib.f5_last_error() and b"dim 1" in lib.f5_last_error()
    bad3 = (C.c_int64 * 3)(512, 31, 64)                                               # 512 / 16 = 32-channel groups, not 64
    assert lib.f5_duration_load_tensor(h, b"transformer.input_embed.conv_pos_embed.conv1d.layers.0.weight", buf, 3, bad3) != 0
    assert b"dim 2" in lib.f5_last_error()
    assert lib.f5_duration_finalize(h, None) != 0 and b"arena" in lib.f5_last_error()


def test_workspace_bytes_bounds_and_monotony(handle):
    lib, h = handle

    def ws(B, n_in, nt):
        n = C.c_size_t()
        rc = lib.f5_duration_workspace_bytes(h, B, n_in, nt, C.byref(n))
        return rc, n.value

    assert ws(1, 3, 2)[0] != 0 and b"N = max(n_in, nt) >= 4" in lib.f5_last_error()
    assert ws(1, 4097, 10)[0] != 0 and b"text_max_pos" in lib.f5_last_error()
    assert ws(1, 10, 4097)[0] != 0 and b"text_max_pos" in lib.f5_last_error()
    assert ws(0, 64, 64)[0] != 0 and ws(1, 0, 64)[0] != 0 and ws(1, 64, 0)[0] != 0
    assert ws(1, 4, 1)[0] == 0 and ws(1, 4096, 4096)[0] == 0
    base = ws(2, 100, 60)
    assert base[0] == 0 and base[1] > 0 and base[1] % 256 == 0
    prev = 0
    for B in (1, 2, 3, 8):
        rc, n = ws(B, 100, 60)
        assert rc == 0 and n >= prev
        prev = n
    prev = 0
    for n_in in (4, 63, 64, 65, 100, 281, 937):
        rc, n = ws(2, n_in, 60)
        assert rc == 0 and n >= prev
        prev = n
    prev = 0
    for nt in (1, 59, 60, 100, 101, 160, 500):
        rc, n = ws(2, 100, nt)
        assert rc == 0 and n >= prev
        prev = n
    assert ws(2, 281, 160)[1] > ws(2, 100, 60)[1]
    # N = max(n_in, nt) decides every buffer but the staging of the caller's inputs: (64, 80) and (80, 64) differ by at most the mel
    # staging buffer [B][N][mel_dim] fp32
    a, b = ws(2, 64, 80), ws(2, 80, 64)
    assert a[0] == 0 and b[0] == 0 and abs(a[1] - b[1]) <= 2 * 80 * 100 * 4 + 256


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "f5tts_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(f5_duration_config), offsetof(f5_duration_config, conv_pos_groups), offsetof(f5_duration_config, text_max_pos),'
                   'sizeof(f5_duration_args), offsetof(f5_duration_args, frame_rate), offsetof(f5_duration_args, workspace_bytes));'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K, A = F5DurationConfig, F5DurationArgs
    assert got == [C.sizeof(K), K.conv_pos_groups.offset, K.text_max_pos.offset, C.sizeof(A), A.frame_rate.offset, A.workspace_bytes.offset]
    assert C.sizeof(K) == 12 * 4
