"""Row-isolated batches, host side (docs/isolate_rows.md): the definition of the mode pinned on the CPU oracle, the inputs shown to
discriminate, argument validation, and the option's place in the C ABI.  No GPU."""
import ctypes as C
import inspect

import pytest

import isolate_oracle as IO
from f5test import E, O, F5TTS_335M
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import F5TTS

# margin over the 6.5e-7 measured (fp32 summation order of one BLAS build against another); the rows are O(1)
SOLO_TOL = 1e-5
MEL_L1_TOL = 1e-3            # the project's parity gate (tests/test_model_gpu.py)


@pytest.fixture(scope="module", params=[True, False], ids=["text_mask", "no_text_mask"])
def measured(request):
    """distances of the plain and of the isolated oracle's batched rows from the plain oracle's solo samples, per text_mask_padding"""
    tmp = request.param
    solo = IO.solo_reference(tmp)
    cfg, w = IO.config(tmp), IO.weights()

    def dist(dit):
        out = IO.batched(dit)
        return [IO.row_distance(out, solo, b) for b in range(3)]

    return tmp, dict(plain=dist(O.DiTOracle(cfg, w)), iso=dist(IO.IsolatedDiTOracle(cfg, w)),
                     **{wo: dist(IO.IsolatedDiTOracle(cfg, w, without=wo)) for wo in ("grn", "convpos", "dwconv")})


def test_isolated_oracle_rows_equal_their_solo_sample(measured):
    tmp, d = measured
    print(f"[isolate] text_mask_padding={tmp} isolated rows vs solo: {d['iso']}")
    assert max(d["iso"]) <= SOLO_TOL, d["iso"]


def test_inputs_discriminate(measured):
    tmp, d = measured
    print(f"[isolate] text_mask_padding={tmp} plain rows vs solo: {d['plain']}")
    assert d["plain"][0] <= SOLO_TOL                # the longest row has no padding
    assert d["plain"][1] > 1e-2 and d["plain"][2] > 1e-2, d["plain"]


def test_each_leak_is_visible_on_its_own(measured):
    """leaving any one of the three pieces as the plain oracle has it puts the short rows beyond the parity gate (the depthwise conv only
    without the text mask: with it the padding of the text path is zero already)"""
    tmp, d = measured
    print(f"[isolate] text_mask_padding={tmp} without grn {d['grn']} convpos {d['convpos']} dwconv {d['dwconv']}")
    for piece in ("grn", "convpos") + (() if tmp else ("dwconv",)):
        assert d[piece][1] > MEL_L1_TOL and d[piece][2] > MEL_L1_TOL, (piece, d[piece])
    if tmp:
        assert max(d["dwconv"]) <= SOLO_TOL, d["dwconv"]


# ---- argument validation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [1, 0, "yes", None, [True]])
def test_isolate_rows_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        E.check_isolate_rows(bad, "f16")
    # before a model is loaded or a reference is read, in both front ends
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        G.generate_many([("Hello there.", None, None)], isolate_rows=bad)
    with pytest.raises(ValueError, match="isolate_rows must be a bool"):
        G.generate("Hello there. And again.", batch_sentences=True, isolate_rows=bad)


def test_isolate_rows_refuses_mxfp8_in_python():
    for prec in ("f16", "bf16", "bf16x3"):
        assert E.check_isolate_rows(True, prec) is True and E.check_isolate_rows(False, prec) is False
    assert E.check_isolate_rows(False, "mxfp8") is False
    with pytest.raises(ValueError, match="isolate_rows=True is not supported on an mxfp8 model"):
        E.check_isolate_rows(True, "mxfp8")


def test_isolate_rows_is_a_call_level_argument_everywhere():
    for fn in (E.Engine.sample, E.Engine.dit_forward, F5TTS.sample, G.generate, G.generate_many):
        p = inspect.signature(fn).parameters["isolate_rows"]
        assert p.default is False, fn
    # not a per-request key: one engine option and one graph per value
    with pytest.raises(ValueError, match="isolate_rows"):
        G.request_controls([dict(isolate_rows=True)], 1, [], dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None, speed=1.0))
    assert G.parse_args(["--text", "x", "--isolate-rows"]).isolate_rows is True
    assert G.parse_args(["--text", "x"]).isolate_rows is False
    assert "isolate_rows" in E.OPTION_NAMES and "isolate_rows" in E.FALLBACK_OPTIONS


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def handles():
    """engine handles without an arena (creating one plans sizes and touches no device)"""
    lib = E.load_library()
    made = []

    def make(precision):
        h = C.c_void_p()
        cfg = E.to_c_config(F5TTS_335M)
        assert lib.f5_engine_create(C.byref(cfg), E.PRECISIONS[precision], C.byref(h)) == 0
        made.append(h)
        return h

    yield lib, make
    for h in made:
        lib.f5_engine_destroy(h)


def test_option_is_a_switch_and_is_listed(handles):
    lib, make = handles
    h = make("f16")
    v = C.c_int(12345)
    assert lib.f5_engine_get_option(h, b"isolate_rows", C.byref(v)) == 0 and v.value == 0          # off by default
    for put, want in ((5, 1), (0, 0), (-7, 1), (1, 1)):
        assert lib.f5_engine_set_option(h, b"isolate_rows", put) == 0
        assert lib.f5_engine_get_option(h, b"isolate_rows", C.byref(v)) == 0 and v.value == want
    assert lib.f5_engine_set_option(h, b"no_such_option", 1) != 0
    msg = lib.f5_last_error().decode()
    # the launch options inside the parentheses, as before; the new option behind them under its own heading
    listed = [n.strip() for n in msg[msg.index("(") + 1:msg.rindex(")")].split(",")]
    assert msg.endswith("; row isolation: isolate_rows"), msg
    assert "isolate_rows" not in listed and sorted(listed + ["isolate_rows"]) == sorted(E.OPTION_NAMES), msg


def test_mxfp8_refuses_the_option_with_its_own_message(handles):
    lib, make = handles
    a = E.F5SampleArgs()
    calls = [("f5_sample", lambda h: lib.f5_sample(h, C.byref(a), None)),
             ("f5_sample_edit", lambda h: lib.f5_sample_edit(h, C.byref(a), C.c_void_p(64), None)),
             ("f5_dit_forward", lambda h: lib.f5_dit_forward(h, C.byref(a), None, C.c_float(0.5), None, None, None))]
    h8 = make("mxfp8")
    assert lib.f5_engine_set_option(h8, b"isolate_rows", 1) == 0
    for name, call in calls:
        assert call(h8) != 0
        msg = lib.f5_last_error().decode()
        assert msg.startswith(name + ": engine option isolate_rows = 1 is not supported in precision mxfp8"), msg
    # ... and only that combination: with the option off, or in another precision, the call gets as far as the next check
    assert lib.f5_engine_set_option(h8, b"isolate_rows", 0) == 0
    h16 = make("f16")
    assert lib.f5_engine_set_option(h16, b"isolate_rows", 1) == 0
    for h in (h8, h16):
        assert lib.f5_sample(h, C.byref(a), None) != 0
        assert lib.f5_last_error() == b"weights are not finalized"


def test_new_entry_points_are_exported():
    lib = E.load_library()
    assert hasattr(lib, "f5_op_convpos_ragged") and hasattr(lib, "f5_op_grn_ragged")
