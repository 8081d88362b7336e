"""Multistep solvers ab2 / ab3, host side (docs/multistep.md): the variable-step weights, their start-up and degenerate spacings, the
workspace plan, the method names on their way down, and the reference helper's own power to tell the rule from three seeded mistakes.
No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import multistep_ref as MS
from f5test import O, TINY, DiTConfig, synthetic_weights
from f5_tts_mlx_amd import cfm
from f5_tts_mlx_amd import engine as E
from f5_tts_mlx_amd import generate as G
from f5_tts_mlx_amd.cfm import ab_weights, prepare_lengths, time_grid

U32 = 2.0 ** -24                   # unit roundoff of fp32: the one rounding of a weight


def _irregular(n, seed):
    r = np.random.default_rng(seed)
    return np.cumsum(np.concatenate([[0.0], r.uniform(0.01, 0.3, n - 1)])).astype(np.float32)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def test_uniform_grid_gives_the_classical_coefficients():
    t = (np.arange(9) / 8).astype(np.float32)                                   # exact in fp32: the spacings are equal in fp64 too
    for order in (2, 3):
        for i in range(8):
            want = np.asarray(MS.UNIFORM[min(order, i + 1)], np.float64).astype(np.float32)     # the fp64 coefficient rounded once
            got = ab_weights(t, i, order)
            assert got.dtype == np.float32 and got.shape == (3,) and np.array_equal(got, want), (order, i, got)
    assert np.array_equal(ab_weights(t, 0, 3), np.float32([1, 0, 0]))            # step 0 is the Euler step, literally
    assert np.array_equal(ab_weights(t, 5, 1), np.float32([1, 0, 0]))


@pytest.mark.parametrize("grid", ["sway", "sway32", "irregular"])
def test_weights_integrate_polynomials_below_their_order(grid):
    """sum_j w_j t_{i-j}^q = (t_{i+1}^{q+1} - t_i^{q+1}) / ((q + 1) h) for q < order.  Bound: every weight is an fp64 value rounded once
    to fp32, so the left side is off by at most u32 sum_j |w_j| |t_{i-j}|^q; the fp64 evaluation of the weights and of both sides adds
    rounding of relative size 2^-53 times the cancellation of b - a and of the right side's difference (below 2^12 on these grids):
    2^-40 of the same sum covers it."""
    t = {"sway": time_grid(6, -1.0), "sway32": time_grid(32, -1.0), "irregular": _irregular(12, 5)}[grid]
    t64 = t.astype(np.float64)
    for order in (2, 3):
        for i in range(len(t) - 1):
            w = ab_weights(t, i, order).astype(np.float64)
            k = min(order, i + 1)
            assert np.count_nonzero(w) == k and np.all(np.isfinite(w)), (order, i, w)
            h = t64[i + 1] - t64[i]
            nodes = np.asarray([t64[i - j] if i - j >= 0 else 0.0 for j in range(3)])
            for q in range(k):
                lhs = float((w * nodes ** q).sum())
                rhs = (t64[i + 1] ** (q + 1) - t64[i] ** (q + 1)) / ((q + 1) * h)
                scale = float((np.abs(w) * np.abs(nodes) ** q).sum())
                assert abs(lhs - rhs) <= (U32 + 2.0 ** -40) * scale, (grid, order, i, q, lhs, rhs)


def test_repeated_grid_points_drop_the_order():
    #               0    1    2    3    4    5    6
    t = np.float32([0.0, 0.1, 0.1, 0.3, 0.4, 0.4, 0.6])
    nz = lambda i, order: int(np.count_nonzero(ab_weights(t, i, order)))          # noqa: E731
    for order in (2, 3):
        for i in range(len(t) - 1):
            assert np.all(np.isfinite(ab_weights(t, i, order))), (order, i)
    assert nz(2, 3) == 1 and nz(2, 2) == 1                                        # a = t2 - t1 = 0: first order
    assert nz(3, 3) == 2 and nz(3, 2) == 2                                        # a = 0.2, b = 0.2: b - a = 0, second order
    assert np.array_equal(ab_weights(t, 4, 3), np.float32([1, 0, 0]))             # a step of length 0: w0 = 1, the others +0
    assert ab_weights(t, 4, 3).tobytes() == np.float32([1, 0, 0]).tobytes()
    assert nz(5, 3) == 1                                                          # a = 0
    t2 = np.float32([0.0, 0.1, 0.3, 0.6])
    assert np.count_nonzero(ab_weights(t2, 1, 3)) == 2 and ab_weights(t2, 1, 3)[2] == 0.0       # start-up: step 1 is second order
    assert np.count_nonzero(ab_weights(t2, 2, 3)) == 3 and np.count_nonzero(ab_weights(t2, 2, 2)) == 2
    # a zero-length step keeps its spacings' order and adds nothing: the weights stay finite
    assert np.array_equal(ab_weights(np.float32([0.0, 0.1, 0.1]), 1, 2), np.float32([1, 0, 0]))
    # a grid that runs backwards in its history (a < 0) is first order as well
    assert np.array_equal(ab_weights(np.float32([0.2, 0.1, 0.3]), 1, 2), np.float32([1, 0, 0]))
    # an absent weight is exactly +0
    assert ab_weights(t2, 1, 3).tobytes()[8:] == np.float32(0.0).tobytes()


def test_odeint_ab_restatements():
    """dy/dt = 2 t on a non-uniform grid: the interpolant of a linear field is exact from the second step on, so ab2 and ab3 pick up only the
    Euler start-up's error t_1^2; dy/dt = 3 t^2: ab3 is exact from the third step on"""
    t = torch.from_numpy(_irregular(9, 3))
    y0 = torch.zeros(2, dtype=torch.float64)
    for fn in (cfm.odeint_ab2, cfm.odeint_ab3):
        y = fn(lambda tt, y: torch.full_like(y, 2.0 * float(tt)), y0, t)
        assert y.shape == (9, 2)
        assert torch.allclose(y[:, 0], t.double() ** 2 - float(t[1]) ** 2 * (torch.arange(9) > 0), atol=1e-6)
    y = cfm.odeint_ab3(lambda tt, y: torch.full_like(y, 3.0 * float(tt) ** 2), y0, t)
    d = y[:, 0] - t.double() ** 3
    assert torch.allclose(d[2:], d[2].expand(7), atol=1e-6) and abs(float(d[2])) > 1e-4
    e = cfm.odeint_euler(lambda tt, y: torch.full_like(y, 2.0 * float(tt)), y0, t)
    assert torch.equal(e[:2], cfm.odeint_ab2(lambda tt, y: torch.full_like(y, 2.0 * float(tt)), y0, t)[:2])


# ---- the reference helper tells the rule from the seeded mistakes ----------------------------------------------------------------------
def test_reference_helper_discriminates():
    """The shapes, grids and strengths of the GPU tests.  Each seeded mistake moves the helper's final mel (mean |delta| over the whole
    output) by more than the bound the GPU test holds f16 to against this helper, 1e-3 A, and so by more than the 1e-3 of bf16x3: a
    comparison in either mode cannot pass by indifference.  (The bf16 bound, 3e-2 A, is wider than what some of the mistakes move: that
    mode is measured against the helper, it does not tell the rule from them.)  Measured, mean |delta|: uniform_weights 0.05 - 0.2,
    stale_history 0.1 - 0.3, no_startup 0.03 - 0.05, with A = 3.9 (ab2) and 11.8 (ab3) on the sway -1 grid of 6 points."""
    ins = MS.inputs()
    dit = O.DiTOracle(TINY, synthetic_weights(TINY, seed=42))
    for route in ("scalar", "rows"):
        for method in ("ab2", "ab3"):
            A = MS.amplification(MS.grids_of(MS.ROUTES[route][0]), MS.ORDER[method])
            assert A > 1.0, (route, method, A)
            good, traj = MS.reference(dit, route, method, ins=ins)
            assert traj.shape == (MS.STEPS, MS.B, MS.N, TINY.mel_dim) and bool(torch.isfinite(good).all())
            for mistake in MS.MISTAKES:
                bad, _ = MS.reference(dit, route, method, mistake=mistake, ins=ins)
                d = float((bad - good).abs().mean())
                print(f"helper [{route}, {method}] A = {A:.3f} {mistake}: mean |delta| = {d:.4f}")
                assert d > 1e-3 * A, (route, method, mistake, d)
    # step 0 of the helper is the oracle's Euler step
    cond, text, y0 = ins
    _, et = O.sample(dit, cond, text, torch.tensor(MS.DURS), y0=y0, steps=MS.STEPS, method="euler", cfg_strength=MS.CFG, sway_sampling_coef=-1.0)
    _, traj = MS.reference(dit, "scalar", "ab3", ins=ins)
    assert float((traj[1] - et[1]).abs().max()) <= 1e-6 and float((traj[2] - et[2]).abs().mean()) > 1e-4


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def _handle(lib, cfg, prec):
    h = C.c_void_p()
    cc = E.to_c_config(cfg)
    assert lib.f5_engine_create(C.byref(cc), E.PRECISIONS[prec], C.byref(h)) == 0, lib.f5_last_error()
    return h


QUERIES = (("f5_workspace_bytes", (), False), ("f5_workspace_bytes_rows", (), True), ("f5_workspace_bytes_dual", (), True),
           ("f5_workspace_bytes_window", (0,), True), ("f5_workspace_bytes_window", (1,), True))


@pytest.mark.parametrize("cfgname,prec,B,N,nt,steps", [("tiny", "bf16x3", 3, 37, 9, 6), ("tiny", "mxfp8", 2, 80, 16, 3),
                                                       ("full", "f16", 2, 937, 120, 32), ("tiny", "f16", 3, 37, 9, 1)])
def test_workspace_plan_is_eulers_plus_the_weight_words(cfgname, prec, B, N, nt, steps):
    assert E.METHODS == dict(euler=0, midpoint=1, rk4=2, ab2=3, ab3=4)
    lib = E.load_library()
    h = _handle(lib, TINY if cfgname == "tiny" else DiTConfig(), prec)
    pad = lambda n: (n + 255) // 256 * 256                           # noqa: E731  (the plan's allocation granule)
    try:
        for fn, extra, per_row in QUERIES:
            def size(method):
                v = C.c_size_t()
                assert getattr(lib, fn)(h, B, N, nt, steps, method, *extra, C.byref(v)) == 0, lib.f5_last_error()
                return v.value

            words = 3 * max(steps - 1, 1) * (B if per_row else 1)
            for m in (3, 4):
                assert size(m) == size(0) + pad(words * 4), (fn, m)                  # one evaluation per step, and the weight triples
            for m in (5, 7, 9, -1, 100):
                v = C.c_size_t()
                assert getattr(lib, fn)(h, B, N, nt, steps, m, *extra, C.byref(v)) != 0, (fn, m)
                assert lib.f5_last_error().decode() == f"Unknown method: {m}", (fn, m)
    finally:
        lib.f5_engine_destroy(h)


# ---- names on their way down -----------------------------------------------------------------------------------------------------------
def test_method_names_reach_every_layer():
    text = torch.zeros((2, 4), dtype=torch.int32)
    for m in ("ab2", "ab3"):
        out = prepare_lengths(text, 6, 2, 20, None, 4096, m)
        assert out[3] == 20
        assert G.parse_args(["--text", "x", "--method", m]).method == m
    with pytest.raises(ValueError, match="Unknown method: heun"):
        prepare_lengths(text, 6, 2, 20, None, 4096, "heun")
    with pytest.raises(ValueError, match="Unknown method: ab4"):
        prepare_lengths(text, 6, 2, 20, None, 4096, "ab4")
    with pytest.raises(SystemExit):
        G.parse_args(["--text", "x", "--method", "ab4"])


def test_f5tts_sample_and_generate_many_pass_the_name_on(monkeypatch, tmp_path):
    import test_multivoice_host as MV
    import test_row_controls_host as RH
    f5, eng, _ = RH._f5(monkeypatch)
    cond, text = torch.zeros((3, 6, 100)), torch.zeros((3, 4), dtype=torch.int32)
    f5.sample(cond, text, duration=20, steps=6, method="ab3", cfg_strength=[0.5, 0.0, 2.0], seed=1)
    assert eng.calls[0]["kw"]["method"] == "ab3"
    # generate_many: the solver is one per call, beside per-request controls
    monkeypatch.setattr(G._audio, "prepare_references", lambda waves, rates, **kw: MV._refs((5 * 256 + 5, 2 * 256)[:len(waves)]))
    wav = str(tmp_path / "ref16k.wav")
    G.write_wav(wav, np.zeros(1600, np.float32), 16_000)
    stub = MV._Stub(lambda mel, lens: mel[:, :-1, 0].repeat_interleave(256, dim=1))
    G.generate_many([("Hello there. How are you? Fine", None, None), ("no punctuation here", wav, "the other voice.")], steps=6, method="ab2",
                    seed=3, estimate_duration=True, f5tts=stub, controls=[dict(cfg_strength=0.5), None])
    assert stub.calls[0]["kw"]["method"] == "ab2" and stub.calls[0]["kw"]["cfg_strength"] == [0.5, 0.5, 2.0]
    with pytest.raises(ValueError, match=r"unknown control\(s\) \['method'\]"):
        G.generate_many([("Hello.", None, None)], f5tts=MV._Stub(lambda mel: mel), controls=[dict(method="ab2")])
