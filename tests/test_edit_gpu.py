"""Speech editing on the GPU: the keep-mask twins of pack_cond_text / splice and the frame gather (bit-exact, both operand types,
guarded buffers, NaN planted in every dropped conditioning frame), the waveform patch (interiors bitwise, fades within the bound of
their two fp32 roundings), f5_sample_edit against f5_sample (prefix mask: the same bits) and against a construction from the oracle's
own pieces (interior spans), the graph cache, the split and bf16x3 routes, and edit_speech end to end on synthetic weights."""
import ctypes as C
import pkgutil

import numpy as np
import pytest
import torch

from f5test import DEV, E, O, P, TINY, operand_mode, op_dtype, report, split_bf16, stream, synth_inputs, synthetic_weights
from f5_tts_mlx_amd import edit as ED
from f5_tts_mlx_amd.cfm import F5TTS
from f5_tts_mlx_amd.dit import DiT

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-3                  # the project's gate (tests/test_model_gpu.py)
U = 2.0 ** -24                     # unit roundoff of fp32
INT32_MAX = 2 ** 31 - 1
DT = 256


# ---- guarded buffers: the payload sits between two runs of a sentinel that must come back untouched ---------------------------------
class Guarded:
    def __init__(self, shape, dtype, guard=64, fill=None):
        self.n = int(np.prod(shape))
        self.g = guard
        self.shape = tuple(shape)
        if dtype.is_floating_point:
            self.sent = torch.full((1,), -12345.0, dtype=dtype)
        else:
            self.sent = torch.full((1,), 0x5A, dtype=dtype)
        self.buf = self.sent.repeat(self.n + 2 * guard).to(DEV)
        if fill is not None:
            self.view().copy_(fill.to(DEV).reshape(self.shape))

    def view(self):
        return self.buf[self.g:self.g + self.n].view(self.shape)

    def intact(self):
        s = self.sent.to(DEV)
        return bool((self.buf[:self.g] == s).all()) and bool((self.buf[self.g + self.n:] == s).all())


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _masks(r, B, N):
    first, last = torch.zeros((B, N), dtype=torch.bool), torch.zeros((B, N), dtype=torch.bool)
    first[:, 0], last[:, N - 1] = True, True
    return dict(random=torch.from_numpy(r.random((B, N)) < 0.5), zeros=torch.zeros((B, N), dtype=torch.bool),
                ones=torch.ones((B, N), dtype=torch.bool), first=first, last=last)


# ---- the three row ops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mel", [1, 100, 128])
@pytest.mark.parametrize("N", [4, 5, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_keep_ops_bit_exact(B, N, mel):
    lib = E.load_library()
    r = np.random.default_rng(1000 * B + 10 * N + mel)
    cond = torch.from_numpy(r.standard_normal((B, N, mel)).astype(np.float32))
    y = torch.from_numpy(r.standard_normal((B, N, mel)).astype(np.float32))
    te = torch.from_numpy(r.standard_normal((2, B, N, DT)).astype(np.float32))
    ld = 128 + DT
    clean = cond.to(DEV)                                     # (device inputs are held in names: a temporary would be freed before the launch)
    for prec in ("bf16", "f16"):
        with operand_mode(prec):
            for mname, keep in _masks(r, B, N).items():
                k3 = keep[..., None]
                poisoned = torch.where(k3, cond, torch.full_like(cond, float("nan")))        # NaN in EVERY dropped conditioning frame
                d_cond, d_keep, d_y, d_te = poisoned.to(DEV), keep.to(torch.uint8).to(DEV), y.to(DEV), te.to(DEV)
                masked = torch.where(k3, cond, torch.zeros_like(cond))
                for nkc in (0, 1):
                    v = torch.zeros((2, B, N, ld))
                    v[..., 128:] = te
                    v[0, ..., :mel] = masked
                    if nkc:
                        v[1, ..., :mel] = masked
                    w_hi, w_lo = split_bf16(v)
                    hi, lo = Guarded((2, B, N, ld), op_dtype()), Guarded((2, B, N, ld), op_dtype())
                    rc = lib.f5_op_pack_cond_text_keep(P(d_cond), P(d_keep), P(d_te), P(hi.view()), P(lo.view()), B, N, mel, DT, nkc, stream())
                    E.check(rc, "f5_op_pack_cond_text_keep")
                    torch.cuda.synchronize()
                    tag = (prec, mname, nkc)
                    assert hi.intact() and lo.intact(), tag
                    assert torch.isfinite(hi.view().float()).all() and torch.isfinite(lo.view().float()).all(), tag
                    assert torch.equal(_bits(hi.view()).cpu(), _bits(w_hi)) and torch.equal(_bits(lo.view()).cpu(), _bits(w_lo)), tag
                    # the edge masks are the old kernel's lens = 0 / lens = N, bit for bit
                    if mname in ("zeros", "ones"):
                        lens = torch.full((B,), 0 if mname == "zeros" else N, dtype=torch.int32, device=DEV)
                        o_hi, o_lo = torch.empty_like(hi.view()), torch.empty_like(lo.view())
                        E.check(lib.f5_op_pack_cond_text(P(clean), P(lens), P(d_te), P(o_hi), P(o_lo), B, N, mel, DT, nkc, stream()), "pack_cond_text")
                        torch.cuda.synchronize()
                        assert torch.equal(_bits(o_hi), _bits(hi.view())) and torch.equal(_bits(o_lo), _bits(lo.view())), tag
                # splice: out = keep ? cond : y
                out = Guarded((B, N, mel), torch.float32)
                E.check(lib.f5_op_splice_keep(P(d_cond), P(d_y), P(d_keep), P(out.view()), B, N, mel, stream()), "f5_op_splice_keep")
                torch.cuda.synchronize()
                assert out.intact() and torch.isfinite(out.view()).all(), (prec, mname)
                assert torch.equal(_bits(out.view()).cpu(), _bits(torch.where(k3, cond, y))), (prec, mname)
                if mname in ("zeros", "ones"):
                    old = torch.empty((B, N, mel), device=DEV)
                    E.check(lib.f5_op_splice(P(clean), P(d_y), P(lens), P(old), B, N, mel, stream()), "f5_op_splice")
                    torch.cuda.synchronize()
                    assert torch.equal(old, out.view()), (prec, mname)
            # and a NaN on the OTHER side of the splice (y under a kept frame) stays out as well
            keep = _masks(r, B, N)["random"]
            ynan = torch.where(keep[..., None], torch.full_like(y, float("nan")), y).to(DEV)
            d_keep = keep.to(torch.uint8).to(DEV)
            got = torch.empty((B, N, mel), device=DEV)
            E.check(lib.f5_op_splice_keep(P(clean), P(ynan), P(d_keep), P(got), B, N, mel, stream()), "f5_op_splice_keep")
            torch.cuda.synchronize()
            assert torch.equal(got.cpu(), torch.where(keep[..., None], cond, y))


@pytest.mark.parametrize("mel", [1, 100, 128])
@pytest.mark.parametrize("N", [4, 5, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_gather_frames_bit_exact(B, N, mel):
    lib = E.load_library()
    r = np.random.default_rng(7000 + 1000 * B + 10 * N + mel)
    n_src = 9
    src = torch.from_numpy(r.standard_normal((B, n_src, mel)).astype(np.float32))
    idx = torch.from_numpy(r.integers(0, n_src, (B, N)).astype(np.int32))
    special = [-1, n_src, INT32_MAX, -INT32_MAX - 1, n_src - 1, 0, -2, n_src + 1]         # the first four are in every case (N >= 4)
    for b in range(B):
        pos = r.permutation(N)[:min(N, len(special))]
        for p, v in zip(pos, special):
            idx[b, p] = v
    assert all(v in idx.tolist()[0] for v in (-1, n_src, INT32_MAX))
    # the source sits between NaN guards: an index that slipped past the range test would bring a NaN (or a neighbour row) along
    g_src = Guarded((B, n_src, mel), torch.float32, guard=4 * mel, fill=src)
    g_src.buf[:g_src.g] = float("nan")
    g_src.buf[g_src.g + g_src.n:] = float("nan")
    cond, keep = Guarded((B, N, mel), torch.float32), Guarded((B, N), torch.uint8)
    d_idx = idx.to(DEV)
    E.check(lib.f5_op_gather_frames(P(g_src.view()), P(d_idx), P(cond.view()), P(keep.view()), B, n_src, N, mel, stream()),
            "f5_op_gather_frames")
    torch.cuda.synchronize()
    valid = (idx >= 0) & (idx < n_src)
    want = torch.stack([src[b].index_select(0, idx[b].clamp(0, n_src - 1).to(torch.int64)) for b in range(B)])
    want = torch.where(valid[..., None], want, torch.zeros_like(want))
    assert cond.intact() and keep.intact()
    assert torch.equal(_bits(cond.view()).cpu(), _bits(want))                               # (bits: a dropped frame is +0.0)
    assert torch.equal(keep.view().cpu(), valid.to(torch.uint8))
    # the Python wrapper is the same call
    c2, k2 = ED.gather_frames(src.to(DEV), idx)
    assert torch.equal(c2, cond.view()) and torch.equal(k2, keep.view())


# ---- the waveform patch --------------------------------------------------------------------------------------------------------------
def _patch_tables(F):
    """four ragged rows, S = 5 (rows with fewer segments pad with empty ones); m = the shortest kept segment each position allows"""
    m1, m2 = max(F, 1), max(2 * F, 1)
    rows = [
        # regenerated | kept of EXACTLY 2 F (a regenerated segment on both sides) | regenerated | kept, long | (pad)
        [(0, 300, -1), (300, 300 + m2, 40), (300 + m2, 900 + m2, -1), (900 + m2, 1500 + m2, 700), (1500 + m2, 1500 + m2, -1)],
        # kept from sample 0 (fade-out only) | regenerated | kept of EXACTLY F, last real segment (fade-in only) | (pads); zeros follow
        [(0, 400 + m1, 0), (400 + m1, 777 + m1, -1), (777 + m1, 777 + 2 * m1, 1200), (777 + 2 * m1, 777 + 2 * m1, 5), (777 + 2 * m1, 777 + 2 * m1, 5)],
        # an EMPTY regenerated segment between two kept ones (a cut): both neighbours fade at the seam
        [(0, 500, 100), (500, 500, -1), (500, 1100, 900), (1100, 1300, -1), (1300, 1300, -1)],
        # a row without audio: every segment empty, the whole row is zeros
        [(0, 0, -1)] * 5,
    ]
    return np.asarray(rows, dtype=np.int32)


def _patch_reference(gen, src, segs, fade, F):
    """fp64 restatement: (value, kind) per sample; kind 0 = zero tail, 1 = gen, 2 = source, 3 = fade"""
    B, L = gen.shape
    val, kind = np.zeros((B, L)), np.zeros((B, L), dtype=np.int8)
    g64, s64, f64 = gen.astype(np.float64), src.astype(np.float64), fade.astype(np.float64)
    for b in range(B):
        S = len(segs[b])
        for k, (d0, d1, s0) in enumerate(segs[b].tolist()):
            for s in range(d0, d1):
                if s0 < 0:
                    val[b, s], kind[b, s] = g64[b, s], 1
                    continue
                o, g = s64[b, s0 + s - d0], g64[b, s]
                i0, i1 = s - d0, d1 - 1 - s
                if i0 < F and k > 0 and segs[b][k - 1][2] < 0:
                    val[b, s], kind[b, s] = g + f64[i0] * (o - g), 3
                elif i1 < F and k + 1 < S and segs[b][k + 1][2] < 0:
                    val[b, s], kind[b, s] = g + f64[i1] * (o - g), 3
                else:
                    val[b, s], kind[b, s] = o, 2
    return val, kind


def _run_patch(segs, F, L, Ls, seed):
    r = np.random.default_rng(seed)
    B = segs.shape[0]
    gen = r.standard_normal((B, L)).astype(np.float32)
    src = r.standard_normal((B, Ls)).astype(np.float32)
    fade = ED.fade_table(F)
    d_gen, d_src = torch.from_numpy(gen).to(DEV), torch.from_numpy(src).to(DEV)
    out = Guarded((B, L), torch.float32, guard=512)
    d_fade = torch.from_numpy(fade.copy()).to(DEV) if F else None
    rc = E.load_library().f5_op_wave_patch(P(d_gen), P(d_src), segs.ctypes.data_as(C.c_void_p), P(d_fade), P(out.view()), B, L, Ls,
                                           segs.shape[1], F, stream())
    E.check(rc, "f5_op_wave_patch")
    torch.cuda.synchronize()
    assert out.intact()
    got = out.view().cpu().numpy()
    val, kind = _patch_reference(gen, src, segs, fade, F)
    exact = kind != 3
    # kept interiors are the source's bits, regenerated interiors gen's bits, the tail +0.0
    assert np.array_equal(got[exact].view(np.int32), val[exact].astype(np.float32).view(np.int32))
    assert (got[kind == 0].view(np.int32) == 0).all()
    # fades: out = fma(f, fl(o - g), g).  fl(o - g) = (o - g)(1 + e1), the fma rounds once: out = (g + f (o - g)(1 + e1))(1 + e2) with
    # |e1|, |e2| <= u, so |out - ref| <= u f |o - g| (1 + u) + u |ref|
    if F:
        n_f = int((kind == 3).sum())
        assert n_f > 0
        for b in range(B):
            for k, (d0, d1, s0) in enumerate(segs[b].tolist()):
                if s0 < 0:
                    continue
                for s in range(d0, d1):
                    if kind[b, s] != 3:
                        continue
                    o, g = float(src[b, s0 + s - d0]), float(gen[b, s])
                    i = s - d0 if (s - d0 < F and k > 0 and segs[b][k - 1][2] < 0) else d1 - 1 - s
                    bound = U * float(fade[i]) * abs(o - g) * (1 + U) + U * abs(val[b, s])
                    assert abs(float(got[b, s]) - val[b, s]) <= bound, (b, s, got[b, s], val[b, s], bound)
    return got, kind


@pytest.mark.parametrize("F", [0, 1, 256])
def test_wave_patch(F):
    segs = _patch_tables(F)
    L = int(segs[:, :, 1].max()) + 333                       # every row ends before L: zeros follow, of different lengths
    got, kind = _run_patch(segs, F, L, 2100, seed=5 + F)
    assert (kind[3] == 0).all() and (got[3] == 0).all()
    assert (kind == 2).any() and (kind == 1).any() and (kind == 0).any()
    # the Python wrapper: the same call (and a table the library refuses is a ValueError)
    r = np.random.default_rng(5 + F)
    gen = torch.from_numpy(r.standard_normal((4, L)).astype(np.float32)).to(DEV)
    src = torch.from_numpy(r.standard_normal((4, 2100)).astype(np.float32)).to(DEV)
    assert np.array_equal(ED.wave_patch(gen, src, segs, F).cpu().numpy().view(np.int32), got.view(np.int32))
    bad = segs.copy()
    bad[0, 1, 0] += 1
    with pytest.raises(ValueError, match="sorted and contiguous"):
        ED.wave_patch(gen, src, bad, F)


def test_wave_patch_64_segments_two_launches():
    """S = 64 and 6 rows: the table travels in two kernel-argument blocks of 5 and 1 rows; row 5 must get ITS segments"""
    S, B, F = 64, 6, 1
    segs = np.zeros((B, S, 3), dtype=np.int32)
    for b in range(B):
        at = 0
        for k in range(S):
            n = (3 + (b + k) % 5) if k % 7 else 0                         # every 7th segment is empty
            segs[b, k] = (at, at + n, -1 if (n == 0 or (k + b) % 2) else 10 * b + k)     # (the empty ones are regenerated: cuts)
            at += n
    _run_patch(segs, F, int(segs[:, :, 1].max()) + 17, 1000, seed=9)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_weights():
    return synthetic_weights(TINY, seed=42)


def _model(weights, precision):
    m = DiT.from_config(TINY, precision=precision, device=DEV)
    m.load_weights(weights)
    return m


@pytest.fixture(scope="module")
def models(tiny_weights):
    return {p: _model(tiny_weights, p) for p in ("f16", "bf16x3")}


CONFIGS = [(1, "euler", 8), (2, "rk4", 4)]


@pytest.mark.parametrize("prec", ["f16", "bf16x3"])
@pytest.mark.parametrize("method,steps", [("euler", 8), ("rk4", 4)])
@pytest.mark.parametrize("B", [1, 2])
def test_prefix_identity(models, B, method, steps, prec):
    """keep[b][n] = n < lens[b] (an all-True edit_mask): f5_sample_edit returns f5_sample's out and trajectory bit for bit, eager and
    graph -- nothing else changed"""
    f5 = F5TTS(transformer=models[prec])
    cond, text, durations, y0 = synth_inputs(TINY, B, 96, nt=20, n_ref=33, seed=17 + B, ragged=B > 1)
    kw = dict(duration=torch.tensor(durations), y0=y0, steps=steps, method=method)
    for graph in (False, True):
        want, want_t = [x.clone() for x in f5.sample(cond, text, use_graph=graph, **kw)]
        got, got_t = f5.sample(cond, text, use_graph=graph, edit_mask=torch.ones((B, 33), dtype=torch.bool), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(got_t, want_t), (graph,)
        # a mask longer than the conditioning changes nothing either: lens_to_mask(lens) & mask
        got2, _ = f5.sample(cond, text, use_graph=graph, edit_mask=torch.ones((B, 96), dtype=torch.bool), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got2, want)


def _edit_keep(B, n_ref=60):
    keep = torch.ones((B, n_ref), dtype=torch.bool)
    keep[:, 20:35] = False                                   # frames 20 ... 34 dropped
    if B > 1:
        only = torch.zeros(n_ref, dtype=torch.bool)
        only[10:50] = True                                   # row 1 keeps only frames among 10 ... 49
        keep[1] &= only
    return keep


_oracle_cache = {}


def _oracle(weights, B, method, steps):
    """(inputs, keep, oracle edit out, oracle edit trajectory, oracle PREFIX out), computed once per configuration.  The edit result is
    built here from the oracle's own pieces: step_cond = where(keep, cond, 0), DiTOracle.forward for the two branches, odeint_* on
    time_grid, the final where."""
    key = (B, method, steps)
    if key not in _oracle_cache:
        N = 96
        cond, text, durations, y0 = synth_inputs(TINY, B, N, nt=20, n_ref=60, seed=17 + B, ragged=B > 1)
        keep = _edit_keep(B)
        dit = O.DiTOracle(TINY, weights)
        kw = dict(steps=steps, method=method, cfg_strength=2.0, sway_sampling_coef=-1.0)
        pre_out, _, aux = O.sample(dit, cond, text, torch.tensor(durations), y0=y0, return_aux=True, **kw)
        cond_p = torch.nn.functional.pad(cond, (0, 0, 0, N - cond.shape[1]))
        km = (torch.nn.functional.pad(keep, (0, N - keep.shape[1]), value=False) & aux["cond_mask"])[..., None]
        step_cond = torch.where(km, cond_p, torch.zeros_like(cond_p))
        mask = aux["mask"]

        def fn(t, x):
            pred = dit.forward(x, step_cond, aux["text"], t, False, False, mask)
            null = dit.forward(x, step_cond, aux["text"], t, True, True, mask)
            return pred + (pred - null) * 2.0

        solver = dict(euler=O.odeint_euler, midpoint=O.odeint_midpoint, rk4=O.odeint_rk4)[method]
        traj = solver(fn, y0, O.time_grid(steps, -1.0))
        out = torch.where(km, cond_p, traj[-1])
        _oracle_cache[key] = dict(cond=cond, text=text, durations=durations, y0=y0, keep=keep, km=km[..., 0], cond_p=cond_p, out=out,
                                  traj=traj, prefix=pre_out, kw=kw)
    return _oracle_cache[key]


@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
@pytest.mark.parametrize("B,method,steps", CONFIGS)
def test_interior_spans_against_oracle(tiny_weights, models, B, method, steps, prec):
    o = _oracle(tiny_weights, B, method, steps)
    f5 = F5TTS(transformer=models[prec])
    out, traj = f5.sample(o["cond"], o["text"], duration=torch.tensor(o["durations"]), y0=o["y0"], edit_mask=o["keep"], **o["kw"])
    torch.cuda.synchronize()
    out, traj = out.cpu(), traj.cpu()
    assert torch.isfinite(out).all()
    _, l1, _ = report(f"edit[{prec}] {method} B{B} final mel vs oracle edit", out, o["out"])
    _, l1t, _ = report(f"edit[{prec}] {method} B{B} trajectory vs oracle edit", traj, o["traj"])
    # the test can see a wrong mask: on the frames BOTH calls regenerate (n >= 60) the prefix result is far outside the gate
    far = float((out[:, 60:] - o["prefix"][:, 60:]).abs().mean())
    print(f"[edit] {prec} {method} B{B}: engine edit vs oracle PREFIX on frames n >= 60: {far:.3e} (gate {MEL_L1_TOL})")
    assert l1 <= MEL_L1_TOL and l1t <= MEL_L1_TOL
    assert torch.equal(out[o["km"]], o["cond_p"][o["km"]])                    # kept frames are cond, bit for bit
    assert int(o["km"].sum()) > 0 and not torch.equal(out[:, 20:35], o["cond_p"][:, 20:35])
    assert far > MEL_L1_TOL


def test_nan_in_dropped_frames_stays_out(tiny_weights, models):
    """NaN in every conditioning frame the mask drops, through the whole engine: the result is the clean call's, bit for bit"""
    o = _oracle(tiny_weights, 1, "euler", 8)
    f5 = F5TTS(transformer=models["f16"])
    kw = dict(duration=torch.tensor(o["durations"]), y0=o["y0"], edit_mask=o["keep"], **o["kw"])
    want, _ = f5.sample(o["cond"], o["text"], **kw)
    want = want.clone()
    dirty = torch.where(o["keep"][..., None], o["cond"], torch.full_like(o["cond"], float("nan")))
    got, _ = f5.sample(dirty, o["text"], **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_graph_cache_one_graph_serves_every_mask(tiny_weights):
    m = _model(tiny_weights, "f16")
    eng, f5 = m.engine, F5TTS(transformer=m)
    cond, text, durations, y0 = synth_inputs(TINY, 2, 96, nt=20, n_ref=60, seed=19, ragged=True)
    kw = dict(duration=torch.tensor(durations), y0=y0, steps=4, method="euler")
    mask_a, mask_b = _edit_keep(2), ~_edit_keep(2)
    eager = {k: [x.clone() for x in f5.sample(cond, text, use_graph=False, edit_mask=mk, **kw)] for k, mk in (("a", mask_a), ("b", mask_b))}
    plain = [x.clone() for x in f5.sample(cond, text, use_graph=False, **kw)]
    assert eng.graph_count() == 0
    assert not torch.equal(eager["a"][0], eager["b"][0]) and not torch.equal(eager["a"][0], plain[0])
    for rep in range(2):
        for k, mk in (("a", mask_a), ("b", mask_b)):
            out, traj = f5.sample(cond, text, use_graph=True, edit_mask=mk, **kw)
            torch.cuda.synchronize()
            assert eng.graph_count() == 1, (rep, k)                       # two masks of one shape replay one graph
            assert torch.equal(out, eager[k][0]) and torch.equal(traj, eager[k][1]), (rep, k)
    out, traj = f5.sample(cond, text, use_graph=True, **kw)               # a plain call of the same shape: its own entry, its own bits
    torch.cuda.synchronize()
    assert eng.graph_count() == 2
    assert torch.equal(out, plain[0]) and torch.equal(traj, plain[1])
    out, _ = f5.sample(cond, text, use_graph=True, edit_mask=mask_a, **kw)     # ... and the edit graph is still the edit graph
    torch.cuda.synchronize()
    assert eng.graph_count() == 2 and torch.equal(out, eager["a"][0])


def test_split_route_gives_each_half_its_rows(tiny_weights):
    """split_batch at B = 4, N = 67 (the second half's mask rows start at byte 134: not word aligned)"""
    m = _model(tiny_weights, "f16")
    eng, f5 = m.engine, F5TTS(transformer=m)
    cond, text, durations, y0 = synth_inputs(TINY, 4, 67, nt=12, n_ref=40, seed=23, ragged=True)
    keep = torch.from_numpy(np.random.default_rng(2).random((4, 40)) < 0.6)
    for graph in (False, True):
        kw = dict(duration=torch.tensor(durations), y0=y0, steps=4, method="euler", edit_mask=keep, use_graph=graph)
        eng.split_batch = 0
        want, want_t = [x.clone() for x in f5.sample(cond, text, **kw)]
        eng.split_batch = 4
        n0 = eng.split_events
        for rep in range(3):                                              # the first call of a shape runs the halves in turn
            out, traj = f5.sample(cond, text, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out, want) and torch.equal(traj, want_t), (graph, rep)
        assert eng.split_events == n0 + 3
    eng.split_batch = 0


def test_bf16x3_routes_honour_the_mask(tiny_weights, models):
    o = _oracle(tiny_weights, 1, "euler", 8)
    args = (o["cond"], o["text"])
    kw = dict(duration=torch.tensor(o["durations"]), y0=o["y0"], edit_mask=o["keep"], **o["kw"])
    x3, _ = F5TTS(transformer=models["bf16x3"]).sample(*args, **kw)
    x3 = x3.clone()
    # (1) the standing fall-back: an f16 engine that has been moved onto its bf16x3 twin
    m = _model(tiny_weights, "f16")
    assert m.engine._ensure_fallback() is not None
    m.engine._use_fallback = True
    out, _ = F5TTS(transformer=m).sample(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[o["km"]], o["cond_p"][o["km"]])
    l1 = float((out.cpu() - o["out"]).abs().mean())
    assert l1 <= MEL_L1_TOL and torch.equal(out, x3), l1
    # (2) the first-call cross-check: the bf16x3 twin runs the same mask, so the two agree inside the gate
    m = _model(tiny_weights, "f16")
    m.engine.verify_calls = 1
    out, _ = F5TTS(transformer=m).sample(*args, **kw)
    torch.cuda.synchronize()
    print(f"[edit] cross-check f16 vs bf16x3 with the mask: {m.engine.last_verify_l1:.3e}")
    assert m.engine.verify_events == 0 and m.engine.last_verify_l1 <= MEL_L1_TOL and not m.engine._use_fallback
    # (3) the re-run after a saturation flag: weights that saturate fp16 (tests/test_model_gpu.py) -- the caller gets the bf16x3 bits
    w = synthetic_weights(TINY, seed=42)
    r = np.random.default_rng(5)
    name = "transformer.transformer_blocks.1.ff.ff.layers.0.layers.0.weight"
    for row in r.integers(0, w[name].shape[0], 4):
        w[name][row] *= 3.0e6
    ref, _ = F5TTS(transformer=_model(w, "bf16x3")).sample(*args, **kw)
    m = _model(w, "f16")
    with pytest.warns(E.OperandRangeWarning, match="re-running it in bf16x3"):
        out, _ = F5TTS(transformer=m).sample(*args, **kw)
    torch.cuda.synchronize()
    assert m.engine.saturation_events == 1 and torch.equal(out, ref)
    assert torch.equal(out.cpu()[o["km"]], o["cond_p"][o["km"]])


# ---- edit_speech end to end ----------------------------------------------------------------------------------------------------------
def test_edit_speech_end_to_end(models):
    from f5_tts_mlx_amd import generate as G
    from f5_tts_mlx_amd.utils import convert_char_to_pinyin
    from f5_tts_mlx_amd.vocos import Vocos, synthetic_vocos_weights
    vocab = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz.,!?'ABCDEFGHIJKLMNOPQRSTUVWXYZ")}
    voc = Vocos(synthetic_vocos_weights(), precision="f16", device=DEV)
    f5 = F5TTS(transformer=models["f16"], vocab_char_map=vocab, vocoder=voc.decode)
    wav = pkgutil.get_data("f5_tts_mlx_amd", "assets/test_en_1_ref_short.wav")
    text = "some call me nature, others call me mother."
    spans = [(1.0, 1.5, 0.8), (3.0, 3.8, 0.5)]                              # one grows, one shrinks
    kw = dict(steps=4, method="euler", seed=5)
    got = ED.edit_speech(wav, text, spans, f5, **kw)
    again = ED.edit_speech(wav, text, spans, f5, **kw)
    raw = ED.edit_speech(wav, text, spans, f5, patch_wave=False, **kw)
    torch.cuda.synchronize()
    audio, sr = G.read_wav(wav)
    audio = torch.from_numpy(np.asarray(audio)).to(torch.float32)
    assert sr == 24000 and float(torch.sqrt(torch.mean(audio ** 2))) >= ED.TARGET_RMS      # no RMS gain: the scaled source is the source
    n_src = audio.shape[0] // 256
    frames = ED.spans_to_frames(spans, n_src)
    assert frames[0][2] > frames[0][1] - frames[0][0] and frames[1][2] < frames[1][1] - frames[1][0]
    src_idx, segs = ED.edit_layout(n_src, frames)
    N = len(src_idx)
    assert got.ndim == 1 and got.shape[0] == 256 * (N - 1) == raw.shape[0] and torch.isfinite(got).all()
    assert torch.equal(got, again)                                          # the same seed: the same bits
    # kept segments outside their fades: the source's samples, bit for bit
    g, a, F = got.cpu(), audio, 256
    n_kept = 0
    for k, (d0, d1, s0) in enumerate(segs.tolist()):
        lo = d0 + (F if k > 0 and segs[k - 1][2] < 0 else 0)
        hi = d1 - (F if k + 1 < len(segs) and segs[k + 1][2] < 0 else 0)
        if s0 < 0:
            assert torch.equal(g[d0:d1], raw.cpu()[d0:d1])                  # regenerated: the vocoded result as it is
            continue
        assert torch.equal(g[lo:hi].view(torch.int32), a[s0 + lo - d0:s0 + hi - d0].view(torch.int32)), k
        n_kept += hi - lo
    assert n_kept > 256 * 300 and len(segs) == 5
    # patch_wave=False: vocoder(sample(...)) on the same conditioning
    mel = f5._mel_spec(audio[None].to(DEV))
    cond, keep = ED.gather_frames(mel, src_idx[None])
    want, _ = f5.sample(cond, text=convert_char_to_pinyin([text]), duration=N, lens=torch.tensor([N - 1]), edit_mask=keep.to(torch.bool),
                        sway_sampling_coef=-1.0, cfg_strength=2.0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(raw, want.reshape(-1))
    assert not torch.equal(raw, got)
