"""Row-isolated duration prediction (docs/duration_rows.md): the inputs the tests share, the per-row solo reference, and
`predict_isolated`, the padded-batch predictor restated in fp64 with the four rules of the mode.

Row b of a padded call has lens[b] mel frames and tokens[b] text ids (one past its last id >= 0); its row length is
L[b] = max(lens[b], tokens[b]), the N a call of that row alone runs at (duration.py:218-220).  In the isolated mode row b reads nothing
from its own positions n >= L[b]:
  conv     the depthwise conv of each text ConvNeXt block leaves taps at n >= L[b] out,
  grn      the block's GRN norms over the row's L[b] positions,
  convpos  both conv-pos convolutions see zeros at n >= L[b],
  keys     every attention gets the key mask n < L[b];
the head's mean stays over n < lens[b].  `without=` leaves one of the four as the plain predictor has it.
"""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from f5test import O
from f5_tts_mlx_amd.duration import synthetic_duration_weights
from oracle import duration_oracle as DO

MODELS = {512: dict(dim=512, depth=3, heads=8), 1024: dict(dim=1024, depth=1, heads=16)}
CASES = {           # name: (dim, n_in, nt, lens, tokens); row 0 is the longest of every case: L[0] = N = max(n_in, nt)
    "mel_longer": (512, 130, 40, (130, 64, 9), (40, 22, 12)),
    "text_longer": (512, 64, 80, (64, 33, 20), (80, 41, 30)),
    "tile_edges": (512, 129, 24, (129, 65, 63, 4), (24, 10, 7, 3)),
    "dim1024": (1024, 72, 20, (72, 40), (20, 9)),
}
RULES = ("conv", "grn", "convpos", "keys")
FRAME_RATE = 93


@lru_cache(maxsize=None)
def weights(dim):
    return synthetic_duration_weights(seed=5, dim=dim, depth=MODELS[dim]["depth"], text_num_embeds=70, text_dim=512, conv_layers=2, ff_mult=2)


def make_inputs(B, n_in, nt, tokens, seed):
    r = np.random.default_rng(seed)
    mel = torch.from_numpy((r.standard_normal((B, n_in, 100)) * 1.5 - 1.0).astype(np.float32))
    text = torch.from_numpy(r.integers(0, 70, (B, nt)).astype(np.int32))
    for b, t in enumerate(tokens):
        text[b, t:] = -1
    return mel, text


@lru_cache(maxsize=None)
def inputs(case):
    """(mel (B, n_in, 100) fp32, text (B, nt) int32 with -1 behind each row's tokens, lens (B,)); shared: callers must not write"""
    _, n_in, nt, lens, tokens = CASES[case]
    B = len(lens)
    mel, text = make_inputs(B, n_in, nt, tokens, seed=B + n_in)
    return mel, text, torch.tensor(lens)


def row_len(case):
    _, _, _, lens, tokens = CASES[case]
    return [max(a, b) for a, b in zip(lens, tokens)]


def model_kw(case):
    m = MODELS[CASES[case][0]]
    return dict(dim=m["dim"], depth=m["depth"], heads=m["heads"])


@lru_cache(maxsize=None)
def solo(case, emulate_bf16=False):
    """seconds (B,) fp64: every row predicted alone on its own lens[b] frames and tokens[b] ids.  Shared: callers must not write."""
    dim, _, _, lens, tokens = CASES[case]
    mel, text, _ = inputs(case)
    rows = [DO.predict(weights(dim), mel[b:b + 1, :lens[b]], text[b:b + 1, :tokens[b]], lens=torch.tensor([lens[b]]),
                       dtype=torch.float64, emulate_bf16=emulate_bf16, **model_kw(case))[0] for b in range(len(lens))]
    return torch.stack(rows)


@lru_cache(maxsize=None)
def padded(case, emulate_bf16=False):
    """the plain predictor on the padded batch: what a row gets next to its batch-mates without the mode"""
    mel, text, lens = inputs(case)
    return DO.predict(weights(CASES[case][0]), mel, text, lens=lens, dtype=torch.float64, emulate_bf16=emulate_bf16, **model_kw(case))


def rel(got, ref):
    """per-row |got - ref| relative to max(1, mean |ref|): the scale of the project's predictor bounds"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
    return ((got - ref).abs() / max(1.0, float(ref.abs().mean()))).tolist()


def frames(seconds):
    """(int(seconds * 93), fractional part) per row"""
    x = torch.as_tensor(seconds).double() * FRAME_RATE
    return [int(v) for v in x.tolist()], [float(v - int(v)) for v in x.tolist()]


class _IsolatedOracle(O.DiTOracle):
    """DiTOracle's text block and conv-pos with a row's positions n >= L[b] kept out (valid: (b, n, 1) bool)"""

    def __init__(self, *args, valid, without="", **kw):
        super().__init__(*args, **kw)
        self.valid, self.without = valid, without

    def _own(self, x, rule):
        return x if self.without == rule else torch.where(self.valid, x, torch.zeros_like(x))

    def convnext_block(self, x, i):
        p = f"transformer.text_embed.text_blocks.layers.{i}."
        residual = x
        x = self.conv1d_cl(self._own(x, "conv"), p + "dwconv", groups=self.cfg.text_dim, padding=3, lowp=False)
        x = self.layer_norm(x, self.w[p + "norm.weight"], self.w[p + "norm.bias"], eps=1e-6)
        x = O._gelu_erf(self.linear(x, p + "pwconv1"))
        gx = torch.linalg.vector_norm(self._own(x, "grn"), ord=2, dim=1, keepdim=True)
        nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
        x = self.w[p + "grn.gamma"] * (x * nx) + self.w[p + "grn.beta"] + x
        return residual + self.linear(x, p + "pwconv2")

    def conv_pos_embed(self, x):
        k, g = self.cfg.conv_pos_kernel, self.cfg.conv_pos_groups
        p = "transformer.input_embed.conv_pos_embed.conv1d.layers."
        x = O._mish(self.conv1d_cl(self._own(x, "convpos"), p + "0", groups=g, padding=k // 2, lowp=True))
        return O._mish(self.conv1d_cl(self._own(x, "convpos"), p + "2", groups=g, padding=k // 2, lowp=True))


def predict_isolated(weights, inp, text, lens, tokens, dim=512, depth=8, heads=8, text_dim=512, conv_layers=2, without="",
                     dtype=torch.float64, emulate_bf16=False):
    """oracle/duration_oracle.py `predict` on the padded batch with the four rules; inp (b, n_in, mel), text (b, nt), lens / tokens (b,)
    -> seconds (b,).  What the rules leave at positions n >= L[b] is never read by a later stage of the same row."""
    assert without in ("",) + RULES, without
    inp = inp.to(dtype)
    batch, seq_len = inp.shape[:2]
    if seq_len < text.shape[1]:
        inp = F.pad(inp, (0, 0, 0, text.shape[1] - seq_len))
        seq_len = text.shape[1]
    lens = torch.as_tensor(lens)
    rowlen = torch.maximum(lens, torch.as_tensor(tokens))
    mask = O.lens_to_mask(lens, seq_len)
    own = O.lens_to_mask(rowlen, seq_len)                                 # (b, n): n < L[b]
    cfg = SimpleNamespace(dim=dim, depth=depth, heads=heads, dim_head=64, mel_dim=inp.shape[-1], text_dim=text_dim,
                          conv_layers=conv_layers, conv_pos_kernel=31, conv_pos_groups=16, freq_embed_dim=256, text_max_pos=4096)
    orc = _IsolatedOracle(cfg, weights, dtype=dtype, emulate_bf16=emulate_bf16, valid=own[..., None], without=without)
    inp = torch.where(mask[..., None], inp, torch.zeros_like(inp))
    t = text.to(torch.int64) + 1
    t = F.pad(t[:, :seq_len], (0, seq_len - text.shape[1]), value=0)
    te = orc.w["transformer.text_embed.text_embed.weight"][t] + orc.freqs_cis[:seq_len][None]
    for i in range(conv_layers):
        te = orc.convnext_block(te, i)
    x = orc.linear(torch.cat((inp, te), dim=-1), "transformer.input_embed.proj")
    x = orc.conv_pos_embed(x) + x
    rope = O.rotary_freqs(64, seq_len)
    keys = None if without == "keys" else own
    for i in range(depth):
        p = f"transformer.transformer_blocks.{i}."
        x = x + orc.attention(orc.layer_norm(x), i, keys, rope)          # (the oracle also zeroes the masked QUERY rows: never read)
        h = O._gelu_tanh(orc.linear(orc.layer_norm(x), p + "ff.ff.layers.0.layers.0"))
        x = x + orc.linear(h, p + "ff.ff.layers.2")
    g = orc.w["transformer.norm_out.weight"]
    x = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + 1e-5) * g
    m = mask[..., None]
    mean = torch.where(m, x, torch.zeros_like(x)).sum(dim=1) / torch.clamp(m.sum(dim=1).to(dtype), min=1)
    return F.softplus(mean @ orc.w["to_pred.layers.0.weight"].T)[:, 0]
