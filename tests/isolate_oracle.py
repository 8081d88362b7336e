"""Row-isolated restatement of the DiT for a padded batch (docs/isolate_rows.md), and the inputs the isolate_rows tests share.

`IsolatedDiTOracle` is the plain oracle with the three places changed through which a row of a padded batch reads its own padding:
  * both conv-pos convolutions read rows n >= dur[b] as zero,
  * the GRN norm of each text ConvNeXt block runs over the row's own dur[b] positions,
  * the block's depthwise convolution reads zero past dur[b].
Attention needs nothing: the key-padding mask of a batch already keeps the padding out.  The lengths are those of the mask the call
carries (`sample()` builds it from the durations for every batch above one row); without a mask nothing is padded and nothing changes.
`without` leaves one of the three as the plain oracle has it ("grn", "convpos", "dwconv"): what the tests use to show that each piece
is visible on its own.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

from f5test import O, TINY, synth_inputs, synthetic_weights

DURATIONS = (128, 37, 70)
SOLVER = dict(steps=4, method="rk4", cfg_strength=2.0, sway_sampling_coef=-1.0)


class IsolatedDiTOracle(O.DiTOracle):
    def __init__(self, *args, without: str = "", **kw):
        super().__init__(*args, **kw)
        assert without in ("", "grn", "convpos", "dwconv"), without
        self.without = without
        self._valid = None                      # (b, n, 1) bool of the forward in flight, None = no padding

    def forward(self, x, cond, text, time, drop_audio_cond, drop_text, mask=None, return_hidden=False):
        self._valid = None if mask is None else mask[:, :, None]
        try:
            return super().forward(x, cond, text, time, drop_audio_cond, drop_text, mask, return_hidden)
        finally:
            self._valid = None

    def _zero_pad(self, x, piece: str):
        if self._valid is None or self.without == piece:
            return x
        return torch.where(self._valid, x, torch.zeros_like(x))

    def convnext_block(self, x, i):
        p = f"transformer.text_embed.text_blocks.layers.{i}."
        residual = x
        x = self.conv1d_cl(self._zero_pad(x, "dwconv"), p + "dwconv", groups=self.cfg.text_dim, padding=3, lowp=False)
        x = self.layer_norm(x, self.w[p + "norm.weight"], self.w[p + "norm.bias"], eps=1e-6)
        x = self.linear(x, p + "pwconv1")
        x = O._gelu_erf(x)
        gx = torch.linalg.vector_norm(self._zero_pad(x, "grn"), ord=2, dim=1, keepdim=True)     # over the row's own positions
        nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
        x = self.w[p + "grn.gamma"] * (x * nx) + self.w[p + "grn.beta"] + x
        x = self.linear(x, p + "pwconv2")
        return residual + x

    def conv_pos_embed(self, x):
        k, g = self.cfg.conv_pos_kernel, self.cfg.conv_pos_groups
        p = "transformer.input_embed.conv_pos_embed.conv1d.layers."
        x = O._mish(self.conv1d_cl(self._zero_pad(x, "convpos"), p + "0", groups=g, padding=k // 2, lowp=True))
        x = O._mish(self.conv1d_cl(self._zero_pad(x, "convpos"), p + "2", groups=g, padding=k // 2, lowp=True))
        return x


def config(text_mask_padding: bool = True):
    """TINY, or TINY with the text mask off (dit.py:186): the padding of the text path is then not even zeroed between the blocks."""
    if text_mask_padding:
        return TINY
    import dataclasses
    return dataclasses.replace(TINY, text_mask_padding=False)


@lru_cache(maxsize=None)
def weights():
    return synthetic_weights(TINY, 42)


@lru_cache(maxsize=None)
def inputs():
    """The ragged batch of the issue: three rows padded to 128 frames, durations 128 / 37 / 70, y0 zero past each duration."""
    cond, text, _, y0 = synth_inputs(TINY, 3, 128, nt=12, n_ref=16, seed=5, ragged=True)
    y0 = y0.clone()
    for b, d in enumerate(DURATIONS):
        y0[b, d:] = 0
    return cond, text, list(DURATIONS), y0


def generated(out, b: int, n_ref: int = 16) -> torch.Tensor:
    """the generated frames of row b of a batched result (b, n, d), or of a solo result (1, dur, d) with b = 0 and the slice given"""
    return out[b, n_ref:DURATIONS[b]]


@lru_cache(maxsize=None)
def solo_reference(text_mask_padding: bool = True):
    """The plain oracle's solo sample() of every row: B = 1, N = dur[b], the row's own y0[:dur].  Computed once per configuration and
    shared; callers must not write into it.  -> a list of (dur[b], mel) tensors."""
    cond, text, durs, y0 = inputs()
    dit = O.DiTOracle(config(text_mask_padding), weights())
    rows = []
    for b, d in enumerate(durs):
        out, _ = O.sample(dit, cond[b:b + 1], text[b:b + 1], torch.tensor([d]), y0=y0[b:b + 1, :d], **SOLVER)
        rows.append(out[0])
    return rows


def row_distance(out, solo_rows, b: int, n_ref: int = 16) -> float:
    """mean |batched row - the same row sampled solo| over the generated frames"""
    a = torch.as_tensor(out)[b, n_ref:DURATIONS[b]].detach().cpu().double()
    return float((a - solo_rows[b][n_ref:DURATIONS[b]].double()).abs().mean())


def batched(dit, text_mask_padding: bool = True):
    cond, text, durs, y0 = inputs()
    out, _ = O.sample(dit, cond, text, torch.tensor(durs), y0=y0, **SOLVER)
    return out
