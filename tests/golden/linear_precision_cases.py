"""Inputs and CPU restatements of the reduced linear precisions of the frame Q-former (``infv_vqf_set_linear_precision``), shared by
``tests/test_linear_precision_cpu.py`` (which checks the conditions the GPU tests rest on, on these very inputs) and
``tests/test_linear_precision_gpu.py``.  Pure numpy / torch on the CPU, regenerated from seeds, nothing stored.

mode 0: fp32 (the operand as it is); mode 1: split-bf16, ``hi = bf16(x)``, ``lo = bf16(x - hi)``, the product
``hi.hi + hi.lo + lo.hi``; mode 2: fp16, the operand rounded to nearest even.

Everything returned here is cached and shared: callers must not write into it."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden.frame_qformer_cases import LN_VISION_EPS
from tests.golden.softmax_tier_cases import ref64

MODES = {"fp32": 0, "split_bf16": 1, "fp16": 2}
UNIT_ROWS = 257                             # one x per K; the smaller M are its leading rows
UNIT_M = (1, 31, 128, 129, 257)
UNIT_K = (64, 128, 768, 3072)               # one k-tile, two k-tiles, the model's two depths
UNIT_N = ((1, 64), (3, 64), (1, 768))       # (n_lin, n_out): (3, 64) is N = 192 -- a tile across stacked segments, a partial N tile
UNIT_W_ROWS = 768                           # one w per K; a narrower case takes its leading rows
FLOOR = 2.0 ** -12                          # no fp16 operand is subnormal (what the f16 MFMA does with those is not measured)
EPI_SHAPE = (129, 128, 192)                 # M, K, N of the epilogue cases
LN_ATOL = 2e-6                              # the project's LayerNorm allowance: 1.7 x torch's own fp32 layer_norm error


def _floored(a: np.ndarray) -> np.ndarray:
    return np.where(np.abs(a) < FLOOR, np.where(a < 0, -FLOOR, FLOOR), a).astype(np.float32)


@functools.lru_cache(maxsize=None)
def unit_inputs(K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [257][K] = randn * (0.5 + rand per row), w [768][K] = 0.05 * randn, fp32, magnitudes below 2^-12 raised to 2^-12."""
    rng = np.random.default_rng(9100 + K)
    x = rng.standard_normal((UNIT_ROWS, K)) * (0.5 + rng.random((UNIT_ROWS, 1)))
    w = 0.05 * rng.standard_normal((UNIT_W_ROWS, K))
    return torch.from_numpy(_floored(x)), torch.from_numpy(_floored(w))


@functools.lru_cache(maxsize=None)
def epilogue_inputs() -> Dict[str, torch.Tensor]:
    """Bias [192], residual [129][192], LayerNorm gamma / beta [192] of the epilogue cases (x and w: ``unit_inputs(128)``)."""
    M, _, N = EPI_SHAPE
    g = torch.Generator().manual_seed(9200)
    return dict(bias=0.1 * torch.randn(N, generator=g), residual=torch.randn(M, N, generator=g),
                gamma=1.0 + 0.1 * torch.randn(N, generator=g), beta=0.1 * torch.randn(N, generator=g))


# ---------------------------------------------------------------------------------------------------- the restatements
def prepared(x: torch.Tensor, mode: int) -> Tuple[torch.Tensor, ...]:
    """The operand as the MFMA of ``mode`` reads it, in float64: (x,), (hi, lo) or (fp16(x),).  x goes through fp32 first."""
    x32 = x.to(torch.float32)
    if mode == 0:
        return (x.to(torch.float64),)
    if mode == 1:
        hi = x32.to(torch.bfloat16)
        lo = (x32 - hi.to(torch.float32)).to(torch.bfloat16)
        return hi.to(torch.float64), lo.to(torch.float64)
    if mode == 2:
        return (x32.to(torch.float16).to(torch.float64),)
    raise ValueError(mode)


def ref_linear(x: torch.Tensor, w: torch.Tensor, mode: int) -> torch.Tensor:
    """x [..., K] . w [N][K]^T: the float64 product of the prepared operands (mode 1: hi.hi + hi.lo + lo.hi)."""
    px, pw = prepared(x, mode), prepared(w, mode)
    if mode == 1:
        return px[0] @ pw[0].T + px[0] @ pw[1].T + px[1] @ pw[0].T
    return px[0] @ pw[0].T


def seq32(x: torch.Tensor, w: torch.Tensor, mode: int) -> torch.Tensor:
    """The same products accumulated sequentially in float32, k ascending; mode 1: per k the kernel's order lo.hi, hi.lo, hi.hi.
    (A product of two bf16 or two fp16 values is exact in fp32, so only the additions round.)"""
    # (k-major copies: step k reads one contiguous row of each operand; the product is exact, so a fused multiply-add rounds once,
    #  as the separate addition would)
    px = [p.to(torch.float32).T.contiguous() for p in prepared(x, mode)]
    pw = [p.to(torch.float32).T.contiguous() for p in prepared(w, mode)]
    pairs = ((1, 0), (0, 1), (0, 0)) if mode == 1 else ((0, 0),)
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(x.shape[1]):
        for a, b in pairs:
            acc.addcmul_(px[a][k][:, None], pw[b][k][None, :])
    return acc


@functools.lru_cache(maxsize=None)
def unit_ref(K: int, mode: int) -> torch.Tensor:
    """``ref_linear`` of ``unit_inputs(K)``: [257][768] float64."""
    return ref_linear(*unit_inputs(K), mode)


@functools.lru_cache(maxsize=None)
def unit_seq32(K: int, mode: int) -> torch.Tensor:
    """``seq32`` of ``unit_inputs(K)``: [257][768] float32."""
    return seq32(*unit_inputs(K), mode)


def epilogue64(acc: torch.Tensor, kind: str) -> torch.Tensor:
    """The float64 epilogue of the three cases on a [129][192] product: ``gelu`` (bias + GELU), ``ln`` (bias + residual +
    LayerNorm, eps 1e-12), ``stacked`` (three 64-wide biases: the same numbers as one 192-wide bias, read per segment)."""
    e = {k: v.to(torch.float64) for k, v in epilogue_inputs().items()}
    y = acc.to(torch.float64) + e["bias"]
    if kind == "gelu":
        return F.gelu(y)
    if kind == "ln":
        return F.layer_norm(y + e["residual"], (y.size(-1),), e["gamma"], e["beta"], 1e-12)
    if kind == "stacked":
        return y
    raise ValueError(kind)


def emu64(sd: dict, shape: dict, vision: torch.Tensor, ln: bool, mode: int, ctx_out: Optional[dict] = None) -> torch.Tensor:
    """``ref64`` with the eight query-side linears of every layer (self q / k / v, self output, cross query, cross output,
    intermediate_query, output_query) replaced by ``ref_linear``; the cross key / value linears and everything else stay exact.
    ``ctx_out``: a dict that receives the cross-attention context [F, Q, hidden] of every cross layer (what the context tap copies)."""
    w = {k: torch.from_numpy(np.asarray(v)).to(torch.float64) for k, v in sd.items()}
    H, Hd = shape["n_heads"], shape["hidden"]
    dh = Hd // H
    lin = lambda x, n: F.linear(x, w[n + ".weight"], w[n + ".bias"])
    qlin = lambda x, n: ref_linear(x, w[n + ".weight"], mode) + w[n + ".bias"]
    lnorm = lambda x, n, eps=1e-12: F.layer_norm(x, (x.size(-1),), w[n + ".weight"], w[n + ".bias"], eps)
    heads = lambda x: x.reshape(x.size(0), x.size(1), H, dh).permute(0, 2, 1, 3)

    def attend(q, k, v):
        p = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-1, -2)) / math.sqrt(dh), dim=-1)
        return torch.matmul(p, heads(v)).permute(0, 2, 1, 3).reshape(q.size(0), q.size(1), Hd)

    k = vision.detach().cpu().to(torch.float64)
    if ln:
        k = lnorm(k, "ln_vision", LN_VISION_EPS)
    h = lnorm(w["query_tokens"], "Qformer.bert.embeddings.LayerNorm").expand(k.size(0), -1, -1)
    for l in range(shape["n_layers"]):
        p = f"Qformer.bert.encoder.layer.{l}."
        a = p + "attention."
        h = lnorm(qlin(attend(qlin(h, a + "self.query"), qlin(h, a + "self.key"), qlin(h, a + "self.value")), a + "output.dense") + h,
                  a + "output.LayerNorm")
        if l % 2 == 0:
            x = p + "crossattention."
            ctx = attend(qlin(h, x + "self.query"), lin(k, x + "self.key"), lin(k, x + "self.value"))
            if ctx_out is not None:
                ctx_out[l] = ctx
            h = lnorm(qlin(ctx, x + "output.dense") + h, x + "output.LayerNorm")
        h = lnorm(qlin(F.gelu(qlin(h, p + "intermediate_query.dense")), p + "output_query.dense") + h, p + "output_query.LayerNorm")
    return h
