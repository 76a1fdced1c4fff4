"""Inputs and CPU restatements of the fp16 cross-attention of the frame Q-former (``infv_vqf_set_attention_precision``), shared by
``tests/test_attention_precision_cpu.py`` (which checks the conditions the GPU tests rest on, on these very inputs) and
``tests/test_attention_precision_gpu.py``.  Pure numpy / torch on the CPU, regenerated from seeds, nothing stored.

The arithmetic of attention mode 1, per frame and head (dh = 64), in float64 with the stated fp16 roundings (``h16``):

    x^  = h16(LN(x)) or h16(x)                        q~' = h16(32 * h16(q) . h16(Wk_h))          (32 = 2^8 / sqrt(64))
    s   = 2^-8 * q~' . x^^T;  p = softmax(s)          p'  = h16(2^10 * p)
    o'  = h16(2^-10 * p' . x^)                        ctx = o' . h16(Wv_h)^T + bv

Everything returned here is cached and shared: callers must not write into it."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden import linear_precision_cases as lc
from tests.golden.frame_qformer_cases import LN_VISION_EPS

ATTN_MODES = {"fp32": 0, "fp16": 1}
F16_TINY = 2.0 ** -14                      # the smallest normal fp16 magnitude
F16_MAX = 65504.0

# the attention alone: the SMALL handle's shape, and one with 96 score rows (a partial 64-row block) and five 64-deep k-tiles
UNIT_SHAPES = {"small": dict(n_heads=2, n_query=8, enc_width=128, hidden=128),
               "wide": dict(n_heads=3, n_query=32, enc_width=320, hidden=192)}
UNIT_TOKENS = (1, 5, 63, 64, 65, 127, 257, 320, 384, 512)  # 384: the first launch above 64 KB of LDS; 512: four key tiles a wave
UNIT_FRAMES = 3                             # F = 1 is the first frame of the same inputs


def h16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest fp16 value (ties to even; beyond 65504: inf), kept as float64."""
    return x.to(torch.float64).to(torch.float16).to(torch.float64)


def heads_of(x: torch.Tensor, H: int) -> torch.Tensor:
    return x.reshape(x.size(0), x.size(1), H, x.size(2) // H).permute(0, 2, 1, 3)


def attend64(q: torch.Tensor, k: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, bv: torch.Tensor, H: int) -> torch.Tensor:
    """The exact cross-attention context in float64: q [F, Q, hidden], tokens k [F, n, d] (normalised already) -> [F, Q, hidden].
    The key bias is constant along a softmax row and is left out."""
    dh = q.size(2) // H
    s = torch.matmul(heads_of(q, H), heads_of(F.linear(k, wk), H).transpose(-1, -2)) / math.sqrt(dh)
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, heads_of(F.linear(k, wv, bv), H)).permute(0, 2, 1, 3).reshape(q.shape)


def attend16(q: torch.Tensor, k: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, bv: torch.Tensor, H: int,
             stats: Optional[dict] = None) -> torch.Tensor:
    """Steps 1-6 of attention mode 1 on float64 inputs.  ``stats`` receives ``qt`` (q~'), ``pp`` (p'), ``xh`` (x^), ``oo`` (o')."""
    dh = q.size(2) // H
    assert dh == 64
    d = k.size(2)
    xh = h16(k)
    qt = h16(32.0 * torch.einsum("fhqc,hce->fhqe", heads_of(h16(q), H), h16(wk).reshape(H, dh, d)))
    s = torch.einsum("fhqe,fje->fhqj", qt, xh) / 256.0
    pp = h16(1024.0 * torch.softmax(s, dim=-1))
    oo = h16(torch.einsum("fhqj,fje->fhqe", pp, xh) / 1024.0)
    ctx = torch.einsum("fhqe,hce->fhqc", oo, h16(wv).reshape(H, dh, d)) + bv.reshape(H, dh)[None, :, None, :]
    if stats is not None:
        stats.update(qt=qt, pp=pp, xh=xh, oo=oo)
    return ctx.permute(0, 2, 1, 3).reshape(q.shape)


def subnormal_share(x: torch.Tensor) -> float:
    """Share of the non-zero entries of x whose magnitude is below fp16's smallest normal."""
    a = x.abs()
    nz = a > 0
    return float(((a < F16_TINY) & nz).sum()) / max(1, int(nz.sum()))


def emu64(sd: dict, shape: dict, vision: torch.Tensor, ln: bool, lin_mode: int, attn_mode: int, ctx_out: Optional[dict] = None,
          stats_out: Optional[dict] = None) -> torch.Tensor:
    """``linear_precision_cases.emu64`` with the cross-attention of every cross layer replaced by ``attend16`` when ``attn_mode`` is 1
    (the key and value linears of the tokens then never run: the mode pre-multiplies the query and projects the context).
    ``stats_out[l]`` receives that layer's ``attend16`` intermediates."""
    w = {k: torch.from_numpy(np.asarray(v)).to(torch.float64) for k, v in sd.items()}
    H, Hd = shape["n_heads"], shape["hidden"]
    dh = Hd // H
    lin = lambda x, n: F.linear(x, w[n + ".weight"], w[n + ".bias"])
    qlin = lambda x, n: lc.ref_linear(x, w[n + ".weight"], lin_mode) + w[n + ".bias"]
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
            if attn_mode:
                st = {} if stats_out is not None else None
                q = qlin(h, x + "self.query")
                ctx = attend16(q, k, w[x + "self.key.weight"], w[x + "self.value.weight"], w[x + "self.value.bias"], H, st)
                if stats_out is not None:
                    st.update(q=q, k=k)                   # the layer's own cross query and the (normalised) tokens it attends over
                    stats_out[l] = st
            else:
                ctx = attend(qlin(h, x + "self.query"), lin(k, x + "self.key"), lin(k, x + "self.value"))
            if ctx_out is not None:
                ctx_out[l] = ctx
            h = lnorm(qlin(ctx, x + "output.dense") + h, x + "output.LayerNorm")
        h = lnorm(qlin(F.gelu(qlin(h, p + "intermediate_query.dense")), p + "output_query.dense") + h, p + "output_query.LayerNorm")
    return h


# ---------------------------------------------------------------------------------------------------- the attention alone
@functools.lru_cache(maxsize=None)
def unit_inputs(shape_name: str, n_tokens: int) -> Dict[str, torch.Tensor]:
    """One cross layer's inputs, fp32: vision [3, n, d] (before the LayerNorm), gamma / beta [d], xq [3, Q, hidden], wk / wv
    [hidden, d], bk / bv [hidden].  The scores have a standard deviation of about 1 (width 128) to 1.5 (width 320): the softmax is
    not flat, and no probability comes near 2^-24, where p' would turn subnormal."""
    s = UNIT_SHAPES[shape_name]
    H, Q, d, Hd = s["n_heads"], s["n_query"], s["enc_width"], s["hidden"]
    g = torch.Generator().manual_seed(8800 + 1000 * sorted(UNIT_SHAPES).index(shape_name) + n_tokens)
    r = lambda *sz: torch.randn(*sz, generator=g)
    return dict(vision=r(UNIT_FRAMES, n_tokens, d) + 0.3, gamma=1.0 + 0.1 * r(d), beta=0.1 * r(d), xq=r(UNIT_FRAMES, Q, Hd),
                wk=0.08 * r(Hd, d), wv=0.05 * r(Hd, d), bk=0.02 * r(Hd), bv=0.02 * r(Hd))


def _unit_tokens(u: Dict[str, torch.Tensor], ln: bool, dtype) -> torch.Tensor:
    k = u["vision"].to(dtype)
    return F.layer_norm(k, (k.size(-1),), u["gamma"].to(dtype), u["beta"].to(dtype), LN_VISION_EPS) if ln else k


@functools.lru_cache(maxsize=None)
def unit_ref(shape_name: str, n_tokens: int, ln: bool, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The exact context [3, Q, hidden] of ``unit_inputs`` in ``dtype`` (float32: what fp32 alone costs)."""
    u = unit_inputs(shape_name, n_tokens)
    t = lambda n: u[n].to(dtype)
    return attend64(t("xq"), _unit_tokens(u, ln, dtype), t("wk"), t("wv"), t("bv"), UNIT_SHAPES[shape_name]["n_heads"])


@functools.lru_cache(maxsize=None)
def unit_emu(shape_name: str, n_tokens: int, ln: bool) -> Tuple[torch.Tensor, dict]:
    """``attend16`` of ``unit_inputs`` and its intermediates."""
    u = unit_inputs(shape_name, n_tokens)
    t = lambda n: u[n].to(torch.float64)
    st: dict = {}
    ctx = attend16(t("xq"), _unit_tokens(u, ln, torch.float64), t("wk"), t("wv"), t("bv"), UNIT_SHAPES[shape_name]["n_heads"], st)
    return ctx, st


def layer_inputs(sd: dict, layer: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(wk, wv, bv) of cross layer ``layer`` of a state dict, float64."""
    x = f"Qformer.bert.encoder.layer.{layer}.crossattention.self."
    t = lambda n: torch.from_numpy(np.asarray(sd[x + n])).to(torch.float64)
    return t("key.weight"), t("value.weight"), t("value.bias")


# ---------------------------------------------------------------------------------------------------- the model cases
SMALL_TOKENS = (5, 64, 257)
MODEL_CASES = tuple(f"small{n}" for n in SMALL_TOKENS) + ("peak16", "peak48", "peak128", "hot257", "dead257", "dead320", "full")
PLAIN_CASES = tuple(f"small{n}" for n in SMALL_TOKENS) + ("full",)      # no crafted key, no gain: the subnormal shares are asserted here


@functools.lru_cache(maxsize=None)
def model_case(case: str):
    """(state dict, shape, vision [F, n, width] fp32, ln_vision on?) of a named case: the small model on 3 x n plain tokens, the
    peaked models at 257 tokens, the hot key at every ``hot_positions(257)``, the dead-padded pair (the padded call's 257 live tokens
    / the same followed by 63 dead keys), the full model on the golden's 3 x 257."""
    from tests.golden import softmax_tier_cases as tc
    from tests.golden.frame_qformer_cases import FULL, GOLDEN_FRAMES, GOLDEN_TOKENS, SMALL, frame_qformer_weights, vision_rows
    if case.startswith("small"):
        return tc.small_sd(), SMALL, tc.tier_vision(3, int(case[5:])), True
    if case.startswith("peak"):
        return tc.peaked_sd(int(case[4:])), SMALL, tc.tier_vision(3, 257), True
    if case == "hot257":
        return tc.small_sd(), SMALL, tc.hot_frames(257), False
    if case == "dead257":
        return tc.small_sd(), SMALL, tc.dead_padded(257, 320)[:, :257].contiguous(), False
    if case == "dead320":
        return tc.small_sd(), SMALL, tc.dead_padded(257, 320), False
    if case == "full":
        return frame_qformer_weights(**FULL), FULL, torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"])), True
    raise ValueError(case)


@functools.lru_cache(maxsize=None)
def model_ref(case: str, dtype: torch.dtype = torch.float64):
    """(hidden, {layer: context}) of the exact model in ``dtype``."""
    from tests.golden import softmax_tier_cases as tc
    sd, shape, x, ln = model_case(case)
    c: dict = {}
    hidden = tc.ref64(sd, shape, x, ln, collect=c, dtype=dtype)
    return hidden, c["ctx"]


@functools.lru_cache(maxsize=None)
def model_emu(case: str, lin_mode: int, attn_mode: int):
    """(hidden, {layer: context}, {layer: attend16 intermediates}) of ``emu64``."""
    sd, shape, x, ln = model_case(case)
    ctx: dict = {}
    st: dict = {}
    hidden = emu64(sd, shape, x, ln, lin_mode, attn_mode, ctx_out=ctx, stats_out=st)
    return hidden, ctx, st
