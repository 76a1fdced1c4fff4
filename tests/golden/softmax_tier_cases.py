"""Inputs that make the row softmax of the short-term attention visible, shared by ``tests/test_softmax_tiers_cpu.py`` (which checks
the constructions themselves in float64) and ``tests/test_softmax_tiers_gpu.py`` (which runs them on the device).  Pure numpy / torch
on the CPU, regenerated from seeds, nothing stored.

With the synthetic weights every cross-attention score lies within about +-0.4, so the softmax is nearly a mean: a wrong maximum
is shift-invariant and overflows nothing, and a pad key that leaks into the sum (score exactly 0) moves the output by about 1 / n.
Two crafted keys remove that blind spot.  The score of key ``k`` in row (layer l, head h, query q) is ``A[l,h,q] . k`` plus a
per-row constant (the key bias), with ``A[l,h,q] = Wk_h^T (Wq h_l)_{q,h} / sqrt(dh)``.  Both cross layers of the small model give
32 rows of 128 columns, so ``pinv(A) @ (t * 1)`` is a key whose score is ``t`` in every row:

* the DEAD key, ``t = -300``: at least 150 below every live score of its row, so ``expf`` gives exactly 0 in fp32 -- the key has
  no mass, bit for bit, and a frame padded with dead keys must equal the frame the kernels pad themselves;
* the HOT key, ``t = +100``: at least 90 above every other score of its row, so a maximum that misses it overflows ``expf``
  (above 88.7) and the row turns inf / NaN.

Layer 2's rows depend on the keys (through layer 0's context), so the construction is iterated; every round rounds the key to
the type the device reads (fp32 or bf16), so the conditions the CPU test asserts hold on the very tensors the device gets.

Everything returned here is cached and shared: callers must not write into it."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden.frame_qformer_cases import LN_VISION_EPS, SMALL, frame_qformer_weights, vision_rows

ATOL = 2e-4                                 # the project's own bound
CROSS_LAYERS = (0, 2)                       # of SMALL: 4 layers, a cross-attention in every second one
T_DEAD, T_HOT = -300.0, 100.0
DEAD_MARGIN, HOT_MARGIN = 150.0, 90.0
ROUNDS = 4

# A: every tier against float64 (F = 3, ln_vision on)
TIER_PADDED = (1023, 1025, 2047, 2049, 8191, 8193)     # both register groups of <2>, a partial and a full <8>, the long kernel
TIER_WHOLE = (1024, 2112, 8256)                        # reg<2>, reg<8>, the three-pass kernel
# B: (n live tokens, n_pad = ceil(n / 64) * 64)
PAD_PAIRS = ((1, 64), (65, 128), (127, 128), (257, 320), (1025, 1088), (2049, 2112), (8129, 8192), (8193, 8256))
# C: the hot key at every reduction seam: first / last lane, the wave boundary (columns 252-259), the register-group boundaries,
# the last live column next to the pad.  (8191 and 8192 fill the last register group of the two <8> kernels, which 2049 and 2112
# leave empty.)
HOT_SIZES = (257, 2049, 8191, 8193, 2112, 8192, 8256)
HOT_POSITIONS = (0, 3, 255, 256, 1020, 1023, 1024, 2047, 2048, 4100, 8191)
HOT_SHORT_SIZES = (256, 2112, 8256)
# D: peaked scores
# (the smallest span of a score row -- max minus min over the keys -- is 0.20 in the plain model and scales with the gain: 3.2 at
# 16, 9.5 at 48, 25.4 at 128 for n = 257, more at the longer rows.  Spans of 8 and of 24 in EVERY row therefore need 48 and 128;
# 16 stays as the mildest case with the floor its own scale gives, 16 * 0.20 rounded down.)
PEAK_GAINS = (16, 48, 128)
PEAK_SPANS = {16: 3.0, 48: 8.0, 128: 24.0}             # the least score span over all rows that the CPU test asserts
PEAK_SIZES = (257, 2049, 8193)
# E: one handle across the tiers
HANDLE_WALK = (8193, 65, 2049, 65, 8256, 1)


@functools.lru_cache(maxsize=None)
def small_sd() -> Dict[str, np.ndarray]:
    return frame_qformer_weights(**SMALL)


@functools.lru_cache(maxsize=None)
def peaked_sd(gain: int) -> Dict[str, np.ndarray]:
    """``small_sd()`` with the cross-attention query weight and bias of both cross layers scaled by ``gain``: the scores spread
    by that factor.  The scale sits in the state dict, so the reference and the device see the same model."""
    sd = dict(small_sd())
    for l in CROSS_LAYERS:
        for leaf in ("weight", "bias"):
            k = f"Qformer.bert.encoder.layer.{l}.crossattention.self.query.{leaf}"
            sd[k] = np.asarray(sd[k] * np.float32(gain), np.float32)
    return sd


# ---------------------------------------------------------------------------------------------------- the reference
def ref64(sd: dict, shape: dict, vision: torch.Tensor, ln: bool, collect: Optional[dict] = None,
          dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The image Q-former in float64 (Qformer.py BertEmbeddings + BertEncoder, all-ones masks, eval mode, no long-term memory):
    vision [F, n, width] (before ``ln_vision`` when ``ln``) -> last hidden state [F, Q, hidden].

    ``collect``: a dict that receives, per cross layer l, ``collect["ctx"][l]`` [F, Q, hidden] (the cross-attention context,
    Qformer.py:303-304: what ``infv_vqf_set_context_tap`` copies), ``collect["scores"][l]`` [F, H, Q, n] and
    ``collect["A"][l]`` [F, H * Q, width] (the score rows without the key bias).  ``dtype=torch.float32`` is the same
    arithmetic in single precision: the measure of what fp32 alone costs."""
    w = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    H, Hd = shape["n_heads"], shape["hidden"]
    dh = Hd // H
    lin = lambda x, n: F.linear(x, w[n + ".weight"], w[n + ".bias"])
    lnorm = lambda x, n, eps=1e-12: F.layer_norm(x, (x.size(-1),), w[n + ".weight"], w[n + ".bias"], eps)
    heads = lambda x: x.reshape(x.size(0), x.size(1), H, dh).permute(0, 2, 1, 3)
    if collect is not None:
        collect.update(ctx={}, scores={}, A={})

    def attend(q, k, v, layer=None):
        s = torch.matmul(heads(q), heads(k).transpose(-1, -2)) / math.sqrt(dh)
        if layer is not None and collect is not None:
            collect["scores"][layer] = s
        p = torch.softmax(s, dim=-1)
        return torch.matmul(p, heads(v)).permute(0, 2, 1, 3).reshape(q.size(0), q.size(1), Hd)

    k = vision.detach().cpu().to(dtype)
    if ln:
        k = lnorm(k, "ln_vision", LN_VISION_EPS)
    h = lnorm(w["query_tokens"], "Qformer.bert.embeddings.LayerNorm").expand(k.size(0), -1, -1)
    for l in range(shape["n_layers"]):
        p = f"Qformer.bert.encoder.layer.{l}."
        a = p + "attention."
        h = lnorm(lin(attend(lin(h, a + "self.query"), lin(h, a + "self.key"), lin(h, a + "self.value")), a + "output.dense") + h,
                  a + "output.LayerNorm")
        if l % 2 == 0:
            x = p + "crossattention."
            q = lin(h, x + "self.query")
            ctx = attend(q, lin(k, x + "self.key"), lin(k, x + "self.value"), layer=l)
            if collect is not None:
                collect["ctx"][l] = ctx
                wk = w[x + "self.key.weight"].reshape(H, dh, -1)
                collect["A"][l] = (torch.einsum("fhqd,hde->fhqe", heads(q), wk) / math.sqrt(dh)).reshape(k.size(0), H * q.size(1), -1)
            h = lnorm(lin(ctx, x + "output.dense") + h, x + "output.LayerNorm")
        h = lnorm(lin(F.gelu(lin(h, p + "intermediate_query.dense")), p + "output_query.dense") + h, p + "output_query.LayerNorm")
    return h


def torch_short_attention(frames, xq, wk, bk, wv, bv, H):
    """Plain PyTorch reference of the short-term cross-attention (Qformer.py:225-301 with zero masks), any head count: the
    restatement of ``tests/test_config_sweep_gpu.py``'s, in the precision of its arguments."""
    dh = xq.shape[1] // H
    K = F.linear(frames, wk, bk)
    V = F.linear(frames, wv, bv)
    heads = lambda x: x.reshape(x.shape[0], H, dh).permute(1, 0, 2)
    s = torch.matmul(heads(xq), heads(K).transpose(-1, -2)) / math.sqrt(dh)
    return torch.matmul(torch.softmax(s, -1), heads(V)).permute(1, 0, 2).reshape(xq.shape[0], -1)


# ---------------------------------------------------------------------------------------------------- the crafted keys
def _rounded(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> the values of ``dtype`` (fp32 or bf16), kept as fp32."""
    return x.to(torch.float32).to(dtype).to(torch.float32)


def craft_keys(x: torch.Tensor, slots, t: float, dtype: torch.dtype = torch.float32, sd: Optional[dict] = None) -> torch.Tensor:
    """``x`` [F, n, width] fp32 (no ``ln_vision``) with the rows ``slots[f]`` of frame f replaced by that frame's key of score
    ``t`` in all 32 cross-attention rows; ROUNDS rounds, the key rounded to ``dtype`` in each."""
    sd = small_sd() if sd is None else sd
    x = _rounded(x.double(), dtype).clone()
    for _ in range(ROUNDS):
        c: dict = {}
        ref64(sd, SMALL, x, False, collect=c)
        for f in range(x.size(0)):
            A = torch.cat([c["A"][l][f] for l in CROSS_LAYERS])                  # [32, width]
            key = torch.linalg.pinv(A) @ torch.full((A.size(0),), t, dtype=torch.float64)
            x[f, slots[f]] = _rounded(key, dtype)
    return x


def hot_positions(n: int) -> Tuple[int, ...]:
    return tuple(sorted({p for p in HOT_POSITIONS + (n - 1,) if 0 <= p < n}))


@functools.lru_cache(maxsize=None)
def tier_vision(n_frames: int, n_tokens: int) -> torch.Tensor:
    """Plain synthetic vision rows [F, n, 128] fp32 (A, D, E)."""
    return torch.from_numpy(vision_rows(n_frames, n_tokens, SMALL["enc_width"], seed=700 + n_tokens))


@functools.lru_cache(maxsize=None)
def dead_padded(n: int, n_pad: int, bf16: bool = False) -> torch.Tensor:
    """B: [2, n_pad, 128] fp32 -- n live rows a frame, then n_pad - n copies of the frame's dead key.  ``[:, :n]`` is the padded
    call's input.  ``bf16``: every value is a bf16 number."""
    x = torch.zeros(2, n_pad, SMALL["enc_width"])
    x[:, :n] = tier_vision(2, n)
    dtype = torch.bfloat16 if bf16 else torch.float32
    return craft_keys(x, [slice(n, n_pad)] * 2, T_DEAD, dtype)


@functools.lru_cache(maxsize=None)
def hot_frames(n: int) -> torch.Tensor:
    """C: [len(hot_positions(n)), n, 128] fp32 -- frame f holds its hot key at position ``hot_positions(n)[f]``."""
    pos = hot_positions(n)
    return craft_keys(tier_vision(len(pos), n), [slice(p, p + 1) for p in pos], T_HOT)


# ---------------------------------------------------------------------------------------------------- C through short_attention
SHORT = dict(n_heads=2, n_query=8, enc_width=128, hidden=128)
# The key weight is drawn at 0.32 rather than the 0.02 of test_short_attention_sweep, and the frames at 0.25: the score rows are
# then long enough that the +100 key has entries of a few tens and the context it dominates (the output here, with no LayerNorm
# behind it) stays within a few units -- the scale at which ATOL, an absolute bound, is the project's bound -- while the live
# scores stay within a few units of 0.  (At 0.02 the key's entries are in the hundreds, the context about 30, and the relative
# 2^-17 of the hi + lo bf16 pieces of the key alone is 2e-4 there.)
SHORT_WK_STD, SHORT_FRAME_STD = 0.32, 0.25


@functools.lru_cache(maxsize=None)
def short_inputs(n_tokens: int) -> Dict[str, torch.Tensor]:
    """frames [n, 128], xq [8, 128], wk / wv [128, 128], bk / bv [128] fp32, and ``hot`` [128]: the key of score +100 in all
    16 rows (one cross layer, so no iteration: the rows do not depend on the keys)."""
    H, Q, dw, hid = SHORT["n_heads"], SHORT["n_query"], SHORT["enc_width"], SHORT["hidden"]
    g = torch.Generator().manual_seed(5000 + n_tokens)
    out = dict(frames=torch.randn(n_tokens, dw, generator=g) * SHORT_FRAME_STD, xq=torch.randn(Q, hid, generator=g),
               wk=torch.randn(hid, dw, generator=g) * SHORT_WK_STD, wv=torch.randn(hid, dw, generator=g) * 0.02,
               bk=torch.randn(hid, generator=g) * 0.02, bv=torch.randn(hid, generator=g) * 0.02)
    dh = hid // H
    q = out["xq"].double().reshape(Q, H, dh).permute(1, 0, 2)                                    # [H, Q, dh]
    A = (torch.einsum("hqd,hde->hqe", q, out["wk"].double().reshape(H, dh, dw)) / math.sqrt(dh)).reshape(H * Q, dw)
    out["hot"] = (torch.linalg.pinv(A) @ torch.full((H * Q,), T_HOT, dtype=torch.float64)).float()
    return out


def short_with_hot(n_tokens: int, pos: int) -> torch.Tensor:
    """``short_inputs(n_tokens)["frames"]`` with the hot key at row ``pos`` (a fresh tensor)."""
    si = short_inputs(n_tokens)
    fr = si["frames"].clone()
    fr[pos] = si["hot"]
    return fr


def short_scores(n_tokens: int, pos: int) -> torch.Tensor:
    """float64 scores [H, Q, n] of ``short_with_hot(n_tokens, pos)``."""
    si = short_inputs(n_tokens)
    H = SHORT["n_heads"]
    dh = SHORT["hidden"] // H
    heads = lambda x: x.reshape(x.shape[0], H, dh).permute(1, 0, 2)
    K = F.linear(short_with_hot(n_tokens, pos).double(), si["wk"].double(), si["bk"].double())
    return torch.matmul(heads(si["xq"].double()), heads(K).transpose(-1, -2)) / math.sqrt(dh)


def short_reference(n_tokens: int, pos: int, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    si = short_inputs(n_tokens)
    t = lambda k: si[k].to(dtype)
    return torch_short_attention(short_with_hot(n_tokens, pos).to(dtype), t("xq"), t("wk"), t("bk"), t("wv"), t("bv"), SHORT["n_heads"])
