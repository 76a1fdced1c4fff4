"""Shapes, synthetic weights and inputs of the frame (image) Q-former tests, shared by ``make_frame_qformer_goldens.py`` (which runs
the real reference encoder on them) and the tests.  Weights and inputs are regenerated from seeds, never stored."""
from __future__ import annotations

import os
import sys
from typing import Dict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from infinite_video_amd import synth

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frame_qformer.npz")
LN_VISION_EPS = 1e-5                       # nn.LayerNorm's default (blip2.py:76), not bert's 1e-12
SEED_FQ = 4242
# the model's image Q-former (blip2.py:47-65 on eva_clip_g: 1408-wide, 257 tokens a frame)
FULL = dict(n_layers=12, hidden=768, inter=3072, enc_width=1408, n_query=32, n_heads=12)
GOLDEN_FRAMES, GOLDEN_TOKENS = 3, 257
GOLDEN_TAPS = (0, 10)                      # the first and the last cross layer
# the small model of the GPU tests: 4 layers (cross layers 0 and 2), 2 heads
SMALL = dict(n_layers=4, hidden=128, inter=256, enc_width=128, n_query=8, n_heads=2)


def frame_qformer_weights(n_layers: int, hidden: int, inter: int, enc_width: int, n_query: int, n_heads: int = 0,
                          seed: int = SEED_FQ) -> Dict[str, np.ndarray]:
    """A state dict under the reference model's checkpoint keys: the encoder from ``synth.videochat2_qformer_weights`` (which has
    the text FFN ``intermediate`` / ``output`` the image Q-former carries and never uses) under ``Qformer.``, plus
    ``Qformer.bert.embeddings.LayerNorm.*``, ``query_tokens`` and ``ln_vision.*``."""
    base = synth.videochat2_qformer_weights(n_layers=n_layers, hidden=hidden, inter=inter, enc_width=enc_width, cross_freq=2,
                                            n_query=n_query, proj_out=64, seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = {"Qformer." + k: v for k, v in base.items() if k.startswith("bert.")}
    out["query_tokens"] = base["query_tokens"]
    f32 = lambda a: np.asarray(a, np.float32)
    out["Qformer.bert.embeddings.LayerNorm.weight"] = f32(1.0 + 0.1 * rng.standard_normal(hidden))
    out["Qformer.bert.embeddings.LayerNorm.bias"] = f32(0.1 * rng.standard_normal(hidden))
    out["ln_vision.weight"] = f32(1.0 + 0.1 * rng.standard_normal(enc_width))
    out["ln_vision.bias"] = f32(0.1 * rng.standard_normal(enc_width))
    return out


def vision_rows(n_frames: int, n_tokens: int, width: int, seed: int = SEED_FQ + 7) -> np.ndarray:
    """Synthetic vision-encoder output [F, n_tokens, width] before ``ln_vision``: rows with their own offset and scale, so the
    LayerNorm has something to do."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_frames, n_tokens, width))
    x = x * (0.5 + rng.random((n_frames, n_tokens, 1))) + 0.3 * rng.standard_normal((n_frames, n_tokens, 1))
    return np.asarray(x, np.float32)


def oracle_weights(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """``sd`` under the names ``oracle.videochat2_oracle.VideoChat2Oracle`` reads (``bert.encoder...``, ``query_tokens``) with a
    zero ``mistral_proj`` (the oracle projects whatever it encodes; the image Q-former has no projection)."""
    out = {k[len("Qformer."):]: v for k, v in sd.items() if k.startswith("Qformer.bert.encoder.")}
    out["query_tokens"] = sd["query_tokens"]
    hidden = sd["query_tokens"].shape[-1]
    out["mistral_proj.weight"] = np.zeros((8, hidden), np.float32)
    out["mistral_proj.bias"] = np.zeros((8,), np.float32)
    return out
