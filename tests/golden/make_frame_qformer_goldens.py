"""Generate tests/golden/frame_qformer.npz by running the REAL reference image Q-former encoder on the CPU.

Build-container only (needs the reference checkout).  Run from the repo root:
    python tests/golden/make_frame_qformer_goldens.py

What runs is the reference's own ``BertEmbeddings(query_embeds=...)`` + ``BertEncoder`` (Qformer.py:55-113, 537-640), configured
as ``Blip2Base.init_Qformer`` configures the image Q-former (blip2.py:47-65): ``BertConfig()`` defaults (== bert-base-uncased; no
network for ``from_pretrained``), ``cross_attention_freq = 2``, ``encoder_width = 1408``, ``query_length = 32`` and the five LTM
attributes ``None``.  The encoder is called as ``encode_short_memory_frame`` calls it (infinityqa.py:259-270): no
``position_embedding_ext``, so no ``LongTermAttention`` runs; all-ones masks; fp32; a batch of 3 frames x 257 tokens of
``F.layer_norm(x, eps = 1e-5)`` (``ln_vision``) of synthetic vision rows.  The module loader is ``make_qformer_goldens.py``'s.
Nothing of the reference is copied into the repository -- only the numbers it produces.
"""
from __future__ import annotations

import os
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden.frame_qformer_cases import (FULL, GOLDEN_FRAMES, GOLDEN_PATH, GOLDEN_TAPS, GOLDEN_TOKENS, LN_VISION_EPS,
                                              frame_qformer_weights, vision_rows)
from tests.golden.make_qformer_goldens import load_reference_qformer


def build(weights):
    qf = load_reference_qformer()
    cfg = qf.BertConfig()
    assert (cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads) == \
        (FULL["n_layers"], FULL["hidden"], FULL["inter"], FULL["n_heads"])
    cfg.encoder_width = FULL["enc_width"]
    cfg.add_cross_attention = True
    cfg.cross_attention_freq = 2
    cfg.query_length = FULL["n_query"]
    ltm_none = dict(num_basis=None, sticky=None, sigmas=None, tau=None, alpha=None)       # blip2.py:55-59
    for k, v in ltm_none.items():
        setattr(cfg, k, v)
    try:
        enc = qf.BertEncoder(cfg)
    except Exception as e:                                   # the LongTermAttention constructor rejects None on the CPU:
        # any value serves -- the module is constructed and never called here (position_embedding_ext is None)
        print(f"BertEncoder(None LTM attributes) raised {type(e).__name__}: {e}; constructing with placeholder values")
        cfg.num_basis, cfg.sticky, cfg.sigmas, cfg.tau, cfg.alpha = 64, True, [0.005, 0.01], 0.75, 1.0
        enc = qf.BertEncoder(cfg)
    emb = qf.BertEmbeddings(cfg)
    sd_emb = {k[len("Qformer.bert.embeddings."):]: torch.from_numpy(v) for k, v in weights.items()
              if k.startswith("Qformer.bert.embeddings.")}
    sd_enc = {k[len("Qformer.bert.encoder."):]: torch.from_numpy(v) for k, v in weights.items()
              if k.startswith("Qformer.bert.encoder.")}
    res = emb.load_state_dict(sd_emb, strict=False)          # word / position embeddings keep their init: query_embeds alone is used
    assert not res.unexpected_keys, res
    res = enc.load_state_dict(sd_enc, strict=False)
    assert not res.unexpected_keys and all(".long_term_attention." in k for k in res.missing_keys), res
    return emb.eval(), enc.eval(), torch.from_numpy(weights["query_tokens"])


def main():
    weights = frame_qformer_weights(**FULL)
    x = torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"]))
    k = F.layer_norm(x, (x.size(-1),), torch.from_numpy(weights["ln_vision.weight"]), torch.from_numpy(weights["ln_vision.bias"]),
                     LN_VISION_EPS)
    os.chdir(tempfile.mkdtemp())
    emb, enc, qtok = build(weights)
    taps = {}

    def tap(name):
        def hook(mod, args, output):
            taps[name] = (output[0] if isinstance(output, tuple) else output).detach().clone()
        return hook

    for l in GOLDEN_TAPS:
        enc.layer[l].crossattention.self.register_forward_hook(tap(f"l{l}_xctx"))     # the cross-attention context (:303-304)
    B, Q = x.size(0), FULL["n_query"]
    with torch.no_grad():
        h0 = emb(query_embeds=qtok.expand(B, -1, -1))                                 # Qformer.py:942-947
        res = enc(h0, None, attention_mask=torch.zeros(B, 1, 1, Q), head_mask=[None] * FULL["n_layers"],
                  encoder_hidden_states=k, encoder_attention_mask=torch.zeros(B, 1, 1, k.size(1)), return_dict=True,
                  query_length=Q)
    out = {"hidden": res.last_hidden_state.numpy().copy(), "h0": h0[0].numpy().copy()}
    for name, v in taps.items():
        out[name] = v.numpy().copy()
    assert out["hidden"].shape == (GOLDEN_FRAMES, Q, FULL["hidden"]) and all(out[f"l{l}_xctx"].shape == out["hidden"].shape for l in GOLDEN_TAPS)
    np.savez_compressed(GOLDEN_PATH, **out)
    print(f"frame_qformer: {sorted(out)}; {os.path.getsize(GOLDEN_PATH) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
