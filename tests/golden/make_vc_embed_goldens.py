"""Generate tests/golden/vc_embed.npz by running the REAL ``BertEmbeddings`` of the reference's VideoChat2 Q-former on the CPU.

Build-container only (needs /root/reference).  Run from the repo root:
    python tests/golden/make_vc_embed_goldens.py

What runs is the reference's own embedding layer (infty-VideoChat2/models/blip2/Qformer.py:54-111), imported by path as
``make_vc_goldens.py`` imports ``BertEncoder``, at vocab 50, 32 positions, hidden 128, 40 query tokens, eval mode, called as
``BertModel.forward`` calls it (``input_ids`` + ``query_embeds``; ``query_embeds`` alone for a video without instruction).  Stored:
the tables, the ids and the output rows -- numbers only, nothing of the reference's program text.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests.golden.make_vc_goldens import load_reference_vc_qformer

VOCAB, MAX_POS, HIDDEN, N_QUERY, EPS = 50, 32, 128, 40, 1e-12
# lengths 5, 0 and 17; id 0, id 49 and a repeated id (7) among them
IDS = ([0, 49, 7, 7, 23], [], [49, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0, 7, 48])
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vc_embed.npz")


def main():
    qf = load_reference_vc_qformer()
    cfg = qf.BertConfig()
    cfg.vocab_size, cfg.max_position_embeddings, cfg.hidden_size, cfg.layer_norm_eps = VOCAB, MAX_POS, HIDDEN, EPS
    emb = qf.BertEmbeddings(cfg).eval()
    rng = np.random.default_rng(20260)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    tables = {"word": rng.normal(0, 0.5, (VOCAB, HIDDEN)), "pos": rng.normal(0, 0.5, (MAX_POS, HIDDEN)),
              "gamma": rng.normal(1, 0.1, HIDDEN), "beta": rng.normal(0, 0.1, HIDDEN), "query_tokens": rng.normal(0, 1.0, (N_QUERY, HIDDEN))}
    tables = {k: np.asarray(v, np.float32) for k, v in tables.items()}
    with torch.no_grad():
        emb.word_embeddings.weight.copy_(f32(tables["word"]))
        emb.position_embeddings.weight.copy_(f32(tables["pos"]))
        emb.LayerNorm.weight.copy_(f32(tables["gamma"]))
        emb.LayerNorm.bias.copy_(f32(tables["beta"]))
        q = f32(tables["query_tokens"]).unsqueeze(0)
        out = dict(tables)
        for v, ids in enumerate(IDS):
            rows = emb(input_ids=torch.tensor([ids], dtype=torch.long) if ids else None, query_embeds=q)
            assert rows.shape == (1, N_QUERY + len(ids), HIDDEN)
            out[f"ids{v}"] = np.asarray(ids, np.int32)
            out[f"rows{v}"] = rows[0].numpy().copy()
    out["eps"] = np.float64(EPS)
    np.savez_compressed(PATH, **out)
    print(f"vc_embed: {len(out)} arrays, {os.path.getsize(PATH) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
