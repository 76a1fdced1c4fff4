"""Generate tests/golden/density.npz: the attention density the REAL Video-LLaMA operator pickles on every forward.

Build-container only (needs the reference checkout, like make_goldens.py, whose loader and layer builder this reuses).  Run
from the repo root:   python tests/golden/make_density_goldens.py

The reference writes ``./alphas_uniform`` at the end of every forward (long_term_attention_gibbs.py:320-343).  This script runs
the golden chains of ``DENSITY_CASES`` exactly as make_goldens.py does and, after every layer's forward of the chain's SECOND
chunk (first-chunk operator behind it) and of its LAST chunk (sticky steps behind it), reads back the pickle that forward just
wrote.  Stored per such call, as float32: ``<case>/c<c>_l<l>_alphas`` [nq, 1, H, 768] and the full scores of the call
``<case>/c<c>_l<l>_scores`` [H, nq, N], for the queries ``<case>/q_idx``.  Query subsampling: every 8th query -- the subsampling
the case's own ``_scores`` use (all queries, every 4th for ``headline``) thinned to every 8th, which keeps the file under the
size limit of a committed file.  Only numbers are stored.
"""
from __future__ import annotations

import os
import pickle
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests.golden.cases import CASES, DENSE_CASES, GOLDEN_DIR, call_seed, case_inputs
from tests.golden.make_goldens import _Recorder, build_layer, load_reference

DENSITY_CASES = ("cfg1_sticky", "peaked", "tau09", "n144", "n96_dense", "headline")
QUERY_STEP = 8
OUT = os.path.join(GOLDEN_DIR, "density.npz")


def run_case(case):
    mod = load_reference(case.variant)
    mod.dist = _Recorder()
    ks, qs, ws = case_inputs(case)
    layers = [build_layer(mod, case, ws[l]) for l in range(case.n_layers)]
    q_idx = np.arange(0, case.Q, QUERY_STEP)
    out = {f"{case.name}/q_idx": q_idx.astype(np.int32)}
    wanted = {1, len(case.chunk_T) - 1}
    with torch.no_grad():
        for c in range(len(case.chunk_T)):
            k = torch.from_numpy(ks[c]).unsqueeze(0)
            for l, m in enumerate(layers):
                q = torch.from_numpy(qs[l]).unsqueeze(0)
                torch.manual_seed(call_seed(case, c, l))
                m.length = m.target_len = k.size(1)
                if os.path.exists("alphas_uniform"):
                    os.remove("alphas_uniform")
                m(k, q, new_doc=(c in case.new_doc_at), layer_n=l)
                if c not in wanted:
                    continue
                with open("alphas_uniform", "rb") as f:
                    alphas = pickle.load(f)                  # [Q, 1, H, 768], the permute of :337
                assert tuple(alphas.shape) == (case.Q, 1, case.H, 768), alphas.shape
                scores = (m.queries / (m.d_head ** 0.5)) @ m.keys.transpose(-1, -2)
                tag = f"{case.name}/c{c}_l{l}"
                out[tag + "_alphas"] = alphas[q_idx].numpy().astype(np.float32).copy()
                out[tag + "_scores"] = scores[0][:, q_idx, :].numpy().astype(np.float32).copy()
    return out


def main():
    os.chdir(tempfile.mkdtemp())                             # the reference writes ./alphas_uniform
    by_name = {c.name: c for c in CASES + DENSE_CASES}
    out = {}
    for name in DENSITY_CASES:
        out.update(run_case(by_name[name]))
        print(name, "done", flush=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
