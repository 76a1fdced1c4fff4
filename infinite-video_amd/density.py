"""Float64 restatements of the attention-density read-outs (``infv_ltm_density``, ``infv_ltm_masses``; kernels:
csrc/ltm_density.hip).  Like ``philox.py`` they mirror the device for tests and serve CPU users who hold a step's scores.

The reference evaluates, after every step, the density of the memory's attention on a grid (long_term_attention_gibbs.py:320-343)

    s(t) = sum_n psi_n(t) S[n];  e = exp(s);  dens = e / trapz(e over the point's segment);  alphas = dens / sum(dens)

and its read-out weighs basis function n with ``alpha[n] = w_n e^{S_n} / (sum_m w_m e^{S_m} + w_out)`` (the ``integral`` of
``expected_value``, :282).  ``scores`` are a step's FULL scores ``[..., N]`` -- key-bias term included: a grid point in no box
(``t = 1.0``) enters as ``exp(0)``, so the bias decides where it stands relative to the rest.
"""
from __future__ import annotations

import numpy as np

from .basis_maps import GridPlan


def grid_scores(scores, grid_plan: GridPlan) -> np.ndarray:
    """s(t_m) [..., M] as the device forms it: the entries of a point added in CSR order in fp32 (exact for one-box points)."""
    S = np.asarray(scores, dtype=np.float32)
    ptr, box, val = grid_plan.pt_ptr, grid_plan.pt_box, grid_plan.pt_val
    M = len(ptr) - 1
    s = np.zeros(S.shape[:-1] + (M,), dtype=np.float32)
    count = np.diff(ptr)
    for j in range(int(count.max(initial=0))):                 # j-th entry of every point that has one
        pts = np.flatnonzero(count > j)
        e = ptr[pts] + j
        s[..., pts] = s[..., pts] + val[e] * S[..., box[e]]
    return s


def reference_alphas(scores, grid_plan: GridPlan) -> np.ndarray:
    """The reference's ``alphas`` (:328-337) of scores ``[H, Q, N]``: float64 ``[Q, 1, H, M]``.  The row maximum is subtracted
    before ``exp`` (the reference does not, :248, and overflows where this stays finite); nothing else differs."""
    s = grid_scores(scores, grid_plan).astype(np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    w = grid_plan.pt_weight.astype(np.float64)
    dens = np.empty_like(e)
    for g in range(len(grid_plan.seg_begin) - 1):
        sl = slice(int(grid_plan.seg_begin[g]), int(grid_plan.seg_begin[g + 1]))
        dens[..., sl] = e[..., sl] / (e[..., sl] * w[sl]).sum(-1, keepdims=True)
    alphas = dens / dens.sum(-1, keepdims=True)
    if alphas.ndim != 3:
        raise ValueError(f"scores must be [H, Q, N], got {np.shape(scores)}")
    return np.ascontiguousarray(alphas.transpose(1, 0, 2)[:, None])


def box_weights(scores, readout_w, w_out: float) -> np.ndarray:
    """alpha ``[..., N]`` of scores ``[..., N]`` (:282 in closed form), float64."""
    S = np.asarray(scores, dtype=np.float64)
    w = np.asarray(readout_w, dtype=np.float64)
    m = np.maximum(S.max(-1, keepdims=True), 0.0)
    e = w * np.exp(S - m)
    return e / (e.sum(-1, keepdims=True) + float(w_out) * np.exp(-m))


def box_masses(scores, readout_w, w_out: float) -> np.ndarray:
    """``mass[n]`` = mean over the H*Q rows of alpha, float64 ``[N]`` -- the device's sum over rows (include/infv_ltm.h states its
    order) runs in float64 too, so the order does not show at fp32."""
    a = box_weights(scores, readout_w, w_out)
    return a.reshape(-1, a.shape[-1]).mean(0)
