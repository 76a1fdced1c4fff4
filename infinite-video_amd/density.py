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


# ---- source weights: the memory traced back to its frames (infv_ltm_source_weights; kernel: csrc/ltm_sources.hip) ----
# The sparse update is linear in the frame means (long_term_attention_gibbs.py:207-216 in closed form), so B[n] = sum over sources
# of W[n][source] * kbar[source] with a W that obeys the update's own recurrence on one-hot rows.  The reference's
# relevant_frames.py:53-69 reads grid point m of segment i of ``alphas`` as frame m + 256 * i, which holds only for a memory that
# was never consolidated.  include/infv_ltm.h states the recurrence and its order; the functions below restate it in numpy.
def _source_steps(plan, bins, n_chunks, new_doc, W, col_begin, frames_per_source, dtype):
    """Yields ``(c, W_c)`` for the chunks of one call; ``W_c`` [N, M] is the matrix after chunk c (a fresh array each time)."""
    T, N = int(plan.T), int(plan.N)
    if plan.dense or plan.psi:
        raise ValueError("source weights exist for sparse box plans only (dense and general-psi plans mix boxes through a dense operator)")
    g = T if frames_per_source is None else int(frames_per_source)
    C, col_begin = int(n_chunks), int(col_begin)
    if C < 1 or g < 1 or T % g or col_begin < 0:
        raise ValueError("need n_chunks >= 1, frames_per_source >= 1 dividing T, col_begin >= 0")
    per = T // g
    M = col_begin + C * per
    cur = np.zeros((N, M), dtype=dtype)
    if not new_doc and col_begin:
        if W is None or np.shape(W)[0] != N or np.shape(W)[1] < col_begin:
            raise ValueError(f"W must be [{N}, >= {col_begin}] to continue a document")
        cur[:, :col_begin] = np.asarray(W)[:, :col_begin]
    if bins is not None:
        bins = np.asarray(bins)
        if bins.shape != (C, plan.S):
            raise ValueError(f"bins must be [{C}, {plan.S}] (one layer of the draw trace), got {bins.shape}")
    ptr, slot = plan.inf_old_ptr, plan.inf_old_slot
    count = np.diff(ptr)
    n_draw = len(plan.bin_box) - 1                             # the draw has n_bins - 1 outcomes

    def injected(row_box, row_begin, row_end, c):
        cnt = np.zeros((N, per), dtype=np.int64)
        for b, lo, hi in zip(row_box, row_begin, row_end):
            np.add.at(cnt[b], np.arange(lo, hi) // g, 1)
        return cnt.astype(dtype), col_begin + c * per

    for c in range(C):
        live = col_begin + (c + 1) * per                       # columns at and beyond are still zero
        new = np.zeros((N, M), dtype=dtype)
        if new_doc and c == 0:
            cnt, at = injected(plan.first_row_box, plan.first_row_begin, plan.first_row_end, c)
            new[:, at:at + per] = plan.first_box_val.astype(dtype)[:, None] * cnt
        else:
            if bins is not None:
                b = bins[c].astype(np.int64)
                ok = (b >= 0) & (b < n_draw)                   # a bin out of range is never an index: a zero row
                idx = np.where(ok, plan.bin_box[np.where(ok, b, 0)], -1)
            else:
                idx = plan.uniform_idx
            acc = np.zeros((N, live), dtype=dtype)
            for j in range(int(count.max(initial=0))):         # j-th stored slot of every box that has one: the CSR order
                boxes = np.flatnonzero(count > j)
                src = idx[slot[ptr[boxes] + j]]
                boxes, src = boxes[src >= 0], src[src >= 0]
                acc[boxes] = acc[boxes] + cur[src, :live]
            cnt, at = injected(plan.inf_row_box, plan.inf_row_begin, plan.inf_row_end, c)
            acc[:, at:at + per] = acc[:, at:at + per] + cnt    # the new frames' count: added last, one number
            new[:, :live] = plan.inf_box_val.astype(dtype)[:, None] * acc
        cur = new
        yield c, cur


def source_weights(plan, bins, n_chunks, new_doc=True, W=None, col_begin=0, frames_per_source=None, dtype=np.float64):
    """``W`` [N, col_begin + n_chunks * T / g] of ONE layer after the call's chunks: ``B[n] = sum_m W[n][m] * kbar[source m]``, source
    m being frames ``[m * g, (m + 1) * g)`` of the video, ``g = frames_per_source`` (default T: one column per chunk).
    ``bins`` [n_chunks, S]: the layer's rows of the draw trace (``LTMEngine.set_trace``), ``None`` for a memory that is not sticky.
    ``new_doc=False`` continues from ``W`` [N, >= col_begin].  With ``dtype=np.float64`` this is the float64 recurrence; with
    ``np.float32`` it is the ordered fp32 form that ``infv_ltm_source_weights`` equals bit for bit."""
    out = None
    for _, out in _source_steps(plan, bins, n_chunks, new_doc, W, col_begin, frames_per_source, dtype):
        pass
    return out


def source_attention(mass_trace, plan, bins, n_chunks, new_doc=True, W=None, col_begin=0, frames_per_source=None,
                     dtype=np.float64, normalise=False):
    """The attention map of the video, chunk by chunk: ``attn[c][m] = sum_n mass_trace[c][n] * W_c[n][m]`` in float64, with
    ``W_c`` the source weights after chunk c -- the mirror of ``attn_all``.  ``mass_trace`` [n_chunks, N]: one layer of
    ``LTMEngine.set_mass_trace``.  Raw by default (rows do not sum to 1: the ridge and the read-out's ``w_out``);
    ``normalise=True`` divides every row by its sum.  Returns ``(W, attn)``."""
    mass = np.asarray(mass_trace, dtype=np.float64)
    rows, out = [], None
    for c, out in _source_steps(plan, bins, n_chunks, new_doc, W, col_begin, frames_per_source, dtype):
        rows.append(mass[c] @ out.astype(np.float64))
    attn = np.stack(rows)
    if normalise:
        attn = attn / attn.sum(-1, keepdims=True)
    return out, attn


def _video_slices(chunk_counts):
    counts = [int(c) for c in chunk_counts]
    if any(c < 0 for c in counts):
        raise ValueError(f"chunk_counts must be non-negative, got {counts}")
    cu = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return counts, cu


def source_weights_videos(plan, bins, chunk_counts, frames_per_source=None, dtype=np.float64):
    """``source_weights`` of V videos whose chunks are PACKED as the lockstep calls pack them (video v's rows at
    ``[cu[v], cu[v+1])``, ``cu`` the running sum of ``chunk_counts``), every video a new document: ``W`` [V, N, M_max] of ONE
    layer, ``M_max = max_v C_v * T / g``; video v's columns at and beyond its own ``M_v`` -- all of them for a video with no
    chunk -- are 0.  ``bins`` [sum C_v, S], or ``None`` for a memory that is not sticky.  The mirror of
    ``infv_ltm_source_weights_videos``: a loop over ``source_weights``."""
    counts, cu = _video_slices(chunk_counts)
    g = int(plan.T if frames_per_source is None else frames_per_source)
    per = plan.T // g
    out = np.zeros((len(counts), int(plan.N), max(counts, default=0) * per), dtype=dtype)
    for v, n in enumerate(counts):
        if n:
            b = None if bins is None else bins[cu[v]:cu[v + 1]]
            out[v, :, :n * per] = source_weights(plan, b, n, frames_per_source=g, dtype=dtype)
    return out


def source_attention_videos(mass_trace, plan, bins, chunk_counts, frames_per_source=None, dtype=np.float64, normalise=False):
    """``source_attention`` of V packed videos: ``(W [V, N, M_max], attn [sum C_v, M_max])``, row ``cu[v] + i`` of ``attn`` being
    chunk i of video v (0 at and beyond the video's ``M_v``).  ``mass_trace`` [sum C_v, N]: one layer of the packed trace
    (``engine.trace_videos``)."""
    counts, cu = _video_slices(chunk_counts)
    g = int(plan.T if frames_per_source is None else frames_per_source)
    per = plan.T // g
    mass = np.asarray(mass_trace, dtype=np.float64)
    W = np.zeros((len(counts), int(plan.N), max(counts, default=0) * per), dtype=dtype)
    attn = np.zeros((int(cu[-1]), W.shape[2]), dtype=np.float64)
    for v, n in enumerate(counts):
        if n:
            b = None if bins is None else bins[cu[v]:cu[v + 1]]
            W[v, :, :n * per], attn[cu[v]:cu[v + 1], :n * per] = source_attention(
                mass[cu[v]:cu[v + 1]], plan, b, n, frames_per_source=g, dtype=dtype, normalise=normalise)
    return W, attn


def top_sources(attn_row, k, frames_per_source=1):
    """The k most attended sources of one row of the attention map, most attended first:
    ``[(source, first_frame, end_frame, weight), ...]`` with the source's frames ``[first_frame, end_frame)`` of the video."""
    a = np.asarray(attn_row, dtype=np.float64).reshape(-1)
    g = int(frames_per_source)
    order = np.argsort(-a, kind="stable")[:max(int(k), 0)]
    return [(int(m), int(m) * g, (int(m) + 1) * g, float(a[m])) for m in order]
