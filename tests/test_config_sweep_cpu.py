"""The configuration sweep's table (tests/golden/sweep_cases.py), checked without a GPU:

* the two independent CPU oracles (reference-shaped ``DenseOracle``, closed-form ``ClosedFormOracle``) agree at every
  point away from the S = 512, H = 12 the goldens pin them at -- so the closed-form oracle is a trustworthy definition of
  the operation for ``tests/test_config_sweep_gpu.py``;
* ``basis_maps.build_plan`` agrees with ``oracle.build_maps`` at every point (``test_plan_matches_oracle_maps`` for
  S != 512);
* the table crosses every host-side gate of the library in both directions, and what each point names as its kernel
  families is what the gates select.
"""
import numpy as np
import pytest
import torch

from infinite_video_amd import basis_maps
from oracle import ltm_oracle as O
from tests.golden import sweep_cases as sc

# The reference-shaped oracle materialises [H, Q, N, 1000] per step (LTM.py:276-282) and rebuilds its operators on every forward
# (LTM.py:298).  The rebuild depends on the chunk length alone, so the layers and chunks of a point share one (``_SharedBuild``:
# same tensors, same arithmetic).  The DENSE chain is the point's first DENSE_CHUNKS chunks -- the first chunk and two
# infinite-memory steps with their draws -- and 2 chunks where one step's integrand exceeds DENSE_ELEMS floats, for the first
# DENSE_LAYERS layers: whole chains of every layer take this file past two minutes on 8 threads (as cut: 81 s measured).  The closed-form oracle and the GPU sweep walk every point's whole chain.
DENSE_CHUNKS = 3
DENSE_LAYERS = 2                  # a layer is an oracle of its own (other weights, other query, other uniforms): two per point
DENSE_ELEMS = 40_000_000


class _SharedBuild(O.DenseOracle):
    """DenseOracle whose per-forward ``_build`` (a pure function of the chunk length and the constructor's shape) is computed
    once per chunk length and shared through ``cache``."""
    cache = None

    def _build(self, L):
        if L not in self.cache:
            super()._build(L)
            self.cache[L] = (self.G_first, self.G_inf, self.uniform_samples, self.bins)
        self.G_first, self.G_inf, self.uniform_samples, self.bins = self.cache[L]


def _agreement_points():
    return [p for p in sc.POINTS if p.d <= 1024 and max(p.Ts) <= 64]


@pytest.mark.parametrize("pt", _agreement_points(), ids=lambda p: p.name)
def test_oracles_agree(pt):
    """DenseOracle (the reference's op sequence, global generator) against ClosedFormOracle (given the same uniforms) over the
    first chunks of the point's chain (DENSE_CHUNKS above): ctx within 1e-6, B within 1e-7 (the bounds ``test_dense_port_chain_matches_reference`` holds against the reference), draws equal."""
    ks, qs, ws, u = sc.point_inputs(pt)
    n = min(pt.chunks, DENSE_CHUNKS if pt.H * pt.Q * pt.N * 1000 <= DENSE_ELEMS else 2)
    shared = {}
    worst_ctx = worst_B = 0.0
    with torch.no_grad():
        for l in range(min(pt.L, DENSE_LAYERS)):
            wk, bk, wv, bv = ws[l]
            pk, pv = torch.nn.Linear(pt.d, pt.dm), torch.nn.Linear(pt.d, pt.dm)
            pk.weight.copy_(torch.from_numpy(wk)); pk.bias.copy_(torch.from_numpy(bk))
            pv.weight.copy_(torch.from_numpy(wv)); pv.bias.copy_(torch.from_numpy(bv))
            dense = _SharedBuild(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, pk, pv, pool_shape=(pt.P,), nb_samples=pt.S)
            dense.cache = shared
            closed = O.ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, wk, bk, wv, bv, tokens_per_frame=pt.P, nb_samples=pt.S)
            for c in range(n):
                torch.manual_seed(sc.call_seed(pt, c, l))
                yd = dense.forward(torch.from_numpy(ks[c]).unsqueeze(0), torch.from_numpy(qs[l]).unsqueeze(0), new_doc=(c == 0))[0].numpy()
                yc = closed.step(ks[c], qs[l], new_doc=(c == 0), u=u[c, l])
                if c and pt.sticky:
                    np.testing.assert_array_equal(dense.last_bins.numpy(), closed.last_bins, err_msg=f"draw of chunk {c} layer {l}")
                worst_ctx = max(worst_ctx, float(np.abs(yd - yc).max()))
                worst_B = max(worst_B, float(np.abs(dense.B_past[0].numpy() - closed.B_past).max()))
    print(f"{pt.name}: max |ctx| diff {worst_ctx:.2e}, max |B| diff {worst_B:.2e} over {n} chunks x {min(pt.L, DENSE_LAYERS)} layers")
    assert worst_ctx <= 1e-6
    assert worst_B <= 1e-7


def _expand(row_box, row_begin, row_end, T):
    col = np.full(T, -1, np.int64)
    for b, s, e in zip(row_box, row_begin, row_end):
        col[s:e] = b
    return col


def _plan_keys():
    return sorted({(T, p.N, p.tau, p.S) for p in sc.POINTS for T in p.Ts} |
                  {(T, 64, tau, S) for S in (4, 100, 102, 1024) for T in (2, 300) for tau in (0.5, 0.9)})


@pytest.mark.parametrize("T,N,tau,S", _plan_keys())
def test_plans_match_oracle_maps(T, N, tau, S):
    p = basis_maps.build_plan(T, N, tau, S)
    assert not p.dense, "sweep points are sparse plans (dense ones belong to the golden cases)"
    m = O.build_maps(T, N, tau, S)
    np.testing.assert_array_equal(_expand(p.first_row_box, p.first_row_begin, p.first_row_end, T), m.first_col)
    inf_col = np.full(S + T, -1, np.int64)
    for b in range(N):
        inf_col[p.inf_old_slot[p.inf_old_ptr[b]:p.inf_old_ptr[b + 1]]] = b
    inf_col[S:] = _expand(p.inf_row_box, p.inf_row_begin, p.inf_row_end, T)
    np.testing.assert_array_equal(inf_col, m.inf_col)
    # the operator values: one 1 / (count + ridge) per box, wherever the oracle's rows land in that box
    for col, val, box_val in ((m.first_col, m.first_val, p.first_box_val), (m.inf_col, m.inf_val, p.inf_box_val)):
        keep = col >= 0
        np.testing.assert_array_equal(box_val[col[keep]], val[keep])
    np.testing.assert_array_equal(p.readout_w, m.w)
    assert p.readout_w_out == pytest.approx(m.w_out, abs=0)
    mod, edge_box, bin_box = O.sticky_bin_rows(N)
    np.testing.assert_array_equal(p.edge_box, edge_box)
    np.testing.assert_array_equal(p.bin_box, bin_box[:128])
    np.testing.assert_array_equal(p.edge_dx, (mod[1:] - mod[:-1]).astype(np.float32))
    np.testing.assert_array_equal(p.uniform_idx, m.uniform_idx)
    assert p.inf_old_ptr[-1] == len(p.inf_old_slot)
    assert inf_col[-1] == -1                                   # the last frame (t = 1.0) lies in no box


def test_named_families_are_what_the_gates_select():
    for pt in sc.POINTS:
        assert pt.families in ("fast", "stages"), pt.name
        assert sc.expected_families(pt) == pt.families, f"{pt.name} names {pt.families}, the gates select {sc.expected_path(pt)}"
        assert pt.gate, pt.name
        assert pt.chunks >= 1 and min(pt.Ts) >= 2


@pytest.mark.parametrize("gate", list(sc.GATES), ids=lambda g: g)
def test_every_gate_is_crossed_in_both_directions(gate):
    """By the one-factor part alone (the random part may be thinned), and only at points where the library evaluates the gate."""
    pred, expr, implied, where = sc.GATES[gate]
    sides = {True: [], False: []}
    for pt in sc.ONE_FACTOR:
        ps = sc._ps(pt)
        if where(pt, ps):
            sides[bool(pred(pt, ps))].append(pt.name)
    assert sides[True], f"no one-factor point passes {gate} ({expr}) where the library evaluates it"
    if implied is None:
        assert sides[False], f"no one-factor point fails {gate} ({expr}) where the library evaluates it"
    else:
        # a gate whose other side no accepted shape reaches there: the table says so, with the reason, instead of leaving a silent hole
        assert not sides[False], f"{gate}: {implied} -- but {sides[False]} fail it"
    for pt in sc.RANDOM:                                           # (the implied reasons hold in the random part too)
        ps = sc._ps(pt)
        assert implied is None or not where(pt, ps) or pred(pt, ps), f"{gate}: {implied} -- but {pt.name} fails it"


def test_implied_lds_bounds_hold_at_the_corner():
    """The three LDS bounds can only fail beyond the other terms of their gates: evaluated at the corner those terms allow."""
    assert sc.chain_lds_bytes(256, 512, 256, 16) <= 160 * 1024
    assert sc.chain_batch_lds_bytes(256, 512, 256, 16) <= 100 * 1024
    assert sc.uc_lds_bytes(256, 8, 256) <= 160 * 1024           # N * tabw <= 2048


def test_vqf_gates_are_crossed_in_both_directions():
    for name, pred in sc.VQF_GATES.items():
        got = {bool(pred(p)) for p in sc.VQF_POINTS}
        assert got == {True, False}, name
    assert len({p.name for p in sc.VQF_POINTS}) == len(sc.VQF_POINTS)


def test_table_shape():
    """Part (b) is the fixed-seed sample the table documents; part (c) lists the refusals; few enough points that the GPU
    sweep stays within its time cap."""
    assert len(sc.RANDOM) == sc.RANDOM_POINTS
    assert [r.name for r in sc.REFUSALS] == ["S1025", "S4096", "d48", "dh32", "Q_gt_max_q"]
    assert all(sc.device_bytes(p) <= 2 << 30 for p in sc.POINTS)
    assert all(p.S <= sc.MAX_NB_SAMPLES for p in sc.POINTS)
