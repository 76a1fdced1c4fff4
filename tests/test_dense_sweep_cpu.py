"""The dense sweep's table (tests/golden/dense_sweep_cases.py), checked without a GPU:

* every point's host plan is dense and of the family the point names; the padding of a num_basis that is no multiple of 16 is
  as ``basis_maps._build_dense_plan`` documents; the plan's operators and psi tables are the reference-shaped oracle's;
* every tile edge and mask of the eight kernels (``EDGES``) is crossed in both directions by the one-factor points;
* every point can fail for the right reason: the oracle's own chain resamples bins whose left edge lies in two boxes and in
  none, and the sticky density has weight at a two-box edge;
* the fp32 oracle is good enough to be the judge: a float64 re-evaluation of the same chain (the fp32 oracle's own operators,
  psi values and bins) lies within a quarter of the GPU test's tolerances;
* six mistakes a kernel could make, restated in numpy over the plan's tables, each change a result by more than four times its
  tolerance at the points listed beside them (``MISTAKES``).
"""
import numpy as np
import pytest
import torch

from infinite_video_amd import basis_maps
from oracle import ltm_oracle as O
from tests.golden import dense_sweep_cases as dc

CTX_TOL, B_TOL, P_RTOL = 1e-4, 2e-5, 2e-5            # tests/test_dense_sweep_gpu.py's bounds
SC_RTOL, SC_ATOL = 1e-4, 2e-5
IDS = lambda p: p.name


def _plans(pt):
    return {T: dc.plan_of(pt, T) for T in sorted(set(pt.Ts))}


# ---------------------------------------------------------------------------------------------------------------------
# the host plans
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", dc.POINTS, ids=IDS)
def test_plan_is_dense_of_the_named_family_and_matches_the_oracle(pt):
    ch = dc.oracle_chain(pt.name)
    N, Np, S = pt.N, pt.N_pad, pt.S
    psi = (lambda t: O.gaussian_membership(t, N, pt.sigmas)) if pt.sigmas else (lambda t: O.box_membership(t, N))
    bins = torch.linspace(0, 1, O.NB_BINS + 1)
    mod = bins.clone()
    mod[0], mod[-1] = -.000001, 1.000001
    t_uni = torch.arange(1, S + 1).float() * pt.tau / S / pt.tau            # LTM.py:137,155, as DenseOracle._build evaluates it
    grid = torch.linspace(0, 1, O.GRID_POINTS)
    for T, p in _plans(pt).items():
        assert dc.family_of(p, pt) == pt.family, f"{pt.name}: T {T} plans {dc.family_of(p, pt)}"
        assert p.first_GT.shape == (Np, T) and p.inf_GT.shape == (Np, S + T)
        # padding (basis_maps._build_dense_plan): zero operator rows, zero read-out weights, no table refers to the extra functions
        assert (p.N_pad or N) == Np
        assert not p.first_GT[N:].any() and not p.inf_GT[N:].any()
        if not pt.sigmas:
            assert p.readout_w.shape == (Np,) and not p.readout_w[N:].any() and (p.readout_w[:N] >= 0).all()
            for tab in (p.bin_box2, p.edge_box2, p.uniform_box2):
                assert tab.max() < N and tab.min() >= -1
                assert (tab[:, 1] < 0).all() or ((tab[:, 1] < 0) | (tab[:, 1] == tab[:, 0] + 1)).all()      # adjacent boxes, ascending
        # operators: the oracle's own (the same ATen sequence through the same LAPACK)
        G_first, G_inf = ch.G[T]
        for name, mine, ref in (("first", p.first_GT[:N], G_first.T), ("inf", p.inf_GT[:N], G_inf.T)):
            diff = float(np.abs(mine - ref).max())
            if pt.sigmas:
                # (ill-conditioned Gram matrix: the GPU test injects the oracle's G whatever this prints)
                print(f"{pt.name} T {T}: max |G_{name}(plan) - G_{name}(oracle)| = {diff:.2e} of {np.abs(ref).max():.2e}")
                assert diff <= 1e-3 * float(np.abs(ref).max())
            else:
                assert diff == 0, f"{pt.name} T {T}: plan and oracle differ in G_{name} by {diff:.2e}"
        # psi wherever the step evaluates it
        if p.psi:
            for name, mine, t in (("psi_edge", p.psi_edge, mod), ("psi_bin", p.psi_bin, bins[:-1]), ("psi_uniform", p.psi_uniform, t_uni),
                                  ("psi_grid", p.psi_grid, grid)):
                assert mine.shape == (len(t), Np), name
                np.testing.assert_array_equal(mine[:, :N], psi(t).numpy(), err_msg=f"{pt.name}: {name}")
                assert not mine[:, N:].any(), f"{pt.name}: {name} gives the padding columns weight"
            assert p.grid_w.shape == (O.GRID_POINTS,) and abs(float(p.grid_w.sum()) - 1) < 1e-6
        else:
            m = {"bin_box2": O.box_membership(bins[:-1], N), "edge_box2": O.box_membership(mod, N), "uniform_box2": O.box_membership(t_uni, N)}
            for name, memb in m.items():
                tab = getattr(p, name)
                got = np.zeros(memb.shape, np.float32)
                for j in range(2):
                    rows = np.nonzero(tab[:, j] >= 0)[0]
                    got[rows, tab[rows, j]] = 1
                np.testing.assert_array_equal(got, memb.numpy(), err_msg=f"{pt.name}: {name}")
            gm = O.box_membership(grid, N).numpy()
            assert gm.sum(1).max() <= 1, "a box2 plan whose read-out grid lies in two boxes"
            wt = np.zeros(O.GRID_POINTS)
            dx = (grid[1:] - grid[:-1]).double().numpy()
            wt[:-1] += dx / 2
            wt[1:] += dx / 2
            np.testing.assert_allclose(p.readout_w[:N], wt @ gm, rtol=0, atol=1e-9)
            assert p.readout_w_out == pytest.approx(float(wt[gm.sum(1) == 0].sum()), abs=1e-12)
        np.testing.assert_array_equal(p.edge_dx, (mod[1:] - mod[:-1]).numpy())


def test_psi01_above_256_is_the_smallest_one():
    """The table's psi01 point above 256: found by search (432 aside, whose grid the issue of the plan builder names)."""
    found = None
    for N in range(257, 512):
        if N == 432:
            continue
        p = basis_maps.build_plan(8, N, 0.75, 64)
        if p.dense and p.psi:
            found = N
            break
    assert found == dc.PSI01_ABOVE_256
    assert dc.BY_NAME[f"psi01_N{found}"].N_pad > 256


def test_gaussian_refusal_point_is_refused_on_the_host_too():
    for r in dc.REFUSALS:
        assert r.N % 16 and r.N % len(r.sigmas) == 0           # refused for the tile alone, not for the widths


# ---------------------------------------------------------------------------------------------------------------------
# the edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", list(dc.EDGES), ids=lambda e: e)
def test_every_edge_is_crossed_in_both_directions(edge):
    """By the one-factor part alone (the random part may be thinned), within the families whose kernels evaluate it."""
    pred, expr, fams, own_copies = dc.EDGES[edge]
    sides = {True: [], False: []}
    for pt in dc.ONE_FACTOR:
        if pt.family in fams:
            sides[bool(pred(pt))].append(pt.name)
    assert sides[True] and sides[False], f"{edge} ({expr}): one side is never taken: {sides}"
    if own_copies:                           # an edge both update / masses kernels have: both sides on the box and on the psi kernels
        for group in (dc.BOX, dc.PSI):
            got = {bool(pred(pt)) for pt in dc.ONE_FACTOR if pt.family in group}
            assert got == {True, False}, f"{edge} ({expr}): families {group} take only {got}"


def test_k_tails_take_every_residue_on_both_update_kernels():
    for group in (dc.BOX, dc.PSI):
        first = {pt.Ts[0] % 4 for pt in dc.ONE_FACTOR if pt.family in group}
        inf = {k % 4 for pt in dc.ONE_FACTOR if pt.family in group for k in dc._Ks(pt)[1:]}
        assert first == {0, 1, 2, 3} and inf == {0, 1, 2, 3}, (group, first, inf)
    rows = {pt.rows for pt in dc.ONE_FACTOR if pt.family in dc.PSI}
    assert {1, 3, 15, 17, 99} <= rows


def test_table_shape():
    assert len(dc.RANDOM) == dc.RANDOM_POINTS
    assert all(pt.family in ("box2", "psi01", "gauss") and pt.edge for pt in dc.POINTS)
    assert all(dc.device_bytes(pt) <= 2 << 30 for pt in dc.POINTS)
    assert all(pt.chunks in (3, 4) and min(pt.Ts) >= 2 for pt in dc.POINTS)
    assert all((pt.sigmas is not None) == (pt.family == "gauss") for pt in dc.POINTS)
    assert dc.BY_NAME[dc.OWN_PLAN_POINT].family == "gauss"
    assert {pt.dtype for pt in dc.ONE_FACTOR} == {"float32", "bfloat16", "float16"}
    assert {pt.family for pt in dc.ONE_FACTOR if not pt.sticky} == {"box2", "psi01", "gauss"}


# ---------------------------------------------------------------------------------------------------------------------
# a point can fail for the right reason
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [p for p in dc.POINTS if p.family != "gauss"], ids=IDS)
def test_special_entries_of_the_family_are_used(pt):
    ch = dc.oracle_chain(pt.name)
    p = dc.plan_of(pt, pt.T)
    if pt.family == "psi01":
        two = np.nonzero(p.psi_grid.sum(1) > 1)[0]
        assert two.size, "a psi01 plan without a grid point in two boxes"
        assert (p.grid_w[two] > 0).all()                      # the read-out of every step weighs them
        return
    tab = p.bin_box2 if pt.sticky else p.uniform_box2
    two, none = tab[:, 1] >= 0, tab[:, 0] < 0
    pos = ch.bins[1:].reshape(-1) if pt.sticky else np.arange(pt.S)
    pos = pos[pos >= 0]
    if two.any():
        assert two[pos].any(), f"{pt.name}: no resampled position lies in two boxes ({int(two.sum())} such entries)"
        assert _second_row_is_resampled(pt), f"{pt.name}: every two-box position resampled has an empty second box (a zero row of B)"
    if none.any():
        assert none[pos].any(), f"{pt.name}: no resampled position lies in no box ({int(none.sum())} such entries)"
    e2 = np.nonzero(p.edge_box2[:, 1] >= 0)[0]
    if pt.sticky and e2.size:
        # bin j - 1 and bin j take half of the density at edge j each: their probability is the weight the two-box edge carries
        e2 = e2[(e2 >= 2) & (e2 <= 126)]
        w = max(float(ch.probs[c, l, j - 1]) for c in range(1, pt.chunks) for l in range(pt.L) for j in e2)
        assert w >= 1e-3, f"{pt.name}: the two-box edges carry {w:.1e} of the sticky density"


# ---------------------------------------------------------------------------------------------------------------------
# the oracle in float64
# ---------------------------------------------------------------------------------------------------------------------
def _oracle64(pt, ch):
    """DenseOracle's chain in float64 arithmetic over the fp32 oracle's own operators, psi values and bins."""
    class D64(dc.shared_build(O.DenseOracle)):
        def __init__(self, *a, forced=None, **k):
            super().__init__(*a, **k)
            self.forced, self.at = forced, 0
            p32 = self._psi
            self._psi32, self._psi = p32, (lambda t: p32(t).double())          # psi VALUES stay the fp32 ones

        def _build(self, L):
            self._psi, keep = self._psi32, self._psi                            # operators as the fp32 oracle inverts them
            super()._build(L)
            self._psi = keep
            self.G_first, self.G_inf, self.uniform_samples = self.G_first.double(), self.G_inf.double(), self.uniform_samples.double()

        def _update(self, x):
            if self.B_past is not None:
                samples = self._psi(self.bins[torch.from_numpy(self.forced[self.at])]) if self.sticky else self.uniform_samples
                x = torch.cat([self.B_past.transpose(-1, -2).matmul(samples.transpose(-1, -2)), x], dim=2)
                B = torch.matmul(x, self.G_inf).permute(0, 2, 1)
            else:
                B = torch.matmul(x, self.G_first).permute(0, 2, 1)
            self.B_past = B.detach()
            self.at += 1
            return B

        def _density(self, t):
            sc = self._scores_at(t)
            return torch.exp(sc) / torch.trapz(torch.exp(sc), t.double(), dim=-1).unsqueeze(-1)

    ks, qs, ws, _ = dc.point_inputs(pt)
    err_ctx = err_B = 0.0
    with torch.no_grad():
        for l in range(pt.L):
            wk, bk, wv, bv = ws[l]
            o = D64(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, dc.linear(pt.d, pt.dm, wk, bk, torch.float64), dc.linear(pt.d, pt.dm, wv, bv, torch.float64),
                    pool_shape=(pt.P,), nb_samples=pt.S, gaussian_sigmas=pt.sigmas, forced=ch.bins[:, l])
            o.cache = {}
            for c in range(pt.chunks):
                y = o.forward(torch.from_numpy(ks[c]).double().unsqueeze(0), torch.from_numpy(qs[l]).double().unsqueeze(0), new_doc=(c == 0))
                err_ctx = max(err_ctx, float(np.abs(y[0].numpy() - ch.ctx[c, l]).max()))
                err_B = max(err_B, float(np.abs(o.B_past[0].numpy() - ch.B[c, l]).max()))
    return err_ctx, err_B


@pytest.mark.parametrize("pt", dc.POINTS, ids=IDS)
def test_fp32_oracle_is_within_a_quarter_of_the_tolerances_of_float64(pt):
    ch = dc.oracle_chain(pt.name)
    err_ctx, err_B = _oracle64(pt, ch)
    print(f"{pt.name}: fp32 oracle against float64: ctx {err_ctx:.2e} (max |ctx| {np.abs(ch.ctx).max():.2e}), B {err_B:.2e} (max |B| {np.abs(ch.B).max():.2e})")
    assert err_ctx <= CTX_TOL / 4 and err_B <= B_TOL / 4


# ---------------------------------------------------------------------------------------------------------------------
# restated mistakes: the device step in numpy (float64) over the plan's tables, teacher-forced with the oracle's bins
# ---------------------------------------------------------------------------------------------------------------------
def _model_chain(pt, mistake=None):
    """(ctx [chunks, L, Q, dm], B [chunks, L, N_pad, d], scores [chunks, L, H, Q, N_pad], probs [chunks, L, 127]) of the step as
    dense_step computes it, with one of MISTAKES made."""
    ks, qs, ws, _ = dc.point_inputs(pt)
    ch = dc.oracle_chain(pt.name)
    n, N, Np, H, Q, S = pt.chunks, pt.N, pt.N_pad, pt.H, pt.Q, pt.S
    ctx = np.zeros((n, pt.L, Q, pt.dm))
    Bs = np.zeros((n, pt.L, Np, pt.d))
    scs = np.zeros((n, pt.L, H, Q, Np))
    probs = np.zeros((n, pt.L, 127))
    for l in range(pt.L):
        wk, bk, wv, bv = (np.asarray(a, np.float64) for a in ws[l])
        qh = qs[l].astype(np.float64).reshape(Q, H, 64).transpose(1, 0, 2) / 8.0
        B = None
        for c, T in enumerate(pt.Ts):
            p = dc.plan_of(pt, T)
            kbar = ks[c].astype(np.float64).reshape(T, pt.P, pt.d).mean(1)
            if B is None:
                GT, x = p.first_GT, kbar
            else:
                GT = p.inf_GT
                pos = ch.bins[c, l] if pt.sticky else np.arange(S)
                if p.psi:
                    old = (p.psi_bin if pt.sticky else p.psi_uniform).astype(np.float64)[pos] @ B
                else:
                    pair = (p.bin_box2 if pt.sticky else p.uniform_box2)[pos]
                    old = np.where(pair[:, :1] >= 0, B[np.maximum(pair[:, 0], 0)], 0.0)
                    if mistake != "row_second_box":                      # dense_update_kernel: b += Bp[b1]
                        old = old + np.where(pair[:, 1:] >= 0, B[np.maximum(pair[:, 1], 0)], 0.0)
                x = np.concatenate([old, kbar])
            K = GT.shape[1]
            if mistake == "k_tail":                                      # the update kernels' loop as k0 + 4 <= K
                K -= K % 4
            B = GT[:, :K].astype(np.float64) @ x[:K]
            Kp, V = B @ wk.T + bk, B @ wv.T + bv
            s = np.einsum("hqc,nhc->hqn", qh, Kp.reshape(Np, H, 64))
            Vh = V.reshape(Np, H, 64).transpose(1, 0, 2)
            dx = p.edge_dx.astype(np.float64)
            if p.psi:
                grid = p.psi_grid.astype(np.float64)
                if mistake == "pad_weight" and Np != N:                  # padding columns as one more real basis function
                    grid = grid.copy()
                    grid[:, N:] = grid[:, :N].mean(1, keepdims=True)
                gw = np.ones(len(grid)) if mistake == "grid_w" else p.grid_w.astype(np.float64)        # psi_grid_kernel: w[i]
                z = s @ p.psi_grid.astype(np.float64).T
                pr = gw * np.exp(z - z.max(-1, keepdims=True))
                alpha = (pr / pr.sum(-1, keepdims=True)) @ grid
                E = s @ p.psi_edge.astype(np.float64).T
            else:
                w = p.readout_w.astype(np.float64).copy()
                if mistake == "pad_weight" and Np != N:
                    w[N:] = w[:N].mean()
                e = w * np.exp(s)
                alpha = e / (e.sum(-1, keepdims=True) + p.readout_w_out)
                eb = p.edge_box2
                E = np.where(eb[:, 0] >= 0, s[..., np.maximum(eb[:, 0], 0)], 0.0)
                if mistake != "edge_second_box":                         # dense_masses_kernel: s += row[b1]
                    E = E + np.where(eb[:, 1] >= 0, s[..., np.maximum(eb[:, 1], 0)], 0.0)
            ctx[c, l] = np.einsum("hqn,hnc->qhc", alpha, Vh).reshape(Q, pt.dm)
            Bs[c, l], scs[c, l] = B, s
            D = np.exp(E - E.max(-1, keepdims=True))
            zt = ((D[..., :-1] + D[..., 1:]) * dx).sum(-1, keepdims=True) / 2
            dxm = dx[0:127] if mistake == "edge_dx" else dx[1:128]       # the masses kernels: edge_dx[lane] for edge_dx[lane + 1]
            mass = ((D[..., 1:128] + D[..., 2:129]) / 2 * dxm / zt).sum((0, 1))
            if c + 1 < n:
                probs[c + 1, l] = mass / mass.sum()
    return ctx, Bs, scs, probs


def _excess(pt, a, b):
    """How far two results of the model are apart, in units of the GPU test's tolerances: the largest of ctx, B, scores, probs."""
    ctx = np.abs(a[0] - b[0]).max() / CTX_TOL
    B = np.abs(a[1] - b[1]).max() / B_TOL
    sc = (np.abs(a[2] - b[2]) / (SC_ATOL + SC_RTOL * np.abs(b[2]))).max()
    pr = 0.0
    if pt.sticky:
        pr = np.abs(a[3][1:] / b[3][1:] - 1).max() / P_RTOL
    return dict(ctx=float(ctx), B=float(B), scores=float(sc), probs=float(pr))


def _two_box_rows(pt):
    p = dc.plan_of(pt, pt.T)
    return pt.family == "box2" and bool(((p.bin_box2 if pt.sticky else p.uniform_box2)[:, 1] >= 0).any())


def _second_row_is_resampled(pt):
    """The oracle's chain resamples a position in two boxes whose SECOND box holds a non-zero row of B (a box no sample position
    falls into has an exactly zero row: G's column for it is zero)."""
    ch = dc.oracle_chain(pt.name)
    for c in range(1, pt.chunks):
        tab = dc.plan_of(pt, pt.Ts[c])
        tab = tab.bin_box2 if pt.sticky else tab.uniform_box2
        for l in range(pt.L):
            b1 = tab[ch.bins[c, l] if pt.sticky else np.arange(pt.S), 1]
            if ch.B[c - 1, l][b1[b1 >= 0]].any():
                return True
    return False


# mistake -> the points it must change by more than four tolerances: every point of the table where the mistaken term is not
# trivially absent, but for the few named in WEAK, where the model shows the change to be smaller (figures: multiples of the
# tolerance of ctx, the only result these two mistakes move)
MISTAKES = {
    "row_second_box": _two_box_rows,
    "edge_second_box": lambda pt: pt.family == "box2" and pt.sticky and bool((dc.plan_of(pt, pt.T).edge_box2[:, 1] >= 0).any()),
    "k_tail": lambda pt: any(k % 4 for k in dc._Ks(pt)),
    "edge_dx": lambda pt: pt.sticky,
    "grid_w": lambda pt: pt.family == "gauss",
    "pad_weight": lambda pt: pt.N_pad != pt.N,
}
WEAK = {
    # the trapezoid weights differ from a constant at the grid's two end points only: 1e-3 of the density's mass there, times how
    # far the values at the ends are from the context -- least with one or three widths at N 16 / 48 and at small shapes
    "grid_w": {"gauss_N16_1sigma": 3.6, "gauss_N48_3sigma": 2.6, "rand00": 2.3, "rand02": 3.0, "rand10": 3.8},
    # one padding column of 48 carries 2% of the softmax weight, four of 304 1.3%, and its value row is the bias bv, which the
    # contexts of these synthetic weights stay close to (|ctx - bv| is a few 1e-3): the GPU sweep cannot see this mistake in the
    # read-out at N 300, and sees it with less than four tolerances at N 47; N 17 and the psi01 points see it 9 to 400-fold
    "pad_weight": {"N47": 3.9, "N300": 0.3},
}


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(pt, mistake=None):
        if (pt.name, mistake) not in cache:
            cache[(pt.name, mistake)] = _model_chain(pt, mistake)
        return cache[(pt.name, mistake)]
    return get


@pytest.mark.parametrize("pt", dc.POINTS, ids=IDS)
def test_model_of_the_step_agrees_with_the_oracle(pt, models):
    """The numpy model the mistakes are made in is the oracle's step, well within the tolerances, padding inert."""
    ch = dc.oracle_chain(pt.name)
    ctx, B, s, probs = models(pt)
    N = pt.N
    assert np.abs(ctx - ch.ctx).max() <= CTX_TOL / 4
    assert np.abs(B[:, :, :N] - ch.B).max() <= B_TOL / 4 and not B[:, :, N:].any()
    np.testing.assert_allclose(s[..., :N], ch.scores, rtol=SC_RTOL / 4, atol=SC_ATOL / 4)
    if pt.sticky:
        # (half, not a quarter: the fp32 oracle takes a bin's mass as the difference of two entries of a cumulative trapezoid that
        #  runs up to 1 -- an absolute 2^-24 on a mass of ~1/127, 7.6e-6 relative, before any sum over heads and queries averages it)
        assert np.abs(probs[1:] / ch.probs[1:] - 1).max() <= P_RTOL / 2


@pytest.mark.parametrize("mistake", list(MISTAKES), ids=lambda m: m)
def test_restated_mistake_changes_the_result_beyond_four_tolerances(mistake, models):
    pts = [pt for pt in dc.POINTS if MISTAKES[mistake](pt)]
    assert len([pt for pt in pts if pt in dc.ONE_FACTOR and pt.name not in WEAK.get(mistake, {})]) >= 3, f"{mistake}: too few one-factor points can see it"
    weak = WEAK.get(mistake, {})
    assert set(weak) <= {pt.name for pt in pts}
    for pt in pts:
        ex = _excess(pt, models(pt, mistake), models(pt))
        print(f"{mistake} at {pt.name}: " + ", ".join(f"{k} x{v:.1f}" for k, v in ex.items()) + " of the tolerance")
        if pt.name in weak:
            assert max(ex.values()) == pytest.approx(weak[pt.name], rel=0.25), f"{mistake} at {pt.name}: the figure beside it is stale: {ex}"
        else:
            assert max(ex.values()) > 4, f"{mistake} at {pt.name} stays within four tolerances: {ex}"
