"""The table of tests/golden/draw_edge_cases.py has the power it claims (no device).

The regimes and uniforms are built as the module's docstring says, ``inverse_cdf_draw`` equals two independent restatements of
the lower bound on them, each mistake a draw kernel could make changes at least one expected bin in the regimes it is said to,
the fp32 search against the round-up of the uniform (chain_batch3_kernel) is equivalent to the float64 compare on every
(uniform, cdf entry) pair of the table, and every routing shape selects the kernel it is there for.
"""
import numpy as np
import pytest
import torch

from oracle.ltm_oracle import categorical_probs, inverse_cdf_draw
from tests.golden import draw_edge_cases as dc
from tests.golden import sweep_cases as sc

S = 512
ALL = dc.REGIME_NAMES
NOT_ONEHOT0 = [n for n in ALL if n != "onehot_0"]


def _u(name, S_=S):
    p = dc.REGIMES[name]
    return np.concatenate([dc.edge_uniforms(p, S_, i) for i in range(dc.n_pieces(p, S_))])


def _draw_with_cdf(cdf32, u):
    """The lower bound of u in a given fp32 cdf (float64 compare)."""
    return np.searchsorted(cdf32.astype(np.float64), u, side="left")


# ---------------------------------------------------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------------------------------------------------
def test_regimes_are_the_documented_constructions():
    assert ALL == ["dense", "plateaus"] + [f"onehot_{j}" for j in (0, 7, 8, 63, 64, 126)] + \
        ["decades_asc", "decades_desc", "unnormalised_big", "unnormalised_small"]
    dense = dc.REGIMES["dense"]
    raw = dc.dense_raw()
    assert (raw > 0).all() and (dense > 0).all()
    assert np.array_equal(dense, categorical_probs(torch.from_numpy(raw)).numpy())      # normalised as the library's input is
    plat = dc.REGIMES["plateaus"]
    zero = np.zeros(dc.NB, bool)
    for lo, hi in ((0, 2), (6, 8), (15, 24), (60, 69), (120, 126)):
        zero[lo:hi + 1] = True
    assert (plat[zero] == 0).all() and np.array_equal(plat[~zero], dense[~zero])
    for j in (0, 7, 8, 63, 64, 126):
        p = dc.REGIMES[f"onehot_{j}"]
        assert p[j] == 1 and p.sum() == 1 and np.count_nonzero(p) == 1
    asc, desc = dc.REGIMES["decades_asc"], dc.REGIMES["decades_desc"]
    assert (np.diff(asc) >= 0).all() and np.array_equal(desc, asc[::-1])
    assert asc.min() >= 2.0 ** -60 and asc.max() <= 1 and asc.max() / asc.min() > 2.0 ** 40      # the sum absorbs terms
    assert np.array_equal(dc.REGIMES["unnormalised_big"], dense * np.float32(3.7))
    assert np.array_equal(dc.REGIMES["unnormalised_small"], dense * np.float32(1.3e-3))
    tiny = np.finfo(np.float32).tiny
    for name in ALL:
        p = dc.REGIMES[name]
        assert p.dtype == np.float32 and p.shape == (127,)
        assert (p[p != 0] >= tiny).all(), f"{name}: a subnormal probability"
        c = dc.oracle_cdf(p)
        assert (c[c != 0] >= tiny).all(), f"{name}: a subnormal cdf entry"


@pytest.mark.parametrize("name", ALL)
def test_edge_uniforms_are_the_documented_construction(name):
    p = dc.REGIMES[name]
    cdf = np.unique(dc.oracle_cdf(p)).astype(np.float64)
    want = set()
    for c in cdf:
        want.update((float(np.nextafter(c, -np.inf)), float(c), float(np.nextafter(c, np.inf))))
    want.update((0.0, 2.0 ** -53, 1.0 - 2.0 ** -53))
    want = {v for v in want if 0.0 <= v < 1.0}
    assert len(want) <= 384
    ev = dc.edge_values(p)
    assert set(ev.tolist()) == want and ev.size == len(want)
    if name == "dense":
        assert ev.size == 381                                   # 126 values below 1 with three doubles each, 1 - 2**-53, 0.0, 2**-53
    for S_ in (512, 102, 100):
        n = dc.n_pieces(p, S_)
        assert n == -(-ev.size // S_)
        seen = set()
        for i in range(n):
            u = dc.edge_uniforms(p, S_, i)
            assert u.shape == (S_,) and u.dtype == np.float64
            assert ((u >= 0.0) & (u < 1.0)).all()
            assert np.array_equal(u, dc.edge_uniforms(p, S_, i))             # seeded: the same values every time
            part = ev[i * S_:(i + 1) * S_]
            slots = np.nonzero(np.isin(u, part))[0]
            assert slots.size == part.size                                   # (no fill value repeats an edge value)
            # the edge values sit in as many different lanes of a wave and threads of the 256-thread kernels as there are of them:
            # in EVERY lane from 64 values on, in EVERY thread (every slot residue mod 256) from min(S, 256) on
            assert len(set((slots % 64).tolist())) == min(part.size, 64, S_)
            assert len(set((slots % 256).tolist())) == min(part.size, 256, S_)
            seen.update(set(u.tolist()) & want)
        assert seen == want, f"{name}, S = {S_}: edge values missing from the pieces"
    # S = 512 holds every edge value in one step, in both passes of the 256-thread kernels (slots below and from 256 on)
    u = dc.edge_uniforms(p, 512)
    slots = np.nonzero(np.isin(u, ev))[0]
    assert dc.count_edges(p, u) == slots.size == ev.size
    assert (slots < 256).any() and (slots >= 256).any()
    if ev.size >= 256:
        assert set((slots % 256).tolist()) == set(range(256)) and set((slots % 64).tolist()) == set(range(64))


def test_slot_order_prefixes_cover_the_lanes_and_threads():
    for S_ in (512, 102, 100, 4):
        order = dc.slot_order(S_)
        assert np.array_equal(np.sort(order), np.arange(S_)) and np.array_equal(order, dc.slot_order(S_))
        for n in range(1, S_ + 1):
            assert len(set((order[:n] % 64).tolist())) == min(n, 64, S_)
            assert len(set((order[:n] % 256).tolist())) == min(n, 256, S_)
    assert not np.array_equal(dc.slot_order(512)[:64] % 64, np.arange(64))      # (seeded, not the identity)


def test_plateau_seams_are_equal_valued_runs_of_the_cdf():
    c = dc.oracle_cdf(dc.REGIMES["plateaus"])
    assert (c[0:3] == 0).all()                                 # leading run: bins 0-2
    for lo, hi in ((6, 8), (15, 24), (60, 69), (120, 126)):
        run = c[lo - 1:hi + 1]                                 # the entry before the run and every entry of it
        assert (run == run[0]).all() and run[0] > 0, f"bins {lo}-{hi}"
    assert c[5] == c[8] and 5 // 8 != 8 // 8                    # a run across two 8-entry search groups
    assert 24 - 15 + 1 > 8                                      # a run longer than a group
    assert c[59] == c[63] == c[64] == c[69]                     # a run across the lane-63 / lane-64 carry
    assert c[119] == c[125] == c[126] == 1                      # the trailing run: the total is reached at bin 119, bins 120-126 are never drawn


# ---------------------------------------------------------------------------------------------------------------------
# the expected bins
# ---------------------------------------------------------------------------------------------------------------------
def _torch_binary_search(cdf64, x):
    """torch.multinomial's own search (aten/src/ATen/native/cpu/MultinomialKernel.cpp), written out."""
    left, right = 0, len(cdf64) - 1
    while left < right:
        mid = left + (right - left) // 2
        if cdf64[mid] < x:
            left = mid + 1
        else:
            right = mid
    return left


@pytest.mark.parametrize("name", ALL)
def test_inverse_cdf_draw_equals_independent_restatements(name):
    p = dc.REGIMES[name]
    u = _u(name)
    expect = inverse_cdf_draw(p, u)
    cdf = dc.oracle_cdf(p)
    c64 = cdf.astype(np.float64)
    count = np.minimum((c64[None, :] < u[:, None]).sum(axis=1), dc.NB - 1)      # linear count of entries below u
    assert np.array_equal(expect, count)
    assert np.array_equal(expect, np.array([_torch_binary_search(c64, x) for x in u]))
    assert np.array_equal(expect, _draw_with_cdf(cdf, u))
    assert expect.min() >= 0 and expect.max() <= dc.NB - 1
    # a drawn bin of probability zero: only u == 0.0 with a leading zero bin (torch's own behaviour)
    zero_drawn = p[expect] == 0
    assert (u[zero_drawn] == 0.0).all() and (expect[zero_drawn] == 0).all()
    assert zero_drawn.any() == (p[0] == 0)                      # (every set of uniforms holds 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the mistakes the table is there to catch
# ---------------------------------------------------------------------------------------------------------------------
def _changed(name, wrong):
    p = dc.REGIMES[name]
    u = _u(name)
    return int((inverse_cdf_draw(p, u) != np.minimum(wrong(p, u), dc.NB - 1)).sum())


def _nearest_f32_search(p, u):
    cdf = dc.oracle_cdf(p)
    return (cdf[None, :] < u.astype(np.float32)[:, None]).sum(axis=1)          # fp32 compare against round-to-nearest


def _side_right(p, u):
    return np.searchsorted(dc.oracle_cdf(p).astype(np.float64), u, side="right")


def _f64_cumsum(p, u):
    c = np.cumsum(p.astype(np.float64))
    cdf = (c / c[-1]).astype(np.float32)                                        # rounded once
    cdf[-1] = 1
    return _draw_with_cdf(cdf, u)


def _times_reciprocal(p, u):
    run = np.float32(0)
    c = np.empty(dc.NB, np.float32)
    for j in range(dc.NB):
        run = np.float32(run + p[j])
        c[j] = run
    cdf = (c * (np.float32(1) / run)).astype(np.float32)
    cdf[-1] = 1
    return _draw_with_cdf(cdf, u)


def _pairwise_scan(p, u):
    """A reassociated scan: the two halves of the wave summed on their own, the carry added at the end."""
    c = np.empty(dc.NB, np.float32)
    run = np.float32(0)
    for j in range(64):
        run = np.float32(run + p[j])
        c[j] = run
    carry, run = run, np.float32(0)
    for j in range(64, dc.NB):
        run = np.float32(run + p[j])
        c[j] = np.float32(carry + run)
    cdf = (c / c[-1]).astype(np.float32)
    cdf[-1] = 1
    return _draw_with_cdf(cdf, u)


def _dropped_carry(p, u):
    """The lane-63 -> lane-64 carry of the systolic scan lost: bins 64.. restart from zero."""
    c = np.empty(dc.NB, np.float32)
    run = np.float32(0)
    for j in range(dc.NB):
        if j == 64:
            run = np.float32(0)
        run = np.float32(run + p[j])
        c[j] = run
    cdf = (c / max(c[63], c[-1])).astype(np.float32)
    cdf[-1] = 1
    return np.minimum((cdf.astype(np.float64)[None, :] < u[:, None]).sum(axis=1), dc.NB - 1)


def _coarse_off_by_one_group(p, u):
    """A slip in the 16-coarse + 8-fine search: the coarse level reads cdf[8k] instead of cdf[8k + 7]."""
    cdf = dc.oracle_cdf(p).astype(np.float64)
    pad = np.concatenate([cdf, [2.0]])
    out = np.empty(len(u), np.int64)
    for i, x in enumerate(u):
        grp = int(sum(pad[8 * k] < x for k in range(16)))
        lo = 8 * grp
        if grp < 16:
            lo += int(sum(pad[8 * grp + t] < x for t in range(7)))
        out[i] = lo
    return out


@pytest.mark.parametrize("name", NOT_ONEHOT0)
def test_round_to_nearest_in_place_of_round_up_changes_a_bin(name):
    below_one = int((np.unique(dc.oracle_cdf(dc.REGIMES[name])) < 1).sum())
    assert _changed(name, _nearest_f32_search) >= max(1, below_one - 1)          # one per distinct cdf value below 1 (0.0 has no double below it in [0, 1))


@pytest.mark.parametrize("name", NOT_ONEHOT0)
def test_upper_bound_in_place_of_lower_bound_changes_a_bin(name):
    below_one = int((np.unique(dc.oracle_cdf(dc.REGIMES[name])) < 1).sum())
    assert _changed(name, _side_right) >= below_one                              # u == c, once per distinct cdf value below 1


def test_the_two_mistakes_change_nothing_where_the_cdf_has_no_edge_below_one():
    assert _changed("onehot_0", _nearest_f32_search) == 0 and _changed("onehot_0", _side_right) == 0


@pytest.mark.parametrize("name", ["dense", "plateaus", "decades_asc", "decades_desc", "unnormalised_big", "unnormalised_small"])
def test_a_float64_cumulative_sum_rounded_once_changes_a_bin(name):
    assert _changed(name, _f64_cumsum) >= 1


@pytest.mark.parametrize("name", ["plateaus", "decades_asc", "decades_desc", "unnormalised_big", "unnormalised_small"])
def test_multiplying_by_the_reciprocal_of_the_total_changes_a_bin(name):
    assert _changed(name, _times_reciprocal) >= 1


@pytest.mark.parametrize("name", ["dense", "plateaus", "decades_asc", "unnormalised_big", "unnormalised_small"])
def test_a_reassociated_scan_changes_a_bin(name):
    assert _changed(name, _pairwise_scan) >= 1


@pytest.mark.parametrize("name", ["dense", "plateaus", "onehot_7", "onehot_8", "onehot_63", "decades_desc", "unnormalised_big"])
def test_a_lost_wave_carry_changes_a_bin(name):
    assert _changed(name, _dropped_carry) >= 1


@pytest.mark.parametrize("name", ["dense", "plateaus", "decades_asc", "unnormalised_small"])
def test_a_slip_in_the_two_level_search_changes_a_bin(name):
    assert _changed(name, _coarse_off_by_one_group) >= 1


def test_the_two_level_search_written_out_is_the_lower_bound():
    """The kernels' search (16 coarse entries cdf[8k + 7], then 7 of the group's 8, pad 2.0, clamp) on the table's inputs."""
    for name in ALL:
        p, u = dc.REGIMES[name], _u(name)
        pad = np.concatenate([dc.oracle_cdf(p).astype(np.float64), [2.0]])
        out = np.empty(len(u), np.int64)
        for i, x in enumerate(u):
            grp = int((pad[7::8] < x).sum())
            lo = 8 * grp + (int((pad[8 * grp:8 * grp + 7] < x).sum()) if grp < 16 else 0)
            out[i] = min(lo, dc.NB - 1)
        assert np.array_equal(out, inverse_cdf_draw(p, u)), name


# ---------------------------------------------------------------------------------------------------------------------
# round_up_f32: the fp32 search of chain_batch3_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fp32_compare_against_the_round_up_equals_the_float64_compare(name):
    p = dc.REGIMES[name]
    cdf = np.concatenate([dc.oracle_cdf(p), np.float32([2.0])])                  # (with the kernels' pad entry)
    for S_ in (512, 100):
        for i in range(dc.n_pieces(p, S_)):
            u = dc.edge_uniforms(p, S_, i)
            uf = dc.round_up_f32(u)
            assert uf.dtype == np.float32
            assert (uf.astype(np.float64) >= u).all()                            # >= u ...
            prev = np.nextafter(uf, np.float32(-np.inf))
            assert ((prev.astype(np.float64) < u) | (uf == 0)).all()             # ... and the smallest such float
            assert np.array_equal(cdf[None, :] < uf[:, None], cdf.astype(np.float64)[None, :] < u[:, None])


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", list(dc.ROLE_S))
def test_role_s_shapes_select_their_kernel(kernel):
    for table in (dc.ROLE_S, dc.ROLE_S_SHORT):
        if kernel not in table:
            continue
        pt = table[kernel]
        path = sc.expected_path(pt)
        assert path.startswith(f"fast:{kernel}+"), f"{pt.name}: {path}"
        assert pt.sticky and pt.chunks == 2
    ps = sc._ps(dc.ROLE_S["chain_batch"])
    assert not sc.GATES["batch3.Q>8"][0](dc.ROLE_S["chain_batch"], ps)
    assert not sc.GATES["batch3.S%4"][0](dc.ROLE_S_SHORT["chain_batch"], sc._ps(dc.ROLE_S_SHORT["chain_batch"]))
    assert not sc.GATES["batch.wgs<=384"][0](dc.ROLE_S["chain_kernel"], sc._ps(dc.ROLE_S["chain_kernel"]))
    assert dc.ROLE_S["chain_batch3"].name == sc.SMALL.name
    assert dc.ROLE_S_SHORT["chain_batch3"].S % 4 == 0 and dc.ROLE_S_SHORT["chain_batch3"].S < 127


def test_per_call_lockstep_dense_and_psi_shapes_take_their_paths():
    from infinite_video_amd import basis_maps
    pt = dc.PER_CALL
    ps = sc._ps(pt)
    assert not ps.dense and sc.videos_supported(pt, ps) and pt.S == 512 and pt.L >= 2
    assert basis_maps.build_plan(dc.DENSE_T, dc.DENSE_N, 0.75).dense
    g = basis_maps.build_gaussian_plan(dc.GAUSS_T, dc.GAUSS_N, 0.75, dc.GAUSS_SIGMAS)
    assert g.dense and g.psi


def test_layer_regimes_cycle_through_every_regime():
    for L in (2, 6):
        seen = []
        for r in range(dc.n_rounds(L)):
            names = dc.layer_regimes(r, L)
            assert len(set(names)) == L                          # a different regime per layer
            seen += names
        assert set(seen) == set(ALL)
