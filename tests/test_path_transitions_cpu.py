"""The table of tests/golden/transition_cases.py itself: every ordered pair of the six operations, every hand-off and variant is
there under a unique name; each shape lands on the kernel path it is there for (by the gates of sweep_cases.py); every oracle
run keeps every draw margin, so the GPU test may demand equal draws without leaving one out; and the whole table's oracle work
stays cheap.  No GPU needed."""
import time

import numpy as np
import pytest

from tests.golden import seam_cases
from tests.golden import sweep_cases as sw
from tests.golden import transition_cases as tc


def _have(**kw):
    return [s for s in tc.SEQUENCES if all(getattr(s, k) == v for k, v in kw.items())]


def test_every_ordered_pair_is_present_at_fast():
    plain = {(s.x, s.y) for s in _have(shape="fast", handoff=None, variant=None)}
    assert plain == {(x, y) for x in tc.OPS for y in tc.OPS} and len(plain) == 36
    assert len(tc.OPS) == 6 and set(tc.PER_CHUNK_Q) | set(tc.LOCKSTEP) | set(tc.TRACED) | set(tc.CHAIN_EXPORTERS) <= set(tc.OPS)


def test_the_other_shapes_hold_the_pairs_the_plan_lists():
    with_fwd_or_cons = {(x, y) for x in tc.OPS for y in tc.OPS if "fwd" in (x, y) or "cons" in (x, y)}
    assert len(with_fwd_or_cons) == 20
    for shape in ("fast_tabw4", "stages"):
        assert {(s.x, s.y) for s in _have(shape=shape)} == with_fwd_or_cons, shape
        assert all(s.handoff is None and s.variant is None for s in _have(shape=shape))
    assert {(s.x, s.y) for s in _have(shape="uniform")} == {(x, "cons") for x in tc.OPS}


def test_every_handoff_and_variant_is_present():
    three = ("fwd", "cons", "vid")
    assert {(s.x, s.y) for s in _have(handoff="state")} == {(x, y) for x in three for y in three}
    chain = {(s.x, s.y) for s in _have(handoff="chain")}
    assert chain == {("cons", y) for y in tc.OPS} | {("pooled", "cons")}
    assert all(s.x in tc.CHAIN_EXPORTERS and s.shape == "fast" for s in _have(handoff="chain"))   # legal only there
    assert all(s.shape == "fast" and s.variant is None for s in tc.SEQUENCES if s.handoff)
    for v in tc.VARIANTS:
        assert {(s.x, s.y) for s in _have(variant=v)} == set(tc.VARIANT_PAIRS), v
        assert all(s.shape == "fast" and s.handoff is None for s in _have(variant=v))
    assert set(tc.VARIANT_PAIRS) == {("fwd", "cons"), ("cons", "cons"), ("vid", "cons"), ("cons", "vid"), ("cons", "cons_q")}


def test_sequence_names_are_unique():
    names = [s.name for s in tc.SEQUENCES] + [s.name for s in tc.DENSE_SEQUENCES]
    assert len(set(names)) == len(names)
    assert tc.BY_NAME.keys() == {s.name for s in tc.SEQUENCES}


def test_the_documents_and_legs_are_what_the_plan_asks_for():
    assert tc.DOC_LEGS == ((3, 3, 1), (1, 2, 1)) and tc.MAX_BATCH_CHUNKS == 2
    for s in tc.SEQUENCES:
        assert tc.SHAPES[s.shape].max_batch_chunks == 2          # a 3-chunk leg spans two sub-batches
        for doc, want in enumerate(tc.DOC_LEGS):
            x, y, z = tc.legs_of(s, doc)
            assert (len(x.chunks), len(y.chunks), len(z.chunks)) == want
            assert x.chunks + y.chunks + z.chunks == tuple(range(sum(want)))
            assert (x.op, y.op, z.op) == (s.x, s.y, "fwd") and x.new_doc and not y.new_doc and not z.new_doc
            for leg in (x, y, z):
                assert {k for k, _, _ in leg.q} == {"chunk" if leg.op in tc.PER_CHUNK_Q else "shared"}
    # document B's first leg is the document's first chunk alone
    assert tc.DOC_LEGS[1][0] == 1


def test_the_variants_change_what_they_name_and_nothing_else():
    base = tc.BY_NAME["fast:cons-cons"]
    for v, field in (("q32_q16", "Q"), ("q16_q32", "Q"), ("qvals", "values"), ("weights", "w")):
        s = tc.BY_NAME[f"fast:cons-cons:{v}"]
        (x, y, z), (bx, by, bz) = tc.legs_of(s, 0), tc.legs_of(base, 0)
        assert z.q == bz.q                                       # the closing fwd always asks with the base query
        got = dict(Qx=x.q[0][1], Qy=y.q[0][1], vx=x.q[0][2], vy=y.q[0][2], wx=x.w, wy=y.w, wz=z.w)
        want = dict(Qx=32, Qy=32, vx=0, vy=0, wx=0, wy=0, wz=0)
        want.update({"q32_q16": dict(Qy=16), "q16_q32": dict(Qx=16), "qvals": dict(vy=1), "weights": dict(wy=1, wz=1)}[v])
        assert got == want, (v, got)
    pt = tc.SHAPES["fast"]
    assert not np.array_equal(tc.query(pt, ("shared", 32, 0), 0, 0), tc.query(pt, ("shared", 32, 1), 0, 0))
    assert not np.array_equal(tc.query(pt, ("chunk", 32, 0), 0, 3), tc.query(pt, ("chunk", 32, 0), 0, 4))
    assert not np.array_equal(tc.weights(pt, 0)[0][0], tc.weights(pt, 1)[0][0])


@pytest.mark.parametrize("claim", list(tc.CLAIMS))
def test_each_shape_lands_on_the_path_it_names(claim):
    pt = tc.claimed_point(claim)
    families, path_parts = tc.CLAIMS[claim]
    assert sw.expected_families(pt) == families, (claim, sw.expected_families(pt))
    path = sw.expected_path(pt) + "+"
    assert all(part in path for part in path_parts), (claim, path)
    ps = sw._ps(pt)
    assert sw.videos_supported(pt, ps) and not ps.dense          # `vid` / `vid_q` run the lockstep kernels at every shape
    if claim == "stages":
        assert not sw.fast_path(pt, ps) and (pt.L * pt.H * pt.Q) == 192
    if claim == "fast_q16":
        assert sw.fast_path(pt, ps) and (pt.L * pt.H * pt.Q) == 128
    if claim == "fast_tabw4":
        assert ps.tabw == 4 and sw.uc_fast_supported(pt, ps)
    if claim == "fast":
        assert ps.tabw != 4 and not sw.uc_fast_supported(pt, ps) and (pt.L * pt.H * pt.Q) == 256


def test_every_shape_value_is_a_one_factor_point_of_the_sweep():
    """... but H 4, which the sweep brackets (H 2 and H 8 on the fused chain, H 3 and H 5 off it): with L 2 it is what puts
    Q 32 and Q 16 both on a multiple of 128 rows."""
    heads = {p.H for p in sw.ONE_FACTOR}
    for pt in tc.SHAPES.values():
        for f in ("N", "d", "P", "S", "T", "L", "Q"):
            assert any(getattr(p, f) == getattr(pt, f) for p in sw.ONE_FACTOR), (pt.name, f)
        assert pt.H in heads or (pt.H == 4 and {2, 3, 5, 8} <= heads), pt.name


def test_dense_sequences_cut_every_sticky_golden_everywhere():
    assert tc.DENSE_STICKY and all(c.dense and c.sticky for c in tc.DENSE_STICKY)
    for c in tc.DENSE_STICKY:
        mine = [s for s in tc.DENSE_SEQUENCES if s.case == c.name]
        assert {s.cut for s in mine} == set(range(1, len(c.chunk_T)))
        assert {(s.x, s.y) for s in mine if s.cut == 1} == {(x, y) for x in tc.DENSE_OPS for y in tc.DENSE_OPS}
    assert set(tc.DENSE_OPS) == {"fwd", "cons", "cons_q", "vid"}


def test_oracle_runs_keep_every_margin_leave_no_draw_out_and_stay_cheap():
    """The precondition of `every drawn bin equal` on the device, and the cost of the table: all of its oracle work, measured
    here, must stay under about 30 s (it took 5.3 s when the table was written)."""
    assert tc.MARGIN is seam_cases.MARGIN and tc.draw_margins is seam_cases.draw_margins and tc.MARGIN == 2e-5
    tc._runs.clear()
    t0 = time.perf_counter()
    keys = tc.run_keys()
    runs = [(s, doc, tc.oracle_run(s, doc)) for s, doc in keys]
    took = time.perf_counter() - t0
    draws = excluded = 0
    for s, doc, r in runs:
        pt = tc.SHAPES[s.shape]
        n = sum(tc.DOC_LEGS[doc])
        assert len(r.ctx) == len(r.B) == n and all(np.isfinite(x).all() for x in r.ctx + r.B)
        for c in range(n):
            draws_here = pt.sticky and c > 0
            assert (r.u[c] is not None) == draws_here and (r.bins[c] is not None) == draws_here, (s.name, doc, c)
            if draws_here:
                assert r.u[c].shape == (pt.L, pt.S) and r.margin[c] >= tc.MARGIN, f"{s.name} doc {doc} chunk {c}: margin {r.margin[c]:.2e}"
        assert r.draws == (n - 1) * pt.L * pt.S * int(pt.sticky)
        draws += r.draws
        excluded += r.excluded
    assert draws > 100000 and excluded == 0, f"{excluded} of {draws} draws would have to be left out"
    assert excluded / draws == 0.0                                # the share of excluded draws
    # every sequence finds its runs in the cache: the 36 pairs of `fast` share four runs per document
    assert len(keys) <= 48 and len({(s.shape, d, tc.schedule_of(s, d)) for s in tc.SEQUENCES for d in (0, 1)}) == len(keys)
    plain = {tc.schedule_of(s, d) for s in tc.SEQUENCES if s.shape == "fast" and not s.variant and not s.handoff for d in (0,)}
    assert len(plain) == 4
    assert took < 30.0, f"the table's oracle work took {took:.1f} s"


def test_swapping_the_oracles_weights_is_a_reprojection():
    """The weights variant swaps ``wk/bk/wv/bv`` of the oracle between two steps.  That equals an oracle built with the new
    weights and handed the old memory and scores: ``step`` derives K and V from ``B_past`` each time and keeps nothing else
    that depends on the weights but ``S_prev``, which is the OLD weights' on purpose (the draw follows the last attention)."""
    from oracle.ltm_oracle import ClosedFormOracle
    pt = tc.SHAPES["fast"]
    w0, w1 = tc.weights(pt, 0)[0], tc.weights(pt, 1)[0]
    q = tc.query(pt, ("shared", pt.Q, 0), 0, 0)[0]
    u = np.random.default_rng(5).random(pt.S)
    a = ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, True, *w0, tokens_per_frame=pt.P)
    a.step(tc.tokens(pt, 0, 0), q, True)
    b = ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, True, *w1, tokens_per_frame=pt.P)
    b.B_past, b.S_prev = a.B_past.copy(), a.S_prev.copy()
    a.wk, a.bk, a.wv, a.bv = (np.asarray(x, np.float32) for x in w1)
    ya, yb = a.step(tc.tokens(pt, 0, 1), q, False, u=u), b.step(tc.tokens(pt, 0, 1), q, False, u=u)
    assert np.array_equal(ya, yb) and np.array_equal(a.B_past, b.B_past) and np.array_equal(a.S_prev, b.S_prev)
    c = ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, True, *w0, tokens_per_frame=pt.P)
    c.step(tc.tokens(pt, 0, 0), q, True)
    assert not np.allclose(c.step(tc.tokens(pt, 0, 1), q, False, u=u), ya, atol=1e-3)     # ... and the weights do matter


# ------------------------------------------------------------------------------------------------ the video Q-former section
def test_vqf_table_holds_all_nine_pairs_and_the_epoch_sequences():
    plain = {(s.x, s.y) for s in tc.VQF_SEQUENCES if not s.epoch}
    assert plain == {(x, y) for x in tc.VQF_OPS for y in tc.VQF_OPS} and len(plain) == 9
    assert tc.VQF_OPS == ("chunk", "video", "videos") and tc.VQF_LEGS == (2, 2, 1) and tc.VQF_VIDEOS == 2
    assert [s.name for s in tc.VQF_SEQUENCES if s.epoch] and len({s.name for s in tc.VQF_SEQUENCES}) == len(tc.VQF_SEQUENCES)
    assert all(s.y == "chunk" for s in tc.VQF_SEQUENCES if s.epoch)          # encode_chunk is what reuses the cached prefix


@pytest.mark.parametrize("epoch", (False, True))
def test_vqf_oracle_runs_keep_every_margin(epoch):
    nx, n = seam_cases.n_cross_of(seam_cases.VQF_BASE), sum(tc.VQF_LEGS)
    ref = tc.vqf_reference(epoch)
    assert len(ref) == tc.VQF_VIDEOS
    for v, (orun, u) in enumerate(ref):
        assert u.shape == (n, nx, seam_cases.S) and len(orun.proj) == len(orun.hidden) == n
        for c in range(n):
            for j in range(nx):
                m = orun.margin[c][j]
                assert (m is None) == (c == 0)
                assert m is None or float(m.min()) >= tc.MARGIN, f"video {v} chunk {c} layer {j}: margin {m.min():.2e}"
    # the changed prefix weight matters from the first chunk of leg Y on, and not before
    plain, changed = tc.vqf_reference(False)[0][0], tc.vqf_reference(True)[0][0]
    c0 = tc.VQF_LEGS[0]
    assert all(np.array_equal(plain.proj[c], changed.proj[c]) for c in range(c0))
    assert float(np.abs(plain.proj[c0] - changed.proj[c0]).max()) > 1e-2
