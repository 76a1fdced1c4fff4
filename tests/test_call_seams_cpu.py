"""The call layouts of tests/golden/seam_cases.py against the seam sizes parsed from csrc/: every layout crosses exactly the
seams it claims, with a probe on both sides of the ones it is there for; the videos that are re-run alone cross none; and the
oracle runs of the probes have every draw margin at MARGIN or more.  Whoever changes a seam constant gets a failure here that
names the layout, not a GPU test that silently stopped crossing anything.  No GPU needed."""
import numpy as np
import pytest

from tests.golden import seam_cases as sc

K = sc.seam_constants()
NAMES = list(sc.LAYOUTS)


def layout_problems(lay, k):
    """What is wrong with a layout under the seam sizes ``k`` (empty: nothing)."""
    bad = []
    got = sc.crossed(lay, k)
    if got != tuple(sorted(lay.claims)):
        bad.append(f"layout {lay.name}: crosses {got}, claims {tuple(sorted(lay.claims))}")
    bounds = sc.boundaries(lay, k)
    for seam in lay.probed:
        if not any(sc.straddles(lay, seam, b) for b in bounds[seam]):
            bad.append(f"layout {lay.name}: no probe has anything on both sides of a {seam} boundary (boundaries {bounds[seam][:4]})")
    for v in lay.probes + sc.spread(lay, k):
        allowed = tuple(sorted(dict(lay.alone_crosses).get(v, ())))
        alone = sc.crossed(lay.alone(v), k)
        if alone != allowed:
            bad.append(f"layout {lay.name}: video {v} alone crosses {alone}, allowed {allowed}")
    return bad


def attention_problems(k):
    a, g = sc.ATTN, k["attn_group"]
    bad = []
    if not a["nb"] > g + 1:
        bad.append(f"layout attention: nb = {a['nb']} does not reach past the group of {g}")
    if not {0, g - 1, g, g + 1} <= set(a["alone"]):
        bad.append(f"layout attention: the chunks run alone {a['alone']} miss one of 0, {g - 1}, {g}, {g + 1}")
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_layout_crosses_what_it_claims_and_nothing_else(name):
    bad = layout_problems(sc.LAYOUTS[name], K)
    assert not bad, "\n".join(bad)


def test_attention_layout_reaches_past_one_table():
    a = sc.ATTN
    assert not attention_problems(K), attention_problems(K)
    assert a["H"] == 2 and a["n_max"] == 65 and max(a["n_valid_cycle"]) == a["n_max"] and min(a["n_valid_cycle"]) == 1
    assert {31, 32, 33, 64, 65} <= set(a["n_valid_cycle"])                  # both sides of the 32-row tile edges


@pytest.mark.parametrize("seam", [s for s in K if s not in ("row_block_video",)])
def test_a_changed_constant_is_noticed(seam):
    """The checks above have teeth: with any one seam four times as large (``short_nb``: both ends), some layout reports it."""
    k = dict(K)
    k[seam] = tuple(4 * x for x in K[seam]) if isinstance(K[seam], tuple) else 4 * K[seam]
    bad = [p for lay in sc.LAYOUTS.values() for p in layout_problems(lay, k)] + attention_problems(k)
    assert bad and all(p.startswith("layout ") for p in bad), (seam, bad)


def test_the_layouts_are_what_the_seams_ask_for():
    L, k = sc.LAYOUTS, K
    rb = k["row_block"]
    a = L["vc_row_blocks"]                                                   # both first boundaries inside, a probe across each
    assert a.n_chunks >= 300 and 2 * rb < a.n_chunks and max(a.counts) == 4 and a.counts.count(0) > 0
    assert {0, 5, 17, 40} <= set(a.text_len)
    for b, p in zip((rb, 2 * rb), a.probes):
        assert sc.straddles(a, "row_block", b) == (p, p) and sc.straddles(a, "copy_rows", b) == (p, p)
        assert (a.cu[p], a.cu[p + 1]) == (b - 1, b + 2) and a.text_len[p] > 0       # chunks b-1 .. b+1, with text
        assert sc.text_rows_before(a, b) > 0                                # t0 != 0 in the block behind the boundary
        assert sc.text_rows_before(a, b - 1) > sc.text_rows_before(a, b - rb)       # ... and the videos before the probe carry text
    g = L["vc_video_groups"]
    vg = k["video_group"]
    assert len(g.counts) >= 260 and max(g.counts) <= 2 and g.shape["alpha"] == 0.75 and k["mean_table"] == vg
    assert g.probes == (vg - 1, vg, len(g.counts) - 1) and all(g.counts[p] >= 1 and g.text_len[p] > 0 for p in g.probes)
    assert sum(1 for t in g.text_len if t == 0) > len(g.text_len) // 2
    assert g.cu[vg] > 0                                                      # chunk0 of the second group is not 0
    t = L["vc_text_ffn"]
    assert t.want_hidden and t.counts == (30, 3, 2) and t.text_len == (500, 500, 7)
    assert t.shape["n_query"] + 500 <= 608
    assert sc.text_rows_before(t, 30) == 15000 < k["text_ffn"] < sc.text_rows_before(t, 33)
    m = L["vc_merge"]
    assert m.n_chunks >= 830 and m.shape["n_query"] == 40
    (p,) = m.probes
    c_seam = k["merge"] // 40
    assert k["merge"] % 40 and (m.cu[p], m.cu[p + 1]) == (c_seam - 1, c_seam + 2)      # the boundary falls inside its middle chunk
    q = L["vqf_blocks_groups"]
    assert len(q.counts) >= 260 and q.n_chunks >= 300 and q.shape["n_layers"] == 2
    assert (q.cu[q.probes[0]], q.cu[q.probes[0] + 1]) == (rb - 1, rb + 2) and q.probes[1:] == (vg - 1, vg)
    assert all(q.counts[p] >= 1 for p in q.probes)
    r = L["vqf_merge"]
    (p,) = r.probes
    assert r.n_chunks >= 1030 and k["merge"] % 32 == 0 and (r.cu[p], r.cu[p + 1]) == (k["merge"] // 32 - 1, k["merge"] // 32 + 2)


@pytest.mark.parametrize("name", NAMES)
def test_every_possible_short_attention_sub_batch_ends_inside_the_call(name):
    """``pick_short_nb`` takes a size from the range parsed out of it (which one depends on tile counts): whichever it takes,
    the call is longer, and a compared video lies wholly behind the first sub-batch."""
    lay = sc.LAYOUTS[name]
    lo, hi = K["short_nb"]
    compared = lay.probes + sc.spread(lay, K)
    for nb in range(lo, hi + 1):
        assert lay.n_chunks > nb, f"layout {name}: {lay.n_chunks} chunks fit one sub-batch of {nb}"
        assert any(lay.cu[v] >= nb for v in compared), f"layout {name}: no compared video behind the first {nb} chunks"
    assert max(v for v, n in enumerate(lay.counts) if n) in compared        # the (partial) last sub-batch is compared too


@pytest.mark.parametrize("name", NAMES)
def test_probe_oracles_keep_every_draw_margin(name):
    """The precondition of equal draws on the device, known before anything goes to the GPU."""
    lay = sc.LAYOUTS[name]
    ref = sc.probe_reference(lay)
    assert set(ref) == set(lay.probes)
    nx = sc.n_cross_of(lay.shape)
    worst = np.inf
    for p, (orun, u) in ref.items():
        n = lay.counts[p]
        assert n >= 1 and u.shape == (n, nx, sc.S) and len(orun.proj) == n
        for c in range(n):
            for j in range(nx):
                m = orun.margin[c][j]
                assert (m is None) == (c == 0), f"layout {name}: probe {p} chunk {c} cross layer {j}"     # every later chunk draws
                if m is not None:
                    worst = min(worst, float(m.min()))
                    assert float(m.min()) >= sc.MARGIN, f"layout {name}: probe {p} chunk {c} cross layer {j}: margin {m.min():.2e}"
        assert all(np.isfinite(x).all() for x in orun.proj + orun.hidden)
    u_all = sc.layout_uniforms(lay)
    for p, (_, u) in ref.items():
        assert np.array_equal(u_all[lay.cu[p]:lay.cu[p + 1]], u)             # the big call hands the probes these uniforms
