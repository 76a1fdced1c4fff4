"""Several independent videos in one call (infv_ltm_consolidate_videos / engine.consolidate_videos) on the MI355X: goldens
inside a batch, batch and split invariance bit for bit, agreement with the single-video path, fallback and refusals."""
import numpy as np
import pytest
import torch

from oracle import ltm_oracle as O
from tests.conftest import record_parity
from tests.golden.cases import CASES, DENSE_CASES, call_uniforms, case_inputs, load_golden

pytestmark = pytest.mark.gpu

CTX_TOL = 1e-4
B_TOL = 2e-5
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _engine(case, dev, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(case.N, case.H, case.dh, case.d, case.P, tau=case.tau, sticky=case.sticky, n_layers=case.n_layers,
                     max_q=case.Q, device=dev, **kw)


def _to(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _golden_video(case):
    ks, qs, ws = case_inputs(case)
    u = np.stack([np.stack([call_uniforms(case, c, l) for l in range(case.n_layers)]) for c in range(len(ks))])
    return np.stack(ks), u, qs, ws


def _batch(case, lens, first_video=0):
    from infinite_video_amd import synth
    T = case.chunk_T[0]
    return synth.video_batch(lens, T, case.P, case.d, case.n_layers, first_video=first_video)


def _run(dev, engines, ks, us, q, projs, new_doc=True):
    from infinite_video_amd.engine import consolidate_videos
    counts = [len(k) for k in ks]
    k = torch.from_numpy(np.concatenate(ks)).to(dev)
    u = torch.from_numpy(np.concatenate(us)).to(dev)
    ctx = consolidate_videos(engines, k, counts, q, projs, u, new_doc=new_doc)
    torch.cuda.synchronize()
    cu = np.concatenate([[0], np.cumsum(counts)])
    return [ctx[cu[v]:cu[v + 1]] for v in range(len(ks))]


@pytest.mark.parametrize("name", ["cfg1_sticky", "peaked", "headline", "cfg1_uniform"])
def test_goldens_inside_a_batch(dev, name):
    """The golden video at position 2 of a batch of synthetic videos of 0, 1, 3 and 8 chunks: it reproduces the reference's
    drawn bins, ctx and B; every synthetic video matches the closed-form oracle free-running."""
    case = BY_NAME[name]
    g = load_golden(case)
    kg, ug, qs, ws = _golden_video(case)
    syn_k, syn_u = _batch(case, [0, 1, 3, 8], first_video=10)
    ks = syn_k[:2] + [kg] + syn_k[2:]
    us = syn_u[:2] + [ug] + syn_u[2:]
    engines = [_engine(case, dev) for _ in ks]
    traces = [e.set_trace(len(k)) if case.sticky else None for e, k in zip(engines, ks)]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    ctxs = _run(dev, engines, ks, us, q, projs)
    for v, (e, k, u, ctx) in enumerate(zip(engines, ks, us, ctxs)):
        ctx = ctx.cpu().numpy()
        orc = [O.ClosedFormOracle(case.N, case.H, case.dh, case.tau, case.sticky, *ws[l], tokens_per_frame=case.P)
               for l in range(case.n_layers)]
        for c in range(len(k)):
            for l in range(case.n_layers):
                ref = orc[l].step(k[c], qs[l], new_doc=(c == 0), u=u[c, l])
                np.testing.assert_allclose(ctx[c, l], ref, rtol=0, atol=CTX_TOL)
                if case.sticky and c > 0:
                    bins = traces[v][0][c, l].cpu().numpy()
                    assert (bins == orc[l].last_bins).all(), f"video {v} chunk {c} layer {l}: {(bins != orc[l].last_bins).sum()} flips"
                if v == 2:
                    tag = f"c{c}_l{l}"
                    np.testing.assert_allclose(ctx[c, l], g[tag + "_ctx"], rtol=0, atol=CTX_TOL)
                    if case.sticky and c > 0:
                        np.testing.assert_array_equal(traces[v][0][c, l].cpu().numpy(), g[tag + "_bins"])
        for l in range(case.n_layers):
            if len(k):
                B = e.export_state(l)[0].cpu().numpy()
                np.testing.assert_allclose(B, orc[l].B_past, rtol=0, atol=B_TOL)
                if v == 2:
                    tag = f"c{len(k) - 1}_l{l}"
                    want = g[tag + "_B"] if case.store_full_B else None
                    if want is not None:
                        np.testing.assert_allclose(B, want, rtol=0, atol=B_TOL)
                    else:
                        np.testing.assert_allclose(B[::16], g[tag + "_Brows"], rtol=0, atol=B_TOL)
            else:
                assert not e.has_memory


def _state(e, case):
    out = []
    for l in range(case.n_layers):
        B, _ = e.export_state(l)
        bins, _, probs = e.last_draw(l)
        out.append((B.cpu(), bins.copy(), probs.copy(), e.last_scores(l, case.Q).copy()))
    return out


def _equal_states(a, b):
    for (Ba, ba, pa, sa), (Bb, bb, pb, sb) in zip(a, b):
        assert torch.equal(Ba, Bb)
        np.testing.assert_array_equal(ba, bb)
        np.testing.assert_array_equal(pa, pb)
        np.testing.assert_array_equal(sa, sb)


def test_batch_invariance_bit_for_bit(dev):
    """One video alone, at position 0 and at position 6 of a batch of 7, and beside videos of other lengths: same bits."""
    case = BY_NAME["cfg1_sticky"]
    kg, ug, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    others_k, others_u = _batch(case, [8, 5, 2, 8, 1, 6], first_video=20)
    runs = {"alone": ([kg], [ug], 0), "first": ([kg] + others_k, [ug] + others_u, 0),
            "last": (others_k + [kg], others_u + [ug], 6)}
    short_k, short_u = _batch(case, [3, 0, 12], first_video=30)
    runs["ragged"] = (short_k[:1] + [kg] + short_k[1:], short_u[:1] + [ug] + short_u[1:], 1)
    res = {}
    for tag, (ks, us, pos) in runs.items():
        engines = [_engine(case, dev) for _ in ks]
        ctx = _run(dev, engines, ks, us, q, projs)[pos]
        res[tag] = (ctx.cpu(), _state(engines[pos], case))
    for tag in ("first", "last", "ragged"):
        assert torch.equal(res[tag][0], res["alone"][0]), tag
        _equal_states(res[tag][1], res["alone"][1])


def test_split_invariance(dev):
    """Chunks [0, 4) with new_doc = 1 then [4, 8) with new_doc = 0 equal one call over [0, 8), bit for bit."""
    case = BY_NAME["cfg1_sticky"]
    ks, us = _batch(case, [8, 8, 8], first_video=40)
    _, _, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    whole = [_engine(case, dev) for _ in ks]
    ctx_w = _run(dev, whole, ks, us, q, projs)
    split = [_engine(case, dev) for _ in ks]
    ctx_a = _run(dev, split, [k[:4] for k in ks], [u[:4] for u in us], q, projs, new_doc=True)
    ctx_b = _run(dev, split, [k[4:] for k in ks], [u[4:] for u in us], q, projs, new_doc=False)
    for v in range(len(ks)):
        assert torch.equal(torch.cat([ctx_a[v], ctx_b[v]]).cpu(), ctx_w[v].cpu())
        _equal_states(_state(split[v], case), _state(whole[v], case))


@pytest.mark.parametrize("name", ["cfg1_sticky", "peaked", "headline"])
def test_matches_the_single_video_path(dev, name):
    """Per video equal to LTMEngine.consolidate on the same inputs (test_consolidate_equals_per_chunk_forward's tolerances);
    afterwards one more per-video forward() continues from the batched state and matches the oracle."""
    case = BY_NAME[name]
    kg, ug, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    ks, us = _batch(case, [2, len(kg)], first_video=50)
    ks, us = [kg] + ks, [ug] + us
    engines = [_engine(case, dev) for _ in ks]
    ctxs = _run(dev, engines, ks, us, q, projs)
    for v, (k, u) in enumerate(zip(ks, us)):
        single = _engine(case, dev)
        ref = single.consolidate(torch.from_numpy(k).to(dev), q, projs, torch.from_numpy(u).to(dev), new_doc=True)
        np.testing.assert_allclose(ctxs[v].cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-5)
        for l in range(case.n_layers):
            np.testing.assert_allclose(engines[v].export_state(l)[0].cpu().numpy(), single.export_state(l)[0].cpu().numpy(),
                                       rtol=0, atol=1e-6)
            np.testing.assert_array_equal(engines[v].last_draw(l)[0], single.last_draw(l)[0])
    # the state lives in the handles: one more chunk through the per-video forward() matches the oracle
    from infinite_video_amd import synth
    v = 1
    orc = [O.ClosedFormOracle(case.N, case.H, case.dh, case.tau, case.sticky, *ws[l], tokens_per_frame=case.P)
           for l in range(case.n_layers)]
    for c in range(len(ks[v])):
        for l in range(case.n_layers):
            orc[l].step(ks[v][c], qs[l], new_doc=(c == 0), u=us[v][c, l])
    k_next = synth.frame_tokens(99, case.chunk_T[0], case.P, case.d, seed=777)
    u_next = synth.gibbs_uniforms(1, case.n_layers, seed=778)[0]
    ctx = engines[v].forward(torch.from_numpy(k_next).to(dev), q, projs, torch.from_numpy(u_next).to(dev), new_doc=False)
    for l in range(case.n_layers):
        np.testing.assert_allclose(ctx[l].cpu().numpy(), orc[l].step(k_next, qs[l], new_doc=False, u=u_next[l]), rtol=0,
                                   atol=CTX_TOL)


def test_scale_64_videos_of_32_chunks(dev):
    """64 videos x 32 chunks at the headline shape (T 256, N 256, L 2, Q 32; 64 videos per step, 4096-row projections), tokens
    made on the device.  Four videos carry armed traces; each is walked by the CPU oracle teacher-forced on its own traced bins
    (test_timed_path_gpu.py's check): ctx within 1e-4 on every chunk, the oracle's own probabilities within 2e-5 relative, its
    own draw equal to the traced bins but for a budget of adjacent-bin flips, final B within 2e-5."""
    from concurrent.futures import ThreadPoolExecutor
    from infinite_video_amd.engine import LTMEngine, consolidate_videos
    from infinite_video_amd import synth
    V, C, T, N, L, Q, P, d, dm, H, S = 64, 32, 256, 256, 2, 32, 32, 768, 768, 12, 512
    gen = torch.Generator(device=dev).manual_seed(5)
    k = torch.randn(V * C, T * P, d, device=dev, generator=gen)
    u = torch.rand(V * C, L, S, device=dev, dtype=torch.float64, generator=gen)
    ws = [synth.layer_projections(l, d, dm, seed=synth.SEED_W + 5000) for l in range(L)]
    qs = [synth.layer_query(l, Q, dm, seed=synth.SEED_Q + 5000) for l in range(L)]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    engines = [LTMEngine(N, H, 64, d, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev) for _ in range(V)]
    watched = [0, 21, 42, 63]
    traces = {v: engines[v].set_trace(C) for v in watched}
    ctx = consolidate_videos(engines, k, [C] * V, q, projs, u, new_doc=True)
    torch.cuda.synchronize()
    for v in watched:
        bins_all = traces[v][0].cpu().numpy()
        probs_all = traces[v][1].cpu().numpy()
        assert (bins_all[1:] >= 0).all() and (bins_all[1:] < 127).all(), f"video {v}: trace not written by every drawing chunk"
        kv = [k[v * C + c].cpu().numpy() for c in range(C)]
        uv = u[v * C:(v + 1) * C].cpu().numpy()
        yv = ctx[v * C:(v + 1) * C].cpu().numpy()
        orcs = [O.ClosedFormOracle(N, H, 64, 0.75, True, *ws[l], tokens_per_frame=P) for l in range(L)]

        def walk(l):
            worst, worst_p, flips = 0.0, 0.0, 0
            for c in range(C):
                out = orcs[l].step(kv[c], qs[l], new_doc=(c == 0), u=uv[c, l] if c else None,
                                   bins_override=bins_all[c, l] if c else None)
                err = float(np.abs(out - yv[c, l]).max())
                assert err <= CTX_TOL, f"video {v} chunk {c} layer {l}: |ctx(batched) - ctx(oracle)| = {err:.3e}"
                worst = max(worst, err)
                if c:
                    dif = orcs[l].last_bins != bins_all[c, l]
                    flips += int(dif.sum())
                    assert np.abs(orcs[l].last_bins[dif] - bins_all[c, l][dif]).max(initial=0) <= 1, "a differing draw is not adjacent"
                    worst_p = max(worst_p, float(np.abs(orcs[l].last_probs / probs_all[c, l, :127] - 1).max()))
            return worst, worst_p, flips

        with ThreadPoolExecutor(max_workers=L) as pool:
            res = list(pool.map(walk, range(L)))
        worst, worst_p, flips = max(r[0] for r in res), max(r[1] for r in res), sum(r[2] for r in res)
        record_parity(f"multi_video 64x32 headline: video {v}: {flips} of {(C - 1) * L * S} oracle draws differ from the batched "
                      f"trace (teacher-forced), max |ctx - oracle| {worst:.2e}, probs {worst_p:.1e} rel")
        assert worst_p <= 2e-5
        assert flips <= max(4, int(4e-5 * C * L * S)), f"video {v}: {flips} flips"
        for l in range(L):
            np.testing.assert_allclose(engines[v].export_state(l)[0].cpu().numpy(), orcs[l].B_past, rtol=0, atol=B_TOL)


def test_more_videos_than_one_group(dev):
    """260 videos (more than the 256 of one workspace group) of 1-3 chunks at the cfg1 shape: every video equals its own
    batched run alone (V = 1) bit for bit, ctx and B, across the group boundary."""
    from infinite_video_amd.engine import consolidate_videos
    case = BY_NAME["cfg1_sticky"]
    _, qs, ws = case_inputs(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    V, T = 260, case.chunk_T[0]
    counts = [1 + (v * 7) % 3 for v in range(V)]
    gen = torch.Generator(device=dev).manual_seed(11)
    k = torch.randn(sum(counts), T * case.P, case.d, device=dev, generator=gen)
    u = torch.rand(sum(counts), case.n_layers, 512, device=dev, dtype=torch.float64, generator=gen)
    engines = [_engine(case, dev) for _ in range(V)]
    ctx = consolidate_videos(engines, k, counts, q, projs, u, new_doc=True)
    cu = np.concatenate([[0], np.cumsum(counts)])
    alone = _engine(case, dev)
    for v in range(V):
        ref = consolidate_videos([alone], k[cu[v]:cu[v + 1]], [counts[v]], q, projs, u[cu[v]:cu[v + 1]], new_doc=True)
        assert torch.equal(ctx[cu[v]:cu[v + 1]], ref), f"video {v}"
        for l in range(case.n_layers):
            assert torch.equal(engines[v].export_state(l)[0], alone.export_state(l)[0]), f"video {v} layer {l}"


def test_fallback_dense_and_bf16_and_refusals(dev):
    from infinite_video_amd.engine import consolidate_videos
    # dense plan (N = 96): each handle's own consolidate, bit for bit
    case = DENSE_CASES[0]
    assert case.N == 96
    ks, us = _batch(case, [3, 1, 4], first_video=60)
    _, qs, ws = case_inputs(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    engines = [_engine(case, dev) for _ in ks]
    ctxs = _run(dev, engines, ks, us, q, projs)
    for v, (k, u) in enumerate(zip(ks, us)):
        single = _engine(case, dev)
        ref = single.consolidate(torch.from_numpy(k).to(dev), q, projs, torch.from_numpy(u).to(dev), new_doc=True)
        assert torch.equal(ctxs[v], ref)
    # bf16 tokens = the fp32 run on bf16-representable values
    case = BY_NAME["cfg1_sticky"]
    ks, us = _batch(case, [3, 5], first_video=70)
    ks = [torch.from_numpy(k).bfloat16().float().numpy() for k in ks]
    _, _, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    e32 = [_engine(case, dev) for _ in ks]
    c32 = _run(dev, e32, ks, us, q, projs)
    e16 = [_engine(case, dev) for _ in ks]
    k16 = torch.from_numpy(np.concatenate(ks)).to(dev).bfloat16()
    c16 = consolidate_videos(e16, k16, [3, 5], q, projs, torch.from_numpy(np.concatenate(us)).to(dev))
    assert torch.equal(torch.cat(c32), c16)
    # refusals leave the memories as they were
    before = [[e.export_state(l)[0].clone() for l in range(2)] for e in e32]
    fresh = _engine(case, dev)
    k1 = torch.from_numpy(np.concatenate([ks[0][:1], ks[1][:1]])).to(dev)
    u1 = torch.from_numpy(np.concatenate([us[0][:1], us[1][:1]])).to(dev)
    with pytest.raises(RuntimeError):
        consolidate_videos([e32[0], fresh], k1, [1, 1], q, projs, u1, new_doc=False)     # a handle without memory
    from infinite_video_amd import _lib
    import ctypes as C
    lib = _lib.load()
    hs = (C.c_void_p * 2)(e32[0]._h.value, e32[0]._h.value)
    cu = (C.c_int32 * 3)(0, 1, 2)
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()), 32,
                                         e32[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0, C.c_void_p(k1.data_ptr()), None)
    assert rc == -1                                                                      # duplicate handle
    cu_bad = (C.c_int32 * 3)(0, 2, 1)
    hs2 = (C.c_void_p * 2)(e32[0]._h.value, e32[1]._h.value)
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs2, C.c_void_p), 2, cu_bad, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         32, e32[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0, None, None)
    assert rc == -1
    from infinite_video_amd.engine import LTMEngine
    e_tau = LTMEngine(case.N, case.H, case.dh, case.d, case.P, tau=0.9, sticky=True, n_layers=2, max_q=case.Q, device=dev)
    e_tau.ensure_plan(8)
    hs3 = (C.c_void_p * 2)(e32[0]._h.value, e_tau._h.value)
    cu_ok = (C.c_int32 * 3)(0, 1, 2)
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs3, C.c_void_p), 2, cu_ok, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         32, e32[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 1, C.c_void_p(k1.data_ptr()), None)
    assert rc == -1 and "plan" in lib.infv_ltm_last_error().decode()     # another tau: another plan (new_doc = 1 not applied)
    after = [[e.export_state(l)[0] for l in range(2)] for e in e32]
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
