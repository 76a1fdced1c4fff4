"""Several videos from frame means with a query per chunk (infv_ltm_steps_videos / engine.steps_videos) on the MI355X: the
shared-query form equals consolidate_videos bit for bit, goldens and the closed-form oracle inside a batch with per-chunk
queries, batch and split invariance bit for bit, agreement with the per-video consolidate_q, fallback and refusals."""
import numpy as np
import pytest
import torch

from oracle import ltm_oracle as O
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
    return synth.video_batch(lens, case.chunk_T[0], case.P, case.d, case.n_layers, first_video=first_video)


def _chunk_queries(case, n, seed):
    """[n, L, Q, dm]: a different query for every chunk (the hidden states of a layer after the first)."""
    from infinite_video_amd import synth
    dm = case.H * case.dh
    if n == 0:
        return np.zeros((0, case.n_layers, case.Q, dm), np.float32)
    return np.stack([np.stack([synth.layer_query(l, case.Q, dm, seed=seed + 97 * c) for l in range(case.n_layers)])
                     for c in range(n)]).astype(np.float32)


def _pool(dev, engine, ks):
    """Packed frame means [sum C_v, T, d] of the videos' tokens (infv_ltm_pool)."""
    k = torch.from_numpy(np.concatenate(ks)).to(dev)
    return engine.pool(k)


def _split(x, counts):
    cu = np.concatenate([[0], np.cumsum(counts)])
    return [x[cu[v]:cu[v + 1]] for v in range(len(counts))]


def _steps(dev, engines, kbar, counts, q, projs, us, new_doc=True):
    from infinite_video_amd.engine import steps_videos
    u = torch.from_numpy(np.concatenate(us)).to(dev)
    ctx = steps_videos(engines, kbar, counts, q, projs, u, new_doc=new_doc)
    torch.cuda.synchronize()
    return _split(ctx, counts)


def _state(e, case):
    out = []
    for l in range(case.n_layers):
        B, mass = e.export_state(l)
        bins, _, probs = e.last_draw(l)
        out.append((B.cpu(), mass.cpu(), bins.copy(), probs.copy(), e.last_scores(l, case.Q).copy()))
    return out


def _equal_states(a, b, tag=""):
    for (Ba, ma, ba, pa, sa), (Bb, mb, bb, pb, sb) in zip(a, b):
        assert torch.equal(Ba, Bb), tag
        assert torch.equal(ma, mb), tag
        np.testing.assert_array_equal(ba, bb, err_msg=tag)
        np.testing.assert_array_equal(pa, pb, err_msg=tag)
        np.testing.assert_array_equal(sa, sb, err_msg=tag)


@pytest.mark.parametrize("name,lens", [("cfg1_sticky", [3, 0, 1, 5]), ("headline", [2, 0, 1])])
def test_shared_query_equals_consolidate_videos(dev, name, lens):
    """Contract (a): q_per_chunk = 0 and kbar = pool(k) give consolidate_videos(k, q)'s bits -- ctx, B, bin masses, draws."""
    from infinite_video_amd.engine import consolidate_videos
    case = BY_NAME[name]
    kg, ug, qs, ws = _golden_video(case)
    syn_k, syn_u = _batch(case, lens, first_video=80)
    ks, us = [kg] + syn_k, [ug] + syn_u
    counts = [len(k) for k in ks]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    ref = [_engine(case, dev) for _ in ks]
    k = torch.from_numpy(np.concatenate(ks)).to(dev)
    u = torch.from_numpy(np.concatenate(us)).to(dev)
    ctx_ref = consolidate_videos(ref, k, counts, q, projs, u, new_doc=True)
    got = [_engine(case, dev) for _ in ks]
    ctx = _steps(dev, got, ref[0].pool(k), counts, q, projs, us)
    assert torch.equal(torch.cat(ctx), ctx_ref)
    for v in range(len(ks)):
        if counts[v]:
            _equal_states(_state(got[v], case), _state(ref[v], case), f"video {v}")


@pytest.mark.parametrize("name", ["cfg1_sticky", "peaked"])
def test_per_chunk_queries_goldens_and_oracle_inside_a_batch(dev, name):
    """The golden video (its reference query on every chunk) at position 1 among synthetic videos of 0, 1 and 3 chunks with a
    different query per chunk: the golden video reproduces the reference's bins, ctx and B; every video matches the closed-form
    oracle walked chunk by chunk under the same queries and uniforms."""
    case = BY_NAME[name]
    g = load_golden(case)
    kg, ug, qs, ws = _golden_video(case)
    syn_k, syn_u = _batch(case, [0, 1, 3], first_video=90)
    ks, us = syn_k[:1] + [kg] + syn_k[1:], syn_u[:1] + [ug] + syn_u[1:]
    counts = [len(k) for k in ks]
    qcs = [_chunk_queries(case, n, seed=5000 + 31 * v) for v, n in enumerate(counts)]
    qcs[1] = np.broadcast_to(np.stack(qs)[None], (counts[1],) + np.stack(qs).shape).astype(np.float32)
    engines = [_engine(case, dev) for _ in ks]
    traces = [e.set_trace(n) if case.sticky and n else None for e, n in zip(engines, counts)]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.ascontiguousarray(np.concatenate(qcs))).to(dev)
    ctxs = _steps(dev, engines, _pool(dev, engines[0], ks), counts, q, projs, us)
    for v, (e, k, u, qc, ctx) in enumerate(zip(engines, ks, us, qcs, ctxs)):
        ctx = ctx.cpu().numpy()
        orc = [O.ClosedFormOracle(case.N, case.H, case.dh, case.tau, case.sticky, *ws[l], tokens_per_frame=case.P)
               for l in range(case.n_layers)]
        for c in range(len(k)):
            for l in range(case.n_layers):
                ref = orc[l].step(k[c], qc[c, l], new_doc=(c == 0), u=u[c, l])
                np.testing.assert_allclose(ctx[c, l], ref, rtol=0, atol=CTX_TOL, err_msg=f"video {v} chunk {c} layer {l}")
                if case.sticky and c > 0:
                    bins = traces[v][0][c, l].cpu().numpy()
                    assert (bins == orc[l].last_bins).all(), f"video {v} chunk {c} layer {l}: {(bins != orc[l].last_bins).sum()} flips"
                if v == 1:
                    tag = f"c{c}_l{l}"
                    np.testing.assert_allclose(ctx[c, l], g[tag + "_ctx"], rtol=0, atol=CTX_TOL)
                    if case.sticky and c > 0:
                        np.testing.assert_array_equal(traces[v][0][c, l].cpu().numpy(), g[tag + "_bins"])
        for l in range(case.n_layers):
            if len(k):
                np.testing.assert_allclose(e.export_state(l)[0].cpu().numpy(), orc[l].B_past, rtol=0, atol=B_TOL)
            else:
                assert not e.has_memory


def test_per_chunk_queries_batch_and_split_invariance(dev):
    """Contract (b) with a query per chunk: one video alone, first, last and between videos of other lengths gives the same
    bits (ctx, B, bin masses, draws, scores); chunks [0, 4) with new_doc then [4, 8) continued equal one call."""
    case = BY_NAME["cfg1_sticky"]
    kg, ug, _, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    qg = _chunk_queries(case, len(kg), seed=6000)
    others_k, others_u = _batch(case, [8, 5, 2, 8, 1, 6], first_video=100)
    others_q = [_chunk_queries(case, len(k), seed=6100 + 13 * i) for i, k in enumerate(others_k)]
    short_k, short_u = _batch(case, [3, 0, 12], first_video=110)
    short_q = [_chunk_queries(case, len(k), seed=6200 + 13 * i) for i, k in enumerate(short_k)]
    runs = {"alone": ([kg], [ug], [qg], 0), "first": ([kg] + others_k, [ug] + others_u, [qg] + others_q, 0),
            "last": (others_k + [kg], others_u + [ug], others_q + [qg], 6),
            "ragged": (short_k[:1] + [kg] + short_k[1:], short_u[:1] + [ug] + short_u[1:], short_q[:1] + [qg] + short_q[1:], 1)}
    res = {}
    for tag, (ks, us, qcs, pos) in runs.items():
        engines = [_engine(case, dev) for _ in ks]
        q = torch.from_numpy(np.concatenate(qcs)).to(dev)
        ctx = _steps(dev, engines, _pool(dev, engines[0], ks), [len(k) for k in ks], q, projs, us)[pos]
        res[tag] = (ctx.cpu(), _state(engines[pos], case))
    for tag in ("first", "last", "ragged"):
        assert torch.equal(res[tag][0], res["alone"][0]), tag
        _equal_states(res[tag][1], res["alone"][1], tag)
    # split invariance: two calls equal one
    ks, us = _batch(case, [8, 8, 8], first_video=120)
    qcs = [_chunk_queries(case, 8, seed=6300 + 13 * i) for i in range(3)]
    whole = [_engine(case, dev) for _ in ks]
    q = torch.from_numpy(np.concatenate(qcs)).to(dev)
    ctx_w = _steps(dev, whole, _pool(dev, whole[0], ks), [8] * 3, q, projs, us)
    split = [_engine(case, dev) for _ in ks]
    qa = torch.from_numpy(np.concatenate([x[:4] for x in qcs])).to(dev)
    qb = torch.from_numpy(np.concatenate([x[4:] for x in qcs])).to(dev)
    ctx_a = _steps(dev, split, _pool(dev, split[0], [k[:4] for k in ks]), [4] * 3, qa, projs, [u[:4] for u in us], new_doc=True)
    ctx_b = _steps(dev, split, _pool(dev, split[0], [k[4:] for k in ks]), [4] * 3, qb, projs, [u[4:] for u in us], new_doc=False)
    for v in range(3):
        assert torch.equal(torch.cat([ctx_a[v], ctx_b[v]]), ctx_w[v]), f"video {v}"
        _equal_states(_state(split[v], case), _state(whole[v], case), f"video {v}")


@pytest.mark.parametrize("name", ["cfg1_sticky", "peaked", "headline"])
def test_per_chunk_queries_match_consolidate_q(dev, name):
    """Contract (c): per video equal to LTMEngine.consolidate_q on the same tokens, per-chunk queries and uniforms, within
    test_multi_video_gpu.py::test_matches_the_single_video_path's tolerances."""
    case = BY_NAME[name]
    kg, ug, _, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    ks, us = _batch(case, [2, len(kg)], first_video=130)
    ks, us = [kg] + ks, [ug] + us
    counts = [len(k) for k in ks]
    qcs = [_chunk_queries(case, n, seed=7000 + 31 * v) for v, n in enumerate(counts)]
    engines = [_engine(case, dev) for _ in ks]
    ctxs = _steps(dev, engines, _pool(dev, engines[0], ks), counts, torch.from_numpy(np.concatenate(qcs)).to(dev), projs, us)
    for v, (k, u, qc) in enumerate(zip(ks, us, qcs)):
        single = _engine(case, dev)
        ref = single.consolidate_q(torch.from_numpy(k).to(dev), torch.from_numpy(qc).to(dev), projs, torch.from_numpy(u).to(dev),
                                   new_doc=True)
        np.testing.assert_allclose(ctxs[v].cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-5, err_msg=f"video {v}")
        for l in range(case.n_layers):
            np.testing.assert_allclose(engines[v].export_state(l)[0].cpu().numpy(), single.export_state(l)[0].cpu().numpy(),
                                       rtol=0, atol=1e-6)
            np.testing.assert_array_equal(engines[v].last_draw(l)[0], single.last_draw(l)[0])


def test_fallback_dense_and_refusals(dev):
    """A dense plan (N = 96) runs each handle's infv_ltm_steps (per-chunk queries: = consolidate_q) or consolidate_pooled
    (shared query: = consolidate), bit for bit.  Refusals leave every memory as it was."""
    from infinite_video_amd.engine import steps_videos
    case = DENSE_CASES[0]
    assert case.N == 96
    ks, us = _batch(case, [3, 1, 4], first_video=140)
    counts = [len(k) for k in ks]
    _, qs, ws = case_inputs(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    qcs = [_chunk_queries(case, n, seed=8000 + 31 * v) for v, n in enumerate(counts)]
    engines = [_engine(case, dev) for _ in ks]
    kbar = _pool(dev, engines[0], ks)
    ctxs = _steps(dev, engines, kbar, counts, torch.from_numpy(np.concatenate(qcs)).to(dev), projs, us)
    q = torch.from_numpy(np.stack(qs)).to(dev)
    shared = [_engine(case, dev) for _ in ks]
    ctxs_shared = _steps(dev, shared, kbar, counts, q, projs, us)
    for v, (k, u, qc) in enumerate(zip(ks, us, qcs)):
        single = _engine(case, dev)
        kt, ut = torch.from_numpy(k).to(dev), torch.from_numpy(u).to(dev)
        assert torch.equal(ctxs[v], single.consolidate_q(kt, torch.from_numpy(qc).to(dev), projs, ut, new_doc=True)), f"video {v}"
        assert torch.equal(ctxs_shared[v], single.consolidate(kt, q, projs, ut, new_doc=True)), f"video {v}"
    # refusals: nothing changes
    case = BY_NAME["cfg1_sticky"]
    ks, us = _batch(case, [3, 5], first_video=150)
    _, _, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    engines = [_engine(case, dev) for _ in ks]
    _steps(dev, engines, _pool(dev, engines[0], ks), [3, 5], q, projs, us)
    before = [[e.export_state(l)[0].clone() for l in range(2)] for e in engines]
    kbar1 = _pool(dev, engines[0], [ks[0][:1], ks[1][:1]])
    u1 = torch.from_numpy(np.concatenate([us[0][:1], us[1][:1]])).to(dev)
    with pytest.raises(RuntimeError):
        steps_videos([engines[0], _engine(case, dev)], kbar1, [1, 1], q, projs, u1, new_doc=False)   # a handle without memory
    from infinite_video_amd.engine import LTMEngine
    e_tau = LTMEngine(case.N, case.H, case.dh, case.d, case.P, tau=0.9, sticky=True, n_layers=2, max_q=case.Q, device=dev)
    with pytest.raises(ValueError, match="configured differently"):
        steps_videos([engines[0], e_tau], kbar1, [1, 1], q, projs, u1, new_doc=True)
    import ctypes as C
    from infinite_video_amd import _lib
    lib = _lib.load()
    e_tau.ensure_plan(8)
    hs = (C.c_void_p * 2)(engines[0]._h.value, e_tau._h.value)
    cu = (C.c_int32 * 3)(0, 1, 2)
    out = torch.empty(2, 2, case.Q, 768, device=dev)
    rc = lib.infv_ltm_steps_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(kbar1.data_ptr()), 8, C.c_void_p(q.data_ptr()), 0,
                                   case.Q, engines[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 1, C.c_void_p(out.data_ptr()),
                                   None)
    assert rc == -1 and "plan" in lib.infv_ltm_last_error().decode()     # another tau: another plan (new_doc = 1 not applied)
    hs = (C.c_void_p * 2)(engines[0]._h.value, engines[0]._h.value)
    rc = lib.infv_ltm_steps_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(kbar1.data_ptr()), 8, C.c_void_p(q.data_ptr()), 0,
                                   case.Q, engines[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 1, C.c_void_p(out.data_ptr()),
                                   None)
    assert rc == -1                                                      # duplicate handle
    torch.cuda.synchronize()
    after = [[e.export_state(l)[0] for l in range(2)] for e in engines]
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_fallback_sparse_plan_above_256_basis_functions(dev):
    """N = 272 at T = 256: a sparse plan the lockstep kernels do not take (N above 256) runs each handle's infv_ltm_steps
    (per-chunk queries: = consolidate_q) or consolidate_pooled (shared query: = consolidate), bit for bit."""
    from infinite_video_amd import synth
    from infinite_video_amd.basis_maps import build_plan
    from infinite_video_amd.engine import LTMEngine, steps_videos
    N, T, H, dh, d, P, L, Q = 272, 256, 12, 64, 768, 32, 2, 32
    assert not build_plan(T, N, 0.75).dense
    counts = [2, 1, 3]
    gen = torch.Generator(device=dev).manual_seed(3)
    k = torch.randn(sum(counts), T * P, d, device=dev, generator=gen)
    u = torch.rand(sum(counts), L, 512, device=dev, dtype=torch.float64, generator=gen)
    ws = [synth.layer_projections(l, d, H * dh) for l in range(L)]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, H * dh) for l in range(L)])).to(dev)
    qc = torch.randn(sum(counts), L, Q, H * dh, device=dev, generator=gen)
    make = lambda: LTMEngine(N, H, dh, d, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev)
    engines = [make() for _ in counts]
    kbar = engines[0].pool(k)
    ctx_q = _split(steps_videos(engines, kbar, counts, qc, projs, u), counts)
    shared = [make() for _ in counts]
    ctx_s = _split(steps_videos(shared, kbar, counts, q, projs, u), counts)
    kv, uv, qv = _split(k, counts), _split(u, counts), _split(qc, counts)
    for v in range(len(counts)):
        single = make()
        assert torch.equal(ctx_q[v], single.consolidate_q(kv[v], qv[v].contiguous(), projs, uv[v].contiguous(), new_doc=True)), v
        assert torch.equal(ctx_s[v], single.consolidate(kv[v], q, projs, uv[v].contiguous(), new_doc=True)), v
