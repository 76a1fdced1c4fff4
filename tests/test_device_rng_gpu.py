"""The device rng of the Gibbs uniforms on the MI355X: with ``set_device_rng`` and ``u=None`` every path draws exactly what
the numpy mirror (``infinite_video_amd.philox``) says -- so every run here is compared, bit for bit, with the same calls on a
fresh engine with the rng off and ``u = philox.gibbs_uniforms(...)``.  Shapes are points of ``tests/golden/sweep_cases.py``
chosen by ``expected_path`` (one per kernel that reads uniforms).  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

from infinite_video_amd import philox
from tests.golden import sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0x9E3779B97F4A7C15
STREAM = 0xFFFFFFFE


# ---------------------------------------------------------------------------------------------------------------- helpers
def mirror(stream, pos0, n_steps, L, S, seed=SEED):
    return torch.from_numpy(philox.gibbs_uniforms(seed, stream, pos0, n_steps, L, S)).to(DEV)


def make_engine(pt, rng, stream=STREAM, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(pt.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=pt.sticky, n_layers=pt.L, max_q=pt.Q, device=DEV,
                     nb_samples=pt.S, max_batch_chunks=pt.max_batch_chunks, rng_seed=SEED if rng else None, rng_stream=stream, **kw)


_INPUTS = {}


def inputs(pt):
    """(k list [T*P, d], q [L, Q, dm], projs) on the device; computed once per point."""
    if pt not in _INPUTS:
        ks, qs, ws, _ = sc.point_inputs(pt)
        _INPUTS[pt] = ([torch.from_numpy(k).to(DEV) for k in ks], torch.from_numpy(qs).to(DEV),
                       [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in w) for w in ws])
    return _INPUTS[pt]


def state(eng):
    torch.cuda.synchronize()
    out = []
    for l in range(eng.L):
        B, mass = eng.export_state(l)
        bins, idx, probs = eng.last_draw(l)
        out.append((B.cpu(), mass.cpu(), bins.copy(), idx.copy(), probs.copy()))
    return out


def assert_same_state(a, b, tag=""):
    assert len(a) == len(b)
    for l, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0], y[0]), f"{tag}: B of layer {l}"
        assert torch.equal(x[1], y[1]), f"{tag}: bin masses of layer {l}"
        for i, what in ((2, "bins"), (3, "idx"), (4, "probs")):
            np.testing.assert_array_equal(x[i], y[i], err_msg=f"{tag}: {what} of layer {l}")


def consolidate_run(pt, rng, eng=None, chunks=None, pos0=0, new_doc=True, **kw):
    """One consolidate call with a trace: (ctx, trace bins, trace probs, engine)."""
    ks, q, projs = inputs(pt)
    eng = eng or make_engine(pt, rng, **kw)
    lo, hi = chunks or (0, pt.chunks)
    k = torch.stack(ks[lo:hi])
    tb, tp = eng.set_trace(hi - lo)
    u = None if rng or not pt.sticky else mirror(STREAM, pos0, hi - lo, pt.L, pt.S)
    ctx = eng.consolidate(k, q, projs, u, new_doc=new_doc)
    eng.sync()
    eng.set_trace(0)
    return ctx, tb, tp, eng


def assert_same_run(a, b, tag):
    assert torch.equal(a[0], b[0]), f"{tag}: ctx"
    assert torch.equal(a[1], b[1]), f"{tag}: trace bins"
    assert torch.equal(a[2], b[2]), f"{tag}: trace probs"
    assert_same_state(state(a[3]), state(b[3]), tag)


# ------------------------------------------------------------------------------------------- 1. the generator on the device
@pytest.mark.parametrize("S,L,pos0,n_steps", [(512, 2, 0, 3), (1, 1, 7, 2), (1023, 3, 2 ** 32 - 2, 1)])
def test_rng_fill_on_the_device_equals_the_mirror(S, L, pos0, n_steps):
    from infinite_video_amd import _lib
    lib = _lib.load()
    out = torch.full((n_steps, L, S), -1.0, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.infv_ltm_rng_fill(SEED, STREAM, pos0, n_steps, L, S, C.c_void_p(out.data_ptr()), stream))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), philox.gibbs_uniforms(SEED, STREAM, pos0, n_steps, L, S))


# ------------------------------------------------------------------------------------ 2. generated == explicit on every path
S511 = replace(sc.SMALL, name="S511", S=511)
N48 = replace(sc.SMALL, name="N48_dense", N=48)
CONSOLIDATE_POINTS = [
    (sc.SMALL, "chain_batch3"),                       # the fused chain: the pre-pass is the generator
    (sc.BY_NAME["H16_Q100"], "chain_kernel"),         # ltm_chain.hip, role S per chunk
    (sc.BY_NAME["S102"], "chain_batch+"),             # chain_batch_kernel reads doubles (S no multiple of 4)
    (sc.BY_NAME["S1000"], "stages"),                  # above 512: the per-chunk step inside consolidate
    (S511, None),                                     # odd S: the last block's second value is unused
    (N48, None),                                      # dense plan
]


@pytest.mark.parametrize("pt,path", CONSOLIDATE_POINTS, ids=[p.name for p, _ in CONSOLIDATE_POINTS])
def test_consolidate_generated_equals_explicit(pt, path):
    if path is not None:
        assert path in sc.expected_path(pt), sc.expected_path(pt)
    gen = consolidate_run(pt, True)
    if pt is N48:
        assert gen[3].ensure_plan(pt.T).dense
    exp = consolidate_run(pt, False)
    assert_same_run(gen, exp, pt.name)
    assert gen[3].rng_position == pt.chunks == exp[3].rng_position
    if pt is sc.SMALL:
        assert (gen[1][1:] >= 0).all()                # the trace holds real draws (chunk 0 draws nothing)


def test_forward_chain_generated_equals_explicit():
    """The per-call stages: four forward calls, the draw inside the projection launch."""
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    engs = [make_engine(pt, True), make_engine(pt, False)]
    u = mirror(STREAM, 0, pt.chunks, pt.L, pt.S)
    for c in range(pt.chunks):
        a = engs[0].forward(ks[c], q, projs, None, new_doc=(c == 0))
        b = engs[1].forward(ks[c], q, projs, u[c] if c else None, new_doc=(c == 0))
        assert torch.equal(a, b), f"ctx of chunk {c}"
        if c:
            assert_same_state(state(engs[0]), state(engs[1]), f"chunk {c}")
    assert engs[0].rng_position == pt.chunks


def test_gaussian_psi_plan_generated_equals_explicit():
    from tests.golden.cases import GAUSS_SIGMAS
    pt = replace(sc.SMALL, name="gauss", T=16, n_chunks=3)
    gen = consolidate_run(pt, True, gaussian_sigmas=GAUSS_SIGMAS)
    assert gen[3].ensure_plan(pt.T).psi
    exp = consolidate_run(pt, False, gaussian_sigmas=GAUSS_SIGMAS)
    assert_same_run(gen, exp, "gaussian psi plan")


def test_consolidate_q_with_per_chunk_queries():
    """infv_ltm_consolidate_q -> infv_ltm_steps: the stand-alone draw kernel, a query per chunk."""
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    k = torch.stack(ks)
    qc = torch.stack([q * (1.0 + 0.125 * c) for c in range(pt.chunks)]).contiguous()
    gen, exp = make_engine(pt, True), make_engine(pt, False)
    a = gen.consolidate_q(k, qc, projs, None, new_doc=True)
    b = exp.consolidate_q(k, qc, projs, mirror(STREAM, 0, pt.chunks, pt.L, pt.S), new_doc=True)
    assert torch.equal(a, b)
    assert_same_state(state(gen), state(exp), "consolidate_q")
    assert gen.rng_position == pt.chunks


# ------------------------------------------------------------------------------------------------------- 3. continuation
PT6 = replace(sc.SMALL, name="small_c6", n_chunks=6)


def test_split_calls_continue_one_stream():
    """6 chunks as 2 + 4 (new_doc=False on the second call) draw positions 0..5 of one stream."""
    gen1 = consolidate_run(PT6, True, chunks=(0, 2))
    gen2 = consolidate_run(PT6, True, eng=gen1[3], chunks=(2, 6), new_doc=False)
    exp1 = consolidate_run(PT6, False, chunks=(0, 2), pos0=0)
    exp2 = consolidate_run(PT6, False, eng=exp1[3], chunks=(2, 6), pos0=2, new_doc=False)
    assert torch.equal(gen1[0], exp1[0]) and torch.equal(gen1[1], exp1[1])
    assert_same_run(gen2, exp2, "second call")
    assert (gen2[1] >= 0).all()                       # every chunk of the second call drew
    assert gen2[3].rng_position == 6
    gen2[3].reset()
    assert gen2[3].rng_position == 0


def test_position_set_after_import_state():
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    src = consolidate_run(pt, True, chunks=(0, 3))[3]
    exported = [tuple(t.clone() for t in src.export_state(l)) for l in range(pt.L)]
    outs = []
    for rng in (True, False):
        eng = make_engine(pt, rng)
        for l in range(pt.L):
            eng.import_state(l, exported[l][0].contiguous(), exported[l][1].contiguous(), projs[l])
        assert eng.rng_position == 0                  # import_state leaves the position alone
        eng.rng_position = 3
        u = None if rng else mirror(STREAM, 3, 1, pt.L, pt.S)[0]
        ctx = eng.forward(ks[3], q, projs, u)
        assert eng.rng_position == 4
        outs.append((ctx, state(eng)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert_same_state(outs[0][1], outs[1][1], "continued on another handle")
    # ... and the position matters: position 0 draws other bins
    eng = make_engine(pt, True)
    for l in range(pt.L):
        eng.import_state(l, exported[l][0].contiguous(), exported[l][1].contiguous(), projs[l])
    eng.forward(ks[3], q, projs, None)
    assert (eng.last_draw(0)[0] != outs[0][1][0][2]).any()


# ----------------------------------------------------------------------------------------------------- 4. lockstep videos
COUNTS = (3, 1, 5, 0, 2)
PT11 = replace(sc.SMALL, name="small_c11", n_chunks=sum(COUNTS))


def videos_run(fn, counts, streams, rng, first=0, order=None):
    """``fn`` = "consolidate_videos" or "steps_videos" over videos cut from PT11's chunks: video v owns chunks
    [cu[v], cu[v+1]) and draws from streams[v].  ``order``: the videos of the call, by index.  Returns per video (ctx, state)."""
    from infinite_video_amd import engine as E
    ks, q, projs = inputs(PT11)
    cu = np.concatenate([[0], np.cumsum(counts)])
    order = list(range(len(counts))) if order is None else order
    engs = [make_engine(PT11, rng, stream=streams[v]) for v in order]
    k = torch.stack([ks[c] for v in order for c in range(cu[v], cu[v + 1])])
    u = None
    if not rng:
        u = torch.cat([mirror(streams[v], 0, counts[v], PT11.L, PT11.S) for v in order if counts[v]])
    cnt = [counts[v] for v in order]
    if fn == "steps_videos":
        ctx = E.steps_videos(engs, engs[0].pool(k), cnt, q, projs, u, new_doc=True)
    else:
        ctx = E.consolidate_videos(engs, k, cnt, q, projs, u, new_doc=True)
    torch.cuda.synchronize()
    cu2 = np.concatenate([[0], np.cumsum(cnt)])
    return {v: (ctx[cu2[i]:cu2[i + 1]].clone(), state(engs[i]) if counts[v] else None, engs[i]) for i, v in enumerate(order)}


@pytest.mark.parametrize("fn", ["consolidate_videos", "steps_videos"])
def test_lockstep_videos_generated_equals_explicit(fn):
    assert sc.videos_supported(PT11, sc.plan_shape(PT11.N, PT11.T, PT11.tau, PT11.S))
    streams = [10 + v for v in range(len(COUNTS))]
    gen = videos_run(fn, COUNTS, streams, True)
    exp = videos_run(fn, COUNTS, streams, False)
    for v, n in enumerate(COUNTS):
        assert torch.equal(gen[v][0], exp[v][0]), f"ctx of video {v}"
        if n:
            assert_same_state(gen[v][1], exp[v][1], f"video {v}")
        assert gen[v][2].rng_position == n == exp[v][2].rng_position
    if fn == "consolidate_videos":
        # a video's bits do not depend on the batch: permuted, and with other videos dropped (same stream)
        perm = videos_run(fn, COUNTS, streams, True, order=[2, 4, 0])
        for v in (2, 4, 0):
            assert torch.equal(perm[v][0], gen[v][0]), f"video {v} in another batch"
            assert_same_state(perm[v][1], gen[v][1], f"video {v} in another batch")
        # the same video under another stream draws other bins
        other = videos_run(fn, COUNTS, [s + 100 for s in streams], True, order=[2])
        assert (other[2][1][0][2] != gen[2][1][0][2]).any()


def test_lockstep_refuses_when_one_engine_has_no_rng():
    from infinite_video_amd import _lib, engine as E
    ks, q, projs = inputs(PT11)
    engs = [make_engine(PT11, True, stream=v) for v in range(3)]
    k = torch.stack(ks[:6])
    E.consolidate_videos(engs, k, [2, 2, 2], q, projs, None, new_doc=True)
    before = [state(e) for e in engs]
    engs[1].clear_device_rng()
    for new_doc in (True, False):
        with pytest.raises(_lib.LTMError) as ei:
            E.consolidate_videos(engs, k, [2, 2, 2], q, projs, None, new_doc=new_doc)
        assert ei.value.code == -1 and "Gibbs uniforms" in str(ei.value)
    for e, b in zip(engs, before):                    # every handle left as it was
        assert e.has_memory and e.rng_position == 2
        assert_same_state(state(e), b, "after the refusal")


# ------------------------------------------------------------------------------------------------------ 5. video Q-former
def qf_model(seed=SEED):
    from tests.golden.qformer_cases import QF_CASES, qf_inputs
    from tests.test_multi_video_qformer_gpu import make_model
    case = {c.name: c for c in QF_CASES}["qf_small"]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    if seed is not None:
        m.use_device_rng(seed)
    return case, m


def qf_mirror(case, base_stream, pos0, n):
    """[n, n_layers, 512]: layer l of a memory whose first stream is base_stream."""
    return torch.stack([mirror(base_stream + l, pos0, n, 1, 512)[:, 0] for l in range(case.n_layers)], dim=1).contiguous()


def qf_frames(case, lens, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(n, case.chunk_T[0] * case.P, case.hidden, device=DEV, generator=gen) for n in lens]


def test_qformer_paths_generated_equal_explicit():
    from tests.test_multi_video_qformer_gpu import ATOL
    case, m = qf_model()
    _, m_off = qf_model(None)
    (f,) = qf_frames(case, [4], 31)
    u = qf_mirror(case, 0, 0, 4)                      # the model's own memories: streams l
    before = torch.random.get_rng_state()
    # chunk by chunk
    per_chunk = []
    for c in range(4):
        hid, emb = m.encode_frames(f[c:c + 1], new_video=(c == 0))
        hid2, emb2 = m_off.encode_frames(f[c:c + 1], new_video=(c == 0), u=u[c])
        assert torch.equal(hid, hid2) and torch.equal(emb, emb2), f"encode_frames chunk {c}"
        per_chunk.append(emb)
    # layer-major, one video
    llama, mean, hidden = m.encode_frames_batch(f, new_video=True, want_hidden=True)
    llama2, mean2, hidden2 = m_off.encode_frames_batch(f, new_video=True, u=u, want_hidden=True)
    assert torch.equal(llama, llama2) and torch.equal(mean, mean2) and torch.equal(hidden, hidden2)
    # many videos, one call: video v's memories draw from streams (v + 1) * n_layers + l
    fs = qf_frames(case, [3, 1, 4], 32)
    fs[2] = f
    uv = torch.cat([qf_mirror(case, (v + 1) * case.n_layers, 0, len(x)) for v, x in enumerate(fs)])
    la, me, hi = m.encode_videos(fs, want_hidden=True)
    lb, mb, hb = m_off.encode_videos(fs, u=uv, want_hidden=True)
    assert torch.equal(la, lb) and torch.equal(me, mb) and torch.equal(hi, hb)
    assert torch.equal(torch.random.get_rng_state(), before), "the global generator was consumed"
    # the three paths agree with each other as they do today (fp32 rounding): per chunk and layer-major on the model's own
    # streams; the batch of videos (video 2 = f, its own streams) against the layer-major path given those uniforms
    torch.testing.assert_close(torch.cat(per_chunk), llama, rtol=0, atol=ATOL)
    l_ref, _, _ = m_off.encode_frames_batch(f, new_video=True, u=uv[4:8].contiguous())
    torch.testing.assert_close(la[4:8], l_ref, rtol=0, atol=ATOL)


def test_encode_long_videos_with_ragged_tails():
    from infinite_video_amd.video_qformer import encode_long_videos
    case, m = qf_model()
    _, m_off = qf_model(None)
    T = case.chunk_T[0]
    gen = torch.Generator(device=DEV).manual_seed(41)
    videos = [torch.randn(n, case.P, case.hidden, device=DEV, generator=gen) for n in (2 * T + 3, T, 5, 3 * T + 2)]
    ids = [5, 6, 7, 8]
    before = torch.random.get_rng_state()
    got = encode_long_videos(m, videos, T, video_ids=ids)
    assert torch.equal(torch.random.get_rng_state(), before)

    def u_of_chunk(v, i):
        return qf_mirror(case, (ids[v] + 1) * case.n_layers, i, 1)[0].cpu()

    want = encode_long_videos(m_off, videos, T, u_of_chunk=u_of_chunk)
    for v in range(len(videos)):
        assert torch.equal(got[v][0], want[v][0]), f"mean of video {v}"
        assert len(got[v][1]) == len(want[v][1])
        for i, (a, b) in enumerate(zip(got[v][1], want[v][1])):
            assert torch.equal(a, b), f"video {v} chunk {i}"


def test_stable_video_ids_make_the_result_independent_of_the_batch():
    case, m = qf_model()
    fs = qf_frames(case, [3, 2, 4], 51)
    la, me, _ = m.encode_videos(fs, video_ids=[7, 8, 9])
    lb, mb, _ = m.encode_videos([fs[2], fs[0]], video_ids=[9, 7])
    assert torch.equal(lb[:4], la[5:9]) and torch.equal(lb[4:], la[:3])
    assert torch.equal(mb[0], me[2]) and torch.equal(mb[1], me[0])
    lc, _, _ = m.encode_videos([fs[2], fs[0]])        # default ids: the index in the call -> other streams
    assert not torch.equal(lc[:4], la[5:9])


# ------------------------------------------------------------------------------------------------------ 6. drop-in module
def dropin_module(case, ws, l):
    from tests.test_module_gpu import _module
    return _module(case, ws, l, DEV)


def test_dropin_module_with_the_device_rng():
    from infinite_video_amd.engine import LTMEngine
    from tests.golden.cases import CASES, case_inputs
    case = CASES[0]
    ks, qs, ws = case_inputs(case)
    mod = dropin_module(case, ws, 0)
    mod.use_device_rng(SEED, 3)
    eng = LTMEngine(case.N, case.H, case.dh, 768, 32, tau=case.tau, sticky=True, n_layers=1, max_q=32, device=DEV)
    projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in ws[0])]
    q = torch.from_numpy(qs[0]).to(DEV)
    u = mirror(3, 0, 4, 1, 512)
    before = torch.random.get_rng_state()
    with torch.no_grad():
        for c in range(4):
            k = torch.from_numpy(ks[c]).to(DEV)
            mod.length = mod.target_len = k.size(0)
            out = mod(k.unsqueeze(0), q.unsqueeze(0), new_doc=(c == 0), layer_n=0)
            ref = eng.forward(k, q.unsqueeze(0).contiguous(), projs, u[c] if c else None, new_doc=(c == 0))
            assert torch.equal(out[0], ref[0]), f"chunk {c}"
            if c:
                assert_same_state(state(mod._engine), state(eng), f"chunk {c}")
    assert torch.equal(torch.random.get_rng_state(), before), "the global generator was consumed"
    assert not hasattr(mod, "_u_ring")
    assert mod._engine.rng_position == 4


def test_dropin_module_default_still_consumes_the_global_generator():
    from tests.golden.cases import CASES, case_inputs
    case = CASES[0]
    ks, qs, ws = case_inputs(case)
    mod = dropin_module(case, ws, 0)
    q = torch.from_numpy(qs[0]).unsqueeze(0).to(DEV)
    torch.manual_seed(99)
    s0 = torch.random.get_rng_state()
    with torch.no_grad():
        mod(torch.from_numpy(ks[0]).unsqueeze(0).to(DEV), q, new_doc=True, layer_n=0)
        assert torch.equal(torch.random.get_rng_state(), s0)                 # the first chunk draws nothing
        for c in (1, 2):
            mod(torch.from_numpy(ks[c]).unsqueeze(0).to(DEV), q, new_doc=False, layer_n=0)
            after = torch.random.get_rng_state()
            torch.random.set_rng_state(s0)
            torch.rand(1024, dtype=torch.float64)                            # 512 + 512 doubles per sticky call
            s0 = torch.random.get_rng_state()
            assert torch.equal(after, s0), f"generator position after sticky call {c}"
    torch.cuda.synchronize()
    assert hasattr(mod, "_u_ring")


# ------------------------------------------------------------------------------------------------------ 7. launch counts
def test_launch_counts_do_not_grow_with_the_rng():
    from infinite_video_amd import _lib, engine as E
    lib = _lib.load()
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    k = torch.stack(ks)
    counts = {}
    for rng in (True, False):
        u = None if rng else mirror(STREAM, 0, pt.chunks, pt.L, pt.S)
        eng = make_engine(pt, rng)
        eng.forward(ks[0], q, projs, None, new_doc=True)
        n0 = lib.infv_ltm_launch_count()
        eng.forward(ks[1], q, projs, None if rng else u[1])
        n1 = lib.infv_ltm_launch_count()
        eng.consolidate(k, q, projs, u, new_doc=True)
        n2 = lib.infv_ltm_launch_count()
        engs = [make_engine(pt, rng, stream=v) for v in range(2)]
        uv = None if rng else torch.cat([mirror(v, 0, 2, pt.L, pt.S) for v in range(2)])
        n3 = lib.infv_ltm_launch_count()
        E.consolidate_videos(engs, k, [2, 2], q, projs, uv, new_doc=True)
        n4 = lib.infv_ltm_launch_count()
        torch.cuda.synchronize()
        counts[rng] = (n1 - n0, n2 - n1, n4 - n3)
    assert counts[True] == counts[False], counts
    assert min(counts[True]) > 0


# ------------------------------------------------------------------------------------------- 8. precedence and refusals
def test_explicit_u_wins_and_still_advances_the_position():
    from tests.golden.sweep_cases import uniforms
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    k = torch.stack(ks)
    u = torch.from_numpy(uniforms(pt)).to(DEV)        # not the rng's values
    on, off = make_engine(pt, True), make_engine(pt, False)
    a = on.consolidate(k, q, projs, u, new_doc=True)
    b = off.consolidate(k, q, projs, u, new_doc=True)
    assert torch.equal(a, b)
    assert_same_state(state(on), state(off), "explicit u with the rng on")
    assert on.rng_position == pt.chunks == off.rng_position
    c = on.forward(ks[0], q, projs, u[1])
    d = off.forward(ks[0], q, projs, u[1])
    assert torch.equal(c, d) and on.rng_position == pt.chunks + 1


def test_refusal_without_rng_is_unchanged_and_clear_restores_it():
    from infinite_video_amd import _lib
    pt = sc.SMALL
    ks, q, projs = inputs(pt)
    eng = make_engine(pt, True)
    eng.forward(ks[0], q, projs, None, new_doc=True)
    eng.forward(ks[1], q, projs, None)                # generated
    eng.clear_device_rng()
    before = state(eng)
    for call in (lambda: eng.forward(ks[2], q, projs, None),
                 lambda: eng.consolidate(torch.stack(ks[2:]), q, projs, None, new_doc=False)):
        with pytest.raises(_lib.LTMError) as ei:
            call()
        assert ei.value.code == -1
        assert "needs the Gibbs uniforms u" in str(ei.value)
    assert eng.rng_position == 2
    assert_same_state(state(eng), before, "after the refusal")


def test_non_sticky_engine_ignores_the_rng():
    pt = sc.BY_NAME["uniform_small"]
    assert not pt.sticky
    a = consolidate_run(pt, True)
    b = consolidate_run(pt, False)
    assert torch.equal(a[0], b[0])
    for l in range(pt.L):
        assert torch.equal(a[3].export_state(l)[0], b[3].export_state(l)[0])
    assert a[3].rng_position == pt.chunks


# ----------------------------------------------------------------------------------------------------------- 9. VideoChat2
def test_videochat2_with_the_device_rng():
    """Two chunks through VideoChat2Encoder: LTM instance i draws from stream i.  The explicit run hands every instance the
    mirror's uniforms of (stream i, position c) where the default path hands it the CPU generator's."""
    from tests.golden.vc_cases import VC_CASE, vc_inputs
    from tests.test_vc_gpu import make_model
    case = VC_CASE
    frames, h0, weights = vc_inputs(case)
    hin = torch.from_numpy(h0).unsqueeze(0).to(DEV)
    T = case.max_int
    blks = [torch.from_numpy(frames[c * T:(c + 1) * T]).to(DEV).reshape(1, -1, case.enc_width) for c in range(2)]
    m = make_model(case, weights, DEV)
    m.use_device_rng(SEED)
    before = torch.random.get_rng_state()
    got = [m.encode_tokens(blks[c], new_video=(c == 0), hidden_in=hin) for c in range(2)]
    assert torch.equal(torch.random.get_rng_state(), before)
    m2 = make_model(case, weights, DEV)
    keep = []
    for i, mod in enumerate(m2.qformer.ltm_modules):
        u = mirror(i, 1, 1, 1, 512)[0, 0].contiguous()            # the only draw: chunk 1
        keep.append(u)
        mod._draw_uniforms = lambda device, _u=u: _u.data_ptr()
        mod._uniforms_used = lambda device: None
    want = [m2.encode_tokens(blks[c], new_video=(c == 0), hidden_in=hin) for c in range(2)]
    torch.cuda.synchronize()
    for c in range(2):
        assert torch.equal(got[c][0], want[c][0]) and torch.equal(got[c][1], want[c][1]), f"chunk {c}"
    for a, b in zip(m.qformer.ltm_modules, m2.qformer.ltm_modules):
        assert_same_state(state(a._engine), state(b._engine), "VideoChat2 LTM instance")
        assert a._engine.rng_position == 2
