"""The two ends of a consolidate call that the hand-over touches: the sum of the outputs kept by the update + read-out kernels
(infv_ltm_set_ctx_sum) and the one-launch payload (infv_ltm_pack_memory).

Headline operator (T=256, N=256, H=12, Q=32, d=768, L=2: the fused chain needs it) on small frames (P=4), sub-batches of 42.
Call lengths: 1 (first chunk only), 2 (+ a one-chunk sub-batch on the split-K projection), 33 (+ one full 32-chunk sub-batch: calls
under 768 chunks use 32), 66 (1 + 32 + 32 + 1), 800 (the one-launch pooling form: 1 + 19 x 42 + 1).

ctx_sum is checked twice: bit for bit against a numpy float32 replay of the order include/infv_ltm.h states, and against the float64
sum within depth * 2^-24 * sum_c |ctx_c| elementwise, where depth is the longest chain of additions one summand passes through in
that order (the standard first-order bound of a fixed summation tree with unit roundoff 2^-24; nothing is tuned)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, DH, D, P, T, Q, L = 256, 12, 64, 768, 4, 256, 32, 2
DM = H * DH
MAXB = 42
LENGTHS = (1, 2, 33, 66, 800)
NB, NM, NS, NC = L * N * D, L * 127, L * H * Q * N, L * Q * DM


def _engine(dev, n=N, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(n, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev, max_batch_chunks=MAXB, **kw)


def _launches():
    from infinite_video_amd import _lib
    return int(_lib.load().infv_ltm_launch_count())


def launch_sizes(n, new_doc=True):
    """Chunks per update + read-out launch of a fused call of n chunks, in launch order."""
    sub = MAXB if n >= 768 else min(MAXB, 32)
    out = [1] if new_doc else []
    rest = n - len(out)
    while rest > 0:
        out.append(min(sub, rest))
        rest -= out[-1]
    return out


def replay_kept(ctx, sizes):
    """sum = (...((0 + S_0) + S_1) + ...), S_b = left-to-right float32 sum of launch b's chunks; -> (sum, longest addition chain)."""
    total = np.zeros(ctx.shape[1:], np.float32)
    c, depth = 0, 0
    for b, nb in enumerate(sizes):
        s = ctx[c].copy()
        for i in range(1, nb):
            s += ctx[c + i]
        total = total + s
        depth = max(depth, (nb - 1) + (len(sizes) - b))
        c += nb
    assert c == ctx.shape[0]
    return total, depth


def replay_fallback(ctx):
    """ctx_sum_kernel: float32 sums over blocks of 64 chunks from 0, then the blocks left to right from 0."""
    n = ctx.shape[0]
    total = np.zeros(ctx.shape[1:], np.float32)
    n_blocks = (n + 63) // 64
    depth = 0
    for b in range(n_blocks):
        s = np.zeros(ctx.shape[1:], np.float32)
        for c in range(64 * b, min(64 * b + 64, n)):
            s += ctx[c]
        total += s
        depth = max(depth, min(64, n - 64 * b) + (n_blocks - b))
    return total, depth


def check_sum(got, ctx, want, depth):
    got = got.reshape(ctx.shape[1:])
    assert np.array_equal(got, want), f"ctx_sum is not the stated order's sum: max |diff| {np.abs(got - want).max():.3e}"
    c64 = ctx.astype(np.float64)
    bound = depth * 2.0 ** -24 * np.abs(c64).sum(0)
    err = np.abs(got.astype(np.float64) - c64.sum(0))
    print(f"[call ends] n={ctx.shape[0]} depth={depth} max err {err.max():.3e} min slack {(bound - err).min():.3e}")
    assert (err <= bound).all()


def check_segments(eng, payload, n, with_scores):
    """Everything but ctx_sum against the entry points that handed it over before; -> the ctx_sum segment (host)."""
    ns = NS if with_scores else 0
    assert payload.numel() == NB + NM + ns + NC + 1
    assert bool(torch.isfinite(payload).all())
    for l in range(L):
        B, mass = eng.export_state(l)
        assert torch.equal(payload[l * N * D:(l + 1) * N * D].reshape(N, D), B)
        assert torch.equal(payload[NB + l * 127:NB + (l + 1) * 127], mass)
    if with_scores:
        assert torch.equal(payload[NB + NM:NB + NM + NS].reshape(L, H, Q, N), eng.last_scores_device(Q))
    assert float(payload[-1]) == float(n)
    return payload[NB + NM + ns:NB + NM + ns + NC].cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def video(dev):
    from infinite_video_amd import synth
    n = max(LENGTHS)
    projs = [tuple(torch.from_numpy(a).to(dev) for a in synth.layer_projections(l, D, DM)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, DM) for l in range(L)])).to(dev)
    u = torch.from_numpy(synth.gibbs_uniforms(n, L)).to(dev)
    k = torch.empty(n, T * P, D, device=dev, dtype=torch.float32)
    gen = torch.Generator(device=dev).manual_seed(synth.SEED_K)
    for i in range(0, n, 64):
        k[i:i + 64].normal_(generator=gen)
    return k, q, projs, u


@pytest.fixture(scope="module")
def engines(dev):
    on, off = _engine(dev), _engine(dev)
    on.set_ctx_sum(True)
    return on, off


def _nan_payload(eng, dev, with_scores):
    return torch.full((eng.payload_numel(Q, with_scores),), float("nan"), device=dev, dtype=torch.float32)


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_of_a_call_that_kept_its_sum(n, dev, video, engines):
    k, q, projs, u = video
    eng = engines[0]
    ctx = eng.consolidate(k[:n], q, projs, u[:n], new_doc=True)
    segs = []
    for with_scores in (False, True):
        out = _nan_payload(eng, dev, with_scores)
        before = _launches()
        got = eng.pack_memory(ctx, with_scores, out=out)
        assert _launches() - before == 1
        eng.sync()
        assert got.data_ptr() == out.data_ptr()
        segs.append(check_segments(eng, out, n, with_scores))
    assert np.array_equal(segs[0], segs[1])
    host = ctx.cpu().numpy()
    check_sum(segs[0], host, *replay_kept(host, launch_sizes(n)))


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_without_a_kept_sum_adds_ctx_up_in_one_more_launch(n, dev, video, engines):
    k, q, projs, u = video
    eng = engines[1]                                              # sums never switched on
    ctx = eng.consolidate(k[:n], q, projs, u[:n], new_doc=True)
    out = _nan_payload(eng, dev, True)
    before = _launches()
    eng.pack_memory(ctx, True, out=out)
    assert _launches() - before == 2
    eng.sync()
    host = ctx.cpu().numpy()
    check_sum(check_segments(eng, out, n, True), host, *replay_fallback(host))


@pytest.mark.parametrize("n", (66, 800))
def test_keeping_the_sum_changes_nothing_else(n, video, engines):
    k, q, projs, u = video
    res = []
    for eng in engines:
        ctx = eng.consolidate(k[:n], q, projs, u[:n], new_doc=True)
        eng.sync()
        res.append((ctx, [eng.export_state(l)[0] for l in range(L)], [eng.last_draw(l) for l in range(L)], eng.last_scores_device(Q)))
    (c0, B0, d0, s0), (c1, B1, d1, s1) = res
    assert torch.equal(c0, c1) and torch.equal(s0, s1)
    for l in range(L):
        assert torch.equal(B0[l], B1[l])
        for a, b in zip(d0[l], d1[l]):
            assert np.array_equal(a, b)


def test_pack_after_a_continuation_sums_the_continuation(dev, video, engines):
    k, q, projs, u = video
    eng = engines[0]
    eng.consolidate(k[:40], q, projs, u[:40], new_doc=True)
    ctx = eng.consolidate(k[40:70], q, projs, u[40:70], new_doc=False)
    out = _nan_payload(eng, dev, False)
    before = _launches()
    eng.pack_memory(ctx, False, out=out)
    assert _launches() - before == 1
    eng.sync()
    host = ctx.cpu().numpy()
    check_sum(check_segments(eng, out, 30, False), host, *replay_kept(host, launch_sizes(30, new_doc=False)))


def test_pack_of_a_foreign_ctx_and_after_a_per_chunk_step(dev, video, engines):
    k, q, projs, u = video
    eng = engines[0]
    ctx = eng.consolidate(k[:33], q, projs, u[:33], new_doc=True)
    foreign = ctx.clone()                                         # same values at another address: the kept sum is not for it
    out = _nan_payload(eng, dev, False)
    before = _launches()
    eng.pack_memory(foreign, False, out=out)
    assert _launches() - before == 2
    eng.sync()
    host = ctx.cpu().numpy()
    check_sum(check_segments(eng, out, 33, False), host, *replay_fallback(host))
    # a per-chunk step moves the memory on: the call's sum no longer describes what the handle holds, whatever ctx is named
    ctx = eng.consolidate(k[:33], q, projs, u[:33], new_doc=True)
    eng.forward(k[33], q, projs, u[33], new_doc=False)
    out.fill_(float("nan"))
    before = _launches()
    eng.pack_memory(ctx, False, out=out)
    assert _launches() - before == 2
    eng.sync()
    host = ctx.cpu().numpy()
    check_sum(check_segments(eng, out, 33, False), host, *replay_fallback(host))


def test_pack_on_a_dense_plan_engine(dev, video):
    """N=48: the fp32 boxes overlap, every call runs chunk by chunk through the dense step and keeps no sum."""
    _, q, projs, u = video
    n, Td, Nd = 5, 8, 48
    eng = _engine(dev, n=Nd)
    eng.set_ctx_sum(True)
    assert eng.ensure_plan(Td).dense
    k = torch.empty(n, Td * P, D, device=dev, dtype=torch.float32).normal_(generator=torch.Generator(device=dev).manual_seed(7))
    ctx = eng.consolidate(k, q, projs, u[:n], new_doc=True)
    out = torch.full((eng.payload_numel(Q, False),), float("nan"), device=dev, dtype=torch.float32)
    before = _launches()
    eng.pack_memory(ctx, False, out=out)
    assert _launches() - before == 2
    eng.sync()
    assert bool(torch.isfinite(out).all())
    nb = L * Nd * D
    for l in range(L):
        B, mass = eng.export_state(l)
        assert torch.equal(out[l * Nd * D:(l + 1) * Nd * D].reshape(Nd, D), B)
        assert torch.equal(out[nb + l * 127:nb + (l + 1) * 127], mass)
    assert float(out[-1]) == float(n)
    host = ctx.cpu().numpy()
    check_sum(out[nb + NM:nb + NM + NC].cpu().numpy(), host, *replay_fallback(host))
    with pytest.raises(Exception):
        eng.pack_memory(ctx, True)                               # no fused step behind this memory: refused like export_chain_state
