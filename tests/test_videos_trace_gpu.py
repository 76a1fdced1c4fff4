"""The attention read-outs of the batched calls on the GPU: the packed mass trace of the lockstep calls
(``infv_ltm_set_videos_mass_trace`` / ``engine.trace_videos``), the source weights of many videos in one launch
(``infv_ltm_source_weights_videos`` / ``engine.source_weights_videos``), both through the video Q-former's batched call, and one
stream-order scenario by the method of tests/test_stream_order_gpu.py.

Bounds.  Bit equality wherever the header promises it: a video's last packed row against ``infv_ltm_masses`` on its handle, a
video's rows whatever else is in the batch, the fallback against each handle's own call, the batched source pass against the
single-video call and against the ordered fp32 mirror, outputs with the trace on against off.  Lockstep against per-call scores
agree within delta(S) = 2e-5 + 1e-4 max|S| (tests/test_ltm_gpu.py), a mass moves by a factor within e^{+-2 delta}: relative
2 delta + EPS with EPS = 2e-6 (tests/test_density_gpu.py), S being the scores of the chunk compared.  A packed row against the
float64 mirror on the device's own scores: EPS + 2^-22 max|S| (the same file).  ``float64(W) pool(k)`` against ``export_state``'s
B: 2e-5 in the max norm (the project's B_TOL).  ``attn_all`` against the float64 mirror on the device's own masses: relative
C (m + 1) 2^-24 + 2^-23 (tests/test_source_weights_gpu.py), C the video's chunks and m the plan's largest number of operator rows in
one box.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, density, synth
from infinite_video_amd.basis_maps import NB_BINS, build_plan
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

EPS = 2e-6
B_TOL = 2e-5
TAU, S = 0.75, 512
H, DH, D, P = 12, 64, 768, 32
DM = H * DH
TN, TQ, TT, TL = 64, 32, 8, 2                                    # the cfg1_sticky shape
COUNTS = [3, 1, 4, 0, 2]
INVALID, UNSUPPORTED, STATE = -1, -2, -4
PATHS = ("consolidate_videos", "steps_shared_q", "steps_q_per_chunk", "steps_from")


def delta(Sc) -> float:
    return 2e-5 + 1e-4 * float(np.abs(Sc).max())


def rel_err(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def ltm_engine(dev, N=TN, L=TL, T=TT, **kw):
    from infinite_video_amd.engine import LTMEngine
    e = LTMEngine(N, H, DH, D, P, tau=TAU, sticky=True, n_layers=L, max_q=TQ, device=dev, **kw)
    e.ensure_plan(T)
    return e


def cu_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


class Inputs:
    """Tokens, frame means, uniforms, one shared and one per-chunk query and the projections of a packed batch, made once."""

    def __init__(self, dev, counts, T=TT, L=TL, seed=7, pooler=None):
        self.counts, self.cu, self.total, self.T, self.L = list(counts), cu_of(counts), int(sum(counts)), T, L
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.k = torch.randn(self.total, T * P, D, device=dev, generator=gen) * 0.5
        self.u = torch.rand(self.total, L, S, device=dev, dtype=torch.float64, generator=gen)
        self.q = torch.from_numpy(np.stack([synth.layer_query(l, TQ, DM) for l in range(L)])).to(dev)
        self.qc = torch.randn(self.total, L, TQ, DM, device=dev, generator=gen)
        self.projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.layer_projections(l, D, DM))
                      for l in range(L)]
        self.kbar = (pooler or ltm_engine(dev, L=L, T=T)).pool(self.k).reshape(self.total, T, D).contiguous()
        # infv_ltm_steps_videos_from: the frame means sit two chunks into a larger block
        self.kbar_from = torch.cat([torch.full((2, T, D), 3.0, device=dev), self.kbar]).contiguous()

    def run(self, path, engines, new_doc=True):
        from infinite_video_amd.engine import consolidate_videos, steps_videos
        if path == "consolidate_videos":
            return consolidate_videos(engines, self.k, self.counts, self.q, self.projs, self.u, new_doc=new_doc)
        if path == "steps_shared_q":
            return steps_videos(engines, self.kbar, self.counts, self.q, self.projs, self.u, new_doc=new_doc)
        if path == "steps_q_per_chunk":
            return steps_videos(engines, self.kbar, self.counts, self.qc, self.projs, self.u, new_doc=new_doc)
        assert path == "steps_from"
        return steps_videos(engines, self.kbar_from, self.counts, self.q, self.projs, self.u, new_doc=new_doc,
                            kbar_chunk0=[int(c) + 2 for c in self.cu[:-1]])

    def q_rows(self, path, v):
        """[C_v, L, Q, dm]: the query of every chunk of video v, as ``LTMEngine.steps`` takes it."""
        a, b = int(self.cu[v]), int(self.cu[v + 1])
        if path == "steps_q_per_chunk":
            return self.qc[a:b].contiguous()
        return self.q[None].expand(b - a, *self.q.shape).contiguous()


@pytest.fixture(scope="module")
def batch(dev):
    return Inputs(dev, COUNTS)


@pytest.fixture(scope="module")
def per_call_reference(dev, batch):
    """Per query kind: every video's own ``steps`` run under the per-handle ``set_mass_trace`` -> packed masses [total, L, N], and
    delta of the scores of every chunk (a second engine stepping chunk by chunk).  Computed once, never changed."""
    out = {}
    for kind in ("steps_shared_q", "steps_q_per_chunk"):
        mass = torch.full((batch.total, TL, TN), float("nan"), device=dev)
        dl = np.zeros((batch.total, TL))
        for v, n in enumerate(batch.counts):
            if not n:
                continue
            a, b = int(batch.cu[v]), int(batch.cu[v + 1])
            e = ltm_engine(dev)
            tr = e.set_mass_trace(n)
            e.steps(batch.kbar[a:b].contiguous(), batch.q_rows(kind, v), batch.projs, batch.u[a:b].contiguous())
            e.sync()
            mass[a:b] = tr
            e.set_mass_trace(0)
            walk = ltm_engine(dev)
            qv = batch.q_rows(kind, v)
            for c in range(n):
                walk.steps(batch.kbar[a + c:a + c + 1].contiguous(), qv[c:c + 1].contiguous(), batch.projs,
                           batch.u[a + c:a + c + 1].contiguous())
                for l in range(TL):
                    dl[a + c, l] = delta(walk.last_scores(l, TQ))
        out[kind] = (mass.cpu().numpy(), dl)
    return out


# ---------------------------------------------------------------------------------------------- the packed masses
@pytest.mark.parametrize("path", PATHS)
def test_packed_masses_of_every_lockstep_entry_point(dev, batch, per_call_reference, path):
    """Counts [3, 1, 4, 0, 2] at the cfg1_sticky shape: every row written and finite, a video's last row the bits of ``masses``
    on its engine, every row within 2 delta + EPS of the video's own ``steps`` run under the per-handle trace, the last rows
    within EPS + 2^-22 max|S| of the float64 mirror on the device's own scores; ctx and every B equal the run with the trace
    off bit for bit; one launch more per step while set, none when off or cleared."""
    from infinite_video_amd.engine import trace_videos
    lib = _lib.load()
    plan = build_plan(TT, TN, TAU)
    engines = [ltm_engine(dev) for _ in COUNTS]

    def run():
        n0 = lib.infv_ltm_launch_count()
        ctx = batch.run(path, engines)
        launches = lib.infv_ltm_launch_count() - n0
        torch.cuda.synchronize()
        return ctx, [e.export_state(l)[0].clone() for e in engines if e.has_memory for l in range(TL)], launches

    run()                                                          # (workspaces grow: not counted)
    ctx0, B0, launches0 = run()
    tr = trace_videos(engines, COUNTS)
    assert tuple(tr.mass.shape) == (batch.total, TL, TN) and bool(torch.isnan(tr.mass).all())
    assert tuple(tr.bins.shape) == (batch.total, TL, S) and bool((tr.bins == -1).all())
    ctx1, B1, launches1 = run()
    mass = tr.mass.clone()
    bins = tr.bins.clone()
    tr.stop()
    tr._mass_buf.fill_(float("nan"))
    ctx2, B2, launches2 = run()
    assert bool(torch.isnan(tr.mass).all())                       # cleared: the call wrote no row
    steps = max(COUNTS)
    print(f"{path}: launches off {launches0}, on {launches1}, cleared {launches2} ({steps} lockstep steps)")
    assert launches1 == launches0 + steps and launches2 == launches0
    assert torch.equal(ctx0, ctx1) and torch.equal(ctx0, ctx2)
    assert len(B0) == len(B1) == len(B2) == TL * sum(1 for n in COUNTS if n)
    assert all(torch.equal(a, b) for a, b in zip(B0, B1)) and all(torch.equal(a, b) for a, b in zip(B0, B2))

    assert bool(torch.isfinite(mass).all())                       # every chunk wrote, a video's first included
    got = mass.cpu().numpy()
    np.testing.assert_allclose(got.sum(-1), 1.0, rtol=0, atol=2e-2)
    # the packed draw trace came for free: every drawing chunk wrote its row, a video's first chunk none
    for v, n in enumerate(COUNTS):
        a = int(batch.cu[v])
        if n:
            assert bool((bins[a] == -1).all()) and bool(((bins[a + 1:a + n] >= 0) & (bins[a + 1:a + n] < NB_BINS - 1)).all())
    ref, dl = per_call_reference["steps_q_per_chunk" if path == "steps_q_per_chunk" else "steps_shared_q"]
    worst, worst64 = 0.0, 0.0
    for v, n in enumerate(COUNTS):
        if not n:
            assert not engines[v].has_memory
            continue
        a, b = int(batch.cu[v]), int(batch.cu[v + 1])
        for l in range(TL):
            assert torch.equal(mass[b - 1, l], engines[v].masses(l, TQ)), f"video {v} layer {l}"
            for c in range(a, b):
                err, tol = rel_err(got[c, l], ref[c, l]), 2 * dl[c, l] + EPS
                print(f"{path} video {v} chunk {c - a} layer {l}: relative |packed - per-call trace| = {err:.3e} (bound {tol:.3e})")
                assert err <= tol
                worst = max(worst, err)
            Sl = engines[v].last_scores(l, TQ)
            e64 = rel_err(got[b - 1, l], density.box_masses(Sl, plan.readout_w[:TN], plan.readout_w_out))
            tol64 = EPS + 2.0 ** -22 * float(np.abs(Sl).max())
            print(f"{path} video {v} layer {l}: relative |last row - float64 mirror on the device's scores| = {e64:.3e} (bound {tol64:.3e})")
            assert e64 <= tol64
            worst64 = max(worst64, e64)
    record_parity(f"[videos trace] {path}: packed masses vs per-call steps trace: max relative {worst:.2e}; last rows vs the float64 "
                  f"mirror: {worst64:.2e}; launches {launches0} -> {launches1} over {steps} steps")


def packed_masses(dev, inputs, engines=None, path="consolidate_videos", capacity=None):
    """One traced lockstep call on fresh engines: (mass [total, L, N], ctx, engines)."""
    from infinite_video_amd.engine import trace_videos
    engines = engines or [ltm_engine(dev) for _ in inputs.counts]
    tr = trace_videos(engines, inputs.counts)
    if capacity is not None:
        e0 = engines[0]
        _lib.check(e0.lib.infv_ltm_set_videos_mass_trace(e0._h, C.c_void_p(tr._mass_buf.data_ptr()), capacity))
    ctx = inputs.run(path, engines)
    torch.cuda.synchronize()
    mass = tr.mass.clone()
    tr.stop()
    return mass, ctx, engines


def test_capacity_and_batch_invariance(dev, batch):
    """A capacity below the total leaves the rows at and beyond it NaN and the rows below it as they are with room for all; one
    video's rows have the same bits alone, first, last and between videos of other lengths."""
    full, _, _ = packed_masses(dev, batch)
    part, _, _ = packed_masses(dev, batch, capacity=5)             # video 2 holds rows 4..7: cut inside a video
    assert torch.equal(part[:5], full[:5]) and bool(torch.isnan(part[5:]).all())
    alone = Inputs(dev, [4], seed=31)

    def inside(counts, pos, seed):
        """The video of ``alone`` at position ``pos`` among other videos."""
        mix = Inputs(dev, counts, seed=seed, pooler=None)
        a, b = int(mix.cu[pos]), int(mix.cu[pos + 1])
        for name in ("k", "u", "qc", "kbar"):
            getattr(mix, name)[a:b] = getattr(alone, name)
        return packed_masses(dev, mix)[0][a:b]

    want = packed_masses(dev, alone)[0]
    assert bool(torch.isfinite(want).all())
    for counts, pos, seed in (([4, 2, 1], 0, 32), ([3, 1, 4], 2, 33), ([6, 0, 4, 1], 2, 34)):
        assert torch.equal(inside(counts, pos, seed), want), (counts, pos)


def test_more_videos_than_one_group(dev):
    """260 videos of 1-3 chunks (past the 256 of one workspace group): every video's rows sit at its packed index and equal its
    own traced run alone bit for bit, across the group boundary."""
    from infinite_video_amd.engine import consolidate_videos, trace_videos
    V = 260
    counts = [1 + (v * 7) % 3 for v in range(V)]
    inp = Inputs(dev, counts, seed=11)
    mass, ctx, engines = packed_masses(dev, inp)
    assert bool(torch.isfinite(mass).all())
    alone = ltm_engine(dev)
    tr = trace_videos([alone], [3])
    for v in range(V):
        a, b = int(inp.cu[v]), int(inp.cu[v + 1])
        tr._mass_buf.fill_(float("nan"))
        ref = consolidate_videos([alone], inp.k[a:b], [b - a], inp.q, inp.projs, inp.u[a:b], new_doc=True)
        assert torch.equal(ctx[a:b], ref), f"video {v}"
        assert torch.equal(mass[a:b], tr.mass[:b - a]), f"video {v}"
        assert bool(torch.isnan(tr.mass[b - a:]).all())
    tr.stop()


# ---------------------------------------------------------------------------------------------- fallback and refusals
def test_fallback_serves_the_trace_through_each_handle(dev):
    """N = 48 has a dense plan: the lockstep call runs each video's own ``consolidate``.  The packed rows equal, bit for bit, each
    engine's own ``consolidate`` under ``set_mass_trace`` -- also under a capacity that cuts a video -- and the handles' own
    traces are as empty afterwards as before."""
    N, counts = 48, [3, 0, 1, 4]
    inp = Inputs(dev, counts, seed=41)
    assert ltm_engine(dev, N=N).ensure_plan(TT).dense
    engines = [ltm_engine(dev, N=N) for _ in counts]
    mass, ctx, _ = packed_masses(dev, inp, engines=engines)
    cut, _, _ = packed_masses(dev, inp, engines=[ltm_engine(dev, N=N) for _ in counts], capacity=6)
    assert tuple(mass.shape) == (inp.total, TL, N)
    for v, n in enumerate(counts):
        if not n:
            continue
        a, b = int(inp.cu[v]), int(inp.cu[v + 1])
        single = ltm_engine(dev, N=N)
        tr = single.set_mass_trace(n)
        ref = single.consolidate(inp.k[a:b], inp.q, inp.projs, inp.u[a:b], new_doc=True)
        single.sync()
        assert torch.equal(ctx[a:b], ref) and torch.equal(mass[a:b], tr), f"video {v}"
    assert torch.equal(cut[:6], mass[:6]) and bool(torch.isnan(cut[6:]).all())
    # the per-handle trace fields were restored: a later single call on a handle of the batch writes no trace and a lockstep
    # call is not refused for a left-over per-handle trace
    again = inp.run("consolidate_videos", engines)
    torch.cuda.synchronize()
    assert torch.equal(again, ctx)


def memory_snapshot(engines):
    return [(e.export_state(l)[0].clone(), e.export_state(l)[1].clone()) for e in engines for l in range(TL)], \
           [e.rng_position for e in engines], [e.has_memory for e in engines]


def assert_untouched(engines, snap):
    state, pos, mem = snap
    now, pos1, mem1 = memory_snapshot(engines)
    assert pos1 == pos and mem1 == mem
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(state, now))


def test_refusals_leave_every_memory_alone(dev, batch):
    from infinite_video_amd.engine import LTMEngine
    counts = [2, 3]
    inp = Inputs(dev, counts, seed=51)
    engines = [ltm_engine(dev) for _ in counts]
    inp.run("consolidate_videos", engines)
    torch.cuda.synchronize()
    snap = memory_snapshot(engines)
    lib = engines[0].lib
    buf = torch.full((inp.total, TL, TN), float("nan"), device=dev)
    ptr = C.c_void_p(buf.data_ptr())
    # a videos trace on a handle that is not the lead: loud, not silently empty
    assert lib.infv_ltm_set_videos_mass_trace(engines[1]._h, ptr, inp.total) == 0
    for path in PATHS:
        for new_doc in (True, False):
            with pytest.raises(_lib.LTMError) as e:
                inp.run(path, engines, new_doc=new_doc)
            assert e.value.code == INVALID and "videos mass trace" in str(e.value)
    torch.cuda.synchronize()
    assert_untouched(engines, snap)
    assert bool(torch.isnan(buf).all())
    assert lib.infv_ltm_set_videos_mass_trace(engines[1]._h, None, 0) == 0
    # the old per-handle trace is still refused, exactly as before
    engines[1].set_mass_trace(4)
    with pytest.raises(_lib.LTMError) as e:
        inp.run("consolidate_videos", engines)
    assert e.value.code == UNSUPPORTED
    engines[1].set_mass_trace(0)
    torch.cuda.synchronize()
    assert_untouched(engines, snap)
    # bad arguments of the setter
    assert lib.infv_ltm_set_videos_mass_trace(engines[0]._h, ptr, -1) == INVALID
    assert lib.infv_ltm_set_videos_mass_trace(engines[0]._h, None, 3) == INVALID
    assert lib.infv_ltm_set_videos_mass_trace(None, ptr, 3) == INVALID
    # general-psi plans: the setter refuses a handle that holds one, and set_psi_plan refuses a traced handle
    gauss = LTMEngine(64, H, DH, D, P, tau=TAU, sticky=True, n_layers=1, max_q=TQ, device=dev, gaussian_sigmas=[0.03, 0.1])
    assert gauss.ensure_plan(TT).psi
    assert lib.infv_ltm_set_videos_mass_trace(gauss._h, ptr, 1) == UNSUPPORTED
    traced = LTMEngine(64, H, DH, D, P, tau=TAU, sticky=True, n_layers=1, max_q=TQ, device=dev, gaussian_sigmas=[0.03, 0.1])
    assert lib.infv_ltm_set_videos_mass_trace(traced._h, ptr, 1) == 0     # (no plan yet: nothing to refuse)
    with pytest.raises(_lib.LTMError) as e:
        traced.ensure_plan(TT)                                     # registers the psi plan: refused
    assert e.value.code == UNSUPPORTED
    assert lib.infv_ltm_set_videos_mass_trace(traced._h, None, 0) == 0
    assert_untouched(engines, snap)


# ---------------------------------------------------------------------------------------------- the batched source pass
def small_engine(dev, N, L=2, sticky=True):
    """A handle whose only use is its plan tables: the pass reads nothing else of it."""
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(N, 1, 64, 32, 1, tau=TAU, sticky=sticky, n_layers=L, max_q=1, device=dev)


def random_bins(seed, n_chunks, L):
    return np.random.default_rng(seed).integers(0, NB_BINS - 1, size=(n_chunks, L, S)).astype(np.int32)


def raw_videos(eng, counts, T, bins, W, g=1, ld=None, mass=None, attn=None, bad=None, reserved=0, cu=None, n_videos=None, stream=None):
    """The entry point itself; returns its status."""
    ptr = lambda t: None if t is None else t.data_ptr()
    cu = np.ascontiguousarray(cu_of(counts).astype(np.int32) if cu is None else np.asarray(cu, np.int32))
    desc = _lib.SourcesVideosDesc(n_videos=len(cu) - 1 if n_videos is None else n_videos, T=T, frames_per_source=g, reserved=reserved,
                                  ld=W.shape[-1] if ld is None else ld, cu=cu.ctypes.data, bins_all=ptr(bins), W_all=ptr(W),
                                  mass_all=ptr(mass), attn_all=ptr(attn), bad_bins=ptr(bad),
                                  hip_stream=torch.cuda.current_stream(eng.device).cuda_stream if stream is None else stream)
    with torch.cuda.device(eng.device):
        return eng.lib.infv_ltm_source_weights_videos(eng._h, C.byref(desc))


SOURCE_CASES = [  # N, T, g, L, sticky, counts
    (256, 16, 1, 2, True, [6, 1, 13, 3]),        # four tiles for the longest video, early-exit tiles for the others, one single chunk
    (272, 16, 1, 2, True, [5, 2]),               # the 32-column tiles of num_basis above 256
    (256, 16, 16, 2, True, [63, 64, 65]),        # the tile width from both sides
    (64, 8, 2, 2, False, [4, 9]),                # not sticky: bins_all = NULL
    (64, 8, 1, 2, True, [2, 0, 3]),              # a video with no chunk in the middle
]


@pytest.mark.parametrize("N,T,g,L,sticky,counts", SOURCE_CASES)
def test_batched_sources_equal_the_single_video_call_and_the_mirror(dev, N, T, g, L, sticky, counts):
    """``W`` and ``attn`` of every video ``torch.equal`` to ``LTMEngine.source_weights`` on its slice and to the ordered fp32
    mirror; columns at and beyond a video's own M_v are 0 in the wrapper's zero-filled buffers; one launch."""
    from infinite_video_amd.engine import source_weights_videos
    eng = small_engine(dev, N, L, sticky)
    plan = eng.ensure_plan(T)
    assert not plan.dense
    total, cu, per = sum(counts), cu_of(counts), T // g
    bins = random_bins(N + total, total, L)
    dbins = torch.from_numpy(bins).to(dev) if sticky else None
    mass = torch.rand(total, L, N, device=dev, generator=torch.Generator(device=dev).manual_seed(total))
    lib = _lib.load()
    n0 = lib.infv_ltm_launch_count()
    W, attn = source_weights_videos(eng, counts, T, dbins, mass=mass, frames_per_source=g)
    assert lib.infv_ltm_launch_count() - n0 == 1
    assert tuple(W.shape) == (len(counts), L, N, max(counts) * per) and tuple(attn.shape) == (total, L, max(counts) * per)
    for l in range(L):
        want = density.source_weights_videos(plan, bins[:, l] if sticky else None, counts, frames_per_source=g, dtype=np.float32)
        assert torch.equal(W[:, l].cpu(), torch.from_numpy(want)), f"layer {l}"
    for v, n in enumerate(counts):
        a, b = int(cu[v]), int(cu[v + 1])
        if not n:
            assert not bool(W[v].any())
            continue
        bv = dbins[a:b].contiguous() if sticky else torch.empty(n, 0, 0, dtype=torch.int32, device=dev)
        W1, attn1 = eng.source_weights(bv, T, frames_per_source=g, mass=mass[a:b].contiguous())
        assert torch.equal(W[v, :, :, :n * per], W1) and not bool(W[v, :, :, n * per:].any()), f"video {v}"
        assert torch.equal(attn[a:b, :, :n * per], attn1) and not bool(attn[a:b, :, n * per:].any()), f"video {v}"
    W_only = source_weights_videos(eng, counts, T, dbins, frames_per_source=g)
    assert torch.equal(W_only, W)


def test_columns_beyond_a_video_are_not_touched(dev):
    """ld above every M_v, NaN sentinels: columns at and beyond a video's own M_v keep them in W_all and in its rows of attn_all,
    and a video with no chunk writes nothing at all."""
    N, T, L, counts = 256, 16, 2, [5, 0, 9, 1]                   # M_v = 80, 0, 144, 16 in a row stride of 200
    eng = small_engine(dev, N, L)
    eng.ensure_plan(T)
    total, cu, ld = sum(counts), cu_of(counts), 200
    bins = torch.from_numpy(random_bins(5, total, L)).to(dev)
    W = torch.full((len(counts), L, N, ld), float("nan"), device=dev)
    mass = torch.rand(total, L, N, device=dev)
    attn = torch.full((total, L, ld), float("nan"), device=dev)
    assert raw_videos(eng, counts, T, bins, W, mass=mass, attn=attn) == 0
    torch.cuda.synchronize()
    for v, n in enumerate(counts):
        a, b, M = int(cu[v]), int(cu[v + 1]), n * T
        assert bool(torch.isnan(W[v, :, :, M:]).all()) and bool(torch.isfinite(W[v, :, :, :M]).all())
        assert bool(torch.isnan(attn[a:b, :, M:]).all()) and bool(torch.isfinite(attn[a:b, :, :M]).all())
        if n:
            W1 = torch.full((L, N, ld), float("nan"), device=dev)
            a1 = torch.full((n, L, ld), float("nan"), device=dev)
            desc = _lib.SourcesDesc(n_chunks=n, T=T, new_doc=1, frames_per_source=1, col_begin=0, ld=ld)
            p = lambda t: C.c_void_p(t.data_ptr())
            assert eng.lib.infv_ltm_source_weights(eng._h, C.byref(desc), p(bins[a:b].contiguous()), p(W1), p(mass[a:b].contiguous()),
                                                   p(a1), None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
            assert torch.equal(W[v, :, :, :M], W1[:, :, :M]) and torch.equal(attn[a:b, :, :M], a1[:, :, :M])


def test_bad_bins_are_counted_once_per_layer_over_the_videos(dev):
    N, T, L, counts = 256, 16, 2, [3, 13, 2]                      # the middle video has four tiles
    eng = small_engine(dev, N, L)
    plan = eng.ensure_plan(T)
    total, cu = sum(counts), cu_of(counts)
    bins = random_bins(9, total, L)
    for v in range(len(counts)):
        bins[cu[v]] = -1                                          # (first chunks read no bins: not counted)
    bins[cu[1] + 6] = -1                                          # one unwritten row in the middle of the four-tile video
    bins[cu[2] + 1, 1, :10] = NB_BINS - 1                         # and ten out-of-range bins of layer 1 in the last video
    db = torch.from_numpy(bins).to(dev)
    W = torch.full((len(counts), L, N, max(counts) * T), float("nan"), device=dev)
    bad = torch.zeros(L, dtype=torch.int32, device=dev)
    assert raw_videos(eng, counts, T, db, W, bad=bad) == 0
    assert bad.tolist() == [S, S + 10]
    for l in range(L):
        want = density.source_weights_videos(plan, bins[:, l], counts, frames_per_source=1, dtype=np.float32)
        for v, n in enumerate(counts):
            assert torch.equal(W[v, l, :, :n * T].cpu(), torch.from_numpy(want[v, :, :n * T]))
    from infinite_video_amd.engine import source_weights_videos
    with pytest.raises(ValueError, match="unwritten trace row"):
        source_weights_videos(eng, counts, T, db, frames_per_source=1)


def test_more_videos_than_one_launch(dev):
    """515 videos of 1-2 chunks at N 16, T 8 (512 travel in one launch's arguments): two launches, every video the mirror's."""
    from infinite_video_amd.engine import source_weights_videos
    N, T, L, V = 16, 8, 1, 515
    counts = [1 + (v * 5) % 2 for v in range(V)]
    counts[3] = 0
    eng = small_engine(dev, N, L)
    plan = eng.ensure_plan(T)
    total = sum(counts)
    bins = random_bins(13, total, L)
    mass = torch.rand(total, L, N, device=dev)
    lib = _lib.load()
    n0 = lib.infv_ltm_launch_count()
    W, attn = source_weights_videos(eng, counts, T, torch.from_numpy(bins).to(dev), mass=mass, frames_per_source=1)
    assert lib.infv_ltm_launch_count() - n0 == 2
    want = density.source_weights_videos(plan, bins[:, 0], counts, frames_per_source=1, dtype=np.float32)
    assert torch.equal(W[:, 0].cpu(), torch.from_numpy(want))
    _, a64 = density.source_attention_videos(mass[:, 0].cpu().numpy(), plan, bins[:, 0], counts, frames_per_source=1, dtype=np.float32)
    got = attn[:, 0].cpu().numpy().astype(np.float64)
    assert np.array_equal(got != 0, a64 != 0)
    nz = a64 != 0
    assert float((np.abs(got[nz] - a64[nz]) / a64[nz]).max()) <= 2.0 ** -23     # float64 sums of the same fp32 W, rounded once


def test_source_refusals_write_nothing(dev):
    from infinite_video_amd.engine import LTMEngine
    T, L, counts = 8, 2, [2, 1]
    n, sentinel = sum(counts), 12345.0

    def refused(eng, code, N=None, **kw):
        N = eng.Np if N is None else N
        W = kw.pop("W", None)
        W = torch.full((len(counts), L, N, 32), sentinel, device=dev) if W is None else W
        for name in ("mass", "attn"):
            if kw.get(name) is True:
                kw[name] = torch.full((n, L, N if name == "mass" else 32), sentinel, device=dev)
        bins = torch.zeros(n, L, S, dtype=torch.int32, device=dev) if kw.pop("sticky_bins", True) else None
        rc = raw_videos(eng, kw.pop("counts", counts), kw.pop("T", T), bins, W, **kw)
        torch.cuda.synchronize()
        assert rc == code, (rc, eng.lib.infv_ltm_last_error())
        assert bool((W == sentinel).all())
        for name in ("mass", "attn"):
            if kw.get(name) is not None:
                assert bool((kw[name] == sentinel).all())

    eng = small_engine(dev, 64, L)
    eng.ensure_plan(T)
    assert raw_videos(eng, counts, T, torch.zeros(n, L, S, dtype=torch.int32, device=dev), torch.empty(2, L, 64, 32, device=dev)) == 0
    refused(eng, STATE, T=4)                                      # no plan for T
    refused(eng, INVALID, g=3)                                    # g does not divide T
    refused(eng, INVALID, g=0)
    refused(eng, INVALID, ld=12)                                  # ld below the longest video's 16 columns
    refused(eng, INVALID, ld=26, W=torch.full((2, L, 64, 26), sentinel, device=dev))   # no multiple of 4
    refused(eng, INVALID, sticky_bins=False)                      # sticky with NULL bins
    refused(eng, INVALID, mass=True)                              # mass_all without attn_all
    refused(eng, INVALID, attn=True)                              # ... and the other way round
    refused(eng, INVALID, W=torch.full((2 * L * 64 * 32 + 1,), sentinel, device=dev)[1:].view(2, L, 64, 32))   # off a 16-byte boundary
    refused(eng, INVALID, reserved=1)
    refused(eng, INVALID, n_videos=0)
    refused(eng, INVALID, cu=[0, 2, 1])                           # not non-decreasing
    refused(eng, INVALID, cu=[-1, 1, 2])                          # a negative start
    refused(eng, INVALID, cu=[0, 0, 0])                           # no chunk at all
    assert eng.lib.infv_ltm_source_weights_videos(eng._h, None) == INVALID
    desc = _lib.SourcesVideosDesc(n_videos=2, T=T, frames_per_source=1, reserved=0, ld=32, cu=None)
    assert eng.lib.infv_ltm_source_weights_videos(eng._h, C.byref(desc)) == INVALID     # null cu (and null W_all)
    plain = small_engine(dev, 64, L, sticky=False)
    plain.ensure_plan(T)
    refused(plain, INVALID)                                       # bins given to a handle that is not sticky
    dense = small_engine(dev, 96, L)
    assert dense.ensure_plan(T).dense
    refused(dense, UNSUPPORTED)                                   # a dense plan
    gauss = LTMEngine(64, 1, 64, 32, 1, tau=TAU, sticky=True, n_layers=L, max_q=1, device=dev, gaussian_sigmas=[0.03, 0.1])
    assert gauss.ensure_plan(T).psi
    refused(gauss, UNSUPPORTED)                                   # a general-psi plan


# ---------------------------------------------------------------------------------------------- end to end
def rows_per_box(plan):
    m = np.diff(plan.inf_old_ptr).astype(np.int64)
    np.add.at(m, plan.inf_row_box, plan.inf_row_end - plan.inf_row_begin)
    return int(m.max())


def test_traced_batch_gives_every_memory_and_attention_map_back(dev):
    """Three videos of 6 / 2 / 5 chunks at T 16, N 64 through ``consolidate_videos`` under ``trace_videos``, then one batched
    source pass on what was recorded: float64(W_v) pool(k_v) is the video's B (2e-5, max norm), and its attention map is the
    float64 mirror's on the device's own masses within C (m + 1) 2^-24 + 2^-23."""
    from infinite_video_amd.engine import source_weights_videos, trace_videos
    T, N, L, counts = 16, 64, 2, [6, 2, 5]
    engines = [ltm_engine(dev, N=N, L=L, T=T) for _ in counts]
    inp = Inputs(dev, counts, T=T, L=L, seed=61, pooler=engines[0])
    plan = engines[0].ensure_plan(T)
    tr = trace_videos(engines, counts)
    inp.run("consolidate_videos", engines)
    torch.cuda.synchronize()
    bins, mass = tr.bins.clone(), tr.mass.contiguous().clone()
    tr.stop()
    W, attn = source_weights_videos(engines[0], counts, T, bins, mass=mass, frames_per_source=1)
    hb, hm, got = bins.cpu().numpy(), mass.cpu().numpy(), attn.cpu().numpy().astype(np.float64)
    worst_b, worst_a = 0.0, 0.0
    for v, n in enumerate(counts):
        a, b = int(inp.cu[v]), int(inp.cu[v + 1])
        kbar = inp.kbar[a:b].reshape(n * T, D).double()
        bound = n * (rows_per_box(plan) + 1) * 2.0 ** -24 + 2.0 ** -23
        for l in range(L):
            B = engines[v].export_state(l)[0].double()
            err = float((W[v, l, :, :n * T].double() @ kbar - B).abs().max())
            print(f"video {v} layer {l}: max |W pool(k) - B| = {err:.3e} (bound {B_TOL:.0e}, max|B| {float(B.abs().max()):.3f})")
            assert err <= B_TOL
            worst_b = max(worst_b, err)
            _, want = density.source_attention(hm[a:b, l], plan, hb[a:b, l], n, frames_per_source=1)
            g = got[a:b, l, :n * T]
            nz = want != 0
            assert np.array_equal(g != 0, nz)
            ea = float((np.abs(g[nz] - want[nz]) / want[nz]).max())
            print(f"video {v} layer {l}: max relative |attn - float64 mirror| = {ea:.3e} (bound {bound:.3e})")
            assert ea <= bound
            worst_a = max(worst_a, ea)
    record_parity(f"[videos trace] 6/2/5 chunks T 16 N 64: max |float64(W) pool(k) - B| = {worst_b:.2e} (bound {B_TOL:.0e}); attn vs the "
                  f"float64 mirror on the device's masses: max relative {worst_a:.2e}")
    _, norm = source_weights_videos(engines[0], counts, T, bins, mass=mass, frames_per_source=1, normalise=True)
    assert torch.allclose(norm.sum(-1), torch.ones_like(norm[..., 0]), rtol=0, atol=1e-5)


def test_traces_through_the_batched_video_qformer(dev):
    """``InfVideoEncoder.encode_videos`` at the ``qf_small`` shape, 3 videos of 4 / 1 / 3 chunks with ``memories=`` given: the
    lead handle of every layer's lockstep call is video 0's engine of that layer, so ``trace_videos`` over the layer's engines is
    honoured.  Outputs equal with and without the traces bit for bit; every layer's packed masses agree with a per-video
    ``encode_frames_batch`` under per-handle traces within 2 delta + EPS, delta from the scores of the same chunk (a per-chunk
    ``encode_frames`` loop)."""
    from infinite_video_amd.engine import trace_videos
    from infinite_video_amd.video_qformer import InfVideoEncoder, VideoMemory
    from tests.golden.qformer_cases import QF_CASES, qf_inputs
    case = next(c for c in QF_CASES if c.name == "qf_small")
    _, weights = qf_inputs(case)
    T, Q, Ln, counts = case.chunk_T[0], case.n_query, case.n_layers, [4, 1, 3]
    cu = cu_of(counts)

    def model():
        m = InfVideoEncoder(num_video_query_token=Q, hidden_size=case.hidden, llama_hidden=case.proj_out, sticky=case.sticky,
                            num_basis=case.N, tau=case.tau, alpha=case.alpha, num_hidden_layers=Ln)
        m.load_reference_state_dict(weights)
        return m.to(dev)

    gen = torch.Generator(device=dev).manual_seed(71)
    frames = torch.randn(sum(counts), T * case.P, case.hidden, device=dev, generator=gen)
    u = torch.rand(sum(counts), Ln, S, dtype=torch.float64, generator=torch.Generator().manual_seed(71))
    m = model()
    plain = m.encode_videos(frames, counts, new_video=True, u=u, want_hidden=True, memories=[VideoMemory(m, dev) for _ in counts])
    mems = [VideoMemory(m, dev) for _ in counts]
    traces = [trace_videos([mem.engines[l] for mem in mems], counts) for l in range(Ln)]
    traced = m.encode_videos(frames, counts, new_video=True, u=u, want_hidden=True, memories=mems)
    torch.cuda.synchronize()
    for a, b in zip(plain, traced):
        assert torch.equal(a, b)
    masses = [t.mass.clone() for t in traces]
    for t in traces:
        t.stop()
    worst = 0.0
    for l in range(Ln):
        assert bool(torch.isfinite(masses[l]).all()), f"layer {l}: a packed row was not written"
    single, loop = model(), model()                                # (new_video = True resets their memories for every video)
    for v, n in enumerate(counts):
        a, b = int(cu[v]), int(cu[v + 1])
        per_handle = [mod._get_engine(dev, Q).set_mass_trace(n) for mod in single.video_Qformer.ltm_modules]
        single.encode_frames_batch(frames[a:b], new_video=True, u=u[a:b])
        torch.cuda.synchronize()
        for c in range(n):
            loop.encode_frames(frames[a + c:a + c + 1], new_video=(c == 0), u=u[a + c])
            for l, mod in enumerate(loop.video_Qformer.ltm_modules):
                tol = 2 * delta(mod._get_engine(dev, Q).last_scores(0, Q)) + EPS
                err = rel_err(masses[l][a + c, 0].cpu().numpy(), per_handle[l][c, 0].cpu().numpy())
                print(f"video {v} chunk {c} layer {l}: relative |packed - per-handle trace| = {err:.3e} (bound {tol:.3e})")
                assert err <= tol
                worst = max(worst, err)
    record_parity(f"[videos trace] encode_videos qf_small, {counts} chunks x {Ln} layers: packed masses vs per-video encode_frames_batch "
                  f"traces: max relative {worst:.2e}")


# ---------------------------------------------------------------------------------------------- stream order
def test_traced_call_and_source_pass_on_a_side_stream(dev):
    """The method of tests/test_stream_order_gpu.py for the two new calls: every input lives in a buffer that holds a DECOY; on a
    side stream and with no host synchronisation in between the test queues a delay, the good values, a traced
    ``consolidate_videos``, ``infv_ltm_source_weights_videos`` on the traces it fills, clones of the outputs, and the decoys
    again.  Everything must equal the synchronised run bit for bit, and the delay must be four times the host time of the block."""
    from infinite_video_amd.engine import consolidate_videos, trace_videos
    from tests.test_stream_order_gpu import issue_delay
    counts, L = [3, 1, 2], TL
    good, decoy = Inputs(dev, counts, seed=81), Inputs(dev, counts, seed=82)
    total, M = good.total, max(counts) * TT
    delay_ms = 60.0

    def run(side):
        engines = [ltm_engine(dev) for _ in counts]
        bufs = {n: getattr(decoy, n).clone() for n in ("k", "u", "q")}
        W = torch.empty(len(counts), L, TN, M, device=dev)
        attn = torch.empty(total, L, M, device=dev)
        bad = torch.zeros(L, dtype=torch.int32, device=dev)
        tr = trace_videos(engines, counts)

        def sequence():
            ctx = consolidate_videos(engines, bufs["k"], counts, bufs["q"], good.projs, bufs["u"], new_doc=True)
            rc = raw_videos(engines[0], counts, TT, tr.bins, W, mass=tr._mass_buf, attn=attn, bad=bad)
            assert rc == 0
            return ctx

        sequence()                                                 # warm, on the decoys: the workspaces grow here, not under the delay
        torch.cuda.synchronize()
        W.fill_(-7.0); attn.fill_(-7.0); tr._mass_buf.fill_(-7.0); tr.bins.fill_(-1)   # (finite sentinels: torch.equal below)
        torch.cuda.synchronize()
        host_ms = 0.0
        if side:
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                issue_delay(delay_ms)
                t0 = time.perf_counter()
                for n in bufs:
                    bufs[n].copy_(getattr(good, n))
                ctx = sequence()
                outs = [t.clone() for t in (ctx, W, attn, tr.mass, tr.bins, bad)]
                for n in bufs:
                    bufs[n].copy_(getattr(decoy, n))
                host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
        else:
            for n in bufs:
                bufs[n].copy_(getattr(good, n))
            torch.cuda.synchronize()
            ctx = sequence()
            torch.cuda.synchronize()
            outs = [t.clone() for t in (ctx, W, attn, tr.mass, tr.bins, bad)]
        tr.stop()
        return outs, host_ms

    want, _ = run(False)
    again, _ = run(False)
    assert all(torch.equal(a, b) for a, b in zip(want, again))     # the synchronised sequence is deterministic: equality is licensed
    got, host_ms = run(True)
    assert delay_ms >= 4 * host_ms, f"delay too short: {delay_ms} ms against {host_ms:.2f} ms of host time"
    for name, a, b in zip(("ctx", "W", "attn", "mass", "bins", "bad_bins"), want, got):
        assert torch.equal(a, b), name
    assert bool((want[1][0] != -7.0).all()) and bool((want[3] != -7.0).all()) and want[5].tolist() == [0] * L   # the longest video's W and every mass row were written
    # the decoys give other numbers: the comparison can see a misordered fill
    dec = consolidate_videos([ltm_engine(dev) for _ in counts], decoy.k, counts, decoy.q, decoy.projs, decoy.u, new_doc=True)
    assert not torch.equal(dec, want[0])
    record_parity(f"[videos trace] stream order: traced consolidate_videos + source_weights_videos behind a {delay_ms:.0f} ms delay on a "
                  f"side stream equal the synchronised run (host issue time {host_ms:.2f} ms)")
