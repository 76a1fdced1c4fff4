"""The lockstep calls over videos whose LAST chunk is short (infv_ltm_videos_tail; engine.consolidate_videos_frames /
steps_videos_frames) on the MI355X.

The yardstick everywhere is the EXISTING entry points run as the two-step form the header states: ``consolidate_videos`` (or
``steps_videos``) on every video's full chunks, then the same entry point with T = the tail length on its last chunk (new_doc = 0,
or the call's new_doc where that chunk is the video's only one).  ctx rows, exported state, draws, scores, traces and the rng
position are compared with ``torch.equal`` / array equality, never against a second run of the new call alone."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, synth
from oracle import ltm_oracle as O
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

TAU = 0.75
DH = 64
INVALID, NO_PLAN, STATE = -1, -3, -4
CTX_TOL, B_TOL = 1e-4, 2e-5                       # tests/test_multi_video_gpu.py's


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class Shape:
    def __init__(self, T, P, d, N, H=1, L=2, Q=4, S=8, sticky=True):
        self.T, self.P, self.d, self.N, self.H, self.L, self.Q, self.S, self.sticky = T, P, d, N, H, L, Q, S, sticky
        self.dm = H * DH

    def engine(self, dev, **kw):
        from infinite_video_amd.engine import LTMEngine
        return LTMEngine(self.N, self.H, DH, self.d, self.P, tau=TAU, sticky=self.sticky, n_layers=self.L, max_q=self.Q, device=dev,
                         nb_samples=self.S, **kw)


BASE = Shape(T=4, P=2, d=32, N=16)
BASE_COUNTS, BASE_TAILS = [3, 1, 2, 0, 1, 2], [2, 4, 3, 0, 3, 2]


def frames_of(counts, tails, T):
    return [0 if c == 0 else (c - 1) * T + t for c, t in zip(counts, tails)]


class Batch:
    """Tokens packed by frame, their frame means, uniforms, a shared and a per-chunk query and the projections; made once."""

    def __init__(self, dev, sh, frames, seed=3):
        from infinite_video_amd.engine import split_frames
        self.sh, self.frames = sh, list(frames)
        self.counts, self.tails, self.cu, self.frame0 = split_frames(frames, sh.T)
        self.total, self.n_frames = int(self.cu[-1]), int(self.frame0[-1])
        self.n_full = [c - 1 if (c and t != sh.T) else c for c, t in zip(self.counts, self.tails)]
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.k = torch.randn(self.n_frames, sh.P, sh.d, device=dev, generator=gen) * 0.5
        self.u = torch.rand(self.total, sh.L, sh.S, device=dev, dtype=torch.float64, generator=gen) if sh.sticky else None
        self.q = torch.from_numpy(np.stack([synth.layer_query(l, sh.Q, sh.dm) for l in range(sh.L)])).to(dev)
        self.qc = torch.randn(self.total, sh.L, sh.Q, sh.dm, device=dev, generator=gen)
        self.ws = [synth.layer_projections(l, sh.d, sh.dm) for l in range(sh.L)]
        self.projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in self.ws]
        self._kbar = None

    def kbar(self, dev):
        if self._kbar is None:                       # frame means of the library's own pooling kernel, per frame
            self._kbar = self.sh.engine(dev).pool(self.k).reshape(self.n_frames, self.sh.d).contiguous()
        return self._kbar


class Traces:
    """Packed draw / mass traces armed by hand on the existing entry points (rows by packed chunk)."""

    def __init__(self, dev, sh, total, Np):
        self.bins = torch.full((total, sh.L, sh.S), -1, device=dev, dtype=torch.int32)
        self.probs = torch.zeros(total, sh.L, 128, device=dev)
        self.mass = torch.full((total, sh.L, Np), float("nan"), device=dev)


def run_new(dev, b, engines, form="tokens", new_doc=True, k=None, frames=None):
    """The call under test.  form: tokens | kbar (shared query) | kbar_qc (a query per chunk)."""
    from infinite_video_amd.engine import consolidate_videos_frames, steps_videos_frames
    frames = b.frames if frames is None else frames
    if form == "tokens":
        ctx, cu = consolidate_videos_frames(engines, b.k if k is None else k, frames, b.sh.T, b.q, b.projs, b.u, new_doc=new_doc)
    else:
        ctx, cu = steps_videos_frames(engines, b.kbar(dev), frames, b.sh.T, b.qc if form == "kbar_qc" else b.q, b.projs, b.u,
                                      new_doc=new_doc)
    assert cu.tolist() == b.cu.tolist()
    return ctx


def run_two_step(dev, b, engines, form="tokens", new_doc=True, k=None, traces=None):
    """The yardstick: the existing lockstep entry points on the full chunks, then on the last chunks at their own length (one call
    per tail length and new_doc value: a video's bits do not depend on the batch)."""
    from infinite_video_amd.engine import consolidate_videos, steps_videos
    sh = b.sh
    x = (b.k if k is None else k) if form == "tokens" else b.kbar(dev)
    ctx = torch.full((b.total, sh.L, sh.Q, sh.dm), float("nan"), device=dev)

    def call(vs, Tc, off, n, nd):
        rows = [torch.arange(int(b.cu[v]) + off[v], int(b.cu[v]) + off[v] + n[v], device=dev) for v in vs]
        rows = torch.cat(rows)
        parts = []
        for v in vs:
            f0 = int(b.frame0[v]) + off[v] * sh.T
            piece = x[f0:f0 + n[v] * Tc]
            parts.append(piece.reshape(n[v], Tc * sh.P, sh.d) if form == "tokens" else piece.reshape(n[v], Tc, sh.d))
        xs = torch.cat(parts).contiguous()
        us = b.u[rows].contiguous() if b.u is not None else None
        es = [engines[v] for v in vs]
        counts = [n[v] for v in vs]
        tmp = None
        if traces is not None:
            at = 0
            for v in vs:
                r = int(b.cu[v]) + off[v]
                _lib.check(es[0].lib.infv_ltm_set_trace(engines[v]._h, _ptr(traces.bins[r:]), _ptr(traces.probs[r:]), n[v]))
                at += n[v]
            tmp = torch.full((at, sh.L, traces.mass.shape[2]), float("nan"), device=dev)
            _lib.check(es[0].lib.infv_ltm_set_videos_mass_trace(es[0]._h, _ptr(tmp), at))
        if form == "tokens":
            out = consolidate_videos(es, xs, counts, b.q, b.projs, us, new_doc=nd)
        else:
            out = steps_videos(es, xs, counts, b.qc[rows].contiguous() if form == "kbar_qc" else b.q, b.projs, us, new_doc=nd)
        ctx[rows] = out
        if traces is not None:
            traces.mass[rows] = tmp
            for v in vs:
                _lib.check(es[0].lib.infv_ltm_set_trace(engines[v]._h, None, None, 0))
            _lib.check(es[0].lib.infv_ltm_set_videos_mass_trace(es[0]._h, None, 0))

    V = len(b.frames)
    zero = [0] * V
    full = [v for v in range(V) if b.n_full[v] > 0]
    if full:
        call(full, sh.T, zero, b.n_full, new_doc)
    groups = {}
    for v in range(V):
        if b.counts[v] > b.n_full[v]:
            groups.setdefault((b.tails[v], bool(new_doc) and b.n_full[v] == 0), []).append(v)
    for (t, nd), vs in sorted(groups.items()):
        call(vs, t, b.n_full, [1] * V, nd)
    return ctx


def state_of(e, sh):
    """Everything a handle exports after a call (host copies), or None for a handle without memory."""
    if not e.has_memory:
        return None
    out = {"pos": e.rng_position}
    for l in range(sh.L):
        B, mass = e.export_state(l)
        out[f"B{l}"], out[f"mass{l}"] = B.cpu(), mass.cpu()
        out[f"scores{l}"] = torch.from_numpy(e.last_scores(l, sh.Q).copy())
        out[f"masses{l}"] = e.masses(l, sh.Q).cpu()
        if sh.sticky:
            bins, idx, probs = e.last_draw(l)
            out[f"bins{l}"], out[f"idx{l}"], out[f"probs{l}"] = torch.from_numpy(bins.copy()), torch.from_numpy(idx.copy()), torch.from_numpy(probs.copy())
    return out


def assert_same_state(a, b, what=""):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a.keys() == b.keys()
    for key in a:
        if key == "pos":
            assert a[key] == b[key], f"{what} rng position"
        else:
            assert torch.equal(a[key], b[key]), f"{what} {key}"


def assert_same_run(dev, b, got_ctx, got_engines, ref_ctx, ref_engines, what=""):
    assert not torch.isnan(ref_ctx).any() and torch.equal(got_ctx, ref_ctx), f"{what} ctx"
    for v, (e, r) in enumerate(zip(got_engines, ref_engines)):
        assert_same_state(state_of(e, b.sh), state_of(r, b.sh), f"{what} video {v}")


def one_more_chunk(dev, b, engines, seed=99):
    """A further full chunk through each handle's own ``forward``: K'/V', the histogram partials and what the handle remembers of its
    last step all enter (only handles that hold a memory)."""
    sh = b.sh
    gen = torch.Generator(device=dev).manual_seed(seed)
    k = torch.randn(sh.T * sh.P, sh.d, device=dev, generator=gen)
    u = torch.rand(sh.L, sh.S, device=dev, dtype=torch.float64, generator=gen) if sh.sticky else None
    return [e.forward(k, b.q, b.projs, u, new_doc=False).cpu() if e.has_memory else None for e in engines]


@pytest.fixture(scope="module")
def base(dev):
    return Batch(dev, BASE, frames_of(BASE_COUNTS, BASE_TAILS, BASE.T))


@pytest.fixture(scope="module")
def base_reference(dev, base):
    """The two-step run of the base case with armed traces: computed once, shared, never changed."""
    engines = [BASE.engine(dev) for _ in base.frames]
    traces = Traces(dev, BASE, base.total, engines[0].Np)
    ctx = run_two_step(dev, base, engines, traces=traces)
    torch.cuda.synchronize()
    return ctx, engines, traces


# ------------------------------------------------------------------------------------------------ 1, 9: base case and traces
def test_base_case_equals_the_two_step_form(dev, base, base_reference):
    """Chunk counts [3,1,2,0,1,2], tails [2,4,3,-,3,2] at T 4: a lone short chunk that starts a document (the tail plan's FIRST
    operator: video 4), a video without frames (3), a full-only video (1), videos sharing a tail length in different steps (tail 3:
    video 4 at step 0, video 2 at step 1; tail 2: video 5 at step 1, video 0 at step 2; many per step: the group-seam test), and
    three plans live in one step (step 1: T 4 for video 0, tail 3 for video 2, tail 2 for video 5)."""
    assert base.counts == BASE_COUNTS and base.tails == BASE_TAILS
    ref_ctx, ref_engines, _ = base_reference
    engines = [BASE.engine(dev) for _ in base.frames]
    ctx = run_new(dev, base, engines)
    assert_same_run(dev, base, ctx, engines, ref_ctx, ref_engines, "base")
    assert not engines[3].has_memory and [e.rng_position for e in engines if e.has_memory] == [3, 1, 2, 1, 2]
    again = [BASE.engine(dev) for _ in base.frames]                  # (stepped on: the shared reference stays as it is)
    assert torch.equal(run_two_step(dev, base, again), ref_ctx)
    for a, r in zip(one_more_chunk(dev, base, engines), one_more_chunk(dev, base, again)):
        assert (a is None and r is None) or torch.equal(a, r)


def test_traces_across_tails(dev, base, base_reference):
    """``trace_videos`` around the new call: packed draw rows and packed mass rows equal those the existing entry points write in
    the two-step form; a video's last mass row has the bits of infv_ltm_masses on its handle."""
    from infinite_video_amd.engine import trace_videos
    _, _, want = base_reference
    engines = [BASE.engine(dev) for _ in base.frames]
    tr = trace_videos(engines, base.counts)
    run_new(dev, base, engines)
    torch.cuda.synchronize()
    assert torch.equal(tr.bins, want.bins) and torch.equal(tr.probs, want.probs)
    assert torch.equal(torch.nan_to_num(tr._mass_buf, nan=-1.0), torch.nan_to_num(want.mass, nan=-1.0))
    assert not torch.isnan(tr.mass).any()
    for v, e in enumerate(engines):
        if base.counts[v]:
            for l in range(BASE.L):
                assert torch.equal(tr.mass[int(base.cu[v + 1]) - 1, l], e.masses(l, BASE.Q)), (v, l)
    drew = [int(base.cu[v]) + c for v in range(len(engines)) for c in range(1, base.counts[v])]
    assert bool((tr.bins[drew] >= 0).all()) and bool((tr.bins[[int(base.cu[v]) for v in (0, 1, 2, 4, 5)]] == -1).all())
    tr.stop()


# ------------------------------------------------------------------------------------------------ 2: other shapes
@pytest.mark.parametrize("d", [96, 288])
def test_other_shapes(dev, d):
    """T 16, N 64, tails 2 and 15, P 3 (the pooling unroll's remainder loop), d 96 (one partial 256-float slice) and 288 (two slices,
    the second partial), L 1, Q 96."""
    sh = Shape(T=16, P=3, d=d, N=64, L=1, Q=96, S=64)
    b = Batch(dev, sh, frames_of([3, 1, 2, 2, 1], [2, 15, 16, 15, 2], 16), seed=5)
    ref_e, new_e = [sh.engine(dev) for _ in b.frames], [sh.engine(dev) for _ in b.frames]
    assert_same_run(dev, b, run_new(dev, b, new_e), new_e, run_two_step(dev, b, ref_e), ref_e, f"d={d}")


# ------------------------------------------------------------------------------------------------ 3: half and fp8 tokens
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float8_e4m3fn], ids=["bf16", "fp16", "fp8"])
def test_narrow_tokens_give_the_bits_of_their_fp32_values(dev, base, dtype):
    kw = {"fp16_tokens": True} if dtype == torch.float16 else {}
    kn = base.k.cpu().to(dtype)                        # (rounded on the host: the device only ever sees the narrow values)
    k32, kn = kn.float().to(dev), kn.to(dev)
    e32, en, ref = ([BASE.engine(dev, **kw) for _ in base.frames] for _ in range(3))
    c32 = run_new(dev, base, e32, k=k32)
    cn = run_new(dev, base, en, k=kn)
    assert_same_run(dev, base, cn, en, c32, e32, str(dtype))
    assert_same_run(dev, base, cn, en, run_two_step(dev, base, ref, k=kn), ref, f"{dtype} two-step")     # the yardstick, on the same tokens


# ------------------------------------------------------------------------------------------------ 4: batch invariance
def test_batch_invariance(dev, base, base_reference):
    """Every video alone, inside the batch and in the reversed batch: equal bits (the batch itself is checked against the two-step
    form in the base case)."""
    ref_ctx, ref_engines, _ = base_reference
    V = len(base.frames)
    order = list(range(V))[::-1]
    from infinite_video_amd.engine import consolidate_videos_frames
    k_rev = torch.cat([base.k[int(base.frame0[v]):int(base.frame0[v + 1])] for v in order])
    u_rev = torch.cat([base.u[int(base.cu[v]):int(base.cu[v + 1])] for v in order])
    e_rev = [BASE.engine(dev) for _ in order]
    ctx_rev, cu_rev = consolidate_videos_frames(e_rev, k_rev, [base.frames[v] for v in order], BASE.T, base.q, base.projs, u_rev)
    for i, v in enumerate(order):
        a, bb = int(base.cu[v]), int(base.cu[v + 1])
        assert torch.equal(ctx_rev[int(cu_rev[i]):int(cu_rev[i + 1])], ref_ctx[a:bb]), f"reversed, video {v}"
        assert_same_state(state_of(e_rev[i], BASE), state_of(ref_engines[v], BASE), f"reversed, video {v}")
        if base.frames[v] == 0:
            continue
        alone = BASE.engine(dev)
        f0, f1 = int(base.frame0[v]), int(base.frame0[v + 1])
        ctx1, _ = consolidate_videos_frames([alone], base.k[f0:f1].contiguous(), [base.frames[v]], BASE.T, base.q, base.projs,
                                            base.u[a:bb].contiguous())
        assert torch.equal(ctx1, ref_ctx[a:bb]), f"alone, video {v}"
        assert_same_state(state_of(alone, BASE), state_of(ref_engines[v], BASE), f"alone, video {v}")


# ------------------------------------------------------------------------------------------------ 5: continuation
def test_continuation_full_chunks_then_only_the_tails(dev, base, base_reference):
    """The full chunks through the existing ``consolidate_videos``, then the new entry with new_doc = 0 holding only the short
    last chunks: equals one call of the new entry (and so the two-step form)."""
    from infinite_video_amd.engine import consolidate_videos, consolidate_videos_frames
    ref_ctx, ref_engines, _ = base_reference
    V, T = len(base.frames), BASE.T
    engines = [BASE.engine(dev) for _ in base.frames]
    has_full = [v for v in range(V) if base.n_full[v] > 0]
    kf = torch.cat([base.k[int(base.frame0[v]):int(base.frame0[v]) + base.n_full[v] * T].reshape(base.n_full[v], T * BASE.P, BASE.d)
                    for v in has_full])
    rows_f = torch.cat([torch.arange(int(base.cu[v]), int(base.cu[v]) + base.n_full[v]) for v in has_full]).to(dev)
    ctx = torch.full_like(ref_ctx, float("nan"))
    ctx[rows_f] = consolidate_videos([engines[v] for v in has_full], kf, [base.n_full[v] for v in has_full], base.q, base.projs,
                                     base.u[rows_f].contiguous(), new_doc=True)
    # only the videos that continue: 0, 2 and 5 (video 4's lone short chunk starts its document: that is the base case's job)
    cont = [v for v in has_full if base.counts[v] > base.n_full[v]]
    assert cont == [0, 2, 5]
    kt = torch.cat([base.k[int(base.frame0[v]) + base.n_full[v] * T:int(base.frame0[v + 1])] for v in cont])
    rows_t = torch.tensor([int(base.cu[v + 1]) - 1 for v in cont], device=dev)
    out, cu = consolidate_videos_frames([engines[v] for v in cont], kt, [base.tails[v] for v in cont], T, base.q, base.projs,
                                        base.u[rows_t].contiguous(), new_doc=False)
    assert cu.tolist() == [0, 1, 2, 3]
    ctx[rows_t] = out
    for v in has_full:
        a, bb = int(base.cu[v]), int(base.cu[v + 1])
        assert torch.equal(ctx[a:bb], ref_ctx[a:bb]), f"video {v}"
        assert_same_state(state_of(engines[v], BASE), state_of(ref_engines[v], BASE), f"video {v}")


# ------------------------------------------------------------------------------------------------ 6: group seam
def test_more_videos_than_one_group(dev):
    """260 videos (more than the 256 of a workspace group) of 1-2 chunks at T 8, N 16, tails cycling through 2..8."""
    sh = Shape(T=8, P=2, d=32, N=16, L=1)
    counts = [1 + (v * 7) % 2 for v in range(260)]
    tails = [2 + v % 7 for v in range(260)]
    b = Batch(dev, sh, frames_of(counts, tails, 8), seed=11)
    ref_e, new_e = [sh.engine(dev) for _ in b.frames], [sh.engine(dev) for _ in b.frames]
    ref = run_two_step(dev, b, ref_e)
    got = run_new(dev, b, new_e)
    assert not torch.isnan(ref).any() and torch.equal(got, ref)
    for v in list(range(0, 260, 13)) + [254, 255, 256, 257, 259]:
        assert_same_state(state_of(new_e[v], sh), state_of(ref_e[v], sh), f"video {v}")


# ------------------------------------------------------------------------------------------------ 7: frame means
def test_frame_means(dev, base, base_reference):
    """With a query per chunk: bit for bit the two-step ``steps_videos`` form.  With the shared query and kbar = pool(k): bit for
    bit the token form."""
    ref_e, new_e = [BASE.engine(dev) for _ in base.frames], [BASE.engine(dev) for _ in base.frames]
    assert_same_run(dev, base, run_new(dev, base, new_e, form="kbar_qc"), new_e, run_two_step(dev, base, ref_e, form="kbar_qc"), ref_e,
                    "per-chunk queries")
    tok_ctx, tok_engines, _ = base_reference
    shared = [BASE.engine(dev) for _ in base.frames]
    assert_same_run(dev, base, run_new(dev, base, shared, form="kbar"), shared, tok_ctx, tok_engines, "shared query")


# ------------------------------------------------------------------------------------------------ 8: non-sticky
def test_non_sticky_engines(dev):
    sh = Shape(T=4, P=2, d=32, N=16, sticky=False)
    b = Batch(dev, sh, frames_of(BASE_COUNTS, BASE_TAILS, 4), seed=8)
    assert b.u is None
    ref_e, new_e = [sh.engine(dev) for _ in b.frames], [sh.engine(dev) for _ in b.frames]
    assert_same_run(dev, b, run_new(dev, b, new_e), new_e, run_two_step(dev, b, ref_e), ref_e, "non-sticky")
    for a, r in zip(one_more_chunk(dev, b, new_e), one_more_chunk(dev, b, ref_e)):
        assert (a is None and r is None) or torch.equal(a, r)


# ------------------------------------------------------------------------------------------------ 10: CPU oracle
def test_against_the_cpu_oracle(dev, base):
    """tests/test_multi_video_gpu.py's check, over chunks of different lengths: the closed-form oracle walks every video teacher-forced
    on the traced bins; ctx within 1e-4 on every chunk, the oracle's own draw equal to the trace but for a small budget of flips to
    an adjacent bin, final B within 2e-5."""
    from infinite_video_amd.engine import trace_videos
    sh = BASE
    engines = [sh.engine(dev) for _ in base.frames]
    tr = trace_videos(engines, base.counts, masses=False)
    ctx = run_new(dev, base, engines).cpu().numpy()
    bins_all = tr.bins.cpu().numpy()
    tr.stop()
    k, u, qs = base.k.cpu().numpy(), base.u.cpu().numpy(), base.q.cpu().numpy()
    flips = drawn = 0
    worst = 0.0
    for v, e in enumerate(engines):
        if not base.counts[v]:
            continue
        orc = [O.ClosedFormOracle(sh.N, sh.H, DH, TAU, True, *base.ws[l], tokens_per_frame=sh.P, nb_samples=sh.S) for l in range(sh.L)]
        for c in range(base.counts[v]):
            Tc = base.tails[v] if c == base.counts[v] - 1 else sh.T
            f0 = int(base.frame0[v]) + c * sh.T
            kc = k[f0:f0 + Tc].reshape(Tc * sh.P, sh.d)
            row = int(base.cu[v]) + c
            for l in range(sh.L):
                out = orc[l].step(kc, qs[l], new_doc=(c == 0), u=u[row, l] if c else None, bins_override=bins_all[row, l] if c else None)
                err = float(np.abs(out - ctx[row, l]).max())
                print(f"video {v} chunk {c} (T {Tc}) layer {l}: |ctx - oracle| = {err:.3e}")
                assert err <= CTX_TOL, (v, c, l, err)
                worst = max(worst, err)
                if c:
                    dif = orc[l].last_bins != bins_all[row, l]
                    flips += int(dif.sum())
                    drawn += sh.S
                    assert np.abs(orc[l].last_bins[dif] - bins_all[row, l][dif]).max(initial=0) <= 1, "a differing draw is not adjacent"
        for l in range(sh.L):
            np.testing.assert_allclose(e.export_state(l)[0].cpu().numpy(), orc[l].B_past, rtol=0, atol=B_TOL)
    assert flips <= max(4, int(4e-5 * drawn)), f"{flips} flips of {drawn} draws"
    record_parity(f"[videos tail] base case vs the CPU oracle: max |ctx - oracle| {worst:.2e}, {flips} of {drawn} draws differ")


# ------------------------------------------------------------------------------------------------ 11: launch census
def test_launch_census(dev, base):
    """The new call issues exactly the launches ``consolidate_videos`` issues for the same chunk counts -- the table launch of the
    group and, per step, pooling, projection, (draw,) update, attend -- and that count itself is what it has always been."""
    from infinite_video_amd.engine import consolidate_videos
    lib = _lib.load()
    sh = BASE
    full = Batch(dev, sh, [c * sh.T for c in base.counts], seed=4)
    e_new, e_old = [sh.engine(dev) for _ in base.frames], [sh.engine(dev) for _ in base.frames]
    k_old = full.k.reshape(full.total, sh.T * sh.P, sh.d)
    for _ in range(2):                                  # (the second round is counted: plans and workspaces exist)
        n0 = lib.infv_ltm_launch_count()
        run_new(dev, base, e_new)
        n1 = lib.infv_ltm_launch_count()
        consolidate_videos(e_old, k_old, base.counts, full.q, full.projs, full.u, new_doc=True)
        n2 = lib.infv_ltm_launch_count()
    steps = max(base.counts)
    expected = 1 + 4 + 5 * (steps - 1)                  # one table launch (6 videos), step 0 draws nothing
    assert n2 - n1 == expected, "consolidate_videos' own count changed"
    assert n1 - n0 == expected
    from infinite_video_amd.engine import trace_videos
    tr = trace_videos(e_new, base.counts)
    n0 = lib.infv_ltm_launch_count()
    run_new(dev, base, e_new)
    assert lib.infv_ltm_launch_count() - n0 == expected + steps      # six per step with the packed mass trace
    tr.stop()


# ------------------------------------------------------------------------------------------------ 12: refusals
def test_refusals_leave_every_handle_as_it_was(dev, base):
    lib = _lib.load()
    sh = BASE
    V = 3
    frames = [10, 4, 7]                                 # tails 2, 4 (full), 3
    b = Batch(dev, sh, frames, seed=21)
    engines = [sh.engine(dev) for _ in range(V)]
    run_new(dev, b, engines)
    torch.cuda.synchronize()
    before = [state_of(e, sh) for e in engines]
    hs = (C.c_void_p * V)(*[e._h.value for e in engines])
    out = torch.zeros(b.total, sh.L, sh.Q, sh.dm, device=dev)
    proj = engines[0]._proj_array(b.projs)

    def desc(**kw):
        cu = np.asarray(kw.pop("cu", b.cu), np.int32)
        tails = np.asarray(kw.pop("tails", b.tails), np.int32)
        d = _lib.VideosTailDesc(hs=C.cast(kw.pop("hs", hs), C.c_void_p), V=kw.pop("V", V), T=sh.T, cu=cu.ctypes.data, tail_T=tails.ctypes.data,
                                k=_ptr(b.k), kbar=None, q=_ptr(b.q), q_per_chunk=0, Q=sh.Q, proj=C.cast(proj, C.c_void_p), u=_ptr(b.u),
                                new_doc=1, reserved=0, ctx=_ptr(out), hip_stream=None)
        for name, val in kw.items():
            setattr(d, name, val)
        d._keep = (cu, tails)
        return d

    def refused(code, word, **kw):
        n0 = lib.infv_ltm_launch_count()
        d = desc(**kw)
        rc = lib.infv_ltm_videos_tail(C.byref(d))
        msg = lib.infv_ltm_last_error().decode()
        assert rc == code and word in msg, (rc, msg, kw)
        assert lib.infv_ltm_launch_count() == n0, "a kernel was launched before the refusal"
        for v, e in enumerate(engines):                 # new_doc = 1 was asked for: the resets did not happen either
            assert_same_state(state_of(e, sh), before[v], f"after refusal {word!r}, video {v}")

    refused(INVALID, "tail_T[0] = 1", tails=[1, 4, 3])
    refused(INVALID, "tail_T[2] = 5", tails=[2, 4, 5])
    refused(INVALID, "tail_T[1] = -2", tails=[2, -2, 3])
    refused(INVALID, "exactly one of k", kbar=_ptr(b.kbar(dev)))                       # both
    refused(INVALID, "exactly one of k", k=None)                                       # neither
    # a handle without a plan for its tail length, the LAST one
    late = sh.engine(dev)
    late.ensure_plan(sh.T)
    run_new(dev, Batch(dev, sh, [4], seed=22), [late])
    hs_late = (C.c_void_p * V)(engines[0]._h.value, engines[1]._h.value, late._h.value)
    late_before = state_of(late, sh)
    refused(NO_PLAN, "T=3", hs=hs_late)
    assert_same_state(state_of(late, sh), late_before, "the handle without the plan")
    # two handles share tail length 2 but hold different plans for it (another tau for that one plan)
    odd = sh.engine(dev)
    odd.ensure_plan(sh.T)
    odd.tau = 0.9
    odd.ensure_plan(2)
    odd.tau = TAU
    hs_odd = (C.c_void_p * V)(engines[0]._h.value, engines[1]._h.value, odd._h.value)
    refused(INVALID, "with the same tail length", hs=hs_odd, tails=[2, 4, 2])
    # what the lockstep calls have always refused
    refused(INVALID, "is also handle", hs=(C.c_void_p * V)(engines[0]._h.value, engines[1]._h.value, engines[0]._h.value))
    refused(INVALID, "cu is not non-decreasing", cu=[0, 3, 2, 4])
    refused(INVALID, "null argument", q=None)
    refused(INVALID, "Q=", Q=sh.Q + 1)
    fresh = sh.engine(dev)
    fresh.ensure_plan(sh.T), fresh.ensure_plan(3)
    refused(STATE, "holds no memory", hs=(C.c_void_p * V)(engines[0]._h.value, engines[1]._h.value, fresh._h.value), new_doc=0)
    assert not fresh.has_memory


# ------------------------------------------------------------------------------------------------ 13: dense-plan fallback
def test_dense_plan_falls_back_to_the_per_handle_calls(dev):
    """N 48: the plans are dense, the call runs each handle's own ``consolidate`` on the full chunks and then on one chunk at the
    tail length -- equal bits, and the packed mass trace is served through each handle's own."""
    from infinite_video_amd.engine import trace_videos
    sh = Shape(T=4, P=2, d=32, N=48)
    b = Batch(dev, sh, frames_of([3, 1, 2, 0, 1], [2, 4, 3, 0, 3], 4), seed=13)
    engines = [sh.engine(dev) for _ in b.frames]
    assert engines[0].ensure_plan(4).dense and engines[0].ensure_plan(3).dense
    tr = trace_videos(engines, b.counts)
    ctx = run_new(dev, b, engines)
    torch.cuda.synchronize()
    for v, e in enumerate(engines):
        if not b.counts[v]:
            assert not e.has_memory
            continue
        single = sh.engine(dev)
        f0, a = int(b.frame0[v]), int(b.cu[v])
        nf, T = b.n_full[v], sh.T
        mt = single.set_mass_trace(max(nf, 1))
        if nf:
            ref = single.consolidate(b.k[f0:f0 + nf * T].reshape(nf, T * sh.P, sh.d).contiguous(), b.q, b.projs,
                                     b.u[a:a + nf].contiguous(), new_doc=True)
            single.sync()
            assert torch.equal(ctx[a:a + nf], ref), f"video {v}, full chunks"
            assert torch.equal(tr.mass[a:a + nf], mt[:nf, :, :sh.N]), f"video {v}, masses of the full chunks"
        if b.counts[v] > nf:
            t = b.tails[v]
            ref = single.consolidate(b.k[f0 + nf * T:f0 + nf * T + t].reshape(1, t * sh.P, sh.d).contiguous(), b.q, b.projs,
                                     b.u[a + nf:a + nf + 1].contiguous(), new_doc=(nf == 0))
            single.sync()
            assert torch.equal(ctx[a + nf:a + nf + 1], ref), f"video {v}, last chunk"
            assert torch.equal(tr.mass[a + nf], mt[0, :, :sh.N]), f"video {v}, masses of the last chunk"
        single.set_mass_trace(0)
        assert_same_state(state_of(e, sh), state_of(single, sh), f"video {v}")
    tr.stop()


# ------------------------------------------------------------------------------------------------ 14: stream order
def test_call_on_a_side_stream_behind_a_delay(dev, base):
    """The scenario of tests/test_videos_trace_gpu.py: every input lives in a buffer that holds a DECOY; on a non-blocking side
    stream, with no host synchronisation in between, the test queues a delay, the good values, the traced call, clones of its
    outputs and the decoys again.  Everything equals the synchronised run bit for bit."""
    from infinite_video_amd.engine import consolidate_videos_frames, trace_videos
    from tests.test_stream_order_gpu import issue_delay
    sh = BASE
    good, decoy = base, Batch(dev, sh, base.frames, seed=82)
    delay_ms = 60.0

    def run(side):
        engines = [sh.engine(dev) for _ in good.frames]
        bufs = {n: getattr(decoy, n).clone() for n in ("k", "u", "q")}
        tr = trace_videos(engines, good.counts)

        def sequence():
            return consolidate_videos_frames(engines, bufs["k"], good.frames, sh.T, bufs["q"], good.projs, bufs["u"], new_doc=True)[0]

        sequence()                                       # warm, on the decoys: plans and workspaces are made here, not under the delay
        torch.cuda.synchronize()
        tr._mass_buf.fill_(-7.0); tr.bins.fill_(-1); tr.probs.fill_(0.0)
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
                outs = [t.clone() for t in (ctx, tr.mass, tr.bins, tr.probs)]
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
            outs = [t.clone() for t in (ctx, tr.mass, tr.bins, tr.probs)]
        tr.stop()
        return outs, [state_of(e, sh) for e in engines], host_ms

    want, want_state, _ = run(False)
    got, got_state, host_ms = run(True)
    assert delay_ms >= 4 * host_ms, f"delay too short: {delay_ms} ms against {host_ms:.2f} ms of host time"
    for name, a, bb in zip(("ctx", "mass", "bins", "probs"), want, got):
        assert torch.equal(a, bb), name
    for v, (a, bb) in enumerate(zip(want_state, got_state)):
        assert_same_state(a, bb, f"video {v}")
    assert bool((want[1] != -7.0).all())                 # every mass row was written
    # the decoys give other numbers: the comparison can see a misordered fill; and the synchronised run is the two-step form's
    dec = consolidate_videos_frames([sh.engine(dev) for _ in good.frames], decoy.k, good.frames, sh.T, decoy.q, good.projs, decoy.u)[0]
    assert not torch.equal(dec, want[0])
    ref_e = [sh.engine(dev) for _ in good.frames]
    assert torch.equal(want[0], run_two_step(dev, good, ref_e))
    record_parity(f"[videos tail] stream order: traced consolidate_videos_frames behind a {delay_ms:.0f} ms delay on a side stream equals "
                  f"the synchronised run (host issue time {host_ms:.2f} ms)")
