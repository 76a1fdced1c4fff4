"""Several instructions per video over ONE copy of its frame tokens (``infv_vqf_vc_encode_streams`` /
``VideoChat2Encoder.encode_streams``, ``infv_ltm_steps_videos_from``).  The call is defined by one sentence -- its results are
bit for bit those of ``encode_videos`` on videos whose frames are copies of the blocks the streams name -- so every test but
the oracle's is a ``torch.equal`` against that replicated call.  All at the small shape ``BASE``.  Needs a real MI355X: run with
``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from infinite_video_amd import synth
from tests.conftest import record_parity
from tests.golden.seam_cases import BASE, S, n_cross_of, small_reference, small_video
from tests.test_vc_videos_gpu import ATOL, armed, memory_bits, same_bits, small_setup, traced_bins

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -2


def dev0():
    return torch.device("cuda:0")


_setups = {}


def setup(dev, **over):
    """(shape, weights, encoder) of ``BASE`` with ``over``, once per session (the encoder's handle and workspaces are reused)."""
    key = tuple(sorted(over.items()))
    if key not in _setups:
        _setups[key] = small_setup(dev, **over)
    return _setups[key]


def block(s, f, n_chunks):
    """Frame tokens [C, T*P, width] of block ``f``."""
    return small_video(s, f, n_chunks, 0)[0]


def rows(s, v, n_text):
    """Encoder input rows [n_query + n_text, hidden] of stream ``v``'s instruction."""
    return small_video(s, v, 0, n_text)[1]


class Case:
    """F blocks, V streams over them, one explicit u: run through ``encode_streams`` and, replicated, through ``encode_videos``."""

    def __init__(self, dev, s, m, counts, frame_src, texts, seed=1):
        self.dev, self.s, self.m = dev, s, m
        self.frame_src, self.texts = list(frame_src), list(texts)
        self.blocks = [block(s, f, n) for f, n in enumerate(counts)]
        self.h0 = [rows(s, v, t) for v, t in enumerate(texts)]
        self.counts = [counts[f] for f in frame_src]             # chunks per stream
        self.use_ltm = s["alpha"] != 1.0
        self.sticky = self.use_ltm and s["sticky"]
        self.u = np.random.default_rng(seed).random((sum(self.counts), n_cross_of(s), S)) if self.sticky else None
        self.cu = np.concatenate([[0], np.cumsum(self.counts)])

    def memories(self):
        from infinite_video_amd.videochat2_qformer import VideoChat2Memory
        return [VideoChat2Memory(self.m, self.dev) for _ in self.frame_src] if self.use_ltm else None

    def _u(self, lo, hi):
        """Rows of u of chunks [lo, hi) of every stream, packed."""
        if self.u is None:
            return None
        return torch.from_numpy(np.concatenate([self.u[self.cu[v] + lo:self.cu[v] + min(hi, n)] for v, n in enumerate(self.counts)]))

    def run(self, shared, mems=None, lo=0, hi=10 ** 6, new_video=True, pick=None):
        """Chunks [lo, hi) of every block.  Returns per stream (proj, mean, hidden, memory bits) -- of the streams in ``pick`` only,
        if given -- and the memories."""
        mems = mems if mems is not None else self.memories()
        hin = [torch.from_numpy(h) for h in self.h0]
        if shared:
            vids = [torch.from_numpy(b[lo:hi]).to(self.dev) for b in self.blocks]
            proj, mean, hid = self.m.encode_streams(vids, self.frame_src, hidden_in=hin, u=self._u(lo, hi), new_video=new_video,
                                                    memories=mems, want_hidden=True)
        else:
            vids = [torch.from_numpy(self.blocks[f][lo:hi]).to(self.dev) for f in self.frame_src]      # a copy per stream
            proj, mean, hid = self.m.encode_videos(vids, hidden_in=hin, u=self._u(lo, hi), new_video=new_video, memories=mems,
                                                   want_hidden=True)
        torch.cuda.synchronize()
        out, r0 = {}, 0
        for v, f in enumerate(self.frame_src):
            n = len(self.blocks[f][lo:hi])
            if pick is None or v in pick:
                # (a stream without chunks: its mean is undefined and its fresh memory holds nothing)
                out[v] = (proj[r0:r0 + n].cpu(), mean[v].cpu() if n else torch.empty(0), hid[v].cpu(),
                          memory_bits(mems[v]) if mems and (n or lo) else [])
            r0 += n
        return out, mems

    def check(self, tag, pick=None, reuse_memories=False):
        got, mems = self.run(True, pick=pick)
        want, _ = self.run(False, mems=mems if reuse_memories else None, pick=pick)     # (new_video starts a reused memory afresh)
        assert sorted(got) == sorted(want) and len(got) > 0
        for v in got:
            same_bits(got[v], want[v], f"{tag}: stream {v} (block {self.frame_src[v]}, {self.texts[v]} text tokens)")
        return got


# ------------------------------------------------------------------------------------------------ 1. shared == replicated
def test_shared_equals_replicated_bit_for_bit():
    dev = dev0()
    s, w, m = setup(dev)
    case = Case(dev, s, m, counts=(5, 2), frame_src=[0, 1, 0, 0, 1], texts=(9, 5, 0, 17, 40))
    got = case.check("ungrouped streams")
    assert len(got) == 5 and got[0][0].shape[0] == 5 and got[1][0].shape[0] == 2
    assert not torch.equal(got[0][0], got[2][0])                 # the instruction does enter: two streams of one block differ


# ------------------------------------------------------------------------------------------------ 2. the identity map
def test_identity_map_equals_encode_videos():
    dev = dev0()
    s, w, m = setup(dev)
    V = len(BASE["counts"])
    Case(dev, s, m, counts=BASE["counts"], frame_src=range(V), texts=BASE["texts"]).check("frame_src = range(V)")


# ------------------------------------------------------------------------------------------------ 3. siblings
def test_a_stream_does_not_see_its_siblings():
    dev = dev0()
    s, w, m = setup(dev)
    texts = (9, 5, 0, 17, 40)
    full = Case(dev, s, m, counts=(5,), frame_src=[0] * 5, texts=texts)
    alone = None
    for n in (1, 2, 5):                                          # alone, beside 1 sibling, beside 4 siblings of its block
        case = Case(dev, s, m, counts=(5,), frame_src=[0] * n, texts=texts[:n])
        case.u = full.u[:5 * n]                                  # stream 0 keeps its uniforms
        got, _ = case.run(True, pick=(0,))
        if alone is None:
            alone = got[0]
        same_bits(got[0], alone, f"stream 0 among {n} streams of its block")


# ------------------------------------------------------------------------------------------------ 4. the oracle
def test_three_streams_of_one_block_against_the_oracle():
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = setup(dev)
    texts = (9, 0, 17)
    k = block(s, 0, 3)
    vids = [(k, rows(s, v, t)) for v, t in enumerate(texts)]
    runs, u = small_reference(s, w, vids, seed=1700)             # margin-safe uniforms: every drawn bin must agree
    mems = [VideoChat2Memory(m, dev) for _ in vids]
    traces = [armed(mem, len(k)) for mem in mems]
    proj, mean, hid = m.encode_streams([torch.from_numpy(k).to(dev)], [0, 0, 0], hidden_in=[torch.from_numpy(h) for _, h in vids],
                                       u=torch.from_numpy(u), memories=mems, want_hidden=True)
    torch.cuda.synchronize()
    worst = 0.0
    for v, orun in enumerate(runs):
        bins = traced_bins(traces[v])
        for c in range(len(k)):
            got_p, got_h = proj[3 * v + c].cpu().numpy(), hid[v][c].cpu().numpy()
            worst = max(worst, float(np.abs(got_p - orun.proj[c]).max()), float(np.abs(got_h - orun.hidden[c]).max()))
            np.testing.assert_allclose(got_p, orun.proj[c], rtol=0, atol=ATOL, err_msg=f"stream {v} chunk {c}")
            np.testing.assert_allclose(got_h, orun.hidden[c], rtol=0, atol=ATOL, err_msg=f"stream {v} chunk {c} hidden")
            for j, ob in enumerate(orun.bins[c]):
                if ob is not None:
                    assert np.array_equal(bins[c][j], ob), f"stream {v} chunk {c} cross layer {j}: draws differ"
        np.testing.assert_allclose(mean[v].cpu().numpy(), np.mean(np.stack(orun.proj), 0), rtol=0, atol=ATOL)
    record_parity(f"vc streams vs oracle, 3 streams x 3 chunks of one block: max |device - oracle| {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 5. the other paths
@pytest.mark.parametrize("name,over", [("T8_exact_fp32", dict(T=8)), ("alpha1", dict(alpha=1.0)), ("not_sticky", dict(sticky=False))])
def test_other_contraction_paths(name, over):
    dev = dev0()
    s, w, m = setup(dev, **over)
    Case(dev, s, m, counts=(5, 2), frame_src=[0, 1, 0, 0, 1], texts=(9, 5, 0, 17, 40)).check(name)


def test_planes_that_do_not_fit(monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB=0 (read at create): no cached planes, so every sub-batch splits the runs of its source chunks."""
    dev = dev0()
    s, w, m = setup(dev)
    case = Case(dev, s, m, counts=(5, 2), frame_src=[0, 1, 0, 0, 1], texts=(9, 5, 0, 17, 40))
    want, _ = case.run(False)                                    # the replicated call on a handle with the default budget
    monkeypatch.setenv("INFV_VQF_SPLIT_CACHE_GB", "0")
    _, _, fresh = small_setup(dev)
    got, _ = Case(dev, s, fresh, counts=(5, 2), frame_src=[0, 1, 0, 0, 1], texts=(9, 5, 0, 17, 40)).run(True)
    for v in want:
        same_bits(got[v], want[v], f"no plane cache: stream {v}")


# ------------------------------------------------------------------------------------------------ 6. a continued call
def test_continued_call_equals_one_call():
    dev = dev0()
    s, w, m = setup(dev)
    case = Case(dev, s, m, counts=(5,), frame_src=[0, 0, 0], texts=(9, 0, 17))
    whole, _ = case.run(True)
    first, mems = case.run(True, lo=0, hi=2)
    second, _ = case.run(True, mems=mems, lo=2, hi=5, new_video=False)
    for v in whole:
        assert torch.equal(torch.cat([first[v][0], second[v][0]]), whole[v][0]), f"stream {v}: projected rows of the two calls"
        assert torch.equal(torch.cat([first[v][2], second[v][2]]), whole[v][2]), f"stream {v}: hidden rows of the two calls"
        for j, (x, y) in enumerate(zip(second[v][3], whole[v][3])):
            for name, t, w_ in zip(("B", "bin masses", "bins", "probabilities"), x, y):
                assert torch.equal(t, w_), f"continued call: stream {v} cross layer {j}: {name} differ"


# ------------------------------------------------------------------------------------------------ 7. seams
def test_many_streams_across_the_row_blocks_and_sub_batches():
    """One block of 3 chunks read by 90 streams: 270 stream-chunks cross the 128- and 256-chunk row blocks and the sub-batches
    of the short-term attention."""
    dev = dev0()
    s, w, m = setup(dev)
    texts = [(5, 0, 17)[v % 3] for v in range(90)]
    Case(dev, s, m, counts=(3,), frame_src=[0] * 90, texts=texts).check("90 streams", pick=(0, 43, 89), reuse_memories=True)


def test_many_streams_across_the_lockstep_group():
    """One block of 1 chunk read by 260 streams, then a second 1-chunk call that continues them, so that every stream draws: the
    lockstep step runs its videos in groups of 256."""
    dev = dev0()
    s, w, m = setup(dev)
    texts = [(5, 0, 17)[v % 3] for v in range(260)]
    case = Case(dev, s, m, counts=(2,), frame_src=[0] * 260, texts=texts)
    pick = (0, 137, 259)
    res = {}
    mems = case.memories()
    for shared in (True, False):
        a, _ = case.run(shared, mems=mems, lo=0, hi=1, new_video=True, pick=pick)
        b, _ = case.run(shared, mems=mems, lo=1, hi=2, new_video=False, pick=pick)
        res[shared] = (a, b)
    for v in pick:
        # (the first chunk of a video draws nothing, so the reused memories still show the earlier run's last draw after call 0:
        #  the memories are compared after the continued call, where every stream has drawn)
        same_bits(res[True][0][v][:3] + ([],), res[False][0][v][:3] + ([],), f"260 streams, call 0: stream {v}")
        same_bits(res[True][1][v], res[False][1][v], f"260 streams, call 1: stream {v}")


# ------------------------------------------------------------------------------------------------ 8. the device rng
def test_device_rng_equals_explicit_philox_uniforms():
    from infinite_video_amd import philox
    dev = dev0()
    s, w, m = setup(dev)
    nx = n_cross_of(s)
    seed, ids = 4242, [7, 3, 5]
    case = Case(dev, s, m, counts=(5, 4), frame_src=[0, 1, 0], texts=(5, 12, 0))
    hin = [torch.from_numpy(h) for h in case.h0]

    def mirror(v, pos0, n):
        return np.stack([philox.gibbs_uniforms(seed, (ids[v] + 1) * nx + j, pos0, n, 1, S)[:, 0] for j in range(nx)], 1)

    def run(rng):
        m.use_device_rng(seed if rng else None)
        mems = case.memories()
        outs = []
        for (lo, hi), new_video in (((0, 3), True), ((3, 5), False)):
            vids = [torch.from_numpy(b[lo:hi]).to(dev) for b in case.blocks]
            uu = np.concatenate([mirror(v, lo, len(case.blocks[f][lo:hi])) for v, f in enumerate(case.frame_src)])
            before = torch.get_rng_state()
            outs.append(m.encode_streams(vids, case.frame_src, hidden_in=hin, new_video=new_video,
                                         u=None if rng else torch.from_numpy(uu), memories=mems, video_ids=ids, want_hidden=True))
            torch.cuda.synchronize()
            assert torch.equal(torch.get_rng_state(), before)   # nothing is drawn on the host
        return outs, [memory_bits(mem) for mem in mems]

    try:
        got, got_mem = run(True)
        want, want_mem = run(False)
    finally:
        m.use_device_rng(None)
    for call in range(2):
        assert torch.equal(got[call][0], want[call][0]) and torch.equal(got[call][1], want[call][1]), f"call {call}: outputs differ"
        for a, b in zip(got[call][2], want[call][2]):
            assert torch.equal(a, b)
    for a, b in zip(got_mem, want_mem):
        for x, y in zip(a, b):
            for t, w_ in zip(x, y):
                assert torch.equal(t, w_)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_through_the_c_abi_leave_the_memories_alone():
    from infinite_video_amd import _lib
    dev = dev0()
    s, w, m = setup(dev)
    lib = _lib.load()
    nx = n_cross_of(s)
    case = Case(dev, s, m, counts=(3, 2), frame_src=[0, 1], texts=(5, 5))
    _, mems = case.run(True)                                     # every memory holds its video
    before = [memory_bits(mem) for mem in mems]
    h = m._vc_handle(dev)
    wts, keep = m._vc_weights(dev)
    frames = torch.from_numpy(np.concatenate(case.blocks)).to(dev)
    hin = torch.from_numpy(np.concatenate(case.h0)).to(dev)
    ud = torch.from_numpy(case.u).to(dev)
    proj = torch.full((5, s["n_query"], s["proj"]), float("nan"), device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    own = [e._h for mem in mems for e in mem.engines]

    def call(handles=None, cu=(0, 3, 5), fcu=(0, 3, 5), src=(0, 1)):
        hs = (C.c_void_p * (2 * nx))(*(handles or own))
        arrs = [(C.c_int32 * len(x))(*x) for x in (cu, fcu, src, (5, 5))]
        cu_a, fcu_a, src_a, tl = [C.cast(a, C.c_void_p) for a in arrs]
        with torch.cuda.device(dev):
            return lib.infv_vqf_vc_encode_streams(h, hs, 2, cu_a, C.c_void_p(frames.data_ptr()), 2, fcu_a, src_a, s["T"], C.byref(wts),
                                                  C.c_void_p(hin.data_ptr()), tl, C.c_void_p(ud.data_ptr()), 0, None,
                                                  C.c_void_p(proj.data_ptr()), None, stream)

    def refused(code, **kw):
        n0 = lib.infv_ltm_launch_count()
        assert call(**kw) == code, kw
        assert lib.infv_ltm_launch_count() == n0, f"{kw}: a refusal launched a kernel"
        torch.cuda.synchronize()
        for mem, was in zip(mems, before):
            assert mem.has_memory
            for x, y in zip(memory_bits(mem), was):
                for t, w_ in zip(x, y):
                    assert torch.equal(t, w_), f"{kw}: a refusal changed a memory"

    refused(INVALID, src=(-1, 1))
    refused(INVALID, src=(0, 2))                                 # frame_src = F
    refused(INVALID, cu=(0, 2, 4), src=(0, 1))                   # stream 0: 2 chunks on a 3-chunk block
    refused(INVALID, fcu=(1, 3, 5))
    refused(INVALID, fcu=(0, 5, 3))                              # decreasing fcu
    refused(INVALID, handles=own[:-1] + [own[0]])                # a repeated handle
    for dtype in (1, 3):                                         # a bf16 and an fp16 token setting on the handle
        _lib.check(lib.infv_vqf_set_token_dtype(h, dtype))
        try:
            refused(UNSUPPORTED)
        finally:
            _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    n0 = lib.infv_ltm_launch_count()
    assert call() == 0                                           # the valid call (continuing both streams) then runs
    torch.cuda.synchronize()
    assert lib.infv_ltm_launch_count() > n0 and bool(torch.isfinite(proj).all())
    del keep


# ------------------------------------------------------------------------------------------------ 10. the LTM layer alone
def _ltm_engines(dev, s, N, n):
    from infinite_video_amd.engine import LTMEngine
    return [LTMEngine(N, s["heads"], 64, s["enc_width"], s["P"], tau=s["tau"], sticky=True, n_layers=1, max_q=s["n_query"], device=dev)
            for _ in range(n)]


def _ltm_state(e):
    B, mass = e.export_state(0)
    bins, _, probs = e.last_draw(0)
    return B.cpu(), mass.cpu(), torch.from_numpy(bins.copy()), torch.from_numpy(probs.copy())


@pytest.mark.parametrize("N", [32, 48])                          # the lockstep kernels; a dense plan: the per-handle fallback
def test_ltm_steps_videos_from(N):
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import steps_videos
    dev = dev0()
    s = BASE
    T, d, Q, dm = s["T"], s["enc_width"], s["n_query"], s["heads"] * 64
    counts, base, blocks = [3, 2, 3, 2], [2, 0, 2, 0], (2, 3)     # 4 handles onto 2 blocks of frame means: [0, 2) and [2, 5)
    rng = np.random.default_rng(50 + N)
    kbar = torch.from_numpy(rng.standard_normal((sum(blocks), T, d)).astype(np.float32)).to(dev)
    replicated = torch.cat([kbar[b:b + n] for b, n in zip(base, counts)])
    q = torch.from_numpy(rng.standard_normal((sum(counts), 1, Q, dm)).astype(np.float32) * 0.1).to(dev)
    u = torch.from_numpy(rng.random((sum(counts), 1, S))).to(dev)
    projs = [tuple(torch.from_numpy(a).to(dev) for a in synth.layer_projections(0, d, dm))]

    want_e = _ltm_engines(dev, s, N, 4)
    want = steps_videos(want_e, replicated, counts, q, projs, u)
    got_e = _ltm_engines(dev, s, N, 4)
    got = steps_videos(got_e, kbar, counts, q, projs, u, kbar_chunk0=base)
    torch.cuda.synchronize()
    assert bool(got_e[0].ensure_plan(T).dense) == (N == 48)
    assert torch.equal(got, want), "ctx differs from the call on the replicated frame means"
    for v, (a, b) in enumerate(zip(got_e, want_e)):
        for name, x, y in zip(("B", "bin masses", "bins", "probabilities"), _ltm_state(a), _ltm_state(b)):
            assert torch.equal(x, y), f"handle {v}: {name} differ"

    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    proj_arr = got_e[0]._proj_array(projs)
    cu = (C.c_int32 * 5)(0, *np.cumsum(counts).tolist())
    ctx = torch.empty_like(want)

    def raw(engines, kb, chunk0):
        hs = (C.c_void_p * 4)(*[e._h.value for e in engines])
        c0 = None if chunk0 is None else C.cast((C.c_int32 * 4)(*chunk0), C.c_void_p)
        with torch.cuda.device(dev):
            rc = lib.infv_ltm_steps_videos_from(C.cast(hs, C.c_void_p), 4, C.cast(cu, C.c_void_p), C.c_void_p(kb.data_ptr()), c0, T,
                                                C.c_void_p(q.data_ptr()), 1, Q, proj_arr, C.c_void_p(u.data_ptr()), 1,
                                                C.c_void_p(ctx.data_ptr()), stream)
        torch.cuda.synchronize()
        return rc

    null_e = _ltm_engines(dev, s, N, 4)                           # NULL kbar_chunk0 is infv_ltm_steps_videos
    for e in null_e:
        e.ensure_plan(T)
    assert raw(null_e, replicated, None) == 0
    assert torch.equal(ctx, want)
    for a, b in zip(null_e, want_e):
        for x, y in zip(_ltm_state(a), _ltm_state(b)):
            assert torch.equal(x, y)
    was = [_ltm_state(e) for e in got_e]
    n0 = lib.infv_ltm_launch_count()
    assert raw(got_e, kbar, [2, 0, -1, 0]) == INVALID             # a negative base: refused, no handle changes (new_doc = 1 resets nothing)
    assert lib.infv_ltm_launch_count() == n0
    for e, w_ in zip(got_e, was):
        assert e.has_memory
        for x, y in zip(_ltm_state(e), w_):
            assert torch.equal(x, y)
