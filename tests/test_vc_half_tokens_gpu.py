"""fp16 / bf16 frame tokens through the batched VideoChat2 encoder (``infv_vqf_vc_encode_videos_tok`` /
``infv_vqf_vc_encode_streams_tok``, reached through ``VideoChat2Encoder.encode_videos`` / ``encode_streams`` on half-precision
tensors).  The contract is one sentence -- for x of a half-precision dtype the call gives the bits it gives for ``x.float()`` -- so
every comparison is ``torch.equal``: an fp16 value is exactly its bf16 hi + lo planes, a bf16 value is its own hi plane, and the
frame means are summed in token order in fp32 whichever kernel computes them.  Small shapes of ``seam_cases.BASE`` choose the
path: P = 4 (the token pass writes the means), P = 12 and P = 6 with T = 32 (a frame does not divide the 64-token tile: pooling at
the token dtype, then the split), P = 12 with T = 8 (96 tokens: fp32 contractions from an fp32 copy).  A per-frame pass that gave
planes and means in one launch for P = 12 / 196 passed these tests bit for bit with one launch fewer, was measured slower than the
two passes for both dtypes (profiles/vc_half_tokens.jsonl) and was deleted; the census below is therefore "no more launches".
Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import record_parity
from tests.golden.seam_cases import S, n_cross_of, small_video
from tests.test_vc_videos_gpu import memory_bits, same_bits, small_setup

pytestmark = pytest.mark.gpu
INVALID = -1
OVER = {"P4_tile_means": {}, "P12_two_passes": dict(P=12), "P12_T8_upcast": dict(P=12, T=8), "P6_T32_two_passes": dict(P=6, T=32)}
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def dev0():
    return torch.device("cuda:0")


_setups = {}


def setup(dev, name):
    """(shape, weights, encoder) of ``BASE`` with ``OVER[name]``, once per session."""
    if name not in _setups:
        _setups[name] = small_setup(dev, **OVER.get(name, {}))
    return _setups[name]


def half_blocks(s, dev, dtype, counts, first=0):
    """Frame tokens of blocks ``first``.. as ``dtype`` on the device."""
    return [torch.from_numpy(small_video(s, first + f, n, 0)[0]).to(dev).to(dtype) for f, n in enumerate(counts)]


def rows(s, v, n_text):
    return torch.from_numpy(small_video(s, v, 0, n_text)[1])


def memories(m, dev, n):
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    return [VideoChat2Memory(m, dev) for _ in range(n)]


def call(m, blocks, frame_src, hin, u, new_video, mems, lo=0, hi=10 ** 6):
    """Chunks [lo, hi) of every block through encode_videos (frame_src None) or encode_streams.  Returns per stream
    (proj, mean, hidden, memory bits) and the launches the call issued."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    vids = [b[lo:hi] for b in blocks]
    src = list(range(len(blocks))) if frame_src is None else list(frame_src)
    counts = [vids[f].size(0) for f in src]
    cu = np.concatenate([[0], np.cumsum([blocks[f].size(0) for f in src])])
    uu = torch.from_numpy(np.concatenate([u[cu[v] + lo:cu[v] + min(hi, blocks[f].size(0))] for v, f in enumerate(src)]))
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    if frame_src is None:
        proj, mean, hid = m.encode_videos(vids, hidden_in=hin, u=uu, new_video=new_video, memories=mems, want_hidden=True)
    else:
        proj, mean, hid = m.encode_streams(vids, src, hidden_in=hin, u=uu, new_video=new_video, memories=mems, want_hidden=True)
    torch.cuda.synchronize()
    launches = lib.infv_ltm_launch_count() - n0
    out, r0 = [], 0
    for v, n in enumerate(counts):
        out.append((proj[r0:r0 + n].cpu(), mean[v].cpu(), hid[v].cpu(), memory_bits(mems[v])))
        r0 += n
    return out, launches


def both_ways(m_half, m_f32, dev, s, dtype, counts, frame_src, tag, seed):
    """The same blocks as ``dtype`` through ``m_half`` and as ``.float()`` through ``m_f32``: new_video on the first two chunks, then
    the rest continued on the same memories.  Every stream's outputs and memories must be the same bits."""
    blocks = half_blocks(s, dev, dtype, counts)
    src = list(range(len(counts))) if frame_src is None else list(frame_src)
    hin = [rows(s, v, t) for v, t in zip(range(len(src)), (5, 0, 17, 9))]
    u = np.random.default_rng(seed).random((sum(counts[f] for f in src), n_cross_of(s), S))
    got = {}
    for kind, m, bl in (("half", m_half, blocks), ("f32", m_f32, [b.float() for b in blocks])):
        assert all(b.dtype == (dtype if kind == "half" else torch.float32) for b in bl)
        mems = memories(m, dev, len(src))
        first, _ = call(m, bl, frame_src, hin, u, True, mems, 0, 2)       # (two chunks: every memory has drawn once)
        rest, _ = call(m, bl, frame_src, hin, u, False, mems, 2)
        got[kind] = (first, rest)
    for part, name in ((0, "first chunks, new_video"), (1, "continued")):
        for v, (a, b) in enumerate(zip(got["half"][part], got["f32"][part])):
            same_bits(a, b, f"{tag}: {name}: stream {v}")
    return blocks, hin, u


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(OVER))
def test_encode_videos_gives_the_bits_of_the_fp32_call(name, dname):
    """encode_videos([k.to(dtype)]) against encode_videos([k.to(dtype).float()]): proj, mean, hidden states and every memory's
    bits, on a new video and continued -- and the launch census of a warm call."""
    dev = dev0()
    s, w, m = setup(dev, name)
    dtype = DTYPES[dname]
    blocks, hin, u = both_ways(m, m, dev, s, dtype, (3,), None, f"{name} {dname} encode_videos", seed=11)
    launches = {}
    for kind, bl in (("half", blocks), ("f32", [b.float() for b in blocks])):
        _, launches[kind] = call(m, bl, None, hin, u, True, memories(m, dev, 1))
    record_parity(f"vc half tokens {name} {dname}: encode_videos == the fp32 call bit for bit; launches {launches}")
    if name == "P12_T8_upcast":
        # 96 tokens: the issue's design is one launch that writes the fp32 copy, then the fp32 path as it stands
        assert launches["half"] == launches["f32"] + 1, launches
    else:
        assert launches["half"] <= launches["f32"], launches


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(OVER))
def test_encode_streams_gives_the_bits_of_the_fp32_call(name, dname):
    """The same through encode_streams with frame_src = (1, 0, 1) over two blocks."""
    dev = dev0()
    s, w, m = setup(dev, name)
    both_ways(m, m, dev, s, DTYPES[dname], (3, 4), (1, 0, 1), f"{name} {dname} encode_streams", seed=12)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", ["P4_tile_means", "P12_two_passes"])
def test_planes_that_do_not_fit_the_cache_give_the_same_bits(name, dname, monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB so small that no plane fits, on the half-precision encoder's handle only (read at its creation):
    token passes per sub-batch, frame means from infv_ltm_pool at the token dtype; streams split each contiguous run of source
    chunks (bf16: the untransposed operand stays the caller's buffer, read through the map) -- against fp32 tokens on an encoder
    with the default budget."""
    dev = dev0()
    s, w, m_f32 = setup(dev, name)
    m_f32._vc_handle(dev)
    monkeypatch.setenv("INFV_VQF_SPLIT_CACHE_GB", "1e-9")
    _, _, m_half = small_setup(dev, **OVER[name])
    m_half._vc_handle(dev)                                            # created under the small budget
    monkeypatch.delenv("INFV_VQF_SPLIT_CACHE_GB")
    dtype = DTYPES[dname]
    both_ways(m_half, m_f32, dev, s, dtype, (3,), None, f"{name} {dname} no cache, encode_videos", seed=13)
    both_ways(m_half, m_f32, dev, s, dtype, (3, 4), (1, 0, 1), f"{name} {dname} no cache, encode_streams", seed=14)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", ["P4_tile_means", "P12_two_passes", "P12_T8_upcast"])
def test_batch_invariance_of_half_precision_videos(name, dname):
    """A probe video alone and at position 2 of three half-precision videos: the same bits."""
    dev = dev0()
    s, w, m = setup(dev, name)
    dtype = DTYPES[dname]
    blocks = [torch.from_numpy(small_video(s, v, n, 0)[0]).to(dev).to(dtype) for v, n in ((3, 2), (4, 1), (0, 3))]
    hin = [rows(s, v, t) for v, t in ((3, 9), (4, 0), (0, 5))]
    rng = np.random.default_rng(15)
    us = [rng.random((b.size(0), n_cross_of(s), S)) for b in blocks]
    alone, _ = call(m, blocks[2:], None, hin[2:], us[2], True, memories(m, dev, 1))
    batch, _ = call(m, blocks, None, hin, np.concatenate(us), True, memories(m, dev, 3))
    same_bits(batch[2], alone[0], f"{name} {dname}: probe at position 2 of 3")


def test_eval_shape_fp16_reads_the_tokens_in_place():
    """T 16, P 196, width 1024, one block of 2 chunks, fp16, want_hidden=False: the bits of the .float() run, and over a warm call
    torch's peak allocation rises by less than an fp32 copy of the frames."""
    dev = dev0()
    s, w, m = small_setup(dev, P=196, T=16, enc_width=1024)
    k = torch.from_numpy(small_video(s, 0, 2, 0)[0]).to(dev).half()
    assert k.shape == (2, 16 * 196, 1024)
    hin = [rows(s, 0, 5)]
    u = torch.from_numpy(np.random.default_rng(16).random((2, n_cross_of(s), S)))
    fp32_copy = k.numel() * 4
    from infinite_video_amd import _lib
    lib = _lib.load()
    out, launches = {}, {}
    for kind in ("f32", "half"):
        frames = k if kind == "half" else k.float()
        mems = memories(m, dev, 1)
        m.encode_videos([frames], hidden_in=hin, u=u, memories=mems)          # warm: workspaces, plans, the handle's buffers
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        n0 = lib.infv_ltm_launch_count()
        proj, mean, hid = m.encode_videos([frames], hidden_in=hin, u=u, memories=mems, want_hidden=False)
        torch.cuda.synchronize()
        launches[kind] = lib.infv_ltm_launch_count() - n0
        rise = torch.cuda.max_memory_allocated(dev) - base
        assert hid is None
        out[kind] = (proj.cpu(), mean.cpu(), memory_bits(mems[0]))
        record_parity(f"vc half tokens eval shape {kind}: peak rise {rise} B (an fp32 copy of the frames: {fp32_copy} B), "
                      f"{launches[kind]} launches")
        if kind == "half":
            assert rise < fp32_copy, (rise, fp32_copy)
    assert torch.equal(out["half"][0], out["f32"][0]) and torch.equal(out["half"][1], out["f32"][1])
    for x, y in zip(out["half"][2], out["f32"][2]):
        for a, b in zip(x, y):
            assert torch.equal(a, b)
    assert launches["half"] <= launches["f32"], launches


# ------------------------------------------------------------------------------------------------ the raw ABI
class Raw:
    """Two videos of two chunks through the C entry points themselves, on memories that already hold a first call."""

    def __init__(self, name="P12_two_passes"):
        from infinite_video_amd import _lib
        self.dev = dev0()
        self.s, _, self.m = setup(self.dev, name)
        self.lib = _lib.load()
        s, dev = self.s, self.dev
        self.nx = n_cross_of(s)
        k = torch.from_numpy(small_video(s, 0, 4, 0)[0]).to(dev)
        self.k16 = k.half()
        self.k32 = self.k16.float()
        h0 = small_video(s, 0, 0, 5)[1]
        self.hin = torch.from_numpy(np.concatenate([h0, h0])).to(dev)
        self.u = torch.from_numpy(np.random.default_rng(17).random((4, self.nx, S))).to(dev)
        self.h = self.m._vc_handle(dev)
        self.wts, self.keep = self.m._vc_weights(dev)
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fresh(self):
        mems = memories(self.m, self.dev, 2)
        for mem in mems:
            for e in mem.engines:
                e.ensure_plan(self.s["T"])
        return mems

    def run(self, mems, fn, frames_ptr, code=None, new_video=1):
        """rc, launches, (proj, mean, hidden) of one call; ``code`` None: the entry point without the argument."""
        s, dev = self.s, self.dev
        Q = s["n_query"]
        hs = (C.c_void_p * (2 * self.nx))(*[e._h for mem in mems for e in mem.engines])
        cu, tl = (C.c_int32 * 3)(0, 2, 4), (C.c_int32 * 2)(5, 5)
        proj = torch.zeros(4, Q, s["proj"], device=dev)
        mean = torch.zeros(2, Q, s["proj"], device=dev)
        hid = torch.zeros(4 * (Q + 5), s["hidden"], device=dev)
        tok = () if code is None else (code,)
        torch.cuda.synchronize()
        n0 = self.lib.infv_ltm_launch_count()
        with torch.cuda.device(dev):
            rc = getattr(self.lib, fn)(self.h, hs, 2, C.cast(cu, C.c_void_p), C.c_void_p(frames_ptr), *tok, s["T"], C.byref(self.wts),
                                       C.c_void_p(self.hin.data_ptr()), C.cast(tl, C.c_void_p), C.c_void_p(self.u.data_ptr()), new_video,
                                       C.c_void_p(hid.data_ptr()), C.c_void_p(proj.data_ptr()), C.c_void_p(mean.data_ptr()), self.stream)
        torch.cuda.synchronize()
        return rc, self.lib.infv_ltm_launch_count() - n0, (proj.cpu(), mean.cpu(), hid.cpu())


def same_raw(a, b, mems_a, mems_b, tag):
    for x, y, what in zip(a, b, ("proj", "mean", "hidden")):
        assert torch.equal(x, y), f"{tag}: {what} differ"
    for ma, mb in zip(mems_a, mems_b):
        for x, y in zip(memory_bits(ma), memory_bits(mb)):
            for t, w_ in zip(x, y):
                assert torch.equal(t, w_), f"{tag}: memories differ"


def test_raw_abi_code_0_is_the_old_entry_point():
    r = Raw()
    for _ in range(2):                                                # (the second round is warm: equal launch counts)
        ma, mb = r.fresh(), r.fresh()
        rc_a, n_a, out_a = r.run(ma, "infv_vqf_vc_encode_videos", r.k32.data_ptr())
        rc_b, n_b, out_b = r.run(mb, "infv_vqf_vc_encode_videos_tok", r.k32.data_ptr(), 0)
        assert rc_a == 0 and rc_b == 0, r.lib.infv_ltm_last_error()
    assert n_a == n_b, (n_a, n_b)
    same_raw(out_a, out_b, ma, mb, "code 0 against the call without the argument")


def test_raw_abi_ignores_the_handles_token_setting():
    """set_token_dtype(3) on the handle: the _tok call with code 0 still reads fp32 tokens, with code 3 fp16 ones -- and the old
    entry point still refuses while the setting stands."""
    from infinite_video_amd import _lib
    r = Raw()
    ma, mb, mc = r.fresh(), r.fresh(), r.fresh()
    rc, _, want = r.run(ma, "infv_vqf_vc_encode_videos_tok", r.k32.data_ptr(), 0)
    assert rc == 0, r.lib.infv_ltm_last_error()
    _lib.check(r.lib.infv_vqf_set_token_dtype(r.h, 3))
    try:
        rc0, _, got0 = r.run(mb, "infv_vqf_vc_encode_videos_tok", r.k32.data_ptr(), 0)
        rc3, _, got3 = r.run(mc, "infv_vqf_vc_encode_videos_tok", r.k16.data_ptr(), 3)
        rc_old, n_old, _ = r.run(r.fresh(), "infv_vqf_vc_encode_videos", r.k32.data_ptr())
    finally:
        _lib.check(r.lib.infv_vqf_set_token_dtype(r.h, 0))
    assert rc0 == 0 and rc3 == 0, r.lib.infv_ltm_last_error()
    assert rc_old == -2 and n_old == 0
    same_raw(got0, want, mb, ma, "code 0 under a handle set to fp16")
    same_raw(got3, want, mc, ma, "code 3 under a handle set to fp16")


def test_raw_abi_refuses_a_misaligned_fp16_pointer():
    r = Raw()
    mems = r.fresh()
    rc, _, _ = r.run(mems, "infv_vqf_vc_encode_videos_tok", r.k16.data_ptr(), 3)
    assert rc == 0, r.lib.infv_ltm_last_error()
    before = [memory_bits(mem) for mem in mems]
    store = torch.zeros(r.k16.numel() + 8, dtype=torch.float16, device=r.dev)
    assert store.data_ptr() % 16 == 0
    store[1:1 + r.k16.numel()] = r.k16.view(-1)
    for off in (1, 4):                                                # 2 and 8 bytes off a 16-byte boundary
        rc, n, _ = r.run(mems, "infv_vqf_vc_encode_videos_tok", store.data_ptr() + 2 * off, 3, new_video=0)
        assert rc == INVALID and n == 0 and b"16-byte" in r.lib.infv_ltm_last_error(), (off, rc, n)
    for mem, was in zip(mems, before):
        for x, y in zip(memory_bits(mem), was):
            for t, w_ in zip(x, y):
                assert torch.equal(t, w_)
    rc, _, _ = r.run(mems, "infv_vqf_vc_encode_videos_tok", r.k16.data_ptr(), 3, new_video=0)   # the aligned pointer then runs
    assert rc == 0, r.lib.infv_ltm_last_error()
