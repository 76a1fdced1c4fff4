"""fp16 frame tokens through the video Q-former on the MI355X (infv_vqf_set_token_dtype(h, INFV_TOKENS_F16 = 3)).

The contract is that of the bf16 tokens (tests/test_vqf_bf16_gpu.py, whose helpers run here on .half() tensors): for
x = randn(...).half() the library gives the bits it gives for x.float().  An fp16 value is exact in fp32 and exactly hi + lo, the
fp16 token pass applies the fp32 pass's split to the same fp32 value and sums the frame means in the same order, and the
contractions are the same three-product kernels on the same planes."""
import ctypes as C

import pytest
import torch

from tests import test_vqf_bf16_gpu as B
from tests.golden.qformer_cases import qf_inputs

pytestmark = pytest.mark.gpu
DEV = B.DEV
BY_NAME = B.BY_NAME
F16 = 3


def synth_videos_f16(case, T, lens, seed):
    """tests.test_vqf_bf16_gpu.synth_videos with .half() where it has .bfloat16(); the first video also carries fp16 subnormals,
    the smallest normal number and +-0."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)
    fs = [torch.randn(n, T * case.P, case.hidden, device=DEV, generator=gen).half() for n in lens]
    if fs and fs[0].numel() > 7 * 4099:
        edge = torch.tensor([2.0 ** -24, -2.0 ** -24, 2.0 ** -15, 0.0, -0.0, 16.0, 2.0 ** -14], device=DEV).half()
        fs[0].view(-1)[torch.arange(edge.numel(), device=DEV) * 4099] = edge
    us = [torch.rand(n, case.n_layers, 512, dtype=torch.float64, generator=cpu) for n in lens]
    return fs, us


@pytest.fixture(autouse=True)
def half_tokens(monkeypatch):
    """The helpers of test_vqf_bf16_gpu build their frames with synth_videos: here they get fp16 frames (their "bf16" leg passes
    the tensors as they are, their "f32" leg passes .float())."""
    monkeypatch.setattr(B, "synth_videos", synth_videos_f16)


@pytest.mark.parametrize("name,T,n_chunks,video_lens,exact", B.CONTRACT_CASES)
def test_fp16_tokens_give_the_bits_of_the_fp32_path(name, T, n_chunks, video_lens, exact):
    """Hidden, llama, means and every memory's B, bin masses, drawn bins and probabilities: torch.equal between x (fp16) and
    x.float() through encode_frames, encode_frames_batch and encode_videos -- split path with and without the wide kernel and
    the whole-video cache, the upcast path (160 tokens), exact fp32, alpha = 1."""
    res = B.run_three_entry_points(BY_NAME[name], T, n_chunks, video_lens, seed=301 + T, exact_fp32=exact)
    assert set(res) == {"f32", "bf16"}                   # (the helper's tag for "the tensors as they are": fp16 here)


def test_fp16_tokens_without_the_whole_video_cache_give_the_same_bits(monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB=0 on the fp16 handle only: per-sub-batch token passes, frame means from the LTM's own pooling of
    the fp16 tokens -- against fp32 tokens on a handle with the default budget."""
    B.run_three_entry_points(BY_NAME["qf_small"], 8, 4, [3, 1, 4], seed=331, env_for_bf16={"INFV_VQF_SPLIT_CACHE_GB": "0"},
                             monkeypatch=monkeypatch)


def test_ragged_encode_long_videos_with_tails():
    """Videos of 20, 16, 5 and 10 frames at max_int 8 (tails of 4, 5 and 2 frames: 128, 160, 64 tokens -- split and upcast paths)."""
    from infinite_video_amd.video_qformer import encode_long_videos
    case = BY_NAME["qf_small"]
    _, weights = qf_inputs(case)
    gen = torch.Generator(device=DEV).manual_seed(341)
    videos = [torch.randn(F, case.P, case.hidden, device=DEV, generator=gen).half() for F in (20, 16, 5, 10)]
    got = {}
    for tag in ("f32", "f16"):
        m = B.make_model(case, weights)
        torch.manual_seed(1234)
        out = encode_long_videos(m, [v if tag == "f16" else v.float() for v in videos], 8)
        torch.cuda.synchronize()
        got[tag] = ([t.cpu() for mean, embs in out for t in [mean] + list(embs)],
                    [s for mem in m._video_memories[:len(videos)] for s in B.engine_state(mem.engines, case)])
    B.assert_same(got["f16"][0], got["f32"][0], "encode_long_videos")
    B.assert_same_state(got["f16"][1], got["f32"][1], "encode_long_videos memories")


def test_c_abi_takes_the_fp16_pointer_itself():
    """infv_vqf_set_token_dtype(h, 3) + infv_vqf_encode_chunk on the fp16 tensor's data_ptr(): the bits of the fp32 call on the
    same values, and of InfVideoEncoder.encode_frames."""
    from infinite_video_amd import _lib
    case = BY_NAME["qf_small"]
    T = 8
    (x,), _ = synth_videos_f16(case, T, [1], seed=351)
    assert x.dtype == torch.float16
    m, lib, h, handles, w, keep = B._raw_setup(case, T)
    xf = x.float()
    _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    rc, hid32, lla32 = B._chunk_call(m, lib, h, handles, xf.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0, lib.infv_ltm_last_error()
    _lib.check(lib.infv_vqf_set_token_dtype(h, F16))
    rc, hid16, lla16 = B._chunk_call(m, lib, h, handles, x.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0, lib.infv_ltm_last_error()
    B.assert_same([hid16, lla16], [hid32, lla32], "encode_chunk through the C ABI")
    _, weights = qf_inputs(case)
    hidden, llama = B.make_model(case, weights).encode_frames(x, new_video=True)
    torch.cuda.synchronize()
    B.assert_same([hid16, lla16], [hidden, llama], "C ABI vs encode_frames")
    del keep


def test_refusals_launch_nothing():
    """An fp16 pointer 2, 4, 8 or 14 bytes off a 16-byte boundary: INFV_ERR_INVALID (-1) and no launch; the handle keeps fp16 and
    the aligned pointer then runs."""
    from infinite_video_amd import _lib
    case = BY_NAME["qf_small"]
    T = 8
    m, lib, h, handles, w, keep = B._raw_setup(case, T)
    n = T * case.P * case.hidden
    store = torch.randn(2 * n + 64, device=DEV).half()
    assert store.data_ptr() % 16 == 0
    _lib.check(lib.infv_vqf_set_token_dtype(h, F16))
    torch.cuda.synchronize()
    before = lib.infv_ltm_launch_count()
    for off in (1, 2, 4, 7):                                   # elements: 2, 4, 8, 14 bytes off a 16-byte boundary
        ptr = store.data_ptr() + 2 * off
        rc, _, _ = B._chunk_call(m, lib, h, handles, ptr, T, w, None, case.n_query, case)
        assert rc == -1 and b"16-byte" in lib.infv_ltm_last_error(), off
        llama = torch.empty(2, case.n_query, case.proj_out, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        assert lib.infv_vqf_encode_video(h, handles, C.c_void_p(ptr), 2, T, C.byref(w), None, 1, None,
                                         C.c_void_p(llama.data_ptr()), None, stream) == -1
    assert lib.infv_vqf_set_token_dtype(h, 2) == -1            # still no code
    assert lib.infv_ltm_launch_count() == before
    rc, hid16, lla16 = B._chunk_call(m, lib, h, handles, store.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0 and lib.infv_ltm_launch_count() > before
    _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    xf = store[:n].float()
    rc, hid32, lla32 = B._chunk_call(m, lib, h, handles, xf.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0
    B.assert_same([hid16, lla16], [hid32, lla32], "after the refusals")
    del keep


def test_batched_videochat2_path_refuses_fp16_tokens():
    """infv_vqf_vc_encode_videos under code 3: INFV_ERR_UNSUPPORTED (-2) before any device work, as for bf16; the memories keep
    their state and the call runs again once the handle is back on fp32."""
    import numpy as np
    from infinite_video_amd import _lib
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    from tests import test_vc_videos_gpu as V
    dev = V.dev0()
    s, w, m = V.small_setup(dev)
    lib = _lib.load()
    nx = V.n_cross_of(s)
    k, h0 = V.small_video(s, 0, 2, 5)
    mems = [VideoChat2Memory(m, dev), VideoChat2Memory(m, dev)]
    u = torch.from_numpy(np.random.default_rng(1).random((4, nx, V.S)))
    kk = torch.from_numpy(np.concatenate([k, k])).to(dev)
    m.encode_videos([kk[:2], kk[2:]], hidden_in=torch.from_numpy(h0), u=u, memories=mems)
    torch.cuda.synchronize()
    before = [V.memory_bits(mem) for mem in mems]
    h = m._vc_handle(dev)
    wts, keep = m._vc_weights(dev)
    hin = torch.from_numpy(np.concatenate([h0, h0])).to(dev)
    ud = u.to(dev)
    proj = torch.empty(4, s["n_query"], s["proj"], device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    k16 = kk.half()

    def call(frames):
        hs = (C.c_void_p * (2 * nx))(*[e._h for mem in mems for e in mem.engines])
        cu_a, tl = (C.c_int32 * 3)(0, 2, 4), (C.c_int32 * 2)(5, 5)
        with torch.cuda.device(dev):
            return lib.infv_vqf_vc_encode_videos(h, hs, 2, C.cast(cu_a, C.c_void_p), C.c_void_p(frames.data_ptr()), s["T"],
                                                 C.byref(wts), C.c_void_p(hin.data_ptr()), C.cast(tl, C.c_void_p),
                                                 C.c_void_p(ud.data_ptr()), 0, None, C.c_void_p(proj.data_ptr()), None, stream)

    _lib.check(lib.infv_vqf_set_token_dtype(h, F16))
    try:
        torch.cuda.synchronize()
        n0 = lib.infv_ltm_launch_count()
        assert call(k16) == -2
        assert lib.infv_ltm_launch_count() == n0
    finally:
        _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    torch.cuda.synchronize()
    for mem, was in zip(mems, before):
        assert mem.has_memory
        for x, y in zip(V.memory_bits(mem), was):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert call(kk) == 0, lib.infv_ltm_last_error()
    torch.cuda.synchronize()
    del keep


def test_no_hidden_upcast_and_no_extra_launches_at_the_headline_shape():
    """Warm encode_frames_batch / encode_videos on PACKED fp16 frames at the headline chunk shape: torch's peak allocation rises by
    less than an fp32 copy of the frames, and the call issues no more launches than on x.float()."""
    from infinite_video_amd import _lib
    from infinite_video_amd.video_qformer import VideoMemory
    case = BY_NAME["qf_headline"]
    T, counts = 256, [3, 1, 4]
    _, weights = qf_inputs(case)
    m = B.make_model(case, weights)
    lib = _lib.load()
    (x,), (u,) = synth_videos_f16(case, T, [sum(counts)], seed=371)
    x32 = x.float()
    fp32_copy = x.numel() * 4
    mems = [VideoMemory(m, DEV) for _ in counts]

    def batch(frames):
        return m.encode_frames_batch(frames, new_video=True, u=u)

    def videos(frames):
        return m.encode_videos(frames, counts, new_video=True, u=u, memories=mems)

    for name, call in (("encode_frames_batch", batch), ("encode_videos", videos)):
        launches = {}
        for tag, frames in (("f32", x32), ("f16", x)):
            call(frames)                                               # warm: workspaces, plans, the handle's buffers
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(DEV)
            base = torch.cuda.memory_allocated(DEV)
            n0 = lib.infv_ltm_launch_count()
            out = call(frames)
            torch.cuda.synchronize()
            launches[tag] = lib.infv_ltm_launch_count() - n0
            rise = torch.cuda.max_memory_allocated(DEV) - base
            del out
            print(f"{name} {tag}: peak rise {rise} B (an fp32 copy of the frames: {fp32_copy} B), {launches[tag]} launches")
            if tag == "f16":
                assert rise < fp32_copy, (name, rise, fp32_copy)
        assert launches["f16"] <= launches["f32"], (name, launches)
