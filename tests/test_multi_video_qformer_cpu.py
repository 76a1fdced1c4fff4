"""Many videos through the video Q-former in one call (infv_vqf_encode_videos / InfVideoEncoder.encode_videos /
encode_long_videos): symbols and declarations, refusals before any device work, Python argument checks, the uniform draw
order and the split into batched chunks and tails.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")


def test_symbols_and_declarations():
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "infv_vqf.h")).read()
    assert re.search(r"^int infv_vqf_encode_videos\(", header, re.M)
    assert "infv_vqf_encode_videos" in _lib._SIGNATURES
    lib = _lib.load()
    assert len(lib.infv_vqf_encode_videos.argtypes) == 13
    assert hasattr(ctypes.CDLL(LIB), "infv_vqf_encode_videos")


def test_c_refusals_before_device_work():
    """Null arrays and a bad cu are refused without a device; V = 0 is a no-op.  (The handle is never dereferenced on these
    paths, so a dummy pointer stands in for it.)"""
    from infinite_video_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    w = _lib.VqfWeights()
    cu_ok = (ctypes.c_int32 * 3)(0, 1, 2)

    def call(h, V, cu, weights=ctypes.byref(w)):
        return lib.infv_vqf_encode_videos(h, None, V, ctypes.cast(cu, ctypes.c_void_p) if cu is not None else None, None, 8,
                                          weights, None, 1, None, None, None, None)

    assert call(None, 2, cu_ok) == -1
    assert call(fake, 2, None) == -1
    assert call(fake, 2, cu_ok, weights=None) == -1
    assert call(fake, -1, cu_ok) == -1
    assert call(fake, 0, cu_ok) == 0


def test_uniform_draw_order_matches_the_per_video_loop():
    """draw_video_uniforms consumes the global generator as looping encode_frames_batch over the videos does."""
    from infinite_video_amd.video_qformer import NB_SAMPLES, draw_video_uniforms
    counts, continuing, L = [3, 1, 0, 2], [False, True, False, True], 2
    torch.manual_seed(7)
    got = draw_video_uniforms(counts, continuing, L)
    after = torch.get_rng_state()
    torch.manual_seed(7)
    want = []
    for c_v, cont in zip(counts, continuing):           # encode_frames_batch's own loop, per video
        u = torch.zeros(c_v, L, NB_SAMPLES, dtype=torch.float64)
        for c in range(0 if cont else 1, c_v):
            for l in range(L):
                u[c, l] = torch.rand(NB_SAMPLES, dtype=torch.float64)
                torch.rand(NB_SAMPLES, dtype=torch.float64)
        want.append(u)
    assert torch.equal(got, torch.cat(want))
    assert torch.equal(torch.get_rng_state(), after)
    assert (got[0] == 0).all() and (got[1] != 0).all() and (got[3] != 0).all()


def test_split_into_batched_chunks_and_tails():
    from infinite_video_amd.video_qformer import split_long_videos
    assert split_long_videos([20, 16, 5, 9, 0], 8) == [(2, 4), (2, 0), (0, 5), (1, 1), (0, 0)]
    with pytest.raises(ValueError):
        split_long_videos([4], 0)


def test_python_argument_checks():
    from infinite_video_amd.video_qformer import InfVideoEncoder, _check_memories, _video_counts
    with pytest.raises(ValueError, match="at least one"):
        _video_counts([])
    with pytest.raises(ValueError, match="non-negative"):
        _video_counts([2, -1])
    with pytest.raises(ValueError, match="1-D"):
        _video_counts(torch.tensor([[1, 2]]))
    assert _video_counts(torch.tensor([1, 0, 3])) == [1, 0, 3]
    m = InfVideoEncoder(num_video_query_token=32, hidden_size=768, llama_hidden=512, num_basis=64, num_hidden_layers=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode_videos(torch.zeros(2, 8 * 32, 768), [1, 1])
    with pytest.raises(ValueError, match="chunk_counts"):
        m.encode_videos(torch.zeros(2, 8 * 32, 768))
    with pytest.raises(ValueError, match="memories for"):
        _check_memories(m, [], 2, torch.device("cpu"))
    with pytest.raises(TypeError, match="VideoMemory"):
        _check_memories(m, [object()], 1, torch.device("cpu"))
