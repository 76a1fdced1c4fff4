"""fp8 e4m3 frame tokens through the batched VideoChat2 encoder (``infv_vqf_vc_encode_videos_tok`` /
``infv_vqf_vc_encode_streams_tok`` with code 4, reached through ``VideoChat2Encoder.encode_videos`` / ``encode_streams`` on
``torch.float8_e4m3fn`` tensors).  The contract is the one of the half-precision tokens (tests/test_vc_half_tokens_gpu.py, whose
helpers run here): the call gives the bits it gives for ``x.float()``.  An e4m3 value is its own bf16 hi plane, so the token pass
writes F_hi and FT_hi alone and the contractions take their two-product form; the frame means are summed in token order in fp32
whichever kernel computes them.  The shapes choose the path: P = 4 (the tile pass writes the means), P = 6 with T = 32 (pooling
at the token dtype, then the split), P = 12 with T = 8 (96 tokens: fp32 contractions from an fp32 copy).
Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_vc_half_tokens_gpu as H
from tests.golden.seam_cases import S, n_cross_of, small_video
from tests.test_vc_videos_gpu import memory_bits, same_bits, small_setup

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
CODE = 4
NAMES = ["P4_tile_means", "P6_T32_two_passes", "P12_T8_upcast"]


@pytest.mark.parametrize("name", NAMES)
def test_encode_videos_gives_the_bits_of_the_fp32_call(name):
    """encode_videos([k.to(fp8)]) against encode_videos([k.to(fp8).float()]): proj, mean, hidden states and every memory's bits, on
    a new video and continued -- and the launch census of a warm call."""
    dev = H.dev0()
    s, w, m = H.setup(dev, name)
    blocks, hin, u = H.both_ways(m, m, dev, s, F8, (3,), None, f"{name} fp8 encode_videos", seed=21)
    assert blocks[0].element_size() == 1
    launches = {}
    for kind, bl in (("f8", blocks), ("f32", [b.float() for b in blocks])):
        _, launches[kind] = H.call(m, bl, None, hin, u, True, H.memories(m, dev, 1))
    if name == "P12_T8_upcast":                                       # one launch writes the fp32 copy, then the fp32 path as it stands
        assert launches["f8"] == launches["f32"] + 1, launches
    else:
        assert launches["f8"] <= launches["f32"], launches


@pytest.mark.parametrize("name", NAMES)
def test_encode_streams_gives_the_bits_of_the_fp32_call(name):
    """Two streams over block 1 and one over block 0 (frame_src = (1, 0, 1)): the written F_hi plane is read through the map."""
    dev = H.dev0()
    s, w, m = H.setup(dev, name)
    H.both_ways(m, m, dev, s, F8, (3, 4), (1, 0, 1), f"{name} fp8 encode_streams", seed=22)


@pytest.mark.parametrize("name", ["P4_tile_means", "P6_T32_two_passes"])
def test_planes_that_do_not_fit_the_cache_give_the_same_bits(name, monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB so small that no plane fits, on the fp8 encoder's handle only (read at its creation): token passes
    per sub-batch (hi planes alone), frame means from infv_ltm_pool at the token dtype; streams split each contiguous run of source
    chunks -- against fp32 tokens on an encoder with the default budget."""
    dev = H.dev0()
    s, w, m_f32 = H.setup(dev, name)
    m_f32._vc_handle(dev)
    monkeypatch.setenv("INFV_VQF_SPLIT_CACHE_GB", "1e-9")
    _, _, m_f8 = small_setup(dev, **H.OVER[name])
    m_f8._vc_handle(dev)                                              # created under the small budget
    monkeypatch.delenv("INFV_VQF_SPLIT_CACHE_GB")
    H.both_ways(m_f8, m_f32, dev, s, F8, (3,), None, f"{name} fp8 no cache, encode_videos", seed=23)
    H.both_ways(m_f8, m_f32, dev, s, F8, (3, 4), (1, 0, 1), f"{name} fp8 no cache, encode_streams", seed=24)


@pytest.mark.parametrize("name", NAMES)
def test_batch_invariance_of_fp8_videos(name):
    """A probe video alone and at position 2 of three fp8 videos: the same bits."""
    dev = H.dev0()
    s, w, m = H.setup(dev, name)
    blocks = [torch.from_numpy(small_video(s, v, n, 0)[0]).to(F8).to(dev) for v, n in ((3, 2), (4, 1), (0, 3))]
    hin = [H.rows(s, v, t) for v, t in ((3, 9), (4, 0), (0, 5))]
    rng = np.random.default_rng(25)
    us = [rng.random((b.size(0), n_cross_of(s), S)) for b in blocks]
    alone, _ = H.call(m, blocks[2:], None, hin[2:], us[2], True, H.memories(m, dev, 1))
    batch, _ = H.call(m, blocks, None, hin, np.concatenate(us), True, H.memories(m, dev, 3))
    same_bits(batch[2], alone[0], f"{name} fp8: probe at position 2 of 3")


def test_other_fp8_encodings_are_refused():
    dev = H.dev0()
    s, w, m = H.setup(dev, "P4_tile_means")
    k = torch.from_numpy(small_video(s, 0, 2, 0)[0])
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            m.encode_videos([k.to(other).to(dev)], hidden_in=[H.rows(s, 0, 5)], memories=H.memories(m, dev, 1))


def test_raw_abi_code_4():
    """infv_vqf_vc_encode_videos_tok with code 4 on the fp8 tensor's pointer: the bits of code 0 on its fp32 copy, whatever the
    handle's own setting; a pointer 1 or 8 bytes off a 16-byte boundary is refused with nothing launched and the memories as they
    were; the vision LayerNorm of fp8 tokens (infv_vqf_vc_encode_img) is refused as unsupported before any device work."""
    from infinite_video_amd import _lib
    r = H.Raw("P6_T32_two_passes")
    k8 = r.k32.cpu().to(F8).to(r.dev)
    k32 = k8.float()
    ma, mb = r.fresh(), r.fresh()
    rc, _, want = r.run(ma, "infv_vqf_vc_encode_videos_tok", k32.data_ptr(), 0)
    assert rc == 0, r.lib.infv_ltm_last_error()
    rc, _, got = r.run(mb, "infv_vqf_vc_encode_videos_tok", k8.data_ptr(), CODE)
    assert rc == 0, r.lib.infv_ltm_last_error()
    H.same_raw(got, want, mb, ma, "code 4 against code 0 on the fp32 copy")
    before = [memory_bits(mem) for mem in mb]
    store = torch.zeros(k8.numel() + 16, dtype=torch.uint8, device=r.dev)
    assert store.data_ptr() % 16 == 0
    for off in (1, 8):
        store[off:off + k8.numel()] = k8.view(torch.uint8).view(-1)
        rc, n, _ = r.run(mb, "infv_vqf_vc_encode_videos_tok", store.data_ptr() + off, CODE, new_video=0)
        assert rc == H.INVALID and n == 0 and b"16-byte" in r.lib.infv_ltm_last_error(), (off, rc, n)
    for mem, was in zip(mb, before):
        for x, y in zip(memory_bits(mem), was):
            for t, w_ in zip(x, y):
                assert torch.equal(t, w_)
    # the vision LayerNorm on fp8 input: out of scope, refused before any device work
    s, dev = r.s, r.dev
    g = torch.ones(s["enc_width"], device=dev)
    front = _lib.VqfVcFront()
    front.vision_ln = _lib.VqfVisionLn(g.data_ptr(), g.data_ptr(), 1e-12)
    hs = (C.c_void_p * (2 * r.nx))(*[e._h for mem in mb for e in mem.engines])
    cu, tl = (C.c_int32 * 3)(0, 2, 4), (C.c_int32 * 2)(5, 5)
    proj = torch.zeros(4, s["n_query"], s["proj"], device=dev)
    torch.cuda.synchronize()
    n0 = r.lib.infv_ltm_launch_count()
    rc = r.lib.infv_vqf_vc_encode_img(r.h, hs, 2, C.cast(cu, C.c_void_p), C.c_void_p(k8.data_ptr()), CODE, 0, None, None, s["T"],
                                      C.byref(r.wts), C.byref(front), C.c_void_p(r.hin.data_ptr()), C.cast(tl, C.c_void_p),
                                      C.c_void_p(r.u.data_ptr()), 0, None, C.c_void_p(proj.data_ptr()), None, r.stream)
    assert rc == -2 and r.lib.infv_ltm_launch_count() == n0, (rc, r.lib.infv_ltm_last_error())
    # ... and with the LayerNorm part off the same call takes fp8 like the _tok call
    front = _lib.VqfVcFront()
    mc = r.fresh()
    hs = (C.c_void_p * (2 * r.nx))(*[e._h for mem in mc for e in mem.engines])
    mean = torch.zeros(2, s["n_query"], s["proj"], device=dev)
    hid = torch.zeros(4 * (s["n_query"] + 5), s["hidden"], device=dev)
    with torch.cuda.device(dev):
        rc = r.lib.infv_vqf_vc_encode_img(r.h, hs, 2, C.cast(cu, C.c_void_p), C.c_void_p(k8.data_ptr()), CODE, 0, None, None, s["T"],
                                          C.byref(r.wts), C.byref(front), C.c_void_p(r.hin.data_ptr()), C.cast(tl, C.c_void_p),
                                          C.c_void_p(r.u.data_ptr()), 1, C.c_void_p(hid.data_ptr()), C.c_void_p(proj.data_ptr()),
                                          C.c_void_p(mean.data_ptr()), r.stream)
    torch.cuda.synchronize()
    assert rc == 0, r.lib.infv_ltm_last_error()
    H.same_raw((proj.cpu(), mean.cpu(), hid.cpu()), want, mc, ma, "encode_img without the LayerNorm, code 4")
