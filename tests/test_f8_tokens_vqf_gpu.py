"""fp8 e4m3 frame tokens through the video Q-former on the MI355X (infv_vqf_set_token_dtype(h, INFV_TOKENS_F8E4M3 = 4)).

The contract is that of the bf16 tokens (tests/test_vqf_bf16_gpu.py, whose helpers run here on torch.float8_e4m3fn tensors): for
x of that dtype the library gives the bits it gives for x.float().  An e4m3 value is exact in fp32 and exactly its own bf16 hi
piece with a zero lo piece, so the fp8 token pass writes the hi planes alone, both contractions run their two-product form, and
the frame means are summed in the fp32 pass's order.  fp8 is the caller's storage choice: nothing here judges its accuracy."""
import ctypes as C

import pytest
import torch

from tests import test_vqf_bf16_gpu as B
from tests.golden.qformer_cases import qf_inputs

pytestmark = pytest.mark.gpu
DEV = B.DEV
BY_NAME = B.BY_NAME
F8 = torch.float8_e4m3fn
CODE = 4


def to_f8(x):
    """Rounded on the host (the byte tensor travels): what a caller who caches fp8 features holds."""
    return x.cpu().to(F8).to(x.device)


def synth_videos_f8(case, T, lens, seed):
    """tests.test_vqf_bf16_gpu.synth_videos with fp8 where it has .bfloat16(); the first video also carries the smallest
    subnormal, the largest finite value and +-0."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)
    fs = [torch.randn(n, T * case.P, case.hidden, device=DEV, generator=gen) for n in lens]
    if fs and fs[0].numel() > 7 * 4099:
        edge = torch.tensor([2.0 ** -9, -2.0 ** -9, 448.0, 0.0, -0.0, -448.0, 2.0 ** -6], device=DEV)
        fs[0].view(-1)[torch.arange(edge.numel(), device=DEV) * 4099] = edge
    fs = [to_f8(f) for f in fs]
    us = [torch.rand(n, case.n_layers, 512, dtype=torch.float64, generator=cpu) for n in lens]
    return fs, us


@pytest.fixture(autouse=True)
def fp8_tokens(monkeypatch):
    """The helpers of test_vqf_bf16_gpu build their frames with synth_videos: here they get fp8 frames (their "bf16" leg passes
    the tensors as they are, their "f32" leg passes .float())."""
    monkeypatch.setattr(B, "synth_videos", synth_videos_f8)


# qf_small at T 8 (256 tokens: the split path and the whole-video planes), T 5 (160 tokens, a multiple of 32 but not of 64: the
# upcast path) and exact fp32; encode_frames per chunk, encode_frames_batch over 3 chunks, encode_videos with counts [2, 3]
CASES = [
    pytest.param("qf_small", 8, 3, [2, 3], False, id="qf_small_T8_split_path"),
    pytest.param("qf_small", 5, 3, [2, 3], False, id="tokens_multiple_of_32_not_64_upcast"),
    pytest.param("qf_small", 8, 3, [2, 3], True, id="exact_fp32"),
]


@pytest.mark.parametrize("name,T,n_chunks,video_lens,exact", CASES)
def test_fp8_tokens_give_the_bits_of_the_fp32_path(name, T, n_chunks, video_lens, exact):
    """Hidden, llama, means and every memory's B, bin masses, drawn bins and probabilities: torch.equal between x (fp8) and
    x.float() through encode_frames, encode_frames_batch and encode_videos."""
    res = B.run_three_entry_points(BY_NAME[name], T, n_chunks, video_lens, seed=401 + T, exact_fp32=exact)
    assert set(res) == {"f32", "bf16"}                   # (the helper's tag for "the tensors as they are": fp8 here)


def test_fp8_tokens_without_the_whole_video_cache_give_the_same_bits(monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB=0 on the fp8 handle only: per-sub-batch token passes, frame means from the LTM's own pooling of
    the fp8 tokens -- against fp32 tokens on a handle with the default budget."""
    B.run_three_entry_points(BY_NAME["qf_small"], 8, 3, [2, 3], seed=431, env_for_bf16={"INFV_VQF_SPLIT_CACHE_GB": "0"},
                             monkeypatch=monkeypatch)


def test_three_way_fp8_fp32_bf16_and_batch_invariance():
    """encode_videos on counts [2, 3]: the fp8 run == the fp32 run on .float() == the bf16 run on .to(torch.bfloat16) (every e4m3
    value is exact in bf16, and both read-in-place types take the two-product contractions); and the second video alone gives
    the bits it gives in the batch."""
    from infinite_video_amd.video_qformer import VideoMemory
    case = BY_NAME["qf_small"]
    _, weights = qf_inputs(case)
    vf, vu = synth_videos_f8(case, 8, [2, 3], seed=441)
    out = {}
    for tag, cast in (("f8", lambda t: t), ("f32", lambda t: t.float()), ("bf16", lambda t: t.float().bfloat16())):
        m = B.make_model(case, weights)
        mems = [VideoMemory(m, DEV) for _ in vf]
        frames = [cast(f) for f in vf]
        assert all(torch.equal(f.float(), g.float()) for f, g in zip(frames, vf))
        llama, mean, hidden = m.encode_videos(frames, new_video=True, u=torch.cat(vu), want_hidden=True, memories=mems)
        torch.cuda.synchronize()
        out[tag] = ([hidden.cpu(), llama.cpu(), mean.cpu()], [s for mem in mems for s in B.engine_state(mem.engines, case)])
    for tag in ("f32", "bf16"):
        B.assert_same(out["f8"][0], out[tag][0], f"fp8 against {tag}")
        B.assert_same_state(out["f8"][1], out[tag][1], f"fp8 against {tag}: memories")
    m = B.make_model(case, weights)
    mem = [VideoMemory(m, DEV)]
    llama, mean, hidden = m.encode_videos([vf[1]], new_video=True, u=vu[1], want_hidden=True, memories=mem)
    torch.cuda.synchronize()
    B.assert_same([hidden.cpu(), llama.cpu(), mean[0].cpu()], [out["f8"][0][0][2:], out["f8"][0][1][2:], out["f8"][0][2][1]],
                  "video 1 alone against video 1 in the batch")
    B.assert_same_state(B.engine_state(mem[0].engines, case), out["f8"][1][case.n_layers:], "video 1 alone: memories")


def _token_pass_alone(nb, T, P, d):
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    from tests.test_vc_token_pass_gpu import Out
    lib = _lib.load()
    n = T * P
    gen = torch.Generator().manual_seed(451)
    x = (torch.randn(nb, n, d, generator=gen) * 3).to(F8).to(DEV)
    xb = x.float().bfloat16()
    assert torch.equal(xb.float(), x.float())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def run(t, code, names, means=True):
        planes = {k: Out(nb * n * d, torch.bfloat16, DEV) for k in names}
        kbar = Out(nb * T * d, torch.float32, DEV) if means else None
        ptr = lambda k: planes[k].ptr if k in planes else None
        torch.cuda.synchronize()
        n0 = lib.infv_ltm_launch_count()
        with torch.cuda.device(DEV):
            rc = lib.infv_vqf_token_pass(C.c_void_p(t.data_ptr()), code, nb, n, d, P, ptr("Fh"), ptr("Fl"), ptr("Th"), ptr("Tl"),
                                         kbar.ptr if kbar else None, stream)
        torch.cuda.synchronize()
        return rc, lib.infv_ltm_launch_count() - n0, planes, kbar

    rc, launches, planes, kbar = run(x, CODE, ("Fh", "Th"))
    assert rc == 0 and launches == 1, (rc, launches, lib.infv_ltm_last_error())
    Fh, Th = planes["Fh"].check("Fh").view(nb, n, d), planes["Th"].check("Th").view(nb, d, n)
    assert torch.equal(Fh, xb) and torch.equal(Th, xb.transpose(1, 2))
    rc, _, ref, ref_kbar = run(xb, 1, ("Th",))
    assert rc == 0, lib.infv_ltm_last_error()
    assert torch.equal(planes["Th"].mid, ref["Th"].check("bf16 Th"))
    eng = LTMEngine(32, 2, 64, d, P, 0.75, True, device=DEV)
    got = kbar.check("kbar").view(nb, T, d)
    assert torch.equal(got, ref_kbar.check("bf16 kbar").view(nb, T, d))
    assert torch.equal(got, eng.pool(x)) and torch.equal(got, eng.pool(x.float()))
    # a lo plane with code 4 is refused before any launch
    rc, launches, _, _ = run(x, CODE, ("Fh", "Fl", "Th", "Tl"))
    assert rc == -1 and launches == 0


def test_token_pass_alone():
    """infv_vqf_token_pass with code 4 (Fl, Tl NULL): Fh is the tokens as bf16 and Th its transpose -- the plane the bf16 pass
    writes on x.bfloat16() -- nothing is written outside them, and the frame means equal infv_ltm_pool's on the fp8 tokens and on
    x.float()."""
    _token_pass_alone(nb=3, T=24, P=4, d=128)                         # 96 tokens: a second, half-filled 64-token tile


@pytest.mark.parametrize("P,T,d,nb", [(4, 8, 64, 1),                  # n = 32: one tile, partial
                                      (4, 24, 64, 2)],                # n = 96: a whole tile plus a partial one, two chunks
                         ids=lambda v: str(v))
def test_token_pass_alone_partial_tiles(P, T, d, nb):
    """The same checks at the partial-tile shapes of tests/test_vc_token_pass_gpu.py."""
    _token_pass_alone(nb=nb, T=T, P=P, d=d)


def test_refusals_launch_nothing():
    """An fp8 pointer 1, 2, 4 or 8 bytes off a 16-byte boundary and an unknown code: INFV_ERR_INVALID (-1) and no launch; the handle
    keeps fp8 and the aligned pointer then runs, with the bits of the fp32 call."""
    from infinite_video_amd import _lib
    case = BY_NAME["qf_small"]
    T = 8
    m, lib, h, handles, w, keep = B._raw_setup(case, T)
    n = T * case.P * case.hidden
    store = to_f8(torch.randn(2 * n + 64, device=DEV))
    assert store.data_ptr() % 16 == 0
    _lib.check(lib.infv_vqf_set_token_dtype(h, CODE))
    torch.cuda.synchronize()
    before = lib.infv_ltm_launch_count()
    for off in (1, 2, 4, 8):
        ptr = store.data_ptr() + off
        rc, _, _ = B._chunk_call(m, lib, h, handles, ptr, T, w, None, case.n_query, case)
        assert rc == -1 and b"16-byte" in lib.infv_ltm_last_error(), off
        llama = torch.empty(2, case.n_query, case.proj_out, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        assert lib.infv_vqf_encode_video(h, handles, C.c_void_p(ptr), 2, T, C.byref(w), None, 1, None,
                                         C.c_void_p(llama.data_ptr()), None, stream) == -1
    for code in (2, 7, 16, -1):
        assert lib.infv_vqf_set_token_dtype(h, code) == -1 and b"unknown" in lib.infv_ltm_last_error()
    assert lib.infv_ltm_launch_count() == before
    rc, hid8, lla8 = B._chunk_call(m, lib, h, handles, store.data_ptr(), T, w, None, case.n_query, case)   # the handle kept fp8
    assert rc == 0 and lib.infv_ltm_launch_count() > before
    _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    xf = store[:n].float()
    rc, hid32, lla32 = B._chunk_call(m, lib, h, handles, xf.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0
    B.assert_same([hid8, lla8], [hid32, lla32], "after the refusals")
    hidden, llama = B.make_model(case, qf_inputs(case)[1]).encode_frames(store[:n].reshape(1, T * case.P, case.hidden), new_video=True)
    torch.cuda.synchronize()
    B.assert_same([hid8, lla8], [hidden, llama], "C ABI vs encode_frames")
    del keep
