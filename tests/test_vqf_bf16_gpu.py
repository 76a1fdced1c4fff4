"""bf16 frame tokens through the video Q-former on the MI355X (infv_vqf_set_token_dtype).

The contract is equality, not a tolerance: for x = randn(...).bfloat16() the library gives the bits it gives for x.float().
A bf16 token is its own hi plane and its lo plane is exactly zero; a bf16 MFMA product with an all-zero operand adds exact
zeros to the fp32 accumulator, so dropping that product (and that plane) changes no value, and nothing else in the schedule
may look at the dtype (torch.equal treats -0 as 0).  Also: the C ABI takes the bf16 pointer itself, Python makes no fp32
copy, batch invariance holds, the two-product contractions alone equal the three-product ones, and refusals launch nothing."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden.qformer_cases import QF_CASES, qf_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c.name: c for c in QF_CASES}
DEV = torch.device("cuda:0")


def make_model(case, weights, exact_fp32=False):
    from infinite_video_amd.video_qformer import InfVideoEncoder
    m = InfVideoEncoder(num_video_query_token=case.n_query, hidden_size=case.hidden, llama_hidden=case.proj_out,
                        sticky=case.sticky, num_basis=case.N, tau=case.tau, alpha=case.alpha,
                        num_hidden_layers=case.n_layers)
    m.load_reference_state_dict(weights)
    m.exact_fp32 = exact_fp32
    return m.to(DEV)


def synth_videos(case, T, lens, seed):
    """Per video: bf16 frames [C_v, T*P, hidden] on the device (finite by construction) and uniforms [C_v, L, 512] (host)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)
    fs = [torch.randn(n, T * case.P, case.hidden, device=DEV, generator=gen).bfloat16() for n in lens]
    us = [torch.rand(n, case.n_layers, 512, dtype=torch.float64, generator=cpu) for n in lens]
    return fs, us


def engine_state(engines, case):
    out = []
    if case.alpha == 1.0:
        return out
    for eng in engines:
        B, mass = eng.export_state(0)
        bins, _, probs = eng.last_draw(0)
        out.append((B.cpu(), mass.cpu(), bins.copy(), probs.copy()))
    return out


def own_state(m, case):
    return engine_state([mod._engine for mod in m.video_Qformer.ltm_modules], case)


def assert_same_state(a, b, tag):
    assert len(a) == len(b), tag
    for (Ba, ma, ba, pa), (Bb, mb, bb, pb) in zip(a, b):
        assert torch.equal(Ba, Bb), tag
        assert torch.equal(ma, mb), tag
        np.testing.assert_array_equal(ba, bb, err_msg=tag)
        np.testing.assert_array_equal(pa, pb, err_msg=tag)


def assert_same(a, b, tag):
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == torch.float32 and x.shape == y.shape, f"{tag} [{i}]"
        assert torch.isfinite(x).all(), f"{tag} [{i}]"
        assert torch.equal(x, y), f"{tag} [{i}]: {int((x != y).sum())} of {x.numel()} elements differ, max |diff| {float((x - y).abs().max()):.3e}"


def run_three_entry_points(case, T, n_chunks, video_lens, seed, exact_fp32=False, env_for_bf16=None, monkeypatch=None):
    """encode_frames chunk by chunk, encode_frames_batch and encode_videos on bf16 frames and on their fp32 copies: outputs and
    memories.  `env_for_bf16`: environment for the bf16 model's handle only (read when the handle is created)."""
    from infinite_video_amd.video_qformer import VideoMemory
    _, weights = qf_inputs(case)
    (x,), (u,) = synth_videos(case, T, [n_chunks], seed)
    vf, vu = synth_videos(case, T, video_lens, seed + 1)
    res = {}
    for tag in ("f32", "bf16"):
        if monkeypatch is not None and env_for_bf16:
            for k, v in env_for_bf16.items():
                if tag == "bf16":
                    monkeypatch.setenv(k, v)
                else:
                    monkeypatch.delenv(k, raising=False)
        cast = (lambda t: t) if tag == "bf16" else (lambda t: t.float())
        out = {}
        m = make_model(case, weights, exact_fp32)
        per = [m.encode_frames(cast(x[c:c + 1]), new_video=(c == 0), u=u[c]) for c in range(n_chunks)]
        torch.cuda.synchronize()
        out["encode_frames"] = [t.cpu() for pair in per for t in pair]
        out["encode_frames state"] = own_state(m, case)
        m = make_model(case, weights, exact_fp32)
        llama, mean, hidden = m.encode_frames_batch(cast(x), new_video=True, u=u, want_hidden=True)
        torch.cuda.synchronize()
        out["encode_frames_batch"] = [hidden.cpu(), llama.cpu(), mean.cpu()]
        out["encode_frames_batch state"] = own_state(m, case)
        m = make_model(case, weights, exact_fp32)
        mems = [VideoMemory(m, DEV) for _ in vf] if case.alpha != 1.0 else []
        llama, mean, hidden = m.encode_videos([cast(f) for f in vf], new_video=True, u=torch.cat(vu), want_hidden=True,
                                              memories=mems or None)
        torch.cuda.synchronize()
        out["encode_videos"] = [hidden.cpu(), llama.cpu(), mean.cpu()]
        out["encode_videos state"] = [s for mem in mems for s in engine_state(mem.engines, case)]
        res[tag] = out
    for key in ("encode_frames", "encode_frames_batch", "encode_videos"):
        assert_same(res["bf16"][key], res["f32"][key], f"{case.name} {key}")
        assert_same_state(res["bf16"][key + " state"], res["f32"][key + " state"], f"{case.name} {key} memories")
    return res


# (name of the QF case, T, chunks of the single video, chunk counts of the batch, exact fp32)
CONTRACT_CASES = [
    pytest.param("qf_small", 8, 4, [3, 1, 4], False, id="qf_small_sticky_alpha0.9"),
    pytest.param("qf_headline", 256, 6, [1, 3, 2], False, id="headline_T256_N256_wide_kernel_and_cache"),
    pytest.param("qf_small", 5, 3, [2, 3], False, id="tokens_multiple_of_32_not_64_fp32_kernels"),
    pytest.param("qf_small", 8, 3, [2, 3], True, id="exact_fp32"),
    pytest.param("qf_alpha1", 8, 3, [2, 1, 3], False, id="alpha1_no_memory"),
]


@pytest.mark.parametrize("name,T,n_chunks,video_lens,exact", CONTRACT_CASES)
def test_bf16_tokens_give_the_bits_of_the_fp32_path(name, T, n_chunks, video_lens, exact):
    """Hidden, llama, means and every memory's B, bin masses, drawn bins and probabilities: torch.equal between x (bf16) and
    x.float() through encode_frames, encode_frames_batch and encode_videos."""
    run_three_entry_points(BY_NAME[name], T, n_chunks, video_lens, seed=101 + T, exact_fp32=exact)


def test_bf16_tokens_without_the_whole_video_cache_give_the_same_bits(monkeypatch):
    """The one decision that sees the dtype -- whether the whole video's operands fit the split cache -- changes no bits: bf16
    tokens on a handle whose budget is too small for the cache (per-sub-batch token passes, frame means from the LTM's own
    pooling of the bf16 tokens) against fp32 tokens on a handle with the default budget."""
    run_three_entry_points(BY_NAME["qf_small"], 8, 4, [3, 1, 4], seed=131, env_for_bf16={"INFV_VQF_SPLIT_CACHE_GB": "0"},
                           monkeypatch=monkeypatch)


def test_ragged_encode_long_videos_with_tails():
    """Videos of 20, 16, 5 and 10 frames at max_int 8: the full chunks of all videos in one encode_videos call (one bf16
    torch.cat), the tails of 4, 5 and 2 frames (128, 160, 64 tokens: split and fp32 kernels) per chunk on each video's
    memory.  bf16 videos against their fp32 copies, same generator state: same bits."""
    from infinite_video_amd.video_qformer import encode_long_videos
    case = BY_NAME["qf_small"]
    _, weights = qf_inputs(case)
    gen = torch.Generator(device=DEV).manual_seed(41)
    videos = [torch.randn(F, case.P, case.hidden, device=DEV, generator=gen).bfloat16() for F in (20, 16, 5, 10)]
    got = {}
    for tag in ("f32", "bf16"):
        m = make_model(case, weights)
        torch.manual_seed(1234)
        out = encode_long_videos(m, [v if tag == "bf16" else v.float() for v in videos], 8)
        torch.cuda.synchronize()
        got[tag] = ([t.cpu() for mean, embs in out for t in [mean] + list(embs)],
                    [s for mem in m._video_memories[:len(videos)] for s in engine_state(mem.engines, case)])
    assert_same(got["bf16"][0], got["f32"][0], "encode_long_videos")
    assert_same_state(got["bf16"][1], got["f32"][1], "encode_long_videos memories")


def _chunk_call(m, lib, h, handles, ptr, T, w, u, Q, case):
    hidden = torch.empty(1, Q, case.hidden, device=DEV)
    llama = torch.empty(1, Q, case.proj_out, device=DEV)
    rc = lib.infv_vqf_encode_chunk(h, handles, C.c_void_p(ptr), T, C.byref(w), C.c_void_p(u.data_ptr() if u is not None else 0),
                                   1, C.c_void_p(hidden.data_ptr()), C.c_void_p(llama.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, hidden, llama


def _raw_setup(case, T):
    """A model, its handle, its memories' handles with a plan for T, and its weights struct."""
    from infinite_video_amd import _lib
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    lib = _lib.load()
    h = m._handle(DEV)
    handles = (C.c_void_p * case.n_layers)()
    for l, mod in enumerate(m.video_Qformer.ltm_modules):
        mod.length = mod.target_len = T * case.P
        eng = mod._get_engine(DEV, case.n_query)
        eng.ensure_plan(T)
        handles[l] = eng._h
    w, keep = m._weights(DEV)
    return m, lib, h, handles, w, keep


def test_c_abi_takes_the_bf16_pointer_itself():
    """infv_vqf_set_token_dtype(h, 1) + infv_vqf_encode_chunk on the bf16 tensor's data_ptr(): the bits of the fp32 call on
    the same values, and of InfVideoEncoder.encode_frames."""
    from infinite_video_amd import _lib
    case = BY_NAME["qf_small"]
    T = 8
    (x,), _ = synth_videos(case, T, [1], seed=151)
    m, lib, h, handles, w, keep = _raw_setup(case, T)
    xf = x.float()
    _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    rc, hid32, lla32 = _chunk_call(m, lib, h, handles, xf.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0, lib.infv_ltm_last_error()
    _lib.check(lib.infv_vqf_set_token_dtype(h, 1))
    rc, hid16, lla16 = _chunk_call(m, lib, h, handles, x.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0, lib.infv_ltm_last_error()
    assert_same([hid16, lla16], [hid32, lla32], "encode_chunk through the C ABI")
    _, weights = qf_inputs(case)
    hidden, llama = make_model(case, weights).encode_frames(x, new_video=True)
    torch.cuda.synchronize()
    assert_same([hid16, lla16], [hidden, llama], "C ABI vs encode_frames")
    del keep


def test_refusals_launch_nothing():
    """A bf16 pointer that is not 16-byte aligned and an unknown dtype: INFV_ERR_INVALID (-1), no launch, dtype unchanged."""
    from infinite_video_amd import _lib
    case = BY_NAME["qf_small"]
    T = 8
    m, lib, h, handles, w, keep = _raw_setup(case, T)
    n = T * case.P * case.hidden
    store = torch.randn(2 * n + 64, device=DEV).bfloat16()
    assert store.data_ptr() % 16 == 0
    _lib.check(lib.infv_vqf_set_token_dtype(h, 1))
    torch.cuda.synchronize()
    before = lib.infv_ltm_launch_count()
    for off in (1, 2, 4, 7):                                   # elements: 2, 4, 8, 14 bytes off a 16-byte boundary
        ptr = store.data_ptr() + 2 * off
        rc, _, _ = _chunk_call(m, lib, h, handles, ptr, T, w, None, case.n_query, case)
        assert rc == -1 and b"16-byte" in lib.infv_ltm_last_error(), off
        llama = torch.empty(2, case.n_query, case.proj_out, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        assert lib.infv_vqf_encode_video(h, handles, C.c_void_p(ptr), 2, T, C.byref(w), None, 1, None,
                                         C.c_void_p(llama.data_ptr()), None, stream) == -1
    for bad in (2, -1, 16):
        assert lib.infv_vqf_set_token_dtype(h, bad) == -1
    assert lib.infv_ltm_launch_count() == before
    # the handle kept bf16: the aligned pointer runs, and gives what the fp32 copy gives
    rc, hid16, lla16 = _chunk_call(m, lib, h, handles, store.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0 and lib.infv_ltm_launch_count() > before
    _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    xf = store[:n].float()
    rc, hid32, lla32 = _chunk_call(m, lib, h, handles, xf.data_ptr(), T, w, None, case.n_query, case)
    assert rc == 0
    assert_same([hid16, lla16], [hid32, lla32], "after the refusals")
    del keep


def test_no_hidden_upcast_and_no_extra_launches_at_the_headline_shape():
    """Warm encode_frames_batch / encode_videos on PACKED bf16 frames: torch's peak allocation rises by less than an fp32 copy
    of the frames would take (the library's workspaces are not torch's), and the call issues no more launches than on
    x.float()."""
    from infinite_video_amd import _lib
    from infinite_video_amd.video_qformer import VideoMemory
    case = BY_NAME["qf_headline"]
    T, counts = 256, [3, 1, 4]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    lib = _lib.load()
    (x,), (u,) = synth_videos(case, T, [sum(counts)], seed=171)
    x32 = x.float()
    fp32_copy = x.numel() * 4
    mems = [VideoMemory(m, DEV) for _ in counts]

    def batch(frames):
        return m.encode_frames_batch(frames, new_video=True, u=u)

    def videos(frames):
        return m.encode_videos(frames, counts, new_video=True, u=u, memories=mems)

    for name, call in (("encode_frames_batch", batch), ("encode_videos", videos)):
        launches = {}
        for tag, frames in (("f32", x32), ("bf16", x)):
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
            if tag == "bf16":
                assert rise < fp32_copy, (name, rise, fp32_copy)
        assert launches["bf16"] <= launches["f32"], (name, launches)


def test_batch_invariance_with_bf16_tokens():
    """One video alone, first, last and between videos of other lengths, all bf16: hidden, llama, mean and its memories' B,
    bin masses and draws are the same bits."""
    from infinite_video_amd.video_qformer import VideoMemory
    case = BY_NAME["qf_small"]
    T = case.chunk_T[0]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    (f0,), (u0,) = synth_videos(case, T, [5], seed=21)
    others_f, others_u = synth_videos(case, T, [3, 1, 7, 2], seed=22)
    assert f0.dtype == torch.bfloat16
    runs = {"alone": ([f0], [u0], 0), "first": ([f0] + others_f, [u0] + others_u, 0),
            "last": (others_f + [f0], others_u + [u0], 4),
            "between": (others_f[:2] + [f0] + others_f[2:], others_u[:2] + [u0] + others_u[2:], 2)}
    res = {}
    for tag, (fs, us, pos) in runs.items():
        mems = [VideoMemory(m, DEV) for _ in fs]
        llama, mean, hidden = m.encode_videos(fs, new_video=True, u=torch.cat(us), want_hidden=True, memories=mems)
        torch.cuda.synchronize()
        cu = np.concatenate([[0], np.cumsum([len(f) for f in fs])])
        out = [hidden[cu[pos]:cu[pos + 1]].cpu(), llama[cu[pos]:cu[pos + 1]].cpu(), mean[pos].cpu()]
        res[tag] = (out, engine_state(mems[pos].engines, case))
    for tag in ("first", "last", "between"):
        assert_same(res[tag][0], res["alone"][0], tag)
        assert_same_state(res[tag][1], res["alone"][1], tag)


_GEMM_CHILD = r'''
import ctypes as C, sys, json
import torch
from infinite_video_amd import _lib
lib = _lib.load()
fn = lib.infv_exp_gemm
fn.restype = C.c_int
fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
dev = torch.device("cuda:0")
out = {}
# the two headline contractions (scores: K = d, read-out: K = T*P) and one shape with a partial 128-tile (128 x 128 kernel only:
# the 384 x 256 kernel takes whole tiles)
for name, M, N, K, pairs in [("scores", 384, 8192, 768, [(5, 3), (6, 4)]), ("readout", 384, 768, 8192, [(5, 3), (6, 4)]),
                             ("partial_tile", 200, 328, 192, [(6, 4)])]:
    g = torch.Generator(device=dev).manual_seed(N)
    A = torch.randn(M, K, device=dev, generator=g)
    B = torch.randn(N, K, device=dev, generator=g).bfloat16().float()       # B already rounded to bf16
    ref = A.double() @ B.double().T
    mag = A.double().abs() @ B.double().abs().T
    res = {}
    for two, three in pairs:
        keep = {}
        for which in (two, three):
            Cc = torch.full((M, N), float("nan"), device=dev)
            rc = fn(which, A.data_ptr(), B.data_ptr(), Cc.data_ptr(), M, N, K)
            assert rc == 0, (name, which, rc)
            keep[which] = Cc
        res[f"{two}=={three}"] = bool(torch.equal(keep[two], keep[three]))
        res[f"err{two}"] = float(((keep[two].double() - ref).abs() / mag).max())
    out[name] = res
json.dump(out, open(sys.argv[1], "w"))
'''


def test_two_product_contraction_equals_the_three_product_one(tmp_path):
    """The GEMM alone (experiments build, infv_exp_gemm): for B already rounded to bf16 the two-product contraction equals
    the three-product one bit for bit -- 384 x 256 tiles (which = 5 vs 3) and 128 x 128 tiles (6 vs 4) at the two headline
    contractions, 128 x 128 tiles at a shape with partial tiles -- and is within the split's 2^-16 relative error of fp64."""
    path = str(tmp_path / "gemm2.json")
    env = dict(os.environ, INFV_LTM_LIBRARY="exp")
    subprocess.run([sys.executable, "-c", _GEMM_CHILD, path], check=True, env=env, cwd=ROOT)
    res = json.load(open(path))
    assert set(res) == {"scores", "readout", "partial_tile"}
    for name, e in res.items():
        for k, v in e.items():
            if "==" in k:
                assert v, (name, k, e)
            else:
                assert v < 4e-5, (name, k, e)
