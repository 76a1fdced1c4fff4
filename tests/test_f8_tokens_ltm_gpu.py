"""fp8 e4m3 frame tokens through the LTM on the MI355X (INFV_TOKENS_F8E4M3 = 4, ``torch.float8_e4m3fn``).

fp8 is the caller's storage choice; the library's contract is equality: every finite e4m3 code is an exact fp32 number, the
kernels widen it with the packed hardware conversion and run the fp32 arithmetic behind it in the same order, so every entry
point gives on x (fp8) the bits it gives on x.float().  The reference of every comparison is that same entry point on x.float()."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden.cases import CASES, call_seed, call_uniforms, case_inputs
from tests.test_module_gpu import _module
from tests.test_multi_video_gpu import _batch, _engine, _equal_states, _golden_video, _state, _to

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in CASES}
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def make_engine(dev, N=64, d=768, P=32, L=2, Q=32, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(N, 12, 64, d, P, tau=.75, sticky=True, n_layers=L, max_q=Q, device=dev, **kw)


def f8(x):
    """The values a caller who caches fp8 features holds (rounded on the host: only the byte tensor travels)."""
    return x.cpu().to(F8).to(x.device)


def bits_equal_with_nans(got, ref):
    """NaN positions by isnan (a NaN's payload is not part of the contract), everything else by bits."""
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], ref.view(torch.int32)[~nan])


def test_pool_widens_every_code(dev):
    """All 256 codes tiled into [T * P, d] = [8 * 32, 768] so that one frame's tokens of a column differ (row r, column c holds code
    (r + 37 c) mod 256): the frame means of the fp8 tensor are those of its fp32 copy, NaN where a frame holds 0x7F or 0xFF.  Then
    the 254 finite codes (the NaN codes replaced by +-448) against the means summed in fp64."""
    T, P, d = 8, 32, 768
    eng = make_engine(dev)
    r, c = torch.arange(T * P).unsqueeze(1), torch.arange(d).unsqueeze(0)
    codes = ((r + 37 * c) % 256).to(torch.uint8)
    x = codes.view(F8).to(dev)
    x32 = codes.view(F8).float().to(dev)                       # widened on the host
    assert int(torch.isnan(x32).sum()) == 2 * T * P * d // 256
    got, ref = eng.pool(x), eng.pool(x32)
    assert got.dtype == torch.float32 and got.shape == (T, d)
    assert bits_equal_with_nans(got, ref)
    assert torch.isnan(ref).any() and not torch.isnan(ref).all()

    finite = codes.clone()
    finite[codes == 0x7F] = 0x7E
    finite[codes == 0xFF] = 0xFE
    x, x32 = finite.view(F8).to(dev), finite.view(F8).float().to(dev)
    assert torch.isfinite(x32).all() and float(x32.abs().max()) == 448.0 and len(torch.unique(finite)) == 254
    got, ref = eng.pool(x), eng.pool(x32)
    assert torch.equal(got, ref)
    want = x32.double().reshape(T, P, d).mean(1)
    scale = x32.double().abs().reshape(T, P, d).sum(1) / P
    # (P - 1 fp32 additions and one division: first-order bound P 2^-24 mean|x|; twice that for the higher orders)
    assert ((got.double() - want).abs() <= scale * (P * 2.0 ** -23)).all()


@pytest.mark.parametrize("P,d,T", [(32, 768, 8), (7, 96, 8), (196, 1024, 16), (32, 1056, 8)],
                         ids=["headline_slice", "24_lanes_P_below_burst", "burst_tail_4", "no_pool_rows_shape"])
def test_pool_shapes(dev, P, d, T):
    eng = make_engine(dev, d=d, P=P)
    gen = torch.Generator(device=dev).manual_seed(P * d)
    x = f8(torch.randn(3, T * P, d, device=dev, generator=gen))
    assert x.dtype == F8 and x.element_size() == 1
    assert torch.equal(eng.pool(x), eng.pool(x.float()))
    if d != 1056:
        return
    # widths without a pool + rows kernel: pool_rows runs the frame pool and the rows kernel
    assert torch.equal(eng.pool_rows(x), eng.pool_rows(x.float()))


@pytest.mark.parametrize("N,T,Cn", [(256, 64, 3), (64, 8, 3)], ids=["N256_T64", "N64_T8"])
def test_pool_rows_and_switching_the_dtype_on_one_handle(dev, N, T, Cn):
    P, d = 32, 768
    eng = make_engine(dev, N=N)
    gen = torch.Generator(device=dev).manual_seed(N + T)
    x = f8(torch.randn(Cn, T * P, d, device=dev, generator=gen))
    x32 = x.float()
    a = eng.pool_rows(x).clone()
    b = eng.pool_rows(x32).clone()
    c = eng.pool_rows(x)
    assert torch.equal(a, b) and torch.equal(c, b)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0


def test_misaligned_tokens(dev):
    """A view 1, 2, 4 or 8 bytes off a 16-byte boundary: the C entry point refuses it before any launch ("16-byte"), the engine's
    tensor method copies it to an aligned fp8 tensor and gives the bits of the aligned run."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    T, P, d = 8, 32, 768
    eng = make_engine(dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    flat = f8(torch.randn(T * P * d + 16, device=dev, generator=gen))
    assert flat.data_ptr() % 16 == 0
    ref = eng.pool(flat[:T * P * d].reshape(T * P, d).float())
    out = torch.empty(T, d, device=dev)
    for off in (1, 2, 4, 8):
        v = flat[off:off + T * P * d].reshape(T * P, d)
        assert v.data_ptr() % 16 == off
        _lib.check(lib.infv_ltm_set_token_dtype(eng._h, 4))
        torch.cuda.synchronize()
        n0 = lib.infv_ltm_launch_count()
        assert lib.infv_ltm_pool(eng._h, C.c_void_p(v.data_ptr()), T, C.c_void_p(out.data_ptr()), None) == -1
        assert b"16-byte" in lib.infv_ltm_last_error() and lib.infv_ltm_launch_count() == n0
        assert torch.equal(eng.pool(v), eng.pool(v.float()))
    assert torch.equal(eng.pool(flat[:T * P * d].reshape(T * P, d)), ref)
    for code in (2, 7, 16, -1):                                 # still unknown; the handle keeps fp8
        assert lib.infv_ltm_set_token_dtype(eng._h, code) == -1 and b"unknown" in lib.infv_ltm_last_error()
    assert lib.infv_ltm_pool(eng._h, C.c_void_p(flat.data_ptr()), T, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def _consolidate_inputs(dev, Cn, seed):
    from infinite_video_amd import synth
    d, H, dh, Q, L = 768, 12, 64, 32, 2
    projs = [tuple(_to(dev, *synth.layer_projections(l, d, H * dh, seed=seed + 1))) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, H * dh, seed=seed + 2) for l in range(L)])).to(dev)
    u = torch.from_numpy(synth.gibbs_uniforms(Cn, L, seed=seed + 3)).to(dev)
    return projs, q, u


def _engine_state(eng, L=2):
    out = []
    for l in range(L):
        B, mass = eng.export_state(l)
        bins, _, probs = eng.last_draw(l)
        out.append((B.cpu(), mass.cpu(), bins.copy(), probs.copy()))
    return out


def _assert_states_equal(a, b):
    for (Ba, ma, ba, pa), (Bb, mb, bb, pb) in zip(a, b):
        assert torch.equal(Ba, Bb) and torch.equal(ma, mb)
        np.testing.assert_array_equal(ba, bb)
        np.testing.assert_array_equal(pa, pb)


@pytest.mark.parametrize("Cn,kw,pool_launches", [(7, dict(max_batch_chunks=3), 3), (800, {}, 2)],
                         ids=["7_chunks_sub_batches_of_3", "800_chunks_one_pooling_launch"])
def test_consolidate(dev, Cn, kw, pool_launches):
    """N 64, T 8, P 32, d 768, 2 layers, Q 32, sticky.  The first chunk of a document runs on its own (one pooling launch); behind
    it, 7 chunks in sub-batches of 3: one pooling launch per sub-batch (1 + 2); 800 chunks (157 MB of fp8 tokens): the ONE pooling
    launch of the call, which also writes the rows' bf16 planes and counts its workgroups in (1 + 1).  ctx of every chunk, B, bin
    masses, last draw and probabilities equal the run's on x.float()."""
    T, P, d = 8, 32, 768
    gen = torch.Generator(device=dev).manual_seed(Cn)
    x = torch.randn(Cn, T * P, d, device=dev, generator=gen).to(F8)           # (rounded on the device: 157 M values)
    projs, q, u = _consolidate_inputs(dev, Cn, seed=2000 + Cn)
    res = {}
    for tag in ("f32", "f8"):
        eng = make_engine(dev, **kw)
        k = x if tag == "f8" else x.float()
        eng.profile(True)
        ctx = eng.consolidate(k, q, projs, u, new_doc=True)
        torch.cuda.synchronize()
        n_pool = eng.profile_read()["pool"][0]
        eng.profile(False)
        res[tag] = (ctx.cpu(), _engine_state(eng), n_pool)
        del k
    assert torch.isfinite(res["f8"][0]).all()
    assert torch.equal(res["f8"][0], res["f32"][0])
    _assert_states_equal(res["f8"][1], res["f32"][1])
    assert res["f8"][2] == res["f32"][2]                            # the same schedule
    assert res["f8"][2] == pool_launches, res["f8"][2]


def test_forward_engine_and_module_without_an_fp32_copy(dev):
    """Three chunks of forward() on fp8 k through LTMEngine and through the drop-in module (VideoChat2 shape: T 16, P 196,
    d 1024): the bits of k.float(); the module's warm call raises torch's peak allocation by less than an fp32 copy of k."""
    case = BY_NAME["vc_shape"]
    assert (case.chunk_T[0], case.P, case.d) == (16, 196, 1024)
    ks, qs, ws = case_inputs(case)
    ks = [torch.from_numpy(k).to(F8).to(dev) for k in ks[:3]]
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    u = torch.from_numpy(np.stack([np.stack([call_uniforms(case, c, l) for l in range(case.n_layers)]) for c in range(3)])).to(dev)
    e8, e32 = _engine(case, dev), _engine(case, dev)
    for c, k in enumerate(ks):
        a = e8.forward(k, q, projs, u[c], new_doc=(c == 0))
        b = e32.forward(k.float(), q, projs, u[c], new_doc=(c == 0))
        assert torch.isfinite(a).all() and torch.equal(a, b), c
    _assert_states_equal(_engine_state(e8, case.n_layers), _engine_state(e32, case.n_layers))

    m8, m32 = _module(case, ws, 0, dev), _module(case, ws, 0, dev)
    q0 = q[0].unsqueeze(0)
    with torch.no_grad():
        for c, k in enumerate(ks):
            torch.manual_seed(call_seed(case, c, 0))
            a = m8(k.unsqueeze(0), q0, new_doc=(c == 0), layer_n=0)
            torch.manual_seed(call_seed(case, c, 0))
            b = m32(k.float().unsqueeze(0), q0, new_doc=(c == 0), layer_n=0)
            assert a.dtype == torch.float32 and torch.equal(a, b), c
            np.testing.assert_array_equal(m8._engine.last_draw(0)[0], m32._engine.last_draw(0)[0])
        k = ks[2].clone().unsqueeze(0)
        torch.manual_seed(5)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = m8(k, q0, new_doc=False, layer_n=0)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"LongTermAttention.forward on fp8 k: peak rise {rise} B, an fp32 copy of k: {k.numel() * 4} B")
    assert torch.isfinite(out).all()
    assert rise < k.numel() * 4


def test_consolidate_videos_and_the_mixed_batch_refusal(dev):
    """Chunk counts [3, 5] at cfg1_sticky: equal to the fp32 run; a batch with one fp8 and one fp32 handle is refused (the token
    dtype is part of "identical configuration"), nothing is launched and every memory stays as it was."""
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import consolidate_videos
    case = BY_NAME["cfg1_sticky"]
    ks, us = _batch(case, [3, 5], first_video=80)
    ks = [torch.from_numpy(k).to(F8) for k in ks]
    _, _, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    u = torch.from_numpy(np.concatenate(us)).to(dev)
    k8 = torch.cat(ks).to(dev)
    e32 = [_engine(case, dev) for _ in ks]
    c32 = consolidate_videos(e32, k8.float(), [3, 5], q, projs, u)
    e8 = [_engine(case, dev) for _ in ks]
    c8 = consolidate_videos(e8, k8, [3, 5], q, projs, u)
    torch.cuda.synchronize()
    assert torch.isfinite(c8).all() and torch.equal(c8, c32)
    for a, b in zip(e8, e32):
        _equal_states(_state(a, case), _state(b, case))
    # mixed batch through the C ABI (the Python wrapper sets every handle's dtype from k): handle 0 fp8, handle 1 fp32
    lib = _lib.load()
    before = [_state(e, case) for e in e8]
    _lib.check(lib.infv_ltm_set_token_dtype(e8[0]._h, 4))
    _lib.check(lib.infv_ltm_set_token_dtype(e8[1]._h, 0))
    hs = (C.c_void_p * 2)(e8[0]._h.value, e8[1]._h.value)
    cu = (C.c_int32 * 3)(0, 1, 2)
    k1 = torch.cat([ks[0][:1], ks[1][:1]]).to(dev)
    u1 = torch.from_numpy(np.concatenate([us[0][:1], us[1][:1]])).to(dev)
    ctx = torch.zeros(2, case.n_layers, case.Q, case.H * case.dh, device=dev)
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         case.Q, e8[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0,
                                         C.c_void_p(ctx.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == -1, lib.infv_ltm_last_error()
    assert lib.infv_ltm_launch_count() == n0
    for e, b in zip(e8, before):
        _equal_states(_state(e, case), b)
    # both fp8 again: the same call runs
    _lib.check(lib.infv_ltm_set_token_dtype(e8[1]._h, 4))
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         case.Q, e8[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0,
                                         C.c_void_p(ctx.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.infv_ltm_last_error()


def test_token_dtype_benchmark_child_runs_the_fp8_leg(dev, capsys):
    """tools/bench_token_dtypes.py: what one child process of the tool does for the fp8 leg, in this process at 3 chunks and one timed
    call: its JSON line, one byte per token element."""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_token_dtypes.py")
    spec = importlib.util.spec_from_file_location("bench_token_dtypes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "float8_e4m3fn" in mod.LEGS
    mod.child("float8_e4m3fn", 3, 1)
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert line["leg"] == "float8_e4m3fn" and line["chunks"] == 3 and line["pool_rows_alone_chunks"] == 3
    assert line["token_bytes"] == 3 * mod.T * mod.P * mod.D
    assert line["median_ms"] > 0 and line["pool_rows_alone_ms"] > 0 and np.isfinite(line["checksum"])
