"""fp16 frame tokens through the LTM on the MI355X (INFV_TOKENS_F16 = 3).

The contract is equality: an fp16 value is exact in fp32, the kernels widen it with the hardware conversion and run the fp32
arithmetic behind it in the same order, so every entry point gives on x (fp16) the bits it gives on x.float()."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden.cases import CASES, call_seed, call_uniforms, case_inputs
from tests.test_module_gpu import _module
from tests.test_multi_video_gpu import _batch, _engine, _equal_states, _golden_video, _state, _to

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def make_engine(dev, N=64, d=768, P=32, L=2, Q=32, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(N, 12, 64, d, P, tau=.75, sticky=True, n_layers=L, max_q=Q, device=dev, fp16_tokens=True, **kw)


def all_finite_halves(dev):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16)
    return x[torch.isfinite(x)].to(dev)


def test_pool_covers_every_finite_fp16_value(dev):
    """All 63 488 finite bit patterns (subnormals, +-0, 65504) tiled into [T*P, d], then randn at 2^-16 (mostly subnormal in fp16)
    and at 1000: the frame means of the fp16 tensor are those of its fp32 copy."""
    T, P, d = 8, 32, 768
    eng = make_engine(dev)
    vals = all_finite_halves(dev)
    assert vals.numel() == 63488
    n = T * P * d
    # a permutation-free tiling: column-major so that one frame's P tokens of a column differ in magnitude and sign
    tiled = vals.repeat((n + vals.numel() - 1) // vals.numel())[:n].reshape(d, T * P).t().contiguous()
    gen = torch.Generator(device=dev).manual_seed(7)
    for tag, x in (("all patterns", tiled),
                   ("subnormal scale", (torch.randn(T * P, d, device=dev, generator=gen) * 2.0 ** -16).half()),
                   ("1000 scale", (torch.randn(T * P, d, device=dev, generator=gen) * 1000).half())):
        assert x.dtype == torch.float16 and torch.isfinite(x).all()
        got, ref = eng.pool(x), eng.pool(x.float())
        assert got.dtype == torch.float32 and torch.equal(got, ref), tag
        # and the widening itself: against the means summed in fp64, within the rounding of an fp32 sum of P terms
        want = x.double().reshape(T, P, d).mean(1)
        scale = x.double().abs().reshape(T, P, d).sum(1) / P
        # (P - 1 fp32 additions and one division: first-order bound 2^-24 sum|x| / ... = P 2^-24 mean|x|; twice that for the higher orders)
        assert ((got.double() - want).abs() <= scale * (P * 2.0 ** -23)).all(), tag


@pytest.mark.parametrize("P,d,T", [(32, 768, 8), (7, 96, 8), (196, 1024, 16), (32, 1056, 8)],
                         ids=["headline_slice", "24_lanes_P_below_burst", "burst_tail_4", "no_pool_rows_shape"])
def test_pool_shapes(dev, P, d, T):
    eng = make_engine(dev, d=d, P=P)
    gen = torch.Generator(device=dev).manual_seed(P * d)
    x = torch.randn(3, T * P, d, device=dev, generator=gen).half()
    assert torch.equal(eng.pool(x), eng.pool(x.float()))
    if d != 1056:
        return
    # widths without a pool + rows kernel: pool_rows and consolidate run the frame pool and the rows kernel
    assert torch.equal(eng.pool_rows(x), eng.pool_rows(x.float()))


@pytest.mark.parametrize("N,T,Cn", [(256, 64, 3), (64, 8, 3)], ids=["N256_T64", "N64_T8"])
def test_pool_rows_and_switching_the_dtype_on_one_handle(dev, N, T, Cn):
    P, d = 32, 768
    eng = make_engine(dev, N=N)
    gen = torch.Generator(device=dev).manual_seed(N + T)
    x = torch.randn(Cn, T * P, d, device=dev, generator=gen).half()
    x32 = x.float()
    a = eng.pool_rows(x).clone()
    b = eng.pool_rows(x32).clone()
    c = eng.pool_rows(x)
    assert torch.equal(a, b) and torch.equal(c, b)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0


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
    it, 7 chunks in sub-batches of 3: one pooling launch per sub-batch (1 + 2); 800 chunks: the ONE pooling launch of the call,
    which also writes the rows' bf16 planes and counts its workgroups in (1 + 1).  ctx of every chunk, B, bin masses, last draw and
    probabilities equal the fp32-token run's."""
    T, P, d = 8, 32, 768
    gen = torch.Generator(device=dev).manual_seed(Cn)
    x = torch.randn(Cn, T * P, d, device=dev, generator=gen).half()
    projs, q, u = _consolidate_inputs(dev, Cn, seed=2000 + Cn)
    res = {}
    for tag in ("f32", "f16"):
        eng = make_engine(dev, **kw)
        k = x if tag == "f16" else x.float()
        eng.profile(True)
        ctx = eng.consolidate(k, q, projs, u, new_doc=True)
        torch.cuda.synchronize()
        n_pool = eng.profile_read()["pool"][0]
        eng.profile(False)
        res[tag] = (ctx.cpu(), _engine_state(eng), n_pool)
        del k
    assert torch.isfinite(res["f16"][0]).all()
    assert torch.equal(res["f16"][0], res["f32"][0])
    _assert_states_equal(res["f16"][1], res["f32"][1])
    assert res["f16"][2] == res["f32"][2]                           # the same schedule
    assert res["f16"][2] == pool_launches, res["f16"][2]


def test_forward_engine_and_module_without_an_fp32_copy(dev):
    """Three chunks of forward() on fp16 k through LTMEngine and through the drop-in module (VideoChat2 shape: T 16, P 196,
    d 1024): the bits of k.float(); the module's warm call raises torch's peak allocation by less than an fp32 copy of k."""
    case = BY_NAME["vc_shape"]
    assert (case.chunk_T[0], case.P, case.d) == (16, 196, 1024)
    ks, qs, ws = case_inputs(case)
    ks = [torch.from_numpy(k).half().to(dev) for k in ks[:3]]                  # the values an fp16 producer holds
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    u = torch.from_numpy(np.stack([np.stack([call_uniforms(case, c, l) for l in range(case.n_layers)]) for c in range(3)])).to(dev)
    e16, e32 = _engine(case, dev, fp16_tokens=True), _engine(case, dev)
    for c, k in enumerate(ks):
        a = e16.forward(k, q, projs, u[c], new_doc=(c == 0))
        b = e32.forward(k.float(), q, projs, u[c], new_doc=(c == 0))
        assert torch.isfinite(a).all() and torch.equal(a, b), c
    _assert_states_equal(_engine_state(e16, case.n_layers), _engine_state(e32, case.n_layers))

    m16, m32 = _module(case, ws, 0, dev), _module(case, ws, 0, dev)
    q0 = q[0].unsqueeze(0)
    with torch.no_grad():
        for c, k in enumerate(ks):
            torch.manual_seed(call_seed(case, c, 0))
            a = m16(k.unsqueeze(0), q0, new_doc=(c == 0), layer_n=0)
            torch.manual_seed(call_seed(case, c, 0))
            b = m32(k.float().unsqueeze(0), q0, new_doc=(c == 0), layer_n=0)
            assert a.dtype == torch.float32 and torch.equal(a, b), c
            np.testing.assert_array_equal(m16._engine.last_draw(0)[0], m32._engine.last_draw(0)[0])
        # warm call on the fp16 module: no fp32 copy of k through torch's allocator
        k = ks[2].clone().unsqueeze(0)
        torch.manual_seed(5)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = m16(k, q0, new_doc=False, layer_n=0)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"LongTermAttention.forward on fp16 k: peak rise {rise} B, an fp32 copy of k: {k.numel() * 4} B")
    assert torch.isfinite(out).all()
    assert rise < k.numel() * 4


def test_consolidate_videos_and_the_mixed_batch_refusal(dev):
    """Chunk counts [3, 5] at cfg1_sticky: equal to the fp32 run; a batch with one fp16 and one fp32 handle is refused (the token
    dtype is part of "identical configuration") and every memory stays as it was."""
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import consolidate_videos
    case = BY_NAME["cfg1_sticky"]
    ks, us = _batch(case, [3, 5], first_video=80)
    ks = [torch.from_numpy(k).half() for k in ks]                              # the values an fp16 producer holds
    _, _, qs, ws = _golden_video(case)
    projs = [tuple(_to(dev, *w)) for w in ws]
    q = torch.from_numpy(np.stack(qs)).to(dev)
    u = torch.from_numpy(np.concatenate(us)).to(dev)
    k16 = torch.cat(ks).to(dev)
    e32 = [_engine(case, dev) for _ in ks]
    c32 = consolidate_videos(e32, k16.float(), [3, 5], q, projs, u)
    with pytest.raises(TypeError):                                            # fp16 is opt-in on an engine's tensor methods
        consolidate_videos(e32, k16, [3, 5], q, projs, u, new_doc=False)
    e16 = [_engine(case, dev, fp16_tokens=True) for _ in ks]
    c16 = consolidate_videos(e16, k16, [3, 5], q, projs, u)
    torch.cuda.synchronize()
    assert torch.equal(c16, c32)
    for a, b in zip(e16, e32):
        _equal_states(_state(a, case), _state(b, case))
    # mixed batch through the C ABI (the Python wrapper sets every handle's dtype from k): handle 0 fp16, handle 1 fp32
    lib = _lib.load()
    before = [_state(e, case) for e in e16]
    _lib.check(lib.infv_ltm_set_token_dtype(e16[0]._h, 3))
    _lib.check(lib.infv_ltm_set_token_dtype(e16[1]._h, 0))
    hs = (C.c_void_p * 2)(e16[0]._h.value, e16[1]._h.value)
    cu = (C.c_int32 * 3)(0, 1, 2)
    k1 = torch.cat([ks[0][:1], ks[1][:1]]).to(dev)
    u1 = torch.from_numpy(np.concatenate([us[0][:1], us[1][:1]])).to(dev)
    ctx = torch.zeros(2, case.n_layers, case.Q, case.H * case.dh, device=dev)
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         case.Q, e16[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0,
                                         C.c_void_p(ctx.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == -1, lib.infv_ltm_last_error()
    assert lib.infv_ltm_launch_count() == n0
    for e, b in zip(e16, before):
        _equal_states(_state(e, case), b)
    # both fp16 again: the same call runs
    _lib.check(lib.infv_ltm_set_token_dtype(e16[1]._h, 3))
    rc = lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), 2, cu, C.c_void_p(k1.data_ptr()), 8, C.c_void_p(q.data_ptr()),
                                         case.Q, e16[0]._proj_array(projs), C.c_void_p(u1.data_ptr()), 0,
                                         C.c_void_p(ctx.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.infv_ltm_last_error()


@pytest.mark.parametrize("leg", ["float32", "bfloat16", "float16"])
def test_token_dtype_benchmark_child_runs_every_leg(dev, leg, capsys):
    """tools/bench_token_dtypes.py: what one child process of the tool does, in this process at 3 chunks and one timed call -- every
    leg, the fp16 one included (its engine has to opt in), prints its JSON line.  Each leg rounds the same randn to its own
    dtype, so the legs' results differ: the line's fields and finiteness are what is checked."""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_token_dtypes.py")
    spec = importlib.util.spec_from_file_location("bench_token_dtypes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.child(leg, 3, 1)
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert line["leg"] == leg and line["chunks"] == 3 and line["pool_rows_alone_chunks"] == 3
    assert line["token_bytes"] == 3 * mod.T * mod.P * mod.D * (4 if leg == "float32" else 2)
    assert line["median_ms"] > 0 and line["pool_rows_alone_ms"] > 0 and np.isfinite(line["checksum"])
