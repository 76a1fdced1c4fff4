"""``infv_ltm_source_weights`` on the GPU: the kernel against its ordered fp32 numpy mirror (``density.source_weights`` with
``dtype=np.float32``) bit for bit, the recorded bins of a real ``consolidate`` call traced back to the frames that made the
memory, the attention map of the video, and everything the entry point refuses.

Bounds.  Kernel against fp32 mirror: equality.  ``float64(W) @ pool(k)`` against ``export_state``'s B: the 2e-5 (max norm) that
tests/test_path_transitions_gpu.py holds B to against the oracle -- W is exact to a few 1e-7 relative, B is what the fp32 update
rounded.  ``attn_all`` against the float64 mirror on the device's own mass trace: every term is non-negative, W's entries carry
at most C * (m + 1) roundings (tests/test_source_weights_cpu.py), the float64 sum adds nothing visible, and the result is rounded
to fp32 once: relative C * (m + 1) * 2^-24 + 2^-23 per non-zero entry.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, density, synth
from infinite_video_amd.basis_maps import NB_BINS, build_plan
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

TAU, S = 0.75, 512
B_TOL = 2e-5                       # tests/test_path_transitions_gpu.py: |B - oracle|, max norm
INVALID, UNSUPPORTED, STATE = -1, -2, -4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def small_engine(dev, N, L=2, sticky=True, **kw):
    """A handle whose only use is its plan tables: the pass reads nothing else of it."""
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(N, 1, 64, 32, 1, tau=TAU, sticky=sticky, n_layers=L, max_q=1, device=dev, **kw)


def random_bins(seed, n_chunks, L):
    return np.random.default_rng(seed).integers(0, NB_BINS - 1, size=(n_chunks, L, S)).astype(np.int32)


def mirror(plan, bins, n_chunks, L, dtype=np.float32, **kw):
    """[L, N, M]: the numpy recurrence, layer by layer."""
    return np.stack([density.source_weights(plan, None if bins is None else bins[:, l], n_chunks, dtype=dtype, **kw) for l in range(L)])


def raw(eng, n_chunks, T, bins, W, new_doc=1, g=1, col_begin=0, ld=None, mass=None, attn=None, bad=None):
    """The entry point itself; returns its status."""
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    desc = _lib.SourcesDesc(n_chunks=n_chunks, T=T, new_doc=new_doc, frames_per_source=g, col_begin=col_begin,
                            ld=W.shape[-1] if ld is None else ld)
    with torch.cuda.device(eng.device):
        return eng.lib.infv_ltm_source_weights(eng._h, C.byref(desc), ptr(bins), ptr(W), ptr(mass), ptr(attn), ptr(bad),
                                               C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))


# ---------------------------------------------------------------------------------------------- the kernel against the mirror
KERNEL_CASES = [  # N, T, chunks, g, L, sticky -- columns = chunks * T / g
    (16, 8, 6, 1, 1, True),          # 48 columns: less than one tile
    (256, 16, 63, 16, 2, True),      # one below the tile width
    (256, 16, 64, 16, 2, True),      # the tile width
    (256, 16, 65, 16, 2, True),      # one above
    (256, 16, 13, 1, 2, True),       # 208 columns: four tiles, the last one partial, later tiles start at later chunks
    (272, 16, 5, 1, 2, True),        # the 32-column tiles of num_basis above 256: 80 columns, the last tile half full
    (272, 16, 33, 16, 2, True),      # ... and one column past a tile
    (64, 8, 1, 8, 2, True),          # g = T with one chunk: a single column, the first-chunk operator alone
    (64, 8, 9, 2, 2, False),         # not sticky: bins_all = NULL, the plan's uniform resampling
    (256, 16, 7, 4, 2, False),
]


@pytest.mark.parametrize("N,T,n_chunks,g,L,sticky", KERNEL_CASES)
def test_kernel_equals_the_ordered_fp32_mirror(dev, N, T, n_chunks, g, L, sticky):
    eng = small_engine(dev, N, L, sticky)
    plan = eng.ensure_plan(T)
    assert not plan.dense
    bins = random_bins(N + n_chunks, n_chunks, L) if sticky else None      # (different bins in every layer)
    want = mirror(plan, bins, n_chunks, L, frames_per_source=g)
    dbins = torch.from_numpy(bins).to(dev) if sticky else torch.empty(n_chunks, 0, 0, dtype=torch.int32, device=dev)
    got = eng.source_weights(dbins, T, frames_per_source=g)
    assert tuple(got.shape) == (L, N, n_chunks * T // g)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert L == 1 or not sticky or n_chunks == 1 or not torch.equal(got[0], got[1])     # (the layers drew differently)


def test_pad_columns_are_not_touched(dev):
    """ld > M: the columns beyond the call's last source keep a NaN sentinel, in every row of every layer -- and in attn_all."""
    N, T, n_chunks, L = 256, 16, 9, 2                             # 144 columns in a row stride of 200
    eng = small_engine(dev, N, L)
    plan = eng.ensure_plan(T)
    bins = random_bins(1, n_chunks, L)
    M, ld = n_chunks * T, 200
    W = torch.full((L, N, ld), float("nan"), device=dev)
    mass = torch.rand(n_chunks, L, N, device=dev)
    attn = torch.full((n_chunks, L, ld), float("nan"), device=dev)
    assert raw(eng, n_chunks, T, torch.from_numpy(bins).to(dev), W, mass=mass, attn=attn) == 0
    assert bool(torch.isnan(W[:, :, M:]).all()) and bool(torch.isnan(attn[:, :, M:]).all())
    assert torch.equal(W[:, :, :M].cpu(), torch.from_numpy(mirror(plan, bins, n_chunks, L, frames_per_source=1)))
    assert bool(torch.isfinite(attn[:, :, :M]).all())             # every live column of every chunk is written
    for c in (0, 3):                                              # ... with zeros where the chunk has seen nothing yet
        assert not bool(attn[c, :, (c + 1) * T:M].any()) and bool((attn[c, :, c * T:(c + 1) * T - 1] > 0).all())   # (a chunk's last frame sits at t = 1.0, in no box)


def test_two_calls_equal_one_and_a_new_document_forgets(dev):
    N, T, g, L, C1, C2 = 256, 16, 16, 2, 5, 70                    # col_begin = 5: inside a tile, no multiple of 4
    eng = small_engine(dev, N, L)
    plan = eng.ensure_plan(T)
    bins = random_bins(2, C1 + C2, L)
    db = torch.from_numpy(bins).to(dev)
    whole = eng.source_weights(db, T, frames_per_source=g)
    W1 = eng.source_weights(db[:C1].contiguous(), T, frames_per_source=g)
    W2 = eng.source_weights(db[C1:].contiguous(), T, new_doc=False, W=W1, col_begin=C1, frames_per_source=g)
    assert tuple(W2.shape) == (L, N, C1 + C2)
    assert torch.equal(W2, whole)
    assert torch.equal(whole.cpu(), torch.from_numpy(mirror(plan, bins, C1 + C2, L, frames_per_source=g)))
    # new_doc = 1 over a carried W: the older columns become 0 whatever they held, the rest is the new document's
    buf = torch.full((L, N, 76), float("nan"), device=dev)
    buf[:, :, :C1] = W1
    assert raw(eng, C2, T, db[C1:].contiguous(), buf, new_doc=1, g=g, col_begin=C1) == 0
    assert not bool(buf[:, :, :C1].any()) and bool(torch.isnan(buf[:, :, C1 + C2:]).all())
    fresh = mirror(plan, bins[C1:], C2, L, frames_per_source=g)
    assert torch.equal(buf[:, :, C1:C1 + C2].cpu(), torch.from_numpy(fresh))
    with pytest.raises(ValueError):
        eng.source_weights(db[C1:].contiguous(), T, new_doc=False, W=None, col_begin=C1, frames_per_source=g)


# ---------------------------------------------------------------------------------------------- end to end
H, DH, D, P = 12, 64, 768, 32
DM = H * DH
E2E = {"headline": (256, 256, 2, 32), "videochat2-like": (16, 64, 2, 32)}     # T, N, L, Q
E2E_CHUNKS = 70                                                  # the first chunk, two full sub-batches of the fused chain, a short one


def rows_per_box(plan):
    m = np.diff(plan.inf_old_ptr).astype(np.int64)
    np.add.at(m, plan.inf_row_box, plan.inf_row_end - plan.inf_row_begin)
    return int(m.max())


@pytest.fixture(scope="module", params=sorted(E2E))
def video(request, dev):
    """One ``consolidate`` call with both traces on, and the pass on what it recorded."""
    from infinite_video_amd.engine import LTMEngine
    T, N, L, Q = E2E[request.param]
    n = E2E_CHUNKS
    eng = LTMEngine(N, H, DH, D, P, tau=TAU, sticky=True, n_layers=L, max_q=Q, device=dev)
    plan = eng.ensure_plan(T)
    gen = torch.Generator(device=dev).manual_seed(17)
    k = torch.randn(n, T * P, D, device=dev, generator=gen) * 0.5
    projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.layer_projections(l, D, DM)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, DM) for l in range(L)])).to(dev)
    u = torch.from_numpy(synth.gibbs_uniforms(n, L)).to(dev)
    bins, _ = eng.set_trace(n)
    mass = eng.set_mass_trace(n)
    eng.consolidate(k, q, projs, u, new_doc=True)
    eng.sync()
    eng.set_trace(0)
    eng.set_mass_trace(0)
    W, attn = eng.source_weights(bins, T, frames_per_source=1, mass=mass.contiguous())
    return dict(name=request.param, eng=eng, plan=plan, T=T, N=N, L=L, n=n, k=k, bins=bins.cpu().numpy(), mass=mass.cpu().numpy(),
                W=W, attn=attn)


def test_recorded_bins_give_the_memory_back(video):
    v = video
    want = mirror(v["plan"], v["bins"], v["n"], v["L"], frames_per_source=1)
    assert torch.equal(v["W"].cpu(), torch.from_numpy(want))
    kbar = v["eng"].pool(v["k"]).reshape(v["n"] * v["T"], D).double()
    worst = 0.0
    for l in range(v["L"]):
        B = v["eng"].export_state(l)[0][:v["N"]].double()
        err = float((v["W"][l].double() @ kbar - B).abs().max())
        print(f"{v['name']} layer {l}: max |W pool(k) - B| = {err:.3e} (max|B| {float(B.abs().max()):.3f})")
        worst = max(worst, err)
    record_parity(f"[source weights] {v['name']}: {v['n']} chunks of the fused chain, g = 1: W equals the fp32 mirror; "
                  f"max |float64(W) pool(k) - export_state B| = {worst:.2e} (bound {B_TOL:.0e})")
    assert worst <= B_TOL


def test_attention_map_against_the_float64_mirror(video):
    v = video
    bound = v["n"] * (rows_per_box(v["plan"]) + 1) * 2.0 ** -24 + 2.0 ** -23
    got = v["attn"].cpu().numpy().astype(np.float64)
    worst = 0.0
    for l in range(v["L"]):
        _, want = density.source_attention(v["mass"][:, l], v["plan"], v["bins"][:, l], v["n"], frames_per_source=1)
        nz = want != 0
        assert np.array_equal(got[:, l] != 0, nz)
        worst = max(worst, float((np.abs(got[:, l][nz] - want[nz]) / want[nz]).max()))
    print(f"{v['name']}: max relative |attn_all - float64 mirror| = {worst:.3e} (bound {bound:.3e})")
    record_parity(f"[source weights] {v['name']}: attn_all vs the float64 mirror on the device's mass trace: max relative {worst:.2e} "
                  f"(bound {bound:.2e})")
    assert worst <= bound
    # the wrapper's normalised form, and the frames the last chunk attends to most
    _, norm = v["eng"].source_weights(torch.from_numpy(v["bins"]).to(v["W"].device), v["T"], frames_per_source=1,
                                      mass=torch.from_numpy(v["mass"]).to(v["W"].device), normalise=True)
    assert torch.allclose(norm.sum(-1), torch.ones_like(norm[..., 0]), rtol=0, atol=1e-5)
    top = density.top_sources(got[-1, 0], 5, frames_per_source=1)
    assert len(top) == 5 and all(0 <= f0 < v["n"] * v["T"] and f1 == f0 + 1 for _, f0, f1, _ in top)


# ---------------------------------------------------------------------------------------------- the memory is left alone
def test_the_pass_does_not_touch_the_memory(dev):
    from infinite_video_amd.engine import LTMEngine
    N, T, L, Q, n1, n2 = 64, 8, 2, 32, 6, 4
    rng = np.random.default_rng(5)
    kbar = torch.from_numpy((rng.standard_normal((n1 + n2, T, D)) * 0.5).astype(np.float32)).to(dev)
    projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.layer_projections(l, D, DM)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, DM) for l in range(L)])).to(dev)
    u = torch.from_numpy(synth.gibbs_uniforms(n1 + n2, L)).to(dev)
    lib = _lib.load()

    def run(with_pass):
        eng = LTMEngine(N, H, DH, D, P, tau=TAU, sticky=True, n_layers=L, max_q=Q, device=dev)
        bins, _ = eng.set_trace(n1)
        eng.consolidate_pooled(kbar[:n1], q, projs, u[:n1], new_doc=True)
        eng.set_trace(0)
        eng.sync()
        if with_pass:
            before = [x.clone() for l in range(L) for x in eng.export_state(l)]
            W = torch.full((L, N, n1 * T), float("nan"), device=dev)
            n0 = lib.infv_ltm_launch_count()
            assert raw(eng, n1, T, bins, W) == 0
            assert lib.infv_ltm_launch_count() - n0 == 1          # one launch, nothing else
            eng.sync()
            assert bool(torch.isfinite(W).all())
            after = [x for l in range(L) for x in eng.export_state(l)]
            assert all(torch.equal(a, b) for a, b in zip(before, after))
        ctx = eng.consolidate_pooled(kbar[n1:], q, projs, u[n1:], new_doc=False)
        eng.sync()
        return ctx, [x.clone() for l in range(L) for x in eng.export_state(l)], eng.rng_position

    ctx_a, mem_a, pos_a = run(True)
    ctx_b, mem_b, pos_b = run(False)
    assert torch.equal(ctx_a, ctx_b) and pos_a == pos_b == n1 + n2
    assert all(torch.equal(a, b) for a, b in zip(mem_a, mem_b))


# ---------------------------------------------------------------------------------------------- bins out of range
def test_an_unwritten_trace_row(dev):
    """A row of -1 (what ``set_trace`` leaves where nothing drew) is never an index: it resamples zero rows, the result equals the
    mirror's with those bins masked, and the counter holds the row's S bins once per layer -- not once per column tile."""
    N, T, n_chunks, L = 256, 16, 13, 2                            # 208 columns: four tiles
    eng = small_engine(dev, N, L)
    plan = eng.ensure_plan(T)
    bins = random_bins(3, n_chunks, L)
    bins[4] = -1
    bins[7, 1, :10] = NB_BINS - 1                                  # the draw has n_bins - 1 outcomes: 127 is out of range too
    bins[0] = -1                                                  # (the first chunk of a document reads no bins: not counted)
    db = torch.from_numpy(bins).to(dev)
    W = torch.full((L, N, n_chunks * T), float("nan"), device=dev)
    bad = torch.zeros(L, dtype=torch.int32, device=dev)
    assert raw(eng, n_chunks, T, db, W, bad=bad) == 0
    assert bad.tolist() == [S, S + 10]
    assert torch.equal(W.cpu(), torch.from_numpy(mirror(plan, bins, n_chunks, L, frames_per_source=1)))
    clean = random_bins(3, n_chunks, L)
    assert not np.array_equal(mirror(plan, clean, n_chunks, L, frames_per_source=1), W.cpu().numpy())
    # without a counter the result is the same; the wrapper reads the counter back and raises
    W2 = torch.full_like(W, float("nan"))
    assert raw(eng, n_chunks, T, db, W2) == 0 and torch.equal(W, W2)
    with pytest.raises(ValueError, match="unwritten trace row"):
        eng.source_weights(db, T, frames_per_source=1)
    # a call that continues a document reads the bins of its first chunk too
    bad.zero_()
    assert raw(eng, 2, T, db[:2].contiguous(), W2, new_doc=0, col_begin=0, bad=bad, ld=W2.shape[-1]) == 0
    assert bad.tolist() == [S, S]


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(dev):
    from infinite_video_amd.engine import LTMEngine
    T, L, n = 8, 2, 3
    sentinel = 12345.0

    def refused(eng, code, N=None, **kw):
        N = eng.Np if N is None else N
        W = kw.pop("W", None)
        W = torch.full((L, N, 32), sentinel, device=dev) if W is None else W
        for name in ("mass", "attn"):
            if kw.get(name) is True:
                kw[name] = torch.full((n, L, N if name == "mass" else 32), sentinel, device=dev)
        sticky = kw.pop("sticky_bins", True)
        bins = torch.zeros(n, L, S, dtype=torch.int32, device=dev) if sticky else None
        rc = raw(eng, kw.pop("n_chunks", n), kw.pop("T", T), bins, W, **kw)
        torch.cuda.synchronize()
        assert rc == code, (rc, eng.lib.infv_ltm_last_error())
        assert bool((W == sentinel).all())
        for name in ("mass", "attn"):
            if kw.get(name) is not None:
                assert bool((kw[name] == sentinel).all())

    eng = small_engine(dev, 64, L)
    eng.ensure_plan(T)
    assert raw(eng, n, T, torch.zeros(n, L, S, dtype=torch.int32, device=dev), torch.empty(L, 64, 32, device=dev)) == 0
    refused(eng, STATE, T=4)                                      # no plan for T
    refused(eng, INVALID, g=3)                                    # g does not divide T
    refused(eng, INVALID, g=0)
    refused(eng, INVALID, ld=20)                                  # ld below col_begin + C * T / g = 24
    refused(eng, INVALID, col_begin=12, ld=32)                    # ... 12 + 24 = 36
    refused(eng, INVALID, ld=26, W=torch.full((L, 64, 26), sentinel, device=dev))   # no multiple of 4
    refused(eng, INVALID, sticky_bins=False)                      # sticky with NULL bins
    refused(eng, INVALID, mass=True)                              # mass_all without attn_all
    refused(eng, INVALID, attn=True)                              # ... and the other way round
    refused(eng, INVALID, n_chunks=0)
    refused(eng, INVALID, col_begin=-4)
    refused(eng, INVALID, W=torch.full((L * 64 * 32 + 1,), sentinel, device=dev)[1:].view(L, 64, 32))   # W off a 16-byte boundary
    assert eng.lib.infv_ltm_source_weights(eng._h, None, None, None, None, None, None, None) == INVALID
    plain = small_engine(dev, 64, L, sticky=False)
    plain.ensure_plan(T)
    refused(plain, INVALID)                                       # bins given to a handle that is not sticky
    dense = small_engine(dev, 96, L)
    assert dense.ensure_plan(T).dense
    refused(dense, UNSUPPORTED)                                   # a dense plan
    gauss = LTMEngine(64, 1, 64, 32, 1, tau=TAU, sticky=True, n_layers=L, max_q=1, device=dev, gaussian_sigmas=[0.03, 0.1])
    assert gauss.ensure_plan(T).psi
    refused(gauss, UNSUPPORTED)                                   # a general-psi plan
