"""Every shape the C ABI accepts, against the CPU oracle: the points of ``tests/golden/sweep_cases.py`` driven through

1. ``engine.consolidate`` (the whole-call path, with ``set_trace`` so every chunk's bins and probabilities come back),
2. a per-chunk ``engine.forward`` chain,
3. where the lockstep kernels take the shape, ``consolidate_videos`` over three videos of unequal length cut from the same
   chunks, and ``steps_videos`` on the pooled frames,

each compared with ``ClosedFormOracle(..., nb_samples=S)`` walked with the path's own bins (as
``test_timed_path_gpu._check_against_oracle`` does): ctx 1e-4, B 2e-5, sticky probabilities 2e-5 relative, last scores
rtol 1e-4 / atol 2e-5, ``last_draw`` indices equal, a draw that differs from the oracle's own an adjacent bin and at most
max(4, 4e-5 * draws) of them per path.  Paths the headers promise bit-identical (``consolidate_pooled`` == ``consolidate``,
``steps_videos`` == ``consolidate_videos``) must be so at every point, ``profile_read()`` must show the kernel families the
table names, and the refusal points must be refused before any kernel is launched.  The video Q-former's short-term attention is
swept at the C ABI against an fp64 torch reference.  Needs a real MI355X: run with ``-m gpu``.

The per-point figures are kept by ``record_parity`` (profiles/config_sweep_parity.txt is a run's copy).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import ltm_oracle as O
from tests.conftest import record_parity
from tests.golden import sweep_cases as sc

pytestmark = pytest.mark.gpu

CTX_TOL = 1e-4
B_TOL = 2e-5
P_RTOL = 2e-5
TORCH_DTYPE = {"float32": torch.float32, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _engine(pt, dev):
    from infinite_video_amd.engine import LTMEngine
    old = os.environ.get("INFV_VPROJ_SPLIT")
    if pt.v_split:
        os.environ["INFV_VPROJ_SPLIT"] = "1"                    # read by infv_ltm_create, per handle
    try:
        return LTMEngine(pt.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=pt.sticky, n_layers=pt.L, max_q=pt.Q, device=dev,
                         nb_samples=pt.S, max_batch_chunks=pt.max_batch_chunks)
    finally:
        if pt.v_split:
            if old is None:
                del os.environ["INFV_VPROJ_SPLIT"]
            else:
                os.environ["INFV_VPROJ_SPLIT"] = old


class _Inputs:
    def __init__(self, pt, dev):
        self.ks, self.qs, self.ws, self.u = sc.point_inputs(pt)
        dt = TORCH_DTYPE[pt.dtype]
        self.k = [torch.from_numpy(k).to(dev).to(dt) for k in self.ks]      # (bf16 points: the values are bf16-exact already)
        self.q = torch.from_numpy(self.qs).to(dev)
        self.projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in self.ws]
        self.u_dev = torch.from_numpy(self.u).to(dev) if pt.sticky else None

    def u_rows(self, lo, hi):
        return None if self.u_dev is None else self.u_dev[lo:hi].contiguous()


def _runs(Ts):
    """Maximal runs of equal chunk length: [(first chunk, one past the last)]; one consolidate call each."""
    out, c0 = [], 0
    for c in range(1, len(Ts) + 1):
        if c == len(Ts) or Ts[c] != Ts[c0]:
            out.append((c0, c))
            c0 = c
    return out


class _Walker:
    """The CPU oracle over a chain of the point's chunks, fed a path's own bins; walks are cached by those bins."""

    def __init__(self, pt, inp):
        self.pt, self.inp, self.cache = pt, inp, {}

    def walk(self, chunk_ids, bins):
        """chunk_ids: the chunks of one document in order; bins [n, L, S] (rows of chunk 0 ignored; -1 rows: the oracle's own
        draw) or None.  Returns (ctx [n, L, Q, dm], own bins, own probs, oracles)."""
        pt = self.pt
        key = (tuple(chunk_ids), None if bins is None else bins.tobytes())
        if key in self.cache:
            return self.cache[key]
        n = len(chunk_ids)
        orcs = [O.ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, *self.inp.ws[l], tokens_per_frame=pt.P, nb_samples=pt.S)
                for l in range(pt.L)]
        ctx = np.empty((n, pt.L, pt.Q, pt.dm), np.float32)
        own_bins = np.full((n, pt.L, pt.S), -1, np.int64)
        own_probs = np.zeros((n, pt.L, 127), np.float32)
        for i, c in enumerate(chunk_ids):
            for l in range(pt.L):
                force = None
                if i and pt.sticky and bins is not None and bins[i, l, 0] >= 0:
                    force = bins[i, l]
                ctx[i, l] = orcs[l].step(self.inp.ks[c], self.inp.qs[l], new_doc=(i == 0), u=self.inp.u[c, l] if (i and pt.sticky) else None,
                                         bins_override=force)
                if i and pt.sticky:
                    own_bins[i, l], own_probs[i, l] = orcs[l].last_bins, orcs[l].last_probs
        self.cache[key] = (ctx, own_bins, own_probs, orcs)
        return self.cache[key]


class _Stats:
    def __init__(self):
        self.ctx = self.B = self.p = self.sc = 0.0
        self.flips = self.draws = 0


def _check_chain(pt, label, walker, chunk_ids, ctx_hip, bins_hip, probs_hip, eng, st):
    """One path's chain against the oracle.  ctx_hip [n, L, Q, dm] host; bins_hip [n, L, S] (int, -1 where the path kept no
    record) or None; probs_hip [n, L, >=127] or None; eng: the engine in the chain's final state."""
    n = len(chunk_ids)
    ctx_ref, own_bins, own_probs, orcs = walker.walk(chunk_ids, bins_hip)
    err = np.abs(ctx_ref - ctx_hip).reshape(n, -1).max(axis=1)
    st.ctx = max(st.ctx, float(err.max()))
    assert err.max() <= CTX_TOL, f"{pt.name} {label}: |ctx(HIP) - ctx(oracle)| = {err.max():.3e} at chunk {int(err.argmax())}"
    flips0, draws0 = st.flips, st.draws
    if pt.sticky and n > 1 and bins_hip is not None:
        for i in range(1, n):
            for l in range(pt.L):
                if bins_hip[i, l, 0] < 0:
                    continue
                d = own_bins[i, l] != bins_hip[i, l]
                st.flips += int(d.sum())
                st.draws += pt.S
                assert np.abs(own_bins[i, l][d] - bins_hip[i, l][d]).max(initial=0) <= 1, \
                    f"{pt.name} {label}: a draw of chunk {i} layer {l} that differs from the oracle's is not an adjacent bin"
                if probs_hip is not None:
                    rel = float(np.abs(own_probs[i, l] / probs_hip[i, l, :127] - 1).max())
                    st.p = max(st.p, rel)
                    assert rel <= P_RTOL, f"{pt.name} {label}: sticky probabilities of chunk {i} layer {l} differ by {rel:.2e} relative"
    # the rule of tests/test_timed_path_gpu.py, per path
    assert st.flips - flips0 <= max(4, int(4e-5 * (st.draws - draws0))), \
        f"{pt.name} {label}: {st.flips - flips0} of {st.draws - draws0} oracle draws differ from the HIP path's"
    if eng is not None:
        for l in range(pt.L):
            eB = float(np.abs(eng.export_state(l)[0].cpu().numpy() - orcs[l].B_past).max())
            st.B = max(st.B, eB)
            assert eB <= B_TOL, f"{pt.name} {label}: |B(HIP) - B(oracle)| = {eB:.3e} in layer {l}"
            got = eng.last_scores(l, pt.Q)
            st.sc = max(st.sc, float(np.abs(got - orcs[l].S_prev).max()))
            np.testing.assert_allclose(got, orcs[l].S_prev, rtol=1e-4, atol=2e-5, err_msg=f"{pt.name} {label}: last scores, layer {l}")
            if pt.sticky and n > 1:
                bins_l, idx_l, _ = eng.last_draw(l)
                if bins_hip is not None and bins_hip[n - 1, l, 0] >= 0:
                    np.testing.assert_array_equal(bins_l, bins_hip[n - 1, l], err_msg=f"{pt.name} {label}: last_draw bins, layer {l}")
                np.testing.assert_array_equal(idx_l, orcs[l].last_idx, err_msg=f"{pt.name} {label}: last_draw indices, layer {l}")


def _families(prof):
    return {k: v[0] for k, v in prof.items()}


def _video_counts(n):
    a = (n + 1) // 2
    b = max(1, (n - a) // 2) if n - a > 0 else 0
    return [x for x in (a, b, n - a - b) if x > 0]


@pytest.mark.parametrize("pt", sc.POINTS, ids=lambda p: p.name)
def test_sweep_point(pt, dev):
    from infinite_video_amd.engine import consolidate_videos, steps_videos
    inp = _Inputs(pt, dev)
    walker = _Walker(pt, inp)
    n, ids = pt.chunks, list(range(pt.chunks))
    st = _Stats()
    ps = sc._ps(pt)

    # ---- 2. the per-chunk forward chain (free-running; it keeps every chunk's own draw) ----
    fwd = _engine(pt, dev)
    ctx_f = np.empty((n, pt.L, pt.Q, pt.dm), np.float32)
    bins_f = np.full((n, pt.L, pt.S), -1, np.int64)
    probs_f = np.zeros((n, pt.L, 127), np.float32)
    for c in ids:
        y = fwd.forward(inp.k[c], inp.q, inp.projs, None if (inp.u_dev is None or c == 0) else inp.u_dev[c], new_doc=(c == 0))
        ctx_f[c] = y.cpu().numpy()
        if c and pt.sticky:
            for l in range(pt.L):
                b, _, p = fwd.last_draw(l)
                bins_f[c, l], probs_f[c, l] = b, p
    _check_chain(pt, "forward chain", walker, ids, ctx_f, bins_f, probs_f, fwd, st)

    # ---- 1. consolidate: one call per run of equal chunk length ----
    eng = _engine(pt, dev)
    eng.profile(True)
    ctx_c = np.empty_like(ctx_f)
    bins_c = np.full((n, pt.L, pt.S), -1, np.int64)
    probs_c = np.zeros((n, pt.L, 127), np.float32)
    pooled_ok = len(_runs(pt.Ts)) == 1
    for (c0, c1) in _runs(pt.Ts):
        tr = eng.set_trace(c1 - c0)
        y = eng.consolidate(torch.stack(inp.k[c0:c1]), inp.q, inp.projs, inp.u_rows(c0, c1), new_doc=(c0 == 0))
        eng.sync()
        ctx_c[c0:c1] = y.cpu().numpy()
        bins_c[c0:c1] = tr[0].cpu().numpy()
        probs_c[c0:c1] = tr[1].cpu().numpy()[:, :, :127]
        eng.set_trace(0)
    fam = _families(eng.profile_read())
    eng.profile(False)
    if pt.families == "fast":
        assert fam["chain"] > 0 and fam["uc"] > 0 and fam["update"] == 0 and fam["attend"] == 0, f"{pt.name}: expected the fused chain, ran {fam}"
        if pt.sticky and n > 1:
            assert (bins_c[1:, :, 0] >= 0).all(), f"{pt.name}: the fused chain left chunks untraced"
    else:
        assert fam["update"] > 0 and fam["attend"] > 0 and fam["chain"] == 0 and fam["uc"] == 0, f"{pt.name}: expected the per-chunk stages, ran {fam}"
        # the per-chunk stages keep no trace: the oracle is walked with the forward chain's bins (the same step, chunk by chunk);
        # the chain's last draw is checked against them below
        bins_c[1:] = np.where(bins_c[1:] >= 0, bins_c[1:], bins_f[1:])
    traced = (bins_c[1:, :, 0] >= 0).all() and pt.families == "fast"
    f0, d0 = st.flips, st.draws
    _check_chain(pt, "consolidate", walker, ids, ctx_c, bins_c if pt.sticky else None, probs_c if traced else None, eng, st)
    if not traced:
        st.flips, st.draws = f0, d0                # (the forward chain's bins stood in: their flips are counted already)

    # ---- consolidate_pooled on pool(k): bit-identical to consolidate (include/infv_ltm.h) ----
    if pooled_ok:
        pe = _engine(pt, dev)
        k_all = torch.stack(inp.k)
        kbar = pe.pool(k_all)
        yp = pe.consolidate_pooled(kbar, inp.q, inp.projs, inp.u_rows(0, n), new_doc=True)
        pe.sync()
        assert np.array_equal(yp.cpu().numpy(), ctx_c), f"{pt.name}: consolidate_pooled differs from consolidate in its bits"
        for l in range(pt.L):
            assert torch.equal(pe.export_state(l)[0], eng.export_state(l)[0]), f"{pt.name}: B of consolidate_pooled differs in its bits"
            if pt.sticky and n > 1:
                np.testing.assert_array_equal(pe.last_draw(l)[0], eng.last_draw(l)[0])
        del pe

    # ---- 3. the lockstep entries over three videos cut from the same chunks ----
    vid = "n/a"
    if pooled_ok and sc.videos_supported(pt, ps):
        counts = _video_counts(n)
        cu = np.concatenate([[0], np.cumsum(counts)])
        engs = [_engine(pt, dev) for _ in counts]
        traces = [e.set_trace(cnt) for e, cnt in zip(engs, counts)]
        engs[0].profile(True)
        k_all = torch.stack(inp.k)
        yv = consolidate_videos(engs, k_all, counts, inp.q, inp.projs, inp.u_rows(0, n), new_doc=True)
        for e in engs:
            e.sync()
        fam_v = _families(engs[0].profile_read())
        engs[0].profile(False)
        assert fam_v["update"] > 0 and fam_v["attend"] > 0 and fam_v["chain"] == 0 and fam_v["uc"] == 0, f"{pt.name}: lockstep step ran {fam_v}"
        if pt.sticky and max(counts) > 1:
            assert fam_v["draw"] > 0, f"{pt.name}: lockstep step ran no draw kernel: {fam_v}"
        yv_h = yv.cpu().numpy()
        for v, e in enumerate(engs):
            lo, hi = int(cu[v]), int(cu[v + 1])
            bv = traces[v][0].cpu().numpy().astype(np.int64)
            pv = traces[v][1].cpu().numpy()[:, :, :127]
            _check_chain(pt, f"consolidate_videos video {v}", walker, list(range(lo, hi)), yv_h[lo:hi], bv if pt.sticky else None,
                         pv if pt.sticky else None, e, st)
            e.set_trace(0)
        engs2 = [_engine(pt, dev) for _ in counts]
        kbar = engs2[0].pool(k_all)
        ys = steps_videos(engs2, kbar, counts, inp.q, inp.projs, inp.u_rows(0, n), new_doc=True)
        for e in engs2:
            e.sync()
        assert torch.equal(ys, yv), f"{pt.name}: steps_videos(pool(k)) differs from consolidate_videos(k) in its bits"
        for e, e2 in zip(engs, engs2):
            for l in range(pt.L):
                assert torch.equal(e.export_state(l)[0], e2.export_state(l)[0]) and torch.equal(e.export_state(l)[1], e2.export_state(l)[1])
                np.testing.assert_array_equal(e.last_draw(l)[0], e2.last_draw(l)[0])
        vid = "x".join(str(c) for c in counts)
        del engs, engs2

    record_parity(f"[config sweep] {pt.name}: path {sc.expected_path(pt)}, ran {','.join(k for k in ('project', 'draw', 'update', 'attend', 'scores', 'chain', 'uc') if fam[k])}, "
                  f"videos {vid}: ctx {st.ctx:.2e}, B {st.B:.2e}, scores {st.sc:.2e}, probs {st.p:.2e} rel, {st.flips} of {st.draws} draws differ")


# ---------------------------------------------------------------------------------------------------------------------
# refusal points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", sc.REFUSALS, ids=lambda r: r.name)
def test_refusal_point(ref, dev):
    """Refused in create or at the first call with INFV_ERR_UNSUPPORTED / INFV_ERR_INVALID and a message, before any kernel
    is launched; a handle that exists stays usable."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    pt = sc.SMALL
    torch.cuda.synchronize()
    if ref.where == "create":
        base = dict(num_basis=pt.N, n_heads=pt.H, head_size=pt.dh, d_in=pt.d, tokens_per_frame=pt.P, n_layers=pt.L, nb_samples=pt.S,
                    sticky=1, max_q=pt.Q, max_batch_chunks=32)
        base.update(ref.cfg)
        cfg = _lib.Config(*(base[k] for k, _ in _lib.Config._fields_))
        h = C.c_void_p()
        before = lib.infv_ltm_launch_count()
        with torch.cuda.device(dev):
            rc = lib.infv_ltm_create(C.byref(cfg), C.byref(h))
        assert rc in (-1, -2), f"{ref.name}: infv_ltm_create returned {rc}"
        assert lib.infv_ltm_last_error(), f"{ref.name}: no message in infv_ltm_last_error()"
        assert lib.infv_ltm_launch_count() == before
        assert not h.value
        record_parity(f"[config sweep] refusal {ref.name}: create -> {rc} ({lib.infv_ltm_last_error().decode()})")
        return
    inp = _Inputs(pt, dev)
    eng = _engine(pt, dev)
    eng.ensure_plan(pt.T)
    Qbad = ref.call_Q
    qbad = torch.zeros(pt.L, Qbad, pt.dm, device=dev)
    out = torch.zeros(pt.chunks, pt.L, Qbad, pt.dm, device=dev)
    k_all = torch.stack(inp.k)
    from infinite_video_amd.engine import _ptr, _stream
    before = lib.infv_ltm_launch_count()
    codes = []
    with torch.cuda.device(dev):
        codes.append(lib.infv_ltm_consolidate(eng._h, _ptr(k_all), pt.chunks, pt.T, _ptr(qbad), Qbad, eng._proj_array(inp.projs), _ptr(inp.u_dev), 1,
                                              _ptr(out), _stream(dev)))
        msg = lib.infv_ltm_last_error()
        codes.append(lib.infv_ltm_forward(eng._h, _ptr(inp.k[0]), pt.T, _ptr(qbad), Qbad, eng._proj_array(inp.projs), None, 1, _ptr(out), _stream(dev)))
        qbad4 = torch.zeros(pt.chunks, pt.L, Qbad, pt.dm, device=dev)
        codes.append(lib.infv_ltm_consolidate_q(eng._h, _ptr(k_all), pt.chunks, pt.T, _ptr(qbad4), Qbad, eng._proj_array(inp.projs), _ptr(inp.u_dev), 1,
                                                _ptr(out), _stream(dev)))
        kbar = torch.zeros(pt.T, pt.d, device=dev)
        codes.append(lib.infv_ltm_forward_into(eng._h, _ptr(inp.k[0]), 0, pt.T, _ptr(kbar), _ptr(qbad), Qbad, eng._proj_array(inp.projs), None, _ptr(out),
                                               _stream(dev)))
    assert all(rc in (-1, -2) for rc in codes), f"{ref.name}: {codes}"
    assert msg and lib.infv_ltm_last_error()
    assert lib.infv_ltm_launch_count() == before, "a kernel was launched before the refusal"
    record_parity(f"[config sweep] refusal {ref.name}: first call -> {codes} ({msg.decode()})")
    # the handle is usable afterwards
    y = eng.consolidate(k_all, inp.q, inp.projs, inp.u_dev, new_doc=True)
    eng.sync()
    st = _Stats()
    walker = _Walker(pt, inp)
    _check_chain(pt, "after the refusal", walker, list(range(pt.chunks)), y.cpu().numpy(), None, None, None, st)
    # ... and refusals on a handle that HOLDS a memory leave it as it was, new_doc or not: too long a query, a sticky step
    # without its uniforms (the first step of forward / forward_into, a later chunk of consolidate_q behind new_doc)
    eng.sync()
    state = [tuple(t.clone() for t in eng.export_state(l)) for l in range(pt.L)]
    draws = [eng.last_draw(l)[0].copy() for l in range(pt.L)]
    qok4 = inp.q.unsqueeze(0).repeat(pt.chunks, 1, 1, 1).contiguous()
    outq = torch.zeros(pt.chunks, pt.L, pt.Q, pt.dm, device=dev)
    before = lib.infv_ltm_launch_count()
    codes = []
    with torch.cuda.device(dev):
        pa = eng._proj_array(inp.projs)
        codes.append(lib.infv_ltm_forward(eng._h, _ptr(inp.k[0]), pt.T, _ptr(qbad), Qbad, pa, _ptr(inp.u_dev[1]), 1, _ptr(out), _stream(dev)))
        codes.append(lib.infv_ltm_forward(eng._h, _ptr(inp.k[0]), pt.T, _ptr(inp.q), pt.Q, pa, None, 0, _ptr(outq), _stream(dev)))
        codes.append(lib.infv_ltm_forward_into(eng._h, _ptr(inp.k[0]), 0, pt.T, _ptr(kbar), _ptr(inp.q), pt.Q, pa, None, _ptr(outq), _stream(dev)))
        codes.append(lib.infv_ltm_consolidate_q(eng._h, _ptr(k_all), pt.chunks, pt.T, _ptr(qbad4), Qbad, pa, _ptr(inp.u_dev), 1, _ptr(out), _stream(dev)))
        codes.append(lib.infv_ltm_consolidate_q(eng._h, _ptr(k_all), pt.chunks, pt.T, _ptr(qok4), pt.Q, pa, None, 1, _ptr(outq), _stream(dev)))
        codes.append(lib.infv_ltm_forward(eng._h, _ptr(inp.k[0]), pt.T + 1, _ptr(inp.q), pt.Q, pa, _ptr(inp.u_dev[1]), 1, _ptr(outq), _stream(dev)))
    assert all(rc in (-1, -2, -3) for rc in codes), f"{ref.name}: on a handle with memory {codes}"     # (-3: no plan for T + 1)
    assert lib.infv_ltm_launch_count() == before, "a kernel was launched before a refusal on a handle with memory"
    assert eng.has_memory, "a refused call reset the memory"
    for l in range(pt.L):
        B, mass = eng.export_state(l)
        assert torch.equal(B, state[l][0]) and torch.equal(mass, state[l][1]), f"a refused call changed the memory of layer {l}"
        np.testing.assert_array_equal(eng.last_draw(l)[0], draws[l])
    record_parity(f"[config sweep] refusal {ref.name}: on a handle with memory -> {codes}, memory unchanged")
    # ... and the chain goes on from it
    k_more = inp.k[1]
    y2 = eng.forward(k_more, inp.q, inp.projs, inp.u_dev[1], new_doc=False)
    ref_eng = _engine(pt, dev)
    ref_eng.consolidate(k_all, inp.q, inp.projs, inp.u_dev, new_doc=True)
    y3 = ref_eng.forward(k_more, inp.q, inp.projs, inp.u_dev[1], new_doc=False)
    assert torch.equal(y2, y3), "the chain after the refusals differs from one that saw none"


# ---------------------------------------------------------------------------------------------------------------------
# video Q-former: infv_vqf_short_attention at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def torch_short_attention(frames, xq, wk, bk, wv, bv, H):
    """Plain PyTorch reference of the short-term cross-attention (Qformer.py:225-301 with zero masks), any head count."""
    dh = xq.shape[1] // H
    K = torch.nn.functional.linear(frames, wk, bk)
    V = torch.nn.functional.linear(frames, wv, bv)
    heads = lambda x: x.reshape(x.shape[0], H, dh).permute(1, 0, 2)
    s = torch.matmul(heads(xq), heads(K).transpose(-1, -2)) / math.sqrt(dh)
    return torch.matmul(torch.softmax(s, -1), heads(V)).permute(1, 0, 2).reshape(xq.shape[0], -1)


@pytest.mark.parametrize("vp", sc.VQF_POINTS, ids=lambda p: p.name)
def test_short_attention_sweep(vp, dev):
    from infinite_video_amd import _lib
    H, dw, Q, nt = vp.n_heads, vp.enc_width, vp.n_query, vp.n_tokens
    hid = 64 * H
    g = torch.Generator().manual_seed(1000 + 7 * H + dw + 3 * Q + nt)
    frames = torch.randn(nt, dw, generator=g)
    xq = torch.randn(Q, hid, generator=g)
    wk, wv = torch.randn(hid, dw, generator=g) * 0.02, torch.randn(hid, dw, generator=g) * 0.02
    bk, bv = torch.randn(hid, generator=g) * 0.02, torch.randn(hid, generator=g) * 0.02
    along = torch.randn(Q, hid, generator=g)
    want_short = torch_short_attention(frames.double(), xq.double(), wk.double(), bk.double(), wv.double(), bv.double(), H)
    lib = _lib.load()
    d = lambda t: t.to(dev).contiguous()
    fr, q, a = d(frames), d(xq), d(along)
    dwk, dbk, dwv, dbv = d(wk), d(bk), d(wv), d(bv)
    worst = {}
    for alpha, use_long, exact in ((0.9, True, True), (1.0, False, True), (0.9, True, False), (1.0, False, False)):
        cfg = _lib.VqfConfig(n_layers=2, n_heads=H, hidden=hid, inter=hid, enc_width=dw, tokens_per_frame=32, n_query=Q, proj_out=64,
                             nb_samples=512, alpha=alpha, ln_eps=1e-12)
        h = C.c_void_p()
        _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
        _lib.check(lib.infv_vqf_set_precision(h, int(exact)))
        key, val = _lib.Linear(dwk.data_ptr(), dbk.data_ptr()), _lib.Linear(dwv.data_ptr(), dbv.data_ptr())
        out = torch.empty(Q, hid, device=dev)
        _lib.check(lib.infv_vqf_short_attention(h, C.c_void_p(fr.data_ptr()), nt, C.c_void_p(q.data_ptr()), C.byref(key), C.byref(val),
                                                C.c_void_p(a.data_ptr() if use_long else 0), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        want = alpha * want_short + (1 - alpha) * along.double() if use_long else want_short
        got = out.cpu().numpy()
        worst[(exact, use_long)] = float(np.abs(got - want.float().numpy()).max())
        _lib.check(lib.infv_vqf_destroy(h))
        tol = dict(atol=2e-5, rtol=1e-4) if exact else dict(atol=1e-4, rtol=1e-3)
        np.testing.assert_allclose(got, want.float().numpy(), **tol, err_msg=f"{vp.name}: exact={exact} long={use_long}")
    split = dw % 64 == 0 and nt % 64 == 0
    record_parity(f"[config sweep] short_attention {vp.name} (H {H}, enc {dw}, Q {Q}, tokens {nt}; default path {'split-bf16' if split else 'exact fp32'}): "
                  f"exact {max(worst[(True, True)], worst[(True, False)]):.2e}, default {max(worst[(False, True)], worst[(False, False)]):.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# video Q-former: the whole-layer entry points away from hidden 768 (InfVideoEncoder fixes 12 heads and enc_width == hidden)
# ---------------------------------------------------------------------------------------------------------------------
QF_ATOL = 2e-4            # tests/test_qformer_gpu.py's bound
QF_CONFIGS = [
    # (id, n_layers, n_heads, inter, enc_width, n_query, P, proj_out)
    ("h512_L1", 1, 8, 1024, 512, 16, 64, 64),
    ("h512_L3", 3, 8, 1024, 512, 16, 64, 64),
    ("h1024_L2", 2, 16, 4096, 1024, 32, 32, 256),
]


def _vqf_weights_struct(w, n_layers, dev):
    from infinite_video_amd import _lib
    keep = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in w.items()}
    lin = lambda name: _lib.Linear(keep[name + ".weight"].data_ptr(), keep[name + ".bias"].data_ptr())
    ln = lambda name: _lib.LayerNorm(keep[name + ".weight"].data_ptr(), keep[name + ".bias"].data_ptr())
    s = _lib.VqfWeights()
    s.query_tokens = keep["video_query_tokens"].data_ptr()
    s.emb_ln = ln("bert.embeddings.LayerNorm")
    for l in range(n_layers):
        p = f"bert.encoder.layer.{l}."
        a, x = p + "attention.", p + "crossattention."
        s.layer[l] = _lib.VqfLayer(lin(a + "self.query"), lin(a + "self.key"), lin(a + "self.value"), lin(a + "output.dense"),
                                   ln(a + "output.LayerNorm"), lin(x + "self.query"), lin(x + "self.key"), lin(x + "self.value"),
                                   lin(x + "output.dense"), ln(x + "output.LayerNorm"), lin(p + "intermediate_query.dense"),
                                   lin(p + "output_query.dense"), ln(p + "output_query.LayerNorm"))
    s.llama_proj = lin("llama_proj")
    return s, keep


@pytest.mark.parametrize("name,L,H,inter,enc,Q,P,proj_out", QF_CONFIGS, ids=[c[0] for c in QF_CONFIGS])
def test_encode_chunk_and_video_off_768(name, L, H, inter, enc, Q, P, proj_out, dev):
    """infv_vqf_encode_chunk (chunk by chunk) and infv_vqf_encode_video (layer-major) against VideoQformerOracle at 2e-4."""
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine
    from oracle.qformer_oracle import VideoQformerOracle
    lib = _lib.load()
    hid, N, tau, alpha, T, Cn, S = 64 * H, 64, 0.75, 0.9, 4, 3, 512
    w = synth.video_qformer_weights(n_layers=L, hidden=hid, inter=inter, enc_width=enc, n_query=Q, proj_out=proj_out)
    frames = np.stack([synth.frame_tokens(c, T, P, enc) for c in range(Cn)])
    u = synth.gibbs_uniforms(Cn, L)
    orc = VideoQformerOracle(w, N, tau, alpha, True, n_layers=L, n_heads=H, tokens_per_frame=P)
    want = [orc.encode_chunk(frames[c], c == 0, u[c]) for c in range(Cn)]
    ws, keep = _vqf_weights_struct(w, L, dev)
    fr, ud = torch.from_numpy(frames).to(dev), torch.from_numpy(u).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cfg = _lib.VqfConfig(n_layers=L, n_heads=H, hidden=hid, inter=inter, enc_width=enc, tokens_per_frame=P, n_query=Q, proj_out=proj_out,
                         nb_samples=S, alpha=alpha, ln_eps=1e-12)
    worst = {}
    for entry in ("encode_chunk", "encode_video"):
        h = C.c_void_p()
        _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
        engs = [LTMEngine(N, H, 64, enc, P, tau=tau, sticky=True, n_layers=1, max_q=Q, device=dev) for _ in range(L)]
        for e in engs:
            e.ensure_plan(T)
        handles = (C.c_void_p * L)(*[e._h.value for e in engs])
        hidden = torch.empty(Cn, Q, hid, device=dev)
        llama = torch.empty(Cn, Q, proj_out, device=dev)
        mean = torch.empty(Q, proj_out, device=dev)
        with torch.cuda.device(dev):
            if entry == "encode_chunk":
                for c in range(Cn):
                    _lib.check(lib.infv_vqf_encode_chunk(h, handles, C.c_void_p(fr[c].data_ptr()), T, C.byref(ws),
                                                         C.c_void_p(ud[c].data_ptr() if c else 0), int(c == 0),
                                                         C.c_void_p(hidden[c].data_ptr()), C.c_void_p(llama[c].data_ptr()), stream))
            else:
                _lib.check(lib.infv_vqf_encode_video(h, handles, C.c_void_p(fr.data_ptr()), Cn, T, C.byref(ws), C.c_void_p(ud.data_ptr()), 1,
                                                     C.c_void_p(hidden.data_ptr()), C.c_void_p(llama.data_ptr()), C.c_void_p(mean.data_ptr()), stream))
        torch.cuda.synchronize()
        for e in engs:
            e.sync()
        hh, ll = hidden.cpu().numpy(), llama.cpu().numpy()
        worst[entry] = max(max(float(np.abs(hh[c] - want[c][0]).max()), float(np.abs(ll[c] - want[c][1]).max())) for c in range(Cn))
        for c in range(Cn):
            np.testing.assert_allclose(hh[c], want[c][0], atol=QF_ATOL, rtol=0, err_msg=f"{name} {entry}: hidden of chunk {c}")
            np.testing.assert_allclose(ll[c], want[c][1], atol=QF_ATOL, rtol=0, err_msg=f"{name} {entry}: llama of chunk {c}")
        if entry == "encode_video":
            np.testing.assert_allclose(mean.cpu().numpy(), np.mean(np.stack([x[1] for x in want]), 0), atol=QF_ATOL, rtol=0)
        for l, e in enumerate(engs):
            np.testing.assert_allclose(e.export_state(0)[0].cpu().numpy(), orc.ltm[l].B_past, atol=B_TOL, rtol=0,
                                       err_msg=f"{name} {entry}: memory of layer {l}")
        _lib.check(lib.infv_vqf_destroy(h))
        del engs
    record_parity(f"[config sweep] video Q-former {name} (hidden {hid}, {H} heads, inter {inter}, enc {enc}, Q {Q}, P {P}, {L} layers): "
                  f"encode_chunk {worst['encode_chunk']:.2e}, encode_video {worst['encode_video']:.2e}")
