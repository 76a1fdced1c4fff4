"""The dense and general-psi LTM steps across the shapes the C ABI accepts: the points of ``tests/golden/dense_sweep_cases.py``
(two-box dense plans, the rectangular psi as 0/1 rows, the Gaussian family; small shapes that each cross a named tile edge or
mask of the kernels of csrc/ltm_dense.hip and csrc/ltm_psi.hip) driven through the library.  Per point:

a. a per-chunk ``forward`` chain, teacher-forced with the bins of the reference-shaped ``DenseOracle`` (``set_bins`` on every
   layer before every sticky step), against that oracle: ctx 1e-4, B 2e-5 on the real rows and exactly zero on the padding rows,
   last scores rtol 1e-4 / atol 2e-5, sticky probabilities 2e-5 relative; the device's own draw (``last_draw``) may differ from
   the oracle's only by adjacent bins, at most max(4, 4e-5 * draws) of them.  Gaussian points run with the oracle's own ridge
   operators injected (``set_dense_operators``), so the GPU host's LAPACK plays no part; one of them also runs with the
   product's own plan under the looser bounds of ``test_gaussian_family_with_the_products_own_plan``;
b. a free-running chain through every entry point the headers promise to loop over the same step -- ``forward``,
   ``consolidate`` (with ``set_trace``), ``consolidate_pooled``, ``steps``, ``consolidate_q`` and, for chains of one chunk length,
   ``consolidate_videos`` / ``steps_videos`` through their per-handle fallback: the same bits;
c. ``profile_read()`` shows DRAW (sticky points), UPDATE and ATTEND and none of SCORES / CHAIN / UC.

A Gaussian num_basis of 40 is refused when the engine is created, before anything is launched.  The per-point figures are kept
by ``record_parity`` (profiles/dense_sweep_parity.txt is a run's copy).  Needs a real MI355X: run with ``-m gpu``.
"""
import numpy as np
import pytest
import torch

from tests.conftest import record_parity
from tests.golden import dense_sweep_cases as dc

pytestmark = pytest.mark.gpu

CTX_TOL = 1e-4
B_TOL = 2e-5
P_RTOL = 2e-5
TORCH_DTYPE = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
FAST_FAMILIES = ("scores", "chain", "uc")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _engine(pt, dev, inject=True):
    """An engine with a plan per chunk length of the point; Gaussian points get the oracle's own operators (``inject``)."""
    from infinite_video_amd.engine import LTMEngine
    eng = LTMEngine(pt.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=pt.sticky, n_layers=pt.L, max_q=pt.Q, device=dev, nb_samples=pt.S,
                    gaussian_sigmas=pt.sigmas, fp16_tokens=(pt.dtype == "float16"))
    for T in sorted(set(pt.Ts)):
        p = eng.ensure_plan(T)
        assert dc.family_of(p, pt) == pt.family
        if pt.sigmas and inject:
            G_first, G_inf = dc.oracle_chain(pt.name).G[T]
            eng.set_dense_operators(T, np.ascontiguousarray(G_first.T), np.ascontiguousarray(G_inf.T))
    return eng


class _Inputs:
    def __init__(self, pt, dev):
        self.ks, self.qs, self.ws, self.u = dc.point_inputs(pt)
        dt = TORCH_DTYPE[pt.dtype]
        self.k = [torch.from_numpy(k).to(dev).to(dt) for k in self.ks]      # (half-precision points: the values are exact in the dtype already)
        self.q = torch.from_numpy(self.qs).to(dev)
        self.projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in self.ws]
        self.u_dev = torch.from_numpy(self.u).to(dev) if pt.sticky else None

    def u_rows(self, lo, hi):
        return None if self.u_dev is None else self.u_dev[lo:hi].contiguous()

    def u_row(self, c):
        return None if (self.u_dev is None or c == 0) else self.u_dev[c]


def _runs(Ts):
    """Maximal runs of equal chunk length: [(first chunk, one past the last)]; one whole-call entry each."""
    out, c0 = [], 0
    for c in range(1, len(Ts) + 1):
        if c == len(Ts) or Ts[c] != Ts[c0]:
            out.append((c0, c))
            c0 = c
    return out


def _raw_B(eng, layer):
    """All N_pad rows of a layer's coefficients (``export_state`` hands out the real ones only)."""
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import _ptr, _stream
    B = torch.empty(eng.Np, eng.d, device=eng.device, dtype=torch.float32)
    mass = torch.empty(128, device=eng.device, dtype=torch.float32)
    with torch.cuda.device(eng.device):
        _lib.check(eng.lib.infv_ltm_export_state(eng._h, layer, _ptr(B), _ptr(mass), _stream(eng.device)))
    return B.cpu().numpy()


def _families(eng):
    return {k: v[0] for k, v in eng.profile_read().items()}


def _check_families(pt, fam, label):
    assert fam["update"] > 0 and fam["attend"] > 0, f"{pt.name} {label}: ran {fam}"
    assert (fam["draw"] > 0) == pt.sticky, f"{pt.name} {label}: draw launches {fam['draw']} on a {'sticky' if pt.sticky else 'uniform'} chain"
    assert all(fam[k] == 0 for k in FAST_FAMILIES), f"{pt.name} {label}: a dense plan ran the fused path: {fam}"


def _state(eng, pt):
    out = []
    for l in range(pt.L):
        B, mass = eng.export_state(l)
        out.append((B.clone(), mass.clone(), eng.last_draw(l)[0].copy() if pt.sticky else None))
    return out


def _same_state(pt, label, a, b):
    for l in range(pt.L):
        assert torch.equal(a[l][0], b[l][0]), f"{pt.name}: B of {label} differs in its bits, layer {l}"
        assert torch.equal(a[l][1], b[l][1]), f"{pt.name}: sticky masses of {label} differ in their bits, layer {l}"
        if pt.sticky:
            np.testing.assert_array_equal(a[l][2], b[l][2], err_msg=f"{pt.name}: last draw of {label}, layer {l}")


@pytest.mark.parametrize("pt", dc.POINTS, ids=lambda p: p.name)
def test_dense_point(pt, dev):
    from infinite_video_amd.engine import consolidate_videos, steps_videos
    inp = _Inputs(pt, dev)
    ch = dc.oracle_chain(pt.name)
    n, N, L = pt.chunks, pt.N, pt.L
    worst = dict(ctx=0.0, B=0.0, sc=0.0, p=0.0)
    flips = draws = 0

    # ---- a. teacher-forced per-chunk chain against the oracle ----
    eng = _engine(pt, dev)
    eng.profile(True)
    for c in range(n):
        if c and pt.sticky:
            for l in range(L):
                eng.set_bins(l, ch.bins[c, l])                      # (dense plans refuse a partial force)
        y = eng.forward(inp.k[c], inp.q, inp.projs, inp.u_row(c), new_doc=(c == 0)).cpu().numpy()
        e = float(np.abs(y - ch.ctx[c]).max())
        worst["ctx"] = max(worst["ctx"], e)
        assert e <= CTX_TOL, f"{pt.name}: |ctx(HIP) - ctx(oracle)| = {e:.3e} at chunk {c}"
        for l in range(L):
            B = _raw_B(eng, l)
            eB = float(np.abs(B[:N] - ch.B[c, l]).max())
            worst["B"] = max(worst["B"], eB)
            assert eB <= B_TOL, f"{pt.name}: |B(HIP) - B(oracle)| = {eB:.3e} at chunk {c}, layer {l}"
            assert not B[N:].any(), f"{pt.name}: a padding row of B is not zero at chunk {c}, layer {l}"
            got = eng.last_scores(l, pt.Q)                           # (padding columns left out)
            worst["sc"] = max(worst["sc"], float(np.abs(got - ch.scores[c, l]).max()))
            np.testing.assert_allclose(got, ch.scores[c, l], rtol=1e-4, atol=2e-5, err_msg=f"{pt.name}: last scores, chunk {c}, layer {l}")
            if c and pt.sticky:
                bins, _, probs = eng.last_draw(l)                    # the step's OWN draw from its own probabilities
                rel = float(np.abs(ch.probs[c, l] / probs - 1).max())
                worst["p"] = max(worst["p"], rel)
                assert rel <= P_RTOL, f"{pt.name}: sticky probabilities of chunk {c}, layer {l} differ by {rel:.2e} relative"
                dif = bins != ch.bins[c, l]
                flips += int(dif.sum())
                draws += pt.S
                assert np.abs(bins[dif] - ch.bins[c, l][dif]).max(initial=0) <= 1, \
                    f"{pt.name}: a draw of chunk {c}, layer {l} that differs from the oracle's is not an adjacent bin"
    fam = _families(eng)
    eng.profile(False)
    _check_families(pt, fam, "forward chain")
    assert draws == pt.draws
    assert flips <= max(4, int(4e-5 * draws)), f"{pt.name}: {flips} of {draws} oracle draws differ from the HIP path's"
    del eng

    # ---- b. free-running: every entry point loops over the same step ----
    fwd = _engine(pt, dev)
    ctx_f = torch.stack([fwd.forward(inp.k[c], inp.q, inp.projs, inp.u_row(c), new_doc=(c == 0)) for c in range(n)])
    want = _state(fwd, pt)
    runs = _runs(pt.Ts)
    q4 = inp.q.unsqueeze(0).repeat(n, 1, 1, 1).contiguous()
    paths = ["forward"]

    cons = _engine(pt, dev)
    cons.profile(True)
    for (c0, c1) in runs:
        tr = cons.set_trace(c1 - c0)
        y = cons.consolidate(torch.stack(inp.k[c0:c1]), inp.q, inp.projs, inp.u_rows(c0, c1), new_doc=(c0 == 0))
        cons.sync()
        assert torch.equal(y, ctx_f[c0:c1]), f"{pt.name}: consolidate differs from the per-chunk chain in its bits (chunks {c0}..{c1 - 1})"
        traced = tr[0].cpu().numpy()
        if pt.sticky and c1 == n and (traced[-1] >= 0).all():        # a trace row, where the per-chunk loop keeps one, is the draw made
            for l in range(L):
                np.testing.assert_array_equal(traced[-1, l], want[l][2], err_msg=f"{pt.name}: consolidate's trace, layer {l}")
        cons.set_trace(0)
    _check_families(pt, _families(cons), "consolidate")
    cons.profile(False)
    _same_state(pt, "consolidate", _state(cons, pt), want)
    paths.append("consolidate")

    pooled, stp, cq = _engine(pt, dev), _engine(pt, dev), _engine(pt, dev)
    for (c0, c1) in runs:
        k_run = torch.stack(inp.k[c0:c1])
        kbar = pooled.pool(k_run)
        y = pooled.consolidate_pooled(kbar, inp.q, inp.projs, inp.u_rows(c0, c1), new_doc=(c0 == 0))
        assert torch.equal(y, ctx_f[c0:c1]), f"{pt.name}: consolidate_pooled differs from the per-chunk chain in its bits"
        y = stp.steps(kbar, q4[c0:c1].contiguous(), inp.projs, inp.u_rows(c0, c1))
        assert torch.equal(y, ctx_f[c0:c1]), f"{pt.name}: steps differs from the per-chunk chain in its bits"
        y = cq.consolidate_q(k_run, q4[c0:c1].contiguous(), inp.projs, inp.u_rows(c0, c1), new_doc=(c0 == 0))
        assert torch.equal(y, ctx_f[c0:c1]), f"{pt.name}: consolidate_q differs from the per-chunk chain in its bits"
    for label, e in (("consolidate_pooled", pooled), ("steps", stp), ("consolidate_q", cq)):
        _same_state(pt, label, _state(e, pt), want)
        paths.append(label)
    del cons, pooled, stp, cq

    # ---- the multi-video entries (per-handle fallback for dense plans): videos of 2 and 1 chunks cut from the same chunks ----
    if len(runs) == 1 and n >= 3:
        counts = [n - 1, 1]
        k_all = torch.stack(inp.k)
        lone = _engine(pt, dev)                                      # the last chunk as a document of its own
        y_lone = lone.forward(inp.k[n - 1], inp.q, inp.projs, None, new_doc=True)
        for label in ("consolidate_videos", "steps_videos"):
            engs = [_engine(pt, dev) for _ in counts]
            engs[0].profile(True)
            if label == "consolidate_videos":
                yv = consolidate_videos(engs, k_all, counts, inp.q, inp.projs, inp.u_rows(0, n), new_doc=True)
            else:
                yv = steps_videos(engs, engs[0].pool(k_all), counts, inp.q, inp.projs, inp.u_rows(0, n), new_doc=True)
            for e in engs:
                e.sync()
            fam_v = _families(engs[0])
            engs[0].profile(False)
            assert fam_v["update"] > 0 and fam_v["attend"] > 0 and all(fam_v[k] == 0 for k in FAST_FAMILIES), f"{pt.name} {label}: ran {fam_v}"
            assert torch.equal(yv[:n - 1], ctx_f[:n - 1]), f"{pt.name}: {label}, video 0 differs from the per-chunk chain in its bits"
            assert torch.equal(yv[n - 1], y_lone), f"{pt.name}: {label}, video 1 differs from its own first chunk in its bits"
            for l in range(L):
                assert torch.equal(engs[1].export_state(l)[0], lone.export_state(l)[0])
            paths.append(label)
            del engs
        # video 0 stops one chunk short of the chain: its memory is the chain's after n - 1 chunks, checked through its outputs
        del lone

    record_parity(f"[dense sweep] {pt.name} ({pt.family}; {pt.edge}): ran {','.join(k for k in ('project', 'draw', 'update', 'attend', 'scores', 'chain', 'uc') if fam[k])}; "
                  f"ctx {worst['ctx']:.2e}, B {worst['B']:.2e}, scores {worst['sc']:.2e}, probs {worst['p']:.2e} rel, {flips} of {draws} draws differ; "
                  f"same bits: {' = '.join(paths)}")


def test_gaussian_point_with_the_products_own_plan(dev):
    """One Gaussian point with NOTHING injected (``basis_maps.build_gaussian_plan`` through this host's LAPACK), under the bounds
    of ``test_gaussian_family_with_the_products_own_plan``: ctx 1e-3, probabilities 1e-3, B to 2e-2 of its scale, differing draws
    adjacent and at most max(2, draws // 500)."""
    pt = dc.BY_NAME[dc.OWN_PLAN_POINT]
    inp = _Inputs(pt, dev)
    ch = dc.oracle_chain(pt.name)
    eng = _engine(pt, dev, inject=False)
    flips = draws = 0
    worst_ctx = worst_b = 0.0
    for c in range(pt.chunks):
        if c and pt.sticky:
            for l in range(pt.L):
                eng.set_bins(l, ch.bins[c, l])
        y = eng.forward(inp.k[c], inp.q, inp.projs, inp.u_row(c), new_doc=(c == 0)).cpu().numpy()
        worst_ctx = max(worst_ctx, float(np.abs(y - ch.ctx[c]).max()))
        for l in range(pt.L):
            if c and pt.sticky:
                bins, _, probs = eng.last_draw(l)
                np.testing.assert_allclose(probs, ch.probs[c, l], rtol=1e-3, atol=1e-7)
                dif = bins != ch.bins[c, l]
                flips += int(dif.sum())
                draws += int(bins.size)
                assert np.abs(bins[dif] - ch.bins[c, l][dif]).max(initial=0) <= 1, "a differing draw is not an adjacent bin"
            B = eng.export_state(l)[0].cpu().numpy()
            worst_b = max(worst_b, float(np.abs(B - ch.B[c, l]).max()) / float(np.abs(ch.B[c, l]).max()))
    record_parity(f"[dense sweep] {pt.name}, the product's own plan: ctx {worst_ctx:.2e}, B (relative) {worst_b:.2e}, {flips} of {draws} draws differ")
    assert worst_ctx <= 1e-3 and worst_b <= 2e-2
    assert flips <= max(2, draws // 500)


@pytest.mark.parametrize("ref", dc.REFUSALS, ids=lambda r: r.name)
def test_gaussian_num_basis_off_the_tile_is_refused(ref, dev):
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    lib = _lib.load()
    torch.cuda.synchronize()
    before = lib.infv_ltm_launch_count()
    pt = dc.GAUSS
    with pytest.raises(ValueError) as ei:
        LTMEngine(ref.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=True, n_layers=pt.L, max_q=pt.Q, device=dev, nb_samples=pt.S,
                  gaussian_sigmas=ref.sigmas)
    assert lib.infv_ltm_launch_count() == before, "a kernel was launched before the refusal"
    record_parity(f"[dense sweep] refusal {ref.name}: engine creation -> ValueError ({ei.value}), nothing launched")
