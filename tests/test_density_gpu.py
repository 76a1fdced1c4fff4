"""The attention-density read-outs on the GPU: ``infv_ltm_density`` / ``infv_ltm_masses`` after a step, the mass trace of the
multi-chunk calls, the drop-in module's ``output_density``.

Bounds.  Scores of the HIP path agree with the reference within delta(S) = 2e-5 + 1e-4 * max|S| (tests/test_ltm_gpu.py).
Through scores perturbed by delta, ``alphas`` moves by a factor within e^{+-4 delta} (numerator, segment integral and grand sum
each move by at most e^{+-delta}... twice over the two normalisations) and a mass by a factor within e^{+-2 delta}.  The
evaluation itself gets EPS = 2e-6 (four times the 4.9e-7 by which the reference's own fp32 pickle differs from the float64
closed form on its own scores) plus 2^-22 * max|S| for the fp32 rounding of s - max.  Measured values are recorded through
``record_parity``.
"""
from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, density, synth
from infinite_video_amd.basis_maps import build_grid_plan, build_plan
from oracle import ltm_oracle as O
from tests.conftest import record_parity
from tests.golden.cases import CASES, DENSE_CASES, GOLDEN_DIR, call_seed, call_uniforms, case_inputs, load_golden

pytestmark = pytest.mark.gpu

EPS = 2e-6
H, DH, D, P = 12, 64, 768, 32
DM = H * DH
BY_NAME = {c.name: c for c in CASES + DENSE_CASES}
DENSITY_CASES = ("cfg1_sticky", "peaked", "tau09", "n144", "n96_dense", "headline")


def delta(S) -> float:
    return 2e-5 + 1e-4 * float(np.abs(S).max())


def rel_err(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_DIR + "/density.npz")


def _engine(dev, N, Q, L=1, variant="VL", **kw):
    from infinite_video_amd.engine import LTMEngine
    d, p = (D, P) if variant == "VL" else (1024, 196)
    return LTMEngine(N, H, DH, d, p, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev, **kw)


def _weights(dev, L, d=D, seed=0):
    ws = [synth.layer_projections(l, d, DM, seed=synth.SEED_W + seed) for l in range(L)]
    return ws, [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in ws]


# ---------------------------------------------------------------------------------------------- the drop-in module
@pytest.mark.parametrize("name", DENSITY_CASES)
def test_module_leaves_the_reference_alphas(dev, golden, name, tmp_path):
    """The golden chain through ``LongTermAttention`` with ``output_density = True``: ``self.alphas`` against the pickle the real
    reference wrote after the same forward (rtol 4 delta + EPS), every drawn bin the reference's, the pickle written through
    ``density_path`` the same tensor."""
    from infinite_video_amd.long_term_attention_gibbs import LongTermAttention
    case, g = BY_NAME[name], load_golden(BY_NAME[name])
    ks, qs, ws = case_inputs(case)
    q_idx = golden[f"{name}/q_idx"]
    mods = []
    for l in range(case.n_layers):
        wk, bk, wv, bv = ws[l]
        pk, pv = torch.nn.Linear(case.d, case.dm), torch.nn.Linear(case.d, case.dm)
        with torch.no_grad():
            pk.weight.copy_(torch.from_numpy(wk)); pk.bias.copy_(torch.from_numpy(bk))
            pv.weight.copy_(torch.from_numpy(wv)); pv.bias.copy_(torch.from_numpy(bv))
        m = LongTermAttention(head_size=case.dh, length=case.d, target_len=case.d, attn_func="softmax", attn_num_basis=case.N,
                              continuous=True, attn_drop=0.1, infinite_memory=True, n_layers=2, n_heads=case.H, affines=True,
                              mask=True, mask_type="cnn", kl_regularizer=False, proj_key=pk.to(dev), proj_value=pv.to(dev),
                              sigma_0=None, mu_0=None, sticky_memories=case.sticky, sigmas=None, tau=case.tau, d_model=case.dm)
        assert m.output_density is False and m.alphas is None
        m.output_density = True
        m.density_path = str(tmp_path / f"alphas_{l}")
        mods.append(m)
    worst, checked = 0.0, 0
    for c in range(len(case.chunk_T)):
        k = torch.from_numpy(ks[c]).unsqueeze(0).to(dev)
        for l, m in enumerate(mods):
            torch.manual_seed(call_seed(case, c, l))
            m(k, torch.from_numpy(qs[l]).unsqueeze(0).to(dev), new_doc=(c in case.new_doc_at), layer_n=l)
            tag = f"c{c}_l{l}"
            if tag + "_bins" in g.files:
                np.testing.assert_array_equal(m._engine.last_draw(0)[0], g[tag + "_bins"])
            key = f"{name}/{tag}_alphas"
            if key not in golden.files:
                continue
            assert tuple(m.alphas.shape) == (case.Q, 1, case.H, 768) and m.alphas.is_cuda
            with open(m.density_path, "rb") as f:
                assert torch.equal(pickle.load(f), m.alphas.cpu())
            want = golden[key]
            tol = 4 * delta(golden[f"{name}/{tag}_scores"]) + EPS
            err = rel_err(m.alphas.cpu().numpy()[q_idx], want)
            print(f"{name} {tag}: max relative |alphas - reference pickle| = {err:.3e} (bound {tol:.3e})")
            assert err <= tol
            worst, checked = max(worst, err), checked + 1
    assert checked == 2 * case.n_layers
    record_parity(f"[density] module {name}: alphas vs the reference pickle over {checked} calls: max relative {worst:.2e}")


# ---------------------------------------------------------------------------------------------- the kernels alone
SHAPES = [  # N, Q, T, variant, q_scale
    (16, 1, 2, "VL", 1.0), (64, 5, 8, "VL", 1.0), (144, 32, 8, "VL", 1.0), (96, 33, 8, "VL", 1.0), (256, 96, 255, "VL", 1.0),
    (272, 32, 8, "VL", 1.0), (64, 96, 8, "VC", 1.0), (64, 32, 8, "VL", 500.0),
]


def _rel_err_fp32(got, want) -> float:
    """Relative error where the value, and the e^{s - max} behind it, are normal fp32 numbers (want >= 1e-30); below that an
    fp32 output cannot hold the float64 value to any relative bound (it underflows), and must merely be as small."""
    big = want >= 1e-30
    assert (got[~big] <= 2e-30).all()
    return rel_err(got[big], want[big])


@pytest.mark.parametrize("N,Q,T,variant,q_scale", SHAPES)
def test_kernels_against_the_mirror_on_the_device_scores(dev, N, Q, T, variant, q_scale):
    """Two forwards, then ``density`` / ``masses`` of each layer against the float64 mirror on the device's own last scores,
    within EPS + 2^-22 max|S|.  N = 144: fp32 boxes; 96: dense plan, grid points in two boxes; 272: beyond the 256 columns of
    one wave pass; Q = 33 / 96: past a row block; the scaled query drives max|S| beyond 90."""
    L = 2
    d, p = (D, P) if variant == "VL" else (1024, 196)
    eng = _engine(dev, N, Q, L, variant)
    ws, projs = _weights(dev, L, d)
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, DM, scale=q_scale) for l in range(L)])).to(dev)
    u = torch.from_numpy(synth.gibbs_uniforms(2, L)).to(dev)
    for c in range(2):
        eng.forward(torch.from_numpy(synth.frame_tokens(c, T, p, d)).to(dev), q, projs, u[c], new_doc=(c == 0))
    plan, gp = build_plan(T, N, 0.75), build_grid_plan(N)
    one = build_grid_plan(N, ((0.0, 1.0, 1000),))
    for l in range(L):
        S = eng.last_scores(l, Q)
        smax = float(np.abs(S).max())
        if q_scale > 1:
            assert smax > 90
        tol = EPS + 2.0 ** -22 * smax
        a = eng.density(l, Q).cpu().numpy()
        assert a.shape == (Q, 1, H, 768) and np.isfinite(a).all()
        e_a = _rel_err_fp32(a, density.reference_alphas(S, gp))
        mass = eng.masses(l, Q).cpu().numpy()
        e_m = rel_err(mass, density.box_masses(S, plan.readout_w[:N], plan.readout_w_out))
        a1 = eng.density(l, Q, ((0.0, 1.0, 1000),)).cpu().numpy()          # a non-reference grid: one segment of 1000 points
        e_1 = _rel_err_fp32(a1, density.reference_alphas(S, one))
        np.testing.assert_allclose(a1.astype(np.float64).sum(-1), 1.0, rtol=0, atol=1e-5)
        print(f"N={N} Q={Q} T={T} {variant} layer {l}: max|S| {smax:.1f}  alphas {e_a:.2e}  masses {e_m:.2e}  one-segment {e_1:.2e}  (bound {tol:.2e})")
        assert max(e_a, e_m, e_1) <= tol
        record_parity(f"[density] kernels N={N} Q={Q} T={T} {variant} x{q_scale:g} layer {l}: alphas {e_a:.2e} masses {e_m:.2e} bound {tol:.2e}")


# ---------------------------------------------------------------------------------------------- the trace
TN, TQ, TT, TL, TS = 64, 32, 8, 2, 512


def _pooled_video(dev, n_chunks, seed=5):
    rng = np.random.default_rng(seed)
    kbar = (rng.standard_normal((n_chunks, TT, D)) * 0.5).astype(np.float32)
    ws, projs = _weights(dev, TL)
    qs = [synth.layer_query(l, TQ, DM) for l in range(TL)]
    u = synth.gibbs_uniforms(n_chunks, TL, seed=77 + seed)
    return kbar, ws, projs, qs, u


def _oracle_masses(kbar, ws, qs, u, bins, chunks=None):
    """Masses of the ClosedFormOracle's scores, walked with the call's own traced bins: [C, L, N] float64, and max delta."""
    plan = build_plan(TT, TN, 0.75)
    n = kbar.shape[0]
    out = np.full((n, TL, TN), np.nan)
    dmax = 0.0
    for l in range(TL):
        orc = O.ClosedFormOracle(TN, H, DH, 0.75, True, *ws[l], tokens_per_frame=1)   # (frame means in: one token per frame)
        for c in range(n):
            q = qs[c][l] if isinstance(qs, np.ndarray) and qs.ndim == 4 else qs[l]
            orc.step(kbar[c], q, new_doc=(c == 0), u=u[c, l] if c else None, bins_override=bins[c, l] if c else None)
            if chunks is None or c in chunks:
                out[c, l] = density.box_masses(orc.S_prev, plan.readout_w, plan.readout_w_out)
            dmax = max(dmax, delta(orc.S_prev))
    return out, dmax


@pytest.mark.parametrize("n_chunks", [70, 200, 800])
def test_trace_of_the_fused_chain(dev, n_chunks):
    """``consolidate_pooled`` on frame means: 70 chunks = the first chunk, two full sub-batches and a short one; 200: the five
    workspace sets wrap; 800: 42-chunk sub-batches and the one-launch pooling form's schedule.  Every row against the oracle
    (rtol 2 delta + EPS); at 800 chunks the oracle still walks the whole call, and every 8th chunk plus every sub-batch's first
    and last chunk is compared."""
    kbar, ws, projs, qs, u = _pooled_video(dev, n_chunks)
    eng = _engine(dev, TN, TQ, TL, max_batch_chunks=42)
    bins_all, _ = eng.set_trace(n_chunks)
    trace = eng.set_mass_trace(n_chunks)
    assert bool(torch.isnan(trace).all())
    ctx = eng.consolidate_pooled(torch.from_numpy(kbar).to(dev), torch.from_numpy(np.stack(qs)).to(dev), projs,
                                 torch.from_numpy(u).to(dev), new_doc=True)
    eng.sync()
    assert bool(torch.isfinite(ctx).all())
    got = trace.cpu().numpy()
    assert np.isfinite(got).all()                                 # every chunk wrote, the document's first included
    chunks = None
    if n_chunks > 200:
        sub = 42
        chunks = {0} | set(range(0, n_chunks, 8))
        for c0 in range(1, n_chunks, sub):
            chunks |= {c0, min(c0 + sub, n_chunks) - 1}
    want, dmax = _oracle_masses(kbar, ws, qs, u, bins_all.cpu().numpy(), chunks)
    sel = sorted(chunks) if chunks is not None else list(range(n_chunks))
    tol = 2 * dmax + EPS
    err = rel_err(got[sel], want[sel])
    print(f"{n_chunks} chunks: max relative |trace - oracle masses| over {len(sel)} rows = {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    np.testing.assert_allclose(got.sum(-1), 1.0, rtol=0, atol=2e-2)             # (the rest is the grid point in no box)
    record_parity(f"[density] fused trace {n_chunks} chunks: {len(sel)} rows vs oracle masses: max relative {err:.2e} (bound {tol:.2e})")
    eng.set_mass_trace(0)
    eng.set_trace(0)


def test_trace_of_the_per_chunk_stages(dev):
    """``steps`` and ``consolidate_q`` (a query per chunk) against the oracle, a dense-plan ``consolidate`` (N = 96) against the
    masses of the real reference's scores; in each the last row has the bits of ``masses`` called afterwards."""
    n = 12
    kbar, ws, projs, qs, u = _pooled_video(dev, n, seed=9)
    qc = np.stack([np.stack([synth.layer_query(l, TQ, DM, seed=synth.SEED_Q + 31 * c) for l in range(TL)]) for c in range(n)])
    kb, qd, ud = torch.from_numpy(kbar).to(dev), torch.from_numpy(qc).to(dev), torch.from_numpy(u).to(dev)
    # steps
    eng = _engine(dev, TN, TQ, TL)
    trace = eng.set_mass_trace(n)
    eng.steps(kb, qd, projs, ud)
    eng.sync()
    free = _engine(dev, TN, TQ, TL)                               # the same chain chunk by chunk, for its drawn bins
    bins = np.zeros((n, TL, TS), np.int32)
    for c in range(n):
        free.step(kb[c], qd[c], projs, ud[c])
        if c:
            bins[c] = np.stack([free.last_draw(l)[0] for l in range(TL)])
    want, dmax = _oracle_masses(kbar, ws, qc, u, bins)
    got = trace.cpu().numpy()
    err = rel_err(got, want)
    assert err <= 2 * dmax + EPS
    for l in range(TL):
        assert torch.equal(trace[n - 1, l], eng.masses(l, TQ))
    record_parity(f"[density] steps trace: max relative {err:.2e} (bound {2 * dmax + EPS:.2e})")
    # consolidate_q: tokens whose frame means are kbar (P identical tokens per frame)
    k = kb[:, :, None, :].expand(n, TT, P, D).reshape(n, TT * P, D).contiguous()
    eng2 = _engine(dev, TN, TQ, TL)
    trace2 = eng2.set_mass_trace(n)
    eng2.consolidate_q(k, qd, projs, ud, new_doc=True)
    eng2.sync()
    err2 = rel_err(trace2.cpu().numpy(), want)
    assert err2 <= 2 * dmax + EPS
    for l in range(TL):
        assert torch.equal(trace2[n - 1, l], eng2.masses(l, TQ))
    # dense plan: the n96_dense golden chain through consolidate
    case = BY_NAME["n96_dense"]
    g = load_golden(case)
    ks, qs96, ws96 = case_inputs(case)
    ks = [x for x, T in zip(ks, case.chunk_T) if T == 16]         # (consolidate takes chunks of one length: the first two)
    ks = ks[:2]
    from infinite_video_amd.engine import LTMEngine
    e96 = LTMEngine(96, H, DH, D, P, tau=case.tau, sticky=True, n_layers=case.n_layers, max_q=case.Q, device=dev)
    assert e96.ensure_plan(16).dense
    t96 = e96.set_mass_trace(len(ks))
    us = np.stack([[call_uniforms(case, c, l) for l in range(case.n_layers)] for c in range(len(ks))])
    e96.consolidate(torch.from_numpy(np.stack(ks)).to(dev), torch.from_numpy(np.stack(qs96)).to(dev),
                    [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in ws96],
                    torch.from_numpy(us).to(dev), new_doc=True)
    e96.sync()
    p96 = build_plan(16, 96, case.tau)
    for c in range(len(ks)):
        for l in range(case.n_layers):
            S = g[f"c{c}_l{l}_scores"]
            want96 = density.box_masses(S, p96.readout_w[:96], p96.readout_w_out)
            assert rel_err(t96[c, l].cpu().numpy(), want96) <= 2 * delta(S) + EPS
    for l in range(case.n_layers):
        assert torch.equal(t96[len(ks) - 1, l], e96.masses(l, case.Q))


def test_trace_capacity_and_trace_on_against_off(dev):
    """Capacity 10 under a 70-chunk call leaves rows >= 10 untouched; the trace changes no output bit (ctx, the chain-state
    blob, the traced bins) and no launch of the default path: off, the call launches what it launched before the trace was
    ever set; on, exactly one launch more per update + read-out launch (the first chunk, two full sub-batches, a short one)."""
    n = 70
    kbar, ws, projs, qs, u = _pooled_video(dev, n, seed=3)
    kb, q, ud = torch.from_numpy(kbar).to(dev), torch.from_numpy(np.stack(qs)).to(dev), torch.from_numpy(u).to(dev)
    lib = _lib.load()

    eng = _engine(dev, TN, TQ, TL)
    bins, _ = eng.set_trace(n)
    nB, nKV = TL * TN * D, TL * TN * 2 * DM

    def blob_parts():
        """The chain-state blob without the K' half of the projected memory, which the fused chain does not maintain."""
        blob = eng.export_chain_state(TQ)
        kv = blob[16 + nB:16 + nB + nKV].reshape(TL, TN, 2, DM)
        return torch.cat([blob[:16 + nB], kv[:, :, 1].reshape(-1), blob[16 + nB + nKV:]]).clone()

    def run(cap):
        tr = eng.set_mass_trace(cap)
        n0 = lib.infv_ltm_launch_count()
        ctx = eng.consolidate_pooled(kb, q, projs, ud, new_doc=True)
        launches = lib.infv_ltm_launch_count() - n0
        eng.sync()
        return ctx, blob_parts(), bins.clone(), tr, launches

    run(n)                                                          # (workspaces grow, plans upload: not counted)
    ctx0, blob0, bins0, _, launches0 = run(0)
    ctx1, blob1, bins1, tr, launches1 = run(10)
    assert torch.equal(ctx0, ctx1) and torch.equal(blob0, blob1) and torch.equal(bins0, bins1)
    assert bool(torch.isfinite(tr[:10]).all()) and bool(torch.isnan(tr[10:]).all())
    assert launches1 == launches0 + 2                               # capacity 10: the first chunk and the sub-batch of chunks 1..32 have rows to write
    ctx2, blob2, bins2, tr2, launches2 = run(n)
    assert torch.equal(ctx0, ctx2) and torch.equal(blob0, blob2) and torch.equal(bins0, bins2)
    assert launches2 == launches0 + 4                               # first chunk + sub-batches of 32, 32 and 5 chunks
    assert bool(torch.isfinite(tr2).all()) and torch.equal(tr2[:10], tr[:10])
    # cleared again, the call launches what it launched before
    ctx3, blob3, bins3, _, launches3 = run(0)
    assert launches3 == launches0 and torch.equal(ctx0, ctx3) and torch.equal(blob0, blob3) and torch.equal(bins0, bins3)


def test_refusals_leave_the_memory_alone(dev):
    from infinite_video_amd.engine import LTMEngine, steps_videos
    n = 3
    kbar, ws, projs, qs, u = _pooled_video(dev, n, seed=4)
    kb, q, ud = torch.from_numpy(kbar).to(dev), torch.from_numpy(np.stack(qs)).to(dev), torch.from_numpy(u).to(dev)
    eng = _engine(dev, TN, TQ, TL)
    # no memory yet
    with pytest.raises(_lib.LTMError) as e:
        eng.masses(0, TQ)
    assert e.value.code == -4
    eng.consolidate_pooled(kb, q, projs, ud, new_doc=True)
    B0 = eng.export_state(0)[0].clone()
    # density without a grid plan (the raw call: LTMEngine.density would register one)
    out = torch.empty(TQ, 1, H, 768, device=dev)
    assert eng.lib.infv_ltm_density(eng._h, 0, TQ, C.c_void_p(out.data_ptr()), None) == -4
    # the lockstep calls refuse a handle with a trace set, before any device work
    other = _engine(dev, TN, TQ, TL)
    other.consolidate_pooled(kb, q, projs, ud, new_doc=True)
    eng.set_mass_trace(4)
    pos = eng.rng_position
    with pytest.raises(_lib.LTMError) as e:
        steps_videos([other, eng], torch.cat([kb, kb]), [n, n], q, projs, torch.cat([ud, ud]), new_doc=True)
    assert e.value.code == -2
    assert eng.has_memory and other.has_memory and eng.rng_position == pos
    assert torch.equal(eng.export_state(0)[0], B0)
    eng.set_mass_trace(0)
    # after import_state the handle keeps no scores
    a = eng.density(0, TQ)
    assert bool(torch.isfinite(a).all())
    eng.import_state(0, B0.contiguous(), None, projs[0])
    for call in (lambda: eng.density(0, TQ), lambda: eng.masses(0, TQ)):
        with pytest.raises(_lib.LTMError) as e:
            call()
        assert e.value.code == -4
    assert torch.equal(eng.export_state(0)[0], B0)
    # after import_chain_state the read-outs equal the exporting handle's
    src = _engine(dev, TN, TQ, TL)
    src.consolidate_pooled(kb, q, projs, ud, new_doc=True)
    dst = _engine(dev, TN, TQ, TL)
    dst.ensure_plan(TT)
    dst.import_chain_state(TQ, src.export_chain_state(TQ))
    for l in range(TL):
        assert torch.equal(dst.density(l, TQ), src.density(l, TQ))
        assert torch.equal(dst.masses(l, TQ), src.masses(l, TQ))
    # general-psi plans: refused by all four
    gauss = LTMEngine(64, H, DH, D, P, tau=0.75, sticky=True, n_layers=1, max_q=TQ, device=dev, gaussian_sigmas=[0.03, 0.1])
    gauss.ensure_plan(TT)
    for call in (lambda: gauss.set_grid_plan(), lambda: gauss.set_mass_trace(4), lambda: gauss.density(0, TQ), lambda: gauss.masses(0, TQ)):
        with pytest.raises(_lib.LTMError) as e:
            call()
        assert e.value.code == -2


def test_trace_through_the_video_qformer(dev):
    """``infv_vqf_encode_video`` steps each layer's handle with the multi-chunk entry points, so a trace set on a layer's handle
    is written by it: 6 chunks at the ``qf_small`` shape against a per-chunk ``encode_chunk`` + ``infv_ltm_masses`` loop (rtol
    2 delta + EPS: layer 0 runs the fused chain in the one call and the per-call step in the loop); the call's outputs keep
    their bits."""
    from dataclasses import replace
    from infinite_video_amd.video_qformer import InfVideoEncoder
    from tests.golden.qformer_cases import QF_CASES, chunk_uniforms, qf_inputs
    case = replace(next(c for c in QF_CASES if c.name == "qf_small"), chunk_T=[8] * 6)
    frames, weights = qf_inputs(case)
    Cn, Q, Ln = len(case.chunk_T), case.n_query, case.n_layers
    k = torch.from_numpy(np.stack(frames)).to(dev)
    u = torch.from_numpy(np.stack([chunk_uniforms(case, c) for c in range(Cn)]))

    def model():
        m = InfVideoEncoder(num_video_query_token=Q, hidden_size=case.hidden, llama_hidden=case.proj_out, sticky=case.sticky,
                            num_basis=case.N, tau=case.tau, alpha=case.alpha, num_hidden_layers=Ln)
        m.load_reference_state_dict(weights)
        return m.to(dev)

    plain, traced, loop = model(), model(), model()
    out0 = plain.encode_frames_batch(k, new_video=True, u=u, want_hidden=True)
    traces = [m._get_engine(dev, Q).set_mass_trace(Cn) for m in traced.video_Qformer.ltm_modules]
    out1 = traced.encode_frames_batch(k, new_video=True, u=u, want_hidden=True)
    torch.cuda.synchronize()
    for a, b in zip(out0, out1):
        assert torch.equal(a, b)
    worst = 0.0
    for c in range(Cn):
        loop.encode_frames(k[c:c + 1], new_video=(c == 0), u=u[c])
        for l, m in enumerate(loop.video_Qformer.ltm_modules):
            eng = m._get_engine(dev, Q)
            tol = 2 * delta(eng.last_scores(0, Q)) + EPS
            err = rel_err(traces[l][c, 0].cpu().numpy(), eng.masses(0, Q).cpu().numpy())
            assert err <= tol, f"chunk {c} layer {l}: {err:.3e} > {tol:.3e}"
            worst = max(worst, err)
    record_parity(f"[density] trace through infv_vqf_encode_video, {Cn} chunks x {Ln} layers: max relative {worst:.2e} vs the per-chunk loop")
