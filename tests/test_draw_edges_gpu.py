"""The Gibbs draw at the edges of its cdf, on every draw path of the library (tests/golden/draw_edge_cases.py).

The library holds six implementations of one contract (csrc/ltm_device.h above ``DrawRegs``): the draw plane of
``step_project_kernel`` (1), ``draw_kernel`` (2), ``draw_videos_kernel`` (3), ``chain_kernel`` (4), ``chain_batch_kernel`` (5) and
``chain_batch3_kernel`` (6, its own scan and an fp32 search against ``round_up_f32(u)``).  With teacher-forced probabilities
(``set_probs``) the contract is exact, and every implementation honours the forcing on the first step of a call: the probabilities
read back equal the forced vector bit for bit, the bins equal ``oracle.ltm_oracle.inverse_cdf_draw`` and the resampled rows are
``plan.bin_box[bins]``.  The uniforms sit just below, at and just above every distinct value of the oracle's fp32 cdf.  Beyond a
call's first step the kernels' own probabilities are traced, and the draw from them is held to the same contract.

Every comparison is ``assert_array_equal``.  Needs a real MI355X: run with ``-m gpu``.  One ``record_parity`` line per
implementation: draws compared, and how many of them were edge values (profiles/draw_edges_gpu_parity.txt is a run's copy).
"""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle.ltm_oracle import inverse_cdf_draw
from tests.conftest import record_parity
from tests.golden import draw_edge_cases as dc
from tests.golden import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _engine(pt, dev, **kw):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(pt.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=True, n_layers=pt.L, max_q=pt.Q, device=dev,
                     nb_samples=pt.S, max_batch_chunks=pt.max_batch_chunks, **kw)


class _Inputs:
    """Tokens of every chunk [T*P, d], the shared query [L, Q, dm], projections and seeded uniforms [chunks, L, S] of a point."""

    def __init__(self, pt, dev):
        ks, qs, ws, u = sc.point_inputs(pt)
        self.k = [torch.from_numpy(k).to(dev) for k in ks]
        self.q = torch.from_numpy(qs).to(dev)
        self.projs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w) for w in ws]
        self.u = u


def _schedule(L, S):
    """Rounds of teacher forcing that cycle through every regime, a different one per layer; a shape with fewer samples than edge
    values takes them piece by piece.  Yields (label, regime names [L], uniforms [L, S])."""
    for r in range(dc.n_rounds(L)):
        names = dc.layer_regimes(r, L)
        pieces = [dc.n_pieces(dc.REGIMES[n], S) for n in names]
        for piece in range(max(pieces)):
            u = np.stack([dc.edge_uniforms(dc.REGIMES[n], S, piece % m) for n, m in zip(names, pieces)])
            yield f"round {r} piece {piece}", names, u


class _Tally:
    def __init__(self):
        self.draws = self.edges = 0

    def line(self, what):
        record_parity(f"[draw edges] {what}: {self.draws} draws compared with inverse_cdf_draw, all equal; {self.edges} of them at edge values")


def _compare(label, names, u, draws, bin_box, tally):
    """draws: per layer (bins, idx, probs) as the library reports them."""
    for l, (name, (bins, idx, probs)) in enumerate(zip(names, draws)):
        p = dc.REGIMES[name] if isinstance(name, str) else name
        tag = f"{label}, layer {l}" + (f" ({name})" if isinstance(name, str) else "")
        np.testing.assert_array_equal(np.asarray(probs)[:dc.NB], p, err_msg=f"{tag}: probabilities fed to the draw")
        expect = inverse_cdf_draw(p, u[l])
        np.testing.assert_array_equal(bins, expect, err_msg=f"{tag}: bins")
        if idx is not None:
            np.testing.assert_array_equal(idx, bin_box[expect], err_msg=f"{tag}: resampled rows")
        tally.draws += int(u[l].size)
        tally.edges += dc.count_edges(p, u[l])


def _forced_rounds(eng, L, S, step, label, tally, bin_box):
    """set_probs(l, regime) per layer, one continuation step with the regimes' edge uniforms, read back, compare."""
    for what, names, u in _schedule(L, S):
        for l, name in enumerate(names):
            eng.set_probs(l, dc.REGIMES[name])
        step(torch.from_numpy(u).to(eng.device))
        _compare(f"{label}, {what}", names, u, [eng.last_draw(l) for l in range(L)], bin_box, tally)


def _families(eng):
    return {k: v[0] for k, v in eng.profile_read().items()}


# ---------------------------------------------------------------------------------------------------------------------
# a. teacher-forced edges, per implementation
# ---------------------------------------------------------------------------------------------------------------------
def test_forced_edges_step_project_kernel(dev):
    """Implementation 1: the draw plane of step_project_kernel (``forward`` on a sparse plan; no separate draw launch)."""
    pt = dc.PER_CALL
    inp, eng, tally = _Inputs(pt, dev), _engine(pt, dev), _Tally()
    plan = eng.ensure_plan(pt.T)
    assert not plan.dense
    eng.forward(inp.k[0], inp.q, inp.projs, None, new_doc=True)
    eng.profile(True)
    _forced_rounds(eng, pt.L, pt.S, lambda u: eng.forward(inp.k[1], inp.q, inp.projs, u, new_doc=False), "forward", tally, plan.bin_box)
    fam = _families(eng)
    assert fam["project"] > 0 and fam["draw"] == 0 and fam["chain"] == 0, f"forward ran {fam}"
    tally.line("1 step_project_kernel (forward)")


def test_forced_edges_draw_kernel_sparse_plan(dev):
    """Implementation 2 on a sparse plan: ``consolidate_q`` continues a memory through chain_step, whose draw is draw_kernel
    (asserted: a DRAW launch) -- also for a call of ONE chunk, which is what each round takes: the forcing reaches a call's first
    step, the per-chunk stages keep no trace, and a second chunk's draw would replace the forced one in ``last_draw``."""
    pt = dc.PER_CALL
    inp, eng, tally = _Inputs(pt, dev), _engine(pt, dev), _Tally()
    plan = eng.ensure_plan(pt.T)
    q4 = inp.q[None].contiguous()
    eng.consolidate_q(inp.k[0][None], q4, inp.projs, None, new_doc=True)
    eng.profile(True)
    _forced_rounds(eng, pt.L, pt.S, lambda u: eng.consolidate_q(inp.k[1][None], q4, inp.projs, u[None], new_doc=False),
                   "consolidate_q", tally, plan.bin_box)
    fam = _families(eng)
    assert fam["draw"] > 0 and fam["chain"] == 0, f"consolidate_q ran {fam}"
    tally.line("2 draw_kernel (consolidate_q, sparse plan)")


@pytest.mark.parametrize("family", ["dense", "psi"])
def test_forced_edges_draw_kernel_dense_and_psi_steps(dev, family):
    """Implementation 2 behind the dense step (a num_basis whose fp32 boxes overlap) and the general-psi step (Gaussian family)."""
    if family == "dense":
        pt = replace(dc.PER_CALL, name="dense", N=dc.DENSE_N, T=dc.DENSE_T)
        eng = _engine(pt, dev)
    else:
        pt = replace(dc.PER_CALL, name="psi", N=dc.GAUSS_N, T=dc.GAUSS_T)
        eng = _engine(pt, dev, gaussian_sigmas=dc.GAUSS_SIGMAS)
    plan = eng.ensure_plan(pt.T)
    assert plan.dense and bool(plan.psi) == (family == "psi")
    inp, tally = _Inputs(pt, dev), _Tally()
    eng.forward(inp.k[0], inp.q, inp.projs, None, new_doc=True)
    eng.profile(True)
    _forced_rounds(eng, pt.L, pt.S, lambda u: eng.forward(inp.k[1], inp.q, inp.projs, u, new_doc=False), f"{family} forward", tally,
                   plan.bin_box)
    assert _families(eng)["draw"] > 0
    tally.line(f"2 draw_kernel ({family} step)")


def run_forced_fast(pt, dev):
    """A first chunk, then one-chunk ``consolidate(new_doc=False)`` calls under teacher forcing: what every round's draw reports.
    (Also the body of the child processes of test_role_s_kernels_agree_on_one_shape.)"""
    inp, eng = _Inputs(pt, dev), _engine(pt, dev)
    eng.ensure_plan(pt.T)
    eng.consolidate(inp.k[0][None], inp.q, inp.projs, None, new_doc=True)
    eng.sync()
    eng.profile(True)
    out = {}
    for i, (what, names, u) in enumerate(_schedule(pt.L, pt.S)):
        for l, name in enumerate(names):
            eng.set_probs(l, dc.REGIMES[name])
        eng.consolidate(inp.k[1][None], inp.q, inp.projs, torch.from_numpy(u[None]).to(dev), new_doc=False)
        eng.sync()
        for l in range(pt.L):
            out[f"bins_{i}_{l}"], out[f"idx_{i}_{l}"], out[f"probs_{i}_{l}"] = eng.last_draw(l)
    fam = _families(eng)
    out["families"] = np.array([fam["chain"], fam["uc"], fam["update"], fam["attend"], fam["draw"]])
    # what tells the role-S kernels apart from outside: the launches of ONE three-chunk continuation call (CHAIN launches by the
    # profile, every kernel launch by the library's own counter)
    before = int(eng.lib.infv_ltm_launch_count())
    eng.consolidate(torch.stack([inp.k[1]] * 3), inp.q, inp.projs, torch.from_numpy(np.stack([inp.u[1]] * 3)).to(dev), new_doc=False)
    eng.sync()
    out["launches_3"] = np.array([_families(eng)["chain"], int(eng.lib.infv_ltm_launch_count()) - before])
    return out


def _check_forced_fast(pt, got, label, tally):
    from infinite_video_amd import basis_maps
    bin_box = basis_maps.build_plan(pt.T, pt.N, pt.tau, pt.S).bin_box
    chain, uc, update, attend, draw = (int(x) for x in got["families"])
    assert chain > 0 and uc > 0 and update == 0 and attend == 0 and draw == 0, f"{label}: expected the fused chain, ran {got['families']}"
    for i, (what, names, u) in enumerate(_schedule(pt.L, pt.S)):
        _compare(f"{label}, {what}", names, u, [(got[f"bins_{i}_{l}"], got[f"idx_{i}_{l}"], got[f"probs_{i}_{l}"]) for l in range(pt.L)],
                 bin_box, tally)


@pytest.mark.parametrize("kernel", list(dc.ROLE_S))
def test_forced_edges_role_s_kernels(dev, kernel):
    """Implementations 4-6: step 0 of the role-S launch of a one-chunk ``consolidate(new_doc=False)`` on the shape that selects
    each kernel (tests/test_draw_edges_cpu.py asserts the selection through ``expected_path``)."""
    pt = dc.ROLE_S[kernel]
    tally = _Tally()
    _check_forced_fast(pt, run_forced_fast(pt, dev), f"{kernel} ({pt.name})", tally)
    tally.line(f"{ {'chain_kernel': 4, 'chain_batch': 5, 'chain_batch3': 6}[kernel] } {kernel} ({pt.name}, consolidate)")


@pytest.mark.parametrize("kernel", list(dc.ROLE_S_SHORT))
def test_forced_edges_role_s_kernels_with_fewer_samples_than_edges(dev, kernel):
    """The persistent kernels at S = 100 / 102: the edge values in pieces, S off the thread stride, a ragged last vector of uniforms."""
    pt = dc.ROLE_S_SHORT[kernel]
    tally = _Tally()
    _check_forced_fast(pt, run_forced_fast(pt, dev), f"{kernel} ({pt.name})", tally)
    tally.line(f"{ {'chain_batch': 5, 'chain_batch3': 6}[kernel] } {kernel} ({pt.name}, consolidate, edge values in pieces)")


# ---------------------------------------------------------------------------------------------------------------------
# b. lockstep
# ---------------------------------------------------------------------------------------------------------------------
def test_forced_edges_lockstep_calls(dev):
    """Implementation 3: ``consolidate_videos`` and ``steps_videos`` with ``new_doc=False`` on four engines, each with its own forced
    regime per layer, one chunk per video.  Engine 2 gets ZERO chunks in the first call: its forcing is one-shot for its next
    *step* (include/infv_ltm.h), so it is still pending, and honoured, in its next call."""
    from infinite_video_amd.engine import consolidate_videos, steps_videos
    pt = dc.PER_CALL
    inp, tally = _Inputs(pt, dev), _Tally()
    V, idle = 4, 2
    engs = [_engine(pt, dev) for _ in range(V)]
    plan = engs[0].ensure_plan(pt.T)
    assert sc.videos_supported(pt, sc._ps(pt))
    consolidate_videos(engs, torch.stack([inp.k[0]] * V), [1] * V, inp.q, inp.projs, None, new_doc=True)
    n = len(dc.REGIME_NAMES)
    names = {v: [dc.REGIME_NAMES[(v * pt.L + l) % n] for l in range(pt.L)] for v in range(V)}

    forced = set()

    def force(vs):
        for v in vs:
            forced.update(names[v])
            for l, name in enumerate(names[v]):
                engs[v].set_probs(l, dc.REGIMES[name])

    def uniforms(vs):
        return {v: np.stack([dc.edge_uniforms(dc.REGIMES[name], pt.S) for name in names[v]]) for v in vs}

    def check(vs, u, label):
        for v in vs:
            _compare(f"{label}, video {v}", names[v], u[v], [engs[v].last_draw(l) for l in range(pt.L)], plan.bin_box, tally)

    # call 1: consolidate_videos, engine `idle` has no chunk
    force(range(V))
    running = [v for v in range(V) if v != idle]
    u1 = uniforms(running)
    engs[0].profile(True)
    consolidate_videos(engs, torch.stack([inp.k[1]] * len(running)), [0 if v == idle else 1 for v in range(V)], inp.q, inp.projs,
                       torch.from_numpy(np.stack([u1[v] for v in running])).to(dev), new_doc=False)
    fam = _families(engs[0])
    assert fam["draw"] > 0 and fam["chain"] == 0, f"consolidate_videos ran {fam}"
    check(running, u1, "consolidate_videos")
    # call 2: steps_videos on all four; the running engines get new regimes, the idle one still holds the forcing of call 1
    for v in running:
        names[v] = [dc.REGIME_NAMES[(V * pt.L + v * pt.L + l) % n] for l in range(pt.L)]
    force(running)
    u2 = uniforms(range(V))
    kbar = engs[0].pool(torch.stack([inp.k[1]] * V))
    steps_videos(engs, kbar, [1] * V, inp.q, inp.projs, torch.from_numpy(np.stack([u2[v] for v in range(V)])).to(dev), new_doc=False)
    check(range(V), u2, "steps_videos")
    assert forced == set(dc.REGIME_NAMES)
    tally.line("3 draw_videos_kernel (consolidate_videos, steps_videos)")


# ---------------------------------------------------------------------------------------------------------------------
# c. the three role-S kernels on one shape
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
import numpy as np, torch
from tests.golden import draw_edge_cases as dc
from tests.test_draw_edges_gpu import run_forced_fast
np.savez(sys.argv[1], **run_forced_fast(dc.ROLE_S["chain_batch3"], torch.device("cuda:0")))
"""
_VARIANTS = {"chain_batch3": {}, "chain_batch": {"INFV_CHAIN_V1": "1"}, "chain_kernel": {"INFV_PERSISTENT": "0"}}


@pytest.mark.parametrize("kernel", list(_VARIANTS))
def test_role_s_kernels_agree_on_one_shape(dev, tmp_path, kernel):
    """The experiments build selects each role-S kernel on the SAME shape (the default, INFV_CHAIN_V1=1, INFV_PERSISTENT=0): the same
    forced regimes and edge uniforms must give the oracle's bins under all three -- and so identical bins.  That the knob took is
    seen in the launches of a three-chunk continuation call, against the same call on the shipped library in this process (whose
    role S is chain_batch3_kernel): one CHAIN launch and the same launches in all for chain_batch3; one CHAIN launch and one launch
    fewer for chain_batch_kernel (it compares in float64: no round_up_uniforms_kernel in front of the chain; alpha_rows_kernel stands
    where alpha_rows2_kernel stood); one CHAIN launch per chunk for chain_kernel."""
    pt = dc.ROLE_S["chain_batch3"]
    path = str(tmp_path / f"{kernel}.npz")
    env = dict(os.environ, INFV_LTM_LIBRARY="exp", **_VARIANTS[kernel])
    for name in ("INFV_CHAIN_V1", "INFV_PERSISTENT"):
        if name not in _VARIANTS[kernel]:
            env.pop(name, None)
    subprocess.run([sys.executable, "-c", _CHILD, path], check=True, env=env, cwd=ROOT, timeout=120)
    got = np.load(path)
    tally = _Tally()
    _check_forced_fast(pt, got, f"{kernel} on {pt.name} (experiments build)", tally)
    ref_chain, ref_all = (int(x) for x in run_forced_fast(pt, dev)["launches_3"])
    chain, all_ = (int(x) for x in got["launches_3"])
    assert ref_chain == 1, f"the shipped library ran {ref_chain} role-S launches for three chunks: not the persistent kernel"
    want = {"chain_batch3": (1, ref_all), "chain_batch": (1, ref_all - 1), "chain_kernel": (3, None)}[kernel]
    assert chain == want[0], f"{kernel}: {chain} role-S launches for three chunks, expected {want[0]}"
    if want[1] is not None:
        assert all_ == want[1], f"{kernel}: {all_} kernel launches for the call, expected {want[1]} ({ref_all} on the shipped library)"
    tally.line(f"{kernel} selected on {pt.name} in the experiments build ({chain} role-S launches, {all_} launches for 3 chunks; shipped: {ref_chain}, {ref_all})")


# ---------------------------------------------------------------------------------------------------------------------
# d. the kernels' own probabilities, beyond step 0
# ---------------------------------------------------------------------------------------------------------------------
def _traced_consolidate(pt, inp, u, dev, cuts):
    """A fresh engine over the point's chunks, one ``consolidate`` call per cut (the first starts the document), every call traced:
    (probs [chunks, L, 127], bins [chunks, L, S]); rows of chunk 0, which draws nothing, stay 0 / -1."""
    eng = _engine(pt, dev)
    probs = np.zeros((pt.chunks, pt.L, dc.NB), np.float32)
    bins = np.full((pt.chunks, pt.L, pt.S), -1, np.int64)
    for c0, c1 in cuts:
        tr = eng.set_trace(c1 - c0)
        eng.consolidate(torch.stack(inp.k[c0:c1]), inp.q, inp.projs, torch.from_numpy(u[c0:c1]).to(dev), new_doc=(c0 == 0))
        eng.sync()
        bins[c0:c1] = tr[0].cpu().numpy()
        probs[c0:c1] = tr[1].cpu().numpy()[:, :, :dc.NB]
        eng.set_trace(0)
        for l in range(pt.L):                                    # the call's last draw as get_draw reports it == its trace row
            if c1 - 1 > 0:
                b, _, p = eng.last_draw(l)
                np.testing.assert_array_equal(b, bins[c1 - 1, l])
                np.testing.assert_array_equal(p, probs[c1 - 1, l])
    return probs, bins


def _edge_last_chunk(pt, u, probs):
    u2 = u.copy()
    for l in range(pt.L):
        u2[-1, l] = dc.edge_uniforms(probs[-1, l], pt.S)
    return u2


def _check_two_passes(pt, label, u, u2, pass1, pass2, tally):
    probs1, bins1 = pass1
    probs2, bins2 = pass2
    # 1. same inputs up to the last chunk's uniforms: the probabilities of EVERY chunk are the same bits -- this is what makes the
    #    uniforms of pass 2 edge values of the cdf the kernel really searches (a failure here is a finding about determinism)
    np.testing.assert_array_equal(probs2, probs1, err_msg=f"{label}: traced probabilities differ between two runs of the same inputs")
    np.testing.assert_array_equal(bins2[:-1], bins1[:-1], err_msg=f"{label}: draws of the unchanged chunks differ between the two runs")
    assert (probs2[1:] > 0).any(axis=-1).all() and (bins2[1:] >= 0).all(), f"{label}: a chunk was left untraced"
    # 2. the last chunk's draw at the edges of its own cdf (and every earlier chunk's draw from its traced probabilities)
    for c in range(pt.chunks - 1, 0, -1):
        names = [probs2[c, l] for l in range(pt.L)]
        before = tally.edges
        _compare(f"{label}, chunk {c}", names, u2[c], [(bins2[c, l], None, probs2[c, l]) for l in range(pt.L)], None, tally)
        if c == pt.chunks - 1:
            assert tally.edges - before >= pt.L * 300, f"{label}: the last chunk's uniforms are not edge values of its cdf"


@pytest.mark.parametrize("kernel", list(dc.ROLE_S))
def test_own_probabilities_beyond_step_0_of_the_role_s_launch(dev, kernel):
    """A 5-chunk ``consolidate`` (first chunk + a 4-step launch): step 3 of the launch reads its uniforms from the other half of the
    double buffer and its masses from the fixed-point ring.  Pass 1 traces the probabilities; pass 2 repeats the call with the last
    chunk's uniforms replaced by the edge values of the traced cdf."""
    pt = replace(dc.ROLE_S[kernel], n_chunks=5)
    inp = _Inputs(pt, dev)
    cuts = [(0, 5)]
    pass1 = _traced_consolidate(pt, inp, inp.u, dev, cuts)
    u2 = _edge_last_chunk(pt, inp.u, pass1[0])
    pass2 = _traced_consolidate(pt, inp, u2, dev, cuts)
    tally = _Tally()
    _check_two_passes(pt, f"{kernel} ({pt.name}), 5-chunk call", inp.u, u2, pass1, pass2, tally)
    tally.line(f"{kernel} ({pt.name}) steps 0-3 of one launch, own probabilities")


def test_own_probabilities_at_step_0_of_a_launch_that_reads_float_partials(dev):
    """The same chunks with the call cut 4 + 1: the edge chunk is step 0 of a launch that takes its masses from the float partial row
    the previous call left (``first_from_parts``)."""
    pt = replace(dc.ROLE_S["chain_batch3"], n_chunks=5)
    inp = _Inputs(pt, dev)
    cuts = [(0, 4), (4, 5)]
    pass1 = _traced_consolidate(pt, inp, inp.u, dev, cuts)
    u2 = _edge_last_chunk(pt, inp.u, pass1[0])
    pass2 = _traced_consolidate(pt, inp, u2, dev, cuts)
    tally = _Tally()
    _check_two_passes(pt, f"chain_batch3 ({pt.name}), call cut 4 + 1", inp.u, u2, pass1, pass2, tally)
    tally.line(f"chain_batch3 ({pt.name}) step 0 from float partials, own probabilities")


def test_own_probabilities_on_the_per_call_path(dev):
    """Three ``forward`` steps behind the first chunk, read back with ``last_draw``; the third at the edges of its own cdf."""
    pt = replace(dc.PER_CALL, n_chunks=4)
    inp = _Inputs(pt, dev)

    def run(u):
        eng = _engine(pt, dev)
        probs = np.zeros((pt.chunks, pt.L, dc.NB), np.float32)
        bins = np.full((pt.chunks, pt.L, pt.S), -1, np.int64)
        for c in range(pt.chunks):
            eng.forward(inp.k[c], inp.q, inp.projs, torch.from_numpy(u[c]).to(dev) if c else None, new_doc=(c == 0))
            for l in range(pt.L if c else 0):
                bins[c, l], _, probs[c, l] = eng.last_draw(l)
        return probs, bins

    pass1 = run(inp.u)
    u2 = _edge_last_chunk(pt, inp.u, pass1[0])
    pass2 = run(u2)
    tally = _Tally()
    _check_two_passes(pt, "forward chain", inp.u, u2, pass1, pass2, tally)
    tally.line("1 step_project_kernel (forward) steps 1-3, own probabilities")


def test_own_probabilities_of_a_later_chunk_of_one_consolidate_q_call(dev):
    """draw_kernel behind the first step of a call: ``consolidate_q`` over four chunks runs chunks 1-3 as ONE sub-batch of
    ``infv_ltm_steps`` (one projection launch, then chain_step per chunk).  That path keeps no trace, so only the last chunk's draw
    can be read back: its probabilities must be the same bits in both passes, and its bins the oracle's at the edges of its cdf."""
    pt = replace(dc.PER_CALL, n_chunks=4)
    inp = _Inputs(pt, dev)
    k, q4 = torch.stack(inp.k), torch.stack([inp.q] * pt.chunks)

    def run(u):
        eng = _engine(pt, dev)
        eng.profile(True)
        eng.consolidate_q(k, q4, inp.projs, torch.from_numpy(u).to(dev), new_doc=True)
        fam = _families(eng)
        assert fam["draw"] == pt.chunks - 1 and fam["chain"] == 0, f"consolidate_q ran {fam}"
        return [eng.last_draw(l) for l in range(pt.L)]

    first = run(inp.u)
    u2 = inp.u.copy()
    for l in range(pt.L):
        u2[-1, l] = dc.edge_uniforms(first[l][2], pt.S)
    second = run(u2)
    tally = _Tally()
    for l in range(pt.L):
        np.testing.assert_array_equal(second[l][2], first[l][2], err_msg=f"layer {l}: probabilities of the last chunk differ between two runs")
    from infinite_video_amd import basis_maps
    _compare("consolidate_q, chunk 3 of 4", [first[l][2] for l in range(pt.L)], u2[-1], second,
             basis_maps.build_plan(pt.T, pt.N, pt.tau, pt.S).bin_box, tally)
    assert tally.edges >= pt.L * 300
    tally.line("2 draw_kernel (consolidate_q, third step of one sub-batch), own probabilities")
