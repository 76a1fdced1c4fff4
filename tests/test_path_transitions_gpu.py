"""One memory carried across every pair of LTM entry points (tests/golden/transition_cases.py): operation X starts two
documents, an optional hand-off moves the memories to fresh engines, operation Y continues them and a closing ``forward``
consumes what Y left.  After every leg every chunk's ctx (1e-4), ``export_state`` B (2e-5), the probabilities of every draw
that can be read back (2e-5) and its bins (equal: tests/test_path_transitions_cpu.py asserts the margins) are held to
``ClosedFormOracle``; ``rng_position`` must equal the chunk count.  Draws come from ``set_trace`` where the path keeps one (fused
chain, lockstep step) and from ``last_draw`` otherwise (``forward`` per chunk; the last chunk of ``consolidate_q`` and of a
``consolidate`` that runs per-chunk stages -- their earlier draws are held through B and ctx, which a wrong draw moves by far
more than the tolerance).  On top: ``new_doc`` resets whatever X left, the documented bit-for-bit relations hold across the
seam, ``export_chain_state`` refuses where it must and changes nothing, and the device rng continues one stream through every
pair.  Dense plans are held to the reference's goldens.  A second section does the same one level up, through the three entry
points of the video Q-former.  Needs a real MI355X: run with ``-m gpu``.

The per-shape figures are kept by ``record_parity`` (profiles/path_transitions_gpu_parity.txt is a run's copy)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from infinite_video_amd import philox, synth
from tests.conftest import record_parity
from tests.golden import cases as gc
from tests.golden import seam_cases
from tests.golden import sweep_cases as sw
from tests.golden import transition_cases as tc
from tests.golden.seam_cases import MARGIN
from tests.test_call_seams_gpu import B_TOL as VQF_B_TOL
from tests.test_ltm_gpu import B_TOL, CTX_TOL, _golden_B_check

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SCORES_TOL = dict(rtol=1e-4, atol=2e-5)      # test_long_video_many_subbatches_matches_oracle's bound on last_scores
INFV_ERR_STATE = -4
RNG_SEED = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------ engines and inputs
def _engine(pt):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(pt.N, pt.H, pt.dh, pt.d, pt.P, tau=pt.tau, sticky=pt.sticky, n_layers=pt.L, max_q=32, device=DEV,
                     nb_samples=pt.S, max_batch_chunks=pt.max_batch_chunks)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _tok(pt, doc, c):
    return _cached(("k", pt.name, doc, c), lambda: torch.from_numpy(tc.tokens(pt, doc, c)).to(DEV))


def _q(pt, spec, doc, c):
    key = ("q", pt.name, spec) + ((doc, c) if spec[0] == "chunk" else ())
    return _cached(key, lambda: torch.from_numpy(tc.query(pt, spec, doc, c)).to(DEV))


def _projs(pt, wset):
    return _cached(("w", pt.name, wset), lambda: [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in w)
                                                  for w in tc.weights(pt, wset)])


def _oracle_uniforms(pt, run):
    """[chunks, L, S] float64 on the device (row 0: the first chunk draws nothing), or None when nothing is drawn."""
    if not pt.sticky:
        return None
    u = np.zeros((len(run.u), pt.L, pt.S))
    for c, uc in enumerate(run.u):
        if uc is not None:
            u[c] = uc
    return torch.from_numpy(u).to(DEV)


def _plain_uniforms(pt, doc):
    if not pt.sticky:
        return None
    return torch.from_numpy(synth.gibbs_uniforms(sum(tc.DOC_LEGS[doc]), pt.L, seed=synth.SEED_U + 11 + doc, nb_samples=pt.S)).to(DEV)


def _bystander(pt, rng=False):
    """The third engine of a continuing lockstep call: an unrelated memory, zero chunks in the call."""
    e = _engine(pt)
    if rng:
        e.set_device_rng(RNG_SEED, 77)
    u = tc.bystander_uniforms(pt)
    for c in range(tc.BYSTANDER_CHUNKS):
        uc = torch.from_numpy(u[c]).to(DEV) if (c and pt.sticky) else None
        e.forward(_tok(pt, tc.BYSTANDER_DOC, c), _q(pt, ("shared", pt.Q, 0), 0, 0), _projs(pt, 0), uc, new_doc=(c == 0))
    return e


def _state(e, pt):
    """Everything a handle shows of its memory, as host arrays (compared bit for bit)."""
    out = [np.int64(e.rng_position)]
    for l in range(pt.L):
        B, mass = e.export_state(l)
        out += [B.cpu().numpy(), mass.cpu().numpy()]
        if pt.sticky:
            out += list(e.last_draw(l))
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ one leg through one operation
class _Out:
    def __init__(self, pt, n, Q):
        self.ctx = np.zeros((n, pt.L, Q, pt.dm), np.float32)
        self.bins = np.full((n, pt.L, pt.S), -1, np.int64)            # -1: this draw cannot be read back
        self.probs = np.zeros((n, pt.L, 127), np.float32)

    def arrays(self):
        return [self.ctx, self.bins, self.probs]


def _last_draw_into(e, pt, leg, out):
    n = len(leg.chunks)
    if pt.sticky and (n > 1 or not leg.new_doc) and out.bins[n - 1, 0, 0] < 0:
        for l in range(pt.L):
            out.bins[n - 1, l], _, out.probs[n - 1, l] = e.last_draw(l)


def _run_leg(pt, op, engs, legs, us, by=None):
    """Advance every document's engine by its leg through ``op`` (``vid_s``: steps_videos with the shared query, the twin of
    ``vid``).  us: per document [chunks, L, S] on the device, or None (nothing drawn, or the device rng draws)."""
    from infinite_video_amd.engine import consolidate_videos, steps_videos
    outs = [_Out(pt, len(leg.chunks), leg.q[0][1]) for leg in legs]
    rows = [None if u is None else u[leg.chunks[0]:leg.chunks[-1] + 1].contiguous() for u, leg in zip(us, legs)]
    projs = _projs(pt, legs[0].w)
    toks = [[_tok(pt, d, c) for c in leg.chunks] for d, leg in enumerate(legs)]
    qs = [[_q(pt, spec, d, c) for spec, c in zip(leg.q, leg.chunks)] for d, leg in enumerate(legs)]
    if op in ("vid", "vid_q", "vid_s"):
        engines = list(engs) + ([by] if by is not None else [])
        counts = [len(leg.chunks) for leg in legs] + ([0] if by is not None else [])
        k = torch.stack([t for d in toks for t in d])
        u = None if rows[0] is None else torch.cat(rows)
        traces = [e.set_trace(len(leg.chunks)) if pt.sticky else None for e, leg in zip(engs, legs)]
        if op == "vid":
            y = consolidate_videos(engines, k, counts, qs[0][0], projs, u, new_doc=legs[0].new_doc)
        else:
            kbar = engs[0].pool(k)
            q = qs[0][0] if op == "vid_s" else torch.stack([x for d in qs for x in d])
            y = steps_videos(engines, kbar, counts, q, projs, u, new_doc=legs[0].new_doc)
        lo = 0
        for e, leg, out, tr in zip(engs, legs, outs, traces):
            e.sync()
            out.ctx[:] = y[lo:lo + len(leg.chunks)].cpu().numpy()
            lo += len(leg.chunks)
            if tr is not None:
                out.bins[:], out.probs[:] = tr[0].cpu().numpy(), tr[1].cpu().numpy()[:, :, :127]
                e.set_trace(0)
        return outs
    for d, (e, leg, out) in enumerate(zip(engs, legs, outs)):
        n = len(leg.chunks)
        if op == "fwd":
            for i, c in enumerate(leg.chunks):
                first = leg.new_doc and i == 0
                out.ctx[i] = e.forward(toks[d][i], qs[d][i], projs, None if (first or us[d] is None) else us[d][c], new_doc=first).cpu().numpy()
                if pt.sticky and not first:
                    for l in range(pt.L):
                        out.bins[i, l], _, out.probs[i, l] = e.last_draw(l)
            continue
        k = torch.stack(toks[d])
        if op in ("cons", "pooled"):
            tr = e.set_trace(n) if pt.sticky else None
            if op == "cons":
                y = e.consolidate(k, qs[d][0], projs, rows[d], new_doc=leg.new_doc)
            else:
                y = e.consolidate_pooled(e.pool(k), qs[d][0], projs, rows[d], new_doc=leg.new_doc)
            e.sync()
            if tr is not None:
                out.bins[:], out.probs[:] = tr[0].cpu().numpy(), tr[1].cpu().numpy()[:, :, :127]
                e.set_trace(0)
        elif op == "cons_q":
            y = e.consolidate_q(k, torch.stack(qs[d]), projs, rows[d], new_doc=leg.new_doc)
        else:
            raise KeyError(op)
        out.ctx[:] = y.cpu().numpy()
        _last_draw_into(e, pt, leg, out)
    return outs


def _on_fused_chain(pt, Q):
    p = replace(pt, Q=Q)
    return sw.fast_path(p, sw._ps(p))


def _hand_over(pt, how, e, Q, wset, rng=None):
    """The memory of ``e`` in a fresh engine; the receiver takes the sender's rng position."""
    e2 = _engine(pt)
    if rng is not None:
        e2.set_device_rng(*rng)
    if how == "state":
        for l in range(pt.L):
            B, mass = e.export_state(l)
            e2.import_state(l, B.contiguous(), mass.contiguous() if pt.sticky else None, _projs(pt, wset)[l])
    else:
        e2.import_chain_state(Q, e.export_chain_state(Q))
    e2.rng_position = e.rng_position
    return e2


# ------------------------------------------------------------------------------------------------ oracle parity
class _Stats:
    def __init__(self):
        self.ctx = self.B = self.p = self.sc = 0.0
        self.draws = self.unread = self.sequences = 0


_STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _evidence():
    yield
    for shape, st in _STATS.items():
        record_parity(f"[path transitions] {shape}: {st.sequences} sequences, worst |ctx - oracle| {st.ctx:.2e}, |B - oracle| {st.B:.2e}, "
                      f"|probs - oracle| {st.p:.2e}, |scores - oracle| {st.sc:.2e}; {st.draws} draws compared, all equal "
                      f"({st.unread} more held through B and ctx only)")


def _check_leg(tag, pt, run, leg, out, e, st):
    n = len(leg.chunks)
    traced = leg.op in ("fwd",) + tc.LOCKSTEP or (leg.op in ("cons", "pooled") and _on_fused_chain(pt, leg.q[0][1]))
    for i, c in enumerate(leg.chunks):
        err = float(np.abs(out.ctx[i] - run.ctx[c]).max())
        st.ctx = max(st.ctx, err)
        assert err <= CTX_TOL, f"{tag}: {leg.op} chunk {c}: |ctx - oracle| = {err:.3e}"
        if not (pt.sticky and c > 0):
            continue
        known = out.bins[i, :, 0] >= 0
        assert known.all() == known.any() == (traced or i == n - 1), f"{tag}: {leg.op} chunk {c}: draws read back {known}"
        if not known.all():
            st.unread += pt.L * pt.S
            continue
        perr = float(np.abs(out.probs[i] - run.probs[c]).max())
        st.p = max(st.p, perr)
        assert perr <= MARGIN, f"{tag}: {leg.op} chunk {c}: |probs - oracle| = {perr:.3e}"
        diff = int((out.bins[i] != run.bins[c]).sum())
        assert diff == 0, f"{tag}: {leg.op} chunk {c}: {diff} of {pt.L * pt.S} drawn bins differ from the oracle's"
        st.draws += pt.L * pt.S
    for l in range(pt.L):
        eB = float(np.abs(e.export_state(l)[0].cpu().numpy() - run.B[leg.chunks[-1]][l]).max())
        st.B = max(st.B, eB)
        assert eB <= B_TOL, f"{tag}: after {leg.op}: |B - oracle| = {eB:.3e} in layer {l}"
    assert e.rng_position == leg.chunks[-1] + 1, f"{tag}: after {leg.op}: rng_position {e.rng_position}"


@pytest.mark.parametrize("name", [s.name for s in tc.SEQUENCES])
def test_sequence_matches_the_oracle(name):
    seq = tc.BY_NAME[name]
    pt = tc.SHAPES[seq.shape]
    st = _STATS.setdefault(seq.shape, _Stats())
    docs = range(len(tc.DOC_LEGS))
    runs = [tc.oracle_run(seq, d) for d in docs]
    us = [_oracle_uniforms(pt, r) for r in runs]
    legs = [tc.legs_of(seq, d) for d in docs]
    engs = [_engine(pt) for _ in docs]
    by = _bystander(pt) if seq.y in tc.LOCKSTEP else None
    by_before = _state(by, pt) if by is not None else None

    def leg(i, by=None):
        now = [l[i] for l in legs]
        outs = _run_leg(pt, now[0].op, engs, now, us, by=by)
        for d in docs:
            _check_leg(f"{name} document {'AB'[d]}", pt, runs[d], now[d], outs[d], engs[d], st)

    leg(0)
    if seq.variant == "weights":
        for e in engs:
            e.reproject(_projs(pt, 1))
    if seq.handoff:
        engs = [_hand_over(pt, seq.handoff, e, legs[0][0].q[0][1], legs[0][0].w) for e in engs]
    leg(1, by)
    leg(2)
    for d in docs:
        for l in range(pt.L):
            got = engs[d].last_scores(l, pt.Q)
            st.sc = max(st.sc, float(np.abs(got - runs[d].scores[l]).max()))
            np.testing.assert_allclose(got, runs[d].scores[l], err_msg=f"{name} document {'AB'[d]}: last scores, layer {l}", **SCORES_TOL)
    if by is not None:
        assert _same(by_before, _state(by, pt)), f"{name}: the engine with zero chunks in the call changed"
    st.sequences += 1


# ------------------------------------------------------------------------------------------------ two device runs, bit for bit
FAST = tc.SHAPES["fast"]


def _play(pt, steps, rng=False, explicit=None, by_in=True):
    """A list of steps -- (operation, leg index) or ("hand", how) or ("fresh",) -- over both documents.  Returns every leg's
    arrays, the final states and the rng position after every leg.  ``rng``: the device rng draws (u = None); ``explicit``: these
    uniforms per document instead of the plain ones.  A leg index of 0 starts the documents anew on the same handles."""
    docs = range(len(tc.DOC_LEGS))
    base = tc.BY_NAME["fast:cons-cons"] if pt is FAST else next(s for s in tc.SEQUENCES if s.shape == pt.name)
    engs = [_engine(pt) for _ in docs]
    if rng:
        for d in docs:
            engs[d].set_device_rng(RNG_SEED, d)
    us = [None if rng else (explicit[d] if explicit is not None else _plain_uniforms(pt, d)) for d in docs]
    got, positions = [], []
    for step in steps:
        if step[0] == "hand":
            Q = pt.Q
            engs = [_hand_over(pt, step[1], e, Q, 0, rng=(RNG_SEED, d) if rng else None) for d, e in enumerate(engs)]
            continue
        op, i = step
        legs = []
        for d in docs:
            if isinstance(i, tuple):                              # several legs of the table as ONE call
                parts = [tc.legs_of(base, d)[j] for j in i]
                chunks, new_doc = tuple(c for x in parts for c in x.chunks), parts[0].new_doc
            else:
                chunks, new_doc = tc.legs_of(base, d)[i].chunks, tc.legs_of(base, d)[i].new_doc
            legs.append(tc.Leg(op, chunks, tc._qspecs(op, chunks, pt.Q, 0), 0, new_doc))
        by = _bystander(pt, rng=rng) if (op in ("vid", "vid_q", "vid_s") and not legs[0].new_doc and by_in) else None
        for o in _run_leg(pt, op, engs, legs, us, by=by):
            got += o.arrays()
        positions.append([e.rng_position for e in engs])
    for e in engs:
        got += _state(e, pt)
    return got, positions, engs


@pytest.mark.parametrize("x", tc.OPS + ("chain_import",))
def test_new_doc_resets_whatever_the_last_operation_left(x):
    """Leg X, then every operation with ``new_doc=True`` on the same handles: bit for bit what fresh engines give (ctx, draws, B,
    masses, rng position).  ``chain_import``: X ends in an ``import_chain_state`` that no call consumed."""
    pt = FAST
    first = [("cons", 0), ("hand", "chain")] if x == "chain_import" else [(x, 0)]
    for y in tc.OPS:
        fresh = _cached(("fresh", y), lambda: _play(pt, [(y, 0), ("fwd", 1)])[0])
        got, _, _ = _play(pt, first + [(y, 0), ("fwd", 1)])
        n_first = 3 * len(tc.DOC_LEGS)                            # leg X's own arrays (a hand-over adds none)
        assert _same(got[n_first:], fresh), f"{x} then {y}(new_doc=True) differs from {y} on fresh engines"


@pytest.mark.parametrize("x", tc.OPS)
def test_documented_bitwise_relations_hold_across_the_seam(x):
    """(X, pooled) == (X, cons) and (X, vid) == (X, steps_videos with the shared query on pooled frames), closing fwd included;
    and no bit of the videos depends on the zero-chunk engine being in the call."""
    pt = FAST
    cons, _, _ = _play(pt, [(x, 0), ("cons", 1), ("fwd", 2)])
    pooled, _, _ = _play(pt, [(x, 0), ("pooled", 1), ("fwd", 2)])
    assert _same(cons, pooled), f"({x}, pooled) differs from ({x}, cons)"
    vid, _, _ = _play(pt, [(x, 0), ("vid", 1), ("fwd", 2)])
    vid_s, _, _ = _play(pt, [(x, 0), ("vid_s", 1), ("fwd", 2)])
    assert _same(vid, vid_s), f"({x}, steps_videos on pooled frames) differs from ({x}, vid)"
    alone, _, _ = _play(pt, [(x, 0), ("vid", 1), ("fwd", 2)], by_in=False)
    assert _same(vid, alone), f"({x}, vid): the videos' bits depend on the third engine"
    vq, _, _ = _play(pt, [(x, 0), ("vid_q", 1), ("fwd", 2)])
    vq_alone, _, _ = _play(pt, [(x, 0), ("vid_q", 1), ("fwd", 2)], by_in=False)
    assert _same(vq, vq_alone), f"({x}, vid_q): the videos' bits depend on the third engine"


@pytest.mark.parametrize("x", tc.CHAIN_EXPORTERS)
def test_chain_state_on_a_fresh_handle_continues_bit_for_bit(x):
    """X -> export_chain_state -> import on a fresh handle -> cons: bit for bit what ONE call over both legs gives (include/infv_ltm.h:
    "as if the exporting handle had gone on itself"; legs of 3 + 3 and 1 + 2 chunks cut the call at a sub-batch boundary, so both
    sides project the same sub-batches).  The exporting handle going on with a SECOND call is not that relation: a continuing call
    cannot know that its query is the last call's and re-derives the scores from K' -- the same values to fp32 rounding, which
    ``fast:cons-cons`` holds to the oracle."""
    pt = FAST
    whole, _, _ = _play(pt, [(x, (0, 1)), ("fwd", 2)])
    moved, _, _ = _play(pt, [(x, 0), ("hand", "chain"), ("cons", 1), ("fwd", 2)])
    nd = len(tc.DOC_LEGS)
    for d in range(nd):
        nx = tc.DOC_LEGS[d][0]
        for j, what in enumerate(("ctx", "bins", "probs")):
            one, first, second = whole[3 * d + j], moved[3 * d + j], moved[3 * nd + 3 * d + j]
            assert np.array_equal(one[:nx], first), f"document {'AB'[d]}: {what} of leg X"
            assert np.array_equal(one[nx:], second), f"document {'AB'[d]}: {what} of the leg behind the hand-off differs from one call's"
    assert _same(whole[3 * nd:], moved[6 * nd:]), "the closing fwd or the final state differs"


# ------------------------------------------------------------------------------------------------ export_chain_state's refusals
def _refused(e, Q):
    from infinite_video_amd._lib import LTMError
    with pytest.raises(LTMError) as err:
        e.export_chain_state(Q)
    assert err.value.code == INFV_ERR_STATE, err.value
    return True


@pytest.mark.parametrize("x", tc.OPS)
def test_export_chain_state_refuses_or_succeeds_by_the_last_operation(x):
    pt = FAST
    _, _, engs = _play(pt, [(x, 0)])
    for e in engs:
        before = _state(e, pt)
        if x in tc.CHAIN_EXPORTERS:
            assert _refused(e, 16)                                # another Q than the last call's
            assert _same(before, _state(e, pt))
            blob = e.export_chain_state(pt.Q)
            assert blob.numel() == e.chain_state_numel(pt.Q)
            nB, nKV = pt.L * pt.N * pt.d, pt.L * pt.N * 2 * pt.dm      # header | B | projected memory | scores | masses
            assert bool(torch.isfinite(blob[16:16 + nB]).all()) and bool(torch.isfinite(blob[16 + nB + nKV:]).all())
            # (the K' half of the projected memory is stale by design after the fused chain: whoever needs it re-projects)
        else:
            assert _refused(e, pt.Q)
        assert _same(before, _state(e, pt)), f"export_chain_state after {x} changed the memory"
    # ... and what the memory does next is what an untouched twin does
    twin, _, _ = _play(pt, [(x, 0), ("fwd", 1)])
    legs = [tc.legs_of(tc.BY_NAME["fast:fwd-fwd"], d)[1] for d in range(len(engs))]
    outs = _run_leg(pt, "fwd", engs, legs, [_plain_uniforms(pt, d) for d in range(len(engs))])
    after = [a for o in outs for a in o.arrays()] + [a for e in engs for a in _state(e, pt)]
    assert _same(after, twin[3 * len(engs):])


def test_export_chain_state_refuses_off_the_fused_chain():
    pt = tc.SHAPES["stages"]
    _, _, engs = _play(pt, [("cons", 0)])
    for e in engs:
        before = _state(e, pt)
        assert _refused(e, pt.Q)
        assert _same(before, _state(e, pt))


def test_import_state_ends_what_the_fused_chain_handed_on():
    """``import_state`` replaces the memory; the fused chain's scores (``Sp``) are then another memory's.  After it
    ``export_chain_state`` refuses, and a chain state imported before it (never consumed) no longer makes the next ``consolidate``
    continue from those scores: the call equals, bit for bit, the same call on a fresh engine given the same ``import_state``.
    (Found by reading ``infv_ltm_import_state`` for this file: it left ``last_fast`` and ``carry_scores`` as they were.)"""
    pt = FAST
    _, _, donors = _play(pt, [("cons", 0)])                       # document A and B after leg X, fused chain
    _, _, (other, _) = _play(pt, [("fwd", 0)])                    # another memory to import: document A after fwd of leg X
    mem = [tuple(x.clone() for x in other.export_state(l)) for l in range(pt.L)]
    leg = tc.Leg("cons", tc.legs_of(tc.BY_NAME["fast:cons-cons"], 0)[1].chunks, tc._qspecs("cons", (3, 4, 5), pt.Q, 0), 0, False)
    us = [_plain_uniforms(pt, 0)]

    def receive(e):
        for l in range(pt.L):
            e.import_state(l, mem[l][0].contiguous(), mem[l][1].contiguous(), _projs(pt, 0)[l])
        e.rng_position = other.rng_position

    fresh = _engine(pt)
    receive(fresh)
    want = _run_leg(pt, "cons", [fresh], [leg], us)[0].arrays() + _state(fresh, pt)
    # a) straight after the fused chain
    a = donors[0]
    receive(a)
    assert _refused(a, pt.Q)
    got = _run_leg(pt, "cons", [a], [leg], us)[0].arrays() + _state(a, pt)
    assert _same(got, want), "consolidate after import_state on a handle whose last step ran in the fused chain"
    # b) after an import_chain_state that no call consumed (document B's chain state: its scores must not be carried)
    b = _engine(pt)
    b.import_chain_state(pt.Q, donors[1].export_chain_state(pt.Q))
    receive(b)
    assert _refused(b, pt.Q)
    got = _run_leg(pt, "cons", [b], [leg], us)[0].arrays() + _state(b, pt)
    assert _same(got, want), "consolidate after import_chain_state + import_state carried the replaced memory's scores"


# ------------------------------------------------------------------------------------------------ device rng
@pytest.mark.parametrize("name", [s.name for s in tc.SEQUENCES if s.shape == "fast" and not s.handoff and not s.variant])
def test_device_rng_continues_one_stream_through_the_pair(name):
    """Two device runs: ``set_device_rng`` with u = None against the same calls given ``philox.gibbs_uniforms`` of positions
    0..6 -- bit for bit; ``rng_position`` is the chunk count after every leg."""
    seq = tc.BY_NAME[name]
    pt = FAST
    steps = [(seq.x, 0), (seq.y, 1), ("fwd", 2)]
    explicit = [torch.from_numpy(philox.gibbs_uniforms(RNG_SEED, d, 0, sum(tc.DOC_LEGS[d]), pt.L, pt.S)).to(DEV) for d in range(len(tc.DOC_LEGS))]
    gen, pos, _ = _play(pt, steps, rng=True)
    exp, pos_e, _ = _play(pt, steps, explicit=explicit)
    want = [list(np.cumsum(legs)[i] for legs in tc.DOC_LEGS) for i in range(3)]
    assert pos == want and pos_e == want, (pos, pos_e)
    assert _same(gen, exp), f"{name}: generated uniforms give other bits than the same uniforms passed in"


@pytest.mark.parametrize("how,x", [("state", "fwd"), ("state", "cons"), ("state", "vid"), ("chain", "cons"), ("chain", "pooled")])
def test_device_rng_position_travels_with_a_hand_off(how, x):
    pt = FAST
    for y in ("cons", "fwd", "vid"):
        steps = [(x, 0), ("hand", how), (y, 1), ("fwd", 2)]
        explicit = [torch.from_numpy(philox.gibbs_uniforms(RNG_SEED, d, 0, sum(tc.DOC_LEGS[d]), pt.L, pt.S)).to(DEV) for d in range(len(tc.DOC_LEGS))]
        gen, pos, _ = _play(pt, steps, rng=True)
        exp, pos_e, _ = _play(pt, steps, explicit=explicit)
        want = [list(np.cumsum(legs)[i] for legs in tc.DOC_LEGS) for i in range(3)]
        assert pos == want and pos_e == want, (how, x, y, pos, pos_e)
        assert _same(gen, exp), f"{x} > {how} > {y}: generated uniforms give other bits than the same uniforms passed in"


# ------------------------------------------------------------------------------------------------ dense plans against the goldens
def _dense_engine(case):
    from infinite_video_amd.engine import LTMEngine
    return LTMEngine(case.N, case.H, case.dh, case.d, case.P, tau=case.tau, sticky=case.sticky, n_layers=case.n_layers,
                     max_q=case.Q, device=DEV, max_batch_chunks=tc.MAX_BATCH_CHUNKS)


def _dense_inputs(case):
    def make():
        ks, qs, ws = gc.case_inputs(case)
        u = np.stack([[gc.call_uniforms(case, c, l) for l in range(case.n_layers)] for c in range(len(case.chunk_T))])
        return ([torch.from_numpy(k).to(DEV) for k in ks], torch.from_numpy(np.stack(qs)).to(DEV),
                [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in w) for w in ws], torch.from_numpy(u).to(DEV),
                gc.load_golden(case))
    return _cached(("dense", case.name), make)


@pytest.mark.parametrize("name", [s.name for s in tc.DENSE_SEQUENCES])
def test_dense_sequence_matches_the_reference(name):
    """Every cut of a dense golden's chunks into two legs: each operation falls back to the per-chunk dense step (one call per run
    of equal chunk length), so every chunk is held to the reference's own run with test_dense_operator_chain_matches_the_reference's
    assertions -- ctx, and after each call B, the last draw and the last scores."""
    from infinite_video_amd.engine import consolidate_videos
    seq = next(s for s in tc.DENSE_SEQUENCES if s.name == name)
    case = tc.DENSE_BY_NAME[seq.case]
    ks, q, projs, u, g = _dense_inputs(case)
    n, L = len(case.chunk_T), case.n_layers
    e = _dense_engine(case)
    assert e.ensure_plan(case.chunk_T[0]).dense
    by = None
    if seq.y == "vid":
        by = _dense_engine(case)
        by.forward(ks[0], q, projs, None, new_doc=True)
        by_before = [x.cpu().numpy() for l in range(L) for x in by.export_state(l)]

    def after_call(c):
        for l in range(L):
            tag = f"c{c}_l{l}"
            if c > 0:
                bins, _, probs = e.last_draw(l)
                np.testing.assert_allclose(probs, g[tag + "_probs"], rtol=2e-5, atol=1e-9)
                np.testing.assert_array_equal(bins, g[tag + "_bins"])
            _golden_B_check(case, g, tag, e.export_state(l)[0].cpu().numpy())
            np.testing.assert_allclose(e.last_scores(l, case.Q), g[tag + "_scores"], rtol=1e-4, atol=2e-5)

    for op, lo, hi in ((seq.x, 0, seq.cut), (seq.y, seq.cut, n)):
        c0 = lo
        while c0 < hi:
            c1 = c0 + 1
            while op != "fwd" and c1 < hi and case.chunk_T[c1] == case.chunk_T[c0]:
                c1 += 1
            new_doc = c0 == 0
            if op == "fwd":
                y = e.forward(ks[c0], q, projs, u[c0] if c0 else None, new_doc=new_doc)[None]
            else:
                k, uu = torch.stack(ks[c0:c1]), u[c0:c1].contiguous()
                if op == "cons":
                    y = e.consolidate(k, q, projs, uu, new_doc=new_doc)
                elif op == "cons_q":
                    y = e.consolidate_q(k, q[None].expand(c1 - c0, -1, -1, -1).contiguous(), projs, uu, new_doc=new_doc)
                else:
                    both = by is not None and not new_doc
                    y = consolidate_videos([e, by] if both else [e], k, [c1 - c0, 0] if both else [c1 - c0], q, projs, uu, new_doc=new_doc)
            e.sync()
            y = y.cpu().numpy()
            for c in range(c0, c1):
                for l in range(L):
                    np.testing.assert_allclose(y[c - c0, l], g[f"c{c}_l{l}_ctx"], rtol=0, atol=CTX_TOL, err_msg=f"{name}: chunk {c} layer {l}")
            after_call(c1 - 1)
            c0 = c1
    assert e.rng_position == n
    if by is not None:
        assert _same(by_before, [x.cpu().numpy() for l in range(L) for x in by.export_state(l)])


# ================================================================================================ the video Q-former level
# The three entry points through the raw C ABI (InfVideoEncoder fixes 12 heads and enc_width == hidden, which VQF_BASE is not;
# these are the calls its encode_frames / encode_frames_batch / encode_videos make, set_weights_epoch included).
QF_ATOL = 2e-4            # tests/test_call_seams_gpu.py's bound on hidden / llama rows


class _Vqf:
    def __init__(self):
        import ctypes as C
        from infinite_video_amd import _lib
        from tests.test_config_sweep_gpu import _vqf_weights_struct
        self.C, self._lib, self.lib = C, _lib, _lib.load()
        s = self.s = seam_cases.VQF_BASE
        self.L = s["n_layers"]
        self.ws, self.keep = _vqf_weights_struct(tc.vqf_weights(), self.L, DEV)
        cfg = _lib.VqfConfig(n_layers=self.L, n_heads=s["heads"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                             tokens_per_frame=s["P"], n_query=s["n_query"], proj_out=s["proj"], nb_samples=seam_cases.S,
                             alpha=s["alpha"], ln_eps=1e-12)
        self.h = C.c_void_p()
        _lib.check(self.lib.infv_vqf_create(C.byref(cfg), C.byref(self.h)))
        self.epoch = 1
        _lib.check(self.lib.infv_vqf_set_weights_epoch(self.h, self.epoch))     # non-zero: encode_chunk reuses layer 0's prefix

    def close(self):
        self._lib.check(self.lib.infv_vqf_destroy(self.h))

    def memory(self):
        from infinite_video_amd.engine import LTMEngine
        s = self.s
        engs = [LTMEngine(s["N"], s["heads"], s["hidden"] // s["heads"], s["enc_width"], s["P"], tau=s["tau"], sticky=s["sticky"],
                          n_layers=1, max_q=s["n_query"], device=DEV) for _ in range(self.L)]
        for e in engs:
            e.ensure_plan(s["T"])
        return engs

    def change_prefix_weight(self):
        """In place (same address): only the epoch tells the library that layer 0's cached prefix is stale."""
        name = tc.VQF_PREFIX_WEIGHT
        self.keep[name].copy_(torch.from_numpy(tc.vqf_weights(True)[name]).to(DEV))
        self.epoch += 1
        self._lib.check(self.lib.infv_vqf_set_weights_epoch(self.h, self.epoch))

    def _stream(self):
        return self.C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def run(self, op, mems, ks, us, new_video):
        """Advance every video's memories by its chunks ks[v] [n, T*P, enc] with uniforms us[v] [n, L, S].  Returns per video
        (hidden [n, Q, hidden], llama [n, Q, proj]) on the host."""
        C, s, lib, check = self.C, self.s, self.lib, self._lib.check
        Q, T = s["n_query"], s["T"]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        out = []
        with torch.cuda.device(DEV):
            if op == "videos":
                V, counts = len(mems), [int(k.shape[0]) for k in ks]
                total = sum(counts)
                k, u = torch.cat(ks).contiguous(), torch.cat(us).contiguous()
                handles = (C.c_void_p * (V * self.L))(*[e._h.value for m in mems for e in m])
                cu = (C.c_int32 * (V + 1))(0, *np.cumsum(counts).tolist())
                hid, lla = torch.empty(total, Q, s["hidden"], device=DEV), torch.empty(total, Q, s["proj"], device=DEV)
                mean = torch.empty(V, Q, s["proj"], device=DEV)
                check(lib.infv_vqf_encode_videos(self.h, handles, V, C.cast(cu, C.c_void_p), ptr(k), T, C.byref(self.ws), ptr(u),
                                                 int(new_video), ptr(hid), ptr(lla), ptr(mean), self._stream()))
                torch.cuda.synchronize()
                lo = 0
                for n in counts:
                    out.append((hid[lo:lo + n].cpu().numpy(), lla[lo:lo + n].cpu().numpy()))
                    lo += n
                return out
            for m, k, u in zip(mems, ks, us):
                n = int(k.shape[0])
                handles = (C.c_void_p * self.L)(*[e._h.value for e in m])
                hid, lla = torch.empty(n, Q, s["hidden"], device=DEV), torch.empty(n, Q, s["proj"], device=DEV)
                if op == "video":
                    mean = torch.empty(Q, s["proj"], device=DEV)
                    check(lib.infv_vqf_encode_video(self.h, handles, ptr(k), n, T, C.byref(self.ws), ptr(u), int(new_video), ptr(hid),
                                                    ptr(lla), ptr(mean), self._stream()))
                else:
                    for c in range(n):
                        first = new_video and c == 0
                        check(lib.infv_vqf_encode_chunk(self.h, handles, ptr(k[c]), T, C.byref(self.ws), C.c_void_p(0) if first else ptr(u[c]),
                                                        int(first), ptr(hid[c]), ptr(lla[c]), self._stream()))
                torch.cuda.synchronize()
                out.append((hid.cpu().numpy(), lla.cpu().numpy()))
        return out


@pytest.mark.parametrize("name", [s.name for s in tc.VQF_SEQUENCES])
def test_vqf_sequence_matches_the_oracle(name):
    """Two videos in legs of 2 + 2 chunks and one closing encode_chunk: hidden and llama rows of every chunk against
    VideoQformerOracle (2e-4), every draw that can be read back equal to the oracle's (``set_trace`` where the LTM path keeps one,
    ``last_draw`` at the end of every call), the memories' B at the end (2e-5)."""
    seq = tc.VQF_BY_NAME[name]
    ref = tc.vqf_reference(seq.epoch)
    vids = range(tc.VQF_VIDEOS)
    q = _Vqf()
    try:
        mems = [q.memory() for _ in vids]
        worst, draws, lo = 0.0, 0, 0
        for i, (op, n) in enumerate(zip((seq.x, seq.y, "chunk"), tc.VQF_LEGS)):
            if i == 1 and seq.epoch:
                q.change_prefix_weight()
            ks = [torch.from_numpy(tc.vqf_chunks(v)[lo:lo + n]).to(DEV) for v in vids]
            us = [torch.from_numpy(ref[v][1][lo:lo + n]).to(DEV).contiguous() for v in vids]
            traces = [[e.set_trace(n) for e in m] for m in mems]
            got = q.run(op, mems, ks, us, new_video=(i == 0))
            for v in vids:
                orun = ref[v][0]
                for e in mems[v]:
                    e.sync()
                for c in range(lo, lo + n):
                    for what, a, b in (("hidden", got[v][0][c - lo], orun.hidden[c]), ("llama", got[v][1][c - lo], orun.proj[c])):
                        err = float(np.abs(a - b).max())
                        worst = max(worst, err)
                        assert err <= QF_ATOL, f"{name}: video {v} chunk {c}: |{what} - oracle| = {err:.3e} after {op}"
                    for l, e in enumerate(mems[v]):
                        if c == 0:
                            continue
                        bins = traces[v][l][0][c - lo, 0].cpu().numpy()
                        if bins[0] < 0 and c == lo + n - 1:
                            bins = e.last_draw(0)[0]
                        if bins[0] >= 0:
                            assert np.array_equal(bins, orun.bins[c][l]), f"{name}: video {v} chunk {c} layer {l}: draws differ from the oracle's"
                            draws += len(bins)
                for e in mems[v]:
                    e.set_trace(0)
                    assert e.rng_position == lo + n
            lo += n
        for v in vids:
            for l, e in enumerate(mems[v]):
                eB = float(np.abs(e.export_state(0)[0].cpu().numpy() - ref[v][0].B[l]).max())
                assert eB <= VQF_B_TOL, f"{name}: video {v} layer {l}: |B - oracle| = {eB:.3e}"
        assert draws >= tc.VQF_VIDEOS * q.L * seam_cases.S * 3          # at least the last draw of every call
        record_parity(f"[path transitions] {name}: worst |rows - oracle| {worst:.2e}, {draws} draws compared, all equal")
    finally:
        q.close()
