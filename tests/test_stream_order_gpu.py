"""Every entry point on a side stream with work in flight around it (tests/golden/stream_cases.py has the cases).

Both headers promise that every call is asynchronous on the caller's ``stream``.  The rest of the suite runs on the default stream
with inputs that were complete long before the call and outputs read after a host synchronisation, where a missing wait between the
caller's stream and an internal one, a join that hands the stream back early, a staging buffer rewritten early or a host setter that
overtakes queued work are all invisible.  Here they become wrong numbers.

The method, once.  A scenario creates its handles and registers every device input with a good value and a DECOY (a second finite
draw of the same generator), then describes its call sequence.  The sequence runs

1. *warm*: once on the fresh handles with the decoys, on the default stream.  The first call of a handle grows its workspaces, and a
   growth synchronises the device (csrc/capi_common.h, reserve_all): under a delay the host would simply wait the delay out and the
   call could not be misordered.  The warm run leaves stale decoy-derived values in every workspace and ends with every memory reset
   by the sequence's own first step.  (``ltm_fresh_handle_first_call`` has no warm run: the first call is what it is about.)
2. *expected* (``mode="sync"``): good values copied in, a host synchronisation between every step, every output cloned.
3. *under test* (``mode="side"``, fresh handles again): on ``s = torch.cuda.Stream()``, from one host thread and with no host
   synchronisation: a delay (``torch.cuda._sleep``), ``buf.copy_(good)`` for every input, the calls, ``out.clone()`` for every
   output, the exports, ``buf.copy_(decoy)`` for every input.  Then one synchronisation, ``get_draw`` and ``infv_ltm_sync``.

Outputs and exported state must be equal bit for bit (``torch.equal``): the first fill fails if an internal stream reads before the
caller's stream has reached the call, the second if the call returns the stream while something still reads an input, the clone if an
output is not complete on the caller's stream.  One control per family runs the synchronised sequence twice (equal bits: that
licenses equality), three controls misorder the fill on the test's own side and must see other numbers.

The delay must be four times the host time of the enqueue block (``time.perf_counter``), or the case fails with "delay too short".
Where the library documents a host wait inside the sequence (``stream_cases.Case.host_wait``) the host time is taken up to that call.
Needs a real MI355X: run with ``-m gpu``."""
import contextlib
import ctypes as C
import gc
import time
import types

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.basis_maps import NB_SAMPLES
from tests.conftest import record_parity
from tests.golden import seam_cases as sm
from tests.golden import stream_cases as st
from tests.golden.frame_qformer_cases import LN_VISION_EPS
from tests.golden.frame_qformer_cases import SMALL as FRAME_SMALL

pytestmark = pytest.mark.gpu
S = NB_SAMPLES
SCENARIOS = {}


def scenario(name):
    def reg(fn):
        assert name not in SCENARIOS
        SCENARIOS[name] = fn
        return fn
    return reg


def dev0():
    return torch.device("cuda:0")


def cur_stream():
    return torch.cuda.current_stream(dev0()).cuda_stream


# ------------------------------------------------------------------------------------------------ the delay
_delay = {}


def cycles_per_ms() -> float:
    """``torch.cuda._sleep`` cycles per millisecond, measured once per session with events on the idle default stream."""
    if "cpm" not in _delay:
        torch.cuda.synchronize()
        n, ms = 1_000_000, 0.0
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 15.0:
                break
            n = int(n * max(2.0, 20.0 / max(ms, 1e-3)))
        assert ms >= 15.0, f"could not calibrate the delay: {n} cycles took {ms} ms"
        _delay["cpm"] = n / ms
        record_parity(f"[stream order] delay calibration: {n} cycles of torch.cuda._sleep took {ms:.2f} ms on the idle default stream")
    return _delay["cpm"]


def issue_delay(ms: float) -> None:
    torch.cuda._sleep(int(ms * cycles_per_ms()))


# ------------------------------------------------------------------------------------------------ the harness
def to_dev(x, dtype=None):
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())       # (the cached generator outputs are read-only)
    x = x.detach().to(dev0())
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.contiguous()


class Env:
    """What a scenario sees: input registration while it sets up, and ``step`` / ``out`` / ``after`` / ``lane`` / ``host_mark`` while
    its call sequence runs in one of the phases warm, pre, sync, side."""

    def __init__(self, case, mode):
        self.case, self.mode, self.phase = case, mode, "setup"
        self.dev = dev0()
        self.inputs, self.lanes, self.warm = [], 1, True
        self.streams, self.outs, self._after, self._cleanup = [], {}, [], []
        self.host_end, self.run_index = None, 0
        self.keep, self.t0, self.marks = [], 0.0, []

    # ---- setup
    def inp(self, good, decoy, dtype=None, lane=0, into=None):
        """A preallocated device input holding the decoy; ``into``: an existing tensor (a module parameter) to use as the buffer."""
        g, d = to_dev(good, dtype), to_dev(decoy, dtype)
        assert g.shape == d.shape and g.dtype == d.dtype
        buf = torch.empty_like(d) if into is None else into
        buf.copy_(d)
        self.inputs.append((buf, g, d, lane))
        return buf

    def cleanup(self, fn):
        self._cleanup.append(fn)

    # ---- while the sequence runs
    @property
    def recording(self):
        return self.phase in ("sync", "side")

    def mark(self, label):
        if self.phase == "side":
            self.marks.append(f"{label} {(time.perf_counter() - self.t0) * 1e3:.2f}")

    def step(self):
        """Between two steps of the sequence: the expected run synchronises the host here, the run under test only notes the host time."""
        if self.phase == "sync":
            torch.cuda.synchronize()
        self.mark(f"step{len(self.marks)}")

    def out(self, **tensors):
        if self.recording:
            for k, t in tensors.items():
                assert k not in self.outs, k
                self.outs[k] = t.detach().clone()                # (on the current stream: complete only if the output is)

    def after(self, fn):
        """``fn() -> {name: array}`` runs after the final synchronisation (get_draw, infv_ltm_sync, host-synchronising wrappers)."""
        if self.recording:
            self._after.append(fn)

    def lane(self, i):
        if self.phase == "side":
            return torch.cuda.stream(self.streams[i])
        return contextlib.nullcontext()

    def host_mark(self):
        """The next call is one the library documents as waiting on the host: the issue time is taken up to here."""
        if self.phase == "side" and self.host_end is None:
            self.host_end = time.perf_counter()

    def fill(self, which, lane=None):
        for buf, g, d, ln in self.inputs:
            if lane is None or ln == lane:
                buf.copy_(g if which == "good" else d)


_fault = []


def run_case(name, mode, misorder=False):
    """``_run_case``; after a HIP error nothing more of this module is started on the device."""
    if _fault:
        pytest.fail(f"not run: {_fault[0]}")
    try:
        return _run_case(name, mode, misorder)
    except Exception as e:                                       # (a failed assertion is an AssertionError without these words)
        if not isinstance(e, AssertionError) and "hip" in str(e).lower():
            _fault.append(f"{name} ({mode}) raised {type(e).__name__}: {str(e)[:200]}")
        raise


def _run_case(name, mode, misorder=False):
    """({output name: host tensor / array}, delay in ms, host issue time in ms) of one run of the case's sequence."""
    case = st.BY_NAME[name]
    with torch.no_grad():
        env = Env(case, mode)
        made = SCENARIOS[name](env)
        pre, calls = made if isinstance(made, tuple) else (None, made)
        delay_ms = host_ms = 0.0
        try:
            torch.cuda.synchronize()
            if env.warm:
                env.phase = "warm"
                if pre:
                    pre()
                calls()
                torch.cuda.synchronize()
            env.run_index = 1
            if pre:
                env.phase = "pre"
                pre()
                torch.cuda.synchronize()
            if mode == "sync":
                env.phase = "sync"
                env.fill("good")
                torch.cuda.synchronize()
                calls()
                torch.cuda.synchronize()
            else:
                env.streams = [torch.cuda.Stream(env.dev) for _ in range(env.lanes)]
                late = torch.cuda.Stream(env.dev) if misorder else None
                cpm = cycles_per_ms() if case.delay_ms else 0.0
                delay_ms = int(case.delay_ms * cpm) / cpm if cpm else 0.0
                env.phase = "side"
                # Handles of earlier cases that the cyclic collector has not freed yet go now, and the collector stays off while the
                # block is issued: destroying a handle synchronises its streams and frees its workspaces, and a collection that
                # happened to start inside the block would wait the delay out on the host.
                gc.collect()
                gc.disable()
                for s in env.streams + ([late] if late is not None else []):
                    with torch.cuda.stream(s):                   # torch's allocator keeps a pool per stream: its first blocks are hipMallocs
                        for n in (1 << 10, 2 << 20, 32 << 20):
                            torch.empty(n, dtype=torch.uint8, device=env.dev)
                torch.cuda.synchronize()
                t0 = env.t0 = time.perf_counter()
                for i, s in enumerate(env.streams):
                    with torch.cuda.stream(s):
                        if case.delay_ms:
                            issue_delay(case.delay_ms)
                        if not misorder:
                            env.fill("good", i)
                if misorder:                                     # the good values arrive on another stream, unordered and too late
                    with torch.cuda.stream(late):
                        issue_delay(case.delay_ms + 250.0)
                        env.fill("good")
                env.mark("filled")
                with torch.cuda.stream(env.streams[0]):
                    calls()
                env.mark("called")
                for i, s in enumerate(env.streams):
                    with torch.cuda.stream(s):
                        env.fill("decoy", i)
                env.mark("refilled")
                t1 = env.host_end if env.host_end is not None else time.perf_counter()
                host_ms = (t1 - t0) * 1e3
                gc.enable()
                torch.cuda.synchronize()
            env.phase = "done"
            outs = {k: v.cpu() for k, v in env.outs.items()}
            for fn in env._after:
                for k, v in fn().items():
                    assert k not in outs, k
                    outs[k] = v.cpu() if isinstance(v, torch.Tensor) else np.array(v, copy=True)
            torch.cuda.synchronize()
        finally:
            gc.enable()
            torch.cuda.synchronize()
            for fn in env._cleanup:
                fn()
    _timeline[name] = ", ".join(env.marks)
    return outs, delay_ms, host_ms


_timeline = {}                                                   # case -> host times (ms) of the last enqueue block, for a failure message


def same(a, b) -> bool:
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and \
            torch.equal(a.view(torch.uint8) if a.dtype == torch.float8_e4m3fn else a, b.view(torch.uint8) if b.dtype == torch.float8_e4m3fn else b)
    return np.array_equal(a, b)


def differing(exp, got):
    assert set(exp) == set(got), sorted(set(exp) ^ set(got))
    return sorted(k for k in exp if not same(exp[k], got[k]))


_expected = {}


def expected(name):
    """The synchronised run of the case, computed once and shared (never modified)."""
    if name not in _expected:
        outs, _, _ = run_case(name, "sync")
        assert outs, name
        if name == "ltm_consolidate_800":                        # (160 MB of ctx: not kept for the session)
            return outs
        _expected[name] = outs
    return _expected[name]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", [c.name for c in st.CASES])
def test_case_on_a_side_stream(name):
    case = st.BY_NAME[name]
    exp = expected(name)
    got, delay_ms, host_ms = run_case(name, "side")
    bad = differing(exp, got)
    short = bool(case.delay_ms) and 4.0 * host_ms > delay_ms
    verdict = "delay too short" if short else ("equal bits" if not bad else f"{len(bad)} of {len(exp)} outputs differ")
    record_parity(f"[stream order] {name} ({case.mechanism}): delay {delay_ms:.1f} ms, host issue {host_ms:.2f} ms, {len(exp)} outputs: {verdict}"
                  + (f"; issue time taken up to: {case.host_wait}" if case.host_wait else ""))
    assert not bad, f"{name}: outputs that differ from the synchronised run: {bad}"
    assert not short, f"{name}: delay too short: host issue {host_ms:.2f} ms against a delay of {delay_ms:.1f} ms (host ms at: {_timeline[name]})"


@pytest.mark.parametrize("family", st.FAMILIES)
def test_control_the_synchronised_sequence_is_deterministic(family):
    name = st.DETERMINISM_CONTROLS[family]
    a = expected(name)
    b, _, _ = run_case(name, "sync")
    bad = differing(a, b)
    record_parity(f"[stream order] control, {family}: {name} synchronised twice: {'equal bits' if not bad else 'DIFFERS in ' + ', '.join(bad)}")
    assert not bad, f"{family}: the synchronised sequence is not deterministic in {bad}"


@pytest.mark.parametrize("name", st.MISORDER_CONTROLS)
def test_control_a_misordered_fill_is_seen(name):
    """The good fill queued behind a longer delay on a second stream with no event to the call's: the call legitimately reads the
    decoy, so its snapshot must differ from the expected result -- the method can fail."""
    exp = expected(name)
    got, delay_ms, host_ms = run_case(name, "side", misorder=True)
    bad = differing(exp, got)
    record_parity(f"[stream order] control, misordered fill: {name}: delay {delay_ms:.1f} ms, host issue {host_ms:.2f} ms, "
                  f"{len(bad)} of {len(exp)} outputs differ")
    main = [k for k in exp if k.startswith(("ctx", "hidden", "llama"))]
    assert main and all(k in bad for k in main), f"{name}: a misordered fill went unseen in {[k for k in main if k not in bad]}"


# ------------------------------------------------------------------------------------------------ LTM scenarios
def ltm_engine(pt, **kw):
    from infinite_video_amd.engine import LTMEngine
    eng = LTMEngine(pt.N, pt.H, 64, pt.d, pt.P, tau=pt.tau, sticky=pt.sticky, n_layers=pt.L, max_q=pt.Q, device=dev0(), nb_samples=pt.S, **kw)
    eng.ensure_plan(pt.T)
    return eng


class LtmIn:
    """The poisoned inputs of one LTM call sequence: tokens (or frame means), queries, projections, uniforms."""

    def __init__(self, env, pt, n_chunks, dtype=torch.float32, video=0, lane=0, kbar=False, q_chunks=0, share=None, tile=1):
        P = 1 if kbar else pt.P
        both = [st.tokens(n_chunks, pt.T, P, pt.d, decoy, video) for decoy in (False, True)]
        if tile > 1:
            both = [to_dev(a, dtype).repeat(tile, 1, 1) for a in both]
        self.k = env.inp(both[0], both[1], dtype, lane)
        self.u = env.inp(st.uniforms(n_chunks * tile, pt.L, pt.S, False, video), st.uniforms(n_chunks * tile, pt.L, pt.S, True, video), None, lane)
        if share is not None:
            self.q, self.projs = share.q, share.projs
            return
        self.q = env.inp(st.queries(pt.L, pt.Q, pt.dm, False, q_chunks), st.queries(pt.L, pt.Q, pt.dm, True, q_chunks), None, lane)
        pg, pd = st.projections(pt.L, pt.d, pt.dm, False), st.projections(pt.L, pt.d, pt.dm, True)
        self.projs = [tuple(env.inp(g, d, None, lane) for g, d in zip(pg[l], pd[l])) for l in range(pt.L)]


def ltm_state(env, eng, tag=""):
    """Exported state of every layer behind the calls, the last draw after the synchronisation."""
    for l in range(eng.L):
        B, mass = eng.export_state(l)
        env.out(**{f"{tag}B{l}": B, f"{tag}mass{l}": mass})

    def draws():
        eng.sync()                                               # (raises if a device-side failure was latched)
        out = {}
        for l in range(eng.L):
            bins, idx, probs = eng.last_draw(l)
            out.update({f"{tag}bins{l}": bins, f"{tag}idx{l}": idx, f"{tag}probs{l}": probs})
        return out
    env.after(draws)


def _consolidate_scenario(n_chunks, then=None, dtype=torch.float32, pt=None, tile=1, ctx_sum=False, **eng_kw):
    def make(env):
        p = pt or st.SMALL
        eng = ltm_engine(p, **eng_kw)
        if ctx_sum:
            eng.set_ctx_sum(True)
        x = LtmIn(env, p, n_chunks, dtype, tile=tile)

        def calls():
            y = eng.consolidate(x.k, x.q, x.projs, x.u, new_doc=True)
            env.step()
            env.out(ctx=y)
            if then:
                then(env, eng, x, y)
            ltm_state(env, eng)
        return calls
    return make


SCENARIOS["ltm_consolidate_4"] = _consolidate_scenario(4)
SCENARIOS["ltm_consolidate_70"] = _consolidate_scenario(70, max_batch_chunks=32)
SCENARIOS["ltm_dense_N96"] = _consolidate_scenario(3, pt=st.DENSE_N96)
SCENARIOS["ltm_gauss"] = _consolidate_scenario(3, pt=st.GAUSS, gaussian_sigmas=st.GAUSS.sigmas)


@scenario("ltm_consolidate_800")
def _(env):
    """800 chunks: the call-long pooling launch with flag_wait_kernel.  The expected run profiles the handle and requires that the
    call issued fewer pooling launches than it has sub-batches: the per-sub-batch form issues one each."""
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 16, tile=50)
    n = 800

    def calls():
        prof = env.phase == "sync"
        if prof:
            eng.profile(True)
        y = eng.consolidate(x.k, x.q, x.projs, x.u, new_doc=True)
        env.step()
        if prof:
            fam = eng.profile_read()
            eng.profile(False)
            sub_batches = (n - 1 + 31) // 32
            assert fam["chain"][0] > 0 and fam["uc"][0] > 0, f"800 chunks did not run the fused chain: {fam}"
            assert 0 < fam["pool"][0] < sub_batches, f"800 chunks did not take the call-long pooling launch: {fam['pool'][0]} pooling launches"
        env.out(ctx=y)
        ltm_state(env, eng)
    return calls


@scenario("ltm_forward_twice")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 2)

    def calls():
        y0 = eng.forward(x.k[0], x.q, x.projs, None, new_doc=True)
        env.step()
        y1 = eng.forward(x.k[1], x.q, x.projs, x.u[1], new_doc=False)
        env.step()
        env.out(ctx0=y0, ctx1=y1)
        ltm_state(env, eng)
    return calls


@scenario("ltm_forward_into_twice")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 2)

    def calls():
        eng.reset()
        pa = eng._proj_array(x.projs)
        kbar = torch.empty(2, pt.T, pt.d, device=env.dev)
        ctx = torch.empty(2, pt.L, pt.Q, pt.dm, device=env.dev)
        for c in range(2):
            eng.forward_into_raw(x.k[c].data_ptr(), 0, pt.T, kbar[c].data_ptr(), x.q.data_ptr(), pt.Q, pa, x.u[c].data_ptr() if c else 0,
                                 ctx[c].data_ptr(), C.c_void_p(cur_stream()))
            env.step()
        env.out(ctx=ctx, kbar=kbar)
        ltm_state(env, eng)
    return calls


@scenario("ltm_pool_rows_step")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 3)

    def calls():
        eng.reset()
        kbar = eng.pool(x.k)
        env.step()
        R = eng.pool_rows(x.k)
        env.step()
        ys = []
        for c in range(3):
            ys.append(eng.step(kbar[c], x.q, x.projs, x.u[c] if c else None))
            env.step()
        env.out(kbar=kbar, rows=R, ctx=torch.stack(ys))
        ltm_state(env, eng)
    return calls


@scenario("ltm_steps")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 4, kbar=True, q_chunks=4)

    def calls():
        eng.reset()
        y = eng.steps(x.k, x.q, x.projs, x.u)
        env.step()
        env.out(ctx=y)
        ltm_state(env, eng)
    return calls


@scenario("ltm_consolidate_q")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 4, q_chunks=4)

    def calls():
        y = eng.consolidate_q(x.k, x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y)
        ltm_state(env, eng)
    return calls


@scenario("ltm_consolidate_pooled")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt)
    x = LtmIn(env, pt, 4, kbar=True)

    def calls():
        y = eng.consolidate_pooled(x.k, x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y)
        ltm_state(env, eng)
    return calls


def _two_calls(new_doc_second, dtype=torch.float32):
    def make(env):
        pt = st.SMALL
        eng = ltm_engine(pt, fp16_tokens=(dtype == torch.float16))
        a = LtmIn(env, pt, 36, dtype, video=0)
        b = LtmIn(env, pt, 36, dtype, video=1, share=a)

        def calls():
            ya = eng.consolidate(a.k, a.q, a.projs, a.u, new_doc=True)
            env.step()
            yb = eng.consolidate(b.k, a.q, a.projs, b.u, new_doc=new_doc_second)
            env.step()
            env.out(ctxA=ya, ctxB=yb)
            ltm_state(env, eng)
        return calls
    return make


SCENARIOS["ltm_two_calls_continue"] = _two_calls(False)
SCENARIOS["ltm_two_calls_new_doc"] = _two_calls(True)
SCENARIOS["ltm_two_calls_f16"] = _two_calls(False, torch.float16)
SCENARIOS["ltm_two_calls_bf16"] = _two_calls(False, torch.bfloat16)
SCENARIOS["ltm_two_calls_f8"] = _two_calls(False, torch.float8_e4m3fn)


def _videos_inputs(env, pt, kbar, q_chunks=0):
    P = 1 if kbar else pt.P
    cat = lambda fn: [np.concatenate([fn(c, decoy, v + 1) for v, c in enumerate(st.RAGGED)]) for decoy in (False, True)]
    k = cat(lambda c, decoy, v: st.tokens(c, pt.T, P, pt.d, decoy, v))
    u = cat(lambda c, decoy, v: st.uniforms(c, pt.L, pt.S, decoy, v))
    x = types.SimpleNamespace()
    x.k, x.u = env.inp(*k), env.inp(*u)
    x.q = env.inp(st.queries(pt.L, pt.Q, pt.dm, False, q_chunks), st.queries(pt.L, pt.Q, pt.dm, True, q_chunks))
    pg, pd = st.projections(pt.L, pt.d, pt.dm, False), st.projections(pt.L, pt.d, pt.dm, True)
    x.projs = [tuple(env.inp(g, d) for g, d in zip(pg[l], pd[l])) for l in range(pt.L)]
    return x


def _videos_state(env, engs):
    for v, e in enumerate(engs):
        ltm_state(env, e, f"v{v}_")


@scenario("ltm_consolidate_videos")
def _(env):
    from infinite_video_amd.engine import consolidate_videos
    pt = st.SMALL
    engs = [ltm_engine(pt) for _ in st.RAGGED]
    x = _videos_inputs(env, pt, kbar=False)

    def calls():
        y = consolidate_videos(engs, x.k, list(st.RAGGED), x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y)
        _videos_state(env, engs)
    return calls


@scenario("ltm_steps_videos")
def _(env):
    from infinite_video_amd.engine import steps_videos
    pt = st.SMALL
    engs = [ltm_engine(pt) for _ in st.RAGGED]
    x = _videos_inputs(env, pt, kbar=True)

    def calls():
        y = steps_videos(engs, x.k, list(st.RAGGED), x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y)
        _videos_state(env, engs)
    return calls


@scenario("ltm_steps_videos_from")
def _(env):
    from infinite_video_amd.engine import steps_videos
    pt = st.SMALL
    engs = [ltm_engine(pt) for _ in st.RAGGED]
    total = sum(st.RAGGED)
    x = _videos_inputs(env, pt, kbar=True, q_chunks=total)
    shared = env.inp(st.tokens(6, pt.T, 1, pt.d, False, 9), st.tokens(6, pt.T, 1, pt.d, True, 9))
    base = (0, 2, 1, 4, 0)                                       # base + count <= 6 for every video of RAGGED

    def calls():
        y = steps_videos(engs, shared, list(st.RAGGED), x.q, x.projs, x.u, new_doc=True, kbar_chunk0=base)
        env.step()
        env.out(ctx=y)
        _videos_state(env, engs)
    return calls


def _then_pack(env, eng, x, y):
    env.out(payload=eng.pack_memory(y))
    env.step()


SCENARIOS["ltm_then_pack_memory"] = _consolidate_scenario(70, then=_then_pack, ctx_sum=True, max_batch_chunks=32)


@scenario("ltm_then_export_import_state")
def _(env):
    pt = st.SMALL
    eng, eng2 = ltm_engine(pt, max_batch_chunks=32), ltm_engine(pt)
    x = LtmIn(env, pt, 70)

    def calls():
        y = eng.consolidate(x.k[:69], x.q, x.projs, x.u[:69], new_doc=True)
        env.step()
        eng2.reset()
        for l in range(pt.L):
            B, mass = eng.export_state(l)
            env.step()
            eng2.import_state(l, B, mass, x.projs[l])
            env.step()
        y2 = eng2.forward(x.k[69], x.q, x.projs, x.u[69], new_doc=False)
        env.step()
        env.out(ctx=y, ctx_after_import=y2)
        ltm_state(env, eng)
        ltm_state(env, eng2, "imp_")
    return calls


@scenario("ltm_then_chain_state")
def _(env):
    pt = st.SMALL
    eng, eng2 = ltm_engine(pt, max_batch_chunks=32), ltm_engine(pt, max_batch_chunks=32)
    x = LtmIn(env, pt, 70)

    def calls():
        eng2.reset()
        y = eng.consolidate(x.k[:35], x.q, x.projs, x.u[:35], new_doc=True)
        env.step()
        blob = eng.export_chain_state(pt.Q)
        env.step()
        eng2.import_chain_state(pt.Q, blob)
        env.step()
        y2 = eng2.consolidate(x.k[35:], x.q, x.projs, x.u[35:], new_doc=False)
        env.step()
        env.out(ctx=y, blob=blob, ctx_continued=y2)
        ltm_state(env, eng)
        ltm_state(env, eng2, "cont_")
    return calls


@scenario("ltm_then_reproject_forward")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt, max_batch_chunks=32)
    x = LtmIn(env, pt, 70)

    def calls():
        y = eng.consolidate(x.k[:69], x.q, x.projs, x.u[:69], new_doc=True)
        env.step()
        eng.reproject(x.projs)
        env.step()
        y2 = eng.forward(x.k[69], x.q, x.projs, x.u[69], new_doc=False)
        env.step()
        env.out(ctx=y, ctx_forward=y2)
        ltm_state(env, eng)
    return calls


@scenario("ltm_then_density_masses")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt, max_batch_chunks=32)
    eng.set_grid_plan()
    x = LtmIn(env, pt, 70)

    def calls():
        y = eng.consolidate(x.k, x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y)
        for l in range(pt.L):
            env.out(**{f"alphas{l}": eng.density(l, pt.Q), f"masses{l}": eng.masses(l, pt.Q)})
            env.step()
        ltm_state(env, eng)
    return calls


@scenario("ltm_then_traces_sources")
def _(env):
    pt = st.SMALL
    eng = ltm_engine(pt, max_batch_chunks=32)
    x = LtmIn(env, pt, 70)

    def calls():
        bins, probs = eng.set_trace(70)
        mass = eng.set_mass_trace(70)
        env.step()
        y = eng.consolidate(x.k, x.q, x.projs, x.u, new_doc=True)
        env.step()
        env.out(ctx=y, trace_bins=bins, trace_probs=probs, trace_mass=mass)
        ltm_state(env, eng)

        def sources():                                           # (the wrapper reads a counter back: behind the synchronisation)
            W, attn = eng.source_weights(bins, pt.T, mass=mass.contiguous())
            return {"W": W, "attn": attn}
        env.after(sources)
    return calls


@scenario("ltm_fresh_handle_first_call")
def _(env):
    """create + first call, five times, the first call on the side stream: infv_ltm_create's null-stream hipMemsets against it."""
    pt = st.SMALL
    env.warm = False
    x = LtmIn(env, pt, 4)
    alive = []

    def calls():
        for r in range(5):
            eng = ltm_engine(pt)
            alive.append(eng)
            y = eng.consolidate(x.k, x.q, x.projs, x.u, new_doc=True)
            env.step()
            env.out(**{f"ctx{r}": y})
            ltm_state(env, eng, f"r{r}_")
    return calls


def _setter(which):
    def make(env):
        pt = st.SMALL
        eng = ltm_engine(pt)
        x = LtmIn(env, pt, 3)
        const = [to_dev(a) for a in (st.tokens(1, pt.T, pt.P, pt.d, False, 5)[0], st.queries(pt.L, pt.Q, pt.dm, False))]
        cproj = [tuple(to_dev(a) for a in p) for p in st.projections(pt.L, pt.d, pt.dm, False)]
        rng = np.random.default_rng(11)
        if which == "bins":
            old, new = (rng.integers(0, 127, (pt.L, pt.S)).astype(np.int32) for _ in range(2))
            setter = eng.set_bins
        else:
            old, new = ((rng.random((pt.L, 127)) + 0.01).astype(np.float32) for _ in range(2))
            setter = eng.set_probs

        def pre():                                               # a memory and an override are in place before the delay starts
            eng.forward(const[0], const[1], cproj, None, new_doc=True)
            torch.cuda.synchronize()
            for l in range(pt.L):
                setter(l, old[l])

        def calls():
            y1 = eng.forward(x.k[1], x.q, x.projs, x.u[1], new_doc=False)     # program order: this step uses the OLD override
            env.step()
            env.host_mark()
            for l in range(pt.L):
                setter(l, new[l])
            y2 = eng.forward(x.k[2], x.q, x.projs, x.u[2], new_doc=False)     # ... and this one the new
            env.step()
            env.out(ctx1=y1, ctx2=y2)
            ltm_state(env, eng)
        return pre, calls
    return make


SCENARIOS["ltm_set_bins_between_forwards"] = _setter("bins")
SCENARIOS["ltm_set_probs_between_forwards"] = _setter("probs")


def _two_engines(consolidate):
    def make(env):
        pt = st.SMALL
        env.lanes = 2
        n = 70 if consolidate else 3
        engs = [ltm_engine(pt, max_batch_chunks=32) for _ in range(2)]
        xs = [LtmIn(env, pt, n, video=i, lane=i) for i in range(2)]

        def calls():
            if consolidate:
                for i in range(2):
                    with env.lane(i):
                        env.out(**{f"e{i}_ctx": engs[i].consolidate(xs[i].k, xs[i].q, xs[i].projs, xs[i].u, new_doc=True)})
                    env.step()
            else:
                for c in range(n):
                    for i in range(2):
                        with env.lane(i):
                            y = engs[i].forward(xs[i].k[c], xs[i].q, xs[i].projs, xs[i].u[c] if c else None, new_doc=(c == 0))
                            env.out(**{f"e{i}_ctx{c}": y})
                        env.step()
            for i in range(2):
                with env.lane(i):
                    ltm_state(env, engs[i], f"e{i}_")
        return calls
    return make


SCENARIOS["ltm_two_engines_forward"] = _two_engines(False)
SCENARIOS["ltm_two_engines_consolidate"] = _two_engines(True)


# ------------------------------------------------------------------------------------------------ the drop-in module
def _module(layer):
    from infinite_video_amd.long_term_attention_gibbs import LongTermAttention
    pt = st.SMALL
    wk, bk, wv, bv = st.projections(2, pt.d, pt.dm, False)[layer]

    def linear(w, b):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        lin.weight.copy_(torch.from_numpy(w))
        lin.bias.copy_(torch.from_numpy(b))
        return lin.to(dev0())
    # constructor kwargs as the reference Q-former passes them (Qformer.py:135-158)
    return LongTermAttention(head_size=64, length=pt.d, target_len=pt.d, attn_func="softmax", attn_num_basis=pt.N, continuous=True,
                             attn_drop=0.1, infinite_memory=True, n_layers=2, n_heads=pt.H, affines=True, mask=True, mask_type="cnn",
                             kl_regularizer=False, proj_key=linear(wk, bk), proj_value=linear(wv, bv), sigma_0=None, mu_0=None,
                             sticky_memories=True, sigmas=None, tau=pt.tau, d_model=pt.dm)


def _module_inputs(env, n_chunks, n_q):
    pt = st.SMALL
    kg, kd = st.tokens(n_chunks, pt.T, pt.P, pt.d, False), st.tokens(n_chunks, pt.T, pt.P, pt.d, True)
    ks = [env.inp(kg[c][None], kd[c][None]) for c in range(n_chunks)]           # one tensor per chunk: the pool cache keys on identity
    qg, qd = st.queries(n_q, pt.Q, pt.dm, False), st.queries(n_q, pt.Q, pt.dm, True)
    qs = [env.inp(qg[l][None], qd[l][None]) for l in range(n_q)]
    return ks, qs


def _module_state(env, m, tag=""):
    ltm_state(env, m._engine, tag)


@scenario("dropin_80_forwards")
def _(env):
    """80 sticky forwards behind one delay: more than the 64 pinned slots of Gibbs uniforms.  The forward that is about to rewrite
    the first slot of a group waits on the host for that group's event (by design), so the issue time is taken over the calls before
    the first such wait."""
    m = _module(0)
    ks, qs = _module_inputs(env, 4, 1)

    def calls():
        torch.manual_seed(20261021)                              # the uniforms come from torch's global CPU generator
        ys = []
        for i in range(80):
            if i == 48:                                          # (well before any slot of this run is reused)
                env.host_mark()
            ys.append(m(ks[i % 4], qs[0], new_doc=(i == 0), layer_n=0))
            env.step()
        env.out(ctx=torch.cat(ys))
        _module_state(env, m)
    return calls


@scenario("dropin_pool_cache_pair")
def _(env):
    ma, mb = _module(0), _module(1)
    ks, qs = _module_inputs(env, 3, 2)

    def calls():
        torch.manual_seed(7)
        ya, yb = [], []
        for c in range(3):
            ya.append(ma(ks[c], qs[0], new_doc=(c == 0), layer_n=0))      # pools ks[c]
            env.step()
            yb.append(mb(ks[c], qs[1], new_doc=(c == 0), layer_n=1))      # steps from the cached frame means
            env.step()
        env.out(ctxA=torch.cat(ya), ctxB=torch.cat(yb))
        _module_state(env, ma, "a_")
        _module_state(env, mb, "b_")
    return calls


# ------------------------------------------------------------------------------------------------ the video Q-former (raw ABI)
class VqfRig:
    """A video Q-former handle at ``seam_cases.VQF_BASE`` with every weight tensor poisoned and one one-layer engine per video and
    layer."""

    def __init__(self, env, n_videos=1, token_dtype=torch.float32):
        from infinite_video_amd.engine import LTMEngine
        s = self.s = sm.VQF_BASE
        self.env, self.lib = env, _lib.load()
        wg, wd = st.vqf_weights(False), st.vqf_weights(True)
        w = self.w = {k: env.inp(np.asarray(wg[k], np.float32), np.asarray(wd[k], np.float32)) for k in wg}
        lin = lambda name: _lib.Linear(w[name + ".weight"].data_ptr(), w[name + ".bias"].data_ptr())
        ln = lambda name: _lib.LayerNorm(w[name + ".weight"].data_ptr(), w[name + ".bias"].data_ptr())
        ws = self.ws = _lib.VqfWeights()
        ws.query_tokens = w["video_query_tokens"].data_ptr()
        ws.emb_ln = ln("bert.embeddings.LayerNorm")
        for l in range(s["n_layers"]):
            p = f"bert.encoder.layer.{l}."
            a, x = p + "attention.", p + "crossattention."
            ws.layer[l] = _lib.VqfLayer(lin(a + "self.query"), lin(a + "self.key"), lin(a + "self.value"), lin(a + "output.dense"),
                                        ln(a + "output.LayerNorm"), lin(x + "self.query"), lin(x + "self.key"), lin(x + "self.value"),
                                        lin(x + "output.dense"), ln(x + "output.LayerNorm"), lin(p + "intermediate_query.dense"),
                                        lin(p + "output_query.dense"), ln(p + "output_query.LayerNorm"))
        ws.llama_proj = lin("llama_proj")
        cfg = _lib.VqfConfig(n_layers=s["n_layers"], n_heads=s["heads"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                             tokens_per_frame=s["P"], n_query=s["n_query"], proj_out=s["proj"], nb_samples=S, alpha=s["alpha"], ln_eps=1e-12)
        self.h = C.c_void_p()
        _lib.check(self.lib.infv_vqf_create(C.byref(cfg), C.byref(self.h)))
        env.cleanup(lambda: self.lib.infv_vqf_destroy(self.h))
        self.dtype = token_dtype
        if token_dtype != torch.float32:
            _lib.check(self.lib.infv_vqf_set_token_dtype(self.h, {torch.bfloat16: 1, torch.float16: 3}[token_dtype]))
        L = s["n_layers"]
        self.engs = [LTMEngine(s["N"], s["heads"], 64, s["enc_width"], s["P"], tau=s["tau"], sticky=s["sticky"], n_layers=1,
                               max_q=s["n_query"], device=env.dev) for _ in range(n_videos * L)]
        for e in self.engs:
            e.ensure_plan(s["T"])
        self.handles = (C.c_void_p * (n_videos * L))(*[e._h.value for e in self.engs])

    def inputs(self, n_chunks):
        s = self.s
        self.frames = self.env.inp(st.tokens(n_chunks, s["T"], s["P"], s["enc_width"], False, 3),
                                   st.tokens(n_chunks, s["T"], s["P"], s["enc_width"], True, 3), self.dtype)
        self.u = self.env.inp(st.uniforms(n_chunks, s["n_layers"], S, False, 3), st.uniforms(n_chunks, s["n_layers"], S, True, 3))

    def outputs(self, n_chunks, n_videos=1):
        s, d = self.s, self.env.dev
        return (torch.empty(n_chunks, s["n_query"], s["hidden"], device=d), torch.empty(n_chunks, s["n_query"], s["proj"], device=d),
                torch.empty(n_videos, s["n_query"], s["proj"], device=d))

    def state(self):
        for i, e in enumerate(self.engs):
            ltm_state(self.env, e, f"m{i}_")


def _vqf_chunks(n_chunks, epoch):
    def make(env):
        r = VqfRig(env)
        r.inputs(n_chunks)

        def calls():
            if epoch:                                            # the weights changed (they were poisoned): a new epoch for this run
                _lib.check(r.lib.infv_vqf_set_weights_epoch(r.h, C.c_uint64(1000 + env.run_index)))
            hidden, llama, _ = r.outputs(n_chunks)
            for c in range(n_chunks):
                _lib.check(r.lib.infv_vqf_encode_chunk(r.h, r.handles, r.frames[c].data_ptr(), r.s["T"], C.byref(r.ws),
                                                       r.u[c].data_ptr() if c else None, int(c == 0), hidden[c].data_ptr(), llama[c].data_ptr(),
                                                       cur_stream()))
                env.step()
            env.out(hidden=hidden, llama=llama)
            r.state()
        return calls
    return make


SCENARIOS["vqf_encode_chunk_twice"] = _vqf_chunks(2, False)
SCENARIOS["vqf_encode_chunk_epoch"] = _vqf_chunks(3, True)


def _vqf_video(dtype):
    def make(env):
        r = VqfRig(env, token_dtype=dtype)
        r.inputs(6)

        def calls():
            hidden, llama, mean = r.outputs(6)
            _lib.check(r.lib.infv_vqf_encode_video(r.h, r.handles, r.frames.data_ptr(), 6, r.s["T"], C.byref(r.ws), r.u.data_ptr(), 1,
                                                   hidden.data_ptr(), llama.data_ptr(), mean.data_ptr(), cur_stream()))
            env.step()
            env.out(hidden=hidden, llama=llama, mean=mean)
            r.state()
        return calls
    return make


SCENARIOS["vqf_encode_video_6"] = _vqf_video(torch.float32)
SCENARIOS["vqf_encode_video_bf16"] = _vqf_video(torch.bfloat16)


@scenario("vqf_encode_videos_3")
def _(env):
    counts = st.VQF_RAGGED
    r = VqfRig(env, n_videos=len(counts))
    total = sum(counts)
    r.inputs(total)
    cu = (C.c_int32 * (len(counts) + 1))(0, *np.cumsum(counts).tolist())

    def calls():
        hidden, llama, mean = r.outputs(total, len(counts))
        _lib.check(r.lib.infv_vqf_encode_videos(r.h, r.handles, len(counts), C.cast(cu, C.c_void_p), r.frames.data_ptr(), r.s["T"], C.byref(r.ws),
                                                r.u.data_ptr(), 1, hidden.data_ptr(), llama.data_ptr(), mean.data_ptr(), cur_stream()))
        env.step()
        env.out(hidden=hidden, llama=llama, mean=mean)
        r.state()
    return calls


@scenario("vqf_short_attention")
def _(env):
    s = sm.VQF_BASE
    lib = _lib.load()
    nt, Q, hid, dw = 96, s["n_query"], s["hidden"], s["enc_width"]
    both = lambda shape, i, scale=1.0: (st.normal(shape, False, i, scale), st.normal(shape, True, i, scale))
    frames, xq, along = env.inp(*both((nt, dw), 1)), env.inp(*both((Q, hid), 2)), env.inp(*both((Q, hid), 3))
    wk, bk, wv, bv = (env.inp(*both(sh, 4 + i, 0.02)) for i, sh in enumerate(((hid, dw), (hid,), (hid, dw), (hid,))))
    cfg = _lib.VqfConfig(n_layers=2, n_heads=s["heads"], hidden=hid, inter=hid, enc_width=dw, tokens_per_frame=32, n_query=Q, proj_out=64,
                         nb_samples=S, alpha=s["alpha"], ln_eps=1e-12)
    h = C.c_void_p()
    _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
    env.cleanup(lambda: lib.infv_vqf_destroy(h))
    key, val = _lib.Linear(wk.data_ptr(), bk.data_ptr()), _lib.Linear(wv.data_ptr(), bv.data_ptr())

    def calls():
        out = torch.empty(Q, hid, device=env.dev)
        _lib.check(lib.infv_vqf_short_attention(h, frames.data_ptr(), nt, xq.data_ptr(), C.byref(key), C.byref(val), along.data_ptr(),
                                                out.data_ptr(), cur_stream()))
        env.step()
        env.out(merged=out)
    return calls


@scenario("vqf_mean")
def _(env):
    lib = _lib.load()
    x = env.inp(st.normal((5, 4096), False, 20), st.normal((5, 4096), True, 20))

    def calls():
        out = torch.empty(4096, device=env.dev)
        _lib.check(lib.infv_vqf_mean(x.data_ptr(), 5, 4096, out.data_ptr(), cur_stream()))
        env.step()
        env.out(mean=out)
    return calls


@scenario("vqf_self_attention")
def _(env):
    lib = _lib.load()
    H, nb, n_max = 2, 4, 65
    cfg = _lib.VqfConfig(1, H, 64 * H, 64 * H, 64, 4, 32, 0, S, 1.0, 1e-12)
    h = C.c_void_p()
    _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
    env.cleanup(lambda: lib.infv_vqf_destroy(h))
    qkv = env.inp(st.normal((nb, n_max, 3 * 64 * H), False, 21), st.normal((nb, n_max, 3 * 64 * H), True, 21))
    nv = (C.c_int32 * nb)(65, 1, 33, 64)

    def calls():
        ctx = torch.zeros(nb, n_max, 64 * H, device=env.dev)
        _lib.check(lib.infv_vqf_self_attention(h, qkv.data_ptr(), nb, n_max, C.cast(nv, C.c_void_p), ctx.data_ptr(), cur_stream()))
        env.step()
        env.out(ctx=ctx)
    return calls


# ------------------------------------------------------------------------------------------------ VideoChat2 (raw ABI on the module's handle)
IDS = ([0, 49, 7, 7, 23], [], [49, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0, 7, 48])
IDS_B = ([5, 5, 48], [1, 2, 3, 4, 5, 6, 7], [9])


def vc_model(decoy, front):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    from tests.test_vc_encode_img_cpu import MAX_POS, VOCAB, front_weights
    s = sm.BASE
    kw = dict(vocab_size=VOCAB, max_position_embeddings=MAX_POS, vision_layernorm=True) if front else {}
    m = VideoChat2Encoder(32, s["n_query"] - 32, s["enc_width"], s["proj"], s["N"], s["sticky"], s["tau"], s["alpha"], s["n_layers"],
                          s["cross_freq"], hidden_size=s["hidden"], intermediate_size=s["inter"], num_attention_heads=s["heads"],
                          tokens_per_frame=s["P"], **kw)
    w = st.vc_weights(decoy)
    m.load_reference_state_dict(dict(w, **front_weights(s, seed=5 + (st.DECOY if decoy else 0))) if front else w)
    return m.to(dev0()).eval()


def poisoned_module(env, good, decoy):
    """``good`` with every parameter registered as a poisoned input (its decoy: the same parameter of ``decoy``)."""
    for (n, p), (n2, pd) in zip(good.named_parameters(), decoy.named_parameters()):
        assert n == n2 and p.shape == pd.shape
        env.inp(p.detach().clone(), pd.detach(), into=p)
    return good


class VcRig:
    def __init__(self, env, counts, texts, dtype=torch.float32, front=False, blocks=None, src=None):
        from infinite_video_amd.videochat2_qformer import VideoChat2Memory
        s = self.s = sm.BASE
        self.env, self.lib = env, _lib.load()
        self.m = poisoned_module(env, vc_model(False, front), vc_model(True, front))
        self.counts, self.texts, self.src = counts, texts, src
        self.blocks = blocks if blocks is not None else counts               # chunks of every distinct block of frame tokens
        V, self.nx, self.Q = len(counts), sm.n_cross_of(s), s["n_query"]
        self.total, n_tok = sum(counts), sum(self.blocks)
        self.code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}[dtype]
        self.frames = env.inp(st.tokens(n_tok, s["T"], s["P"], s["enc_width"], False, 4), st.tokens(n_tok, s["T"], s["P"], s["enc_width"], True, 4), dtype)
        self.u = env.inp(st.uniforms(self.total, self.nx, S, False, 4), st.uniforms(self.total, self.nx, S, True, 4))
        rows = lambda w: np.concatenate([sm.small_video(s, v, 0, t, w)[1] for v, t in enumerate(texts)])
        self.hin = None if front else env.inp(rows(st.vc_weights(False)), rows(st.vc_weights(True)))
        self.mems = [VideoChat2Memory(self.m, env.dev) for _ in counts]
        self.handles = (C.c_void_p * (V * self.nx))()
        for v, mem in enumerate(self.mems):
            for j, e in enumerate(mem.engines):
                e.ensure_plan(s["T"])
                self.handles[v * self.nx + j] = e._h
        self.h = self.m._vc_handle(env.dev)
        self.cu = (C.c_int32 * (V + 1))(0, *np.cumsum(counts).tolist())
        self.tl = (C.c_int32 * V)(*texts)
        self.fcu = (C.c_int32 * (len(self.blocks) + 1))(0, *np.cumsum(self.blocks).tolist())
        self.srcs = (C.c_int32 * V)(*src) if src is not None else None

    def call(self, fn, front=None):
        """One raw call of ``fn`` into fresh output buffers; returns (hidden, proj, mean)."""
        s, d, env = self.s, self.env.dev, self.env
        V = len(self.counts)
        rows = sum(n * (self.Q + t) for n, t in zip(self.counts, self.texts))
        hidden, proj = torch.zeros(rows, s["hidden"], device=d), torch.zeros(self.total, self.Q, s["proj"], device=d)
        mean = torch.zeros(V, self.Q, s["proj"], device=d)
        wts, keep = self.m._vc_weights(d)
        env.keep.append(keep)
        head = [self.h, self.handles, V, C.cast(self.cu, C.c_void_p), self.frames.data_ptr()]
        tok = [self.code] if fn.endswith(("_tok", "_img")) else []
        blocks = [len(self.blocks), C.cast(self.fcu, C.c_void_p), C.cast(self.srcs, C.c_void_p) if self.srcs is not None else None] \
            if "streams" in fn else ([0, None, None] if fn.endswith("_img") else [])
        fr = [C.byref(front)] if fn.endswith("_img") else []
        tail = [self.hin.data_ptr() if self.hin is not None else None, C.cast(self.tl, C.c_void_p), self.u.data_ptr(), 1, hidden.data_ptr(),
                proj.data_ptr(), mean.data_ptr(), cur_stream()]
        _lib.check(getattr(self.lib, fn)(*head, *tok, *blocks, s["T"], C.byref(wts), *fr, *tail))
        # (the mean row of a video without chunks is undefined and not read; slices, not an index list: that would be a host-to-device copy)
        return hidden, proj, torch.cat([mean[v:v + 1] for v, n in enumerate(self.counts) if n])

    def state(self):
        for v, mem in enumerate(self.mems):
            if self.counts[v]:
                for j, e in enumerate(mem.engines):
                    ltm_state(self.env, e, f"v{v}x{j}_")


def _vc(fn, dtype=torch.float32, streams=False):
    def make(env):
        if streams:
            r = VcRig(env, (3, 3), (5, 17), dtype, blocks=(3,), src=(0, 0))
        else:
            r = VcRig(env, sm.BASE["counts"], sm.BASE["texts"], dtype)

        def calls():
            hidden, proj, mean = r.call(fn)
            env.step()
            env.out(hidden=hidden, proj=proj, mean=mean)
            r.state()
        return calls
    return make


SCENARIOS["vc_encode_videos"] = _vc("infv_vqf_vc_encode_videos")
SCENARIOS["vc_encode_streams"] = _vc("infv_vqf_vc_encode_streams", streams=True)
SCENARIOS["vc_encode_videos_tok_f16"] = _vc("infv_vqf_vc_encode_videos_tok", torch.float16)
SCENARIOS["vc_encode_streams_tok_f16"] = _vc("infv_vqf_vc_encode_streams_tok", torch.float16, streams=True)


@scenario("vc_encode_img_f16")
def _(env):
    r = VcRig(env, sm.BASE["counts"], tuple(len(x) for x in IDS), torch.float16, front=True)

    def calls():
        front, keep = r.m._front(env.dev, True, [list(x) for x in IDS])
        env.keep.append(keep)
        hidden, proj, mean = r.call("infv_vqf_vc_encode_img", front)
        env.step()
        env.out(hidden=hidden, proj=proj, mean=mean)
        r.state()
    return calls


@scenario("vc_embed_twice")
def _(env):
    """Two embedding calls with different ids behind one delay.  The second call waits on the host for ev_ids (the first call's copy
    out of the pinned staging buffer) before it rewrites the buffer, so the issue time is taken up to it."""
    m = poisoned_module(env, vc_model(False, True), vc_model(True, True))

    def calls():
        a = m.embed_instructions([torch.tensor(x, dtype=torch.int64) for x in IDS], env.dev)
        env.step()
        env.host_mark()
        b = m.embed_instructions([torch.tensor(x, dtype=torch.int64) for x in IDS_B], env.dev)
        env.step()
        env.out(rowsA=torch.cat(a), rowsB=torch.cat(b))
    return calls


@scenario("vc_layernorm_two_streams")
def _(env):
    lib = _lib.load()
    env.lanes = 2
    d = 64
    rows = (37, 300)
    both = lambda shape, i, scale=1.0: (st.normal(shape, False, i, scale), st.normal(shape, True, i, scale))
    xs = [env.inp(*both((rows[i], d), 30 + i), lane=i) for i in range(2)]
    gs = [env.inp(*(1.0 + a for a in both((d,), 32 + i, 0.1)), lane=i) for i in range(2)]
    bs = [env.inp(*both((d,), 34 + i, 0.1), lane=i) for i in range(2)]

    def calls():
        for r in range(2):
            for i in range(2):
                with env.lane(i):
                    out = torch.empty(rows[i], d, device=env.dev)
                    _lib.check(lib.infv_vqf_layernorm_tokens(xs[i].data_ptr(), 0, rows[i], d, gs[i].data_ptr(), bs[i].data_ptr(), 1e-5,
                                                             out.data_ptr(), cur_stream()))
                    env.out(**{f"ln{i}_{r}": out})
                env.step()
    return calls


@scenario("vc_token_pass")
def _(env):
    lib = _lib.load()
    nb, P, T, d = 3, 4, 16, 64
    n = P * T
    frames = env.inp(st.tokens(nb, T, P, d, False, 6), st.tokens(nb, T, P, d, True, 6), torch.float16)

    def calls():
        planes = [torch.zeros(nb * n * d, dtype=torch.bfloat16, device=env.dev) for _ in range(4)]
        kbar = torch.zeros(nb, T, d, device=env.dev)
        _lib.check(lib.infv_vqf_token_pass(frames.data_ptr(), 3, nb, n, d, P, *[p.data_ptr() for p in planes], kbar.data_ptr(), cur_stream()))
        env.step()
        env.out(Fh=planes[0], Fl=planes[1], Th=planes[2], Tl=planes[3], kbar=kbar)
    return calls


# ------------------------------------------------------------------------------------------------ the frame Q-former
def frame_model(decoy, lin="fp32", attn="fp32"):
    from infinite_video_amd.frame_qformer import FrameQformerEncoder
    sh = FRAME_SMALL
    m = FrameQformerEncoder(num_query_token=sh["n_query"], vision_width=sh["enc_width"], num_hidden_layers=sh["n_layers"], hidden_size=sh["hidden"],
                            intermediate_size=sh["inter"], num_attention_heads=sh["n_heads"], linear_precision=lin, attention_precision=attn,
                            vision_layernorm=True)
    m.load_reference_state_dict(st.frame_weights(decoy))
    return m.to(dev0()).eval()


def _frame(lin="fp32", attn="fp32", n_calls=1, tap=None, poison_weights=True):
    """``poison_weights=False``: the reduced precisions cache their weight planes under a weights epoch, a change of weights is a new
    epoch, and the first call of a new epoch allocates its planes, which synchronises the device -- no call can be queued behind a
    delay across it.  The warm run builds the planes; both calls under test reuse them."""
    def make(env):
        sh = FRAME_SMALL
        m = poisoned_module(env, frame_model(False, lin, attn), frame_model(True, lin, attn)) if poison_weights else frame_model(False, lin, attn)
        xs = [env.inp(st.vision(3, False)[::(1 if i == 0 else -1)].copy(), st.vision(3, True)[::(1 if i == 0 else -1)].copy()) for i in range(n_calls)]
        lib = _lib.load()

        def calls():
            for i, x in enumerate(xs):
                dst = None
                if tap is not None:
                    dst = torch.zeros(3, sh["n_query"], sh["hidden"], device=env.dev)
                    _lib.check(lib.infv_vqf_set_context_tap(m._handle(env.dev), tap, dst.data_ptr()))
                y = m.encode_frames(x)
                env.step()
                env.out(**{f"hidden{i}": y})
                if dst is not None:
                    env.out(**{f"tap{i}": dst})
        return calls
    return make


SCENARIOS["frame_encode_fp32"] = _frame()
SCENARIOS["frame_encode_split_bf16"] = _frame("split_bf16", "fp32", 2, poison_weights=False)
SCENARIOS["frame_encode_fp16"] = _frame("fp16", "fp16", 2, poison_weights=False)
SCENARIOS["frame_context_tap"] = _frame(tap=2)


def _frame_handle(env):
    sh = FRAME_SMALL
    lib = _lib.load()
    cfg = _lib.VqfConfig(1, sh["n_heads"], sh["hidden"], sh["inter"], sh["enc_width"], 1, sh["n_query"], 0, S, 1.0, 1e-12)
    h = C.c_void_p()
    _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
    env.cleanup(lambda: lib.infv_vqf_destroy(h))
    return lib, h


@scenario("frame_linear")
def _(env):
    lib, h = _frame_handle(env)
    M, K, n_out = 70, 128, 128
    both = lambda shape, i, scale=1.0: (st.normal(shape, False, i, scale), st.normal(shape, True, i, scale))
    x = env.inp(*both((M, K), 40))
    ws = [env.inp(*both((n_out, K), 41 + i, 0.05)) for i in range(2)]
    bs = [env.inp(*both((n_out,), 43 + i, 0.05)) for i in range(2)]
    res = env.inp(*both((M, 2 * n_out), 45))
    g, b = env.inp(*(1.0 + a for a in both((2 * n_out,), 46, 0.1))), env.inp(*both((2 * n_out,), 47, 0.1))
    lin = (_lib.Linear * 2)(*[_lib.Linear(ws[i].data_ptr(), bs[i].data_ptr()) for i in range(2)])
    ln = _lib.LayerNorm(g.data_ptr(), b.data_ptr())

    def calls():
        y = torch.zeros(M, 2 * n_out, device=env.dev)
        _lib.check(lib.infv_vqf_linear(h, x.data_ptr(), M, K, lin, 2, n_out, 1, res.data_ptr(), M, C.byref(ln), y.data_ptr(), cur_stream()))
        env.step()
        env.out(y=y)
    return calls


@scenario("frame_cross_attention")
def _(env):
    lib, h = _frame_handle(env)
    sh = FRAME_SMALL
    F_, Q, hid, dw = 3, sh["n_query"], sh["hidden"], sh["enc_width"]
    both = lambda shape, i, scale=1.0: (st.normal(shape, False, i, scale), st.normal(shape, True, i, scale))
    vis = env.inp(st.vision(F_, False), st.vision(F_, True))
    xq = env.inp(*both((F_, Q, hid), 50))
    wk, wv, bv = env.inp(*both((hid, dw), 51, 0.05)), env.inp(*both((hid, dw), 52, 0.05)), env.inp(*both((hid,), 53, 0.05))
    g, b = env.inp(*(1.0 + a for a in both((dw,), 54, 0.1))), env.inp(*both((dw,), 55, 0.1))
    key, value = _lib.Linear(wk.data_ptr(), None), _lib.Linear(wv.data_ptr(), bv.data_ptr())
    ln = _lib.VqfVisionLn(g.data_ptr(), b.data_ptr(), LN_VISION_EPS)

    def calls():
        ctx = torch.zeros(F_, Q, hid, device=env.dev)
        _lib.check(lib.infv_vqf_frame_cross_attention(h, F_, vis.data_ptr(), 0, st.FRAME_TOKENS, C.byref(ln), xq.data_ptr(), C.byref(key),
                                                      C.byref(value), ctx.data_ptr(), cur_stream()))
        env.step()
        env.out(ctx=ctx)
    return calls
