"""The batched Q-former calls across their launch-group and row-block seams (tests/golden/seam_cases.py has the layouts,
tests/test_call_seams_cpu.py shows that each one crosses what it claims): one big call per layout through the raw C ABI into
NaN-filled outputs; the probes and a fixed spread of other videos re-run alone (V = 1) on fresh memories must give the same bits;
the probes must agree with the CPU oracle on both sides of every seam, draws included; every row that belongs to a chunk must
have been written.  ``infv_vqf_self_attention`` is taken past one length/offset table on its own.  Needs a real MI355X: run with
``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import record_parity
from tests.golden import seam_cases as sc
from tests.test_vc_videos_gpu import ATOL, _att_handle, _att_ref, _att_run, armed, memory_bits, same_bits, small_setup, traced_bins

pytestmark = pytest.mark.gpu
B_TOL = 2e-5             # the project's bound on B (tests/test_config_sweep_gpu.py)
K = sc.seam_constants()


def dev0():
    return torch.device("cuda:0")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Memories:
    """One video's one-layer engines (what ``memory_bits`` / ``armed`` read of a ``VideoChat2Memory``)."""

    def __init__(self, engines):
        self.engines = engines


# ------------------------------------------------------------------------------------------------ the two encoders, raw
class VcCaller:
    """``infv_vqf_vc_encode_videos`` on a ``VideoChat2Encoder``'s handle and weights, into NaN-filled outputs."""

    def __init__(self, lay, dev):
        self.lay, self.dev = lay, dev
        self.s, self.w, self.m = small_setup(dev, **{a: b for a, b in lay.shape.items() if a not in ("texts", "counts")})

    def memories(self):
        from infinite_video_amd.videochat2_qformer import VideoChat2Memory
        return VideoChat2Memory(self.m, self.dev)

    def __call__(self, vids, text_len, u, mems):
        """vids [(chunks, encoder input rows)]; returns per video (proj, mean or None, hidden) on the host and the raw outputs."""
        from infinite_video_amd import _lib
        s, m, dev = self.s, self.m, self.dev
        V, Q, Hd, nx = len(vids), s["n_query"], s["hidden"], sc.n_cross_of(s)
        counts = [len(k) for k, _ in vids]
        total = sum(counts)
        frames = torch.from_numpy(np.concatenate([k for k, _ in vids])).to(dev)
        hin = torch.from_numpy(np.concatenate([h for _, h in vids])).to(dev)
        ud = torch.from_numpy(u).to(dev)
        assert tuple(ud.shape) == (total, nx, sc.S) and [len(h) - Q for _, h in vids] == list(text_len)
        handles = (C.c_void_p * (V * nx))()
        for v, mem in enumerate(mems):
            for j, e in enumerate(mem.engines):
                e.ensure_plan(s["T"])
                handles[v * nx + j] = e._h
        rows = sum(n * (Q + t) for n, t in zip(counts, text_len))
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        hidden, proj, mean = nan(rows, Hd), nan(total, Q, s["proj"]), nan(V, Q, s["proj"])
        cu = (C.c_int32 * (V + 1))(0, *np.cumsum(counts).tolist())
        tl = (C.c_int32 * V)(*text_len)
        wts, keep = m._vc_weights(dev)
        with torch.cuda.device(dev):
            rc = _lib.load().infv_vqf_vc_encode_videos(
                m._vc_handle(dev), handles, V, C.cast(cu, C.c_void_p), C.c_void_p(frames.data_ptr()), s["T"], C.byref(wts),
                C.c_void_p(hin.data_ptr()), C.cast(tl, C.c_void_p), C.c_void_p(ud.data_ptr()), 1,
                C.c_void_p(hidden.data_ptr()) if self.lay.want_hidden else None, C.c_void_p(proj.data_ptr()),
                C.c_void_p(mean.data_ptr()), _stream(dev))
        torch.cuda.synchronize()
        del keep
        assert rc == 0, _lib.load().infv_ltm_last_error()
        proj, mean, hidden = proj.cpu(), mean.cpu(), hidden.cpu()
        out, c0, r0 = [], 0, 0
        for v, (n, t) in enumerate(zip(counts, text_len)):
            out.append((proj[c0:c0 + n], mean[v] if n else None, hidden[r0:r0 + n * (Q + t)].view(n, Q + t, Hd)))
            c0, r0 = c0 + n, r0 + n * (Q + t)
        return out, (proj, hidden)


class VqfCaller:
    """``infv_vqf_encode_videos`` on a handle of its own, one one-layer ``LTMEngine`` per video and layer."""

    def __init__(self, lay, dev):
        from infinite_video_amd import _lib
        from tests.test_config_sweep_gpu import _vqf_weights_struct
        self.lay, self.dev, self.s = lay, dev, lay.shape
        s = self.s
        self.w = sc.layout_weights(lay)
        self.ws, self.keep = _vqf_weights_struct(self.w, s["n_layers"], dev)
        cfg = _lib.VqfConfig(n_layers=s["n_layers"], n_heads=s["heads"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                             tokens_per_frame=s["P"], n_query=s["n_query"], proj_out=s["proj"], nb_samples=sc.S, alpha=s["alpha"],
                             ln_eps=1e-12)
        self.h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().infv_vqf_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        from infinite_video_amd import _lib
        _lib.load().infv_vqf_destroy(self.h)

    def memories(self):
        from infinite_video_amd.engine import LTMEngine
        s = self.s
        return Memories([LTMEngine(s["N"], s["heads"], 64, s["enc_width"], s["P"], tau=s["tau"], sticky=s["sticky"], n_layers=1,
                                   max_q=s["n_query"], device=self.dev) for _ in range(s["n_layers"])])

    def __call__(self, vids, text_len, u, mems):
        from infinite_video_amd import _lib
        s, dev = self.s, self.dev
        V, Q, Hd, L = len(vids), s["n_query"], s["hidden"], s["n_layers"]
        counts = [len(k) for k, _ in vids]
        total = sum(counts)
        frames = torch.from_numpy(np.concatenate([k for k, _ in vids])).to(dev)
        ud = torch.from_numpy(u).to(dev)
        assert tuple(ud.shape) == (total, L, sc.S)
        handles = (C.c_void_p * (V * L))()
        for v, mem in enumerate(mems):
            for l, e in enumerate(mem.engines):
                e.ensure_plan(s["T"])
                handles[v * L + l] = e._h
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        hidden, proj, mean = nan(total, Q, Hd), nan(total, Q, s["proj"]), nan(V, Q, s["proj"])
        cu = (C.c_int32 * (V + 1))(0, *np.cumsum(counts).tolist())
        with torch.cuda.device(dev):
            rc = _lib.load().infv_vqf_encode_videos(
                self.h, handles, V, C.cast(cu, C.c_void_p), C.c_void_p(frames.data_ptr()), s["T"], C.byref(self.ws),
                C.c_void_p(ud.data_ptr()), 1, C.c_void_p(hidden.data_ptr()), C.c_void_p(proj.data_ptr()), C.c_void_p(mean.data_ptr()),
                _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0, _lib.load().infv_ltm_last_error()
        proj, mean, hidden = proj.cpu(), mean.cpu(), hidden.cpu()
        out, c0 = [], 0
        for v, n in enumerate(counts):
            out.append((proj[c0:c0 + n], mean[v] if n else None, hidden[c0:c0 + n]))
            c0 += n
        return out, (proj, hidden)


# ------------------------------------------------------------------------------------------------ one layout
def check_layout(name, caller):
    """The big call of layout ``name``; returns (worst |device - oracle| over the probes, videos compared bit for bit)."""
    lay = caller.lay
    cu, nx = lay.cu, sc.n_cross_of(lay.shape)
    ref = sc.probe_reference(lay)
    u = sc.layout_uniforms(lay)
    vids = [sc.layout_video(lay, v) for v in range(len(lay.counts))]
    if lay.path == "vqf":
        vids = [(k, np.zeros((0, lay.shape["hidden"]), np.float32)) for k, _ in vids]
    mems = [caller.memories() for _ in lay.counts]
    traces = {p: armed(mems[p], lay.counts[p]) for p in lay.probes}
    big, (proj, hidden) = caller(vids, lay.text_len, u, mems)
    # ---- every row that belongs to a chunk was written (proj_mean rows of videos without chunks are undefined: not read)
    assert bool(torch.isfinite(proj).all()), f"{name}: projected rows of chunks {_bad_chunks(proj)} were not written"
    if lay.want_hidden:
        assert bool(torch.isfinite(hidden).all()), f"{name}: hidden rows were not written"
    for v, n in enumerate(lay.counts):
        if n:
            assert bool(torch.isfinite(big[v][1]).all()), f"{name}: mean of video {v} was not written"
    big_bits = {v: memory_bits(mems[v]) for v in lay.probes + sc.spread(lay, K)}
    # ---- against the oracle: the probes, on both sides of the seams
    worst = 0.0
    for p, (orun, _) in ref.items():
        got_p, got_m, got_h = big[p]
        bins = traced_bins(traces[p])
        for c in range(lay.counts[p]):
            tag = f"{name}: probe {p} chunk {c} (chunk {cu[p] + c} of the call)"
            for j, ob in enumerate(orun.bins[c]):
                if ob is not None:
                    assert np.array_equal(bins[c][j], ob), f"{tag}: draws of cross layer {j} differ"
            np.testing.assert_allclose(got_p[c].numpy(), orun.proj[c], rtol=0, atol=ATOL, err_msg=tag + " projected")
            np.testing.assert_allclose(got_h[c].numpy(), orun.hidden[c], rtol=0, atol=ATOL, err_msg=tag + " hidden")
            worst = max(worst, float(np.abs(got_p[c].numpy() - orun.proj[c]).max()), float(np.abs(got_h[c].numpy() - orun.hidden[c]).max()))
        want_mean = np.mean(np.stack(orun.proj), 0)
        np.testing.assert_allclose(got_m.numpy(), want_mean, rtol=0, atol=ATOL, err_msg=f"{name}: mean of probe {p}")
        worst = max(worst, float(np.abs(got_m.numpy() - want_mean).max()))
        for j in range(nx):
            B = big_bits[p][j][0].numpy()
            np.testing.assert_allclose(B, orun.B[j], rtol=0, atol=B_TOL, err_msg=f"{name}: probe {p}: B of cross layer {j}")
    # ---- bit for bit: the probes and the spread, each alone on fresh memories with its own uniforms
    compared = 0
    for v in lay.probes + sc.spread(lay, K):
        assert lay.counts[v] > 0
        mem = caller.memories()
        alone, _ = caller([vids[v]], [lay.text_len[v]], u[cu[v]:cu[v + 1]], [mem])
        same_bits(big[v] + (big_bits[v],), alone[0] + (memory_bits(mem),), f"{name}: video {v} (chunks {cu[v]}..{cu[v + 1] - 1}) vs alone")
        compared += 1
    record_parity(f"call seams {name} ({len(lay.counts)} videos, {lay.n_chunks} chunks; crosses {', '.join(sorted(lay.claims))}): "
                  f"max |device - oracle| over {len(ref)} probes {worst:.3e}, {compared} videos equal their run alone bit for bit")
    return worst, compared


def _bad_chunks(proj):
    bad = (~torch.isfinite(proj)).flatten(1).any(1).nonzero().flatten().tolist()
    return bad[:8]


@pytest.mark.parametrize("name", ["vc_video_groups", "vc_text_ffn", "vc_merge"])
def test_vc_encode_videos_across_seams(name):
    check_layout(name, VcCaller(sc.LAYOUTS[name], dev0()))


def test_vc_row_blocks_then_a_smaller_call_on_the_same_handle():
    """The row-block layout, then the BASE 3-video call on the same module: the same bits as a fresh module gives (stale
    workspace contents behind the smaller call's rows and workspaces that do not grow are harmless)."""
    dev = dev0()
    caller = VcCaller(sc.LAYOUTS["vc_row_blocks"], dev)
    check_layout("vc_row_blocks", caller)
    s = caller.s
    vids = [sc.small_video(s, v, n, t, caller.w) for v, (n, t) in enumerate(zip(sc.BASE["counts"], sc.BASE["texts"]))]
    u = np.random.default_rng(31).random((sum(sc.BASE["counts"]), sc.n_cross_of(s), sc.S))
    fresh = VcCaller(sc.LAYOUTS["vc_row_blocks"], dev)
    assert fresh.m is not caller.m
    res = []
    for who in (caller, fresh):
        mems = [who.memories() for _ in vids]
        out, _ = who(vids, list(sc.BASE["texts"]), u, mems)
        res.append([(o, memory_bits(mem) if len(k) else None) for o, mem, (k, _) in zip(out, mems, vids)])   # (no chunk: no memory)
    for v, n in enumerate(sc.BASE["counts"]):
        if n:
            same_bits(res[0][v][0] + (res[0][v][1],), res[1][v][0] + (res[1][v][1],), f"after the large call: video {v}")
    record_parity("call seams: the BASE 3-video call after the 301-chunk call on the same handle equals a fresh module's bit for bit")


@pytest.mark.parametrize("name", ["vqf_blocks_groups", "vqf_merge"])
def test_vqf_encode_videos_across_seams(name):
    caller = VqfCaller(sc.LAYOUTS[name], dev0())
    try:
        check_layout(name, caller)
    finally:
        caller.close()


# ------------------------------------------------------------------------------------------------ the attention table
def test_self_attention_past_one_length_table():
    """nb = 258 chunks in one call (two launches with their own tables and rebased bases): chunks 0, 255, 256 and 257 equal their
    nb = 1 runs bit for bit, every chunk keeps test_self_attention_kernel_against_fp64's bound (max |err| vs fp64 at most 4x
    torch-fp32's own), rows past n_valid are zero and never read (they hold NaN)."""
    from infinite_video_amd import _lib
    a = sc.ATTN
    H, nb, n_max = a["H"], a["nb"], a["n_max"]
    dev = dev0()
    h = _att_handle(H, dev)
    try:
        gen = torch.Generator().manual_seed(258)
        qkv = torch.randn(nb, n_max, 3 * 64 * H, generator=gen)
        lens = [a["n_valid_cycle"][b % len(a["n_valid_cycle"])] for b in range(nb)]
        poisoned = qkv.clone()
        for b, n in enumerate(lens):
            poisoned[b, n:] = float("nan")                     # a key beyond the valid length that is read shows as NaN
        rc, ctx = _att_run(h, poisoned.to(dev), lens)
        assert rc == 0
        ctx = ctx.cpu()
        worst = 0.0
        for b, n in enumerate(lens):
            got = ctx[b]
            assert bool(torch.isfinite(got).all()), f"chunk {b}: rows not written, or a row beyond n_valid was read"
            assert bool((got[n:] == 0).all()), f"chunk {b}: padding rows must be written as zeros"
            ref64 = _att_ref(qkv[b, :n], H, torch.float64)
            err = float((got[:n].double() - ref64).abs().max())
            err_ref = float((_att_ref(qkv[b, :n], H, torch.float32).double() - ref64).abs().max())
            assert err <= 4 * err_ref, (b, n, err, err_ref)
            worst = max(worst, err / max(err_ref, 1e-30))
        for b in a["alone"]:
            n = lens[b]
            rc, one = _att_run(h, qkv[b:b + 1, :n].contiguous().to(dev), None)
            assert rc == 0
            assert torch.equal(one[0].cpu(), ctx[b, :n]), f"chunk {b} (n = {n}) differs from its nb = 1 run"
        record_parity(f"call seams vc_self_attention H={H} nb={nb} n_max={n_max}: worst kernel / torch-fp32 max|err| ratio {worst:.2f} "
                      f"(bound 4), {len(a['alone'])} chunks equal their nb = 1 runs bit for bit")
    finally:
        _lib.load().infv_vqf_destroy(h)
