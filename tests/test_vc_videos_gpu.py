"""The VideoChat2 Q-former layer-major over the packed chunks of many videos (``infv_vqf_self_attention``,
``infv_vqf_vc_encode_videos`` / ``VideoChat2Encoder.encode_videos``): the self-attention kernel alone, the golden video alone
and inside a batch, small shapes against the CPU oracle, batch invariance bit for bit, agreement with the per-chunk binding,
the device rng, refusals and the per-handle fallback.  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from infinite_video_amd import synth
from oracle.ltm_oracle import DenseOracle, inverse_cdf_draw
from oracle.videochat2_oracle import VideoChat2Oracle
from tests.conftest import record_parity
# the small shape, its synthetic videos and the margin-safe oracle runs are shared with the seam tests (one copy)
from tests.golden.seam_cases import (BASE, MARGIN, S, OracleRun, draw_margins, n_cross_of, small_oracle, small_reference,
                                     small_video)
from tests.golden.vc_cases import VC_CASE, chunk_uniforms, load_vc_golden, vc_inputs

pytestmark = pytest.mark.gpu
ATOL = 2e-4              # test_vc_gpu.py's ATOL, DESIGN.md section 5


def dev0():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
ATT_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 104, 160, 608)      # the tile edges and the cap
ATT_TRIPLES = ((1, 608, 33), (31, 32, 104), (63, 64, 65), (160, 608, 1))


def _att_handle(H, dev):
    from infinite_video_amd import _lib
    c = _lib.VqfConfig(1, H, 64 * H, 64 * H, 64, 4, 32, 0, S, 1.0, 1e-12)
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().infv_vqf_create(C.byref(c), C.byref(h)))
    return h


def _att_run(h, qkv, n_valid):
    from infinite_video_amd import _lib
    nb, n_max, w3 = qkv.shape
    ctx = torch.full((nb, n_max, w3 // 3), float("nan"), device=qkv.device)
    nv = None if n_valid is None else (C.c_int32 * nb)(*n_valid)
    rc = _lib.load().infv_vqf_self_attention(h, C.c_void_p(qkv.data_ptr()), nb, n_max, None if nv is None else C.cast(nv, C.c_void_p),
                                             C.c_void_p(ctx.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ctx


def _att_ref(qkv, H, dtype):
    """softmax(Q K^T / 8) V of one chunk's valid rows [n][3 * hidden] on the CPU in ``dtype``."""
    n, hid = qkv.shape[0], qkv.shape[1] // 3
    x = qkv.to(dtype)
    sp = lambda t: t.reshape(n, H, 64).permute(1, 0, 2)
    q, k, v = sp(x[:, :hid]), sp(x[:, hid:2 * hid]), sp(x[:, 2 * hid:])
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / 8.0, dim=-1)
    return torch.matmul(p, v).permute(1, 0, 2).reshape(n, hid)


@pytest.mark.parametrize("H", [1, 12])
def test_self_attention_kernel_against_fp64(H):
    """Bound: the kernel's max error against fp64 is at most 4x the max error of the reference's own arithmetic (torch fp32
    softmax(QK^T/8)V on the CPU) against the same fp64 -- the margin covers a different but fixed summation order."""
    from infinite_video_amd import _lib
    dev = dev0()
    h = _att_handle(H, dev)
    try:
        gen = torch.Generator().manual_seed(100 + H)
        alone = {}
        for n in ATT_LENGTHS:                                  # every length alone, n_valid = NULL
            qkv = torch.randn(1, n, 3 * 64 * H, generator=gen)
            rc, ctx = _att_run(h, qkv.to(dev), None)
            assert rc == 0
            got = ctx[0].cpu()
            ref64 = _att_ref(qkv[0], H, torch.float64)
            err = float((got.double() - ref64).abs().max())
            err_ref = float((_att_ref(qkv[0], H, torch.float32).double() - ref64).abs().max())
            record_parity(f"vc_self_attention H={H} n={n} alone: kernel max|err| {err:.3e}  torch-fp32 max|err| {err_ref:.3e}")
            assert err <= 4 * err_ref, (n, err, err_ref)
            alone[n] = (qkv[0], got)
        for lens in ATT_TRIPLES:                               # nb = 3 with mixed valid lengths, padded to the longest
            n_max = max(lens)
            qkv = torch.randn(3, n_max, 3 * 64 * H, generator=gen)     # (padding rows hold finite junk that must not be read)
            for b, n in enumerate(lens):
                qkv[b, :n] = alone[n][0]
            poisoned = qkv.clone()
            for b, n in enumerate(lens):
                poisoned[b, n:] = float("nan")                 # a key beyond the valid length that is read shows as NaN
            rc, ctx = _att_run(h, poisoned.to(dev), lens)
            assert rc == 0
            for b, n in enumerate(lens):
                got = ctx[b].cpu()
                assert torch.equal(got[:n], alone[n][1]), f"H={H} lens={lens}: chunk {b} (n={n}) differs from its run alone"
                assert bool((got[n:] == 0).all()), "padding rows must be written as zeros"
                ref64 = _att_ref(qkv[b, :n], H, torch.float64)
                err = float((got[:n].double() - ref64).abs().max())
                err_ref = float((_att_ref(qkv[b, :n], H, torch.float32).double() - ref64).abs().max())
                record_parity(f"vc_self_attention H={H} n={n} in {lens}: kernel max|err| {err:.3e}  torch-fp32 max|err| {err_ref:.3e}")
                assert err <= 4 * err_ref
        rc, _ = _att_run(h, torch.zeros(1, 609, 3 * 64 * H, device=dev), None)
        assert rc == -2                                         # INFV_ERR_UNSUPPORTED
        rc, _ = _att_run(h, torch.zeros(2, 8, 3 * 64 * H, device=dev), (8, 9))
        assert rc == -1
    finally:
        _lib.load().infv_vqf_destroy(h)


# ------------------------------------------------------------------------------------------------ oracle-side helpers
def armed(mem, n_chunks):
    return [e.set_trace(n_chunks) if n_chunks else None for e in mem.engines]


def traced_bins(traces):
    """[C][n_cross][S] from the per-engine traces (rows of steps that drew nothing stay -1)."""
    torch.cuda.synchronize()
    per = [t[0][:, 0].cpu().numpy() for t in traces]
    return [[per[j][c] for j in range(len(per))] for c in range(per[0].shape[0])]


def compare_draws(tag, dev_bins, orun):
    """Device draws against the oracle's: equal wherever the oracle's margin is at least MARGIN; tighter draws are compared,
    counted and recorded.  Returns the (chunk, layer) of the first flipped draw, or None."""
    total = tight = flips = 0
    first = None
    for c in range(len(orun.bins)):
        for j, ob in enumerate(orun.bins[c]):
            if ob is None:
                continue
            db, m = dev_bins[c][j], orun.margin[c][j]
            wide = m >= MARGIN
            assert np.array_equal(db[wide], ob[wide]), f"{tag}: chunk {c} cross layer {j}: a draw with margin >= {MARGIN} differs"
            n_flip = int((db[~wide] != ob[~wide]).sum())
            if n_flip and first is None:
                first = (c, j)
            total, tight, flips = total + ob.size, tight + int((~wide).sum()), flips + n_flip
    record_parity(f"{tag}: {total} draws, {tight} with oracle margin < {MARGIN} ({100.0 * tight / max(total, 1):.2f} %), "
                  f"{flips} of those flipped" + (f" (first at chunk {first[0]}, cross layer {first[1]})" if first else ""))
    assert tight <= 0.01 * max(total, 1)
    return first


# ------------------------------------------------------------------------------------------------ 2./3. the golden video
def golden_model(dev, alpha=None):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    case = VC_CASE
    frames, h0, weights = vc_inputs(case)
    m = VideoChat2Encoder(32, case.n_query - 32, case.enc_width, case.proj_out, case.N, case.sticky, case.tau,
                          case.alpha if alpha is None else alpha, case.n_layers, case.cross_freq)
    m.load_reference_state_dict(weights)
    return m.to(dev).eval(), frames, h0, weights


_golden = {}


def golden_reference():
    """The golden video through the oracle, once per session (shared by the tests below; never modified)."""
    if "orun" not in _golden:
        case = VC_CASE
        frames, h0, weights = vc_inputs(case)
        T = case.max_int
        chunks = [frames[c * T:(c + 1) * T].reshape(-1, case.enc_width) for c in range(case.num_samples)]
        u = np.stack([chunk_uniforms(case, c) for c in range(case.num_samples)])
        orc = VideoChat2Oracle(weights, case.N, case.tau, case.alpha, case.sticky, case.n_layers, case.cross_freq, 12, case.n_query, case.P)
        _golden.update(orun=OracleRun(orc, chunks, h0, u), chunks=chunks, u=u, h0=h0, weights=weights)
    return _golden


def check_golden_video(tag, proj, mean, hid, mem, dev_bins):
    case = VC_CASE
    g = load_vc_golden(case)
    ref = golden_reference()
    orun = ref["orun"]
    first = compare_draws(tag, dev_bins, orun)
    n_fix = case.num_samples if first is None else first[0]      # chunks the fixture still speaks for
    if first is not None:                                        # a tight draw flipped: the oracle with the device's bins
        orc = VideoChat2Oracle(ref["weights"], case.N, case.tau, case.alpha, case.sticky, case.n_layers, case.cross_freq, 12,
                               case.n_query, case.P)
        orun = OracleRun(orc, ref["chunks"], ref["h0"], ref["u"], bins=dev_bins)
    proj, hid = proj.cpu().numpy(), hid.cpu().numpy()
    worst = 0.0
    for c in range(case.num_samples):
        np.testing.assert_allclose(proj[c], orun.proj[c], rtol=0, atol=ATOL, err_msg=f"{tag}: chunk {c} vs oracle")
        np.testing.assert_allclose(hid[c], orun.hidden[c], rtol=0, atol=ATOL, err_msg=f"{tag}: chunk {c} hidden vs oracle")
        worst = max(worst, float(np.abs(proj[c] - orun.proj[c]).max()))
        if c < n_fix:
            np.testing.assert_allclose(proj[c], g[f"c{c}_mistral"], rtol=0, atol=ATOL, err_msg=f"{tag}: chunk {c} vs fixture")
            if f"c{c}_hidden" in g.files:
                np.testing.assert_allclose(hid[c], g[f"c{c}_hidden"], rtol=0, atol=ATOL)
    want_mean = g["mean_mistral"] if first is None else np.mean(np.stack(orun.proj), 0)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean, rtol=0, atol=ATOL, err_msg=f"{tag}: mean")
    c_last = case.num_samples - 1
    for j in range(case.n_ltm):
        B = mem.export_state(j)[0].cpu().numpy().astype(np.float64).sum(1)
        want = g[f"c{c_last}_l{2 * j}_Bsum"] if first is None else orun.Bsum[j]
        np.testing.assert_allclose(B, want, rtol=0, atol=1e-3, err_msg=f"{tag}: B row sums of cross layer {j}")
    record_parity(f"{tag}: max |proj - oracle| over {case.num_samples} chunks {worst:.3e}")


def test_golden_video_alone():
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    case = VC_CASE
    dev = dev0()
    ref = golden_reference()
    m, frames, h0, _ = golden_model(dev)
    mem = VideoChat2Memory(m, dev)
    traces = armed(mem, case.num_samples)
    video = torch.from_numpy(np.stack(ref["chunks"])).to(dev)
    proj, mean, hid = m.encode_videos([video], hidden_in=torch.from_numpy(h0), u=torch.from_numpy(ref["u"]), memories=[mem],
                                      want_hidden=True)
    bins = traced_bins(traces)
    assert proj.shape == (case.num_samples, case.n_query, case.proj_out) and hid[0].shape == (case.num_samples, case.n_query + case.n_text, case.hidden)
    check_golden_video("vc golden video, V = 1", proj, mean[0], hid[0], mem, bins)
    _golden["device"] = (proj.cpu(), mean[0].cpu(), hid[0].cpu())


def test_golden_video_inside_a_batch():
    """The golden video at position 1 among synthetic videos of 0, 1 and 3 chunks with text lengths 0, (8), 5 and 40."""
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    case = VC_CASE
    dev = dev0()
    ref = golden_reference()
    m, frames, h0, weights = golden_model(dev)
    n_tok = case.max_int * case.P
    synth_video = lambda v, n: torch.from_numpy(np.stack([synth.frame_tokens(100 * v + c, case.max_int, case.P, case.enc_width)
                                                          for c in range(n)]) if n else np.zeros((0, n_tok, case.enc_width), np.float32))
    q_rows = h0[:case.n_query]
    h_of = lambda v, n: torch.from_numpy(np.concatenate([q_rows, synth.layer_query(20 + v, n, case.hidden)], 0) if n else q_rows.copy())
    counts, texts = [0, case.num_samples, 1, 3], [0, case.n_text, 5, 40]
    videos = [synth_video(0, 0), torch.from_numpy(np.stack(ref["chunks"])), synth_video(2, 1), synth_video(3, 3)]
    hins = [h_of(0, 0), torch.from_numpy(h0), h_of(2, 5), h_of(3, 40)]
    rng = np.random.default_rng(5)
    u = np.concatenate([ref["u"], rng.random((4, case.n_ltm, S))])
    mems = [VideoChat2Memory(m, dev) for _ in counts]
    traces = armed(mems[1], case.num_samples)
    proj, mean, hid = m.encode_videos([v.to(dev) for v in videos], hidden_in=hins, u=torch.from_numpy(u), memories=mems, want_hidden=True)
    bins = traced_bins(traces)
    assert bool(torch.isfinite(proj).all()) and all(bool(torch.isfinite(x).all()) for x in hid)
    assert [tuple(x.shape) for x in hid] == [(c, case.n_query + t, case.hidden) for c, t in zip(counts, texts)]
    gp, gm, gh = proj[:case.num_samples], mean[1], hid[1]
    check_golden_video("vc golden video at position 1 of 4", gp, gm, gh, mems[1], bins)
    if "device" in _golden:                                     # batch invariance on the way: the same bits as alone
        assert torch.equal(gp.cpu(), _golden["device"][0]) and torch.equal(gm.cpu(), _golden["device"][1]) and torch.equal(gh.cpu(), _golden["device"][2])


# ------------------------------------------------------------------------------------------------ 4. small shapes
SMALL = {
    "base": {},
    "T8_exact_fp32": dict(T=8),
    "cross_freq1": dict(cross_freq=1),
    "cross_freq3": dict(cross_freq=3),
    "one_layer": dict(n_layers=1),
    "q32": dict(n_query=32),
    "q96": dict(n_query=96),
    "no_text": dict(texts=(0, 0, 0)),
    "alpha1": dict(alpha=1.0),
    "not_sticky": dict(sticky=False),
}


def small_setup(dev, **over):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    s = dict(BASE, **over)
    w = synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"], s["n_query"],
                                         s["proj"], seed=synth.SEED_VC + 31)
    m = VideoChat2Encoder(32, s["n_query"] - 32, s["enc_width"], s["proj"], s["N"], s["sticky"], s["tau"], s["alpha"], s["n_layers"],
                          s["cross_freq"], hidden_size=s["hidden"], intermediate_size=s["inter"], num_attention_heads=s["heads"],
                          tokens_per_frame=s["P"])
    m.load_reference_state_dict(w)
    return s, w, m.to(dev).eval()


@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes_against_the_oracle(name):
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = small_setup(dev, **SMALL[name])
    vids = [small_video(s, v, c, t) for v, (c, t) in enumerate(zip(s["counts"], s["texts"]))]
    runs, u = small_reference(s, w, vids, seed=900)
    use_ltm = s["alpha"] != 1.0
    mems = [VideoChat2Memory(m, dev) for _ in vids] if use_ltm else None
    traces = [armed(mem, len(k)) if s["sticky"] and len(k) else None for mem, (k, _) in zip(mems, vids)] if use_ltm else None
    torch.manual_seed(3)
    before = torch.get_rng_state()
    proj, mean, hid = m.encode_videos([torch.from_numpy(k).to(dev) for k, _ in vids], hidden_in=[torch.from_numpy(h) for _, h in vids],
                                      u=torch.from_numpy(u) if use_ltm and s["sticky"] else None, memories=mems, want_hidden=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), before)           # explicit u / no memory: the generator is untouched
    if not use_ltm:
        assert len(m._vc_memories) == 0                         # alpha = 1: no handles
    row, worst = 0, 0.0
    for v, ((k, _), orun) in enumerate(zip(vids, runs)):
        for c in range(len(k)):
            got_p, got_h = proj[row + c].cpu().numpy(), hid[v][c].cpu().numpy()
            np.testing.assert_allclose(got_p, orun.proj[c], rtol=0, atol=ATOL, err_msg=f"{name}: video {v} chunk {c}")
            np.testing.assert_allclose(got_h, orun.hidden[c], rtol=0, atol=ATOL, err_msg=f"{name}: video {v} chunk {c} hidden")
            worst = max(worst, float(np.abs(got_p - orun.proj[c]).max()), float(np.abs(got_h - orun.hidden[c]).max()))
        if len(k):
            np.testing.assert_allclose(mean[v].cpu().numpy(), np.mean(np.stack(orun.proj), 0), rtol=0, atol=ATOL)
            if use_ltm and s["sticky"]:
                bins = traced_bins(traces[v])
                for c in range(len(k)):
                    for j, ob in enumerate(orun.bins[c]):
                        if ob is not None:
                            assert np.array_equal(bins[c][j], ob), f"{name}: video {v} chunk {c} cross layer {j}: draws differ"
        row += len(k)
    record_parity(f"vc small shape {name}: max |device - oracle| {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 5. invariance
def memory_bits(mem):
    out = []
    for j, e in enumerate(mem.engines):
        B, mass = e.export_state(0)
        bins, idx, probs = e.last_draw(0)
        out.append((B.cpu(), mass.cpu(), torch.from_numpy(bins.copy()), torch.from_numpy(probs.copy())))
    return out


def same_bits(a, b, tag):
    pa, ma, ha, sa = a
    pb, mb, hb, sb = b
    assert torch.equal(pa, pb), f"{tag}: projected rows differ"
    assert torch.equal(ma, mb), f"{tag}: mean differs"
    assert torch.equal(ha, hb), f"{tag}: hidden rows differ"
    for j, (x, y) in enumerate(zip(sa, sb)):
        for name, t, w in zip(("B", "bin masses", "bins", "probabilities"), x, y):
            assert torch.equal(t, w), f"{tag}: cross layer {j}: {name} differ"


def test_batch_invariance_bit_for_bit():
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = small_setup(dev)
    nx = n_cross_of(s)
    rng = np.random.default_rng(77)
    vid = {v: small_video(s, v, n, t) for v, n, t in ((0, 5, 9), (1, 2, 5), (2, 3, 17), (3, 1, 0))}
    us = {v: rng.random((len(vid[v][0]), nx, S)) for v in vid}

    def run(order, texts=None, chunks=None, new_video=True, mems=None):
        """The videos of ``order`` in one call; returns {video: (proj, mean, hidden, memory bits)} and the memories."""
        ks, hs, uu = [], [], []
        for v in order:
            k, h0 = vid[v] if texts is None or v not in texts else small_video(s, v, len(vid[v][0]), texts[v])
            lo, hi = (0, len(k)) if chunks is None or v not in chunks else chunks[v]
            ks.append(torch.from_numpy(k[lo:hi]).to(dev)), hs.append(torch.from_numpy(h0)), uu.append(us[v][lo:hi])
        mems = mems or {v: VideoChat2Memory(m, dev) for v in order}
        proj, mean, hid = m.encode_videos(ks, hidden_in=hs, u=torch.from_numpy(np.concatenate(uu)), new_video=new_video,
                                          memories=[mems[v] for v in order], want_hidden=True)
        torch.cuda.synchronize()
        out, r0 = {}, 0
        for i, v in enumerate(order):
            n = ks[i].size(0)
            out[v] = (proj[r0:r0 + n].cpu(), mean[i].cpu(), hid[i].cpu(), memory_bits(mems[v]))
            r0 += n
        return out, mems

    alone, _ = run([0])
    for order in ([0, 1, 2], [1, 2, 0], [1, 0, 3, 2]):
        got, _ = run(order)
        same_bits(got[0], alone[0], f"video 0 in {order}")
    got, _ = run([1, 0, 2], texts={1: 40, 2: 0})               # the neighbours' text lengths change
    same_bits(got[0], alone[0], "video 0 beside other text lengths")
    first, mems = run([1, 0], chunks={0: (0, 2)})              # chunks [0, 2) with new_video, then [2, 5) continued
    second, _ = run([0, 2], chunks={0: (2, 5)}, new_video=False, mems={0: mems[0], 2: _fresh_started(m, dev, run, 2)})
    whole = alone[0]
    assert torch.equal(torch.cat([first[0][0], second[0][0]]), whole[0]), "projected rows of the two calls differ from one call"
    assert torch.equal(torch.cat([first[0][2], second[0][2]]), whole[2]), "hidden rows of the two calls differ from one call"
    for j, (x, y) in enumerate(zip(second[0][3], whole[3])):
        for name, t, w_ in zip(("B", "bin masses", "bins", "probabilities"), x, y):
            assert torch.equal(t, w_), f"continued call: cross layer {j}: {name} differ"


def _fresh_started(m, dev, run, v):
    """A memory of video ``v`` that holds its first chunk, so that a continuing call may carry the video along."""
    _, mems = run([v], chunks={v: (0, 1)})
    return mems[v]


# ------------------------------------------------------------------------------------------------ 6. the per-chunk binding
def test_agrees_with_the_per_chunk_binding_at_the_eval_shape():
    """4 videos x 3 chunks, 16 text tokens: every chunk within 2e-4 of ``encode_tokens`` on the same frames and uniforms, and the
    torch generator ends where the loop leaves it."""
    case = VC_CASE
    dev = dev0()
    m, frames, h0, _ = golden_model(dev)
    T = case.max_int
    chunk = lambda i: torch.from_numpy(frames[(i % 8) * T:(i % 8 + 1) * T].reshape(1, -1, case.enc_width)).to(dev)
    videos = [[chunk(2 * v + c) for c in range(3)] for v in range(4)]
    texts = [torch.from_numpy(synth.layer_query(60 + v, 16, case.hidden)).unsqueeze(0).to(dev) for v in range(4)]
    torch.manual_seed(2024)
    want = []
    for v in range(4):
        for c in range(3):
            want.append(m.encode_tokens(videos[v][c], texts[v], new_video=(c == 0))[0][0].cpu())
    end_loop = torch.get_rng_state()
    torch.manual_seed(2024)
    proj, mean, _ = m.encode_videos([torch.cat(v) for v in videos], text_embeds=texts)
    assert torch.equal(torch.get_rng_state(), end_loop)
    worst = 0.0
    for i in range(12):
        worst = max(worst, float((proj[i].cpu() - want[i]).abs().max()))
        np.testing.assert_allclose(proj[i].cpu().numpy(), want[i].numpy(), rtol=0, atol=ATOL, err_msg=f"video {i // 3} chunk {i % 3}")
    for v in range(4):
        np.testing.assert_allclose(mean[v].cpu().numpy(), torch.stack(want[3 * v:3 * v + 3]).mean(0).numpy(), rtol=0, atol=ATOL)
    record_parity(f"vc encode_videos vs encode_tokens loop, 4 videos x 3 chunks, 16 text tokens: max |diff| {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 7. device rng
def test_device_rng_equals_explicit_philox_uniforms():
    from infinite_video_amd import philox
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = small_setup(dev)
    nx = n_cross_of(s)
    seed, ids, counts = 4242, [7, 3], [(3, 2), (2, 2)]          # per video: chunks of the first call, of the continuing call
    vids = [small_video(s, v, a + b, t) for v, ((a, b), t) in enumerate(zip(counts, (5, 12)))]

    def mirror(v, pos0, n):
        return np.stack([philox.gibbs_uniforms(seed, (ids[v] + 1) * nx + j, pos0, n, 1, S)[:, 0] for j in range(nx)], 1)

    def run(rng):
        m.use_device_rng(seed if rng else None)
        mems = [VideoChat2Memory(m, dev) for _ in vids]
        outs = []
        for call, new_video in ((0, True), (1, False)):
            ks, uu = [], []
            for v, (k, _) in enumerate(vids):
                lo = 0 if call == 0 else counts[v][0]
                hi = counts[v][0] if call == 0 else counts[v][0] + counts[v][1]
                ks.append(torch.from_numpy(k[lo:hi]).to(dev))
                uu.append(mirror(v, lo, hi - lo))
            before = torch.get_rng_state()
            outs.append(m.encode_videos(ks, hidden_in=[torch.from_numpy(h) for _, h in vids], new_video=new_video,
                                        u=None if rng else torch.from_numpy(np.concatenate(uu)), memories=mems, video_ids=ids,
                                        want_hidden=True))
            torch.cuda.synchronize()
            assert torch.equal(torch.get_rng_state(), before)   # nothing is drawn on the host
        return outs, [memory_bits(mem) for mem in mems]

    try:
        got, got_mem = run(True)
        want, want_mem = run(False)
    finally:
        m.use_device_rng(None)
    for call in range(2):
        assert torch.equal(got[call][0], want[call][0]) and torch.equal(got[call][1], want[call][1]), f"call {call}: outputs differ"
        for a, b in zip(got[call][2], want[call][2]):
            assert torch.equal(a, b)
    for a, b in zip(got_mem, want_mem):
        for x, y in zip(a, b):
            for t, w_ in zip(x, y):
                assert torch.equal(t, w_)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_through_the_c_abi_leave_the_memories_alone():
    from infinite_video_amd import _lib
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = small_setup(dev)
    lib = _lib.load()
    nx = n_cross_of(s)
    k, h0 = small_video(s, 0, 2, 5)
    mems = [VideoChat2Memory(m, dev), VideoChat2Memory(m, dev)]
    u = torch.from_numpy(np.random.default_rng(1).random((4, nx, S)))
    kk = torch.from_numpy(np.concatenate([k, k])).to(dev)
    m.encode_videos([kk[:2], kk[2:]], hidden_in=torch.from_numpy(h0), u=u, memories=mems)
    torch.cuda.synchronize()
    before = [memory_bits(mem) for mem in mems]
    h = m._vc_handle(dev)
    wts, keep = m._vc_weights(dev)
    hin = torch.from_numpy(np.concatenate([h0, h0])).to(dev)
    ud = u.to(dev)
    proj = torch.empty(4, s["n_query"], s["proj"], device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(handles=None, cu=(0, 2, 4), T=s["T"], weights=None, texts=(5, 5), frames=kk):
        hs = (C.c_void_p * (2 * nx))(*(handles or [e._h for mem in mems for e in mem.engines]))
        cu_a, tl = (C.c_int32 * 3)(*cu), (C.c_int32 * 2)(*texts)
        with torch.cuda.device(dev):
            return lib.infv_vqf_vc_encode_videos(h, hs, 2, C.cast(cu_a, C.c_void_p), C.c_void_p(frames.data_ptr()), T,
                                                 C.byref(weights or wts), C.c_void_p(hin.data_ptr()), C.cast(tl, C.c_void_p),
                                                 C.c_void_p(ud.data_ptr()), 0, None, C.c_void_p(proj.data_ptr()), None, stream)

    INVALID, UNSUPPORTED = -1, -2
    assert call(cu=(1, 2, 4)) == INVALID and call(cu=(0, 3, 2)) == INVALID                       # bad cu
    own = [e._h for mem in mems for e in mem.engines]
    assert call(handles=own[:-1] + [own[0]]) == INVALID                                         # a repeated handle
    many = (_lib.VqfVcLayer * 25)(*[wts.layers[i % wts.n_layers] for i in range(25)])
    assert call(weights=_lib.VqfVcWeights(25, 0, many, wts.mistral_proj)) == UNSUPPORTED         # 25 layers
    assert call(T=12) == UNSUPPORTED                                                            # T * P = 48
    assert call(texts=(5, 609 - s["n_query"])) == UNSUPPORTED                                   # 609 tokens in all
    _lib.check(lib.infv_vqf_set_token_dtype(h, 1))
    try:
        assert call() == UNSUPPORTED                                                            # a bf16 token setting
    finally:
        _lib.check(lib.infv_vqf_set_token_dtype(h, 0))
    torch.cuda.synchronize()
    for mem, was in zip(mems, before):
        assert mem.has_memory
        for x, y in zip(memory_bits(mem), was):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    del keep


# ------------------------------------------------------------------------------------------------ 9. fallback
class DenseStep:
    """The LTM of one cross layer as the reference-shaped ``DenseOracle``, behind ``ClosedFormOracle.step``'s signature.  At
    num_basis 48 fp32 boxes overlap at some points, so the closed form does not apply (``box_index`` raises) and
    ``VideoChat2Oracle`` cannot build its own LTMs.  ``DenseOracle`` draws from torch's global generator, so the uniforms of a
    step are those of a seed: ``torch.rand(S, float64)`` right after ``torch.manual_seed(seed)`` (``sweep_cases.uniforms``).
    The seed of each step is the first from ``seed0`` upwards at which every oracle margin is at least MARGIN (asserted), so
    that the draws agree and 2e-4 speaks for the arithmetic alone."""

    def __init__(self, s, w, layer, seed0):
        p = f"bert.encoder.layer.{layer}.crossattention.self."
        lin = {}
        for name in ("key", "value"):
            wt = torch.from_numpy(np.asarray(w[p + name + ".weight"], np.float32))
            lin[name] = torch.nn.Linear(wt.shape[1], wt.shape[0])
            with torch.no_grad():
                lin[name].weight.copy_(wt)
                lin[name].bias.copy_(torch.from_numpy(np.asarray(w[p + name + ".bias"], np.float32)))
        self.o = DenseOracle(s["N"], s["heads"], s["hidden"] // s["heads"], s["tau"], s["sticky"], lin["key"], lin["value"],
                             pool_shape=(s["P"],))
        self.seed, self.u = seed0, []                            # uniforms of the steps made so far (None: nothing drawn)

    def step(self, k, q, new_doc, u=None):
        kt, qt = torch.from_numpy(np.asarray(k, np.float32))[None], torch.from_numpy(np.asarray(q, np.float32))[None]
        if new_doc or self.o.B_past is None or not self.o.sticky:
            with torch.no_grad():
                out = self.o.forward(kt, qt, new_doc)
            self.u.append(None)
            return out[0].numpy()
        state = self.o.B_past, self.o.queries, self.o.keys, self.o.values
        uu = None
        for _ in range(2):                                       # the probabilities (any seed gives them), then the step itself
            self.o.B_past, self.o.queries, self.o.keys, self.o.values = state
            with torch.random.fork_rng(), torch.no_grad():
                torch.manual_seed(self.seed)
                out = self.o.forward(kt, qt, False)
            probs = self.o.last_probs.reshape(-1).numpy()
            if uu is None:
                for _ in range(1000):                            # a seed passes with probability ~0.07 (512 draws, 127 edges)
                    self.seed += 1
                    uu = torch.rand(S, dtype=torch.float64, generator=torch.Generator().manual_seed(self.seed)).numpy()
                    if float(draw_margins(probs, uu).min()) >= MARGIN:
                        break
        assert float(draw_margins(probs, uu).min()) >= MARGIN    # the precondition of equal draws
        assert np.array_equal(inverse_cdf_draw(probs, uu), self.o.last_bins.numpy())       # uu is what the generator gave
        self.u.append(uu)
        return out[0].numpy()


def test_dense_plan_memories_take_the_per_handle_fallback():
    """num_basis 48: a dense plan, which the lockstep kernels do not take -- ``infv_ltm_steps_videos`` runs each handle in turn.
    The oracle is ``VideoChat2Oracle`` around ``DenseOracle`` LTMs (``DenseStep``)."""
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    dev = dev0()
    s, w, m = small_setup(dev, N=48)
    vids = [small_video(s, v, c, t) for v, (c, t) in enumerate(zip(s["counts"], s["texts"]))]
    nx = n_cross_of(s)
    want, us = [], []
    for v, (k, h0) in enumerate(vids):
        orc = small_oracle(dict(s, N=32), w)                     # (its own closed-form LTMs are replaced before any step)
        steps = [DenseStep(s, w, l, 5000 + 1000 * v + 100 * j) for j, l in enumerate(sorted(orc.ltm))]
        orc.ltm = dict(zip(sorted(orc.ltm), steps))
        want.append([orc.encode_chunk(k[c], h0, c == 0) for c in range(len(k))])
        us.append(np.stack([[np.zeros(S) if st.u[c] is None else st.u[c] for st in steps] for c in range(len(k))])
                  if len(k) else np.zeros((0, nx, S)))
    mems = [VideoChat2Memory(m, dev) for _ in vids]
    proj, mean, hid = m.encode_videos([torch.from_numpy(k).to(dev) for k, _ in vids], hidden_in=[torch.from_numpy(h) for _, h in vids],
                                      u=torch.from_numpy(np.concatenate(us)), memories=mems, want_hidden=True)
    torch.cuda.synchronize()
    assert all(e.ensure_plan(s["T"]).dense for mem in mems for e in mem.engines)
    row, worst = 0, 0.0
    for v, (k, h0) in enumerate(vids):
        for c in range(len(k)):
            want_h, want_p = want[v][c]
            np.testing.assert_allclose(proj[row + c].cpu().numpy(), want_p, rtol=0, atol=ATOL, err_msg=f"video {v} chunk {c}")
            np.testing.assert_allclose(hid[v][c].cpu().numpy(), want_h, rtol=0, atol=ATOL)
            worst = max(worst, float(np.abs(proj[row + c].cpu().numpy() - want_p).max()))
        row += len(k)
    record_parity(f"vc dense-plan fallback (num_basis 48): max |device - oracle| {worst:.3e}")
