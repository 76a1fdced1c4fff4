"""``VideoChat2Encoder.encode_img_videos`` / ``infv_vqf_vc_encode_img``: encode_img from the vision encoder's raw output (fp32 /
fp16 / bf16, read in place; ``vision_layernorm`` runs inside the token pass) and the tokenizer's ids (the embedding layer runs on the
device).  Two kinds of checks:

* bits -- the fused call against the two-step form it replaces, ``encode_videos(vision_tokens_layernorm(raw),
  hidden_in=embed_instructions(ids))``, with ``torch.equal`` on projected rows, means, hidden rows and every memory's B, masses, bins
  and probabilities, on a new video's first two chunks and continued; over the paths of ``test_vc_half_tokens_gpu.OVER`` (tile pass
  with the means; pooling with the LayerNorm on load, then the split; the fp32 fallback), a width of 192, streams, a cache budget no
  plane fits, and batch positions;
* values -- the two exported pieces against float64 on the CPU, within 4 x the error torch's own float32 ``layer_norm`` makes on the
  same inputs (the summation orders differ), the embedding rows also against the golden of the reference's ``BertEmbeddings``, and
  the whole call against ``oracle/videochat2_oracle.py`` fed torch-computed LayerNorm tokens and embedding rows.

Raw tokens are ``small_video`` tokens scaled by 8 with a per-column offset, so that the mean and the variance matter; one all-constant
token row rides along for finiteness and the bitwise checks and is left out of the value comparison alone (var = 0 with eps = 1e-12
amplifies rounding in torch as well).  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infinite_video_amd import synth
from tests.conftest import record_parity
from tests.golden.seam_cases import BASE, S, n_cross_of, small_reference, small_video
from tests.test_vc_encode_img_cpu import MAX_POS, VOCAB, front_weights
from tests.test_vc_half_tokens_gpu import OVER as HALF_OVER
from tests.test_vc_half_tokens_gpu import Raw, memories, rows, same_raw
from tests.test_vc_videos_gpu import ATOL, armed, memory_bits, same_bits, traced_bins

pytestmark = pytest.mark.gpu
OVER = dict(HALF_OVER, W192_three_per_lane=dict(enc_width=192))       # d / 64 = 3 values per lane, a width that is no power of two
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CONST_ROW = (0, 1)                                                     # (chunk, token) of the all-constant row of every block with chunks
IDS = ([0, 49, 7, 7, 23], [], [49, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0, 7, 48], [3, 3, 3, 44, 0, 1, 2, 9, 9])   # lengths 5, 0, 17, 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vc_embed.npz")


def dev0():
    return torch.device("cuda:0")


_setups = {}


def new_model(s, w, fw, dev):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    m = VideoChat2Encoder(32, s["n_query"] - 32, s["enc_width"], s["proj"], s["N"], s["sticky"], s["tau"], s["alpha"], s["n_layers"],
                          s["cross_freq"], hidden_size=s["hidden"], intermediate_size=s["inter"], num_attention_heads=s["heads"],
                          tokens_per_frame=s["P"], vocab_size=VOCAB, max_position_embeddings=MAX_POS, vision_layernorm=True)
    m.load_reference_state_dict(dict(w, **fw))
    return m.to(dev).eval()


def setup(dev, name):
    """(shape, weights, front weights, encoder with both new modules) of ``BASE`` with ``OVER[name]``, once per session."""
    if name not in _setups:
        s = dict(BASE, **OVER[name])
        w = synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"], s["n_query"],
                                             s["proj"], seed=synth.SEED_VC + 31)
        fw = front_weights(s)
        _setups[name] = (s, w, fw, new_model(s, w, fw, dev))
    return _setups[name]


def raw_block(s, v, n):
    """What a vision encoder might hand over: video ``v``'s tokens x 8 plus a per-column offset, fp32 [n, T*P, width]; the token
    ``CONST_ROW`` is constant."""
    k = small_video(s, v, n, 0)[0]
    x = (k * np.float32(8.0) + np.linspace(-3.0, 3.0, s["enc_width"], dtype=np.float32)).astype(np.float32)
    if n:
        x[CONST_ROW] = np.float32(2.5)
    return x


def raw_blocks(s, dev, dtype, counts, first=0):
    return [torch.from_numpy(raw_block(s, first + f, n)).to(dev).to(dtype) for f, n in enumerate(counts)]


def run(m, img, blocks, frame_src, extra, u, new_video, mems, lo=0, hi=10 ** 6):
    """Chunks [lo, hi) of every block through encode_img_videos (``img``) or encode_videos / encode_streams.  Returns per stream
    (proj, mean, hidden, memory bits) and the launches the call issued."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    vids = [b[lo:hi] for b in blocks]
    src = list(range(len(blocks))) if frame_src is None else list(frame_src)
    counts = [vids[f].size(0) for f in src]
    cu = np.concatenate([[0], np.cumsum([blocks[f].size(0) for f in src])])
    uu = torch.from_numpy(np.concatenate([u[cu[v] + lo:cu[v] + min(hi, blocks[f].size(0))] for v, f in enumerate(src)]))
    kw = dict(u=uu, new_video=new_video, memories=mems, want_hidden=True, **extra)
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    if img:
        proj, mean, hid = m.encode_img_videos(vids, frame_src=frame_src, **kw)
    elif frame_src is None:
        proj, mean, hid = m.encode_videos(vids, **kw)
    else:
        proj, mean, hid = m.encode_streams(vids, src, **kw)
    torch.cuda.synchronize()
    launches = lib.infv_ltm_launch_count() - n0
    out, r0 = [], 0
    for v, n in enumerate(counts):
        out.append((proj[r0:r0 + n].cpu(), mean[v].cpu(), hid[v].cpu(), memory_bits(mems[v])))
        r0 += n
    return out, launches


def both_ways(m_img, m_two, dev, s, dtype, counts, frame_src, tag, seed, ids=None):
    """The raw blocks as ``dtype`` through ``m_img.encode_img_videos`` and, normalised by ``vision_tokens_layernorm`` (and embedded by
    ``embed_instructions`` where ``ids`` are given), through ``m_two.encode_videos`` / ``encode_streams``: new_video on the first two
    chunks, then the rest continued on the same memories.  Every stream's outputs and memories must be the same bits."""
    blocks = raw_blocks(s, dev, dtype, counts)
    normed = [m_two.vision_tokens_layernorm(b) for b in blocks]
    assert all(b.dtype == dtype for b in blocks) and all(b.dtype == torch.float32 and bool(torch.isfinite(b).all()) for b in normed)
    src = list(range(len(counts))) if frame_src is None else list(frame_src)
    if ids is None:
        hin = [rows(s, v, t) for v, t in zip(range(len(src)), (5, 0, 17, 9))]
        extra_img = extra_two = dict(hidden_in=hin)
    else:
        ids = [torch.tensor(x, dtype=torch.long) for x in ids[:len(src)]]
        extra_img, extra_two = dict(input_ids=ids), dict(hidden_in=m_two.embed_instructions(ids, device=dev))
    u = np.random.default_rng(seed).random((sum(counts[f] for f in src), n_cross_of(s), S))
    got, launches = {}, {}
    for kind, m, bl, extra in (("img", m_img, blocks, extra_img), ("two", m_two, normed, extra_two)):
        mems = memories(m, dev, len(src))
        first, _ = run(m, kind == "img", bl, frame_src, extra, u, True, mems, 0, 2)      # (two chunks: every memory has drawn once)
        rest, launches[kind] = run(m, kind == "img", bl, frame_src, extra, u, False, mems, 2)
        got[kind] = (first, rest)
    for part, name in ((0, "first chunks, new_video"), (1, "continued")):
        for v, (a, b) in enumerate(zip(got["img"][part], got["two"][part])):
            same_bits(a, b, f"{tag}: {name}: stream {v}")
            assert all(bool(torch.isfinite(t).all()) for t in a[:3])
    return launches


# ------------------------------------------------------------------------------------------------ bits: the vision LayerNorm
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(OVER))
def test_raw_tokens_give_the_bits_of_the_two_step_call(name, dname):
    """encode_img_videos(raw) against encode_videos(vision_tokens_layernorm(raw)) for every source dtype and token-pass path."""
    dev = dev0()
    s, w, fw, m = setup(dev, name)
    launches = both_ways(m, m, dev, s, DTYPES[dname], (3,), None, f"{name} {dname} encode_img_videos", seed=21)
    record_parity(f"vc encode_img {name} {dname}: the fused call == LayerNorm copy + fp32 call bit for bit; launches {launches}")
    # the statistics launch, and on the fp32 fallback the launch that writes the normalised copy, are all the fused call adds
    assert launches["img"] <= launches["two"] + (2 if name == "P12_T8_upcast" else 1), launches


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(OVER))
def test_raw_tokens_through_streams_give_the_same_bits(name, dname):
    """The same through frame_src = (1, 0, 1) over two blocks: the statistics and the planes of the distinct chunks only."""
    dev = dev0()
    s, w, fw, m = setup(dev, name)
    both_ways(m, m, dev, s, DTYPES[dname], (3, 4), (1, 0, 1), f"{name} {dname} encode_img_videos, streams", seed=22)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", ["P4_tile_means", "P12_two_passes"])
def test_planes_that_do_not_fit_the_cache_give_the_same_bits(name, dname, monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB too small for any plane on the fused encoder's handle (read at its creation): token passes with the
    LayerNorm on load per sub-batch, and per contiguous run of source chunks under streams -- against the two-step form on an
    encoder with the default budget."""
    dev = dev0()
    s, w, fw, m_two = setup(dev, name)
    m_two._vc_handle(dev)
    monkeypatch.setenv("INFV_VQF_SPLIT_CACHE_GB", "1e-9")
    m_img = new_model(s, w, fw, dev)
    m_img._vc_handle(dev)                                             # created under the small budget
    monkeypatch.delenv("INFV_VQF_SPLIT_CACHE_GB")
    both_ways(m_img, m_two, dev, s, DTYPES[dname], (3,), None, f"{name} {dname} no cache", seed=23)
    both_ways(m_img, m_two, dev, s, DTYPES[dname], (3, 4), (1, 0, 1), f"{name} {dname} no cache, streams", seed=24)


# ------------------------------------------------------------------------------------------------ bits: the embedding layer
@pytest.mark.parametrize("name", ["P4_tile_means", "P12_T8_upcast"])
def test_input_ids_give_the_bits_of_embedded_rows(name):
    """encode_img_videos(raw, input_ids) against encode_videos(LN(raw), hidden_in=embed_instructions(ids)): text lengths 5, 0, 17,
    videos and streams."""
    dev = dev0()
    s, w, fw, m = setup(dev, name)
    both_ways(m, m, dev, s, torch.float16, (3, 4, 3), None, f"{name} ids, videos", seed=25, ids=IDS)
    both_ways(m, m, dev, s, torch.float16, (3, 4), (1, 0, 1), f"{name} ids, streams", seed=26, ids=IDS)


def test_batch_invariance_of_raw_tokens_and_ids():
    """A probe video alone, last of three, and beside other text lengths: the same bits."""
    dev = dev0()
    s, w, fw, m = setup(dev, "P12_two_passes")
    blocks = [torch.from_numpy(raw_block(s, v, n)).to(dev).half() for v, n in ((3, 2), (4, 1), (0, 3))]
    ids = lambda *ii: [torch.tensor(IDS[i], dtype=torch.long) for i in ii]
    rng = np.random.default_rng(27)
    us = [rng.random((b.size(0), n_cross_of(s), S)) for b in blocks]
    alone, _ = run(m, True, blocks[2:], None, dict(input_ids=ids(0)), us[2], True, memories(m, dev, 1))
    for tag, others in (("text lengths 17, 0", (2, 1)), ("text lengths 9, 17", (3, 2))):
        batch, _ = run(m, True, blocks, None, dict(input_ids=ids(*others, 0)), np.concatenate(us), True, memories(m, dev, 3))
        same_bits(batch[2], alone[0], f"probe last of three, beside {tag}")


# ------------------------------------------------------------------------------------------------ both parts off: the _tok call
def run_img_raw(r, mems, frames_ptr, code, front, new_video=1):
    """``Raw.run`` through infv_vqf_vc_encode_img (videos: frame_src NULL)."""
    s, dev = r.s, r.dev
    Q = s["n_query"]
    hs = (C.c_void_p * (2 * r.nx))(*[e._h for mem in mems for e in mem.engines])
    cu, tl = (C.c_int32 * 3)(0, 2, 4), (C.c_int32 * 2)(5, 5)
    proj = torch.zeros(4, Q, s["proj"], device=dev)
    mean = torch.zeros(2, Q, s["proj"], device=dev)
    hid = torch.zeros(4 * (Q + 5), s["hidden"], device=dev)
    torch.cuda.synchronize()
    n0 = r.lib.infv_ltm_launch_count()
    with torch.cuda.device(dev):
        rc = r.lib.infv_vqf_vc_encode_img(r.h, hs, 2, C.cast(cu, C.c_void_p), C.c_void_p(frames_ptr), code, 0, None, None, s["T"],
                                          C.byref(r.wts), None if front is None else C.byref(front), C.c_void_p(r.hin.data_ptr()),
                                          C.cast(tl, C.c_void_p), C.c_void_p(r.u.data_ptr()), new_video, C.c_void_p(hid.data_ptr()),
                                          C.c_void_p(proj.data_ptr()), C.c_void_p(mean.data_ptr()), r.stream)
    torch.cuda.synchronize()
    return rc, r.lib.infv_ltm_launch_count() - n0, (proj.cpu(), mean.cpu(), hid.cpu())


@pytest.mark.parametrize("code", [0, 3])
def test_both_parts_off_is_the_tok_call(code):
    """front NULL, and a front with gamma and word NULL, against infv_vqf_vc_encode_videos_tok on the same tensors: the same bits and
    the same number of launches."""
    from infinite_video_amd import _lib
    r = Raw()
    off = _lib.VqfVcFront(_lib.VqfVisionLn(None, None, 1e-12), _lib.VqfVcEmb(None, None, _lib.LayerNorm(None, None), 0, 0, None), None, 0)
    k = r.k32 if code == 0 else r.k16
    for _ in range(2):                                                # (the second round is warm: equal launch counts)
        ma, mb, mc = r.fresh(), r.fresh(), r.fresh()
        rc_a, n_a, out_a = r.run(ma, "infv_vqf_vc_encode_videos_tok", k.data_ptr(), code)
        rc_b, n_b, out_b = run_img_raw(r, mb, k.data_ptr(), code, None)
        rc_c, n_c, out_c = run_img_raw(r, mc, k.data_ptr(), code, off)
        assert rc_a == 0 and rc_b == 0 and rc_c == 0, r.lib.infv_ltm_last_error()
    assert n_a == n_b == n_c, (n_a, n_b, n_c)
    same_raw(out_b, out_a, mb, ma, "front NULL against the _tok call")
    same_raw(out_c, out_a, mc, ma, "both parts off against the _tok call")


# ------------------------------------------------------------------------------------------------ values
def within_four_times_torch(got, x64, ref64_fn, ref32_fn, keep, tag):
    """|got - float64| <= 4 x max |torch float32 - float64| on the same inputs (rows ``keep``); both numbers are recorded."""
    want = ref64_fn(x64)
    torch_err = float((ref32_fn(x64.float()).double() - want)[keep].abs().max())
    err = float((got.double() - want)[keep].abs().max())
    record_parity(f"{tag}: max |kernel - float64| {err:.3e}; torch float32 layer_norm on the same inputs {torch_err:.3e} (bound: 4 x)")
    assert torch_err > 0
    assert err <= 4 * torch_err, (tag, err, torch_err)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", ["P4_tile_means", "W192_three_per_lane", "eval_width_1024"])
def test_vision_tokens_layernorm_against_float64(name, dname):
    dev = dev0()
    if name == "eval_width_1024":                                     # the model's width: 16 values per lane
        s, fw = dict(BASE, enc_width=1024, T=4), front_weights(dict(BASE, enc_width=1024))
        w = synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"], s["n_query"],
                                             s["proj"], seed=synth.SEED_VC + 31)
        m = new_model(s, w, fw, dev)
    else:
        s, w, fw, m = setup(dev, name)
    x = torch.from_numpy(raw_block(s, 1, 3)).to(DTYPES[dname])        # (rounded to the source dtype first: the kernel widens exactly)
    got = m.vision_tokens_layernorm(x.to(dev)).cpu()
    assert got.dtype == torch.float32 and got.shape == x.shape and bool(torch.isfinite(got).all())
    g, b = torch.from_numpy(fw["vision_layernorm.weight"]), torch.from_numpy(fw["vision_layernorm.bias"])
    keep = torch.ones(x.shape[:2], dtype=torch.bool)
    keep[CONST_ROW] = False                                           # the one row left out: var = 0
    d = s["enc_width"]
    within_four_times_torch(got, x.double(), lambda t: F.layer_norm(t, (d,), g.double(), b.double(), 1e-12),
                            lambda t: F.layer_norm(t, (d,), g, b, 1e-12), keep, f"vc encode_img vision LayerNorm {name} {dname}")
    assert torch.equal(got[CONST_ROW], b)                             # mean exact, x - mean = 0: the row is beta


def embedding_rows_torch(tables, ids, dtype):
    """cat(query_tokens, word[ids] + pos[:n]) -> LayerNorm, as Qformer.py:93-109, in ``dtype``; returns (input rows, output rows)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    x = t(tables["query_tokens"])
    if len(ids):
        x = torch.cat([x, t(tables["word"])[torch.tensor(ids, dtype=torch.long)] + t(tables["pos"])[:len(ids)]], 0)
    return x, F.layer_norm(x, (x.size(-1),), t(tables["gamma"]), t(tables["beta"]), float(tables["eps"]))


def test_embed_instructions_against_float64_and_the_reference_golden():
    """The tables of tests/golden/vc_embed.npz (vocab 50, 32 positions, hidden 128, 40 query tokens) loaded into the encoder: the
    kernel's rows against float64, within 4 x the error of torch's float32 LayerNorm on the same rows, and against the rows the
    reference's own BertEmbeddings produced -- they are float32 results too, so the distance to them is bounded by the kernel's
    error plus theirs (triangle inequality): 4 x + 1 x the torch error."""
    dev = dev0()
    gold = np.load(GOLDEN)
    s, w, fw, _ = setup(dev, "P4_tile_means")
    assert gold["word"].shape == (VOCAB, s["hidden"]) and gold["pos"].shape == (MAX_POS, s["hidden"]) and \
        gold["query_tokens"].shape == (s["n_query"], s["hidden"])
    fw = dict(fw, **{"bert.embeddings.word_embeddings.weight": gold["word"], "bert.embeddings.position_embeddings.weight": gold["pos"],
                     "bert.embeddings.LayerNorm.weight": gold["gamma"], "bert.embeddings.LayerNorm.bias": gold["beta"]})
    m = new_model(s, dict(w, query_tokens=gold["query_tokens"][None]), fw, dev)
    ids = [gold[f"ids{v}"].tolist() for v in range(3)]
    assert [len(x) for x in ids] == [5, 0, 17] and 0 in ids[0] and 49 in ids[0] and ids[0].count(7) == 2
    got = [r.cpu() for r in m.embed_instructions([torch.tensor(x, dtype=torch.long) for x in ids], device=dev)]
    tables = {k: gold[k] for k in ("word", "pos", "gamma", "beta", "query_tokens", "eps")}
    for v, x in enumerate(ids):
        assert got[v].shape == (s["n_query"] + len(x), s["hidden"])
        _, want64 = embedding_rows_torch(tables, x, torch.float64)
        _, want32 = embedding_rows_torch(tables, x, torch.float32)
        golden = torch.from_numpy(gold[f"rows{v}"])
        torch_err = max(float((want32.double() - want64).abs().max()), float((golden.double() - want64).abs().max()))
        err = float((got[v].double() - want64).abs().max())
        to_golden = float((got[v] - golden).abs().max())
        record_parity(f"vc encode_img embedding rows, {len(x)} ids: max |kernel - float64| {err:.3e}, |kernel - reference golden| "
                      f"{to_golden:.3e}; torch float32 on the same rows {torch_err:.3e} (bounds: 4 x, 5 x)")
        assert torch_err > 0 and err <= 4 * torch_err and to_golden <= 5 * torch_err, (v, err, to_golden, torch_err)
    assert torch.equal(got[0][:s["n_query"]], got[1]) and torch.equal(got[2][:s["n_query"]], got[1])   # the query rows: the same for every video


def test_raw_tokens_and_ids_against_the_oracle():
    """encode_img_videos on raw fp32 tokens + ids against oracle/videochat2_oracle.py fed torch-computed LayerNorm tokens and
    embedding rows, with test_small_shapes_against_the_oracle's tolerances: 2e-4, every drawn bin equal."""
    dev = dev0()
    s, w, fw, m = setup(dev, "P4_tile_means")
    g, b = torch.from_numpy(fw["vision_layernorm.weight"]), torch.from_numpy(fw["vision_layernorm.bias"])
    tables = {"word": fw["bert.embeddings.word_embeddings.weight"], "pos": fw["bert.embeddings.position_embeddings.weight"],
              "gamma": fw["bert.embeddings.LayerNorm.weight"], "beta": fw["bert.embeddings.LayerNorm.bias"],
              "query_tokens": w["query_tokens"][0], "eps": 1e-12}
    counts = (2, 0, 3)
    raws = [raw_block(s, v, n) for v, n in enumerate(counts)]
    vids = [(F.layer_norm(torch.from_numpy(x), (s["enc_width"],), g, b, 1e-12).numpy(),
             embedding_rows_torch(tables, IDS[v], torch.float32)[1].numpy()) for v, x in enumerate(raws)]
    runs, u = small_reference(s, w, vids, seed=901)
    mems = memories(m, dev, len(vids))
    traces = [armed(mem, n) if n else None for mem, n in zip(mems, counts)]
    proj, mean, hid = m.encode_img_videos([torch.from_numpy(x).to(dev) for x in raws],
                                          input_ids=[torch.tensor(IDS[v], dtype=torch.long) for v in range(len(vids))],
                                          u=torch.from_numpy(u), memories=mems, want_hidden=True)
    torch.cuda.synchronize()
    row, worst = 0, 0.0
    for v, (n, orun) in enumerate(zip(counts, runs)):
        for c in range(n):
            got_p, got_h = proj[row + c].cpu().numpy(), hid[v][c].cpu().numpy()
            np.testing.assert_allclose(got_p, orun.proj[c], rtol=0, atol=ATOL, err_msg=f"video {v} chunk {c}")
            np.testing.assert_allclose(got_h, orun.hidden[c], rtol=0, atol=ATOL, err_msg=f"video {v} chunk {c} hidden")
            worst = max(worst, float(np.abs(got_p - orun.proj[c]).max()), float(np.abs(got_h - orun.hidden[c]).max()))
        if n:
            np.testing.assert_allclose(mean[v].cpu().numpy(), np.mean(np.stack(orun.proj), 0), rtol=0, atol=ATOL)
            bins = traced_bins(traces[v])
            for c in range(n):
                for j, ob in enumerate(orun.bins[c]):
                    if ob is not None:
                        assert np.array_equal(bins[c][j], ob), f"video {v} chunk {c} cross layer {j}: draws differ"
        row += n
    record_parity(f"vc encode_img raw tokens + ids against the oracle: max |device - oracle| {worst:.3e}")
