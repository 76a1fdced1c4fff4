"""Call layouts that cross the host-side seams of the batched Q-former calls (``infv_ltm_steps_videos``,
``infv_vqf_encode_videos``, ``infv_vqf_vc_encode_videos``, ``infv_vqf_self_attention``), as data: per layout the shape, the chunk
count and text length of every video and which videos are "probes" -- videos placed so that they own chunks, rows or video
slots on both sides of a seam.  ``seam_constants`` reads the sizes of the seams out of ``csrc/``; ``boundaries`` / ``crossed`` /
``straddles`` say where a layout meets them.  The margin-safe oracle runs of the probes (``OracleRun``, ``small_reference``) live
here too, shared by ``tests/test_vc_videos_gpu.py`` and the seam tests.  Pure Python: nothing here touches a device."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from infinite_video_amd import synth
from oracle.ltm_oracle import ClosedFormOracle, categorical_probs
from oracle.qformer_oracle import VideoQformerOracle
from oracle.videochat2_oracle import VideoChat2Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "infinite-video_amd", "csrc")
MARGIN = 2e-5            # the project's bound on probabilities: draws with a wider margin must agree
S = synth.NB_SAMPLES

# ------------------------------------------------------------------------------------------------ the seams, from csrc/
_CONSTANTS = {                                                   # name -> (file, regex with the value(s) as groups)
    "row_block": ("vqf_internal.h", r"constexpr int kRowBlockVideos = (\d+);"),
    "row_block_video": ("vqf_internal.h", r"constexpr int kRowBlockVideo = (\d+);"),
    "text_ffn": ("vqf_internal.h", r"constexpr long kTextFfnRows = (\d+);"),
    "merge": ("vqf_internal.h", r"constexpr long kMergeRows = (\d+);"),
    "mean_table": ("vqf_internal.h", r"constexpr int kMeanSegs = (\d+);"),
    "copy_rows": ("vqf_internal.h", r"constexpr int kRowSegs = (\d+);"),
    "attn_group": ("vqf_internal.h", r"constexpr int kVcAttnGroup = (\d+);"),
    "video_group": ("ltm_capi.hip", r"constexpr int kVideoGroup = (\d+);"),
    "short_nb": ("vqf_capi.hip", r"for \(int nb = (\d+); nb <= (\d+) && nb <= C; \+\+nb\)"),     # pick_short_nb: (lowest, highest)
}
# the sites that must use the names (a literal that came back would leave the constant read here without meaning)
_USES = {
    "row_block": ("vqf_capi.hip", r"rb_max = multi \? kRowBlockVideos : kRowBlockVideo;", r"RB = C < kRowBlockVideos \? C : kRowBlockVideos;"),
    "text_ffn": ("vqf_capi.hip", r"TB = Tt < kTextFfnRows \? Tt : kTextFfnRows;"),
    "merge": ("vqf_capi.hip", r"m0 \+= kMergeRows\)"),
    "mean_table": ("vqf_kernels.hip", r"v0 \+= kMeanSegs\)"),
    "copy_rows": ("vqf_kernels.hip", r"s0 \+= kRowSegs\)"),
    "attn_group": ("vqf_kernels.hip", r"b0 \+= kVcAttnGroup\)"),
    "video_group": ("ltm_capi.hip", r"group = V < kVideoGroup \? V : kVideoGroup;"),
    "short_nb": ("vqf_capi.hip", r"if \(C > (\d+)\) \{"),
}


def seam_constants(csrc: str = CSRC) -> Dict[str, object]:
    """{seam: size} parsed from the sources (``short_nb``: the (lowest, highest) sub-batch size ``pick_short_nb`` may pick)."""
    text, out = {}, {}
    read = lambda f: text.setdefault(f, open(os.path.join(csrc, f)).read())
    for name, (f, rx) in _CONSTANTS.items():
        m = re.findall(rx, read(f))
        if len(m) != 1:
            raise ValueError(f"seam constant {name}: {len(m)} matches of /{rx}/ in {f}")
        out[name] = tuple(int(x) for x in m[0]) if isinstance(m[0], tuple) else int(m[0])
    for name, (f, *rxs) in _USES.items():
        for rx in rxs:
            if not re.search(rx, read(f)):
                raise ValueError(f"seam constant {name}: its site /{rx}/ is not in {f}")
    lo = re.search(_USES["short_nb"][1], read("vqf_capi.hip"))
    if int(lo.group(1)) != out["short_nb"][0]:
        raise ValueError("pick_short_nb: the threshold `C > n` and the lowest sub-batch size differ")
    return out


# ------------------------------------------------------------------------------------------------ shapes
# the small VideoChat2 shape of tests/test_vc_videos_gpu.py; a layout changes only what it states
BASE = dict(hidden=128, heads=2, inter=256, enc_width=64, P=4, T=16, N=32, proj=64, n_layers=4, cross_freq=2, n_query=40,
            texts=(5, 0, 17), counts=(2, 0, 3), alpha=0.75, sticky=True, tau=0.75)
# the smallest shape the raw C ABI of the video Q-former takes (tests/test_config_sweep_gpu.py's style)
VQF_BASE = dict(hidden=128, heads=2, inter=256, enc_width=64, P=32, T=4, N=64, proj=64, n_layers=2, n_query=32, alpha=0.9,
                sticky=True, tau=0.75)
ATTN = dict(H=2, nb=258, n_max=65, n_valid_cycle=(1, 31, 32, 33, 64, 65), alone=(0, 255, 256, 257))


@dataclass(frozen=True)
class Layout:
    name: str
    path: str                          # "vc": infv_vqf_vc_encode_videos, "vqf": infv_vqf_encode_videos
    shape: dict
    counts: Tuple[int, ...]            # chunks of every video
    text_len: Tuple[int, ...]          # text tokens of every video ("vqf": all 0)
    probes: Tuple[int, ...]            # videos with an oracle, placed across the seams in `probed`
    claims: Tuple[str, ...]            # every seam the call crosses
    probed: Tuple[str, ...]            # the seams a probe must have something on both sides of
    want_hidden: bool = True
    alone_crosses: Tuple[Tuple[int, Tuple[str, ...]], ...] = ()   # videos whose run alone still crosses a seam (stated, not hidden)

    @property
    def cu(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    @property
    def n_chunks(self) -> int:
        return int(sum(self.counts))

    def alone(self, v: int) -> "Layout":
        """Video ``v`` as a call of its own (V = 1)."""
        return Layout(f"{self.name}[{v}]", self.path, self.shape, (self.counts[v],), (self.text_len[v],), (), (), (), self.want_hidden)


def _fill(pattern, texts, chunk_probes, video_probes, min_chunks, min_videos, probe_text, last_is_probe=False):
    """Counts / text lengths / probe indices: fillers cycle through ``pattern`` and ``texts``; ``chunk_probes`` {first chunk: n}
    places a probe video of n chunks that starts at exactly that chunk, ``video_probes`` {video: n} one at that video index."""
    counts, text, probes = [], [], []
    c = i = 0
    pending = dict(chunk_probes)
    while c < min_chunks or len(counts) < min_videos or pending or any(v >= len(counts) for v in video_probes):
        v = len(counts)
        nxt = min(pending) if pending else None
        if v in video_probes:
            n, probe = video_probes[v], True
        elif nxt is not None and c == nxt:
            n, probe = pending.pop(nxt), True
        else:
            n, probe = pattern[i % len(pattern)], False
            if nxt is not None:
                n = min(n, nxt - c)
        assert nxt is None or c + (0 if probe and c == nxt else n) <= nxt or probe and c == nxt, "a probe overran a chunk target"
        counts.append(n)
        text.append(probe_text[len(probes) % len(probe_text)] if probe else texts[i % len(texts)])
        if probe:
            probes.append(v)
        else:
            i += 1
        c += n
    if last_is_probe:
        counts.append(1), text.append(probe_text[len(probes) % len(probe_text)]), probes.append(len(counts) - 1)
    return tuple(counts), tuple(text), tuple(probes)


def _layouts() -> Dict[str, Layout]:
    out = {}
    # row blocks of the token GEMMs / the self-attention and the copy-row tables (VC): boundaries 128 and 256 inside the call
    c, t, p = _fill((1, 3, 0, 4, 2, 2, 0, 1), (5, 0, 17, 40, 5, 17), {127: 3, 255: 3}, {}, 300, 0, probe_text=(17, 5))
    out["vc_row_blocks"] = Layout("vc_row_blocks", "vc", dict(BASE), c, t, p, ("row_block", "copy_rows", "short_nb"),
                                  ("row_block", "copy_rows"))
    # lockstep video groups and the per-video mean table (VC): 0 to 2 chunks, few enough that no row block ends inside
    c, t, p = _fill((1, 0, 0, 2, 0, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0, 5), {}, {255: 2, 256: 1}, 0, 260, probe_text=(17, 5, 40),
                    last_is_probe=True)
    out["vc_video_groups"] = Layout("vc_video_groups", "vc", dict(BASE), c, t, p, ("video_group", "mean_table", "short_nb"),
                                    ("video_group", "mean_table"))
    # blocks of the text FFN (VC): A fills 15000 text rows, B's second chunk straddles row 16384, hidden_out requested
    out["vc_text_ffn"] = Layout("vc_text_ffn", "vc", dict(BASE), (30, 3, 2), (500, 500, 7), (1,), ("text_ffn", "short_nb"),
                                ("text_ffn",), alone_crosses=((0, ("short_nb",)),))
    # launches of the alpha-merge epilogue (VC, n_query 40): row 32768 falls inside chunk 819; fillers of 8 chunks, which a run
    # alone takes in one short-attention sub-batch
    c, t, p = _fill((8,), (0,), {818: 3}, {}, 830, 0, probe_text=(5,))
    out["vc_merge"] = Layout("vc_merge", "vc", dict(BASE), c, t, p, ("merge", "row_block", "copy_rows", "short_nb"), ("merge",))
    # the video Q-former through the raw ABI: row blocks, mean table and video groups in one call (layer 1 steps the memories
    # with per-chunk queries) ...
    c, t, p = _fill((1, 2, 0, 1, 1, 3, 1, 0), (0,), {127: 3}, {255: 2, 256: 1}, 300, 260, probe_text=(0,))
    out["vqf_blocks_groups"] = Layout("vqf_blocks_groups", "vqf", dict(VQF_BASE), c, t, p,
                                      ("row_block", "mean_table", "video_group", "short_nb"), ("row_block", "mean_table", "video_group"))
    # ... and the merge epilogue (Q 32: row 32768 is the first row of chunk 1024)
    c, t, p = _fill((8,), (0,), {1023: 3}, {}, 1030, 0, probe_text=(0,))
    out["vqf_merge"] = Layout("vqf_merge", "vqf", dict(VQF_BASE), c, t, p, ("merge", "row_block", "short_nb"), ("merge",))
    return out


LAYOUTS = _layouts()


# ------------------------------------------------------------------------------------------------ where a layout meets the seams
def _units(lay: Layout) -> Dict[str, int]:
    """How far the call reaches along the unit each seam counts in."""
    Q = lay.shape["n_query"]
    C, V = lay.n_chunks, len(lay.counts)
    ltm = lay.shape["alpha"] != 1.0
    text_rows = int(sum(n * t for n, t in zip(lay.counts, lay.text_len)))
    return {"row_block": C, "copy_rows": C if lay.path == "vc" else 0, "mean_table": V, "video_group": V if ltm else 0,
            "text_ffn": text_rows if lay.path == "vc" else 0, "merge": C * Q if ltm else 0}


def boundaries(lay: Layout, k: Dict[str, object]) -> Dict[str, List[int]]:
    """{seam: the indices (chunk, video, text row or query row) at which a new piece starts inside the call}.  ``attn_group`` is
    met through the encoders only where a row block is longer than a group; ``short_nb`` lists the lowest and highest sub-batch
    size when the call has more chunks than that size (which size is taken depends on the device-side tile counts)."""
    out = {}
    for name, n in _units(lay).items():
        out[name] = list(range(k[name], n, k[name]))
    C = lay.n_chunks
    out["attn_group"] = list(range(k["attn_group"], min(C, k["row_block"]), k["attn_group"])) if lay.path == "vc" else []
    out["short_nb"] = [nb for nb in k["short_nb"] if C > nb]
    return out


def crossed(lay: Layout, k: Dict[str, object]) -> Tuple[str, ...]:
    return tuple(sorted(name for name, b in boundaries(lay, k).items() if b))


def straddles(lay: Layout, seam: str, b: int) -> Optional[Tuple[int, int]]:
    """The probes (video before, video after) that hold the units ``b - 1`` and ``b`` of ``seam``; None if no probe does."""
    cu, Q = lay.cu, lay.shape["n_query"]
    if seam in ("mean_table", "video_group"):                   # video slots: both neighbours are probes with chunks
        ok = b - 1 in lay.probes and b in lay.probes and lay.counts[b - 1] > 0 and lay.counts[b] > 0
        return (b - 1, b) if ok else None
    for p in lay.probes:
        if seam in ("row_block", "copy_rows", "attn_group"):
            lo, hi = cu[p], cu[p + 1]
        elif seam == "merge":
            lo, hi = cu[p] * Q, cu[p + 1] * Q
        elif seam == "text_ffn":                                # one chunk's text rows on both sides
            t0 = int(sum(n * t for n, t in zip(lay.counts[:p], lay.text_len[:p])))
            hit = [c for c in range(lay.counts[p]) if t0 + c * lay.text_len[p] <= b - 1 and b < t0 + (c + 1) * lay.text_len[p]]
            lo, hi = (b - 1, b + 1) if hit else (0, 0)
        else:
            raise KeyError(seam)
        if lo <= b - 1 and b < hi:
            return (p, p)
    return None


def text_rows_before(lay: Layout, chunk: int) -> int:
    """Packed text rows of the chunks before ``chunk`` (``toff[chunk]`` of the C side)."""
    per_chunk = np.repeat(np.asarray(lay.text_len), np.asarray(lay.counts))
    return int(per_chunk[:chunk].sum())


def spread(lay: Layout, k: Dict[str, object], n_interior: int = 3) -> Tuple[int, ...]:
    """The fixed set of non-probe videos that are re-run alone: the first and last video with chunks of every video group and of
    the row blocks that matter (the first, the last and every one a probe has chunks in), and a few interior ones."""
    cu = lay.cu
    has = [v for v, n in enumerate(lay.counts) if n > 0 and v not in lay.probes]
    pick = set()
    edges = sorted(set([0] + boundaries(lay, k)["row_block"] + [lay.n_chunks]))
    blocks = list(zip(edges[:-1], edges[1:]))
    for i, (lo, hi) in enumerate(blocks):                       # row blocks: by chunk
        if i not in (0, len(blocks) - 1) and not any(cu[p] < hi and cu[p + 1] > lo for p in lay.probes):
            continue
        inside = [v for v in has if cu[v] < hi and cu[v + 1] > lo]
        pick.update(inside[:1] + inside[-1:])
    edges = sorted(set([0] + boundaries(lay, k)["video_group"] + [len(lay.counts)]))
    for lo, hi in zip(edges[:-1], edges[1:]):                   # video groups: by video
        inside = [v for v in has if lo <= v < hi]
        pick.update(inside[:1] + inside[-1:])
    rest = [v for v in has if v not in pick]
    pick.update(rest[(i + 1) * len(rest) // (n_interior + 1)] for i in range(n_interior) if rest)
    return tuple(sorted(pick))


# ------------------------------------------------------------------------------------------------ inputs
_weights = {}


def layout_weights(lay: Layout) -> dict:
    s = lay.shape
    key = (lay.path,) + tuple(sorted((a, b) for a, b in s.items() if not isinstance(b, tuple)))
    if key not in _weights:
        if lay.path == "vc":
            _weights[key] = synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"],
                                                             s["n_query"], s["proj"], seed=synth.SEED_VC + 31)
        else:
            _weights[key] = synth.video_qformer_weights(n_layers=s["n_layers"], hidden=s["hidden"], inter=s["inter"],
                                                        enc_width=s["enc_width"], n_query=s["n_query"], proj_out=s["proj"])
    return _weights[key]


def small_video(s, v, n_chunks, n_text, w=None):
    """(chunks [C, T*P, width], encoder input rows [n_query + n_text, hidden]) of synthetic video ``v``."""
    k = np.stack([synth.frame_tokens(c, s["T"], s["P"], s["enc_width"], seed=synth.SEED_K + 1000 * (v + 1)) for c in range(n_chunks)]) \
        if n_chunks else np.zeros((0, s["T"] * s["P"], s["enc_width"]), np.float32)
    if w is None:
        w = synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"], s["n_query"],
                                             s["proj"], seed=synth.SEED_VC + 31)
    rows = [w["query_tokens"][0] * np.float32(50.0)]
    if n_text:
        rows.append(synth.layer_query(40 + v, n_text, s["hidden"]))
    return k, np.concatenate(rows, 0).astype(np.float32)


def layout_video(lay: Layout, v: int):
    """(chunks, encoder input rows or None) of video ``v`` of a layout."""
    if lay.path == "vc":
        return small_video(lay.shape, v, lay.counts[v], lay.text_len[v], layout_weights(lay))
    s = lay.shape
    n = lay.counts[v]
    k = np.stack([synth.frame_tokens(c, s["T"], s["P"], s["enc_width"], seed=synth.SEED_K + 1000 * (v + 1)) for c in range(n)]) \
        if n else np.zeros((0, s["T"] * s["P"], s["enc_width"]), np.float32)
    return k, None


def n_cross_of(s):
    return len(range(0, s["n_layers"], s.get("cross_freq", 1)))


# ------------------------------------------------------------------------------------------------ oracle-side helpers
def draw_margins(probs, u):
    """Distance of every uniform to the nearest edge of the oracle's fp32 cdf (``inverse_cdf_draw``'s construction)."""
    probs = np.asarray(probs, np.float32)
    run, cdf = np.float32(0), np.empty(len(probs), np.float32)
    for j in range(len(probs)):
        run = np.float32(run + probs[j])
        cdf[j] = run
    cdf = (cdf / run).astype(np.float32)
    cdf[-1] = np.float32(1)
    edges = np.concatenate([[0.0], cdf.astype(np.float64)])
    return np.abs(np.asarray(u, np.float64)[:, None] - edges[None, :]).min(1)


class OracleRun:
    """One video through ``VideoChat2Oracle`` (or, with ``h0 = None``, ``VideoQformerOracle``) chunk by chunk, keeping per chunk the
    outputs and per LTM step the oracle's own bins and margins.  ``bins`` [C][n_cross][S] hands every LTM step those bins
    (``ClosedFormOracle.step``'s ``bins_override``); ``safe_rng``: draw the uniforms here, step by step, re-drawing any that
    falls within MARGIN of an edge of the oracle's cdf."""

    def __init__(self, orc, chunks, h0, u=None, bins=None, safe_rng=None):
        self.hidden, self.proj, self.bins, self.margin, self.u = [], [], [], [], []
        layers = sorted(orc.ltm) if isinstance(orc.ltm, dict) else list(range(len(orc.ltm)))
        state = {"c": 0}
        rec_b, rec_m, rec_u = {}, {}, {}

        def patched(j, o):
            def step(k, q, new_doc, uu=None):
                stepping = o.sticky and o.B_past is not None and not new_doc
                if stepping and safe_rng is not None:
                    probs = categorical_probs(torch.from_numpy(o.sticky_p_raw(o.S_prev))).numpy()
                    uu = safe_rng.random(S)
                    for _ in range(64):
                        bad = draw_margins(probs, uu) < MARGIN
                        if not bad.any():
                            break
                        uu[bad] = safe_rng.random(int(bad.sum()))
                ov = None if bins is None or not stepping else bins[state["c"]][j]
                out = ClosedFormOracle.step(o, k, q, new_doc, uu, bins_override=ov)
                if stepping:
                    rec_b[j], rec_m[j], rec_u[j] = o.last_bins.copy(), draw_margins(o.last_probs, uu), np.asarray(uu).copy()
                return out
            return step

        for j, l in enumerate(layers):
            orc.ltm[l].step = patched(j, orc.ltm[l])
        try:
            for c, k in enumerate(chunks):
                state["c"] = c
                rec_b.clear(), rec_m.clear(), rec_u.clear()
                uc = None if u is None else u[c]
                hid, pr = orc.encode_chunk(k, c == 0, uc) if h0 is None else orc.encode_chunk(k, h0, c == 0, uc)
                self.hidden.append(hid)
                self.proj.append(pr)
                self.bins.append([rec_b.get(j) for j in range(len(layers))])
                self.margin.append([rec_m.get(j) for j in range(len(layers))])
                self.u.append([rec_u.get(j) for j in range(len(layers))])
        finally:
            for l in layers:
                del orc.ltm[l].step
        self.B = [None if orc.ltm[l].B_past is None else np.asarray(orc.ltm[l].B_past).copy() for l in layers]
        self.Bsum = [None if b is None else b.astype(np.float64).sum(1) for b in self.B]


def small_oracle(s, w):
    return VideoChat2Oracle(w, s["N"], s["tau"], s["alpha"], s["sticky"], s["n_layers"], s["cross_freq"], s["heads"], s["n_query"], s["P"])


def vqf_oracle(s, w):
    return VideoQformerOracle(w, s["N"], s["tau"], s["alpha"], s["sticky"], n_layers=s["n_layers"], n_heads=s["heads"],
                              tokens_per_frame=s["P"])


def small_reference(s, w, vids, seed, make_oracle=small_oracle):
    """Oracle runs of the videos with uniforms drawn step by step so that every margin is at least MARGIN (asserted).  With
    ~127 cdf edges a uniform falls within 2e-5 of one with probability ~0.5 %, so no seed of a plain generator clears the
    thousands of draws of a run: the uniforms that would are re-drawn, deterministically from ``seed``."""
    runs, us = [], []
    nx = n_cross_of(s)
    for v, (k, h0) in enumerate(vids):
        orun = OracleRun(make_oracle(s, w), list(k), h0, safe_rng=np.random.default_rng(seed + v))
        u = np.zeros((len(k), nx, S))
        for c in range(len(k)):
            for j in range(nx):
                if orun.u[c][j] is not None:
                    u[c, j] = orun.u[c][j]
                    assert float(orun.margin[c][j].min()) >= MARGIN          # the precondition of exact draws
        runs.append(orun)
        us.append(u)
    return runs, np.concatenate(us)


_references = {}


def probe_reference(lay: Layout):
    """{probe video: (OracleRun, its uniforms [C_v, n_cross, S])}, once per session (shared, never modified): only probes get an
    oracle, fillers do not."""
    if lay.name not in _references:
        w = layout_weights(lay)
        out = {}
        for p in lay.probes:
            runs, u = small_reference(lay.shape, w, [layout_video(lay, p)], seed=7000 + 13 * p,
                                      make_oracle=small_oracle if lay.path == "vc" else vqf_oracle)
            out[p] = (runs[0], u)
        _references[lay.name] = out
    return _references[lay.name]


def layout_uniforms(lay: Layout, seed: int = 4100) -> np.ndarray:
    """[C, n_cross, S] float64 of the whole call: the probes' margin-safe uniforms at their chunks, a plain generator elsewhere."""
    u = np.random.default_rng(seed).random((lay.n_chunks, n_cross_of(lay.shape), S))
    cu = lay.cu
    for p, (_, up) in probe_reference(lay).items():
        u[cu[p]:cu[p + 1]] = up
    return u
