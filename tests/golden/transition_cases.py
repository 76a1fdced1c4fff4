"""Sequences of LTM entry points that carry ONE memory from call to call, as data: which operation starts a document, what
hands the memory on, which operation continues it -- every ordered pair of the six operations, the two hand-offs between
engines, and the variants in which the query length, the query values or the weights change at the seam.  A data module like
``sweep_cases.py`` and ``seam_cases.py``: no fixtures, inputs from ``infinite_video_amd.synth``, expected values from
``oracle.ltm_oracle.ClosedFormOracle`` at test time (``oracle_run``), with the Gibbs uniforms drawn step by step so that every
draw keeps ``seam_cases.MARGIN`` to the edges of the oracle's cdf.  ``tests/test_path_transitions_cpu.py`` checks the table
itself, ``tests/test_path_transitions_gpu.py`` drives it through the library.  Pure Python: nothing here touches a device.

A sequence runs two documents: A in legs of 3 + 3 + 1 chunks, B in legs of 1 + 2 + 1 -- B's first leg is only the document's
first chunk, so the first draw of its second leg finds what a first-chunk-only call left behind.  Leg X starts the document
(``new_doc``), leg Y continues it, and a closing ``fwd`` of one chunk consumes everything Y left (histogram, K', ``cur``)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from infinite_video_amd import synth
from oracle.ltm_oracle import ClosedFormOracle, categorical_probs
from tests.golden import cases as gc
from tests.golden import sweep_cases as sw
from tests.golden.seam_cases import MARGIN, draw_margins

# ------------------------------------------------------------------------------------------------ operations and hand-offs
OPS = ("fwd", "cons", "pooled", "cons_q", "vid", "vid_q")
PER_CHUNK_Q = ("cons_q", "vid_q")                   # a different query per chunk; the others share one query per call
LOCKSTEP = ("vid", "vid_q")                         # both documents' engines in one call (+ a bystander when continuing)
TRACED = ("cons", "pooled", "vid", "vid_q")         # set_trace returns every chunk's draw (fused chain and lockstep kernels)
CHAIN_EXPORTERS = ("cons", "pooled")                # export_chain_state is legal after these, on a fused-chain shape
HANDOFFS = ("state", "chain")
VARIANTS = ("q32_q16", "q16_q32", "qvals", "weights")
VARIANT_PAIRS = (("fwd", "cons"), ("cons", "cons"), ("vid", "cons"), ("cons", "vid"), ("cons", "cons_q"))
DOC_LEGS = ((3, 3, 1), (1, 2, 1))                   # documents A and B: chunks of leg X, leg Y and the closing fwd
MAX_BATCH_CHUNKS = 2                                # a 3-chunk leg spans two sub-batches

# ------------------------------------------------------------------------------------------------ shapes
# the smallest at which each kernel family is reached; every value is a one-factor point of sweep_cases.py
_FAST = replace(sw.SMALL, name="fast", gate="transitions", families="fast", N=64, H=4, d=96, P=7, S=512, T=8, L=2, Q=32,
                max_batch_chunks=MAX_BATCH_CHUNKS)
SHAPES: Dict[str, sw.SweepPoint] = {
    "fast": _FAST,
    "fast_tabw4": replace(_FAST, name="fast_tabw4", N=256),
    "stages": replace(_FAST, name="stages", families="stages", H=3),
    "uniform": replace(_FAST, name="uniform", sticky=False),
}
# what each shape is there for: (families of `cons`, substrings of sweep_cases.expected_path)
CLAIMS = {
    "fast": ("fast", ("chain_batch3", "+uc+")),
    "fast_q16": ("fast", ("chain_batch3", "+uc+")),          # `fast` called with Q 16 (L*H*Q = 128)
    "fast_tabw4": ("fast", ("chain_batch3", "+uc_fast+")),
    "stages": ("stages", ("stages:attend_small",)),
    "uniform": ("fast", ("chain_batch+", "+uc+")),
}


def claimed_point(claim: str) -> sw.SweepPoint:
    return replace(SHAPES["fast"], name="fast_q16", Q=16) if claim == "fast_q16" else SHAPES[claim]


# ------------------------------------------------------------------------------------------------ sequences
@dataclass(frozen=True)
class Sequence:
    name: str
    shape: str
    x: str
    y: str
    handoff: Optional[str] = None      # None: the same engine goes on; "state" / "chain": a fresh engine receives the memory
    variant: Optional[str] = None


QSpec = Tuple[str, int, int]           # ("shared" | "chunk", Q, value set)


@dataclass(frozen=True)
class Leg:
    op: str
    chunks: Tuple[int, ...]            # chunk ids of the document
    q: Tuple[QSpec, ...]               # the query of every chunk
    w: int                             # weight set
    new_doc: bool


def _sequences() -> List[Sequence]:
    out = [Sequence(f"fast:{x}-{y}", "fast", x, y) for x in OPS for y in OPS]
    for shape in ("fast_tabw4", "stages"):
        out += [Sequence(f"{shape}:{x}-{y}", shape, x, y) for x in OPS for y in OPS if {x, y} & {"fwd", "cons"}]
    out += [Sequence(f"uniform:{x}-cons", "uniform", x, "cons") for x in OPS]
    out += [Sequence(f"fast:{x}>state>{y}", "fast", x, y, handoff="state") for x in ("fwd", "cons", "vid") for y in ("fwd", "cons", "vid")]
    out += [Sequence(f"fast:cons>chain>{y}", "fast", "cons", y, handoff="chain") for y in OPS]
    out += [Sequence("fast:pooled>chain>cons", "fast", "pooled", "cons", handoff="chain")]
    out += [Sequence(f"fast:{x}-{y}:{v}", "fast", x, y, variant=v) for (x, y) in VARIANT_PAIRS for v in VARIANTS]
    return out


SEQUENCES = _sequences()
BY_NAME = {s.name: s for s in SEQUENCES}


def _qspecs(op: str, chunks, Q: int, values: int) -> Tuple[QSpec, ...]:
    return tuple(("chunk" if op in PER_CHUNK_Q else "shared", Q, values) for _ in chunks)


def legs_of(seq: Sequence, doc: int) -> Tuple[Leg, Leg, Leg]:
    """(leg X, leg Y, the closing fwd) of document ``doc``.  The closing fwd uses the base query (Q 32, value set 0) and leg Y's
    weights."""
    nx, ny, nz = DOC_LEGS[doc]
    cx, cy, cz = tuple(range(nx)), tuple(range(nx, nx + ny)), tuple(range(nx + ny, nx + ny + nz))
    Q = SHAPES[seq.shape].Q
    qx = qy = Q
    vy = wy = 0
    if seq.variant == "q32_q16":
        qy = 16
    elif seq.variant == "q16_q32":
        qx = 16
    elif seq.variant == "qvals":
        vy = 1
    elif seq.variant == "weights":
        wy = 1
    return (Leg(seq.x, cx, _qspecs(seq.x, cx, qx, 0), 0, True), Leg(seq.y, cy, _qspecs(seq.y, cy, qy, vy), wy, False),
            Leg("fwd", cz, _qspecs("fwd", cz, Q, 0), wy, False))


def schedule_of(seq: Sequence, doc: int):
    """Per chunk (query spec, weight set): all an oracle run depends on besides the shape and the document."""
    return tuple((q, leg.w) for leg in legs_of(seq, doc) for q in leg.q)


# ------------------------------------------------------------------------------------------------ inputs
def tokens(pt: sw.SweepPoint, doc: int, chunk: int) -> np.ndarray:
    return synth.frame_tokens(chunk, pt.T, pt.P, pt.d, seed=synth.SEED_K + 1000 * (doc + 1))


def query(pt: sw.SweepPoint, spec: QSpec, doc: int, chunk: int) -> np.ndarray:
    """[L, Q, dm] of one chunk: a shared query depends on its value set only, a per-chunk one also on document and chunk."""
    kind, Q, values = spec
    seed = synth.SEED_Q + 7 * values if kind == "shared" else synth.SEED_Q + 100 + 1000 * values + 10 * chunk + doc
    return np.stack([synth.layer_query(l, Q, pt.dm, seed=seed) for l in range(pt.L)])


def weights(pt: sw.SweepPoint, wset: int):
    return [synth.layer_projections(l, pt.d, pt.dm, seed=synth.SEED_W + 50 * wset) for l in range(pt.L)]


BYSTANDER_DOC, BYSTANDER_CHUNKS = 2, 2              # the unrelated memory of the third engine: two fwd steps of a third document


def bystander_uniforms(pt: sw.SweepPoint) -> np.ndarray:
    return synth.gibbs_uniforms(BYSTANDER_CHUNKS, pt.L, seed=synth.SEED_U + 5, nb_samples=pt.S)


# ------------------------------------------------------------------------------------------------ oracle runs
class Run:
    """One document under one schedule through the oracle, chunk by chunk.  Per chunk: ctx [L, Q, dm], B [L, N, d] after it and,
    from the second chunk of a sticky memory on, the uniforms u [L, S], the oracle's bins [L, S], probabilities [L, 127] and the
    smallest margin.  ``scores`` [L][H, Q, N]: the last step's.  ``excluded``: draws a comparison would have to leave out (margin
    below MARGIN after the re-draws) -- the CPU test asserts 0."""

    def __init__(self, pt: sw.SweepPoint, doc: int, sched):
        self.ctx, self.B, self.u, self.bins, self.probs, self.margin = [], [], [], [], [], []
        self.draws = self.excluded = self.redrawn = 0
        rng = np.random.default_rng(zlib.crc32(repr((pt.name, doc, sched)).encode()))
        orcs = [ClosedFormOracle(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, *weights(pt, 0)[l], tokens_per_frame=pt.P, nb_samples=pt.S)
                for l in range(pt.L)]
        w_now = 0
        for c, (spec, wset) in enumerate(sched):
            if wset != w_now:
                # the oracle re-projects K and V from B_past in every step (ClosedFormOracle.step), so new weights are new attributes
                for l, o in enumerate(orcs):
                    o.wk, o.bk, o.wv, o.bv = (np.asarray(a, np.float32) for a in weights(pt, wset)[l])
                w_now = wset
            k, q = tokens(pt, doc, c), query(pt, spec, doc, c)
            ctx, u, bins, probs, margin = [], [], [], [], np.inf
            for l, o in enumerate(orcs):
                uu = None
                if c and pt.sticky:
                    p = categorical_probs(torch.from_numpy(o.sticky_p_raw(o.S_prev))).numpy()
                    uu = rng.random(pt.S)
                    for _ in range(64):
                        bad = draw_margins(p, uu) < MARGIN
                        if not bad.any():
                            break
                        self.redrawn += int(bad.sum())
                        uu[bad] = rng.random(int(bad.sum()))
                ctx.append(o.step(k, q[l], new_doc=(c == 0), u=uu))
                if uu is not None:
                    m = draw_margins(o.last_probs, uu)
                    self.draws += pt.S
                    self.excluded += int((m < MARGIN).sum())
                    margin = min(margin, float(m.min()))
                    u.append(uu), bins.append(o.last_bins.copy()), probs.append(np.asarray(o.last_probs, np.float32).copy())
            self.ctx.append(np.stack(ctx))
            self.B.append(np.stack([o.B_past for o in orcs]))
            self.u.append(np.stack(u) if u else None)
            self.bins.append(np.stack(bins) if bins else None)
            self.probs.append(np.stack(probs) if probs else None)
            self.margin.append(margin)
        self.scores = [o.S_prev.copy() for o in orcs]


_runs: Dict[tuple, Run] = {}


def oracle_run(seq: Sequence, doc: int) -> Run:
    """Cached by (shape, document, schedule): the 36 pairs of a shape share four runs per document.  Shared, never modified."""
    key = (seq.shape, doc, schedule_of(seq, doc))
    if key not in _runs:
        _runs[key] = Run(SHAPES[seq.shape], doc, key[2])
    return _runs[key]


def run_keys() -> List[tuple]:
    """Every distinct oracle run of the table, as (sequence that needs it, document)."""
    seen, out = set(), []
    for s in SEQUENCES:
        for doc in range(len(DOC_LEGS)):
            key = (s.shape, doc, schedule_of(s, doc))
            if key not in seen:
                seen.add(key)
                out.append((s, doc))
    return out


# ------------------------------------------------------------------------------------------------ dense plans: the goldens
# On a dense plan every operation falls back to the per-chunk dense step; the sticky cases of DENSE_CASES carry their own
# inputs, uniforms (cases.call_uniforms) and expected values (the reference's run, tests/golden/*.npz).
DENSE_OPS = ("fwd", "cons", "cons_q", "vid")
DENSE_STICKY = tuple(c for c in gc.DENSE_CASES if c.sticky)


@dataclass(frozen=True)
class DenseSequence:
    name: str
    case: str
    x: str
    y: str
    cut: int                           # leg X: chunks [0, cut), leg Y: the rest


DENSE_SEQUENCES = [DenseSequence(f"dense:{c.name}:{x}-{y}@{cut}", c.name, x, y, cut)
                   for c in DENSE_STICKY for cut in range(1, len(c.chunk_T)) for x in DENSE_OPS for y in DENSE_OPS]
DENSE_BY_NAME = {c.name: c for c in DENSE_STICKY}

assert len({s.name for s in SEQUENCES} | {s.name for s in DENSE_SEQUENCES}) == len(SEQUENCES) + len(DENSE_SEQUENCES)


# ------------------------------------------------------------------------------------------------ one level up: the video Q-former
# Its three entry points reach the LTM through different calls (encode_chunk: a per-call step per layer; encode_video:
# consolidate_pooled on layer 0 and steps on the later layers; encode_videos: steps_videos) and share the layer-0 prefix cache
# (infv_vqf_set_weights_epoch).  Shape: seam_cases.VQF_BASE, the smallest the raw C ABI takes.
VQF_OPS = ("chunk", "video", "videos")
VQF_LEGS = (2, 2, 1)                                # leg X, leg Y, one closing encode_chunk
VQF_VIDEOS = 2                                      # both go through every operation; `videos` takes them in one call
VQF_PREFIX_WEIGHT = "bert.embeddings.LayerNorm.weight"       # (scaling the query tokens themselves would vanish in that LayerNorm)


@dataclass(frozen=True)
class VqfSequence:
    name: str
    x: str
    y: str
    epoch: bool = False                # a prefix weight changes between the legs and the epoch is bumped


VQF_SEQUENCES = [VqfSequence(f"vqf:{x}-{y}", x, y) for x in VQF_OPS for y in VQF_OPS] + \
                [VqfSequence("vqf:chunk-chunk:epoch", "chunk", "chunk", epoch=True), VqfSequence("vqf:video-chunk:epoch", "video", "chunk", epoch=True)]
VQF_BY_NAME = {s.name: s for s in VQF_SEQUENCES}


def vqf_weights(changed: bool = False) -> dict:
    from tests.golden import seam_cases as sc
    s = sc.VQF_BASE
    w = dict(synth.video_qformer_weights(n_layers=s["n_layers"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                                         n_query=s["n_query"], proj_out=s["proj"]))
    if changed:
        w[VQF_PREFIX_WEIGHT] = (np.asarray(w[VQF_PREFIX_WEIGHT], np.float32) * np.float32(1.25)).astype(np.float32)
    return w


def vqf_chunks(v: int) -> np.ndarray:
    from tests.golden import seam_cases as sc
    s = sc.VQF_BASE
    return np.stack([synth.frame_tokens(c, s["T"], s["P"], s["enc_width"], seed=synth.SEED_K + 1000 * (v + 1)) for c in range(sum(VQF_LEGS))])


_vqf_refs: Dict[bool, list] = {}


def vqf_reference(epoch: bool):
    """Per video (OracleRun, uniforms [chunks, layers, S]) with every margin at MARGIN or more (seam_cases.small_reference's
    construction); ``epoch``: from the first chunk of leg Y on the oracle holds the changed prefix weight."""
    from tests.golden import seam_cases as sc
    if epoch not in _vqf_refs:
        s, nx, out = sc.VQF_BASE, sc.n_cross_of(sc.VQF_BASE), []
        for v in range(VQF_VIDEOS):
            k = vqf_chunks(v)
            orc = sc.vqf_oracle(s, vqf_weights())

            def chunks(orc=orc, k=k):
                for c, kc in enumerate(k):
                    if epoch and c == VQF_LEGS[0]:
                        orc.w = {a: torch.from_numpy(np.asarray(b, np.float32)) for a, b in vqf_weights(True).items()}
                    yield kc

            orun = sc.OracleRun(orc, chunks(), None, safe_rng=np.random.default_rng(9100 + v))
            u = np.zeros((len(k), nx, sc.S))
            for c in range(len(k)):
                for j in range(nx):
                    if orun.u[c][j] is not None:
                        u[c, j] = orun.u[c][j]
            out.append((orun, u))
        _vqf_refs[epoch] = out
    return _vqf_refs[epoch]
