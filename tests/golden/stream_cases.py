"""The stream-order cases, as data: every entry point that takes a ``void* stream`` run on a side stream with work in flight
around it (``tests/test_stream_order_gpu.py`` has the method and one scenario per case; ``tests/test_stream_order_cpu.py`` checks
this table against the two headers).

A case names the C entry points it drives, its shape, the device inputs it poisons and the host-side mechanism it is there to
cross.  ``poisoned`` inputs are preallocated, hold a DECOY while the caller's stream is still busy with a delay, receive the good
values by a copy queued on that stream ahead of the call, and are overwritten with the decoy again right behind it.  A decoy is a
second finite draw of the generator the good values come from (``infinite_video_amd.synth`` under another seed): a misordered read
gives other valid numbers, never a bad index.  No decoy is NaN or Inf and a decoy of uniforms stays in [0, 1).

Nothing here touches a device."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from infinite_video_amd import synth
from tests.golden import dense_sweep_cases as dc
from tests.golden import seam_cases as sm
from tests.golden import sweep_cases as sc
from tests.golden.frame_qformer_cases import SMALL as FRAME_SMALL

DECOY = 50021                   # added to a generator's seed for the decoy draw
FRAME_TOKENS = 65               # tokens per frame of the frame Q-former cases: one whole 64-token tile and a tail of one
RAGGED = (3, 1, 4, 2, 5)        # chunks of the five videos of the lockstep cases
VQF_RAGGED = (2, 1, 3)          # chunks of the three videos of infv_vqf_encode_videos

# ---------------------------------------------------------------------------------------------------------------------
# the mechanisms (host code that orders work across streams, or holds state between calls), and why each is here
# ---------------------------------------------------------------------------------------------------------------------
MECHANISMS: Dict[str, str] = {
    "per_chunk_stages": "the per-chunk stage kernels and infv_ltm_pool / _step on the caller's stream (ltm_capi.hip); "
                        "consolidate_per_chunk for dense and general-psi plans",
    "fork_join": "ltm_consolidate.hip forks a call over the process-wide non-blocking streams ucs / pools / side behind ev_start / ev_q "
                 "and joins in consolidate_join on ev_uc",
    "ring_reuse": "sub-batches of one call reuse the workspace sets and ring slots behind ev_p / ev_s / ev_uc / ev_r",
    "flag_wait": "calls of 768+ chunks: one call-long pooling launch, the GEMM stream held by flag_wait_kernel on completion counts",
    "call_seam": "the tail of one consolidate call against the prologue of the next: ev_start, clear_call_events, wv_split_valid",
    "lockstep": "the lockstep multi-video calls: one launch per stage and step on the caller's stream, the video table in the arguments",
    "read_out_after_call": "an export, pack, re-projection or density read-out queued behind a consolidate call with no host sync",
    "create_memsets": "infv_ltm_create clears its state with hipMemset on the null stream, which a non-blocking stream does not wait for",
    "null_stream_setters": "infv_ltm_set_probs / infv_ltm_set_bins copy from the host with no stream argument",
    "shared_streams": "two handles on two caller streams share ucs / pools / side (shared_streams) and process-wide buffers",
    "uniform_ring": "LongTermAttention._draw_uniforms: the draw kernel reads a 64-slot pinned ring guarded by an event every 16 calls",
    "pool_cache": "the drop-in module's _pool_cache: a second module steps from the frame means the first one pooled",
    "vqf_side_stream": "vqf_video.hip / vqf_vc.hip run the memories of the later layers on the shared worker stream under ev_main / ev_side",
    "weights_epoch": "vqf_video.hip caches layer 0's prefix, vqf_capi.hip the weight planes, across calls while the weights epoch stands",
    "ids_staging": "run_embed reuses a pinned id staging buffer behind ev_ids",
    "ln_stats": "infv_vqf_layernorm_tokens keeps its row statistics in a process-wide buffer behind the last_read event",
    "caller_stream_only": "single-stream helpers exported for tests: every launch on the caller's stream",
}
# the mechanisms the issue lists under "Why this is next": each needs a case
REQUIRED_MECHANISMS = ("fork_join", "ring_reuse", "flag_wait", "vqf_side_stream", "ids_staging", "ln_stats", "weights_epoch",
                       "uniform_ring", "null_stream_setters")

# entry points with a `void* stream` that no case drives, and why
EXCLUSIONS: Dict[str, str] = {
    "infv_ltm_sync": "synchronises `stream` by definition; every scenario calls it after the final synchronisation to read the latched error",
    "infv_ltm_get_draw": "copies to HOST buffers and synchronises `stream` by definition; every LTM scenario reads it after the synchronisation",
    "infv_ltm_rng_fill": "one launch on the caller's stream that reads no device input and touches no handle: nothing to order",
}


@dataclass(frozen=True)
class Case:
    name: str
    family: str                    # "ltm" | "dropin" | "vqf" | "vc" | "frame"
    entries: Tuple[str, ...]       # C entry points with a `void* stream` the scenario calls on the side stream
    shape: str
    poisoned: Tuple[str, ...]      # the device inputs that are poisoned before and after the call
    mechanism: str                 # key of MECHANISMS
    delay_ms: float = 40.0         # 0: no delay (the delay cannot hold what the case is about)
    unpoisoned: str = ""           # why an input the call reads is not poisoned (or why none can be)
    host_wait: str = ""            # a host wait the library documents inside the sequence: the issue time is taken up to it


_SMALL = "sweep_cases.SMALL: N 64, T 8, P 32, d 768, L 2, Q 32, sticky, explicit u"
_LTM_IN = ("k", "q", "wk", "bk", "wv", "bv", "u")
_LTM_KBAR = ("kbar", "q", "wk", "bk", "wv", "bv", "u")
_VQF = "seam_cases.VQF_BASE: hidden 128, 2 heads, enc 64, P 32, T 4, N 64, 2 layers, Q 32, alpha 0.9"
_VQF_IN = ("frames", "weights", "u")
_VC = "seam_cases.BASE: hidden 128, 2 heads, enc 64, P 4, T 16, N 32, 4 layers, cross every 2nd, Q 40"
_VC_IN = ("frames", "hidden_in", "weights", "u")
_FRAME = f"frame_qformer_cases.SMALL, 3 frames of {FRAME_TOKENS} tokens"
_PLANES = ("new weights are a new weights epoch, whose first call allocates the cached planes and so synchronises the device: "
           "the warm run builds the planes, the calls under test reuse them")
_MODULE_W = "the module's own nn.Linear parameters are its state, not an argument of the call"


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- LTM
    add("ltm_forward_twice", "ltm", ("infv_ltm_forward",), _SMALL, _LTM_IN, "per_chunk_stages")
    add("ltm_forward_into_twice", "ltm", ("infv_ltm_forward_into",), _SMALL, _LTM_IN, "per_chunk_stages")
    add("ltm_pool_rows_step", "ltm", ("infv_ltm_pool", "infv_ltm_pool_rows", "infv_ltm_step"), _SMALL + ", 3 chunks", _LTM_IN, "per_chunk_stages")
    add("ltm_steps", "ltm", ("infv_ltm_steps",), _SMALL + ", 4 chunks", _LTM_KBAR, "per_chunk_stages")
    add("ltm_consolidate_q", "ltm", ("infv_ltm_consolidate_q",), _SMALL + ", 4 chunks", _LTM_IN, "per_chunk_stages")
    add("ltm_consolidate_pooled", "ltm", ("infv_ltm_consolidate_pooled",), _SMALL + ", 4 chunks", _LTM_KBAR, "fork_join")
    add("ltm_consolidate_4", "ltm", ("infv_ltm_consolidate",), _SMALL + ", 4 chunks: one sub-batch", _LTM_IN, "fork_join")
    add("ltm_consolidate_70", "ltm", ("infv_ltm_consolidate",), _SMALL + ", 70 chunks, max_batch_chunks 32: three sub-batches", _LTM_IN, "ring_reuse")
    add("ltm_consolidate_800", "ltm", ("infv_ltm_consolidate",), _SMALL + ", 800 chunks (16 distinct, tiled): past the 768-chunk gate",
        _LTM_IN, "flag_wait", delay_ms=80.0)
    add("ltm_two_calls_continue", "ltm", ("infv_ltm_consolidate",), _SMALL + ", videos A and B of 36 chunks, B with new_doc=0", _LTM_IN, "call_seam")
    add("ltm_two_calls_new_doc", "ltm", ("infv_ltm_consolidate",), _SMALL + ", videos A and B of 36 chunks, B with new_doc=1", _LTM_IN, "call_seam")
    for dt in ("f16", "bf16", "f8"):
        add(f"ltm_two_calls_{dt}", "ltm", ("infv_ltm_consolidate",), _SMALL + f", videos A and B of 36 chunks, {dt} tokens", _LTM_IN, "call_seam")
    add("ltm_dense_N96", "ltm", ("infv_ltm_consolidate",), "dense_sweep_cases N96: two-box plan, N 96, S 128, d 64, 3 chunks", _LTM_IN, "per_chunk_stages")
    add("ltm_gauss", "ltm", ("infv_ltm_consolidate",), "dense_sweep_cases gauss_base: Gaussian general-psi plan, N 32, 3 chunks", _LTM_IN, "per_chunk_stages")
    add("ltm_consolidate_videos", "ltm", ("infv_ltm_consolidate_videos",), _SMALL + f", videos of {RAGGED} chunks", _LTM_IN, "lockstep")
    add("ltm_steps_videos", "ltm", ("infv_ltm_steps_videos",), _SMALL + f", videos of {RAGGED} chunks", _LTM_KBAR, "lockstep")
    add("ltm_steps_videos_from", "ltm", ("infv_ltm_steps_videos_from",), _SMALL + f", videos of {RAGGED} chunks over 6 shared chunks of frame means",
        _LTM_KBAR, "lockstep")
    add("ltm_then_pack_memory", "ltm", ("infv_ltm_consolidate", "infv_ltm_pack_memory"), _SMALL + ", 70 chunks, set_ctx_sum on", _LTM_IN, "read_out_after_call")
    add("ltm_then_export_import_state", "ltm", ("infv_ltm_consolidate", "infv_ltm_export_state", "infv_ltm_import_state", "infv_ltm_forward"),
        _SMALL + ", 70 chunks, then a forward on the importing handle", _LTM_IN, "read_out_after_call")
    add("ltm_then_chain_state", "ltm", ("infv_ltm_consolidate", "infv_ltm_export_chain_state", "infv_ltm_import_chain_state"),
        _SMALL + ", 35 chunks, hand-over, 35 more on a second handle", _LTM_IN, "read_out_after_call")
    add("ltm_then_reproject_forward", "ltm", ("infv_ltm_consolidate", "infv_ltm_reproject", "infv_ltm_forward"), _SMALL + ", 69 chunks + 1", _LTM_IN,
        "read_out_after_call")
    add("ltm_then_density_masses", "ltm", ("infv_ltm_consolidate", "infv_ltm_density", "infv_ltm_masses"), _SMALL + ", 70 chunks", _LTM_IN, "read_out_after_call")
    add("ltm_then_traces_sources", "ltm", ("infv_ltm_consolidate", "infv_ltm_source_weights"), _SMALL + ", 70 chunks, set_trace and set_mass_trace on",
        _LTM_IN, "read_out_after_call")
    add("ltm_fresh_handle_first_call", "ltm", ("infv_ltm_consolidate",), _SMALL + ", 4 chunks, 5 x (create, first call)", _LTM_IN, "create_memsets", delay_ms=0.0)
    add("ltm_set_bins_between_forwards", "ltm", ("infv_ltm_forward",), _SMALL, _LTM_IN, "null_stream_setters",
        host_wait="infv_ltm_set_bins synchronises the device before its copy")
    add("ltm_set_probs_between_forwards", "ltm", ("infv_ltm_forward",), _SMALL, _LTM_IN, "null_stream_setters",
        host_wait="infv_ltm_set_probs synchronises the device before its copy")
    add("ltm_two_engines_forward", "ltm", ("infv_ltm_forward",), _SMALL + ", 3 chunks each, two engines on two streams", _LTM_IN, "shared_streams")
    add("ltm_two_engines_consolidate", "ltm", ("infv_ltm_consolidate",), _SMALL + ", 70 chunks each, two engines on two streams", _LTM_IN, "shared_streams")
    # ---- drop-in module
    add("dropin_80_forwards", "dropin", ("infv_ltm_forward_into",), _SMALL + ", 80 sticky forwards over 4 chunks", ("k", "q"), "uniform_ring",
        unpoisoned=_MODULE_W, host_wait="call 65 waits for the event of the ring group it is about to overwrite")
    add("dropin_pool_cache_pair", "dropin", ("infv_ltm_forward_into", "infv_ltm_step"), _SMALL + ", two modules on one k, 3 chunks", ("k", "q"), "pool_cache",
        unpoisoned=_MODULE_W)
    # ---- video Q-former
    add("vqf_short_attention", "vqf", ("infv_vqf_short_attention",), _VQF + ", 96 tokens", ("frames", "xq", "key", "value", "a_long"), "caller_stream_only")
    add("vqf_encode_chunk_twice", "vqf", ("infv_vqf_encode_chunk",), _VQF + ", 2 chunks", _VQF_IN, "vqf_side_stream")
    add("vqf_encode_chunk_epoch", "vqf", ("infv_vqf_encode_chunk",), _VQF + ", 3 chunks under a non-zero weights epoch", _VQF_IN, "weights_epoch")
    add("vqf_encode_video_6", "vqf", ("infv_vqf_encode_video",), _VQF + ", 6 chunks", _VQF_IN, "vqf_side_stream")
    add("vqf_encode_videos_3", "vqf", ("infv_vqf_encode_videos",), _VQF + f", videos of {VQF_RAGGED} chunks", _VQF_IN, "vqf_side_stream")
    add("vqf_encode_video_bf16", "vqf", ("infv_vqf_encode_video",), _VQF + ", 6 chunks, bf16 tokens", _VQF_IN, "vqf_side_stream")
    add("vqf_mean", "vqf", ("infv_vqf_mean",), "5 x 4096 floats", ("in",), "caller_stream_only")
    add("vqf_self_attention", "vqf", ("infv_vqf_self_attention",), "2 heads, 4 chunks of up to 65 rows", ("qkv",), "caller_stream_only")
    # ---- VideoChat2
    add("vc_encode_videos", "vc", ("infv_vqf_vc_encode_videos",), _VC + ", videos of (2, 0, 3) chunks", _VC_IN, "vqf_side_stream", delay_ms=60.0)
    add("vc_encode_streams", "vc", ("infv_vqf_vc_encode_streams",), _VC + ", 2 streams over one block of 3 chunks", _VC_IN, "vqf_side_stream", delay_ms=60.0)
    add("vc_encode_videos_tok_f16", "vc", ("infv_vqf_vc_encode_videos_tok",), _VC + ", fp16 tokens", _VC_IN, "vqf_side_stream", delay_ms=60.0)
    add("vc_encode_streams_tok_f16", "vc", ("infv_vqf_vc_encode_streams_tok",), _VC + ", fp16 tokens, 2 streams over one block", _VC_IN, "vqf_side_stream",
        delay_ms=60.0)
    add("vc_encode_img_f16", "vc", ("infv_vqf_vc_encode_img",), _VC + ", fp16 vision output, ids on the host", ("frames", "weights", "u"), "ids_staging",
        delay_ms=60.0, unpoisoned="the instruction ids are a HOST array: the library stages them through its pinned buffer")
    add("vc_embed_twice", "vc", ("infv_vqf_vc_embed",), _VC + ", two calls with different ids", ("weights",), "ids_staging",
        unpoisoned="the ids are a HOST array", host_wait="the second call waits for ev_ids before it rewrites the pinned buffer")
    add("vc_layernorm_two_streams", "vc", ("infv_vqf_layernorm_tokens",), "width 64, 37 rows on one stream and 300 on another, interleaved",
        ("frames", "gamma", "beta"), "ln_stats")
    add("vc_token_pass", "vc", ("infv_vqf_token_pass",), "fp16 tokens [3][64][64], 4 per frame", ("frames",), "caller_stream_only")
    # ---- frame Q-former
    add("frame_encode_fp32", "frame", ("infv_vqf_encode_frames",), _FRAME, ("vision", "weights"), "caller_stream_only")
    add("frame_encode_split_bf16", "frame", ("infv_vqf_encode_frames",), _FRAME + ", split_bf16 linears, two calls under one epoch", ("vision",),
        "weights_epoch", unpoisoned=_PLANES)
    add("frame_encode_fp16", "frame", ("infv_vqf_encode_frames",), _FRAME + ", fp16 linears and fp16 attention, two calls under one epoch",
        ("vision",), "weights_epoch", unpoisoned=_PLANES)
    add("frame_linear", "frame", ("infv_vqf_linear",), "x [70][128] through two stacked [128][128] linears, GELU, residual, LayerNorm",
        ("x", "w", "b", "residual", "ln"), "caller_stream_only")
    add("frame_cross_attention", "frame", ("infv_vqf_frame_cross_attention",), _FRAME, ("vision", "xq", "key", "value", "ln"), "caller_stream_only")
    add("frame_context_tap", "frame", ("infv_vqf_encode_frames",), _FRAME + ", context tap of layer 2 set before the call", ("vision", "weights"),
        "caller_stream_only")
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
FAMILIES = ("ltm", "dropin", "vqf", "vc", "frame")
# one control per family: the synchronised sequence twice, torch.equal
DETERMINISM_CONTROLS = {"ltm": "ltm_consolidate_70", "dropin": "dropin_pool_cache_pair", "vqf": "vqf_encode_video_6", "vc": "vc_encode_videos",
                        "frame": "frame_encode_fp32"}
# the good fill queued on a second stream with no event to the call's: the call legitimately sees the decoy
MISORDER_CONTROLS = ("ltm_consolidate_70", "vqf_encode_video_6", "dropin_pool_cache_pair")


# ---------------------------------------------------------------------------------------------------------------------
# the generators: good values and their decoys (numpy, cached, never modified)
# ---------------------------------------------------------------------------------------------------------------------
def _off(decoy: bool) -> int:
    return DECOY if decoy else 0


@functools.lru_cache(maxsize=None)
def tokens(n_chunks: int, T: int, P: int, d: int, decoy: bool, video: int = 0) -> np.ndarray:
    """[n_chunks, T*P, d] fp32 frame tokens of video ``video``."""
    seed = synth.SEED_K + 1000 * video + _off(decoy)
    out = np.stack([synth.frame_tokens(c, T, P, d, seed=seed) for c in range(n_chunks)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def queries(L: int, Q: int, dm: int, decoy: bool, n_chunks: int = 0) -> np.ndarray:
    """[L, Q, dm], or one per chunk [n_chunks, L, Q, dm]."""
    seed = synth.SEED_Q + _off(decoy)
    if n_chunks:
        out = np.stack([np.stack([synth.layer_query(100 * (c + 1) + l, Q, dm, seed=seed) for l in range(L)]) for c in range(n_chunks)])
    else:
        out = np.stack([synth.layer_query(l, Q, dm, seed=seed) for l in range(L)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def projections(L: int, d: int, dm: int, decoy: bool):
    """Per layer (wk, bk, wv, bv)."""
    return tuple(synth.layer_projections(l, d, dm, seed=synth.SEED_W + _off(decoy)) for l in range(L))


@functools.lru_cache(maxsize=None)
def uniforms(n_chunks: int, L: int, S: int, decoy: bool, video: int = 0) -> np.ndarray:
    """[n_chunks, L, S] float64 in [0, 1)."""
    out = synth.gibbs_uniforms(n_chunks, L, seed=synth.SEED_U + 17 * video + _off(decoy), nb_samples=S)
    out.setflags(write=False)
    return out


def normal(shape, decoy: bool, index: int = 0, scale: float = 1.0) -> np.ndarray:
    """A plain N(0, scale) block from synth's counter-based generator (helper inputs: xq, qkv, residuals, ...)."""
    return synth._normal(synth.SEED_Q + 7 + _off(decoy), index, tuple(shape), scale)


def vqf_weights(decoy: bool) -> dict:
    s = sm.VQF_BASE
    return synth.video_qformer_weights(n_layers=s["n_layers"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                                       n_query=s["n_query"], proj_out=s["proj"], seed=synth.SEED_QF + _off(decoy))


def vc_weights(decoy: bool) -> dict:
    s = sm.BASE
    return synth.videochat2_qformer_weights(s["n_layers"], s["hidden"], s["inter"], s["enc_width"], s["cross_freq"], s["n_query"], s["proj"],
                                            seed=synth.SEED_VC + 31 + _off(decoy))


def frame_weights(decoy: bool) -> dict:
    from tests.golden.frame_qformer_cases import SEED_FQ, frame_qformer_weights
    return frame_qformer_weights(**FRAME_SMALL, seed=SEED_FQ + _off(decoy))


def vision(n_frames: int, decoy: bool) -> np.ndarray:
    from tests.golden.frame_qformer_cases import SEED_FQ, vision_rows
    return vision_rows(n_frames, FRAME_TOKENS, FRAME_SMALL["enc_width"], seed=SEED_FQ + 7 + _off(decoy))


def smallest_decoys():
    """{name: array} of every decoy generator at the smallest shape it is used in -- what the CPU test checks for finiteness."""
    out = {"tokens": tokens(2, 2, 2, 32, True), "queries": queries(1, 1, 64, True), "queries_per_chunk": queries(1, 1, 64, True, 2),
           "uniforms": uniforms(2, 1, 4, True), "normal": normal((4, 4), True), "vision": vision(1, True)}
    for l, p in enumerate(projections(1, 32, 64, True)):
        for n, a in zip(("wk", "bk", "wv", "bv"), p):
            out[f"proj{l}.{n}"] = a
    for fam, w in (("vqf", vqf_weights(True)), ("vc", vc_weights(True)), ("frame", frame_weights(True))):
        for k, v in w.items():
            out[f"{fam}.{k}"] = np.asarray(v)
    return out


SMALL = sc.SMALL
DENSE_N96 = dc.BY_NAME["N96"]
GAUSS = dc.GAUSS
