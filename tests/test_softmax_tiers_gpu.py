"""The row softmax of the short-term attention at every row-length tier and reduction seam, on the device.

``launch_softmax_rows_split_pad`` picks by padded row length (``<2>`` up to 2048, ``<8>`` up to 8192, the long kernel beyond),
``launch_softmax_rows_split`` likewise for whole rows (``reg<2>``, ``reg<8>``, the three-pass kernel), and
``qf_softmax_rows_kernel`` serves the fp32 contractions.  The synthetic inputs give scores within +-0.4, where a wrong maximum or a
leaked pad key cannot be seen; the constructions of ``tests/golden/softmax_tier_cases.py`` (checked in float64 by
``tests/test_softmax_tiers_cpu.py``) make both visible:

A. every tier against the float64 restatement, output and both cross-attention contexts;
B. a frame the kernels pad themselves equals, bit for bit, the same frame padded with dead keys (score -300: ``expf`` gives 0);
C. a hot key (score +100: a maximum that misses it overflows ``expf``) at every reduction seam, through ``infv_vqf_encode_frames``
   and through ``infv_vqf_short_attention`` in both precisions;
D. peaked scores (the cross-attention query scaled in the state dict);
E. one handle carried across the tiers equals a fresh handle at every step.

Small model throughout: 4 layers (cross layers 0 and 2), 2 heads, hidden 128, ``enc_width`` 128, 8 queries: 16 score rows per
frame and layer.  ATOL is the project's own 2e-4."""
import ctypes as C
import functools

import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.frame_qformer import FrameQformerEncoder
from tests.conftest import record_parity
from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import SMALL

pytestmark = pytest.mark.gpu
ATOL = tc.ATOL
CROSS = tc.CROSS_LAYERS


def dev():
    return torch.device("cuda:0")


def new_model(ln: bool, gain: int = 0) -> FrameQformerEncoder:
    """A model of its own (its own handle and workspaces) from ``small_sd()``, or ``peaked_sd(gain)``."""
    sd = tc.peaked_sd(gain) if gain else tc.small_sd()
    m = FrameQformerEncoder(num_query_token=SMALL["n_query"], vision_width=SMALL["enc_width"], num_hidden_layers=SMALL["n_layers"],
                            hidden_size=SMALL["hidden"], intermediate_size=SMALL["inter"], num_attention_heads=SMALL["n_heads"],
                            vision_layernorm=ln)
    m.load_reference_state_dict({k: v for k, v in sd.items() if ln or not k.startswith("ln_vision.")})
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def model(ln: bool, gain: int = 0) -> FrameQformerEncoder:
    return new_model(ln, gain)


def encode(m: FrameQformerEncoder, x: torch.Tensor):
    """``encode_frames`` once per cross layer with that layer's context tapped (a tap serves one call): the output and
    {layer: context [F, Q, hidden]}, on the CPU.  The calls must agree on the output to the bit."""
    x = x.to(dev())
    taps, out = {}, None
    for l in CROSS:
        tap = torch.full((x.size(0), SMALL["n_query"], SMALL["hidden"]), float("nan"), device=dev())
        _lib.check(_lib.load().infv_vqf_set_context_tap(m._handle(dev()), l, C.c_void_p(tap.data_ptr())))
        got = m.encode_frames(x)
        assert out is None or torch.equal(got, out)
        out, taps[l] = got, tap.cpu()
    return out.cpu(), taps


def reference(sd, x: torch.Tensor, ln: bool):
    c = {}
    out = tc.ref64(sd, SMALL, x, ln, collect=c)
    return out, c["ctx"]


def worst_errors(out, taps, ref, ref_ctx) -> dict:
    w = {"out": float((out.double() - ref).abs().max())}
    for l in CROSS:
        w[f"ctx{l}"] = float((taps[l].double() - ref_ctx[l]).abs().max())
    return w


def fmt(w: dict) -> str:
    return ", ".join(f"{k} {v:.3e}" for k, v in w.items())


# ---------------------------------------------------------------------------------------------------- A. every tier
@pytest.mark.parametrize("n_tokens", tc.TIER_PADDED + tc.TIER_WHOLE)
def test_every_tier_against_float64(n_tokens):
    """F = 3, ``ln_vision`` on, fp32 tokens.  Padded 1023 / 1025 (both register groups of ``<2>``), 2047 / 2049 (``<2>`` full,
    ``<8>`` partial), 8191 / 8193 (``<8>`` full, the long kernel); whole 1024 (``reg<2>``), 2112 (``reg<8>``), 8256 (three passes)."""
    x = tc.tier_vision(3, n_tokens)
    out, taps = encode(model(True), x)
    w = worst_errors(out, taps, *reference(tc.small_sd(), x, True))
    record_parity(f"softmax tiers A: 3 x {n_tokens} tokens ({'padded' if n_tokens % 64 else 'whole'}): max |device - float64| {fmt(w)}")
    assert all(v <= ATOL for v in w.values()), w


# ---------------------------------------------------------------------------------------------------- B. pad keys are dead keys
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,n_pad", tc.PAD_PAIRS)
def test_pad_keys_are_exactly_dead_keys(n, n_pad, bf16):
    """The padded call on n live tokens against the whole-tile call on the same tokens followed by n_pad - n dead keys: same K,
    same kernel shapes, same per-thread order, so "zero row with 0.f mass" against "finite row whose expf is 0" must agree to
    the bit, in the output and in both contexts.  bf16 tokens take the ``own_hi`` branches (no lo planes)."""
    full = tc.dead_padded(n, n_pad, bf16)
    dtype = torch.bfloat16 if bf16 else torch.float32
    m = model(False)
    out_p, taps_p = encode(m, full[:, :n].contiguous().to(dtype))
    out_u, taps_u = encode(m, full.to(dtype))
    ref, ref_ctx = reference(tc.small_sd(), full, False)
    wp, wu = worst_errors(out_p, taps_p, ref, ref_ctx), worst_errors(out_u, taps_u, ref, ref_ctx)
    same = {"out": torch.equal(out_p, out_u), **{f"ctx{l}": torch.equal(taps_p[l], taps_u[l]) for l in CROSS}}
    record_parity(f"softmax tiers B: 2 x {n} tokens padded to {n_pad} ({'bf16' if bf16 else 'fp32'}): padded {fmt(wp)}; dead keys {fmt(wu)}; "
                  f"identical {same}")
    assert all(v <= ATOL for v in wp.values()), wp
    assert all(v <= ATOL for v in wu.values()), wu
    assert all(same.values()), same


# ---------------------------------------------------------------------------------------------------- C. the hot key
@pytest.mark.parametrize("n_tokens", tc.HOT_SIZES)
def test_hot_key_at_every_reduction_seam(n_tokens):
    """One frame per position: the first and the last lane, the wave boundary, the register-group boundaries, the last live
    column.  A maximum that misses the hot key overflows ``expf``."""
    x = tc.hot_frames(n_tokens)
    pos = tc.hot_positions(n_tokens)
    out, taps = encode(model(False), x)
    ref = tc.ref64(tc.small_sd(), SMALL, x, False)
    bad = [p for f, p in enumerate(pos) if not (torch.isfinite(out[f]).all() and torch.isfinite(taps[0][f]).all())]
    err = (out.double() - ref).abs().flatten(1).max(1).values
    record_parity(f"softmax tiers C: hot key in {n_tokens} tokens at {list(pos)}: max |device - float64| {float(err.max()):.3e}"
                  f"{', non-finite at ' + str(bad) if bad else ''}")
    assert not bad, f"non-finite output or layer-0 context with the hot key at {bad}"
    assert float(err.max()) <= ATOL, {p: float(e) for p, e in zip(pos, err)}


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "fp32"])
@pytest.mark.parametrize("n_tokens", tc.HOT_SHORT_SIZES)
def test_hot_key_through_short_attention(n_tokens, exact):
    """``infv_vqf_short_attention``, one cross layer: precision 0 runs the split softmax on whole rows, precision 1 runs
    ``qf_softmax_rows_kernel``."""
    lib = _lib.load()
    S = tc.SHORT
    si = tc.short_inputs(n_tokens)
    d = lambda t: t.to(dev()).contiguous()
    fr, q, wk, bk, wv, bv, hot = (d(si[k]) for k in ("frames", "xq", "wk", "bk", "wv", "bv", "hot"))
    fr = fr.clone()
    cfg = _lib.VqfConfig(n_layers=1, n_heads=S["n_heads"], hidden=S["hidden"], inter=S["hidden"], enc_width=S["enc_width"],
                         tokens_per_frame=32, n_query=S["n_query"], proj_out=64, nb_samples=512, alpha=1.0, ln_eps=1e-12)
    h = C.c_void_p()
    _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
    worst, bad = 0.0, []
    try:
        _lib.check(lib.infv_vqf_set_precision(h, exact))
        key, val = _lib.Linear(wk.data_ptr(), bk.data_ptr()), _lib.Linear(wv.data_ptr(), bv.data_ptr())
        for p in tc.hot_positions(n_tokens):
            keep = fr[p].clone()
            fr[p] = hot
            out = torch.full((S["n_query"], S["hidden"]), float("nan"), device=dev())
            _lib.check(lib.infv_vqf_short_attention(h, C.c_void_p(fr.data_ptr()), n_tokens, C.c_void_p(q.data_ptr()), C.byref(key), C.byref(val),
                                                    C.c_void_p(0), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            got = out.cpu()
            fr[p] = keep
            if not torch.isfinite(got).all():
                bad.append(p)
                continue
            worst = max(worst, float((got.double() - tc.short_reference(n_tokens, p)).abs().max()))
    finally:
        _lib.check(lib.infv_vqf_destroy(h))
    record_parity(f"softmax tiers C: short_attention hot key in {n_tokens} tokens ({'exact fp32' if exact else 'split-bf16'}): "
                  f"max |device - float64| {worst:.3e}{', non-finite at ' + str(bad) if bad else ''}")
    assert not bad, f"non-finite output with the hot key at {bad}"
    assert worst <= ATOL


# ---------------------------------------------------------------------------------------------------- D. peaked scores
@pytest.mark.parametrize("n_tokens", tc.PEAK_SIZES)
@pytest.mark.parametrize("gain", tc.PEAK_GAINS)
def test_peaked_scores_against_float64(gain, n_tokens):
    x = tc.tier_vision(3, n_tokens)
    out, taps = encode(model(True, gain), x)
    w = worst_errors(out, taps, *reference(tc.peaked_sd(gain), x, True))
    record_parity(f"softmax tiers D: query gain {gain}, 3 x {n_tokens} tokens: max |device - float64| {fmt(w)}")
    assert all(v <= ATOL for v in w.values()), w


# ---------------------------------------------------------------------------------------------------- E. one handle across tiers
def test_one_handle_across_the_tiers_is_a_fresh_handle_each_time():
    """Long row, short row and back on one handle: stale pad columns of S, a changed ldS or stale P planes would show against a
    model that has seen nothing else."""
    carried = new_model(True)
    for step, n in enumerate(tc.HANDLE_WALK):
        x = tc.tier_vision(3, n).to(dev())
        got = carried.encode_frames(x)
        fresh = new_model(True).encode_frames(x)
        assert not torch.isnan(got).any()
        assert torch.equal(got, fresh), f"step {step}: {n} tokens after {tc.HANDLE_WALK[:step]}"
