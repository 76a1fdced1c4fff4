"""``infv_vqf_encode_frames`` on the device: the per-frame image Q-former (``encode_short_memory_frame`` after the vision encoder).

Small model unless stated: 4 layers (cross layers 0 and 2), 2 heads, hidden 128, inter 256, ``enc_width`` 128, 8 query tokens, weights
from the synthetic generators.  ATOL is the project's own 2e-4 (tests/test_vc_gpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infinite_video_amd import _lib, synth
from infinite_video_amd.basis_maps import NB_SAMPLES
from infinite_video_amd.frame_qformer import FrameQformerEncoder
from infinite_video_amd.video_qformer import InfVideoEncoder, ShortMemoryBuffer
from oracle.videochat2_oracle import VideoChat2Oracle
from tests.conftest import record_parity
from tests.golden.frame_qformer_cases import (FULL, GOLDEN_FRAMES, GOLDEN_PATH, GOLDEN_TAPS, GOLDEN_TOKENS, LN_VISION_EPS, SMALL,
                                              frame_qformer_weights, oracle_weights, vision_rows)
from tests.golden.softmax_tier_cases import ref64           # the float64 restatement of the image Q-former

pytestmark = pytest.mark.gpu
ATOL = 2e-4
INVALID, UNSUPPORTED = -1, -2


def dev():
    return torch.device("cuda:0")


def _model(shape: dict, ln: bool, sd=None) -> FrameQformerEncoder:
    sd = frame_qformer_weights(**shape) if sd is None else sd
    m = FrameQformerEncoder(num_query_token=shape["n_query"], vision_width=shape["enc_width"], num_hidden_layers=shape["n_layers"],
                            hidden_size=shape["hidden"], intermediate_size=shape["inter"], num_attention_heads=shape["n_heads"],
                            vision_layernorm=ln)
    m.load_reference_state_dict({k: v for k, v in sd.items() if ln or not k.startswith("ln_vision.")})
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def small_sd():
    return frame_qformer_weights(**SMALL)


@functools.lru_cache(maxsize=None)
def small_model(ln: bool) -> FrameQformerEncoder:
    return _model(SMALL, ln, small_sd())


@functools.lru_cache(maxsize=None)
def small_vision(n_frames: int, n_tokens: int) -> torch.Tensor:
    return torch.from_numpy(vision_rows(n_frames, n_tokens, SMALL["enc_width"], seed=100 + n_tokens)).to(dev())


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def raw_encode(m: FrameQformerEncoder, x: torch.Tensor, out: torch.Tensor, *, ln=None, n_frames=None, n_tokens=None, code=None,
               out_code=None, handle=None, w=None, rows=None, vision_ptr=None, out_ptr=None):
    """One ``infv_vqf_encode_frames`` call with every argument open to the refusal tests; returns the status."""
    (w0, vis), keep = m._weights(dev())
    ln = hasattr(m, "ln_vision") if ln is None else ln
    rows = m.query_rows(dev()) if rows is None else rows
    codes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3, torch.float8_e4m3fn: 4}
    rc = _lib.load().infv_vqf_encode_frames(
        m._handle(dev()) if handle is None else handle, x.size(0) if n_frames is None else n_frames,
        C.c_void_p(x.data_ptr() if vision_ptr is None else vision_ptr), codes[x.dtype] if code is None else code,
        x.size(1) if n_tokens is None else n_tokens, C.byref(w0 if w is None else w), C.byref(vis) if ln else None,
        C.c_void_p(rows if isinstance(rows, int) else rows.data_ptr()), C.c_void_p(out.data_ptr() if out_ptr is None else out_ptr),
        codes[out.dtype] if out_code is None else out_code, stream())
    del keep
    return rc


def launches() -> int:
    return int(_lib.load().infv_ltm_launch_count())


# ---------------------------------------------------------------------------------------------------- 1. bit anchor
@pytest.mark.parametrize("n_tokens", [64, 128])
def test_whole_tiles_are_vc_encode_videos_bit_for_bit(n_tokens):
    """n_tokens % 64 == 0: the call IS infv_vqf_vc_encode_videos on F one-chunk videos (alpha 1, T 1, no text) -- bits and launches."""
    lib = _lib.load()
    m = small_model(False)
    n_f, Q, Hd = 5, SMALL["n_query"], SMALL["hidden"]
    x = small_vision(n_f, n_tokens)
    rows = m.query_rows(dev())
    (w, _), keep = m._weights(dev())
    cfg = _lib.VqfConfig(1, SMALL["n_heads"], Hd, SMALL["inter"], SMALL["enc_width"], n_tokens, Q, 0, NB_SAMPLES, 1.0, 1e-12)
    h = C.c_void_p()
    _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
    try:
        cu = (C.c_int32 * (n_f + 1))(*range(n_f + 1))
        tl = (C.c_int32 * n_f)(*([0] * n_f))
        hin = rows.repeat(n_f, 1).contiguous()
        ref = torch.full((n_f, Q, Hd), float("nan"), device=dev())
        got = torch.full((n_f, Q, Hd), float("nan"), device=dev())
        for _ in range(2):                                    # (the second round runs on grown workspaces: the counted one)
            l0 = launches()
            _lib.check(lib.infv_vqf_vc_encode_videos(h, None, n_f, C.cast(cu, C.c_void_p), C.c_void_p(x.data_ptr()), 1, C.byref(w),
                                                     C.c_void_p(hin.data_ptr()), C.cast(tl, C.c_void_p), None, 1,
                                                     C.c_void_p(ref.data_ptr()), None, None, stream()))
            l1 = launches()
            _lib.check(raw_encode(m, x, got))
            l2 = launches()
        torch.cuda.synchronize()
        assert torch.equal(got, ref) and not torch.isnan(ref).any()
        assert l1 - l0 == l2 - l1 > 0
    finally:
        lib.infv_vqf_destroy(h)
    del keep


# ---------------------------------------------------------------------------------------------------- 2. partial tiles
@functools.lru_cache(maxsize=None)
def small_oracle():
    return VideoChat2Oracle(oracle_weights(small_sd()), 64, 0.75, 1.0, True, n_layers=SMALL["n_layers"], cross_freq=2,
                            n_heads=SMALL["n_heads"], n_query=SMALL["n_query"], tokens_per_frame=257)


@pytest.mark.parametrize("n_tokens", [1, 5, 63, 65, 127, 257])
def test_partial_tiles_against_float64_and_the_oracle(n_tokens):
    """Token counts the short-term attention refused before (no multiple of 32): every output element within ATOL of a float64
    restatement, and of ``VideoChat2Oracle(alpha=1.0)``."""
    m = small_model(True)
    x = small_vision(3, n_tokens)
    got = m.encode_frames(x).cpu()
    ref = ref64(small_sd(), SMALL, x, True)
    worst = float((got.double() - ref).abs().max())
    sd = small_sd()
    k32 = F.layer_norm(x.cpu(), (x.size(-1),), torch.from_numpy(sd["ln_vision.weight"]), torch.from_numpy(sd["ln_vision.bias"]),
                       LN_VISION_EPS).numpy()
    h0 = m.query_rows(dev()).cpu().numpy()
    orc = small_oracle()
    worst_o = max(float(np.abs(orc.encode_chunk(k32[f], h0, True)[0] - got[f].numpy()).max()) for f in range(3))
    record_parity(f"frame_qformer small model 3 x {n_tokens} tokens: max |device - float64| {worst:.3e}, max |device - oracle| {worst_o:.3e}")
    assert worst <= ATOL
    assert worst_o <= ATOL


# ---------------------------------------------------------------------------------------------------- 3. golden
def test_full_model_against_the_reference_golden():
    """12 layers, 768, 1408, 32 queries, 3 x 257 tokens: the real reference encoder's hidden states and the cross-attention context
    of the first and the last cross layer."""
    g = np.load(GOLDEN_PATH)
    m = _model(FULL, True)
    x = torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"])).to(dev())
    lib = _lib.load()
    worst = {}
    out = None
    for l in GOLDEN_TAPS:
        tap = torch.full((GOLDEN_FRAMES, FULL["n_query"], FULL["hidden"]), float("nan"), device=dev())
        _lib.check(lib.infv_vqf_set_context_tap(m._handle(dev()), l, C.c_void_p(tap.data_ptr())))
        out = m.encode_frames(x)
        worst[f"l{l}_xctx"] = float(np.abs(tap.cpu().numpy() - g[f"l{l}_xctx"]).max())
    worst["hidden"] = float(np.abs(out.cpu().numpy() - g["hidden"]).max())
    worst["h0"] = float(np.abs(m.query_rows(dev()).cpu().numpy() - g["h0"]).max())
    record_parity("frame_qformer full model 3 x 257 tokens vs the reference golden: " +
                  ", ".join(f"max |{k}| {v:.3e}" for k, v in sorted(worst.items())))
    assert all(v <= ATOL for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------- 4. source types
@pytest.mark.parametrize("n_tokens", [65, 257])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("ln", [True, False])
def test_half_vision_is_the_run_on_its_float_values(n_tokens, dtype, ln):
    m = small_model(ln)
    x = small_vision(3, n_tokens).to(dtype)
    assert torch.equal(m.encode_frames(x), m.encode_frames(x.float()))


@pytest.mark.parametrize("n_tokens", [65, 257])
def test_fp8_vision_without_layernorm_is_the_run_on_its_float_values(n_tokens):
    m = small_model(False)
    x = small_vision(3, n_tokens).to(torch.float8_e4m3fn)
    got = m.encode_frames(x)
    assert torch.equal(got, m.encode_frames(x.float())) and not torch.isnan(got).any()


def test_fp8_vision_with_layernorm_is_unsupported_and_launches_nothing():
    m = small_model(True)
    x = small_vision(3, 65).to(torch.float8_e4m3fn)
    out = torch.full((3, SMALL["n_query"], SMALL["hidden"]), 7.0, device=dev())
    l0 = launches()
    assert raw_encode(m, x, out) == UNSUPPORTED
    assert launches() == l0 and b"fp8" in _lib.load().infv_ltm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        m.encode_frames(x)


# ---------------------------------------------------------------------------------------------------- 5. LayerNorm on load
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_layernorm_on_load_is_the_call_on_the_normalised_tensor(dtype):
    m_ln, m_plain = small_model(True), small_model(False)
    x = small_vision(3, 65).to(dtype)
    ln = m_ln.ln_vision
    y = torch.empty(x.shape, device=dev(), dtype=torch.float32)
    _lib.check(_lib.load().infv_vqf_layernorm_tokens(C.c_void_p(x.data_ptr()), {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}[dtype],
                                                     x.size(0) * x.size(1), x.size(2), C.c_void_p(ln.weight.data_ptr()),
                                                     C.c_void_p(ln.bias.data_ptr()), float(ln.eps), C.c_void_p(y.data_ptr()), stream()))
    assert torch.equal(m_ln.encode_frames(x), m_plain.encode_frames(y))


# ---------------------------------------------------------------------------------------------------- 6. output types
@pytest.mark.parametrize("n_tokens", [64, 65])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_output_is_the_rounded_fp32_result(n_tokens, dtype):
    m = small_model(True)
    x = small_vision(3, n_tokens)
    assert torch.equal(m.encode_frames(x, out_dtype=dtype), m.encode_frames(x).to(dtype))


def test_fp16_buffer_written_in_place_feeds_encode_video():
    """The frame tokens written straight into an fp16 ``ShortMemoryBuffer`` are what ``buffer.replace(fp32 result)`` stores, and
    ``encode_video`` reads both to the same bits."""
    shape = dict(n_layers=2, hidden=768, inter=256, enc_width=128, n_query=32, n_heads=12)
    fq = _model(shape, True)
    x = torch.from_numpy(vision_rows(8, 65, 128, seed=5)).to(dev()).half()
    wq = synth.video_qformer_weights(proj_out=512)
    enc = InfVideoEncoder(llama_hidden=512, num_basis=64, tau=0.75, alpha=0.9, sticky=True)
    enc.load_reference_state_dict(wq)
    enc = enc.to(dev())
    direct = ShortMemoryBuffer(32, 768, capacity_frames=16, dtype=torch.float16, device=dev())
    fq.encode_short_memory_frame(x, direct, n_frame=6)
    assert len(direct) == 7
    via = ShortMemoryBuffer(32, 768, capacity_frames=16, dtype=torch.float16, device=dev()).replace(fq.encode_frames(x), 6)
    assert torch.equal(direct.store[:7], via.store[:7])
    outs = []
    for buf in (direct, via):
        enc.short_memory_buffer = buf
        torch.manual_seed(0)
        outs.append(enc.encode_video(new_video=True)[0].clone())
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()
    f8 = ShortMemoryBuffer(32, 768, capacity_frames=16, dtype=torch.float8_e4m3fn, device=dev())
    fq.encode_short_memory_frame(x, f8, n_frame=2)           # (an fp8 buffer: replace() on the fp32 result)
    assert len(f8) == 3 and torch.equal(f8.store[:3].float(), fq.encode_frames(x[:3]).to(torch.float8_e4m3fn).float())


# ---------------------------------------------------------------------------------------------------- 7. batch invariance
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ln", [True, False])
def test_a_frame_does_not_depend_on_the_batch_or_its_neighbours(ln, dtype):
    m = small_model(ln)
    x = small_vision(3, 65).to(dtype)
    base = m.encode_frames(x)
    assert torch.equal(m.encode_frames(x[1:2])[0], base[1])
    many = small_vision(17, 65).to(dtype).clone()
    many[16] = x[1]
    assert torch.equal(m.encode_frames(many)[16], base[1])
    poisoned = x.clone()
    poisoned[2] = float("nan")
    got = m.encode_frames(poisoned)
    assert torch.equal(got[:2], base[:2])                     # frame 1's last tile ends where frame 2's rows begin
    assert torch.isnan(got[2]).any() and not torch.isnan(got[:2]).any()


# ---------------------------------------------------------------------------------------------------- 8. plane cache off
def test_plane_cache_off_gives_the_same_bits(monkeypatch):
    """INFV_VQF_SPLIT_CACHE_GB is read when a handle is created: a fresh model creates its handle under 0 and splits the tokens
    per sub-batch instead of once per call."""
    x = small_vision(3, 65)
    cached = small_model(True).encode_frames(x)
    monkeypatch.setenv("INFV_VQF_SPLIT_CACHE_GB", "0")
    fresh = _model(SMALL, True, small_sd())
    l0 = launches()
    uncached = fresh.encode_frames(x)
    n_uncached = launches() - l0
    monkeypatch.delenv("INFV_VQF_SPLIT_CACHE_GB")
    l0 = launches()
    small_model(True).encode_frames(x)
    assert n_uncached == launches() - l0 + 1                 # one token pass per cross layer (two) instead of one per call
    assert torch.equal(uncached, cached)


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_output_untouched():
    lib = _lib.load()
    m = small_model(True)
    x = small_vision(3, 65)
    Q, Hd = SMALL["n_query"], SMALL["hidden"]
    out = torch.full((3, Q, Hd), 7.0, device=dev())
    (w, _), keep = m._weights(dev())
    odd = torch.zeros(3 * 65 * SMALL["enc_width"] + 4, device=dev())[1:]             # 4 bytes past a 16-byte boundary
    odd_out = torch.zeros(3 * Q * Hd + 4, device=dev())[1:]
    lay = lambda n: _lib.VqfVcWeights(n, 0, w.layers, _lib.Linear(None, None))
    proj = torch.zeros(8, Hd, device=dev())
    with_proj = _lib.VqfVcWeights(w.n_layers, 0, w.layers, _lib.Linear(proj.data_ptr(), None))
    cases = [
        ("null handle", dict(handle=C.c_void_p(0)), INVALID),
        ("null vision", dict(vision_ptr=0), INVALID),
        ("null out", dict(out_ptr=0), INVALID),
        ("null query_rows", dict(rows=0), INVALID),
        ("F < 0", dict(n_frames=-1), INVALID),
        ("unknown token dtype", dict(code=2), INVALID),
        ("unknown token dtype", dict(code=9), INVALID),
        ("unknown output dtype", dict(out_code=2), INVALID),
        ("fp8 output", dict(out_code=4), UNSUPPORTED),
        ("misaligned vision", dict(vision_ptr=odd.data_ptr()), INVALID),
        ("misaligned out", dict(out_ptr=odd_out.data_ptr()), INVALID),
        ("n_tokens < 1", dict(n_tokens=0), INVALID),
        ("no layers", dict(w=lay(0)), INVALID),
        ("too many layers", dict(w=lay(_lib.VC_MAX_LAYERS + 1)), UNSUPPORTED),
        ("a projection present", dict(w=with_proj), INVALID),
    ]
    for what, kw, status in cases:
        l0 = launches()
        rc = raw_encode(m, x, out, **kw)
        msg = lib.infv_ltm_last_error().decode()
        assert rc == status, (what, rc, msg)
        assert msg, what
        assert launches() == l0, what
    # the fp32 contractions take whole 32-token blocks only
    _lib.check(lib.infv_vqf_set_precision(m._handle(dev()), 1))
    try:
        l0 = launches()
        assert raw_encode(m, x, out) == UNSUPPORTED and launches() == l0
    finally:
        _lib.check(lib.infv_vqf_set_precision(m._handle(dev()), 0))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert raw_encode(m, x, out, n_frames=0) == 0                                     # F == 0 is not an error, and writes nothing
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    del keep


def test_fp32_contractions_run_on_whole_32_token_blocks():
    """infv_vqf_set_precision(h, 1) with n_tokens % 32 == 0 (96: no multiple of 64) runs the fp32 kernels; the split-bf16 default
    pads 96 to 128.  Both within ATOL of float64."""
    m = small_model(True)
    x = small_vision(3, 96)
    ref = ref64(small_sd(), SMALL, x, True)
    split = m.encode_frames(x).cpu()
    _lib.check(_lib.load().infv_vqf_set_precision(m._handle(dev()), 1))
    try:
        exact = m.encode_frames(x).cpu()
    finally:
        _lib.check(_lib.load().infv_vqf_set_precision(m._handle(dev()), 0))
    assert float((split.double() - ref).abs().max()) <= ATOL
    assert float((exact.double() - ref).abs().max()) <= ATOL


def test_many_frames_cross_every_host_table_seam():
    """More frames than one launch's row table (128), one self-attention group (256) and one row block hold: a frame deep in the
    call is the frame alone."""
    m = small_model(True)
    x = small_vision(3, 5)
    many = x[:1].repeat(300, 1, 1).contiguous()
    many[299] = x[1]
    many[128] = x[2]
    got = m.encode_frames(many, out_dtype=torch.float16)
    base = m.encode_frames(x, out_dtype=torch.float16)
    assert torch.equal(got[299], base[1]) and torch.equal(got[128], base[2]) and torch.equal(got[0], base[0])
    assert torch.equal(got[1:128], got[0:1].expand(127, -1, -1))
