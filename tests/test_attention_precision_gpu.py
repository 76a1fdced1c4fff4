"""The cross-attention of the frame Q-former with fp16 operands (``infv_vqf_set_attention_precision``), on the device.

1. the attention alone (``infv_vqf_frame_cross_attention``) against the float64 context of the same layer, within twice the error of
   the float64 emulation of the mode's roundings (``tests/test_attention_precision_cpu.py`` shows that error to be at least 5 x what
   fp32 costs on these inputs, so the bound allows the mode's rounding and nothing else);
2. the softmax edges through the mode; 3. the small and 4. the full model; 5. source dtypes and 6. batch invariance, bit for bit;
7. the handle: plane cache, refusals, launch counts; 8. what the f16 MFMA does with a subnormal operand, measured.

Every test but the last calls one of the two new symbols: none of them passes on a library without them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.basis_maps import NB_SAMPLES
from infinite_video_amd.frame_qformer import ATTENTION_PRECISIONS, LINEAR_PRECISIONS, FrameQformerEncoder
from tests.conftest import record_parity
from tests.golden import attention_precision_cases as ac
from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import FULL, GOLDEN_FRAMES, GOLDEN_PATH, GOLDEN_TAPS, LN_VISION_EPS, SMALL

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -2
PAIRS = tuple((lin, attn) for lin in LINEAR_PRECISIONS for attn in ATTENTION_PRECISIONS)


def dev():
    return torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def launches() -> int:
    return int(_lib.load().infv_ltm_launch_count())


def counted(fn):
    l0 = launches()
    out = fn()
    return out, launches() - l0


def worst(a, b) -> float:
    return float((a.double().cpu() - b.double().cpu()).abs().max())


class RawHandle:
    """A handle of its own at the C ABI (weights epoch 0 unless set: the planes are rebuilt in every call)."""

    def __init__(self, shape: dict, attn: int = 0, lin: int = 0, tokens_per_frame: int = 1):
        self.h = C.c_void_p()
        cfg = _lib.VqfConfig(1, shape["n_heads"], shape["hidden"], shape.get("inter", 256), shape["enc_width"], tokens_per_frame,
                             shape["n_query"], 0, NB_SAMPLES, 1.0, 1e-12)
        _lib.check(_lib.load().infv_vqf_create(C.byref(cfg), C.byref(self.h)))
        if lin:
            _lib.check(_lib.load().infv_vqf_set_linear_precision(self.h, lin))
        if attn:
            _lib.check(_lib.load().infv_vqf_set_attention_precision(self.h, attn))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.load().infv_vqf_destroy(self.h)


def new_model(shape: dict, sd: dict, lin: str = "fp32", attn: str = "fp32", vision_layernorm: bool = True) -> FrameQformerEncoder:
    m = FrameQformerEncoder(num_query_token=shape["n_query"], vision_width=shape["enc_width"], num_hidden_layers=shape["n_layers"],
                            hidden_size=shape["hidden"], intermediate_size=shape["inter"], num_attention_heads=shape["n_heads"],
                            linear_precision=lin, attention_precision=attn, vision_layernorm=vision_layernorm)
    m.load_reference_state_dict({k: v for k, v in sd.items() if vision_layernorm or not k.startswith("ln_vision.")})
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def small_model(lin: str, attn: str, ln: bool = True) -> FrameQformerEncoder:
    return new_model(SMALL, tc.small_sd(), lin, attn, ln)


TOKEN_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3, torch.float8_e4m3fn: 4}


def cross_attention(h, vision: torch.Tensor, ln, xq: torch.Tensor, wk, wv, bv, bk=None) -> torch.Tensor:
    """``infv_vqf_frame_cross_attention`` on handle h: vision [F, n, d] on the device in its own dtype, ln = (gamma, beta) or None."""
    key = _lib.Linear(wk.data_ptr(), bk.data_ptr() if bk is not None else None)
    value = _lib.Linear(wv.data_ptr(), bv.data_ptr())
    vis = _lib.VqfVisionLn(ln[0].data_ptr(), ln[1].data_ptr(), LN_VISION_EPS) if ln else None
    ctx = torch.full(tuple(xq.shape), float("nan"), device=dev())
    _lib.check(_lib.load().infv_vqf_frame_cross_attention(h, vision.size(0), C.c_void_p(vision.data_ptr()), TOKEN_CODES[vision.dtype],
                                                          vision.size(1), C.byref(vis) if ln else None, C.c_void_p(xq.data_ptr()),
                                                          C.byref(key), C.byref(value), C.c_void_p(ctx.data_ptr()), stream()))
    return ctx


# ---------------------------------------------------------------------------------------------------- 1. the attention alone
@pytest.mark.parametrize("ln", (True, False), ids=("ln", "plain"))
@pytest.mark.parametrize("shape_name", sorted(ac.UNIT_SHAPES))
def test_attention_alone_within_twice_the_emulation_error(shape_name, ln):
    """max |ctx - ref64| <= 2 x E_ref, E_ref = max |attend16 - ref64| over the same frames, for n in 1 .. 512 and F in 1, 3.  The
    device rounds its intermediates from fp32 values, the emulation from float64 values: a flipped rounding costs what the rounding
    costs.  The mode-0 result of the same entry is another tensor."""
    shape = ac.UNIT_SHAPES[shape_name]
    with RawHandle(shape, 1) as fast, RawHandle(shape, 0) as plain:
        for n in ac.UNIT_TOKENS:
            u = {k: v.to(dev()) for k, v in ac.unit_inputs(shape_name, n).items()}
            ref, emu = ac.unit_ref(shape_name, n, ln), ac.unit_emu(shape_name, n, ln)[0]
            for n_f in (1, 3):
                args = (u["vision"][:n_f].contiguous(), (u["gamma"], u["beta"]) if ln else None, u["xq"][:n_f].contiguous(), u["wk"], u["wv"],
                        u["bv"], u["bk"])
                got = cross_attention(fast.h, *args)
                assert not torch.isnan(got).any()
                e_ref, err = worst(emu[:n_f], ref[:n_f]), worst(got, ref[:n_f])
                record_parity(f"attention precision 1: {shape_name} n {n} F {n_f} ln {int(ln)}: max |ctx - ref64| {err:.3e}, E_ref {e_ref:.3e}, "
                              f"|ctx - emu64| {worst(got, emu[:n_f]):.3e}")
                assert err <= 2.0 * e_ref, (n, n_f, err, e_ref)
                base = cross_attention(plain.h, *args)                     # mode 0 on the same arguments: fp32-class, another tensor
                assert worst(base, ref[:n_f]) <= tc.ATOL and not torch.equal(base, got), (n, n_f)


def test_mode_0_of_the_new_entry_is_the_default_path_bit_for_bit():
    """The small model with layer 0's cross-query weight zeroed: that layer's query rows are its query bias, whatever the hidden
    states are, so the stand-alone entry can be given the very xq the encoder computes.  Its mode-0 context equals the context tap
    of the default path on that layer, bit for bit and launch for launch of the attention, at 64 and at 257 tokens."""
    sd = dict(tc.small_sd())
    p = "Qformer.bert.encoder.layer.0.crossattention.self."
    sd[p + "query.weight"] = np.zeros_like(sd[p + "query.weight"])
    sd[p + "query.bias"] = np.asarray(np.random.default_rng(77).standard_normal(SMALL["hidden"]), np.float32)
    m = new_model(SMALL, sd)
    lib = _lib.load()
    layer = m.Qformer.bert.encoder.layer[0].crossattention.self
    for n in (64, 257):
        x = tc.tier_vision(3, n).to(dev())
        tap = torch.full((3, SMALL["n_query"], SMALL["hidden"]), float("nan"), device=dev())
        _lib.check(lib.infv_vqf_set_context_tap(m._handle(dev()), 0, C.c_void_p(tap.data_ptr())))
        m.encode_frames(x)
        xq = layer.query.bias.detach().expand(3, SMALL["n_query"], -1).contiguous()
        with RawHandle(SMALL) as rh:
            got = cross_attention(rh.h, x, (m.ln_vision.weight.detach(), m.ln_vision.bias.detach()), xq, layer.key.weight.detach(),
                                  layer.value.weight.detach(), layer.value.bias.detach(), layer.key.bias.detach())
        assert torch.equal(got, tap), n


# ---------------------------------------------------------------------------------------------------- 2. softmax edges
def run_case(case: str, lin: str = "fp32", attn: str = "fp16") -> torch.Tensor:
    sd, shape, x, ln = ac.model_case(case)
    m = small_model(lin, attn, ln) if sd is tc.small_sd() else new_model(shape, sd, lin, attn, ln)
    return m.encode_frames(x.to(dev())).cpu()


@pytest.mark.parametrize("case", ("hot257", "peak16", "peak48", "peak128"))
def test_softmax_edges_through_the_mode(case):
    """The hot key (+100 in every row) at every ``hot_positions(257)``, and the peaked models: within 2 x E_ref of float64."""
    ref = ac.model_ref(case)[0]
    e_ref = worst(ac.model_emu(case, 0, 1)[0], ref)
    got = run_case(case)
    err = worst(got, ref)
    record_parity(f"attention precision 2: {case}: max |hidden - ref64| {err:.3e}, E_ref {e_ref:.3e}; fp32 attention {worst(run_case(case, attn='fp32'), ref):.3e}")
    assert torch.isfinite(got).all() and err <= 2.0 * e_ref


def test_dead_keys_carry_no_mass():
    """The padded call at 257 tokens and the call on the same tokens followed by 63 dead keys (score -300: expf gives 0) are both
    within 2 x E_ref of the reference; whether they are the same bits is recorded."""
    ref = ac.model_ref("dead257")[0]
    e_ref = worst(ac.model_emu("dead257", 0, 1)[0], ref)
    a, b = run_case("dead257"), run_case("dead320")
    record_parity(f"attention precision 2: dead keys 257 / 320: max |hidden - ref64| {worst(a, ref):.3e} / {worst(b, ref):.3e}, E_ref {e_ref:.3e}, "
                  f"bit-equal {torch.equal(a, b)}")
    assert worst(a, ref) <= 2.0 * e_ref and worst(b, ref) <= 2.0 * e_ref


# ---------------------------------------------------------------------------------------------------- 3. the small model
@pytest.mark.parametrize("n_tokens", ac.SMALL_TOKENS)
def test_small_model_all_six_pairs(n_tokens):
    case = f"small{n_tokens}"
    ref = ac.model_ref(case)[0]
    got, err = {}, {}
    for lin, attn in PAIRS:
        got[lin, attn] = run_case(case, lin, attn)
        err[lin, attn] = worst(got[lin, attn], ref)
    e_ref = {lin: worst(ac.model_emu(case, LINEAR_PRECISIONS[lin], 1)[0], ref) for lin in LINEAR_PRECISIONS}
    record_parity(f"attention precision 3: small model 3 x {n_tokens}: max |hidden - ref64| " +
                  ", ".join(f"({l}, {a}) {v:.3e}" for (l, a), v in err.items()) + "; E_ref with fp16 attention " +
                  ", ".join(f"{l} {v:.3e}" for l, v in e_ref.items()))
    for lin in LINEAR_PRECISIONS:
        assert err[lin, "fp16"] <= 2.0 * e_ref[lin], (lin, err, e_ref)
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not torch.equal(got[a], got[b]), (a, b)


# ---------------------------------------------------------------------------------------------------- 4. the full model
def test_full_model_against_the_reference_golden():
    """12 layers, 768, 1408, 32 queries, 3 x 257 tokens: the reference encoder's hidden states and the cross-attention contexts of
    layers 0 and 10, for (fp32, fp16) and (fp16, fp16): each within 2 x E_ref of its own emulation."""
    g = np.load(GOLDEN_PATH)
    sd, shape, x, _ = ac.model_case("full")
    ref, ref_ctx = ac.model_ref("full")
    lib = _lib.load()
    for lin in ("fp32", "fp16"):
        emu, emu_ctx, _ = ac.model_emu("full", LINEAR_PRECISIONS[lin], 1)
        e_ref = {"hidden": worst(emu, ref)}
        e_ref.update({f"l{l}_xctx": worst(emu_ctx[l], ref_ctx[l]) for l in GOLDEN_TAPS})
        m = new_model(FULL, sd, lin, "fp16")
        err, out = {}, None
        for l in GOLDEN_TAPS:
            tap = torch.full((GOLDEN_FRAMES, FULL["n_query"], FULL["hidden"]), float("nan"), device=dev())
            _lib.check(lib.infv_vqf_set_context_tap(m._handle(dev()), l, C.c_void_p(tap.data_ptr())))
            out = m.encode_frames(x.to(dev()))
            err[f"l{l}_xctx"] = float(np.abs(tap.cpu().numpy() - g[f"l{l}_xctx"]).max())
        err["hidden"] = float(np.abs(out.cpu().numpy() - g["hidden"]).max())
        record_parity(f"attention precision 4: full model 3 x 257 vs the reference golden, ({lin}, fp16): " +
                      ", ".join(f"max |{k}| {v:.3e}" for k, v in sorted(err.items())) + "; E_ref " +
                      ", ".join(f"{k} {v:.3e}" for k, v in sorted(e_ref.items())) + f"; |hidden - emu64| {worst(out, emu):.3e}")
        assert all(err[k] <= 2.0 * e_ref[k] for k in err), (lin, err, e_ref)
        del m


# ---------------------------------------------------------------------------------------------------- 5. source dtypes
@pytest.mark.parametrize("n_tokens", (64, 257))
def test_source_and_output_dtypes_bit_for_bit(n_tokens):
    """fp16, bf16 and (LayerNorm off) fp8 e4m3 vision give the bits of the run on ``vision.float()``; fp16 and bf16 output buffers
    hold ``(fp32 result of the mode).to(dtype)``."""
    x = tc.tier_vision(3, n_tokens).to(dev())
    for ln, dtypes in ((True, (torch.float16, torch.bfloat16)), (False, (torch.float16, torch.bfloat16, torch.float8_e4m3fn))):
        m = small_model("fp32", "fp16", ln)
        for dt in dtypes:
            xs = x.to(dt)
            want = m.encode_frames(xs.float())
            assert torch.equal(m.encode_frames(xs), want), (ln, dt)
            assert not torch.isnan(want).any()
        want = m.encode_frames(x)
        for dt in (torch.float16, torch.bfloat16):
            out = torch.full(tuple(want.shape), float("nan"), device=dev(), dtype=dt)
            m.encode_frames(x, out_dtype=dt, out=out)
            assert torch.equal(out, want.to(dt)), (ln, dt)


# ---------------------------------------------------------------------------------------------------- 6. batch invariance
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32_vision", "fp16_vision"))
def test_a_frame_does_not_depend_on_the_batch(dtype):
    """Bit for bit: frame 3 of a 5-frame call, every frame of F = 17, of F = 129 (across the 128-frame row block of the linears) and
    of F = 258 (a sub-batch of 256 frames of the attention and a tail of two: frames 256 and 257 repeat frames 0 and 1) equal the
    1-frame call; the same at 257 tokens with F = 5; a frame whose successor is all NaN equals its 1-frame call."""
    m = small_model("fp32", "fp16")
    x = tc.tier_vision(129, 5).to(dev()).to(dtype)
    single = torch.cat([m.encode_frames(x[f:f + 1]) for f in range(129)])
    assert torch.equal(m.encode_frames(x[:5])[3], single[3])
    for n_f in (17, 129):
        assert torch.equal(m.encode_frames(x[:n_f]), single[:n_f]), n_f
    twice = torch.cat([x, x])
    assert torch.equal(m.encode_frames(twice), torch.cat([single, single]))
    assert not torch.equal(single, small_model("fp32", "fp32").encode_frames(x))
    for n in (5, 257):
        y = tc.tier_vision(5, n).to(dev()).to(dtype)
        one = torch.cat([m.encode_frames(y[f:f + 1]) for f in range(5)])
        assert torch.equal(m.encode_frames(y), one), n
        z = y[:2].clone()
        z[1] = float("nan")
        got = m.encode_frames(z)
        assert torch.equal(got[0], one[0]) and torch.isnan(got[1]).all(), n


# ---------------------------------------------------------------------------------------------------- 7. the handle
def raw_encode(m: FrameQformerEncoder, h, x: torch.Tensor, out: torch.Tensor) -> int:
    (w, vis), keep = m._weights(dev())
    rows = m.query_rows(dev())
    rc = _lib.load().infv_vqf_encode_frames(h, x.size(0), C.c_void_p(x.data_ptr()), 0, x.size(1), C.byref(w), C.byref(vis),
                                            C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()), 0, stream())
    del keep
    return rc


def test_weight_planes_are_cached_until_the_weights_change():
    x = tc.tier_vision(3, 257).to(dev())
    base = new_model(SMALL, tc.small_sd())
    base.encode_frames(x)                                                            # (grows the workspaces)
    _, n0 = counted(lambda: base.encode_frames(x))
    m = new_model(SMALL, tc.small_sd(), "fp32", "fp16")
    y1, n1 = counted(lambda: m.encode_frames(x))
    y2, n2 = counted(lambda: m.encode_frames(x))
    assert n2 < n1 and torch.equal(y1, y2)                                           # the second call builds no plane
    assert n1 - n2 == 2 * len(tc.CROSS_LAYERS)                                       # (two plane launches per cross layer)
    assert n2 < n0, (n0, n2)                                                         # no slab sum, no split launches
    # an in-place update of one key weight is seen: the call of a fresh encoder loaded with the changed weights
    p = m.Qformer.bert.encoder.layer[2].crossattention.self.key.weight
    with torch.no_grad():
        p.mul_(1.5)
    y3, n3 = counted(lambda: m.encode_frames(x))
    fresh = new_model(SMALL, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, "fp32", "fp16")
    assert torch.equal(y3, fresh.encode_frames(x)) and not torch.equal(y3, y2) and n3 == n1
    # weights epoch 0 at the raw ABI: the planes are rebuilt in every call
    with RawHandle(SMALL, 1) as rh:
        a, b = torch.full_like(y1, float("nan")), torch.full_like(y1, float("nan"))
        _, na = counted(lambda: _lib.check(raw_encode(fresh, rh.h, x, a)))
        _, nb = counted(lambda: _lib.check(raw_encode(fresh, rh.h, x, b)))
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, y3) and na == nb == n1, (na, nb, n1)
    record_parity(f"attention precision 7: small model 3 x 257 tokens: launches (fp32, fp32) {n0}, (fp32, fp16) first call {n1}, cached {n2}, "
                  f"epoch 0 {na}")


def test_other_entry_points_refuse_and_mode_0_is_the_handle_that_never_left_it():
    lib = _lib.load()
    m = small_model("fp32", "fp32")
    n_f, n_tokens, Q, Hd = 2, 64, SMALL["n_query"], SMALL["hidden"]
    x = tc.tier_vision(n_f, n_tokens).to(dev())
    rows = m.query_rows(dev())
    (w, _), keep = m._weights(dev())
    cu = (C.c_int32 * (n_f + 1))(*range(n_f + 1))
    tl = (C.c_int32 * n_f)(*([0] * n_f))
    hin = rows.repeat(n_f, 1).contiguous()
    layer = m.Qformer.bert.encoder.layer[0].crossattention.self
    key = _lib.Linear(layer.key.weight.data_ptr(), layer.key.bias.data_ptr())
    value = _lib.Linear(layer.value.weight.data_ptr(), layer.value.bias.data_ptr())
    xq = torch.randn(Q, Hd, device=dev())

    def videos(h, out):
        return lib.infv_vqf_vc_encode_videos(h, None, n_f, C.cast(cu, C.c_void_p), C.c_void_p(x.data_ptr()), 1, C.byref(w),
                                             C.c_void_p(hin.data_ptr()), C.cast(tl, C.c_void_p), None, 1, C.c_void_p(out.data_ptr()),
                                             None, None, stream())

    def short(h, out):
        return lib.infv_vqf_short_attention(h, C.c_void_p(x.data_ptr()), n_tokens, C.c_void_p(xq.data_ptr()), C.byref(key),
                                            C.byref(value), None, C.c_void_p(out.data_ptr()), stream())

    with RawHandle(SMALL, 0, 0, n_tokens) as rh, RawHandle(SMALL, 0, 0, n_tokens) as plain:
        _lib.check(lib.infv_vqf_set_attention_precision(rh.h, 1))
        assert lib.infv_vqf_set_attention_precision(rh.h, 2) == INVALID               # ... and the setting is kept:
        for call, shape in ((videos, (n_f, Q, Hd)), (short, (Q, Hd))):
            out = torch.full(shape, float("nan"), device=dev())
            (rc, n) = counted(lambda: call(rh.h, out))
            torch.cuda.synchronize()
            assert rc == UNSUPPORTED and n == 0 and torch.isnan(out).all()
            assert b"infv_vqf_set_attention_precision" in lib.infv_ltm_last_error()
        _lib.check(lib.infv_vqf_set_attention_precision(rh.h, 0))
        res = {}
        for tag, h in (("was_fp16", rh.h), ("plain", plain.h)):
            out = torch.full((n_f, Q, Hd), float("nan"), device=dev())
            _lib.check(videos(h, out))                                                # (grows the workspaces)
            rc, n = counted(lambda: videos(h, out))
            torch.cuda.synchronize()
            assert rc == 0
            res[tag] = (out, n)
        assert torch.equal(res["was_fp16"][0], res["plain"][0]) and res["was_fp16"][1] == res["plain"][1] > 0
    del keep
    # the same through the encoder: back on "fp32" it is the encoder that never left it
    back = new_model(SMALL, tc.small_sd(), "fp32", "fp16")
    y16 = back.encode_frames(x)
    back.set_attention_precision("fp32")
    back.encode_frames(x)
    y32, n32 = counted(lambda: back.encode_frames(x))
    m.encode_frames(x)
    ref, n_ref = counted(lambda: m.encode_frames(x))
    assert torch.equal(y32, ref) and n32 == n_ref and not torch.equal(y16, ref)


def test_refusals_of_the_new_entry_launch_nothing():
    shape = ac.UNIT_SHAPES["small"]
    u = {k: v.to(dev()) for k, v in ac.unit_inputs("small", 64).items()}
    lib = _lib.load()
    key, value = _lib.Linear(u["wk"].data_ptr(), None), _lib.Linear(u["wv"].data_ptr(), u["bv"].data_ptr())
    ctx = torch.full(tuple(u["xq"].shape), float("nan"), device=dev())

    def call(h, vision, code, n, xq=u["xq"]):
        return lib.infv_vqf_frame_cross_attention(h, 3, C.c_void_p(vision.data_ptr() if vision is not None else None), code, n, None,
                                                  C.c_void_p(xq.data_ptr()), C.byref(key), C.byref(value), C.c_void_p(ctx.data_ptr()), stream())

    with RawHandle(shape, 1) as rh:
        big = torch.zeros(3, 513, shape["enc_width"], device=dev())
        for args, want in (((u["vision"], 9, 64), INVALID), ((u["vision"], 0, 0), INVALID), ((None, 0, 64), INVALID),
                           ((big, 0, 513), UNSUPPORTED), ((u["vision"], 0, 64, u["xq"].view(-1)[1:]), INVALID)):
            (rc, n) = counted(lambda: call(rh.h, *args))
            assert rc == want and n == 0, (args[1:3], rc, n)
        torch.cuda.synchronize()
        assert torch.isnan(ctx).all()


# ---------------------------------------------------------------------------------------------------- 8. subnormal operands
def test_f16_mfma_on_a_subnormal_operand_is_measured():
    """Through ``infv_vqf_linear`` in fp16 (mode 2): x[0][0] = 2^-20 (an fp16 subnormal), w[0][0] = 2^10, everything else zero.
    y[0][0] is 2^-10 (the MFMA keeps subnormal operands) or 0 (it flushes them)."""
    x = torch.zeros(1, 64, device=dev())
    w = torch.zeros(64, 64, device=dev())
    x[0, 0], w[0, 0] = 2.0 ** -20, 2.0 ** 10
    y = torch.full((1, 64), float("nan"), device=dev())
    lin = (_lib.Linear * 1)(_lib.Linear(w.data_ptr(), None))
    with RawHandle(SMALL, 0, 2) as rh:
        _lib.check(_lib.load().infv_vqf_linear(rh.h, C.c_void_p(x.data_ptr()), 1, 64, lin, 1, 64, 0, None, 1, None, C.c_void_p(y.data_ptr()),
                                               stream()))
    got = float(y[0, 0])
    record_parity(f"attention precision 8: f16 MFMA with a subnormal operand (2^-20 x 2^10): y = {got!r}: "
                  f"{'kept' if got == 2.0 ** -10 else 'flushed' if got == 0.0 else 'neither'}")
    assert got in (2.0 ** -10, 0.0) and float(y[0, 1:].abs().max()) == 0.0
