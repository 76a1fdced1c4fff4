"""The query-side linears of the frame Q-former in split-bf16 and fp16 (``infv_vqf_set_linear_precision``), on the device.

1. the linear alone (``infv_vqf_linear``) against the float64 product of the prepared operands, within twice the error of the
   sequential fp32 sum of the same products (``tests/test_linear_precision_cpu.py`` shows that a mode's own rounding is 5 to 100
   times that error on these inputs, so the bound tells the modes apart);
2. the epilogues on a reduced product;
3. the small and 4. the full model: split-bf16 within the project's 2e-4 of float64, fp16 within twice what the float64 emulation
   of the fp16 operands costs;
5. batch invariance, bit for bit; 6. the weight-plane cache; 7. the refusals of every other entry point.

Every test calls ``infv_vqf_set_linear_precision`` or ``infv_vqf_linear``: none passes on a library without them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.basis_maps import NB_SAMPLES
from infinite_video_amd.frame_qformer import LINEAR_PRECISIONS, FrameQformerEncoder
from tests.conftest import record_parity
from tests.golden import linear_precision_cases as lc
from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import (FULL, GOLDEN_FRAMES, GOLDEN_PATH, GOLDEN_TAPS, GOLDEN_TOKENS, SMALL,
                                              frame_qformer_weights, vision_rows)

pytestmark = pytest.mark.gpu
ATOL = tc.ATOL                              # the project's own 2e-4
INVALID, UNSUPPORTED = -1, -2
NAMES = {v: k for k, v in LINEAR_PRECISIONS.items()}


def dev():
    return torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def launches() -> int:
    return int(_lib.load().infv_ltm_launch_count())


def worst(a, b) -> float:
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def small_cfg(n_tokens: int = 1):
    return _lib.VqfConfig(1, SMALL["n_heads"], SMALL["hidden"], SMALL["inter"], SMALL["enc_width"], n_tokens, SMALL["n_query"], 0,
                          NB_SAMPLES, 1.0, 1e-12)


class RawHandle:
    """A handle of its own at the C ABI (weights epoch 0 unless set: every linear rebuilds its planes)."""

    def __init__(self, mode: int = 0, tokens_per_frame: int = 1):
        self.h = C.c_void_p()
        cfg = small_cfg(tokens_per_frame)
        _lib.check(_lib.load().infv_vqf_create(C.byref(cfg), C.byref(self.h)))
        if mode:
            _lib.check(_lib.load().infv_vqf_set_linear_precision(self.h, mode))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.load().infv_vqf_destroy(self.h)


def new_model(shape: dict, sd: dict, precision: str = "fp32") -> FrameQformerEncoder:
    m = FrameQformerEncoder(num_query_token=shape["n_query"], vision_width=shape["enc_width"], num_hidden_layers=shape["n_layers"],
                            hidden_size=shape["hidden"], intermediate_size=shape["inter"], num_attention_heads=shape["n_heads"],
                            linear_precision=precision)
    m.load_reference_state_dict(sd)
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def small_model(precision: str) -> FrameQformerEncoder:
    return new_model(SMALL, tc.small_sd(), precision)


# ---------------------------------------------------------------------------------------------------- 1. the linear alone
def run_linear(h, x, ws, bs=None, act=0, residual=None, ln=None) -> torch.Tensor:
    """``infv_vqf_linear`` of x [M][K] through the stacked weights ``ws`` (each [n_out][K]) on handle h."""
    n_lin, n_out = len(ws), ws[0].size(0)
    lin = (_lib.Linear * n_lin)(*[_lib.Linear(w.data_ptr(), bs[i].data_ptr() if bs else None) for i, w in enumerate(ws)])
    y = torch.full((x.size(0), n_lin * n_out), float("nan"), device=dev())
    lnorm = _lib.LayerNorm(ln[0].data_ptr(), ln[1].data_ptr()) if ln else None
    _lib.check(_lib.load().infv_vqf_linear(h, C.c_void_p(x.data_ptr()), x.size(0), x.size(1), lin, n_lin, n_out, act,
                                           C.c_void_p(residual.data_ptr()) if residual is not None else None,
                                           residual.size(0) if residual is not None else 1, C.byref(lnorm) if ln else None,
                                           C.c_void_p(y.data_ptr()), stream()))
    return y


@pytest.mark.parametrize("n_lin,n_out", lc.UNIT_N)
@pytest.mark.parametrize("K", lc.UNIT_K)
def test_linear_alone_within_twice_the_sequential_fp32_error(K, n_lin, n_out):
    """max |y - ref_linear_m| <= 2 x max |seq32_m - ref_linear_m| (the right side over the 257-row problem) for M = 1, 31, 128,
    129, 257 in modes 1 and 2.  The sequential fp32 sum of the same products is the reference arithmetic; the factor 2 allows for
    the MFMA's other grouping of the same additions.  Mode 0 runs beside them as a control: recorded, not asserted."""
    N = n_lin * n_out
    x_cpu, w_cpu = lc.unit_inputs(K)
    x = x_cpu.to(dev())
    ws = [w_cpu[i * n_out:(i + 1) * n_out].clone().to(dev()) for i in range(n_lin)]           # every segment a tensor of its own
    full = {}
    for mode in (0, 1, 2):
        ref = lc.unit_ref(K, mode)[:, :N]
        bound = 2.0 * worst(lc.unit_seq32(K, mode)[:, :N], ref)
        with RawHandle(mode) as rh:
            errs = {}
            for M in lc.UNIT_M:
                y = run_linear(rh.h, x[:M].contiguous(), ws)
                assert not torch.isnan(y).any()
                errs[M] = worst(y, ref[:M])
                if M == lc.UNIT_ROWS:
                    full[mode] = y
        record_parity(f"linear precision 1: K {K} N {n_lin} x {n_out} {NAMES[mode]}: max |y - ref_linear| " +
                      ", ".join(f"M {M}: {e:.3e}" for M, e in errs.items()) + f"; bound 2 x seq32 = {bound:.3e}; worst ratio to seq32 "
                      f"{2.0 * max(errs.values()) / bound:.3f}")
        if mode:
            assert all(e <= bound for e in errs.values()), (mode, errs, bound)
    assert not torch.equal(full[1], full[0]) and not torch.equal(full[2], full[1])


# ---------------------------------------------------------------------------------------------------- 2. epilogues
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("kind", ("gelu", "ln", "stacked"))
def test_epilogues_on_a_reduced_product(kind, mode):
    """(M 129, K 128, N 192): bias + GELU, bias + residual + LayerNorm, the stacked three-bias form, against the float64 epilogue
    of ``ref_linear_m``.  Bound: ``seq32_m`` pushed through the same float64 epilogue, x 2, plus the project's 2e-6 for the LayerNorm."""
    M, K, N = lc.EPI_SHAPE
    x_cpu, w_cpu = lc.unit_inputs(K)
    e = {k: v.to(dev()) for k, v in lc.epilogue_inputs().items()}
    x = x_cpu[:M].contiguous().to(dev())
    with RawHandle(mode) as rh:
        if kind == "stacked":
            ws = [w_cpu[i * 64:(i + 1) * 64].clone().to(dev()) for i in range(3)]
            y = run_linear(rh.h, x, ws, bs=[e["bias"][i * 64:(i + 1) * 64].clone() for i in range(3)])
        else:
            ws = [w_cpu[:N].contiguous().to(dev())]
            if kind == "gelu":
                y = run_linear(rh.h, x, ws, bs=[e["bias"]], act=1)
            else:
                y = run_linear(rh.h, x, ws, bs=[e["bias"]], residual=e["residual"], ln=(e["gamma"], e["beta"]))
    ref = lc.epilogue64(lc.unit_ref(K, mode)[:M, :N], kind)
    bound = 2.0 * worst(lc.epilogue64(lc.unit_seq32(K, mode)[:M, :N], kind), ref) + (lc.LN_ATOL if kind == "ln" else 0.0)
    err = worst(y, ref)
    record_parity(f"linear precision 2: epilogue {kind} {NAMES[mode]}: max |y - float64 epilogue of ref_linear| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------- 3. the small model
@pytest.mark.parametrize("n_tokens", (5, 64, 257))
def test_small_model(n_tokens):
    """Three frames, ``ln_vision`` on.  Split-bf16 within 2e-4 of float64; fp16 within 2 x E_ref_2 = max |emu64_2 - ref64| (the
    device rounds intermediate activations from fp32 values, the emulation from float64 values: a flipped rounding costs what the
    rounding itself costs).  |gpu_2 - emu64_2| is recorded.  Both differ from the fp32 output."""
    x = tc.tier_vision(3, n_tokens)
    ref = tc.ref64(tc.small_sd(), SMALL, x, True)
    emu2 = lc.emu64(tc.small_sd(), SMALL, x, True, 2)
    e_ref2 = worst(emu2, ref)
    got = {name: small_model(name).encode_frames(x.to(dev())).cpu() for name in LINEAR_PRECISIONS}
    err = {name: worst(g, ref) for name, g in got.items()}
    record_parity(f"linear precision 3: small model 3 x {n_tokens} tokens: max |device - float64| " +
                  ", ".join(f"{k} {v:.3e}" for k, v in err.items()) + f"; E_ref_2 {e_ref2:.3e}; |fp16 device - emu64_2| {worst(got['fp16'], emu2):.3e}")
    assert err["split_bf16"] <= ATOL
    assert err["fp16"] <= 2.0 * e_ref2
    assert not torch.equal(got["split_bf16"], got["fp32"]) and not torch.equal(got["fp16"], got["fp32"])


# ---------------------------------------------------------------------------------------------------- 4. the full model
def test_full_model_against_the_reference_golden():
    """12 layers, 768, 1408, 32 queries, 3 x 257 tokens: the real reference encoder's hidden states and the cross-attention context of
    the first and the last cross layer.  Split-bf16 within 2e-4 (the CPU emulation predicts 4.2e-5); fp16 within 2 x E_ref_2, of
    the hidden states and of each context."""
    g = np.load(GOLDEN_PATH)
    sd = frame_qformer_weights(**FULL)
    x = torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"]))
    ref_ctx, emu_ctx = {}, {}
    ref = tc.ref64(sd, FULL, x, True, collect=ref_ctx)
    e_ref2 = {"hidden": worst(lc.emu64(sd, FULL, x, True, 2, ctx_out=emu_ctx), ref)}
    for l in GOLDEN_TAPS:
        e_ref2[f"l{l}_xctx"] = worst(emu_ctx[l], ref_ctx["ctx"][l])
    lib = _lib.load()
    for name in ("split_bf16", "fp16"):
        m = new_model(FULL, sd, name)
        err, out = {}, None
        for l in GOLDEN_TAPS:
            tap = torch.full((GOLDEN_FRAMES, FULL["n_query"], FULL["hidden"]), float("nan"), device=dev())
            _lib.check(lib.infv_vqf_set_context_tap(m._handle(dev()), l, C.c_void_p(tap.data_ptr())))
            out = m.encode_frames(x.to(dev()))
            err[f"l{l}_xctx"] = float(np.abs(tap.cpu().numpy() - g[f"l{l}_xctx"]).max())
        err["hidden"] = float(np.abs(out.cpu().numpy() - g["hidden"]).max())
        record_parity(f"linear precision 4: full model 3 x 257 tokens vs the reference golden, {name}: " +
                      ", ".join(f"max |{k}| {v:.3e}" for k, v in sorted(err.items())) +
                      "; E_ref_2 " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(e_ref2.items())))
        if name == "split_bf16":
            assert all(v <= ATOL for v in err.values()), err
        else:
            assert all(err[k] <= 2.0 * e_ref2[k] for k in err), (err, e_ref2)
        del m


# ---------------------------------------------------------------------------------------------------- 5. batch invariance
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32_vision", "fp16_vision"))
@pytest.mark.parametrize("name", ("split_bf16", "fp16"))
def test_a_frame_does_not_depend_on_the_batch(name, dtype):
    """Bit for bit: frame 3 of a 5-frame call, every frame of F = 17 (M = 136: across the 128-row tile) and of F = 129 (across
    kRowBlockVideos, a tail block of one frame) equal the 1-frame call on that frame; an fp16 output buffer holds
    ``(fp32 result of that mode).to(float16)``."""
    m = small_model(name)
    x = tc.tier_vision(129, 5).to(dev()).to(dtype)
    single = torch.cat([m.encode_frames(x[f:f + 1]) for f in range(129)])
    assert torch.equal(m.encode_frames(x[:5])[3], single[3])
    for n_f in (17, 129):
        got = m.encode_frames(x[:n_f])
        assert torch.equal(got, single[:n_f]), n_f
        half = torch.full((n_f, SMALL["n_query"], SMALL["hidden"]), float("nan"), device=dev(), dtype=torch.float16)
        m.encode_frames(x[:n_f], out_dtype=torch.float16, out=half)
        assert torch.equal(half, got.to(torch.float16)), n_f
    assert not torch.equal(single, small_model("fp32").encode_frames(x))


# ---------------------------------------------------------------------------------------------------- 6. the plane cache
def raw_encode(m: FrameQformerEncoder, h, x: torch.Tensor, out: torch.Tensor) -> int:
    (w, vis), keep = m._weights(dev())
    rows = m.query_rows(dev())
    rc = _lib.load().infv_vqf_encode_frames(h, x.size(0), C.c_void_p(x.data_ptr()), 0, x.size(1), C.byref(w), C.byref(vis),
                                            C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()), 0, stream())
    del keep
    return rc


def counted(fn):
    l0 = launches()
    out = fn()
    return out, launches() - l0


@pytest.mark.parametrize("name", ("split_bf16", "fp16"))
def test_weight_planes_are_cached_until_the_weights_change(name):
    x = tc.tier_vision(3, 65).to(dev())
    base = new_model(SMALL, tc.small_sd())
    base.encode_frames(x)                                                            # (grows the workspaces)
    _, n0 = counted(lambda: base.encode_frames(x))
    m = new_model(SMALL, tc.small_sd(), name)
    y1, n1 = counted(lambda: m.encode_frames(x))
    y2, n2 = counted(lambda: m.encode_frames(x))
    assert n2 == n0 and n1 > n0, (n0, n1, n2)                                        # the second call builds no plane
    assert torch.equal(y1, y2)
    # an in-place update of one weight: the next call is the call of a fresh encoder loaded with the changed weights.
    # (The update goes through the parameter itself: a write through ``p.data`` does not bump ``p._version``, which is what the
    # encoder's weight signature -- and with it the handle's weights epoch -- is made of; see FrameQformerEncoder.set_linear_precision.)
    p = m.Qformer.bert.encoder.layer[1].intermediate_query.dense.weight
    with torch.no_grad():
        p.mul_(1.5)
    y3, n3 = counted(lambda: m.encode_frames(x))
    fresh = new_model(SMALL, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, name)
    assert torch.equal(y3, fresh.encode_frames(x)) and not torch.equal(y3, y2)
    assert n3 == n1                                                                  # every plane was rebuilt
    # weights epoch 0 at the raw ABI: the planes are rebuilt in every call
    with RawHandle(LINEAR_PRECISIONS[name]) as rh:
        a = torch.full_like(y1, float("nan"))
        b = torch.full_like(y1, float("nan"))
        _, na = counted(lambda: _lib.check(raw_encode(fresh, rh.h, x, a)))
        _, nb = counted(lambda: _lib.check(raw_encode(fresh, rh.h, x, b)))
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, y3)
        assert na == nb == n1, (na, nb, n1)
    record_parity(f"linear precision 6: small model 3 x 65 tokens {name}: launches fp32 {n0}, first call {n1}, cached {n2}, epoch 0 {na}")


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_other_entry_points_refuse_a_reduced_handle():
    lib = _lib.load()
    m = small_model("fp32")
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

    with RawHandle(0, n_tokens) as rh, RawHandle(0, n_tokens) as plain:
        _lib.check(lib.infv_vqf_set_linear_precision(rh.h, 1))
        assert lib.infv_vqf_set_linear_precision(rh.h, 7) == INVALID                  # ... and the setting is kept:
        for call, shape in ((videos, (n_f, Q, Hd)), (short, (Q, Hd))):
            out = torch.full(shape, float("nan"), device=dev())
            (rc, n) = counted(lambda: call(rh.h, out))
            torch.cuda.synchronize()
            assert rc == UNSUPPORTED and n == 0 and torch.isnan(out).all()
            assert b"infv_vqf_set_linear_precision" in lib.infv_ltm_last_error()
        # back on mode 0 the call is what it is on a handle that never set a mode: bits and launches
        _lib.check(lib.infv_vqf_set_linear_precision(rh.h, 0))
        res = {}
        for tag, h in (("was_reduced", rh.h), ("plain", plain.h)):
            out = torch.full((n_f, Q, Hd), float("nan"), device=dev())
            _lib.check(videos(h, out))                                                # (grows the workspaces)
            rc, n = counted(lambda: videos(h, out))
            torch.cuda.synchronize()
            assert rc == 0
            res[tag] = (out, n)
        assert torch.equal(res["was_reduced"][0], res["plain"][0]) and res["was_reduced"][1] == res["plain"][1] > 0
        assert not torch.isnan(res["plain"][0]).any()
    del keep
    # the same through the encoder: back on "fp32" it is the encoder that never left it
    back = new_model(SMALL, tc.small_sd(), "fp16")
    y16 = back.encode_frames(x)
    back.set_linear_precision("fp32")
    back.encode_frames(x)
    y32, n32 = counted(lambda: back.encode_frames(x))
    m.encode_frames(x)
    ref, n_ref = counted(lambda: m.encode_frames(x))
    assert torch.equal(y32, ref) and n32 == n_ref and not torch.equal(y16, ref)
