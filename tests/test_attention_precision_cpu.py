"""The fp16 cross-attention of the frame Q-former without a device: the exported symbols and the documented header, the refusals
that need no device, the Python names, and -- on the very inputs the GPU tests use -- the conditions their bounds rest on: that the
mode's own rounding is far larger than fp32 noise, that the two power-of-two scalings keep the fp16 operands out of the subnormal
range, and that nothing overflows fp16."""
import ctypes as C
import os
import re

import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.frame_qformer import ATTENTION_PRECISIONS, LINEAR_PRECISIONS, FrameQformerEncoder
from tests.golden import attention_precision_cases as ac
from tests.golden import linear_precision_cases as lc
from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def worst(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


# ---------------------------------------------------------------------------------------------------- 1. the interface
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("infv_vqf_set_attention_precision", "infv_vqf_frame_cross_attention"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.infv_ltm_abi_version() == 6 and _lib.ABI_VERSION == 6                  # additive symbols, same ABI


def test_ctypes_lists_match_the_header():
    """The argument count and the integer / pointer kind of every argument of the two prototypes, read from the header."""
    header = open(os.path.join(ROOT, "include", "infv_vqf.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("infv_vqf_set_attention_precision", "infv_vqf_frame_cross_attention"):
        m = re.search(r"int " + name + r"\((.*?)\);", header, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, ctypes_args = _lib._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(ctypes_args), (name, args)
        for a, t in zip(args, ctypes_args):
            is_ptr = "*" in a or a.startswith("infv_vqf_handle")
            assert is_ptr == (t is C.c_void_p or hasattr(t, "contents")), (name, a, t)
            if not is_ptr:
                assert t is C.c_int32 and a.startswith("int32_t"), (name, a, t)


def test_header_says_what_the_mode_rounds():
    header = open(os.path.join(ROOT, "include", "infv_vqf.h")).read()
    for needle in ("fp16(32 * sum_c fp16(q[c]) * fp16(Wk[c][:]))", "2^8 / sqrt(64)", "fp16(2^10 * p)", "fp16(2^-10 * sum_j", "65504",
                   "|q~| >= 256", "INFV_ERR_UNSUPPORTED before any launch", "461 MB", "26 MB", "infv_vqf_set_context_tap works in both modes"):
        assert needle in header, needle


# ---------------------------------------------------------------------------------------------------- 2. refusals without a device
def test_both_entry_points_validate_on_the_host():
    lib = _lib.load()
    for mode in (0, 1, 2, -1):
        assert lib.infv_vqf_set_attention_precision(None, mode) == INVALID           # a null handle, whatever the mode
    assert b"null" in lib.infv_ltm_last_error()
    assert lib.infv_vqf_frame_cross_attention(None, 1, None, 0, 64, None, None, None, None, None, None) == INVALID
    assert b"frame_cross_attention" in lib.infv_ltm_last_error()


# ---------------------------------------------------------------------------------------------------- 3. the Python names
def test_python_names_are_validated_before_any_device_call():
    small = dict(num_query_token=SMALL["n_query"], vision_width=SMALL["enc_width"], num_hidden_layers=SMALL["n_layers"],
                 hidden_size=SMALL["hidden"], intermediate_size=SMALL["inter"], num_attention_heads=SMALL["n_heads"])
    assert ATTENTION_PRECISIONS == {"fp32": 0, "fp16": 1} == ac.ATTN_MODES
    assert FrameQformerEncoder(**small).attention_precision == "fp32"
    for lin in LINEAR_PRECISIONS:
        for name in ATTENTION_PRECISIONS:
            m = FrameQformerEncoder(linear_precision=lin, attention_precision=name, **small)
            assert (m.linear_precision, m.attention_precision) == (lin, name) and m._vqf is None
    for bad in ("bf16", "FP16", "split_bf16", "", None, 1):
        with pytest.raises(ValueError, match="fp16.*fp32"):
            FrameQformerEncoder(attention_precision=bad, **small)
        m = FrameQformerEncoder(**small)
        with pytest.raises(ValueError, match="fp16.*fp32"):
            m.set_attention_precision(bad)
        assert m.attention_precision == "fp32" and m._vqf is None
    m = FrameQformerEncoder(**small)
    m.set_attention_precision("fp16")
    assert m.attention_precision == "fp16" and m.linear_precision == "fp32" and m._vqf is None


# ---------------------------------------------------------------------------------------------------- 4. what the GPU bounds rest on
@pytest.mark.parametrize("ln", (True, False), ids=("ln", "plain"))
@pytest.mark.parametrize("shape_name", sorted(ac.UNIT_SHAPES))
def test_unit_cases_the_mode_dwarfs_fp32_and_stays_in_range(shape_name, ln):
    for n in ac.UNIT_TOKENS:
        ref = ac.unit_ref(shape_name, n, ln)
        emu, st = ac.unit_emu(shape_name, n, ln)
        e_ref, e32 = worst(emu, ref), worst(ac.unit_ref(shape_name, n, ln, torch.float32), ref)
        print(f"{shape_name} n {n} ln {ln}: E_ref {e_ref:.3e}, fp32 {e32:.3e}, subnormal q~' {ac.subnormal_share(st['qt']):.2e} p' "
              f"{ac.subnormal_share(st['pp']):.2e}")
        assert e_ref >= 5 * e32, (n, e_ref, e32)
        assert ac.subnormal_share(st["qt"]) < 1e-3 and ac.subnormal_share(st["pp"]) < 1e-3
        for k in ("qt", "pp", "xh", "oo"):
            assert torch.isfinite(st[k]).all() and float(st[k].abs().max()) <= ac.F16_MAX, k


@pytest.mark.parametrize("case", ac.MODEL_CASES)
def test_model_cases_the_mode_dwarfs_fp32_and_stays_in_range(case):
    """E_ref = max |emu64 - ref64| >= 5 x the fp32 restatement's error for the hidden states (fp32 linears, fp16 attention) and for
    every cross layer's context; less than 1e-3 of the non-zero q~' and p' are fp16-subnormal on the plain cases; nothing overflows
    fp16 on any case -- the hot and the dead keys included."""
    ref, ref_ctx = ac.model_ref(case)
    r32, r32_ctx = ac.model_ref(case, torch.float32)
    emu, emu_ctx, st = ac.model_emu(case, 0, 1)
    e_ref, e32 = worst(emu, ref), worst(r32, ref)
    print(f"{case}: hidden E_ref {e_ref:.3e}, fp32 {e32:.3e}")
    assert e_ref >= 5 * e32
    for l in emu_ctx:
        e_l, e32_l = worst(emu_ctx[l], ref_ctx[l]), worst(r32_ctx[l], ref_ctx[l])
        print(f"{case}: layer {l} context E_ref {e_l:.3e}, fp32 {e32_l:.3e}, subnormal q~' {ac.subnormal_share(st[l]['qt']):.2e} p' "
              f"{ac.subnormal_share(st[l]['pp']):.2e}, max |q~'| {float(st[l]['qt'].abs().max()):.1f} max |x^| {float(st[l]['xh'].abs().max()):.1f}")
        assert e_l >= 5 * e32_l
        for k in ("qt", "pp", "xh", "oo"):
            assert torch.isfinite(st[l][k]).all() and float(st[l][k].abs().max()) <= ac.F16_MAX, (l, k)
        if case in ac.PLAIN_CASES:
            assert ac.subnormal_share(st[l]["qt"]) < 1e-3 and ac.subnormal_share(st[l]["pp"]) < 1e-3
    if case == "full":
        e_ref22 = worst(ac.model_emu(case, 2, 1)[0], ref)
        print(f"{case}: hidden E_ref with fp16 linears {e_ref22:.3e}")
        assert e_ref22 >= 5 * e32


def test_dead_keys_and_the_padded_call_agree_exactly_in_the_emulation():
    a, b = ac.model_emu("dead257", 0, 1)[0], ac.model_emu("dead320", 0, 1)[0]
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 5. the restatement, mode off
@pytest.mark.parametrize("lin_mode", (0, 2))
def test_emulation_with_the_attention_mode_off_is_the_linear_emulation(lin_mode):
    x = tc.tier_vision(3, 65)
    ctx_a, ctx_b = {}, {}
    a = ac.emu64(tc.small_sd(), SMALL, x, True, lin_mode, 0, ctx_out=ctx_a)
    b = lc.emu64(tc.small_sd(), SMALL, x, True, lin_mode, ctx_out=ctx_b)
    assert torch.equal(a, b) and all(torch.equal(ctx_a[l], ctx_b[l]) for l in ctx_b)
    assert not torch.equal(ac.emu64(tc.small_sd(), SMALL, x, True, lin_mode, 1), a)


def test_unit_emulation_is_the_model_emulation_of_one_layer():
    """The single-layer restatement the stand-alone entry is tested against is the model's layer: ``attend16`` on the cross query
    that ``emu64`` computed for a layer, over the model's normalised tokens and that layer's weights read from the state dict,
    gives the layer's context; the exact restatement ``attend64`` on the reference's query gives the reference's context to float64
    rounding (it drops the key bias and projects in another order)."""
    sd, shape, x, ln = ac.model_case("small64")
    _, ctx, st = ac.model_emu("small64", 0, 1)
    H = shape["n_heads"]
    for l in ctx:
        wk, wv, bv = ac.layer_inputs(sd, l)
        assert torch.equal(ac.attend16(st[l]["q"], st[l]["k"], wk, wv, bv, H), ctx[l]), l
    c: dict = {}
    tc.ref64(sd, shape, x, ln, collect=c)
    wk, wv, bv = ac.layer_inputs(sd, 0)
    # (layer 0: nothing in front of it is rounded with fp32 linears, so the emulation's query is the reference's)
    assert float((ac.attend64(st[0]["q"], st[0]["k"], wk, wv, bv, H) - c["ctx"][0]).abs().max()) < 1e-12
