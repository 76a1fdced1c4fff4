"""The reduced linear precisions of the frame Q-former without a device: the exported symbols and the documented header, the Python
names, and -- on the very inputs the GPU tests use -- the conditions those tests rest on: that a reduced mode's own rounding is far
larger than what a summation order can move, so a bound of twice the sequential-fp32 error tells a right kernel from a wrong one."""
import os

import pytest
import torch

from infinite_video_amd import _lib
from infinite_video_amd.frame_qformer import LINEAR_PRECISIONS, FrameQformerEncoder
from tests.golden import linear_precision_cases as lc
from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import (FULL, GOLDEN_FRAMES, GOLDEN_TOKENS, SMALL, frame_qformer_weights, vision_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worst(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


# ---------------------------------------------------------------------------------------------------- the interface
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("infv_vqf_set_linear_precision", "infv_vqf_linear"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.infv_ltm_abi_version() == 6 and _lib.ABI_VERSION == 6                  # additive symbols, same ABI


def test_header_documents_both_entry_points():
    header = open(os.path.join(ROOT, "include", "infv_vqf.h")).read()
    for needle in ("int infv_vqf_set_linear_precision(infv_vqf_handle h, int32_t mode);", "int infv_vqf_linear(infv_vqf_handle h,",
                   "lo.hi, hi.lo, hi.hi", "65504", "INFV_ERR_UNSUPPORTED before any launch", "Gibbs draw", "370 MB", "185 MB",
                   "not measured"):
        assert needle in header, needle


def test_setter_validates_on_the_host():
    lib = _lib.load()
    for mode in (0, 1, 2, 7, -1):
        assert lib.infv_vqf_set_linear_precision(None, mode) == -1                   # INFV_ERR_INVALID: a null handle, whatever the mode
    assert b"null" in lib.infv_ltm_last_error()
    assert lib.infv_vqf_linear(None, None, 1, 64, None, 1, 64, 0, None, 1, None, None, None) == -1


def test_python_names_are_validated_before_any_device_call():
    small = dict(num_query_token=SMALL["n_query"], vision_width=SMALL["enc_width"], num_hidden_layers=SMALL["n_layers"],
                 hidden_size=SMALL["hidden"], intermediate_size=SMALL["inter"], num_attention_heads=SMALL["n_heads"])
    assert LINEAR_PRECISIONS == {"fp32": 0, "split_bf16": 1, "fp16": 2} == lc.MODES
    assert FrameQformerEncoder(**small).linear_precision == "fp32"
    for name in LINEAR_PRECISIONS:
        m = FrameQformerEncoder(linear_precision=name, **small)
        assert m.linear_precision == name and m._vqf is None                         # no handle yet: nothing touched a device
    for bad in ("bf16", "FP16", "", None, 1):
        with pytest.raises(ValueError):
            FrameQformerEncoder(linear_precision=bad, **small)
        m = FrameQformerEncoder(**small)
        with pytest.raises(ValueError):
            m.set_linear_precision(bad)
        assert m.linear_precision == "fp32" and m._vqf is None
    m = FrameQformerEncoder(**small)
    m.set_linear_precision("fp16")
    assert m.linear_precision == "fp16" and m._vqf is None


# ---------------------------------------------------------------------------------------------------- the restatements
def test_emulation_in_mode_0_is_the_float64_reference():
    x = tc.tier_vision(3, 65)
    assert torch.equal(lc.emu64(tc.small_sd(), SMALL, x, True, 0), tc.ref64(tc.small_sd(), SMALL, x, True))


def test_unit_inputs_hold_no_fp16_subnormal():
    for K in lc.UNIT_K:
        for t in lc.unit_inputs(K):
            assert float(t.abs().min()) >= lc.FLOOR and torch.equal(t.half().float().abs() >= 2.0 ** -14, torch.ones_like(t, dtype=torch.bool))


@pytest.mark.parametrize("K", lc.UNIT_K)
def test_a_fp16_rounding_dwarfs_the_summation_order(K):
    """(a) max |ref_linear_2 - ref_linear_0| >= 100 x max |seq32_2 - ref_linear_2|: a kernel that skipped the rounding, or rounded
    something else, is outside twice the sequential error by a factor of 50."""
    mode_cost = worst(lc.unit_ref(K, 2), lc.unit_ref(K, 0))
    order_cost = worst(lc.unit_seq32(K, 2), lc.unit_ref(K, 2))
    print(f"K = {K}: fp16 rounding {mode_cost:.3e}, sequential fp32 sum {order_cost:.3e}")
    assert mode_cost >= 100 * order_cost


@pytest.mark.parametrize("K", (64, 128))
def test_b_dropped_lo_lo_term_is_visible_at_short_depth(K):
    """(b) max |ref_linear_1 - ref_linear_0| >= 5 x max |seq32_1 - ref_linear_1| at K = 64 and 128 only: at K >= 768 mode 1 is
    fp32-class and cannot be told from mode 0 by error size."""
    mode_cost = worst(lc.unit_ref(K, 1), lc.unit_ref(K, 0))
    order_cost = worst(lc.unit_seq32(K, 1), lc.unit_ref(K, 1))
    print(f"K = {K}: split-bf16 {mode_cost:.3e}, sequential fp32 sum {order_cost:.3e}")
    assert mode_cost >= 5 * order_cost


@pytest.mark.parametrize("name,shape,n_tokens", [("small", SMALL, 65), ("full", FULL, GOLDEN_TOKENS)])
def test_c_fp16_model_error_dwarfs_fp32(name, shape, n_tokens):
    """(c) E_ref_2 = max |emu64_2 - ref64| >= 20 x the fp32 restatement's error, on the model inputs of the GPU tests."""
    if name == "small":
        sd, x = tc.small_sd(), tc.tier_vision(3, n_tokens)
    else:
        sd, x = frame_qformer_weights(**FULL), torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"]))
    ref = tc.ref64(sd, shape, x, True)
    e2 = worst(lc.emu64(sd, shape, x, True, 2), ref)
    e32 = worst(tc.ref64(sd, shape, x, True, dtype=torch.float32), ref)
    print(f"{name}: E_ref_2 {e2:.3e}, fp32 restatement {e32:.3e}")
    assert e2 >= 20 * e32
