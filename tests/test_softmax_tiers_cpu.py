"""The constructions of ``tests/golden/softmax_tier_cases.py`` checked in float64 on the very tensors the device tests read: the
dead key is dead (at least 150 under every live score of its row), the hot key is hot (at least 90 over every other score), the
peaked models are peaked, and the reference itself -- restated in fp32 -- stays within ATOL / 10 of float64, so the bound the
device is held to is not spent on the reference.  No GPU."""
import pytest
import torch

from tests.golden import softmax_tier_cases as tc
from tests.golden.frame_qformer_cases import SMALL

CROSS = tc.CROSS_LAYERS


def evaluate(sd, x, ln, dtype=torch.float64):
    c = {}
    out = tc.ref64(sd, SMALL, x, ln, collect=c, dtype=dtype)
    return out, c


def test_the_margins_are_what_fp32_expf_needs():
    """expf of the dead margin is exactly 0 and expf of the hot margin is inf in fp32: what the two constructions rest on."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    assert float(torch.exp(f32(-tc.DEAD_MARGIN))) == 0.0
    assert torch.isinf(torch.exp(f32(tc.HOT_MARGIN)))
    assert float(torch.exp(f32(-104.0))) == 0.0 and -104.0 > -tc.DEAD_MARGIN          # (0 from about -103.98 on: 150 leaves room)


def test_the_score_rows_are_the_scores_up_to_a_row_constant():
    """``collect["A"]`` . key differs from the reference's own scores by one constant per row (the key bias): the rows the
    crafted keys are solved against are the rows the softmax sees."""
    x = tc.tier_vision(3, 65)
    _, c = evaluate(tc.small_sd(), x, False)
    for l in CROSS:
        s = c["scores"][l]                                                          # [F, H, Q, n]
        mine = torch.einsum("fre,fne->frn", c["A"][l], x.double()).reshape(s.shape)
        shift = s - mine
        assert float((shift - shift[..., :1]).abs().max()) < 1e-12
        assert float(s.abs().max()) < 0.5                                           # the flat regime the crafted keys leave


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,n_pad", tc.PAD_PAIRS)
def test_dead_keys_are_dead(n, n_pad, bf16):
    x = tc.dead_padded(n, n_pad, bf16)
    assert tuple(x.shape) == (2, n_pad, SMALL["enc_width"]) and n_pad == -(-n // 64) * 64 and x.dtype == torch.float32
    assert bool(torch.isfinite(x).all())
    if bf16:
        assert torch.equal(x, x.to(torch.bfloat16).float())
    else:
        assert torch.equal(x[:, :n], tc.tier_vision(2, n))
    assert torch.equal(x[:, n:], x[:, n:n + 1].expand(-1, n_pad - n, -1))            # copies of ONE key per frame
    _, c = evaluate(tc.small_sd(), x, False)
    for l in CROSS:
        s = c["scores"][l]
        live_max = s[..., :n].max(-1).values
        margin = float((live_max[..., None] - s[..., n:]).min())
        assert margin >= tc.DEAD_MARGIN, (l, margin)


@pytest.mark.parametrize("n", tc.HOT_SIZES)
def test_hot_keys_are_hot_and_the_reference_holds_in_fp32(n):
    x = tc.hot_frames(n)
    pos = tc.hot_positions(n)
    assert x.size(0) == len(pos) and pos[-1] == n - 1 and pos[0] == 0
    assert bool(torch.isfinite(x).all())
    out, c = evaluate(tc.small_sd(), x, False)
    for l in CROSS:
        s = c["scores"][l].clone()
        for f, p in enumerate(pos):
            hot = s[f, :, :, p].clone()
            s[f, :, :, p] = -float("inf")
            margin = float((hot - s[f].max(-1).values).min())
            assert margin >= tc.HOT_MARGIN, (l, p, margin)
    out32 = tc.ref64(tc.small_sd(), SMALL, x, False, dtype=torch.float32)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(out32).all())
    assert float((out32.double() - out).abs().max()) <= tc.ATOL / 10


@pytest.mark.parametrize("n", tc.HOT_SHORT_SIZES)
def test_short_attention_hot_key_is_hot_and_the_reference_holds_in_fp32(n):
    worst = 0.0
    for p in tc.hot_positions(n):
        s = tc.short_scores(n, p)
        hot = s[:, :, p].clone()
        s[:, :, p] = -float("inf")
        margin = float((hot - s.max(-1).values).min())
        assert margin >= tc.HOT_MARGIN, (p, margin)
        ref = tc.short_reference(n, p)
        worst = max(worst, float((tc.short_reference(n, p, torch.float32).double() - ref).abs().max()))
        assert float(ref.abs().max()) < 16.0                                        # the output stays at the scale ATOL is meant for
    assert worst <= tc.ATOL / 10


@pytest.mark.parametrize("n", tc.PEAK_SIZES)
@pytest.mark.parametrize("gain", tc.PEAK_GAINS)
def test_peaked_models_are_peaked_and_the_reference_holds_in_fp32(gain, n):
    x = tc.tier_vision(3, n)
    out, c = evaluate(tc.peaked_sd(gain), x, True)
    span = min(float((c["scores"][l].max(-1).values - c["scores"][l].min(-1).values).min()) for l in CROSS)
    assert span >= tc.PEAK_SPANS[gain], span
    out32, c32 = evaluate(tc.peaked_sd(gain), x, True, torch.float32)
    worst = max([float((out32.double() - out).abs().max())] + [float((c32["ctx"][l].double() - c["ctx"][l]).abs().max()) for l in CROSS])
    assert worst <= tc.ATOL / 10


def test_the_cases_cover_every_tier_and_seam():
    """The sizes name the kernels: padded rows up to 2048 / up to 8192 / beyond, whole rows likewise, and the hot key visits the
    wave boundary, the register-group boundaries and the last live column."""
    pad = lambda n: -(-n // 64) * 64
    tiers = lambda sizes: {0 if pad(n) <= 2048 else 1 if pad(n) <= 8192 else 2 for n in sizes}
    assert all(n % 64 for n in tc.TIER_PADDED) and tiers(tc.TIER_PADDED) == {0, 1, 2}
    assert any(1024 < n <= 2048 for n in tc.TIER_PADDED)                            # the second register group of <2>
    assert all(n % 64 == 0 for n in tc.TIER_WHOLE) and tiers(tc.TIER_WHOLE) == {0, 1, 2}
    assert all(n_pad == pad(n) and n % 64 for n, n_pad in tc.PAD_PAIRS) and tiers(n for n, _ in tc.PAD_PAIRS) == {0, 1, 2}
    assert tiers(tc.HOT_SIZES) == {0, 1, 2} and tiers(tc.HOT_SHORT_SIZES) == {0, 1, 2}
    assert {255, 256, 1023, 1024, 8192} <= set(tc.hot_positions(8193))
    assert tiers(tc.HANDLE_WALK) == {0, 1, 2}
