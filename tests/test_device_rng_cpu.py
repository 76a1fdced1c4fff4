"""The device rng of the Gibbs uniforms without a GPU: the numpy mirror (infinite_video_amd.philox) against the Random123
known answers of Philox4x32-10, the stream definition of include/infv_ltm.h pinned by two values, the C implementation
(csrc/philox.h through infv_ltm_rng_fill_host, computed on the CPU) against the mirror, and the new symbols.  Every
comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infv_ltm_set_rng", "infv_ltm_get_rng_position", "infv_ltm_set_rng_position", "infv_ltm_rng_fill",
               "infv_ltm_rng_fill_host")
SEED = 0x9E3779B97F4A7C15                # a 64-bit seed with a non-zero high word
STREAM = 0xFFFFFFFE
FILL_SHAPES = [(512, 2, 0, 3), (1, 1, 7, 2), (1023, 3, 2 ** 32 - 2, 1)]      # (S, L, pos0, n_steps)


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    from infinite_video_amd import philox
    out = philox.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert out.dtype == np.uint32 and out.shape == (4,)
    assert _hex(out) == want


def test_philox_is_vectorised():
    from infinite_video_amd import philox
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], np.uint64)
    key = np.array([[0, 0], [0xFFFFFFFF] * 2], np.uint64)
    out = philox.philox4x32_10(ctr, key)
    assert _hex(out[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(out[1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_u53_stays_below_one():
    from infinite_video_amd import philox
    top = float(philox.u53(0xFFFFFFFF, 0xFFFFFFFF))
    assert top < 1.0 and top == 1.0 - 2.0 ** -53
    assert float(philox.u53(0, 0)) == 0.0


def test_first_uniforms_of_the_zero_stream():
    from infinite_video_amd import philox
    u = philox.gibbs_uniforms(0, 0, 0, 1, 1, 2)
    assert u.shape == (1, 1, 2) and u.dtype == np.float64
    assert u[0, 0, 0] == 0.39904647231489565
    assert u[0, 0, 1] == 0.7357127860596914


def test_stream_definition():
    """ctr = (s >> 1, layer, pos, stream_id), key = (seed lo, seed hi); slots (2p, 2p + 1) share one block; odd S drops the last
    block's second value; pos wraps at 2^32."""
    from infinite_video_amd import philox
    u = philox.gibbs_uniforms(SEED, STREAM, 2 ** 32 - 1, 2, 3, 5)
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], np.uint64)
    for i, pos in enumerate((2 ** 32 - 1, 0)):
        for l in range(3):
            for s in range(5):
                w = philox.philox4x32_10(np.array([s >> 1, l, pos, STREAM], np.uint64), key)
                want = philox.u53(w[2], w[3]) if s & 1 else philox.u53(w[0], w[1])
                assert u[i, l, s] == float(want)


@pytest.mark.parametrize("S,L,pos0,n_steps", FILL_SHAPES)
def test_rng_fill_host_equals_the_mirror(S, L, pos0, n_steps):
    from infinite_video_amd import _lib, philox
    lib = _lib.load()
    out = np.full((n_steps, L, S), -1.0, np.float64)
    rc = lib.infv_ltm_rng_fill_host(SEED, STREAM, pos0, n_steps, L, S, ctypes.c_void_p(out.ctypes.data))
    assert rc == 0, lib.infv_ltm_last_error()
    want = philox.gibbs_uniforms(SEED, STREAM, pos0, n_steps, L, S)
    assert want.shape == out.shape
    np.testing.assert_array_equal(out, want)
    assert (out >= 0).all() and (out < 1).all()


def test_new_symbols_are_declared_and_exported():
    from infinite_video_amd import _lib
    header = open(os.path.join(ROOT, "include", "infv_ltm.h")).read()
    assert _lib.ABI_VERSION == 6
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"^int\s+{name}\s*\(", header, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int
    assert "long_term_attention_gibbs.py:204-206" in header


def test_refusals_without_a_device():
    from infinite_video_amd import _lib
    lib = _lib.load()
    assert lib.infv_ltm_set_rng(None, 1, 1, 0) == -1
    assert b"null" in lib.infv_ltm_last_error()
    pos = ctypes.c_uint32(5)
    assert lib.infv_ltm_get_rng_position(None, ctypes.byref(pos)) == -1
    assert lib.infv_ltm_set_rng_position(None, 3) == -1
    buf = np.zeros(4, np.float64)
    assert lib.infv_ltm_rng_fill_host(0, 0, 0, 1, 0, 4, ctypes.c_void_p(buf.ctypes.data)) == -1
    assert lib.infv_ltm_rng_fill_host(0, 0, 0, 1, 1, 4, None) == -1
    assert lib.infv_ltm_rng_fill_host(0, 0, 0, 0, 1, 4, None) == 0           # nothing to write
    assert lib.infv_ltm_rng_fill(0, 0, 0, -1, 1, 4, None, None) == -1


def test_mirror_refuses_values_that_do_not_fit():
    from infinite_video_amd import philox
    with pytest.raises(ValueError):
        philox.gibbs_uniforms(1 << 64, 0, 0, 1, 1, 2)
    with pytest.raises(ValueError):
        philox.gibbs_uniforms(0, 1 << 32, 0, 1, 1, 2)
