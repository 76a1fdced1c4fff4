"""The attention read-outs of the batched calls without a GPU: the two new symbols (``infv_ltm_set_videos_mass_trace``,
``infv_ltm_source_weights_videos``) are exported and bound, the ABI is still 6, the new call declares no ``void* stream`` (its
stream is a field of the descriptor, so tests/golden/stream_cases.py stays complete as it is), the ctypes descriptor has the
layout the header states, and the numpy ``*_videos`` mirrors equal a loop over the single-video mirrors on ragged counts.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from infinite_video_amd import _lib, density
from infinite_video_amd.basis_maps import NB_BINS, build_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.75


def header_text():
    with open(os.path.join(ROOT, "include", "infv_ltm.h")) as f:
        return f.read()


def test_symbols_are_exported_and_bound_and_the_abi_is_6():
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6 == _lib.ABI_VERSION
    assert "#define INFV_LTM_ABI_VERSION 6" in header_text()
    for name in ("infv_ltm_set_videos_mass_trace", "infv_ltm_source_weights_videos"):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
        assert f"int {name}(" in header_text()
    assert lib.infv_ltm_set_videos_mass_trace.argtypes == [C.c_void_p, C.c_void_p, C.c_int64]
    assert len(lib.infv_ltm_source_weights_videos.argtypes) == 2
    # both refuse a null handle on the host, before anything else
    assert lib.infv_ltm_set_videos_mass_trace(None, None, 0) == -1
    assert lib.infv_ltm_source_weights_videos(None, None) == -1


def test_the_new_calls_declare_no_stream_parameter_and_the_stream_table_stays_complete():
    from tests import test_stream_order_cpu as so
    names = so.stream_entry_points()
    assert "infv_ltm_source_weights" in names                         # (the parser does find the single-video call)
    assert "infv_ltm_source_weights_videos" not in names and "infv_ltm_set_videos_mass_trace" not in names
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    m = re.search(r"\bint\s+infv_ltm_source_weights_videos\s*\(([^;{}]*?)\)\s*;", text, re.S)
    assert m and "stream" not in m.group(1)
    assert re.search(r"void\s*\*\s*hip_stream\s*;", text)             # the field that carries it
    so.test_every_stream_entry_point_has_a_case_or_a_stated_exclusion()
    # the header says why, so nobody moves the stream back into the parameter list
    assert "FIELD of the descriptor" in header_text() and "tests/golden/stream_cases.py" in header_text()


# offset of every field of infv_ltm_sources_videos_desc, written from the header: four int32, one int64, seven pointers
DESC_LAYOUT = (("n_videos", 0, 4), ("T", 4, 4), ("frames_per_source", 8, 4), ("reserved", 12, 4), ("ld", 16, 8), ("cu", 24, 8),
               ("bins_all", 32, 8), ("W_all", 40, 8), ("mass_all", 48, 8), ("attn_all", 56, 8), ("bad_bins", 64, 8),
               ("hip_stream", 72, 8))


def test_descriptor_layout_matches_the_header():
    assert C.sizeof(_lib.SourcesVideosDesc) == 80
    assert [f[0] for f in _lib.SourcesVideosDesc._fields_] == [n for n, _, _ in DESC_LAYOUT]
    for name, offset, size in DESC_LAYOUT:
        field = getattr(_lib.SourcesVideosDesc, name)
        assert (field.offset, field.size) == (offset, size), name
    # the header declares the same fields in the same order
    body = re.search(r"typedef struct \{([^}]*)\} infv_ltm_sources_videos_desc;", header_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    declared = [re.split(r"[\s\*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
    assert declared == [n for n, _, _ in DESC_LAYOUT]


def test_numpy_mirrors_equal_the_per_video_loop():
    """Ragged counts with a zero-length video in the middle, sticky and not, g = 1 and g = T, both dtypes."""
    T, N, counts = 8, 16, [3, 1, 0, 4, 2]
    plan = build_plan(T, N, TAU)
    rng = np.random.default_rng(3)
    total = sum(counts)
    cu = np.concatenate([[0], np.cumsum(counts)])
    bins = rng.integers(0, NB_BINS - 1, size=(total, plan.S)).astype(np.int32)
    mass = rng.random((total, N))
    for sticky in (True, False):
        for g in (1, T):
            for dtype in (np.float64, np.float32):
                b = bins if sticky else None
                per = T // g
                W = density.source_weights_videos(plan, b, counts, frames_per_source=g, dtype=dtype)
                W2, attn = density.source_attention_videos(mass, plan, b, counts, frames_per_source=g, dtype=dtype)
                assert W.shape == (len(counts), N, max(counts) * per) and W.dtype == dtype
                assert attn.shape == (total, max(counts) * per) and attn.dtype == np.float64
                assert np.array_equal(W, W2)
                for v, n in enumerate(counts):
                    if n == 0:
                        assert not W[v].any()
                        continue
                    bv = None if b is None else b[cu[v]:cu[v + 1]]
                    one = density.source_weights(plan, bv, n, frames_per_source=g, dtype=dtype)
                    assert np.array_equal(W[v, :, :n * per], one) and not W[v, :, n * per:].any()
                    _, a = density.source_attention(mass[cu[v]:cu[v + 1]], plan, bv, n, frames_per_source=g, dtype=dtype)
                    assert np.array_equal(attn[cu[v]:cu[v + 1], :n * per], a) and not attn[cu[v]:cu[v + 1], n * per:].any()
    # a video alone equals the same video inside the batch
    alone = density.source_weights_videos(plan, bins[cu[3]:cu[4]], [counts[3]], frames_per_source=1)
    assert np.array_equal(alone[0], density.source_weights_videos(plan, bins, counts, frames_per_source=1)[3])
    _, norm = density.source_attention_videos(mass, plan, bins, counts, frames_per_source=1, normalise=True)
    np.testing.assert_allclose(norm.sum(-1), 1.0, rtol=0, atol=1e-12)
