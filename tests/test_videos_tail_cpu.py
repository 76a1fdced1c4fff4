"""The lockstep calls over videos whose last chunk is short (``infv_ltm_videos_tail``), without a GPU: the frame -> (chunk, tail)
split and the packing offsets against a plain-Python restatement of ``torch.split``, the ``ValueError``s, the entry point in the
header (no ``void* stream`` parameter: the stream is a field of the descriptor), its ctypes binding and descriptor layout, the
plan tables the call shares between chunk lengths, and the new kernels in the shipped code object."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, engine
from infinite_video_amd.basis_maps import build_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    with open(os.path.join(ROOT, "include", "infv_ltm.h")) as f:
        return f.read()


def restated_split(frames, T):
    """What ``torch.split(video, T, dim=1)`` hands the driver, video after video: the lengths of its pieces."""
    counts, tails, cu, frame0 = [], [], [0], [0]
    for f in frames:
        pieces = [int(p.shape[0]) for p in torch.split(torch.zeros(f), T)] if f else []
        counts.append(len(pieces))
        tails.append(pieces[-1] if pieces else 0)
        cu.append(cu[-1] + len(pieces))
        frame0.append(frame0[-1] + f)
    return counts, tails, cu, frame0


@pytest.mark.parametrize("T", [2, 4, 8, 16, 256])
def test_split_frames_equals_the_restatement(T):
    rng = np.random.default_rng(T)
    frames = [0, 2, T, T + 2, 2 * T, 3 * T - 1, 5 * T + T // 2 + (2 if T == 2 else 0)] + \
             [int(f) for f in rng.integers(0, 6 * T, size=40)]
    frames = [f + 1 if f % T == 1 else f for f in frames]
    counts, tails, cu, frame0 = engine.split_frames(frames, T)
    r_counts, r_tails, r_cu, r_frame0 = restated_split(frames, T)
    assert counts == r_counts and tails == r_tails
    assert cu.dtype == np.int32 and cu.tolist() == r_cu
    assert frame0.dtype == np.int64 and frame0.tolist() == r_frame0
    for v, f in enumerate(frames):                                    # the layout the header states
        assert f == (max(counts[v] - 1, 0) * T + tails[v])
        assert counts[v] == -(-f // T) and (tails[v] == 0) == (f == 0) and (f == 0 or 2 <= tails[v] <= T)
    assert engine.split_frames(torch.tensor(frames), T)[0] == counts  # a 1-D tensor is a list


def test_split_frames_refusals_name_the_video():
    with pytest.raises(ValueError, match="video 2 has 9 frames"):
        engine.split_frames([8, 6, 9], 4)
    with pytest.raises(ValueError, match="video 0 has 1 frames"):
        engine.split_frames([1], 4)
    with pytest.raises(ValueError, match=r"frame_counts\[1\] = -3"):
        engine.split_frames([4, -3], 4)
    with pytest.raises(ValueError, match="T must be at least 2"):
        engine.split_frames([4], 1)


def test_frames_wrappers_check_their_arguments_before_any_library_call():
    with pytest.raises(ValueError, match="at least one engine"):
        engine.consolidate_videos_frames([], torch.zeros(0, 2, 32), [], 4, torch.zeros(1, 4, 64), [])
    with pytest.raises(ValueError, match="video 1 has 5 frames"):
        engine.steps_videos_frames([object(), object()], torch.zeros(9, 32), [4, 5], 4, torch.zeros(1, 4, 64), [])
    with pytest.raises(ValueError, match="2 entries for 1 engines"):
        engine.consolidate_videos_frames([object()], torch.zeros(8, 2, 32), [4, 4], 4, torch.zeros(1, 4, 64), [])


def test_header_declares_the_entry_point_without_a_stream_parameter():
    from tests import test_stream_order_cpu as so
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    m = re.search(r"\bint\s+infv_ltm_videos_tail\s*\(([^;{}]*?)\)\s*;", text, re.S)
    assert m and "stream" not in m.group(1) and "infv_ltm_videos_tail_desc" in m.group(1)
    assert "infv_ltm_videos_tail" not in so.stream_entry_points()
    so.test_every_stream_entry_point_has_a_case_or_a_stated_exclusion()
    body = re.search(r"typedef struct \{([^}]*)\} infv_ltm_videos_tail_desc;", header_text(), re.S).group(1)
    assert re.search(r"void\s*\*\s*hip_stream\s*;", body)
    assert "#define INFV_LTM_ABI_VERSION 6" in header_text()          # additive


# offset and size of every field of infv_ltm_videos_tail_desc, written from the header
DESC_LAYOUT = (("hs", 0, 8), ("V", 8, 4), ("T", 12, 4), ("cu", 16, 8), ("tail_T", 24, 8), ("k", 32, 8), ("kbar", 40, 8), ("q", 48, 8),
               ("q_per_chunk", 56, 4), ("Q", 60, 4), ("proj", 64, 8), ("u", 72, 8), ("new_doc", 80, 4), ("reserved", 84, 4),
               ("ctx", 88, 8), ("hip_stream", 96, 8))


def test_binding_and_descriptor_layout():
    lib = _lib.load()
    assert "infv_ltm_videos_tail" in _lib.EXPORTED_SYMBOLS
    fn = lib.infv_ltm_videos_tail
    assert fn.restype is C.c_int and len(fn.argtypes) == 1
    assert C.sizeof(_lib.VideosTailDesc) == 104
    for name, offset, size in DESC_LAYOUT:
        field = getattr(_lib.VideosTailDesc, name)
        assert (field.offset, field.size) == (offset, size), name
    body = re.search(r"typedef struct \{([^}]*)\} infv_ltm_videos_tail_desc;", header_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    declared = [re.split(r"[\s\*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
    assert declared == [n for n, _, _ in DESC_LAYOUT] == [f[0] for f in _lib.VideosTailDesc._fields_]
    # host-side refusals that need no device and no handle
    INVALID = -1
    assert fn(None) == INVALID and b"null descriptor" in lib.infv_ltm_last_error()
    d = _lib.VideosTailDesc()
    assert fn(C.byref(d)) == INVALID and b"tail_T" in lib.infv_ltm_last_error()
    tails = (C.c_int32 * 1)(0)
    d.tail_T = C.cast(tails, C.c_void_p)
    assert fn(C.byref(d)) == INVALID and b"exactly one of k" in lib.infv_ltm_last_error()       # neither
    d.k = d.kbar = 16
    assert fn(C.byref(d)) == INVALID and b"exactly one of k" in lib.infv_ltm_last_error()       # both
    d.kbar = None
    d.reserved = 1
    assert fn(C.byref(d)) == INVALID and b"reserved" in lib.infv_ltm_last_error()
    d.reserved, d.q_per_chunk = 0, 2
    assert fn(C.byref(d)) == INVALID and b"q_per_chunk" in lib.infv_ltm_last_error()


@pytest.mark.parametrize("N,tau", [(16, 0.75), (64, 0.75), (64, 0.5), (256, 0.75)])
def test_tables_shared_between_chunk_lengths_do_not_depend_on_T(N, tau):
    """The draw, the attend and the box masses of a step run ONCE for videos of different chunk lengths: the tables they read --
    ``plan.sticky()`` (edge_box, edge_dx, bin_box), the read-out weights ``w`` / ``w_out`` and ``uniform_idx`` -- must be the same
    for every T of one (num_basis, tau, nb_samples).  (The library checks the same equality per call, by digest.)"""
    base = build_plan(16, N, tau)
    assert not base.dense
    for T in (2, 3, 4, 7, 8, 15, 255, 256):
        p = build_plan(T, N, tau)
        for name in ("edge_box", "edge_dx", "bin_box", "readout_w", "uniform_idx"):
            assert np.array_equal(getattr(p, name), getattr(base, name)), (T, name)
        assert p.readout_w_out == base.readout_w_out and p.S == base.S


def llvm_bin():
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf")):
        pytest.skip("ROCm LLVM binutils not found")
    return llvm


def test_shipped_library_holds_the_tail_kernels_without_scratch(tmp_path):
    """One table kernel, the pooling form per token type (fp8 under its own name, as the other pooling kernels), gather, projection
    and update: no scratch, no spills, and no LDS beyond the projection tile's (``project_videos_kernel``'s 18432 bytes)."""
    llvm = llvm_bin()
    lib = "libinfv_ltm.so"
    shutil.copy(os.path.join(os.path.dirname(_lib.LIB_PATH), lib), tmp_path / lib)
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=tmp_path, capture_output=True, check=True)
    kernels, cur = {}, {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
        for line in notes.split("\n"):
            m = re.search(r"\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|wavefront_size):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "wavefront_size":
                if "name" in cur:
                    kernels[cur["name"]] = cur
                cur = {}
            else:
                cur[m.group(1)] = m.group(2)
    expect = {"video_tables_kernel": 1, "pool_videos_tail_kernel": 3, "pool_videos_tail_f8_kernel": 1, "gather_videos_tail_kernel": 1,
              "project_videos_tail_kernel": 1, "update_videos_tail_kernel": 1}
    for frag, count in expect.items():
        hits = [n for n in kernels if frag in n]
        assert len(hits) == count, (frag, hits)
        for n in hits:
            k = kernels[n]
            assert int(k.get("private_segment_fixed_size", 0)) == 0, n
            assert int(k.get("vgpr_spill_count", 0)) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, n
            lds = int(k.get("group_segment_fixed_size", 0))
            assert lds == (18432 if "project" in n else 0), (n, lds)
    twin = [kernels[n] for n in kernels if "project_videos_kernel" in n]
    assert len(twin) == 1 and int(twin[0]["group_segment_fixed_size"]) == 18432
