"""Several videos from frame means, with a query per chunk (infv_ltm_steps_videos / engine.steps_videos): the symbol, its
declaration, the C refusals and the Python argument checks that run before any device work.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")


def test_library_exports_steps_videos_in_abi_6():
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6
    assert "infv_ltm_steps_videos" in _lib._SIGNATURES
    header = open(os.path.join(ROOT, "include", "infv_ltm.h")).read()
    assert re.search(r"^int infv_ltm_steps_videos\(", header, re.M)
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6
    fn = lib.infv_ltm_steps_videos
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert hasattr(ctypes.CDLL(LIB), "infv_ltm_steps_videos")


def _call(lib, hs, V, cu, kbar=None, q_per_chunk=0, q=None, proj=None, ctx=None):
    return lib.infv_ltm_steps_videos(hs, V, cu, kbar, 8, q, q_per_chunk, 32, proj, None, 1, ctx, None)


def test_steps_videos_refusals_before_device_work():
    """Refused without reading a handle or touching a device: no handle array, a bad q_per_chunk, a decreasing cu, a null or
    repeated handle, null arrays.  V = 0 is a no-op."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64).value                      # never dereferenced by the checks below
    hs = (ctypes.c_void_p * 2)(fake, fake)
    hs_p = ctypes.cast(hs, ctypes.c_void_p)
    cu_ok = (ctypes.c_int32 * 3)(0, 1, 2)
    assert _call(lib, None, 0, cu_ok) == -1
    assert _call(lib, hs_p, 0, cu_ok) == 0
    assert _call(lib, hs_p, 0, None) == -1
    assert _call(lib, hs_p, 2, cu_ok, q_per_chunk=2) == -1
    assert "q_per_chunk" in lib.infv_ltm_last_error().decode()
    assert _call(lib, hs_p, 2, (ctypes.c_int32 * 3)(0, 2, 1)) == -1
    assert "non-decreasing" in lib.infv_ltm_last_error().decode()
    assert _call(lib, hs_p, 2, (ctypes.c_int32 * 3)(-1, 0, 1)) == -1
    assert _call(lib, hs_p, 2, cu_ok) == -1
    assert "also handle" in lib.infv_ltm_last_error().decode()
    hs_null = (ctypes.c_void_p * 2)(fake, None)
    assert _call(lib, ctypes.cast(hs_null, ctypes.c_void_p), 2, cu_ok) == -1
    assert "null" in lib.infv_ltm_last_error().decode()
    hs2 = (ctypes.c_void_p * 2)(fake, ctypes.c_void_p(128).value)
    buf = (ctypes.c_float * 4)()
    assert _call(lib, ctypes.cast(hs2, ctypes.c_void_p), 2, cu_ok, kbar=None, q=ctypes.addressof(buf), proj=None) == -1
    assert "null argument" in lib.infv_ltm_last_error().decode()
    # consolidate_videos shares the checks: a repeated handle is refused before it is read
    assert lib.infv_ltm_consolidate_videos(hs_p, 2, cu_ok, None, 8, None, 32, None, None, 1, None, None) == -1
    assert "also handle" in lib.infv_ltm_last_error().decode()


def _fake_engine(**over):
    """An LTMEngine that never touched a device: only the attributes the argument checks read (host tensors)."""
    import torch
    from infinite_video_amd.engine import LTMEngine
    e = LTMEngine.__new__(LTMEngine)
    cfg = dict(N=64, Np=64, H=12, dh=64, d=768, P=32, L=2, S=512, sticky=True, tau=0.75, gaussian_sigmas=None,
               device=torch.device("cpu"), dm=768, max_q=32, _h=None)
    cfg.update(over)
    for k, v in cfg.items():
        setattr(e, k, v)
    return e


def test_steps_videos_python_argument_checks():
    import torch
    from infinite_video_amd.engine import steps_videos
    a, b = _fake_engine(), _fake_engine()
    kbar = torch.zeros(3, 8, 768)
    q = torch.zeros(2, 32, 768)
    with pytest.raises(ValueError, match="at least one"):
        steps_videos([], kbar, [], q, [])
    with pytest.raises(ValueError, match="entries"):
        steps_videos([a, b], kbar, [3], q, [])
    with pytest.raises(ValueError, match="non-negative"):
        steps_videos([a, b], kbar, [4, -1], q, [])
    with pytest.raises(ValueError, match="1-D"):
        steps_videos([a, b], kbar, torch.tensor([[1, 2]]), q, [])
    with pytest.raises(ValueError, match="twice"):
        steps_videos([a, a], kbar, [1, 2], q, [])
    with pytest.raises(ValueError, match="configured differently"):
        steps_videos([a, _fake_engine(N=128, Np=128)], kbar, [1, 2], q, [])
    with pytest.raises(TypeError):
        steps_videos([a, b], kbar.double(), [1, 2], q, [])
    with pytest.raises(ValueError, match="kbar must be"):
        steps_videos([a, b], kbar, [1, 1], q, [])                              # 3 rows for 2 chunks
    with pytest.raises(ValueError, match="kbar must be"):
        steps_videos([a, b], torch.zeros(3, 8, 512), [1, 2], q, [])
    with pytest.raises(ValueError, match="kbar must be"):
        steps_videos([a, b], torch.zeros(3, 8 * 768), [1, 2], q, [])
    with pytest.raises(ValueError, match="q must be"):
        steps_videos([a, b], kbar, [1, 2], torch.zeros(2, 2, 32, 768), [])     # per-chunk q for 2 of 3 chunks
    with pytest.raises(ValueError, match="q must be"):
        steps_videos([a, b], kbar, [1, 2], torch.zeros(3, 1, 32, 768), [])     # one layer of two
    with pytest.raises(ValueError, match="q must be"):
        steps_videos([a, b], kbar, [1, 2], torch.zeros(3, 2, 33, 768), [])     # Q above max_q
    with pytest.raises(ValueError, match="q must be"):
        steps_videos([a, b], kbar, [1, 2], torch.zeros(2, 32, 512), [])
    with pytest.raises(ValueError, match="u must be"):
        steps_videos([a, b], kbar, [1, 2], q, [], u=torch.zeros(2, 2, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="16-byte"):
        steps_videos([a, b], torch.zeros(3 * 8 * 768 + 1)[1:].view(3, 8, 768), [1, 2], q, [])
    with pytest.raises(ValueError, match="at least one"):                     # lists are packed after the engine checks
        steps_videos([], [kbar[:1]], None, q, [], u=[])
