"""Several videos in one call (infv_ltm_consolidate_videos): the symbol, its declaration and the Python argument checks that
run before any device work.  No GPU needed."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")


def test_library_exports_consolidate_videos_and_abi_6():
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6
    assert "infv_ltm_consolidate_videos" in _lib._SIGNATURES
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6
    fn = lib.infv_ltm_consolidate_videos
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    raw = ctypes.CDLL(LIB)
    assert hasattr(raw, "infv_ltm_consolidate_videos")


def test_consolidate_videos_refusals_before_device_work():
    """V = 0, a duplicate handle and a cu that decreases are refused by the C entry point without touching a device."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    cu = (ctypes.c_int32 * 3)(0, 2, 1)
    hs = (ctypes.c_void_p * 2)(ctypes.c_void_p(1).value, ctypes.c_void_p(1).value)
    assert lib.infv_ltm_consolidate_videos(None, 0, cu, None, 8, None, 32, None, None, 1, None, None) == -1      # no handle array
    assert lib.infv_ltm_consolidate_videos(ctypes.cast(hs, ctypes.c_void_p), 0, cu, None, 8, None, 32, None, None, 1, None,
                                           None) == 0                                                           # no video
    assert lib.infv_ltm_consolidate_videos(ctypes.cast(hs, ctypes.c_void_p), 2, cu, None, 8, None, 32, None, None, 1, None,
                                           None) == -1
    assert "non-decreasing" in lib.infv_ltm_last_error().decode()


def _fake_engine(**over):
    """An LTMEngine that never touched a device: only the attributes the argument checks read."""
    import torch
    from infinite_video_amd.engine import LTMEngine
    e = LTMEngine.__new__(LTMEngine)
    cfg = dict(N=64, Np=64, H=12, dh=64, d=768, P=32, L=2, S=512, sticky=True, tau=0.75, gaussian_sigmas=None,
               device=torch.device("cuda", 0), dm=768, max_q=32, _h=None)
    cfg.update(over)
    for k, v in cfg.items():
        setattr(e, k, v)
    return e


def test_consolidate_videos_python_argument_checks():
    import torch
    from infinite_video_amd.engine import consolidate_videos
    a, b = _fake_engine(), _fake_engine()
    k = torch.zeros(3, 8 * 32, 768)
    q = torch.zeros(2, 32, 768)
    with pytest.raises(ValueError, match="entries"):
        consolidate_videos([a, b], k, [3], q, [])
    with pytest.raises(ValueError, match="non-negative"):
        consolidate_videos([a, b], k, [4, -1], q, [])
    with pytest.raises(ValueError, match="1-D"):
        consolidate_videos([a, b], k, torch.tensor([[1, 2]]), q, [])
    with pytest.raises(ValueError, match="twice"):
        consolidate_videos([a, a], k, [1, 2], q, [])
    with pytest.raises(ValueError, match="configured differently"):
        consolidate_videos([a, _fake_engine(N=128, Np=128)], k, [1, 2], q, [])
    with pytest.raises(ValueError, match="configured differently"):
        consolidate_videos([a, _fake_engine(sticky=False)], k, [1, 2], q, [])
    with pytest.raises(ValueError, match="at least one"):
        consolidate_videos([], k, [], q, [])
