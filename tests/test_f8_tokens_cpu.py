"""fp8 e4m3 frame tokens (INFV_TOKENS_F8E4M3 = 4, ``torch.float8_e4m3fn``), the part that needs no GPU: the declaration beside the
enum, the second Python dtype table, the refusal of the other fp8 encodings, refusals before any device work, the exactness of
every finite code in bf16, and the kernels of the shipped code object."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_vqf_bf16_cpu import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn
INVALID, UNSUPPORTED = -1, -2

# the fp8 kernels by (a fragment of) their mangled name, and how many instantiations of each ship
NEW_KERNELS = {"pool_frames_f8_kernel": 2,           # padded 512-thread, plain 256-thread
               "pool_rows2_f8_kernel": 4,            # {8, 4 loads per burst} x {rows only, rows + bf16 planes}
               "pool_videos_f8_kernel": 1,
               "split_transpose_f8_kernel": 1,
               "upcast_f8_kernel": 1}
# name fragments the earlier tests count: no fp8 kernel may contain one
PINNED = ("pool_frames_kernel", "pool_rows2_kernel", "pool_frames_f16_kernel", "pool_rows2_f16_kernel", "split_gemm_wide_kernel",
          "split_gemm_kernel", "transpose_bf16_kernel", "upcast_bf16_kernel", "split_transpose_f16_kernel", "upcast_f16_kernel",
          "pool_videos_kernelINS_6TokF16E")


def test_header_declares_the_code_beside_the_enum():
    header = open(os.path.join(ROOT, "include", "infv_ltm.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\} infv_token_dtype;", header).group(1)
    codes = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in enum.split(",")))
    assert codes == {"INFV_TOKENS_F32": 0, "INFV_TOKENS_BF16": 1, "INFV_TOKENS_F16": 3}          # the enum body is unchanged
    assert re.search(r"^#define INFV_TOKENS_F8E4M3 4\b", header, re.M)
    assert "e4m3fn" in header and "e5m2" in header and "fnuz" in header                        # which fp8 it is, and which not
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6 and _lib.load().infv_ltm_abi_version() == 6                  # additive: no new symbol, same ABI


def test_python_tables_and_the_other_fp8_encodings():
    from infinite_video_amd import engine
    from infinite_video_amd.video_qformer import ShortMemoryBuffer, _dev_tokens
    assert engine.TOKEN_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}    # unchanged
    assert engine.F8_TOKEN_DTYPES == {F8: 4}
    assert [engine.token_code(t) for t in (torch.float32, torch.bfloat16, torch.float16, F8)] == [0, 1, 3, 4]
    assert engine.token_code(torch.float64) is None and engine.token_code(torch.uint8) is None
    cpu = torch.device("cpu")
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            engine.token_code(other)
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            _dev_tokens(torch.zeros(2, 64, 16).to(other), cpu)
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            ShortMemoryBuffer(4, 8, capacity_frames=16, dtype=other)


def test_short_memory_buffer_round_trip():
    from infinite_video_amd.video_qformer import ShortMemoryBuffer
    P, d = 4, 8
    frames = (torch.arange(9 * P * d, dtype=torch.float32).reshape(9, P, d) % 16) / 8.0 - 1.0   # exact in e4m3
    buf = ShortMemoryBuffer(P, d, capacity_frames=16, dtype=F8).replace(frames)
    out = buf.frames()
    assert out.dtype == F8 and out.shape == (1, 9 * P, d) and out.element_size() == 1
    assert torch.equal(out.float().reshape(9, P, d), frames)
    rounded = ShortMemoryBuffer(P, d, capacity_frames=16, dtype=F8).replace(frames * 0.3)      # what .to(float8_e4m3fn) gives
    assert torch.equal(rounded.frames().view(torch.uint8).reshape(9, P, d), (frames * 0.3).to(F8).view(torch.uint8))


def test_dev_tokens_passes_aligned_fp8_through_and_realigns():
    from infinite_video_amd.video_qformer import _dev_tokens
    cpu = torch.device("cpu")
    x = torch.randn(2, 64, 16).to(F8)
    assert x.data_ptr() % 16 == 0
    t, code = _dev_tokens(x, cpu)
    assert code == 4 and t.dtype == F8 and t.data_ptr() == x.data_ptr()                      # passed through: no copy
    store = torch.randn(2 * 64 * 16 + 16).to(F8)
    for off in (1, 2, 4, 8):
        v = store[off:off + 2 * 64 * 16].reshape(2, 64, 16)
        assert v.data_ptr() % 16 == off
        t, code = _dev_tokens(v, cpu)
        assert code == 4 and t.dtype == F8 and t.data_ptr() % 16 == 0
        assert torch.equal(t.view(torch.uint8), v.view(torch.uint8))
    t, code = _dev_tokens(x.transpose(1, 2), cpu)
    assert code == 4 and t.is_contiguous() and t.dtype == F8 and t.data_ptr() % 16 == 0


def test_every_finite_e4m3_code_is_exact_in_bf16():
    """254 finite codes (0x7F and 0xFF are the NaNs): each widens to an fp32 value that is its own bf16 hi piece with a zero lo
    piece, so the two-product contractions see the fp32 value itself.  Largest 448, smallest non-zero 2^-9."""
    x8 = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8)
    x = x8.float()
    nan = torch.isnan(x)
    assert nan.nonzero().flatten().tolist() == [0x7F, 0xFF]
    x = x[~nan]
    assert x.numel() == 254 and torch.isfinite(x).all()
    assert torch.equal(x.to(F8).view(torch.uint8), x8.view(torch.uint8)[~nan])               # fp8 -> fp32 -> fp8 is the identity
    hi = x.bfloat16()
    assert torch.equal(hi.float(), x)                                                          # hi = the value
    assert torch.count_nonzero((x - hi.float()).bfloat16().float()) == 0                       # lo = 0
    assert float(x.abs().max()) == 448.0 and float(x[x != 0].abs().min()) == 2.0 ** -9


def test_refusals_before_device_work():
    """Through null / fake handles, as tests/test_vc_half_tokens_cpu.py does: nothing below may read the handle or touch a device."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    err = lambda: lib.infv_ltm_last_error()
    for fn in (lib.infv_ltm_set_token_dtype, lib.infv_vqf_set_token_dtype):
        assert fn(None, 4) == INVALID                # null handle, known code
        assert fn(None, 2) == INVALID
    assert lib.infv_ltm_forward_into(None, None, 4, 8, None, None, 32, None, None, None, None) == INVALID
    fake = C.c_void_p(64)
    layers = (_lib.VqfVcLayer * 1)()
    w = _lib.VqfVcWeights(1, 0, layers, _lib.Linear(None, None))
    i32 = lambda *x: (C.c_int32 * len(x))(*x)
    cu, fcu, src, tl = i32(0, 1, 2), i32(0, 1), i32(0, 0), i32(0, 0)
    p = lambda a: C.cast(a, C.c_void_p)
    base = 4096                                                    # a 16-byte aligned address that is never read

    def videos(frames, code):
        return lib.infv_vqf_vc_encode_videos_tok(fake, None, 2, p(cu), C.c_void_p(frames), code, 16, C.byref(w), None, p(tl),
                                                 None, 1, None, None, None, None)

    def streams(frames, code):
        return lib.infv_vqf_vc_encode_streams_tok(fake, None, 2, p(cu), C.c_void_p(frames), code, 1, p(fcu), p(src), 16,
                                                  C.byref(w), None, p(tl), None, 1, None, None, None, None)

    def img(frames, code, gamma):
        front = _lib.VqfVcFront(_lib.VqfVisionLn(gamma, gamma, 1e-12), _lib.VqfVcEmb(None, None, _lib.LayerNorm(None, None), 0, 0, None),
                                None, 0)
        return lib.infv_vqf_vc_encode_img(fake, None, 2, p(cu), C.c_void_p(frames), code, 0, None, None, 16, C.byref(w),
                                          C.byref(front), None, p(tl), None, 1, None, None, None, None)

    for call in (videos, streams):
        for code in (2, 7, 16, -1):
            assert call(base, code) == INVALID, (call.__name__, code)
            assert b"unknown token dtype" in err()
        for off in (1, 2, 4, 8):
            assert call(base + off, 4) == INVALID, (call.__name__, off)
            assert b"16-byte" in err()
    # the vision LayerNorm of fp8 tokens is out of scope: unsupported, decided before the handle is read
    assert img(base, 4, 0x1000) == UNSUPPORTED and b"fp8" in err()
    assert img(base, 2, 0x1000) == INVALID and b"unknown token dtype" in err()
    for off in (1, 2, 4, 8):                                       # ... and with the LayerNorm off it is the _tok call
        assert img(base + off, 4, None) == INVALID and b"16-byte" in err()
    assert lib.infv_vqf_layernorm_tokens(C.c_void_p(base), 4, 4, 64, C.c_void_p(base), C.c_void_p(base), 1e-12, C.c_void_p(base),
                                         None) == UNSUPPORTED

    def tpass(code=4, nb=1, n=64, d=64, P=4, frames=base, Fh=base, Fl=0, Th=base, Tl=0, kbar=base):
        v = lambda x: C.c_void_p(x) if x else None
        return lib.infv_vqf_token_pass(v(frames), code, nb, n, d, P, v(Fh), v(Fl), v(Th), v(Tl), v(kbar), None)

    assert tpass(Fl=base) == INVALID and b"fp8" in err()           # a lo plane with code 4
    assert tpass(Tl=base) == INVALID and tpass(Fh=0) == INVALID and tpass(Th=0) == INVALID and tpass(frames=0) == INVALID
    for off in (1, 2, 4, 8):
        assert tpass(frames=base + off) == INVALID and b"16-byte" in err()
    assert tpass(Th=base + 8) == INVALID and tpass(Fh=base + 8) == INVALID
    assert tpass(d=48) == INVALID and tpass(n=40) == INVALID and tpass(n=96, P=5) == INVALID
    for code in (2, 7):
        assert tpass(code=code) == INVALID and b"unknown token dtype" in err()
    assert tpass(n=192, P=6) == UNSUPPORTED and tpass(n=192, P=12) == UNSUPPORTED    # no one-pass form with the means


def test_shipped_code_object_holds_the_fp8_kernels(tmp_path):
    notes = _kernel_notes(tmp_path)
    for frag, count in NEW_KERNELS.items():
        hits = [n for n in notes if frag in n]
        assert len(hits) == count, (frag, hits)
        for n in hits:
            k = notes[n]
            assert not any(p in n for p in PINNED), n
            assert k["private_segment_fixed_size"] == 0, n                       # no scratch
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, n
    # each fp8 pooling form has at least the waves per SIMD of its bf16 sibling: 512 // registers (granule 8), at most 8
    def waves(k):
        return min(8, 512 // (8 * ((k["vgpr_count"] + 7) // 8)))

    def the(frag):
        hits = [n for n in notes if frag in n]
        assert len(hits) == 1, (frag, hits)
        return notes[hits[0]]

    for f8, bf16 in (("pool_frames_f8_kernelILi4ELi512EE", "pool_frames_kernelILi4ELi512ENS_7TokBF16EE"),
                     ("pool_frames_f8_kernelILi16ELi256EE", "pool_frames_kernelILi16ELi256ENS_7TokBF16EE"),
                     ("pool_rows2_f8_kernelILi4ELb0EE", "pool_rows2_kernelILi4ENS_7TokBF16ELb0EE"),
                     ("pool_rows2_f8_kernelILi8ELb0EE", "pool_rows2_kernelILi8ENS_7TokBF16ELb0EE"),
                     ("pool_rows2_f8_kernelILi4ELb1EE", "pool_rows2_kernelILi4ENS_7TokBF16ELb1EE"),
                     ("pool_rows2_f8_kernelILi8ELb1EE", "pool_rows2_kernelILi8ENS_7TokBF16ELb1EE"),
                     ("pool_videos_f8_kernel", "pool_videos_kernelINS_7TokBF16E")):
        assert waves(the(f8)) >= waves(the(bf16)), (f8, the(f8), the(bf16))
