"""fp16 frame tokens (INFV_TOKENS_F16 = 3), the part that needs no GPU: the declaration, the Python dtype table, refusals before
any device work, the exact hi + lo split of every finite fp16 value, and the kernels of the shipped code object."""
import ctypes
import os
import re

import torch

from tests.test_vqf_bf16_cpu import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the fp16 kernels by (a fragment of) their mangled name, and how many instantiations of each ship
NEW_KERNELS = {"pool_frames_f16_kernel": 2,          # padded 512-thread, plain 256-thread
               "pool_rows2_f16_kernel": 4,           # {8, 4 loads per burst} x {rows only, rows + bf16 planes}
               "pool_videos_kernelINS_6TokF16E": 1,
               "split_transpose_f16_kernel": 1,
               "upcast_f16_kernel": 1}
# name fragments the earlier tests count: no fp16 kernel may contain one
PINNED = ("pool_frames_kernel", "pool_rows2_kernel", "split_gemm_wide_kernel", "split_gemm_kernel", "transpose_bf16_kernel",
          "upcast_bf16_kernel")


def test_header_declares_the_code():
    header = open(os.path.join(ROOT, "include", "infv_ltm.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\} infv_token_dtype;", header).group(1)
    codes = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in enum.split(",")))
    assert codes == {"INFV_TOKENS_F32": 0, "INFV_TOKENS_BF16": 1, "INFV_TOKENS_F16": 3}
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6 and _lib.load().infv_ltm_abi_version() == 6          # additive: no new symbol, same ABI


def test_python_layer_takes_float16():
    from infinite_video_amd.engine import TOKEN_DTYPES
    from infinite_video_amd.video_qformer import ShortMemoryBuffer, _dev_tokens
    assert TOKEN_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}
    P, d = 4, 8
    frames = torch.arange(9 * P * d, dtype=torch.float32).reshape(9, P, d) / 64.0          # exact in fp16
    buf = ShortMemoryBuffer(P, d, capacity_frames=16, dtype=torch.float16).replace(frames)
    assert buf.frames().dtype == torch.float16 and buf.frames().shape == (1, 9 * P, d)
    assert torch.equal(buf.frames().float().reshape(9, P, d), frames)
    cpu = torch.device("cpu")
    x = torch.randn(2, 64, 16).half()
    t, code = _dev_tokens(x, cpu)
    assert code == 3 and t.dtype == torch.float16 and t.data_ptr() == x.data_ptr()          # passed through: no copy
    off = torch.randn(2 * 64 * 16 + 8).half()[1:1 + 2 * 64 * 16].reshape(2, 64, 16)          # 2 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 != 0
    t, code = _dev_tokens(off, cpu)
    assert code == 3 and t.dtype == torch.float16 and t.data_ptr() % 16 == 0 and torch.equal(t, off)
    t, code = _dev_tokens(x.transpose(1, 2), cpu)
    assert code == 3 and t.is_contiguous() and t.dtype == torch.float16
    t, code = _dev_tokens(x.double(), cpu)
    assert code == 0 and t.dtype == torch.float32


def test_refusals_before_device_work():
    from infinite_video_amd import _lib
    lib = _lib.load()
    for fn in (lib.infv_ltm_set_token_dtype, lib.infv_vqf_set_token_dtype):
        assert fn(None, 3) == -1                     # null handle, known code
        assert lib.infv_ltm_last_error()
        assert fn(None, 2) == -1
    assert lib.infv_ltm_forward_into(None, None, 3, 8, None, None, 32, None, None, None, None) == -1


def test_every_finite_fp16_value_is_hi_plus_lo_exactly():
    """x = hi + lo with hi = bf16(x), lo = bf16(x - hi), for all 63 488 finite fp16 bit patterns (subnormals, both zeros and
    65504 among them), and a third piece would be zero: the three-product contraction sees the fp32 value itself."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x16 = bits.view(torch.float16)
    x16 = x16[torch.isfinite(x16)]
    assert x16.numel() == 63488
    x = x16.float()
    assert torch.equal(x.half(), x16)                                       # fp16 -> fp32 is exact
    hi = x.bfloat16()
    r1 = x - hi.float()
    lo = r1.bfloat16()
    assert torch.equal(hi.float() + lo.float(), x)
    assert torch.equal(hi.double() + lo.double(), x.double())
    assert torch.count_nonzero(r1 - lo.float()) == 0                        # the third piece
    assert float(x.abs().max()) == 65504.0 and float(x[x != 0].abs().min()) == 2.0 ** -24


def test_shipped_code_object_holds_the_fp16_kernels(tmp_path):
    notes = _kernel_notes(tmp_path)
    for frag, count in NEW_KERNELS.items():
        hits = [n for n in notes if frag in n]
        assert len(hits) == count, (frag, hits)
        for n in hits:
            k = notes[n]
            assert not any(p in n for p in PINNED), n
            assert k["private_segment_fixed_size"] == 0, n                       # no scratch
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, n
    # the fp16 pooling forms within the occupancy step of their bf16 siblings: waves per SIMD = 512 // registers (granule 8), at most 8
    def waves(k):
        return min(8, 512 // (8 * ((k["vgpr_count"] + 7) // 8)))

    def the(frag):
        hits = [n for n in notes if frag in n]
        assert len(hits) == 1, (frag, hits)
        return notes[hits[0]]

    for f16, bf16 in (("pool_frames_f16_kernelILi4ELi512EE", "pool_frames_kernelILi4ELi512ENS_7TokBF16EE"),
                      ("pool_frames_f16_kernelILi16ELi256EE", "pool_frames_kernelILi16ELi256ENS_7TokBF16EE"),
                      ("pool_rows2_f16_kernelILi4ELb0EE", "pool_rows2_kernelILi4ENS_7TokBF16ELb0EE"),
                      ("pool_rows2_f16_kernelILi8ELb0EE", "pool_rows2_kernelILi8ENS_7TokBF16ELb0EE"),
                      ("pool_rows2_f16_kernelILi4ELb1EE", "pool_rows2_kernelILi4ENS_7TokBF16ELb1EE"),
                      ("pool_rows2_f16_kernelILi8ELb1EE", "pool_rows2_kernelILi8ENS_7TokBF16ELb1EE"),
                      ("pool_videos_kernelINS_6TokF16E", "pool_videos_kernelINS_7TokBF16E")):
        assert waves(the(f16)) >= waves(the(bf16)), (f16, the(f16), the(bf16))
