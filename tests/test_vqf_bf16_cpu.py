"""bf16 frame tokens through the video Q-former (infv_vqf_set_token_dtype): declaration, export and ctypes entry, refusals
that need no device, and what the shipped gfx950 code object holds for the new path -- the two-product 384 x 256 contraction
and the bf16 token pass, without scratch, the wide kernel within the 256 registers its two waves per SIMD allow.
No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_symbol_declaration_and_abi():
    from infinite_video_amd import _lib
    assert _lib.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "infv_vqf.h")).read()
    assert re.search(r"^int infv_vqf_set_token_dtype\(infv_vqf_handle h, int32_t dtype\);", header, re.M)
    # the four entry points take the tokens as untyped memory; argument counts are those of the fp32-only ABI
    for name, n_args in (("infv_vqf_short_attention", 9), ("infv_vqf_encode_chunk", 10), ("infv_vqf_encode_video", 12),
                         ("infv_vqf_encode_videos", 13)):
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert "const void* frames" in decl and "const float* frames" not in decl, name
        assert len(decl.split(",")) == n_args, name
        assert len(_lib._SIGNATURES[name][1]) == n_args, name
    assert "infv_vqf_set_token_dtype" in _lib._SIGNATURES and "infv_vqf_set_token_dtype" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6
    assert lib.infv_vqf_set_token_dtype.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert hasattr(ctypes.CDLL(LIB), "infv_vqf_set_token_dtype")


def test_refusals_before_device_work():
    """A null handle is refused; with a dummy handle the argument checks of the bf16-capable entry points still come before
    anything is dereferenced (the pattern of test_multi_video_qformer_cpu.py)."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    assert lib.infv_vqf_set_token_dtype(None, 1) == -1
    assert b"null" in lib.infv_ltm_last_error()
    assert lib.infv_vqf_set_token_dtype(None, 7) == -1
    fake = ctypes.c_void_p(64)
    w = _lib.VqfWeights()
    cu_ok = (ctypes.c_int32 * 3)(0, 1, 2)
    cu = ctypes.cast(cu_ok, ctypes.c_void_p)
    assert lib.infv_vqf_encode_videos(None, None, 2, cu, None, 8, ctypes.byref(w), None, 1, None, None, None, None) == -1
    assert lib.infv_vqf_encode_videos(fake, None, 2, None, None, 8, ctypes.byref(w), None, 1, None, None, None, None) == -1
    assert lib.infv_vqf_encode_videos(fake, None, 0, cu, None, 8, ctypes.byref(w), None, 1, None, None, None, None) == 0
    assert lib.infv_vqf_encode_video(fake, None, None, 2, 8, ctypes.byref(w), None, 1, None, None, None, None) == -1
    assert lib.infv_vqf_encode_video(fake, None, ctypes.c_void_p(2), 0, 8, ctypes.byref(w), None, 1, None, None, None, None) == -1
    assert lib.infv_vqf_encode_chunk(fake, None, None, 8, ctypes.byref(w), None, 1, None, None, None) == -1
    assert lib.infv_vqf_encode_chunk(fake, None, ctypes.c_void_p(2), 8, None, None, 1, None, None, None) == -1
    assert lib.infv_vqf_short_attention(fake, None, 256, None, None, None, None, None, None) == -1


def _kernel_notes(tmp_path):
    """name -> metadata (ints) of every kernel in the shipped library's gfx950 code objects (llvm-readelf --notes)."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm LLVM binutils not found")
    d = tmp_path / "notes"
    d.mkdir()
    shutil.copy(LIB, d / "libinfv_ltm.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "libinfv_ltm.so"], cwd=d, capture_output=True, check=True)
    out = {}
    for f in sorted(os.listdir(d)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f], cwd=d, capture_output=True, text=True, check=True).stdout
        cur = {}
        # a kernel's keys come in alphabetical order (.agpr_count ... .wavefront_size): a record ends at .wavefront_size
        for line in notes.split("\n"):
            m = re.search(r"\.(name|vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                          r"wavefront_size):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "wavefront_size":
                if "name" in cur:
                    name = cur.pop("name")
                    out[name] = {k: int(v) for k, v in cur.items()}
                cur = {}
            else:
                cur[m.group(1)] = m.group(2)
    return out


def test_shipped_code_object_holds_the_bf16_token_kernels(tmp_path):
    notes = _kernel_notes(tmp_path)

    def one(frag):
        hits = [n for n in notes if frag in n]
        assert len(hits) == 1, (frag, hits)
        return notes[hits[0]]

    # split_gemm_wide_kernel<PROBE = 0, NPROD>: one instantiation per product count, no timing probes in the shipped build
    assert len([n for n in notes if "split_gemm_wide_kernel" in n]) == 2
    wide3, wide2 = one("split_gemm_wide_kernelILi0ELi3EE"), one("split_gemm_wide_kernelILi0ELi2EE")
    assert len([n for n in notes if "split_gemm_kernel" in n]) == 2
    narrow2 = one("split_gemm_kernelILi2EE")
    one("split_gemm_kernelILi3EE")
    token_pass = one("transpose_bf16_kernel")
    upcast = one("upcast_bf16_kernel")
    for name, k in (("wide2", wide2), ("narrow2", narrow2), ("token pass", token_pass), ("upcast", upcast), ("wide3", wide3)):
        assert k["private_segment_fixed_size"] == 0, name                      # no scratch
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, name
    # two waves per SIMD (amdgpu_waves_per_eu(2, 2)): 512 registers per SIMD lane, 256 per wave, accumulators included
    assert wide2["vgpr_count"] <= 256                                          # (.vgpr_count is the unified total on gfx950)
    assert wide2["vgpr_count"] <= wide3["vgpr_count"]                          # (one B plane less to hold)
