"""Host side of the one-launch hand-over payload: engines without ``pack_memory`` keep the torch assembly, the header, the ctypes
table and the payload layout agree."""
import os
import re

import numpy as np
import torch

from infinite_video_amd import _lib
from infinite_video_amd.video_memory import pack_local_memory, unpack_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, N, D, Q, DM, H = 2, 16, 32, 3, 64, 1


class _PlainEngine:
    """The surface pack_local_memory needs from an engine that has no pack_memory (bench.py's stand-in, the CPU oracles)."""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.L = L
        self.B = [torch.randn(N, D, generator=g) for _ in range(L)]
        self.mass = [torch.rand(127, generator=g) for _ in range(L)]
        self.scores = torch.randn(L, H, Q, N, generator=g)

    def export_state(self, l):
        return self.B[l], self.mass[l]

    def last_scores_device(self, q):
        return self.scores


def test_engines_without_pack_memory_keep_the_torch_assembly():
    eng = _PlainEngine()
    ctx = torch.randn(5, L, Q, DM, generator=torch.Generator().manual_seed(4))
    for with_scores in (False, True):
        want = torch.cat([b.reshape(-1) for b in eng.B] + eng.mass + ([eng.scores.reshape(-1)] if with_scores else []) +
                         [ctx.sum(0).reshape(-1), torch.tensor([5.0])])
        got = pack_local_memory(eng, ctx, with_scores)
        assert torch.equal(got, want)
        mem = unpack_memory(got, 1, L, N, D, Q, DM, H if with_scores else 0)
        assert torch.equal(mem.ctx_sum[0], ctx.sum(0)) and float(mem.count[0]) == 5.0


def test_an_engine_with_pack_memory_is_asked_for_the_payload():
    class Packing(_PlainEngine):
        def pack_memory(self, ctx, with_scores=False):
            self.asked = (ctx, with_scores)
            return torch.zeros(1)
    eng = Packing()
    ctx = torch.zeros(2, L, Q, DM)
    assert pack_local_memory(eng, ctx, True).numel() == 1 and eng.asked[0] is ctx and eng.asked[1] is True


def test_header_binding_and_abi_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "infv_ltm.h")).read()
    m = re.search(r"#define INFV_LTM_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == _lib.ABI_VERSION == _lib.load().infv_ltm_abi_version()
    for name in ("infv_ltm_set_ctx_sum", "infv_ltm_pack_memory"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    # argument validation needs no device
    assert _lib.load().infv_ltm_pack_memory(None, 1, 1, None, 0, 0, None, None) == -1
    assert _lib.load().infv_ltm_set_ctx_sum(None, 1) == -1


def test_payload_size_of_the_binding_matches_unpack_memory():
    """LTMEngine.payload_numel is what pack_memory allocates; unpack_memory must accept exactly that many floats and cut it where
    the kernel's segments start (B | masses | scores | ctx_sum | count)."""
    from infinite_video_amd.engine import LTMEngine
    eng = LTMEngine.__new__(LTMEngine)                         # no device: only the shape attributes the size depends on
    eng.L, eng.N, eng.d, eng.H, eng.dm = 2, 48, 768, 12, 768
    for q, with_scores in ((32, False), (32, True), (5, True)):
        n = eng.payload_numel(q, with_scores)
        payload = torch.arange(n, dtype=torch.float32)
        mem = unpack_memory(payload, 1, eng.L, eng.N, eng.d, q, eng.dm, eng.H if with_scores else 0)
        nB, nM = eng.L * eng.N * eng.d, eng.L * 127
        nS = eng.L * eng.H * q * eng.N if with_scores else 0
        assert float(mem.B.reshape(-1)[0]) == 0.0 and float(mem.bin_mass.reshape(-1)[0]) == float(nB)
        if with_scores:
            assert float(mem.scores.reshape(-1)[0]) == float(nB + nM)
        assert float(mem.ctx_sum.reshape(-1)[0]) == float(nB + nM + nS) and float(mem.count[0]) == float(n - 1)
        assert mem.ctx_sum.shape == (1, eng.L, q, eng.dm)
    eng._h = None                                              # (__del__ finds no handle)
