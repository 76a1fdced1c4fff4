"""Several instructions per video over one copy of its frame tokens (infv_ltm_steps_videos_from, infv_vqf_vc_encode_streams,
VideoChat2Encoder.encode_streams, encode_long_video_prompts_vc): declarations, exported symbols, the ctypes argument lists
against the headers, the Python argument checks and the generator order of the fallback loop.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")
LTM_H, VQF_H = os.path.join(ROOT, "include", "infv_ltm.h"), os.path.join(ROOT, "include", "infv_vqf.h")
HEADERS = {"infv_ltm_steps_videos_from": LTM_H, "infv_ltm_steps_videos": LTM_H,
           "infv_vqf_vc_encode_streams": VQF_H, "infv_vqf_vc_encode_videos": VQF_H}
# the sibling each call extends, and the arguments it adds to the sibling's list (name -> position)
SIBLING = {"infv_ltm_steps_videos_from": ("infv_ltm_steps_videos", {"kbar_chunk0": 4}),
           "infv_vqf_vc_encode_streams": ("infv_vqf_vc_encode_videos", {"F": 5, "fcu": 6, "frame_src": 7})}


def _args(sym):
    """[(type, name)] of the declaration of ``sym`` in its header (comments stripped)."""
    h = re.sub(r"/\*.*?\*/", "", open(HEADERS[sym]).read(), flags=re.S)
    m = re.search(r"^int " + sym + r"\((.*?)\);", h, re.M | re.S)
    assert m, f"{sym} is not declared"
    out = []
    for a in m.group(1).split(","):
        a = re.sub(r"\s+", " ", a).strip()
        typ, name = re.match(r"(.*?)(\w+)$", a).groups()
        out.append((typ.strip().replace(" *", "*"), name))
    return out


def test_headers_declare_the_entry_points():
    for sym, (sib, added) in SIBLING.items():
        new, old = _args(sym), _args(sib)
        assert len(new) == len(old) + len(added), sym
        for name, pos in added.items():
            assert new[pos][1] == name, (sym, pos, new[pos])
        assert [a for i, a in enumerate(new) if i not in added.values()] == old, f"{sym} is {sib} plus {sorted(added)}"
    assert dict((n, t) for t, n in _args("infv_ltm_steps_videos_from"))["kbar_chunk0"] == "const int32_t*"
    types = dict((n, t) for t, n in _args("infv_vqf_vc_encode_streams"))
    assert types["F"] == "int32_t" and types["fcu"] == "const int32_t*" and types["frame_src"] == "const int32_t*"
    assert types["frames"] == "const float*"


def test_library_exports_them_and_the_abi_version_stays():
    from infinite_video_amd import _lib
    raw = ctypes.CDLL(LIB)
    for sym in SIBLING:
        assert hasattr(raw, sym), sym
        assert sym in _lib._SIGNATURES and sym in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert re.search(r"#define INFV_LTM_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "infv_ltm.h")).read())


def test_ctypes_argument_lists_match_the_declarations():
    from infinite_video_amd import _lib
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for sym, (sib, added) in SIBLING.items():
        res, args = _lib._SIGNATURES[sym]
        decl = _args(sym)
        assert res is ctypes.c_int and len(args) == len(decl), sym
        for (typ, name), ct in zip(decl, args):
            if typ in scalar:
                assert ct is scalar[typ], (sym, name, typ)
            else:                                                 # every pointer and handle travels as a pointer-sized argument
                assert typ.endswith("*") or typ.endswith("_handle"), (sym, name, typ)
                assert ctypes.sizeof(ct) == ctypes.sizeof(ctypes.c_void_p), (sym, name)
        sib_args = _lib._SIGNATURES[sib][1]
        kept = [a for i, a in enumerate(args) if i not in added.values()]
        assert kept == list(sib_args), f"{sym}: the arguments it shares with {sib} have other ctypes"


def test_c_refusals_that_need_no_device():
    from infinite_video_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    layers = (_lib.VqfVcLayer * 1)()
    w = _lib.VqfVcWeights(1, 0, layers, _lib.Linear(None, None))
    arr = lambda *x: ctypes.cast((ctypes.c_int32 * len(x))(*x), ctypes.c_void_p)
    keep = []

    def call(cu=(0, 1, 2), F=1, fcu=(0, 1), src=(0, 0), tl=(0, 0), V=2):
        a = [None if x is None else (ctypes.c_int32 * len(x))(*x) for x in (cu, fcu, src, tl)]
        keep.append(a)
        p = [None if x is None else ctypes.cast(x, ctypes.c_void_p) for x in a]
        return lib.infv_vqf_vc_encode_streams(fake, None, V, p[0], None, F, p[1], p[2], 16, ctypes.byref(w), None, p[3], None, 1,
                                              None, None, None, None)

    assert call(fcu=None) == -1 and call(src=None) == -1
    assert call(F=0) == -1
    assert call(fcu=(1, 2)) == -1                                  # fcu[0] != 0
    assert call(F=2, fcu=(0, 2, 1)) == -1                          # decreasing fcu
    assert call(src=(0, -1)) == -1 and call(src=(1, 0)) == -1      # frame_src out of range
    assert call(cu=(0, 2, 3)) == -1                                # stream 0 has 2 chunks, its block 1
    assert call(V=0) == 0
    assert b"vc_encode_streams" in lib.infv_ltm_last_error()
    # the LTM layer: a negative base before any handle is read
    cu = arr(0, 1)
    assert lib.infv_ltm_steps_videos_from(ctypes.cast((ctypes.c_void_p * 1)(64), ctypes.c_void_p), 1, cu, fake, arr(-1), 4, fake, 1, 8,
                                          None, None, 1, fake, None) == -1
    assert b"kbar_chunk0" in lib.infv_ltm_last_error()


def _model(**kw):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    return VideoChat2Encoder(32, 8, 64, 64, 32, True, 0.75, 0.75, 2, 2, hidden_size=128, intermediate_size=256,
                             num_attention_heads=2, tokens_per_frame=4, **kw)


def test_python_argument_checks_raise_before_any_library_call(monkeypatch):
    from infinite_video_amd import _lib
    from infinite_video_amd import videochat2_qformer as vc

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    m = _model()
    v = lambda c, T: torch.zeros(c, T * 4, 64)
    te = lambda n: torch.zeros(1, n, 128)
    with pytest.raises(ValueError, match="2 text_embeds for 3 videos"):
        m.encode_streams([v(2, 16)], [0, 0, 0], text_embeds=[te(3), te(4)])            # frame_src of the wrong length
    with pytest.raises(ValueError, match=r"frame_src\[1\] = 1 outside \[0, 1\)"):
        m.encode_streams([v(2, 16)], [0, 1])
    with pytest.raises(ValueError, match=r"frame_src\[0\] = -1 outside"):
        m.encode_streams([v(2, 16), v(1, 16)], [-1, 1])
    shared = object()
    with pytest.raises(ValueError, match="1 memories for 2 videos"):
        m.encode_streams([v(2, 16)], [0, 0], memories=[shared])                        # the wrong number of memories
    with pytest.raises(ValueError, match="appears twice"):
        m.encode_streams([v(2, 16)], [0, 0], memories=[shared, shared])
    with pytest.raises(ValueError, match="video_ids"):
        m.encode_streams([v(2, 16)], [0, 0], video_ids=[1])
    with pytest.raises(ValueError, match="at least one stream"):
        m.encode_streams([v(2, 16)], [])
    with pytest.raises(ValueError, match=r"u must be \[5, 1, 512\]"):                   # chunks per STREAM: 2 + 1 + 2
        m.encode_streams([v(2, 16), v(1, 16)], [0, 1, 0], u=torch.zeros(3, 1, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="one call takes one chunk length"):
        m.encode_streams([v(2, 16), v(1, 8)], [0, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode_streams([v(2, 16)], [0, 0])                                           # (CPU tensors: no fallback)
    with pytest.raises(ValueError, match="1 memories for 2 instructions"):
        vc.encode_long_video_prompts_vc(m, torch.zeros(32, 4, 64), 2, [te(3), te(4)], memories=[shared])
    with pytest.raises(ValueError, match="at least one instruction"):
        vc.encode_long_video_prompts_vc(m, torch.zeros(32, 4, 64), 2, [])


def test_prompts_fallback_consumes_the_generator_as_the_loop_does(monkeypatch):
    """A frame count that does not batch (36 frames in 8: chunks of 5 and one of 1): every instruction takes encode_long_video_vc
    in turn, so the generator ends where the loop leaves it and encode_tokens sees the loop's calls in the loop's order."""
    from infinite_video_amd import videochat2_qformer as vc
    m = _model()
    frames = torch.arange(36 * 4 * 64, dtype=torch.float32).reshape(36, 4, 64)
    assert vc.batched_chunks_vc(36, 8, 4) is None
    tes = [torch.zeros(1, n, 128) for n in (3, 0, 7)]
    calls = []

    def stub(self, image_embeds, text_embeds=None, new_video=False, hidden_in=None):
        # what the real one draws per chunk on a continued sticky memory: one block of 1024 per LTM instance
        if not new_video:
            for _ in self.qformer.ltm_modules:
                torch.rand(1024, dtype=torch.float64)
        calls.append((tuple(image_embeds.shape), None if text_embeds is None else text_embeds.size(1), bool(new_video)))
        return torch.full((1, self.n_query, 64), float(len(calls))), None

    monkeypatch.setattr(vc.VideoChat2Encoder, "encode_tokens", stub)
    torch.manual_seed(5)
    want = [vc.encode_long_video_vc(m, frames, 8, te) for te in tes]
    want_calls, want_state = list(calls), torch.get_rng_state()
    calls.clear()
    torch.manual_seed(5)
    got = vc.encode_long_video_prompts_vc(m, frames, 8, tes)
    assert torch.equal(torch.get_rng_state(), want_state)
    assert calls == want_calls and len(calls) == 3 * 8
    assert len(got) == 3
    for (gm, ge), (wm, we) in zip(got, want):
        assert torch.equal(gm, wm) and len(ge) == len(we) == 8
