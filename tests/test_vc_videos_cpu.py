"""The batched VideoChat2 path (infv_vqf_self_attention, infv_vqf_vc_encode_videos, VideoChat2Encoder.encode_videos,
encode_long_videos_vc): declarations, exported symbols, struct layout against the header, refusals that need no device, the
Python argument checks and the uniform draw order.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")
HEADER = os.path.join(ROOT, "include", "infv_vqf.h")
NEW_SYMBOLS = ("infv_vqf_self_attention", "infv_vqf_vc_encode_videos")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)      # comments stripped


def _struct_fields(header, name):
    """[(type, field)] of ``typedef struct { ... } name;`` in declaration order."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", header).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+\w+\s*\*|\w+)\s*(.*)$", decl, re.S)
        typ = re.sub(r"\s+", " ", m.group(1)).strip()
        for f in m.group(2).split(","):
            out.append((typ, f.strip()))
    return out


def test_header_declares_the_entry_points_and_structs():
    h = _header()
    for sym in NEW_SYMBOLS:
        assert re.search(r"^int " + sym + r"\(", h, re.M), sym
    assert re.search(r"\}\s*infv_vqf_vc_layer\s*;", h) and re.search(r"\}\s*infv_vqf_vc_weights\s*;", h)
    assert re.search(r"#define INFV_VQF_VC_MAX_LAYERS 24\b", h) and re.search(r"#define INFV_VQF_VC_MAX_TOKENS 608\b", h)
    n_args = lambda sym: len(re.search(r"^int " + sym + r"\((.*?)\);", h, re.M | re.S).group(1).split(","))
    assert n_args("infv_vqf_self_attention") == 7 and n_args("infv_vqf_vc_encode_videos") == 15


def test_library_exports_them_and_the_abi_version_stays():
    from infinite_video_amd import _lib
    raw = ctypes.CDLL(LIB)
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), sym
        assert sym in _lib._SIGNATURES
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert len(lib.infv_vqf_self_attention.argtypes) == 7 and len(lib.infv_vqf_vc_encode_videos.argtypes) == 15
    assert re.search(r"#define INFV_LTM_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "infv_ltm.h")).read())


def test_ctypes_structs_match_the_header():
    from infinite_video_amd import _lib
    h = _header()
    ctype_of = {"infv_linear": _lib.Linear, "infv_layernorm": _lib.LayerNorm, "int32_t": ctypes.c_int32,
                "const infv_vqf_vc_layer*": ctypes.POINTER(_lib.VqfVcLayer)}
    for name, cls in (("infv_vqf_vc_layer", _lib.VqfVcLayer), ("infv_vqf_vc_weights", _lib.VqfVcWeights)):
        fields = _struct_fields(h, name)
        assert [f for _, f in fields] == [f for f, _ in cls._fields_], name
        for (typ, f), (_, ct) in zip(fields, cls._fields_):
            assert ctype_of[typ.replace(" *", "*")] is ct, (name, f, typ)
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.Linear) == 2 * ptr and ctypes.sizeof(_lib.LayerNorm) == 2 * ptr
    assert ctypes.sizeof(_lib.VqfVcLayer) == 16 * 2 * ptr + 8                   # 16 pointer pairs + has_cross + reserved
    assert _lib.VqfVcLayer.has_cross.offset == 5 * 2 * ptr and _lib.VqfVcLayer.x_q.offset == 5 * 2 * ptr + 8
    assert ctypes.sizeof(_lib.VqfVcWeights) == 8 + ptr + 2 * ptr and _lib.VqfVcWeights.layers.offset == 8
    assert _lib.VC_MAX_LAYERS == 24 and _lib.VC_MAX_TOKENS == 608


def test_c_refusals_that_need_no_device():
    """Null arguments, a bad cu, too many layers and too many tokens are refused before the handle is used for device work."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    assert lib.infv_vqf_self_attention(None, fake, 1, 8, None, fake, None) == -1
    assert lib.infv_vqf_self_attention(fake, fake, 1, 609, None, fake, None) == -2
    layers = (_lib.VqfVcLayer * 1)()
    w = _lib.VqfVcWeights(1, 0, layers, _lib.Linear(None, None))
    cu, tl = (ctypes.c_int32 * 3)(0, 1, 2), (ctypes.c_int32 * 2)(0, 0)

    def call(h, V, cu_, weights, tl_):
        return lib.infv_vqf_vc_encode_videos(h, None, V, ctypes.cast(cu_, ctypes.c_void_p) if cu_ is not None else None, None, 16,
                                             ctypes.byref(weights) if weights is not None else None, None,
                                             ctypes.cast(tl_, ctypes.c_void_p) if tl_ is not None else None, None, 1, None, None,
                                             None, None)

    assert call(None, 2, cu, w, tl) == -1
    assert call(fake, 2, None, w, tl) == -1
    assert call(fake, 2, cu, None, tl) == -1
    assert call(fake, 2, cu, w, None) == -1
    assert call(fake, -1, cu, w, tl) == -1
    assert call(fake, 0, cu, w, tl) == 0


def _model(**kw):
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    return VideoChat2Encoder(32, 8, 64, 64, 32, True, 0.75, 0.75, 2, 2, hidden_size=128, intermediate_size=256,
                             num_attention_heads=2, tokens_per_frame=4, **kw)


def test_small_shapes_can_be_built_and_defaults_stay():
    from infinite_video_amd.videochat2_qformer import _Cfg, init_Qformer
    c = _Cfg()
    assert (c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_hidden_layers) == (768, 3072, 12, 12)
    q, tokens = init_Qformer(96, 1024, 0.75, 0.75, True, 64)
    assert tokens.shape == (1, 96, 768) and q.config.intermediate_size == 3072 and len(q.cross_layers) == 6
    m = _model()
    assert m.n_query == 40 and m.tokens_per_frame == 4 and m.query_tokens.shape == (1, 40, 128)
    assert all(x.tokens_per_frame == 4 and x.encoder_width == 64 for x in m.qformer.ltm_modules)
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder
    assert VideoChat2Encoder.tokens_per_frame == 196


def test_python_argument_checks_raise_before_any_library_call(monkeypatch):
    from infinite_video_amd import _lib
    from infinite_video_amd import videochat2_qformer as vc

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    m = _model()
    v = lambda c, T: torch.zeros(c, T * 4, 64)
    with pytest.raises(ValueError, match="one call takes one chunk length"):
        m.encode_videos([v(2, 16), v(1, 8)])                                   # mixed T
    shared = object()
    with pytest.raises(ValueError, match="appears twice"):
        m.encode_videos([v(1, 16), v(1, 16)], memories=[shared, shared])       # a repeated memory
    with pytest.raises(ValueError, match="1 memories for 2 videos"):
        m.encode_videos([v(1, 16), v(1, 16)], memories=[shared])               # the wrong number of memories
    with pytest.raises(TypeError, match="VideoChat2Memory"):
        m.encode_videos([v(1, 16)], memories=[shared])
    with pytest.raises(ValueError, match="at most 512"):
        m.encode_videos([v(1, 16)], text_embeds=torch.zeros(1, 513, 128))      # text longer than 512
    with pytest.raises(ValueError, match="at most 512"):
        m.encode_videos([v(1, 16)], hidden_in=torch.zeros(40 + 513, 128))
    with pytest.raises(ValueError, match="video_ids"):
        m.encode_videos([v(1, 16)], video_ids=[1, 2])
    with pytest.raises(ValueError, match="at least one"):
        m.encode_videos([])
    with pytest.raises(ValueError, match=r"must be \[C, T\*4, 64\]"):
        m.encode_videos([torch.zeros(1, 62, 64)])
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode_videos([v(1, 16)])                                            # (CPU tensors: no fallback)
    with pytest.raises(ValueError, match="memories for"):
        vc.encode_long_videos_vc(m, [torch.zeros(32, 4, 64)], 2, memories=[])


def test_uniform_draw_order_is_the_loops():
    """draw_vc_uniforms consumes the global generator as the loop of encode_tokens does: video by video, chunk by chunk, per
    LTM instance one block of 1024 whose first 512 are the draw; nothing on a new video's first chunk."""
    from infinite_video_amd.videochat2_qformer import draw_vc_uniforms
    counts, continuing, n_cross = [3, 1, 0, 2], [False, True, False, False], 6
    torch.manual_seed(11)
    got = draw_vc_uniforms(counts, continuing, n_cross)
    after = torch.get_rng_state()
    torch.manual_seed(11)
    want = torch.zeros(sum(counts), n_cross, 512, dtype=torch.float64)
    row = 0
    for c_v, cont in zip(counts, continuing):
        for c in range(c_v):
            if c > 0 or cont:
                for j in range(n_cross):                     # LongTermAttention._draw_uniforms: one torch.rand(2 * 512) per step
                    want[row + c, j] = torch.rand(1024, dtype=torch.float64)[:512]
        row += c_v
    assert torch.equal(got, want)
    assert torch.equal(torch.get_rng_state(), after)
    assert (got[0] == 0).all() and (got[1] != 0).all() and (got[3] != 0).all() and (got[4] == 0).all()


def test_which_videos_take_the_batched_call():
    from infinite_video_amd.videochat2_qformer import batched_chunks_vc
    assert batched_chunks_vc(128, 8, 196) == 16               # the eval shape: 8 chunks of 16 frames
    assert batched_chunks_vc(120, 5, 196) == 24
    assert batched_chunks_vc(100, 8, 196) is None             # torch.chunk gives 13, ..., 9: unequal chunks
    assert batched_chunks_vc(36, 4, 196) is None              # 9 frames: 1764 tokens, no multiple of 32
    assert batched_chunks_vc(16, 8, 196) is None              # 2 frames per chunk: 392 tokens
    assert batched_chunks_vc(0, 8, 196) is None
    assert batched_chunks_vc(64, 8, 4) == 8
