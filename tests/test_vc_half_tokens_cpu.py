"""fp16 / bf16 frame tokens on the batched VideoChat2 path (infv_vqf_vc_encode_videos_tok, infv_vqf_vc_encode_streams_tok,
infv_vqf_token_pass): declarations, exported symbols, the ctypes argument lists against the header and the refusals that need no
device.  No GPU needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "infinite-video_amd", "libinfv_ltm.so")
VQF_H = os.path.join(ROOT, "include", "infv_vqf.h")
# the call each new one extends: the same argument list plus token_dtype right behind frames
SIBLING = {"infv_vqf_vc_encode_videos_tok": "infv_vqf_vc_encode_videos", "infv_vqf_vc_encode_streams_tok": "infv_vqf_vc_encode_streams"}
NEW = tuple(SIBLING) + ("infv_vqf_token_pass",)
INVALID, UNSUPPORTED = -1, -2


def _args(sym):
    """[(type, name)] of the declaration of ``sym`` in the header (comments stripped)."""
    h = re.sub(r"/\*.*?\*/", "", open(VQF_H).read(), flags=re.S)
    m = re.search(r"^int " + sym + r"\((.*?)\);", h, re.M | re.S)
    assert m, f"{sym} is not declared"
    out = []
    for a in m.group(1).split(","):
        a = re.sub(r"\s+", " ", a).strip()
        typ, name = re.match(r"(.*?)(\w+)$", a).groups()
        out.append((typ.strip().replace(" *", "*"), name))
    return out


def test_header_declares_them_as_the_old_calls_plus_token_dtype():
    for sym, sib in SIBLING.items():
        new, old = _args(sym), _args(sib)
        pos = [n for _, n in old].index("frames") + 1
        assert new[pos] == ("int32_t", "token_dtype"), (sym, new[pos])
        assert new[pos - 1] == ("const void*", "frames") and old[pos - 1] == ("const float*", "frames")
        kept = new[:pos - 1] + new[pos + 1:]
        assert kept == old[:pos - 1] + old[pos:], f"{sym} is {sib} plus token_dtype behind frames"
    assert _args("infv_vqf_token_pass") == [
        ("const void*", "frames"), ("int32_t", "token_dtype"), ("int32_t", "nb"), ("int32_t", "n_tokens"), ("int32_t", "d"),
        ("int32_t", "tokens_per_frame"), ("void*", "Fh"), ("void*", "Fl"), ("void*", "Th"), ("void*", "Tl"), ("float*", "kbar"),
        ("void*", "stream")]


def test_library_exports_them_and_the_abi_version_stays():
    from infinite_video_amd import _lib
    raw = ctypes.CDLL(LIB)
    for sym in NEW:
        assert hasattr(raw, sym), sym
        assert sym in _lib._SIGNATURES and sym in _lib.EXPORTED_SYMBOLS
    assert _lib.load().infv_ltm_abi_version() == 6 and _lib.ABI_VERSION == 6


def test_ctypes_argument_lists_match_the_declarations():
    from infinite_video_amd import _lib
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for sym in NEW:
        res, args = _lib._SIGNATURES[sym]
        decl = _args(sym)
        assert res is ctypes.c_int and len(args) == len(decl), sym
        for (typ, name), ct in zip(decl, args):
            if typ in scalar:
                assert ct is scalar[typ], (sym, name, typ)
            else:                                                 # every pointer and handle travels as a pointer-sized argument
                assert typ.endswith("*") or typ.endswith("_handle"), (sym, name, typ)
                assert ctypes.sizeof(ct) == ctypes.sizeof(ctypes.c_void_p), (sym, name)
    for sym, sib in SIBLING.items():
        args, sib_args = _lib._SIGNATURES[sym][1], _lib._SIGNATURES[sib][1]
        pos = [n for _, n in _args(sib)].index("frames") + 1
        assert args[:pos] + args[pos + 1:] == list(sib_args), f"{sym}: the arguments it shares with {sib} have other ctypes"


def test_refusals_that_need_no_device():
    """Through a fake handle, as tests/test_vc_streams_cpu.py does: nothing below may read the handle or touch a device."""
    from infinite_video_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    layers = (_lib.VqfVcLayer * 1)()
    w = _lib.VqfVcWeights(1, 0, layers, _lib.Linear(None, None))
    i32 = lambda *x: (ctypes.c_int32 * len(x))(*x)
    cu, fcu, src, tl = i32(0, 1, 2), i32(0, 1), i32(0, 0), i32(0, 0)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    base = 4096                                                    # a 16-byte aligned address that is never read

    def videos(frames, code):
        return lib.infv_vqf_vc_encode_videos_tok(fake, None, 2, p(cu), ctypes.c_void_p(frames), code, 16, ctypes.byref(w), None, p(tl),
                                                 None, 1, None, None, None, None)

    def streams(frames, code):
        return lib.infv_vqf_vc_encode_streams_tok(fake, None, 2, p(cu), ctypes.c_void_p(frames), code, 1, p(fcu), p(src), 16,
                                                  ctypes.byref(w), None, p(tl), None, 1, None, None, None, None)

    for call in (videos, streams):
        for code in (2, 7, -1):
            assert call(base, code) == INVALID, (call.__name__, code)
            assert b"unknown token dtype" in lib.infv_ltm_last_error()
        for code in (1, 3):
            assert call(base + 2, code) == INVALID, (call.__name__, code)
            assert b"16-byte" in lib.infv_ltm_last_error()
    assert lib.infv_vqf_vc_encode_streams_tok(fake, None, 2, p(cu), ctypes.c_void_p(base), 3, 1, None, p(src), 16, ctypes.byref(w), None,
                                              p(tl), None, 1, None, None, None, None) == INVALID

    def tpass(code=3, nb=1, n=64, d=64, P=4, frames=base, Fh=base, Fl=base, Th=base, Tl=base, kbar=base):
        v = lambda x: ctypes.c_void_p(x) if x else None
        return lib.infv_vqf_token_pass(v(frames), code, nb, n, d, P, v(Fh), v(Fl), v(Th), v(Tl), v(kbar), None)

    assert tpass(d=48) == INVALID
    assert tpass(n=40) == INVALID
    assert tpass(code=1) == INVALID and b"bf16" in lib.infv_ltm_last_error()       # bf16 with a non-NULL Fl
    assert tpass(code=1, Fh=0, Tl=0) == INVALID                                      # ... Fl alone is enough
    for code in (2, 7):
        assert tpass(code=code) == INVALID
    assert tpass(frames=base + 2) == INVALID and tpass(code=1, Fh=0, Fl=0, Tl=0, Th=base + 8) == INVALID
    assert tpass(Fl=0) == INVALID and tpass(Th=0) == INVALID and tpass(frames=0) == INVALID
    assert tpass(n=96, P=5) == INVALID                                               # 5 does not divide 96
    # no one-pass form with the means: a frame that does not divide the 64-token tile, whatever the token type
    assert tpass(n=192, P=6) == UNSUPPORTED and tpass(code=1, n=192, P=6, Fh=0, Fl=0, Tl=0) == UNSUPPORTED
    assert tpass(code=0, n=192, P=12) == UNSUPPORTED and tpass(code=3, n=192, P=12) == UNSUPPORTED
    assert b"token_pass" in lib.infv_ltm_last_error()

