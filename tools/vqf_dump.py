#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of the library on the Q-former entry points: a fixed list of small calls on seeded ``synth``
inputs, run in a fresh child process per build; every output, every exported memory and the ``infv_ltm_launch_count()`` delta of
each call go into an ``.npz``, and the two files must agree with ``np.array_equal`` on the arrays' bytes (the mean of a video without a
chunk is NaN, which compares unequal to itself as a number: the bytes say whether the bits agree).

usage: python tools/vqf_dump.py OTHER_LIBRARY.so [REPORT.txt]     (the other build against the one in the tree)

The list (shapes: tests/golden/seam_cases.py's BASE and VQF_BASE, the frame Q-former's SMALL): ``encode_videos`` with counts (2, 0, 3)
and texts (5, 0, 17) and ``encode_streams`` with blocks (5, 2) and frame_src [0, 1, 0, 0, 1], from fp32, fp16, bf16 and fp8 tokens, each
on a default handle, on one created under INFV_VQF_SPLIT_CACHE_GB=0 and on one with set_precision(h, 1); ``encode_img_videos`` from fp16
vision output with the vision LayerNorm and ids; ``encode_frames`` at 65 and 128 tokens per frame with bf16 output; ``encode_chunk``,
``encode_video`` and ``infv_vqf_encode_videos``; every call with memories followed by one with new_video = 0 on the same memories;
``infv_vqf_token_pass`` with the frame means from each token dtype at (P, T, d, nb) = (4, 24, 64, 2), a whole tile plus a partial one.  The
whole list runs twice on the same handles, the second time in reverse order: a handle sees growing, then non-growing calls."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(path):
    import torch
    from infinite_video_amd import _lib
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    from tests.golden import seam_cases as sc
    from tests.golden import transition_cases as tc
    from tests.golden.frame_qformer_cases import SMALL, vision_rows
    from tests.test_frame_qformer_gpu import _model as frame_model
    from tests.test_path_transitions_gpu import _Vqf
    from tests.test_vc_encode_img_cpu import MAX_POS, VOCAB, front_weights, small_model
    from tests.test_vc_videos_gpu import small_setup

    dev, lib = torch.device("cuda:0"), _lib.load()
    out, s = {}, sc.BASE
    host = lambda t: (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()

    def counted(key, fn):
        n0 = lib.infv_ltm_launch_count()
        res = fn()
        torch.cuda.synchronize()
        out[key + "/launches"] = np.int64(lib.infv_ltm_launch_count() - n0)
        return res

    def keep_vc(key, res, mems):
        proj, mean, hid = res
        out[key + "/proj"], out[key + "/mean"] = host(proj), host(mean)
        for v, h in enumerate(hid):
            out[f"{key}/hidden{v}"] = host(h)
        for v, mem in enumerate(mems):
            for j, e in enumerate(mem.engines):
                if not e.has_memory:                            # (a video without a chunk)
                    continue
                B, mass = e.export_state(0)
                out[f"{key}/B{v}.{j}"], out[f"{key}/mass{v}.{j}"] = host(B), host(mass)

    # ---- the VideoChat2 encoder: three handles
    def vc_model(env=None, exact=False):
        if env:
            os.environ.update(env)
        m = small_setup(dev)[2]
        h = m._vc_handle(dev)                                  # (INFV_VQF_SPLIT_CACHE_GB is read when the handle is created)
        for k in env or {}:
            del os.environ[k]
        _lib.check(lib.infv_vqf_set_precision(h, int(exact)))
        return m
    models = {"default": vc_model(), "nocache": vc_model({"INFV_VQF_SPLIT_CACHE_GB": "0"}), "exact": vc_model(exact=True)}
    blocks = [torch.from_numpy(sc.small_video(s, f, n, 0)[0]).to(dev) for f, n in enumerate((5, 2))]
    videos = [torch.from_numpy(sc.small_video(s, v, n, 0)[0]).to(dev) for v, n in enumerate(s["counts"])]
    w_vc = sc.layout_weights(sc.Layout("dump", "vc", dict(s), (), (), (), (), ()))
    rows = lambda texts: [torch.from_numpy(sc.small_video(s, v, 0, t, w_vc)[1]) for v, t in enumerate(texts)]
    nx = sc.n_cross_of(s)
    uniforms = lambda n, seed: torch.from_numpy(np.random.default_rng(seed).random((n, nx, sc.S)))
    dtypes = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn}

    def vc_case(tag, model, form, dt):
        def run():
            m = models[model]
            src = [0, 1, 0, 0, 1] if form == "streams" else None
            toks = [(x * 0.3).to(dtypes[dt]) for x in (blocks if src else videos)]
            texts = (5, 0, 17, 5, 0) if src else s["texts"]
            total = sum(int(toks[f].shape[0]) for f in src) if src else sum(s["counts"])
            mems = [VideoChat2Memory(m, dev) for _ in texts]
            for i, new in enumerate((True, False)):             # the second call continues the same memories
                if i == 1 and not src:                          # (only a video that has a memory can continue it)
                    live = [v for v, n in enumerate(s["counts"]) if n]
                    toks, mems, texts = [toks[v] for v in live], [mems[v] for v in live], [texts[v] for v in live]
                kw = dict(hidden_in=rows(texts), new_video=new, u=uniforms(total, 50 + i), memories=mems, want_hidden=True)
                key = f"{tag}/vc/{model}/{form}/{dt}/call{i}"
                res = counted(key, lambda: m.encode_streams(toks, src, **kw) if src else m.encode_videos(toks, **kw))
                keep_vc(key, res, mems)
        return run

    # ---- encode_img behind the vision encoder: the vision LayerNorm and the embedding layer in front
    _, w_img, m_img = small_model(vocab_size=VOCAB, max_position_embeddings=MAX_POS, vision_layernorm=True)
    m_img.load_reference_state_dict(dict(w_img, **front_weights(s)))
    m_img = m_img.to(dev).eval()

    def img_case(tag):
        def run():
            ids = [torch.arange(t) % VOCAB for t in s["texts"]]
            mems = [VideoChat2Memory(m_img, dev) for _ in ids]
            vis = [v.half() for v in videos]
            for i, new in enumerate((True, False)):
                if i == 1:                                      # (only a video that has a memory can continue it)
                    live = [v for v, n in enumerate(s["counts"]) if n]
                    vis, mems, ids = [vis[v] for v in live], [mems[v] for v in live], [ids[v] for v in live]
                key = f"{tag}/img/call{i}"
                res = counted(key, lambda: m_img.encode_img_videos(vis, input_ids=ids, new_video=new,
                                                                   u=uniforms(sum(s["counts"]), 60 + i), memories=mems, want_hidden=True))
                keep_vc(key, res, mems)
        return run

    # ---- the per-frame image Q-former
    m_frames = frame_model(SMALL, True)

    def frames_case(tag, n_tokens):
        def run():
            x = torch.from_numpy(vision_rows(3, n_tokens, SMALL["enc_width"], seed=100 + n_tokens)).to(dev)
            key = f"{tag}/frames/{n_tokens}"
            out[key + "/out"] = host(counted(key, lambda: m_frames.encode_frames(x, out_dtype=torch.bfloat16)))
        return run

    # ---- the video Q-former through the raw C ABI
    q = _Vqf()

    def vqf_case(tag, op):
        def run():
            vids = range(tc.VQF_VIDEOS)
            mems = [q.memory() for _ in vids]
            for i, new in enumerate((True, False)):
                ks = [torch.from_numpy(tc.vqf_chunks(v)[2 * i:2 * i + 2]).to(dev) for v in vids]
                us = [torch.from_numpy(np.random.default_rng(70 + 10 * i + v).random((2, q.L, sc.S))).to(dev) for v in vids]
                key = f"{tag}/vqf/{op}/call{i}"
                res = counted(key, lambda: q.run(op, mems, ks, us, new))
                for v, (hid, lla) in enumerate(res):
                    out[f"{key}/hidden{v}"], out[f"{key}/llama{v}"] = hid, lla
                for v, mem in enumerate(mems):
                    for l, e in enumerate(mem):
                        B, mass = e.export_state(0)
                        out[f"{key}/B{v}.{l}"], out[f"{key}/mass{v}.{l}"] = host(B), host(mass)
        return run

    # ---- the token pass alone, with the frame means: 96 tokens a chunk, a whole 64-token tile plus a partial one
    def pass_case(tag, dt):
        def run():
            P, T, d, nb = 4, 24, 64, 2
            n = T * P
            x = torch.from_numpy(np.random.default_rng(80).standard_normal((nb, n, d))).float().to(dtypes[dt]).to(dev)
            names = {"bf16": ("Th",), "f8": ("Fh", "Th")}.get(dt, ("Fh", "Fl", "Th", "Tl"))
            planes = {k: torch.zeros(nb * n * d, dtype=torch.bfloat16, device=dev) for k in names}
            kbar = torch.zeros(nb * T * d, dtype=torch.float32, device=dev)
            ptr = lambda k: C.c_void_p(planes[k].data_ptr()) if k in planes else None
            key = f"{tag}/pass/{dt}"
            with torch.cuda.device(dev):
                _lib.check(counted(key, lambda: lib.infv_vqf_token_pass(
                    C.c_void_p(x.data_ptr()), {"f32": 0, "bf16": 1, "f16": 3, "f8": 4}[dt], nb, n, d, P, ptr("Fh"), ptr("Fl"), ptr("Th"),
                    ptr("Tl"), C.c_void_p(kbar.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))))
            out[key + "/kbar"] = host(kbar)
            for k, t in planes.items():
                out[f"{key}/{k}"] = host(t)
        return run

    def cases(tag):
        lst = [vc_case(tag, model, form, dt) for model in models for dt in dtypes for form in ("videos", "streams")]
        lst += [img_case(tag), frames_case(tag, 65), frames_case(tag, 128)] + [pass_case(tag, dt) for dt in dtypes]
        return lst + [vqf_case(tag, op) for op in ("chunk", "video", "videos")]

    for run in cases("forward") + cases("reverse")[::-1]:
        run()
    q.close()
    np.savez(path, **out)


def main():
    other = os.path.abspath(sys.argv[1])
    report = sys.argv[2] if len(sys.argv) > 2 else None
    dumps = []
    for name, lib in (("other", other), ("tree", "")):
        env = dict(os.environ, INFV_LTM_LIBRARY=lib)
        path = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env=env, cwd=ROOT, timeout=900)
        dumps.append({k: v for k, v in np.load(path).items()})
        os.remove(path)
    a, b = dumps
    raw = lambda x: np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
    lines = [f"vqf_dump: {other} against the tree's build: {len(a)} arrays of the other build, {len(b)} of the tree's"]
    bad = sorted(set(a) ^ set(b))
    lines += [f"only in one dump: {k}" for k in bad]
    launches = 0
    for k in sorted(set(a) & set(b)):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not np.array_equal(raw(a[k]), raw(b[k])):
            bad.append(k)
            lines.append(f"DIFFERENT {k}: other {a[k].ravel()[:4]} tree {b[k].ravel()[:4]}")
        if k.endswith("/launches"):
            launches += 1
            lines.append(f"{k}: {int(a[k])} = {int(b[k])}" if int(a[k]) == int(b[k]) else f"{k}: {int(a[k])} != {int(b[k])}")
    # the only values that are not finite: the mean of the video without a chunk, in the calls that have one
    empty_mean = lambda k: k.endswith("/call0/mean") and ("/videos/" in k or "/img/" in k)
    finite = all(np.isfinite(v.astype(np.float64)).all() for k, v in b.items() if v.dtype.kind == "f" and not empty_mean(k))
    lines.append(f"{len(b) - launches} arrays and {launches} launch counts compared bit for bit; every float array finite "
                 f"(but the NaN mean of the video without a chunk): {finite}")
    lines.append("VQF_DUMP_OK" if not bad and finite and len(b) > launches else "VQF_DUMP_FAIL")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    sys.exit(0 if lines[-1] == "VQF_DUMP_OK" else 1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
