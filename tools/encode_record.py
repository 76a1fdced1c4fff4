#!/usr/bin/env python3
"""Same launches, same bits: a fixed list of small calls of the video Q-former entry points, recorded on ONE build of the library per
process -- per call one JSON line with the ``infv_ltm_launch_count()`` delta and a SHA-256 of every output buffer and every memory.

    python tools/encode_record.py run OUT.jsonl [LIBRARY.so] [--arrays OUT.npz]     (library: the argument, else INFV_LTM_LIBRARY, else the tree's)
    python tools/encode_record.py compare PARENT.jsonl PARENT_AGAIN.jsonl BRANCH.jsonl [RECORD.jsonl]

``compare`` wants two runs of the parent build and one of this build (three separate processes).  A call whose hashes differ between
the two parent runs is reported as not reproducible; for it, the ``--arrays`` files (same names, ``.npz``) give the maximum absolute
difference parent vs branch beside parent vs parent.  Every other call must agree in its launch count and in every hash.

The calls (shapes: tests/golden/seam_cases.py's VQF_BASE and BASE, the frame Q-former's SMALL; uniforms drawn on the host from fixed
seeds): on the raw C ABI ``encode_chunk`` x 3 chunks with weights epoch 0 and x 3 with epoch 5 (layer 0's prefix cache), ``encode_video``
with 9 chunks (pick_short_nb's search runs) and new_video 1 then 0, ``encode_videos`` with counts (2, 0, 3) -- as they are, with
alpha == 1 (no memories), from bf16 tokens, and with set_precision(h, 1) (the fp32 contractions); ``vc_encode_videos``,
``vc_encode_streams``, ``vc_encode_img`` and ``encode_frames``; ``encode_frames`` with the fp16 attention precision and bf16 output."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(out_path, arrays_path):
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine
    from infinite_video_amd.videochat2_qformer import VideoChat2Memory
    from tests.golden import seam_cases as sc
    from tests.golden import transition_cases as tc
    from tests.golden.frame_qformer_cases import SMALL, vision_rows
    from tests.test_config_sweep_gpu import _vqf_weights_struct
    from tests.test_frame_qformer_gpu import _model as frame_model
    from tests.test_vc_encode_img_cpu import MAX_POS, VOCAB, front_weights, small_model
    from tests.test_vc_videos_gpu import small_setup

    dev, lib = torch.device("cuda:0"), _lib.load()
    host = lambda t: (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines, arrays = [], {}

    def record(key, fn, outputs):
        """Run fn, then hash what ``outputs()`` returns: {name: tensor or ndarray}."""
        torch.cuda.synchronize()
        n0 = lib.infv_ltm_launch_count()
        with torch.cuda.device(dev):
            fn()
        torch.cuda.synchronize()
        n = int(lib.infv_ltm_launch_count() - n0)
        bufs = {k: (host(v) if torch.is_tensor(v) else np.asarray(v)) for k, v in outputs().items()}
        for k, v in bufs.items():
            arrays[f"{key}/{k}"] = v
        lines.append({"call": key, "launches": n,
                      "sha256": {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(bufs.items())}})

    # ---- the video Q-former through the raw C ABI
    s = sc.VQF_BASE
    L, Q, T, S = s["n_layers"], s["n_query"], s["T"], sc.S
    ws, keep = _vqf_weights_struct(tc.vqf_weights(), L, dev)
    chunks = lambda v, n: torch.from_numpy(np.stack([synth.frame_tokens(c, T, s["P"], s["enc_width"], seed=synth.SEED_K + 1000 * (v + 1))
                                                     for c in range(n)]))
    uniforms = lambda n, seed: torch.from_numpy(np.random.default_rng(seed).random((n, L, S))).to(dev)

    def vqf_block(tag, alpha=s["alpha"], tok=torch.float32, exact=False):
        cfg = _lib.VqfConfig(n_layers=L, n_heads=s["heads"], hidden=s["hidden"], inter=s["inter"], enc_width=s["enc_width"],
                             tokens_per_frame=s["P"], n_query=Q, proj_out=s["proj"], nb_samples=S, alpha=alpha, ln_eps=1e-12)
        h = C.c_void_p()
        _lib.check(lib.infv_vqf_create(C.byref(cfg), C.byref(h)))
        _lib.check(lib.infv_vqf_set_token_dtype(h, {torch.float32: 0, torch.bfloat16: 1}[tok]))
        _lib.check(lib.infv_vqf_set_precision(h, int(exact)))
        use_ltm = alpha != 1.0

        def memory():
            if not use_ltm:
                return []
            engs = [LTMEngine(s["N"], s["heads"], s["hidden"] // s["heads"], s["enc_width"], s["P"], tau=s["tau"], sticky=s["sticky"],
                              n_layers=1, max_q=Q, device=dev) for _ in range(L)]
            for e in engs:
                e.ensure_plan(T)
            return engs

        handles = lambda mems: (C.c_void_p * max(1, len(mems) * L))(*[e._h.value for m in mems for e in m]) if use_ltm else None

        def state(mems):
            out = {}
            for v, m in enumerate(mems):
                for l, e in enumerate(m):
                    if e.has_memory:
                        out[f"B{v}.{l}"], out[f"mass{v}.{l}"] = e.export_state(0)
            return out

        def outs(n, mean_rows):
            hid, lla = torch.zeros(n, Q, s["hidden"], device=dev), torch.zeros(n, Q, s["proj"], device=dev)
            return hid, lla, (torch.zeros(mean_rows, Q, s["proj"], device=dev) if mean_rows else None)

        # encode_chunk: 3 chunks with epoch 0, then 3 with epoch 5 on the same memories
        mem, k, u = memory(), (chunks(0, 6) * 0.3).to(tok).to(dev), uniforms(6, 11)
        for epoch, c0 in ((0, 0), (5, 3)):
            _lib.check(lib.infv_vqf_set_weights_epoch(h, epoch))
            for c in range(c0, c0 + 3):
                hid, lla, _ = outs(1, 0)
                record(f"{tag}/encode_chunk/epoch{epoch}/chunk{c}",
                       lambda: _lib.check(lib.infv_vqf_encode_chunk(h, handles([mem]), ptr(k[c]), T, C.byref(ws), ptr(u[c]), int(c == 0),
                                                                    ptr(hid), ptr(lla), stream())),
                       lambda: dict(state([mem]), hidden=hid, llama=lla))
        _lib.check(lib.infv_vqf_set_weights_epoch(h, 0))
        # encode_video: 9 chunks, new_video 1 then 0
        mem, k = memory(), (chunks(1, 18) * 0.3).to(tok).to(dev)
        for i in range(2):
            hid, lla, mean = outs(9, 1)
            u = uniforms(9, 21 + i)
            record(f"{tag}/encode_video/new_video{1 - i}",
                   lambda: _lib.check(lib.infv_vqf_encode_video(h, handles([mem]), ptr(k[9 * i:]), 9, T, C.byref(ws), ptr(u), 1 - i, ptr(hid),
                                                                ptr(lla), ptr(mean), stream())),
                   lambda: dict(state([mem]), hidden=hid, llama=lla, mean=mean))
        # encode_videos: counts (2, 0, 3)
        counts = (2, 0, 3)
        mems, k, u = [memory() for _ in counts], (chunks(2, 5) * 0.3).to(tok).to(dev), uniforms(5, 31)
        cu = (C.c_int32 * 4)(0, *np.cumsum(counts).tolist())
        hid, lla, mean = outs(5, 3)
        record(f"{tag}/encode_videos",
               lambda: _lib.check(lib.infv_vqf_encode_videos(h, handles(mems), 3, C.cast(cu, C.c_void_p), ptr(k), T, C.byref(ws), ptr(u), 1,
                                                             ptr(hid), ptr(lla), ptr(mean), stream())),
               lambda: dict(state(mems), hidden=hid, llama=lla, mean=mean))
        _lib.check(lib.infv_vqf_destroy(h))

    vqf_block("vqf")
    vqf_block("vqf_alpha1", alpha=1.0)
    vqf_block("vqf_bf16", tok=torch.bfloat16)
    vqf_block("vqf_exact", exact=True)

    # ---- the VideoChat2 encoder and the frame Q-former, through their modules
    b = sc.BASE
    model = small_setup(dev)[2]
    w_vc = sc.layout_weights(sc.Layout("record", "vc", dict(b), (), (), (), (), ()))
    rows = lambda texts: [torch.from_numpy(sc.small_video(b, v, 0, t, w_vc)[1]) for v, t in enumerate(texts)]
    vc_u = lambda n, seed: torch.from_numpy(np.random.default_rng(seed).random((n, sc.n_cross_of(b), S)))
    videos = [torch.from_numpy(sc.small_video(b, v, n, 0)[0]).to(dev) for v, n in enumerate(b["counts"])]
    blocks = [torch.from_numpy(sc.small_video(b, f, n, 0)[0]).to(dev) for f, n in enumerate((5, 2))]

    def vc_outputs(res, mems):
        proj, mean, hid = res[0]
        out = {"proj": proj, "mean": mean, **{f"hidden{v}": x for v, x in enumerate(hid)}}
        for v, mem in enumerate(mems):
            for j, e in enumerate(mem.engines):
                if e.has_memory:
                    out[f"B{v}.{j}"], out[f"mass{v}.{j}"] = e.export_state(0)
        return out

    def vc_call(key, fn, n_mems, m=model):
        mems, res = [VideoChat2Memory(m, dev) for _ in range(n_mems)], []
        record(key, lambda: res.append(fn(mems)), lambda: vc_outputs(res, mems))

    vc_call("vc/encode_videos", lambda mems: model.encode_videos(videos, hidden_in=rows(b["texts"]), new_video=True, u=vc_u(5, 41),
                                                                 memories=mems, want_hidden=True), 3)
    src = [0, 1, 0, 0, 1]
    vc_call("vc/encode_streams", lambda mems: model.encode_streams(blocks, src, hidden_in=rows((5, 0, 17, 5, 0)), new_video=True,
                                                                   u=vc_u(19, 42), memories=mems, want_hidden=True), 5)
    _, w_img, m_img = small_model(vocab_size=VOCAB, max_position_embeddings=MAX_POS, vision_layernorm=True)
    m_img.load_reference_state_dict(dict(w_img, **front_weights(b)))
    m_img = m_img.to(dev).eval()
    ids = [torch.arange(t) % VOCAB for t in b["texts"]]
    vc_call("vc/encode_img", lambda mems: m_img.encode_img_videos([v.half() for v in videos], input_ids=ids, new_video=True, u=vc_u(5, 43),
                                                                  memories=mems, want_hidden=True), 3, m_img)
    m_frames = frame_model(SMALL, True)
    x = torch.from_numpy(vision_rows(3, 65, SMALL["enc_width"], seed=165)).to(dev)
    for prec, dt in (("fp32", torch.float32), ("fp16", torch.bfloat16)):
        m_frames.set_attention_precision(prec)
        res = []
        record(f"frames/encode_frames/attention_{prec}/{str(dt).split('.')[1]}",
               lambda: res.append(m_frames.encode_frames(x, out_dtype=dt)), lambda: {"out": res[0]})

    with open(out_path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    if arrays_path:
        np.savez(arrays_path, **arrays)
    print(f"encode_record: {len(lines)} calls, {sum(len(ln['sha256']) for ln in lines)} buffers on {_lib.LIB_PATH} -> {out_path}")


def compare(parent, again, branch, record_path):
    load = lambda p: {ln["call"]: ln for ln in map(json.loads, open(p))}
    a, a2, b = load(parent), load(again), load(branch)
    npz = lambda p: np.load(p[:-len(".jsonl")] + ".npz") if os.path.exists(p[:-len(".jsonl")] + ".npz") else None
    arr = {"a": npz(parent), "a2": npz(again), "b": npz(branch)}
    ok, out = set(a) == set(a2) == set(b), []
    for call in sorted(set(a) & set(a2) & set(b)):
        line = {"call": call, "launches": {"parent": a[call]["launches"], "branch": b[call]["launches"]}, "buffers": len(a[call]["sha256"]),
                "parent_reproducible": a[call] == a2[call], "equal": a[call] == b[call]}
        if not line["parent_reproducible"] and all(x is not None for x in arr.values()):
            diff = lambda x, y, k: float(np.nanmax(np.abs(x[k].astype(np.float64) - y[k].astype(np.float64))))
            keys = [f"{call}/{k}" for k in a[call]["sha256"]]
            line["max_abs_parent_vs_parent"] = max(diff(arr["a"], arr["a2"], k) for k in keys)
            line["max_abs_parent_vs_branch"] = max(diff(arr["a"], arr["b"], k) for k in keys)
        ok = ok and (line["equal"] or not line["parent_reproducible"]) and line["launches"]["parent"] == line["launches"]["branch"]
        out.append(line)
    out.append({"summary": True, "calls": len(out), "buffers": sum(x["buffers"] for x in out), "all_launch_counts_equal":
                all(x["launches"]["parent"] == x["launches"]["branch"] for x in out), "all_hashes_equal": all(x["equal"] for x in out),
                "calls_the_parent_does_not_reproduce": [x["call"] for x in out if not x["parent_reproducible"]], "ok": ok})
    text = "".join(json.dumps(x) + "\n" for x in out)
    sys.stdout.write(text)
    if record_path:
        with open(record_path, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    if args[:1] == ["run"] and len(args) >= 2:
        if len(args) > 2:
            os.environ["INFV_LTM_LIBRARY"] = os.path.abspath(args[2])
        run(args[1], args[1][:-len(".jsonl")] + ".npz" if "--arrays" in sys.argv else None)
    elif args[:1] == ["compare"] and len(args) >= 4:
        compare(args[1], args[2], args[3], args[4] if len(args) > 4 else None)
    else:
        sys.exit(__doc__)
