"""fp16 / bf16 / fp8 e4m3 frame tokens on the batched VideoChat2 path against fp32 tokens, at the eval shape of the reference's VideoChat2
drivers (T 16, P 196, width 1024, N 64, 96 query tokens, 12 layers, alpha 0.75, sticky, mistral_proj 4096).  Three measurements,
each in fresh child processes, one GPU process at a time, the sides alternated round by round; a child warms up once and times
`--calls` calls.  One JSON line each, appended to profiles/vc_half_tokens.jsonl:

    timeout -k 10 1100 python tools/bench_vc_token_dtypes.py [--parent-tree TREE]

(a) "call": encode_videos at 16 videos x 8 chunks and encode_streams at 8 blocks x 8 chunks with K = 4 instructions, the tokens
    held as fp32, fp16, bf16, fp8 e4m3 (torch.float8_e4m3fn: the caller's storage choice, quoted next to bf16 of the same run;
    --out profiles/vc_f8_tokens.jsonl), and as fp16 cast to fp32 inside every call (what a half-precision producer paid before).  Wall ms per
    call around a device synchronisation (median over all calls of all rounds), the library's launches per call, and the drop of
    torch.cuda.mem_get_info's free bytes over the first call (the library's workspaces are not torch's).
(b) "token_pass": the token pass alone through infv_vqf_token_pass with HIP events, 128 chunks, fp16 and bf16: infv_ltm_pool at the
    token dtype + the 64-token-tile pass without the means (what ships), and beside it a one-launch form with the means wherever
    the library has one for P = 196.  The committed line was taken with such a form (one workgroup per frame); it lost for both
    dtypes and was deleted, so a run on this tree times the two passes alone.
(c) "parent_vs_branch" (with --parent-tree: a checkout of the parent commit, built): encode_videos 16 x 8 on fp32 tokens, alternated
    child by child.  No existing kernel's source changed, so the branch's median must lie inside the spread of the parent's own
    round medians.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, P, D, N_TEXT, CHUNKS = 16, 196, 1024, 16, 8
KINDS = ("f32", "f16", "bf16", "f8", "f16_cast")
PASS_CHUNKS = 128


def child_call(a):
    sys.path.insert(0, a.root)
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.videochat2_qformer import NB_SAMPLES, VideoChat2Encoder, VideoChat2Memory
    dev = torch.device("cuda:0")
    m = VideoChat2Encoder(num_basis=64, sticky=True, tau=0.75, alpha=0.75)
    m.load_reference_state_dict(synth.videochat2_qformer_weights())
    m = m.to(dev).eval()
    n_cross = len(m.qformer.cross_layers)
    gen = torch.Generator(device=dev).manual_seed(1)
    streams = a.child == "streams"
    F, K = (8, 4) if streams else (16, 1)
    held = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn, "f16_cast": torch.float16}[a.kind]
    blocks = [torch.randn(CHUNKS, T * P, D, device=dev, generator=gen).to(held) for _ in range(F)]
    texts = [torch.randn(1, N_TEXT, 768, device=dev, generator=gen) for _ in range(K)]
    V = F * K
    src = [v % F for v in range(V)]
    te = [texts[v // F] for v in range(V)]
    u = torch.rand(V * CHUNKS, n_cross, NB_SAMPLES, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dev)
    mems = [VideoChat2Memory(m, dev) for _ in range(V)]
    lib = _lib.load()

    def fn():
        vids = [b.float() for b in blocks] if a.kind == "f16_cast" else blocks
        if streams:
            return m.encode_streams(vids, src, text_embeds=te, u=u, memories=mems)
        return m.encode_videos(vids, text_embeds=te, u=u, memories=mems)

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    out = fn()                                                  # warm-up: workspaces, plans, code objects
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    digest = float(out[1].double().sum())
    del out
    n0 = lib.infv_ltm_launch_count()
    fn()
    torch.cuda.synchronize()
    launches = lib.infv_ltm_launch_count() - n0
    ms = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({"ms": [round(x, 3) for x in ms], "launches": int(launches), "free_drop_bytes": int(free0 - free1),
                                  "frame_bytes_held": int(sum(b.numel() * b.element_size() for b in blocks)), "mean_digest": digest}), flush=True)


def child_pass(a):
    sys.path.insert(0, a.root)
    import torch
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = T * P
    res = {}
    for name, dtype, code in (("f16", torch.float16, 3), ("bf16", torch.bfloat16, 1)):
        x = torch.randn(PASS_CHUNKS, n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).to(dtype)
        planes = [torch.empty(PASS_CHUNKS * n * D, dtype=torch.bfloat16, device=dev) for _ in range(1 if code == 1 else 4)]
        Fh, Fl, Th, Tl = (None, None, planes[0], None) if code == 1 else planes
        kbar = torch.empty(PASS_CHUNKS, T, D, device=dev)
        kbar2 = torch.empty_like(kbar)
        eng = LTMEngine(64, 12, 64, D, P, 0.75, True, device=dev, fp16_tokens=True)
        _lib.check(lib.infv_ltm_set_token_dtype(eng._h, code))
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def one_pass():
            return lib.infv_vqf_token_pass(ptr(x), code, PASS_CHUNKS, n, D, P, ptr(Fh), ptr(Fl), ptr(Th), ptr(Tl), ptr(kbar), stream)

        have_one = one_pass() == 0                              # (-2: no one-launch form with the means for this P)

        def two_passes():
            _lib.check(lib.infv_ltm_pool(eng._h, ptr(x), PASS_CHUNKS * T, ptr(kbar2), stream))
            _lib.check(lib.infv_vqf_token_pass(ptr(x), code, PASS_CHUNKS, n, D, P, ptr(Fh), ptr(Fl), ptr(Th), ptr(Tl), None, stream))

        ms = {"one_pass": [], "two_passes": []}
        for rep in range(a.calls + 2):                          # alternated; the first two rounds warm up
            for key, fn in ((("one_pass", one_pass),) if have_one else ()) + (("two_passes", two_passes),):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    ms[key].append(e0.elapsed_time(e1))
        in_bytes = x.numel() * 2
        out_bytes = sum(p.numel() * 2 for p in planes) + kbar.numel() * 4
        r = res[name] = {"two_passes_ms": round(statistics.median(ms["two_passes"]), 4),
                         "two_passes_ms_min_max": [round(min(ms["two_passes"]), 4), round(max(ms["two_passes"]), 4)],
                         "two_passes_bytes": 2 * in_bytes + out_bytes, "timed_rounds": a.calls}
        r["two_passes_GBps"] = round(r["two_passes_bytes"] / r["two_passes_ms"] / 1e6, 1)
        if have_one:
            r.update(one_pass_ms=round(statistics.median(ms["one_pass"]), 4),
                     one_pass_ms_min_max=[round(min(ms["one_pass"]), 4), round(max(ms["one_pass"]), 4)],
                     one_pass_bytes=in_bytes + out_bytes, means_bit_equal=bool(torch.equal(kbar, kbar2)))
            r["one_pass_GBps"] = round(r["one_pass_bytes"] / r["one_pass_ms"] / 1e6, 1)
        del x, planes, kbar, kbar2, eng
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, root, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:                                      # a fault, an abort or a time limit: nothing more is started
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} ended with status {p.returncode}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"child {args} printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("videos", "streams", "pass"))
    ap.add_argument("--kind", choices=KINDS, default="f32")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=("call", "token_pass", "parent_vs_branch"), nargs="*")
    ap.add_argument("--sides", choices=("videos", "streams"), nargs="*", default=("videos", "streams"), help="which calls the \"call\" measure times")
    ap.add_argument("--parent-tree", metavar="TREE")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vc_half_tokens.jsonl"))
    a = ap.parse_args()
    if a.child == "pass":
        return child_pass(a)
    if a.child:
        return child_call(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    shape = {"T": T, "P": P, "width": D, "N": 64, "Q": 96, "layers": 12, "alpha": 0.75, "text_tokens": N_TEXT, "proj": 4096,
             "chunks_per_block": CHUNKS}
    want = set(a.only or ("call", "token_pass", "parent_vs_branch"))

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    if "token_pass" in want:
        res = run_child(["--child", "pass", "--calls", str(max(a.calls, 10))], ROOT, a.child_timeout)
        emit(dict(measure="token_pass", T=T, P=P, width=D, chunks=PASS_CHUNKS, timing="HIP events", **res))
    if "call" in want:
        for side in a.sides:
            per, last = {k: [] for k in KINDS}, {}
            for r in range(a.rounds):
                for kind in KINDS:                              # alternated child by child, so that drift hits all alike
                    res = run_child(["--child", side, "--kind", kind, "--calls", str(a.calls)], ROOT, a.child_timeout)
                    per[kind] += res["ms"]
                    last[kind] = res
            line = dict(shape, measure="call", call="encode_" + side, blocks=8 if side == "streams" else 16, k=4 if side == "streams" else 1,
                        rounds=a.rounds, timed_calls_per_kind=a.rounds * a.calls)
            for kind in KINDS:
                line[kind] = {"ms": round(statistics.median(per[kind]), 2), "ms_min_max": [round(min(per[kind]), 2), round(max(per[kind]), 2)],
                              "launches": last[kind]["launches"], "free_drop_bytes": last[kind]["free_drop_bytes"],
                              "frame_bytes_held": last[kind]["frame_bytes_held"]}
            line["f16_equals_f16_cast"] = last["f16"]["mean_digest"] == last["f16_cast"]["mean_digest"]
            emit(line)
    if "parent_vs_branch" in want and a.parent_tree:
        meds = {"parent": [], "branch": []}
        launches = {}
        for r in range(max(a.rounds, 3)):
            for name, root in (("parent", os.path.abspath(a.parent_tree)), ("branch", ROOT)):
                res = run_child(["--child", "videos", "--kind", "f32", "--calls", str(a.calls)], root, a.child_timeout)
                meds[name].append(statistics.median(res["ms"]))
                launches[name] = res["launches"]
        mp, mb = statistics.median(meds["parent"]), statistics.median(meds["branch"])
        line = dict(shape, measure="parent_vs_branch", call="encode_videos", tokens="fp32", videos=16, chunks=16 * CHUNKS,
                    rounds=len(meds["parent"]), calls_per_round=a.calls,
                    parent_ms=round(mp, 2), parent_round_medians=[round(x, 2) for x in meds["parent"]],
                    branch_ms=round(mb, 2), branch_round_medians=[round(x, 2) for x in meds["branch"]],
                    branch_minus_parent_ms=round(mb - mp, 2), launches_per_call={k: int(v) for k, v in launches.items()})
        line["inside_parent_spread"] = bool(min(meds["parent"]) <= mb <= max(meds["parent"]))
        emit(line)


if __name__ == "__main__":
    main()
