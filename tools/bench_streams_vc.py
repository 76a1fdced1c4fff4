"""K instructions per video over ONE copy of its frame tokens (VideoChat2Encoder.encode_streams) against the existing path,
encode_videos with every video passed K times, at the eval shape of the reference's VideoChat2 drivers (T 16, P 196, width
1024, N 64, 96 query tokens, 12 layers, alpha 0.75, sticky, mistral_proj 4096): 8 blocks x 8 chunks, K = 1, 4, 8 instructions
of 16 tokens per block, grouped by instruction (stream v reads block v % 8).  Every (side, K) runs in child processes of its
own, the two sides alternated round by round; a child warms up once and times `--calls` calls, wall time around a device
synchronisation.  Per side: ms per call (median over all calls of all rounds), the library's launches per call and the drop of
torch.cuda.mem_get_info's free bytes over the first call (the library's workspaces are not torch's; the drop also holds the
call's own torch tensors: the packed copy of the frames it is handed and its outputs).  Both sides get the same explicit
uniforms, and the child of the streams side checks its projected rows against the replicated call bit for bit (`--check`, K = 4
in the last round only: it holds both sides' memory).  One JSON line per K, appended to profiles/vc_streams_bench.jsonl:

    timeout -k 10 1100 python tools/bench_streams_vc.py

`--parent-vs-branch TREE` instead times encode_videos at 16 videos x 8 chunks on the package under TREE (a checkout of the
parent commit, built) and on this one, alternated child by child, and writes profiles/vc_streams_parent_vs_branch.jsonl: the
map-less path must not have moved, so the difference of the medians is set beside the spread of the parent's own medians.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, P, D, N_TEXT, BLOCKS, CHUNKS = 16, 196, 1024, 16, 8, 8
KS = (1, 4, 8)


def child(a):
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
    F = 16 if a.child == "videos16" else BLOCKS
    K = 1 if a.child == "videos16" else a.k
    blocks = [torch.randn(CHUNKS, T * P, D, device=dev, generator=gen) for _ in range(F)]
    texts = [torch.randn(1, N_TEXT, 768, device=dev, generator=gen) for _ in range(K)]
    V = F * K
    src = [v % F for v in range(V)]                             # grouped by instruction: the streams of a block are F apart
    te = [texts[v // F] for v in range(V)]
    u = torch.rand(V * CHUNKS, n_cross, NB_SAMPLES, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dev)
    mems = [VideoChat2Memory(m, dev) for _ in range(V)]
    lib = _lib.load()

    def streams():
        return m.encode_streams(blocks, src, text_embeds=te, u=u, memories=mems)

    def videos():                                               # the existing path: every video handed in K times
        return m.encode_videos([blocks[s] for s in src], text_embeds=te, u=u, memories=mems)

    fn = streams if a.child == "streams" else videos
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    out = fn()                                                  # warm-up: workspaces, plans, code objects
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
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
    res = {"side": a.child, "k": K, "ms": [round(x, 3) for x in ms], "launches": int(launches), "free_drop_bytes": int(free0 - free1),
           "frame_bytes_handed_in": int(sum(blocks[s].numel() for s in (src if a.child != "streams" else range(F))) * 4)}
    if a.check and a.child == "streams":
        want = videos()
        torch.cuda.synchronize()
        res["bit_equal_to_replicated"] = bool(torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]))
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


def summary(ms):
    return {"ms": round(statistics.median(ms), 2), "ms_min_max": [round(min(ms), 2), round(max(ms), 2)], "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("streams", "videos", "videos16"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--parent-vs-branch", metavar="TREE")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a)
    shape = {"T": T, "P": P, "width": D, "N": 64, "Q": 96, "layers": 12, "alpha": 0.75, "text_tokens": N_TEXT, "proj": 4096,
             "chunks_per_block": CHUNKS}
    if a.parent_vs_branch:
        out = a.out or os.path.join(ROOT, "profiles", "vc_streams_parent_vs_branch.jsonl")
        meds = {"parent": [], "branch": []}
        launches = {}
        for r in range(a.rounds):                               # alternated child by child, so that drift hits both alike
            for name, root in (("parent", os.path.abspath(a.parent_vs_branch)), ("branch", ROOT)):
                res = run_child(["--child", "videos16", "--calls", str(a.calls)], root, a.child_timeout)
                meds[name].append(statistics.median(res["ms"]))
                launches[name] = res["launches"]
        mp, mb = statistics.median(meds["parent"]), statistics.median(meds["branch"])
        line = dict(shape, call="encode_videos", videos=16, chunks=16 * CHUNKS, rounds=a.rounds, calls_per_round=a.calls,
                    parent_ms=round(mp, 2), parent_round_medians=[round(x, 2) for x in meds["parent"]],
                    branch_ms=round(mb, 2), branch_round_medians=[round(x, 2) for x in meds["branch"]],
                    branch_minus_parent_ms=round(mb - mp, 2),
                    parent_spread_ms=round(max(meds["parent"]) - min(meds["parent"]), 2),
                    launches_per_call={k: int(v) for k, v in launches.items()})
        line["inside_parent_spread"] = bool(abs(mb - mp) <= line["parent_spread_ms"])
    else:
        out = a.out or os.path.join(ROOT, "profiles", "vc_streams_bench.jsonl")
        line = None
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if line is not None:
        print(json.dumps(line), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
        return
    for k in a.ks:
        per = {"streams": [], "videos": []}
        last = {}
        for r in range(a.rounds):
            for side in ("streams", "videos"):
                args = ["--child", side, "--k", str(k), "--calls", str(a.calls)]
                if side == "streams" and k == 4 and r == a.rounds - 1:
                    args.append("--check")
                res = run_child(args, ROOT, a.child_timeout)
                per[side] += res["ms"]
                last[side] = res
        s, v = summary(per["streams"]), summary(per["videos"])
        line = dict(shape, blocks=BLOCKS, k=k, streams=BLOCKS * k, stream_chunks=BLOCKS * k * CHUNKS, distinct_chunks=BLOCKS * CHUNKS,
                    rounds=a.rounds,
                    streams_ms=s["ms"], streams_ms_min_max=s["ms_min_max"], replicated_ms=v["ms"], replicated_ms_min_max=v["ms_min_max"],
                    replicated_over_streams=round(v["ms"] / s["ms"], 3), timed_calls_per_side=s["calls"],
                    launches_per_call_streams=last["streams"]["launches"], launches_per_call_replicated=last["videos"]["launches"],
                    free_drop_bytes_streams=last["streams"]["free_drop_bytes"], free_drop_bytes_replicated=last["videos"]["free_drop_bytes"],
                    frame_bytes_handed_in_streams=last["streams"]["frame_bytes_handed_in"],
                    frame_bytes_handed_in_replicated=last["videos"]["frame_bytes_handed_in"])
        if "bit_equal_to_replicated" in last["streams"]:
            line["bit_equal_to_replicated"] = last["streams"]["bit_equal_to_replicated"]
        print(json.dumps(line), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
