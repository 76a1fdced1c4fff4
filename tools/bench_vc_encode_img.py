"""encode_img from the vision encoder's fp16 output and the tokenizer's ids, at the eval shape of the reference's VideoChat2 drivers
(T 16, P 196, width 1024, 16 videos x 8 chunks, 16 instruction tokens, N 64, 96 query tokens, 12 layers, alpha 0.75, sticky,
mistral_proj 4096).  Three legs over the same values, each in fresh child processes, one GPU process at a time, alternated round by
round; a child warms up once and times `--calls` calls.  One JSON line each, appended to profiles/vc_encode_img.jsonl:

    timeout -k 10 1100 python tools/bench_vc_encode_img.py [--parent-tree TREE]

  (a) "torch"     what a caller did before: torch's layer_norm under fp16 autocast (an fp32 tensor, videochat2_it_mistral.py:195) +
                  the embedding layer in torch (Qformer.py:54-111) + encode_videos
  (b) "two_step"  the library's two-step form: vision_tokens_layernorm (ln_tokens_kernel into an fp32 copy) + embed_instructions +
                  encode_videos on the copy
  (c) "fused"     encode_img_videos: the LayerNorm inside the token pass, the embedding layer inside the call, no fp32 copy

Per leg: wall ms per call around a device synchronisation (the median of every round and their spread), the drop of
torch.cuda.mem_get_info's free bytes over the first call (the library's workspaces are not torch's) and the library's launches per
call.  (b) and (c) must give the same bits (the digest of the per-video means is compared); (c) ships as encode_img_videos if its
median lies inside or below the spread of (b)'s round medians.
"parent_vs_branch" (with --parent-tree: a checkout of the parent commit, built): the map-less encode_videos on fp32 tokens, alternated
child by child -- the branch's median must lie inside the spread of the parent's own round medians.
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
T, P, D, N_TEXT, CHUNKS, VIDEOS = 16, 196, 1024, 16, 8, 16
VOCAB, MAX_POS = 30522, 512
LEGS = ("torch", "two_step", "fused")


def child(a):
    sys.path.insert(0, a.root)
    import torch
    import torch.nn.functional as F
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.videochat2_qformer import NB_SAMPLES, VideoChat2Encoder, VideoChat2Memory
    dev = torch.device("cuda:0")
    front = a.leg != "parent"                                   # (the parent commit has no such arguments)
    kw = dict(vocab_size=VOCAB, max_position_embeddings=MAX_POS, vision_layernorm=True) if front else {}
    torch.manual_seed(4)
    m = VideoChat2Encoder(num_basis=64, sticky=True, tau=0.75, alpha=0.75, **kw)
    m.load_reference_state_dict(synth.videochat2_qformer_weights(), strict=False)
    if front:
        with torch.no_grad():
            m.vision_layernorm.weight.normal_(1.0, 0.1)
            m.vision_layernorm.bias.normal_(0.0, 0.1)
            m.qformer.bert.embeddings.word_embeddings.weight.mul_(0.02)
            m.qformer.bert.embeddings.position_embeddings.weight.mul_(0.02)
    m = m.to(dev).eval()
    n_cross = len(m.qformer.cross_layers)
    gen = torch.Generator(device=dev).manual_seed(1)
    held = torch.float32 if a.leg == "parent" else torch.float16
    blocks = [(torch.randn(CHUNKS, T * P, D, device=dev, generator=gen) * 3 + 0.5).to(held) for _ in range(VIDEOS)]
    ids = [torch.randint(0, VOCAB, (N_TEXT,), generator=torch.Generator().manual_seed(10 + v)) for v in range(VIDEOS)]
    text = torch.randn(1, N_TEXT, 768, device=dev, generator=gen)
    u = torch.rand(VIDEOS * CHUNKS, n_cross, NB_SAMPLES, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dev)
    mems = [VideoChat2Memory(m, dev) for _ in range(VIDEOS)]
    lib = _lib.load()

    def fn():
        if a.leg == "parent":
            return m.encode_videos(blocks, text_embeds=text, u=u, memories=mems)
        if a.leg == "fused":
            return m.encode_img_videos(blocks, input_ids=ids, u=u, memories=mems)
        if a.leg == "two_step":
            return m.encode_videos([m.vision_tokens_layernorm(b) for b in blocks], hidden_in=m.embed_instructions(ids, device=dev), u=u,
                                   memories=mems)
        ln, e = m.vision_layernorm, m.qformer.bert.embeddings
        with torch.no_grad():
            with torch.autocast("cuda", dtype=torch.float16):
                normed = [F.layer_norm(b, (D,), ln.weight, ln.bias, ln.eps) for b in blocks]
            assert normed[0].dtype == torch.float32                 # autocast runs layer_norm in fp32
            pos = e.position_embeddings.weight[:N_TEXT]
            rows = [e.LayerNorm(torch.cat([m.query_tokens[0], e.word_embeddings(i.to(dev)) + pos], 0)) for i in ids]
        return m.encode_videos(normed, hidden_in=rows, u=u, memories=mems)

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


def run_child(args, root, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:                                      # a fault, an abort or a time limit: nothing more is started
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} ended with status {p.returncode}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
            print(f"# {' '.join(args)} ({os.path.basename(root)}): median {statistics.median(res['ms']):.2f} ms", file=sys.stderr, flush=True)
            return res
    raise SystemExit(f"child {args} printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS + ("parent",))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("legs", "parent_vs_branch"), nargs="*")
    ap.add_argument("--parent-tree", metavar="TREE")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vc_encode_img.jsonl"))
    a = ap.parse_args()
    if a.leg:
        return child(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    shape = {"T": T, "P": P, "width": D, "N": 64, "Q": 96, "layers": 12, "alpha": 0.75, "text_tokens": N_TEXT, "proj": 4096,
             "videos": VIDEOS, "chunks_per_video": CHUNKS, "vision_output": "fp16"}
    want = set(a.only or ("legs", "parent_vs_branch"))

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    if "legs" in want:
        meds, last = {k: [] for k in LEGS}, {}
        for r in range(a.rounds):
            for leg in LEGS:                                    # alternated child by child, so that drift hits all alike
                res = run_child(["--leg", leg, "--calls", str(a.calls)], ROOT, a.child_timeout)
                meds[leg].append(statistics.median(res["ms"]))
                last[leg] = res
        line = dict(shape, measure="legs", rounds=a.rounds, calls_per_round=a.calls)
        for leg in LEGS:
            line[leg] = {"ms": round(statistics.median(meds[leg]), 2), "round_medians": [round(x, 2) for x in meds[leg]],
                         "launches": last[leg]["launches"], "free_drop_bytes": last[leg]["free_drop_bytes"],
                         "frame_bytes_held": last[leg]["frame_bytes_held"]}
        line["fused_equals_two_step"] = last["fused"]["mean_digest"] == last["two_step"]["mean_digest"]
        line["torch_digest_rel_diff"] = abs(last["torch"]["mean_digest"] - last["fused"]["mean_digest"]) / max(abs(last["torch"]["mean_digest"]), 1e-30)
        line["fused_inside_or_below_two_step_spread"] = bool(line["fused"]["ms"] <= max(meds["two_step"]))
        emit(line)
    if "parent_vs_branch" in want and a.parent_tree:
        meds, launches = {"parent": [], "branch": []}, {}
        for r in range(max(a.rounds, 3)):
            for name, root in (("parent", os.path.abspath(a.parent_tree)), ("branch", ROOT)):
                res = run_child(["--leg", "parent", "--calls", str(a.calls)], root, a.child_timeout)
                meds[name].append(statistics.median(res["ms"]))
                launches[name] = res["launches"]
        mp, mb = statistics.median(meds["parent"]), statistics.median(meds["branch"])
        line = dict(shape, measure="parent_vs_branch", call="encode_videos", tokens="fp32", rounds=len(meds["parent"]),
                    calls_per_round=a.calls, parent_ms=round(mp, 2), parent_round_medians=[round(x, 2) for x in meds["parent"]],
                    branch_ms=round(mb, 2), branch_round_medians=[round(x, 2) for x in meds["branch"]],
                    branch_minus_parent_ms=round(mb - mp, 2), launches_per_call={k: int(v) for k, v in launches.items()})
        line["inside_parent_spread"] = bool(min(meds["parent"]) <= mb <= max(meds["parent"]))
        emit(line)


if __name__ == "__main__":
    main()
