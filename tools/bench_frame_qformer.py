"""The per-frame image Q-former (``encode_short_memory_frame`` after the vision encoder) on the HIP path against plain PyTorch, at
the reference's shape: F = 256 frames x 257 tokens x 1408 (fp16 vision output), bert-base with 12 layers, 32 query tokens.

    timeout -k 10 900 python tools/bench_frame_qformer.py

Two legs, each in fresh child processes, one GPU process at a time, alternated round by round; a child warms up once and times
``--calls`` calls around a device synchronisation.  The parent stops at the first child that ends abnormally or runs out of time.

(a) "torch": a plain torch forward of the same parameter tree under fp16 autocast -- ``ln_vision``, the embeddings LayerNorm, twelve
    BertLayers with a cross-attention in every second one -- whose rows are appended to a Python list frame by frame, as the
    reference fills ``short_memory_buffer`` (infinityqa.py:259-278).
(b) "hip": ``FrameQformerEncoder.encode_short_memory_frame`` into an fp16 ``ShortMemoryBuffer`` (``infv_vqf_encode_frames``: the
    LayerNorm on load, planes padded from 257 to 320 tokens, the last layer writing fp16 rows into the buffer).

One JSON line, appended to profiles/frame_qformer.jsonl: per leg the median of the round medians (ms per call), the round medians,
the drop of ``torch.cuda.mem_get_info``'s free bytes over the first call, the library's launches per call (``infv_ltm_launch_count``),
and the largest difference between the two legs' frame tokens.

``--linear-precision fp32,split_bf16,fp16`` runs one "hip" leg per arithmetic of the query-side linears
(``FrameQformerEncoder.set_linear_precision``) beside the torch leg, and adds each leg's ratio to torch and to the fp32 leg; the drop
of free device memory over a leg's first call then includes its weight planes.  ``--parent-root DIR`` adds a leg that runs the fp32
path of another build of the library (a checkout with its own ``libinfv_ltm.so``), alternated with the others: the parent-against-
branch comparison.  ``--attention-precision fp32,fp16`` multiplies the hip legs: one per (linear, attention) pair asked for
(``FrameQformerEncoder.set_attention_precision``; a leg with the fp16 attention is named ``hip_<linear>_attn_fp16`` and its memory drop
includes the fp16 token planes).  Any of these options needs ``--out``: the default file keeps the two-leg lines.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, TOKENS, WIDTH = 256, 257, 1408


def torch_forward(m, x):
    """The image Q-former of ``m`` in stock PyTorch (all-ones masks, eval mode, no long-term memory) -> [F, Q, hidden]."""
    import torch
    import torch.nn.functional as F
    cfg = m.config
    H, dh = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    heads = lambda t: t.view(t.size(0), t.size(1), H, dh).permute(0, 2, 1, 3)

    def attend(att, q_in, kv_in):
        q, k, v = heads(att.query(q_in)), heads(att.key(kv_in)), heads(att.value(kv_in))
        p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh), dim=-1)
        return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(q_in.size(0), q_in.size(1), H * dh)

    k = m.ln_vision(x)
    h = m.Qformer.bert.embeddings.LayerNorm(m.query_tokens).expand(x.size(0), -1, -1)
    for layer in m.Qformer.bert.encoder.layer:
        a = layer.attention
        h = a.output(attend(a.self, h, h), h)
        if layer.has_cross_attention:
            c = layer.crossattention
            h = c.output(attend(c.self, h, k), h)
        h = layer.output_query(layer.intermediate_query(h), h)
    return h


def child(a):
    sys.path.insert(0, a.root)
    import torch
    from infinite_video_amd import _lib
    from infinite_video_amd.frame_qformer import FrameQformerEncoder
    from infinite_video_amd.video_qformer import ShortMemoryBuffer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = FrameQformerEncoder().to(dev).eval()
    if a.precision != "fp32":                                          # (a parent build has no such method and is never asked)
        m.set_linear_precision(a.precision)
    if a.attention != "fp32":
        m.set_attention_precision(a.attention)
    for p in m.parameters():
        p.requires_grad = False
    x = torch.randn(a.frames, TOKENS, WIDTH, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).half()
    lib = _lib.load()
    buf = ShortMemoryBuffer(m.n_query, m.config.hidden_size, capacity_frames=2049, dtype=torch.float16, device=dev)

    def leg_torch():
        short_memory_buffer = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            q_hidden_state = torch_forward(m, x)
        for cur_frame, frame in enumerate(q_hidden_state, 1):          # infinityqa.py:272-277
            if cur_frame <= 2048:
                short_memory_buffer.append(frame)
        return short_memory_buffer

    def leg_hip():
        return m.encode_short_memory_frame(x, buf)

    fn = leg_torch if a.child == "torch" else leg_hip
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    out = fn()                                                         # warm-up: workspaces, code objects, tuned GEMMs
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    res = {"free_drop_bytes": int(free0 - free1)}
    if a.child == "hip":                                               # (the other leg's rows, once: how far apart the two are)
        ref = torch.stack(leg_torch()).float()
        res["max_abs_diff_to_torch_leg"] = float((buf.store[:len(buf)].float() - ref).abs().max())
        del ref
    del out
    n0 = lib.infv_ltm_launch_count()
    fn()
    torch.cuda.synchronize()
    res["launches"] = int(lib.infv_ltm_launch_count() - n0)
    ms = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    res["ms"] = [round(v, 3) for v in ms]
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", ROOT] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:                                              # a fault, an abort or a time limit: nothing more is started
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} ended with status {p.returncode}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"child {args} printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("torch", "hip"))
    ap.add_argument("--precision", default="fp32", help="(child) linear precision of the hip leg")
    ap.add_argument("--attention", default="fp32", help="(child) attention precision of the hip leg")
    ap.add_argument("--attention-precision", default="", help="comma-separated: the hip legs run per (linear, attention) pair (fp32, fp16)")
    ap.add_argument("--linear-precision", default="", help="comma-separated: one hip leg per name (fp32, split_bf16, fp16)")
    ap.add_argument("--parent-root", default="", help="a checkout of another build: one more fp32 hip leg from there")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_qformer.jsonl"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.linear_precision or a.attention_precision or a.parent_root:
        return main_legs(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    meds, last = {"torch": [], "hip": []}, {}
    for _ in range(a.rounds):
        for leg in ("torch", "hip"):                                   # alternated child by child, so that drift hits both alike
            res = run_child(["--child", leg, "--frames", str(a.frames), "--calls", str(a.calls)], a.child_timeout)
            meds[leg].append(statistics.median(res["ms"]))
            last[leg] = res
    line = {"measure": "encode_short_memory_frame", "frames": a.frames, "tokens": TOKENS, "width": WIDTH, "vision_dtype": "fp16",
            "layers": 12, "queries": 32, "hidden": 768, "buffer_dtype": "fp16", "rounds": a.rounds, "calls_per_round": a.calls}
    for leg in ("torch", "hip"):
        line[leg] = {"ms": round(statistics.median(meds[leg]), 3), "round_medians_ms": [round(v, 3) for v in meds[leg]],
                     "free_drop_bytes": last[leg]["free_drop_bytes"], "launches": last[leg]["launches"]}
    line["hip"]["max_abs_diff_to_torch_leg"] = last["hip"]["max_abs_diff_to_torch_leg"]
    line["torch_over_hip"] = round(line["torch"]["ms"] / line["hip"]["ms"], 3)
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main_legs(a):
    """torch, one hip leg per (linear, attention) precision pair, and the parent build's fp32 leg, alternated child by child."""
    if os.path.abspath(a.out) == os.path.join(ROOT, "profiles", "frame_qformer.jsonl"):
        raise SystemExit("--linear-precision / --attention-precision / --parent-root need --out (profiles/frame_qformer.jsonl keeps the two-leg lines)")
    names = [n for n in a.linear_precision.split(",") if n] or ["fp32"]
    legs = {"torch": ["--child", "torch"]}
    for n in names:
        for att in [t for t in a.attention_precision.split(",") if t] or ["fp32"]:
            legs["hip_" + n + ("" if att == "fp32" else "_attn_" + att)] = ["--child", "hip", "--precision", n, "--attention", att]
    if a.parent_root:
        legs["parent_fp32"] = ["--root", os.path.abspath(a.parent_root), "--child", "hip"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    meds, last = {k: [] for k in legs}, {}
    for _ in range(a.rounds):
        for leg, args in legs.items():
            res = run_child(args + ["--frames", str(a.frames), "--calls", str(a.calls)], a.child_timeout)
            meds[leg].append(statistics.median(res["ms"]))
            last[leg] = res
    line = {"measure": "encode_short_memory_frame", "frames": a.frames, "tokens": TOKENS, "width": WIDTH, "vision_dtype": "fp16",
            "layers": 12, "queries": 32, "hidden": 768, "buffer_dtype": "fp16", "rounds": a.rounds, "calls_per_round": a.calls}
    for leg in legs:
        line[leg] = {"ms": round(statistics.median(meds[leg]), 3), "round_medians_ms": [round(v, 3) for v in meds[leg]],
                     "free_drop_bytes": last[leg]["free_drop_bytes"], "launches": last[leg]["launches"]}
        if "max_abs_diff_to_torch_leg" in last[leg]:
            line[leg]["max_abs_diff_to_torch_leg"] = last[leg]["max_abs_diff_to_torch_leg"]
    for leg in legs:
        if leg != "torch":
            line[leg]["over_torch"] = round(line[leg]["ms"] / line["torch"]["ms"], 3)
            if "hip_fp32" in line and leg != "hip_fp32":
                line[leg]["over_hip_fp32"] = round(line[leg]["ms"] / line["hip_fp32"]["ms"], 3)
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
