"""infv_ltm_consolidate on the 2048-chunk headline video (T 256, P 32, d 768, N 256, 2 layers, Q 32, sticky) with fp32, bf16,
fp16 and fp8 e4m3 frame tokens: 51.5 GB of tokens at fp32, 25.8 GB at either half format, 12.9 GB at one byte per element.

One CHILD PROCESS per leg and round (a fresh HIP context, the tokens of that dtype only), the legs ALTERNATED within a round
(fp32 bf16 fp16 fp8, fp32 bf16 fp16 fp8, ...), at least five rounds.  A child warms the call, times `--reps` calls with device events
and reports their median; it also reports the pooling launch alone (infv_ltm_pool_rows on the first 512 chunks, device time from
infv_ltm_profile_*), which is the kernel that reads the tokens.

    timeout -k 10 1100 python tools/bench_token_dtypes.py --rounds 5

fp16 moves bf16's bytes through the same loads, so the yardstick for fp16 is the bf16 leg of the same run on the same box: the
summary line states whether fp16's median (over the rounds' medians) exceeds bf16's by more than the spread (max - min) of bf16's
own per-round medians.  fp8 (torch.float8_e4m3fn, the caller's storage choice) is quoted next to the bf16 leg of the same run too,
with the free device memory the first call of each leg took.  One JSON line per child and one summary line are appended to
profiles/f8_tokens.jsonl (--out).

--parent-lib PATH (a libinfv_ltm.so built from the parent commit) runs the fp32 leg alone, alternated between that library and this
tree's: no existing kernel's source changed, so the branch's median must lie inside the spread of the parent's own round medians.

    timeout -k 10 600 python tools/bench_token_dtypes.py --parent-lib PATH --out profiles/f8_tokens_parent_vs_branch.jsonl"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, P, D, N, L, Q = 256, 32, 768, 256, 2, 32
LEGS = ("float32", "bfloat16", "float16", "float8_e4m3fn")


def child(dtype_name: str, chunks: int, reps: int):
    import numpy as np
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine
    dev = torch.device("cuda:0")
    dtype = getattr(torch, dtype_name)
    gen = torch.Generator(device=dev).manual_seed(1)
    k = torch.empty(chunks, T * P, D, device=dev, dtype=dtype)
    for c0 in range(0, chunks, 32):                                # (no fp32 tensor of the whole video beside k)
        k[c0:c0 + 32] = torch.randn(min(32, chunks - c0), T * P, D, device=dev, generator=gen).to(dtype)
    u = torch.rand(chunks, L, 512, device=dev, dtype=torch.float64, generator=gen)
    projs = [tuple(torch.from_numpy(x).to(dev) for x in synth.layer_projections(l, D, 768)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, 768) for l in range(L)])).to(dev)
    eng = LTMEngine(N, 12, 64, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev,
                    fp16_tokens=dtype == torch.float16)          # (fp16 tensors are opt-in on an engine's tensor methods)
    out = torch.empty(chunks, L, Q, 768, device=dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    eng.consolidate(k, q, projs, u, new_doc=True, out=out)        # warm-up: plans, workspaces (the library's are not torch's)
    torch.cuda.synchronize()
    first_call_bytes = free0 - torch.cuda.mem_get_info(dev)[0]
    eng.consolidate(k, q, projs, u, new_doc=True, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.consolidate(k, q, projs, u, new_doc=True, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    # the pooling launch alone: pool + rows of the first 512 chunks, nothing beside it on the chip
    n_alone = min(512, chunks)
    eng.pool_rows(k[:n_alone])
    torch.cuda.synchronize()
    eng.profile(True)
    alone = []
    for _ in range(reps):
        eng.pool_rows(k[:n_alone])
        n, t = eng.profile_read()["pool"]
        alone.append(t / max(n, 1))
    eng.profile(False)
    med = statistics.median(ms)
    tok_bytes = k.numel() * k.element_size()
    alone_med = statistics.median(alone)
    print(json.dumps({"leg": dtype_name, "chunks": chunks, "reps": reps, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "chunks_per_s": round(chunks / med * 1e3, 1), "token_bytes": tok_bytes,
                      "first_call_free_drop_bytes": int(first_call_bytes), "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
                      "pool_rows_alone_chunks": n_alone, "pool_rows_alone_ms": round(alone_med, 3),
                      "pool_rows_alone_GBps": round(tok_bytes * n_alone / chunks / alone_med / 1e6, 1),
                      "checksum": float(out.double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunks", type=int, default=2048)
    ap.add_argument("--child", choices=LEGS)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-lib", metavar="PATH", help="fp32 leg alone, alternated between this build of the parent commit and this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f8_tokens.jsonl"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.chunks, a.reps)
    if a.rounds < 5:
        ap.error("at least five rounds")

    def run_child(leg, rnd, library=None):
        env = dict(os.environ)
        if library:
            env["INFV_LTM_LIBRARY"] = os.path.abspath(library)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--chunks", str(a.chunks), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=a.child_timeout, cwd=ROOT, env=env)
        if r.returncode != 0:                                      # stop here: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child {leg} of round {rnd} ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().split("\n")[-1])
        line["round"] = rnd
        return line

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.parent_lib:
        lines = []
        for rnd in range(a.rounds):
            for side, library in (("parent", a.parent_lib), ("branch", None)):     # alternated child by child
                line = dict(run_child("float32", rnd, library), side=side)
                print(json.dumps(line), flush=True)
                lines.append(line)
        per = {side: [l["median_ms"] for l in lines if l["side"] == side] for side in ("parent", "branch")}
        mp, mb = statistics.median(per["parent"]), statistics.median(per["branch"])
        summary = {"summary": True, "measure": "parent_vs_branch", "leg": "float32", "chunks": a.chunks, "rounds": a.rounds,
                   "reps_per_child": a.reps, "parent_ms": round(mp, 3), "branch_ms": round(mb, 3), "round_medians_ms": per,
                   "branch_minus_parent_ms": round(mb - mp, 3), "parent_spread_ms": round(max(per["parent"]) - min(per["parent"]), 3),
                   "inside_parent_spread": bool(min(per["parent"]) <= mb <= max(per["parent"])),
                   "same_checksum": len({l["checksum"] for l in lines}) == 1}
        print(json.dumps(summary), flush=True)
        with open(a.out, "a") as f:
            for l in lines + [summary]:
                f.write(json.dumps(l) + "\n")
        return
    lines = []
    for rnd in range(a.rounds):
        for leg in LEGS:                                           # alternated: one fresh process per leg and round, one at a time
            line = run_child(leg, rnd)
            print(json.dumps(line), flush=True)
            lines.append(line)
    per = {leg: [l["median_ms"] for l in lines if l["leg"] == leg] for leg in LEGS}
    alone = {leg: [l["pool_rows_alone_ms"] for l in lines if l["leg"] == leg] for leg in LEGS}
    med = {leg: statistics.median(v) for leg, v in per.items()}
    spread_bf16 = max(per["bfloat16"]) - min(per["bfloat16"])
    summary = {"summary": True, "chunks": a.chunks, "rounds": a.rounds, "reps_per_child": a.reps,
               "median_of_round_medians_ms": {k: round(v, 3) for k, v in med.items()},
               "chunks_per_s": {k: round(a.chunks / v * 1e3, 1) for k, v in med.items()},
               "round_medians_ms": per,
               "bf16_spread_ms": round(spread_bf16, 3),
               "fp16_minus_bf16_ms": round(med["float16"] - med["bfloat16"], 3),
               "fp16_within_bf16_spread": bool(med["float16"] - med["bfloat16"] <= spread_bf16),
               "fp8_minus_bf16_ms": round(med["float8_e4m3fn"] - med["bfloat16"], 3),
               "pool_rows_alone_ms": {k: round(statistics.median(v), 3) for k, v in alone.items()},
               "fp8_pool_rows_alone_faster_than_bf16": bool(statistics.median(alone["float8_e4m3fn"]) < statistics.median(alone["bfloat16"])),
               "first_call_free_drop_bytes": {leg: [l["first_call_free_drop_bytes"] for l in lines if l["leg"] == leg][-1] for leg in LEGS},
               "token_bytes": {leg: [l["token_bytes"] for l in lines if l["leg"] == leg][-1] for leg in LEGS},
               "same_checksum_fp16_rounds": len({l["checksum"] for l in lines if l["leg"] == "float16"}) == 1}
    print(json.dumps(summary), flush=True)
    with open(a.out, "a") as f:
        for l in lines + [summary]:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
