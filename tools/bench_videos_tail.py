"""Videos whose last chunk is short through ONE lockstep call (engine.consolidate_videos_frames, infv_ltm_videos_tail) against what
a caller had to do before it: ``consolidate_videos`` on the full chunks, then every short last chunk through its own engine's
``consolidate``.  Headline chunk shape (T 256, N 256, L 2, Q 32, fp32 tokens); two mixes: 256 videos of 7 full chunks plus a tail
drawn uniformly from 2..255 frames, and 64 videos of 31 full chunks plus such a tail.

One CHILD PROCESS per leg, mix and round (a fresh HIP context), the legs ALTERNATED within a round, three rounds by default.  A
child warms its leg once (plans, workspaces), times ``--reps`` calls with device events and reports their median and the kernel
launches of one call.  One JSON line per child and one summary line per mix (time per call, launches per call, the spread of the
round medians of each leg) are appended to profiles/videos_tail.jsonl (--out):

    timeout -k 10 1100 python tools/bench_videos_tail.py

--parent-lib PATH (a libinfv_ltm.so built from the parent commit) times the EXISTING ``consolidate_videos`` at 256 x 8 alternated
between that library and this tree's: no existing kernel changed, so the branch's median must lie inside the spread of the
parent's own round medians.

    timeout -k 10 600 python tools/bench_videos_tail.py --parent-lib PATH"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, P, D, N, L, Q, S = 256, 32, 768, 256, 2, 32, 512
MIXES = {"256x7+tail": (256, 7), "64x31+tail": (64, 31)}
LEGS = ("one_call", "full_then_tails")


def child(leg: str, mix: str, reps: int):
    import ctypes as C
    import numpy as np
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine, consolidate_videos, consolidate_videos_frames
    dev = torch.device("cuda:0")
    if leg == "parent_check" and not hasattr(C.CDLL(_lib.LIB_PATH), "infv_ltm_videos_tail"):
        _lib._SIGNATURES.pop("infv_ltm_videos_tail")               # a build of the parent commit: the leg does not call the new symbol
    lib = _lib.load()
    projs = [tuple(torch.from_numpy(x).to(dev) for x in synth.layer_projections(l, D, 768)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, 768) for l in range(L)])).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    mk = lambda: LTMEngine(N, 12, 64, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev)

    def tokens(n_frames):
        k = torch.empty(n_frames, P, D, device=dev)
        for f0 in range(0, n_frames, 8192):                        # (no second tensor of the whole batch beside k)
            k[f0:f0 + 8192] = torch.randn(min(8192, n_frames - f0), P, D, device=dev, generator=gen)
        return k

    if leg == "parent_check":                                      # the existing call, untouched by this change: 256 x 8 full chunks
        V, C = 256, 8
        engines = [mk() for _ in range(V)]
        k = tokens(V * C * T).reshape(V * C, T * P, D)
        u = torch.rand(V * C, L, S, device=dev, dtype=torch.float64, generator=gen)
        call = lambda: consolidate_videos(engines, k, [C] * V, q, projs, u, new_doc=True)
        total = V * C
    else:
        V, full = MIXES[mix]
        tails = np.random.default_rng(7).integers(2, 256, size=V).tolist()      # uniform over 2..255
        frames = [full * T + t for t in tails]
        frame0 = np.concatenate([[0], np.cumsum(frames)])
        total = V * (full + 1)
        engines = [mk() for _ in range(V)]
        k = tokens(int(frame0[-1]))
        u = torch.rand(total, L, S, device=dev, dtype=torch.float64, generator=gen)
        if leg == "one_call":
            call = lambda: consolidate_videos_frames(engines, k, frames, T, q, projs, u, new_doc=True)[0]
        else:
            # what a caller did before: the full chunks packed for the batched call (made once, outside the timing), then one
            # per-handle call per short last chunk
            k_full = torch.cat([k[int(frame0[v]):int(frame0[v]) + full * T] for v in range(V)]).reshape(V * full, T * P, D)
            rows_full = torch.cat([torch.arange(v * (full + 1), v * (full + 1) + full) for v in range(V)]).to(dev)
            u_full = u[rows_full].contiguous()
            k_tail = [k[int(frame0[v]) + full * T:int(frame0[v + 1])].reshape(1, tails[v] * P, D) for v in range(V)]
            u_tail = [u[v * (full + 1) + full:v * (full + 1) + full + 1] for v in range(V)]

            def call():
                out = consolidate_videos(engines, k_full, [full] * V, q, projs, u_full, new_doc=True)
                last = [e.consolidate(k_tail[v], q, projs, u_tail[v], new_doc=False) for v, e in enumerate(engines)]
                return out, last
    call()                                                         # warm-up: plans, workspaces
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    out = call()
    torch.cuda.synchronize()
    launches = int(lib.infv_ltm_launch_count() - n0)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    first = out[0] if isinstance(out, tuple) else out
    med = statistics.median(ms)
    print(json.dumps({"leg": leg, "mix": mix if leg != "parent_check" else "256x8", "videos": V, "chunks": total, "reps": reps,
                      "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                      "chunks_per_s": round(total / med * 1e3, 1), "launches_per_call": launches,
                      "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
                      "checksum": float(first.double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mixes", nargs="+", choices=sorted(MIXES), default=list(MIXES))
    ap.add_argument("--child", choices=LEGS + ("parent_check",))
    ap.add_argument("--mix", choices=sorted(MIXES), default="256x7+tail")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--parent-lib", metavar="PATH", help="consolidate_videos at 256 x 8 alone, alternated between this build of the parent commit and this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "videos_tail.jsonl"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.mix, a.reps)
    if a.rounds < 3:
        ap.error("at least three rounds")

    def run_child(leg, mix, rnd, library=None):
        env = dict(os.environ)
        if library:
            env["INFV_LTM_LIBRARY"] = os.path.abspath(library)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--mix", mix, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=a.child_timeout, cwd=ROOT, env=env)
        if r.returncode != 0:                                      # stop here: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child {leg} / {mix} of round {rnd} ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().split("\n")[-1])
        line["round"] = rnd
        return line

    def spread(v):
        return round(max(v) - min(v), 3)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    lines = []
    if a.parent_lib:
        for rnd in range(a.rounds):
            for side, library in (("parent", a.parent_lib), ("branch", None)):      # alternated child by child
                line = dict(run_child("parent_check", "256x7+tail", rnd, library), side=side)
                print(json.dumps(line), flush=True)
                lines.append(line)
        per = {side: [l["median_ms"] for l in lines if l["side"] == side] for side in ("parent", "branch")}
        mp, mb = statistics.median(per["parent"]), statistics.median(per["branch"])
        summaries = [{"summary": True, "measure": "parent_vs_branch", "call": "consolidate_videos", "mix": "256x8", "rounds": a.rounds,
                      "reps_per_child": a.reps, "parent_ms": round(mp, 3), "branch_ms": round(mb, 3), "round_medians_ms": per,
                      "branch_minus_parent_ms": round(mb - mp, 3), "parent_spread_ms": spread(per["parent"]),
                      "inside_parent_spread": bool(min(per["parent"]) <= mb <= max(per["parent"])),
                      "launches_per_call": sorted({l["launches_per_call"] for l in lines}),
                      "same_checksum": len({l["checksum"] for l in lines}) == 1}]
    else:
        summaries = []
        for mix in a.mixes:
            mine = []
            for rnd in range(a.rounds):
                for leg in LEGS:                                   # alternated: one fresh process per leg and round, one at a time
                    line = run_child(leg, mix, rnd)
                    print(json.dumps(line), flush=True)
                    mine.append(line)
            per = {leg: [l["median_ms"] for l in mine if l["leg"] == leg] for leg in LEGS}
            med = {leg: statistics.median(v) for leg, v in per.items()}
            summaries.append({"summary": True, "mix": mix, "videos": mine[0]["videos"], "chunks": mine[0]["chunks"], "rounds": a.rounds,
                              "reps_per_child": a.reps, "ms_per_call": {k: round(v, 3) for k, v in med.items()},
                              "launches_per_call": {leg: [l["launches_per_call"] for l in mine if l["leg"] == leg][-1] for leg in LEGS},
                              "round_medians_ms": per, "round_median_spread_ms": {leg: spread(v) for leg, v in per.items()},
                              "one_call_over_full_then_tails": round(med["one_call"] / med["full_then_tails"], 3),
                              "one_call_is_faster": bool(med["one_call"] < med["full_then_tails"])})
            lines += mine
    for s in summaries:
        print(json.dumps(s), flush=True)
    with open(a.out, "a") as f:
        for l in lines + summaries:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
