"""Many short videos through ONE batched call (engine.consolidate_videos) against a loop of per-video consolidate(), at the
headline shape (T 256, N 256, L 2, Q 32, fp32 tokens).  One JSON line per configuration; run one configuration per process:

    timeout -k 10 600 python tools/bench_videos.py --config 64x32
    timeout -k 10 600 python tools/bench_videos.py --config ragged
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

CONFIGS = {"256x8": [8] * 256, "64x32": [32] * 64, "16x128": [128] * 16,
           # ragged mix: 64 videos of 4..60 chunks (a dataset's length spread), 2048 chunks in all
           "ragged": [4 + (7 * i) % 57 for i in range(64)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine, consolidate_videos
    counts = CONFIGS[a.config]
    V, total = len(counts), sum(counts)
    T, N, L, Q, P, d, dm = 256, 256, 2, 32, 32, 768, 768
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    k = torch.randn(total, T * P, d, device=dev, generator=gen)
    u = torch.rand(total, L, 512, device=dev, dtype=torch.float64, generator=gen)
    projs = [tuple(torch.from_numpy(x).to(dev) for x in synth.layer_projections(l, d, dm)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, dm) for l in range(L)])).to(dev)
    mk = lambda: LTMEngine(N, 12, 64, d, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev)
    eng_b, eng_s = [mk() for _ in range(V)], [mk() for _ in range(V)]
    cu = np.concatenate([[0], np.cumsum(counts)])
    tr_b = [e.set_trace(c) for e, c in zip(eng_b, counts)]
    tr_s = [e.set_trace(c) for e, c in zip(eng_s, counts)]
    lib = _lib.load()

    def batched():
        return consolidate_videos(eng_b, k, counts, q, projs, u, new_doc=True)

    def loop():
        return [e.consolidate(k[cu[v]:cu[v + 1]], q, projs, u[cu[v]:cu[v + 1]], new_doc=True) for v, e in enumerate(eng_s)]

    def timed(fn):
        best = None
        for _ in range(a.reps + 1):                    # first call: warm-up (workspaces, plans)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best, out

    n0 = lib.infv_ltm_launch_count()
    torch.cuda.synchronize()
    batched()
    torch.cuda.synchronize()
    launches = lib.infv_ltm_launch_count() - n0
    t_b, ctx_b = timed(batched)
    t_s, ctx_s = timed(loop)
    # device time per kernel family (HIP events around every launch of the batched call; the events' own gaps included)
    eng_b[0].profile(True)
    batched()
    prof = {name: {"launches": n, "ms": round(ms, 3)} for name, (n, ms) in eng_b[0].profile_read().items() if n}
    eng_b[0].profile(False)
    flips = sum(int((tb[0][1:] != ts[0][1:]).sum()) for tb, ts in zip(tr_b, tr_s))
    err = max(float((ctx_b[cu[v]:cu[v + 1]] - ctx_s[v]).abs().max()) for v in range(V))
    # per-step device time: the same videos advanced one chunk per call (lockstep steps as separate calls), HIP events
    steps = []
    for s in range(max(counts)):
        act = [v for v in range(V) if counts[v] > s]
        kk = torch.stack([k[cu[v] + s] for v in act])
        uu = torch.stack([u[cu[v] + s] for v in act])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        consolidate_videos([eng_b[v] for v in act], kk, [1] * len(act), q, projs, uu, new_doc=(s == 0))
        e1.record()
        e1.synchronize()
        steps.append(e0.elapsed_time(e1))
    print(json.dumps({
        "config": a.config, "videos": V, "chunks": total, "shape": {"T": T, "N": N, "L": L, "Q": Q, "tokens": "fp32"},
        "batched_chunks_per_s": round(total / t_b, 1), "per_video_loop_chunks_per_s": round(total / t_s, 1),
        "speedup": round(t_s / t_b, 3), "batched_ms": round(t_b * 1e3, 3), "loop_ms": round(t_s * 1e3, 3),
        "launches_per_step": round(launches / max(counts), 2), "launches_per_call": int(launches),
        "step_ms": {"min": round(min(steps), 4), "median": round(statistics.median(steps), 4), "max": round(max(steps), 4),
                    "steps": len(steps)},
        "kernel_ms_in_batched_call": prof,
        "draw_flips_vs_loop": flips, "drawn_bins": int(sum(max(c - 1, 0) for c in counts) * L * 512),
        "max_abs_ctx_diff_vs_loop": err}), flush=True)


if __name__ == "__main__":
    main()
