"""Many short videos through the video Q-former in ONE call (InfVideoEncoder.encode_videos) against a loop of per-video
encode_frames_batch calls on the same frames and uniforms, at the headline chunk shape (T 256, P 32, d 768, N 256, Q 32,
2 layers, alpha 0.9, sticky, llama 4096, fp32 tokens).  Device-event timing after a warm-up; appends one JSON line per
configuration to profiles/multi_video_qformer_bench.jsonl (--out).  Run one configuration per process:

    timeout -k 10 600 python tools/bench_videos_qformer.py --config 128x4
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

CONFIGS = {"128x4": [4] * 128, "64x8": [8] * 64, "16x32": [32] * 16,
           "ragged": [1 + (5 * i) % 12 for i in range(64)]}       # 64 videos of 1-12 chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_video_qformer_bench.jsonl"))
    a = ap.parse_args()
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.video_qformer import InfVideoEncoder, VideoMemory
    counts = CONFIGS[a.config]
    V, total = len(counts), sum(counts)
    T, P, d, L = 256, 32, 768, 2
    dev = torch.device("cuda:0")
    m = InfVideoEncoder(num_basis=256, tau=0.75, alpha=0.9, sticky=True)
    m.load_reference_state_dict(synth.video_qformer_weights())
    m = m.to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randn(total, T * P, d, device=dev, generator=gen)
    u = torch.rand(total, L, 512, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dev)
    cu = [0]
    for c in counts:
        cu.append(cu[-1] + c)
    mems = [VideoMemory(m, dev) for _ in range(V)]
    lib = _lib.load()

    def batched():
        return m.encode_videos(frames, counts, new_video=True, u=u, memories=mems)

    def loop():
        out = []
        for v in range(V):
            llama, _, _ = m.encode_frames_batch(frames[cu[v]:cu[v + 1]], new_video=True, u=u[cu[v]:cu[v + 1]])
            out.append(llama)
        return torch.cat(out)

    def timed(fn):
        fn()                                                      # warm-up (workspaces, plans)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), out

    n0 = lib.infv_ltm_launch_count()
    batched()
    launches_b = lib.infv_ltm_launch_count() - n0
    n0 = lib.infv_ltm_launch_count()
    loop()
    launches_l = lib.infv_ltm_launch_count() - n0
    ms_b, (llama_b, _, _) = timed(batched)
    ms_l, llama_l = timed(loop)
    diff = (llama_b - llama_l).abs().amax(dim=(1, 2))
    line = {"config": a.config, "videos": V, "chunks": total, "T": T, "N": 256, "Q": 32, "layers": L, "alpha": 0.9,
            "llama": 4096, "batched_ms": round(ms_b, 3), "loop_ms": round(ms_l, 3),
            "batched_chunks_per_s": round(total / ms_b * 1e3, 1), "loop_chunks_per_s": round(total / ms_l * 1e3, 1),
            "speedup": round(ms_l / ms_b, 3), "launches_per_call_batched": int(launches_b), "launches_per_call_loop": int(launches_l),
            # a flipped Gibbs draw moves a chunk's output far beyond rounding: chunks beyond 2e-4 count the flips' effect
            "chunks_beyond_2e-4_vs_loop": int((diff > 2e-4).sum()), "max_abs_dllama_vs_loop": float(diff.max())}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
