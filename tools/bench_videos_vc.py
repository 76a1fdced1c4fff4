"""Many short videos through the VideoChat2 Q-former in ONE call (VideoChat2Encoder.encode_videos, what encode_long_videos_vc issues)
against the loop of encode_long_video_vc over the same videos, at the eval shape of the reference's four VideoChat2 drivers
(T 16, P 196, width 1024, N 64, 96 query tokens, 12 layers, alpha 0.75, sticky, 16 instruction tokens, mistral_proj 4096).
The two alternate in one process, five rounds after a warm-up each, wall time around a device synchronisation (the loop is
host-bound); both draw their Gibbs uniforms from torch's CPU generator.  Appends one JSON line per split to
profiles/multi_video_vc_bench.jsonl (--out).  Run one split per process:

    timeout -k 10 900 python tools/bench_videos_vc.py --config 64x8
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

import torch            # noqa: E402

CONFIGS = {"1x8": [8], "16x8": [8] * 16, "64x8": [8] * 64, "8x64": [64] * 8,
           "ragged": [1 + (5 * i) % 12 for i in range(64)]}       # 64 videos of 1-12 chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_video_vc_bench.jsonl"))
    a = ap.parse_args()
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.videochat2_qformer import VideoChat2Encoder, VideoChat2Memory, encode_long_video_vc
    counts = CONFIGS[a.config]
    V, total = len(counts), sum(counts)
    T, P, d, n_text = 16, 196, 1024, 16
    dev = torch.device("cuda:0")
    m = VideoChat2Encoder(num_basis=64, sticky=True, tau=0.75, alpha=0.75)
    m.load_reference_state_dict(synth.videochat2_qformer_weights())
    m = m.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    videos = [torch.randn(c * T, P, d, device=dev, generator=gen) for c in counts]
    text = torch.randn(1, n_text, 768, device=dev, generator=gen)
    mems = [VideoChat2Memory(m, dev) for _ in range(V)]
    lib = _lib.load()

    chunked = [v.reshape(c, T * P, d) for v, c in zip(videos, counts)]     # torch.chunk(video, C_v): equal chunks of T frames

    def batched():
        return m.encode_videos(chunked, text_embeds=text, memories=mems)

    def loop():
        return [encode_long_video_vc(m, videos[v], counts[v], text) for v in range(V)]

    def once(fn, seed):
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    once(batched, 0), once(loop, 0)                              # warm-up (workspaces, plans)
    n0 = lib.infv_ltm_launch_count()
    _, out_b = once(batched, 0)
    launches_b = lib.infv_ltm_launch_count() - n0
    n0 = lib.infv_ltm_launch_count()
    _, out_l = once(loop, 0)
    launches_l = lib.infv_ltm_launch_count() - n0                # (the library's own launches; the loop's BERT blocks are torch's)
    ms_b, ms_l = [], []
    for r in range(a.rounds):                                    # alternating, so that drift hits both alike
        ms_b.append(once(batched, r + 1)[0])
        ms_l.append(once(loop, r + 1)[0])
    diff = torch.stack([(out_b[1][v] - out_l[v][0][0]).abs().max() for v in range(V)])
    med_b, med_l = statistics.median(ms_b), statistics.median(ms_l)
    line = {"config": a.config, "videos": V, "chunks": total, "T": T, "P": P, "N": 64, "Q": 96, "layers": 12, "alpha": 0.75,
            "text_tokens": n_text, "proj": 4096, "rounds": a.rounds,
            "batched_ms": round(med_b, 2), "batched_ms_min_max": [round(min(ms_b), 2), round(max(ms_b), 2)],
            "loop_ms": round(med_l, 2), "loop_ms_min_max": [round(min(ms_l), 2), round(max(ms_l), 2)],
            "batched_chunks_per_s": round(total / med_b * 1e3, 1), "loop_chunks_per_s": round(total / med_l * 1e3, 1),
            "speedup": round(med_l / med_b, 3), "loop_spread": round((max(ms_l) - min(ms_l)) / med_l, 4),
            "launches_per_call_batched": int(launches_b), "library_launches_per_call_loop": int(launches_l),
            # a flipped Gibbs draw moves a video's mean beyond rounding: videos beyond 2e-4 count the flips' effect
            "videos_beyond_2e-4_vs_loop": int((diff > 2e-4).sum()), "max_abs_dmean_vs_loop": float(diff.max())}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
