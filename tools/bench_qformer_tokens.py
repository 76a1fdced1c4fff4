"""bf16 (or, with --dtype float16, fp16) frame tokens through the video Q-former against fp32 tokens, at the headline chunk shape (T 256, P 32, d 768, N 256,
Q 32, 2 layers, alpha 0.9, sticky, llama 4096).  Three legs on the same values, ALTERNATED within the process (a b c a b c ...),
device-event timing after a warm-up of every leg, median and min-max of each:

  a  fp32 tokens (x.float() prepared outside the timed window)      -- the existing path
  b  bf16 tokens, native (infv_vqf_set_token_dtype)
  c  bf16 tokens the way the library handled them before: x.float() inside the timed window, then (a)

One configuration per process; one JSON line appended to profiles/vqf_bf16_tokens.jsonl (--out):

    timeout -k 10 600 python tools/bench_qformer_tokens.py --config video252

--dtype float16 runs legs b and c on fp16 tokens: b reads them in place (INFV_TOKENS_F16: one token pass at 2 bytes per element,
then the three-product contractions of leg a), c is "fp16 tokens cast to fp32 first", what a user of fp16 tokens did before.
The counts from the shapes then are: token pass 2 + 8 bytes per element, contractions as for fp32 tokens.

--dtype float8_e4m3fn runs legs b and c on fp8 e4m3 tokens (the caller's storage choice): b reads them in place (INFV_TOKENS_F8E4M3:
one token pass at 1 byte per element that writes the two hi planes, then the two-product contractions of bf16 tokens), c is "fp8
tokens cast to fp32 first".  Counts: token pass 1 + 4 bytes per element, contractions as for bf16 tokens.  Quote it next to a
--dtype bfloat16 line of the same run (profiles/vqf_f8_tokens.jsonl holds both).

--legs a times leg (a) only and touches nothing of the bf16 interface (the same script then runs against a build of an earlier
commit: the fp32 path before / after).  Bytes and bf16-MFMA FLOP per chunk are computed from the shapes, so that the
achieved rates stand next to the counts."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

RAGGED = [1 + (5 * i) % 12 for i in range(64)]                    # tools/bench_videos_qformer.py's mix: 64 videos of 1-12 chunks
CONFIGS = {"video252": ("encode_frames_batch", [252]), "videos128x4": ("encode_videos", [4] * 128),
           "ragged": ("encode_videos", RAGGED), "chunk": ("encode_frames", [8])}
T, P, D, L, Q, H = 256, 32, 768, 2, 32, 12


def counts_from_shapes():
    """Per chunk, from the shapes alone: bytes of the token pass and of the token planes the four contractions stream (two
    per layer: scores reads F, read-out reads FT), and bf16-MFMA FLOP of those contractions."""
    n = T * P
    elems = n * D
    rows = H * Q
    f32 = {"token_pass_bytes": elems * (4 + 8), "contraction_token_bytes": L * 2 * elems * 4,
           "mfma_flop": L * 2 * 3 * 2 * rows * n * D}
    bf16 = {"token_pass_bytes": elems * (2 + 2), "contraction_token_bytes": L * 2 * elems * 2,
            "mfma_flop": L * 2 * 2 * 2 * rows * n * D}
    f16 = dict(f32, token_pass_bytes=elems * (2 + 8))
    f8 = dict(bf16, token_pass_bytes=elems * (1 + 4))
    return {"fp32_tokens": f32, "bf16_tokens": bf16, "fp16_tokens": f16, "fp8_tokens": f8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="abc", choices=["abc", "a", "b"])
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16", "float8_e4m3fn"], help="the token format of legs b and c")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vqf_bf16_tokens.jsonl"))
    a = ap.parse_args()
    if a.rounds < 5 and a.legs == "abc":
        ap.error("at least five rounds")
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.video_qformer import InfVideoEncoder, VideoMemory
    entry, counts = CONFIGS[a.config]
    V, total = len(counts), sum(counts)
    dev = torch.device("cuda:0")
    m = InfVideoEncoder(num_basis=256, tau=0.75, alpha=0.9, sticky=True)
    m.load_reference_state_dict(synth.video_qformer_weights())
    m = m.to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    half = getattr(torch, a.dtype)
    short = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float8_e4m3fn: "fp8"}[half]
    x = torch.empty(total, T * P, D, device=dev, dtype=half)
    for c0 in range(0, total, 32):                                 # (no fp32 tensor of the whole video beside the two below)
        x[c0:c0 + 32] = torch.randn(min(32, total - c0), T * P, D, device=dev, generator=gen).to(half)
    x32 = x.float() if a.legs != "b" else None
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    u = torch.rand(total, L, 512, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(dev)
    mems = [VideoMemory(m, dev) for _ in range(V)] if entry == "encode_videos" else None
    lib = _lib.load()

    def call(frames):
        if entry == "encode_frames_batch":
            return m.encode_frames_batch(frames, new_video=True, u=u)[0]
        if entry == "encode_videos":
            return m.encode_videos(frames, counts, new_video=True, u=u, memories=mems)[0]
        out = None
        for c in range(total):                                      # the per-chunk path: one video, chunk by chunk
            out = m.encode_frames(frames[c:c + 1], new_video=(c == 0), u=u[c])[1]
        return out

    legs = {"a": lambda: call(x32), "b": lambda: call(x), "c": lambda: call(x.float())}
    legs = {k: v for k, v in legs.items() if k in a.legs}
    launches, peak, outs = {}, {}, {}
    first_call = {}
    for k, fn in legs.items():                                      # warm-up of every leg: workspaces, plans, allocator
        fn()
        torch.cuda.synchronize()
        first_call[k] = int(free0 - torch.cuda.mem_get_info(dev)[0])   # free device memory taken so far (legs run in order a, b, c)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        n0 = lib.infv_ltm_launch_count()
        outs[k] = fn().clone()
        torch.cuda.synchronize()
        launches[k] = int(lib.infv_ltm_launch_count() - n0)
        peak[k] = int(torch.cuda.max_memory_allocated(dev) - base)
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    line = {"config": a.config, "entry": entry, "videos": V, "chunks": total, "T": T, "N": 256, "Q": Q, "layers": L, "alpha": 0.9,
            "llama": 4096, "rounds": a.rounds, "legs": a.legs, "tag": a.tag, "library": os.path.basename(_lib.LIB_PATH),
            "half_dtype": a.dtype, f"tokens_bytes_{short}": x.numel() * x.element_size(), "counts_per_chunk_from_shapes": counts_from_shapes()}
    names = {"a": "fp32_tokens", "b": f"{short}_tokens_native", "c": f"{short}_tokens_upcast_in_window"}
    for k in legs:
        med = statistics.median(ms[k])
        line[names[k]] = {"median_ms": round(med, 3), "min_ms": round(min(ms[k]), 3), "max_ms": round(max(ms[k]), 3),
                          "chunks_per_s": round(total / med * 1e3, 1), "ms_per_chunk": round(med / total, 4),
                          "launches_per_call": launches[k], "torch_peak_rise_bytes": peak[k],
                          "free_drop_after_first_call_bytes": first_call[k]}
    if "a" in legs and "b" in legs:
        line["b_equals_a_bit_for_bit"] = bool(torch.equal(outs["a"], outs["b"]))
        line["b_over_c"] = round(statistics.median(ms["b"]) / statistics.median(ms["c"]), 4)
        line["b_over_a"] = round(statistics.median(ms["b"]) / statistics.median(ms["a"]), 4)
        per_chunk_s = statistics.median(ms["b"]) / total * 1e-3
        cnt = counts_from_shapes()[f"{short}_tokens"]
        line[f"{short}_achieved"] = {"token_bytes_GBps": round((cnt["token_pass_bytes"] + cnt["contraction_token_bytes"]) / per_chunk_s / 1e9, 1),
                                 "mfma_TFLOPs": round(cnt["mfma_flop"] / per_chunk_s / 1e12, 1)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
