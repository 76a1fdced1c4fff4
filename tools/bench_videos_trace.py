"""What the attention read-outs of the batched calls cost (include/infv_ltm.h: infv_ltm_set_videos_mass_trace,
infv_ltm_source_weights_videos).  Two parts, each leg in a CHILD PROCESS of its own (a fresh HIP context), the legs ALTERNATED
within a round, three rounds by default; a child warms its call, times `--reps` calls with device events and reports their median.

  1. consolidate_videos at the headline chunk shape (T 256, N 256, L 2, Q 32, P 32, bf16 tokens), 256 videos x 8 chunks and
     64 x 32.  Legs: off (no trace), on (the packed mass trace set on the lead engine: one launch more per lockstep step), and
     parent_off (no trace, on a build of the parent commit: `--parent-lib PATH`, skipped without it).  The summary states whether
     the off leg lies inside the parent's own round-to-round spread, and the launch counts.
  2. infv_ltm_source_weights_videos (one launch) against a loop of infv_ltm_source_weights per video, random bins and masses:
     vc64 / vc64_attn   64 videos x 8 chunks at T 16, N 64, g 1, L 1 (the VideoChat2 evaluation shape), without / with attn_all
     head256_attn       256 videos x 8 chunks at T 256, N 256, g 16, L 2, with attn_all
     each as `<cfg>:batched` and `<cfg>:loop`.

    timeout -k 10 900 python tools/bench_videos_trace.py [--parent-lib /path/to/parent/libinfv_ltm.so]

One JSON line per child and one summary line per part are appended to profiles/videos_trace.jsonl (--out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, DH, D, P, S = 12, 64, 768, 32, 512
CALL_CONFIGS = {"256x8": [8] * 256, "64x32": [32] * 64}
SRC_CONFIGS = {  # T, N, g, L, videos, chunks, attn
    "vc64": (16, 64, 1, 1, 64, 8, False), "vc64_attn": (16, 64, 1, 1, 64, 8, True), "head256_attn": (256, 256, 16, 2, 256, 8, True)}
CALL_LEGS = tuple(f"{c}:{leg}" for c in CALL_CONFIGS for leg in ("off", "on", "parent_off"))
SRC_LEGS = tuple(f"{c}:{leg}" for c in SRC_CONFIGS for leg in ("batched", "loop"))


def _timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def child_call(leg, reps):
    """consolidate_videos; `parent_off` runs in a process whose INFV_LTM_LIBRARY names the parent's library (set by main)."""
    import ctypes as C
    import numpy as np
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine, consolidate_videos
    cfg, kind = leg.split(":")
    if kind == "parent_off":                                       # the parent's library has every symbol but the two this tool is about
        for name in ("infv_ltm_set_videos_mass_trace", "infv_ltm_source_weights_videos"):
            _lib._SIGNATURES.pop(name, None)
    counts = CALL_CONFIGS[cfg]
    V, total = len(counts), sum(counts)
    T, N, L, Q = 256, 256, 2, 32
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    k = torch.randn(total, T * P, D, device=dev, generator=gen, dtype=torch.bfloat16)
    u = torch.rand(total, L, S, device=dev, dtype=torch.float64, generator=gen)
    projs = [tuple(torch.from_numpy(x).to(dev) for x in synth.layer_projections(l, D, H * DH)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, H * DH) for l in range(L)])).to(dev)
    engines = [LTMEngine(N, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev) for _ in range(V)]
    lib = _lib.load()
    mass = None
    if kind == "on":
        mass = torch.full((total, L, N), float("nan"), device=dev)
        _lib.check(lib.infv_ltm_set_videos_mass_trace(engines[0]._h, C.c_void_p(mass.data_ptr()), total))

    def call():
        return consolidate_videos(engines, k, counts, q, projs, u, new_doc=True)
    call()
    torch.cuda.synchronize()
    n0 = int(lib.infv_ltm_launch_count())
    ctx = call()
    launches = int(lib.infv_ltm_launch_count()) - n0
    torch.cuda.synchronize()
    ms = _timed(call, reps)
    line = {"part": "call", "leg": leg, "videos": V, "chunks": total, "steps": max(counts), "reps": reps,
            "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "launches_per_call": launches, "library": os.path.basename(_lib.LIB_PATH), "checksum": float(ctx.double().sum())}
    if mass is not None:
        line["mass_rows_written"] = int(torch.isfinite(mass).all(-1).all(-1).sum())
    print(json.dumps(line), flush=True)


def child_sources(leg, reps):
    import ctypes as C
    import numpy as np
    import torch
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    cfg, kind = leg.split(":")
    T, N, g, L, V, chunks, with_attn = SRC_CONFIGS[cfg]
    dev = torch.device("cuda:0")
    total, M = V * chunks, chunks * (T // g)
    gen = torch.Generator(device=dev).manual_seed(1)
    bins = torch.randint(0, 127, (total, L, S), device=dev, dtype=torch.int32, generator=gen)
    mass = torch.rand(total, L, N, device=dev, generator=gen) / N
    eng = LTMEngine(N, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=32, device=dev)
    eng.ensure_plan(T)
    W = torch.empty(V, L, N, M, device=dev)
    attn = torch.empty(total, L, M, device=dev) if with_attn else None
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    cu = np.ascontiguousarray(np.arange(V + 1, dtype=np.int32) * chunks)
    if kind == "batched":
        desc = _lib.SourcesVideosDesc(n_videos=V, T=T, frames_per_source=g, reserved=0, ld=M, cu=cu.ctypes.data, bins_all=ptr(bins),
                                      W_all=ptr(W), mass_all=ptr(mass if with_attn else None), attn_all=ptr(attn), bad_bins=None,
                                      hip_stream=stream)

        def call():                                                # the entry point alone: no allocation, no read-back
            _lib.check(lib.infv_ltm_source_weights_videos(eng._h, C.byref(desc)))
    else:
        desc1 = _lib.SourcesDesc(n_chunks=chunks, T=T, new_doc=1, frames_per_source=g, col_begin=0, ld=M)
        vp = lambda t, v, rows: C.c_void_p(0 if t is None else t.data_ptr() + v * rows * t.element_size())
        args = [(vp(bins, v, chunks * L * S), vp(W, v, L * N * M), vp(mass if with_attn else None, v, chunks * L * N),
                 vp(attn, v, chunks * L * M)) for v in range(V)]
        st = C.c_void_p(stream)

        def call():
            for b, w, m, a_ in args:
                _lib.check(lib.infv_ltm_source_weights(eng._h, C.byref(desc1), b, w, m, a_, None, st))
    call()
    torch.cuda.synchronize()
    n0 = int(lib.infv_ltm_launch_count())
    call()
    launches = int(lib.infv_ltm_launch_count()) - n0
    torch.cuda.synchronize()
    ms = _timed(call, reps)
    line = {"part": "sources", "leg": leg, "videos": V, "chunks_per_video": chunks, "T": T, "N": N, "g": g, "L": L, "attn": with_attn,
            "reps": reps, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "launches_per_call": launches, "checksum": float(W.double().sum())}
    if with_attn:
        line["attn_checksum"] = float(attn.double().sum())
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--src-reps", type=int, default=20)
    ap.add_argument("--parts", default="call,sources")
    ap.add_argument("--parent-lib", default=None, help="libinfv_ltm.so built from the parent commit (the parent_off legs)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "videos_trace.jsonl"))
    a = ap.parse_args()
    if a.child:
        return (child_call if a.child in CALL_LEGS else child_sources)(a.child, a.reps)
    parts = [p for p in a.parts.split(",") if p]

    def run_child(leg, rnd, reps):
        env = dict(os.environ)
        if leg.endswith(":parent_off"):
            env["INFV_LTM_LIBRARY"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(reps)], capture_output=True,
                           text=True, timeout=a.child_timeout, cwd=ROOT, env=env)
        if r.returncode != 0:                                      # stop here: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child {leg} of round {rnd} ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().split("\n")[-1])
        line["round"] = rnd
        print(json.dumps(line), flush=True)
        return line

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = []
    if "call" in parts:
        legs = [l for l in CALL_LEGS if a.parent_lib or not l.endswith(":parent_off")]
        lines = [run_child(leg, rnd, a.reps) for rnd in range(a.rounds) for leg in legs]
        per = {leg: [l["median_ms"] for l in lines if l["leg"] == leg] for leg in legs}
        med = {leg: round(statistics.median(v), 3) for leg, v in per.items()}
        spread = {leg: round(max(v) - min(v), 3) for leg, v in per.items()}
        summary = {"summary": True, "measure": "videos_trace_call", "rounds": a.rounds, "reps_per_child": a.reps, "median_ms": med,
                   "round_medians_ms": per, "spread_ms": spread,
                   "launches_per_call": {leg: sorted({l["launches_per_call"] for l in lines if l["leg"] == leg}) for leg in legs},
                   "checksums": {leg: sorted({l["checksum"] for l in lines if l["leg"] == leg}) for leg in legs}}
        for cfg in CALL_CONFIGS:
            off, on, par = f"{cfg}:off", f"{cfg}:on", f"{cfg}:parent_off"
            summary[cfg] = {"trace_cost_ms": round(med[on] - med[off], 3), "on_over_off": round(med[on] / med[off], 4),
                            "trace_cost_us_per_step": round((med[on] - med[off]) * 1e3 / max(CALL_CONFIGS[cfg]), 2)}
            if par in med:
                summary[cfg].update(off_minus_parent_ms=round(med[off] - med[par], 3), parent_spread_ms=spread[par],
                                    off_inside_parent_spread=bool(min(per[par]) <= med[off] <= max(per[par])),
                                    same_launches_as_parent=summary["launches_per_call"][off] == summary["launches_per_call"][par])
        print(json.dumps(summary), flush=True)
        out += lines + [summary]
    if "sources" in parts:
        lines = [run_child(leg, rnd, a.src_reps) for rnd in range(a.rounds) for leg in SRC_LEGS]
        per = {leg: [l["median_ms"] for l in lines if l["leg"] == leg] for leg in SRC_LEGS}
        med = {leg: round(statistics.median(v), 4) for leg, v in per.items()}
        summary = {"summary": True, "measure": "videos_trace_sources", "rounds": a.rounds, "reps_per_child": a.src_reps, "median_ms": med,
                   "round_medians_ms": per, "spread_ms": {leg: round(max(v) - min(v), 4) for leg, v in per.items()},
                   "loop_over_batched": {c: round(med[f"{c}:loop"] / med[f"{c}:batched"], 2) for c in SRC_CONFIGS},
                   "launches_per_call": {leg: sorted({l["launches_per_call"] for l in lines if l["leg"] == leg}) for leg in SRC_LEGS},
                   "same_checksums": {c: sorted({l["checksum"] for l in lines if l["leg"] == f"{c}:batched"}) ==
                                         sorted({l["checksum"] for l in lines if l["leg"] == f"{c}:loop"}) for c in SRC_CONFIGS}}
        print(json.dumps(summary), flush=True)
        out += lines + [summary]
    with open(a.out, "a") as f:
        for l in out:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
