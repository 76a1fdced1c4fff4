"""What tracing the memory back to its frames costs (include/infv_ltm.h, "Source weights"), on the headline shape: T 256, N 256,
2 layers, sticky, a 2048-chunk video -- the call bench.py times -- with random bins (the pass reads bins, not a memory).

One CHILD PROCESS per leg and round (a fresh HIP context), the legs ALTERNATED within a round, three rounds by default.  Legs:

  g256 / g256_attn     infv_ltm_source_weights with one column per chunk (g = 256, M = 2048), without / with attn_all
  g16 / g16_attn       ... with 16 frames per column (M = 32768)
  torch_g256 / torch_g16   the same recurrence as a plain torch loop on the device: per chunk and layer an index_select of the
                       resampled rows of W and an index_add_ into their boxes, the new frames' counts added, one multiplication.
                       (Its additions are atomics in no fixed order: same values to rounding, not the kernel's bits.)

A child warms its call, times `--reps` calls (`--torch-reps` for the loop) with device events and reports their median, and the
kernel legs the launches of one call.  The summary gives each leg's median over the rounds with its spread (max - min of the
round medians) and the ratio torch loop / kernel.

    timeout -k 10 900 python tools/bench_source_weights.py

One JSON line per child and one summary line per run are appended to profiles/source_weights.jsonl (--out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N, L, S, H, DH, D, P = 256, 256, 2, 512, 12, 64, 768, 32
LEGS = ("g256", "g256_attn", "g16", "g16_attn", "torch_g256", "torch_g16")


def _inputs(dev, chunks):
    import torch
    gen = torch.Generator(device=dev).manual_seed(1)
    bins = torch.randint(0, 127, (chunks, L, S), device=dev, dtype=torch.int32, generator=gen)
    mass = torch.rand(chunks, L, N, device=dev, generator=gen) / N
    return bins, mass


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


def child_kernel(leg, chunks, reps):
    import ctypes as C
    import torch
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    dev = torch.device("cuda:0")
    g = 256 if leg.startswith("g256") else 16
    with_attn = leg.endswith("_attn")
    bins, mass = _inputs(dev, chunks)
    eng = LTMEngine(N, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=32, device=dev)
    eng.ensure_plan(T)
    M = chunks * (T // g)
    W = torch.empty(L, N, M, device=dev)
    attn = torch.empty(chunks, L, M, device=dev) if with_attn else None
    desc = _lib.SourcesDesc(n_chunks=chunks, T=T, new_doc=1, frames_per_source=g, col_begin=0, ld=M)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():                                                    # the entry point alone: no allocation, no read-back
        _lib.check(lib.infv_ltm_source_weights(eng._h, C.byref(desc), ptr(bins), ptr(W), ptr(mass if with_attn else None), ptr(attn),
                                               None, stream))
    call()
    torch.cuda.synchronize()
    n0 = int(lib.infv_ltm_launch_count())
    call()
    launches = int(lib.infv_ltm_launch_count()) - n0
    torch.cuda.synchronize()
    ms = _timed(call, reps)
    med = statistics.median(ms)
    line = {"leg": leg, "chunks": chunks, "g": g, "columns": M, "reps": reps, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "launches_per_call": launches, "checksum": float(W.double().sum())}
    if with_attn:
        line["attn_checksum"] = float(attn.double().sum())
    print(json.dumps(line), flush=True)


def child_torch(leg, chunks, reps):
    import numpy as np
    import torch
    from infinite_video_amd.basis_maps import build_plan
    dev = torch.device("cuda:0")
    g = 256 if leg.endswith("g256") else 16
    per = T // g
    bins, _ = _inputs(dev, chunks)
    plan = build_plan(T, N, 0.75)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    entry_box = to(np.repeat(np.arange(N), np.diff(plan.inf_old_ptr)), torch.int64)
    entry_slot = to(plan.inf_old_slot, torch.int64)
    bin_box = to(np.where(plan.bin_box < 0, N, plan.bin_box), torch.int64)      # row N of the extended W is the zero row

    def counts(row_box, row_begin, row_end):
        cnt = np.zeros((N, per), np.float32)
        for b, lo, hi in zip(row_box, row_begin, row_end):
            np.add.at(cnt[b], np.arange(lo, hi) // g, 1)
        return to(cnt, torch.float32)
    cnt_first = counts(plan.first_row_box, plan.first_row_begin, plan.first_row_end)
    cnt_inf = counts(plan.inf_row_box, plan.inf_row_begin, plan.inf_row_end)
    val_first, val_inf = to(plan.first_box_val, torch.float32)[:, None], to(plan.inf_box_val, torch.float32)[:, None]
    M = chunks * per
    W = torch.zeros(L, N + 1, M, device=dev)

    def call():
        W.zero_()
        W[:, :N, :per] = val_first * cnt_first
        for c in range(1, chunks):
            live = (c + 1) * per
            for l in range(L):
                src = bin_box[bins[c, l].long()][entry_slot]
                acc = torch.zeros(N, live, device=dev)
                acc.index_add_(0, entry_box, W[l, :, :live].index_select(0, src))
                acc[:, c * per:] += cnt_inf
                W[l, :N, :live] = val_inf * acc
    call()
    torch.cuda.synchronize()
    ms = _timed(call, reps)
    med = statistics.median(ms)
    print(json.dumps({"leg": leg, "chunks": chunks, "g": g, "columns": M, "reps": reps, "median_ms": round(med, 3),
                      "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "checksum": float(W[:, :N].double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--chunks", type=int, default=2048)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--child", choices=LEGS)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_weights.jsonl"))
    a = ap.parse_args()
    if a.child:
        return (child_torch if a.child.startswith("torch") else child_kernel)(a.child, a.chunks, a.reps)
    legs = [x for x in a.legs.split(",") if x]

    def run_child(leg, rnd):
        reps = a.torch_reps if leg.startswith("torch") else a.reps
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--chunks", str(a.chunks), "--reps", str(reps)],
                           capture_output=True, text=True, timeout=a.child_timeout, cwd=ROOT)
        if r.returncode != 0:                                      # stop here: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"child {leg} of round {rnd} ended with status {r.returncode}")
        line = json.loads(r.stdout.strip().split("\n")[-1])
        line["round"] = rnd
        print(json.dumps(line), flush=True)
        return line

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    lines = []
    for rnd in range(a.rounds):
        for leg in legs:
            lines.append(run_child(leg, rnd))
    per = {leg: [l["median_ms"] for l in lines if l["leg"] == leg] for leg in legs}
    med = {leg: round(statistics.median(v), 3) for leg, v in per.items()}
    summary = {"summary": True, "measure": "source_weights", "chunks": a.chunks, "rounds": a.rounds, "reps_per_child": a.reps,
               "torch_reps_per_child": a.torch_reps, "median_ms": med, "round_medians_ms": per,
               "spread_ms": {leg: round(max(v) - min(v), 3) for leg, v in per.items()},
               "torch_over_kernel": {g: round(med["torch_" + g] / med[g], 1) for g in ("g256", "g16") if g in med and "torch_" + g in med},
               "launches_per_call": {leg: sorted({l["launches_per_call"] for l in lines if l["leg"] == leg}) for leg in legs
                                     if not leg.startswith("torch")},
               "checksums": {leg: sorted({l["checksum"] for l in lines if l["leg"] == leg}) for leg in legs}}
    print(json.dumps(summary), flush=True)
    with open(a.out, "a") as f:
        for l in lines + [summary]:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
