"""What the attention-density read-outs cost (include/infv_ltm.h, "Read-outs ..."), on the headline shape: T 256, P 32, d 768,
N 256, 2 layers, Q 32, sticky, fp32 tokens, max_batch_chunks 42 (bench.py's call).

One CHILD PROCESS per leg and round (a fresh HIP context), the legs ALTERNATED within a round, three rounds by default.  Legs:

  trace_off / trace_on   infv_ltm_consolidate on the 2048-chunk video without / with a mass trace (infv_ltm_set_mass_trace): a
                         child warms the call, times `--reps` calls with device events and reports their median and the
                         kernel launches of one call.  The summary gives the ratio on / off and says whether the difference
                         exceeds the spread (max - min) of the trace-off leg's own round medians.
  density                infv_ltm_density alone (layer 0, after a 64-chunk consolidate): device time per call, median of 200.
  module_off / module_on the drop-in LongTermAttention.forward with output_density off / on: steady-state sticky calls on one
                         layer, end-to-end us per call, median of five blocks of 200 calls (bench.py's module_forward_us).

    timeout -k 10 900 python tools/bench_density_trace.py

--parent-lib PATH (a libinfv_ltm.so built from the parent commit) runs the trace_off leg alone, alternated between that library
and this tree's: nothing in that leg's launches changed, so this tree's median must lie inside the spread of the parent's own
round medians; the summary reports the numbers either way.

    timeout -k 10 600 python tools/bench_density_trace.py --parent-lib PATH

One JSON line per child and one summary line per run are appended to profiles/density_trace.jsonl (--out).  For the per-launch
time of the trace kernel run ONE child under the kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_density_trace.py --child trace_on --reps 3"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, P, D, N, L, Q, H, DH = 256, 32, 768, 256, 2, 32, 12, 64
LEGS = ("trace_off", "trace_on", "density", "module_off", "module_on")
NEW_SYMBOLS = ("infv_ltm_set_grid_plan", "infv_ltm_density", "infv_ltm_masses", "infv_ltm_set_mass_trace")


def _video(dev, chunks):
    import numpy as np
    import torch
    from infinite_video_amd import synth
    gen = torch.Generator(device=dev).manual_seed(1)
    k = torch.empty(chunks, T * P, D, device=dev, dtype=torch.float32)
    for c0 in range(0, chunks, 32):
        k[c0:c0 + 32].normal_(generator=gen)
    u = torch.rand(chunks, L, 512, device=dev, dtype=torch.float64, generator=gen)
    projs = [tuple(torch.from_numpy(x).to(dev) for x in synth.layer_projections(l, D, H * DH)) for l in range(L)]
    q = torch.from_numpy(np.stack([synth.layer_query(l, Q, H * DH) for l in range(L)])).to(dev)
    return k, q, projs, u


def child_consolidate(leg: str, chunks: int, reps: int):
    import torch
    from infinite_video_amd import _lib
    if os.environ.get("INFV_LTM_LIBRARY"):                         # a build of the parent commit lacks the new entry points
        for name in NEW_SYMBOLS:
            _lib._SIGNATURES.pop(name, None)
    from infinite_video_amd.engine import LTMEngine
    dev = torch.device("cuda:0")
    k, q, projs, u = _video(dev, chunks)
    eng = LTMEngine(N, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev, max_batch_chunks=42)
    trace = eng.set_mass_trace(chunks) if leg == "trace_on" else None
    out = torch.empty(chunks, L, Q, H * DH, device=dev)
    for _ in range(2):                                             # warm-up: plans, workspaces
        eng.consolidate(k, q, projs, u, new_doc=True, out=out)
    torch.cuda.synchronize()
    lib = _lib.load()
    n0 = int(lib.infv_ltm_launch_count())
    eng.consolidate(k, q, projs, u, new_doc=True, out=out)
    launches = int(lib.infv_ltm_launch_count()) - n0
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.consolidate(k, q, projs, u, new_doc=True, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    line = {"leg": leg, "chunks": chunks, "reps": reps, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "chunks_per_s": round(chunks / med * 1e3, 1), "launches_per_call": launches,
            "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
            "checksum": float(out.double().sum())}
    if trace is not None:
        line["trace_finite"] = bool(torch.isfinite(trace).all())
        line["trace_row_sum_min"] = float(trace.sum(-1).min())
    print(json.dumps(line), flush=True)


def child_density(reps: int):
    import torch
    from infinite_video_amd.engine import LTMEngine
    dev = torch.device("cuda:0")
    k, q, projs, u = _video(dev, 64)
    eng = LTMEngine(N, H, DH, D, P, tau=0.75, sticky=True, n_layers=L, max_q=Q, device=dev, max_batch_chunks=42)
    eng.consolidate(k, q, projs, u, new_doc=True)
    for _ in range(20):
        eng.density(0, Q)
        eng.masses(0, Q)
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("density", lambda: eng.density(0, Q)), ("masses", lambda: eng.masses(0, Q))):
        us = []
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        res[name + "_device_us"] = round(statistics.median(us), 2)
    print(json.dumps(dict({"leg": "density", "what": "infv_ltm_density / infv_ltm_masses alone, layer 0, N 256, Q 32, 768 points, "
                           "device time between events around one call, median of 200"}, **res)), flush=True)


def child_module(leg: str):
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.long_term_attention_gibbs import LongTermAttention
    dev = torch.device("cuda:0")
    wk, bk, wv, bv = synth.layer_projections(0, D, H * DH)
    pk, pv = torch.nn.Linear(D, H * DH), torch.nn.Linear(D, H * DH)
    with torch.no_grad():
        pk.weight.copy_(torch.from_numpy(wk)); pk.bias.copy_(torch.from_numpy(bk))
        pv.weight.copy_(torch.from_numpy(wv)); pv.bias.copy_(torch.from_numpy(bv))
    m = LongTermAttention(head_size=DH, length=D, target_len=D, attn_func="softmax", attn_num_basis=N, continuous=True,
                          attn_drop=0.1, infinite_memory=True, n_layers=L, n_heads=H, affines=True, mask=True, mask_type="cnn",
                          kl_regularizer=False, proj_key=pk.to(dev), proj_value=pv.to(dev), sigma_0=None, mu_0=None,
                          sticky_memories=True, sigmas=None, tau=0.75, d_model=H * DH)
    m.output_density = leg == "module_on"
    gen = torch.Generator(device=dev).manual_seed(1)
    ks = [torch.randn(1, T * P, D, device=dev, generator=gen) for _ in range(8)]
    qq = torch.randn(1, Q, H * DH, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    torch.manual_seed(0)
    for c in range(300):
        m(ks[c % len(ks)], qq, new_doc=(c == 0), layer_n=0)
    torch.cuda.synchronize()
    n, res = 200, []
    lib = _lib.load()
    l0 = int(lib.infv_ltm_launch_count())
    for _ in range(5):
        t0 = time.perf_counter()
        for c in range(n):
            m(ks[c % len(ks)], qq, new_doc=False, layer_n=0)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0, t1 - t0))
    launches = (int(lib.infv_ltm_launch_count()) - l0) / (5 * n)
    res.sort()
    e2e, host = res[len(res) // 2]
    print(json.dumps({"leg": leg, "end_to_end_us": round(1e6 * e2e / n, 2), "host_issue_us": round(1e6 * host / n, 2),
                      "best_block_us": round(1e6 * res[0][0] / n, 2), "launches_per_call": launches}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunks", type=int, default=2048)
    ap.add_argument("--child", choices=LEGS)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-lib", metavar="PATH", help="trace_off leg alone, alternated between this build of the parent commit and this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_trace.jsonl"))
    a = ap.parse_args()
    if a.child in ("trace_off", "trace_on"):
        return child_consolidate(a.child, a.chunks, a.reps)
    if a.child == "density":
        return child_density(a.reps)
    if a.child:
        return child_module(a.child)

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
        print(json.dumps(line), flush=True)
        return line

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    lines = []
    if a.parent_lib:
        for rnd in range(a.rounds):
            for side, library in (("parent", a.parent_lib), ("branch", None)):
                lines.append(dict(run_child("trace_off", rnd, library), side=side))
        per = {side: [l["median_ms"] for l in lines if l["side"] == side] for side in ("parent", "branch")}
        mp, mb = statistics.median(per["parent"]), statistics.median(per["branch"])
        summary = {"summary": True, "measure": "parent_vs_branch", "leg": "trace_off", "chunks": a.chunks, "rounds": a.rounds,
                   "reps_per_child": a.reps, "parent_ms": round(mp, 3), "branch_ms": round(mb, 3), "round_medians_ms": per,
                   "branch_minus_parent_ms": round(mb - mp, 3), "parent_spread_ms": round(max(per["parent"]) - min(per["parent"]), 3),
                   "inside_parent_spread": bool(min(per["parent"]) <= mb <= max(per["parent"])),
                   "launches_per_call": {side: sorted({l["launches_per_call"] for l in lines if l["side"] == side}) for side in per},
                   "same_checksum": len({l["checksum"] for l in lines}) == 1}
    else:
        for rnd in range(a.rounds):
            for leg in LEGS:
                lines.append(run_child(leg, rnd))
        per = {leg: [l["median_ms"] for l in lines if l["leg"] == leg] for leg in ("trace_off", "trace_on")}
        off, on = statistics.median(per["trace_off"]), statistics.median(per["trace_on"])
        spread = max(per["trace_off"]) - min(per["trace_off"])
        mod = {leg: statistics.median([l["end_to_end_us"] for l in lines if l["leg"] == leg]) for leg in ("module_off", "module_on")}
        last = lambda leg, key: [l[key] for l in lines if l["leg"] == leg][-1]
        summary = {"summary": True, "measure": "trace_and_density", "chunks": a.chunks, "rounds": a.rounds, "reps_per_child": a.reps,
                   "trace_off_ms": round(off, 3), "trace_on_ms": round(on, 3), "round_medians_ms": per,
                   "on_over_off": round(on / off, 4), "on_minus_off_ms": round(on - off, 3), "trace_off_spread_ms": round(spread, 3),
                   "trace_costs_more_than_the_off_spread": bool(on - off > spread),
                   "launches_per_call": {"trace_off": last("trace_off", "launches_per_call"), "trace_on": last("trace_on", "launches_per_call")},
                   "same_checksum": len({l["checksum"] for l in lines if "checksum" in l}) == 1,
                   "density_device_us": statistics.median([l["density_device_us"] for l in lines if l["leg"] == "density"]),
                   "masses_device_us": statistics.median([l["masses_device_us"] for l in lines if l["leg"] == "density"]),
                   "module_forward_us": {k: round(v, 2) for k, v in mod.items()},
                   "module_launches_per_call": {leg: last(leg, "launches_per_call") for leg in mod}}
    print(json.dumps(summary), flush=True)
    with open(a.out, "a") as f:
        for l in lines + [summary]:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
