#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of the library on the LTM entry points (the counterpart of tools/vqf_dump.py): a fixed list
of calls on seeded inputs, run in a fresh child process per build, one after the other, each under its own time limit; every ``ctx``,
per layer the exported ``B`` and bin mass, ``last_draw``, the chain-state blob, the packed memory and the ``infv_ltm_launch_count()``
delta of each call go into an ``.npz``, and the two files must agree on their bytes.

usage: python tools/ltm_dump.py OTHER_DIR [REPORT.txt]      (OTHER_DIR holds the other build's libinfv_ltm.so and libinfv_ltm_exp.so)

Shipped against shipped, one child per build: the list below, forward and then in reverse ON THE SAME HANDLES, so that every workspace
is seen growing and not growing.  Experiments build against experiments build: the 70 + 5 chunk case under each entry of
tests/test_timed_path_gpu.py's ``_VARIANTS``, a child per build and entry (the knobs are read once per process).

The list.  Headline shape (tests/test_timed_path_gpu.py, max_batch_chunks=42): 70 chunks then a 5-chunk continuation on a default
handle and on handles created under INFV_PROJ_X6=0 and INFV_VPROJ_SPLIT=1; one 768-chunk fp32 call with tokens generated on the
device (the shortest call that takes the call-long pooling launch, its planes and the small-tile last sub-batch).  Small shape
(N 64, T 8, Q 32, 2 layers), every call followed by a new_doc=0 call: consolidate_pooled; consolidate from fp16, bf16 and fp8 tokens;
u=None with the device rng; set_ctx_sum then pack_memory; a draw trace; Q=8, which fused_chain_holds refuses; a dense (Gaussian)
plan.  The lockstep calls: consolidate_videos, steps_videos with a shared and a per-chunk query and steps_videos_from with chunk
counts (2, 0, 3), new_doc 1 then 0; 257 one-chunk videos (more than kVideoGroup); N=272, which videos_supported refuses."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = dict(N=64, H=12, dh=64, d=768, P=32, T=8, Q=32, L=2)


def child(path, mode):
    import torch
    from infinite_video_amd import _lib, synth
    from infinite_video_amd.engine import LTMEngine, consolidate_videos, steps_videos
    from tests.golden.cases import GAUSS_SIGMAS
    from tests.test_timed_path_gpu import _engine, _video

    dev, lib = torch.device("cuda:0"), _lib.load()
    out, tag = {}, ["forward"]
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    def counted(key, fn):
        n0 = lib.infv_ltm_launch_count()
        res = fn()
        torch.cuda.synchronize()
        out[key + "/launches"] = np.int64(lib.infv_ltm_launch_count() - n0)
        out[key + "/ctx"] = host(res)
        return res

    def keep(key, e, Q=None, fast=True):
        e.sync()
        for l in range(e.L):
            B, mass = e.export_state(l)
            out[f"{key}/B{l}"], out[f"{key}/mass{l}"] = host(B), host(mass)
            for name, a in zip(("bins", "idx", "probs"), e.last_draw(l)):
                out[f"{key}/{name}{l}"] = a
        if fast and Q:
            out[key + "/blob"] = host(e.export_chain_state(Q).view(torch.int32))

    def made_under(env, make):                                  # (INFV_PROJ_X6 / INFV_VPROJ_SPLIT are read when the handle is created)
        os.environ.update(env)
        e = make()
        for k in env:
            del os.environ[k]
        return e

    # ---- headline shape: 70 chunks, then a 5-chunk continuation (two 32-chunk sub-batches + a short one)
    k75, q_h, projs_h, u75, _, _ = _video(dev, 75)

    def variant_case(name, e):
        def run():
            key = f"{tag[0]}/variant/{name}"
            counted(key + "/a", lambda: e.consolidate(k75[:70], q_h, projs_h, u75[:70], new_doc=True))
            counted(key + "/b", lambda: e.consolidate(k75[70:], q_h, projs_h, u75[70:], new_doc=False))
            keep(key, e, 32)
        return run

    if mode == "exp":
        variant_case("knobs", _engine(dev, max_batch_chunks=42))()
        np.savez(path, **out)
        return

    heads = {"default": _engine(dev, max_batch_chunks=42),
             "x6_off": made_under({"INFV_PROJ_X6": "0"}, lambda: _engine(dev, max_batch_chunks=42)),
             "vsplit": made_under({"INFV_VPROJ_SPLIT": "1"}, lambda: _engine(dev, max_batch_chunks=42))}

    def long_case():
        def run():
            k = torch.empty(768, 256 * 32, 768, device=dev, dtype=torch.float32)
            gen = torch.Generator(device=dev).manual_seed(31)
            for i in range(0, 768, 64):
                k[i:i + 64].normal_(generator=gen)
            u = torch.from_numpy(synth.gibbs_uniforms(768, 2, seed=32)).to(dev)
            key = f"{tag[0]}/long768"
            counted(key, lambda: heads["default"].consolidate(k, q_h, projs_h, u, new_doc=True))
            keep(key, heads["default"], 32)
        return run

    # ---- small shape
    s = SMALL
    dm = s["H"] * s["dh"]
    ws = [synth.layer_projections(l, s["d"], dm) for l in range(s["L"])]
    projs = [tuple(torch.from_numpy(a).to(dev) for a in w) for w in ws]
    qs = lambda Q: torch.from_numpy(np.stack([synth.layer_query(l, Q, dm) for l in range(s["L"])])).to(dev)
    toks = lambda c0, n: torch.from_numpy(np.stack([synth.frame_tokens(c, s["T"], s["P"], s["d"]) for c in range(c0, c0 + n)])).to(dev)
    unif = lambda n, seed: torch.from_numpy(synth.gibbs_uniforms(n, s["L"], seed=seed)).to(dev)
    small = lambda **kw: LTMEngine(s["N"], s["H"], s["dh"], s["d"], s["P"], tau=0.75, sticky=True, n_layers=s["L"], max_q=s["Q"],
                                   device=dev, **kw)
    k9, k4 = toks(0, 9), toks(9, 4)
    engines = {n: small() for n in ("pooled", "f16", "bf16", "f8", "sum", "trace", "q8")}
    engines["f16"].fp16_tokens = True
    engines["rng"] = small(rng_seed=77, rng_stream=3)
    engines["dense"] = small(gaussian_sigmas=GAUSS_SIGMAS)
    engines["sum"].set_ctx_sum(True)

    def small_case(name):
        def run():
            e, key, Q = engines[name], f"{tag[0]}/small/{name}", 8 if name == "q8" else s["Q"]
            cast = {"f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn}.get(name)
            if name == "trace":
                tr = e.set_trace(13)
            for i, (k, new) in enumerate(((k9, True), (k4, False))):
                u = None if name == "rng" else unif(k.shape[0], 40 + i)
                if name == "pooled":
                    call = lambda: e.consolidate_pooled(e.pool(k), qs(Q), projs, u, new_doc=new)
                else:
                    kk = (k * 0.3).to(cast) if cast else k
                    call = lambda: e.consolidate(kk, qs(Q), projs, u, new_doc=new)
                ctx = counted(f"{key}/call{i}", call)
                keep(f"{key}/call{i}", e, Q, fast=name not in ("q8", "dense"))
                if name == "sum":
                    out[f"{key}/call{i}/packed"] = host(e.pack_memory(ctx, with_scores=True))
            if name == "trace":
                out[key + "/trace_bins"], out[key + "/trace_probs"] = host(tr[0]), host(tr[1])
                e.set_trace(0)
        return run

    # ---- the lockstep calls
    def videos_case(name, counts, N=s["N"]):
        mk = lambda: LTMEngine(N, s["H"], s["dh"], s["d"], s["P"], tau=0.75, sticky=True, n_layers=s["L"], max_q=s["Q"], device=dev)
        es = [mk() for _ in counts]

        def run():
            key = f"{tag[0]}/videos/{name}/{len(counts)}x{N}"
            for i, new in enumerate((True, False)):
                cs = counts if new else [c for c in counts if c]
                live = es if new else [e for e, c in zip(es, counts) if c]      # (only a video that has a memory can continue it)
                k = toks(20 * i, sum(cs))
                u = unif(sum(cs), 50 + i)
                kbar = es[0].pool(k)
                if name == "tokens":
                    call = lambda: consolidate_videos(live, k, cs, qs(s["Q"]), projs, u, new_doc=new)
                elif name == "steps":
                    call = lambda: steps_videos(live, kbar, cs, qs(s["Q"]), projs, u, new_doc=new)
                elif name == "steps_q":
                    call = lambda: steps_videos(live, kbar, cs, qs(s["Q"]).unsqueeze(0).repeat(sum(cs), 1, 1, 1) * 1.01, projs, u, new_doc=new)
                else:                                              # every video reads the block's first chunks
                    call = lambda: steps_videos(live, kbar, cs, qs(s["Q"]), projs, u, new_doc=new, kbar_chunk0=[0] * len(cs))
                counted(f"{key}/call{i}", call)
                for v in (0, len(live) - 1):
                    keep(f"{key}/call{i}/v{v}", live[v], fast=False)
        return run

    def cases():
        lst = [variant_case(n, e) for n, e in heads.items()] + [long_case()]
        lst += [small_case(n) for n in engines]
        lst += [videos_case(n, (2, 0, 3)) for n in ("tokens", "steps", "steps_q", "steps_from")]
        return lst + [videos_case("tokens", (1,) * 257), videos_case("steps", (2, 0, 3), N=272)]

    lst = cases()
    for run in lst + lst[::-1]:                                    # the same handles again, last case first
        run()
        if run is lst[-1]:
            tag[0] = "reverse"
    np.savez(path, **out)


def run_children(other_lib, tree_lib, mode, env_add):
    dumps = []
    for lib in (other_lib, tree_lib):
        path = tempfile.mktemp(suffix=".npz")
        env = dict(os.environ, INFV_LTM_LIBRARY=lib, **env_add)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, mode], check=True, env=env, cwd=ROOT, timeout=900)
        print(f"[ltm_dump] {mode} {env_add} {lib or 'tree'}: done", file=sys.stderr, flush=True)
        dumps.append({k: v for k, v in np.load(path).items()})
        os.remove(path)
    return dumps


def compare(title, a, b, lines):
    raw = lambda x: np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
    bad = sorted(set(a) ^ set(b))
    lines += [f"{title}: only in one dump: {k}" for k in bad]
    launches = []
    for k in sorted(set(a) & set(b)):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not np.array_equal(raw(a[k]), raw(b[k])):
            bad.append(k)
            lines.append(f"{title}: DIFFERENT {k}: other {a[k].ravel()[:4]} tree {b[k].ravel()[:4]}")
        if k.endswith("/launches"):
            launches.append(f"{k.rsplit('/', 1)[0]} {int(b[k])}")
    finite = all(np.isfinite(v.astype(np.float64)).all() for v in b.values() if v.dtype.kind == "f")
    lines.append(f"{title}: {len(b) - len(launches)} arrays and {len(launches)} launch counts agree bit for bit: {not bad}; "
                 f"every float array finite: {finite}")
    lines.append(f"{title}: launches per call: " + ", ".join(launches))
    return not bad and finite and len(b) > len(launches)


def main():
    from tests.test_timed_path_gpu import _VARIANTS
    other = os.path.abspath(sys.argv[1])
    report = sys.argv[2] if len(sys.argv) > 2 else None
    lines = [f"ltm_dump: the build in {other} against the tree's"]
    ok = compare("shipped", *run_children(os.path.join(other, "libinfv_ltm.so"), "", "shipped", {}), lines)
    for v in _VARIANTS:
        title = "exp " + (" ".join(f"{k}={x}" for k, x in v.items()) or "(no knob)")
        ok = compare(title, *run_children(os.path.join(other, "libinfv_ltm_exp.so"), "exp", "exp", v), lines) and ok
    lines.append("LTM_DUMP_OK" if ok else "LTM_DUMP_FAIL")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
