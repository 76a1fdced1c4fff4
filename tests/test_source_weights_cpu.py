"""The source weights without a GPU: the numpy mirror of ``infv_ltm_source_weights`` (``density.source_weights``) against the
closed-form oracle, its grouping and continuation laws, its fp32 form against its float64 form, and the exported symbol.

Identity.  The sparse update is linear in the frame means, so ``W @ kbar`` must reproduce the oracle's ``B_past`` when both walk
the same bins.  The oracle's ``B`` is fp32 (a handful of roundings per chunk), ``W`` is float64: the bound is 1e-6 * max|B|,
about ten times the 6e-8 .. 9e-8 this comparison gives at the three shapes.

fp32 against float64.  Every term of the recurrence is non-negative, so relative errors only add up: a chunk rounds an entry at
most m + 1 times (at most m - 1 additions of resampled rows and one of the count, m being the plan's largest number of operator
rows in one box, and one multiplication), C chunks C * (m + 1) times, each by at most 2^-24.
"""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest

from infinite_video_amd import _lib, density
from infinite_video_amd.basis_maps import NB_BINS, build_plan
from oracle.ltm_oracle import ClosedFormOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.75
SHAPES = ((8, 16, 6), (32, 64, 5), (256, 256, 4))                 # (T, N, chunks)
D = 8                                                            # width of the frame means: the identity holds per column


def random_bins(rng, C, S):
    return rng.integers(0, NB_BINS - 1, size=(C, S)).astype(np.int32)


def oracle_run(T, N, sticky, kbar, bins, resets=(0,)):
    """B_past after every chunk of ``kbar`` [C, T, D] with the oracle resampling ``bins``; a reset before the chunks in ``resets``."""
    rng = np.random.default_rng(5)
    w = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)
    orc = ClosedFormOracle(N, 1, D, TAU, sticky, w(D, D), w(D), w(D, D), w(D), tokens_per_frame=1)
    q = w(2, D)
    out = []
    for c in range(kbar.shape[0]):
        orc.step(kbar[c], q, new_doc=c in resets, u=rng.random(512), bins_override=bins[c] if sticky else None)
        out.append(orc.B_past.copy())
    return out


def rows_per_box(plan):
    m = np.diff(plan.inf_old_ptr).astype(np.int64)
    np.add.at(m, plan.inf_row_box, plan.inf_row_end - plan.inf_row_begin)
    return int(m.max())


@pytest.mark.parametrize("sticky", (True, False), ids=("sticky", "uniform"))
@pytest.mark.parametrize("T,N,C", SHAPES)
def test_w_times_frames_is_the_memory(T, N, C, sticky):
    rng = np.random.default_rng(T + N)
    plan = build_plan(T, N, TAU)
    assert not plan.dense
    kbar = rng.standard_normal((C, T, D)).astype(np.float32)
    bins = random_bins(rng, C, plan.S)
    B = oracle_run(T, N, sticky, kbar, bins)[-1]
    W = density.source_weights(plan, bins if sticky else None, C, frames_per_source=1)
    assert W.shape == (N, C * T) and W.dtype == np.float64
    err = np.abs(W @ kbar.reshape(C * T, D).astype(np.float64) - B).max() / np.abs(B).max()
    print(f"T={T} N={N} C={C} sticky={sticky}: max |W kbar - B_past| / max|B| = {err:.3e}")
    assert err <= 1e-6


def test_a_document_reset_zeroes_the_older_columns():
    T, N, C1, C2 = 8, 16, 3, 3
    rng = np.random.default_rng(11)
    plan = build_plan(T, N, TAU)
    kbar = rng.standard_normal((C1 + C2, T, D)).astype(np.float32)
    bins = random_bins(rng, C1 + C2, plan.S)
    B = oracle_run(T, N, True, kbar, bins, resets=(0, C1))[-1]
    W1 = density.source_weights(plan, bins[:C1], C1, frames_per_source=1)
    assert np.abs(W1).max() > 0
    W2 = density.source_weights(plan, bins[C1:], C2, new_doc=True, W=W1, col_begin=C1 * T, frames_per_source=1)
    assert W2.shape == (N, (C1 + C2) * T)
    assert not W2[:, :C1 * T].any()
    err = np.abs(W2 @ kbar.reshape(-1, D).astype(np.float64) - B).max() / np.abs(B).max()
    assert err <= 1e-6


@pytest.mark.parametrize("T,N,C", SHAPES[:2])
def test_grouped_columns_are_column_sums(T, N, C):
    rng = np.random.default_rng(3)
    plan = build_plan(T, N, TAU)
    bins = random_bins(rng, C, plan.S)
    W1 = density.source_weights(plan, bins, C, frames_per_source=1)
    for g in (4, T):
        Wg = density.source_weights(plan, bins, C, frames_per_source=g)
        assert Wg.shape == (N, C * T // g)
        np.testing.assert_allclose(Wg, W1.reshape(N, C * T // g, g).sum(-1), rtol=1e-12, atol=0)
    # the default is one column per chunk
    assert np.array_equal(density.source_weights(plan, bins, C), density.source_weights(plan, bins, C, frames_per_source=T))


@pytest.mark.parametrize("g", (1, 4))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_two_calls_equal_one(dtype, g):
    T, N, C1, C2 = 8, 16, 2, 4
    rng = np.random.default_rng(4)
    plan = build_plan(T, N, TAU)
    bins = random_bins(rng, C1 + C2, plan.S)
    whole = density.source_weights(plan, bins, C1 + C2, frames_per_source=g, dtype=dtype)
    W1 = density.source_weights(plan, bins[:C1], C1, frames_per_source=g, dtype=dtype)
    W2 = density.source_weights(plan, bins[C1:], C2, new_doc=False, W=W1, col_begin=W1.shape[1], frames_per_source=g, dtype=dtype)
    assert whole.dtype == dtype and np.array_equal(W2, whole)
    with pytest.raises(ValueError):
        density.source_weights(plan, bins[C1:], C2, new_doc=False, W=None, col_begin=W1.shape[1], frames_per_source=g)


@pytest.mark.parametrize("T,N,C", SHAPES)
def test_fp32_mirror_against_float64(T, N, C):
    rng = np.random.default_rng(9)
    plan = build_plan(T, N, TAU)
    bins = random_bins(rng, C, plan.S)
    W64 = density.source_weights(plan, bins, C, frames_per_source=1)
    W32 = density.source_weights(plan, bins, C, frames_per_source=1, dtype=np.float32)
    assert W32.dtype == np.float32
    assert np.array_equal(W32 != 0, W64 != 0)                    # non-negative terms: nothing cancels, nothing appears
    nz = W64 != 0
    rel = np.abs(W32.astype(np.float64)[nz] - W64[nz]) / W64[nz]
    bound = C * (rows_per_box(plan) + 1) * 2.0 ** -24
    print(f"T={T} N={N} C={C}: max relative |fp32 - float64| = {rel.max():.3e}, bound {bound:.3e}")
    assert rel.max() <= bound


def test_a_bin_out_of_range_is_a_zero_row():
    T, N, C = 8, 16, 3
    rng = np.random.default_rng(6)
    plan = build_plan(T, N, TAU)
    bins = random_bins(rng, C, plan.S)
    bad = bins.copy()
    bad[1, ::3] = -1
    bad[2, 5] = NB_BINS - 1
    got = density.source_weights(plan, bad, C, frames_per_source=1)
    # below the range and above it are the same thing: no row
    assert np.array_equal(got, density.source_weights(plan, np.where(bad < 0, 10 ** 6, bad), C, frames_per_source=1))
    # the rows such a bin would resample are absent from the sum
    want = density.source_weights(plan, bins, C, frames_per_source=1)
    assert (got <= want).all() and (got < want).any()


def test_attention_map_and_top_sources():
    T, N, C, g = 8, 16, 4, 4
    rng = np.random.default_rng(8)
    plan = build_plan(T, N, TAU)
    bins = random_bins(rng, C, plan.S)
    mass = rng.uniform(0, 1, (C, N))
    W, attn = density.source_attention(mass, plan, bins, C, frames_per_source=g)
    assert attn.shape == (C, C * T // g) and np.array_equal(W, density.source_weights(plan, bins, C, frames_per_source=g))
    assert np.allclose(attn[-1], mass[-1] @ W, rtol=1e-13)
    for c in range(C - 1):                                       # chunk c cannot attend to frames it has not seen
        assert not attn[c, (c + 1) * T // g:].any() and attn[c, :(c + 1) * T // g].all()
    _, norm = density.source_attention(mass, plan, bins, C, frames_per_source=g, normalise=True)
    assert np.allclose(norm.sum(-1), 1.0, rtol=1e-13)
    top = density.top_sources(attn[-1], 3, frames_per_source=g)
    order = np.argsort(-attn[-1], kind="stable")[:3]
    assert [t[0] for t in top] == list(order)
    assert all(t[1] == t[0] * g and t[2] == (t[0] + 1) * g and t[3] == attn[-1][t[0]] for t in top)


def test_mirror_refuses_what_the_kernel_refuses():
    with pytest.raises(ValueError):
        density.source_weights(build_plan(8, 96, TAU), None, 2)   # a dense plan
    plan = build_plan(8, 16, TAU)
    with pytest.raises(ValueError):
        density.source_weights(plan, None, 2, frames_per_source=3)
    with pytest.raises(ValueError):
        density.source_weights(plan, None, 0)
    with pytest.raises(ValueError):
        density.source_weights(plan, np.zeros((3, plan.S), np.int32), 2)


def test_library_exports_the_symbol_and_the_header_states_the_order():
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6 == _lib.ABI_VERSION
    assert "infv_ltm_source_weights" in _lib.EXPORTED_SYMBOLS
    assert lib.infv_ltm_source_weights is not None
    with open(os.path.join(ROOT, "include", "infv_ltm.h")) as f:
        header = f.read()
    assert "#define INFV_LTM_ABI_VERSION 6" in header
    assert "int infv_ltm_source_weights(" in header and "} infv_ltm_sources_desc;" in header
    for phrase in ("in stored order", "acc += W_old[idx[s]][m]", "added LAST as one fp32 number", "W_new[n][m] = inf_box_val[n] * acc",
                   "W_new[n][m] = first_box_val[n] * cnt_first(n, m)", "long_term_attention_gibbs.py:207-216",
                   "relevant_frames.py:53-69"):
        assert phrase in header, phrase


def test_refusals_in_a_sanitized_host_program(tmp_path):
    """tools/sources_host_check.cpp: the entry point refuses what the header says it refuses, before any device work and with
    nothing launched, the host code built under -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the host check"
    exe = str(tmp_path / "sources_host_check")
    cmd = [hipcc, "-O1", "-g", "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sources_host_check.cpp"),
           os.path.join(ROOT, "infinite-video_amd", "csrc", "ltm_sources.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr[-4000:]
    assert "sources host check: ok" in ran.stdout
    assert "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
