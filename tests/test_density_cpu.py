"""The attention-density read-outs without a GPU: the float64 mirror against the reference's own pickle, the grid plan, the
exported symbols, and the refusals of the setters in a stand-alone host program under the address / undefined-behaviour
sanitizers.

Bound of the mirror against the golden ``alphas``: the reference's own fp32 arithmetic lies within 4.9e-7 (relative) of the
float64 closed form on its own scores; the comparison gets four times that, EPS = 2e-6.
"""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from infinite_video_amd import _lib, density
from infinite_video_amd.basis_maps import REFERENCE_DENSITY_SEGMENTS, build_grid_plan
from tests.golden.cases import CASES, DENSE_CASES, GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2e-6
DENSITY_CASES = ("cfg1_sticky", "peaked", "tau09", "n144", "n96_dense", "headline")
BY_NAME = {c.name: c for c in CASES + DENSE_CASES}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "density.npz"))


@pytest.mark.parametrize("name", DENSITY_CASES)
def test_mirror_equals_the_reference_pickle(golden, name):
    case = BY_NAME[name]
    gp = build_grid_plan(case.N)
    calls = sorted(k[:-len("_alphas")] for k in golden.files if k.startswith(name + "/") and k.endswith("_alphas"))
    assert len(calls) == 2 * case.n_layers                       # every layer of the second and of the last chunk
    worst = 0.0
    for tag in calls:
        want = golden[tag + "_alphas"].astype(np.float64)        # [nq, 1, H, 768]
        got = density.reference_alphas(golden[tag + "_scores"], gp)
        assert got.shape == want.shape
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    print(f"{name}: max relative |mirror - reference pickle| = {worst:.3e} over {len(calls)} calls")
    assert worst <= EPS


def test_reference_grid_plan():
    gp = build_grid_plan(64)
    assert gp.segments == REFERENCE_DENSITY_SEGMENTS
    assert len(gp.t) == 768 and list(gp.seg_begin) == [0, 256, 512, 768]
    count = np.diff(gp.pt_ptr)
    assert count[-1] == 0 and gp.t[-1] == 1.0                    # t = 1.0 lies in no box
    assert (count[:-1] == 1).all()                               # a box partition: one entry of value 1 everywhere else
    assert (gp.pt_val == 1).all()
    assert gp.t[255] == 0.25 == gp.t[256] and gp.t[511] == 0.5 == gp.t[512]   # the seams are present twice
    for g, (lo, hi, _) in enumerate(gp.segments):                # the weights of a segment sum to its length
        w = gp.pt_weight[gp.seg_begin[g]:gp.seg_begin[g + 1]].astype(np.float64)
        assert abs(w.sum() - (hi - lo)) <= 1e-6
    # membership is the reference's fp32 box test: 0.25 is the lower bound of box 16 of 64
    assert gp.pt_box[gp.pt_ptr[255]] == 16 and gp.pt_box[gp.pt_ptr[256]] == 16


def test_overlapping_boxes_give_two_entry_points():
    gp = build_grid_plan(96)
    count = np.diff(gp.pt_ptr)
    assert count.max() == 2 and (count == 2).sum() >= 1
    m = int(np.flatnonzero(count == 2)[0])
    a, b = gp.pt_box[gp.pt_ptr[m]:gp.pt_ptr[m + 1]]
    assert b == a + 1                                            # adjacent boxes, ascending
    # s(t) at such a point is the fp32 sum of the two scores, in CSR order
    S = np.zeros((1, 1, 96), np.float32)
    S[0, 0, a], S[0, 0, b] = 1.25, -0.5
    assert density.grid_scores(S, gp)[0, 0, m] == np.float32(0.75)


def test_other_grids():
    gp = build_grid_plan(64, ((0.0, 1.0, 1000),))
    assert len(gp.t) == 1000 and list(gp.seg_begin) == [0, 1000]
    rng = np.random.default_rng(0)
    a = density.reference_alphas(rng.standard_normal((3, 5, 64)).astype(np.float32), gp)
    assert a.shape == (5, 1, 3, 1000)
    assert np.allclose(a.sum(-1), 1.0, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        build_grid_plan(64, ((0.0, 1.0, 1),))
    with pytest.raises(ValueError):
        build_grid_plan(64, ((0.0, 1.0, 5000),))


def test_mirror_stays_finite_where_the_reference_formula_overflows():
    gp = build_grid_plan(64)
    rng = np.random.default_rng(1)
    S = rng.uniform(-200, 200, size=(2, 3, 64)).astype(np.float32)
    S[0, 0, 7] = 200.0
    assert np.abs(S).max() == 200.0
    a = density.reference_alphas(S, gp)
    assert np.isfinite(a).all() and np.allclose(a.sum(-1), 1.0, atol=1e-12)
    m = density.box_masses(S, np.full(64, 1 / 64), 1e-3)
    assert np.isfinite(m).all() and 0.99 < m.sum() <= 1.0
    # the reference's own formula (:248, no maximum subtracted) in its own fp32
    s = torch.from_numpy(density.grid_scores(S, gp))
    t = torch.from_numpy(gp.t[:256])
    with np.errstate(all="ignore"):
        prob = torch.exp(s[..., :256]) / torch.trapz(torch.exp(s[..., :256]), t, dim=-1).unsqueeze(-1)
    assert not torch.isfinite(prob).all()


def test_box_masses_closed_form():
    rng = np.random.default_rng(2)
    S = rng.standard_normal((2, 4, 16))
    w = rng.uniform(0.01, 0.1, 16)
    a = density.box_weights(S, w, 0.001)
    want = w * np.exp(S) / ((w * np.exp(S)).sum(-1, keepdims=True) + 0.001)
    assert np.allclose(a, want, rtol=1e-13)
    assert np.allclose(density.box_masses(S, w, 0.001), want.reshape(-1, 16).mean(0), rtol=1e-13)


def test_library_exports_the_symbols():
    lib = _lib.load()
    assert lib.infv_ltm_abi_version() == 6 == _lib.ABI_VERSION
    for name in ("infv_ltm_set_grid_plan", "infv_ltm_density", "infv_ltm_masses", "infv_ltm_set_mass_trace"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "include", "infv_ltm.h")) as f:
        header = f.read()
    assert "#define INFV_LTM_ABI_VERSION 6" in header
    for name in ("infv_ltm_set_grid_plan", "infv_ltm_density", "infv_ltm_masses", "infv_ltm_set_mass_trace"):
        assert f"int {name}(" in header


def test_refusals_in_a_sanitized_host_program(tmp_path):
    """tools/density_host_check.cpp: the setters and the two read-outs refuse what the header says they refuse, before any
    device work, with the host code built under -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the host check"
    exe = str(tmp_path / "density_host_check")
    cmd = [hipcc, "-O1", "-g", "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "density_host_check.cpp"),
           os.path.join(ROOT, "infinite-video_amd", "csrc", "ltm_density.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr[-4000:]
    assert "density host check: ok" in ran.stdout
    assert "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
