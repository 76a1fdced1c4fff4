"""The Gibbs draw at the edges of its cdf: probability regimes, edge uniforms and the shapes that route a call to each of
the library's implementations of the draw.  Seeded, nothing stored; the arithmetic is numpy's (torch enters once, through
``oracle.ltm_oracle.categorical_probs``, which normalises ``dense`` as the library's input is normalised, and the routing shapes
are those of ``tests/golden/sweep_cases.py``).

The contract (csrc/ltm_device.h above ``DrawRegs``; ``oracle.ltm_oracle.inverse_cdf_draw``; pinned against
``torch.multinomial`` in tests/test_oracle_golden.py): the fp32 SEQUENTIAL running sum of the 127 bin probabilities in bin
order, divided by its total, the last bucket forced to 1, a lower-bound search of each float64 uniform (``cdf[j] < u``).
Given identical probabilities the draw is bit-exact, so every comparison made from this table is integer bins against
``inverse_cdf_draw``, equal or not: there is no tolerance anywhere in it.

One consequence of the lower bound that the tests state instead of hiding: ``u == 0.0`` is above no cdf entry, so it draws
bin 0 even when bin 0 has probability zero.  That is torch's own behaviour (``torch.multinomial`` returns the lower bound of
its uniform in the cdf and never looks at the bucket's mass), and it is the ONLY way a regime of this table draws a bin of
probability zero: ``u == 0.0`` with a leading zero bin.

What each regime is for
  dense               random, strictly positive, normalised as ``categorical_probs`` does: the everyday input.
  plateaus            ``dense`` with runs of zero bins -> runs of EQUAL cdf entries: a leading run (bins 0-2), a run across the
                      seam of two 8-entry search groups (6-8), a run longer than a group (15-24), a run across the lane-63 /
                      lane-64 carry of the systolic scan (60-69) and a trailing run (120-126).  Not renormalised: the total is
                      well below 1, so the division matters too.
  onehot_j            all mass in one bin, j at a group's start / end and at the wave seam.
  decades_asc / desc  masses 2**uniform(-60, 0), sorted: the fp32 sum absorbs terms, so the sequential scan and any other
                      association differ in the last bit of many entries.  Not normalised.
  unnormalised_*      ``dense`` times 3.7 and times 1.3e-3: ``c / run`` against ``c * (1 / run)``.
No non-zero probability is subnormal (what the hardware's scan and division do with fp32 subnormals is a separate question).

Uniforms: ``edge_uniforms(p, S)`` holds, for every distinct value c of the oracle's own fp32 cdf of p, the doubles just below,
at and just above c that lie in [0, 1), plus 0.0, 2**-53 and 1 - 2**-53 -- at most 384 values -- filled up to S with seeded
uniforms.  The edge values take the first slots of a seeded slot order built so that they land in every lane of a wave and every
thread of the 256-thread draw kernels wherever the regime has 64 / 256 of them (``slot_order``).  A shape with fewer samples than edge values takes them in consecutive pieces,
one step per piece (``n_pieces``).
"""
from __future__ import annotations

import zlib
from collections import OrderedDict
from dataclasses import replace
from typing import Dict, List

import numpy as np

from tests.golden import sweep_cases as sc

NB = 127                                   # bins drawn from (kBins - 1)
# Whether ``c * (1 / run)`` differs from ``c / run`` anywhere depends on the total ``run`` alone (for some totals the two agree in
# all 127 entries), so not every seed gives every regime the power the CPU test asserts: this is the first seed from 20261020 on
# at which each mistake restated in tests/test_draw_edges_cpu.py changes a bin in every regime it is listed for.
SEED = 20261023
PLATEAU_RUNS = ((0, 2), (6, 8), (15, 24), (60, 69), (120, 126))      # inclusive bin ranges set to zero
ONEHOT_BINS = (0, 7, 8, 63, 64, 126)
MAX_EDGE_VALUES = 3 * NB + 3


# ---------------------------------------------------------------------------------------------------------------------
# probability regimes
# ---------------------------------------------------------------------------------------------------------------------
def dense_raw() -> np.ndarray:
    """The unnormalised masses behind ``dense``: strictly positive, up to a factor 1000 between bins."""
    return (np.random.default_rng(SEED).random(NB) ** 2 + 1e-3).astype(np.float32)


def _dense() -> np.ndarray:
    import torch
    from oracle.ltm_oracle import categorical_probs
    return categorical_probs(torch.from_numpy(dense_raw())).numpy().astype(np.float32)


def _regimes() -> "OrderedDict[str, np.ndarray]":
    dense = _dense()
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    out["dense"] = dense
    plat = dense.copy()
    for lo, hi in PLATEAU_RUNS:
        plat[lo:hi + 1] = 0
    out["plateaus"] = plat
    for j in ONEHOT_BINS:
        p = np.zeros(NB, np.float32)
        p[j] = 1
        out[f"onehot_{j}"] = p
    dec = np.sort((2.0 ** np.random.default_rng(SEED + 1).uniform(-60, 0, NB)).astype(np.float32))
    out["decades_asc"] = dec
    out["decades_desc"] = np.ascontiguousarray(dec[::-1])
    out["unnormalised_big"] = (dense * np.float32(3.7)).astype(np.float32)
    out["unnormalised_small"] = (dense * np.float32(1.3e-3)).astype(np.float32)
    for name, p in out.items():
        assert p.dtype == np.float32 and p.shape == (NB,), name
        nz = p[p != 0]
        assert (p >= 0).all() and nz.size and (nz >= np.finfo(np.float32).tiny).all(), f"{name}: negative or subnormal entry"
    return out


REGIMES: "OrderedDict[str, np.ndarray]" = _regimes()
REGIME_NAMES: List[str] = list(REGIMES)


# ---------------------------------------------------------------------------------------------------------------------
# the cdf and its edges
# ---------------------------------------------------------------------------------------------------------------------
def oracle_cdf(p: np.ndarray) -> np.ndarray:
    """The fp32 cdf ``inverse_cdf_draw`` searches (its own statements; tests/test_draw_edges_cpu.py ties the two together)."""
    p = np.asarray(p, np.float32)
    run = np.float32(0)
    cdf = np.empty(len(p), np.float32)
    for j in range(len(p)):
        run = np.float32(run + p[j])
        cdf[j] = run
    cdf = (cdf / run).astype(np.float32)
    cdf[-1] = np.float32(1)
    return cdf


def edge_values(p: np.ndarray) -> np.ndarray:
    """Sorted, distinct float64 edge values of the regime: around every distinct cdf value, and the ends of [0, 1)."""
    c = np.unique(oracle_cdf(p)).astype(np.float64)
    v = np.concatenate([np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf), [0.0, 2.0 ** -53, 1.0 - 2.0 ** -53]])
    v = np.unique(v[(v >= 0.0) & (v < 1.0)])
    assert v.size <= MAX_EDGE_VALUES
    return v


def n_pieces(p: np.ndarray, S: int) -> int:
    """Steps of S uniforms that it takes to present every edge value of the regime."""
    return -(-edge_values(p).size // S)


def slot_order(S: int) -> np.ndarray:
    """A seeded order of the S sample slots in which every prefix of n slots holds min(n, 64, S) different residues mod 64 (the lanes
    of a wave) and min(n, 256, S) different residues mod 256 (the threads of the 256-thread draw kernels): the first 64 slots are one
    per lane, the next up to 192 complete the thread residues, the rest follow.  Depends on S alone."""
    cand = np.random.default_rng([SEED, S]).permutation(S)
    lanes, threads, tiers = set(), set(), ([], [], [])
    for s in cand:
        if s % 64 not in lanes:
            lanes.add(s % 64)
            threads.add(s % 256)
            tiers[0].append(s)
    for s in cand:
        if s % 256 not in threads:
            threads.add(s % 256)
            tiers[1].append(s)
    taken = set(tiers[0]) | set(tiers[1])
    tiers[2].extend(s for s in cand if s not in taken)
    order = np.array(tiers[0] + tiers[1] + tiers[2], np.int64)
    assert np.array_equal(np.sort(order), np.arange(S))
    return order


def edge_uniforms(p: np.ndarray, S: int, piece: int = 0) -> np.ndarray:
    """Exactly S float64 uniforms in [0, 1): piece ``piece`` of the regime's edge values (all of them when S holds them) in a seeded
    order at the first slots of ``slot_order(S)``, seeded uniforms in the remaining slots.  So n edge values land in min(n, 64, S)
    different lanes and min(n, 256, S) different threads of the draw kernels' strides: in every one of them where the regime has
    that many (tests/test_draw_edges_cpu.py asserts these counts for every regime and piece)."""
    ev = edge_values(p)
    part = ev[piece * S:(piece + 1) * S]
    assert part.size or piece == 0
    key = zlib.crc32(np.asarray(p, np.float32).tobytes())
    rng = np.random.default_rng([SEED, key, S, piece])
    u = np.empty(S, np.float64)
    order = slot_order(S)
    u[order[:part.size]] = rng.permutation(part)
    u[order[part.size:]] = rng.random(S - part.size)
    return u


def count_edges(p: np.ndarray, u: np.ndarray) -> int:
    """How many of the uniforms are edge values of the regime (the parity lines state it)."""
    return int(np.isin(u, edge_values(p)).sum())


def round_up_f32(u: np.ndarray) -> np.ndarray:
    """numpy mirror of csrc/philox.h ``round_up_f32``: the smallest float >= u (what chain_batch3_kernel's search compares
    against: ``c < uf`` in fp32 must equal ``(double)c < u``)."""
    u = np.asarray(u, np.float64)
    f = u.astype(np.float32)                                  # round to nearest even
    bits = f.view(np.uint32).copy()
    bits[f.astype(np.float64) < u] += np.uint32(1)            # u >= 0: the next float up is the next bit pattern
    return bits.view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# routing: one shape per implementation of the draw (shapes of tests/golden/sweep_cases.py)
# ---------------------------------------------------------------------------------------------------------------------
def _route(pt: sc.SweepPoint) -> sc.SweepPoint:
    return replace(pt, n_chunks=2, chunk_T=None)              # the first chunk and one continuation step


# role-S kernel of infv_ltm_consolidate -> the shape that selects it (asserted through sweep_cases.expected_path on the CPU)
ROLE_S: Dict[str, sc.SweepPoint] = {
    "chain_batch3": _route(sc.SMALL),                         # the shipped headline path: own scan, fp32 search
    "chain_batch": _route(sc.BY_NAME["H16_Q8"]),              # fails batch3.Q>8: persistent, float64 compare
    "chain_kernel": _route(sc.BY_NAME["vc2_wgs"]),            # fails batch.wgs<=384: one launch per chunk, draw_finish<kNT, 1>
}
# ... and two with fewer samples than edge values (several pieces; S off the 256-thread stride, ragged last float4 of uniforms)
ROLE_S_SHORT: Dict[str, sc.SweepPoint] = {
    "chain_batch3": _route(sc.BY_NAME["S100"]),
    "chain_batch": _route(sc.BY_NAME["S102"]),                # fails batch3.S%4
}
PER_CALL = _route(sc.SMALL)                                   # sparse plan: step_project_kernel (forward), draw_kernel (steps), lockstep
DENSE_N, DENSE_T = 96, 16                                     # a num_basis whose fp32 boxes overlap: dense plan, draw_kernel
GAUSS_N, GAUSS_T, GAUSS_SIGMAS = 64, 16, (0.03, 0.1)          # the Gaussian family: psi plan, draw_kernel


def layer_regimes(round_: int, L: int) -> List[str]:
    """A different regime per layer; rounds 0 .. n_rounds(L) - 1 cycle through all of them."""
    n = len(REGIME_NAMES)
    return [REGIME_NAMES[(round_ * L + l) % n] for l in range(L)]


def n_rounds(L: int) -> int:
    return -(-len(REGIME_NAMES) // L)
