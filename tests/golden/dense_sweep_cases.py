"""Sweep points of the DENSE and general-psi LTM steps (``dense_step``, csrc/ltm_capi.hip, over the kernels of
csrc/ltm_dense.hip and csrc/ltm_psi.hip): what ``basis_maps.build_plan`` gives most ``num_basis`` values -- every N that is no
multiple of 16 (padded), every multiple whose fp32 boxes overlap where the step looks -- and the Gaussian family.

A data module like ``sweep_cases.py``, whose sparse plans it complements: no fixtures are stored.  The inputs come from
``infinite_video_amd.synth`` and ``sweep_cases.uniforms``' seeding rule exactly as ``sweep_cases.point_inputs`` makes them; the
expected values come from the reference-shaped ``oracle.ltm_oracle.DenseOracle`` at test time (``oracle_chain``: computed once per
point and shared).  ``tests/test_dense_sweep_cpu.py`` checks the table itself (families, padding, operators and psi tables against
the oracle's, every tile edge really crossed, a float64 re-evaluation of the oracle, the mistakes each point can see);
``tests/test_dense_sweep_gpu.py`` drives every point through the library.

The shapes are the smallest that still cross the edge a point names (``edge``), never the workload's: the base is N 48, H 2, Q 8,
d 64, P 2, S 64, L 1, T 8 (a two-box plan), the Gaussian base N 32 with sigmas (0.05, 0.1).  The tile edges and masks of the eight
kernels are written down ONCE here, as predicates over a point (``EDGES``), next to the C expression they mirror.

Families (``family_of``):
  * ``box2``   dense operators, two-box tables for the histogram edges and the resampling points, closed-form read-out
               (dense_update_kernel, dense_masses_kernel, attend_small_kernel / attend_kernel);
  * ``psi01``  the rectangular psi itself as dense 0/1 rows, because a point of the 1000-point read-out grid lies in two boxes
               (psi_gemm / psi_update / psi_masses / psi_grid / psi_ctx kernels);
  * ``gauss``  the reference's Gaussian family through the same general-psi kernels.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from infinite_video_amd import basis_maps
from tests.golden import sweep_cases as sc

CHUNKS = 3                      # chunks of a chain (the ragged chains and T3_S64 name their own four)


@dataclass(frozen=True)
class DensePoint:
    name: str
    edge: str                      # the tile edge or mask this point is there to cross
    family: str                    # "box2" | "psi01" | "gauss"
    N: int = 48
    H: int = 2
    d: int = 64
    P: int = 2
    S: int = 64
    Q: int = 8                     # max_q == Q at every point
    L: int = 1
    tau: float = 0.75
    sticky: bool = True
    chunk_T: Tuple[int, ...] = (8, 8, 8)
    dtype: str = "float32"         # token dtype: float32 | bfloat16 | float16
    sigmas: Optional[Tuple[float, ...]] = None     # the Gaussian family's widths (gauss points only)

    @property
    def dh(self) -> int: return 64
    @property
    def dm(self) -> int: return 64 * self.H
    @property
    def Ts(self) -> Tuple[int, ...]: return tuple(self.chunk_T)
    @property
    def chunks(self) -> int: return len(self.chunk_T)
    @property
    def T(self) -> int: return max(self.chunk_T)
    @property
    def N_pad(self) -> int: return basis_maps.padded_N(self.N)
    @property
    def rows(self) -> int: return self.L * self.H * self.Q            # rows of the general-psi GEMMs and of psi_grid_kernel
    @property
    def draws(self) -> int: return (self.chunks - 1) * self.L * self.S if self.sticky else 0


BASE = DensePoint("box2_base", "base point (two-box plan, no tail anywhere but Q % 4 == 0 rows)", "box2")
GAUSS = replace(BASE, name="gauss_base", edge="Gaussian base point", family="gauss", N=32, sigmas=(0.05, 0.1))
PSI01_ABOVE_256 = 259           # the smallest psi01 num_basis in 257..511 (432 aside); test_dense_sweep_cpu.py finds it by search


def plan_of(pt: DensePoint, T: int) -> basis_maps.Plan:
    if pt.sigmas:
        return basis_maps.build_gaussian_plan(T, pt.N, pt.tau, tuple(pt.sigmas), pt.S)
    return basis_maps.build_plan(T, pt.N, pt.tau, pt.S)


def family_of(plan: basis_maps.Plan, pt: DensePoint) -> str:
    if not plan.dense:
        return "sparse"
    if pt.sigmas:
        return "gauss"
    return "psi01" if plan.psi else "box2"


# ---------------------------------------------------------------------------------------------------------------------
# the tile edges and masks of the kernels, mirrored from the C sources: name -> (predicate(pt), C expression, families it is
# evaluated in, whether the box kernels and the psi kernels each hold a copy of it).  Both sides of every predicate must occur among
# the one-factor points of those families -- within the box2 points and within the psi points where each has its own copy.
# ---------------------------------------------------------------------------------------------------------------------
def _Ks(pt: DensePoint) -> List[int]:
    """K of the update kernels over the point's chain: T on the first chunk, S + T afterwards."""
    return [T if c == 0 else pt.S + T for c, T in enumerate(pt.Ts)]


BOX, PSI, ALL = ("box2",), ("psi01", "gauss"), ("box2", "psi01", "gauss")
EDGES: Dict[str, Tuple[Callable, str, Tuple[str, ...], bool]] = {
    "update.first_K%4": (lambda pt: pt.Ts[0] % 4 == 0, "dense_update_kernel / psi_update_kernel: r < K on the first chunk (K = T)", ALL, True),
    "update.inf_K%4": (lambda pt: all(k % 4 == 0 for k in _Ks(pt)[1:]), "dense_update_kernel / psi_update_kernel: r < K with K = S + T", ALL, True),
    "update.(d/16)%4": (lambda pt: (pt.d // 16) % 4 == 0, "dense_update_kernel / psi_update_kernel: if (c0 >= d) return", ALL, True),
    "update.N_pad/16>7": (lambda pt: pt.N_pad // 16 > 7, "launch_dense_update / launch_psi_update: grid.y = N / 16", ALL, True),
    "update.L>2": (lambda pt: pt.L > 2, "launch_dense_update / launch_psi_update: grid.z = n_layers", ALL, True),
    "masses.Q%4": (lambda pt: pt.Q % 4 == 0, "dense_masses_kernel / psi_masses_kernel: for (q = wave; q < Q; q += 4)", ALL, True),
    "masses.Q<4": (lambda pt: pt.Q < 4, "dense_masses_kernel / psi_masses_kernel: idle waves", ALL, True),
    "masses.H==1": (lambda pt: pt.H == 1, "launch_dense_masses / launch_psi_masses: grid.x = H", ALL, True),
    "gemm.(L*H*Q)%16": (lambda pt: pt.rows % 16 == 0, "psi_gemm_kernel: a_ok = m0 + i < M, the store's row mask (M = L*H*Q)", PSI, False),
    "grid.(L*H*Q)%4": (lambda pt: pt.rows % 4 == 0, "psi_grid_kernel: if (r >= n_rows) return", PSI, False),
    "ctx.dm%256": (lambda pt: pt.dm % 256 == 0, "psi_ctx_kernel: if (col >= dm) return", PSI, False),
    "ctx.dm<256": (lambda pt: pt.dm < 256, "psi_ctx_kernel: a single, partly filled block", PSI, False),
    "attend.N_pad>256": (lambda pt: pt.N_pad > 256, "launch_attend: attend_kernel, not attend_small_kernel; 17+ basis tiles of the psi GEMMs", ALL, True),
    "padded": (lambda pt: pt.N_pad != pt.N, "basis_maps.padded_N: inert basis functions behind the real ones", ("box2", "psi01"), False),
    "draw.S%256": (lambda pt: pt.S % 256 == 0, "draw kernels: passes of 256 threads over S", ALL, False),
    "draw.S>256": (lambda pt: pt.S > 256, "draw kernels: more than one pass", ALL, False),
    "sticky": (lambda pt: pt.sticky, "dense_step: bins / bins_stride, or uniform_box2 / psi_uniform with bins_stride 0", ALL, True),
}


# ---------------------------------------------------------------------------------------------------------------------
# a) one factor at a time around the base points
# ---------------------------------------------------------------------------------------------------------------------
def _b(name, edge, **kw) -> DensePoint:
    if "T" in kw:
        kw["chunk_T"] = (kw.pop("T"),) * CHUNKS
    return replace(BASE, name=name, edge=edge, **kw)


def _g(name, edge, **kw) -> DensePoint:
    if "T" in kw:
        kw["chunk_T"] = (kw.pop("T"),) * CHUNKS
    return replace(GAUSS, name=name, edge=edge, **kw)


def _p01(name, edge, **kw) -> DensePoint:
    return _b(name, edge, family="psi01", **kw)


def _one_factor() -> List[DensePoint]:
    pts = [BASE, GAUSS]
    # N, box2.  (S stays 64 where the boxes then still hold rows: with N boxes over S + T samples a box past ~S is empty, its row of B
    #  is exactly zero, and a lost second-box term would change nothing -- N 96, 320, 384 take S 128 and N 112 S 256, the smallest
    #  of 64, 128, 256 at which the oracle's chain resamples a two-box bin whose second row is non-zero)
    pts += [_b("N17", "pad 32: 15 inert rows", N=17), _b("N47", "pad 48: one inert row short of no padding", N=47),
            _b("N96", "6 basis tiles, 8 two-box bins", N=96, S=128), _b("N112", "7 basis tiles, one two-box bin", N=112, S=256),
            _b("N192", "12 basis tiles: the N/16 grid past 7", N=192), _b("N240", "15 basis tiles", N=240),
            _b("N320", "dense plan on attend_kernel (N > 256)", N=320, S=128),
            _b("N384", "dense plan on attend_kernel, 39 two-box bins", N=384, S=128),
            _b("N300", "pad 304: padded and above 256", N=300)]
    # N, psi01
    pts += [_p01("psi01_N18", "smallest psi01 num_basis (pad 32)", N=18), _p01("psi01_N37", "pad 48", N=37),
            _p01("psi01_N63", "pad 64: one inert column", N=63), _p01("psi01_N126", "pad 128", N=126),
            _p01(f"psi01_N{PSI01_ABOVE_256}", "psi01 above 256 (pad 272): 17 basis tiles, attend_kernel supplies the scores", N=PSI01_ABOVE_256)]
    # N, gauss
    pts += [_g("gauss_N16_1sigma", "one basis tile, one width", N=16, sigmas=(0.1,)),
            _g("gauss_N48_3sigma", "three widths", N=48, sigmas=(0.02, 0.05, 0.2)),
            _g("gauss_N128", "8 basis tiles", N=128, sigmas=(0.03, 0.1)),
            _g("gauss_N272", "psi read-out over 17 basis tiles (N > 256)", N=272, sigmas=(0.03, 0.1))]
    # K tails of the update kernels: T % 4 and (S + T) % 4 each take 1, 2 and 3, on dense_update_kernel and on psi_update_kernel
    for T, S in ((5, 102), (7, 100), (3, 64), (2, 64), (5, 64), (6, 64)):
        why = f"k tail: T % 4 = {T % 4}, (S + T) % 4 = {(S + T) % 4}"
        # (T 3 runs four chunks: the first chunk fills three boxes, and only the fourth resamples a two-box bin with a second row)
        pts.append(replace(_b(f"T{T}_S{S}", why + ("; S off the draw's threads" if S != 64 else ""), T=T, S=S),
                           chunk_T=(T,) * (4 if T == 3 else CHUNKS)))
        pts.append(_g(f"gauss_T{T}_S{S}", why, T=T, S=S))
    # S: the draw's passes; K = S + T up to 1324
    for S, why in ((4, "fewer samples than one wave"), (256, "one pass of the draw's 256 threads"), (512, "two passes"),
                   (1000, "S off 256 in the 4-pass draw, K = 1008"), (1024, "largest S the draw kernels hold")):
        pts.append(_b(f"S{S}", why, S=S))
    pts.append(_g("gauss_S1000", "1000 resampled rows of Y = Psi_bin . B, K = 1008", S=1000))
    pts.append(_b("T300_S1024", "K = 1324: the longest contraction of the update", T=300, S=1024))
    # T
    pts += [_b("T255", "odd T, K = 255 / 319", T=255), _b("T300", "T > S: K = 300 / 364", T=300),
            _g("gauss_T255", "odd T on the psi update", T=255),
            _b("T_ragged", "a plan per chunk length (K 8, 69, 66, 72)", chunk_T=(8, 5, 2, 8)),
            _g("gauss_T_ragged", "a plan per chunk length on the psi update", chunk_T=(8, 5, 2, 8))]
    # tau
    pts += [_b("tau05", "tau 0.5", tau=0.5), _b("tau09", "tau 0.9", tau=0.9), _g("gauss_tau05", "tau 0.5", tau=0.5)]
    # d: the update's 4 waves of 16 columns
    for d, why in ((32, "d/16 = 2: waves 2 and 3 leave"), (96, "d/16 = 6: second block half empty"), (160, "d/16 = 10"),
                   (1056, "66 column tiles"), (1408, "EVA ViT-g width")):
        pts.append(_b(f"d{d}", why, d=d))
    pts += [_g("gauss_d32", "psi update with waves 2 and 3 leaving; Y = Psi_bin . B with 2 column tiles", d=32),
            _g("gauss_d96", "psi update, second block half empty", d=96)]
    # H: the masses' grid; dm of psi_ctx_kernel
    pts += [_b("H1", "one masses workgroup per layer", H=1), _b("H12", "the workload's head count", H=12),
            _g("gauss_H1", "dm 64: a quarter block of psi_ctx_kernel", H=1), _g("gauss_H4", "dm 256: one whole block", H=4),
            _g("gauss_H5", "dm 320: ragged last block", H=5), _g("gauss_H12", "dm 768: three whole blocks", H=12),
            _g("gauss_H20", "dm 1280: five blocks", H=20)]
    # Q: 4 rows per pass of the masses kernels, idle waves; with H and L, the row count L*H*Q of the psi GEMMs (16) and psi_grid (4)
    for Q in (1, 2, 3, 5, 9, 33, 96):
        pts.append(_b(f"Q{Q}", f"masses: Q = {Q} ({'idle waves' if Q < 4 else f'Q % 4 = {Q % 4}'})", Q=Q))
    pts += [_g("gauss_H1_Q1", "L*H*Q = 1: one row of the psi GEMMs, three idle psi_grid waves", H=1, Q=1),
            _g("gauss_H1_Q3", "L*H*Q = 3", H=1, Q=3), _g("gauss_H3_Q5", "L*H*Q = 15: one short of a row tile", H=3, Q=5),
            _g("gauss_H1_Q17", "L*H*Q = 17: one past a row tile", H=1, Q=17),
            _g("gauss_L3_H1_Q33", "L*H*Q = 99 with the 129- and 1000-column tails", L=3, H=1, Q=33),
            _g("gauss_H2_Q96", "L*H*Q = 192: 12 whole row tiles", Q=96),
            _p01("psi01_N37_H1_Q9", "L*H*Q = 9 with padded psi rows", N=37, H=1, Q=9)]
    # L
    pts += [_b("L3", "the L grid past 2", L=3), _b("L8", "INFV_LTM_MAX_LAYERS", L=8), _g("gauss_L8", "8 layers on the psi kernels", L=8)]
    # non-sticky: bins_stride 0, uniform_box2 / psi_uniform
    pts += [_b("uniform_box2", "non-sticky: uniform_box2 with bins_stride 0", sticky=False),
            _p01("uniform_psi01_N37", "non-sticky: psi_uniform 0/1 rows, Y of S positions", N=37, sticky=False),
            _g("uniform_gauss", "non-sticky: psi_uniform, Y of S positions", sticky=False)]
    # half-precision tokens
    pts += [_b("bf16_tokens", "bf16 frame tokens into the dense step", dtype="bfloat16"),
            _g("fp16_tokens_gauss", "fp16 frame tokens into the psi step", dtype="float16")]
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# b) a fixed-seed random sample of combinations of the values above, restricted to plans that come out dense
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_POINTS = 12
RANDOM_SEED = 20261020
_VALUES = dict(
    N=(17, 47, 48, 96, 112, 192, 240, 300, 320, 384, 18, 37, 63, 126, PSI01_ABOVE_256, 64, 256), S=(4, 64, 100, 102, 256, 512, 1000, 1024),
    T=(2, 3, 5, 6, 7, 8, 255, 300), tau=(0.5, 0.75, 0.9), d=(32, 64, 96, 160, 1056, 1408), H=(1, 2, 5, 12, 20), Q=(1, 2, 3, 5, 8, 9, 33, 96),
    L=(1, 3, 8), P=(1, 2, 7), sticky=(True, True, True, False), dtype=("float32", "float32", "bfloat16", "float16"),
    gauss=(None, None, None, (16, (0.1,)), (48, (0.02, 0.05, 0.2)), (128, (0.03, 0.1)), (272, (0.03, 0.1))))
ORACLE_ELEMS = 24_000_000       # the reference-shaped oracle materialises [H, Q, N, 1000] per layer and step: keep a point's cheap


def device_bytes(pt: DensePoint) -> int:
    """``sweep_cases.device_bytes`` at the point's shape (a per-chunk engine: sub-batches of one chunk)."""
    return sc.device_bytes(sc.SweepPoint(pt.name, "", "", N=pt.N_pad, H=pt.H, d=pt.d, P=pt.P, S=pt.S, chunk_T=pt.Ts, Q=pt.Q, L=pt.L,
                                         tau=pt.tau, sticky=pt.sticky, dtype="float32" if pt.dtype == "float32" else "bfloat16",
                                         max_batch_chunks=1))


def _random_sample() -> List[DensePoint]:
    rng = np.random.default_rng(RANDOM_SEED)
    keys = list(_VALUES)
    pts: List[DensePoint] = []
    while len(pts) < RANDOM_POINTS:
        kw = {k: _VALUES[k][int(rng.integers(len(_VALUES[k])))] for k in keys}
        kw = {k: (v.item() if hasattr(v, "item") else v) for k, v in kw.items()}
        gauss = kw.pop("gauss")
        if gauss is not None:
            kw["N"], kw["sigmas"] = gauss
        kw["chunk_T"] = (kw.pop("T"),) * CHUNKS
        pt = DensePoint(f"rand{len(pts):02d}", "random combination", "", **kw)
        if pt.L * pt.H * pt.Q * pt.N * 1000 > ORACLE_ELEMS or device_bytes(pt) > 2 << 30:
            continue
        try:
            fam = family_of(plan_of(pt, pt.T), pt)
        except (basis_maps.UnsupportedBasis, ValueError):
            continue
        if fam == "sparse":
            continue                                          # (sparse plans: sweep_cases.py)
        pts.append(replace(pt, family=fam, edge=f"random combination: {fam}"))
    return pts


@dataclass(frozen=True)
class Refusal:
    name: str
    N: int
    sigmas: Tuple[float, ...]


REFUSALS = [Refusal("gauss_N40", 40, (0.05, 0.1))]            # a Gaussian num_basis that is no multiple of 16

ONE_FACTOR = _one_factor()
RANDOM = _random_sample()
POINTS: List[DensePoint] = ONE_FACTOR + RANDOM
assert len({p.name for p in POINTS}) == len(POINTS), "dense sweep point names must be unique"
BY_NAME = {p.name: p for p in POINTS}
OWN_PLAN_POINT = "gauss_N48_3sigma"       # also run with the product's own operators (the host's LAPACK), under looser bounds


# ---------------------------------------------------------------------------------------------------------------------
# inputs and expected values of a point (nothing is stored)
# ---------------------------------------------------------------------------------------------------------------------
def point_inputs(pt: DensePoint):
    """(ks, qs, ws, u) exactly as ``sweep_cases.point_inputs`` makes them; half-precision points hold values exact in their
    dtype, as fp32."""
    import torch
    from infinite_video_amd import synth
    ks = [synth.frame_tokens(c, T, pt.P, pt.d) for c, T in enumerate(pt.Ts)]
    if pt.dtype != "float32":
        dt = {"bfloat16": torch.bfloat16, "float16": torch.float16}[pt.dtype]
        ks = [torch.from_numpy(k).to(dt).float().numpy() for k in ks]
    qs = np.stack([synth.layer_query(l, pt.Q, pt.dm) for l in range(pt.L)])
    ws = [synth.layer_projections(l, pt.d, pt.dm) for l in range(pt.L)]
    return ks, qs, ws, sc.uniforms(pt)


def linear(d: int, dm: int, w: np.ndarray, b: np.ndarray, dtype=None):
    import torch
    m = torch.nn.Linear(d, dm)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(np.ascontiguousarray(w)))
        m.bias.copy_(torch.from_numpy(np.ascontiguousarray(b)))
    return m.to(dtype) if dtype is not None else m


@dataclass
class Chain:
    """The free-running DenseOracle chain of a point, every layer an oracle of its own."""
    ctx: np.ndarray            # [chunks, L, Q, dm]
    B: np.ndarray              # [chunks, L, N, d]
    scores: np.ndarray         # [chunks, L, H, Q, N]
    bins: np.ndarray           # [chunks, L, S] int64, -1 where no draw was made
    probs: np.ndarray          # [chunks, L, 127]
    G: Dict[int, Tuple[np.ndarray, np.ndarray]]     # T -> (G_first [T, N], G_inf [S + T, N]) of DenseOracle._build


def shared_build(base):
    """``base`` (a DenseOracle class) whose per-forward ``_build`` is computed once per chunk length and shared through ``cache``:
    the same tensors, the same arithmetic (tests/test_config_sweep_cpu.py does the same)."""
    class Shared(base):
        cache = None

        def _build(self, L):
            if L not in self.cache:
                super()._build(L)
                self.cache[L] = (self.G_first, self.G_inf, self.uniform_samples, self.bins)
            self.G_first, self.G_inf, self.uniform_samples, self.bins = self.cache[L]
    return Shared


@lru_cache(maxsize=None)
def oracle_chain(name: str) -> Chain:
    import torch
    from oracle import ltm_oracle as O
    pt = BY_NAME[name]
    ks, qs, ws, _ = point_inputs(pt)
    n = pt.chunks
    out = Chain(np.empty((n, pt.L, pt.Q, pt.dm), np.float32), np.empty((n, pt.L, pt.N, pt.d), np.float32),
                np.empty((n, pt.L, pt.H, pt.Q, pt.N), np.float32), np.full((n, pt.L, pt.S), -1, np.int64),
                np.zeros((n, pt.L, 127), np.float32), {})
    cache = {}
    cls = shared_build(O.DenseOracle)
    with torch.no_grad():
        for l in range(pt.L):
            wk, bk, wv, bv = ws[l]
            o = cls(pt.N, pt.H, pt.dh, pt.tau, pt.sticky, linear(pt.d, pt.dm, wk, bk), linear(pt.d, pt.dm, wv, bv), pool_shape=(pt.P,),
                    nb_samples=pt.S, gaussian_sigmas=pt.sigmas)
            o.cache = cache
            for c in range(n):
                torch.manual_seed(sc.call_seed(pt, c, l))          # the draw then consumes sweep_cases.uniforms(pt)[c, l]
                y = o.forward(torch.from_numpy(ks[c]).unsqueeze(0), torch.from_numpy(qs[l]).unsqueeze(0), new_doc=(c == 0))
                out.ctx[c, l], out.B[c, l], out.scores[c, l] = y[0].numpy(), o.B_past[0].numpy(), o.scores().numpy()
                if c and pt.sticky:
                    out.bins[c, l], out.probs[c, l] = o.last_bins.numpy(), o.last_probs.numpy()
    out.G = {T: (g[0].numpy(), g[1].numpy()) for T, g in cache.items()}
    return out
