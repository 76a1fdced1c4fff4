"""Sweep points of the configuration range the C ABI accepts (include/infv_ltm.h, include/infv_vqf.h).

A data module like ``cases.py`` -- but it holds no fixtures: every input is regenerated from
``infinite_video_amd.synth`` and the expected values come from ``oracle.ltm_oracle.ClosedFormOracle`` /
``oracle.qformer_oracle`` at test time.  ``tests/test_config_sweep_cpu.py`` checks the table itself (the two oracles
agree at every point, the host plans match the oracle's maps, every gate is crossed in both directions);
``tests/test_config_sweep_gpu.py`` drives every point through the library.  Every point here has a SPARSE plan; the dense and
general-psi plans (most ``num_basis`` values: every N off 16, most multiples of 16, the Gaussian family) are swept in
``dense_sweep_cases.py`` / ``tests/test_dense_sweep_cpu.py`` / ``tests/test_dense_sweep_gpu.py``.

The library picks its kernels from the shape through a cascade of host-side gates.  They are written down ONCE here, as
plain Python predicates over a point and its host plan (``GATES``), next to the C expression they mirror.  Every point
names the gate it is there to cross (``gate``) and the kernel families it is expected to run (``families``: the
``infv_kernel`` ids ``LTMEngine.profile_read()`` reports).  ``expected_families`` derives the families from the
predicates; the CPU test asserts that derivation equals what each hand-written point names, the GPU test asserts that the
library reports them -- a point that drifts onto another path is a failure, not a quietly lost case.

Families cannot tell every pair of kernels apart; where they cannot, the path string of ``expected_path`` says which kernel
the gates select:
  * ``chain_kernel`` (one launch per chunk), ``chain_batch_kernel`` and ``chain_batch3_kernel`` (persistent) all count as
    CHAIN.  Which persistent form runs is decided by ``chain_batch3_shape_ok``; whether the persistent form runs at all also
    needs ``chain_batch_resident`` -- an occupancy query of the device, which no host-side predicate can mirror;
  * ``uc_kernel`` and ``uc_fast_kernel`` both count as UC (``uc_fast_supported`` decides);
  * ``attend_small_kernel`` (N <= 256) and ``attend_kernel`` (N > 256) both count as ATTEND;
  * the per-chunk step draws inside its projection launch (``step_project_kernel``), so a per-chunk chain reports PROJECT,
    UPDATE and ATTEND and no separate DRAW; the lockstep multi-video step reports DRAW.
``dh`` stays 64: the ABI refuses anything else.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from infinite_video_amd import basis_maps

STAGES = ("project", "update", "attend")          # per-chunk stage kernels (infv_ltm_forward's step)
FAST = ("scores", "chain", "uc")                  # whole-call fast path (SCORES: only when a call continues a memory)
MAX_NB_SAMPLES = 1024                             # infv_ltm_create refuses more (the draw kernels hold S slots in LDS)


@dataclass(frozen=True)
class SweepPoint:
    name: str
    gate: str                      # the gate (or tile edge) this point is there to cross
    families: str                  # "stages" | "fast": what infv_ltm_consolidate is expected to run
    N: int = 64
    H: int = 12
    d: int = 768
    P: int = 32
    S: int = 512
    T: int = 8
    chunk_T: Optional[Tuple[int, ...]] = None     # ragged chain: frames of every chunk (overrides T / n_chunks)
    Q: int = 32                    # max_q == Q at every point
    L: int = 2
    tau: float = 0.75
    sticky: bool = True
    dtype: str = "float32"         # token dtype: float32 | bfloat16
    max_batch_chunks: int = 32
    n_chunks: int = 4              # chunks of the consolidate call (chunk 0 starts the document)
    v_split: bool = False          # INFV_VPROJ_SPLIT=1 at create: V' half of a >= 1024-row projection as a split-bf16 contraction

    @property
    def dh(self) -> int: return 64
    @property
    def dm(self) -> int: return 64 * self.H
    @property
    def Ts(self) -> Tuple[int, ...]:
        return tuple(self.chunk_T) if self.chunk_T else (self.T,) * self.n_chunks
    @property
    def chunks(self) -> int: return len(self.Ts)
    @property
    def draws(self) -> int: return (self.chunks - 1) * self.L * self.S if self.sticky else 0


SMALL = SweepPoint("small_base", "base point (tabw 12: uc_kernel, chain_batch3)", "fast")
HEAD = dict(N=256, T=256)          # headline base: only where a gate depends on N, T or the row count M


# ---------------------------------------------------------------------------------------------------------------------
# the gates, mirrored from the C sources
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PlanShape:
    dense: bool
    rows_first: int
    rows_inf: int
    tabw: int
    points_ok: bool
    @property
    def rows_max(self) -> int: return max(self.rows_first, self.rows_inf)


def plan_shape(N: int, T: int, tau: float, S: int) -> PlanShape:
    """What infv_ltm_set_plan derives from the host plan (ltm_capi.hip: upload_operator's tabw, set_plan's points_ok)."""
    p = basis_maps.build_plan(T, N, tau, S)
    if p.dense:
        return PlanShape(True, 0, 0, 4, False)
    mx = int(np.diff(p.inf_old_ptr).max(initial=0))
    tabw = 4 if mx < 4 else (mx + 3) & ~3
    nb = len(p.bin_box)
    ok = p.edge_box[0] == -1 and p.edge_box[nb] == -1 and bool((p.bin_box >= 0).all()) and \
        bool((p.edge_box[1:nb] == p.bin_box[1:]).all())
    return PlanShape(False, len(p.first_row_box), len(p.inf_row_box), tabw, bool(ok))


def _take(sizes) -> int:
    return sum((n + 3) & ~3 for n in sizes)


def chain_lds_bytes(N, S, rows, tabw) -> int:       # ltm_chain.hip: chain_smem
    return 4 * _take([128, S, 1024, 64, N * tabw, N, N, N, 128, 132, 128, 8 * (N + 4), 8 * (N + 2), 8 * (rows + 1), 8 * 132, 8 * 128])


def chain_batch_lds_bytes(N, S, rows, tabw) -> int:  # ltm_chain_batch.hip: batch_smem
    return 4 * _take([128, S, 1024, 64, N * tabw, N * tabw, N, N, N, 128, 132, 128, 8 * (N + 4), 8 * (N + 4), 8 * (N + 2),
                      8 * (rows + 1), 8 * 132, 8 * 128])


def uc_lds_bytes(N, tabw, rows) -> int:             # ltm_uc.hip: uc_smem
    return 4 * _take([N * 33, N * 33, N * tabw, N, N, rows * 32, 32 * (N + 2), 32, 8 * 64 * 4])


def chain_supported(pt, ps) -> bool:                # ltm_chain.hip
    return (pt.N <= 256 and pt.N % 16 == 0 and pt.S <= 512 and ps.rows_max <= 256 and ps.tabw <= 16 and ps.tabw % 4 == 0 and
            pt.N * ps.tabw <= 4096 and chain_lds_bytes(pt.N, pt.S, ps.rows_max, ps.tabw) <= 160 * 1024)


def uc_supported(pt, ps) -> bool:                   # ltm_uc.hip
    return (pt.N <= 256 and pt.N % 16 == 0 and pt.N * ps.tabw <= 2048 and ps.rows_max * 32 <= 8192 and pt.d % 32 == 0 and
            pt.dm % 64 == 0 and ps.tabw % 4 == 0 and uc_lds_bytes(pt.N, ps.tabw, ps.rows_max) <= 160 * 1024)


def fast_path(pt, ps) -> bool:                      # ltm_consolidate.hip, consolidate_impl: the gate in front of the fused chain
    return (not ps.dense and chain_supported(pt, ps) and (pt.L * pt.H * pt.Q) % 128 == 0 and (pt.L * pt.dm) % 128 == 0 and
            uc_supported(pt, ps) and pt.Q <= 256)         # (Q <= 256: qtilde_supported, the fused chain's pre-multiplied queries)


def chain_s_tiles(Q) -> int: return (Q + 7) // 8


def chain_batch_supported(pt, ps) -> bool:          # ltm_chain_batch.hip (n_blocks = H * chain_s_tiles(Q) * L)
    return (pt.N <= 256 and pt.N % 16 == 0 and pt.S <= 512 and ps.rows_inf <= 256 and ps.tabw <= 16 and ps.tabw % 4 == 0 and
            pt.H * chain_s_tiles(pt.Q) * pt.L <= 384 and chain_batch_lds_bytes(pt.N, pt.S, ps.rows_inf, ps.tabw) <= 100 * 1024)


def chain_batch3_shape_ok(pt, ps) -> bool:          # ltm_chain_batch.hip (draw_mode 1 = sticky; rpw 2 needs 4 * rows <= 256, Q > 8)
    return (pt.sticky and ps.points_ok and 2 * ps.rows_inf <= 256 and pt.S <= 512 and pt.S % 4 == 0 and pt.Q % 4 == 0 and
            4 * ps.rows_inf <= 256 and pt.Q > 8)


def uc_fast_supported(pt, ps) -> bool:              # ltm_uc.hip
    return ps.tabw == 4 and pt.Q <= 32 and pt.N % 64 == 0 and pt.N <= 256


def videos_supported(pt, ps) -> bool:               # ltm_kernels.hip + videos_impl: the lockstep kernels take the shape
    return (not ps.dense and 0 < pt.N <= 256 and pt.N % 16 == 0 and 0 < pt.S <= 1024 and pt.d % 32 == 0 and
            (pt.L * 2 * pt.dm) % 64 == 0 and 1 <= pt.L <= 8)


def pool_rows2_supported(pt, ps=None) -> bool:      # ltm_kernels.hip
    return pt.d % 4 == 0 and ((pt.d // 4 + 63) // 64) * 4 * 64 <= 1024


def _ps(pt) -> PlanShape:
    """Plan shape of the point's call (ragged chains: every chunk length has its own plan; the gates read the call's)."""
    return plan_shape(pt.N, max(pt.Ts), pt.tau, pt.S)


def _sub_rows(pt, ps) -> int:
    """Rows M of the largest projection GEMM of the point's consolidate call (sub-batches of min(max_batch_chunks, 32)
    chunks behind the document's first chunk; calls below 768 chunks)."""
    sub = min(pt.max_batch_chunks if pt.max_batch_chunks > 0 else 32, 32)
    return min(sub, pt.chunks - 1) * ps.rows_inf


def _always(pt, ps) -> bool: return not ps.dense
def _on_fast(pt, ps) -> bool: return fast_path(pt, ps)
def _on_batch(pt, ps) -> bool: return fast_path(pt, ps) and chain_batch_supported(pt, ps)
def _on_vsplit(pt, ps) -> bool: return fast_path(pt, ps) and pt.v_split and _sub_rows(pt, ps) >= 1024


# name -> (predicate(pt, ps), C expression, None or the reason only one side can occur among shapes the ABI accepts,
#          where(pt, ps): the library evaluates the gate at this point -- a side counts as crossed only there)
GATES: Dict[str, Tuple[Callable, str, Optional[str], Callable]] = {
    "chain.S<=512": (lambda pt, ps: pt.S <= 512, "chain_supported: S <= kNT", None, _always),
    "chain.N*tabw<=4096": (lambda pt, ps: pt.N * ps.tabw <= 4096, "chain_supported: N * tabw <= 8 * kNT",
                           "sparse plans have N * tabw <= ~2 S (S slots spread over the boxes below tau): 4096 needs S > 1024", _always),
    "chain.tabw<=16": (lambda pt, ps: ps.tabw <= 16, "chain_supported: tabw <= kMaxTabw", None, _always),
    "chain.lds": (lambda pt, ps: chain_lds_bytes(pt.N, pt.S, ps.rows_max, ps.tabw) <= 160 * 1024, "chain_lds_bytes <= 160 KiB",
                  "implied by N <= 256, S <= 512, tabw <= 16, rows <= 256 (61 KB at that corner)", _always),
    "fast.(L*H*Q)%128": (lambda pt, ps: (pt.L * pt.H * pt.Q) % 128 == 0, "consolidate_impl: (L*H*Q) % 128", None, _always),
    "fast.(L*dm)%128": (lambda pt, ps: (pt.L * pt.dm) % 128 == 0, "consolidate_impl: (L*dm) % 128", None, _always),
    "fast.Q<=256": (lambda pt, ps: pt.Q <= 256, "consolidate_impl: qtilde_supported(Q)", None, _always),
    "fast.uc_supported": (lambda pt, ps: uc_supported(pt, ps), "consolidate_impl: uc_supported",
                          "implied by chain_supported for sparse plans with S <= 512 (N * tabw <= 2048, 160 KB at N 256, tabw 16, rows 256)",
                          lambda pt, ps: not ps.dense and chain_supported(pt, ps)),
    "batch.tabw<=16": (lambda pt, ps: ps.tabw <= 16, "chain_batch_supported: tabw <= 16",
                       "chain_supported, in front of it, has the same term", _on_fast),
    "batch.wgs<=384": (lambda pt, ps: pt.H * chain_s_tiles(pt.Q) * pt.L <= 384, "chain_batch_supported: n_blocks <= 384", None, _on_fast),
    "batch3.sticky": (lambda pt, ps: pt.sticky, "chain_batch3_shape_ok: draw_mode == 1", None, _on_batch),
    "batch3.points_ok": (lambda pt, ps: ps.points_ok, "chain_batch3_shape_ok: the histogram edges are the bins' left edges", None, _on_batch),
    "batch3.rows<=64": (lambda pt, ps: 4 * ps.rows_inf <= 256, "chain_batch3_rpw: 4 * rows <= 64 * kB2Ld", None, _on_batch),
    "batch3.S%4": (lambda pt, ps: pt.S % 4 == 0, "chain_batch3_shape_ok: S % 4", None, _on_batch),
    "batch3.Q%4": (lambda pt, ps: pt.Q % 4 == 0, "chain_batch3_shape_ok: Q % 4", None, _on_batch),
    "batch3.Q>8": (lambda pt, ps: pt.Q > 8, "chain_batch3_rpw: Q > kBRows", None, _on_batch),
    "uc_fast.tabw==4": (lambda pt, ps: ps.tabw == 4, "uc_fast_supported: tabw == 4", None, _on_fast),
    "uc_fast.Q<=32": (lambda pt, ps: pt.Q <= 32, "uc_fast_supported: Q <= kUcQ", None, lambda pt, ps: fast_path(pt, ps) and ps.tabw == 4),
    "uc_fast.N%64": (lambda pt, ps: pt.N % 64 == 0, "uc_fast_supported: N % 64", None, lambda pt, ps: fast_path(pt, ps) and ps.tabw == 4),
    "videos.S<=1024": (lambda pt, ps: pt.S <= 1024, "videos_supported: S <= 1024", "infv_ltm_create refuses nb_samples > 1024", _always),
    "videos.N<=256": (lambda pt, ps: pt.N <= 256, "videos_supported: N <= 256", None, _always),
    "videos.(2*L*dm)%64": (lambda pt, ps: (2 * pt.L * pt.dm) % 64 == 0, "videos_supported: (L*2*dm) % 64",
                           "dm = 64 H is a multiple of 64", _always),
    "pool_rows2.d<=1024": (lambda pt, ps: pool_rows2_supported(pt), "pool_rows2_supported: ceil(d/256) * 256 <= 1024", None,
                           lambda pt, ps: fast_path(pt, ps) and pt.chunks > 1),
    "gemm.M>=1024": (lambda pt, ps: _sub_rows(pt, ps) >= 1024, "project_chunks_fast / launch_gemm: M >= 1024", None, _on_fast),
    "gemm.d%64": (lambda pt, ps: pt.d % 64 == 0, "split-bf16 V' projection (INFV_VPROJ_SPLIT): d % 64", None, _on_vsplit),
    "gemm.v_cols%128": (lambda pt, ps: (pt.L * pt.dm) % 128 == 0, "split-bf16 V' projection: v_cols % 128",
                        "the fused chain's own gate (L*dm) % 128 stands in front of it", _on_vsplit),
    # "n_chunks >= 768" (the call-long pooling launch, 42-chunk sub-batches) stays with tests/test_timed_path_gpu.py: too long for a sweep
}


def expected_families(pt: SweepPoint) -> str:
    return "fast" if fast_path(pt, _ps(pt)) else "stages"


def expected_path(pt: SweepPoint) -> str:
    """The kernels the gates select, finer than the families (recorded in profiles/config_sweep_parity.txt)."""
    ps = _ps(pt)
    if ps.dense:
        return "dense"
    if not fast_path(pt, ps):
        return "stages:attend_small" if pt.N <= 256 else "stages:attend_kernel"
    role_s = "chain_kernel"
    if chain_batch_supported(pt, ps):       # (+ chain_batch_resident on the device)
        role_s = "chain_batch3" if chain_batch3_shape_ok(pt, ps) else "chain_batch"
    uc = "uc_fast" if uc_fast_supported(pt, ps) else "uc"
    gemm = "gemm_x6" if _sub_rows(pt, ps) >= 1024 else "gemm_splitk"
    return f"fast:{role_s}+{uc}+{gemm}" + ("+vsplit" if pt.v_split else "")


# ---------------------------------------------------------------------------------------------------------------------
# a) one factor at a time around the two base points
# ---------------------------------------------------------------------------------------------------------------------
def _p(name, gate, families, **kw) -> SweepPoint:
    return replace(SMALL, name=name, gate=gate, families=families, **kw)


def _one_factor() -> List[SweepPoint]:
    pts = [SMALL, _p("head_base", "uc_fast_supported (tabw 4, N % 64) on the headline base", "fast", **HEAD)]
    # S: draw strides (256 threads), S % 4 (chain_batch3), chain_supported S <= 512, kMaxTabw (S 1000: tabw 24), create's bound
    for S, why, fam in ((4, "fewer samples than one wave", "fast"), (64, "one wave of samples", "fast"),
                        (100, "S off the draw's 256 threads, S % 4 == 0", "fast"), (102, "S % 4 != 0: chain_batch_kernel", "fast"),
                        (256, "one pass of the draw's 256 threads (tabw 8)", "fast"), (508, "last S % 4 == 0 below 512", "fast"),
                        (516, "first S past chain_supported", "stages"), (1000, "S off 256 in the 4-pass draw, tabw 24 > kMaxTabw", "stages"),
                        (1024, "largest S the draw kernels hold", "stages")):
        pts.append(_p(f"S{S}", why, fam, S=S))
    # H
    pts += [_p("H1_L1", "(L*dm) % 128 != 0", "stages", H=1, L=1),
            _p("H1_L2", "L*H*Q = 64 off 128 with (L*dm) % 128 == 0", "stages", H=1),
            _p("H2", "L*H*Q = 128: smallest fast-path head count", "fast", H=2),
            _p("H3", "L*H*Q = 192 off 128", "stages", H=3),
            _p("H5", "L*H*Q = 320 off 128, dm 320", "stages", H=5),
            _p("H8", "dm 512", "fast", H=8), _p("H16", "dm 1024", "fast", H=16),
            _p("H20", "dm 1280: 640 update threads, 5 GEMM column tiles per half", "fast", H=20)]
    # d
    for d, why in ((32, "d/4 = 8 lanes: one k-tile, no split-K"), (96, "d % 64 != 0, d/4 = 24 below 64 lanes"),
                   (160, "d % 64 != 0, d/4 = 40 off 64 lanes"), (1024, "last width pool_rows2 takes"),
                   (1056, "first width past pool_rows2_supported"), (1408, "EVA ViT-g width"), (2048, "two passes of 1024 update threads")):
        pts.append(_p(f"d{d}", why, "fast", d=d))
    # P
    for P, why in ((1, "no pooling sum"), (2, "below the pooling unroll"), (7, "odd, below the unroll of 8 / 16"),
                   (49, "3 unrolled trips + 1 tail"), (196, "VideoChat2 tokens per frame"), (257, "CLS + 256 patches: tail of 1")):
        pts.append(_p(f"P{P}", why, "fast", P=P))
    # Q (max_q == Q): tile edges of attend_small (4), role S (8), alpha_rows2 / uc (32), attend (16)
    for Q in (1, 4, 5, 8, 9, 12, 31, 33, 36, 64, 96, 97, 128, 256):
        fam = "fast" if (2 * 12 * Q) % 128 == 0 else "stages"
        why = {64: "two uc passes of 32 rows", 96: "three uc passes", 128: "192 role-S workgroups",
               256: "768 role-S tiles of 8 rows > 384: no persistent role S"}.get(Q, f"tile edge Q={Q} of the per-chunk attend (4-row tiles)")
        pts.append(_p(f"Q{Q}", why, fam, Q=Q))
    # ... and the same edges on the fast path, where H = 16 puts every Q % 4 == 0 on it (role S 8 / 16 rows, uc 32 rows)
    for Q, why in ((4, "Q <= 8: chain_batch_kernel, half a role-S tile"), (8, "Q == kBRows: chain_batch_kernel"),
                   (12, "first Q on chain_batch3 (Q > 8), ragged 16-row tile"), (36, "Q > 32: uc_kernel second pass of 4 rows"),
                   (100, "ragged 16-row role-S tile and ragged uc pass")):
        pts.append(_p(f"H16_Q{Q}", why, "fast", H=16, Q=Q))
    # ... past 256 rows: the fused chain's pre-multiplied queries (qtilde_kernel: one thread per row of 256, 64 KB of LDS) stop there
    pts += [_p("Q257_L1", "first Q past qtilde_supported, off 128", "stages", Q=257, L=1),
            _p("Q384_L1", "L*H*Q = 4608 on 128 but Q > 256: per-chunk stages", "stages", Q=384, L=1),
            _p("H16_Q264_L1", "L*H*Q = 4224 on 128 but Q > 256: per-chunk stages", "stages", H=16, Q=264, L=1),
            _p("head_Q64", "uc_fast refused by Q > 32 alone (tabw 4, N % 64 == 0)", "fast", Q=64, n_chunks=3, **HEAD)]
    pts.append(_p("H16_Q5", "Q % 4 != 0 with H 16", "stages", H=16, Q=5))
    pts.append(_p("H16_Q6", "fast path with Q % 4 != 0 (L 4: L*H*Q = 384): chain_batch_kernel", "fast", H=16, Q=6, L=4))
    # L
    pts += [_p("L1", "one layer (L*H*Q = 384)", "fast", L=1), _p("L3", "L*H*Q = 1152", "fast", L=3),
            _p("L5", "L*H*Q = 1920", "fast", L=5), _p("L8", "INFV_LTM_MAX_LAYERS", "fast", L=8),
            _p("vc2_wgs", "VideoChat2 H 12, Q 96, L 6: 432 role-S workgroups > 384", "fast", Q=96, L=6)]
    # N at S 512 (48, 96, 192, ... plan dense: dense_sweep_cases.py)
    pts += [_p("N16", "44 slots per box > kMaxTabw, N % 64 != 0", "stages", N=16),
            _p("N32", "24 slots per box > kMaxTabw", "stages", N=32),
            _p("N128", "tabw 8", "fast", N=128),
            _p("N256", "tabw 4 with 7 new rows: uc_fast", "fast", N=256),
            _p("N272", "N > 256: attend_kernel (16-row tiles), lockstep entries fall back", "stages", N=272),
            _p("N272_Q33", "attend_kernel with a ragged third 16-row tile", "stages", N=272, Q=33),
            _p("N512", "largest num_basis the sweep runs (attend_kernel: 91 KB of LDS)", "stages", N=512),
            _p("N80", "sparse plan whose histogram edges are not the bins' left edges (points_ok false): chain_batch_kernel", "fast", N=80),
            _p("N144_S256", "uc_fast refused by N % 64 alone (tabw 4)", "fast", N=144, S=256)]
    # T with N 64
    for T, why in ((2, "one new row"), (3, "two new rows"), (255, "odd T, 16 new rows"), (256, "16 new rows"),
                   (300, "T > S/2: frame ranges of 18-19 frames")):
        pts.append(_p(f"T{T}", why, "fast", T=T))
    pts.append(_p("T_ragged", "a plan per chunk length, one call per chunk", "fast", chunk_T=(8, 5, 2, 8, 7)))
    # tau
    pts += [_p("tau05", "tabw 16 == kMaxTabw", "fast", tau=0.5), _p("tau09", "6 new rows, tabw 12", "fast", tau=0.9),
            _p("head_tau05", "128 new rows per chunk: 4 * rows > 256, no 16-row role-S tiles", "fast", tau=0.5, **HEAD),
            _p("head_tau09", "26 new rows per chunk", "fast", tau=0.9, **HEAD)]
    # sticky = False where the paths differ
    pts += [_p("uniform_small", "non-sticky fast path (draw_mode 2: chain_batch_kernel)", "fast", sticky=False),
            _p("uniform_H3", "non-sticky per-chunk stages", "stages", sticky=False, H=3),
            # (non-sticky S = 1000 is not a one-factor point: it sums 24 resampled rows per box and the two CPU oracles then differ by
            #  1.3e-7 in B -- 24-term fp32 sums in another order at |B| up to 0.49 -- which is over the 1e-7 their agreement check
            #  holds; on the GPU the combination runs in the random part)
            _p("uniform_S516", "non-sticky, first S past chain_supported", "stages", sticky=False, S=516),
            _p("uniform_head", "non-sticky uc_fast", "fast", sticky=False, n_chunks=3, **HEAD)]
    # bf16 tokens
    pts += [_p("bf16_d96_P7", "bf16 pooling, d/4 = 24 lanes, P below the unroll", "fast", dtype="bfloat16", d=96, P=7),
            _p("bf16_d1056", "bf16 pool_frames + rows kernels (no pool_rows2 shape)", "fast", dtype="bfloat16", d=1056)]
    # chunks per call and max_batch_chunks
    pts += [_p("c1", "first chunk only: no draw, no sub-batch", "fast", n_chunks=1),
            _p("c2", "one infinite-memory chunk", "fast", n_chunks=2)]
    for maxC in (1, 3, 32):
        for n, tag in ((maxC, "maxC"), (maxC + 1, "maxC+1"), (2 * maxC + 1, "2maxC+1")):
            if (maxC, n) in ((1, 1), (1, 2)):
                continue                                     # c1 / c2 with sub-batches of one chunk: below
            pts.append(_p(f"maxC{maxC}_c{n}", f"{tag} chunks with sub-batches of {maxC}", "fast", max_batch_chunks=maxC, n_chunks=n))
    pts += [_p("maxC1_c1", "maxC chunks with sub-batches of 1", "fast", max_batch_chunks=1, n_chunks=1),
            _p("maxC1_c2", "maxC + 1 chunks with sub-batches of 1", "fast", max_batch_chunks=1, n_chunks=2)]
    # headline base either side of M = rows * chunks = 1024 (64 new rows per chunk)
    pts += [_p("head_M960", "sub-batch of 15 chunks: M = 960 < 1024, split-K fp32 GEMM", "fast", n_chunks=16, **HEAD),
            _p("head_M1024", "sub-batch of 16 chunks: M = 1024, six-product bf16 GEMM", "fast", n_chunks=17, **HEAD),
            _p("head_M1024_d96_vsplit", "split-bf16 V' projection refused by d % 64: exact fp32 GEMM on the UC stream", "fast",
               n_chunks=17, d=96, v_split=True, **HEAD),
            _p("head_M1024_vsplit", "split-bf16 V' projection (d % 64 == 0, v_cols % 128 == 0)", "fast", n_chunks=17, v_split=True, **HEAD)]
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# b) a fixed-seed random sample of combinations of the values above
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_POINTS = 32
RANDOM_SEED = 20261016
_VALUES = dict(
    S=(4, 64, 100, 102, 256, 508, 512, 516, 1000, 1024), H=(1, 2, 3, 5, 8, 12, 16, 20), d=(32, 96, 160, 768, 1024, 1056, 1408, 2048),
    P=(1, 2, 7, 32, 49, 196, 257), Q=(1, 4, 5, 8, 9, 12, 31, 32, 33, 36, 64, 96, 97, 128, 256), L=(1, 2, 3, 5, 6, 8),
    N=(16, 32, 64, 128, 256), T=(2, 3, 8, 255, 256, 300), tau=(0.5, 0.75, 0.9), sticky=(True, True, True, False),
    dtype=("float32", "float32", "bfloat16"), max_batch_chunks=(1, 3, 32), n_chunks=(1, 2, 3, 4, 7))


def device_bytes(pt: SweepPoint) -> int:
    """Upper estimate of what one engine and the call's inputs and outputs hold on the device."""
    tok = sum(pt.Ts) * pt.P * pt.d * (2 if pt.dtype == "bfloat16" else 4)
    state = 2 * pt.L * pt.N * (pt.d + 2 * pt.dm) * 4 + 3 * pt.L * pt.H * pt.Q * pt.N * 4
    ring = (5 * min(pt.max_batch_chunks, 32) + 2) * pt.L * pt.H * pt.Q * (pt.N + 128) * 4
    out = pt.chunks * pt.L * pt.Q * pt.dm * 4
    return tok + state + ring + out


def _random_sample() -> List[SweepPoint]:
    rng = np.random.default_rng(RANDOM_SEED)
    keys = list(_VALUES)
    pts: List[SweepPoint] = []
    while len(pts) < RANDOM_POINTS:
        kw = {k: _VALUES[k][int(rng.integers(len(_VALUES[k])))] for k in keys}
        kw = {k: (v.item() if hasattr(v, "item") else v) for k, v in kw.items()}
        pt = replace(SMALL, name=f"rand{len(pts):02d}", gate="random combination", families="", **kw)
        try:
            if basis_maps.build_plan(pt.T, pt.N, pt.tau, pt.S).dense:
                continue                                      # (dense plans: swept in dense_sweep_cases.py)
        except (basis_maps.UnsupportedBasis, ValueError):
            continue
        if device_bytes(pt) > 2 << 30:
            continue
        pts.append(replace(pt, families=expected_families(pt), gate="random combination: " + expected_path(pt)))
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# c) refusal points: (name, config overrides, call-time Q or None, expected codes)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Refusal:
    name: str
    where: str                     # "create" | "call"
    cfg: Dict[str, int]            # overrides of the small base's infv_ltm_config
    call_Q: Optional[int] = None   # query length passed to the first call (Q > max_q)


REFUSALS = [
    Refusal("S1025", "create", dict(nb_samples=1025)),
    Refusal("S4096", "create", dict(nb_samples=4096)),
    Refusal("d48", "create", dict(d_in=48)),
    Refusal("dh32", "create", dict(head_size=32)),
    Refusal("Q_gt_max_q", "call", dict(max_q=32), call_Q=33),
]

ONE_FACTOR = _one_factor()
RANDOM = _random_sample()
POINTS: List[SweepPoint] = ONE_FACTOR + RANDOM
assert len({p.name for p in POINTS}) == len(POINTS), "sweep point names must be unique"
BY_NAME = {p.name: p for p in POINTS}


def refusal_as_point(r: Refusal) -> SweepPoint:
    """A refusal point in the gates' coordinates (the S refusals are what crosses ``videos.S<=1024``)."""
    return replace(SMALL, name=r.name, gate="refusal", S=r.cfg.get("nb_samples", SMALL.S), d=r.cfg.get("d_in", SMALL.d))


# ---------------------------------------------------------------------------------------------------------------------
# video Q-former: infv_vqf_short_attention (vqf_capi.hip: enc_width % 64 and n_tokens % 64 select the split-bf16 GEMMs)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class VqfPoint:
    name: str
    n_heads: int = 12
    enc_width: int = 768
    n_query: int = 32
    n_tokens: int = 96


VQF_BASE = VqfPoint("vqf_base")


def _vqf_points() -> List[VqfPoint]:
    pts = [VQF_BASE]
    pts += [replace(VQF_BASE, name=f"heads{h}", n_heads=h) for h in (1, 4, 16, 21)]
    pts += [replace(VQF_BASE, name=f"enc{w}", enc_width=w) for w in (32, 96, 1024, 1408)]
    pts += [replace(VQF_BASE, name=f"nq{q}", n_query=q) for q in (1, 5, 33, 96, 256)]
    pts += [replace(VQF_BASE, name=f"tok{t}", n_tokens=t) for t in (32, 64, 3136, 8192)]
    rng = np.random.default_rng(RANDOM_SEED + 1)
    pick = lambda v: int(v[int(rng.integers(len(v)))])
    for i in range(8):
        pts.append(VqfPoint(f"vqf_rand{i}", pick((1, 4, 12, 16, 21)), pick((32, 96, 768, 1024, 1408)),
                            pick((1, 5, 32, 33, 96, 256)), pick((32, 64, 96, 3136, 8192))))
    return pts


VQF_POINTS = _vqf_points()
VQF_GATES = {
    "vqf.enc_width%64": lambda p: p.enc_width % 64 == 0,
    "vqf.n_tokens%64": lambda p: p.n_tokens % 64 == 0,
}


# ---------------------------------------------------------------------------------------------------------------------
# inputs of a point (infinite_video_amd.synth; nothing is stored)
# ---------------------------------------------------------------------------------------------------------------------
def call_seed(pt: SweepPoint, chunk: int, layer: int) -> int:
    """Seed of torch's CPU generator in front of the forward of (chunk, layer), as the golden cases do it."""
    return 70000 + 100 * chunk + layer


def uniforms(pt: SweepPoint) -> np.ndarray:
    """u [chunks, L, S] float64: what ``torch.rand(S, float64)`` returns right after ``torch.manual_seed(call_seed)`` --
    the draw the reference-shaped DenseOracle makes from the global generator seeded the same way."""
    import torch
    u = np.empty((pt.chunks, pt.L, pt.S), np.float64)
    for c in range(pt.chunks):
        for l in range(pt.L):
            g = torch.Generator().manual_seed(call_seed(pt, c, l))
            u[c, l] = torch.rand(pt.S, dtype=torch.float64, generator=g).numpy()
    return u


def point_inputs(pt: SweepPoint):
    """(ks, qs, ws, u): tokens of every chunk [T_c*P, d] fp32 (rounded to bf16 values when the point passes bf16 tokens),
    queries [L, Q, dm], projections per layer, uniforms [chunks, L, S]."""
    import torch
    from infinite_video_amd import synth
    ks = [synth.frame_tokens(c, T, pt.P, pt.d) for c, T in enumerate(pt.Ts)]
    if pt.dtype == "bfloat16":
        ks = [torch.from_numpy(k).to(torch.bfloat16).float().numpy() for k in ks]
    qs = np.stack([synth.layer_query(l, pt.Q, pt.dm) for l in range(pt.L)])
    ws = [synth.layer_projections(l, pt.d, pt.dm) for l in range(pt.L)]
    return ks, qs, ws, uniforms(pt)
