"""Thin torch-facing wrapper of one ``infv_ltm_handle``: device pointers in, device tensors out.

PyTorch is plumbing here (device memory, the current HIP stream); every number is produced by
the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .basis_maps import (NB_BINS, NB_SAMPLES, REFERENCE_DENSITY_SEGMENTS, GridPlan, Plan, build_gaussian_plan, build_grid_plan,
                         build_plan, padded_N)

ProjTensors = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]   # (wk, bk, wv, bv)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _np_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


TOKEN_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}      # infv_token_dtype (2 is not a code)
# INFV_TOKENS_F8E4M3, declared beside the enum: OCP e4m3fn, one byte per element, the caller's storage choice (e.g.
# ``tokens.to(torch.float8_e4m3fn)`` when caching features).  The library neither quantises nor scales: its results on the fp8 tensor
# are the bits of its results on ``tensor.float()``.
F8_TOKEN_DTYPES = {torch.float8_e4m3fn: 4}
_OTHER_FP8 = tuple(getattr(torch, n) for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n))


def token_code(dtype) -> Optional[int]:
    """The token dtype code the kernels read ``dtype`` under (``TOKEN_DTYPES`` and ``F8_TOKEN_DTYPES``), or None for a dtype
    they do not read in place.  The fp8 encodings other than OCP e4m3fn raise: silently widening them would hide that the one-byte
    layout the kernels read is ``torch.float8_e4m3fn`` alone."""
    if dtype in _OTHER_FP8:
        raise TypeError(f"fp8 frame tokens must be torch.float8_e4m3fn (OCP e4m3, no scale), got {dtype}")
    code = TOKEN_DTYPES.get(dtype)
    return F8_TOKEN_DTYPES.get(dtype) if code is None else code


def aligned_tokens(k: torch.Tensor) -> torch.Tensor:
    """``k`` itself where the kernels can read it in place, else a contiguous, 16-byte aligned copy in its own dtype."""
    if not k.is_contiguous() or k.data_ptr() % 16:
        k = k.clone(memory_format=torch.contiguous_format)
        if k.data_ptr() % 16:                       # (an allocator that hands out less than 16-byte alignment: none known)
            raise RuntimeError("could not allocate a 16-byte aligned copy of the frame tokens")
    return k


def _check_dev(t: torch.Tensor, device: torch.device, name: str, dtype=torch.float32):
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, engine is on {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


class LTMEngine:
    """``n_layers`` LTM instances (one per cross-attention layer) stepped together on one GPU."""

    def __init__(self, num_basis: int, n_heads: int, head_size: int, d_in: int, tokens_per_frame: int,
                 tau: float, sticky: bool, n_layers: int = 1, max_q: int = 32,
                 device: Optional[torch.device] = None, nb_samples: int = NB_SAMPLES,
                 max_batch_chunks: int = 32, gaussian_sigmas: Optional[Sequence[float]] = None,
                 rng_seed: Optional[int] = None, rng_stream: int = 0, fp16_tokens: bool = False):
        """``fp16_tokens``: the tensor methods (``pool``, ``pool_rows``, ``forward``, ``consolidate*``) also take ``torch.float16``
        frame tokens and read them in place (INFV_TOKENS_F16: the bits of the run on ``k.float()``).  Off by default -- an engine
        then refuses fp16 tensors with a ``TypeError`` as it always has; the attribute of the same name may be set later.  The raw
        entry points (``forward_into_raw``, ``pool_into``) take the code from their caller and are not gated.
        ``rng_seed``: turn the device rng on at creation (``set_device_rng``).  ``gaussian_sigmas``: use the reference's Gaussian basis family (``add_gaussian_basis_functions``,
        long_term_attention_gibbs.py:167-174: centres ``linspace(0, 1, num_basis // len(sigmas))`` x these widths) instead
        of the rectangular one the active reference module builds; every step then takes the dense per-call path."""
        self.lib = _lib.load()
        self.fp16_tokens = bool(fp16_tokens)
        if not torch.cuda.is_available():
            raise RuntimeError("LTMEngine needs a HIP device (no CPU fallback exists)")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.H, self.dh, self.d, self.P = num_basis, n_heads, head_size, d_in, tokens_per_frame
        self.dm = n_heads * head_size
        self.tau, self.sticky, self.L, self.S = float(tau), bool(sticky), n_layers, nb_samples
        self.max_q = max_q
        self.gaussian_sigmas = tuple(float(x) for x in gaussian_sigmas) if gaussian_sigmas else None
        # the reference takes any --num_basis (run_inference_inf_video_llama_nextqa.py:61); the kernels tile the basis dimension
        # by 16, so the device holds Np = the next multiple of 16 -- the extra basis functions are inert (basis_maps.padded_N)
        self.Np = padded_N(num_basis)
        if self.Np != num_basis and self.gaussian_sigmas:
            raise ValueError("the Gaussian family needs num_basis to be a multiple of 16")
        cfg = _lib.Config(self.Np, n_heads, head_size, d_in, tokens_per_frame, n_layers, nb_samples,
                          int(self.sticky), max_q, max_batch_chunks)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_create(C.byref(cfg), C.byref(handle)))
        self._h = handle
        self.ctx_sum_on = False
        self._plans = {}
        self._token_dtype = torch.float32
        self.rng_seed, self.rng_stream = None, 0
        if rng_seed is not None:
            self.set_device_rng(rng_seed, rng_stream)

    # ------------------------------------------------------------------ device rng
    def set_device_rng(self, seed: int, stream: int = 0):
        """Draw the Gibbs uniforms on the device (Philox4x32-10, include/infv_ltm.h "Device rng"): from now on ``u=None`` on an
        existing sticky memory is generated by the kernels from ``(seed, stream, layer, rng_position, slot)``; an explicit
        ``u`` still wins.  ``philox.gibbs_uniforms(seed, stream, pos0, n_steps, L, S)`` reproduces the values on the host."""
        seed, stream = int(seed), int(stream)
        if not 0 <= seed < 1 << 64 or not 0 <= stream < 1 << 32:
            raise ValueError("seed must fit 64 bits and stream 32 bits, unsigned")
        _lib.check(self.lib.infv_ltm_set_rng(self._h, 1, seed, stream))
        self.rng_seed, self.rng_stream = seed, stream

    def clear_device_rng(self):
        """Back to the default: a sticky step on an existing memory needs explicit ``u``."""
        _lib.check(self.lib.infv_ltm_set_rng(self._h, 0, 0, 0))
        self.rng_seed, self.rng_stream = None, 0

    @property
    def rng_position(self) -> int:
        """Steps taken since the last reset: the chunk index the next step draws for (0 = first chunk of a document)."""
        pos = C.c_uint32()
        _lib.check(self.lib.infv_ltm_get_rng_position(self._h, C.byref(pos)))
        return int(pos.value)

    @rng_position.setter
    def rng_position(self, pos: int):
        if not 0 <= int(pos) < 1 << 32:
            raise ValueError("rng_position must fit 32 bits, unsigned")
        _lib.check(self.lib.infv_ltm_set_rng_position(self._h, int(pos)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self.lib.infv_ltm_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ plans
    def ensure_plan(self, T: int) -> Plan:
        if T in self._plans:
            return self._plans[T]
        p = (build_gaussian_plan(int(T), self.N, self.tau, self.gaussian_sigmas, self.S) if self.gaussian_sigmas
             else build_plan(int(T), self.N, self.tau, self.S))
        arrs = dict(
            first_row_box=_np_i32(p.first_row_box), first_row_begin=_np_i32(p.first_row_begin),
            first_row_end=_np_i32(p.first_row_end), first_box_val=_np_f32(p.first_box_val),
            inf_row_box=_np_i32(p.inf_row_box), inf_row_begin=_np_i32(p.inf_row_begin),
            inf_row_end=_np_i32(p.inf_row_end), inf_box_val=_np_f32(p.inf_box_val),
            inf_old_ptr=_np_i32(p.inf_old_ptr), inf_old_slot=_np_i32(p.inf_old_slot),
            readout_w=_np_f32(p.readout_w), edge_box=_np_i32(p.edge_box), edge_dx=_np_f32(p.edge_dx),
            bin_box=_np_i32(p.bin_box), uniform_idx=_np_i32(p.uniform_idx))
        ip = lambda k: arrs[k].ctypes.data_as(_lib.i32p)
        fp = lambda k: arrs[k].ctypes.data_as(_lib.f32p)
        s = _lib.PlanStruct(
            T=int(T), first_rows=len(p.first_row_box), first_row_box=ip("first_row_box"),
            first_row_begin=ip("first_row_begin"), first_row_end=ip("first_row_end"),
            first_box_val=fp("first_box_val"), inf_rows=len(p.inf_row_box), inf_row_box=ip("inf_row_box"),
            inf_row_begin=ip("inf_row_begin"), inf_row_end=ip("inf_row_end"), inf_box_val=fp("inf_box_val"),
            inf_old_ptr=ip("inf_old_ptr"), inf_old_slot=ip("inf_old_slot"), readout_w=fp("readout_w"),
            readout_w_out=p.readout_w_out, n_bins=NB_BINS, edge_box=ip("edge_box"), edge_dx=fp("edge_dx"),
            bin_box=ip("bin_box"), uniform_idx=ip("uniform_idx"))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_plan(self._h, C.byref(s)))
            if p.dense:
                # num_basis whose fp32 boxes overlap where the step looks: dense operators (x . G on fp32 MFMA) and
                # two-box tables; every entry point then takes the per-call dense step
                dn = dict(first_GT=_np_f32(p.first_GT), inf_GT=_np_f32(p.inf_GT), bin_box2=_np_i32(p.bin_box2),
                          edge_box2=_np_i32(p.edge_box2), uniform_box2=_np_i32(p.uniform_box2))
                ds = _lib.DensePlanStruct(
                    T=int(T), first_K=int(p.first_GT.shape[1]), first_GT=dn["first_GT"].ctypes.data_as(_lib.f32p),
                    inf_K=int(p.inf_GT.shape[1]), inf_GT=dn["inf_GT"].ctypes.data_as(_lib.f32p),
                    bin_box2=dn["bin_box2"].ctypes.data_as(_lib.i32p), edge_box2=dn["edge_box2"].ctypes.data_as(_lib.i32p),
                    uniform_box2=dn["uniform_box2"].ctypes.data_as(_lib.i32p))
                _lib.check(self.lib.infv_ltm_set_dense_plan(self._h, C.byref(ds)))
            if p.psi:
                # a basis family whose psi(t) is a dense row (the reference's Gaussian family): psi wherever the step evaluates it
                pn = {k: _np_f32(getattr(p, k)) for k in ("psi_edge", "psi_bin", "psi_uniform", "psi_grid", "grid_w")}
                ps = _lib.PsiPlanStruct(T=int(T), n_grid=int(p.psi_grid.shape[0]),
                                        **{k: v.ctypes.data_as(_lib.f32p) for k, v in pn.items()})
                _lib.check(self.lib.infv_ltm_set_psi_plan(self._h, C.byref(ps)))
        self._plans[T] = p
        return p

    def set_dense_operators(self, T: int, first_GT: np.ndarray, inf_GT: Optional[np.ndarray] = None):
        """Replace the operators of chunk length ``T`` by caller-supplied DENSE ones (``first_GT`` [N, T], ``inf_GT`` [N, S + T],
        transposed ``G`` of long_term_attention_gibbs.py:68-84): every step of that length then runs the dense kernels
        (``B = x . G`` on fp32 MFMA).  The resampling / histogram tables stay those of the rectangular basis -- this is the
        operator-level hook for another basis family (e.g. ``basis_maps.gaussian_first_operator_T``), not a second model."""
        from .basis_maps import NB_BINS as _NB, boxes2_of
        self.ensure_plan(T)
        first = _np_f32(first_GT)
        inf = _np_f32(inf_GT) if inf_GT is not None else np.zeros((self.N, self.S + T), np.float32)
        if first.shape != (self.N, T) or inf.shape != (self.N, self.S + T):
            raise ValueError(f"operators must be [{self.N}, {T}] and [{self.N}, {self.S + T}]")
        if self.Np != self.N:
            first = _np_f32(np.concatenate([first, np.zeros((self.Np - self.N, T), np.float32)]))
            inf = _np_f32(np.concatenate([inf, np.zeros((self.Np - self.N, self.S + T), np.float32)]))
        bins = torch.linspace(0, 1, _NB + 1)
        mod = bins.clone()
        mod[0] = -.000001
        mod[-1] = 1.000001
        t_uni = (torch.arange(1, self.S + 1).float() * self.tau / self.S) / self.tau
        tabs = [_np_i32(boxes2_of(x, self.N)) for x in (bins[:-1], mod, t_uni)]
        ds = _lib.DensePlanStruct(
            T=int(T), first_K=int(T), first_GT=first.ctypes.data_as(_lib.f32p), inf_K=int(self.S + T),
            inf_GT=inf.ctypes.data_as(_lib.f32p), bin_box2=tabs[0].ctypes.data_as(_lib.i32p),
            edge_box2=tabs[1].ctypes.data_as(_lib.i32p), uniform_box2=tabs[2].ctypes.data_as(_lib.i32p))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_dense_plan(self._h, C.byref(ds)))

    # ------------------------------------------------------------------ helpers
    def _proj_array(self, projs: Sequence[ProjTensors]):
        if len(projs) != self.L:
            raise ValueError(f"expected projections for {self.L} layers, got {len(projs)}")
        # the same weight tensors call after call (the per-chunk loop): validated once, the ctypes array is reused
        key = tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t.device) for p in projs for t in p)
        cached = getattr(self, "_proj_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        arr = (_lib.Proj * self.L)()
        for l, (wk, bk, wv, bv) in enumerate(projs):
            for name, t, shape in (("wk", wk, (self.dm, self.d)), ("bk", bk, (self.dm,)),
                                   ("wv", wv, (self.dm, self.d)), ("bv", bv, (self.dm,))):
                _check_dev(t, self.device, f"{name}[{l}]")
                if tuple(t.shape) != shape:
                    raise ValueError(f"{name}[{l}] has shape {tuple(t.shape)}, expected {shape}")
            arr[l] = _lib.Proj(wk.data_ptr(), bk.data_ptr(), wv.data_ptr(), bv.data_ptr())
        self._proj_cache = (key, arr, [tuple(p) for p in projs])      # (the tensors are kept alive with their addresses)
        return arr

    def _check_q(self, q: torch.Tensor) -> int:
        _check_dev(q, self.device, "q")
        if q.dim() != 3 or q.shape[0] != self.L or q.shape[2] != self.dm:
            raise ValueError(f"q must be [{self.L}, Q, {self.dm}], got {tuple(q.shape)}")
        if q.shape[1] > self.max_q:
            raise ValueError(f"Q={q.shape[1]} exceeds max_q={self.max_q}")
        return int(q.shape[1])

    def _check_u(self, u: Optional[torch.Tensor], lead: Tuple[int, ...]):
        if u is None:
            return
        _check_dev(u, self.device, "u", torch.float64)
        if tuple(u.shape) != lead + (self.L, self.S):
            raise ValueError(f"u must be {lead + (self.L, self.S)}, got {tuple(u.shape)}")

    @property
    def has_memory(self) -> bool:
        return bool(_lib.check(self.lib.infv_ltm_has_memory(self._h)))

    def reset(self):
        _lib.check(self.lib.infv_ltm_reset(self._h))

    def _tokens(self, k: torch.Tensor):
        """Frame tokens may be fp32 (the reference's layout), fp16 (what its fp16 producer holds: read at half the bytes, same
        bits as the fp32 run) or bf16 (a producer that rounds them): tell the handle which one this call passes."""
        code = token_code(k.dtype)
        if code is None or (k.dtype == torch.float16 and not self.fp16_tokens):
            raise TypeError("frame tokens must be float32, bfloat16 or float8_e4m3fn (float16 on an engine created with "
                            f"fp16_tokens=True), got {k.dtype}")
        if code == 4 and k.device == self.device:   # fp8 is read in 4-byte vectors: a view off a 16-byte boundary is copied, in fp8
            k = aligned_tokens(k)
        _check_dev(k, self.device, "k", k.dtype)
        # always: the dtype is sticky state of the handle and other users of the handle (the video Q-former's C path) set it
        # too, so a Python-side cache of it could go stale
        _lib.check(self.lib.infv_ltm_set_token_dtype(self._h, code))
        self._token_dtype = k.dtype
        self._token_code = code
        return k

    # ------------------------------------------------------------------ operators
    def pool(self, k: torch.Tensor) -> torch.Tensor:
        """k [..., T*P, d] (fp32, bf16 or fp8 e4m3; fp16 on an engine with fp16_tokens=True) -> frame means [..., T, d] fp32   (reference :304)."""
        k = self._tokens(k)
        if k.shape[-1] != self.d or k.shape[-2] % self.P:
            raise ValueError(f"k must be [..., T*{self.P}, {self.d}], got {tuple(k.shape)}")
        n_frames = k.numel() // (self.P * self.d)
        out = torch.empty(k.shape[:-2] + (k.shape[-2] // self.P, self.d), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_pool(self._h, _ptr(k), n_frames, _ptr(out), _stream(self.device)))
        return out

    def pool_rows(self, k: torch.Tensor) -> torch.Tensor:
        """k [C, T*P, d] (fp32, bf16 or fp8 e4m3; fp16 with fp16_tokens=True) -> the memory's new rows R [C, rows, d] fp32: frame means (reference :304) summed
        per box row with the operator's weights (reference :216), one pass over the tokens.  Sparse plans only."""
        k = self._tokens(k)
        if k.dim() != 3 or k.shape[-1] != self.d or k.shape[-2] % self.P:
            raise ValueError(f"k must be [C, T*{self.P}, {self.d}], got {tuple(k.shape)}")
        n_chunks, T = int(k.shape[0]), int(k.shape[1]) // self.P
        self.ensure_plan(T)
        rows = _lib.check(self.lib.infv_ltm_new_rows(self._h, T))
        out = torch.empty(n_chunks, rows, self.d, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_pool_rows(self._h, _ptr(k), n_chunks, T, _ptr(out), _stream(self.device)))
        return out

    def step(self, kbar: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
             u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One chunk from pooled frames kbar [T, d]; q [L, Q, dm]; u [L, S] f64 -> ctx [L, Q, dm]."""
        _check_dev(kbar, self.device, "kbar")
        T = int(kbar.shape[0])
        Q = self._check_q(q)
        self._check_u(u, ())
        self.ensure_plan(T)
        ctx = torch.empty(self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_step(self._h, _ptr(kbar), T, _ptr(q), Q, self._proj_array(projs),
                                               _ptr(u), _ptr(ctx), _stream(self.device)))
        return ctx

    # -- lean entry points of the drop-in module's per-call path: the caller has validated shapes / dtypes / devices once for
    #    this call signature; nothing is re-checked here, no context manager is entered (the caller's device is current)
    def pool_into(self, k: torch.Tensor, kbar: torch.Tensor, n_frames: int, token_code: int, stream: C.c_void_p):
        # (``token_code``: any token dtype code -- 0 fp32, 1 bf16, 3 fp16, 4 fp8 e4m3; the caller vouches for it, ``fp16_tokens`` does not gate it)
        # the token dtype is sticky state of the C handle and other callers of the same handle change it (the video
        # Q-former's C path forces fp32): always set it, one cheap host call, never trust a Python-side cache
        _lib.check(self.lib.infv_ltm_set_token_dtype(self._h, token_code))
        rc = self.lib.infv_ltm_pool(self._h, C.c_void_p(k.data_ptr()), n_frames, C.c_void_p(kbar.data_ptr()), stream)
        if rc < 0:
            _lib.check(rc)

    def step_raw(self, kbar_ptr: int, T: int, q_ptr: int, Q: int, proj_arr, u_ptr: int, ctx_ptr: int, stream: C.c_void_p):
        """infv_ltm_step on raw addresses; ``u_ptr`` may be pinned host memory (the draw reads its 4 KB through the mapping)."""
        rc = self.lib.infv_ltm_step(self._h, C.c_void_p(kbar_ptr), T, C.c_void_p(q_ptr), Q, proj_arr,
                                    C.c_void_p(u_ptr) if u_ptr else None, C.c_void_p(ctx_ptr), stream)
        if rc < 0:
            _lib.check(rc)

    def forward_into_raw(self, k_ptr: int, token_code: int, T: int, kbar_ptr: int, q_ptr: int, Q: int, proj_arr, u_ptr: int,
                         ctx_ptr: int, stream: C.c_void_p):
        """infv_ltm_forward_into on raw addresses (``token_code``: 0 fp32, 1 bf16, 3 fp16, 4 fp8 e4m3; not gated by ``fp16_tokens``): set the token dtype, pool k into the caller's kbar, step from it -- ONE C call
        (the drop-in module's steady-state forward; ``pool_into`` + ``step_raw`` were three)."""
        rc = self.lib.infv_ltm_forward_into(self._h, C.c_void_p(k_ptr), token_code, T, C.c_void_p(kbar_ptr), C.c_void_p(q_ptr), Q,
                                            proj_arr, C.c_void_p(u_ptr) if u_ptr else None, C.c_void_p(ctx_ptr), stream)
        if rc < 0:
            _lib.check(rc)

    def forward(self, k: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
                u: Optional[torch.Tensor] = None, new_doc: bool = False) -> torch.Tensor:
        """LongTermAttention.forward for all layers: k [T*P, d], q [L, Q, dm] -> ctx [L, Q, dm]."""
        k = self._tokens(k)
        if k.dim() != 2 or k.shape[1] != self.d or k.shape[0] % self.P:
            raise ValueError(f"k must be [T*{self.P}, {self.d}], got {tuple(k.shape)}")
        T = k.shape[0] // self.P
        Q = self._check_q(q)
        self._check_u(u, ())
        self.ensure_plan(T)
        ctx = torch.empty(self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_forward(self._h, _ptr(k), T, _ptr(q), Q, self._proj_array(projs),
                                                  _ptr(u), int(new_doc), _ptr(ctx), _stream(self.device)))
        return ctx

    def consolidate(self, k: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
                    u: Optional[torch.Tensor] = None, new_doc: bool = True,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Whole-video loop: k [C, T*P, d] (fp32, bf16 or fp8 e4m3; fp16 with fp16_tokens=True), q [L, Q, dm], u [C, L, S] -> ctx [C, L, Q, dm]."""
        k = self._tokens(k)
        if k.dim() != 3 or k.shape[2] != self.d or k.shape[1] % self.P:
            raise ValueError(f"k must be [C, T*{self.P}, {self.d}], got {tuple(k.shape)}")
        Cn, T = int(k.shape[0]), k.shape[1] // self.P
        Q = self._check_q(q)
        self._check_u(u, (Cn,))
        self.ensure_plan(T)
        if out is None:
            out = torch.empty(Cn, self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        else:
            _check_dev(out, self.device, "out")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_consolidate(self._h, _ptr(k), Cn, T, _ptr(q), Q, self._proj_array(projs),
                                                      _ptr(u), int(new_doc), _ptr(out), _stream(self.device)))
        return out

    def consolidate_pooled(self, kbar: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
                           u: Optional[torch.Tensor] = None, new_doc: bool = True) -> torch.Tensor:
        """consolidate() from frame means the caller already holds: kbar [C, T, d] fp32 (= pool() of the tokens).
        Bit-identical to consolidate() on those tokens; the pooling stage drops out."""
        _check_dev(kbar, self.device, "kbar")
        if kbar.dim() != 3 or kbar.shape[2] != self.d or kbar.dtype != torch.float32:
            raise ValueError(f"kbar must be fp32 [C, T, {self.d}], got {kbar.dtype} {tuple(kbar.shape)}")
        Cn, T = int(kbar.shape[0]), int(kbar.shape[1])
        Q = self._check_q(q)
        self._check_u(u, (Cn,))
        self.ensure_plan(T)
        out = torch.empty(Cn, self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_consolidate_pooled(self._h, _ptr(kbar), Cn, T, _ptr(q), Q, self._proj_array(projs),
                                                             _ptr(u), int(new_doc), _ptr(out), _stream(self.device)))
        return out

    def consolidate_q(self, k: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
                      u: Optional[torch.Tensor] = None, new_doc: bool = True) -> torch.Tensor:
        """Whole-video loop with a DIFFERENT query per chunk (a cross-attention layer after the first, Qformer.py:211):
        k [C, T*P, d], q [C, L, Q, dm], u [C, L, S] -> ctx [C, L, Q, dm].  Pooling and new-row projections are batched,
        the memory chain runs chunk by chunk; equals C calls of forward()."""
        k = self._tokens(k)
        if k.dim() != 3 or k.shape[2] != self.d or k.shape[1] % self.P:
            raise ValueError(f"k must be [C, T*{self.P}, {self.d}], got {tuple(k.shape)}")
        Cn, T = int(k.shape[0]), k.shape[1] // self.P
        _check_dev(q, self.device, "q")
        if q.dim() != 4 or q.shape[0] != Cn or q.shape[1] != self.L or q.shape[3] != self.dm or q.shape[2] > self.max_q:
            raise ValueError(f"q must be [{Cn}, {self.L}, Q <= {self.max_q}, {self.dm}], got {tuple(q.shape)}")
        Q = int(q.shape[2])
        self._check_u(u, (Cn,))
        self.ensure_plan(T)
        out = torch.empty(Cn, self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_consolidate_q(self._h, _ptr(k), Cn, T, _ptr(q), Q, self._proj_array(projs),
                                                        _ptr(u), int(new_doc), _ptr(out), _stream(self.device)))
        return out

    def steps(self, kbar: torch.Tensor, q: torch.Tensor, projs: Sequence[ProjTensors],
              u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``consolidate_q`` from frame means, on the memory as it stands (infv_ltm_steps): kbar [C, T, d] fp32, q [C, L, Q, dm],
        u [C, L, S] -> ctx [C, L, Q, dm]."""
        _check_dev(kbar, self.device, "kbar")
        _check_dev(q, self.device, "q")
        if kbar.dim() != 3 or kbar.shape[2] != self.d:
            raise ValueError(f"kbar must be fp32 [C, T, {self.d}], got {tuple(kbar.shape)}")
        Cn, T = int(kbar.shape[0]), int(kbar.shape[1])
        if q.dim() != 4 or q.shape[0] != Cn or q.shape[1] != self.L or q.shape[3] != self.dm or q.shape[2] > self.max_q:
            raise ValueError(f"q must be [{Cn}, {self.L}, Q <= {self.max_q}, {self.dm}], got {tuple(q.shape)}")
        Q = int(q.shape[2])
        self._check_u(u, (Cn,))
        self.ensure_plan(T)
        out = torch.empty(Cn, self.L, Q, self.dm, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_steps(self._h, _ptr(kbar), Cn, T, _ptr(q), Q, self._proj_array(projs), _ptr(u),
                                               _ptr(out), _stream(self.device)))
        return out

    # ------------------------------------------------------------------ state
    def export_state(self, layer: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(B_past [N, d], unnormalised sticky bin masses [127]) of one layer."""
        B = torch.empty(self.Np, self.d, device=self.device, dtype=torch.float32)
        mass = torch.empty(NB_BINS, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_export_state(self._h, layer, _ptr(B), _ptr(mass), _stream(self.device)))
        return B[:self.N], mass[:NB_BINS - 1]

    def import_state(self, layer: int, B: torch.Tensor, bin_mass: Optional[torch.Tensor], proj: ProjTensors):
        _check_dev(B, self.device, "B")
        if tuple(B.shape) != (self.N, self.d):
            raise ValueError(f"B must be [{self.N}, {self.d}]")
        if self.Np != self.N:                                   # inert rows of the padding basis functions
            B = torch.cat([B, torch.zeros(self.Np - self.N, self.d, device=B.device, dtype=B.dtype)])
        if bin_mass is not None:
            _check_dev(bin_mass, self.device, "bin_mass")
            if bin_mass.numel() != NB_BINS - 1:
                raise ValueError(f"bin_mass must have {NB_BINS - 1} entries")
        p = _lib.Proj(*(t.data_ptr() for t in proj))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_import_state(self._h, layer, _ptr(B), _ptr(bin_mass), C.byref(p),
                                                       _stream(self.device)))

    def set_ctx_sum(self, on: bool = True):
        """Have the fused ``consolidate`` keep the sum of its outputs as it stores them (infv_ltm_set_ctx_sum): ``pack_memory``
        of that call's ``ctx`` is then one launch that re-reads none of them."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_ctx_sum(self._h, int(bool(on))))
        self.ctx_sum_on = bool(on)

    def payload_numel(self, Q: int, with_scores: bool = False) -> int:
        """Floats of the hand-over payload: B | bin masses | (scores) | ctx_sum | count (video_memory.unpack_memory's layout)."""
        return (self.L * self.N * self.d + self.L * (NB_BINS - 1) + (self.L * self.H * Q * self.N if with_scores else 0) +
                self.L * Q * self.dm + 1)

    def pack_memory(self, ctx: torch.Tensor, with_scores: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The hand-over payload of the ``consolidate`` call that returned ``ctx`` [C, L, Q, dm], written by one kernel launch
        (infv_ltm_pack_memory; one more when the engine holds no sum for this ``ctx``): what ``video_memory.pack_local_memory``
        assembles, with ``ctx.sum(0)`` in the order include/infv_ltm.h states."""
        _check_dev(ctx, self.device, "ctx")
        if ctx.dim() != 4 or ctx.shape[1] != self.L or ctx.shape[3] != self.dm or ctx.shape[2] > self.max_q or not ctx.is_contiguous():
            raise ValueError(f"ctx must be contiguous [C, {self.L}, Q <= {self.max_q}, {self.dm}], got {tuple(ctx.shape)}")
        Cn, Q = int(ctx.shape[0]), int(ctx.shape[2])
        if out is None:
            payload = torch.empty(self.payload_numel(Q, with_scores), device=self.device, dtype=torch.float32)
        else:
            payload = out
            _check_dev(payload, self.device, "out")
            if payload.dim() != 1 or payload.numel() != self.payload_numel(Q, with_scores) or not payload.is_contiguous():
                raise ValueError(f"out must be a contiguous fp32 vector of {self.payload_numel(Q, with_scores)} elements")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_pack_memory(self._h, self.N, Q, _ptr(ctx), Cn, int(bool(with_scores)), _ptr(payload),
                                                     _stream(self.device)))
        return payload

    def export_chain_state(self, Q: int) -> torch.Tensor:
        """Everything ``consolidate`` carries from chunk to chunk as one fp32 device tensor (infv_ltm_export_chain_state):
        importing it into another engine and calling ``consolidate(..., new_doc=False)`` with the same query and weights
        continues the chain bit for bit."""
        n = int(self.lib.infv_ltm_chain_state_bytes(self._h, Q))
        if n <= 0:
            raise ValueError(f"bad query length {Q}")
        blob = torch.empty(n // 4, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_export_chain_state(self._h, Q, _ptr(blob), _stream(self.device)))
        return blob

    def import_chain_state(self, Q: int, blob: torch.Tensor):
        _check_dev(blob, self.device, "blob")
        if blob.numel() * 4 != int(self.lib.infv_ltm_chain_state_bytes(self._h, Q)):
            raise ValueError("chain-state blob does not match this engine's shape")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_import_chain_state(self._h, Q, _ptr(blob), _stream(self.device)))

    def chain_state_numel(self, Q: int) -> int:
        return int(self.lib.infv_ltm_chain_state_bytes(self._h, Q)) // 4

    def last_scores_device(self, Q: int) -> torch.Tensor:
        """Bias-free scores of the last step under the last call's query, [L, H, Q, N] on the device: the scores slice of the
        chain-state blob (layout: include/infv_ltm.h, infv_ltm_export_chain_state).  What SURVEY.md section 8e lists beside
        ``B_past`` in the all-gather payload: with them a peer can re-derive the sticky density on any grid."""
        blob = self.export_chain_state(Q)
        Np = self.Np                                                            # (the handle's basis count: padded to a multiple of 16)
        off = 16 + self.L * Np * self.d + self.L * Np * 2 * self.dm             # header (16 int32) | B | projected memory | scores | masses
        return blob[off:off + self.L * self.H * Q * Np].reshape(self.L, self.H, Q, Np)[..., :self.N]

    def reproject(self, projs: Sequence[ProjTensors]):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_reproject(self._h, self._proj_array(projs), _stream(self.device)))

    def last_draw(self, layer: int, want_scores: bool = False):
        """(bins [S], idx [S], probs [127][, scores [H,Q,N]]) of the last sticky step (host numpy)."""
        bins = np.empty(self.S, np.int32)
        idx = np.empty(self.S, np.int32)
        probs = np.empty(NB_BINS - 1, np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_get_draw(
                self._h, layer, bins.ctypes.data_as(_lib.i32p), idx.ctypes.data_as(_lib.i32p),
                probs.ctypes.data_as(_lib.f32p), None, _stream(self.device)))
        return bins, idx, probs

    def last_scores(self, layer: int, Q: int) -> np.ndarray:
        sc = np.empty((self.H, Q, self.Np), np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_get_draw(self._h, layer, None, None, None,
                                                  sc.ctypes.data_as(_lib.f32p), _stream(self.device)))
        return sc[:, :, :self.N]

    def set_probs(self, layer: int, probs: np.ndarray):
        p = _np_f32(probs)
        if p.size != NB_BINS - 1:
            raise ValueError(f"probs must have {NB_BINS - 1} entries")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_probs(self._h, layer, p.ctypes.data_as(_lib.f32p)))

    def set_bins(self, layer: int, bins: np.ndarray):
        """Forced draw of the next per-call step of ``layer`` (see infv_ltm_set_bins)."""
        b = _np_i32(bins)
        if b.size != self.S:
            raise ValueError(f"bins must have {self.S} entries")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_bins(self._h, layer, b.ctypes.data_as(_lib.i32p)))

    def set_trace(self, n_chunks: int):
        """Record the draw of every chunk of the following consolidate() calls: returns device tensors
        (bins [n_chunks, L, S] int32 initialised to -1, probs [n_chunks, L, 128] fp32); ``n_chunks = 0`` stops tracing."""
        if n_chunks <= 0:
            self._trace = None
            _lib.check(self.lib.infv_ltm_set_trace(self._h, None, None, 0))
            return None
        bins = torch.full((n_chunks, self.L, self.S), -1, device=self.device, dtype=torch.int32)
        probs = torch.zeros(n_chunks, self.L, NB_BINS, device=self.device, dtype=torch.float32)
        self._trace = (bins, probs)                       # keep the buffers alive while the library writes them
        _lib.check(self.lib.infv_ltm_set_trace(self._h, _ptr(bins), _ptr(probs), n_chunks))
        return bins, probs

    # ------------------------------------------------------------------ attention density (include/infv_ltm.h, "Read-outs ...")
    def set_grid_plan(self, segments=REFERENCE_DENSITY_SEGMENTS) -> GridPlan:
        """Register the grid of ``density``: ``segments`` of ``(lo, hi, n_points)`` (default: the reference's three 256-point
        segments, long_term_attention_gibbs.py:328-334).  Re-registered only when the segments change."""
        gp = build_grid_plan(self.N, tuple(tuple(s) for s in segments))
        if getattr(self, "_grid_plan", None) is gp:
            return gp
        arrs = (_np_i32(gp.seg_begin), _np_f32(gp.pt_weight), _np_i32(gp.pt_ptr), _np_i32(gp.pt_box), _np_f32(gp.pt_val))
        s = _lib.GridPlanStruct(
            n_points=len(gp.pt_weight), n_segments=len(gp.seg_begin) - 1, seg_begin=arrs[0].ctypes.data_as(_lib.i32p),
            pt_weight=arrs[1].ctypes.data_as(_lib.f32p), pt_ptr=arrs[2].ctypes.data_as(_lib.i32p),
            pt_box=arrs[3].ctypes.data_as(_lib.i32p), pt_val=arrs[4].ctypes.data_as(_lib.f32p))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_set_grid_plan(self._h, C.byref(s)))
        self._grid_plan = gp
        return gp

    def density(self, layer: int, Q: int, segments=REFERENCE_DENSITY_SEGMENTS) -> torch.Tensor:
        """The reference's ``alphas`` of the memory's last step of ``layer`` (infv_ltm_density): device fp32 ``[Q, 1, H, M]``,
        the layout the reference pickles (:337)."""
        gp = self.set_grid_plan(segments)
        out = torch.empty(Q, 1, self.H, len(gp.pt_weight), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_density(self._h, layer, Q, _ptr(out), _stream(self.device)))
        return out

    def masses(self, layer: int, Q: int) -> torch.Tensor:
        """What the read-out of the last step used: the mean over heads and queries of the softmax weights of every basis
        function (infv_ltm_masses), device fp32 ``[N]``."""
        out = torch.empty(self.Np, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_masses(self._h, layer, Q, _ptr(out), _stream(self.device)))
        return out[:self.N]

    def set_mass_trace(self, n_chunks: int) -> Optional[torch.Tensor]:
        """Record the masses of every chunk of the following ``steps`` / ``consolidate*`` calls (infv_ltm_set_mass_trace):
        returns the device tensor ``[n_chunks, L, N]`` fp32, NaN-initialised, that chunk c < n_chunks of a call writes row c
        of; ``n_chunks = 0`` stops tracing."""
        if n_chunks <= 0:
            self._mass_trace = None
            _lib.check(self.lib.infv_ltm_set_mass_trace(self._h, None, 0))
            return None
        buf = torch.full((n_chunks, self.L, self.Np), float("nan"), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.infv_ltm_set_mass_trace(self._h, _ptr(buf), n_chunks))
        self._mass_trace = buf                             # keep the buffer alive while the library writes it
        return buf[..., :self.N]

    def source_weights(self, bins: Optional[torch.Tensor], T: int, new_doc: bool = True, W: Optional[torch.Tensor] = None,
                       col_begin: int = 0, frames_per_source: Optional[int] = None, mass: Optional[torch.Tensor] = None,
                       normalise: bool = False):
        """Trace the memory back to the frames of the video (infv_ltm_source_weights; ``density.source_weights`` is its numpy
        mirror): ``W`` [L, N, M] with ``B[l][n] = sum_m W[l][n][m] * kbar[source m]``, source m being frames
        ``[m * g, (m + 1) * g)``, ``g = frames_per_source`` (default T: one column per chunk), ``M = col_begin + C * T / g``.

        ``bins`` [C, L, S] int32: the draws of the C chunks as ``set_trace`` recorded them (an engine that is not sticky reads only
        the chunk count ``bins.shape[0]`` of it, or takes ``None`` and the count from ``mass``).  ``new_doc=False`` continues a
        document: pass the ``W`` the call before returned and its column count as ``col_begin``; the result equals one call over
        all the chunks.  With ``mass`` [C, L, N] (``set_mass_trace`` of the same call) also returns ``attn`` [C, L, M], the
        attention map of the video after every chunk -- raw, or every row divided by its sum with ``normalise``.
        The call is one launch, but this wrapper then reads a counter of out-of-range bins back: a HOST SYNC.  Any such bin (an
        unwritten trace row holds -1) raises ``ValueError``; the raw entry point resamples a zero row for it instead."""
        if bins is None and mass is None:
            raise ValueError("bins or mass must say how many chunks the call has")
        C_ = int(bins.shape[0] if bins is not None else mass.shape[0])
        g = int(T if frames_per_source is None else frames_per_source)
        if C_ < 1 or g < 1 or T % g or col_begin < 0:
            raise ValueError("need at least one chunk, frames_per_source >= 1 dividing T, col_begin >= 0")
        self.ensure_plan(T)
        if self.sticky:
            if bins is None or tuple(bins.shape) != (C_, self.L, self.S):
                raise ValueError(f"a sticky engine needs bins [{C_}, {self.L}, {self.S}]")
            _check_dev(bins, self.device, "bins", torch.int32)
        else:
            bins = None
        if mass is not None:
            if tuple(mass.shape) != (C_, self.L, self.N):
                raise ValueError(f"mass must be [{C_}, {self.L}, {self.N}]")
            if self.Np != self.N:
                mass = torch.nn.functional.pad(mass, (0, self.Np - self.N))
            mass = mass.contiguous()
            _check_dev(mass, self.device, "mass")
        M = int(col_begin) + C_ * (T // g)
        ld = (M + 3) // 4 * 4
        buf = torch.empty(self.L, self.Np, ld, device=self.device, dtype=torch.float32)
        if not new_doc and col_begin:
            if W is None or tuple(W.shape[:2]) != (self.L, self.N) or W.shape[2] < col_begin:
                raise ValueError(f"W must be [{self.L}, {self.N}, >= {col_begin}] to continue a document")
            buf[:, :self.N, :col_begin] = W[:, :, :col_begin]
            buf[:, self.N:, :col_begin] = 0
        attn = torch.empty(C_, self.L, ld, device=self.device, dtype=torch.float32) if mass is not None else None
        bad = torch.zeros(self.L, device=self.device, dtype=torch.int32)
        desc = _lib.SourcesDesc(n_chunks=C_, T=int(T), new_doc=int(bool(new_doc)), frames_per_source=g,
                                col_begin=int(col_begin), ld=ld)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_source_weights(self._h, C.byref(desc), _ptr(bins), _ptr(buf), _ptr(mass), _ptr(attn),
                                                        _ptr(bad), _stream(self.device)))
        n_bad = bad.cpu()                                  # (the host sync)
        if int(n_bad.sum()):
            raise ValueError(f"bins outside [0, {NB_BINS - 1}) per layer: {n_bad.tolist()} (an unwritten trace row holds -1)")
        Wout = buf[:, :self.N, :M]
        if attn is None:
            return Wout
        attn = attn[:, :, :M]
        if normalise:
            attn = attn / attn.sum(-1, keepdim=True)
        return Wout, attn

    def sync(self):
        """Wait for the engine's work on the current stream and raise if a device-side failure was latched
        (the persistent chain kernel of consolidate() timed out: its outputs are invalid)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.infv_ltm_sync(self._h, _stream(self.device)))

    # ------------------------------------------------------------------ measurement
    def profile(self, on: bool):
        """Bracket every kernel launch of this engine with HIP events (bench.py's roofline leg)."""
        _lib.check(self.lib.infv_ltm_profile_enable(self._h, int(on)))

    def profile_read(self):
        """{kernel: (launches, total device ms)} since profiling was enabled; synchronises."""
        out = {}
        for i, name in enumerate(_lib.KERNELS):
            n, ms = C.c_int64(), C.c_double()
            _lib.check(self.lib.infv_ltm_profile_read(self._h, i, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out


def _same_config(a: LTMEngine, b: LTMEngine) -> bool:
    return ((a.N, a.Np, a.H, a.dh, a.d, a.P, a.L, a.S, a.sticky, a.tau, a.gaussian_sigmas, a.device) ==
            (b.N, b.Np, b.H, b.dh, b.d, b.P, b.L, b.S, b.sticky, b.tau, b.gaussian_sigmas, b.device))


def _video_engines(engines: Sequence[LTMEngine], chunk_counts, what: str):
    """The argument checks shared by the multi-video calls: (engines, cu) with cu the host int32 running sum of chunk_counts."""
    engines = list(engines)
    V = len(engines)
    if V == 0:
        raise ValueError(f"{what} needs at least one engine")
    if isinstance(chunk_counts, torch.Tensor):
        if chunk_counts.dim() != 1:
            raise ValueError("chunk_counts must be a list or a 1-D tensor")
        chunk_counts = chunk_counts.tolist()
    counts = [int(c) for c in chunk_counts]
    if len(counts) != V:
        raise ValueError(f"chunk_counts has {len(counts)} entries for {V} engines")
    if any(c < 0 for c in counts):
        raise ValueError(f"chunk_counts must be non-negative, got {counts}")
    e0 = engines[0]
    seen = set()
    for i, e in enumerate(engines):
        if not isinstance(e, LTMEngine):
            raise TypeError(f"engines[{i}] is not an LTMEngine")
        if id(e) in seen:
            raise ValueError(f"engines[{i}] appears twice: every video needs its own engine")
        seen.add(id(e))
        if not _same_config(e0, e):
            raise ValueError(f"engines[{i}] is configured differently from engines[0]")
    cu = np.zeros(V + 1, np.int32)
    cu[1:] = np.cumsum(counts)
    return engines, cu


def consolidate_videos(engines: Sequence[LTMEngine], k, chunk_counts, q: torch.Tensor, projs: Sequence[ProjTensors],
                       u=None, new_doc: bool = True) -> torch.Tensor:
    """Step V independent videos together (infv_ltm_consolidate_videos): engine v holds video v's memory.

    ``k`` is PACKED, [sum C_v, T*P, d] (fp32, bf16 or fp8 e4m3; fp16 if every engine has fp16_tokens=True) with video v's chunks at rows [cu[v], cu[v+1]) where cu is the running
    sum of ``chunk_counts`` (a list or 1-D tensor), and ``u`` likewise [sum C_v, L, S] float64 (None when not sticky).
    ``k`` (and ``u``) may also be lists of per-video [C_v, T*P, d] ([C_v, L, S]) tensors: they are then packed, which COPIES
    every video's tokens once.  ``q`` [L, Q, dm] and ``projs`` are shared by all videos.  new_doc=True starts every memory
    afresh; new_doc=False continues each engine's memory.  Returns ctx [sum C_v, L, Q, dm], packed the same way.
    Afterwards each engine is in the state its own ``consolidate`` on its chunks would have left it in."""
    if isinstance(k, (list, tuple)) and chunk_counts is None:
        chunk_counts = [int(x.shape[0]) for x in k]
    engines, cu = _video_engines(engines, chunk_counts, "consolidate_videos")
    if isinstance(k, (list, tuple)):
        k = torch.cat(list(k)) if len(k) else k
    if isinstance(u, (list, tuple)):
        u = torch.cat(list(u))
    V, e0 = len(engines), engines[0]
    total = int(cu[-1])
    if token_code(k.dtype) is None:
        raise TypeError(f"frame tokens must be float32, float16, bfloat16 or float8_e4m3fn, got {k.dtype}")
    if k.dtype == torch.float16 and not all(e.fp16_tokens for e in engines):   # (before any handle's dtype is touched)
        raise TypeError("float16 frame tokens need engines created with fp16_tokens=True")
    _check_dev(k, e0.device, "k", k.dtype)
    if k.dim() != 3 or k.shape[0] != total or k.shape[2] != e0.d or k.shape[1] % e0.P:
        raise ValueError(f"k must be [{total}, T*{e0.P}, {e0.d}], got {tuple(k.shape)}")
    T = int(k.shape[1]) // e0.P
    Q = e0._check_q(q)
    e0._check_u(u, (total,))
    for e in engines:
        k = e._tokens(k)                               # (a misaligned fp8 view is copied once: the copy is aligned for the rest)
        e.ensure_plan(T)
        e._check_q(q)
    proj_arr = e0._proj_array(projs)
    out = torch.empty(total, e0.L, Q, e0.dm, device=e0.device, dtype=torch.float32)
    hs = (C.c_void_p * V)(*[e._h.value for e in engines])
    with torch.cuda.device(e0.device):
        _lib.check(e0.lib.infv_ltm_consolidate_videos(C.cast(hs, C.c_void_p), V, C.c_void_p(cu.ctypes.data), _ptr(k), T, _ptr(q), Q, proj_arr,
                                                      _ptr(u), int(new_doc), _ptr(out), _stream(e0.device)))
    return out


def steps_videos(engines: Sequence[LTMEngine], kbar, chunk_counts, q: torch.Tensor, projs: Sequence[ProjTensors],
                 u=None, new_doc: bool = True, kbar_chunk0: Optional[Sequence[int]] = None) -> torch.Tensor:
    """``consolidate_videos`` from frame means, with an optional query per chunk (infv_ltm_steps_videos).

    ``kbar`` is PACKED [sum C_v, T, d] fp32 (``pool()`` of the tokens), or a list of per-video [C_v, T, d] tensors (packed with
    one copy).  ``q`` is either [L, Q, dm], shared by every chunk, or [sum C_v, L, Q, dm], one query per chunk (a cross-attention
    layer after the first, as ``steps`` takes it); ``q.dim()`` decides.  ``u``, ``chunk_counts``, ``new_doc`` and the result
    ctx [sum C_v, L, Q, dm] are ``consolidate_videos``'s.  With a shared query and kbar = pool(k) the bits equal
    ``consolidate_videos(k, q)``'s; each video's bits do not depend on the rest of the batch.

    ``kbar_chunk0`` [V] (infv_ltm_steps_videos_from): chunk i of video v reads its frame means at ``kbar[kbar_chunk0[v] + i]``,
    so several memories may step from one block of frame means; ``kbar`` is then PACKED [n, T, d] with every
    ``kbar_chunk0[v] + C_v <= n`` and ``chunk_counts`` is required.  ``u``, ``q`` and the result stay packed by video.  The
    bits are those of the call on a kbar that holds each video's own copy."""
    if isinstance(kbar, (list, tuple)) and chunk_counts is None:
        chunk_counts = [int(x.shape[0]) for x in kbar]
    engines, cu = _video_engines(engines, chunk_counts, "steps_videos")
    if isinstance(kbar, (list, tuple)):
        kbar = torch.cat(list(kbar)) if len(kbar) else kbar
    if isinstance(u, (list, tuple)):
        u = torch.cat(list(u))
    V, e0 = len(engines), engines[0]
    total = int(cu[-1])
    _check_dev(kbar, e0.device, "kbar")
    base = None
    if kbar_chunk0 is not None:
        base = np.ascontiguousarray(np.asarray(list(kbar_chunk0), dtype=np.int64))
        if base.shape != (V,):
            raise ValueError(f"{base.size} kbar_chunk0 entries for {V} videos")
        if kbar.dim() != 3 or kbar.shape[2] != e0.d:
            raise ValueError(f"kbar must be fp32 [n, T, {e0.d}], got {tuple(kbar.shape)}")
        if np.any(base + np.diff(cu) > kbar.shape[0]) or np.any(np.abs(base) >= 2 ** 31):
            raise ValueError(f"kbar_chunk0 + chunk_counts reaches beyond kbar's {kbar.shape[0]} chunks")
        base = np.ascontiguousarray(base.astype(np.int32))          # (a negative entry is the library's refusal)
    elif kbar.dim() != 3 or kbar.shape[0] != total or kbar.shape[2] != e0.d:
        raise ValueError(f"kbar must be fp32 [{total}, T, {e0.d}], got {tuple(kbar.shape)}")
    if kbar.data_ptr() % 16:
        raise ValueError("kbar must start at a 16-byte boundary (the chunks are copied as float4)")
    T = int(kbar.shape[1])
    if q.dim() == 4:
        _check_dev(q, e0.device, "q")
        if q.shape[0] != total or q.shape[1] != e0.L or q.shape[3] != e0.dm or q.shape[2] > e0.max_q:
            raise ValueError(f"q must be [{e0.L}, Q, {e0.dm}] or [{total}, {e0.L}, Q <= {e0.max_q}, {e0.dm}], got {tuple(q.shape)}")
        Q, per_chunk = int(q.shape[2]), 1
    else:
        Q, per_chunk = e0._check_q(q), 0
    e0._check_u(u, (total,))
    for e in engines:
        e.ensure_plan(T)
    proj_arr = e0._proj_array(projs)
    out = torch.empty(total, e0.L, Q, e0.dm, device=e0.device, dtype=torch.float32)
    hs = (C.c_void_p * V)(*[e._h.value for e in engines])
    with torch.cuda.device(e0.device):
        if base is not None:
            _lib.check(e0.lib.infv_ltm_steps_videos_from(C.cast(hs, C.c_void_p), V, C.c_void_p(cu.ctypes.data), _ptr(kbar),
                                                         C.c_void_p(base.ctypes.data), T, _ptr(q), per_chunk, Q, proj_arr, _ptr(u),
                                                         int(new_doc), _ptr(out), _stream(e0.device)))
        else:
            _lib.check(e0.lib.infv_ltm_steps_videos(C.cast(hs, C.c_void_p), V, C.c_void_p(cu.ctypes.data), _ptr(kbar), T, _ptr(q),
                                                    per_chunk, Q, proj_arr, _ptr(u), int(new_doc), _ptr(out), _stream(e0.device)))
    return out


def split_frames(frame_counts, T: int):
    """How ``torch.split(video, T, dim=1)`` cuts videos of ``frame_counts`` frames: ``(chunk_counts, tails, cu, frame0)`` -- video v
    has ``ceil(F_v / T)`` chunks, the last of ``tails[v]`` frames (T: full; 0 for a video without frames); ``cu`` [V+1] int32 is the
    running sum of the chunk counts (where u, ctx and per-chunk queries sit) and ``frame0`` [V+1] int64 that of the frame counts
    (where k / kbar sit).  A last chunk of ONE frame has an empty operator in the reference (LTM.py:79-82): ``ValueError``."""
    if isinstance(frame_counts, torch.Tensor):
        frame_counts = frame_counts.tolist()
    frames = [int(f) for f in frame_counts]
    T = int(T)
    if T < 2:
        raise ValueError(f"T must be at least 2, got {T}")
    counts, tails = [], []
    for v, f in enumerate(frames):
        if f < 0:
            raise ValueError(f"frame_counts[{v}] = {f} is negative")
        if f % T == 1:
            raise ValueError(f"video {v} has {f} frames: its last chunk would hold one frame (T = {T}), which the reference cannot step")
        counts.append(-(-f // T))
        tails.append(0 if f == 0 else f - (counts[-1] - 1) * T)
    cu = np.zeros(len(frames) + 1, np.int32)
    cu[1:] = np.cumsum(counts)
    frame0 = np.zeros(len(frames) + 1, np.int64)
    frame0[1:] = np.cumsum(frames)
    return counts, tails, cu, frame0


def _videos_tail(what: str, engines, x, tokens: bool, frame_counts, T: int, q: torch.Tensor, projs, u, new_doc: bool):
    """infv_ltm_videos_tail over frame tokens (``tokens``) or frame means, ``x`` packed by frame."""
    if isinstance(x, (list, tuple)):
        if frame_counts is None:
            frame_counts = [int(t.shape[0]) for t in x]
        x = torch.cat(list(x)) if len(x) else x
    counts, tails, cu, frame0 = split_frames(frame_counts, T)
    engines, cu = _video_engines(engines, counts, what)
    if isinstance(u, (list, tuple)):
        u = torch.cat(list(u))
    V, e0 = len(engines), engines[0]
    total, n_frames = int(cu[-1]), int(frame0[-1])
    if tokens:
        if token_code(x.dtype) is None:
            raise TypeError(f"frame tokens must be float32, float16, bfloat16 or float8_e4m3fn, got {x.dtype}")
        if x.dtype == torch.float16 and not all(e.fp16_tokens for e in engines):
            raise TypeError("float16 frame tokens need engines created with fp16_tokens=True")
        _check_dev(x, e0.device, "k", x.dtype)
        if x.dim() != 3 or tuple(x.shape) != (n_frames, e0.P, e0.d):
            raise ValueError(f"k must be [{n_frames}, {e0.P}, {e0.d}] (packed by frame), got {tuple(x.shape)}")
    else:
        _check_dev(x, e0.device, "kbar")
        if x.dim() != 2 or tuple(x.shape) != (n_frames, e0.d):
            raise ValueError(f"kbar must be fp32 [{n_frames}, {e0.d}] (packed by frame), got {tuple(x.shape)}")
        if x.data_ptr() % 16:
            raise ValueError("kbar must start at a 16-byte boundary (the frames are copied as float4)")
    if q.dim() == 4 and not tokens:
        _check_dev(q, e0.device, "q")
        if q.shape[0] != total or q.shape[1] != e0.L or q.shape[3] != e0.dm or q.shape[2] > e0.max_q:
            raise ValueError(f"q must be [{e0.L}, Q, {e0.dm}] or [{total}, {e0.L}, Q <= {e0.max_q}, {e0.dm}], got {tuple(q.shape)}")
        Q, per_chunk = int(q.shape[2]), 1
    else:
        Q, per_chunk = e0._check_q(q), 0
    e0._check_u(u, (total,))
    for v, e in enumerate(engines):
        if tokens:
            x = e._tokens(x)
        e.ensure_plan(T)
        if counts[v] and tails[v] != T:
            e.ensure_plan(tails[v])
        if not per_chunk:
            e._check_q(q)
    proj_arr = e0._proj_array(projs)
    out = torch.empty(total, e0.L, Q, e0.dm, device=e0.device, dtype=torch.float32)
    hs = (C.c_void_p * V)(*[e._h.value for e in engines])
    tail_T = _np_i32(tails)
    desc = _lib.VideosTailDesc(hs=C.cast(hs, C.c_void_p), V=V, T=int(T), cu=cu.ctypes.data, tail_T=tail_T.ctypes.data,
                               k=_ptr(x) if tokens else None, kbar=None if tokens else _ptr(x), q=_ptr(q), q_per_chunk=per_chunk, Q=Q,
                               proj=C.cast(proj_arr, C.c_void_p), u=_ptr(u), new_doc=int(new_doc), reserved=0, ctx=_ptr(out),
                               hip_stream=_stream(e0.device))
    with torch.cuda.device(e0.device):
        _lib.check(e0.lib.infv_ltm_videos_tail(C.byref(desc)))
    return out, cu


def consolidate_videos_frames(engines: Sequence[LTMEngine], k, frame_counts, T: int, q: torch.Tensor, projs: Sequence[ProjTensors],
                              u=None, new_doc: bool = True):
    """``consolidate_videos`` for videos cut the way the reference cuts them, ``torch.split(video, T, dim=1)``: video v has
    ``frame_counts[v]`` frames, ``ceil(F_v / T)`` chunks, and a last chunk of ``F_v - (C_v - 1) * T`` frames that steps with the
    plan for its own length (infv_ltm_videos_tail) -- in the same launches as everybody else's chunk of that step.

    ``k`` is PACKED BY FRAME, [sum F_v, P, d] (any token dtype ``consolidate_videos`` takes), or a list of per-video [F_v, P, d]
    tensors (packed with one copy; ``frame_counts`` may then be None).  ``u`` [sum C_v, L, S] and the result stay packed by CHUNK.
    ``q`` [L, Q, dm] and ``projs`` are shared.  A video with ``F_v % T == 1`` raises ``ValueError``: a chunk of one frame has an
    empty operator.  Returns ``(ctx [sum C_v, L, Q, dm], cu)`` with ``cu`` the int32 running sum of the chunk counts.  Per video
    the bits are those of ``consolidate_videos`` on its full chunks followed by ``consolidate_videos(new_doc=False)`` on its last
    chunk at that chunk's length; ``trace_videos`` over the chunk counts records the call like any lockstep call."""
    return _videos_tail("consolidate_videos_frames", engines, k, True, frame_counts, T, q, projs, u, new_doc)


def steps_videos_frames(engines: Sequence[LTMEngine], kbar, frame_counts, T: int, q: torch.Tensor, projs: Sequence[ProjTensors],
                        u=None, new_doc: bool = True):
    """``consolidate_videos_frames`` from frame means, with an optional query per chunk: ``kbar`` is PACKED BY FRAME
    [sum F_v, d] fp32 (or a list of per-video [F_v, d] tensors), ``q`` [L, Q, dm] or [sum C_v, L, Q, dm] as ``steps_videos`` takes
    it.  Returns ``(ctx, cu)``.  Per video the bits are those of ``steps_videos`` on its full chunks followed by
    ``steps_videos(new_doc=False)`` on its last chunk; with a shared query and kbar = pool(k), those of the token form."""
    return _videos_tail("steps_videos_frames", engines, kbar, False, frame_counts, T, q, projs, u, new_doc)


class VideosTrace:
    """The packed traces of the lockstep calls, as ``trace_videos`` armed them: ``bins`` [total, L, S] int32 (-1 where nothing
    drew: a video's first chunk), ``probs`` [total, L, 128] and ``mass`` [total, L, N] fp32 (NaN where nothing wrote; ``None``
    without ``masses``), row ``cu[v] + i`` being chunk i of video v.  The object keeps the buffers alive while the library
    writes them; ``stop()`` clears every trace it set."""

    def __init__(self, engines, cu, bins, probs, mass_buf):
        self.engines, self.cu = engines, cu
        self.bins, self.probs, self._mass_buf = bins, probs, mass_buf
        self.mass = None if mass_buf is None else mass_buf[..., :engines[0].N]

    def stop(self):
        for e in self.engines:
            _lib.check(e.lib.infv_ltm_set_trace(e._h, None, None, 0))
            e._trace = None
        e0 = self.engines[0]
        _lib.check(e0.lib.infv_ltm_set_videos_mass_trace(e0._h, None, 0))
        e0._videos_mass_trace = None


def trace_videos(engines: Sequence[LTMEngine], chunk_counts, masses: bool = True) -> VideosTrace:
    """Record the draws and the box masses of the following lockstep calls (``consolidate_videos`` / ``steps_videos``, and the
    batched encoders that run on them) over ``engines`` with these ``chunk_counts``, PACKED as those calls pack ctx.

    The draw trace is per handle and indexed by the call's step, so engine v is armed (infv_ltm_set_trace) with its own slice
    ``[cu[v], cu[v+1])`` of one packed tensor; the masses are the call-level trace of the lead engine
    (infv_ltm_set_videos_mass_trace on ``engines[0]``), one launch more per lockstep step.  Returns a ``VideosTrace``; its
    ``bins`` and ``mass`` are what ``source_weights_videos`` takes.  Call ``.stop()`` when done."""
    engines, cu = _video_engines(engines, chunk_counts, "trace_videos")
    e0 = engines[0]
    total = int(cu[-1])
    if total < 1:
        raise ValueError("trace_videos needs at least one chunk")
    bins = torch.full((total, e0.L, e0.S), -1, device=e0.device, dtype=torch.int32)
    probs = torch.zeros(total, e0.L, NB_BINS, device=e0.device, dtype=torch.float32)
    mass_buf = torch.full((total, e0.L, e0.Np), float("nan"), device=e0.device, dtype=torch.float32) if masses else None
    tr = VideosTrace(engines, cu, bins, probs, mass_buf)
    for v, e in enumerate(engines):
        n = int(cu[v + 1] - cu[v])
        if n:
            _lib.check(e.lib.infv_ltm_set_trace(e._h, _ptr(bins[cu[v]:]), _ptr(probs[cu[v]:]), n))
            e._trace = (bins, probs)
        else:
            _lib.check(e.lib.infv_ltm_set_trace(e._h, None, None, 0))
            e._trace = None
    if masses:
        _lib.check(e0.lib.infv_ltm_set_videos_mass_trace(e0._h, _ptr(mass_buf), total))
        e0._videos_mass_trace = mass_buf
    return tr


def source_weights_videos(engine: LTMEngine, chunk_counts, T: int, bins: Optional[torch.Tensor], mass: Optional[torch.Tensor] = None,
                          frames_per_source: Optional[int] = None, normalise: bool = False):
    """Trace the memories of V videos back to their frames in ONE launch per 512 videos (infv_ltm_source_weights_videos;
    ``density.source_weights_videos`` is its numpy mirror).  ``bins`` [total, L, S] and ``mass`` [total, L, N] are PACKED as
    ``trace_videos`` records them; every video is a new document.  Returns ``W`` [V, L, N, M_max] with
    ``M_max = max_v C_v * T / g`` (video v's columns at and beyond ``C_v * T / g`` are 0) and, with ``mass``, ``attn``
    [total, L, M_max] -- raw, or every row divided by its sum with ``normalise``.  ``engine`` supplies only the plan for T; an
    engine that is not sticky takes ``bins=None``.
    Like ``LTMEngine.source_weights`` this wrapper reads a counter of out-of-range bins back: a HOST SYNC.  Any such bin (an
    unwritten trace row holds -1) raises ``ValueError``."""
    counts = [int(c) for c in (chunk_counts.tolist() if isinstance(chunk_counts, torch.Tensor) else chunk_counts)]
    if not counts or any(c < 0 for c in counts) or sum(counts) < 1:
        raise ValueError("chunk_counts must be non-negative with at least one chunk")
    V, total = len(counts), sum(counts)
    cu = np.zeros(V + 1, np.int32)
    cu[1:] = np.cumsum(counts)
    g = int(T if frames_per_source is None else frames_per_source)
    if g < 1 or T % g:
        raise ValueError("frames_per_source must be >= 1 and divide T")
    e = engine
    e.ensure_plan(T)
    if e.sticky:
        if bins is None or tuple(bins.shape) != (total, e.L, e.S):
            raise ValueError(f"a sticky engine needs bins [{total}, {e.L}, {e.S}]")
        _check_dev(bins, e.device, "bins", torch.int32)
        bins = bins.contiguous()
    else:
        bins = None
    if mass is not None:
        if tuple(mass.shape) != (total, e.L, e.N):
            raise ValueError(f"mass must be [{total}, {e.L}, {e.N}]")
        if e.Np != e.N:
            mass = torch.nn.functional.pad(mass, (0, e.Np - e.N))
        mass = mass.contiguous()
        _check_dev(mass, e.device, "mass")
    M = max(counts) * (T // g)
    ld = (M + 3) // 4 * 4
    buf = torch.zeros(V, e.L, e.Np, ld, device=e.device, dtype=torch.float32)
    attn = torch.zeros(total, e.L, ld, device=e.device, dtype=torch.float32) if mass is not None else None
    bad = torch.zeros(e.L, device=e.device, dtype=torch.int32)
    desc = _lib.SourcesVideosDesc(n_videos=V, T=int(T), frames_per_source=g, reserved=0, ld=ld, cu=cu.ctypes.data,
                                  bins_all=_ptr(bins), W_all=_ptr(buf), mass_all=_ptr(mass), attn_all=_ptr(attn), bad_bins=_ptr(bad),
                                  hip_stream=_stream(e.device))
    with torch.cuda.device(e.device):
        _lib.check(e.lib.infv_ltm_source_weights_videos(e._h, C.byref(desc)))
    n_bad = bad.cpu()                                      # (the host sync)
    if int(n_bad.sum()):
        raise ValueError(f"bins outside [0, {NB_BINS - 1}) per layer: {n_bad.tolist()} (an unwritten trace row holds -1)")
    Wout = buf[:, :, :e.N, :M]
    if attn is None:
        return Wout
    attn = attn[:, :, :M]
    if normalise:
        attn = attn / attn.sum(-1, keepdim=True)
    return Wout, attn
