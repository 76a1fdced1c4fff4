"""The per-frame image Q-former of Video-LLaMA on the HIP path: the producer of the frame tokens.

``InfinityQA.encode_short_memory_frame`` (infty-Video-LLaMA/InfVideoLLaMA/models/infinityqa.py:251-278) runs
``ln_vision(visual_encoder(frames))`` -- a tensor ``[T, 257, 1408]`` -- through the image Q-former (blip2.py:47-65: bert-base, 12
layers, 32 query tokens, a cross-attention in every second layer, ``encoder_width`` 1408) and fills ``short_memory_buffer`` from the
result.  The Q-former is called without ``position_embedding_ext``, so none of its ``LongTermAttention`` modules runs whatever
``alpha`` is (Qformer.py:216, :303).

:class:`FrameQformerEncoder` carries that Q-former's parameters under the reference's names and runs it in ONE C call
(``infv_vqf_encode_frames``): the vision encoder's raw output is read in place in its own dtype, ``ln_vision`` is applied while the
tokens are read, the 257 tokens of a frame go through planes padded to 320, and the last layer writes the frame tokens in the dtype
the video Q-former reads them in -- straight into a :class:`ShortMemoryBuffer` (:meth:`encode_short_memory_frame`).  No CPU or
eager-PyTorch fallback exists.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .basis_maps import NB_SAMPLES
from .engine import aligned_tokens, token_code
from .video_qformer import ShortMemoryBuffer, _dev_f32
from .videochat2_qformer import _Cfg, _Intermediate, _Output, _SelfOutput

OUT_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}       # out_dtype codes of infv_vqf_encode_frames
LINEAR_PRECISIONS = {"fp32": 0, "split_bf16": 1, "fp16": 2}                # mode codes of infv_vqf_set_linear_precision
ATTENTION_PRECISIONS = {"fp32": 0, "fp16": 1}                              # mode codes of infv_vqf_set_attention_precision


def _linear_precision_code(name) -> int:
    if not isinstance(name, str) or name not in LINEAR_PRECISIONS:
        raise ValueError(f"linear_precision must be one of {sorted(LINEAR_PRECISIONS)}, got {name!r}")
    return LINEAR_PRECISIONS[name]


def _attention_precision_code(name) -> int:
    if not isinstance(name, str) or name not in ATTENTION_PRECISIONS:
        raise ValueError(f"attention_precision must be one of {sorted(ATTENTION_PRECISIONS)}, got {name!r}")
    return ATTENTION_PRECISIONS[name]


class _SelfAttention(nn.Module):                       # Qformer.py:115-175 without the LongTermAttention (never called here)
    def __init__(self, cfg, is_cross_attention: bool):
        super().__init__()
        self.query = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        kv_in = cfg.encoder_width if is_cross_attention else cfg.hidden_size
        self.key = nn.Linear(kv_in, cfg.hidden_size)
        self.value = nn.Linear(kv_in, cfg.hidden_size)


class _Attention(nn.Module):                           # Qformer.py:327-332
    def __init__(self, cfg, is_cross_attention=False):
        super().__init__()
        self.self = _SelfAttention(cfg, is_cross_attention)
        self.output = _SelfOutput(cfg)


class _Layer(nn.Module):                               # Qformer.py:419-441; the text FFN is never used (no text rows) and not kept
    def __init__(self, cfg, layer_num):
        super().__init__()
        self.layer_num = layer_num
        self.attention = _Attention(cfg)
        self.has_cross_attention = layer_num % cfg.cross_attention_freq == 0
        if self.has_cross_attention:
            self.crossattention = _Attention(cfg, is_cross_attention=True)
        self.intermediate_query = _Intermediate(cfg)
        self.output_query = _Output(cfg)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg, i) for i in range(cfg.num_hidden_layers)])


class _Embeddings(nn.Module):                          # Qformer.py:55-113 with query_embeds alone: the LayerNorm (dropout: eval)
    def __init__(self, cfg):
        super().__init__()
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Bert(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)


class _Qformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.bert = _Bert(cfg)


def _droppable(key: str) -> bool:
    """Checkpoint keys of the model's image Q-former that ``encode_short_memory_frame`` never uses."""
    if key.startswith("Qformer.cls."):
        return True
    if key in ("Qformer.bert.embeddings.word_embeddings.weight", "Qformer.bert.embeddings.position_embeddings.weight",
               "Qformer.bert.embeddings.position_ids"):
        return True
    if key.startswith("Qformer.bert.encoder.layer."):
        rest = key[len("Qformer.bert.encoder.layer."):].split(".", 1)
        if len(rest) == 2 and rest[0].isdigit():
            tail = rest[1]
            # the text FFN (Qformer.py:431-432), and the LongTermAttention's own tensors (not called: position_embedding_ext is None)
            return tail.startswith("intermediate.") or tail.startswith("output.") or ".long_term_attention." in tail
    return False


class FrameQformerEncoder(nn.Module):
    """``self.Qformer`` / ``self.query_tokens`` / ``self.ln_vision`` of the reference model (blip2.py:47-65, infinityqa.py:104-118),
    and ``encode_short_memory_frame``'s body after the vision encoder."""

    def __init__(self, num_query_token: int = 32, vision_width: int = 1408, num_hidden_layers: int = 12,
                 cross_attention_freq: int = 2, vision_layernorm: bool = True, ln_eps: float = 1e-5, hidden_size: int = 768,
                 intermediate_size: int = 3072, num_attention_heads: int = 12, linear_precision: str = "fp32",
                 attention_precision: str = "fp32"):
        super().__init__()
        _linear_precision_code(linear_precision)
        _attention_precision_code(attention_precision)
        self.linear_precision = linear_precision
        self.attention_precision = attention_precision
        cfg = _Cfg(encoder_width=vision_width, num_hidden_layers=num_hidden_layers, cross_attention_freq=cross_attention_freq,
                   query_length=num_query_token, hidden_size=hidden_size, intermediate_size=intermediate_size,
                   num_attention_heads=num_attention_heads, alpha=1.0)
        self.n_query = int(num_query_token)
        self.Qformer = _Qformer(cfg)
        self.query_tokens = nn.Parameter(torch.zeros(1, num_query_token, hidden_size))
        nn.init.normal_(self.query_tokens, mean=0.0, std=0.02)
        if vision_layernorm:                              # blip2.py:83 (nn.LayerNorm's default eps)
            self.ln_vision = nn.LayerNorm(vision_width, eps=ln_eps)
        self._vqf = None                                  # (handle, device)
        self._vqf_state = None                            # (linear precision, weights epoch) the handle was last given
        self._plane_gen = 0                               # bumped by set_linear_precision: part of the weights epoch
        self._w_cache = None
        self._q_cache = None

    @property
    def config(self):
        return self.Qformer.config

    # ------------------------------------------------------------------ weights
    def load_reference_state_dict(self, sd: dict, strict: bool = True):
        """``sd`` under the model's own checkpoint keys: ``Qformer.bert.encoder.layer.N...``, ``Qformer.bert.embeddings.LayerNorm.*``,
        ``query_tokens``, ``ln_vision.*``.  What the image Q-former never uses is dropped: ``Qformer.cls.*``, the word / position
        embeddings and ``position_ids``, the text FFN ``intermediate`` / ``output`` of every layer.  Under ``strict`` any other
        unknown key, and any key of the module that ``sd`` lacks, raises KeyError; a tensor of another shape always raises
        ValueError."""
        own = {k: torch.as_tensor(v) for k, v in sd.items() if not _droppable(k)}
        mine = self.state_dict()
        for k, v in own.items():
            if k in mine and tuple(v.shape) != tuple(mine[k].shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} in the state dict, {tuple(mine[k].shape)} in the module")
        res = self.load_state_dict(own, strict=False)
        if strict and (res.missing_keys or res.unexpected_keys):
            raise KeyError(f"state dict mismatch: missing {res.missing_keys}, unexpected {res.unexpected_keys}")
        return res

    def set_linear_precision(self, name: str) -> None:
        """The arithmetic of the query-side linears (``infv_vqf_set_linear_precision``): ``"fp32"`` (default), ``"split_bf16"``
        (three bf16 MFMA products on hi / lo pieces, fp32-class) or ``"fp16"`` (operands rounded to fp16, fp32 accumulation: what the
        reference's fp16 autocast computes).  Applied to this encoder's own handle at the next call; the weight planes of the reduced
        modes are cached in the handle until a parameter moves or changes in place.  A write through ``p.data`` does not bump
        ``p._version`` and is therefore not seen: after one, call this method again (every call starts a new set of planes)."""
        _linear_precision_code(name)
        self.linear_precision = name
        self._plane_gen = getattr(self, "_plane_gen", 0) + 1

    def set_attention_precision(self, name: str) -> None:
        """The arithmetic of the cross-attention (``infv_vqf_set_attention_precision``): ``"fp32"`` (default: the split-bf16
        contractions, fp32-class) or ``"fp16"`` (tokens, pre-multiplied query, probabilities and context rounded to fp16, fp32
        accumulation: what the reference's fp16 autocast computes; values beyond fp16's range become inf).  Independent of
        :meth:`set_linear_precision`.  Applied at the next call; the fp16 key / value weight planes live in the handle's plane cache
        and follow its rules."""
        _attention_precision_code(name)
        self.attention_precision = name
        self._plane_gen = getattr(self, "_plane_gen", 0) + 1

    def _weights(self, device):
        """ctypes view of the parameters (``infv_vqf_vc_weights``; the text FFN members stay NULL, they are never read), rebuilt only
        when a parameter moved or changed in place."""
        src = list(self.parameters())
        sig = (str(device),) + tuple((p.data_ptr(), p._version, p.dtype) for p in src)
        if self._w_cache is not None and self._w_cache[0] == sig:
            return self._w_cache[1], self._w_cache[2]
        keep = []

        def t(x):
            y = _dev_f32(x, device)
            keep.append(y)
            return y.data_ptr()

        lin = lambda m: _lib.Linear(t(m.weight), t(m.bias))
        ln = lambda m: _lib.LayerNorm(t(m.weight), t(m.bias))
        none_l, none_n = _lib.Linear(None, None), _lib.LayerNorm(None, None)
        layers = self.Qformer.bert.encoder.layer
        arr = (_lib.VqfVcLayer * len(layers))()
        for i, layer in enumerate(layers):
            a = layer.attention
            x = layer.crossattention if layer.has_cross_attention else None
            arr[i] = _lib.VqfVcLayer(
                lin(a.self.query), lin(a.self.key), lin(a.self.value), lin(a.output.dense), ln(a.output.LayerNorm),
                int(x is not None), 0,
                lin(x.self.query) if x else none_l, lin(x.self.key) if x else none_l, lin(x.self.value) if x else none_l,
                lin(x.output.dense) if x else none_l, ln(x.output.LayerNorm) if x else none_n,
                lin(layer.intermediate_query.dense), lin(layer.output_query.dense), ln(layer.output_query.LayerNorm),
                none_l, none_l, none_n)
        w = _lib.VqfVcWeights(len(layers), 0, arr, none_l)
        vis = _lib.VqfVisionLn(None, None, 0.0)
        if hasattr(self, "ln_vision"):
            vis = _lib.VqfVisionLn(t(self.ln_vision.weight), t(self.ln_vision.bias), float(self.ln_vision.eps))
        keep.append(arr)
        self._w_cache = (sig, (w, vis), keep)
        return (w, vis), keep

    def query_rows(self, device) -> torch.Tensor:
        """``Qformer.bert.embeddings(query_embeds=query_tokens)`` in eval mode (Qformer.py:108-112): the embeddings LayerNorm of the
        query tokens, [n_query, hidden] fp32 on ``device`` -- the rows every frame starts from.  Cached on the storage address and
        in-place version of the three parameters it reads."""
        emb = self.Qformer.bert.embeddings.LayerNorm
        sig = (str(device),) + tuple((p.data_ptr(), p._version) for p in (self.query_tokens, emb.weight, emb.bias))
        if self._q_cache is not None and self._q_cache[0] == sig:
            return self._q_cache[1]
        with torch.no_grad():
            q = _dev_f32(self.query_tokens, device)[0]
            rows = F.layer_norm(q, (q.size(-1),), _dev_f32(emb.weight, device), _dev_f32(emb.bias, device), emb.eps).contiguous()
        self._q_cache = (sig, rows)
        return rows

    # ------------------------------------------------------------------ handle
    def _handle(self, device):
        if self._vqf is not None and self._vqf[1] == device:
            return self._vqf[0]
        self._release()
        cfg = self.config
        # (tokens_per_frame, alpha and proj_out of the handle are not read by infv_vqf_encode_frames)
        c = _lib.VqfConfig(1, cfg.num_attention_heads, cfg.hidden_size, cfg.intermediate_size, cfg.encoder_width, 1, self.n_query, 0,
                           NB_SAMPLES, 1.0, float(cfg.layer_norm_eps))
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_create(C.byref(c), C.byref(h)))
        self._vqf = (h, device)
        self._vqf_state = None
        return h

    def _apply_linear_precision(self, h, device) -> None:
        """The mode, and the weights epoch the handle's plane cache lives by: the signature ``_weights`` computes (storage address,
        in-place version and dtype of every parameter), so an in-place update or ``load_state_dict`` invalidates the planes."""
        mode = LINEAR_PRECISIONS[self.linear_precision]
        attn = ATTENTION_PRECISIONS[getattr(self, "attention_precision", "fp32")]
        epoch = (hash((self._w_cache[0], getattr(self, "_plane_gen", 0))) & 0x7FFFFFFFFFFFFFFF) | 1 if mode or attn else 0
        if self._vqf_state == (mode, attn, epoch):
            return
        lib = _lib.load()
        with torch.cuda.device(device):
            _lib.check(lib.infv_vqf_set_linear_precision(h, mode))
            _lib.check(lib.infv_vqf_set_attention_precision(h, attn))
            _lib.check(lib.infv_vqf_set_weights_epoch(h, C.c_uint64(epoch)))
        self._vqf_state = (mode, attn, epoch)

    def _release(self):
        vqf, self._vqf = getattr(self, "_vqf", None), None
        if vqf:
            try:
                _lib.load().infv_vqf_destroy(vqf[0])
            except Exception:
                pass

    def __del__(self):
        self._release()

    # ------------------------------------------------------------------ the image Q-former over F frames
    def encode_frames(self, vision_out: torch.Tensor, out_dtype=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Qformer.bert(query_embeds=query_tokens, encoder_hidden_states=ln_vision(vision_out)).last_hidden_state`` for F frames
        in one C call (``infv_vqf_encode_frames``).

        ``vision_out`` [F, n_tok, width]: the vision encoder's output BEFORE ``ln_vision`` (a model built with
        ``vision_layernorm=False`` takes the normalised tokens), fp32, fp16 or bf16, read in place (cloned only where it is not
        contiguous or not 16-byte aligned); float64 goes in as fp32; ``torch.float8_e4m3fn`` is read in place too, but only without
        the LayerNorm.  ``n_tok`` is any positive count.  ``out_dtype``: float32 (default), float16 or bfloat16 -- the 2-byte
        types are the bits of ``(fp32 result).to(dtype)``, written by the last layer's epilogue.  ``out``: a contiguous
        [F, n_query, hidden] tensor of that type on the device, written in place and returned.  A frame's result does not depend on
        the other frames of the call (bit for bit)."""
        cfg = self.config
        if vision_out.dim() != 3 or vision_out.size(2) != cfg.encoder_width or vision_out.size(1) < 1:
            raise ValueError(f"vision_out must be [F, n_tok >= 1, {cfg.encoder_width}], got {tuple(vision_out.shape)}")
        if not vision_out.is_cuda:
            raise RuntimeError("the frame Q-former runs on the HIP device only (no CPU fallback)")
        device = vision_out.device
        with_ln = hasattr(self, "ln_vision")
        code = token_code(vision_out.dtype)                   # (an fp8 encoding other than e4m3fn raises TypeError there)
        if code == 4 and with_ln:
            raise ValueError("fp8 vision tokens are read only without the vision LayerNorm (build with vision_layernorm=False)")
        x = aligned_tokens(vision_out.detach()) if code is not None else _dev_f32(vision_out, device)
        if code is None:
            x, code = aligned_tokens(x), 0
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in OUT_DTYPES:
            raise TypeError(f"out_dtype must be float32, float16 or bfloat16 (the library does not quantise), got {out_dtype}")
        n_f, Q, Hd = int(x.size(0)), self.n_query, cfg.hidden_size
        if out is None:
            out = torch.empty(n_f, Q, Hd, device=device, dtype=out_dtype)
        else:
            if tuple(out.shape) != (n_f, Q, Hd) or out.dtype != out_dtype or out.device != device or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous [{n_f}, {Q}, {Hd}] {out_dtype} tensor on {device}")
            if out.data_ptr() % 16:
                raise ValueError("out must be 16-byte aligned")
        if n_f == 0:
            return out
        (w, vis), keep = self._weights(device)
        rows = self.query_rows(device)
        h = self._handle(device)
        self._apply_linear_precision(h, device)
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_encode_frames(
                h, n_f, C.c_void_p(x.data_ptr()), code, int(x.size(1)), C.byref(w),
                C.byref(vis) if with_ln else None, C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()), OUT_DTYPES[out_dtype],
                C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        del keep
        return out

    @staticmethod
    def kept_frames(n_frames: int, n_frame: int = 2048) -> int:
        """Frames ``encode_short_memory_frame`` keeps of ``n_frames``: those with ``cur_frame <= n_frame`` (infinityqa.py:275-277)."""
        return min(int(n_frames), int(n_frame) + 1)

    def encode_short_memory_frame(self, vision_out: torch.Tensor, buffer: ShortMemoryBuffer, n_frame: int = 2048) -> ShortMemoryBuffer:
        """The body of ``InfinityQA.encode_short_memory_frame`` after the vision encoder (infinityqa.py:259-278): only the frames
        with ``cur_frame <= n_frame`` are encoded, and their tokens are written directly into ``buffer.store`` in the buffer's dtype
        (an fp8 buffer goes through ``buffer.replace`` on the fp32 result: the library does not quantise)."""
        cfg = self.config
        if (buffer.P, buffer.d) != (self.n_query, cfg.hidden_size):
            raise ValueError(f"the buffer holds [{buffer.P}, {buffer.d}] frames, the Q-former writes [{self.n_query}, {cfg.hidden_size}]")
        if vision_out.dim() != 3:
            raise ValueError(f"vision_out must be [F, n_tok, {cfg.encoder_width}], got {tuple(vision_out.shape)}")
        keep = self.kept_frames(vision_out.size(0), n_frame)
        if keep > buffer.store.size(0):
            raise ValueError(f"{keep} frames exceed the buffer's capacity of {buffer.store.size(0)}")
        if buffer.store.dtype not in OUT_DTYPES:
            return buffer.replace(self.encode_frames(vision_out[:keep]), n_frame)
        self.encode_frames(vision_out[:keep], out_dtype=buffer.store.dtype, out=buffer.store[:keep])
        buffer.n = keep
        return buffer
