"""VideoChat2 binding of the LTM path (BASELINE configs[4]).

The VideoChat2 Q-former (infty-VideoChat2/models/blip2/Qformer.py) is a 12-layer bert-base encoder with a
cross-attention in every second layer (``cross_attention_freq = 2``, blip2.py:62): six ``LongTermAttention``
instances, the hook fires on every cross-attention (no ``position_embedding_ext`` test, Qformer.py:215-222) with
``sigmas = 1``; frames are 14x14 UMT-L patches of width 1024 (blip2/long_term_attention_gibbs.py:291,304); the
cross-attention query is the 96 query tokens (32 + 64 extra, configs/config_mistral.json), the instruction's text
tokens only ride along in the self-attention and have their own FFN (Qformer.py:473-505).

What runs where (the hook, the merge and the op are the path; "rest of BERT stays
stock PyTorch-ROCm"):

* HIP, through the C ABI -- per cross-attention layer: the LTM operator (``LongTermAttentionVC`` ->
  ``infv_ltm_forward``; the six layers share ONE pooled copy of the chunk's frames), the short-term cross-attention
  over the chunk's ``T*196`` tokens re-associated around the frame tokens, and the merge
  ``alpha * short + (1 - alpha) * long`` fused into its epilogue (``infv_vqf_short_attention``);
* stock PyTorch on the same device -- the BERT scaffolding around it: self-attention over the 96 + text tokens, the
  attention output blocks, the two FFNs.

``VideoChat2Encoder.encode_tokens`` is the counterpart of ``encode_img`` after the vision encoder
(videochat2_it_mistral.py:196-252), ``encode_long_video_vc`` that of the eval loop ``infer_*_inf``
(eval_code/run_nextqa_mistral.py:141-152).  Parameters live under the reference's state-dict names.

``VideoChat2Encoder.encode_videos`` / ``encode_long_videos_vc`` are the batched counterparts for harnesses that walk many
short videos: ONE C call (``infv_vqf_vc_encode_videos``) runs the whole encoder -- BERT scaffolding included -- layer-major
over the packed chunks of every video, each video's six memories in its own :class:`VideoChat2Memory`.

``VideoChat2Encoder.encode_img_videos`` starts two steps earlier in ``encode_img``: at the vision encoder's output before
``vision_layernorm`` (videochat2_it_mistral.py:195), in its own dtype, and at the tokenizer's ids (:204-223, Qformer.py:54-111).
``infv_vqf_vc_encode_img`` applies the LayerNorm while the tokens are read and runs the embedding layer on the device; the model
carries ``vision_layernorm`` and ``qformer.bert.embeddings`` when built with ``vision_layernorm=True`` / ``vocab_size=...``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .basis_maps import NB_SAMPLES
from .qformer_hook import LongTermMemoryHook
from .engine import token_code
from .video_qformer import TOKEN_DTYPES, VideoMemory, _cumsum, _dev_f32, draw_video_uniforms

MAX_TXT_LEN = 512              # max_txt_len of the instruction (configs/config_mistral.json)


class _Cfg:
    """The BertConfig attributes Blip2Base.init_Qformer sets (blip2.py:54-66) plus bert-base defaults."""

    def __init__(self, **kw):
        self.hidden_size = 768
        self.num_attention_heads = 12
        self.intermediate_size = 3072
        self.layer_norm_eps = 1e-12
        self.num_hidden_layers = 12
        self.add_cross_attention = True
        self.cross_attention_freq = 2
        self.sigmas = 1
        self.__dict__.update(kw)


class _SelfOutput(nn.Module):                         # Qformer.py:313-324
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dense(hidden_states) + input_tensor)


class _SelfAttention(nn.Module):                      # Qformer.py:115-175
    def __init__(self, cfg, is_cross_attention: bool):
        super().__init__()
        self.is_cross_attention = is_cross_attention
        self.H = cfg.num_attention_heads
        self.dh = cfg.hidden_size // cfg.num_attention_heads
        self.query = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        kv_in = cfg.encoder_width if is_cross_attention else cfg.hidden_size
        self.key = nn.Linear(kv_in, cfg.hidden_size)
        self.value = nn.Linear(kv_in, cfg.hidden_size)
        if is_cross_attention:
            # construction, call and merge rules of Qformer.py:135-159,215-222,302-303 (VideoChat2 variant)
            hook = LongTermMemoryHook(cfg, self.key, self.value, self.H, self.dh, variant="VC")
            object.__setattr__(self, "_hook", hook)           # keep the state-dict names of the reference:
            self.long_term_attention = hook.long_term_attention   # ...crossattention.self.long_term_attention

    def self_attention(self, hidden_states):              # Qformer.py:232-300 with all-ones masks, eval mode
        n = hidden_states.size(1)
        split = lambda x: x.view(1, n, self.H, self.dh).permute(0, 2, 1, 3)
        q, k, v = split(self.query(hidden_states)), split(self.key(hidden_states)), split(self.value(hidden_states))
        probs = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(self.dh), dim=-1)
        return torch.matmul(probs, v).permute(0, 2, 1, 3).reshape(1, n, self.H * self.dh)


class _Attention(nn.Module):                          # Qformer.py:327-332
    def __init__(self, cfg, is_cross_attention=False):
        super().__init__()
        self.self = _SelfAttention(cfg, is_cross_attention)
        self.output = _SelfOutput(cfg)


class _Intermediate(nn.Module):                       # Qformer.py:387-401
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)

    def forward(self, x):
        return F.gelu(self.dense(x))


class _Output(nn.Module):                             # Qformer.py:404-416
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dense(hidden_states) + input_tensor)


class _Layer(nn.Module):                              # Qformer.py:419-441
    def __init__(self, cfg, layer_num):
        super().__init__()
        self.layer_num = layer_num
        self.attention = _Attention(cfg)
        self.has_cross_attention = cfg.add_cross_attention and layer_num % cfg.cross_attention_freq == 0
        if self.has_cross_attention:
            self.crossattention = _Attention(cfg, is_cross_attention=True)
        self.intermediate = _Intermediate(cfg)
        self.output = _Output(cfg)
        self.intermediate_query = _Intermediate(cfg)
        self.output_query = _Output(cfg)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg, i) for i in range(cfg.num_hidden_layers)])


class _Embeddings(nn.Module):                          # Qformer.py:54-111 (parameters only: the forward is the HIP kernel)
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Bert(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        if getattr(cfg, "vocab_size", None) is not None:      # opt-in: older state dicts carry no bert.embeddings.*
            self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)


class VideoChat2Qformer(nn.Module):
    """``self.qformer`` of VideoChat2_it_mistral with ``cls = None`` (videochat2_it_mistral.py:64-80): ``.bert.encoder``."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.bert = _Bert(cfg)

    @property
    def cross_layers(self) -> List[_Layer]:
        return [l for l in self.bert.encoder.layer if l.has_cross_attention]

    @property
    def ltm_modules(self):
        return [l.crossattention.self.long_term_attention for l in self.cross_layers]


def init_Qformer(num_query_token: int, vision_width: int, tau: float, alpha: float, sticky: bool, num_basis: int,
                 num_hidden_layers: int = 12, cross_attention_freq: int = 2, hidden_size: int = 768,
                 intermediate_size: int = 3072, num_attention_heads: int = 12, vocab_size: Optional[int] = None,
                 max_position_embeddings: int = 512):
    """Counterpart of ``Blip2Base.init_Qformer`` (blip2.py:47-77): (Q-former, query tokens).  The three arguments after
    ``cross_attention_freq`` default to bert-base; tests build small shapes with them.  ``vocab_size`` creates
    ``bert.embeddings`` (Qformer.py:54-111)."""
    cfg = _Cfg(vocab_size=vocab_size, max_position_embeddings=max_position_embeddings,
               encoder_width=vision_width, sticky=sticky, num_basis=num_basis, tau=tau, alpha=alpha,
               cross_attention_freq=cross_attention_freq, query_length=num_query_token,
               num_hidden_layers=num_hidden_layers, hidden_size=hidden_size, intermediate_size=intermediate_size,
               num_attention_heads=num_attention_heads)
    qformer = VideoChat2Qformer(cfg)
    query_tokens = nn.Parameter(torch.zeros(1, num_query_token, cfg.hidden_size))
    nn.init.normal_(query_tokens, mean=0.0, std=0.02)
    return qformer, query_tokens


class VideoChat2Memory(VideoMemory):
    """One video's long-term memories for :meth:`VideoChat2Encoder.encode_videos`: a one-layer ``LTMEngine`` per
    cross-attention layer (six in the model), created as ``LongTermAttentionVC._get_engine`` creates the model's own.
    ``export_state(i)`` / ``last_draw(i)`` read cross layer i's memory.  ``video_id`` names the video's device-rng streams:
    cross layer i draws from stream ``(video_id + 1) * n_cross + i`` (the model's own modules keep stream i).
    Attention read-outs of a batch go around the call as for :class:`VideoMemory`, one packed trace per cross layer:
    ``engine.trace_videos([m.engines[i] for m in memories], counts)`` before ``encode_videos(..., memories=memories)``."""

    def __init__(self, model: "VideoChat2Encoder", device: torch.device, video_id: int = 0):
        from .engine import LTMEngine
        self.device = device
        self.video_id = int(video_id)
        self.engines = [LTMEngine(m.attn_num_basis, m.n_head, m.head_size, m.encoder_width, m.tokens_per_frame, tau=m.tau,
                                  sticky=bool(m.sticky_memories), n_layers=1, max_q=max(model.n_query, 32), device=device,
                                  nb_samples=m.nb_samples)
                        for m in model.qformer.ltm_modules]
        self.set_device_rng(getattr(model, "_device_rng_seed", None))

    def _check(self, model: "VideoChat2Encoder", device: torch.device):
        if len(self.engines) != len(model.qformer.ltm_modules):
            raise ValueError("memory has another number of cross layers than the model")
        if self.device != device:
            raise ValueError(f"memory is on {self.device}, frames are on {device}")


def _check_vc_memories(model: "VideoChat2Encoder", memories, V: int) -> list:
    """Every video its own VideoChat2Memory; refused before any library call."""
    memories = list(memories)
    if len(memories) != V:
        raise ValueError(f"{len(memories)} memories for {V} videos")
    seen = set()
    for i, mem in enumerate(memories):
        if id(mem) in seen:
            raise ValueError(f"memories[{i}] appears twice: every video needs its own memory")
        seen.add(id(mem))
    for i, mem in enumerate(memories):
        if not isinstance(mem, VideoChat2Memory):
            raise TypeError(f"memories[{i}] is not a VideoChat2Memory")
    return memories


def draw_vc_uniforms(counts: Sequence[int], continuing: Sequence[bool], n_cross: int) -> torch.Tensor:
    """Gibbs uniforms [sum C_v, n_cross, 512] float64 from torch's global CPU generator in the order the loop of
    ``encode_tokens`` consumes it: video by video, chunk by chunk, per LTM instance 512 for the bin draw and 512 discarded
    (the in-bin draw); the first chunk of a video that is not ``continuing`` draws nothing (its rows stay 0)."""
    return draw_video_uniforms(counts, continuing, n_cross)


class VideoChat2Encoder(nn.Module):
    """The part of ``VideoChat2_it_mistral`` between the vision encoder and the LLM: Q-former (with the LTM in every
    cross-attention) + ``mistral_proj`` on the query part (videochat2_it_mistral.py:64-69,199-252)."""

    tokens_per_frame = 14 * 14

    def __init__(self, num_query_token: int = 32, extra_num_query_token: int = 64, vision_width: int = 1024,
                 llm_hidden: int = 4096, num_basis: int = 256, sticky: bool = True, tau: float = 0.75,
                 alpha: float = 0.75, num_hidden_layers: int = 12, cross_attention_freq: int = 2, hidden_size: int = 768,
                 intermediate_size: int = 3072, num_attention_heads: int = 12, tokens_per_frame: Optional[int] = None,
                 vocab_size: Optional[int] = None, max_position_embeddings: int = 512, vision_layernorm: bool = False):
        super().__init__()
        self.n_query = num_query_token + extra_num_query_token
        self.qformer, self.query_tokens = init_Qformer(self.n_query, vision_width, tau, alpha, sticky, num_basis,
                                                       num_hidden_layers, cross_attention_freq, hidden_size,
                                                       intermediate_size, num_attention_heads, vocab_size,
                                                       max_position_embeddings)
        if vision_layernorm:                              # blip2.py:88, applied at videochat2_it_mistral.py:195
            self.vision_layernorm = nn.LayerNorm(vision_width, eps=1e-12)
        self.mistral_proj = nn.Linear(self.qformer.config.hidden_size, llm_hidden)
        self._vqf = None
        self._vqf_dev = None
        self._vc = None                                   # handle of the batched path (encode_videos): (handle, device)
        self._vc_memories: List["VideoChat2Memory"] = []  # default pool of encode_videos
        self._device_rng_seed: Optional[int] = None
        if tokens_per_frame is not None:                  # (small test shapes; the model has 14 x 14 patches per frame)
            self.tokens_per_frame = int(tokens_per_frame)
        for m in self.qformer.ltm_modules:                # the memories pool frames of this encoder's shape
            m.tokens_per_frame, m.encoder_width = self.tokens_per_frame, vision_width

    def use_device_rng(self, seed: Optional[int]):
        """Draw the Gibbs uniforms of every cross-attention's memory on the device (``LongTermAttention.use_device_rng``): the
        i-th LTM instance draws from stream ``i``; torch's global generator is left alone.  ``seed=None`` turns it off."""
        for i, m in enumerate(self.qformer.ltm_modules):
            m.use_device_rng(seed, i)
        self._device_rng_seed = None if seed is None else int(seed)

    # ------------------------------------------------------------------ weights
    def load_reference_state_dict(self, sd: dict, strict: bool = True):
        """``sd`` under the reference's names: ``bert.encoder.layer.*``, ``query_tokens`` (query + extra query tokens
        concatenated, videochat2_it_mistral.py:199-203), ``mistral_proj.*``; for a model built with them also
        ``bert.embeddings.*`` (its ``position_ids`` buffer is dropped) and ``vision_layernorm.*``."""
        t = lambda v: torch.as_tensor(v)
        own = {"qformer." + k: t(v) for k, v in sd.items() if k.startswith("bert.") and k != "bert.embeddings.position_ids"}
        own.update({k: t(v) for k, v in sd.items() if k.startswith("vision_layernorm.")})
        own["query_tokens"] = t(sd["query_tokens"])
        for k in ("mistral_proj.weight", "mistral_proj.bias"):
            own[k] = t(sd[k])
        res = self.load_state_dict(own, strict=False)
        if strict:
            bad = [k for k in res.missing_keys if ".long_term_attention.proj_" not in k]   # aliases of key / value (Qformer.py:156-157)
            if bad or res.unexpected_keys:
                raise KeyError(f"state dict mismatch: missing {bad}, unexpected {res.unexpected_keys}")
        return res

    # ------------------------------------------------------------------ HIP short-term cross-attention
    def _short_handle(self, device):
        if self._vqf is not None and self._vqf_dev == device:
            return self._vqf
        self._release()
        cfg = self.qformer.config
        c = _lib.VqfConfig(1, cfg.num_attention_heads, cfg.hidden_size, cfg.intermediate_size, cfg.encoder_width,
                           self.tokens_per_frame, self.n_query, 0, NB_SAMPLES, float(cfg.alpha), float(cfg.layer_norm_eps))
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_create(C.byref(c), C.byref(h)))
        self._vqf, self._vqf_dev = h, device
        return h

    def _release(self):
        h, self._vqf = self._vqf, None
        if h:
            try:
                _lib.load().infv_vqf_destroy(h)
            except Exception:
                pass
        vc, self._vc = getattr(self, "_vc", None), None
        if vc:
            try:
                _lib.load().infv_vqf_destroy(vc[0])
            except Exception:
                pass

    def __del__(self):
        self._release()

    def _cross_attention(self, layer: _Layer, k: torch.Tensor, xq: torch.Tensor, a_long) -> torch.Tensor:
        """merged = alpha * softmax(xq K^T / sqrt(dh)) V + (1 - alpha) * a_long   (Qformer.py:223-303), on the HIP path."""
        att = layer.crossattention.self
        dev = k.device
        if k.size(0) % 32:
            # frame counts that are not a multiple of 8 (196 * T tokens, T % 8 != 0): the HIP contraction tiles the token
            # axis in 32s; the eval loop never produces such chunks (num_segments = max_int * num_samples,
            # run_nextqa_mistral.py:544-547), so they take the stock-PyTorch cross-attention on the same device
            H, dh = att.H, att.dh
            split = lambda x: x.view(1, -1, H, dh).permute(0, 2, 1, 3)
            kk, vv = split(att.key(k.unsqueeze(0))), split(att.value(k.unsqueeze(0)))
            probs = torch.softmax(torch.matmul(split(xq), kk.transpose(-1, -2)) / math.sqrt(dh), dim=-1)
            short = torch.matmul(probs, vv).permute(0, 2, 1, 3).reshape(1, -1, H * dh)
            alpha = self.qformer.config.alpha
            return short if isinstance(a_long, int) else alpha * short + (1 - alpha) * a_long
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        wk, bk, wv, bv = f32(att.key.weight), f32(att.key.bias), f32(att.value.weight), f32(att.value.bias)
        key, val = _lib.Linear(wk.data_ptr(), bk.data_ptr()), _lib.Linear(wv.data_ptr(), bv.data_ptr())
        q = f32(xq[0])
        along = None if isinstance(a_long, int) else f32(a_long[0])
        out = torch.empty(self.n_query, self.qformer.config.hidden_size, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().infv_vqf_short_attention(
                self._short_handle(dev), C.c_void_p(k.data_ptr()), k.size(0), C.c_void_p(q.data_ptr()), C.byref(key),
                C.byref(val), C.c_void_p(0 if along is None else along.data_ptr()), C.c_void_p(out.data_ptr()),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out.unsqueeze(0)

    # ------------------------------------------------------------------ many videos, layer-major, one call
    def _vc_handle(self, device):
        """Handle of the batched path: the short-term handle's shape plus ``mistral_proj``'s width."""
        if self._vc is not None and self._vc[1] == device:
            return self._vc[0]
        if self._vc is not None:
            _lib.load().infv_vqf_destroy(self._vc[0])
            self._vc = None
        cfg = self.qformer.config
        c = _lib.VqfConfig(1, cfg.num_attention_heads, cfg.hidden_size, cfg.intermediate_size, cfg.encoder_width,
                           self.tokens_per_frame, self.n_query, self.mistral_proj.out_features, NB_SAMPLES, float(cfg.alpha),
                           float(cfg.layer_norm_eps))
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_create(C.byref(c), C.byref(h)))
        self._vc = (h, device)
        return h

    def _vc_weights(self, device):
        """ctypes view of the parameters (``infv_vqf_vc_weights``), rebuilt only when a parameter moved or changed in place."""
        layers = self.qformer.bert.encoder.layer
        src = [p for p in self.parameters()]
        sig = (str(device),) + tuple((p.data_ptr(), p._version, p.dtype) for p in src)
        cached = getattr(self, "_vc_w_cache", None)
        if cached is not None and cached[0] == sig:
            return cached[1], cached[2]
        keep = []

        def t(x):
            y = _dev_f32(x, device)
            keep.append(y)
            return y.data_ptr()

        lin = lambda m: _lib.Linear(t(m.weight), t(m.bias))
        ln = lambda m: _lib.LayerNorm(t(m.weight), t(m.bias))
        none_l, none_n = _lib.Linear(None, None), _lib.LayerNorm(None, None)
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
                lin(layer.intermediate.dense), lin(layer.output.dense), ln(layer.output.LayerNorm))
        w = _lib.VqfVcWeights(len(layers), 0, arr, lin(self.mistral_proj))
        keep.append(arr)
        self._vc_w_cache = (sig, w, keep)
        return w, keep

    def _vc_inputs(self, V: int, text_embeds, hidden_in) -> List[torch.Tensor]:
        """Per video the encoder input rows [n_query + n_text_v, hidden] (``encode_tokens``' rule, video by video)."""
        cfg = self.qformer.config

        def per_video(x, what):
            if x is None or isinstance(x, torch.Tensor):
                return [x] * V
            x = list(x)
            if len(x) != V:
                raise ValueError(f"{len(x)} {what} for {V} videos")
            return x

        rows = []
        for v, (te, hi) in enumerate(zip(per_video(text_embeds, "text_embeds"), per_video(hidden_in, "hidden_in"))):
            if hi is not None:
                r = hi.reshape(-1, hi.size(-1))
                if r.size(0) < self.n_query:
                    raise ValueError(f"hidden_in of video {v} has {r.size(0)} rows, fewer than the {self.n_query} query tokens")
            else:
                r = self.query_tokens[0]
                if te is not None:
                    r = torch.cat([r.to(torch.float32), te.reshape(-1, te.size(-1)).to(device=r.device, dtype=torch.float32)], 0)
            if r.size(-1) != cfg.hidden_size:
                raise ValueError(f"encoder input rows of video {v} must have width {cfg.hidden_size}")
            if r.size(0) - self.n_query > MAX_TXT_LEN:
                raise ValueError(f"video {v} has {r.size(0) - self.n_query} text tokens, at most {MAX_TXT_LEN} are supported")
            rows.append(r)
        return rows

    def encode_videos(self, videos: Sequence[torch.Tensor], text_embeds=None, hidden_in=None, new_video: bool = True,
                      u: Optional[torch.Tensor] = None, memories: Optional[Sequence["VideoChat2Memory"]] = None,
                      video_ids: Optional[Sequence[int]] = None, want_hidden: bool = False):
        """Many videos through the VideoChat2 Q-former in ONE C call (``infv_vqf_vc_encode_videos``): the whole encoder, layer-major
        over the packed chunks of every video, on the HIP path.

        ``videos``: a list of [C_v, T*P, width] frame-token tensors that all share one T (a video may have no chunk).  If every
        tensor is fp16, or every one bf16, the tokens are read in place (``infv_vqf_vc_encode_videos_tok``) and the results are
        the bits of the call on ``tokens.float()``; anything else goes in as fp32.
        ``text_embeds`` / ``hidden_in``: as in :meth:`encode_tokens`, one tensor for every video or a list with one entry per
        video (entries may be None); every chunk of a video starts from the same rows.  ``memories[v]``: video v's
        :class:`VideoChat2Memory` (by default a reused pool of the encoder; the model's own modules are untouched).
        Returns (inputs_mistral [sum C_v, n_query, llm_hidden], per-video means [V, n_query, llm_hidden], per-video last hidden
        states -- a list of [C_v, n_query + n_text_v, hidden] -- or None).  A video's outputs and memories do not depend on the
        rest of the batch (bit for bit); they agree with looping :meth:`encode_tokens` to fp32 rounding.
        ``u`` [sum C_v, n_cross, 512] float64; by default drawn from torch's global CPU generator exactly as that loop consumes
        it (video by video, chunk by chunk, 512 + 512 per LTM instance, nothing on a new video's first chunk).  With
        :meth:`use_device_rng` and ``u=None`` nothing is drawn on the host: cross layer i of video id ``video_ids[v]`` (default:
        v) draws from stream ``(id + 1) * n_cross + i``; the model's own modules keep stream i."""
        return self._vc_call("encode_videos", videos, None, text_embeds, hidden_in, new_video, u, memories, video_ids, want_hidden)

    def encode_streams(self, videos: Sequence[torch.Tensor], frame_src: Sequence[int], text_embeds=None, hidden_in=None,
                       new_video: bool = True, u: Optional[torch.Tensor] = None,
                       memories: Optional[Sequence["VideoChat2Memory"]] = None, video_ids: Optional[Sequence[int]] = None,
                       want_hidden: bool = False):
        """Several instructions per video over ONE copy of its frame tokens (``infv_vqf_vc_encode_streams``).  The Q-former
        takes the instruction as input (videochat2_it_mistral.py:204-223), so queries, draws and memories depend on it; the
        frame tokens do not.

        ``videos``: the F distinct [C_f, T*P, width] frame-token tensors (fp16 / bf16 as in :meth:`encode_videos`).  ``frame_src[v]``: the block stream v reads, in any
        order; several streams may name one block.  ``text_embeds`` / ``hidden_in`` (one for all or one per stream),
        ``memories`` and ``video_ids`` are per STREAM; ``u`` is [sum over streams of C, n_cross, 512].  Returns
        :meth:`encode_videos`'s triple, per stream, and its bits: those of ``encode_videos([videos[s] for s in frame_src], ...)``
        -- without the copies, with one token pass over the distinct chunks.  The default host uniforms are drawn stream by
        stream exactly as ``draw_vc_uniforms`` draws them for that many videos; with :meth:`use_device_rng` stream v draws from
        the stream ids ``encode_videos`` gives video id ``video_ids[v]`` (default: v)."""
        return self._vc_call("encode_streams", videos, frame_src, text_embeds, hidden_in, new_video, u, memories, video_ids, want_hidden)

    def _check_input_ids(self, input_ids, V: int) -> List[List[int]]:
        """Per video / stream the instruction's token ids as a list of ints; ValueError before any device call."""
        emb = self.qformer.bert.embeddings
        vocab, max_pos = emb.word_embeddings.num_embeddings, emb.position_embeddings.num_embeddings
        if isinstance(input_ids, torch.Tensor) or input_ids is None:
            input_ids = [input_ids] * V
        input_ids = list(input_ids)
        if len(input_ids) != V:
            raise ValueError(f"{len(input_ids)} input_ids for {V} videos")
        out = []
        for v, ids in enumerate(input_ids):
            if ids is None:
                out.append([])
                continue
            ids = torch.as_tensor(ids)
            if ids.dim() != 1 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
                raise ValueError(f"input_ids[{v}] must be a 1-D integer tensor")
            n = int(ids.numel())
            if n > max_pos:
                raise ValueError(f"input_ids[{v}] has {n} tokens, the position table has {max_pos} rows")
            if n > MAX_TXT_LEN:
                raise ValueError(f"video {v} has {n} text tokens, at most {MAX_TXT_LEN} are supported")
            lst = [int(x) for x in ids.detach().cpu().tolist()]
            for t_, x in enumerate(lst):
                if not 0 <= x < vocab:
                    raise ValueError(f"input_ids[{v}][{t_}] = {x} outside [0, {vocab})")
            out.append(lst)
        return out

    def _front(self, device, vision: bool, ids: Optional[List[List[int]]]):
        """(``infv_vqf_vc_front``, what it points to) with the vision LayerNorm and / or the embedding layer switched on."""
        keep = []

        def t(x):
            y = _dev_f32(x, device)
            keep.append(y)
            return y.data_ptr()

        vis = _lib.VqfVisionLn(None, None, 0.0)
        if vision:
            ln = self.vision_layernorm
            vis = _lib.VqfVisionLn(t(ln.weight), t(ln.bias), float(ln.eps))
        emb, ids_p = _lib.VqfVcEmb(None, None, _lib.LayerNorm(None, None), 0, 0, None), None
        if ids is not None:
            e = self.qformer.bert.embeddings
            emb = _lib.VqfVcEmb(t(e.word_embeddings.weight), t(e.position_embeddings.weight),
                                _lib.LayerNorm(t(e.LayerNorm.weight), t(e.LayerNorm.bias)), e.word_embeddings.num_embeddings,
                                e.position_embeddings.num_embeddings, t(self.query_tokens[0]))
            flat = [x for lst in ids for x in lst]
            arr = (C.c_int32 * max(len(flat), 1))(*flat)
            keep.append(arr)
            ids_p = C.cast(arr, C.c_void_p)
        return _lib.VqfVcFront(vis, emb, ids_p, 0), keep

    def encode_img_videos(self, videos: Sequence[torch.Tensor], input_ids=None, frame_src: Optional[Sequence[int]] = None,
                          hidden_in=None, new_video: bool = True, u: Optional[torch.Tensor] = None,
                          memories: Optional[Sequence["VideoChat2Memory"]] = None, video_ids: Optional[Sequence[int]] = None,
                          want_hidden: bool = False):
        """``encode_img`` behind the vision encoder in ONE C call (``infv_vqf_vc_encode_img``): from the vision encoder's output
        and the tokenizer's ids to ``inputs_mistral`` (videochat2_it_mistral.py:195, :204-223, :252).

        ``videos``: the vision encoder's output blocks [C, T*P, width] BEFORE ``vision_layernorm``, all fp32, all fp16 or all
        bf16, read in place (cloned only where a block is not contiguous or not 16-byte aligned); the LayerNorm runs inside the
        token pass, no fp32 copy of the tokens is made.  ``frame_src``: None (video v reads ``videos[v]``) or the block of every
        stream, as in :meth:`encode_streams`.  ``input_ids``: one 1-D integer tensor per video / stream (an entry may be None: no
        instruction); the embedding layer (Qformer.py:54-111) runs on the device, over the query tokens too.  ``hidden_in``
        instead of ``input_ids`` hands over ready encoder input rows as :meth:`encode_videos` takes them.  Everything else, and
        the returned triple, is :meth:`encode_videos`'s.  The results are the bits of
        ``encode_videos(vision_tokens_layernorm(videos), hidden_in=embed_instructions(input_ids))``.
        Raises RuntimeError if the model was built without ``vision_layernorm=True``, or without ``vocab_size`` where the
        embedding layer is needed; ValueError on bad ids (negative, >= vocab, more than ``max_position_embeddings``)."""
        if not hasattr(self, "vision_layernorm"):
            raise RuntimeError("encode_img_videos needs the vision LayerNorm: build the model with vision_layernorm=True")
        if input_ids is not None and hidden_in is not None:
            raise ValueError("input_ids and hidden_in are both given: one of them makes the encoder input rows")
        if hidden_in is None and not hasattr(self.qformer.bert, "embeddings"):
            raise RuntimeError("encode_img_videos needs the embedding layer (build the model with vocab_size=...) or hidden_in")
        name = "encode_img_videos"
        return self._vc_call(name, videos, frame_src, None, hidden_in, new_video, u, memories, video_ids, want_hidden,
                             img=True, input_ids=input_ids)

    def vision_tokens_layernorm(self, tokens: torch.Tensor) -> torch.Tensor:
        """``vision_layernorm`` of [..., width] fp32 / fp16 / bf16 tokens as an fp32 tensor, by the kernels and the arithmetic of
        :meth:`encode_img_videos` (``infv_vqf_layernorm_tokens``): the reference form of its bits."""
        if not hasattr(self, "vision_layernorm"):
            raise RuntimeError("vision_tokens_layernorm needs the vision LayerNorm: build the model with vision_layernorm=True")
        if not tokens.is_cuda:
            raise RuntimeError("the VideoChat2 binding runs on the HIP device only (no CPU fallback)")
        ln = self.vision_layernorm
        if tokens.size(-1) != ln.normalized_shape[0]:
            raise ValueError(f"tokens must have width {ln.normalized_shape[0]}")
        device = tokens.device
        x = tokens.detach() if tokens.dtype in TOKEN_DTYPES else tokens.detach().float()
        if not x.is_contiguous() or x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
        g, b = _dev_f32(ln.weight, device), _dev_f32(ln.bias, device)
        out = torch.empty(x.shape, device=device, dtype=torch.float32)
        if x.numel() == 0:
            return out
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_layernorm_tokens(
                C.c_void_p(x.data_ptr()), TOKEN_DTYPES[x.dtype], x.numel() // x.size(-1), x.size(-1), C.c_void_p(g.data_ptr()),
                C.c_void_p(b.data_ptr()), float(ln.eps), C.c_void_p(out.data_ptr()),
                C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return out

    def embed_instructions(self, input_ids, device=None) -> List[torch.Tensor]:
        """Per video the encoder input rows [n_query + n_text_v, hidden] the embedding layer gives (Qformer.py:54-111:
        ``LayerNorm(cat(query_tokens, word(ids) + position))``), by ``infv_vqf_vc_embed``; ``input_ids``: a list with one 1-D
        integer tensor (or None) per video."""
        if not hasattr(self.qformer.bert, "embeddings"):
            raise RuntimeError("embed_instructions needs the embedding layer: build the model with vocab_size=...")
        device = self.query_tokens.device if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the VideoChat2 binding runs on the HIP device only (no CPU fallback)")
        V = len(input_ids)
        ids = self._check_input_ids(input_ids, V)
        front, keep = self._front(device, False, ids)
        Q, Hd = self.n_query, self.qformer.config.hidden_size
        tl = (C.c_int32 * max(V, 1))(*[len(x) for x in ids])
        out = torch.empty(sum(Q + len(x) for x in ids), Hd, device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            _lib.check(_lib.load().infv_vqf_vc_embed(self._vc_handle(device), C.byref(front), V, C.cast(tl, C.c_void_p),
                                                     C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        del keep
        return list(out.split([Q + len(x) for x in ids]))

    def _vc_call(self, name, videos, frame_src, text_embeds, hidden_in, new_video, u, memories, video_ids, want_hidden,
                 img=False, input_ids=None):
        """Body of :meth:`encode_videos` (``frame_src`` None: video v reads ``videos[v]``), :meth:`encode_streams` and
        :meth:`encode_img_videos` (``img``: the vision LayerNorm, and with ``hidden_in`` None the embedding layer, run inside the
        call).  Everything a caller can get wrong on the host raises ValueError before any device call."""
        videos = list(videos)
        F = len(videos)
        if F == 0:
            raise ValueError(f"{name} needs at least one video")
        streams = frame_src is not None
        if streams:
            frame_src = [int(s) for s in frame_src]
            for v, s_ in enumerate(frame_src):
                if not 0 <= s_ < F:
                    raise ValueError(f"frame_src[{v}] = {s_} outside [0, {F})")
            if not frame_src:
                raise ValueError(f"{name} needs at least one stream")
        V = len(frame_src) if streams else F
        cfg = self.qformer.config
        P, Q = self.tokens_per_frame, self.n_query
        n_cross = len(self.qformer.cross_layers)
        for v, f in enumerate(videos):
            if f.dim() != 3 or f.size(2) != cfg.encoder_width or f.size(1) % P or f.size(1) == 0:
                raise ValueError(f"videos[{v}] must be [C, T*{P}, {cfg.encoder_width}], got {tuple(f.shape)}")
            if f.size(1) != videos[0].size(1):
                raise ValueError(f"videos[{v}] has T = {f.size(1) // P}, videos[0] has T = {videos[0].size(1) // P}: "
                                 "one call takes one chunk length")
        T = videos[0].size(1) // P
        block_counts = [int(f.size(0)) for f in videos]
        counts = [block_counts[s_] for s_ in frame_src] if streams else block_counts   # chunks per stream
        total = sum(counts)
        ids = self._check_input_ids(input_ids, V) if img and hidden_in is None else None   # (the embedding layer runs in the call)
        rows = self._vc_inputs(V, text_embeds, hidden_in) if ids is None else None
        text_len = [int(r.size(0)) - Q for r in rows] if ids is None else [len(x) for x in ids]
        use_ltm = cfg.alpha != 1.0 and n_cross > 0
        if use_ltm and memories is not None:
            memories = _check_vc_memories(self, memories, V)
        if video_ids is not None and len(video_ids) != V:
            raise ValueError(f"{len(video_ids)} video_ids for {V} videos")
        if u is not None and use_ltm and tuple(u.shape) != (total, n_cross, NB_SAMPLES):
            raise ValueError(f"u must be [{total}, {n_cross}, {NB_SAMPLES}]")
        if not all(f.is_cuda for f in videos):
            raise RuntimeError("the VideoChat2 binding runs on the HIP device only (no CPU fallback)")
        device = videos[0].device
        llm = self.mistral_proj.out_features
        if total == 0 and not (use_ltm and new_video):
            return (torch.empty(0, Q, llm, device=device), torch.full((V, Q, llm), float("nan"), device=device),
                    [torch.empty(0, Q + n, cfg.hidden_size, device=device) for n in text_len] if want_hidden else None)
        # fp16 / bf16 / fp8 e4m3fn tokens (every block of one such type) are read in place by the _tok entry points: no fp32 copy, no
        # cat of one block, a clone only where a view is not contiguous or not 16-byte aligned; anything else goes in as fp32, as
        # before (an fp8 encoding other than e4m3fn raises TypeError)
        codes = [token_code(f.dtype) for f in videos]
        half = videos[0].dtype if codes[0] and \
            all(f.dtype == videos[0].dtype and f.device == device for f in videos) else None
        if half is None:
            frames = _dev_f32(torch.cat(videos) if F > 1 else videos[0], device)
            if img and frames.data_ptr() % 16:
                frames = frames.clone(memory_format=torch.contiguous_format)
        else:
            frames = torch.cat(videos) if F > 1 else videos[0].detach()
            if not frames.is_contiguous() or frames.data_ptr() % 16:
                frames = frames.clone(memory_format=torch.contiguous_format)
        tok = () if half is None else (token_code(half),)      # the argument the _tok entry points take behind `frames`
        lib = _lib.load()
        hin = torch.cat([_dev_f32(r, device) for r in rows]).contiguous() if rows is not None else None
        handles = None
        if not use_ltm:
            u = None                                          # (no memory: nothing is drawn)
        else:
            if memories is None:
                while len(self._vc_memories) < V:
                    self._vc_memories.append(VideoChat2Memory(self, device))
                memories = self._vc_memories[:V]
            for mem in memories:
                mem._check(self, device)
            handles = (C.c_void_p * (V * n_cross))()
            for v, mem in enumerate(memories):
                for i, eng in enumerate(mem.engines):
                    eng.ensure_plan(T)
                    handles[v * n_cross + i] = eng._h
                mem.set_device_rng(self._device_rng_seed, (video_ids[v] if video_ids is not None else v)
                                   if self._device_rng_seed is not None else None)
            if u is None and self._device_rng_seed is None and bool(cfg.sticky):
                u = draw_vc_uniforms(counts, [not new_video and mem.has_memory for mem in memories], n_cross)
            if u is not None:
                u = u.to(device=device, dtype=torch.float64).contiguous()
                if tuple(u.shape) != (total, n_cross, NB_SAMPLES):
                    raise ValueError(f"u must be [{total}, {n_cross}, {NB_SAMPLES}]")
        w, keep = self._vc_weights(device)
        n_rows = sum(c * (Q + n) for c, n in zip(counts, text_len))
        hidden = torch.empty(n_rows, cfg.hidden_size, device=device, dtype=torch.float32) if want_hidden else None
        proj = torch.empty(total, Q, llm, device=device, dtype=torch.float32)
        mean = torch.empty(V, Q, llm, device=device, dtype=torch.float32)
        cu = (C.c_int32 * (V + 1))(0, *_cumsum(counts))
        tl = (C.c_int32 * V)(*text_len)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if img:
            front, keep_front = self._front(device, True, ids)
            fcu = (C.c_int32 * (F + 1))(0, *_cumsum(block_counts))
            src = (C.c_int32 * V)(*frame_src) if streams else None
            with torch.cuda.device(device):
                _lib.check(lib.infv_vqf_vc_encode_img(
                    self._vc_handle(device), handles, V, C.cast(cu, C.c_void_p), C.c_void_p(frames.data_ptr()),
                    token_code(frames.dtype), F, C.cast(fcu, C.c_void_p), C.cast(src, C.c_void_p) if streams else None, T,
                    C.byref(w), C.byref(front), C.c_void_p(0 if hin is None else hin.data_ptr()), C.cast(tl, C.c_void_p),
                    C.c_void_p(0 if u is None else u.data_ptr()), int(bool(new_video)),
                    C.c_void_p(0 if hidden is None else hidden.data_ptr()), C.c_void_p(proj.data_ptr()), C.c_void_p(mean.data_ptr()),
                    stream))
            del keep_front
        tail = (T, C.byref(w), C.c_void_p(0 if hin is None else hin.data_ptr()), C.cast(tl, C.c_void_p), C.c_void_p(0 if u is None else u.data_ptr()),
                int(bool(new_video)), C.c_void_p(0 if hidden is None else hidden.data_ptr()), C.c_void_p(proj.data_ptr()),
                C.c_void_p(mean.data_ptr()), stream)
        with torch.cuda.device(device):
            if img:
                pass                                          # (issued above)
            elif streams:
                fcu = (C.c_int32 * (F + 1))(0, *_cumsum(block_counts))
                src = (C.c_int32 * V)(*frame_src)
                _lib.check((lib.infv_vqf_vc_encode_streams_tok if tok else lib.infv_vqf_vc_encode_streams)(
                    self._vc_handle(device), handles, V, C.cast(cu, C.c_void_p), C.c_void_p(frames.data_ptr()), *tok, F,
                    C.cast(fcu, C.c_void_p), C.cast(src, C.c_void_p), *tail))
            else:
                _lib.check((lib.infv_vqf_vc_encode_videos_tok if tok else lib.infv_vqf_vc_encode_videos)(
                    self._vc_handle(device), handles, V, C.cast(cu, C.c_void_p), C.c_void_p(frames.data_ptr()), *tok, *tail))
        del keep
        hid = None
        if want_hidden:
            hid, r0 = [], 0
            for c, n in zip(counts, text_len):
                hid.append(hidden[r0:r0 + c * (Q + n)].view(c, Q + n, cfg.hidden_size))
                r0 += c * (Q + n)
        return proj, mean, hid

    # ------------------------------------------------------------------ encode_img after the vision encoder
    def encode_tokens(self, image_embeds: torch.Tensor, text_embeds: Optional[torch.Tensor] = None,
                      new_video: bool = False, hidden_in: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """image_embeds [1, T*196, 1024] (layer-normed vision tokens, videochat2_it_mistral.py:194-196);
        text_embeds [1, n_text, hidden] = the embedding layer's rows for the instruction (or None);
        ``hidden_in`` overrides the whole encoder input [1, n_query + n_text, hidden] (tests).
        Returns (inputs_mistral [1, n_query, llm_hidden], last_hidden_state)."""
        if not image_embeds.is_cuda:
            raise RuntimeError("the VideoChat2 binding runs on the HIP device only (no CPU fallback)")
        if image_embeds.dim() != 3 or image_embeds.size(0) != 1:
            raise ValueError("image_embeds must be [1, T*196, width] (batch 1)")
        cfg = self.qformer.config
        P = self.tokens_per_frame
        if image_embeds.size(2) != cfg.encoder_width or image_embeds.size(1) % P:
            raise ValueError(f"image_embeds must be [1, T*{P}, {cfg.encoder_width}]")
        k = image_embeds[0].detach().to(torch.float32).contiguous()
        if hidden_in is not None:
            hidden = hidden_in.to(torch.float32)
        else:
            hidden = self.query_tokens.to(torch.float32)
            if text_embeds is not None:
                hidden = torch.cat([hidden, text_embeds.to(torch.float32)], dim=1)      # Qformer.py:100-106 (embeddings output)
        nq = self.n_query
        use_ltm = cfg.alpha != 1.0
        with torch.no_grad():
            for layer in self.qformer.bert.encoder.layer:
                att = layer.attention
                attention_output = att.output(att.self.self_attention(hidden), hidden)   # Qformer.py:445-458
                query_out = attention_output[:, :nq, :]
                if layer.has_cross_attention:                                            # :463-481
                    x = layer.crossattention
                    hook = x.self._hook
                    xq = x.self.query(query_out)                                         # mixed_query_layer (:209)
                    a_long = hook.long_term(image_embeds, xq, None, layer.layer_num, new_video) if use_ltm else 0
                    merged = self._cross_attention(layer, k, xq, a_long)
                    query_out = x.output(merged, query_out)
                out = layer.output_query(layer.intermediate_query(query_out), query_out)  # :483-488
                if attention_output.size(1) > nq:                                        # text tokens: their own FFN (:489-496)
                    txt = attention_output[:, nq:, :]
                    out = torch.cat([out, layer.output(layer.intermediate(txt), txt)], dim=1)
                hidden = out
            inputs_mistral = self.mistral_proj(hidden[:, :nq, :])                        # videochat2_it_mistral.py:252
        return inputs_mistral, hidden


def encode_long_video_vc(model: VideoChat2Encoder, frame_tokens: torch.Tensor, num_samples: int,
                         text_embeds: Optional[torch.Tensor] = None, hidden_in: Optional[torch.Tensor] = None):
    """The VideoChat2 eval loop (eval_code/run_nextqa_mistral.py:141-152): ``torch.chunk(video, num_samples, dim=1)``
    over frames, ``new_video`` true on the first chunk only, mean of the stacked per-chunk embeddings.
    frame_tokens [F, 196, width] -> (mean [1, n_query, llm_hidden], per-chunk list)."""
    embs = []
    new_video = True
    for blk in torch.chunk(frame_tokens, num_samples, dim=0):
        emb, _ = model.encode_tokens(blk.reshape(1, -1, blk.size(-1)), text_embeds, new_video, hidden_in)
        embs.append(emb)
        new_video = False
    return torch.mean(torch.stack(embs), dim=0, keepdim=True).squeeze(0), embs


def batched_chunks_vc(n_frames: int, num_samples: int, tokens_per_frame: int) -> Optional[int]:
    """Frames per chunk if ``torch.chunk(video, num_samples)`` cuts ``n_frames`` frames into equal chunks whose token count
    the HIP contractions tile (a multiple of 32); None if the video has to take the per-chunk loop."""
    if n_frames <= 0 or num_samples <= 0:
        return None
    T = -(-n_frames // num_samples)                         # torch.chunk: ceil-sized chunks, the last one may be shorter
    if n_frames % T or (T * tokens_per_frame) % 32:
        return None
    return T


def encode_long_videos_vc(model: VideoChat2Encoder, frame_tokens_list: Sequence[torch.Tensor], num_samples: int,
                          text_embeds=None, hidden_in=None, memories: Optional[Sequence[VideoChat2Memory]] = None,
                          video_ids: Optional[Sequence[int]] = None):
    """Batched counterpart of :func:`encode_long_video_vc` over many videos: ``frame_tokens_list[v]`` [F_v, 196, width] is cut
    by ``torch.chunk(video, num_samples)`` as the eval loop cuts it; the videos whose chunks are equal and tile (see
    :func:`batched_chunks_vc`) go through :meth:`VideoChat2Encoder.encode_videos`, one call per chunk length; the others take
    the per-chunk loop on the model's own modules.  ``text_embeds`` / ``hidden_in``: one for all or one per video.
    ``memories`` / ``video_ids``: one per video, used by the batched ones.  The global generator is consumed video by video
    as the loop over :func:`encode_long_video_vc` consumes it (nothing with :meth:`VideoChat2Encoder.use_device_rng`).
    Returns a list of (mean [1, n_query, llm_hidden], per-chunk list) per video."""
    V = len(frame_tokens_list)
    P = model.tokens_per_frame
    cfg = model.qformer.config
    n_cross = len(model.qformer.cross_layers)
    per_video = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * V
    tes, his = per_video(text_embeds), per_video(hidden_in)
    if len(tes) != V or len(his) != V:
        raise ValueError("text_embeds / hidden_in: one for all videos or one per video")
    if memories is not None and len(memories) != V:
        raise ValueError(f"{len(memories)} memories for {V} videos")
    if video_ids is not None and len(video_ids) != V:
        raise ValueError(f"{len(video_ids)} video_ids for {V} videos")
    host_u = cfg.alpha != 1.0 and bool(cfg.sticky) and model._device_rng_seed is None and n_cross > 0
    out: List = [None] * V
    groups: dict = {}
    for v, ft in enumerate(frame_tokens_list):                  # in video order: the generator is consumed as the loop does
        T = batched_chunks_vc(int(ft.size(0)), num_samples, P)
        if T is None:
            out[v] = encode_long_video_vc(model, ft, num_samples, tes[v], his[v])
            continue
        n_c = int(ft.size(0)) // T
        u_v = draw_vc_uniforms([n_c], [False], n_cross) if host_u else None
        groups.setdefault(T, []).append((v, ft.reshape(n_c, T * P, ft.size(-1)), u_v))
    for T, items in groups.items():
        idx = [v for v, _, _ in items]
        proj, mean, _ = model.encode_videos(
            [f for _, f, _ in items], [tes[v] for v in idx], [his[v] for v in idx], True,
            torch.cat([u_v for _, _, u_v in items]) if host_u else None,
            None if memories is None else [memories[v] for v in idx],
            None if video_ids is None else [video_ids[v] for v in idx])
        r0 = 0
        for j, (v, f, _) in enumerate(items):
            n_c = int(f.size(0))
            out[v] = (mean[j:j + 1], [proj[r0 + c:r0 + c + 1] for c in range(n_c)])
            r0 += n_c
    return out


def encode_long_video_prompts_vc(model: VideoChat2Encoder, frame_tokens: torch.Tensor, num_samples: int,
                                 text_embeds_list: Sequence[Optional[torch.Tensor]], hidden_in_list=None,
                                 memories: Optional[Sequence[VideoChat2Memory]] = None,
                                 video_ids: Optional[Sequence[int]] = None):
    """K instructions asked of ONE video (the eval loop with the question passed to the Q-former,
    eval_code/run_nextqa_mistral.py:141-152 with ``system_q``): ``frame_tokens`` [F, 196, width] is cut as
    :func:`encode_long_video_vc` cuts it, and every instruction of ``text_embeds_list`` is a stream of
    :meth:`VideoChat2Encoder.encode_streams` over the one copy of its chunks.  Where the cut does not batch (see
    :func:`batched_chunks_vc`) it is the loop over :func:`encode_long_video_vc`, instruction by instruction; the global generator
    is consumed in that loop's order either way (not at all with :meth:`VideoChat2Encoder.use_device_rng`).
    ``hidden_in_list``: None or one entry per instruction; ``memories`` / ``video_ids``: one per instruction.
    Returns a list of (mean [1, n_query, llm_hidden], per-chunk list) per instruction."""
    tes = list(text_embeds_list)
    K = len(tes)
    if K == 0:
        raise ValueError("encode_long_video_prompts_vc needs at least one instruction")
    his = [None] * K if hidden_in_list is None else list(hidden_in_list)
    if len(his) != K:
        raise ValueError(f"{len(his)} hidden_in for {K} instructions")
    if memories is not None and len(memories) != K:
        raise ValueError(f"{len(memories)} memories for {K} instructions")
    if video_ids is not None and len(video_ids) != K:
        raise ValueError(f"{len(video_ids)} video_ids for {K} instructions")
    P = model.tokens_per_frame
    T = batched_chunks_vc(int(frame_tokens.size(0)), num_samples, P)
    if T is None:
        return [encode_long_video_vc(model, frame_tokens, num_samples, tes[k], his[k]) for k in range(K)]
    cfg = model.qformer.config
    n_cross = len(model.qformer.cross_layers)
    n_c = int(frame_tokens.size(0)) // T
    host_u = cfg.alpha != 1.0 and bool(cfg.sticky) and model._device_rng_seed is None and n_cross > 0
    u = draw_vc_uniforms([n_c] * K, [False] * K, n_cross) if host_u else None
    proj, mean, _ = model.encode_streams([frame_tokens.reshape(n_c, T * P, frame_tokens.size(-1))], [0] * K, tes, his, True, u,
                                         memories, video_ids)
    return [(mean[k:k + 1], [proj[k * n_c + c:k * n_c + c + 1] for c in range(n_c)]) for k in range(K)]
