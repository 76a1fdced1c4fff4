"""The frame (image) Q-former without a device: the CPU oracle against the golden of the real reference encoder, the state-dict
mapping, the exported symbol and the frame-count arithmetic of ``encode_short_memory_frame``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infinite_video_amd import _lib
from infinite_video_amd.frame_qformer import FrameQformerEncoder
from infinite_video_amd.video_qformer import ShortMemoryBuffer
from oracle.videochat2_oracle import VideoChat2Oracle
from tests.golden.frame_qformer_cases import (FULL, GOLDEN_FRAMES, GOLDEN_PATH, GOLDEN_TAPS, GOLDEN_TOKENS, LN_VISION_EPS, SMALL,
                                              frame_qformer_weights, oracle_weights, vision_rows)

ATOL = 2e-4                                # the project's own (tests/test_vc_gpu.py)


def test_oracle_reproduces_the_reference_golden():
    """``VideoChat2Oracle(alpha=1.0, n_query=32, tokens_per_frame=257)``, as it is, is the image Q-former: the golden holds the real
    reference ``BertEmbeddings`` + ``BertEncoder`` on 3 frames x 257 tokens."""
    g = np.load(GOLDEN_PATH)
    sd = frame_qformer_weights(**FULL)
    q = torch.from_numpy(sd["query_tokens"][0])
    h0 = F.layer_norm(q, (q.size(-1),), torch.from_numpy(sd["Qformer.bert.embeddings.LayerNorm.weight"]),
                      torch.from_numpy(sd["Qformer.bert.embeddings.LayerNorm.bias"]), 1e-12).numpy()
    assert np.abs(h0 - g["h0"]).max() <= 1e-6                       # h0 is layer_norm(query_tokens), nothing else
    x = torch.from_numpy(vision_rows(GOLDEN_FRAMES, GOLDEN_TOKENS, FULL["enc_width"]))
    k = F.layer_norm(x, (x.size(-1),), torch.from_numpy(sd["ln_vision.weight"]), torch.from_numpy(sd["ln_vision.bias"]),
                     LN_VISION_EPS).numpy()
    orc = VideoChat2Oracle(oracle_weights(sd), 64, 0.75, 1.0, True, n_layers=FULL["n_layers"], cross_freq=2,
                           n_heads=FULL["n_heads"], n_query=FULL["n_query"], tokens_per_frame=GOLDEN_TOKENS)
    for f in range(GOLDEN_FRAMES):
        hid, _ = orc.encode_chunk(k[f], h0, True)
        assert np.abs(hid - g["hidden"][f]).max() <= ATOL
        for l in GOLDEN_TAPS:
            assert np.abs(orc.taps[f"l{l}_xctx"] - g[f"l{l}_xctx"][f]).max() <= ATOL


def _small_model():
    return FrameQformerEncoder(num_query_token=SMALL["n_query"], vision_width=SMALL["enc_width"], num_hidden_layers=SMALL["n_layers"],
                               hidden_size=SMALL["hidden"], intermediate_size=SMALL["inter"], num_attention_heads=SMALL["n_heads"])


def test_parameter_tree_carries_the_reference_names():
    names = set(_small_model().state_dict())
    assert {"query_tokens", "ln_vision.weight", "ln_vision.bias", "Qformer.bert.embeddings.LayerNorm.weight",
            "Qformer.bert.encoder.layer.0.crossattention.self.key.weight",
            "Qformer.bert.encoder.layer.3.output_query.LayerNorm.bias"} <= names
    assert not any(".layer.1.crossattention." in n for n in names)      # cross-attention in every second layer
    assert _small_model().ln_vision.eps == 1e-5


def test_load_reference_state_dict():
    sd = frame_qformer_weights(**SMALL)
    hidden = SMALL["hidden"]
    # what a checkpoint of the model also holds and the image Q-former never uses
    extra = {"Qformer.cls.predictions.bias": np.zeros(11, np.float32),
             "Qformer.cls.predictions.transform.dense.weight": np.zeros((hidden, hidden), np.float32),
             "Qformer.bert.embeddings.word_embeddings.weight": np.zeros((11, hidden), np.float32),
             "Qformer.bert.embeddings.position_embeddings.weight": np.zeros((5, hidden), np.float32),
             "Qformer.bert.embeddings.position_ids": np.arange(5)[None]}
    assert any(k.startswith("Qformer.bert.encoder.layer.1.intermediate.") for k in sd)        # the text FFN is in the key set
    m = _small_model()
    res = m.load_reference_state_dict({**sd, **extra}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    own = m.state_dict()
    assert not any(k.startswith("Qformer.cls.") or "word_embeddings" in k or ".layer.1.intermediate." in k for k in own)
    for k in ("query_tokens", "ln_vision.weight", "Qformer.bert.encoder.layer.2.crossattention.self.value.weight",
              "Qformer.bert.embeddings.LayerNorm.bias"):
        assert torch.equal(own[k], torch.from_numpy(sd[k]))
    with pytest.raises(KeyError):
        _small_model().load_reference_state_dict({**sd, "Qformer.bert.encoder.layer.0.nonsense.weight": np.zeros(3, np.float32)})
    with pytest.raises(KeyError):
        _small_model().load_reference_state_dict({k: v for k, v in sd.items() if k != "ln_vision.bias"})
    _small_model().load_reference_state_dict({**sd, "nonsense": np.zeros(3, np.float32)}, strict=False)
    bad = dict(sd)
    bad["Qformer.bert.encoder.layer.0.crossattention.self.key.weight"] = np.zeros((hidden, SMALL["enc_width"] + 64), np.float32)
    with pytest.raises(ValueError):
        _small_model().load_reference_state_dict(bad)
    with pytest.raises(ValueError):
        _small_model().load_reference_state_dict({**sd, "query_tokens": sd["query_tokens"][:, :-1]}, strict=False)


def test_symbol_is_exported_by_the_built_library():
    assert "infv_vqf_encode_frames" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), "infv_vqf_encode_frames")


@pytest.mark.parametrize("n_frames,n_frame", [(0, 2048), (1, 2048), (5, 3), (5, 4), (5, 5), (7, 0), (9, 8), (3, 2048)])
def test_kept_frames_is_the_buffer_rule(n_frames, n_frame):
    """``encode_short_memory_frame`` encodes the frames ``ShortMemoryBuffer.replace`` would keep: min(F, n_frame + 1)."""
    buf = ShortMemoryBuffer(2, 4, capacity_frames=16)
    buf.replace(torch.zeros(n_frames, 2, 4), n_frame)
    keep = FrameQformerEncoder.kept_frames(n_frames, n_frame)
    assert keep == len(buf) == min(n_frames, n_frame + 1)


def test_encode_short_memory_frame_refuses_on_the_host():
    m = _small_model()
    x = torch.zeros(3, 5, SMALL["enc_width"])
    with pytest.raises(ValueError):                                  # another frame shape than the Q-former writes
        m.encode_short_memory_frame(x, ShortMemoryBuffer(SMALL["n_query"] + 1, SMALL["hidden"], capacity_frames=4))
    with pytest.raises(ValueError):                                  # more kept frames than the buffer holds
        m.encode_short_memory_frame(x, ShortMemoryBuffer(SMALL["n_query"], SMALL["hidden"], capacity_frames=2))
    with pytest.raises(RuntimeError):                                # no CPU fallback
        m.encode_frames(x)
    with pytest.raises(ValueError):
        m.encode_frames(torch.zeros(3, 5, SMALL["enc_width"] + 1))
