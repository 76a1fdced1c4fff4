"""Host mirror of the device rng (csrc/philox.h): Philox4x32-10 and the Gibbs-uniform stream built on it.

numpy only -- no torch, no GPU.  ``gibbs_uniforms`` returns exactly what the kernels generate when an engine's device rng is
on and ``u`` is None, so feeding it back as explicit ``u`` (to the engine with the rng off, or to the CPU oracle) replays a
device-rng run draw for draw.

Stream (include/infv_ltm.h, "Device rng"):
    key = (seed & 0xffffffff, seed >> 32)
    ctr = (s >> 1, layer, pos, stream_id)          s: sample slot, pos: chunk index within the document
    u[s even] = u53(w0, w1), u[s odd] = u53(w2, w3) of the block (w0, w1, w2, w3)
    u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl constants of the key schedule
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key) -> np.ndarray:
    """ctr [..., 4], key [..., 2] (broadcast against each other, values below 2^32) -> the output block [..., 4] uint32."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    lead = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], lead).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], lead).copy() for i in range(2)]
    m0, m1 = np.uint64(M0), np.uint64(M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> s32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def u53(a, b) -> np.ndarray:
    """Two 32-bit words -> a float64 in [0, 1) with 53 random bits (numpy's construction)."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)


def gibbs_uniforms(seed: int, stream_id: int, pos0: int, n_steps: int, n_layers: int, S: int) -> np.ndarray:
    """u [n_steps, n_layers, S] float64: step i draws at position (pos0 + i) mod 2^32.  Row 0 of a run that starts a document
    (pos0 = 0) belongs to the first chunk, which draws nothing."""
    seed, stream_id, pos0 = int(seed), int(stream_id), int(pos0)
    if not 0 <= seed < 1 << 64 or not 0 <= stream_id < 1 << 32 or not 0 <= pos0 < 1 << 32:
        raise ValueError("seed must fit 64 bits, stream_id and pos0 32 bits, unsigned")
    pairs = (S + 1) // 2
    ctr = np.empty((n_steps, n_layers, pairs, 4), np.uint64)
    ctr[..., 0] = np.arange(pairs, dtype=np.uint64)
    ctr[..., 1] = np.arange(n_layers, dtype=np.uint64)[None, :, None]
    ctr[..., 2] = ((np.arange(n_steps, dtype=np.uint64) + np.uint64(pos0)) & _MASK)[:, None, None]
    ctr[..., 3] = stream_id
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    u = np.empty((n_steps, n_layers, 2 * pairs), np.float64)
    u[..., 0::2] = u53(w[..., 0], w[..., 1])
    u[..., 1::2] = u53(w[..., 2], w[..., 3])
    return np.ascontiguousarray(u[..., :S])
