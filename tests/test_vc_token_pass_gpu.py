"""The token pass alone, through ``infv_vqf_token_pass``: fp32 / fp16 / bf16 frame tokens -> the split planes, their transposed copies
and the frame means.  Everything is ``torch.equal``: the planes do not depend on tokens_per_frame, so the same call with
tokens_per_frame = 4 is their reference -- and, for fp32 and fp16 tokens, the split computed on the host (hi = bf16(x),
lo = bf16(x - hi), round to nearest even); the frame means are ``infv_ltm_pool``'s bits at the token dtype and on ``tokens.float()``.

A one-pass form WITH the means exists where a frame divides the pass's 64-token tile.  For the other frame sizes (12, 68, 196, 6) a
per-frame kernel was built, passed every check below bit for bit on an MI355X and was then measured against pooling + this pass
at 128 eval-shape chunks: 1.395 against 0.854 ms for fp16 tokens, 0.585 against 0.443 ms for bf16 (profiles/vc_half_tokens.jsonl).
It lost for both and was deleted, so for those sizes the call with the means is refused without a launch and the encoders take
the two passes -- which is what this file then checks: planes from the pass, means from the pooling at the token dtype.
Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import record_parity

pytestmark = pytest.mark.gpu
UNSUPPORTED = -2
PAD = 64                                            # sentinel elements on either side of every output
CODES = {torch.float32: 0, torch.float16: 3, torch.bfloat16: 1}
# (P, T, d, nb)
CASES = [(12, 16, 64, 2),                           # frames straddle tiles
         (68, 16, 64, 1),                           # one full tile plus 4 rows
         (196, 16, 64, 2),                          # the real frame
         (196, 16, 128, 3),                         # slab and chunk strides
         (4, 16, 64, 2), (32, 4, 128, 2),           # P divides 64: planes and means in one launch
         (4, 8, 64, 1),                             # n = 32: one tile, partial
         (4, 24, 64, 2),                            # n = 96: a whole tile plus a partial one, two chunks
         (32, 3, 128, 2),                           # n = 96: the partial tile holds exactly one frame, two column tiles
         (6, 32, 64, 1)]                            # no one-pass form: refused without a launch


def dev0():
    return torch.device("cuda:0")


def tokens(P, T, d, nb, dtype, seed):
    """normal(0, 1) x 2^k, k per element from [-8, 8]; a few elements forced to +-0, the largest finite value, the smallest
    subnormal and its negative -- of the dtype's own range.  fp32: +-0 alone -- no subnormals and nothing beyond the bf16 range, so
    both pieces of the split are exact round-to-nearest conversions of normal numbers on the host as on the device."""
    rng = np.random.default_rng(seed)
    n = T * P
    x = rng.standard_normal((nb, n, d)) * np.exp2(rng.integers(-8, 9, (nb, n, d)))
    t = torch.from_numpy(x).to(dtype)
    if dtype == torch.float32:
        edge = torch.tensor([0.0, -0.0], dtype=dtype)
    else:
        fi = torch.finfo(dtype)
        tiny = fi.smallest_normal * fi.eps          # the smallest subnormal: 2^-24 (fp16), 2^-133 (bf16)
        edge = torch.tensor([0.0, -0.0, fi.max, tiny, -tiny, -fi.max], dtype=torch.float64).to(dtype)
        assert float(edge[3]) > 0 and float(edge[3].double()) == tiny
    flat = t.view(-1)
    flat[(torch.arange(edge.numel()) * 1031 + 7) % flat.numel()] = edge
    return t


def sequential_sums(t, P):
    """One fp32 accumulator per (frame, column), the frame's tokens added in token order -- on the host.  Returns the sums
    [nb, T, d] and the tokens as [nb, T, d, P] fp32 (a frame's tokens contiguous)."""
    x = np.ascontiguousarray(t.float().numpy().reshape(t.shape[0], -1, P, t.shape[-1]).transpose(0, 1, 3, 2))
    acc = np.zeros(x.shape[:3], np.float32)
    for p in range(P):
        acc = (acc + x[..., p]).astype(np.float32)
    return acc, x


def pairwise_sums(x):
    """The same sums by halving (fp32): another order of the same additions."""
    if x.shape[-1] == 1:
        return x[..., 0]
    h = x.shape[-1] // 2
    return (pairwise_sums(x[..., :h]) + pairwise_sums(x[..., h:])).astype(np.float32)


class Out:
    """An output buffer with PAD sentinel elements on either side; the interior starts as NaN."""

    def __init__(self, numel, dtype, dev):
        self.buf = torch.empty(numel + 2 * PAD, dtype=dtype, device=dev)
        self.sentinel = 1.5 if dtype == torch.float32 else -3.0
        self.buf.fill_(self.sentinel)
        self.mid = self.buf[PAD:PAD + numel]
        self.mid.fill_(float("nan"))
        assert self.mid.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.mid.data_ptr())

    def check(self, tag):
        assert bool((self.buf[:PAD] == self.sentinel).all()) and bool((self.buf[-PAD:] == self.sentinel).all()), f"{tag}: wrote outside"
        assert bool(torch.isfinite(self.mid.float()).all()), f"{tag}: an element was not written"
        return self.mid


def run_pass(lib, t, P, with_means):
    """(rc, launches, {plane name: tensor}, kbar or None) of one infv_vqf_token_pass call on tokens t [nb, n, d]."""
    dev = t.device
    nb, n, d = t.shape
    bf = t.dtype == torch.bfloat16
    names = ("Th",) if bf else ("Fh", "Fl", "Th", "Tl")
    planes = {k: Out(nb * n * d, torch.bfloat16, dev) for k in names}
    kbar = Out(nb * (n // P) * d, torch.float32, dev) if with_means else None
    ptr = lambda k: planes[k].ptr if k in planes else None
    torch.cuda.synchronize()
    n0 = lib.infv_ltm_launch_count()
    with torch.cuda.device(dev):
        rc = lib.infv_vqf_token_pass(C.c_void_p(t.data_ptr()), CODES[t.dtype], nb, n, d, P, ptr("Fh"), ptr("Fl"), ptr("Th"), ptr("Tl"),
                                     kbar.ptr if kbar else None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.infv_ltm_launch_count() - n0, planes, kbar


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("P,T,d,nb", CASES, ids=lambda v: str(v))
def test_token_pass_planes_and_frame_means(P, T, d, nb, dtype):
    from infinite_video_amd import _lib
    from infinite_video_amd.engine import LTMEngine
    lib = _lib.load()
    dev = dev0()
    host = tokens(P, T, d, nb, dtype, seed=17 * P + d + nb)
    # the inputs discriminate: summing a frame in token order is not what a pairwise sum gives, somewhere
    seq, x = sequential_sums(host, P)
    other = pairwise_sums(x)
    assert (seq != other).any(), "the summation order is not being tested by these inputs"
    if P >= 16:                                                       # (numpy sums short rows in order; longer ones pairwise)
        assert (seq != np.sum(x, axis=-1, dtype=np.float32)).any()
    means = seq / np.float32(P)
    t = host.to(dev)
    tag = f"token pass P={P} T={T} d={d} nb={nb} {dtype}"

    rc, launches, planes, kbar = run_pass(lib, t, P, True)
    one_pass = 64 % P == 0
    if not one_pass:                                                  # refused before any launch; the planes-only call then runs
        assert rc == UNSUPPORTED and launches == 0, (rc, launches)
        for k, o in planes.items():                                   # nothing ran: the interior is still NaN
            assert bool(torch.isnan(o.mid.float()).all()), k
        rc, launches, planes, kbar = run_pass(lib, t, P, False)
    assert rc == 0, lib.infv_ltm_last_error()
    assert launches == 1, launches

    rc4, _, ref, _ = run_pass(lib, t, 4, False)                       # planes only, through the existing kernels
    assert rc4 == 0, lib.infv_ltm_last_error()
    for k in planes:
        assert torch.equal(planes[k].check(f"{tag} {k}"), ref[k].check(f"{tag} reference {k}")), f"{tag}: plane {k} differs"
    # (what the planes are: hi + lo is the token exactly, transposed copies are transposes)
    n = T * P
    if dtype == torch.bfloat16:
        assert torch.equal(planes["Th"].mid.view(nb, d, n), t.transpose(1, 2))
    else:
        if dtype == torch.float16:
            hi, lo = planes["Fh"].mid.view(nb, n, d).float(), planes["Fl"].mid.view(nb, n, d).float()
            assert torch.equal(hi + lo, t.float())
        # the split on the host: torch rounds float32 -> bfloat16 to nearest even, as the device's conversion does
        ref_hi = host.float().bfloat16()
        ref_lo = (host.float() - ref_hi.float()).bfloat16()
        assert torch.equal(planes["Fh"].mid.view(nb, n, d).cpu(), ref_hi), f"{tag}: Fh differs from bf16(x) on the host"
        assert torch.equal(planes["Fl"].mid.view(nb, n, d).cpu(), ref_lo), f"{tag}: Fl differs from bf16(x - bf16(x)) on the host"
        assert torch.equal(planes["Tl"].mid.view(nb, d, n), planes["Fl"].mid.view(nb, n, d).transpose(1, 2))
        assert torch.equal(planes["Th"].mid.view(nb, d, n), planes["Fh"].mid.view(nb, n, d).transpose(1, 2))

    eng = LTMEngine(32, 2, 64, d, P, 0.75, True, device=dev, fp16_tokens=True)
    if one_pass:
        got = kbar.check(f"{tag} kbar").view(nb, T, d)
        assert torch.equal(got, eng.pool(t)), f"{tag}: frame means differ from infv_ltm_pool at the token dtype"
    else:                                                             # the means the encoders use for this frame size
        got = eng.pool(t)
    assert torch.equal(got, eng.pool(t.float())), f"{tag}: frame means differ from infv_ltm_pool on tokens.float()"
    worst = float((got.cpu() - torch.from_numpy(means)).abs().max())
    assert worst == 0.0, f"{tag}: frame means differ from the host's sequential fp32 sum by {worst}"
    record_parity(f"{tag}: planes == the pass at P = 4, means ({'one pass' if one_pass else 'infv_ltm_pool at the token dtype'}) == infv_ltm_pool on .float() == host sequential sum; "
                  f"{int((seq != other).sum())} of {seq.size} sums differ from a pairwise sum")
