"""Many videos through the video Q-former in one call (infv_vqf_encode_videos / InfVideoEncoder.encode_videos) on the MI355X:
goldens inside a batch, batch and split invariance bit for bit, agreement with the per-video path, encode_long_videos with
ragged tails and the global generator, alpha = 1, and refusals."""
import numpy as np
import pytest
import torch

from tests.conftest import record_parity
from tests.golden.qformer_cases import QF_CASES, chunk_uniforms, load_qf_golden, qf_inputs

pytestmark = pytest.mark.gpu
ATOL = 2e-4
BY_NAME = {c.name: c for c in QF_CASES}
DEV = torch.device("cuda:0")


def make_model(case, weights):
    from infinite_video_amd.video_qformer import InfVideoEncoder
    m = InfVideoEncoder(num_video_query_token=case.n_query, hidden_size=case.hidden, llama_hidden=case.proj_out,
                        sticky=case.sticky, num_basis=case.N, tau=case.tau, alpha=case.alpha,
                        num_hidden_layers=case.n_layers)
    m.load_reference_state_dict(weights)
    return m.to(DEV)


def synth_videos(case, T, lens, seed):
    """Per video: frames [C_v, T*P, hidden] on the device and uniforms [C_v, L, 512] float64 (host)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)
    fs = [torch.randn(n, T * case.P, case.hidden, device=DEV, generator=gen) for n in lens]
    us = [torch.rand(n, case.n_layers, 512, dtype=torch.float64, generator=cpu) for n in lens]
    return fs, us


def memories_of(m, V):
    from infinite_video_amd.video_qformer import VideoMemory
    return [VideoMemory(m, DEV) for _ in range(V)]


def run(m, fs, us, memories=None, new_video=True):
    llama, mean, hidden = m.encode_videos(fs, new_video=new_video, u=torch.cat(us), want_hidden=True, memories=memories)
    torch.cuda.synchronize()
    cu = np.concatenate([[0], np.cumsum([len(f) for f in fs])])
    return [(hidden[cu[v]:cu[v + 1]], llama[cu[v]:cu[v + 1]], mean[v]) for v in range(len(fs))]


def memory_state(mem, case):
    out = []
    if case.alpha == 1.0:
        return out
    for l in range(case.n_layers):
        B, mass = mem.export_state(l)
        bins, _, probs = mem.last_draw(l)
        out.append((B.cpu(), mass.cpu(), bins.copy(), probs.copy()))
    return out


def assert_same_state(a, b, tag):
    for (Ba, ma, ba, pa), (Bb, mb, bb, pb) in zip(a, b):
        assert torch.equal(Ba, Bb), tag
        assert torch.equal(ma, mb), tag
        np.testing.assert_array_equal(ba, bb, err_msg=tag)
        np.testing.assert_array_equal(pa, pb, err_msg=tag)


GOLDEN_CASES = [c for c in QF_CASES if len(set(c.chunk_T)) == 1] + [QF_CASES[0]]


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=lambda c: c.name + ("_first2" if len(set(c.chunk_T)) > 1 else ""))
def test_goldens_inside_a_batch(case):
    """The golden video at position 1 among synthetic videos of 0, 1 and 3 chunks: per-chunk hidden and llama, its mean and
    the final B row sums match the reference (test_layer_major_whole_video_matches_goldens_and_per_chunk's tolerances)."""
    n = len(case.chunk_T) if len(set(case.chunk_T)) == 1 else 2
    T = case.chunk_T[0]
    frames, weights = qf_inputs(case)
    g = load_qf_golden(case)
    m = make_model(case, weights)
    kg = torch.from_numpy(np.stack(frames[:n])).to(DEV)
    ug = torch.from_numpy(np.stack([chunk_uniforms(case, c) for c in range(n)]))
    fs, us = synth_videos(case, T, [0, 1, 3], seed=11)
    fs.insert(1, kg)
    us.insert(1, ug)
    mems = memories_of(m, len(fs))
    hidden, llama, mean = run(m, fs, us, mems)[1]
    for c in range(n):
        np.testing.assert_allclose(hidden[c].cpu().numpy(), g[f"c{c}_hidden"], atol=ATOL, err_msg=f"hidden c{c}")
        np.testing.assert_allclose(llama[c].cpu().numpy(), g[f"c{c}_llama"], atol=ATOL, err_msg=f"llama c{c}")
    want = np.mean(np.stack([g[f"c{c}_llama"] for c in range(n)]), 0)
    np.testing.assert_allclose(mean.cpu().numpy(), want, atol=ATOL)
    if case.alpha != 1.0:
        for l in range(case.n_layers):
            Bsum = mems[1].export_state(l)[0].double().sum(1).cpu().numpy()
            np.testing.assert_allclose(Bsum, g[f"c{n - 1}_l{l}_Bsum"], atol=5e-4, err_msg=f"final B l{l}")


def test_batch_and_split_invariance_bit_for_bit():
    """One video alone, first, last and between videos of other lengths: hidden, llama, mean and its memories' B, bin
    masses and draws are the same bits.  Chunks [0, 2) with new_video then [2, 5) continued equal one call."""
    case = BY_NAME["qf_small"]
    T = case.chunk_T[0]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    (f0,), (u0,) = synth_videos(case, T, [5], seed=21)
    others_f, others_u = synth_videos(case, T, [3, 1, 7, 2], seed=22)
    runs = {"alone": ([f0], [u0], 0), "first": ([f0] + others_f, [u0] + others_u, 0),
            "last": (others_f + [f0], others_u + [u0], 4),
            "between": (others_f[:2] + [f0] + others_f[2:], others_u[:2] + [u0] + others_u[2:], 2)}
    res = {}
    for tag, (fs, us, pos) in runs.items():
        mems = memories_of(m, len(fs))
        out = run(m, fs, us, mems)[pos]
        res[tag] = ([t.cpu() for t in out], memory_state(mems[pos], case))
    for tag in ("first", "last", "between"):
        for a, b in zip(res[tag][0], res["alone"][0]):
            assert torch.equal(a, b), tag
        assert_same_state(res[tag][1], res["alone"][1], tag)
    # split invariance: two calls equal one
    fs, us = synth_videos(case, T, [5, 4, 6], seed=23)
    whole_mems = memories_of(m, 3)
    whole = run(m, fs, us, whole_mems)
    split_mems = memories_of(m, 3)
    a = run(m, [f[:2] for f in fs], [u[:2] for u in us], split_mems, new_video=True)
    b = run(m, [f[2:] for f in fs], [u[2:] for u in us], split_mems, new_video=False)
    for v in range(3):
        assert torch.equal(torch.cat([a[v][0], b[v][0]]), whole[v][0]), f"video {v} hidden"
        assert torch.equal(torch.cat([a[v][1], b[v][1]]), whole[v][1]), f"video {v} llama"
        assert_same_state(memory_state(split_mems[v], case), memory_state(whole_mems[v], case), f"video {v}")


def test_agrees_with_the_per_video_path_at_the_headline_shape():
    """T 256, N 256: each video against encode_frames_batch on the same frames and uniforms (the per-video path takes its
    GEMM shapes from the chunk count, so the values agree to rounding); chunk by chunk within 2e-4."""
    case = BY_NAME["qf_headline"]
    T = case.chunk_T[0]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    fs, us = synth_videos(case, T, [1, 3, 5, 2], seed=31)
    got = run(m, fs, us, memories_of(m, len(fs)))
    worst, differing = 0.0, 0
    for v, (f, u) in enumerate(zip(fs, us)):
        llama, mean, hidden = m.encode_frames_batch(f, new_video=True, u=u, want_hidden=True)
        torch.cuda.synchronize()
        err = (got[v][1] - llama).abs().amax(dim=(1, 2)).cpu().numpy()
        differing += int((err > ATOL).sum())
        worst = max(worst, float(err.max()))
        np.testing.assert_allclose(got[v][0].cpu().numpy(), hidden.cpu().numpy(), atol=ATOL, err_msg=f"video {v}")
        np.testing.assert_allclose(got[v][2].cpu().numpy(), mean[0].cpu().numpy(), atol=ATOL, err_msg=f"video {v}")
    record_parity(f"multi_video_qformer headline 1,3,5,2 chunks vs encode_frames_batch per video: {differing} chunks beyond "
                  f"{ATOL:g}, max |llama diff| {worst:.2e}")
    assert differing == 0


def test_encode_long_videos_ragged_tails_and_global_generator():
    """Videos of 20, 16, 5 and 10 frames at max_int 8 (full chunks batched, tails per chunk on each video's memory): the global
    generator ends in the per-video loop's state, and every mean and chunk agrees with the loop within 2e-4."""
    from infinite_video_amd.video_qformer import encode_long_video, encode_long_videos
    case = BY_NAME["qf_small"]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    gen = torch.Generator(device=DEV).manual_seed(41)
    videos = [torch.randn(F, case.P, case.hidden, device=DEV, generator=gen) for F in (20, 16, 5, 10)]
    torch.manual_seed(1234)
    ref = [encode_long_video(m, x, 8, batched=True) for x in videos]
    state_ref = torch.get_rng_state()
    torch.manual_seed(1234)
    got = encode_long_videos(m, videos, 8)
    assert torch.equal(torch.get_rng_state(), state_ref)
    for v, ((mr, er), (mg, eg)) in enumerate(zip(ref, got)):
        assert len(er) == len(eg), f"video {v}"
        np.testing.assert_allclose(mg.cpu().numpy(), mr.cpu().numpy(), atol=ATOL, err_msg=f"video {v} mean")
        for c, (a, b) in enumerate(zip(eg, er)):
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=ATOL, err_msg=f"video {v} chunk {c}")


def test_alpha1_and_refusals():
    """alpha = 1 (no memory) agrees with the per-video path; a repeated memory and a memory of another configuration are
    refused, and every memory is left as it was."""
    case = BY_NAME["qf_alpha1"]
    T = case.chunk_T[0]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    fs, us = synth_videos(case, T, [2, 1, 3], seed=51)
    got = run(m, fs, us)
    for v, f in enumerate(fs):
        llama, mean, hidden = m.encode_frames_batch(f, new_video=True, want_hidden=True)
        np.testing.assert_allclose(got[v][1].cpu().numpy(), llama.cpu().numpy(), atol=ATOL)
        np.testing.assert_allclose(got[v][2].cpu().numpy(), mean[0].cpu().numpy(), atol=ATOL)
    case = BY_NAME["qf_small"]
    _, weights = qf_inputs(case)
    m = make_model(case, weights)
    fs, us = synth_videos(case, T, [2, 3], seed=52)
    mems = memories_of(m, 2)
    run(m, fs, us, mems)
    before = [memory_state(x, case) for x in mems]
    with pytest.raises(ValueError, match="twice"):
        m.encode_videos(fs, new_video=False, u=torch.cat(us), memories=[mems[0], mems[0]])
    from infinite_video_amd.video_qformer import InfVideoEncoder, VideoMemory
    other = InfVideoEncoder(num_video_query_token=case.n_query, hidden_size=case.hidden, llama_hidden=case.proj_out,
                            sticky=case.sticky, num_basis=case.N, tau=0.9, alpha=case.alpha, num_hidden_layers=case.n_layers)
    with pytest.raises(ValueError, match="configured differently"):
        m.encode_videos(fs, new_video=False, u=torch.cat(us), memories=[mems[0], VideoMemory(other, DEV)])
    with pytest.raises(ValueError, match="memories for"):
        m.encode_videos(fs, new_video=False, u=torch.cat(us), memories=[mems[0]])
    for x, b in zip(mems, before):
        assert_same_state(memory_state(x, case), b, "after refusals")
