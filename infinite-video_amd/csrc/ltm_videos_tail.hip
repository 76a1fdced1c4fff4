// A short last chunk per video in the lockstep calls (infv_ltm_videos_tail).
//
// Included at the end of ltm_kernels.hip, not a translation unit of its own: its kernels are written over that file's
// __device__ bodies (gemm_nt_tile, update_body; pool_videos_body's sum) so that a video's arithmetic is the one of
// infv_ltm_consolidate_videos with T = its chunk's length, and no existing kernel changes.
//
// Of the five stages of a lockstep step only three know how many frames a chunk has: pooling / gather, the new-row projection and
// the update (through the operator).  Here each of them takes that per video rank: the frames of rank j's chunk of step s and the
// operator that goes with them come from the rank-indexed side table VideoTail (ltm_internal.h) where s is the video's last step
// and that chunk is short, and are T and the step's operator (a kernel argument, as in the existing kernels) everywhere else.  The
// operator of a short chunk is read through a pointer to its plan's device-resident views (Plan::views): a step holds any mix of
// tail lengths at the same launches.  The draw, the attend and the box masses do not depend on T and stay the existing launches.
// (A build that compiles every csrc/*.hip as a unit, tools/build_variant.sh, gets an empty unit from this file.)
#ifdef INFV_LTM_KERNELS_UNIT
#include "ltm_device.h"

namespace infv {

__device__ __forceinline__ bool tail_is_short(const VideoTail& t, int s) { return s == t.len - 1 && t.op_last != nullptr; }
__device__ __forceinline__ int tail_frames(const VideoTail& t, int s, int T) { return tail_is_short(t, s) ? t.tail : T; }
__device__ __forceinline__ OperatorView tail_operator(const VideoTail& t, int s, const OperatorView& op_full) {
    return tail_is_short(t, s) ? *t.op_last : op_full;
}

// ---- both tables of a group in launch_video_table's launches ----
struct VideoTablesChunk {
    VideoDesc d[kVideoTableChunk];
    VideoTail t[kVideoTableChunk];
};
static_assert(sizeof(VideoTablesChunk) <= 3584, "kernel arguments of launch_video_tables stay inside the 4 KiB limit");
__global__ __launch_bounds__(64) void video_tables_kernel(VideoDesc* __restrict__ vd_dst, VideoTail* __restrict__ vt_dst,
                                                          VideoTablesChunk c, int n) {
    constexpr int dwords = sizeof(VideoDesc) / 8, twords = sizeof(VideoTail) / 8;
    static_assert(sizeof(VideoTail) % 8 == 0, "VideoTail is copied in 8-byte words");
    const unsigned long long* dsrc = reinterpret_cast<const unsigned long long*>(c.d);
    const unsigned long long* tsrc = reinterpret_cast<const unsigned long long*>(c.t);
    unsigned long long* dout = reinterpret_cast<unsigned long long*>(vd_dst);
    unsigned long long* tout = reinterpret_cast<unsigned long long*>(vt_dst);
    for (int i = threadIdx.x; i < n * dwords; i += 64) dout[i] = dsrc[i];
    for (int i = threadIdx.x; i < n * twords; i += 64) tout[i] = tsrc[i];
}

hipError_t launch_video_tables(VideoDesc* vd_dst, const VideoDesc* descs, VideoTail* vt_dst, const VideoTail* tails, int n,
                               hipStream_t stream) {
    for (int i = 0; i < n; i += kVideoTableChunk) {
        VideoTablesChunk c;
        const int m = n - i < kVideoTableChunk ? n - i : kVideoTableChunk;
        memset(&c, 0, sizeof(c));
        memcpy(c.d, descs + i, (size_t)m * sizeof(VideoDesc));
        memcpy(c.t, tails + i, (size_t)m * sizeof(VideoTail));
        INFV_LAUNCH(video_tables_kernel, dim3(1), dim3(64), 0, stream, vd_dst + i, vt_dst + i, c, m);
    }
    return hipGetLastError();
}

// ---- pooling: pool_videos_body's units and sum (P loads in flight, summed in token order, / P) over the frames the chunk has;
//      the video's frames start at its own first frame of the packed k, its chunk of step s at s * T frames beyond ----
template <class Tok>
__device__ __forceinline__ void pool_videos_tail_body(const void* __restrict__ k_, float* __restrict__ kbar, const VideoStep& vs,
                                                      const TailStep& ts, int P, int d4, int slices) {
    typedef typename Tok::vec tvec;
    constexpr int UNROLL = 16;
    const int T = ts.T;
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= (long)vs.n * T * slices) return;
    const long fr = unit / slices;                      // j * T + f: the slots keep their T-frame stride
    const int c4 = (int)(unit - fr * slices) * 64 + lane;
    if (c4 >= d4) return;
    const int j = (int)(fr / T), f = (int)(fr - (long)j * T);
    const VideoTail t = ts.vt[j];
    if (f >= tail_frames(t, vs.s, T)) return;           // (a short chunk leaves the rest of its slot as it was: nothing reads it)
    const long frame = t.frame0 + (long)vs.s * T + f;
    const tvec* src = reinterpret_cast<const tvec*>(k_) + frame * (long)P * d4 + c4;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    int p = 0;
    for (; p + UNROLL <= P; p += UNROLL) {
        tvec v[UNROLL];
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) v[i] = __builtin_nontemporal_load(src + (long)(p + i) * d4);
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) acc += Tok::widen(v[i]);
    }
    for (; p < P; ++p) acc += Tok::widen(__builtin_nontemporal_load(src + (long)p * d4));
    const float fp = (float)P;
    acc.x /= fp; acc.y /= fp; acc.z /= fp; acc.w /= fp;
    reinterpret_cast<floatx4*>(kbar)[fr * d4 + c4] = acc;
}
template <class Tok>
__global__ __launch_bounds__(256) void pool_videos_tail_kernel(const void* __restrict__ k_, float* __restrict__ kbar, VideoStep vs,
                                                               TailStep ts, int P, int d4, int slices) {
    pool_videos_tail_body<Tok>(k_, kbar, vs, ts, P, d4, slices);
}
// (fp8: a kernel of its own name over the same body, as the pooling kernels of ltm_kernels.hip)
__global__ __launch_bounds__(256) void pool_videos_tail_f8_kernel(const void* __restrict__ k_, float* __restrict__ kbar, VideoStep vs,
                                                                  TailStep ts, int P, int d4, int slices) {
    pool_videos_tail_body<TokF8>(k_, kbar, vs, ts, P, d4, slices);
}
template <class Tok> struct PoolVideosTailFn { static auto get() { return pool_videos_tail_kernel<Tok>; } };
template <> struct PoolVideosTailFn<TokF8> { static auto get() { return pool_videos_tail_f8_kernel; } };

hipError_t launch_pool_videos_tail(const void* k, tok_code tok, const VideoStep& vs, const TailStep& ts, int P, int d, float* kbar,
                                   hipStream_t stream) {
    const int d4 = d / 4, slices = (d4 + 63) / 64;
    const long n_units = (long)vs.n * ts.T * slices;
    if (n_units == 0) return hipSuccess;
    const dim3 grid((unsigned)((n_units + 3) / 4));
    return with_token_type(tok, [&](auto t) {
        INFV_LAUNCH(PoolVideosTailFn<decltype(t)>::get(), grid, dim3(256), 0, stream, k, kbar, vs, ts, P, d4, slices);
        return hipGetLastError();
    });
}

// one thread per float4 of video rank j's chunk of this step (frame means the caller pooled, packed by frame): plain copies
__global__ __launch_bounds__(256) void gather_videos_tail_kernel(const float* __restrict__ kbar, float* __restrict__ out, VideoStep vs,
                                                                 TailStep ts, int d4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    const VideoTail t = ts.vt[j];
    if (i >= (long)tail_frames(t, vs.s, ts.T) * d4) return;
    const long frame = t.frame0 + (long)vs.s * ts.T;
    reinterpret_cast<floatx4*>(out)[(long)j * ts.T * d4 + i] = reinterpret_cast<const floatx4*>(kbar)[frame * d4 + i];
}

hipError_t launch_gather_videos_tail(const float* kbar, const VideoStep& vs, const TailStep& ts, int d, float* out, hipStream_t stream) {
    if (d % 4) return hipErrorInvalidValue;
    const long chunk4 = (long)ts.T * d / 4;
    if (vs.n == 0 || chunk4 == 0) return hipSuccess;
    INFV_LAUNCH(gather_videos_tail_kernel, dim3((unsigned)((chunk4 + 255) / 256), vs.n), dim3(256), 0, stream, kbar, out, vs, ts, d / 4);
    return hipGetLastError();
}

// ---- new-row projection: project_videos_kernel's tile (gemm_nt_tile<64, 64, true>, one K slab, no split-K), the rows of video
//      rank j built from the tables of ITS operator.  Every rank owns `tiles` 64-row tiles = row_slots row slots of the
//      workspace, so a tile never mixes two operators; gemm_nt_tile takes the rank's own row bound (first slot + its row count):
//      slots at or beyond the operator's rows are neither built nor stored, and a tile of nothing but such slots returns at once. ----
__global__ __launch_bounds__(256) void project_videos_tail_kernel(const float* __restrict__ kbar, long kbar_stride, VideoStep vs,
                                                                  TailStep ts, OperatorView op_full, int tiles, int K, WSegs segs,
                                                                  float* __restrict__ C, int ldc) {
    __shared__ __attribute__((aligned(16))) float smem[2 * 64 * kLdsStride];
    const int j = blockIdx.x / tiles, tile = blockIdx.x - j * tiles;
    const OperatorView op = tail_operator(ts.vt[j], vs.s, op_full);
    if (tile * 64 >= op.rows) return;
    const int row_slots = tiles * 64;
    const RowsA ra{kbar, op.row_begin, op.row_end, op.row_box, op.box_val, row_slots, kbar_stride};
    gemm_nt_tile<64, 64, true>(nullptr, ra, j * row_slots + op.rows, K, segs, C, ldc, 0, K, 0, smem, smem + 64 * kLdsStride);
}

hipError_t launch_project_videos_tail(const float* kbar, const VideoStep& vs, const TailStep& ts, int d, int dm, int n_layers,
                                      const OperatorView& op_full, int row_slots, const ProjPtrs& proj, float* Pnew, hipStream_t stream) {
    const int n_cols = n_layers * 2 * dm;
    if (vs.n == 0) return hipSuccess;
    if (n_cols % 64 || d % kBK || row_slots <= 0 || row_slots % 64) return hipErrorInvalidValue;
    const int tiles = row_slots / 64;
    INFV_LAUNCH(project_videos_tail_kernel, dim3(vs.n * tiles, n_cols / 64), dim3(256), 0, stream, kbar, (long)ts.T * d, vs, ts, op_full,
                tiles, d, kv_segs(proj, 0, n_layers, dm), Pnew, n_cols);
    return hipGetLastError();
}

// ---- update: update_videos_kernel with the video's own operator (its projected rows sit at rank j's row slots) ----
__global__ __launch_bounds__(1024) void update_videos_tail_kernel(VideoStep vs, TailStep ts, OperatorView op_full, int N, int d4, int dm4,
                                                                  int n_layers, int S, const int32_t* __restrict__ idx_shared,
                                                                  const float* __restrict__ kbar, long kbar_stride,
                                                                  const float* __restrict__ Pnew, long p_stride) {
    const int j = blockIdx.z;
    const VideoDesc* v = vs.vd + j;
    const OperatorView op = tail_operator(ts.vt[j], vs.s, op_full);
    const int cur = v->cur0 ^ (vs.s & 1);
    const int32_t* idx = idx_shared != nullptr ? idx_shared : v->idx;
    update_body(blockIdx.x, blockIdx.y, op, N, d4, dm4, n_layers, idx, idx_shared != nullptr ? 0 : S, nullptr, Pnew + j * p_stride, 1, 0,
                v->B[cur], v->KV[cur], v->B[cur ^ 1], v->KV[cur ^ 1], kbar + j * kbar_stride, nullptr);
}

hipError_t launch_update_videos_tail(const VideoStep& vs, const TailStep& ts, const OperatorView& op_full, int row_slots, int N, int d,
                                     int dm, int n_layers, int S, const int32_t* idx_shared, const float* kbar, const float* Pnew,
                                     hipStream_t stream) {
    if (vs.n == 0) return hipSuccess;
    const int total4 = d / 4 + 2 * (dm / 4);
    const int nt = total4 >= 1024 ? 1024 : ((total4 + 63) / 64) * 64;
    INFV_LAUNCH(update_videos_tail_kernel, dim3(N, n_layers, vs.n), dim3(nt), 0, stream, vs, ts, op_full, N, d / 4, dm / 4, n_layers, S,
                idx_shared, kbar, (long)ts.T * d, Pnew, (long)row_slots * n_layers * 2 * dm);
    return hipGetLastError();
}

}  // namespace infv
#endif  // INFV_LTM_KERNELS_UNIT
