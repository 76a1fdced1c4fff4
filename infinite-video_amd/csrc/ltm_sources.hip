// Source weights of the memory (include/infv_ltm.h: infv_ltm_source_weights): which frames of the video a basis function holds.
//
// The sparse update is linear in the frame means, B_new[n] = val[n] * (sum of resampled old rows + sum of the box's new frames)
// (long_term_attention_gibbs.py:207-216 in closed form), so B[n] = sum over sources of W[n][source] * kbar[source] with a W that
// obeys the same recurrence on one-hot rows.  The reference maps a grid point of its `alphas` straight to a frame index
// (relevant_frames.py:53-69), which holds only for a memory that was never consolidated; this pass walks the bins a whole call
// drew and keeps the mixture.  One kernel, on no default path:
//     source_weights_kernel<TILE>   one workgroup per (tile of TILE columns, layer).  Columns are independent, so the workgroup
//                                   keeps its [N x TILE] slice of W twice in LDS (old / new), walks the chunks of the call in
//                                   order with ONE barrier per chunk and writes the slice back once.  Nothing crosses
//                                   workgroups: no flags, no atomics on W.
//     source_weights_videos_kernel<TILE>   the same walk with a video index in the grid (infv_ltm_source_weights_videos): one
//                                   launch for the packed bins / masses of a lockstep call.
// Lane mapping: a thread owns 4 consecutive columns (one 16-byte LDS slot) of a box; with TILE = 64 a row is one 256-byte bank
// row and the 16 lanes of every ds_read_b128 group hold the 16 different slots of it, whatever rows they gather: conflict-free.
// With TILE = 32 (num_basis above 256) two rows share a bank row and a gather may be 2-way.
// Arithmetic: fp32 additions in CSR order, the new frames' count added last as one fp32 number, one multiplication -- nothing an
// FMA could contract.  density.source_weights(dtype=float32) states the same order in numpy and equals this bit for bit.
#include "ltm_device.h"

namespace infv {

constexpr int kSwNT = 512;                     // threads of a workgroup (8 waves)
constexpr int kSwMaxN = 512;                   // num_basis the two LDS slices hold (TILE 64 up to 256, TILE 32 up to 512)
constexpr int kSwSlots = kMaxSamples / kSwNT;  // CSR entries a thread resolves per chunk (S <= 1024)

struct SourcesArgs {
    int N, S, T, C, L, g, new_doc, sticky, n_bins;
    long col_begin, ld, M;                     // M = col_begin + C * T / g: columns at and beyond it are not touched
    OperatorView first, inf;
    const int32_t* bin_box;                    // [n_bins]
    const int32_t* uniform_idx;                // [S]
    const int32_t* bins_all;                   // [C][L][S] or nullptr (not sticky)
    float* W;                                  // [L][N][ld]
    const float* mass_all;                     // [C][L][N] or nullptr
    float* attn_all;                           // [C][L][ld] or nullptr
    int32_t* bad_bins;                         // [L] or nullptr
};

// frames of [begin, end) of the chunk whose column is the one that starts at chunk-relative frame `lo` (g frames wide)
__device__ inline float frames_in(long lo, int g, int begin, int end) {
    const long a = lo > begin ? lo : (long)begin, b = lo + g < end ? lo + g : (long)end;
    return b > a ? (float)(b - a) : 0.f;
}

// the walk of workgroup (tile, layer l) over the chunks of one call: both kernels below run it
template <int TILE>
__device__ __forceinline__ void source_weights_body(const SourcesArgs& a, const unsigned tile, const int l) {
    constexpr int QUADS = TILE / 4, ROWS = kSwNT / QUADS, GROUPS = kSwNT / TILE;
    extern __shared__ floatx4 sw_lds[];
    const int N = a.N, t = threadIdx.x;
    const size_t slice = (size_t)N * QUADS;                                      // W before the chunk: sw_lds + cur * slice; after it: the other one
    double* part = reinterpret_cast<double*>(sw_lds + 2 * slice);                // [2][GROUPS][TILE]
    int32_t* src = reinterpret_cast<int32_t*>(part + 2 * kSwNT);                 // [2][kMaxSamples] source box of CSR entry j, -1: none
    int32_t* ptr = src + 2 * kMaxSamples;                                        // [N + 1]
    int32_t* rb = ptr + N + 1;                                                   // [N] new frames of box n: [rb, re)
    int32_t* re = rb + N;
    float* val = reinterpret_cast<float*>(re + N);                               // [N]

    const long m0 = (long)tile * TILE;
    const int quad = t % QUADS, row0 = t / QUADS;
    const long mq = m0 + 4 * quad;                                               // first column of this thread's slot
    float* Wl = a.W + (long)l * N * a.ld;

    const int nnz = a.inf.old_ptr ? a.inf.old_ptr[N] : 0;
    for (int n = t; n < N; n += kSwNT) {
        ptr[n] = a.inf.old_ptr ? a.inf.old_ptr[n] : 0;
        const int r = a.inf.box_row[n];
        rb[n] = r >= 0 ? a.inf.row_begin[r] : 0;
        re[n] = r >= 0 ? a.inf.row_end[r] : 0;
        val[n] = a.inf.box_val[n];
    }
    if (t == 0) ptr[N] = nnz;

    // a tile with no column below col_begin holds zeros until the first chunk that injects into it
    const bool fresh = a.new_doc || m0 >= a.col_begin;
    int c0 = 0;
    if (m0 >= a.col_begin) {
        const long c = (m0 - a.col_begin) * a.g / a.T;
        c0 = c < a.C ? (int)c : a.C;
    }
    for (int n = row0; n < N; n += ROWS) {
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (!fresh && mq < a.col_begin) {                                        // (mq < col_begin <= ld, both multiples of 4 apart: in bounds)
            v = *reinterpret_cast<const floatx4*>(Wl + (long)n * a.ld + mq);
            if (mq + 1 >= a.col_begin) v.y = 0.f;
            if (mq + 2 >= a.col_begin) v.z = 0.f;
            if (mq + 3 >= a.col_begin) v.w = 0.f;
        }
        sw_lds[(size_t)n * QUADS + quad] = v;
    }
    if (a.attn_all)
        for (int c = 0; c < c0; ++c)
            if (t < TILE && m0 + t < a.M) a.attn_all[((long)c * a.L + l) * a.ld + m0 + t] = 0.f;

    // the CSR entries this thread resolves per chunk, and the bins of the next chunk in flight
    int my_slot[kSwSlots], bnext[kSwSlots], ball[kSwSlots];
#pragma unroll
    for (int k = 0; k < kSwSlots; ++k) {
        const int j = t + k * kSwNT;
        my_slot[k] = j < nnz ? a.inf.old_slot[j] : -1;
        bnext[k] = ball[k] = 0;
    }
    const bool count_bad = a.bad_bins && a.sticky && tile == 0;
    auto fetch = [&](int c) {
        if (!a.sticky || (a.new_doc && c == 0)) return;
        const int32_t* b = a.bins_all + ((long)c * a.L + l) * a.S;
#pragma unroll
        for (int k = 0; k < kSwSlots; ++k) {
            if (my_slot[k] >= 0) bnext[k] = b[my_slot[k]];
            if (count_bad && t + k * kSwNT < a.S) ball[k] = b[t + k * kSwNT];
        }
    };
    if (!a.sticky) {
#pragma unroll
        for (int k = 0; k < kSwSlots; ++k)
            if (my_slot[k] >= 0) src[t + k * kSwNT] = a.uniform_idx[my_slot[k]];
    }
    int bad = 0;
    if (c0 < a.C) fetch(c0);

    // attn[c][l][m] = sum_n mass[c][l][n] * W_c[n][m] in float64: group k adds rows k, k + GROUPS, ... in increasing order, the
    // groups are added in order from 0, one rounding to fp32.  Partials of W_{c-1} are formed beside the update of chunk c (both
    // only read the old slice) and combined one chunk later: no barrier of their own.
    const int pg = t / TILE, pc = t % TILE;
    auto attn_partial = [&](const floatx4* Wc, int c, int slot) {
        const float* Wf = reinterpret_cast<const float*>(Wc);
        const float* mass = a.mass_all + ((long)c * a.L + l) * N;
        double s = 0.0;
        for (int n = pg; n < N; n += GROUPS) s += (double)mass[n] * (double)Wf[(size_t)n * TILE + pc];
        part[(size_t)slot * kSwNT + t] = s;
    };
    auto attn_combine = [&](int c, int slot) {
        if (t >= TILE || m0 + t >= a.M) return;
        double s = 0.0;
        for (int k = 0; k < GROUPS; ++k) s += part[(size_t)slot * kSwNT + k * TILE + t];
        a.attn_all[((long)c * a.L + l) * a.ld + m0 + t] = (float)s;
    };

    int cur = 0;
    for (int c = c0; c < a.C; ++c) {
        const bool first = a.new_doc && c == 0;
        const int sb = a.sticky ? (c & 1) * kMaxSamples : 0;
        if (a.sticky && !first) {
#pragma unroll
            for (int k = 0; k < kSwSlots; ++k) {
                // a bin outside [0, n_bins - 1) is never used as an index: it resamples a zero row
                const bool ok = bnext[k] >= 0 && bnext[k] < a.n_bins - 1;
                if (my_slot[k] >= 0) src[sb + t + k * kSwNT] = ok ? a.bin_box[bnext[k]] : -1;
                if (count_bad && t + k * kSwNT < a.S && (ball[k] < 0 || ball[k] >= a.n_bins - 1)) ++bad;
            }
        }
        if (c + 1 < a.C) fetch(c + 1);
        __syncthreads();
        const floatx4* Wo = sw_lds + cur * slice;
        floatx4* Wn = sw_lds + (cur ^ 1) * slice;
        if (a.attn_all) {
            if (c - 1 >= c0) attn_partial(Wo, c - 1, c & 1);
            if (c - 2 >= c0) attn_combine(c - 2, (c - 1) & 1);
        }
        const OperatorView& op = first ? a.first : a.inf;
        const long lo = (mq - a.col_begin) * a.g - (long)c * a.T;                // chunk-relative first frame of column mq
        const bool inject = lo + 4l * a.g > 0 && lo < a.T;
        for (int n = row0; n < N; n += ROWS) {
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
            if (!first)
                for (int j = ptr[n]; j < ptr[n + 1]; ++j) {
                    const int s = src[sb + j];
                    if (s >= 0) acc += Wo[(size_t)s * QUADS + quad];
                }
            if (inject) {
                int begin = rb[n], end = re[n];
                if (first) {
                    const int r = op.box_row[n];
                    begin = r >= 0 ? op.row_begin[r] : 0;
                    end = r >= 0 ? op.row_end[r] : 0;
                }
                acc.x += frames_in(lo, a.g, begin, end);
                acc.y += frames_in(lo + a.g, a.g, begin, end);
                acc.z += frames_in(lo + 2l * a.g, a.g, begin, end);
                acc.w += frames_in(lo + 3l * a.g, a.g, begin, end);
            }
            const float v = first ? op.box_val[n] : val[n];
            acc.x = v * acc.x; acc.y = v * acc.y; acc.z = v * acc.z; acc.w = v * acc.w;
            Wn[(size_t)n * QUADS + quad] = acc;
        }
        cur ^= 1;
    }
    __syncthreads();
    if (a.attn_all && c0 < a.C) {
        attn_partial(sw_lds + cur * slice, a.C - 1, a.C & 1);
        if (a.C - 2 >= c0) attn_combine(a.C - 2, (a.C - 1) & 1);
        __syncthreads();
        attn_combine(a.C - 1, a.C & 1);
    }
    for (int n = row0; n < N; n += ROWS) {
        const floatx4 v = sw_lds[cur * slice + (size_t)n * QUADS + quad];
        float* out = Wl + (long)n * a.ld + mq;
        if (mq + 4 <= a.M) {
            *reinterpret_cast<floatx4*>(out) = v;
        } else {
            if (mq < a.M) out[0] = v.x;
            if (mq + 1 < a.M) out[1] = v.y;
            if (mq + 2 < a.M) out[2] = v.z;
        }
    }
    if (count_bad && bad) atomicAdd(a.bad_bins + l, bad);
}

template <int TILE>
__global__ __launch_bounds__(kSwNT) void source_weights_kernel(SourcesArgs a) {
    source_weights_body<TILE>(a, blockIdx.x, blockIdx.y);
}

// Many videos in one grid (infv_ltm_source_weights_videos): workgroup (tile, l, v) runs the walk above over video v's chunks
// [cu[v], cu[v + 1]) of the packed arrays as a new document from column 0, into W_all[v] and its own rows of attn_all.  The grid
// is as wide as the longest video: a workgroup whose tile starts at or beyond its video's M_v returns at once (a video with no
// chunk has M_v = 0).  cu travels in the kernel's arguments: no device table, nothing that outlives the launch.
constexpr int kSwVideos = 512;                 // videos per launch
struct SourcesVideosArgs {
    SourcesArgs base;                          // C, M, col_begin, new_doc are set per video; W is W_all of this launch's first video
    int32_t cu[kSwVideos + 1];                 // cu[v0 .. v0 + n] of the call
};
static_assert(sizeof(SourcesVideosArgs) <= 3072, "kernel arguments stay well inside the 4 KiB limit");

template <int TILE>
__global__ __launch_bounds__(kSwNT) void source_weights_videos_kernel(SourcesVideosArgs va) {
    const int v = blockIdx.z;
    const long c_begin = va.cu[v];
    SourcesArgs a = va.base;
    a.C = va.cu[v + 1] - va.cu[v];
    a.M = (long)a.C * (a.T / a.g);
    if ((long)blockIdx.x * TILE >= a.M) return;
    if (a.bins_all) a.bins_all += c_begin * a.L * a.S;
    a.W += (long)v * a.L * a.N * a.ld;
    if (a.attn_all) {
        a.mass_all += c_begin * a.L * a.N;
        a.attn_all += c_begin * a.L * a.ld;
    }
    source_weights_body<TILE>(a, blockIdx.x, blockIdx.y);
}

size_t source_weights_lds_bytes(int N, int tile) {
    return 2 * (size_t)N * tile * sizeof(float) + 2 * kSwNT * sizeof(double) + 2 * kMaxSamples * sizeof(int32_t) +
           (size_t)(4 * N + 1) * sizeof(int32_t);
}

hipError_t launch_source_weights(const SourcesArgs& a, hipStream_t stream) {
    if (a.N <= 0 || a.N > kSwMaxN || a.S > kMaxSamples || a.L <= 0 || a.L > 65535 || a.M <= 0) return hipErrorInvalidValue;
    const int tile = a.N <= 256 ? 64 : 32;
    const long tiles = (a.M + tile - 1) / tile;
    if (tiles > 0x7fffffffl) return hipErrorInvalidValue;
    const size_t lds = source_weights_lds_bytes(a.N, tile);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static bool attr_set = false;                  // the slices take up to 128 KB: above the 64 KB a kernel gets unasked
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(source_weights_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(source_weights_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const dim3 grid((unsigned)tiles, (unsigned)a.L);
    if (tile == 64) INFV_LAUNCH(source_weights_kernel<64>, grid, dim3(kSwNT), lds, stream, a);
    else INFV_LAUNCH(source_weights_kernel<32>, grid, dim3(kSwNT), lds, stream, a);
    return hipGetLastError();
}

// `a`: the call's tables, strides and packed arrays (W = W_all; C, M, col_begin and new_doc are the kernel's to set); cu: HOST [V + 1].
// ceil(V / kSwVideos) launches; a launch whose videos all have no chunk is not issued.
hipError_t launch_source_weights_videos(const SourcesArgs& a, const int32_t* cu, int V, hipStream_t stream) {
    if (a.N <= 0 || a.N > kSwMaxN || a.S > kMaxSamples || a.L <= 0 || a.L > 65535 || V <= 0) return hipErrorInvalidValue;
    const int tile = a.N <= 256 ? 64 : 32;
    const size_t lds = source_weights_lds_bytes(a.N, tile);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(source_weights_videos_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(source_weights_videos_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    for (int v0 = 0; v0 < V; v0 += kSwVideos) {
        const int n = V - v0 < kSwVideos ? V - v0 : kSwVideos;
        SourcesVideosArgs va{};
        va.base = a;
        va.base.new_doc = 1; va.base.col_begin = 0;
        va.base.W = a.W + (long)v0 * a.L * a.N * a.ld;
        int longest = 0;
        for (int i = 0; i <= n; ++i) va.cu[i] = cu[v0 + i];
        for (int i = 0; i < n; ++i) longest = va.cu[i + 1] - va.cu[i] > longest ? va.cu[i + 1] - va.cu[i] : longest;
        const long tiles = ((long)longest * (a.T / a.g) + tile - 1) / tile;
        if (tiles == 0) continue;
        if (tiles > 0x7fffffffl) return hipErrorInvalidValue;
        const dim3 grid((unsigned)tiles, (unsigned)a.L, (unsigned)n);
        if (tile == 64) INFV_LAUNCH(source_weights_videos_kernel<64>, grid, dim3(kSwNT), lds, stream, va);
        else INFV_LAUNCH(source_weights_videos_kernel<32>, grid, dim3(kSwNT), lds, stream, va);
    }
    return hipGetLastError();
}

}  // namespace infv

// ---- the entry points (include/infv_ltm.h) ----
#include "ltm_handle.h"

using namespace infv;

extern "C" int infv_ltm_source_weights_videos(infv_ltm_handle h, const infv_ltm_sources_videos_desc* d) {
    if (int rc = check_handle(h)) return rc;
    if (!d || !d->cu || !d->W_all) return fail(INFV_ERR_INVALID, "source_weights_videos: null descriptor, cu or W_all");
    const int V = d->n_videos;
    if (V < 1) return fail(INFV_ERR_INVALID, "source_weights_videos: n_videos=%d", V);
    if (d->reserved != 0) return fail(INFV_ERR_INVALID, "source_weights_videos: reserved must be 0");
    if (d->cu[0] < 0) return fail(INFV_ERR_INVALID, "source_weights_videos: cu[0] = %d is negative", d->cu[0]);
    int longest = 0;
    for (int v = 0; v < V; ++v) {
        if (d->cu[v + 1] < d->cu[v]) return fail(INFV_ERR_INVALID, "source_weights_videos: cu is not non-decreasing at video %d", v);
        longest = d->cu[v + 1] - d->cu[v] > longest ? d->cu[v + 1] - d->cu[v] : longest;
    }
    if (d->cu[V] == 0) return fail(INFV_ERR_INVALID, "source_weights_videos: no chunk at all (cu[V] = 0)");
    if (d->T < 1) return fail(INFV_ERR_INVALID, "source_weights_videos: T=%d", d->T);
    const int g = d->frames_per_source;
    if (g < 1 || d->T % g) return fail(INFV_ERR_INVALID, "source_weights_videos: frames_per_source=%d does not divide T=%d", g, d->T);
    const int64_t M = (int64_t)longest * (d->T / g);
    if (d->ld < M || d->ld % 4)
        return fail(INFV_ERR_INVALID, "source_weights_videos: ld=%lld must be a multiple of 4 and at least %lld (the longest video)",
                    (long long)d->ld, (long long)M);
    if (reinterpret_cast<uintptr_t>(d->W_all) & 15u) return fail(INFV_ERR_INVALID, "source_weights_videos: W_all must be 16-byte aligned");
    if (h->cfg.sticky && !d->bins_all)
        return fail(INFV_ERR_INVALID, "source_weights_videos: a sticky handle needs the packed bins of the call (infv_ltm_set_trace on every handle)");
    if (!h->cfg.sticky && d->bins_all) return fail(INFV_ERR_INVALID, "source_weights_videos: bins given to a handle that is not sticky");
    if ((d->mass_all == nullptr) != (d->attn_all == nullptr))
        return fail(INFV_ERR_INVALID, "source_weights_videos: mass_all and attn_all go together");
    auto it = h->plans.find(d->T);
    if (it == h->plans.end()) return fail(INFV_ERR_STATE, "source_weights_videos: no plan registered for chunk length T=%d", d->T);
    const Plan& plan = *it->second;
    if (plan.dense.on || plan.dense.psi_on)
        return fail(INFV_ERR_UNSUPPORTED, "source_weights_videos: the plan for T=%d is dense or general-psi (its update mixes two boxes through a dense operator)", d->T);
    if (h->N > kSwMaxN) return fail(INFV_ERR_UNSUPPORTED, "source_weights_videos: num_basis=%d above %d", h->N, kSwMaxN);
    SourcesArgs a;
    memset(&a, 0, sizeof(a));
    a.N = h->N; a.S = h->S; a.T = d->T; a.L = h->L; a.g = g; a.new_doc = 1;
    a.sticky = h->cfg.sticky ? 1 : 0; a.n_bins = plan.n_bins;
    a.ld = d->ld;
    a.first = plan.first.view(); a.inf = plan.inf.view();
    a.bin_box = plan.bin_box.as<int32_t>(); a.uniform_idx = plan.uniform_idx.as<int32_t>();
    a.bins_all = d->bins_all; a.W = d->W_all; a.mass_all = d->mass_all; a.attn_all = d->attn_all; a.bad_bins = d->bad_bins;
    HIP_TRY(launch_source_weights_videos(a, d->cu, V, static_cast<hipStream_t>(d->hip_stream)));
    return INFV_OK;
}

extern "C" int infv_ltm_source_weights(infv_ltm_handle h, const infv_ltm_sources_desc* d, const int32_t* bins_all, float* W,
                                       const float* mass_all, float* attn_all, int32_t* bad_bins, void* stream) {
    if (int rc = check_handle(h)) return rc;
    if (!d || !W) return fail(INFV_ERR_INVALID, "source_weights: null descriptor or W");
    if (d->n_chunks < 1) return fail(INFV_ERR_INVALID, "source_weights: n_chunks=%d", d->n_chunks);
    if (d->T < 1) return fail(INFV_ERR_INVALID, "source_weights: T=%d", d->T);
    const int g = d->frames_per_source;
    if (g < 1 || d->T % g) return fail(INFV_ERR_INVALID, "source_weights: frames_per_source=%d does not divide T=%d", g, d->T);
    if (d->col_begin < 0) return fail(INFV_ERR_INVALID, "source_weights: negative col_begin");
    if (d->col_begin > (int64_t)1 << 40) return fail(INFV_ERR_INVALID, "source_weights: col_begin out of range");
    const int64_t M = d->col_begin + (int64_t)d->n_chunks * (d->T / g);
    if (d->ld < M || d->ld % 4) return fail(INFV_ERR_INVALID, "source_weights: ld=%lld must be a multiple of 4 and at least %lld",
                                            (long long)d->ld, (long long)M);
    if (reinterpret_cast<uintptr_t>(W) & 15u) return fail(INFV_ERR_INVALID, "source_weights: W must be 16-byte aligned");
    if (h->cfg.sticky && !bins_all) return fail(INFV_ERR_INVALID, "source_weights: a sticky handle needs the bins of the call (infv_ltm_set_trace)");
    if (!h->cfg.sticky && bins_all) return fail(INFV_ERR_INVALID, "source_weights: bins given to a handle that is not sticky");
    if ((mass_all == nullptr) != (attn_all == nullptr))
        return fail(INFV_ERR_INVALID, "source_weights: mass_all and attn_all go together");
    auto it = h->plans.find(d->T);
    if (it == h->plans.end()) return fail(INFV_ERR_STATE, "source_weights: no plan registered for chunk length T=%d", d->T);
    const Plan& plan = *it->second;
    if (plan.dense.on || plan.dense.psi_on)
        return fail(INFV_ERR_UNSUPPORTED, "source_weights: the plan for T=%d is dense or general-psi (its update mixes two boxes through a dense operator)", d->T);
    if (h->N > kSwMaxN) return fail(INFV_ERR_UNSUPPORTED, "source_weights: num_basis=%d above %d", h->N, kSwMaxN);
    SourcesArgs a;
    memset(&a, 0, sizeof(a));
    a.N = h->N; a.S = h->S; a.T = d->T; a.C = d->n_chunks; a.L = h->L; a.g = g; a.new_doc = d->new_doc ? 1 : 0;
    a.sticky = h->cfg.sticky ? 1 : 0; a.n_bins = plan.n_bins;
    a.col_begin = d->col_begin; a.ld = d->ld; a.M = M;
    a.first = plan.first.view(); a.inf = plan.inf.view();
    a.bin_box = plan.bin_box.as<int32_t>(); a.uniform_idx = plan.uniform_idx.as<int32_t>();
    a.bins_all = bins_all; a.W = W; a.mass_all = mass_all; a.attn_all = attn_all; a.bad_bins = bad_bins;
    HIP_TRY(launch_source_weights(a, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}
