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

template <int TILE>
__global__ __launch_bounds__(kSwNT) void source_weights_kernel(SourcesArgs a) {
    constexpr int QUADS = TILE / 4, ROWS = kSwNT / QUADS, GROUPS = kSwNT / TILE;
    extern __shared__ floatx4 sw_lds[];
    const int N = a.N, t = threadIdx.x, l = blockIdx.y;
    const size_t slice = (size_t)N * QUADS;                                      // W before the chunk: sw_lds + cur * slice; after it: the other one
    double* part = reinterpret_cast<double*>(sw_lds + 2 * slice);                // [2][GROUPS][TILE]
    int32_t* src = reinterpret_cast<int32_t*>(part + 2 * kSwNT);                 // [2][kMaxSamples] source box of CSR entry j, -1: none
    int32_t* ptr = src + 2 * kMaxSamples;                                        // [N + 1]
    int32_t* rb = ptr + N + 1;                                                   // [N] new frames of box n: [rb, re)
    int32_t* re = rb + N;
    float* val = reinterpret_cast<float*>(re + N);                               // [N]

    const long m0 = (long)blockIdx.x * TILE;
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
    const bool count_bad = a.bad_bins && a.sticky && blockIdx.x == 0;
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

}  // namespace infv

// ---- the entry point (include/infv_ltm.h) ----
#include "ltm_handle.h"

using namespace infv;

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
