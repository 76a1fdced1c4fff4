// The cross-attention of infv_vqf_encode_frames with fp16 operands and fp32 accumulation (infv_vqf_set_attention_precision(h, 1)):
// what the reference's fp16 autocast computes, on the f16 MFMA.  Per frame f, head h (dh = 64), with x^ = fp16(tokens) from
// token_pass_f16_kernel (token_pass.hip) as X [F][n_pad][d] and XT [F][d][n_pad], pad rows exact zeros:
//   q~' = fp16( 32 * sum_c fp16(q[h*64+c]) * fp16(Wk[h*64+c][:]) )          qtilde_f16_kernel   (32 = 2^8 / sqrt(64))
//   s[j] = 2^-8 * sum_e q~'[e] * x^[j][e];  p = softmax over the first n columns (fp32, maximum subtracted);  p' = fp16(2^10 * p)
//   o' = fp16( 2^-10 * sum_j p'[j] * x^[j][:] )                              attn_f16_kernel: the scores never reach memory
//   ctx[h*64+c] = sum_e o'[e] * fp16(Wv[h*64+c][e]) + bv[h*64+c]             vproj_f16_kernel
// The two powers of two keep q~' and p' out of fp16's subnormal range; beyond fp16's range a value becomes inf, as `.half()` gives.
// A lane's MFMA fragment is 8 consecutive k of one row; the two small products read it from global memory as it lies, the attention
// kernel stages its operands through LDS.
// A frame's tiles, k order and reductions do not depend on the batch; rows past a frame's own read zeros and are not stored.
#include "vqf_internal.h"
#include "ltm_device.h"

namespace infv {

namespace {
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
__device__ inline floatx16 mfma_f16(halfx8 a, halfx8 b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ inline halfx8 load8(const _Float16* p) { return __builtin_bit_cast(halfx8, *reinterpret_cast<const uint4*>(p)); }
__device__ inline halfx8 zero8() { return __builtin_bit_cast(halfx8, make_uint4(0u, 0u, 0u, 0u)); }
// row of accumulator register r inside a 32 x 32 tile (the column is lane & 31)
__device__ inline int acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }
__device__ inline float half_max(float v) {                   // over the 32 lanes that share lane >> 5; fixed order
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ inline float half_sum(float v) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
}  // namespace

// plane[h][e][c] = fp16(Wk[h*64 + c][e]): the key weight of head h transposed, so that a row is the 64-deep k run of column e
__global__ __launch_bounds__(256) void attn_f16_key_plane_kernel(const float* __restrict__ wk, int d, long n, _Float16* __restrict__ plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i & 63);
    const long he = i >> 6;
    const int e = (int)(he % d), h = (int)(he / d);
    plane[i] = (_Float16)wk[((long)h * 64 + c) * d + e];
}

hipError_t launch_attn_f16_key_plane(const float* wk, int H, int d, void* plane, hipStream_t stream) {
    const long n = (long)H * d * 64;
    if (n <= 0) return hipSuccess;
    INFV_LAUNCH(attn_f16_key_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, wk, d, n, static_cast<_Float16*>(plane));
    return hipGetLastError();
}

// qt[f][h*Q + q][e] = fp16(32 * sum_c fp16(xq[f*Q + q][h*64 + c]) * wkT[h][e][c]).  64 x 64 tiles of (query row, e), 4 waves as
// 2 x 2, K = 64 in four steps; grid (ceil(nb*Q / 64), d / 64, H).
__global__ __launch_bounds__(256) void qtilde_f16_kernel(AttnF16 a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1, h = blockIdx.z;
    const int M = a.nb * a.Q, hidden = a.H * 64;
    const int m = blockIdx.x * 64 + wm * 32 + li;
    const int e = blockIdx.y * 64 + wn * 32 + li;
    const float* xr = a.xq + (long)m * hidden + h * 64 + kh * 8;
    const _Float16* wr = static_cast<const _Float16*>(a.wkT) + ((long)h * a.d + e) * 64 + kh * 8;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        halfx8 av = zero8();
        if (m < M) {
            const floatx4 x0 = *reinterpret_cast<const floatx4*>(xr + ks * 16), x1 = *reinterpret_cast<const floatx4*>(xr + ks * 16 + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { av[k] = (_Float16)x0[k]; av[4 + k] = (_Float16)x1[k]; }
        }
        acc = mfma_f16(av, load8(wr + ks * 16), acc);
    }
    _Float16* qt = static_cast<_Float16*>(a.qt);
    const int rows = a.H * a.Q;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = blockIdx.x * 64 + wm * 32 + acc_row(r, kh);
        if (mr < M) {
            const int f = mr / a.Q, q = mr - f * a.Q;
            qt[((long)f * rows + h * a.Q + q) * a.d + e] = (_Float16)(32.0f * acc[r]);
        }
    }
}

// One workgroup: 64 score rows (h*Q + q) of one frame against all n_pad keys, then their context rows.  Wave w owns the 32-column
// key tiles w, w + 4, ... (at most NTW of them) of both 32-row halves, so the scores of the block live in 2 * NTW accumulators per
// lane; row maxima and sums go lane -> 32-lane half -> the four waves through LDS, in one order.  p' is written to LDS as the A
// operand of the context product, whose 32-column tiles of d again go wave by wave, 128 columns a pass.
// Both products stage their global operands through LDS in 64-deep k-tiles -- 16-byte loads, eight lanes to a 128-byte row segment,
// the next tile in flight in registers while this one is multiplied (linear_gemm_kernel's scheme) -- and read the MFMA fragments
// from rows 144 bytes apart.  grid (ceil(H*Q / 64), nb).  Dynamic LDS (attn_f16_lds_bytes): the score stage (64 + n_pad rows), later
// reused by p' (64 rows of n_pad + 8 halves) and the context stage (128 rows); then 2 x 4 x 64 floats of reductions.
constexpr int kAPitch = 144;                      // bytes per staged row: 64 halves + 16 B
template <int NTW>
__global__ __launch_bounds__(256) void attn_f16_kernel(AttnF16 a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
    const int rows = a.H * a.Q, d = a.d, n = a.n, n_pad = a.n_pad, f = blockIdx.y, rb = blockIdx.x * 64;
    const int ntile = n_pad / 32, pitch = n_pad + 8;
    const int p_bytes = 64 * pitch * 2;
    const int s_bytes = (64 + n_pad) * kAPitch, c_bytes = p_bytes + 128 * kAPitch;
    _Float16* P = reinterpret_cast<_Float16*>(smem);
    unsigned char* cstage = smem + p_bytes;                    // the context product's stage, behind p'
    float* redm = reinterpret_cast<float*>(smem + (s_bytes > c_bytes ? s_bytes : c_bytes));
    float* reds = redm + 256;
    const _Float16* qt = static_cast<const _Float16*>(a.qt) + (long)f * rows * d;
    const _Float16* X = static_cast<const _Float16*>(a.X) + (long)f * n_pad * d;
    const _Float16* XT = static_cast<const _Float16*>(a.XT) + (long)f * d * n_pad;

    // ---- scores: stage rows [0, 64) = q~' rows rb .. (zeros past the frame's own), rows [64, 64 + n_pad) = the keys
    constexpr int NLD = 2 + 4 * NTW;                           // 16-byte units per thread and k-tile: (64 + n_pad) * 8 / 256 at most
    const int n_units = (64 + n_pad) * 8;
    const _Float16* src[NLD];
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int e = tid + 256 * u, r = e >> 3, seg = (e & 7) * 8;
        src[u] = nullptr;
        if (e < n_units) {
            if (r >= 64) src[u] = X + (long)(r - 64) * d + seg;
            else if (rb + r < rows) src[u] = qt + (long)(rb + r) * d + seg;
        }
    }
    uint4 stg[NLD];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) stg[u] = src[u] ? *reinterpret_cast<const uint4*>(src[u] + k0) : make_uint4(0u, 0u, 0u, 0u);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int e = tid + 256 * u;
            if (e < n_units) *reinterpret_cast<uint4*>(smem + (e >> 3) * kAPitch + (e & 7) * 16) = stg[u];
        }
    };
    floatx16 acc[2][NTW];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][t][r] = 0.f;
    bool tile_ok[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) tile_ok[t] = wave + 4 * t < ntile;   // (wave-uniform)
    load_tile(0);
    for (int k0 = 0; k0 < d; k0 += 64) {                       // (d % 64 == 0)
        store_tile();
        __syncthreads();
        if (k0 + 64 < d) load_tile(k0 + 64);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            halfx8 av[2], bv[NTW];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = load8(reinterpret_cast<const _Float16*>(smem + (i * 32 + li) * kAPitch + ks * 32 + kh * 16));
#pragma unroll
            for (int t = 0; t < NTW; ++t)
                if (tile_ok[t]) bv[t] = load8(reinterpret_cast<const _Float16*>(smem + (64 + (wave + 4 * t) * 32 + li) * kAPitch + ks * 32 + kh * 16));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < NTW; ++t)
                    if (tile_ok[t]) acc[i][t] = mfma_f16(av[i], bv[t], acc[i][t]);
        }
        __syncthreads();
    }

    // ---- softmax over the first n columns, fp32
    bool live[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) live[t] = tile_ok[t] && (wave + 4 * t) * 32 + li < n;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                acc[i][t][r] *= 0.00390625f;                   // 2^-8, exact
                mx = fmaxf(mx, live[t] ? acc[i][t][r] : -INFINITY);
            }
            mx = half_max(mx);
            if (li == 0) redm[wave * 64 + i * 32 + acc_row(r, kh)] = mx;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i * 32 + acc_row(r, kh);
            const float mx = fmaxf(fmaxf(redm[row], redm[64 + row]), fmaxf(redm[128 + row], redm[192 + row]));
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                acc[i][t][r] = live[t] ? expf(acc[i][t][r] - mx) : 0.f;
                sum += acc[i][t][r];
            }
            sum = half_sum(sum);
            if (li == 0) reds[wave * 64 + row] = sum;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i * 32 + acc_row(r, kh);
            const float inv = 1024.0f / ((reds[row] + reds[64 + row]) + (reds[128 + row] + reds[192 + row]));
#pragma unroll
            for (int t = 0; t < NTW; ++t)
                if (tile_ok[t]) P[row * pitch + (wave + 4 * t) * 32 + li] = (_Float16)(acc[i][t][r] * inv);
        }

    // ---- context: o'[row][e] = fp16(2^-10 * sum_j p'[row][j] * x^[j][e]); per pass 128 columns of d (32 per wave), the keys in
    // 64-deep tiles staged from the transposed plane (rows past d read zeros; d % 64 == 0, so a wave's 32 columns are in or out whole)
    _Float16* O = static_cast<_Float16*>(a.o) + (long)f * rows * d;
    const int nk = n_pad / 64, n_iter = ((d + 127) / 128) * nk;
    uint4 cst[4];
    auto load_ctx = [&](int it) {
        const int e0 = (it / nk) * 128, k0 = (it % nk) * 64;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, r = e >> 3;
            cst[u] = e0 + r < d ? *reinterpret_cast<const uint4*>(XT + (long)(e0 + r) * n_pad + k0 + (e & 7) * 8) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    floatx16 oc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oc[i][r] = 0.f;
    load_ctx(0);
    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u;
            *reinterpret_cast<uint4*>(cstage + (e >> 3) * kAPitch + (e & 7) * 16) = cst[u];
        }
        __syncthreads();                                       // (the first one also publishes p')
        if (it + 1 < n_iter) load_ctx(it + 1);
        const int kc = it % nk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const halfx8 b = load8(reinterpret_cast<const _Float16*>(cstage + (wave * 32 + li) * kAPitch + ks * 32 + kh * 16));
#pragma unroll
            for (int i = 0; i < 2; ++i) oc[i] = mfma_f16(load8(P + (i * 32 + li) * pitch + kc * 64 + ks * 16 + kh * 8), b, oc[i]);
        }
        if (kc == nk - 1) {
            const int e0 = (it / nk) * 128 + wave * 32;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rb + i * 32 + acc_row(r, kh);
                    if (row < rows && e0 < d) O[(long)row * d + e0 + li] = (_Float16)(oc[i][r] * 0.0009765625f);   // 2^-10, exact
                    oc[i][r] = 0.f;
                }
        }
        __syncthreads();
    }
}

// ctx[f*Q + q][h*64 + c] = sum_e o'[f][h*Q + q][e] * wv16[h*64 + c][e] + bv[h*64 + c].  64 (frame, query) rows x the 64 columns of
// head h, 4 waves as 2 x 2; grid (ceil(nb*Q / 64), H).
__global__ __launch_bounds__(256) void vproj_f16_kernel(AttnF16 a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1, h = blockIdx.y;
    const int M = a.nb * a.Q, rows = a.H * a.Q, d = a.d, hidden = a.H * 64;
    const int m = blockIdx.x * 64 + wm * 32 + li;
    const bool ok = m < M;
    const int f = ok ? m / a.Q : 0, q = ok ? m - f * a.Q : 0;
    const _Float16* ar = static_cast<const _Float16*>(a.o) + ((long)f * rows + h * a.Q + q) * d + kh * 8;
    const _Float16* br = static_cast<const _Float16*>(a.wv16) + (long)(h * 64 + wn * 32 + li) * d + kh * 8;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k64 = 0; k64 < d; k64 += 64)                      // (d % 64 == 0)
#pragma unroll
        for (int k0 = k64; k0 < k64 + 64; k0 += 16) acc = mfma_f16(ok ? load8(ar + k0) : zero8(), load8(br + k0), acc);
    const int col = h * 64 + wn * 32 + li;
    const float bias = a.bv ? a.bv[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = blockIdx.x * 64 + wm * 32 + acc_row(r, kh);
        if (mr < M) a.ctx[(long)mr * hidden + col] = acc[r] + bias;
    }
}

size_t attn_f16_lds_bytes(int n_pad) {
    const size_t score = (size_t)(64 + n_pad) * kAPitch, ctx = (size_t)64 * (n_pad + 8) * 2 + 128 * kAPitch;
    return (score > ctx ? score : ctx) + 2 * 256 * sizeof(float);
}

hipError_t launch_attn_f16(const AttnF16& a, hipStream_t stream) {
    if (a.nb <= 0) return hipSuccess;
    if (a.Q < 1 || a.H < 1 || a.d < 64 || a.d % 64 || a.n < 1 || a.n > a.n_pad || a.n_pad % 64 || a.n_pad > kAttnF16MaxPad || a.nb > 65535 ||
        !a.xq || !a.wkT || !a.wv16 || !a.X || !a.XT || !a.qt || !a.o || !a.ctx)
        return hipErrorInvalidValue;
    const int M = a.nb * a.Q, rows = a.H * a.Q;
    INFV_LAUNCH(qtilde_f16_kernel, dim3((M + 63) / 64, a.d / 64, a.H), dim3(256), 0, stream, a);
    const dim3 grid((rows + 63) / 64, a.nb);
    const size_t lds = attn_f16_lds_bytes(a.n_pad);
    if (lds > 64 * 1024) {                                      // n_pad = 384: 66 KB of dynamic LDS, 512: 87 KB -- an opt-in per device
        constexpr int kMaxDev = 64;
        static bool attr_set[kMaxDev] = {};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxDev || !attr_set[dev]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_f16_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_f16_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            if (dev >= 0 && dev < kMaxDev) attr_set[dev] = true;
        }
    }
    switch ((a.n_pad / 32 + 3) / 4) {                           // key tiles per wave: the kernel shape depends on the frame's n alone
        case 1: INFV_LAUNCH(attn_f16_kernel<1>, grid, dim3(256), lds, stream, a); break;
        case 2: INFV_LAUNCH(attn_f16_kernel<2>, grid, dim3(256), lds, stream, a); break;
        case 3: INFV_LAUNCH(attn_f16_kernel<3>, grid, dim3(256), lds, stream, a); break;
        default: INFV_LAUNCH(attn_f16_kernel<4>, grid, dim3(256), lds, stream, a); break;
    }
    INFV_LAUNCH(vproj_f16_kernel, dim3((M + 63) / 64, a.H), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace infv
