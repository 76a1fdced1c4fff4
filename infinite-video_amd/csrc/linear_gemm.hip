// The query-side linears of infv_vqf_encode_frames in reduced arithmetic (infv_vqf_set_linear_precision): C = x . W^T with the
// fp32 activations x read as they lie and prepared on the way into LDS, the weights read from 2-byte planes prepared once.
//   split-bf16 (bf16, three products): x and W carried as hi = bf16(v), lo = bf16(v - hi); per k-step lo.hi, hi.lo, hi.hi on the
//     bf16 MFMA with fp32 accumulation -- the scheme and the order of split_gemm_kernel<3> (split_gemm.hip).
//   fp16 (one product): x and W rounded to nearest-even fp16 (beyond 65504: inf, as `.half()` gives); one f16 MFMA per k-step.
// The result only feeds the frame tokens; it never reaches the scores of a Gibbs draw (the entry points that do refuse the mode).
#include "vqf_internal.h"
#include "ltm_device.h"

namespace infv {

namespace {
constexpr int kLBK = 64;                          // k per tile (four 32x32x16 steps)
constexpr int kLPitch = 2 * kLBK + 16;            // bytes per LDS row: 64 elements + 16 B (b128 reads spread over all banks)
constexpr int kLArr = 128 * kLPitch;              // bytes of one operand array tile (128 rows)

template <class E> struct LinElem;
template <> struct LinElem<__bf16> {
    typedef __bf16 frag __attribute__((ext_vector_type(8)));
    static __device__ inline floatx16 mfma(frag a, frag b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct LinElem<_Float16> {
    typedef _Float16 frag __attribute__((ext_vector_type(8)));
    static __device__ inline floatx16 mfma(frag a, frag b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

template <class E>
__device__ inline unsigned pack2e(E a, E b) {
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}
// 8 fp32 values -> 8 elements hi = E(x) and (LO) 8 elements lo = E(x - hi), 16 bytes each
template <class E, bool LO>
__device__ inline void prepare8(floatx4 x0, floatx4 x1, uint4& hi, uint4& lo) {
    E h[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? x0[e] : x1[e - 4];
        h[e] = (E)x;
        if (LO) l[e] = (E)(x - (float)h[e]);
    }
    hi = make_uint4(pack2e(h[0], h[1]), pack2e(h[2], h[3]), pack2e(h[4], h[5]), pack2e(h[6], h[7]));
    if (LO) lo = make_uint4(pack2e(l[0], l[1]), pack2e(l[2], l[3]), pack2e(l[4], l[5]), pack2e(l[6], l[7]));
}
}  // namespace

// ------------------------------------------------------------------------------------------------------
// 128 x 128 x 64 tiles, 4 waves as 2 x 2, register prefetch of the next k-tile: split_gemm_kernel's shape with the A operand
// staged as fp32 (32 floats per thread and k-tile) and prepared between the registers and LDS -- no activation plane in global
// memory, no launch beside the GEMM's own.  One tile shape and one k order whatever M is, no split-K, rows at or beyond M and
// weight rows at or beyond N read as zeros: row m of C depends on row m of x and on W alone.
// ------------------------------------------------------------------------------------------------------
template <class E, int NPROD>
__global__ __launch_bounds__(256) void linear_gemm_kernel(LinearGemm g) {
    constexpr bool LO = NPROD == 3;
    constexpr int NA = LO ? 2 : 1;                // arrays per operand: hi (, lo)
    typedef typename LinElem<E>::frag frag;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware tile order, as in split_gemm_kernel, but n fastest: the ids one XCD receives are a contiguous run of the (n fastest,
    // then m) order.  Here the big operand is A (fp32, thousands of rows, read by every one of the N / 128 column tiles) and the
    // weight planes are a few MB: the column tiles of one block of rows are resident on one XCD and the block reaches that L2 once.
    int bx, by;
    {
        const unsigned nwg = gridDim.x * gridDim.y;
        const unsigned orig = blockIdx.x + gridDim.x * blockIdx.y;
        const unsigned xcd = orig & 7u, q = nwg >> 3, r = nwg & 7u;            // bijective for any nwg
        const unsigned v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        by = (int)(v % gridDim.y);
        bx = (int)(v / gridDim.y);
    }
    const int m0 = bx * 128, n0 = by * 128;
    const int ntiles = g.K / kLBK;

    // staging: thread -> (row = tid >> 1, one half of the row's k-tile segment)
    const int row = tid >> 1, half = tid & 1;
    const bool a_ok = m0 + row < g.M, b_ok = n0 + row < g.N;
    const floatx4* srcA = reinterpret_cast<const floatx4*>(g.A + (long)(m0 + row) * g.lda + half * (kLBK / 2));
    const long b_off = (long)(n0 + row) * g.ldb + half * (kLBK / 2);
    const uint4* srcB[2] = {reinterpret_cast<const uint4*>(static_cast<const E*>(g.B_hi) + b_off),
                            reinterpret_cast<const uint4*>(static_cast<const E*>(LO ? g.B_lo : g.B_hi) + b_off)};
    floatx4 ra[kLBK / 8];
    uint4 rb[NA][kLBK / 16];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int v = 0; v < kLBK / 8; ++v) ra[v] = a_ok ? srcA[t * (kLBK / 4) + v] : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int v = 0; v < kLBK / 16; ++v) rb[a][v] = b_ok ? srcB[a][t * (kLBK / 8) + v] : make_uint4(0u, 0u, 0u, 0u);
    };
    auto store_tile = [&]() {
        unsigned char* dst = smem + row * kLPitch + half * kLBK;
#pragma unroll
        for (int v = 0; v < kLBK / 16; ++v) {
            uint4 hi, lo;
            prepare8<E, LO>(ra[2 * v], ra[2 * v + 1], hi, lo);
            *reinterpret_cast<uint4*>(dst + v * 16) = hi;
            if (LO) *reinterpret_cast<uint4*>(dst + kLArr + v * 16) = lo;
#pragma unroll
            for (int a = 0; a < NA; ++a) *reinterpret_cast<uint4*>(dst + (NA + a) * kLArr + v * 16) = rb[a][v];
        }
    };

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int li = lane & 31, kh = lane >> 5;
    if (ntiles > 0) load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t + 1);
#pragma unroll
        for (int ks = 0; ks < kLBK / 16; ++ks) {
            frag ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int off = (wm * 64 + i * 32 + li) * kLPitch + ks * 32 + kh * 16;
                ah[i] = *reinterpret_cast<const frag*>(smem + off);
                if (LO) al[i] = *reinterpret_cast<const frag*>(smem + kLArr + off);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int off = (wn * 64 + j * 32 + li) * kLPitch + ks * 32 + kh * 16;
                bh[j] = *reinterpret_cast<const frag*>(smem + NA * kLArr + off);
                if (LO) bl[j] = *reinterpret_cast<const frag*>(smem + (NA + 1) * kLArr + off);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (LO) acc[i][j] = LinElem<E>::mfma(al[i], bh[j], acc[i][j]);
                    if (LO) acc[i][j] = LinElem<E>::mfma(ah[i], bl[j], acc[i][j]);
                    acc[i][j] = LinElem<E>::mfma(ah[i], bh[j], acc[i][j]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int o = n0 + wn * 64 + j * 32 + li;
                if (m < g.M && o < g.N) g.C[(long)m * g.ldc + o] = acc[i][j][r];
            }
}

hipError_t launch_linear_gemm(const LinearGemm& g, int mode, hipStream_t stream) {
    if (mode != 1 && mode != 2) return hipErrorInvalidValue;
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    if (g.K <= 0 || g.K % kLBK || g.lda % 4 || g.ldb % 8 || !g.A || !g.B_hi || !g.C || (mode == 1 && !g.B_lo)) return hipErrorInvalidValue;
    {                                                   // the split form's four tiles (73.7 KB) live in dynamic LDS
        static bool attr_set = false;
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(linear_gemm_kernel<__bf16, 3>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
    }
    const dim3 grid((g.M + 127) / 128, (g.N + 127) / 128);
    if (mode == 1) INFV_LAUNCH((linear_gemm_kernel<__bf16, 3>), grid, dim3(256), 4 * kLArr, stream, g);
    else INFV_LAUNCH((linear_gemm_kernel<_Float16, 1>), grid, dim3(256), 2 * kLArr, stream, g);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// x [rows][cols] fp32 (leading dimension ld_in) -> out [rows][cols] fp16, round to nearest even (leading dimension ld_out): the
// fp16 sibling of launch_split_rows, for the weight planes
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void round_rows_f16_kernel(const float* __restrict__ x, long ld_in, long rows, int cols4,
                                                             _Float16* __restrict__ out, long ld_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols4) return;
    const long r = i / cols4;
    const int c = (int)(i - r * cols4) * 4;
    const floatx4 v = *reinterpret_cast<const floatx4*>(x + r * ld_in + c);
    *reinterpret_cast<uint2*>(out + r * ld_out + c) =
        make_uint2(pack2e((_Float16)v[0], (_Float16)v[1]), pack2e((_Float16)v[2], (_Float16)v[3]));
}

hipError_t launch_round_rows_f16(const float* x, long ld_in, long rows, int cols, void* out, long ld_out, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (cols % 4 || ld_in % 4 || ld_out % 4) return hipErrorInvalidValue;
    const long n = rows * (cols / 4);
    INFV_LAUNCH(round_rows_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, ld_in, rows, cols / 4,
                static_cast<_Float16*>(out), ld_out);
    return hipGetLastError();
}

}  // namespace infv
