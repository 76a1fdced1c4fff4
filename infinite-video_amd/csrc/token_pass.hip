// The token side of the split-bf16 contractions (split_gemm.hip) for gfx950: what stands between the frame tokens as the producer
// stores them -- fp32, bf16, fp16 or fp8 e4m3, with or without the vision LayerNorm -- and the bf16 hi / lo planes the GEMMs read.
//   the token pass        F [n][d] -> F_hi / F_lo [n][d], FT_hi / FT_lo [d][n] and the frame means, 64 x 64 tiles through LDS;
//                         plain, with the LayerNorm applied on load, and padded (frames of 257 tokens); the padded stages with
//                         another output policy also write the fp16 plane and its transpose for attention_f16.hip
//   the upcasts           tokens -> an fp32 copy, where the split path does not apply
//   the LayerNorm pieces  token_ln_stats_kernel, ln_tokens_kernel
//   the row softmax       fp32 scores -> split bf16 P_hi / P_lo, whole rows and padded rows
// Every kernel is a few lines over `__device__ __forceinline__` stages written once: the fill of the tile, tile -> transposed
// planes, the frame means, the two softmax bodies.
#include "vqf_internal.h"
#include "ltm_device.h"

#include <type_traits>

namespace infv {

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------------
// Frame tokens of a chunk, both ways round:  F [n][d] ->  F_hi/F_lo [n][d]   (B operand of the score contraction)
//                                                        FT_hi/FT_lo [d][n]  (B operand of the token-mean contraction)
// 64 x 64 tiles through LDS; grid (n / 64, d / 64, chunks).  The tile is kept as fp32, 65 words a row, whatever the token type
// (bf16 tokens alone keep it packed, see transpose_bf16_kernel).
// ------------------------------------------------------------------------------------------------------
typedef float TokenTile[64][65];

// What the stages store from an fp32 tile value: the element type of the planes and the conversion.  SplitBf16 (the default of
// every stage) is the split-bf16 contractions' hi = bf16(x), lo = bf16(x - hi); RoundF16 is the fp16 attention's single plane,
// fp16(x) to nearest even (beyond 65504: inf), which has no lo piece.
struct SplitBf16 {
    typedef __bf16 elem;
    static constexpr bool kHasLo = true;
    static __device__ __forceinline__ void cvt(float x, __bf16& hi, __bf16& lo) { split2(x, hi, lo); }
};
struct RoundF16 {
    typedef _Float16 elem;
    static constexpr bool kHasLo = false;
    static __device__ __forceinline__ void cvt(float x, _Float16& hi, _Float16& lo) { hi = (_Float16)x; lo = (_Float16)0.f; }
};
__device__ inline unsigned pack2(_Float16 a, _Float16 b) {
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}

// Fill stage, 4 columns per thread: load the rows r0 + r < n of the tile at (r0, c0) of chunk blockIdx.z from the source F
// (n rows a chunk), widen, apply the LayerNorm (LN: stats [chunks * n] addresses the launch's first chunk), split, store
// F_hi / F_lo (`ld` rows a chunk), fill the tile.  Rows at or beyond n are zeros in the tile.  The source is read inside ONE token
// row (d % 64 == 0: no load straddles a row).
// PAD = false: ld == n; rows at or beyond n are not stored, both planes are.
// PAD = true: ld == n_pad; every row of the tile is stored, pad rows as zeros (r0 + r < n_pad), and the last tile of a frame never
// touches the next frame's first rows or the bytes behind the buffer -- the row test predicates the load alone.  Whether a tile is
// the partial one is uniform over the workgroup (blockIdx.x).  Fl == nullptr (bf16 / fp8 tokens without LayerNorm: the value is its
// own hi piece, lo is exactly 0): the lo plane is not written.
template <class Tok, bool LN, bool PAD, class Out = SplitBf16>
__device__ __forceinline__ void tile_fill4(TokenTile& tile, const void* __restrict__ F, int n, int ld, int d,
                                           const float2* __restrict__ stats, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, typename Out::elem* __restrict__ Fh,
                                           typename Out::elem* __restrict__ Fl) {
    typedef typename Tok::vec tvec;
    typedef typename Out::elem oelem;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long cin = (long)blockIdx.z * n * d, cout = (long)blockIdx.z * ld * d;     // the chunk's first element in F, in the planes
    const tvec* src = reinterpret_cast<const tvec*>(F);
    // (the compile-time halves of the two store rules)
    auto stored = [&](int r) { if constexpr (PAD) return true; else return r0 + r < n; };
    auto has_lo = [&](const oelem* lo) { if constexpr (!Out::kHasLo) return false; else if constexpr (PAD) return lo != nullptr; else return true; };
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int e = tid + 256 * p;                 // 1024 groups of 4 columns
        const int r = e >> 4, c4 = (e & 15) * 4;
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < n) {
            v = Tok::widen(src[(cin + (long)(r0 + r) * d + c0 + c4) >> 2]);
            if constexpr (LN)
                v = token_ln4(v, stats[(long)blockIdx.z * n + r0 + r], *reinterpret_cast<const floatx4*>(gamma + c0 + c4),
                              *reinterpret_cast<const floatx4*>(beta + c0 + c4));
        }
        oelem h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { Out::cvt(v[k], h[k], l[k]); tile[r][c4 + k] = v[k]; }
        if (stored(r)) {
            const long o = cout + (long)(r0 + r) * d + c0 + c4;
            *reinterpret_cast<uint2*>(Fh + o) = make_uint2(pack2(h[0], h[1]), pack2(h[2], h[3]));
            if (has_lo(Fl)) *reinterpret_cast<uint2*>(Fl + o) = make_uint2(pack2(l[0], l[1]), pack2(l[2], l[3]));
        }
    }
}

// Tile -> transposed planes FT_hi / FT_lo [d][ld] of the chunk whose first element is `cb`: row = column c of the tile, TPT (4 or
// 8) consecutive tokens per thread, one 8- or 16-byte store a plane (n % TPT == 0: a multiple of 32).  LO = false (fp8: no lo
// plane exists): FT_hi alone.  PAD as in the fill: every row is stored and Tl == nullptr skips the lo plane.
// ds_write_b32 / ds_read_b32 are served per 32-lane half over 32 banks.  With 8 tokens per thread a half writes 4 rows x 8 column
// groups at banks (r + 8 j + k) % 32 and reads 4 columns x 8 row groups at (8 i + k + c) % 32 -- 16 distinct banks, each twice: the
// 2-way pattern of the 4-wide fp32 pass in both directions (not measured with the conflict counter; the pass is bound by its
// global traffic).
template <int TPT, bool LO, bool PAD, class Out = SplitBf16>
__device__ __forceinline__ void tile_to_planes(const TokenTile& tile, long cb, int n, int ld, typename Out::elem* __restrict__ Th,
                                               typename Out::elem* __restrict__ Tl) {
    static_assert(!LO || Out::kHasLo, "no lo plane of this element type");
    static_assert(TPT == 4 || TPT == 8, "8- or 16-byte stores");
    constexpr int SH = TPT == 4 ? 4 : 3;             // 64 / TPT = 1 << SH threads along the tokens of one column
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    auto stored = [&](int rt) { if constexpr (PAD) return true; else return r0 + rt < n; };
    auto has_lo = [&]() { if constexpr (!LO) return false; else if constexpr (PAD) return Tl != nullptr; else return true; };
#pragma unroll
    for (int p = 0; p < 16 / TPT; ++p) {
        const int e = tid + 256 * p;
        const int c = e >> SH, rt = (e & ((1 << SH) - 1)) * TPT;
        if (stored(rt)) {
            typename Out::elem h[TPT], l[TPT];
#pragma unroll
            for (int k = 0; k < TPT; ++k) Out::cvt(tile[rt + k][c], h[k], l[k]);
            const long o = cb + (long)(c0 + c) * ld + r0 + rt;
            if constexpr (TPT == 4) {
                *reinterpret_cast<uint2*>(Th + o) = make_uint2(pack2(h[0], h[1]), pack2(h[2], h[3]));
                if (has_lo()) *reinterpret_cast<uint2*>(Tl + o) = make_uint2(pack2(l[0], l[1]), pack2(l[2], l[3]));
            } else {
                *reinterpret_cast<uint4*>(Th + o) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
                if (has_lo()) *reinterpret_cast<uint4*>(Tl + o) = make_uint4(pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7]));
            }
        }
    }
}

// The frame means kbar[chunk][n / P][d] (the long-term memory's pooled frames, Qformer.py:236) from the same tile: P divides 64,
// so a tile holds 64 / P whole frames; their P tokens are summed in token order and divided by P exactly as pool_frames_kernel
// does, so the two agree bit for bit -- for every token type, on the same values -- and the frame tokens are read once.
// `at(row, col)` reads the tile as fp32.
template <class At>
__device__ __forceinline__ void tile_frame_means(At at, int n, int d, float* __restrict__ kbar, int P) {
    if (kbar) {
        const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
        const int fpt = 64 / P;                      // frames per tile
        for (int e = threadIdx.x; e < fpt * 64; e += 256) {
            const int f = e >> 6, c = e & 63;
            if (r0 + (f + 1) * P <= n) {
                float acc = 0.f;
                for (int p = 0; p < P; ++p) acc += at(f * P + p, c);
                kbar[((long)blockIdx.z * (n / P) + r0 / P + f) * d + c0 + c] = acc / (float)P;
            }
        }
    }
}
struct TileAt {
    const TokenTile& tile;
    __device__ float operator()(int r, int c) const { return tile[r][c]; }
};

// fp32 tokens.  With kbar != nullptr the same pass also writes the frame means.
__global__ __launch_bounds__(256) void split_transpose_kernel(const float* __restrict__ F, int n, int d,
                                                              __bf16* __restrict__ Fh, __bf16* __restrict__ Fl,
                                                              __bf16* __restrict__ Th, __bf16* __restrict__ Tl,
                                                              float* __restrict__ kbar, int P) {
    __shared__ TokenTile tile;
    tile_fill4<TokF32, false, false>(tile, F, n, n, d, nullptr, nullptr, nullptr, Fh, Fl);
    __syncthreads();
    tile_to_planes<4, true, false>(tile, (long)blockIdx.z * n * d, n, n, Th, Tl);
    tile_frame_means(TileAt{tile}, n, d, kbar, P);
}

// fp16 tokens (what the reference's fp16 producer holds): F [n][d] read at 2 bytes per element in 16-byte vectors of 8.  An fp16
// value is exact in fp32 and split2() is the function the fp32 pass applies, so F_hi / F_lo, FT_hi / FT_lo and the frame means are
// the fp32 pass's bits on the same values (hi + lo is the token exactly: 11 significand bits = 8 + 3).  Stores are 16 bytes of 8 bf16.
__global__ __launch_bounds__(256) void split_transpose_f16_kernel(const _Float16* __restrict__ F, int n, int d,
                                                                  __bf16* __restrict__ Fh, __bf16* __restrict__ Fl,
                                                                  __bf16* __restrict__ Th, __bf16* __restrict__ Tl,
                                                                  float* __restrict__ kbar, int P) {
    __shared__ TokenTile tile;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long cb = (long)blockIdx.z * n * d;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = tid + 256 * p;                 // 512 vectors of 8 fp16
        const int r = e >> 3, c8 = (e & 7) * 8;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < n) raw = *reinterpret_cast<const uint4*>(F + cb + (long)(r0 + r) * d + c0 + c8);
        const halfx8 v = __builtin_bit_cast(halfx8, raw);
        __bf16 h[8], l[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float x = (float)v[k]; split2(x, h[k], l[k]); tile[r][c8 + k] = x; }
        if (r0 + r < n) {
            const long o = cb + (long)(r0 + r) * d + c0 + c8;
            *reinterpret_cast<uint4*>(Fh + o) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
            *reinterpret_cast<uint4*>(Fl + o) = make_uint4(pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7]));
        }
    }
    __syncthreads();
    tile_to_planes<8, true, false>(tile, cb, n, n, Th, Tl);
    tile_frame_means(TileAt{tile}, n, d, kbar, P);
}

// fp8 e4m3 tokens (a storage format the caller chose): F [n][d] at 1 byte per element, read in 16-byte vectors of 16.  An e4m3 value
// widens exactly to fp32 (widen_f8x4, ltm_device.h) and is exactly its own bf16 hi piece with a zero lo piece (4 significand bits),
// so only the hi planes exist: F_hi [n][d] (the B operand of the score contraction: the caller's buffer holds no bf16) and
// FT_hi [d][n]; both contractions then run their two-product form, as for bf16 tokens, bit for bit the three-product run on the
// same values.  The frame means come from the widened fp32 tile as in the fp32 pass; the transposed half is the fp16 pass's.
__global__ __launch_bounds__(256) void split_transpose_f8_kernel(const unsigned char* __restrict__ F, int n, int d,
                                                                 __bf16* __restrict__ Fh, __bf16* __restrict__ Th,
                                                                 float* __restrict__ kbar, int P) {
    __shared__ TokenTile tile;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long cb = (long)blockIdx.z * n * d;
    {
        const int r = tid >> 2, c16 = (tid & 3) * 16;     // 256 vectors of 16 fp8
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < n) raw = *reinterpret_cast<const uint4*>(F + cb + (long)(r0 + r) * d + c0 + c16);
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
        unsigned h2[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const floatx4 x = widen_f8x4(w[q]);
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[r][c16 + 4 * q + k] = x[k];
            h2[2 * q] = pack2((__bf16)x[0], (__bf16)x[1]);
            h2[2 * q + 1] = pack2((__bf16)x[2], (__bf16)x[3]);
        }
        if (r0 + r < n) {
            uint4* dst = reinterpret_cast<uint4*>(Fh + cb + (long)(r0 + r) * d + c0 + c16);
            dst[0] = make_uint4(h2[0], h2[1], h2[2], h2[3]);
            dst[1] = make_uint4(h2[4], h2[5], h2[6], h2[7]);
        }
    }
    __syncthreads();
    tile_to_planes<8, false, false>(tile, cb, n, n, Th, nullptr);
    tile_frame_means(TileAt{tile}, n, d, kbar, P);
}

// bf16 tokens: F [n][d] bf16 is the score contraction's B operand as it stands (hi = the token, lo = 0 exactly), so only
// FT_hi [d][n] is written -- and the frame means.  16-byte loads and stores of 8 bf16.  The tile stays packed: LDS rows are 66 bf16
// (33 words) apart, so the transposed read of a wave (8 columns x 8 row groups) touches 32 distinct banks.
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const __bf16* __restrict__ F, int n, int d, __bf16* __restrict__ Th,
                                                             float* __restrict__ kbar, int P) {
    __shared__ unsigned tile[64 * 33];               // [64 tokens][66 bf16]
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long cb = (long)blockIdx.z * n * d;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = tid + 256 * p;                 // 512 vectors of 8 bf16
        const int r = e >> 3, c8 = (e & 7) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < n) v = *reinterpret_cast<const uint4*>(F + cb + (long)(r0 + r) * d + c0 + c8);
        unsigned* t = tile + r * 33 + (c8 >> 1);
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
    __syncthreads();
    const unsigned short* th = reinterpret_cast<const unsigned short*>(tile);
    // transposed: row = column c of the tile, 8 consecutive tokens per thread
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = tid + 256 * p;
        const int c = e >> 3, r8 = (e & 7) * 8;
        if (r0 + r8 < n) {                           // n % 8 == 0 (multiple of 32)
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (unsigned)th[(r8 + 2 * k) * 66 + c] | ((unsigned)th[(r8 + 2 * k + 1) * 66 + c] << 16);
            *reinterpret_cast<uint4*>(Th + cb + (long)(c0 + c) * n + r0 + r8) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    tile_frame_means([&](int r, int c) { return __uint_as_float((unsigned)th[r * 66 + c] << 16); }, n, d, kbar, P);
}

// The token pass of `nb` <= 32768 chunks (grid.z) for any token type: the launch prepare_split issues.  kbar != nullptr needs
// token_pass_gives_means(P): a frame that divides the 64-token tile.  (A per-frame form for P = 196 -- one workgroup per frame,
// slab and chunk, the column sums kept in registers across sub-tiles -- was measured at 128 eval-shape chunks and lost to pooling
// + this pass for fp16 and bf16 tokens alike, profiles/vc_half_tokens.jsonl; it is gone.)  bf16: Fh / Fl / Tl are not written;
// fp8: Fl / Tl are not written.
bool token_pass_gives_means(int P) { return P >= 1 && 64 % P == 0; }

hipError_t launch_token_pass(const void* F, tok_code tok, int nb, int n, int d, void* Fh_, void* Fl_, void* Th_, void* Tl_,
                             hipStream_t stream, float* kbar, int P) {
    if (n % 32 || d % 64) return hipErrorInvalidValue;
    if (kbar && (!token_pass_gives_means(P) || n % P)) return hipErrorInvalidValue;
    const dim3 grid((n + 63) / 64, d / 64, nb);
    __bf16 *Fh = static_cast<__bf16*>(Fh_), *Fl = static_cast<__bf16*>(Fl_), *Th = static_cast<__bf16*>(Th_), *Tl = static_cast<__bf16*>(Tl_);
    switch (tok) {                                   // (kernels of their own names and argument lists: a value may be its own hi piece)
        case INFV_TOKENS_F32: INFV_LAUNCH(split_transpose_kernel, grid, dim3(256), 0, stream, static_cast<const float*>(F), n, d, Fh, Fl, Th, Tl, kbar, P); break;
        case INFV_TOKENS_F16: INFV_LAUNCH(split_transpose_f16_kernel, grid, dim3(256), 0, stream, static_cast<const _Float16*>(F), n, d, Fh, Fl, Th, Tl, kbar, P); break;
        case INFV_TOKENS_BF16: INFV_LAUNCH(transpose_bf16_kernel, grid, dim3(256), 0, stream, static_cast<const __bf16*>(F), n, d, Th, kbar, P); break;
        case INFV_TOKENS_F8E4M3:
            if (!Fh || !Th) return hipErrorInvalidValue;
            INFV_LAUNCH(split_transpose_f8_kernel, grid, dim3(256), 0, stream, static_cast<const unsigned char*>(F), n, d, Fh, Th, kbar, P);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// Tokens -> an fp32 copy, exact: bf16 / fp16 / fp8 tokens where the split path does not apply run the fp32 kernels from this copy.
// x [n] -> y [n] fp32, 16 bytes of x per thread: n % 8 == 0 (bf16, fp16), n % 16 == 0 (fp8).
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void upcast_bf16_kernel(const __bf16* __restrict__ x, float* __restrict__ y, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const uint4 v = reinterpret_cast<const uint4*>(x)[i];
    floatx4 a = {__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u)};
    floatx4 b = {__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u), __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u)};
    reinterpret_cast<floatx4*>(y)[2 * i] = a;
    reinterpret_cast<floatx4*>(y)[2 * i + 1] = b;
}

__global__ __launch_bounds__(256) void upcast_f16_kernel(const _Float16* __restrict__ x, float* __restrict__ y, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const halfx8 v = __builtin_bit_cast(halfx8, reinterpret_cast<const uint4*>(x)[i]);
    floatx4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    floatx4 b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
    reinterpret_cast<floatx4*>(y)[2 * i] = a;
    reinterpret_cast<floatx4*>(y)[2 * i + 1] = b;
}

__global__ __launch_bounds__(256) void upcast_f8_kernel(const unsigned char* __restrict__ x, float* __restrict__ y, long n16) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const uint4 v = reinterpret_cast<const uint4*>(x)[i];
    floatx4* dst = reinterpret_cast<floatx4*>(y) + 4 * i;
    dst[0] = widen_f8x4(v.x); dst[1] = widen_f8x4(v.y); dst[2] = widen_f8x4(v.z); dst[3] = widen_f8x4(v.w);
}

// (the kernel of a token type, the type of its source pointer and the elements one of its threads converts)
template <class Tok> struct UpcastFn;
template <> struct UpcastFn<TokBF16> { typedef __bf16 elem; static constexpr int per = 8; static auto get() { return upcast_bf16_kernel; } };
template <> struct UpcastFn<TokF16> { typedef _Float16 elem; static constexpr int per = 8; static auto get() { return upcast_f16_kernel; } };
template <> struct UpcastFn<TokF8> { typedef unsigned char elem; static constexpr int per = 16; static auto get() { return upcast_f8_kernel; } };

hipError_t launch_upcast(const void* x, tok_code tok, float* y, long n, hipStream_t stream) {
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if constexpr (std::is_same<Tok, TokF32>::value) {
            return hipErrorInvalidValue;             // (fp32 tokens are their own copy: no caller asks)
        } else {
            typedef UpcastFn<Tok> Up;
            if (n <= 0) return hipSuccess;
            if (n % Up::per) return hipErrorInvalidValue;
            for (long o = 0; o < n; o += (1l << 33)) {          // (grid.x limit)
                const long m = n - o < (1l << 33) ? n - o : (1l << 33);
                INFV_LAUNCH(Up::get(), dim3((unsigned)((m / Up::per + 255) / 256)), dim3(256), 0, stream,
                            static_cast<const typename Up::elem*>(x) + o, y + o, m / Up::per);
            }
            return hipGetLastError();
        }
    });
}

// ------------------------------------------------------------------------------------------------------
// The vision LayerNorm of the frame tokens (videochat2_it_mistral.py:195: nn.LayerNorm(width, eps = 1e-12) between the vision
// encoder's fp16 output and the Q-former), applied while the tokens are read at their own dtype -- no fp32 copy of them.
//   token_ln_stats_kernel   (mean, 1 / sqrt(var + eps)) per token row, 8 bytes per token
//   ln_tokens_kernel        y = token_ln(x) as an fp32 tensor: the reference form of the bits, and the fallback where the split path
//                           does not apply (as upcast_f16_kernel / upcast_bf16_kernel are for plain tokens)
//   split_transpose_ln_kernel   split_transpose_kernel's stages over y computed on load (the pooling form is in ltm_kernels.hip)
// Every consumer calls token_ln() of ltm_device.h on values widened exactly, so all of them see the bits ln_tokens_kernel writes.
// ------------------------------------------------------------------------------------------------------
// One wave per token row: the row is read once into registers (NV float4 per lane, lanes beyond the row idle), the mean is a
// fixed-order reduction (per lane in column order, then an xor butterfly over the wave) divided by d, the variance a second
// reduction of (x - mean)^2 from the registers (two-pass, biased, as nn.LayerNorm).  No atomics; the order does not depend on the grid.
template <class Tok, int NV>
__global__ __launch_bounds__(256) void token_ln_stats_kernel(const void* __restrict__ F, long n_rows, int d4, float eps,
                                                             float2* __restrict__ stats) {
    typedef typename Tok::vec tvec;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const tvec* src = reinterpret_cast<const tvec*>(F) + row * d4;
    floatx4 x[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        x[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (lane + 64 * i < d4) x[i] = Tok::widen(src[lane + 64 * i]);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (x[i].x + x[i].y) + (x[i].z + x[i].w);      // (idle slots hold zeros)
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float mu = s / (float)(4 * d4);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (lane + 64 * i < d4) {
            const floatx4 dx = x[i] - mu;
            q += (dx.x * dx.x + dx.y * dx.y) + (dx.z * dx.z + dx.w * dx.w);
        }
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float var = q / (float)(4 * d4);
    if (lane == 0) stats[row] = make_float2(mu, 1.0f / sqrtf(var + eps));
}

hipError_t launch_token_ln_stats(const void* F, tok_code tok, long n_rows, int d, float eps, void* stats, hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    if (d < 64 || d % 64 || d > kTokenLnMaxWidth || (n_rows + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    float2* st = static_cast<float2*>(stats);
    const int d4 = d / 4;
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if constexpr (kTokHasLn<Tok>) {
            if (d4 <= 64) INFV_LAUNCH((token_ln_stats_kernel<Tok, 1>), grid, dim3(256), 0, stream, F, n_rows, d4, eps, st);
            else if (d4 <= 256) INFV_LAUNCH((token_ln_stats_kernel<Tok, 4>), grid, dim3(256), 0, stream, F, n_rows, d4, eps, st);
            else INFV_LAUNCH((token_ln_stats_kernel<Tok, 16>), grid, dim3(256), 0, stream, F, n_rows, d4, eps, st);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    });
}

template <class Tok>
__global__ __launch_bounds__(256) void ln_tokens_kernel(const void* __restrict__ F, long n_vec, int d4, const float2* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const long row = i / d4;
    const int c4 = (int)(i - row * d4);
    const floatx4 x = Tok::widen(reinterpret_cast<const typename Tok::vec*>(F)[i]);
    reinterpret_cast<floatx4*>(y)[i] = token_ln4(x, stats[row], reinterpret_cast<const floatx4*>(gamma)[c4],
                                                 reinterpret_cast<const floatx4*>(beta)[c4]);
}

hipError_t launch_ln_tokens(const void* F, tok_code tok, long n_rows, int d, const void* stats, const float* gamma, const float* beta,
                            float* y, hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    if (d < 64 || d % 64) return hipErrorInvalidValue;
    const int d4 = d / 4;
    const long step = 0x7fffffffL * 256 / d4;           // rows per launch (grid.x limit)
    const float2* st = static_cast<const float2*>(stats);
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if constexpr (kTokHasLn<Tok>) {
            for (long r0 = 0; r0 < n_rows; r0 += step) {
                const long m = n_rows - r0 < step ? n_rows - r0 : step;
                const long n_vec = m * d4;
                const void* src = static_cast<const char*>(F) + r0 * d * (long)token_bytes(tok);
                INFV_LAUNCH(ln_tokens_kernel<Tok>, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, stream, src, n_vec, d4, st + r0,
                            gamma, beta, y + r0 * d);
            }
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    });
}

// split_transpose_kernel over y = token_ln(F): F [n][d] of the token type is read once (4 columns per thread), normalised on load
// into the tile and from there everything is the fp32 pass's -- F_hi / F_lo, FT_hi / FT_lo and, with kbar, the frame means in token
// order.  A normalised value is a general fp32 number, so every token type writes all four planes.
// stats [chunks * n] addresses the launch's first chunk.
template <class Tok>
__global__ __launch_bounds__(256) void split_transpose_ln_kernel(const void* __restrict__ F, int n, int d, const float2* __restrict__ stats,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 __bf16* __restrict__ Fh, __bf16* __restrict__ Fl,
                                                                 __bf16* __restrict__ Th, __bf16* __restrict__ Tl,
                                                                 float* __restrict__ kbar, int P) {
    __shared__ TokenTile tile;
    tile_fill4<Tok, true, false>(tile, F, n, n, d, stats, gamma, beta, Fh, Fl);
    __syncthreads();
    tile_to_planes<4, true, false>(tile, (long)blockIdx.z * n * d, n, n, Th, Tl);
    tile_frame_means(TileAt{tile}, n, d, kbar, P);
}

hipError_t launch_token_pass_ln(const void* F, tok_code tok, int nb, int n, int d, const void* stats, const float* gamma,
                                const float* beta, void* Fh_, void* Fl_, void* Th_, void* Tl_, hipStream_t stream, float* kbar, int P) {
    if (nb <= 0) return hipSuccess;
    if (n % 32 || d % 64 || nb > 32768) return hipErrorInvalidValue;
    if (kbar && (!token_pass_gives_means(P) || n % P)) return hipErrorInvalidValue;
    const dim3 grid((n + 63) / 64, d / 64, nb);
    const float2* st = static_cast<const float2*>(stats);
    __bf16 *Fh = static_cast<__bf16*>(Fh_), *Fl = static_cast<__bf16*>(Fl_), *Th = static_cast<__bf16*>(Th_), *Tl = static_cast<__bf16*>(Tl_);
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if constexpr (kTokHasLn<Tok>) {
            INFV_LAUNCH(split_transpose_ln_kernel<Tok>, grid, dim3(256), 0, stream, F, n, d, st, gamma, beta, Fh, Fl, Th, Tl, kbar, P);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    });
}

// ------------------------------------------------------------------------------------------------------
// The padded forms of the token pass and the row softmax (infv_vqf_encode_frames): a frame of n tokens where n is no multiple of
// 64 -- a ViT hands over 257 = class token + 16 x 16 patches.  The contractions need K and the leading dimensions in multiples of
// 64, so the planes are kept at n_pad = ceil(n / 64) * 64 tokens per frame: F_hi / F_lo [.][n_pad][d], FT_hi / FT_lo [.][d][n_pad],
// rows at or beyond n exact zeros.  The softmax gives the pad keys no mass (exact zeros in P_hi / P_lo), so the context
// contraction over K = n_pad adds exact zeros.  n % 64 == 0 never comes here: it takes the unpadded kernels, launch for launch.
// ------------------------------------------------------------------------------------------------------
// split_transpose_kernel / split_transpose_ln_kernel for any token type with the source at n tokens per frame and the planes at
// n_pad: the PAD form of the stages.  Whether a tile is the partial one is uniform over the workgroup (blockIdx.x).
template <class Tok, bool LN>
__global__ __launch_bounds__(256) void token_pass_pad_kernel(const void* __restrict__ F, int n, int n_pad, int d,
                                                             const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, __bf16* __restrict__ Fh,
                                                             __bf16* __restrict__ Fl, __bf16* __restrict__ Th, __bf16* __restrict__ Tl) {
    __shared__ TokenTile tile;
    tile_fill4<Tok, LN, true>(tile, F, n, n_pad, d, stats, gamma, beta, Fh, Fl);     // source: n rows a frame; planes: n_pad
    __syncthreads();
    tile_to_planes<4, true, true>(tile, (long)blockIdx.z * n_pad * d, n, n_pad, Th, Tl);
}

hipError_t launch_token_pass_pad(const void* F, tok_code tok, int nb, int n, int n_pad, int d, const void* stats, const float* gamma,
                                 const float* beta, void* Fh_, void* Fl_, void* Th_, void* Tl_, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    if (n < 1 || n_pad % 64 || n_pad < n || n_pad - n >= 64 || d < 64 || d % 64 || nb > 32768 || !Fh_ || !Th_) return hipErrorInvalidValue;
    if (stats && (!gamma || !beta || tok == INFV_TOKENS_F8E4M3)) return hipErrorInvalidValue;
    const bool own_hi = !stats && (tok == INFV_TOKENS_BF16 || tok == INFV_TOKENS_F8E4M3);   // no lo planes
    if (own_hi ? (Fl_ || Tl_) : (!Fl_ || !Tl_)) return hipErrorInvalidValue;
    const dim3 grid(n_pad / 64, d / 64, nb);
    const float2* st = static_cast<const float2*>(stats);
    __bf16 *Fh = static_cast<__bf16*>(Fh_), *Fl = static_cast<__bf16*>(Fl_), *Th = static_cast<__bf16*>(Th_), *Tl = static_cast<__bf16*>(Tl_);
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if (!st) {
            INFV_LAUNCH((token_pass_pad_kernel<Tok, false>), grid, dim3(256), 0, stream, F, n, n_pad, d, st, gamma, beta, Fh, Fl, Th, Tl);
            return hipGetLastError();
        }
        if constexpr (kTokHasLn<Tok>) {
            INFV_LAUNCH((token_pass_pad_kernel<Tok, true>), grid, dim3(256), 0, stream, F, n, n_pad, d, st, gamma, beta, Fh, Fl, Th, Tl);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    });
}

// ------------------------------------------------------------------------------------------------------
// The fp16 form of the padded pass (infv_vqf_set_attention_precision(h, 1); the consumer is attention_f16.hip): the PAD stages with
// RoundF16 in place of the split -- the same fill (a token type's widen(), token_ln4() where the LayerNorm is on, exactly n rows
// of a frame read), ONE rounding of the fp32 tile value to fp16 on the way out, so every source type gives the bits of its values
// passed as fp32.  Writes X [.][n_pad][d] and XT [.][d][n_pad], rows at or beyond n exact zeros.  n % 64 == 0 comes here too
// (n_pad == n).
// ------------------------------------------------------------------------------------------------------
template <class Tok, bool LN>
__global__ __launch_bounds__(256) void token_pass_f16_kernel(const void* __restrict__ F, int n, int n_pad, int d,
                                                             const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, _Float16* __restrict__ X,
                                                             _Float16* __restrict__ XT) {
    __shared__ TokenTile tile;
    tile_fill4<Tok, LN, true, RoundF16>(tile, F, n, n_pad, d, stats, gamma, beta, X, nullptr);
    __syncthreads();
    tile_to_planes<8, false, true, RoundF16>(tile, (long)blockIdx.z * n_pad * d, n, n_pad, XT, nullptr);
}

hipError_t launch_token_pass_f16(const void* F, tok_code tok, int nb, int n, int n_pad, int d, const void* stats, const float* gamma,
                                 const float* beta, void* X_, void* XT_, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    if (n < 1 || n_pad % 64 || n_pad < n || n_pad - n >= 64 || d < 64 || d % 64 || nb > 32768 || !X_ || !XT_) return hipErrorInvalidValue;
    if (stats && (!gamma || !beta || tok == INFV_TOKENS_F8E4M3)) return hipErrorInvalidValue;
    const dim3 grid(n_pad / 64, d / 64, nb);
    const float2* st = static_cast<const float2*>(stats);
    _Float16 *X = static_cast<_Float16*>(X_), *XT = static_cast<_Float16*>(XT_);
    return with_token_type(tok, [&](auto t) {
        using Tok = decltype(t);
        if (!st) {
            INFV_LAUNCH((token_pass_f16_kernel<Tok, false>), grid, dim3(256), 0, stream, F, n, n_pad, d, st, gamma, beta, X, XT);
            return hipGetLastError();
        }
        if constexpr (kTokHasLn<Tok>) {
            INFV_LAUNCH((token_pass_f16_kernel<Tok, true>), grid, dim3(256), 0, stream, F, n, n_pad, d, st, gamma, beta, X, XT);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    });
}

// ------------------------------------------------------------------------------------------------------
// Row softmax of fp32 scores [n_rows][len] (leading dimension ld), written as split bf16 P_hi / P_lo (ld_out); one workgroup a row.
// PAD: the softmax runs over the first `len` columns of a row of padded length len_pad (len <= len_pad): columns [len, len_pad)
// never enter the max or the sum -- whatever finite or non-finite value they hold -- and are written as exact zeros into P_hi /
// P_lo.  The row is read in 16-byte vectors up to len_pad (inside the row's allocation); the column test selects per element.
// PAD = false: len_pad == len and the column test is not compiled.
// ------------------------------------------------------------------------------------------------------
// Rows of any length in three passes over the row.
template <bool PAD>
__device__ __forceinline__ void softmax_rows_split_body(const float* __restrict__ S, int len, int len_pad, long ld,
                                                        __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    __shared__ float red[4];
    const float* row = S + (long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    auto live = [&](int col) { if constexpr (PAD) return col < len; else return true; };
    float mx = -INFINITY;
    for (int c = tid * 4; c < len_pad; c += 1024) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(row + c);
        if constexpr (PAD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) mx = fmaxf(mx, c + k < len ? v[k] : -INFINITY);
        } else {
            mx = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        }
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = tid * 4; c < len_pad; c += 1024) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(row + c);
        float ex[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ex[k] = live(c + k) ? expf(v[k] - mx) : 0.f;
        sum += (ex[0] + ex[1]) + (ex[2] + ex[3]);
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    __bf16* ph = Ph + (long)blockIdx.x * ld_out;
    __bf16* pl = Pl + (long)blockIdx.x * ld_out;
    for (int c = tid * 4; c < len_pad; c += 1024) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(row + c);
        __bf16 h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split2_mul(live(c + k) ? expf(v[k] - mx) : 0.f, inv, h[k], l[k]);
        *reinterpret_cast<uint2*>(ph + c) = make_uint2(pack2(h[0], h[1]), pack2(h[2], h[3]));
        *reinterpret_cast<uint2*>(pl + c) = make_uint2(pack2(l[0], l[1]), pack2(l[2], l[3]));
    }
}

// The same softmax for rows of up to 1024 * NV floats, each row read ONCE: a thread keeps its NV float4 in registers
// between the max, the sum and the write (same per-thread order of operations as the three-pass body above: same bits).
template <int NV, bool PAD>
__device__ __forceinline__ void softmax_rows_split_reg_body(const float* __restrict__ S, int len, int len_pad, long ld,
                                                            __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    __shared__ float red[4];
    const float* row = S + (long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    auto live = [&](int col) { if constexpr (PAD) return col < len; else return true; };
    floatx4 v[NV];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (c < len_pad) {
            v[i] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(row + c));
            if constexpr (PAD) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[i][k] = c + k < len ? v[i][k] : -INFINITY;
            }
            mx = fmaxf(mx, fmaxf(fmaxf(v[i][0], v[i][1]), fmaxf(v[i][2], v[i][3])));
        }
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (c < len_pad) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[i][k] = live(c + k) ? expf(v[i][k] - mx) : 0.f;
            sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    __bf16* ph = Ph + (long)blockIdx.x * ld_out;
    __bf16* pl = Pl + (long)blockIdx.x * ld_out;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (c < len_pad) {
            __bf16 h[4], l[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split2_mul(v[i][k], inv, h[k], l[k]);
            *reinterpret_cast<uint2*>(ph + c) = make_uint2(pack2(h[0], h[1]), pack2(h[2], h[3]));
            *reinterpret_cast<uint2*>(pl + c) = make_uint2(pack2(l[0], l[1]), pack2(l[2], l[3]));
        }
    }
}

__global__ __launch_bounds__(256) void softmax_rows_split_kernel(const float* __restrict__ S, int len, long ld,
                                                                 __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    softmax_rows_split_body<false>(S, len, len, ld, Ph, Pl, ld_out);
}
template <int NV>
__global__ __launch_bounds__(256) void softmax_rows_split_reg_kernel(const float* __restrict__ S, int len, long ld,
                                                                     __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    softmax_rows_split_reg_body<NV, false>(S, len, len, ld, Ph, Pl, ld_out);
}
template <int NV>
__global__ __launch_bounds__(256) void softmax_rows_split_pad_kernel(const float* __restrict__ S, int len, int len_pad, long ld,
                                                                     __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    softmax_rows_split_reg_body<NV, true>(S, len, len_pad, ld, Ph, Pl, ld_out);
}
// rows beyond 8192 columns
__global__ __launch_bounds__(256) void softmax_rows_split_pad_long_kernel(const float* __restrict__ S, int len, int len_pad, long ld,
                                                                          __bf16* __restrict__ Ph, __bf16* __restrict__ Pl, long ld_out) {
    softmax_rows_split_body<true>(S, len, len_pad, ld, Ph, Pl, ld_out);
}

hipError_t launch_softmax_rows_split(const float* S, long n_rows, int len, long ld, void* Ph_, void* Pl_, long ld_out,
                                     hipStream_t stream) {
    if (len % 4 || ld % 4 || ld_out % 4) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_rows);
    __bf16 *Ph = static_cast<__bf16*>(Ph_), *Pl = static_cast<__bf16*>(Pl_);
    if (len <= 2048) INFV_LAUNCH(softmax_rows_split_reg_kernel<2>, grid, dim3(256), 0, stream, S, len, ld, Ph, Pl, ld_out);
    else if (len <= 8192) INFV_LAUNCH(softmax_rows_split_reg_kernel<8>, grid, dim3(256), 0, stream, S, len, ld, Ph, Pl, ld_out);
    else INFV_LAUNCH(softmax_rows_split_kernel, grid, dim3(256), 0, stream, S, len, ld, Ph, Pl, ld_out);
    return hipGetLastError();
}

hipError_t launch_softmax_rows_split_pad(const float* S, long n_rows, int len, int len_pad, long ld, void* Ph_, void* Pl_, long ld_out,
                                         hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    if (len < 1 || len > len_pad || len_pad % 4 || len_pad > ld || len_pad > ld_out || ld % 4 || ld_out % 4 || n_rows > 0x7fffffffL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_rows);
    __bf16 *Ph = static_cast<__bf16*>(Ph_), *Pl = static_cast<__bf16*>(Pl_);
    if (len_pad <= 2048) INFV_LAUNCH(softmax_rows_split_pad_kernel<2>, grid, dim3(256), 0, stream, S, len, len_pad, ld, Ph, Pl, ld_out);
    else if (len_pad <= 8192) INFV_LAUNCH(softmax_rows_split_pad_kernel<8>, grid, dim3(256), 0, stream, S, len, len_pad, ld, Ph, Pl, ld_out);
    else INFV_LAUNCH(softmax_rows_split_pad_long_kernel, grid, dim3(256), 0, stream, S, len, len_pad, ld, Ph, Pl, ld_out);
    return hipGetLastError();
}

}  // namespace infv
