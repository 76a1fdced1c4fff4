// Internal interface between the video Q-former C ABI (vqf_capi.hip, vqf_video.hip, vqf_vc.hip) and its gfx950 kernels (vqf_kernels.hip).
#pragma once
#include "knobs.h"
#include "../../include/infv_ltm.h"      // tok_code
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace infv {

constexpr int kQfMaxSeg = 4;

// Host-side seams of the layer-major calls (vqf_video.hip, vqf_vc.hip): a large call is cut into pieces of these sizes, each with its own
// offset arithmetic.  tests/golden/seam_cases.py reads them from here.
constexpr int kRowBlockVideo = 64;       // chunks per row block of the query-token GEMMs, infv_vqf_encode_video
constexpr int kRowBlockVideos = 128;     // ... of the batch-invariant calls (infv_vqf_encode_videos, infv_vqf_vc_encode_videos)
constexpr long kTextFfnRows = 16384;     // packed text rows per block of the VideoChat2 text FFN
constexpr long kMergeRows = 32768;       // rows per launch of the alpha-merge epilogue

// C[z][m][o] (+)= sum_k A[b][m][k] * Bop[b][k][o]   for z = b * splitk + s, k in split s.
// The batch index b = bo * inner + bi addresses operands as  X + bi * strideX + bo * strideX2  (inner = 0: one level).
//   NT: Bop[k][o] = B[o][k]  (B rows are output columns; up to kQfMaxSeg row segments of seg_rows rows each)
//   NN: Bop[k][o] = B[k][o]
struct QfGemm {
    const float* A;  long lda;  long strideA;      // per-batch stride (0 = shared)
    const float* B[kQfMaxSeg];  long ldb;  long strideB;  int seg_rows;
    float* C;  long ldc;  long strideC;  long split_stride;
    int M, N, k_per_split, splitk, nbatch;
    int K;                                           // total depth; 0 = splitk * k_per_split (the last split may be shorter)
    int inner;  long strideA2, strideB2, strideC2;   // optional second batch level (zero-initialised = unused)
    int tile;                                        // 0: 128 x 128 tiles where M and N reach 128, else 64 x 64; 64 / 128: that tile
    const int32_t* b_map;                            // device [nbatch] or nullptr: batch entry b reads B at b_map[b] * strideB (one batch level)
};
hipError_t launch_qf_gemm(const QfGemm& g, bool nn, hipStream_t stream);
int qf_pick_splitk(int M, int N, int K, int nbatch);
// split-K that fills whole rounds of the 256 CUs: returns the split count and the (32-aligned) depth per split
int qf_pick_splitk_fill(int M, int N, int K, int nbatch, int* k_per_split);

enum QfAct { QF_ACT_NONE = 0, QF_ACT_GELU = 1 };
// out[m][:] = LN?( scale * act( sum_s parts[s][m][:] + bias ) + res_scale * residual[m % res_rows] )    one workgroup per row
struct QfEpilogue {
    const float* parts;  int nsplit;  long split_stride;  long ld_in;
    const float* bias[kQfMaxSeg];  int seg_cols;               // bias segment s covers columns [s*seg_cols, (s+1)*seg_cols); nullptr = none
    int act;
    float scale, res_scale;                                    // set both to 1 for a plain residual add
    const float* residual;  long ld_res;  int res_rows;        // residual row = m % res_rows (broadcast of a shared [res_rows] block)
    const float* gamma;  const float* beta;  float eps;        // LayerNorm if gamma != nullptr
    float* out;  long ld_out;
    int M, width;
};
hipError_t launch_qf_epilogue(const QfEpilogue& e, hipStream_t stream);

// qkv [nb*Q][3*hidden] (bias applied) -> ctx [nb*Q][hidden]; softmax(q k^T / sqrt(dh)) v per head, Q <= 32, dh = 64
hipError_t launch_qf_self_attention(const float* qkv, int nb, int Q, int H, float* ctx, hipStream_t stream);

// Self-attention over the n_valid[b] <= kVcAttnMaxN query + text tokens of chunk b (VideoChat2), dh = 64.  Row r of chunk b
// lives at row  b * rows0 + r  of qkv0 / ctx0 when r < nsplit, else at row  off1[b] + r - nsplit  of qkv1 / ctx1 (query rows
// in a regular block, text rows packed behind an offset table; nsplit = rows0 = n_max and off1 = nullptr: one padded block).
// qkv rows are [3*hidden] (bias applied), ctx rows [hidden].  Rows [n_valid[b], n_alloc) of the first block are written as
// zeros; keys at or beyond n_valid[b] are never read.  n_valid / off1 are HOST arrays (they travel in kernel arguments).
constexpr int kVcAttnMaxN = 608;
constexpr int kVcAttnGroup = 256;
struct VcAttn {
    const float* qkv0; long rows0; int nsplit; const float* qkv1;
    float* ctx0; float* ctx1;
    int H; int n_alloc;
};
hipError_t launch_qf_vc_self_attention(const VcAttn& a, int nb, const int32_t* n_valid, const int32_t* off1, hipStream_t stream);
// dst rows [dst_row[s], +n_rows[s]) = src rows [src_row[s], +n_rows[s]) for n_segs segments (HOST tables), rows of `width` floats
constexpr int kRowSegs = 128;
hipError_t launch_qf_copy_rows(const float* src, float* dst, const int32_t* dst_row, const int32_t* src_row, const int32_t* n_rows,
                               int n_segs, int width, hipStream_t stream);

// dst[0, n) = tab[0, n): a HOST int32 table written to device memory through kernel arguments (no host buffer outlives the call)
constexpr int kMapChunk = 512;
hipError_t launch_qf_write_map(int32_t* dst, const int32_t* tab, int n, hipStream_t stream);

// qt[b][h*Q + q][j] = sum_e xq[b][q][h*64 + e] / sqrt(64) * Wk[h*64 + e][j]
hipError_t launch_qf_qtilde(const float* xq, int nb, int Q, int H, int d, const float* wk, float* qt, hipStream_t stream);

// in-place softmax of rows [n_rows][len] (leading dimension ld)
hipError_t launch_qf_softmax_rows(float* S, long n_rows, int len, long ld, hipStream_t stream);

// parts[0][i] = sum_s parts[s][i]  (slabs `stride` floats apart, n a multiple of 4)
hipError_t launch_qf_sum_slabs(float* parts, int nsplit, long stride, long n, hipStream_t stream);

// ---- split-bf16 contractions (split_gemm.hip) ----
// C[z][m][o] = sum_k (A_hi + A_lo)[b][m][k] * (B_hi + B_lo)[b][o][k], z = b * splitk + s; all operands K-contiguous bf16
struct SplitGemm {
    const __bf16* A_hi; const __bf16* A_lo; long lda, strideA;
    const __bf16* B_hi; const __bf16* B_lo; long ldb, strideB;       // B_lo == nullptr: B is bf16 as it stands (two products)
    float* C; long ldc, strideC, split_stride;
    int M, N, K, k_per_split, splitk, nbatch;
    long long* wg_stamps;            // residency / loop-cycle experiment (wg_stamps.h), or nullptr
    int wide;                        // 0: the 384 x 256 kernel where whole tiles fill the chip; 1: wherever whole tiles apply
    const int32_t* b_map;            // device [nbatch] or nullptr: batch entry b reads its B operand at b_map[b] * strideB (A, C and
                                     // the split-K slabs keep indexing by b; nullptr = b itself)
};
hipError_t launch_split_gemm(const SplitGemm& g, hipStream_t stream, int lds_pad = 0);
// fp32-accurate contraction from three bf16 planes per operand (six partial products, fp32 accumulation): C = A . B^T
struct SplitGemm6 {
    const __bf16* A[3]; long lda;    // planes of the [M][K] operand, k-tile-major (launch_split3_rows; lda unused)
    const __bf16* B[3]; long ldb;    // planes of the [N][K] operand, k-tile-major
    float* C; long ldc;
    int M, N, K;
    long long* wg_stamps;            // residency experiment (wg_stamps.h), or nullptr
    int narrow;                      // 1: the 128 x 128 kernel even where the 384 x 256 one applies (tests: the two agree bit for bit)
};
hipError_t launch_gemm_x6(const SplitGemm6& g, hipStream_t stream);
// x [rows][cols] fp32 = rows row0.. of an operand with rows_total rows -> p0 + p1 + p2 = x, bf16 planes in k-tile-major order
// (element (r, c) at ((c / 16) * rows_total + r) * 16 + c % 16); cols % 16 == 0
hipError_t launch_split3_rows(const float* x, long ld_in, long rows, int cols, void* p0, void* p1, void* p2, long row0, long rows_total,
                              hipStream_t stream);
int shared_worker_stream(hipStream_t* out);   // ltm_consolidate.hip: the process-wide worker streams
int split_gemm_pick_splitk(int M, int N, int K, int nbatch, int* k_per_split);
long split_gemm_wide_tile_count(int M, int N);   // tiles of the 384 x 256 kernel per batch entry, 0 if the shape has no whole ones   // fills the chip with the tile shape that will run
// x [rows][cols] fp32 -> hi = bf16(x), lo = bf16(x - hi)
hipError_t launch_split_rows(const float* x, long ld_in, long rows, int cols, void* hi, void* lo, long ld_out, hipStream_t stream);
// ---- the query-side linears of infv_vqf_encode_frames in reduced arithmetic (linear_gemm.hip; infv_vqf_set_linear_precision) ----
// C [M][N] fp32 = A [M][K] fp32 (prepared on the way into LDS) . B [N][K]^T from 2-byte planes.  mode 1: bf16 hi / lo planes, three
// products per k-step (lo.hi, hi.lo, hi.hi); mode 2: one fp16 plane (B_lo unused), one product.  K % 64 == 0, lda % 4 == 0,
// ldb % 8 == 0, 16-byte aligned operands.  128 x 128 x 64 tiles and one k order whatever M is, no split-K.
struct LinearGemm {
    const float* A; long lda;
    const void* B_hi; const void* B_lo; long ldb;
    float* C; long ldc;
    int M, N, K;
};
hipError_t launch_linear_gemm(const LinearGemm& g, int mode, hipStream_t stream);
// x [rows][cols] fp32 -> out [rows][cols] fp16, round to nearest even (beyond 65504: inf)
hipError_t launch_round_rows_f16(const float* x, long ld_in, long rows, int cols, void* out, long ld_out, hipStream_t stream);
// ---- the cross-attention of infv_vqf_encode_frames with fp16 operands (attention_f16.hip; infv_vqf_set_attention_precision) ----
constexpr int kAttnF16MaxPad = 512;      // keys a frame may have, padded: the scores of a 64-row block stay in accumulators
constexpr int kAttnF16Frames = 256;      // frames per sub-batch (the fp16 q~' and o' workspaces are sized by it): 1536 workgroups at 12 x 32 rows
// F [nb][n][d] of any token type (stats != nullptr: token_ln(F) applied on load, not for fp8) -> X [nb][n_pad][d] = fp16(value),
// round to nearest even, and its transposed copy XT [nb][d][n_pad]; rows at or beyond n zeros; n_pad % 64 == 0, nb <= 32768
// (token_pass.hip)
hipError_t launch_token_pass_f16(const void* F, tok_code tok, int nb, int n, int n_pad, int d, const void* stats, const float* gamma,
                                 const float* beta, void* X, void* XT, hipStream_t stream);
// plane [H][d][64] = fp16(wk [H * 64][d]) transposed per head
hipError_t launch_attn_f16_key_plane(const float* wk, int H, int d, void* plane, hipStream_t stream);
// ctx [nb * Q][H * 64] fp32 = the cross-attention context of nb frames (three launches: q~', scores + softmax + context, value
// projection).  xq [nb * Q][H * 64] fp32; wkT from launch_attn_f16_key_plane; wv16 [H * 64][d] fp16; bv [H * 64] or nullptr;
// X / XT the frames' planes; qt, o: fp16 workspaces [nb][H * Q][d].  n_pad <= kAttnF16MaxPad, d % 64 == 0
struct AttnF16 {
    const float* xq; const void* wkT; const void* wv16; const float* bv;
    const void* X; const void* XT;
    void* qt; void* o; float* ctx;
    int nb, Q, H, d, n, n_pad;
};
hipError_t launch_attn_f16(const AttnF16& a, hipStream_t stream);
// ---- frame tokens and score rows -> the contractions' bf16 planes (token_pass.hip) ----
// x [n] bf16 / fp16 / fp8 e4m3 -> y [n] fp32 (exact); n % 8 == 0, fp8: n % 16 == 0.  fp32 tokens are refused
hipError_t launch_upcast(const void* x, tok_code tok, float* y, long n, hipStream_t stream);
// bytes per element of a token type
inline size_t token_bytes(tok_code tok) { return tok == INFV_TOKENS_F32 ? 4 : tok == INFV_TOKENS_F8E4M3 ? 1 : 2; }
// The token pass of nb <= 32768 chunks F [nb][n][d] of any token type -> the bf16 planes Fh/Fl [nb][n][d] and Th/Tl [nb][d][n] and, with kbar,
// the frame means [nb][n / P][d] (needs token_pass_gives_means(P)).  fp32 / fp16: all four planes (hi/lo); bf16: Th alone, the untransposed
// operand is F itself; fp8 e4m3: Fh and Th, a value is its own hi piece
bool token_pass_gives_means(int P);
hipError_t launch_token_pass(const void* F, tok_code tok, int nb, int n, int d, void* Fh, void* Fl, void* Th, void* Tl,
                             hipStream_t stream, float* kbar, int P);
// ---- vision LayerNorm of the frame tokens (videochat2_it_mistral.py:195), y = token_ln(x) of ltm_device.h (token_pass.hip) ----
constexpr int kTokenLnMaxWidth = 4096;   // a token row is held in one wave's registers: 16 float4 per lane
// stats[row] = (mean, 1 / sqrt(var + eps)) of n_rows token rows of width d (d % 64 == 0, d <= kTokenLnMaxWidth); stats: float2
hipError_t launch_token_ln_stats(const void* F, tok_code tok, long n_rows, int d, float eps, void* stats, hipStream_t stream);
// y [n_rows][d] fp32 = token_ln(F): the reference form of the bits, and the operand of the fp32 contractions
hipError_t launch_ln_tokens(const void* F, tok_code tok, long n_rows, int d, const void* stats, const float* gamma, const float* beta,
                            float* y, hipStream_t stream);
// launch_token_pass over y = token_ln(F) applied on load: all four planes for every token type, kbar as there
hipError_t launch_token_pass_ln(const void* F, tok_code tok, int nb, int n, int d, const void* stats, const float* gamma,
                                const float* beta, void* Fh, void* Fl, void* Th, void* Tl, hipStream_t stream, float* kbar, int P);
// launch_pool (ltm_kernels.hip) over y = token_ln(k) applied on load: the bits of launch_pool on ln_tokens_kernel's tensor
hipError_t launch_pool_ln(const void* k, tok_code tok, const void* stats, const float* gamma, const float* beta, float* kbar,
                          int64_t n_frames, int P, int d, hipStream_t stream);
// The VideoChat2 embedding layer (Qformer.py:54-111): out row m = LN(query_tokens[-src[m] - 1]) where src[m] < 0, else
// LN(word[src[m]] + position[pos[m]]); src / pos: DEVICE int32 [n_rows], validated on the host; width <= 4096
hipError_t launch_qf_vc_embed(const float* word, const float* position, const float* query_tokens, const float* gamma, const float* beta,
                              float eps, const int32_t* src, const int32_t* pos, int n_rows, int width, float* out, hipStream_t stream);

// softmax of fp32 score rows, written as bf16 hi/lo (token_pass.hip)
hipError_t launch_softmax_rows_split(const float* S, long n_rows, int len, long ld, void* Ph, void* Pl, long ld_out, hipStream_t stream);

// ---- padded forms for frames whose token count is no multiple of 64 (infv_vqf_encode_frames; token_pass.hip) ----
// F [nb][n][d] of any token type (stats != nullptr: token_ln(F) applied on load, not for fp8) -> Fh/Fl [nb][n_pad][d] and
// Th/Tl [nb][d][n_pad], n_pad = ceil(n / 64) * 64, rows at or beyond n zeros; rows of the next frame are never read.
// bf16 / fp8 tokens without LayerNorm: Fl and Tl must be nullptr (Fh IS written: the caller's buffer has another stride).  nb <= 32768
hipError_t launch_token_pass_pad(const void* F, tok_code tok, int nb, int n, int n_pad, int d, const void* stats, const float* gamma,
                                 const float* beta, void* Fh, void* Fl, void* Th, void* Tl, hipStream_t stream);
// softmax over columns [0, len) of fp32 score rows of padded length len_pad; columns [len, len_pad) of Ph / Pl are written as zeros
hipError_t launch_softmax_rows_split_pad(const float* S, long n_rows, int len, int len_pad, long ld, void* Ph, void* Pl, long ld_out,
                                         hipStream_t stream);
// launch_qf_epilogue with the row written as bf16 / fp16 (round to nearest even) into out16 [M][ld_out16]; e.out is not read.
// Needs what the 16-byte form of the epilogue needs (qf_epilogue_cast_applies); no scalar form exists.
bool qf_epilogue_cast_applies(const QfEpilogue& e, const void* out16, long ld_out16);
hipError_t launch_qf_epilogue_cast(const QfEpilogue& e, void* out16, long ld_out16, tok_code out_dtype, hipStream_t stream);

// out[m][:] = mean over nb of in[b][m][:]
hipError_t launch_qf_mean(const float* in, int nb, long n, float* out, hipStream_t stream);
constexpr int kMeanSegs = 256;           // videos per launch of launch_qf_mean_segments (the table travels in kernel arguments)
// out[v][:] = mean over b in [cu[v], cu[v+1]) of in[b][:] for v < V, summed in b order as qf_mean_kernel (cu: host array [V+1])
hipError_t launch_qf_mean_segments(const float* in, const int32_t* cu, int V, long n, float* out, hipStream_t stream);

}  // namespace infv
