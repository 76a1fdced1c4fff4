// Private to the host units of the video Q-former C ABI (vqf_capi.hip: handle, plane caches, shared steps, stand-alone entry points;
// vqf_video.hip: encode_chunk and the layer-major encode_video / encode_videos; vqf_vc.hip: the VideoChat2 / frame path): the handle,
// the descriptors of the shared steps, and the steps themselves.
#pragma once
#include "../../include/infv_vqf.h"
#include "capi_common.h"
#include "vqf_internal.h"

#include <memory>
#include <vector>

// The 2-byte planes of one (stacked) weight of a reduced-precision linear: [n_lin * n_out][K] bf16 hi and lo (mode 1) or fp16 (mode 2, hi alone)
struct LinPlanes {
    const float* w[infv::kQfMaxSeg] = {}; int n_lin = 0, n_out = 0, K = 0;
    infv::DeviceBuf hi, lo;
};

// The fp16 planes of one cross layer's key and value weights (infv_vqf_set_attention_precision(h, 1)): kT [H][d][64] = Wk per head,
// transposed; v16 [hidden][d] = Wv as it lies
struct AttnPlanes {
    const float* wk = nullptr; const float* wv = nullptr; int H = 0, d = 0;
    infv::DeviceBuf kT, v16;
};

struct infv_vqf_s {
    using DeviceBuf = infv::DeviceBuf;
    infv_vqf_config cfg;
    int dev = 0;
    bool exact_fp32 = false;
    infv::tok_code tok = INFV_TOKENS_F32;       // element type of the `frames` arguments (infv_vqf_set_token_dtype)
    // chunk-independent prefix of layer 0 (embedding LayerNorm, self-attention block, cross query, pre-multiplied query):
    // reused across encode_chunk calls while the host keeps the weights epoch unchanged (0 = never reuse)
    unsigned long long epoch = 0, c_epoch = 0;
    bool c_valid = false, c_qt_valid = false, c_qsplit_valid = false;
    DeviceBuf c_h1, c_xq, c_qt, c_qh, c_ql;
    // workspaces (grown on demand; a growing call synchronises the device first)
    DeviceBuf part, h_a, h_b, h1, h2, qkv, sa, xq, along, qt, S, O, merged, inter, kbar;
    DeviceBuf sFh, sFl, sTh, sTl, sPh, sPl, sQh, sQl;   // split-bf16 operands of the short-term attention
    DeviceBuf wFh, wFl, wTh, wTl;                       // the same split of a WHOLE video's frame tokens (layer-major path)
    DeviceBuf up;                                       // fp32 copy of fp16 / bf16 tokens where the split path does not apply
    int tap_layer = -1; float* tap_dst = nullptr;       // infv_vqf_set_context_tap: consumed by the next infv_vqf_encode_frames
    bool fuse = true;                                   // one pass over the frame tokens: split + transpose + frame means
    double split_cache_gb = 64.0;                       // budget for a whole video's split tokens (INFV_VQF_SPLIT_CACHE_GB at create)
    // whole-video (layer-major) path
    DeviceBuf vA, v1, v2, vxq, valong, vshort, vmerged, vqkv, vsa, vinter, vu, vkbar, v_h1s, v_xqs;
    DeviceBuf tA, t1, tqkv, tsa, tinter;                // packed text rows of the VideoChat2 path (infv_vqf_vc_encode_videos)
    DeviceBuf smap;                                     // infv_vqf_vc_encode_streams: source chunk of every stream-chunk (int32; grown, never shrunk)
    // infv_vqf_vc_encode_img: (mean, 1 / sqrt(var + eps)) of every distinct token row; the embedding layer's output rows; the row
    // table of the embedding kernel on the device and its pinned staging buffer (reused once ev_ids, recorded behind the copy, has passed)
    DeviceBuf lnstats, embrows, ids_dev;
    int32_t* ids_pin = nullptr;
    size_t ids_pin_n = 0;
    hipEvent_t ev_ids = nullptr;
    bool ids_in_flight = false;
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    // infv_vqf_set_linear_precision: the arithmetic of the query-side linears of infv_vqf_encode_frames, and the weight planes of the
    // reduced modes -- kept while the non-zero weights epoch lp_epoch stands (epoch 0: one scratch pair, rewritten by every linear)
    int lin_mode = 0;
    std::vector<std::unique_ptr<LinPlanes>> lp;
    unsigned long long lp_epoch = 0;
    LinPlanes lp_scratch;
    // infv_vqf_set_attention_precision: the arithmetic of the cross-attention of infv_vqf_encode_frames.  The key / value weight
    // planes of mode 1 live by the rules of the linears' planes (lp_epoch); aX / aXT are a call's fp16 token planes, aQt / aO the
    // fp16 pre-multiplied queries and context rows of one sub-batch
    int attn_mode = 0;
    std::vector<std::unique_ptr<AttnPlanes>> ap;
    AttnPlanes ap_scratch;
    DeviceBuf aX, aXT, aQt, aO;
    ~infv_vqf_s() {
        if (side) (void)hipStreamSynchronize(side);           // (a stream of the process-wide set: not destroyed here)
        if (ev_main) (void)hipEventDestroy(ev_main);
        if (ev_side) (void)hipEventDestroy(ev_side);
        if (ev_ids) { (void)hipEventSynchronize(ev_ids); (void)hipEventDestroy(ev_ids); }
        if (ids_pin) (void)hipHostFree(ids_pin);
    }
};

namespace infv {
#pragma GCC visibility push(hidden)   // shared by the three units, no part of the library's exported symbols

// y = epilogue( x [M][K] . W^T ) with up to 3 stacked weight matrices of n_out rows each
struct LinearCall {
    const float* x; int M, K;
    const infv_linear* lin[kQfMaxSeg]; int n_lin; int n_out;      // output width = n_lin * n_out
    int act = QF_ACT_NONE;
    const float* residual = nullptr; int res_rows = 1;
    const infv_layernorm* ln = nullptr;
    float* y;
    bool inv = false;      // batch invariant (infv_vqf_encode_videos): 128 x 128 tiles, no split-K, whatever M is
    bool reduced = false;  // a query-side linear of infv_vqf_encode_frames (or infv_vqf_linear): the handle's linear precision applies
    void* y16 = nullptr; tok_code y16_dtype = INFV_TOKENS_F32;   // y16 != nullptr: the rows go out as bf16 / fp16 instead of y (infv_vqf_encode_frames)
};
int run_linear(infv_vqf_s* h, const LinearCall& c, hipStream_t stream);
int linear_planes(infv_vqf_s* h, const LinearCall& c, const LinPlanes** out, hipStream_t stream);
int attn_planes(infv_vqf_s* h, const infv_linear* key, const infv_linear* value, const AttnPlanes** out, hipStream_t stream);

// Split-bf16 copies of frame tokens produced ahead of the attention (prepare_split): [.][n_tokens][d] and [.][d][n_tokens]
// (bf16 tokens: Fh is the caller's buffer itself, Fl and Tl are nullptr -- the contractions then run their two-product form;
//  fp16 tokens: four planes as for fp32, written by a pass that reads 2 bytes per element;
//  fp8 tokens: Fh and Th written by a pass that reads 1 byte per element, Fl and Tl nullptr -- an e4m3 value is its own hi piece)
struct SplitRef { const __bf16 *Fh, *Fl, *Th, *Tl; };
// the cached planes of a whole call, from chunk c0 on
inline SplitRef split_ref_at(const SplitRef& w, int c0, long chunk_k) {
    const long o = (long)c0 * chunk_k;
    return SplitRef{w.Fh + o, w.Fl ? w.Fl + o : nullptr, w.Th + o, w.Tl ? w.Tl + o : nullptr};
}
// infv_vqf_encode_videos takes the short-term attention's split-K counts as for this many chunks per sub-batch, whatever the
// sub-batch holds: a chunk's summation order then does not depend on the rest of the batch
constexpr int kInvariantNb = 16;

bool split_path(const infv_vqf_s* h, int n_tokens);
// element `elems` of a token buffer of either dtype
inline const void* tok_at(const void* frames, tok_code tok, long elems) {
    return static_cast<const char*>(frames) + elems * (long)token_bytes(tok);
}
// bytes of bf16 planes prepare_split writes per token element, for the plane-cache budget: bf16 tokens 2 (FT_hi alone), fp8 tokens 4
// (F_hi and FT_hi), fp32 / fp16 tokens and every normalised token (`ln`: a general fp32 number) 8 (all four planes)
// (padded planes, infv_vqf_encode_frames: bf16 tokens cannot be read in place at another stride, so their F_hi is written too: 4)
inline double plane_bytes(tok_code tok, bool ln, bool padded = false) {
    return ln ? 8.0 : tok == INFV_TOKENS_BF16 ? (padded ? 4.0 : 2.0) : tok == INFV_TOKENS_F8E4M3 ? 4.0 : 8.0;
}
// fp16 / bf16 / fp8 tokens where the split path does not apply: frames / tok become an fp32 copy in the handle's workspace, for the fp32 kernels
int fp32_tokens_unless_split(infv_vqf_s* h, const void*& frames, tok_code& tok, int n_tokens, size_t elems, hipStream_t stream);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The vision LayerNorm applied while the tokens are read (infv_vqf_vc_encode_img): stats [rows][2] = (mean, 1 / sqrt(var + eps))
// of the token rows of the buffer the call addresses (row 0 = its first token), gamma / beta [enc_width] on the device
struct TokLn { const float* stats; const float* gamma; const float* beta; };

// ONE pass over the frame tokens of `nb` chunks: hi/lo bf16 split, its transposed copy and (kbar != nullptr) the frame
// means the long-term memories consume.  The tokens do not depend on the layer, so every layer's short-term attention
// and every layer's memory share this pass (the reference reads them once per layer and once more for the pooling:
// Qformer.py:236, 278-291).
struct TokenPass {
    const void* frames; tok_code tok; int nb, n_tokens;
    float* kbar = nullptr;
    bool whole = false;            // the video-sized buffers of the layer-major path
    // the planes of these nb chunks go to chunks [dst0, dst0 + nb) of buffers reserved for cap chunks (0, 0: [0, nb) of nb);
    // *ref always addresses chunk 0 of the buffers
    int dst0 = 0, cap = 0;
    const TokLn* ln = nullptr;     // the planes (and means) of token_ln(frames); ln->stats addresses frames' first token
    int n_live = 0;                // > 0 and != n_tokens: frames holds n_live tokens a chunk, the planes n_tokens = ceil(n_live / 64) * 64 (pad: zeros)
};
int prepare_split(infv_vqf_s* h, const TokenPass& p, SplitRef* ref, hipStream_t stream);

// frames [nb][n_tokens][d]; xq: per-chunk [nb*Q][hidden] (shared_q = false) or one [Q][hidden] block used by every
// chunk (shared_q = true: layer 0 of the video Q-former, whose query does not depend on the chunk)
//   -> merged [nb*Q][hidden] = alpha * short-term context + (1 - alpha) * along   (along == nullptr: short-term only)
struct ShortAttn {
    const void* frames; tok_code tok;        // (fp16, bf16, fp8: only where split_path() holds)
    int nb, n_tokens;
    const float* xq; bool shared_q;
    const infv_linear* key; const infv_linear* value;
    const float* along = nullptr; float* merged = nullptr;
    bool use_cache = false;                  // nb == 1, shared_q: the pre-multiplied query lives in the handle's layer-0 cache
    const SplitRef* pre = nullptr;           // the caller split these tokens already (shared by the layers)
    hipEvent_t along_ready = nullptr;        // `along` is produced on another stream: wait here, before the merge
    int inv_nb = 0;                          // > 0: batch invariant -- split-K counts and kernel shapes as for inv_nb chunks, whatever nb is
    const int32_t* b_map = nullptr;          // device [nb]: chunk b reads chunk b_map[b] of frames / *pre (several streams over one block)
    bool t_identity = false;                 // the transposed plane of *pre holds the sub-batch's chunks in order: only the untransposed operand goes through b_map
    int n_live = 0;                          // > 0 and != n_tokens: *pre holds planes padded to n_tokens, only the first n_live keys of a chunk exist
};
int short_attention(infv_vqf_s* h, const ShortAttn& a, hipStream_t stream);

int refuse_reduced(const infv_vqf_s* h, const char* name);
int ensure_streams(infv_vqf_s* h);
int check_front_emb(const char* name, const infv_vqf_vc_front* f, int V, const int32_t* text_len);
int run_embed(infv_vqf_s* h, const infv_vqf_vc_front* f, int V, const int32_t* text_len, float* out, hipStream_t stream);
int check_offsets(const char* name, const char* tab, const int32_t* t, int n);
int check_distinct_handles(const char* name, const infv_ltm_handle* ltm, int n, const char* per);

// ---- where a layer-major call is cut (the seams; sizes in vqf_internal.h).  All of them are decided in vqf_capi.hip, whichever path
//      asks, next to alpha_merge's: tests/golden/seam_cases.py reads the sizes and their sites from one unit.
struct CallBlocks { int RB, NB; };   // chunks per row block of the query-token GEMMs, per sub-batch of the short-term attention
int pick_short_nb(const infv_vqf_s* h, int C, int n_tokens);
CallBlocks video_call_blocks(const infv_vqf_s* h, int C, int n_tokens, bool multi);   // infv_vqf_encode_video / _videos (multi)
CallBlocks vc_call_blocks(const infv_vqf_s* h, int C, int n_tokens);                  // the VideoChat2 / frame path: always batch invariant
long text_ffn_block(long Tt);                                                         // packed text rows per block of the VideoChat2 text FFN

// ---- steps shared by the layer-major calls (the stages of encode_impl and of vc_impl) and, with one block, by encode_chunk ----

// Chunks [0, C) in blocks of B:  for (RowBlock b : RowBlocks{C, B, stride})  yields the first chunk, the chunk count and the first
// element of chunk c0 in a [C][stride] activation buffer.
struct RowBlock { int c0, nb; long r0; };
struct RowBlocks {                                            // (the range is its own iterator)
    int C, B; long stride; int c0 = 0;
    RowBlocks begin() const { return *this; }
    RowBlocks end() const { return *this; }
    bool operator!=(const RowBlocks&) const { return c0 < C; }
    void operator++() { c0 += B; }
    RowBlock operator*() const { return RowBlock{c0, C - c0 < B ? C - c0 : B, c0 * stride}; }
};

// The rows of one block, what shapes their GEMMs (LinearCall's inv / reduced) and the stream they run on
struct BlockRows { int rows; bool inv, reduced; hipStream_t stream; };
int embed_query_tokens(infv_vqf_s* h, const infv_vqf_weights* w, hipStream_t stream);
int query_self_block(infv_vqf_s* h, const BlockRows& r, const infv_vqf_layer& L, const float* x, bool whole, float* h1, float* xq);
// cross output of a block: y = LayerNorm( x . x_o^T + bias + residual ), residual row m % res_rows (Qformer.py:306-311)
int cross_output(infv_vqf_s* h, const BlockRows& r, const infv_linear* x_o, const infv_layernorm* ln, const float* x, const float* residual,
                 int res_rows, float* y);
// FFN of a block (Qformer.py:519-522): y = LayerNorm( gelu(x . in^T) . out^T + x ) through the scratch rows `inter`; y16 != nullptr: the
// rows go out as bf16 / fp16 (y16_dtype) instead of y
struct FfnRef { const infv_linear *in, *out; const infv_layernorm* ln; };
int ffn_rows(infv_vqf_s* h, const BlockRows& r, const FfnRef& f, const float* x, float* inter, float* y, void* y16 = nullptr,
             tok_code y16_dtype = INFV_TOKENS_F32);
int ltm_u_slice(infv_vqf_s* h, const double* u, int l, int n_layers_in_u, int C, hipStream_t stream);
int alpha_merge(infv_vqf_s* h, long M, hipStream_t stream);
// the videos of a packed call: cu [V + 1] (host), or cu == nullptr: all chunks are one video's
struct VideoSegs { const int32_t* cu; int V; };
int project_and_mean(infv_vqf_s* h, RowBlocks blocks, const infv_linear* proj, bool inv, float* out, float* mean, VideoSegs videos,
                     hipStream_t stream);

#pragma GCC visibility pop
}  // namespace infv
