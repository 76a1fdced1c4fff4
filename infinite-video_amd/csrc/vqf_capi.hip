// C ABI of the video Q-former path (include/infv_vqf.h): workspace + launch sequence of one chunk.
#include "../../include/infv_vqf.h"
#include "capi_common.h"
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>
#include "vqf_internal.h"

#include <cstdlib>
#include <new>

using namespace infv;

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
    infv_vqf_config cfg;
    int dev = 0;
    bool exact_fp32 = false;
    tok_code tok = INFV_TOKENS_F32;             // element type of the `frames` arguments (infv_vqf_set_token_dtype)
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

namespace {

int check_cfg(const infv_vqf_config& c) {
    if (c.n_layers < 1 || c.n_layers > INFV_VQF_MAX_LAYERS) return fail(INFV_ERR_INVALID, "n_layers must be 1..%d", INFV_VQF_MAX_LAYERS);
    if (c.n_heads < 1 || c.hidden != c.n_heads * 64) return fail(INFV_ERR_UNSUPPORTED, "hidden must be n_heads * 64");
    // (the whole-layer entry points need n_query <= 32 and tokens_per_frame % 32 == 0 and check it themselves;
    //  infv_vqf_short_attention alone also serves the VideoChat2 shape: 96 query tokens, 196 tokens per frame)
    if (c.n_query < 1 || c.n_query > 256) return fail(INFV_ERR_UNSUPPORTED, "n_query must be 1..256");
    if (c.hidden % 64 || c.inter % 64 || c.enc_width % 32 || (c.proj_out % 64)) return fail(INFV_ERR_UNSUPPORTED, "widths must be multiples of 64 (enc_width: 32)");
    if (c.hidden > 4096 || c.inter > 4096 || c.proj_out > 4096 || 3 * c.hidden > 4096) return fail(INFV_ERR_UNSUPPORTED, "row widths above 4096 are not supported");
    if (c.nb_samples < 1) return fail(INFV_ERR_INVALID, "nb_samples must be >= 1");
    if (c.tokens_per_frame < 1) return fail(INFV_ERR_INVALID, "tokens_per_frame must be positive");
    return INFV_OK;
}

int check_layer_cfg(const infv_vqf_config& c) {       // what the fused per-layer kernels of encode_chunk / encode_video are built for
    if (c.n_query > 32) return fail(INFV_ERR_UNSUPPORTED, "encode_chunk / encode_video need n_query <= 32 (this handle: %d)", c.n_query);
    if (c.tokens_per_frame % 32) return fail(INFV_ERR_UNSUPPORTED, "encode_chunk / encode_video need tokens_per_frame %% 32 == 0");
    return INFV_OK;
}

// Every entry point but infv_vqf_encode_frames (and infv_vqf_linear, infv_vqf_frame_cross_attention) while a reduced linear precision
// or the fp16 attention precision is set: their query rows feed the memories' Gibbs draw, and reduced products never feed the scores
// of the draw (split_gemm.hip); the fp16 attention exists for the frame call alone
int refuse_reduced(const infv_vqf_s* h, const char* name) {
    if (h->lin_mode == 0 && h->attn_mode == 0) return INFV_OK;
    if (h->lin_mode == 0)
        return fail(INFV_ERR_UNSUPPORTED, "%s: the handle's attention precision is %d, which only infv_vqf_encode_frames and "
                                          "infv_vqf_frame_cross_attention run (infv_vqf_set_attention_precision(h, 0) selects the "
                                          "split-bf16 attention again)", name, h->attn_mode);
    return fail(INFV_ERR_UNSUPPORTED, "%s: the handle's linear precision is %d, which only infv_vqf_encode_frames runs "
                                      "(infv_vqf_set_linear_precision(h, 0) selects fp32 again)", name, h->lin_mode);
}

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

// Drops the cached weight planes (work in flight may still read them: the device is synchronised first)
int drop_linear_planes(infv_vqf_s* h) {
    if (h->lp.empty() && h->ap.empty()) return INFV_OK;
    HIP_TRY(hipDeviceSynchronize());
    h->lp.clear();
    h->ap.clear();
    return INFV_OK;
}

// The fp16 planes of a cross layer's key and value weights, cached as the linears' planes are: keyed on (weight pointers, shape)
// while the non-zero weights epoch stands; epoch 0 rebuilds them into one scratch pair in every call.
int attn_planes(infv_vqf_s* h, const infv_linear* key, const infv_linear* value, const AttnPlanes** out, hipStream_t stream) {
    const int H = h->cfg.n_heads, d = h->cfg.enc_width;
    AttnPlanes* p = nullptr;
    if (h->epoch == 0) {
        p = &h->ap_scratch;
    } else {
        if (h->lp_epoch != h->epoch) {
            if (int rc = drop_linear_planes(h)) return rc;
            h->lp_epoch = h->epoch;
        }
        for (const auto& e : h->ap)
            if (e->wk == key->w && e->wv == value->w && e->H == H && e->d == d) { *out = e.get(); return INFV_OK; }
        std::unique_ptr<AttnPlanes> fresh(new (std::nothrow) AttnPlanes());
        if (!fresh) return fail(INFV_ERR_INVALID, "out of host memory");
        p = fresh.get();
        h->ap.push_back(std::move(fresh));
    }
    const size_t bytes = (size_t)H * 64 * d * 2;
    hipError_t e = reserve_all({{p->kT, bytes}, {p->v16, bytes}});
    if (e == hipSuccess) e = launch_attn_f16_key_plane(key->w, H, d, p->kT.p, stream);
    if (e == hipSuccess) e = launch_round_rows_f16(value->w, d, (long)H * 64, d, p->v16.p, d, stream);
    if (e != hipSuccess) {
        if (p != &h->ap_scratch) h->ap.pop_back();
        return fail(INFV_ERR_HIP, "weight planes of the fp16 cross-attention: %s", hipGetErrorString(e));
    }
    p->wk = key->w; p->wv = value->w; p->H = H; p->d = d;
    *out = p;
    return INFV_OK;
}

// The planes of c's (stacked) weight in the handle's reduced mode: one contiguous [n_lin * n_out][K] set, so the GEMM sees one B and
// a tile may straddle the segments.  Keyed on (weight pointers, shape); the mode and the epoch are the whole cache's.
int linear_planes(infv_vqf_s* h, const LinearCall& c, const LinPlanes** out, hipStream_t stream) {
    const int mode = h->lin_mode;
    LinPlanes* p = nullptr;
    if (h->epoch == 0) {
        p = &h->lp_scratch;
    } else {
        if (h->lp_epoch != h->epoch) {
            if (int rc = drop_linear_planes(h)) return rc;
            h->lp_epoch = h->epoch;
        }
        for (const auto& e : h->lp) {
            bool same = e->n_lin == c.n_lin && e->n_out == c.n_out && e->K == c.K;
            for (int i = 0; same && i < c.n_lin; ++i) same = e->w[i] == c.lin[i]->w;
            if (same) { *out = e.get(); return INFV_OK; }
        }
        std::unique_ptr<LinPlanes> fresh(new (std::nothrow) LinPlanes());
        if (!fresh) return fail(INFV_ERR_INVALID, "out of host memory");
        p = fresh.get();
        h->lp.push_back(std::move(fresh));
    }
    const size_t bytes = (size_t)c.n_lin * c.n_out * c.K * 2;
    hipError_t e = reserve_all({{p->hi, bytes}, {p->lo, mode == 1 ? bytes : 0}});
    for (int i = 0; e == hipSuccess && i < c.n_lin; ++i) {
        const size_t o = (size_t)i * c.n_out * c.K * 2;
        if (mode == 1) e = launch_split_rows(c.lin[i]->w, c.K, c.n_out, c.K, p->hi.as<char>() + o, p->lo.as<char>() + o, c.K, stream);
        else e = launch_round_rows_f16(c.lin[i]->w, c.K, c.n_out, c.K, p->hi.as<char>() + o, c.K, stream);
    }
    if (e != hipSuccess) {
        if (p != &h->lp_scratch) h->lp.pop_back();             // (nothing in flight reads planes that were never handed out)
        return fail(INFV_ERR_HIP, "weight planes of a reduced-precision linear: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < c.n_lin; ++i) p->w[i] = c.lin[i]->w;
    p->n_lin = c.n_lin; p->n_out = c.n_out; p->K = c.K;
    *out = p;
    return INFV_OK;
}

int run_linear(infv_vqf_s* h, const LinearCall& c, hipStream_t stream) {
    const int width = c.n_lin * c.n_out;
    const int mode = c.reduced ? h->lin_mode : 0;
    const int sk = c.inv || mode ? 1 : qf_pick_splitk(c.M, width, c.K, 1);
    const size_t need = (size_t)sk * c.M * width * sizeof(float);
    HIP_TRY(reserve_all({{h->part, need}}));
    const long split_stride = (long)c.M * width;
    if (mode) {                                                // split-bf16 / fp16: one launch, as the fp32 GEMM is
        const LinPlanes* p = nullptr;
        if (int rc = linear_planes(h, c, &p, stream)) return rc;
        LinearGemm g{};
        g.A = c.x; g.lda = c.K; g.B_hi = p->hi.p; g.B_lo = p->lo.p; g.ldb = c.K;
        g.C = h->part.as<float>(); g.ldc = width; g.M = c.M; g.N = width; g.K = c.K;
        HIP_TRY(launch_linear_gemm(g, mode, stream));
    } else {
    QfGemm g{};
    g.A = c.x; g.lda = c.K; g.strideA = 0;
    for (int i = 0; i < c.n_lin; ++i) g.B[i] = c.lin[i]->w;
    g.ldb = c.K; g.strideB = 0; g.seg_rows = c.n_out;
    g.C = h->part.as<float>(); g.ldc = width; g.strideC = 0; g.split_stride = split_stride;
    g.M = c.M; g.N = width; g.k_per_split = c.K / sk; g.splitk = sk; g.nbatch = 1; g.tile = c.inv ? 128 : 0;
    HIP_TRY(launch_qf_gemm(g, false, stream));
    }
    QfEpilogue e{};
    e.parts = h->part.as<float>(); e.nsplit = sk; e.split_stride = split_stride; e.ld_in = width;
    for (int i = 0; i < c.n_lin; ++i) e.bias[i] = c.lin[i]->b;
    e.seg_cols = c.n_out; e.act = c.act; e.scale = 1.f; e.res_scale = 1.f;
    e.residual = c.residual; e.ld_res = width; e.res_rows = c.res_rows;
    e.gamma = c.ln ? c.ln->gamma : nullptr; e.beta = c.ln ? c.ln->beta : nullptr; e.eps = h->cfg.ln_eps;
    e.out = c.y; e.ld_out = width; e.M = c.M; e.width = width;
    if (c.y16) HIP_TRY(launch_qf_epilogue_cast(e, c.y16, width, c.y16_dtype, stream));
    else HIP_TRY(launch_qf_epilogue(e, stream));
    return INFV_OK;
}

// frames [nb][n_tokens][d]; xq: per-chunk [nb*Q][hidden] (shared_q = false) or one [Q][hidden] block used by every
// chunk (shared_q = true: layer 0 of the video Q-former, whose query does not depend on the chunk)
//   -> merged [nb*Q][hidden] = alpha * short-term context + (1 - alpha) * along   (along == nullptr: short-term only)
// Split-bf16 copies of frame tokens produced ahead of the attention (prepare_split): [.][n_tokens][d] and [.][d][n_tokens]
// (bf16 tokens: Fh is the caller's buffer itself, Fl and Tl are nullptr -- the contractions then run their two-product form;
//  fp16 tokens: four planes as for fp32, written by a pass that reads 2 bytes per element;
//  fp8 tokens: Fh and Th written by a pass that reads 1 byte per element, Fl and Tl nullptr -- an e4m3 value is its own hi piece)
struct SplitRef { const __bf16 *Fh, *Fl, *Th, *Tl; };
// infv_vqf_encode_videos takes the short-term attention's split-K counts as for this many chunks per sub-batch, whatever the
// sub-batch holds: a chunk's summation order then does not depend on the rest of the batch
constexpr int kInvariantNb = 16;

static bool split_path(const infv_vqf_s* h, int n_tokens) {
    static const bool want_fp32 = [] { const char* e = getenv("INFV_VQF_FP32"); return e && atoi(e) != 0; }();
    return !want_fp32 && !h->exact_fp32 && h->cfg.enc_width % 64 == 0 && n_tokens % 64 == 0;   // (odd frame counts: exact-fp32 kernels)
}

// ONE pass over the frame tokens of `nb` chunks: hi/lo bf16 split, its transposed copy and (kbar != nullptr) the frame
// means the long-term memories consume.  The tokens do not depend on the layer, so every layer's short-term attention
// and every layer's memory share this pass (the reference reads them once per layer and once more for the pooling:
// Qformer.py:236, 278-291).  `whole` selects the video-sized buffers of the layer-major path.
// element `elems` of a token buffer of either dtype
static const void* tok_at(const void* frames, tok_code tok, long elems) {
    return static_cast<const char*>(frames) + elems * (long)token_bytes(tok);
}

// bytes of bf16 planes prepare_split writes per token element, for the plane-cache budget: bf16 tokens 2 (FT_hi alone), fp8 tokens 4
// (F_hi and FT_hi), fp32 / fp16 tokens and every normalised token (`ln`: a general fp32 number) 8 (all four planes)
// (padded planes, infv_vqf_encode_frames: bf16 tokens cannot be read in place at another stride, so their F_hi is written too: 4)
static double plane_bytes(tok_code tok, bool ln, bool padded = false) {
    return ln ? 8.0 : tok == INFV_TOKENS_BF16 ? (padded ? 4.0 : 2.0) : tok == INFV_TOKENS_F8E4M3 ? 4.0 : 8.0;
}

// fp16 / bf16 / fp8 tokens where the split path does not apply: frames / tok become an fp32 copy in the handle's workspace, for the fp32 kernels
static int fp32_tokens_unless_split(infv_vqf_s* h, const void*& frames, tok_code& tok, int n_tokens, size_t elems, hipStream_t stream) {
    if (tok == INFV_TOKENS_F32 || split_path(h, n_tokens)) return INFV_OK;
    HIP_TRY(reserve_all({{h->up, elems * sizeof(float)}}));
    HIP_TRY(launch_upcast(frames, tok, h->up.as<float>(), (long)elems, stream));
    frames = h->up.p; tok = INFV_TOKENS_F32;
    return INFV_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The vision LayerNorm applied while the tokens are read (infv_vqf_vc_encode_img): stats [rows][2] = (mean, 1 / sqrt(var + eps))
// of the token rows of the buffer the call addresses (row 0 = its first token), gamma / beta [enc_width] on the device
struct TokLn { const float* stats; const float* gamma; const float* beta; };

// dst0 / cap: the planes of these nb chunks go to chunks [dst0, dst0 + nb) of buffers reserved for cap chunks (0, 0: [0, nb) of nb);
// *ref always addresses chunk 0 of the buffers
static int prepare_split(infv_vqf_s* h, const void* frames_, tok_code tok, int nb, int n_tokens, float* kbar, bool whole, SplitRef* ref,
                         hipStream_t stream, int dst0 = 0, int cap = 0,
                         const TokLn* ln = nullptr /* the planes (and means) of token_ln(frames); ln->stats addresses frames_' first token */,
                         int n_live = 0 /* > 0 and != n_tokens: frames_ holds n_live tokens a chunk, the planes n_tokens = ceil(n_live / 64) * 64 (pad: zeros) */) {
    const int d = h->cfg.enc_width, P = h->cfg.tokens_per_frame;
    const bool padded = n_live > 0 && n_live != n_tokens;   // padded planes: no frame means
    if (padded && kbar) return fail(INFV_ERR_INVALID, "prepare_split: no frame means from padded planes");
    // Which planes the pass writes.  A normalised value is a general fp32 number, as an fp32 / fp16 token is: all four.  An e4m3
    // value has no lo piece: F_hi and T_hi.  bf16 tokens are read in place, only the transposed copy is written -- except into padded
    // planes, whose stride the caller's buffer does not have: F_hi too.
    const bool lo = ln || tok == INFV_TOKENS_F32 || tok == INFV_TOKENS_F16;
    const bool hi = lo || tok == INFV_TOKENS_F8E4M3 || padded;
    const size_t szF = (size_t)(cap > dst0 + nb ? cap : dst0 + nb) * n_tokens * d * 2;
    const size_t d0 = (size_t)dst0 * n_tokens * d;
    DeviceBuf& Fh = whole ? h->wFh : h->sFh; DeviceBuf& Fl = whole ? h->wFl : h->sFl;
    DeviceBuf& Th = whole ? h->wTh : h->sTh; DeviceBuf& Tl = whole ? h->wTl : h->sTl;
    HIP_TRY(reserve_all({{Fh, hi ? szF : 0}, {Fl, lo ? szF : 0}, {Th, szF}, {Tl, lo ? szF : 0}}));
    const int rows_in = padded ? n_live : n_tokens;           // token rows a chunk holds in frames_
    for (int c0 = 0; c0 < nb; c0 += 32768) {                   // grid.z limit
        const int n = nb - c0 < 32768 ? nb - c0 : 32768;
        const size_t o = d0 + (size_t)c0 * n_tokens * d;
        const void* src = tok_at(frames_, tok, (long)((size_t)c0 * rows_in * d));
        const float* stats = ln ? ln->stats + 2 * (size_t)c0 * rows_in : nullptr;
        __bf16* fh = hi ? Fh.as<__bf16>() + o : nullptr; __bf16* fl = lo ? Fl.as<__bf16>() + o : nullptr;
        __bf16* th = Th.as<__bf16>() + o;                 __bf16* tl = lo ? Tl.as<__bf16>() + o : nullptr;
        float* kb = kbar ? kbar + (size_t)c0 * (n_tokens / P) * d : nullptr;
        if (padded)
            HIP_TRY(launch_token_pass_pad(src, tok, n, n_live, n_tokens, d, stats, ln ? ln->gamma : nullptr, ln ? ln->beta : nullptr, fh, fl, th, tl, stream));
        else if (ln)
            HIP_TRY(launch_token_pass_ln(src, tok, n, n_tokens, d, stats, ln->gamma, ln->beta, fh, fl, th, tl, stream, kb, P));
        else
            HIP_TRY(launch_token_pass(src, tok, n, n_tokens, d, fh, fl, th, tl, stream, kb, P));
    }
    // (bf16 read in place: Fh is THESE chunks of the caller's buffer, whatever dst0 is)
    *ref = SplitRef{hi ? Fh.as<__bf16>() : static_cast<const __bf16*>(frames_), lo ? Fl.as<__bf16>() : nullptr, Th.as<__bf16>(),
                    lo ? Tl.as<__bf16>() : nullptr};
    return INFV_OK;
}


int short_attention(infv_vqf_s* h, const void* frames_, tok_code tok /* fp16, bf16: only where split_path() holds */, int nb, int n_tokens, const float* xq, bool shared_q,
                    const infv_linear* key, const infv_linear* value, const float* along, float* merged,
                    hipStream_t stream, bool use_cache = false, const SplitRef* pre = nullptr,
                    hipEvent_t along_ready = nullptr /* `along` is produced on another stream: wait here, before the merge */,
                    int inv_nb = 0 /* > 0: batch invariant -- split-K counts and kernel shapes as for inv_nb chunks, whatever nb is */,
                    const int32_t* b_map = nullptr /* device [nb]: chunk b reads chunk b_map[b] of frames_ / *pre (several streams over one block) */,
                    bool t_identity = false /* the transposed plane of *pre holds the sub-batch's chunks in order: only the untransposed operand goes through b_map */,
                    int n_live = 0 /* > 0 and != n_tokens: *pre holds planes padded to n_tokens, only the first n_live keys of a chunk exist */) {
    const infv_vqf_config& c = h->cfg;
    const bool padded = n_live > 0 && n_live != n_tokens;
    if (padded && (!pre || !split_path(h, n_tokens) || n_live > n_tokens)) return fail(INFV_ERR_INVALID, "padded keys need the caller's split planes");
    const int Q = c.n_query, H = c.n_heads, d = c.enc_width, rows = H * Q;
    if (n_tokens < 32 || n_tokens % 32) return fail(INFV_ERR_INVALID, "n_tokens must be a positive multiple of 32");
    const int nb_pick = inv_nb > 0 ? inv_nb : nb;
    int kps = n_tokens;
    int sk = qf_pick_splitk_fill(rows, d, n_tokens, nb_pick, &kps);
    if (split_path(h, n_tokens)) sk = split_gemm_pick_splitk(rows, d, n_tokens, nb_pick, &kps);   // (64-deep k-tiles, its own tile shapes)
    const int nq = shared_q ? 1 : nb;
    // leading dimension of the score matrix: padded by 256 B so that its rows (the A operand of the second
    // contraction, one 128-B line per row per k-tile) do not all map to the same memory channel
    const long ldS = n_tokens + 64;
    const size_t needS = (size_t)nb * rows * ldS * sizeof(float);
    const size_t needO = (size_t)sk * nb * rows * d * sizeof(float);
    const size_t needQt = (size_t)nq * rows * d * sizeof(float);
    HIP_TRY(reserve_all({{h->S, needS}, {h->O, needO}, {h->qt, needQt}}));
    float* qt = h->qt.as<float>();
    if (use_cache) {                                           // nq == 1: the cached query block of layer 0
        const size_t szq = (size_t)rows * d;
        bool grew = false;
        HIP_TRY(reserve_all({{h->c_qt, szq * 4}, {h->c_qh, szq * 2}, {h->c_ql, szq * 2}}, &grew));
        if (grew) h->c_qt_valid = h->c_qsplit_valid = false;
        qt = h->c_qt.as<float>();
    }
    if (!use_cache || !h->c_qt_valid) {
        HIP_TRY(launch_qf_qtilde(xq, nq, Q, H, d, key->w, qt, stream));
        if (use_cache) { h->c_qt_valid = true; h->c_qsplit_valid = false; }
    }
    // Both big contractions ( [H*Q x d x n_tokens] each ) run as split-bf16 (three bf16 MFMA products, fp32 accumulate):
    // their rounding (~1e-5) only feeds the read-out.  INFV_VQF_FP32=1 selects the exact-fp32 MFMA kernels instead.
    if (split_path(h, n_tokens)) {
        const size_t szP = (size_t)nb * rows * n_tokens * 2, szQ = (size_t)nq * rows * d * 2;
        HIP_TRY(reserve_all({{h->sPh, szP}, {h->sPl, szP}, {h->sQh, szQ}, {h->sQl, szQ}}));
        SplitRef sr;
        if (pre) sr = *pre;                                   // the caller split these tokens already (shared by the layers)
        else if (int rc = prepare_split(h, frames_, tok, nb, n_tokens, nullptr, false, &sr, stream)) return rc;
        void* qh = use_cache ? h->c_qh.p : h->sQh.p; void* ql = use_cache ? h->c_ql.p : h->sQl.p;
        if (!use_cache || !h->c_qsplit_valid) {
            HIP_TRY(launch_split_rows(qt, d, (long)nq * rows, d, qh, ql, d, stream));
            if (use_cache) h->c_qsplit_valid = true;
        }
        SplitGemm g{};                                        // S[b] = qt[b] . frames[b]^T
        g.A_hi = static_cast<const __bf16*>(qh); g.A_lo = static_cast<const __bf16*>(ql); g.lda = d; g.strideA = shared_q ? 0 : (long)rows * d;
        g.B_hi = sr.Fh; g.B_lo = sr.Fl; g.ldb = d; g.strideB = (long)n_tokens * d;
        g.C = h->S.as<float>(); g.ldc = ldS; g.strideC = (long)rows * ldS; g.split_stride = 0;
        g.M = rows; g.N = n_tokens; g.K = d; g.k_per_split = d; g.splitk = 1; g.nbatch = nb; g.wide = inv_nb > 0; g.b_map = b_map;
        HIP_TRY(launch_split_gemm(g, stream));
        if (padded) HIP_TRY(launch_softmax_rows_split_pad(h->S.as<float>(), (long)nb * rows, n_live, n_tokens, ldS, h->sPh.p, h->sPl.p, n_tokens, stream));
        else HIP_TRY(launch_softmax_rows_split(h->S.as<float>(), (long)nb * rows, n_tokens, ldS, h->sPh.p, h->sPl.p, n_tokens, stream));
        SplitGemm p{};                                        // O[b] = P[b] . frames[b]
        p.A_hi = h->sPh.as<__bf16>(); p.A_lo = h->sPl.as<__bf16>(); p.lda = n_tokens; p.strideA = (long)rows * n_tokens;
        p.B_hi = sr.Th; p.B_lo = sr.Tl; p.ldb = n_tokens; p.strideB = (long)d * n_tokens;
        p.C = h->O.as<float>(); p.ldc = d; p.strideC = (long)rows * d; p.split_stride = (long)nb * rows * d;
        p.M = rows; p.N = d; p.K = n_tokens; p.k_per_split = kps; p.splitk = sk; p.nbatch = nb; p.wide = inv_nb > 0; p.b_map = t_identity ? nullptr : b_map;
        HIP_TRY(launch_split_gemm(p, stream));
    } else {
    if (tok != INFV_TOKENS_F32) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 tokens reached the fp32 contractions");      // (callers upcast first)
    const float* frames = static_cast<const float*>(frames_);
    QfGemm g{};                                             // S[b] = qt[b] . frames[b]^T
    g.A = qt; g.lda = d; g.strideA = shared_q ? 0 : (long)rows * d;
    g.B[0] = frames; g.ldb = d; g.strideB = (long)n_tokens * d; g.seg_rows = n_tokens;
    g.C = h->S.as<float>(); g.ldc = ldS; g.strideC = (long)rows * ldS; g.split_stride = 0;
    g.M = rows; g.N = n_tokens; g.k_per_split = d; g.splitk = 1; g.nbatch = nb; g.b_map = b_map;
    HIP_TRY(launch_qf_gemm(g, false, stream));
    HIP_TRY(launch_qf_softmax_rows(h->S.as<float>(), (long)nb * rows, n_tokens, ldS, stream));
    QfGemm p{};                                             // O[b] = P[b] . frames[b]
    p.A = h->S.as<float>(); p.lda = ldS; p.strideA = (long)rows * ldS;
    p.B[0] = frames; p.ldb = d; p.strideB = (long)n_tokens * d; p.seg_rows = d;
    p.C = h->O.as<float>(); p.ldc = d; p.strideC = (long)rows * d; p.split_stride = (long)nb * rows * d;
    p.M = rows; p.N = d; p.k_per_split = kps; p.splitk = sk; p.nbatch = nb; p.K = n_tokens; p.b_map = b_map;
    HIP_TRY(launch_qf_gemm(p, true, stream));
    }
    const long o_split_stride = (long)nb * rows * d;
    // per-head value projection as a GEMM batched over (chunk, head): [Q x d] . Wv_h^T -> [Q x 64], then
    // bias + merge with the long-term context in the row epilogue (Qformer.py:298-304)
    HIP_TRY(launch_qf_sum_slabs(h->O.as<float>(), sk, o_split_stride, (long)nb * rows * d, stream));
    const int M2 = nb * Q, hidden = c.hidden;
    int sk2 = 8;
    while (sk2 > 1 && (d % (32 * sk2) || nb_pick * H * sk2 > 4096)) sk2 >>= 1;
    const size_t needP = (size_t)sk2 * M2 * hidden * sizeof(float);
    HIP_TRY(reserve_all({{h->part, needP}}));
    QfGemm v{};
    v.A = h->O.as<float>(); v.lda = d; v.strideA = (long)Q * d; v.strideA2 = (long)rows * d;   // inner = head, outer = chunk
    v.B[0] = value->w; v.ldb = d; v.strideB = 64L * d; v.strideB2 = 0; v.seg_rows = 64;
    v.C = h->part.as<float>(); v.ldc = hidden; v.strideC = 64; v.strideC2 = (long)Q * hidden;
    v.split_stride = (long)M2 * hidden;
    v.M = Q; v.N = 64; v.k_per_split = d / sk2; v.splitk = sk2; v.nbatch = nb * H; v.inner = H;
    HIP_TRY(launch_qf_gemm(v, false, stream));
    QfEpilogue e{};
    e.parts = h->part.as<float>(); e.nsplit = sk2; e.split_stride = (long)M2 * hidden; e.ld_in = hidden;
    e.bias[0] = value->b; e.seg_cols = hidden; e.act = QF_ACT_NONE;
    e.scale = along ? c.alpha : 1.f; e.res_scale = (float)(1.0 - (double)c.alpha);
    e.residual = along; e.ld_res = hidden; e.res_rows = M2;
    e.out = merged; e.ld_out = hidden; e.M = M2; e.width = hidden; e.eps = c.ln_eps;
    if (along_ready) HIP_TRY(hipStreamWaitEvent(stream, along_ready, 0));
    HIP_TRY(launch_qf_epilogue(e, stream));
    return INFV_OK;
}

int ensure_streams(infv_vqf_s* h) {
    if (h->side) return INFV_OK;
    // one of the LTM library's shared worker streams rather than a stream of its own: the runtime multiplexes a process's
    // streams onto 4 hardware queues, and a fifth stream that lands on the caller's queue serialises the two schedules
    // (layer-major path inside bench.py: 0.26 instead of 0.155 ms per chunk)
    if (int rc = shared_worker_stream(&h->side)) return rc;
    HIP_TRY(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming));
    return INFV_OK;
}

// The embedding layer in front of the VideoChat2 encoder (infv_vqf_vc_front.emb): everything a caller can get wrong, checked on the
// host before any launch or memory change -- no id can index outside its table on the device.
int check_front_emb(const char* name, const infv_vqf_vc_front* f, int V, const int32_t* text_len) {
    const auto& e = f->emb;
    if (!e.pos || !e.ln.gamma || !e.ln.beta || !e.query_tokens || e.vocab < 1 || e.max_pos < 1)
        return fail(INFV_ERR_INVALID, "%s: the embedding layer needs word, pos, ln, query_tokens, vocab >= 1 and max_pos >= 1", name);
    long n_text = 0;
    for (int v = 0; v < V; ++v) {
        if (text_len[v] < 0) return fail(INFV_ERR_INVALID, "%s: text_len[%d] = %d is negative", name, v, text_len[v]);
        if (text_len[v] > e.max_pos)
            return fail(INFV_ERR_INVALID, "%s: video %d has %d text tokens, the position table has %d rows", name, v, text_len[v], e.max_pos);
        n_text += text_len[v];
    }
    if (n_text > 0 && !f->input_ids) return fail(INFV_ERR_INVALID, "%s: text tokens without input_ids", name);
    long i = 0;
    for (int v = 0; v < V; ++v)
        for (int t = 0; t < text_len[v]; ++t, ++i)
            if (f->input_ids[i] < 0 || f->input_ids[i] >= e.vocab)
                return fail(INFV_ERR_INVALID, "%s: video %d: input id %d at position %d is outside [0, %d)", name, v, f->input_ids[i], t, e.vocab);
    return INFV_OK;
}

// Packed encoder input rows of V videos, video v's n_query + text_len[v] rows (query rows first), into out: the row table goes
// through the handle's pinned buffer, whose reuse waits for the event recorded behind the previous call's copy.
int run_embed(infv_vqf_s* h, const infv_vqf_vc_front* f, int V, const int32_t* text_len, float* out, hipStream_t stream) {
    const int Q = h->cfg.n_query, Hd = h->cfg.hidden;
    long n = 0;
    for (int v = 0; v < V; ++v) n += Q + text_len[v];
    if (n == 0) return INFV_OK;
    if (n > 0x3fffffffL) return fail(INFV_ERR_UNSUPPORTED, "embedding layer: %ld rows in one call", n);
    if (!h->ev_ids) HIP_TRY(hipEventCreateWithFlags(&h->ev_ids, hipEventDisableTiming));
    if (h->ids_in_flight) { HIP_TRY(hipEventSynchronize(h->ev_ids)); h->ids_in_flight = false; }   // the last copy has read the buffer
    if ((size_t)(2 * n) > h->ids_pin_n) {
        if (h->ids_pin) { HIP_TRY(hipHostFree(h->ids_pin)); h->ids_pin = nullptr; h->ids_pin_n = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->ids_pin), (size_t)(2 * n) * sizeof(int32_t), hipHostMallocDefault));
        h->ids_pin_n = (size_t)(2 * n);
    }
    HIP_TRY(reserve_all({{h->ids_dev, (size_t)(2 * n) * sizeof(int32_t)}}));
    int32_t* src = h->ids_pin; int32_t* pos = h->ids_pin + n;
    long m = 0, i = 0;
    for (int v = 0; v < V; ++v) {
        for (int q = 0; q < Q; ++q, ++m) { src[m] = -(q + 1); pos[m] = 0; }
        for (int t = 0; t < text_len[v]; ++t, ++m, ++i) { src[m] = f->input_ids[i]; pos[m] = t; }   // positions start at 0 at the first text token
    }
    HIP_TRY(hipMemcpyAsync(h->ids_dev.p, h->ids_pin, (size_t)(2 * n) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(h->ev_ids, stream));
    h->ids_in_flight = true;
    HIP_TRY(launch_qf_vc_embed(f->emb.word, f->emb.pos, f->emb.query_tokens, f->emb.ln.gamma, f->emb.ln.beta, h->cfg.ln_eps,
                               h->ids_dev.as<int32_t>(), h->ids_dev.as<int32_t>() + n, (int)n, Hd, out, stream));
    return INFV_OK;
}

// a table of packed offsets t [n + 1] (cu, fcu): starts at 0, never decreases
int check_offsets(const char* name, const char* tab, const int32_t* t, int n) {
    if (t[0] != 0) return fail(INFV_ERR_INVALID, "%s: %s[0] = %d, not 0", name, tab, t[0]);
    for (int i = 0; i < n; ++i)
        if (t[i + 1] < t[i])
            return fail(INFV_ERR_INVALID, "%s: %s is not non-decreasing (%s[%d] = %d > %s[%d] = %d)", name, tab, tab, i, t[i], tab, i + 1, t[i + 1]);
    return INFV_OK;
}

// the n memory handles of a batched call: none null, none twice (`per`: what each memory belongs to beside its video)
int check_distinct_handles(const char* name, const infv_ltm_handle* ltm, int n, const char* per) {
    std::vector<infv_ltm_handle> all(ltm, ltm + n);
    for (int i = 0; i < n; ++i)
        if (!all[i]) return fail(INFV_ERR_INVALID, "%s: LTM handle %d is null", name, i);
    std::sort(all.begin(), all.end());
    if (std::adjacent_find(all.begin(), all.end()) != all.end())
        return fail(INFV_ERR_INVALID, "%s: an LTM handle appears twice (every video and %s needs its own memory)", name, per);
    return INFV_OK;
}

// embeddings of the video Q-former: LayerNorm of the learned query tokens (Qformer.py:108-112; chunk-independent) -> h->h_a
int embed_query_tokens(infv_vqf_s* h, const infv_vqf_weights* w, hipStream_t stream) {
    const int Hd = h->cfg.hidden;
    QfEpilogue e{};
    e.parts = w->query_tokens; e.nsplit = 1; e.ld_in = Hd; e.seg_cols = Hd; e.scale = 1.f; e.res_scale = 1.f;
    e.gamma = w->emb_ln.gamma; e.beta = w->emb_ln.beta; e.eps = h->cfg.ln_eps;
    e.out = h->h_a.as<float>(); e.ld_out = Hd; e.M = h->cfg.n_query; e.width = Hd; e.res_rows = 1;
    HIP_TRY(launch_qf_epilogue(e, stream));
    return INFV_OK;
}

// Self-attention over the query tokens of the nb chunks at x + output dense + LayerNorm -> h1 (Qformer.py:442-470 -> BertAttention),
// then the cross query -> xq.  whole: through the row-block scratch of the layer-major calls, else the one-chunk scratch.
int query_self_block(infv_vqf_s* h, const infv_vqf_layer& L, const float* x, int nb, bool inv, bool whole, float* h1, float* xq, hipStream_t stream) {
    const int Q = h->cfg.n_query, Hd = h->cfg.hidden;
    float* qkv_y = (whole ? h->vqkv : h->qkv).as<float>(); float* sa = (whole ? h->vsa : h->sa).as<float>();
    LinearCall qkv{x, nb * Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
    qkv.inv = inv; qkv.y = qkv_y;
    if (int rc = run_linear(h, qkv, stream)) return rc;
    HIP_TRY(launch_qf_self_attention(qkv_y, nb, Q, h->cfg.n_heads, sa, stream));
    LinearCall so{sa, nb * Q, Hd, {&L.self_o}, 1, Hd};
    so.inv = inv; so.residual = x; so.res_rows = nb * Q; so.ln = &L.self_ln; so.y = h1;
    if (int rc = run_linear(h, so, stream)) return rc;
    LinearCall q{h1, nb * Q, Hd, {&L.x_q}, 1, Hd};
    q.inv = inv; q.y = xq;
    return run_linear(h, q, stream);
}

}  // namespace

extern "C" {

int infv_vqf_create(const infv_vqf_config* cfg, infv_vqf_handle* out) {
    if (!cfg || !out) return fail(INFV_ERR_INVALID, "null argument");
    if (int rc = check_cfg(*cfg)) return rc;
    infv_vqf_s* h = new (std::nothrow) infv_vqf_s();
    if (!h) return fail(INFV_ERR_INVALID, "out of host memory");
    h->cfg = *cfg;
    {   // INFV_VQF_FUSE=0 (read per handle, for A/B tests): separate pooling pass + one split pass per layer, as in round 1
        const char* e = getenv("INFV_VQF_FUSE");
        h->fuse = !e || atoi(e) != 0;
        if (const char* g = getenv("INFV_VQF_SPLIT_CACHE_GB")) h->split_cache_gb = atof(g);
    }
    HIP_TRY(hipGetDevice(&h->dev));
    const infv_vqf_config& c = *cfg;
    const size_t row = (size_t)c.n_query * sizeof(float);
    hipError_t e = hipSuccess;
    auto rs = [&](DeviceBuf& b, size_t n) { if (e == hipSuccess) e = b.reserve(n); };
    rs(h->h_a, row * c.hidden); rs(h->h_b, row * c.hidden); rs(h->h1, row * c.hidden); rs(h->h2, row * c.hidden);
    rs(h->qkv, row * 3 * c.hidden); rs(h->sa, row * c.hidden); rs(h->xq, row * c.hidden); rs(h->along, row * c.hidden);
    rs(h->merged, row * c.hidden); rs(h->inter, row * c.inter);
    if (e != hipSuccess) { delete h; return fail(INFV_ERR_HIP, "workspace allocation failed: %s", hipGetErrorString(e)); }
    *out = h;
    return INFV_OK;
}

int infv_vqf_destroy(infv_vqf_handle h) {
    if (!h) return INFV_OK;
    (void)hipDeviceSynchronize();
    delete h;
    return INFV_OK;
}

int infv_vqf_set_precision(infv_vqf_handle h, int32_t exact_fp32) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    h->exact_fp32 = exact_fp32 != 0;
    return INFV_OK;
}

int infv_vqf_set_token_dtype(infv_vqf_handle h, int32_t dtype) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    if (!token_dtype_known(dtype)) return fail(INFV_ERR_INVALID, "set_token_dtype: unknown token dtype %d", dtype);
    h->tok = static_cast<tok_code>(dtype);
    return INFV_OK;
}

int infv_vqf_set_weights_epoch(infv_vqf_handle h, uint64_t epoch) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    h->epoch = epoch;
    return INFV_OK;
}

int infv_vqf_set_linear_precision(infv_vqf_handle h, int32_t mode) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 2) return fail(INFV_ERR_INVALID, "set_linear_precision: unknown mode %d (0 fp32, 1 split-bf16, 2 fp16)", mode);
    if (mode != h->lin_mode)
        if (int rc = drop_linear_planes(h)) return rc;        // the planes are the old mode's
    h->lin_mode = mode;
    return INFV_OK;
}

int infv_vqf_set_attention_precision(infv_vqf_handle h, int32_t mode) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 1) return fail(INFV_ERR_INVALID, "set_attention_precision: unknown mode %d (0 split-bf16 / fp32, 1 fp16)", mode);
    if (mode != h->attn_mode)
        if (int rc = drop_linear_planes(h)) return rc;        // (one cache, one rule: a change of mode drops it)
    h->attn_mode = mode;
    return INFV_OK;
}

int infv_vqf_linear(infv_vqf_handle h, const float* x, int32_t M, int32_t K, const infv_linear* lin, int32_t n_lin, int32_t n_out,
                    int32_t act, const float* residual, int32_t res_rows, const infv_layernorm* ln, float* y, void* stream) {
    // ---- every refusal before any launch or memory change ----
    if (!h || !x || !lin || !y) return fail(INFV_ERR_INVALID, "linear: null handle, x, lin or y");
    if (n_lin < 1 || n_lin > kQfMaxSeg) return fail(INFV_ERR_INVALID, "linear: n_lin = %d outside 1..%d", n_lin, kQfMaxSeg);
    if (M < 1) return fail(INFV_ERR_INVALID, "linear: M = %d, must be >= 1", M);
    if (K < 64 || K % 64 || n_out < 64 || n_out % 64) return fail(INFV_ERR_UNSUPPORTED, "linear: K and n_out must be positive multiples of 64");
    if (K > 4096 || (long)n_lin * n_out > 4096) return fail(INFV_ERR_UNSUPPORTED, "linear: row widths above 4096 are not supported");
    if ((long)M * n_lin * n_out > 0x7fffffffL) return fail(INFV_ERR_UNSUPPORTED, "linear: %d rows of %d in one call", M, n_lin * n_out);
    if (act != QF_ACT_NONE && act != QF_ACT_GELU) return fail(INFV_ERR_INVALID, "linear: unknown activation %d", act);
    if (residual && res_rows < 1) return fail(INFV_ERR_INVALID, "linear: res_rows = %d, must be >= 1", res_rows);
    if (ln && (!ln->gamma || !ln->beta)) return fail(INFV_ERR_INVALID, "linear: LayerNorm without gamma or beta");
    bool aligned = aligned16(x) && aligned16(y) && aligned16(residual) && (!ln || (aligned16(ln->gamma) && aligned16(ln->beta)));
    for (int i = 0; i < n_lin; ++i) {
        if (!lin[i].w) return fail(INFV_ERR_INVALID, "linear: lin[%d].w is null", i);
        aligned = aligned && aligned16(lin[i].w) && aligned16(lin[i].b);
    }
    if (!aligned) return fail(INFV_ERR_INVALID, "linear: every pointer must be 16-byte aligned");
    LinearCall c{x, M, K, {}, n_lin, n_out};
    for (int i = 0; i < n_lin; ++i) c.lin[i] = &lin[i];
    c.act = act; c.residual = residual; c.res_rows = residual ? res_rows : 1; c.ln = ln; c.y = y; c.inv = true; c.reduced = true;
    return run_linear(h, c, static_cast<hipStream_t>(stream));
}

int infv_vqf_short_attention(infv_vqf_handle h, const void* frames, int32_t n_tokens, const float* xq,
                             const infv_linear* key, const infv_linear* value, const float* a_long,
                             float* merged, void* stream) {
    if (!h || !frames || !xq || !key || !value || !merged || !key->w || !value->w || !value->b)
        return fail(INFV_ERR_INVALID, "null argument");
    if (int rc = refuse_reduced(h, "short_attention")) return rc;
    tok_code tok = h->tok;
    if (tok != INFV_TOKENS_F32 && !aligned16(frames)) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 frames must be 16-byte aligned");
    if (n_tokens < 32 || n_tokens % 32) return fail(INFV_ERR_INVALID, "n_tokens must be a positive multiple of 32");
    if (int rc = fp32_tokens_unless_split(h, frames, tok, n_tokens, (size_t)n_tokens * h->cfg.enc_width, static_cast<hipStream_t>(stream))) return rc;
    return short_attention(h, frames, tok, 1, n_tokens, xq, false, key, value, a_long, merged, static_cast<hipStream_t>(stream));
}

int infv_vqf_encode_chunk(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t T,
                          const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, void* stream_) {
    if (!h || !frames || !w) return fail(INFV_ERR_INVALID, "null argument");
    if (int rc = refuse_reduced(h, "encode_chunk")) return rc;
    const infv_vqf_config& c = h->cfg;
    if (int rc = check_layer_cfg(c)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool use_ltm = c.alpha != 1.0f;                      // Qformer.py:220-223
    if (use_ltm && !ltm) return fail(INFV_ERR_INVALID, "alpha != 1 needs the per-layer LTM handles");
    if (T < 1) return fail(INFV_ERR_INVALID, "T must be >= 1");
    if (llama_out && (c.proj_out <= 0 || !w->llama_proj.w)) return fail(INFV_ERR_INVALID, "llama_out without llama_proj");
    const int Q = c.n_query, Hd = c.hidden, n_tokens = T * c.tokens_per_frame;
    tok_code tok = h->tok;
    if (tok != INFV_TOKENS_F32 && !aligned16(frames)) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 frames must be 16-byte aligned");
    if (use_ltm)
        if (int rc = ensure_streams(h)) return rc;
    if (int rc = fp32_tokens_unless_split(h, frames, tok, n_tokens, (size_t)n_tokens * c.enc_width, stream)) return rc;

    // The prefix of layer 0 (embedding LayerNorm -> self-attention block -> cross query) depends on the weights only,
    // not on the chunk: with a non-zero weights epoch it is computed once and reused until the epoch changes.
    const bool caching = h->epoch != 0;
    const bool prefix_cached = caching && h->c_valid && h->c_epoch == h->epoch;
    if (caching && !prefix_cached) {
        const size_t sz = (size_t)Q * Hd * sizeof(float);
        HIP_TRY(reserve_all({{h->c_h1, sz}, {h->c_xq, sz}}));
        h->c_valid = false; h->c_qt_valid = false; h->c_qsplit_valid = false;
    }
    if (!prefix_cached)
        if (int rc = embed_query_tokens(h, w, stream)) return rc;
    float* hcur = h->h_a.as<float>();
    float* hnext = h->h_b.as<float>();

    if (use_ltm) {
        HIP_TRY(reserve_all({{h->kbar, (size_t)T * c.enc_width * sizeof(float)}}));
        if (new_video)
            for (int l = 0; l < c.n_layers; ++l)
                if (int rc = infv_ltm_reset(ltm[l])) return rc;
    }
    // one pass over the chunk's tokens serves the pooling and the split operands of every layer's short-term attention
    SplitRef sref; const SplitRef* pre = nullptr;
    const bool fused_pool = h->fuse && split_path(h, n_tokens) && 64 % c.tokens_per_frame == 0;
    if (h->fuse && split_path(h, n_tokens)) {
        if (int rc = prepare_split(h, frames, tok, 1, n_tokens, use_ltm && fused_pool ? h->kbar.as<float>() : nullptr, false, &sref, stream)) return rc;
        pre = &sref;
    }
    if (use_ltm && !fused_pool) {
        // (the LTM handle's token dtype is sticky state an earlier caller may have set)
        if (int rc = infv_ltm_set_token_dtype(ltm[0], tok)) return rc;
        if (int rc = infv_ltm_pool(ltm[0], frames, T, h->kbar.as<float>(), stream_)) return rc;   // shared by all layers
    }

    for (int l = 0; l < c.n_layers; ++l) {
        const infv_vqf_layer& L = w->layer[l];
        const bool l0c = caching && l == 0;                   // this layer's prefix lives in the cache buffers
        float* h1 = l0c ? h->c_h1.as<float>() : h->h1.as<float>();
        float* xqb = l0c ? h->c_xq.as<float>() : h->xq.as<float>();
        if (!(l0c && prefix_cached)) {
            if (int rc = query_self_block(h, L, hcur, 1, false, false, h1, xqb, stream)) return rc;
            if (l0c) { h->c_valid = true; h->c_epoch = h->epoch; }
        }
        const float* along = nullptr;
        hipEvent_t along_ready = nullptr;
        if (use_ltm) {
            // The memory step and the short-term attention both start from the cross query and meet only in the merge
            // (Qformer.py:216-223 vs :225-302, :303-304): the step's three launches go to the shared worker stream and run
            // beside the attention's contractions; the merge epilogue waits for them.
            infv_ltm_proj pr{};
            pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
            const double* ul = u ? u + (size_t)l * c.nb_samples : nullptr;
            HIP_TRY(hipEventRecord(h->ev_main, stream));              // cross query, pooled frames, the previous layer's merge
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
            if (int rc = infv_ltm_step(ltm[l], h->kbar.as<float>(), T, xqb, Q, &pr, ul,
                                       h->along.as<float>(), h->side)) return rc;
            HIP_TRY(hipEventRecord(h->ev_side, h->side));
            along = h->along.as<float>();
            along_ready = h->ev_side;
        }
        if (int rc = short_attention(h, frames, tok, 1, n_tokens, xqb, false, &L.x_k, &L.x_v, along,
                                     h->merged.as<float>(), stream, l0c, pre, along_ready)) return rc;
        LinearCall xo{h->merged.as<float>(), Q, Hd, {&L.x_o}, 1, Hd};
        xo.residual = h1; xo.res_rows = Q; xo.ln = &L.x_ln; xo.y = h->h2.as<float>();
        if (int rc = run_linear(h, xo, stream)) return rc;
        // ---- query FFN (Qformer.py:519-522)
        LinearCall fi{h->h2.as<float>(), Q, Hd, {&L.ffn_in}, 1, c.inter};
        fi.act = QF_ACT_GELU; fi.y = h->inter.as<float>();
        if (int rc = run_linear(h, fi, stream)) return rc;
        LinearCall fo{h->inter.as<float>(), Q, c.inter, {&L.ffn_out}, 1, Hd};
        fo.residual = h->h2.as<float>(); fo.res_rows = Q; fo.ln = &L.ffn_ln; fo.y = hnext;
        if (int rc = run_linear(h, fo, stream)) return rc;
        float* t = hcur; hcur = hnext; hnext = t;
    }
    if (hidden_out)
        HIP_TRY(hipMemcpyAsync(hidden_out, hcur, (size_t)Q * Hd * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (llama_out) {
        LinearCall pj{hcur, Q, Hd, {&w->llama_proj}, 1, c.proj_out};
        pj.y = llama_out;
        if (int rc = run_linear(h, pj, stream)) return rc;
    }
    return INFV_OK;
}

// chunks per sub-batch of the short-term attention of a layer-major call over C chunks
static int pick_short_nb(const infv_vqf_s* h, int C, int n_tokens) {
    const infv_vqf_config& c = h->cfg;
    const int Q = c.n_query;
    int NB = C;
    if (C > 8) {
        auto fill = [](long wgs) { return (double)wgs / (double)(((wgs + 255) / 256) * 256); };
        // with the 384 x 256 kernel (split path, whole tiles): workgroups of the scores contraction, and of the read-out with the
        // split-K count that fills best -- both should come out as whole rounds (headline: 32 chunks = 1024 and 96 x 8)
        const long ts = split_path(h, n_tokens) ? split_gemm_wide_tile_count(c.n_heads * Q, n_tokens) : 0;
        const long tr = split_path(h, n_tokens) ? split_gemm_wide_tile_count(c.n_heads * Q, c.enc_width) : 0;
        const int tiles = ((c.n_heads * Q + 127) / 128) * ((c.enc_width + 127) / 128);
        double best = -1.0;
        for (int nb = 8; nb <= 32 && nb <= C; ++nb) {
            double eff;
            if (ts > 0 && tr > 0) {
                double er = 0.0;
                for (int sk = 1; sk <= 16; ++sk) er = std::max(er, fill(tr * nb * sk) - 0.004 * sk);
                eff = 0.5 * (fill(ts * nb) + er);
            } else {
                eff = fill((long)tiles * nb);
            }
            if (eff >= best - 1e-9) { best = eff; NB = nb; }
        }
    }
    {
        static const int nb_env = exp_int("INFV_VQF_NB", 0);   // (sweeps)
        if (nb_env > 0) NB = nb_env < C ? nb_env : C;
    }
    return NB;
}

// ---- steps shared by the layer-major calls (encode_impl and the stages of vc_impl) ----

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

// the cached planes of a whole call, from chunk c0 on
static SplitRef split_ref_at(const SplitRef& w, int c0, long chunk_k) {
    const long o = (long)c0 * chunk_k;
    return SplitRef{w.Fh + o, w.Fl ? w.Fl + o : nullptr, w.Th + o, w.Tl ? w.Tl + o : nullptr};
}

// u[:, l, :] of u [C][n_layers_in_u][S] -> contiguous [C][S] in h->vu, for the one-layer memory handles (u == nullptr: nothing)
static int ltm_u_slice(infv_vqf_s* h, const double* u, int l, int n_layers_in_u, int C, hipStream_t stream) {
    if (!u) return INFV_OK;
    const size_t S = (size_t)h->cfg.nb_samples;
    HIP_TRY(hipMemcpy2DAsync(h->vu.p, S * sizeof(double), u + (size_t)l * S, (size_t)n_layers_in_u * S * sizeof(double), S * sizeof(double),
                             (size_t)C, hipMemcpyDeviceToDevice, stream));
    return INFV_OK;
}

// vmerged = alpha * vshort + (1 - alpha) * valong over the M rows of the whole call
static int alpha_merge(infv_vqf_s* h, long M, hipStream_t stream) {
    const infv_vqf_config& c = h->cfg;
    const long Hd = c.hidden;
    for (long m0 = 0; m0 < M; m0 += kMergeRows) {
        QfEpilogue em{};
        em.parts = h->vshort.as<float>() + m0 * Hd; em.nsplit = 1; em.ld_in = Hd; em.seg_cols = c.hidden;
        em.scale = c.alpha; em.res_scale = (float)(1.0 - (double)c.alpha);
        em.residual = h->valong.as<float>() + m0 * Hd; em.ld_res = Hd; em.res_rows = (int)(M - m0 < kMergeRows ? M - m0 : kMergeRows);
        em.out = h->vmerged.as<float>() + m0 * Hd; em.ld_out = Hd; em.M = em.res_rows; em.width = c.hidden; em.eps = c.ln_eps;
        HIP_TRY(launch_qf_epilogue(em, stream));
    }
    return INFV_OK;
}

// The tail of a call: out (nullptr: scratch, only the mean is wanted) = the rows of h->vA through `proj`, block by block; then
// mean (nullptr: none) = the mean of every video's chunks (cu [V + 1]), or of all chunks (cu == nullptr).
static int project_and_mean(infv_vqf_s* h, RowBlocks blocks, const infv_linear* proj, bool inv, float* out, float* mean, const int32_t* cu,
                            int V, hipStream_t stream) {
    const infv_vqf_config& c = h->cfg;
    const long row = (long)c.n_query * c.proj_out;             // projected elements of a chunk
    if (!out) {
        HIP_TRY(reserve_all({{h->S, (size_t)blocks.C * row * sizeof(float)}}));
        out = h->S.as<float>();
    }
    for (RowBlock b : blocks) {
        LinearCall pj{h->vA.as<float>() + b.r0, b.nb * c.n_query, c.hidden, {proj}, 1, c.proj_out};
        pj.inv = inv; pj.y = out + b.c0 * row;
        if (int rc = run_linear(h, pj, stream)) return rc;
    }
    if (mean && cu) HIP_TRY(launch_qf_mean_segments(out, cu, V, row, mean, stream));
    else if (mean) HIP_TRY(launch_qf_mean(out, blocks.C, row, mean, stream));
    return INFV_OK;
}

// The layer-major body of infv_vqf_encode_video (multi = false: one video, ltm [n_layers]) and infv_vqf_encode_videos (multi:
// V videos packed by the host array cu, ltm [V][n_layers]; every choice that shapes a GEMM or contraction is taken from
// per-chunk quantities or constants, and each layer's memories step through infv_ltm_steps_videos).
static int encode_impl(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t n_chunks, int32_t T,
                       const infv_vqf_weights* w, const double* u, int32_t new_video, float* hidden_out, float* llama_out,
                       float* llama_mean, void* stream_, int32_t V, const int32_t* cu, bool multi) {
    const infv_vqf_config& c = h->cfg;
    if (int rc = check_layer_cfg(c)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool use_ltm = c.alpha != 1.0f;
    if (use_ltm && !ltm) return fail(INFV_ERR_INVALID, "alpha != 1 needs the per-layer LTM handles");
    if (T < 1) return fail(INFV_ERR_INVALID, "T must be >= 1");
    if ((llama_out || llama_mean) && (c.proj_out <= 0 || !w->llama_proj.w)) return fail(INFV_ERR_INVALID, "llama output without llama_proj");
    tok_code tok = h->tok;
    if (tok != INFV_TOKENS_F32 && !aligned16(frames)) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 frames must be 16-byte aligned");
    if (int rc = ensure_streams(h)) return rc;
    const int Q = c.n_query, Hd = c.hidden, C = n_chunks, S = c.nb_samples;
    const int n_tokens = T * c.tokens_per_frame;
    const long chunk_k = (long)n_tokens * c.enc_width;
    if (int rc = fp32_tokens_unless_split(h, frames, tok, n_tokens, (size_t)C * chunk_k, stream)) return rc;
    const long M = (long)C * Q;                               // rows of the whole-video activations
    // ---- workspaces: whole-video activations + per-block scratch ----
    const int rb_max = multi ? kRowBlockVideos : kRowBlockVideo;   // (batch invariant: the row count does not shape the GEMMs)
    const int RB = C < rb_max ? C : rb_max;                   // chunks per row block of the query-token GEMMs
    // chunks per sub-batch of the short-term attention: the second contraction has few, long tiles per chunk
    // (rows/128 x d/128 = 18 at the headline shape, K = T*P), so pick the count whose tile total fills whole rounds
    // of the 256 CUs (16 chunks = 288 tiles ran at 56 % of 14 chunks' rate per tile)
    const int NB = pick_short_nb(h, C, n_tokens);
    {
        const size_t act = (size_t)M * Hd * sizeof(float), row = (size_t)Q * Hd * sizeof(float), f = sizeof(float);
        HIP_TRY(reserve_all({{h->vA, act}, {h->v1, act}, {h->v2, act}, {h->vxq, act}, {h->vshort, act}, {h->vmerged, act},
                             {h->valong, use_ltm ? act : 0}, {h->vu, use_ltm ? (size_t)C * S * sizeof(double) : 0},
                             {h->vkbar, use_ltm ? (size_t)C * T * c.enc_width * f : 0}, {h->vqkv, (size_t)RB * 3 * row},
                             {h->vsa, (size_t)RB * row}, {h->vinter, (size_t)RB * Q * c.inter * f}, {h->v_h1s, row}, {h->v_xqs, row}}));
    }
    // ---- ONE pass over the whole video's frame tokens: split-bf16 operands of every layer's short-term attention and
    //      the frame means of every layer's memory.  The copies take 2 x the tokens' bytes (12.7 GB for the headline's
    //      252 chunks): kept for the call when they fit INFV_VQF_SPLIT_CACHE_GB (default 64 of the 288 GB). ----
    SplitRef wref{}; bool have_w = false, have_kbar = false;
    {
        const double budget_gb = h->split_cache_gb;
        const double need_gb = plane_bytes(tok, false) * (double)C * (double)chunk_k / 1e9;
        if (h->fuse && split_path(h, n_tokens) && need_gb <= budget_gb) {
            have_kbar = use_ltm && 64 % c.tokens_per_frame == 0;
            if (int rc = prepare_split(h, frames, tok, C, n_tokens, have_kbar ? h->vkbar.as<float>() : nullptr, true, &wref, stream)) return rc;
            have_w = true;
        }
    }
    const RowBlocks row_blocks{C, RB, (long)Q * Hd}, short_blocks{C, NB, (long)Q * Hd};
    const int ltm_dtype = tok;   // (what the fallbacks below hand the memories)
    if (multi && use_ltm && !have_kbar) {                    // the frame means every layer's memories step from
        if (int rc = infv_ltm_set_token_dtype(ltm[0], ltm_dtype)) return rc;
        if (int rc = infv_ltm_pool(ltm[0], frames, (int64_t)C * T, h->vkbar.as<float>(), stream_)) return rc;
    }
    std::vector<infv_ltm_handle> hs_l(multi ? V : 0);         // layer l's handles of every video
    auto layer_handles = [&](int l) { for (int v = 0; v < V; ++v) hs_l[v] = ltm[(size_t)v * c.n_layers + l]; };
    float* vA = h->vA.as<float>(); float* v1 = h->v1.as<float>(); float* v2 = h->v2.as<float>();
    float* vxq = h->vxq.as<float>(); float* valong = h->valong.as<float>();
    float* vshort = h->vshort.as<float>(); float* vmerged = h->vmerged.as<float>();

    if (int rc = embed_query_tokens(h, w, stream)) return rc;

    auto ltm_u = [&](int l) { return ltm_u_slice(h, u, l, c.n_layers, C, stream); };

    for (int l = 0; l < c.n_layers; ++l) {
        const infv_vqf_layer& L = w->layer[l];
        infv_ltm_proj pr{};
        pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
        const bool shared = (l == 0);                         // layer 0: the hidden states entering it do not depend on the chunk
        const float* res1;                                    // residual / input of the cross-attention block
        int res1_rows;
        if (shared) {
            // ---- self-attention block + cross query once ----
            if (int rc = query_self_block(h, L, h->h_a.as<float>(), 1, multi, false, h->v_h1s.as<float>(), h->v_xqs.as<float>(), stream)) return rc;
            res1 = h->v_h1s.as<float>(); res1_rows = Q;
            // ---- long-term memory of every chunk with the constant query: the whole-video fast path ----
            if (use_ltm && multi) {                           // every video's memory with the shared query, in lockstep
                if (int rc = ltm_u(l)) return rc;
                layer_handles(l);
                if (int rc = infv_ltm_steps_videos(hs_l.data(), V, cu, h->vkbar.as<float>(), T, h->v_xqs.as<float>(), 0, Q, &pr,
                                                   u ? h->vu.as<double>() : nullptr, new_video, valong, stream_)) return rc;
            } else if (use_ltm) {
                if (int rc = ltm_u(l)) return rc;
                if (have_kbar) {
                    if (int rc = infv_ltm_consolidate_pooled(ltm[l], h->vkbar.as<float>(), C, T, h->v_xqs.as<float>(), Q, &pr,
                                                             u ? h->vu.as<double>() : nullptr, new_video, valong, stream_)) return rc;
                } else if (int rc = infv_ltm_set_token_dtype(ltm[l], ltm_dtype)) {
                    return rc;
                } else if (int rc = infv_ltm_consolidate(ltm[l], frames, C, T, h->v_xqs.as<float>(), Q, &pr,
                                                         u ? h->vu.as<double>() : nullptr, new_video, valong, stream_)) return rc;
            }
            // ---- short-term attention, merged with the long-term context ----
            for (RowBlock b : short_blocks) {
                const SplitRef sr = split_ref_at(wref, b.c0, chunk_k);   // the cached split of chunks c0.. (else: split per sub-batch)
                if (int rc = short_attention(h, tok_at(frames, tok, b.c0 * chunk_k), tok, b.nb, n_tokens, h->v_xqs.as<float>(), true, &L.x_k, &L.x_v,
                                             use_ltm ? valong + b.r0 : nullptr, vmerged + b.r0, stream,
                                             false, have_w ? &sr : nullptr, nullptr, multi ? kInvariantNb : 0)) return rc;
            }
        } else {
            // ---- self-attention block + cross query of every chunk (row blocks) ----
            for (RowBlock b : row_blocks)
                if (int rc = query_self_block(h, L, vA + b.r0, b.nb, multi, true, v1 + b.r0, vxq + b.r0, stream)) return rc;
            res1 = v1; res1_rows = (int)M;
            // ---- long-term memory with per-chunk queries: the sequential per-call chain, on the side stream, while
            //      the main stream runs this layer's short-term attention ----
            if (use_ltm) {
                if (int rc = ltm_u(l)) return rc;
                HIP_TRY(hipEventRecord(h->ev_main, stream));
                HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
                if (multi) {                                  // every video's memory with its chunks' queries, in lockstep
                    layer_handles(l);
                    if (int rc = infv_ltm_steps_videos(hs_l.data(), V, cu, h->vkbar.as<float>(), T, vxq, 1, Q, &pr,
                                                       u ? h->vu.as<double>() : nullptr, new_video, valong, h->side)) return rc;
                } else {
                if (new_video)
                    if (int rc = infv_ltm_reset(ltm[l])) return rc;
                if (!have_kbar) {
                    if (int rc = infv_ltm_set_token_dtype(ltm[l], ltm_dtype)) return rc;
                    if (int rc = infv_ltm_pool(ltm[l], frames, (int64_t)C * T, h->vkbar.as<float>(), h->side)) return rc;
                }
                // per-chunk queries: new-row projections of all chunks in one GEMM, then the chain chunk by chunk
                if (int rc = infv_ltm_steps(ltm[l], h->vkbar.as<float>(), C, T, vxq, Q, &pr, u ? h->vu.as<double>() : nullptr,
                                            valong, h->side)) return rc;
                }
                HIP_TRY(hipEventRecord(h->ev_side, h->side));
            }
            for (RowBlock b : short_blocks) {
                const SplitRef sr = split_ref_at(wref, b.c0, chunk_k);
                if (int rc = short_attention(h, tok_at(frames, tok, b.c0 * chunk_k), tok, b.nb, n_tokens, vxq + b.r0, false, &L.x_k, &L.x_v,
                                             nullptr, (use_ltm ? vshort : vmerged) + b.r0, stream, false,
                                             have_w ? &sr : nullptr, nullptr, multi ? kInvariantNb : 0)) return rc;
            }
            if (use_ltm) {
                HIP_TRY(hipStreamWaitEvent(stream, h->ev_side, 0));
                if (int rc = alpha_merge(h, M, stream)) return rc;
            }
        }
        // ---- cross-attention output + query FFN of every chunk (row blocks) ----
        for (RowBlock b : row_blocks) {
            const int nb = b.nb; const long r0 = b.r0;
            LinearCall xo{vmerged + r0, nb * Q, Hd, {&L.x_o}, 1, Hd};
            xo.inv = multi; xo.residual = shared ? res1 : res1 + r0; xo.res_rows = shared ? res1_rows : nb * Q; xo.ln = &L.x_ln; xo.y = v2 + r0;
            if (int rc = run_linear(h, xo, stream)) return rc;
            LinearCall fi{v2 + r0, nb * Q, Hd, {&L.ffn_in}, 1, c.inter};
            fi.inv = multi; fi.act = QF_ACT_GELU; fi.y = h->vinter.as<float>();
            if (int rc = run_linear(h, fi, stream)) return rc;
            LinearCall fo{h->vinter.as<float>(), nb * Q, c.inter, {&L.ffn_out}, 1, Hd};
            fo.inv = multi; fo.residual = v2 + r0; fo.res_rows = nb * Q; fo.ln = &L.ffn_ln; fo.y = vA + r0;
            if (int rc = run_linear(h, fo, stream)) return rc;
        }
    }
    if (hidden_out)
        HIP_TRY(hipMemcpyAsync(hidden_out, vA, (size_t)M * Hd * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (llama_out || llama_mean)
        if (int rc = project_and_mean(h, row_blocks, &w->llama_proj, multi, llama_out, llama_mean, multi ? cu : nullptr, V, stream)) return rc;
    return INFV_OK;
}

int infv_vqf_encode_video(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t n_chunks,
                          int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, float* llama_mean, void* stream_) {
    if (!h || !frames || !w || n_chunks < 1) return fail(INFV_ERR_INVALID, "bad argument");
    if (int rc = refuse_reduced(h, "encode_video")) return rc;
    return encode_impl(h, ltm, frames, n_chunks, T, w, u, new_video, hidden_out, llama_out, llama_mean, stream_, 1, nullptr, false);
}

int infv_vqf_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                           int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video, float* hidden_out,
                           float* llama_out, float* llama_mean, void* stream_) {
    // ---- validation before any device work or memory change ----
    if (!h || !cu || !w || V < 0) return fail(INFV_ERR_INVALID, "encode_videos: bad arguments");
    if (V == 0) return INFV_OK;
    if (int rc = check_offsets("encode_videos", "cu", cu, V)) return rc;
    if (int rc = refuse_reduced(h, "encode_videos")) return rc;      // (the first read of the handle)
    const bool use_ltm = h->cfg.alpha != 1.0f;
    const int n_h = use_ltm ? V * h->cfg.n_layers : 0;
    if (use_ltm) {
        if (!ltm) return fail(INFV_ERR_INVALID, "encode_videos: alpha != 1 needs the per-layer LTM handles of every video");
        if (int rc = check_distinct_handles("encode_videos", ltm, n_h, "layer")) return rc;
    }
    if (cu[V] == 0) {                                         // no chunk: new_video still starts every memory afresh
        if (use_ltm && new_video)
            for (int i = 0; i < n_h; ++i) infv_ltm_reset(ltm[i]);
        return INFV_OK;
    }
    if (!frames) return fail(INFV_ERR_INVALID, "encode_videos: null frames");
    return encode_impl(h, ltm, frames, cu[V], T, w, u, new_video, hidden_out, llama_out, llama_mean, stream_, V, cu, true);
}

int infv_vqf_self_attention(infv_vqf_handle h, const float* qkv, int32_t nb, int32_t n_max, const int32_t* n_valid,
                            float* ctx, void* stream) {
    if (!h || !qkv || !ctx || nb < 0 || n_max < 1) return fail(INFV_ERR_INVALID, "self_attention: bad arguments");
    if (n_max > INFV_VQF_VC_MAX_TOKENS)
        return fail(INFV_ERR_UNSUPPORTED, "self_attention: %d tokens, at most %d are supported", n_max, INFV_VQF_VC_MAX_TOKENS);
    if (nb == 0) return INFV_OK;
    std::vector<int32_t> nv(nb, n_max);
    if (n_valid)
        for (int b = 0; b < nb; ++b) {
            if (n_valid[b] < 1 || n_valid[b] > n_max)
                return fail(INFV_ERR_INVALID, "self_attention: n_valid[%d] = %d outside 1..n_max = %d", b, n_valid[b], n_max);
            nv[b] = n_valid[b];
        }
    VcAttn a{};
    a.qkv0 = qkv; a.rows0 = n_max; a.nsplit = n_max; a.qkv1 = qkv; a.ctx0 = ctx; a.ctx1 = ctx; a.H = h->cfg.n_heads; a.n_alloc = n_max;
    HIP_TRY(launch_qf_vc_self_attention(a, nb, nv.data(), nullptr, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

// infv_vqf_encode_frames through vc_impl: F one-chunk "videos" without text rows or memories.  The token count of a frame is an
// argument (any value >= 1: the planes are padded to the next multiple of 64), every frame starts from the same query rows, and
// the last layer's rows go out in out_dtype.  The handle's tokens_per_frame, alpha and proj_out are not read.
struct FrameCall { int n_tokens; void* out; tok_code out_dtype; };

// One call of the VideoChat2 encoder.  The entry points fill the arguments by name; vc_validate adds what it decides from them, the
// token stages what they leave for the layers.  Stream v reads its own chunks [cu[v], cu[v+1]) of `frames` (fcu == nullptr:
// videos) or block frame_src[v] of the F blocks packed by fcu (streams).
struct VcCall {
    // ---- arguments
    const char* name = nullptr;                                // prefixes the refusals
    const infv_ltm_handle* ltm = nullptr;
    int32_t V = 0; const int32_t* cu = nullptr;
    const void* frames = nullptr;                              // (vc_front_tokens may replace frames and tok by an fp32 copy)
    bool tok_arg = false;                                      // token_dtype is an argument of the call: the handle's setting is not read
    int32_t token_dtype = INFV_TOKENS_F32;                     // (else fp32, refused unless the handle's setting is fp32 too)
    int32_t F = 0; const int32_t* fcu = nullptr; const int32_t* frame_src = nullptr;
    int32_t T = 0;
    const infv_vqf_vc_weights* w = nullptr;
    const float* hidden_in = nullptr;                          // (vc_input_rows replaces it by the embedding layer's rows)
    const int32_t* text_len = nullptr;
    const double* u = nullptr;
    int32_t new_video = 0;
    float* hidden_out = nullptr; float* proj_out = nullptr; float* proj_mean = nullptr;
    hipStream_t stream = nullptr;
    const infv_vqf_vc_front* front = nullptr;                  // infv_vqf_vc_encode_img: vision LayerNorm and / or embedding layer in front
    const FrameCall* fc = nullptr;                             // infv_vqf_encode_frames: every chunk is one frame of fc->n_tokens tokens
    // ---- decided by vc_validate
    tok_code tok = INFV_TOKENS_F32;
    bool streams = false;
    bool vis_ln = false, emb = false;                          // the vision LayerNorm runs inside the token pass; the embedding layer writes the input rows
    bool pad = false;                                          // frames: planes and score rows padded to the next multiple of 64
    bool attn16 = false;                                       // frames: the handle's attention precision is fp16 (attention_f16.hip)
    int n_live = 0, n_tokens = 0;                              // tokens a chunk holds in `frames`; keys it has in the contractions (pad keys: zeros, no mass)
    int n_cross = 0, n_h = 0; bool use_ltm = false;
    int C = 0, Cf = 0;                                         // chunks (0 after validation: the call is complete); distinct chunks of frame tokens
    long chunk_k = 0, src_k = 0;                               // elements of a chunk in the planes, and in `frames` (the same unless padded)
    int RB = 0, NB = 0;                                        // chunks per row block of the token GEMMs, per sub-batch of the short-term attention
    long M = 0;                                                // query rows of the call
    long Tt = 0, TB = 0, tb_max = 0;                           // (vc_tables) text rows: all, per block of the text FFN, of the largest row block
    // ---- left by vc_front_tokens and vc_token_pass
    TokLn ln_{}; const TokLn* ln = nullptr;                    // the vision LayerNorm on load (split path), else nullptr
    SplitRef wref{}; bool have_w = false, have_kbar = false;   // the planes of all Cf chunks, kept for the call; the frame means came with them
};

// The per-chunk host tables: its video's text length, the offset of its packed text rows, its rows in hidden_in / hidden_out
struct VcTables {
    std::vector<int32_t> n_valid, toff, q_dst, q_src, t_src, tl, o_q, o_t, q_n;
    std::vector<int32_t> src_chunk, kbar0;                     // streams: each stream-chunk's source chunk, each stream's first one
    std::vector<int32_t> off1;                                 // scratch of vc_self_block [RB]
    std::vector<infv_ltm_handle> hs_l;                         // scratch of vc_cross_block: one layer's memories [V]
};

// ---- what infv_vqf_encode_frames (through vc_validate) and infv_vqf_frame_cross_attention both decide about a frame call, written once
// The vision LayerNorm's arguments: what the struct and the token type alone decide ...
static int check_vision_ln_args(const char* name, bool vis_ln, const infv_vqf_vision_ln& vl, tok_code tok) {
    if (vis_ln && !vl.beta) return fail(INFV_ERR_INVALID, "%s: vision_ln.gamma without vision_ln.beta", name);
    // (the vision LayerNorm of fp8 tokens is not built: no vision encoder emits fp8)
    if (vis_ln && tok == INFV_TOKENS_F8E4M3) return fail(INFV_ERR_UNSUPPORTED, "%s: no vision LayerNorm of fp8 frame tokens", name);
    return INFV_OK;
}
// ... and what the handle's width decides
static int check_vision_ln_width(const char* name, bool vis_ln, const infv_vqf_config& c) {
    if (vis_ln && (c.enc_width % 64 || c.enc_width > kTokenLnMaxWidth))
        return fail(INFV_ERR_UNSUPPORTED, "%s: the vision LayerNorm needs enc_width = %d to be a multiple of 64, at most %d", name, c.enc_width,
                    kTokenLnMaxWidth);
    return INFV_OK;
}
// The token count of a frame: k.n_live, k.pad, k.n_tokens and k.attn16 from n_live and the handle's precisions
static int frame_token_shape(const infv_vqf_s* h, VcCall& k, int n_live) {
    const char* name = k.name;
    const infv_vqf_config& c = h->cfg;
    k.n_live = n_live;
    if (n_live < 1) return fail(INFV_ERR_INVALID, "%s: n_tokens = %d, must be >= 1", name, n_live);
    if (n_live > 0x7fffffff - 128) return fail(INFV_ERR_UNSUPPORTED, "%s: n_tokens = %d is too large", name, n_live);
    if (c.enc_width % 64) return fail(INFV_ERR_UNSUPPORTED, "%s: enc_width = %d is no multiple of 64", name, c.enc_width);
    k.attn16 = h->attn_mode != 0;
    k.pad = n_live % 64 != 0 && (k.attn16 || split_path(h, 64));                  // (the fp16 attention always reads padded planes)
    if (k.attn16 && (n_live + 63) / 64 * 64 > kAttnF16MaxPad)
        return fail(INFV_ERR_UNSUPPORTED, "%s: the fp16 attention (infv_vqf_set_attention_precision) takes at most %d tokens a frame, got %d",
                    name, kAttnF16MaxPad, n_live);
    if (n_live % 32 && !k.pad)
        return fail(INFV_ERR_UNSUPPORTED, "%s: the fp32 contractions (set_precision(h, 1) / INFV_VQF_FP32) need n_tokens %% 32 == 0, got %d", name, n_live);
    k.n_tokens = k.pad ? (n_live + 63) / 64 * 64 : n_live;
    return INFV_OK;
}
// The sizes the stages read, once the call has C chunks over Cf distinct ones of k.n_tokens (k.n_live in `frames`) tokens
static void vc_call_sizes(const infv_vqf_s* h, VcCall& k, int C, int Cf) {
    const infv_vqf_config& c = h->cfg;
    k.C = C;
    k.Cf = Cf;
    k.M = (long)C * c.n_query;
    k.chunk_k = (long)k.n_tokens * c.enc_width;
    k.src_k = (long)k.n_live * c.enc_width;
    k.RB = C < kRowBlockVideos ? C : kRowBlockVideos;
    k.NB = pick_short_nb(h, C, k.n_tokens);
}

// ---- validation before any device work or memory change.  Returns with k.C == 0 where nothing is left to do.
static int vc_validate(const infv_vqf_s* h, VcCall& k) {
    const char* name = k.name;
    const infv_vqf_vc_front* front = k.front; const FrameCall* fc = k.fc;
    const int32_t V = k.V, F = k.F; const int32_t *cu = k.cu, *fcu = k.fcu, *text_len = k.text_len;
    const infv_vqf_vc_weights* w = k.w;
    if (!h || !cu || !w || !text_len || V < 0) return fail(INFV_ERR_INVALID, "%s: bad arguments", name);
    if (front && front->reserved != 0) return fail(INFV_ERR_INVALID, "%s: front->reserved must be 0", name);
    k.vis_ln = front && front->vision_ln.gamma;
    k.emb = front && front->emb.word;
    if (k.emb && k.hidden_in) return fail(INFV_ERR_INVALID, "%s: the embedding layer and hidden_in are both given (one of them writes the input rows)", name);
    if (k.tok_arg && !token_dtype_known(k.token_dtype)) return fail(INFV_ERR_INVALID, "%s: unknown token dtype %d", name, k.token_dtype);
    k.tok = k.tok_arg ? static_cast<tok_code>(k.token_dtype) : INFV_TOKENS_F32;
    if (k.vis_ln)
        if (int rc = check_vision_ln_args(name, true, front->vision_ln, k.tok)) return rc;
    if (k.tok != INFV_TOKENS_F32 && k.frames && !aligned16(k.frames)) return fail(INFV_ERR_INVALID, "%s: fp16 / bf16 / fp8 frames must be 16-byte aligned", name);
    if (k.vis_ln && k.frames && !aligned16(k.frames)) return fail(INFV_ERR_INVALID, "%s: frames must be 16-byte aligned for the vision LayerNorm", name);
    if (V == 0) return INFV_OK;
    const infv_vqf_config& c = h->cfg;
    if (int rc = check_offsets(name, "cu", cu, V)) return rc;
    k.streams = fcu != nullptr;
    if (k.streams) {
        if (!k.frame_src || F < 1) return fail(INFV_ERR_INVALID, "%s: bad arguments", name);
        if (int rc = check_offsets(name, "fcu", fcu, F)) return rc;
        for (int v = 0; v < V; ++v) {
            const int s = k.frame_src[v];
            if (s < 0 || s >= F) return fail(INFV_ERR_INVALID, "%s: frame_src[%d] = %d outside [0, %d)", name, v, s, F);
            if (cu[v + 1] - cu[v] != fcu[s + 1] - fcu[s])
                return fail(INFV_ERR_INVALID, "%s: stream %d has %d chunks, its block %d has %d", name, v, cu[v + 1] - cu[v], s,
                            fcu[s + 1] - fcu[s]);
        }
    }
    if (w->n_layers < 1 || !w->layers) return fail(INFV_ERR_INVALID, "%s: no layers", name);
    if (w->n_layers > INFV_VQF_VC_MAX_LAYERS)
        return fail(INFV_ERR_UNSUPPORTED, "%s: %d layers, at most %d are supported", name, w->n_layers, INFV_VQF_VC_MAX_LAYERS);
    if (!fc)                                                   // (the first read of the handle: what the arguments alone decide comes first)
        if (int rc = refuse_reduced(h, name)) return rc;
    const int Q = c.n_query, Ln = w->n_layers;
    for (int v = 0; v < V; ++v) {
        if (text_len[v] < 0) return fail(INFV_ERR_INVALID, "%s: text_len[%d] = %d is negative", name, v, text_len[v]);
        if (Q + text_len[v] > INFV_VQF_VC_MAX_TOKENS)
            return fail(INFV_ERR_UNSUPPORTED, "%s: video %d attends over %d + %d tokens, at most %d are supported", name,
                        v, Q, text_len[v], INFV_VQF_VC_MAX_TOKENS);
    }
    if (k.emb)
        if (int rc = check_front_emb(name, front, V, text_len)) return rc;
    if (k.T < 1) return fail(INFV_ERR_INVALID, "%s: T must be >= 1", name);
    if (fc) {
        if (int rc = frame_token_shape(h, k, fc->n_tokens)) return rc;
    } else {
        k.n_live = k.n_tokens = k.T * c.tokens_per_frame;
        if (k.n_live % 32) return fail(INFV_ERR_UNSUPPORTED, "%s: T * tokens_per_frame = %d is no multiple of 32", name, k.n_live);
    }
    if (int rc = check_vision_ln_width(name, k.vis_ln, c)) return rc;
    if (!k.tok_arg && h->tok != INFV_TOKENS_F32)
        return fail(INFV_ERR_UNSUPPORTED, "%s: fp16 / bf16 frame tokens are not supported on this path (the _tok entry point takes them)", name);
    for (int l = 0; l < Ln; ++l) k.n_cross += w->layers[l].has_cross != 0;
    k.use_ltm = !fc && c.alpha != 1.0f && k.n_cross > 0;       // (frames: position_embedding_ext == None, no memory is called)
    k.n_h = k.use_ltm ? V * k.n_cross : 0;
    if (k.use_ltm) {
        if (!k.ltm) return fail(INFV_ERR_INVALID, "%s: alpha != 1 needs the LTM handles of every video and cross layer", name);
        if (int rc = check_distinct_handles(name, k.ltm, k.n_h, "cross layer")) return rc;
    }
    if ((k.proj_out || k.proj_mean) && (c.proj_out <= 0 || !w->mistral_proj.w))
        return fail(INFV_ERR_INVALID, "%s: projected output without mistral_proj", name);
    if (fc && fc->out_dtype != INFV_TOKENS_F32) {             // the last layer's epilogue writes the 2-byte rows: its 16-byte form only
        const infv_vqf_vc_layer& L = w->layers[Ln - 1];
        if (!aligned16(L.q_ffn_out.b) || !aligned16(L.q_ffn_ln.gamma) || !aligned16(L.q_ffn_ln.beta) || !L.q_ffn_ln.gamma || !L.q_ffn_ln.beta)
            return fail(INFV_ERR_INVALID, "%s: bf16 / fp16 output needs the last layer's q_ffn_out.b and q_ffn_ln 16-byte aligned", name);
    }
    if (fc && h->tap_dst && (h->tap_layer >= Ln || !w->layers[h->tap_layer].has_cross))
        return fail(INFV_ERR_INVALID, "%s: the context tap names layer %d, which is no cross-attention layer of these weights", name, h->tap_layer);
    if (cu[V] == 0) {                                         // no chunk: new_video still starts every memory afresh
        if (k.use_ltm && k.new_video)
            for (int i = 0; i < k.n_h; ++i) infv_ltm_reset(k.ltm[i]);
        return INFV_OK;
    }
    if (!k.frames || (!k.hidden_in && !k.emb)) return fail(INFV_ERR_INVALID, "%s: null frames or hidden_in", name);
    vc_call_sizes(h, k, cu[V], k.streams ? fcu[F] : cu[V]);
    return INFV_OK;
}

static void vc_tables(const infv_vqf_s* h, VcCall& k, VcTables& t) {
    const int Q = h->cfg.n_query, C = k.C, V = k.V;
    const int32_t* cu = k.cu;
    t.n_valid.resize(C); t.toff.assign(C + 1, 0); t.q_dst.resize(C); t.q_src.resize(C); t.t_src.resize(C); t.tl.resize(C);
    t.o_q.resize(C); t.o_t.resize(C); t.q_n.assign(C, Q);
    int32_t in_row = 0;
    for (int v = 0; v < V; ++v) {
        for (int cc = cu[v]; cc < cu[v + 1]; ++cc) {
            t.tl[cc] = k.text_len[v]; t.n_valid[cc] = Q + k.text_len[v]; t.toff[cc + 1] = t.toff[cc] + k.text_len[v];
            t.q_dst[cc] = cc * Q; t.q_src[cc] = k.fc ? 0 : in_row; t.t_src[cc] = in_row + Q;   // (frames: one block of query rows for all)
            t.o_q[cc] = cc * Q + t.toff[cc]; t.o_t[cc] = t.o_q[cc] + Q;
        }
        in_row += Q + k.text_len[v];
    }
    if (k.streams) {
        t.src_chunk.resize(C); t.kbar0.resize(V);
        for (int v = 0; v < V; ++v) {
            t.kbar0[v] = k.fcu[k.frame_src[v]];
            for (int i = 0; i < cu[v + 1] - cu[v]; ++i) t.src_chunk[cu[v] + i] = t.kbar0[v] + i;
        }
    }
    const long Tt = k.Tt = t.toff[C];
    k.TB = Tt < kTextFfnRows ? Tt : kTextFfnRows;
    for (RowBlock b : RowBlocks{C, k.RB, 0}) k.tb_max = std::max<long>(k.tb_max, t.toff[b.c0 + b.nb] - t.toff[b.c0]);
    t.off1.resize(k.RB);
    t.hs_l.resize(k.use_ltm ? V : 0);
}

// The vision LayerNorm's statistics, and -- where the fp32 contractions run -- the fp32 copy of the distinct chunks they read
static int vc_front_tokens(infv_vqf_s* h, VcCall& k) {
    const infv_vqf_config& c = h->cfg;
    if (k.vis_ln && k.n_cross > 0) {
        // (mean, 1 / sqrt(var + eps)) of every DISTINCT token row, once per call: 8 bytes per token
        const infv_vqf_vision_ln& vl = k.front->vision_ln;
        const size_t rows = (size_t)k.Cf * k.n_live;
        HIP_TRY(reserve_all({{h->lnstats, rows * 2 * sizeof(float)}}));
        HIP_TRY(launch_token_ln_stats(k.frames, k.tok, (long)rows, c.enc_width, vl.eps, h->lnstats.p, k.stream));
        if (k.attn16 || split_path(h, k.n_tokens)) {
            k.ln_ = TokLn{h->lnstats.as<float>(), vl.gamma, vl.beta};
            k.ln = &k.ln_;
        } else {                                               // the fp32 contractions from the normalised fp32 copy
            HIP_TRY(reserve_all({{h->up, rows * c.enc_width * sizeof(float)}}));
            HIP_TRY(launch_ln_tokens(k.frames, k.tok, (long)rows, c.enc_width, h->lnstats.p, vl.gamma, vl.beta, h->up.as<float>(), k.stream));
            k.frames = h->up.p; k.tok = INFV_TOKENS_F32;
        }
    }
    if (k.n_cross == 0 || k.attn16) return INFV_OK;           // (the fp16 token pass reads every token type in place)
    return fp32_tokens_unless_split(h, k.frames, k.tok, k.n_tokens, (size_t)k.Cf * k.chunk_k, k.stream);
}

static int vc_workspaces(infv_vqf_s* h, const VcCall& k) {
    const infv_vqf_config& c = h->cfg;
    const size_t f = sizeof(float), Hd = c.hidden, rb = (size_t)k.RB * c.n_query;
    const size_t act = (size_t)k.M * Hd * f, tact = (size_t)k.Tt * Hd * f;
    HIP_TRY(reserve_all({{h->smap, k.streams ? (size_t)k.C * sizeof(int32_t) : 0},
                         {h->vA, act}, {h->v1, act}, {h->v2, act}, {h->vxq, act}, {h->vshort, act}, {h->vmerged, act},
                         {h->valong, k.use_ltm ? act : 0}, {h->vu, k.use_ltm ? (size_t)k.C * c.nb_samples * sizeof(double) : 0},
                         {h->vkbar, k.use_ltm ? (size_t)k.Cf * k.T * c.enc_width * f : 0},
                         {h->vqkv, rb * 3 * Hd * f}, {h->vsa, rb * Hd * f}, {h->vinter, rb * c.inter * f},
                         {h->tA, tact}, {h->t1, tact}, {h->tqkv, (size_t)k.tb_max * 3 * Hd * f}, {h->tsa, (size_t)k.tb_max * Hd * f},
                         {h->tinter, (size_t)k.TB * c.inter * f}}));
    return INFV_OK;
}

// Every chunk starts from its video's encoder input rows: the embedding layer's (Qformer.py:54-111) or hidden_in
static int vc_input_rows(infv_vqf_s* h, VcCall& k, const VcTables& t) {
    const int Q = h->cfg.n_query, Hd = h->cfg.hidden;
    if (k.emb) {
        long n_in = 0;
        for (int v = 0; v < k.V; ++v) n_in += Q + k.text_len[v];
        HIP_TRY(reserve_all({{h->embrows, (size_t)n_in * Hd * sizeof(float)}}));
        if (int rc = run_embed(h, k.front, k.V, k.text_len, h->embrows.as<float>(), k.stream)) return rc;
        k.hidden_in = h->embrows.as<float>();
    }
    HIP_TRY(launch_qf_copy_rows(k.hidden_in, h->vA.as<float>(), t.q_dst.data(), t.q_src.data(), t.q_n.data(), k.C, Hd, k.stream));
    if (k.Tt > 0) HIP_TRY(launch_qf_copy_rows(k.hidden_in, h->tA.as<float>(), t.toff.data(), t.t_src.data(), t.tl.data(), k.C, Hd, k.stream));
    return INFV_OK;
}

// ONE pass over the frame tokens: split-bf16 operands of every cross layer's short-term attention (kept for the call when they fit
// INFV_VQF_SPLIT_CACHE_GB) and the frame means every cross layer's memories step from; then the stream map.
static int vc_token_pass(infv_vqf_s* h, VcCall& k, const VcTables& t) {
    if (k.n_cross == 0) return INFV_OK;
    const infv_vqf_config& c = h->cfg;
    if (k.attn16) {                                            // the fp16 plane and its transposed copy, once per call, for all cross layers
        const size_t sz = (size_t)k.Cf * k.chunk_k * 2;
        HIP_TRY(reserve_all({{h->aX, sz}, {h->aXT, sz}}));
        for (int c0 = 0; c0 < k.Cf; c0 += 32768) {             // grid.z limit
            const int n = k.Cf - c0 < 32768 ? k.Cf - c0 : 32768;
            const size_t o = (size_t)c0 * k.chunk_k * 2;
            HIP_TRY(launch_token_pass_f16(tok_at(k.frames, k.tok, (long)c0 * k.src_k), k.tok, n, k.n_live, k.n_tokens, c.enc_width,
                                          k.ln ? k.ln->stats + 2 * (size_t)c0 * k.n_live : nullptr, k.ln ? k.ln->gamma : nullptr,
                                          k.ln ? k.ln->beta : nullptr, h->aX.as<char>() + o, h->aXT.as<char>() + o, k.stream));
        }
        return INFV_OK;
    }
    float* kbar = h->vkbar.as<float>();
    // (streams: the distinct chunks only; bf16 tokens: only the transposed plane is written, as in infv_vqf_encode_video)
    const double need_gb = plane_bytes(k.tok, k.ln != nullptr, k.pad) * (double)k.Cf * (double)k.chunk_k / 1e9;
    if (h->fuse && split_path(h, k.n_tokens) && need_gb <= h->split_cache_gb) {
        k.have_kbar = k.use_ltm && token_pass_gives_means(c.tokens_per_frame);   // (where a frame divides the 64-token tile)
        if (int rc = prepare_split(h, k.frames, k.tok, k.Cf, k.n_tokens, k.have_kbar ? kbar : nullptr, true, &k.wref, k.stream, 0, 0, k.ln,
                                   k.pad ? k.n_live : 0)) return rc;
        k.have_w = true;
    }
    if (k.use_ltm && !k.have_kbar && k.ln) {                   // pooling with the LayerNorm on load: the means of the normalised tokens
        HIP_TRY(launch_pool_ln(k.frames, k.tok, k.ln->stats, k.ln->gamma, k.ln->beta, kbar, (int64_t)k.Cf * k.T, c.tokens_per_frame, c.enc_width,
                               k.stream));
    } else if (k.use_ltm && !k.have_kbar) {
        if (int rc = infv_ltm_set_token_dtype(k.ltm[0], k.tok)) return rc;
        const int rc_pool = infv_ltm_pool(k.ltm[0], k.frames, (int64_t)k.Cf * k.T, kbar, k.stream);
        if (int rc = infv_ltm_set_token_dtype(k.ltm[0], INFV_TOKENS_F32)) return rc;   // (left on fp32, as before)
        if (rc_pool) return rc_pool;
    }
    // the chunk map reaches the device in kernel arguments, once per call: no host buffer outlives the call, nothing waits on the host
    if (k.streams) HIP_TRY(launch_qf_write_map(h->smap.as<int32_t>(), t.src_chunk.data(), k.C, k.stream));
    return INFV_OK;
}

// The frame operand of the short-term attention of stream-chunks [c0, c0 + nb): `frames` (fp32 path) or the planes `pre`, and the
// map the contractions read them through (nullptr: chunk b of the sub-batch is entry b).
//   videos:  the cached planes at c0, else the caller's tokens at c0 (split per sub-batch inside short_attention)
//   streams: the cached planes of the DISTINCT chunks, or the caller's tokens on the fp32 path, read through the map; where the
//            planes do not fit, each contiguous run of source chunks is split into the sub-batch's own planes (identity map)
struct VcOperand {
    int rc = INFV_OK;
    SplitRef pre{}; bool has_pre = false;
    const void* frames = nullptr;
    const int32_t* map = nullptr;
    bool t_identity = false;   // the transposed plane holds the sub-batch in order: only the untransposed operand goes through the map
};
static VcOperand vc_operand_at(infv_vqf_s* h, const VcCall& k, const VcTables& t, int c0, int nb) {
    VcOperand op;
    const TokLn* ln = k.ln;
    op.frames = tok_at(k.frames, k.tok, (long)c0 * k.src_k);
    if (!k.streams) {
        if (k.have_w) {
            op.pre = split_ref_at(k.wref, c0, k.chunk_k); op.has_pre = true;
        } else if (ln || k.pad) {                              // the split per sub-batch short_attention would issue, with the LayerNorm on load / padded
            TokLn lc{};
            if (ln) lc = TokLn{ln->stats + 2 * (size_t)c0 * k.n_live, ln->gamma, ln->beta};
            op.rc = prepare_split(h, op.frames, k.tok, nb, k.n_tokens, nullptr, false, &op.pre, k.stream, 0, 0, ln ? &lc : nullptr, k.pad ? k.n_live : 0);
            op.has_pre = true;
        }
        return op;
    }
    op.map = h->smap.as<int32_t>() + c0;
    if (k.have_w) { op.pre = k.wref; op.has_pre = true; return op; }
    if (!split_path(h, k.n_tokens)) { op.frames = k.frames; return op; }
    op.map = nullptr;
    const int32_t* src = t.src_chunk.data() + c0;
    for (int b0 = 0; b0 < nb && op.rc == INFV_OK;) {
        int b1 = b0 + 1;
        while (b1 < nb && src[b1] == src[b1 - 1] + 1) ++b1;
        TokLn lc{};
        if (ln) lc = TokLn{ln->stats + 2 * (size_t)src[b0] * k.n_tokens, ln->gamma, ln->beta};
        op.rc = prepare_split(h, tok_at(k.frames, k.tok, (long)src[b0] * k.chunk_k), k.tok, b1 - b0, k.n_tokens, nullptr, false, &op.pre, k.stream,
                              b0, nb, ln ? &lc : nullptr);
        b0 = b1;
    }
    if (k.tok == INFV_TOKENS_BF16 && !ln) {                   // the untransposed operand is the caller's buffer: read through the map,
        op.pre.Fh = static_cast<const __bf16*>(k.frames);      // while the transposed plane just written holds the sub-batch in order
        op.map = h->smap.as<int32_t>() + c0; op.t_identity = true;
    }
    op.has_pre = true;
    return op;
}

// Layer l: self-attention over query + text tokens, output dense + LayerNorm, cross query (row blocks of chunks)
static int vc_self_block(infv_vqf_s* h, const VcCall& k, VcTables& t, int l) {
    const infv_vqf_config& c = h->cfg;
    const infv_vqf_vc_layer& L = k.w->layers[l];
    const int Q = c.n_query, Hd = c.hidden;
    const bool text_out = k.Tt > 0 && (l < k.w->n_layers - 1 || k.hidden_out);   // the last layer's text rows feed nothing but hidden_out
    float* vA = h->vA.as<float>(); float* v1 = h->v1.as<float>(); float* tA = h->tA.as<float>(); float* t1 = h->t1.as<float>();
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)Q * Hd}) {
        const int nb = b.nb;
        const long r0 = b.r0, t0 = t.toff[b.c0], tn = t.toff[b.c0 + nb] - t0;
        LinearCall qkv{vA + r0, nb * Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
        qkv.inv = true; qkv.reduced = k.fc != nullptr; qkv.y = h->vqkv.as<float>();
        if (int rc = run_linear(h, qkv, k.stream)) return rc;
        if (tn > 0) {
            LinearCall qkt{tA + t0 * Hd, (int)tn, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
            qkt.inv = true; qkt.y = h->tqkv.as<float>();
            if (int rc = run_linear(h, qkt, k.stream)) return rc;
        }
        for (int i = 0; i < nb; ++i) t.off1[i] = t.toff[b.c0 + i] - (int32_t)t0;
        VcAttn a{};
        a.qkv0 = h->vqkv.as<float>(); a.rows0 = Q; a.nsplit = Q; a.qkv1 = h->tqkv.as<float>();
        a.ctx0 = h->vsa.as<float>(); a.ctx1 = h->tsa.as<float>(); a.H = c.n_heads; a.n_alloc = 0;
        HIP_TRY(launch_qf_vc_self_attention(a, nb, t.n_valid.data() + b.c0, t.off1.data(), k.stream));
        LinearCall so{h->vsa.as<float>(), nb * Q, Hd, {&L.self_o}, 1, Hd};
        so.inv = true; so.reduced = k.fc != nullptr; so.residual = vA + r0; so.res_rows = nb * Q; so.ln = &L.self_ln; so.y = v1 + r0;
        if (int rc = run_linear(h, so, k.stream)) return rc;
        if (tn > 0 && text_out) {
            LinearCall st{h->tsa.as<float>(), (int)tn, Hd, {&L.self_o}, 1, Hd};
            st.inv = true; st.residual = tA + t0 * Hd; st.res_rows = (int)tn; st.ln = &L.self_ln; st.y = t1 + t0 * Hd;
            if (int rc = run_linear(h, st, k.stream)) return rc;
        }
        if (L.has_cross) {
            LinearCall xq{v1 + r0, nb * Q, Hd, {&L.x_q}, 1, Hd};
            xq.inv = true; xq.reduced = k.fc != nullptr; xq.y = h->vxq.as<float>() + r0;
            if (int rc = run_linear(h, xq, k.stream)) return rc;
        }
    }
    return INFV_OK;
}

// The short-term attention of every chunk of the call, in sub-batches, from the operands vc_token_pass left:
// xq [C * Q][hidden] -> out [C * Q][hidden].  Frames under the fp16 attention precision take attention_f16.hip's three launches.
static int vc_short_attention(infv_vqf_s* h, const VcCall& k, const VcTables& t, const float* xq, const infv_linear* key,
                              const infv_linear* value, float* out) {
    const infv_vqf_config& c = h->cfg;
    const int Q = c.n_query, Hd = c.hidden;
    if (k.attn16) {
        const AttnPlanes* p = nullptr;
        if (int rc = attn_planes(h, key, value, &p, k.stream)) return rc;
        const int NB = k.C < kAttnF16Frames ? k.C : kAttnF16Frames;
        const size_t sz = (size_t)NB * c.n_heads * Q * c.enc_width * 2;
        HIP_TRY(reserve_all({{h->aQt, sz}, {h->aO, sz}}));
        for (RowBlock b : RowBlocks{k.C, NB, (long)Q * Hd}) {
            AttnF16 a{};
            a.xq = xq + b.r0; a.wkT = p->kT.p; a.wv16 = p->v16.p; a.bv = value->b;
            a.X = h->aX.as<char>() + (size_t)b.c0 * k.chunk_k * 2; a.XT = h->aXT.as<char>() + (size_t)b.c0 * k.chunk_k * 2;
            a.qt = h->aQt.p; a.o = h->aO.p; a.ctx = out + b.r0;
            a.nb = b.nb; a.Q = Q; a.H = c.n_heads; a.d = c.enc_width; a.n = k.n_live; a.n_pad = k.n_tokens;
            HIP_TRY(launch_attn_f16(a, k.stream));
        }
        return INFV_OK;
    }
    for (RowBlock b : RowBlocks{k.C, k.NB, (long)Q * Hd}) {
        const VcOperand op = vc_operand_at(h, k, t, b.c0, b.nb);
        if (op.rc) return op.rc;
        if (int rc = short_attention(h, op.frames, k.tok, b.nb, k.n_tokens, xq + b.r0, false, key, value, nullptr, out + b.r0, k.stream, false,
                                     op.has_pre ? &op.pre : nullptr, nullptr, kInvariantNb, op.map, op.t_identity, k.pad ? k.n_live : 0)) return rc;
    }
    return INFV_OK;
}

// Cross layer l, the j-th of them: its V memories with per-chunk queries on the worker stream, beside the short-term attention;
// the merge of the two; the context tap; the cross output
static int vc_cross_block(infv_vqf_s* h, const VcCall& k, VcTables& t, int l, int j) {
    const infv_vqf_config& c = h->cfg;
    const infv_vqf_vc_layer& L = k.w->layers[l];
    const int Q = c.n_query, Hd = c.hidden;
    float* vxq = h->vxq.as<float>(); float* vmerged = h->vmerged.as<float>();
    if (k.use_ltm) {
        infv_ltm_proj pr{};
        pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
        if (int rc = ltm_u_slice(h, k.u, j, k.n_cross, k.C, k.stream)) return rc;
        HIP_TRY(hipEventRecord(h->ev_main, k.stream));
        HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
        for (int v = 0; v < k.V; ++v) t.hs_l[v] = k.ltm[(size_t)v * k.n_cross + j];
        if (int rc = infv_ltm_steps_videos_from(t.hs_l.data(), k.V, k.cu, h->vkbar.as<float>(), k.streams ? t.kbar0.data() : nullptr, k.T, vxq, 1,
                                                Q, &pr, k.u ? h->vu.as<double>() : nullptr, k.new_video, h->valong.as<float>(), h->side)) return rc;
        HIP_TRY(hipEventRecord(h->ev_side, h->side));
    }
    if (int rc = vc_short_attention(h, k, t, vxq, &L.x_k, &L.x_v, k.use_ltm ? h->vshort.as<float>() : vmerged)) return rc;
    if (k.use_ltm) {
        HIP_TRY(hipStreamWaitEvent(k.stream, h->ev_side, 0));
        if (int rc = alpha_merge(h, k.M, k.stream)) return rc;
    }
    if (k.fc && h->tap_dst && l == h->tap_layer)               // (tests: this layer's cross-attention context, Qformer.py:303-304)
        HIP_TRY(hipMemcpyAsync(h->tap_dst, vmerged, (size_t)k.M * Hd * sizeof(float), hipMemcpyDeviceToDevice, k.stream));
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)Q * Hd}) {
        LinearCall xo{vmerged + b.r0, b.nb * Q, Hd, {&L.x_o}, 1, Hd};
        xo.inv = true; xo.reduced = k.fc != nullptr; xo.residual = h->v1.as<float>() + b.r0; xo.res_rows = b.nb * Q; xo.ln = &L.x_ln; xo.y = h->v2.as<float>() + b.r0;
        if (int rc = run_linear(h, xo, k.stream)) return rc;
    }
    return INFV_OK;
}

// Layer l: query FFN on the query rows, text FFN on the text rows (Qformer.py:483-496)
static int vc_ffn_block(infv_vqf_s* h, const VcCall& k, int l) {
    const infv_vqf_config& c = h->cfg;
    const infv_vqf_vc_layer& L = k.w->layers[l];
    const int Q = c.n_query, Hd = c.hidden;
    const bool last = l == k.w->n_layers - 1;
    const float* qin = L.has_cross ? h->v2.as<float>() : h->v1.as<float>();   // the query rows entering the query FFN
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)Q * Hd}) {
        LinearCall fi{qin + b.r0, b.nb * Q, Hd, {&L.q_ffn_in}, 1, c.inter};
        fi.inv = true; fi.reduced = k.fc != nullptr; fi.act = QF_ACT_GELU; fi.y = h->vinter.as<float>();
        if (int rc = run_linear(h, fi, k.stream)) return rc;
        LinearCall fo{h->vinter.as<float>(), b.nb * Q, c.inter, {&L.q_ffn_out}, 1, Hd};
        fo.inv = true; fo.reduced = k.fc != nullptr; fo.residual = qin + b.r0; fo.res_rows = b.nb * Q; fo.ln = &L.q_ffn_ln; fo.y = h->vA.as<float>() + b.r0;
        if (k.fc && last && k.fc->out_dtype != INFV_TOKENS_F32) {   // the frame tokens leave in the type their consumer reads: no fp32 row is written
            fo.y16 = static_cast<char*>(k.fc->out) + 2 * b.r0; fo.y16_dtype = k.fc->out_dtype;
        }
        if (int rc = run_linear(h, fo, k.stream)) return rc;
    }
    if (!(k.Tt > 0 && (!last || k.hidden_out))) return INFV_OK;   // the last layer's text rows feed nothing but hidden_out
    float* tA = h->tA.as<float>(); float* t1 = h->t1.as<float>();
    const long Tt = k.Tt, TB = k.TB;
    for (long m0 = 0; m0 < Tt; m0 += TB) {
        const int m = (int)(Tt - m0 < TB ? Tt - m0 : TB);
        LinearCall fi{t1 + m0 * Hd, m, Hd, {&L.t_ffn_in}, 1, c.inter};
        fi.inv = true; fi.act = QF_ACT_GELU; fi.y = h->tinter.as<float>();
        if (int rc = run_linear(h, fi, k.stream)) return rc;
        LinearCall fo{h->tinter.as<float>(), m, c.inter, {&L.t_ffn_out}, 1, Hd};
        fo.inv = true; fo.residual = t1 + m0 * Hd; fo.res_rows = m; fo.ln = &L.t_ffn_ln; fo.y = tA + m0 * Hd;
        if (int rc = run_linear(h, fo, k.stream)) return rc;
    }
    return INFV_OK;
}

static int vc_outputs(infv_vqf_s* h, const VcCall& k, const VcTables& t) {
    const int Hd = h->cfg.hidden;
    if (k.hidden_out) {
        HIP_TRY(launch_qf_copy_rows(h->vA.as<float>(), k.hidden_out, t.o_q.data(), t.q_dst.data(), t.q_n.data(), k.C, Hd, k.stream));
        if (k.Tt > 0) HIP_TRY(launch_qf_copy_rows(h->tA.as<float>(), k.hidden_out, t.o_t.data(), t.toff.data(), t.tl.data(), k.C, Hd, k.stream));
    }
    if (k.proj_out || k.proj_mean)
        return project_and_mean(h, RowBlocks{k.C, k.RB, (long)h->cfg.n_query * Hd}, &k.w->mistral_proj, true, k.proj_out, k.proj_mean, k.cu, k.V,
                                k.stream);
    return INFV_OK;
}

// The body of the six entry points below: the stages above, in call order
static int vc_impl(infv_vqf_handle h, VcCall& k) {
    if (int rc = vc_validate(h, k)) return rc;
    if (k.C == 0) return INFV_OK;                              // no video or no chunk
    if (k.use_ltm)
        if (int rc = ensure_streams(h)) return rc;
    VcTables t;
    vc_tables(h, k, t);
    if (int rc = vc_front_tokens(h, k)) return rc;
    if (int rc = vc_workspaces(h, k)) return rc;
    if (int rc = vc_input_rows(h, k, t)) return rc;
    if (int rc = vc_token_pass(h, k, t)) return rc;
    for (int l = 0, j_cross = 0; l < k.w->n_layers; ++l) {
        if (int rc = vc_self_block(h, k, t, l)) return rc;
        if (k.w->layers[l].has_cross)
            if (int rc = vc_cross_block(h, k, t, l, j_cross++)) return rc;
        if (int rc = vc_ffn_block(h, k, l)) return rc;
    }
    return vc_outputs(h, k, t);
}

int infv_vqf_vc_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                              int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len,
                              const double* u, int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean,
                              void* stream_) {
    VcCall k;
    k.name = "vc_encode_videos"; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.T = T; k.w = w; k.hidden_in = hidden_in;
    k.text_len = text_len; k.u = u; k.new_video = new_video; k.hidden_out = hidden_out; k.proj_out = proj_out; k.proj_mean = proj_mean;
    k.stream = static_cast<hipStream_t>(stream_);
    return vc_impl(h, k);
}

int infv_vqf_vc_encode_streams(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                               int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w,
                               const float* hidden_in, const int32_t* text_len, const double* u, int32_t new_video,
                               float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (!fcu || !frame_src) return fail(INFV_ERR_INVALID, "vc_encode_streams: bad arguments");
    VcCall k;
    k.name = "vc_encode_streams"; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.F = F; k.fcu = fcu; k.frame_src = frame_src; k.T = T;
    k.w = w; k.hidden_in = hidden_in; k.text_len = text_len; k.u = u; k.new_video = new_video; k.hidden_out = hidden_out;
    k.proj_out = proj_out; k.proj_mean = proj_mean; k.stream = static_cast<hipStream_t>(stream_);
    return vc_impl(h, k);
}

int infv_vqf_vc_encode_videos_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                  int32_t token_dtype, int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in,
                                  const int32_t* text_len, const double* u, int32_t new_video, float* hidden_out, float* proj_out,
                                  float* proj_mean, void* stream_) {
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_videos_tok: unknown token dtype %d", token_dtype);
    VcCall k;
    k.name = "vc_encode_videos_tok"; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.tok_arg = true; k.token_dtype = token_dtype; k.T = T;
    k.w = w; k.hidden_in = hidden_in; k.text_len = text_len; k.u = u; k.new_video = new_video; k.hidden_out = hidden_out;
    k.proj_out = proj_out; k.proj_mean = proj_mean; k.stream = static_cast<hipStream_t>(stream_);
    return vc_impl(h, k);
}

int infv_vqf_vc_encode_streams_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                   int32_t token_dtype, int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T,
                                   const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len, const double* u,
                                   int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (!fcu || !frame_src) return fail(INFV_ERR_INVALID, "vc_encode_streams_tok: bad arguments");
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_streams_tok: unknown token dtype %d", token_dtype);
    VcCall k;
    k.name = "vc_encode_streams_tok"; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.tok_arg = true; k.token_dtype = token_dtype;
    k.F = F; k.fcu = fcu; k.frame_src = frame_src; k.T = T; k.w = w; k.hidden_in = hidden_in; k.text_len = text_len; k.u = u;
    k.new_video = new_video; k.hidden_out = hidden_out; k.proj_out = proj_out; k.proj_mean = proj_mean;
    k.stream = static_cast<hipStream_t>(stream_);
    return vc_impl(h, k);
}

int infv_vqf_vc_encode_img(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames, int32_t token_dtype,
                           int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w,
                           const infv_vqf_vc_front* front, const float* hidden_in, const int32_t* text_len, const double* u, int32_t new_video,
                           float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_img: unknown token dtype %d", token_dtype);
    if (frame_src && !fcu) return fail(INFV_ERR_INVALID, "vc_encode_img: bad arguments");
    VcCall k;
    k.name = "vc_encode_img"; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.tok_arg = true; k.token_dtype = token_dtype;
    if (frame_src) { k.F = F; k.fcu = fcu; k.frame_src = frame_src; }   // NULL: videos (F and fcu are not read)
    k.T = T; k.w = w; k.front = front; k.hidden_in = hidden_in; k.text_len = text_len; k.u = u; k.new_video = new_video;
    k.hidden_out = hidden_out; k.proj_out = proj_out; k.proj_mean = proj_mean; k.stream = static_cast<hipStream_t>(stream_);
    return vc_impl(h, k);
}

int infv_vqf_encode_frames(infv_vqf_handle h, int32_t F, const void* vision, int32_t token_dtype, int32_t n_tokens,
                           const infv_vqf_vc_weights* w, const infv_vqf_vision_ln* ln, const float* query_rows, void* out, int32_t out_dtype,
                           void* stream_) {
    // ---- what vc_validate does not see; everything else is refused there, before any launch or memory change ----
    const char* name = "encode_frames";
    if (!h || !w || !query_rows) return fail(INFV_ERR_INVALID, "%s: null handle, weights or query_rows", name);
    if (F < 0) return fail(INFV_ERR_INVALID, "%s: F = %d is negative", name, F);
    if (!token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "%s: unknown token dtype %d", name, token_dtype);
    if (out_dtype == INFV_TOKENS_F8E4M3) return fail(INFV_ERR_UNSUPPORTED, "%s: no fp8 output (the library does not quantise)", name);
    if (out_dtype != INFV_TOKENS_F32 && out_dtype != INFV_TOKENS_BF16 && out_dtype != INFV_TOKENS_F16)
        return fail(INFV_ERR_INVALID, "%s: unknown output dtype %d", name, out_dtype);
    if (w->mistral_proj.w || w->mistral_proj.b) return fail(INFV_ERR_INVALID, "%s: the image Q-former has no projection (mistral_proj must be absent)", name);
    if (F > 0 && (!vision || !out)) return fail(INFV_ERR_INVALID, "%s: null vision or out", name);
    if (!aligned16(vision) || !aligned16(out)) return fail(INFV_ERR_INVALID, "%s: vision and out must be 16-byte aligned", name);
    if (!aligned16(query_rows)) return fail(INFV_ERR_INVALID, "%s: query_rows must be 16-byte aligned", name);
    if (n_tokens < 1) return fail(INFV_ERR_INVALID, "%s: n_tokens = %d, must be >= 1", name, n_tokens);
    if ((long)F * h->cfg.n_query > 0x3fffffffL) return fail(INFV_ERR_UNSUPPORTED, "%s: %d frames in one call", name, F);
    infv_vqf_vc_front front{};
    if (ln && ln->gamma) front.vision_ln = *ln;
    std::vector<int32_t> cu((size_t)F + 1), text_len((size_t)(F > 0 ? F : 1), 0);
    for (int f = 0; f <= F; ++f) cu[f] = f;
    const FrameCall fc{n_tokens, out, static_cast<tok_code>(out_dtype)};
    VcCall k;
    k.name = name; k.V = F; k.cu = cu.data(); k.frames = vision; k.tok_arg = true; k.token_dtype = token_dtype; k.T = 1; k.w = w;
    k.hidden_in = query_rows; k.text_len = text_len.data(); k.hidden_out = out_dtype == INFV_TOKENS_F32 ? static_cast<float*>(out) : nullptr;
    k.stream = static_cast<hipStream_t>(stream_); k.front = &front; k.fc = &fc;
    const int rc = vc_impl(h, k);
    h->tap_layer = -1; h->tap_dst = nullptr;                  // a tap serves one call
    return rc;
}

// One cross-attention of infv_vqf_encode_frames alone: the stages of vc_impl that a cross layer's attention consists of, over a call
// descriptor filled here (no weights, no query rows: xq is given)
int infv_vqf_frame_cross_attention(infv_vqf_handle h, int32_t F, const void* vision, int32_t token_dtype, int32_t n_tokens,
                                   const infv_vqf_vision_ln* ln, const float* xq, const infv_linear* key, const infv_linear* value,
                                   float* ctx, void* stream_) {
    // ---- every refusal before any launch or memory change ----
    const char* name = "frame_cross_attention";
    if (!h || !key || !value || !key->w || !value->w) return fail(INFV_ERR_INVALID, "%s: null handle, key or value", name);
    if (F < 0) return fail(INFV_ERR_INVALID, "%s: F = %d is negative", name, F);
    if (!token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "%s: unknown token dtype %d", name, token_dtype);
    if (F > 0 && (!vision || !xq || !ctx)) return fail(INFV_ERR_INVALID, "%s: null vision, xq or ctx", name);
    if (!aligned16(vision) || !aligned16(xq) || !aligned16(ctx) || !aligned16(key->w) || !aligned16(value->w))
        return fail(INFV_ERR_INVALID, "%s: vision, xq, ctx and the weights must be 16-byte aligned", name);
    const infv_vqf_config& c = h->cfg;
    if ((long)F * c.n_query > 0x3fffffffL) return fail(INFV_ERR_UNSUPPORTED, "%s: %d frames in one call", name, F);
    // ---- the frame checks of infv_vqf_encode_frames (vc_validate), through the helpers the two share ----
    infv_vqf_vc_front front{};
    if (ln && ln->gamma) front.vision_ln = *ln;
    VcCall k;
    k.name = name; k.V = F; k.frames = vision; k.tok_arg = true; k.token_dtype = token_dtype; k.T = 1; k.front = &front;
    k.stream = static_cast<hipStream_t>(stream_);
    k.tok = static_cast<tok_code>(token_dtype);
    k.vis_ln = front.vision_ln.gamma != nullptr;
    if (int rc = check_vision_ln_args(name, k.vis_ln, front.vision_ln, k.tok)) return rc;
    if (int rc = frame_token_shape(h, k, n_tokens)) return rc;
    if (int rc = check_vision_ln_width(name, k.vis_ln, c)) return rc;
    if (F == 0) return INFV_OK;
    k.n_cross = 1;
    vc_call_sizes(h, k, F, F);                                 // (no workspace of vc_workspaces is used: xq and ctx are the caller's)
    const FrameCall fc{n_tokens, nullptr, INFV_TOKENS_F32};
    k.fc = &fc;
    VcTables t;
    if (int rc = vc_front_tokens(h, k)) return rc;
    if (int rc = vc_token_pass(h, k, t)) return rc;
    return vc_short_attention(h, k, t, xq, key, value, ctx);
}

int infv_vqf_set_context_tap(infv_vqf_handle h, int32_t layer, float* dst) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    if (dst && (layer < 0 || layer >= INFV_VQF_VC_MAX_LAYERS)) return fail(INFV_ERR_INVALID, "set_context_tap: layer %d outside [0, %d)", layer, INFV_VQF_VC_MAX_LAYERS);
    h->tap_layer = dst ? layer : -1; h->tap_dst = dst;
    return INFV_OK;
}

int infv_vqf_layernorm_tokens(const void* frames, int32_t token_dtype, int64_t n_rows, int32_t d, const float* gamma, const float* beta,
                              float eps, float* out_f32, void* stream_) {
    // ---- every refusal before any launch ----
    if (!token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "layernorm_tokens: unknown token dtype %d", token_dtype);
    if (token_dtype == INFV_TOKENS_F8E4M3) return fail(INFV_ERR_UNSUPPORTED, "layernorm_tokens: no vision LayerNorm of fp8 frame tokens");
    if (!frames || !gamma || !beta || !out_f32 || n_rows < 0) return fail(INFV_ERR_INVALID, "layernorm_tokens: bad arguments");
    if (d < 64 || d % 64) return fail(INFV_ERR_INVALID, "layernorm_tokens: d must be a positive multiple of 64");
    if (d > kTokenLnMaxWidth) return fail(INFV_ERR_UNSUPPORTED, "layernorm_tokens: d = %d, at most %d is supported", d, kTokenLnMaxWidth);
    if (!aligned16(frames) || !aligned16(out_f32) || !aligned16(gamma) || !aligned16(beta))
        return fail(INFV_ERR_INVALID, "layernorm_tokens: frames, gamma, beta and out must be 16-byte aligned");
    if (n_rows == 0) return INFV_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the per-row statistics live in a process-wide buffer, grown on demand (the encoders keep theirs in the handle)
    // (a call on another stream waits for the event recorded behind the last reader before it overwrites them)
    static std::mutex mu;
    static DeviceBuf* stats = new DeviceBuf();
    static hipEvent_t last_read = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    HIP_TRY(reserve_all({{*stats, (size_t)n_rows * 2 * sizeof(float)}}));
    if (!last_read) HIP_TRY(hipEventCreateWithFlags(&last_read, hipEventDisableTiming));
    else HIP_TRY(hipStreamWaitEvent(stream, last_read, 0));
    const tok_code tok = static_cast<tok_code>(token_dtype);
    HIP_TRY(launch_token_ln_stats(frames, tok, (long)n_rows, d, eps, stats->p, stream));
    HIP_TRY(launch_ln_tokens(frames, tok, (long)n_rows, d, stats->p, gamma, beta, out_f32, stream));
    HIP_TRY(hipEventRecord(last_read, stream));
    return INFV_OK;
}

int infv_vqf_vc_embed(infv_vqf_handle h, const infv_vqf_vc_front* front, int32_t V, const int32_t* text_len, float* out_rows, void* stream_) {
    // ---- every refusal before any launch or memory change ----
    if (!h || !front || !text_len || V < 0) return fail(INFV_ERR_INVALID, "vc_embed: bad arguments");
    if (int rc = refuse_reduced(h, "vc_embed")) return rc;
    if (front->reserved != 0) return fail(INFV_ERR_INVALID, "vc_embed: front->reserved must be 0");
    if (!front->emb.word) return fail(INFV_ERR_INVALID, "vc_embed: no embedding tables (emb.word is NULL)");
    if (int rc = check_front_emb("vc_embed", front, V, text_len)) return rc;
    for (int v = 0; v < V; ++v)
        if (h->cfg.n_query + text_len[v] > INFV_VQF_VC_MAX_TOKENS)
            return fail(INFV_ERR_UNSUPPORTED, "vc_embed: video %d has %d + %d tokens, at most %d are supported", v, h->cfg.n_query, text_len[v],
                        INFV_VQF_VC_MAX_TOKENS);
    if (V == 0) return INFV_OK;
    if (!out_rows) return fail(INFV_ERR_INVALID, "vc_embed: null out_rows");
    return run_embed(h, front, V, text_len, out_rows, static_cast<hipStream_t>(stream_));
}

int infv_vqf_token_pass(const void* frames, int32_t token_dtype, int32_t nb, int32_t n_tokens, int32_t d, int32_t tokens_per_frame,
                        void* Fh, void* Fl, void* Th, void* Tl, float* kbar, void* stream) {
    // ---- every refusal before any launch ----
    if (!token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "token_pass: unknown token dtype %d", token_dtype);
    const tok_code tok = static_cast<tok_code>(token_dtype);
    if (!frames || !Th || nb < 0) return fail(INFV_ERR_INVALID, "token_pass: bad arguments");
    if (tok == INFV_TOKENS_BF16 ? (Fh || Fl || Tl) : tok == INFV_TOKENS_F8E4M3 ? (!Fh || Fl || Tl) : (!Fh || !Fl || !Tl))
        return fail(INFV_ERR_INVALID, "token_pass: bf16 tokens take Th alone (Fh, Fl, Tl NULL), fp8 tokens Fh and Th (Fl, Tl NULL), "
                                      "fp32 / fp16 tokens all four planes");
    if (n_tokens < 32 || n_tokens % 32) return fail(INFV_ERR_INVALID, "token_pass: n_tokens must be a positive multiple of 32");
    if (d < 64 || d % 64) return fail(INFV_ERR_INVALID, "token_pass: d must be a positive multiple of 64");
    if (!aligned16(frames) || !aligned16(Fh) || !aligned16(Fl) || !aligned16(Th) || !aligned16(Tl))
        return fail(INFV_ERR_INVALID, "token_pass: frames and planes must be 16-byte aligned");
    if (kbar && (tokens_per_frame < 1 || n_tokens % tokens_per_frame))
        return fail(INFV_ERR_INVALID, "token_pass: tokens_per_frame must divide n_tokens");
    if (kbar && !token_pass_gives_means(tokens_per_frame))
        return fail(INFV_ERR_UNSUPPORTED, "token_pass: no one-pass form with the frame means for tokens_per_frame = %d (it must divide 64)",
                    tokens_per_frame);
    const size_t chunk = (size_t)n_tokens * d;
    for (int c0 = 0; c0 < nb; c0 += 32768) {                   // grid.z limit
        const int n = nb - c0 < 32768 ? nb - c0 : 32768;
        const size_t o = (size_t)c0 * chunk;
        auto at = [&](void* p) -> void* { return p ? static_cast<__bf16*>(p) + o : nullptr; };
        HIP_TRY(launch_token_pass(tok_at(frames, tok, (long)o), tok, n, n_tokens, d, at(Fh), at(Fl), at(Th), at(Tl), static_cast<hipStream_t>(stream),
                                  kbar ? kbar + (size_t)c0 * (n_tokens / tokens_per_frame) * d : nullptr, tokens_per_frame));
    }
    return INFV_OK;
}

int infv_vqf_mean(const float* in, int32_t n, int64_t elems, float* out, void* stream) {
    if (!in || !out || n < 1 || elems < 1) return fail(INFV_ERR_INVALID, "bad argument");
    HIP_TRY(launch_qf_mean(in, n, elems, out, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

}  // extern "C"
