// C ABI of the video Q-former path (include/infv_vqf.h): workspace + launch sequence of one chunk.
#include "../../include/infv_vqf.h"
#include "capi_common.h"
#include <algorithm>
#include <mutex>
#include <vector>
#include "vqf_internal.h"

#include <cstdlib>
#include <new>

using namespace infv;

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

// y = epilogue( x [M][K] . W^T ) with up to 3 stacked weight matrices of n_out rows each
struct LinearCall {
    const float* x; int M, K;
    const infv_linear* lin[kQfMaxSeg]; int n_lin; int n_out;      // output width = n_lin * n_out
    int act = QF_ACT_NONE;
    const float* residual = nullptr; int res_rows = 1;
    const infv_layernorm* ln = nullptr;
    float* y;
    bool inv = false;      // batch invariant (infv_vqf_encode_videos): 128 x 128 tiles, no split-K, whatever M is
    void* y16 = nullptr; tok_code y16_dtype = INFV_TOKENS_F32;   // y16 != nullptr: the rows go out as bf16 / fp16 instead of y (infv_vqf_encode_frames)
};

int run_linear(infv_vqf_s* h, const LinearCall& c, hipStream_t stream) {
    const int width = c.n_lin * c.n_out;
    const int sk = c.inv ? 1 : qf_pick_splitk(c.M, width, c.K, 1);
    const size_t need = (size_t)sk * c.M * width * sizeof(float);
    if (need > h->part.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->part.reserve(need)); }
    QfGemm g{};
    g.A = c.x; g.lda = c.K; g.strideA = 0;
    for (int i = 0; i < c.n_lin; ++i) g.B[i] = c.lin[i]->w;
    g.ldb = c.K; g.strideB = 0; g.seg_rows = c.n_out;
    g.C = h->part.as<float>(); g.ldc = width; g.strideC = 0; g.split_stride = (long)c.M * width;
    g.M = c.M; g.N = width; g.k_per_split = c.K / sk; g.splitk = sk; g.nbatch = 1; g.tile = c.inv ? 128 : 0;
    HIP_TRY(launch_qf_gemm(g, false, stream));
    QfEpilogue e{};
    e.parts = h->part.as<float>(); e.nsplit = sk; e.split_stride = g.split_stride; e.ld_in = width;
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

// fp16 / bf16 / fp8 tokens where the split path does not apply: an fp32 copy in the handle's workspace for today's fp32 kernels
static int upcast_tokens(infv_vqf_s* h, const void* frames, tok_code tok, size_t elems, const float** out, hipStream_t stream) {
    if (elems * sizeof(float) > h->up.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->up.reserve(elems * sizeof(float))); }
    if (tok == INFV_TOKENS_F16) HIP_TRY(launch_upcast_f16(frames, h->up.as<float>(), (long)elems, stream));
    else if (tok == INFV_TOKENS_F8E4M3) HIP_TRY(launch_upcast_f8(frames, h->up.as<float>(), (long)elems, stream));
    else HIP_TRY(launch_upcast_bf16(frames, h->up.as<float>(), (long)elems, stream));
    *out = h->up.as<float>();
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
    const int d = h->cfg.enc_width;
    const size_t szF = (size_t)(cap > dst0 + nb ? cap : dst0 + nb) * n_tokens * d * 2;
    const size_t d0 = (size_t)dst0 * n_tokens * d;
    DeviceBuf& Fh = whole ? h->wFh : h->sFh; DeviceBuf& Fl = whole ? h->wFl : h->sFl;
    DeviceBuf& Th = whole ? h->wTh : h->sTh; DeviceBuf& Tl = whole ? h->wTl : h->sTl;
    if (n_live > 0 && n_live != n_tokens) {                  // padded planes: no frame means, bf16 tokens get their F_hi too
        if (kbar) return fail(INFV_ERR_INVALID, "prepare_split: no frame means from padded planes");
        const bool own_hi = !ln && (tok == INFV_TOKENS_BF16 || tok == INFV_TOKENS_F8E4M3);
        if (szF > Fh.bytes || szF > Th.bytes || (!own_hi && (szF > Fl.bytes || szF > Tl.bytes))) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(Fh.reserve(szF)); HIP_TRY(Th.reserve(szF));
            if (!own_hi) { HIP_TRY(Fl.reserve(szF)); HIP_TRY(Tl.reserve(szF)); }
        }
        for (int c0 = 0; c0 < nb; c0 += 32768) {               // grid.z limit
            const int n = nb - c0 < 32768 ? nb - c0 : 32768;
            const size_t o = (size_t)c0 * n_tokens * d, oi = (size_t)c0 * n_live * d;
            HIP_TRY(launch_token_pass_pad(tok_at(frames_, tok, (long)oi), tok, n, n_live, n_tokens, d, ln ? ln->stats + 2 * (size_t)c0 * n_live : nullptr,
                                          ln ? ln->gamma : nullptr, ln ? ln->beta : nullptr, Fh.as<__bf16>() + d0 + o,
                                          own_hi ? nullptr : Fl.as<__bf16>() + d0 + o, Th.as<__bf16>() + d0 + o,
                                          own_hi ? nullptr : Tl.as<__bf16>() + d0 + o, stream));
        }
        *ref = SplitRef{Fh.as<__bf16>(), own_hi ? nullptr : Fl.as<__bf16>(), Th.as<__bf16>(), own_hi ? nullptr : Tl.as<__bf16>()};
        return INFV_OK;
    }
    const int P = h->cfg.tokens_per_frame;
    if (tok == INFV_TOKENS_BF16 && !ln) {                    // read in place: only the transposed copy is written
        if (szF > Th.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(Th.reserve(szF)); }
        const __bf16* fb = static_cast<const __bf16*>(frames_);
        for (int c0 = 0; c0 < nb; c0 += 32768) {               // grid.z limit
            const int n = nb - c0 < 32768 ? nb - c0 : 32768;
            const size_t o = (size_t)c0 * n_tokens * d;
            HIP_TRY(launch_token_pass(fb + o, tok, n, n_tokens, d, nullptr, nullptr, Th.as<__bf16>() + d0 + o, nullptr, stream,
                                      kbar ? kbar + (size_t)c0 * (n_tokens / P) * d : nullptr, P));
        }
        *ref = SplitRef{fb, nullptr, Th.as<__bf16>(), nullptr};   // (Fh: THESE chunks, whatever dst0 is)
        return INFV_OK;
    }
    if (tok == INFV_TOKENS_F8E4M3 && !ln) {                  // the hi planes alone: an e4m3 value has no lo piece
        if (szF > Fh.bytes || szF > Th.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(Fh.reserve(szF)); HIP_TRY(Th.reserve(szF)); }
        for (int c0 = 0; c0 < nb; c0 += 32768) {               // grid.z limit
            const int n = nb - c0 < 32768 ? nb - c0 : 32768;
            const size_t o = (size_t)c0 * n_tokens * d;
            HIP_TRY(launch_token_pass(tok_at(frames_, tok, (long)o), tok, n, n_tokens, d, Fh.as<__bf16>() + d0 + o, nullptr,
                                      Th.as<__bf16>() + d0 + o, nullptr, stream, kbar ? kbar + (size_t)c0 * (n_tokens / P) * d : nullptr, P));
        }
        *ref = SplitRef{Fh.as<__bf16>(), nullptr, Th.as<__bf16>(), nullptr};
        return INFV_OK;
    }
    if (szF > Fh.bytes || szF > Fl.bytes || szF > Th.bytes || szF > Tl.bytes) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(Fh.reserve(szF)); HIP_TRY(Fl.reserve(szF)); HIP_TRY(Th.reserve(szF)); HIP_TRY(Tl.reserve(szF));
    }
    for (int c0 = 0; c0 < nb; c0 += 32768) {                   // grid.z limit
        const int n = nb - c0 < 32768 ? nb - c0 : 32768;
        const size_t o = (size_t)c0 * n_tokens * d;
        float* kb = kbar ? kbar + (size_t)c0 * (n_tokens / P) * d : nullptr;
        if (ln) {                                              // a normalised value is a general fp32 number: four planes for every token type
            HIP_TRY(launch_token_pass_ln(tok_at(frames_, tok, (long)o), tok, n, n_tokens, d, ln->stats + 2 * (size_t)c0 * n_tokens, ln->gamma, ln->beta,
                                         Fh.as<__bf16>() + d0 + o, Fl.as<__bf16>() + d0 + o, Th.as<__bf16>() + d0 + o, Tl.as<__bf16>() + d0 + o, stream, kb, P));
            continue;
        }
        HIP_TRY(launch_token_pass(tok_at(frames_, tok, (long)o), tok, n, n_tokens, d, Fh.as<__bf16>() + d0 + o, Fl.as<__bf16>() + d0 + o,
                                  Th.as<__bf16>() + d0 + o, Tl.as<__bf16>() + d0 + o, stream, kb, P));
    }
    *ref = SplitRef{Fh.as<__bf16>(), Fl.as<__bf16>(), Th.as<__bf16>(), Tl.as<__bf16>()};
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
    if (needS > h->S.bytes || needO > h->O.bytes || needQt > h->qt.bytes) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(h->S.reserve(needS)); HIP_TRY(h->O.reserve(needO)); HIP_TRY(h->qt.reserve(needQt));
    }
    float* qt = h->qt.as<float>();
    void* qh = h->sQh.p; void* ql = h->sQl.p;
    if (use_cache) {                                           // nq == 1: the cached query block of layer 0
        const size_t szq = (size_t)rows * d;
        if (szq * 4 > h->c_qt.bytes) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(h->c_qt.reserve(szq * 4)); HIP_TRY(h->c_qh.reserve(szq * 2)); HIP_TRY(h->c_ql.reserve(szq * 2));
            h->c_qt_valid = h->c_qsplit_valid = false;
        }
        qt = h->c_qt.as<float>(); qh = h->c_qh.p; ql = h->c_ql.p;
    }
    if (!use_cache || !h->c_qt_valid) {
        HIP_TRY(launch_qf_qtilde(xq, nq, Q, H, d, key->w, qt, stream));
        if (use_cache) { h->c_qt_valid = true; h->c_qsplit_valid = false; }
    }
    // Both big contractions ( [H*Q x d x n_tokens] each ) run as split-bf16 (three bf16 MFMA products, fp32 accumulate):
    // their rounding (~1e-5) only feeds the read-out.  INFV_VQF_FP32=1 selects the exact-fp32 MFMA kernels instead.
    if (split_path(h, n_tokens)) {
        const size_t szP = (size_t)nb * rows * n_tokens * 2, szQ = (size_t)nq * rows * d * 2;
        if (szP > h->sPh.bytes || szQ > h->sQh.bytes) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(h->sPh.reserve(szP)); HIP_TRY(h->sPl.reserve(szP)); HIP_TRY(h->sQh.reserve(szQ)); HIP_TRY(h->sQl.reserve(szQ));
        }
        SplitRef sr;
        if (pre) sr = *pre;                                   // the caller split these tokens already (shared by the layers)
        else if (int rc = prepare_split(h, frames_, tok, nb, n_tokens, nullptr, false, &sr, stream)) return rc;
        if (use_cache) {                                      // (the buffers may just have been (re)allocated above)
            qh = h->c_qh.p; ql = h->c_ql.p;
        } else {
            qh = h->sQh.p; ql = h->sQl.p;
        }
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
    if (needP > h->part.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->part.reserve(needP)); }
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
    if ((size_t)(2 * n) * sizeof(int32_t) > h->ids_dev.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->ids_dev.reserve((size_t)(2 * n) * sizeof(int32_t))); }
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

int infv_vqf_short_attention(infv_vqf_handle h, const void* frames, int32_t n_tokens, const float* xq,
                             const infv_linear* key, const infv_linear* value, const float* a_long,
                             float* merged, void* stream) {
    if (!h || !frames || !xq || !key || !value || !merged || !key->w || !value->w || !value->b)
        return fail(INFV_ERR_INVALID, "null argument");
    tok_code tok = h->tok;
    if (tok != INFV_TOKENS_F32 && !aligned16(frames)) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 frames must be 16-byte aligned");
    if (n_tokens < 32 || n_tokens % 32) return fail(INFV_ERR_INVALID, "n_tokens must be a positive multiple of 32");
    if (tok != INFV_TOKENS_F32 && !split_path(h, n_tokens)) {
        const float* f32 = nullptr;
        if (int rc = upcast_tokens(h, frames, tok, (size_t)n_tokens * h->cfg.enc_width, &f32, static_cast<hipStream_t>(stream))) return rc;
        frames = f32; tok = INFV_TOKENS_F32;
    }
    return short_attention(h, frames, tok, 1, n_tokens, xq, false, key, value, a_long, merged, static_cast<hipStream_t>(stream));
}

int infv_vqf_encode_chunk(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t T,
                          const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, void* stream_) {
    if (!h || !frames || !w) return fail(INFV_ERR_INVALID, "null argument");
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
    if (tok != INFV_TOKENS_F32 && !split_path(h, n_tokens)) {  // today's fp32 kernels from an fp32 copy
        const float* f32 = nullptr;
        if (int rc = upcast_tokens(h, frames, tok, (size_t)n_tokens * c.enc_width, &f32, stream)) return rc;
        frames = f32; tok = INFV_TOKENS_F32;
    }

    // The prefix of layer 0 (embedding LayerNorm -> self-attention block -> cross query) depends on the weights only,
    // not on the chunk: with a non-zero weights epoch it is computed once and reused until the epoch changes.
    const bool caching = h->epoch != 0;
    const bool prefix_cached = caching && h->c_valid && h->c_epoch == h->epoch;
    if (caching && !prefix_cached) {
        const size_t sz = (size_t)Q * Hd * sizeof(float);
        if (sz > h->c_h1.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->c_h1.reserve(sz)); HIP_TRY(h->c_xq.reserve(sz)); }
        h->c_valid = false; h->c_qt_valid = false; h->c_qsplit_valid = false;
    }
    if (!prefix_cached) {
        // embeddings: LayerNorm of the learned query tokens (Qformer.py:108-112)
        QfEpilogue e{};
        e.parts = w->query_tokens; e.nsplit = 1; e.split_stride = 0; e.ld_in = Hd; e.seg_cols = Hd;
        e.gamma = w->emb_ln.gamma; e.beta = w->emb_ln.beta; e.eps = c.ln_eps; e.scale = 1.f; e.res_scale = 1.f;
        e.out = h->h_a.as<float>(); e.ld_out = Hd; e.M = Q; e.width = Hd; e.res_rows = 1;
        HIP_TRY(launch_qf_epilogue(e, stream));
    }
    float* hcur = h->h_a.as<float>();
    float* hnext = h->h_b.as<float>();

    if (use_ltm) {
        const size_t need = (size_t)T * c.enc_width * sizeof(float);
        if (need > h->kbar.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->kbar.reserve(need)); }
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
            // ---- self-attention over the query tokens + output (Qformer.py:442-470 -> BertAttention)
            LinearCall qkv{hcur, Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
            qkv.y = h->qkv.as<float>();
            if (int rc = run_linear(h, qkv, stream)) return rc;
            HIP_TRY(launch_qf_self_attention(h->qkv.as<float>(), 1, Q, c.n_heads, h->sa.as<float>(), stream));
            LinearCall so{h->sa.as<float>(), Q, Hd, {&L.self_o}, 1, Hd};
            so.residual = hcur; so.res_rows = Q; so.ln = &L.self_ln; so.y = h1;
            if (int rc = run_linear(h, so, stream)) return rc;
            // ---- cross-attention: query, long-term memory, short-term attention, merge, output
            LinearCall xq{h1, Q, Hd, {&L.x_q}, 1, Hd};
            xq.y = xqb;
            if (int rc = run_linear(h, xq, stream)) return rc;
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
        static const int nb_env = [] { const char* e = exp_env("INFV_VQF_NB"); return e ? atoi(e) : 0; }();   // (sweeps)
        if (nb_env > 0) NB = nb_env < C ? nb_env : C;
    }
    return NB;
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
    if (tok != INFV_TOKENS_F32 && !split_path(h, n_tokens)) {  // today's fp32 kernels from an fp32 copy
        const float* f32 = nullptr;
        if (int rc = upcast_tokens(h, frames, tok, (size_t)C * chunk_k, &f32, stream)) return rc;
        frames = f32; tok = INFV_TOKENS_F32;
    }
    const long M = (long)C * Q;                               // rows of the whole-video activations
    // ---- workspaces: whole-video activations + per-block scratch ----
    const int rb_max = multi ? kRowBlockVideos : kRowBlockVideo;   // (batch invariant: the row count does not shape the GEMMs)
    const int RB = C < rb_max ? C : rb_max;                   // chunks per row block of the query-token GEMMs
    // chunks per sub-batch of the short-term attention: the second contraction has few, long tiles per chunk
    // (rows/128 x d/128 = 18 at the headline shape, K = T*P), so pick the count whose tile total fills whole rounds
    // of the 256 CUs (16 chunks = 288 tiles ran at 56 % of 14 chunks' rate per tile)
    const int NB = pick_short_nb(h, C, n_tokens);
    {
        const size_t act = (size_t)M * Hd * sizeof(float);
        bool grow = act > h->vA.bytes || (size_t)RB * Q * 3 * Hd * sizeof(float) > h->vqkv.bytes ||
                    (size_t)RB * Q * c.inter * sizeof(float) > h->vinter.bytes ||
                    (use_ltm && ((size_t)C * S * sizeof(double) > h->vu.bytes || (size_t)C * T * c.enc_width * sizeof(float) > h->vkbar.bytes));
        if (grow) HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(h->vA.reserve(act)); HIP_TRY(h->v1.reserve(act)); HIP_TRY(h->v2.reserve(act)); HIP_TRY(h->vxq.reserve(act));
        HIP_TRY(h->vshort.reserve(act)); HIP_TRY(h->vmerged.reserve(act));
        if (use_ltm) {
            HIP_TRY(h->valong.reserve(act));
            HIP_TRY(h->vu.reserve((size_t)C * S * sizeof(double)));
            HIP_TRY(h->vkbar.reserve((size_t)C * T * c.enc_width * sizeof(float)));
        }
        HIP_TRY(h->vqkv.reserve((size_t)RB * Q * 3 * Hd * sizeof(float)));
        HIP_TRY(h->vsa.reserve((size_t)RB * Q * Hd * sizeof(float)));
        HIP_TRY(h->vinter.reserve((size_t)RB * Q * c.inter * sizeof(float)));
        HIP_TRY(h->v_h1s.reserve((size_t)Q * Hd * sizeof(float)));
        HIP_TRY(h->v_xqs.reserve((size_t)Q * Hd * sizeof(float)));
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
    auto pre_at = [&](int c0, SplitRef* r) -> const SplitRef* {  // the cached split of chunks c0.. (nullptr: split per sub-batch)
        if (!have_w) return nullptr;
        const long o = (long)c0 * chunk_k;
        *r = SplitRef{wref.Fh + o, wref.Fl ? wref.Fl + o : nullptr, wref.Th + o, wref.Tl ? wref.Tl + o : nullptr};
        return r;
    };
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

    // embeddings: LayerNorm of the learned query tokens (chunk-independent)
    QfEpilogue e0{};
    e0.parts = w->query_tokens; e0.nsplit = 1; e0.ld_in = Hd; e0.seg_cols = Hd; e0.scale = 1.f; e0.res_scale = 1.f;
    e0.gamma = w->emb_ln.gamma; e0.beta = w->emb_ln.beta; e0.eps = c.ln_eps;
    e0.out = h->h_a.as<float>(); e0.ld_out = Hd; e0.M = Q; e0.width = Hd; e0.res_rows = 1;
    HIP_TRY(launch_qf_epilogue(e0, stream));

    auto ltm_u = [&](int l) -> int {                          // u[:, l, :] -> contiguous [C][S] for a one-layer handle
        if (!u) return INFV_OK;
        HIP_TRY(hipMemcpy2DAsync(h->vu.p, (size_t)S * sizeof(double), u + (size_t)l * S, (size_t)c.n_layers * S * sizeof(double),
                                 (size_t)S * sizeof(double), (size_t)C, hipMemcpyDeviceToDevice, stream));
        return INFV_OK;
    };

    for (int l = 0; l < c.n_layers; ++l) {
        const infv_vqf_layer& L = w->layer[l];
        infv_ltm_proj pr{};
        pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
        const bool shared = (l == 0);                         // layer 0: the hidden states entering it do not depend on the chunk
        const float* res1;                                    // residual / input of the cross-attention block
        int res1_rows;
        if (shared) {
            // ---- self-attention block + cross query once ----
            LinearCall qkv{h->h_a.as<float>(), Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
            qkv.inv = multi;
            qkv.y = h->qkv.as<float>();
            if (int rc = run_linear(h, qkv, stream)) return rc;
            HIP_TRY(launch_qf_self_attention(h->qkv.as<float>(), 1, Q, c.n_heads, h->sa.as<float>(), stream));
            LinearCall so{h->sa.as<float>(), Q, Hd, {&L.self_o}, 1, Hd};
            so.inv = multi;
            so.residual = h->h_a.as<float>(); so.res_rows = Q; so.ln = &L.self_ln; so.y = h->v_h1s.as<float>();
            if (int rc = run_linear(h, so, stream)) return rc;
            LinearCall xq{h->v_h1s.as<float>(), Q, Hd, {&L.x_q}, 1, Hd};
            xq.inv = multi;
            xq.y = h->v_xqs.as<float>();
            if (int rc = run_linear(h, xq, stream)) return rc;
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
            for (int c0 = 0; c0 < C; c0 += NB) {
                const int nb = C - c0 < NB ? C - c0 : NB;
                SplitRef sr;
                if (int rc = short_attention(h, tok_at(frames, tok, c0 * chunk_k), tok, nb, n_tokens, h->v_xqs.as<float>(), true, &L.x_k, &L.x_v,
                                             use_ltm ? valong + (long)c0 * Q * Hd : nullptr, vmerged + (long)c0 * Q * Hd, stream,
                                             false, pre_at(c0, &sr), nullptr, multi ? kInvariantNb : 0)) return rc;
            }
        } else {
            // ---- self-attention block + cross query of every chunk (row blocks) ----
            for (int c0 = 0; c0 < C; c0 += RB) {
                const int nb = C - c0 < RB ? C - c0 : RB;
                const long r0 = (long)c0 * Q * Hd;
                LinearCall qkv{vA + r0, nb * Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
                qkv.inv = multi;
                qkv.y = h->vqkv.as<float>();
                if (int rc = run_linear(h, qkv, stream)) return rc;
                HIP_TRY(launch_qf_self_attention(h->vqkv.as<float>(), nb, Q, c.n_heads, h->vsa.as<float>(), stream));
                LinearCall so{h->vsa.as<float>(), nb * Q, Hd, {&L.self_o}, 1, Hd};
                so.inv = multi;
                so.residual = vA + r0; so.res_rows = nb * Q; so.ln = &L.self_ln; so.y = v1 + r0;
                if (int rc = run_linear(h, so, stream)) return rc;
                LinearCall xq{v1 + r0, nb * Q, Hd, {&L.x_q}, 1, Hd};
                xq.inv = multi;
                xq.y = vxq + r0;
                if (int rc = run_linear(h, xq, stream)) return rc;
            }
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
            for (int c0 = 0; c0 < C; c0 += NB) {
                const int nb = C - c0 < NB ? C - c0 : NB;
                SplitRef sr;
                if (int rc = short_attention(h, tok_at(frames, tok, c0 * chunk_k), tok, nb, n_tokens, vxq + (long)c0 * Q * Hd, false, &L.x_k, &L.x_v,
                                             nullptr, (use_ltm ? vshort : vmerged) + (long)c0 * Q * Hd, stream, false,
                                             pre_at(c0, &sr), nullptr, multi ? kInvariantNb : 0)) return rc;
            }
            if (use_ltm) {
                HIP_TRY(hipStreamWaitEvent(stream, h->ev_side, 0));
                for (long m0 = 0; m0 < M; m0 += kMergeRows) {  // merged = alpha * short + (1 - alpha) * long
                    QfEpilogue em{};
                    em.parts = vshort + m0 * Hd; em.nsplit = 1; em.ld_in = Hd; em.seg_cols = Hd;
                    em.scale = c.alpha; em.res_scale = (float)(1.0 - (double)c.alpha);
                    em.residual = valong + m0 * Hd; em.ld_res = Hd; em.res_rows = (int)(M - m0 < kMergeRows ? M - m0 : kMergeRows);
                    em.out = vmerged + m0 * Hd; em.ld_out = Hd; em.M = em.res_rows; em.width = Hd; em.eps = c.ln_eps;
                    HIP_TRY(launch_qf_epilogue(em, stream));
                }
            }
        }
        // ---- cross-attention output + query FFN of every chunk (row blocks) ----
        for (int c0 = 0; c0 < C; c0 += RB) {
            const int nb = C - c0 < RB ? C - c0 : RB;
            const long r0 = (long)c0 * Q * Hd;
            LinearCall xo{vmerged + r0, nb * Q, Hd, {&L.x_o}, 1, Hd};
            xo.inv = multi;
            xo.residual = shared ? res1 : res1 + r0; xo.res_rows = shared ? res1_rows : nb * Q; xo.ln = &L.x_ln; xo.y = v2 + r0;
            if (int rc = run_linear(h, xo, stream)) return rc;
            LinearCall fi{v2 + r0, nb * Q, Hd, {&L.ffn_in}, 1, c.inter};
            fi.inv = multi;
            fi.act = QF_ACT_GELU; fi.y = h->vinter.as<float>();
            if (int rc = run_linear(h, fi, stream)) return rc;
            LinearCall fo{h->vinter.as<float>(), nb * Q, c.inter, {&L.ffn_out}, 1, Hd};
            fo.inv = multi;
            fo.residual = v2 + r0; fo.res_rows = nb * Q; fo.ln = &L.ffn_ln; fo.y = vA + r0;
            if (int rc = run_linear(h, fo, stream)) return rc;
        }
    }
    if (hidden_out)
        HIP_TRY(hipMemcpyAsync(hidden_out, vA, (size_t)M * Hd * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (llama_out || llama_mean) {
        float* lo = llama_out;
        if (!lo) {                                             // only the mean is wanted: project into scratch
            const size_t need = (size_t)M * c.proj_out * sizeof(float);
            if (need > h->S.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->S.reserve(need)); }
            lo = h->S.as<float>();
        }
        for (int c0 = 0; c0 < C; c0 += RB) {
            const int nb = C - c0 < RB ? C - c0 : RB;
            LinearCall pj{vA + (long)c0 * Q * Hd, nb * Q, Hd, {&w->llama_proj}, 1, c.proj_out};
            pj.inv = multi;
            pj.y = lo + (long)c0 * Q * c.proj_out;
            if (int rc = run_linear(h, pj, stream)) return rc;
        }
        if (llama_mean && multi) HIP_TRY(launch_qf_mean_segments(lo, cu, V, (long)Q * c.proj_out, llama_mean, stream));
        else if (llama_mean) HIP_TRY(launch_qf_mean(lo, C, (long)Q * c.proj_out, llama_mean, stream));
    }
    return INFV_OK;
}

int infv_vqf_encode_video(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t n_chunks,
                          int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, float* llama_mean, void* stream_) {
    if (!h || !frames || !w || n_chunks < 1) return fail(INFV_ERR_INVALID, "bad argument");
    return encode_impl(h, ltm, frames, n_chunks, T, w, u, new_video, hidden_out, llama_out, llama_mean, stream_, 1, nullptr, false);
}

int infv_vqf_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                           int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video, float* hidden_out,
                           float* llama_out, float* llama_mean, void* stream_) {
    // ---- validation before any device work or memory change ----
    if (!h || !cu || !w || V < 0) return fail(INFV_ERR_INVALID, "encode_videos: bad arguments");
    if (V == 0) return INFV_OK;
    if (cu[0] != 0) return fail(INFV_ERR_INVALID, "encode_videos: cu[0] = %d, not 0", cu[0]);
    for (int v = 0; v < V; ++v)
        if (cu[v + 1] < cu[v]) return fail(INFV_ERR_INVALID, "encode_videos: cu is not non-decreasing (cu[%d] = %d > cu[%d] = %d)",
                                            v, cu[v], v + 1, cu[v + 1]);
    const bool use_ltm = h->cfg.alpha != 1.0f;
    const int n_h = use_ltm ? V * h->cfg.n_layers : 0;
    if (use_ltm) {
        if (!ltm) return fail(INFV_ERR_INVALID, "encode_videos: alpha != 1 needs the per-layer LTM handles of every video");
        std::vector<infv_ltm_handle> all(ltm, ltm + n_h);
        for (int i = 0; i < n_h; ++i)
            if (!all[i]) return fail(INFV_ERR_INVALID, "encode_videos: LTM handle %d is null", i);
        std::sort(all.begin(), all.end());
        if (std::adjacent_find(all.begin(), all.end()) != all.end())
            return fail(INFV_ERR_INVALID, "encode_videos: an LTM handle appears twice (every video and layer needs its own memory)");
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

// The body of infv_vqf_vc_encode_videos (fcu == nullptr: stream v reads its own chunks [cu[v], cu[v+1]) of `frames`) and of
// infv_vqf_vc_encode_streams (stream v reads block frame_src[v] of the F blocks packed by fcu).  `name` prefixes the refusals.
static int vc_impl(const char* name, infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                   int32_t token_dtype /* < 0: the entry points without the argument -- fp32, refused unless the handle's setting is fp32 too */,
                   int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in,
                   const int32_t* text_len, const double* u, int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean,
                   void* stream_, const infv_vqf_vc_front* front = nullptr /* infv_vqf_vc_encode_img: vision LayerNorm and / or embedding layer in front */,
                   const FrameCall* fc = nullptr /* infv_vqf_encode_frames: every chunk is one frame of fc->n_tokens tokens */) {
    // ---- validation before any device work or memory change ----
    if (!h || !cu || !w || !text_len || V < 0) return fail(INFV_ERR_INVALID, "%s: bad arguments", name);
    if (front && front->reserved != 0) return fail(INFV_ERR_INVALID, "%s: front->reserved must be 0", name);
    const bool vis_ln = front && front->vision_ln.gamma;       // the vision LayerNorm runs inside the token pass
    const bool emb = front && front->emb.word;                 // the embedding layer writes the encoder input rows
    if (vis_ln && !front->vision_ln.beta) return fail(INFV_ERR_INVALID, "%s: vision_ln.gamma without vision_ln.beta", name);
    if (emb && hidden_in) return fail(INFV_ERR_INVALID, "%s: the embedding layer and hidden_in are both given (one of them writes the input rows)", name);
    const bool tok_arg = token_dtype >= 0;                     // the dtype is an argument of the call: the handle's setting is not read
    if (tok_arg && !token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "%s: unknown token dtype %d", name, token_dtype);
    tok_code tok = tok_arg ? static_cast<tok_code>(token_dtype) : INFV_TOKENS_F32;
    // (the vision LayerNorm of fp8 tokens is not built: no vision encoder emits fp8)
    if (vis_ln && tok == INFV_TOKENS_F8E4M3) return fail(INFV_ERR_UNSUPPORTED, "%s: no vision LayerNorm of fp8 frame tokens", name);
    if (tok != INFV_TOKENS_F32 && frames && !aligned16(frames)) return fail(INFV_ERR_INVALID, "%s: fp16 / bf16 / fp8 frames must be 16-byte aligned", name);
    if (vis_ln && frames && !aligned16(frames)) return fail(INFV_ERR_INVALID, "%s: frames must be 16-byte aligned for the vision LayerNorm", name);
    if (V == 0) return INFV_OK;
    const infv_vqf_config& c = h->cfg;
    if (cu[0] != 0) return fail(INFV_ERR_INVALID, "%s: cu[0] = %d, not 0", name, cu[0]);
    for (int v = 0; v < V; ++v)
        if (cu[v + 1] < cu[v]) return fail(INFV_ERR_INVALID, "%s: cu is not non-decreasing (cu[%d] = %d > cu[%d] = %d)", name,
                                            v, cu[v], v + 1, cu[v + 1]);
    const bool streams = fcu != nullptr;
    if (streams) {
        if (!frame_src || F < 1) return fail(INFV_ERR_INVALID, "%s: bad arguments", name);
        if (fcu[0] != 0) return fail(INFV_ERR_INVALID, "%s: fcu[0] = %d, not 0", name, fcu[0]);
        for (int f = 0; f < F; ++f)
            if (fcu[f + 1] < fcu[f]) return fail(INFV_ERR_INVALID, "%s: fcu is not non-decreasing (fcu[%d] = %d > fcu[%d] = %d)",
                                                name, f, fcu[f], f + 1, fcu[f + 1]);
        for (int v = 0; v < V; ++v) {
            const int s = frame_src[v];
            if (s < 0 || s >= F) return fail(INFV_ERR_INVALID, "%s: frame_src[%d] = %d outside [0, %d)", name, v, s, F);
            if (cu[v + 1] - cu[v] != fcu[s + 1] - fcu[s])
                return fail(INFV_ERR_INVALID, "%s: stream %d has %d chunks, its block %d has %d", name, v, cu[v + 1] - cu[v], s,
                            fcu[s + 1] - fcu[s]);
        }
    }
    if (w->n_layers < 1 || !w->layers) return fail(INFV_ERR_INVALID, "%s: no layers", name);
    if (w->n_layers > INFV_VQF_VC_MAX_LAYERS)
        return fail(INFV_ERR_UNSUPPORTED, "%s: %d layers, at most %d are supported", name, w->n_layers, INFV_VQF_VC_MAX_LAYERS);
    const int Q = c.n_query, Hd = c.hidden, S = c.nb_samples, Ln = w->n_layers;
    for (int v = 0; v < V; ++v) {
        if (text_len[v] < 0) return fail(INFV_ERR_INVALID, "%s: text_len[%d] = %d is negative", name, v, text_len[v]);
        if (Q + text_len[v] > INFV_VQF_VC_MAX_TOKENS)
            return fail(INFV_ERR_UNSUPPORTED, "%s: video %d attends over %d + %d tokens, at most %d are supported", name,
                        v, Q, text_len[v], INFV_VQF_VC_MAX_TOKENS);
    }
    if (emb)
        if (int rc = check_front_emb(name, front, V, text_len)) return rc;
    if (T < 1) return fail(INFV_ERR_INVALID, "%s: T must be >= 1", name);
    const int n_live = fc ? fc->n_tokens : T * c.tokens_per_frame;   // tokens a chunk holds in `frames`
    if (!fc && n_live % 32) return fail(INFV_ERR_UNSUPPORTED, "%s: T * tokens_per_frame = %d is no multiple of 32", name, n_live);
    bool pad = false;                                          // frames: planes and score rows padded to the next multiple of 64
    if (fc) {
        if (n_live < 1) return fail(INFV_ERR_INVALID, "%s: n_tokens = %d, must be >= 1", name, n_live);
        if (n_live > 0x7fffffff - 128) return fail(INFV_ERR_UNSUPPORTED, "%s: n_tokens = %d is too large", name, n_live);
        if (c.enc_width % 64) return fail(INFV_ERR_UNSUPPORTED, "%s: enc_width = %d is no multiple of 64", name, c.enc_width);
        pad = n_live % 64 != 0 && split_path(h, 64);
        if (n_live % 32 && !pad)
            return fail(INFV_ERR_UNSUPPORTED, "%s: the fp32 contractions (set_precision(h, 1) / INFV_VQF_FP32) need n_tokens %% 32 == 0, got %d", name, n_live);
    }
    const int n_tokens = pad ? (n_live + 63) / 64 * 64 : n_live;   // keys a chunk has in the contractions (pad keys: zeros, no mass)
    if (vis_ln && (c.enc_width % 64 || c.enc_width > kTokenLnMaxWidth))
        return fail(INFV_ERR_UNSUPPORTED, "%s: the vision LayerNorm needs enc_width = %d to be a multiple of 64, at most %d", name, c.enc_width,
                    kTokenLnMaxWidth);
    if (!tok_arg && h->tok != INFV_TOKENS_F32)
        return fail(INFV_ERR_UNSUPPORTED, "%s: fp16 / bf16 frame tokens are not supported on this path (the _tok entry point takes them)", name);
    int n_cross = 0;
    for (int l = 0; l < Ln; ++l) n_cross += w->layers[l].has_cross != 0;
    const bool use_ltm = !fc && c.alpha != 1.0f && n_cross > 0;   // (frames: position_embedding_ext == None, no memory is called)
    const int n_h = use_ltm ? V * n_cross : 0;
    if (use_ltm) {
        if (!ltm) return fail(INFV_ERR_INVALID, "%s: alpha != 1 needs the LTM handles of every video and cross layer", name);
        std::vector<infv_ltm_handle> all(ltm, ltm + n_h);
        for (int i = 0; i < n_h; ++i)
            if (!all[i]) return fail(INFV_ERR_INVALID, "%s: LTM handle %d is null", name, i);
        std::sort(all.begin(), all.end());
        if (std::adjacent_find(all.begin(), all.end()) != all.end())
            return fail(INFV_ERR_INVALID, "%s: an LTM handle appears twice (every video and cross layer needs its own memory)", name);
    }
    if ((proj_out || proj_mean) && (c.proj_out <= 0 || !w->mistral_proj.w))
        return fail(INFV_ERR_INVALID, "%s: projected output without mistral_proj", name);
    if (fc && fc->out_dtype != INFV_TOKENS_F32) {             // the last layer's epilogue writes the 2-byte rows: its 16-byte form only
        const infv_vqf_vc_layer& L = w->layers[Ln - 1];
        if (!aligned16(L.q_ffn_out.b) || !aligned16(L.q_ffn_ln.gamma) || !aligned16(L.q_ffn_ln.beta) || !L.q_ffn_ln.gamma || !L.q_ffn_ln.beta)
            return fail(INFV_ERR_INVALID, "%s: bf16 / fp16 output needs the last layer's q_ffn_out.b and q_ffn_ln 16-byte aligned", name);
    }
    if (fc && h->tap_dst && (h->tap_layer >= Ln || !w->layers[h->tap_layer].has_cross))
        return fail(INFV_ERR_INVALID, "%s: the context tap names layer %d, which is no cross-attention layer of these weights", name, h->tap_layer);
    const int C = cu[V];
    if (C == 0) {                                             // no chunk: new_video still starts every memory afresh
        if (use_ltm && new_video)
            for (int i = 0; i < n_h; ++i) infv_ltm_reset(ltm[i]);
        return INFV_OK;
    }
    if (!frames || (!hidden_in && !emb)) return fail(INFV_ERR_INVALID, "%s: null frames or hidden_in", name);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (use_ltm)
        if (int rc = ensure_streams(h)) return rc;

    // ---- host tables: per chunk its video's text length, the offset of its packed text rows, its rows in hidden_in / hidden_out
    std::vector<int32_t> n_valid(C), toff(C + 1, 0), q_dst(C), q_src(C), t_src(C), tl(C), o_q(C), o_t(C), q_n(C, Q);
    {
        int32_t in_row = 0, c_i = 0;
        for (int v = 0; v < V; ++v) {
            for (int cc = cu[v]; cc < cu[v + 1]; ++cc, ++c_i) {
                tl[cc] = text_len[v]; n_valid[cc] = Q + text_len[v]; toff[cc + 1] = toff[cc] + text_len[v];
                q_dst[cc] = cc * Q; q_src[cc] = fc ? 0 : in_row; t_src[cc] = in_row + Q;   // (frames: one block of query rows for all)
                o_q[cc] = cc * Q + toff[cc]; o_t[cc] = o_q[cc] + Q;
            }
            in_row += Q + text_len[v];
        }
    }
    const long M = (long)C * Q, Tt = toff[C];
    const long chunk_k = (long)n_tokens * c.enc_width;         // elements of a chunk in the planes ...
    const long src_k = (long)n_live * c.enc_width;             // ... and in `frames` (the same unless padded)
    const int Cf = streams ? fcu[F] : C;                       // distinct chunks of frame tokens
    TokLn ln_{}; const TokLn* ln = nullptr;                    // the vision LayerNorm on load (split path), else nullptr
    if (vis_ln && n_cross > 0) {
        // (mean, 1 / sqrt(var + eps)) of every DISTINCT token row, once per call: 8 bytes per token
        const size_t rows = (size_t)Cf * n_live;
        if (rows * 2 * sizeof(float) > h->lnstats.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->lnstats.reserve(rows * 2 * sizeof(float))); }
        HIP_TRY(launch_token_ln_stats(frames, tok, (long)rows, c.enc_width, front->vision_ln.eps, h->lnstats.p, stream));
        if (split_path(h, n_tokens)) {
            ln_ = TokLn{h->lnstats.as<float>(), front->vision_ln.gamma, front->vision_ln.beta};
            ln = &ln_;
        } else {                                               // the fp32 contractions from the normalised fp32 copy of the distinct chunks
            const size_t elems = rows * c.enc_width;
            if (elems * sizeof(float) > h->up.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->up.reserve(elems * sizeof(float))); }
            HIP_TRY(launch_ln_tokens(frames, tok, (long)rows, c.enc_width, h->lnstats.p, front->vision_ln.gamma, front->vision_ln.beta,
                                     h->up.as<float>(), stream));
            frames = h->up.p; tok = INFV_TOKENS_F32;
        }
    }
    if (tok != INFV_TOKENS_F32 && n_cross > 0 && !split_path(h, n_tokens)) {   // today's fp32 kernels from an fp32 copy of the distinct chunks
        const float* f32 = nullptr;
        if (int rc = upcast_tokens(h, frames, tok, (size_t)Cf * chunk_k, &f32, stream)) return rc;
        frames = f32; tok = INFV_TOKENS_F32;
    }
    std::vector<int32_t> src_chunk, kbar0;                     // streams: each stream-chunk's source chunk, each stream's first one
    if (streams) {
        src_chunk.resize(C); kbar0.resize(V);
        for (int v = 0; v < V; ++v) {
            kbar0[v] = fcu[frame_src[v]];
            for (int i = 0; i < cu[v + 1] - cu[v]; ++i) src_chunk[cu[v] + i] = kbar0[v] + i;
        }
    }
    const int RB = C < kRowBlockVideos ? C : kRowBlockVideos;  // chunks per row block of the token GEMMs (batch invariant: any size)
    const long TB = Tt < kTextFfnRows ? Tt : kTextFfnRows;     // text rows per block of the text FFN
    long tb_max = 0;                                           // text rows of the largest row block
    for (int c0 = 0; c0 < C; c0 += RB) { const int c1 = c0 + RB < C ? c0 + RB : C; tb_max = std::max<long>(tb_max, toff[c1] - toff[c0]); }
    const int NB = pick_short_nb(h, C, n_tokens);
    {
        const size_t act = (size_t)M * Hd * sizeof(float), tact = (size_t)Tt * Hd * sizeof(float);
        const bool grow = act > h->vA.bytes || act > h->v1.bytes || act > h->v2.bytes || act > h->vxq.bytes || act > h->vshort.bytes ||
                          act > h->vmerged.bytes || (use_ltm && act > h->valong.bytes) ||
                          (size_t)RB * Q * 3 * Hd * sizeof(float) > h->vqkv.bytes || (size_t)RB * Q * Hd * sizeof(float) > h->vsa.bytes ||
                          (size_t)RB * Q * c.inter * sizeof(float) > h->vinter.bytes || tact > h->tA.bytes || tact > h->t1.bytes ||
                          (size_t)tb_max * 3 * Hd * sizeof(float) > h->tqkv.bytes || (size_t)tb_max * Hd * sizeof(float) > h->tsa.bytes ||
                          (size_t)TB * c.inter * sizeof(float) > h->tinter.bytes ||
                          (use_ltm && ((size_t)C * S * sizeof(double) > h->vu.bytes || (size_t)Cf * T * c.enc_width * sizeof(float) > h->vkbar.bytes)) ||
                          (streams && (size_t)C * sizeof(int32_t) > h->smap.bytes);
        if (grow) HIP_TRY(hipDeviceSynchronize());
        if (streams) HIP_TRY(h->smap.reserve((size_t)C * sizeof(int32_t)));
        HIP_TRY(h->vA.reserve(act)); HIP_TRY(h->v1.reserve(act)); HIP_TRY(h->v2.reserve(act)); HIP_TRY(h->vxq.reserve(act));
        HIP_TRY(h->vshort.reserve(act)); HIP_TRY(h->vmerged.reserve(act));
        if (use_ltm) {
            HIP_TRY(h->valong.reserve(act));
            HIP_TRY(h->vu.reserve((size_t)C * S * sizeof(double)));
            HIP_TRY(h->vkbar.reserve((size_t)Cf * T * c.enc_width * sizeof(float)));
        }
        HIP_TRY(h->vqkv.reserve((size_t)RB * Q * 3 * Hd * sizeof(float)));
        HIP_TRY(h->vsa.reserve((size_t)RB * Q * Hd * sizeof(float)));
        HIP_TRY(h->vinter.reserve((size_t)RB * Q * c.inter * sizeof(float)));
        if (Tt > 0) {
            HIP_TRY(h->tA.reserve(tact)); HIP_TRY(h->t1.reserve(tact));
            HIP_TRY(h->tqkv.reserve((size_t)tb_max * 3 * Hd * sizeof(float)));
            HIP_TRY(h->tsa.reserve((size_t)tb_max * Hd * sizeof(float)));
            HIP_TRY(h->tinter.reserve((size_t)TB * c.inter * sizeof(float)));
        }
    }
    float* vA = h->vA.as<float>(); float* v1 = h->v1.as<float>(); float* v2 = h->v2.as<float>();
    float* vxq = h->vxq.as<float>(); float* valong = h->valong.as<float>();
    float* vshort = h->vshort.as<float>(); float* vmerged = h->vmerged.as<float>();
    float* tA = h->tA.as<float>(); float* t1 = h->t1.as<float>();

    if (emb) {                                                 // the embedding layer writes the packed encoder input rows (Qformer.py:54-111)
        long n_in = 0;
        for (int v = 0; v < V; ++v) n_in += Q + text_len[v];
        const size_t need = (size_t)n_in * Hd * sizeof(float);
        if (need > h->embrows.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->embrows.reserve(need)); }
        if (int rc = run_embed(h, front, V, text_len, h->embrows.as<float>(), stream)) return rc;
        hidden_in = h->embrows.as<float>();
    }
    // ---- every chunk starts from its video's encoder input rows
    HIP_TRY(launch_qf_copy_rows(hidden_in, vA, q_dst.data(), q_src.data(), q_n.data(), C, Hd, stream));
    if (Tt > 0) HIP_TRY(launch_qf_copy_rows(hidden_in, tA, toff.data(), t_src.data(), tl.data(), C, Hd, stream));

    // ---- ONE pass over the frame tokens: split-bf16 operands of every cross layer's short-term attention (kept for the call
    //      when they fit INFV_VQF_SPLIT_CACHE_GB) and the frame means every cross layer's memories step from
    SplitRef wref{}; bool have_w = false, have_kbar = false;
    if (n_cross > 0) {
        // (streams: the distinct chunks only; bf16 tokens: only the transposed plane is written, as in infv_vqf_encode_video)
        const double need_gb = plane_bytes(tok, ln != nullptr, pad) * (double)Cf * (double)chunk_k / 1e9;
        if (h->fuse && split_path(h, n_tokens) && need_gb <= h->split_cache_gb) {
            have_kbar = use_ltm && token_pass_gives_means(c.tokens_per_frame);   // (where a frame divides the 64-token tile)
            if (int rc = prepare_split(h, frames, tok, Cf, n_tokens, have_kbar ? h->vkbar.as<float>() : nullptr, true, &wref, stream, 0, 0, ln,
                                       pad ? n_live : 0)) return rc;
            have_w = true;
        }
        if (use_ltm && !have_kbar && ln) {                     // pooling with the LayerNorm on load: the means of the normalised tokens
            HIP_TRY(launch_pool_ln(frames, tok, ln->stats, ln->gamma, ln->beta, h->vkbar.as<float>(), (int64_t)Cf * T, c.tokens_per_frame,
                                   c.enc_width, stream));
        } else if (use_ltm && !have_kbar) {
            if (int rc = infv_ltm_set_token_dtype(ltm[0], tok)) return rc;
            const int rc_pool = infv_ltm_pool(ltm[0], frames, (int64_t)Cf * T, h->vkbar.as<float>(), stream_);
            if (int rc = infv_ltm_set_token_dtype(ltm[0], INFV_TOKENS_F32)) return rc;   // (left on fp32, as before)
            if (rc_pool) return rc_pool;
        }
    }
    // the chunk map reaches the device in kernel arguments, once per call: no host buffer outlives the call, nothing waits on the host
    if (streams && n_cross > 0) HIP_TRY(launch_qf_write_map(h->smap.as<int32_t>(), src_chunk.data(), C, stream));
    // The frame operand of the short-term attention of stream-chunks [c0, c0 + nb): *fr (fp32 path) or the planes *r, and the map
    // the contractions read them through (nullptr: chunk b of the sub-batch is entry b).
    //   videos:  today's -- the cached planes at c0, else the caller's tokens at c0 (split per sub-batch inside short_attention)
    //   streams: the cached planes of the DISTINCT chunks, or the caller's tokens on the fp32 path, read through the map; where the
    //            planes do not fit, each contiguous run of source chunks is split into the sub-batch's own planes (identity map)
    auto operand_at = [&](int c0, int nb, SplitRef* r, const SplitRef** pre, const void** fr, const int32_t** map, bool* t_identity) -> int {
        *pre = nullptr; *map = nullptr; *t_identity = false; *fr = tok_at(frames, tok, (long)c0 * src_k);
        if (!streams) {
            if (have_w) {
                const long o = (long)c0 * chunk_k;
                *r = SplitRef{wref.Fh + o, wref.Fl ? wref.Fl + o : nullptr, wref.Th + o, wref.Tl ? wref.Tl + o : nullptr};
                *pre = r;
            } else if (ln || pad) {                            // the split per sub-batch short_attention would issue, with the LayerNorm on load / padded
                TokLn lc{};
                if (ln) lc = TokLn{ln->stats + 2 * (size_t)c0 * n_live, ln->gamma, ln->beta};
                if (int rc = prepare_split(h, *fr, tok, nb, n_tokens, nullptr, false, r, stream, 0, 0, ln ? &lc : nullptr, pad ? n_live : 0)) return rc;
                *pre = r;
            }
            return INFV_OK;
        }
        if (have_w) { *r = wref; *pre = r; *map = h->smap.as<int32_t>() + c0; return INFV_OK; }
        if (!split_path(h, n_tokens)) { *fr = frames; *map = h->smap.as<int32_t>() + c0; return INFV_OK; }
        for (int b0 = 0; b0 < nb;) {
            int b1 = b0 + 1;
            while (b1 < nb && src_chunk[c0 + b1] == src_chunk[c0 + b1 - 1] + 1) ++b1;
            TokLn lc{};
            if (ln) lc = TokLn{ln->stats + 2 * (size_t)src_chunk[c0 + b0] * n_tokens, ln->gamma, ln->beta};
            if (int rc = prepare_split(h, tok_at(frames, tok, (long)src_chunk[c0 + b0] * chunk_k), tok, b1 - b0, n_tokens, nullptr, false, r,
                                       stream, b0, nb, ln ? &lc : nullptr)) return rc;
            b0 = b1;
        }
        if (tok == INFV_TOKENS_BF16 && !ln) {                         // the untransposed operand is the caller's buffer: read through the map,
            r->Fh = static_cast<const __bf16*>(frames);        // while the transposed plane just written holds the sub-batch in order
            *map = h->smap.as<int32_t>() + c0; *t_identity = true;
        }
        *pre = r;
        return INFV_OK;
    };
    std::vector<infv_ltm_handle> hs_l(use_ltm ? V : 0);
    std::vector<int32_t> off1(RB);

    int j_cross = 0;
    for (int l = 0; l < Ln; ++l) {
        const infv_vqf_vc_layer& L = w->layers[l];
        const bool cross = L.has_cross != 0;
        const bool last = l == Ln - 1;
        const bool text_out = Tt > 0 && (!last || hidden_out);   // the last layer's text rows feed nothing but hidden_out
        // ---- self-attention over query + text tokens, output dense + LayerNorm, cross query (row blocks of chunks) ----
        for (int c0 = 0; c0 < C; c0 += RB) {
            const int nb = C - c0 < RB ? C - c0 : RB;
            const long r0 = (long)c0 * Q * Hd, t0 = toff[c0], tn = toff[c0 + nb] - t0;
            LinearCall qkv{vA + r0, nb * Q, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
            qkv.inv = true; qkv.y = h->vqkv.as<float>();
            if (int rc = run_linear(h, qkv, stream)) return rc;
            if (tn > 0) {
                LinearCall qkt{tA + t0 * Hd, (int)tn, Hd, {&L.self_q, &L.self_k, &L.self_v}, 3, Hd};
                qkt.inv = true; qkt.y = h->tqkv.as<float>();
                if (int rc = run_linear(h, qkt, stream)) return rc;
            }
            for (int b = 0; b < nb; ++b) off1[b] = toff[c0 + b] - (int32_t)t0;
            VcAttn a{};
            a.qkv0 = h->vqkv.as<float>(); a.rows0 = Q; a.nsplit = Q; a.qkv1 = h->tqkv.as<float>();
            a.ctx0 = h->vsa.as<float>(); a.ctx1 = h->tsa.as<float>(); a.H = c.n_heads; a.n_alloc = 0;
            HIP_TRY(launch_qf_vc_self_attention(a, nb, n_valid.data() + c0, off1.data(), stream));
            LinearCall so{h->vsa.as<float>(), nb * Q, Hd, {&L.self_o}, 1, Hd};
            so.inv = true; so.residual = vA + r0; so.res_rows = nb * Q; so.ln = &L.self_ln; so.y = v1 + r0;
            if (int rc = run_linear(h, so, stream)) return rc;
            if (tn > 0 && text_out) {
                LinearCall st{h->tsa.as<float>(), (int)tn, Hd, {&L.self_o}, 1, Hd};
                st.inv = true; st.residual = tA + t0 * Hd; st.res_rows = (int)tn; st.ln = &L.self_ln; st.y = t1 + t0 * Hd;
                if (int rc = run_linear(h, st, stream)) return rc;
            }
            if (cross) {
                LinearCall xq{v1 + r0, nb * Q, Hd, {&L.x_q}, 1, Hd};
                xq.inv = true; xq.y = vxq + r0;
                if (int rc = run_linear(h, xq, stream)) return rc;
            }
        }
        const float* qin = v1;                                 // the query rows entering the query FFN
        if (cross) {
            // ---- this layer's V memories with per-chunk queries on the worker stream, beside the short-term attention ----
            if (use_ltm) {
                infv_ltm_proj pr{};
                pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
                if (u)                                         // u[:, j, :] -> contiguous [C][S] for the one-layer handles
                    HIP_TRY(hipMemcpy2DAsync(h->vu.p, (size_t)S * sizeof(double), u + (size_t)j_cross * S, (size_t)n_cross * S * sizeof(double),
                                             (size_t)S * sizeof(double), (size_t)C, hipMemcpyDeviceToDevice, stream));
                HIP_TRY(hipEventRecord(h->ev_main, stream));
                HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
                for (int v = 0; v < V; ++v) hs_l[v] = ltm[(size_t)v * n_cross + j_cross];
                if (int rc = infv_ltm_steps_videos_from(hs_l.data(), V, cu, h->vkbar.as<float>(), streams ? kbar0.data() : nullptr, T, vxq, 1,
                                                        Q, &pr, u ? h->vu.as<double>() : nullptr, new_video, valong, h->side)) return rc;
                HIP_TRY(hipEventRecord(h->ev_side, h->side));
            }
            for (int c0 = 0; c0 < C; c0 += NB) {
                const int nb = C - c0 < NB ? C - c0 : NB;
                SplitRef sr; const SplitRef* pre; const void* fr; const int32_t* map; bool t_identity;
                if (int rc = operand_at(c0, nb, &sr, &pre, &fr, &map, &t_identity)) return rc;
                if (int rc = short_attention(h, fr, tok, nb, n_tokens, vxq + (long)c0 * Q * Hd, false, &L.x_k, &L.x_v,
                                             nullptr, (use_ltm ? vshort : vmerged) + (long)c0 * Q * Hd, stream, false,
                                             pre, nullptr, kInvariantNb, map, t_identity, pad ? n_live : 0)) return rc;
            }
            if (use_ltm) {
                HIP_TRY(hipStreamWaitEvent(stream, h->ev_side, 0));
                for (long m0 = 0; m0 < M; m0 += kMergeRows) {  // merged = alpha * short + (1 - alpha) * long
                    QfEpilogue em{};
                    em.parts = vshort + m0 * Hd; em.nsplit = 1; em.ld_in = Hd; em.seg_cols = Hd;
                    em.scale = c.alpha; em.res_scale = (float)(1.0 - (double)c.alpha);
                    em.residual = valong + m0 * Hd; em.ld_res = Hd; em.res_rows = (int)(M - m0 < kMergeRows ? M - m0 : kMergeRows);
                    em.out = vmerged + m0 * Hd; em.ld_out = Hd; em.M = em.res_rows; em.width = Hd; em.eps = c.ln_eps;
                    HIP_TRY(launch_qf_epilogue(em, stream));
                }
            }
            if (fc && h->tap_dst && l == h->tap_layer)         // (tests: this layer's cross-attention context, Qformer.py:303-304)
                HIP_TRY(hipMemcpyAsync(h->tap_dst, vmerged, (size_t)M * Hd * sizeof(float), hipMemcpyDeviceToDevice, stream));
            for (int c0 = 0; c0 < C; c0 += RB) {
                const int nb = C - c0 < RB ? C - c0 : RB;
                const long r0 = (long)c0 * Q * Hd;
                LinearCall xo{vmerged + r0, nb * Q, Hd, {&L.x_o}, 1, Hd};
                xo.inv = true; xo.residual = v1 + r0; xo.res_rows = nb * Q; xo.ln = &L.x_ln; xo.y = v2 + r0;
                if (int rc = run_linear(h, xo, stream)) return rc;
            }
            qin = v2;
            ++j_cross;
        }
        // ---- query FFN on the query rows, text FFN on the text rows (Qformer.py:483-496) ----
        for (int c0 = 0; c0 < C; c0 += RB) {
            const int nb = C - c0 < RB ? C - c0 : RB;
            const long r0 = (long)c0 * Q * Hd;
            LinearCall fi{qin + r0, nb * Q, Hd, {&L.q_ffn_in}, 1, c.inter};
            fi.inv = true; fi.act = QF_ACT_GELU; fi.y = h->vinter.as<float>();
            if (int rc = run_linear(h, fi, stream)) return rc;
            LinearCall fo{h->vinter.as<float>(), nb * Q, c.inter, {&L.q_ffn_out}, 1, Hd};
            fo.inv = true; fo.residual = qin + r0; fo.res_rows = nb * Q; fo.ln = &L.q_ffn_ln; fo.y = vA + r0;
            if (fc && last && fc->out_dtype != INFV_TOKENS_F32) {   // the frame tokens leave in the type their consumer reads: no fp32 row is written
                fo.y16 = static_cast<char*>(fc->out) + 2 * r0; fo.y16_dtype = fc->out_dtype;
            }
            if (int rc = run_linear(h, fo, stream)) return rc;
        }
        if (text_out)
            for (long m0 = 0; m0 < Tt; m0 += TB) {
                const int m = (int)(Tt - m0 < TB ? Tt - m0 : TB);
                LinearCall fi{t1 + m0 * Hd, m, Hd, {&L.t_ffn_in}, 1, c.inter};
                fi.inv = true; fi.act = QF_ACT_GELU; fi.y = h->tinter.as<float>();
                if (int rc = run_linear(h, fi, stream)) return rc;
                LinearCall fo{h->tinter.as<float>(), m, c.inter, {&L.t_ffn_out}, 1, Hd};
                fo.inv = true; fo.residual = t1 + m0 * Hd; fo.res_rows = m; fo.ln = &L.t_ffn_ln; fo.y = tA + m0 * Hd;
                if (int rc = run_linear(h, fo, stream)) return rc;
            }
    }
    if (hidden_out) {
        HIP_TRY(launch_qf_copy_rows(vA, hidden_out, o_q.data(), q_dst.data(), q_n.data(), C, Hd, stream));
        if (Tt > 0) HIP_TRY(launch_qf_copy_rows(tA, hidden_out, o_t.data(), toff.data(), tl.data(), C, Hd, stream));
    }
    if (proj_out || proj_mean) {
        float* lo = proj_out;
        if (!lo) {                                             // only the mean is wanted: project into scratch
            const size_t need = (size_t)M * c.proj_out * sizeof(float);
            if (need > h->S.bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(h->S.reserve(need)); }
            lo = h->S.as<float>();
        }
        for (int c0 = 0; c0 < C; c0 += RB) {
            const int nb = C - c0 < RB ? C - c0 : RB;
            LinearCall pj{vA + (long)c0 * Q * Hd, nb * Q, Hd, {&w->mistral_proj}, 1, c.proj_out};
            pj.inv = true; pj.y = lo + (long)c0 * Q * c.proj_out;
            if (int rc = run_linear(h, pj, stream)) return rc;
        }
        if (proj_mean) HIP_TRY(launch_qf_mean_segments(lo, cu, V, (long)Q * c.proj_out, proj_mean, stream));
    }
    return INFV_OK;
}

int infv_vqf_vc_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                              int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len,
                              const double* u, int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean,
                              void* stream_) {
    return vc_impl("vc_encode_videos", h, ltm, V, cu, frames, -1, 0, nullptr, nullptr, T, w, hidden_in, text_len, u, new_video, hidden_out,
                   proj_out, proj_mean, stream_);
}

int infv_vqf_vc_encode_streams(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                               int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w,
                               const float* hidden_in, const int32_t* text_len, const double* u, int32_t new_video,
                               float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (!fcu || !frame_src) return fail(INFV_ERR_INVALID, "vc_encode_streams: bad arguments");
    return vc_impl("vc_encode_streams", h, ltm, V, cu, frames, -1, F, fcu, frame_src, T, w, hidden_in, text_len, u, new_video, hidden_out,
                   proj_out, proj_mean, stream_);
}

int infv_vqf_vc_encode_videos_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                  int32_t token_dtype, int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in,
                                  const int32_t* text_len, const double* u, int32_t new_video, float* hidden_out, float* proj_out,
                                  float* proj_mean, void* stream_) {
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_videos_tok: unknown token dtype %d", token_dtype);
    return vc_impl("vc_encode_videos_tok", h, ltm, V, cu, frames, token_dtype, 0, nullptr, nullptr, T, w, hidden_in, text_len, u, new_video,
                   hidden_out, proj_out, proj_mean, stream_);
}

int infv_vqf_vc_encode_streams_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                   int32_t token_dtype, int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T,
                                   const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len, const double* u,
                                   int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (!fcu || !frame_src) return fail(INFV_ERR_INVALID, "vc_encode_streams_tok: bad arguments");
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_streams_tok: unknown token dtype %d", token_dtype);
    return vc_impl("vc_encode_streams_tok", h, ltm, V, cu, frames, token_dtype, F, fcu, frame_src, T, w, hidden_in, text_len, u, new_video,
                   hidden_out, proj_out, proj_mean, stream_);
}

int infv_vqf_vc_encode_img(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames, int32_t token_dtype,
                           int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w,
                           const infv_vqf_vc_front* front, const float* hidden_in, const int32_t* text_len, const double* u, int32_t new_video,
                           float* hidden_out, float* proj_out, float* proj_mean, void* stream_) {
    if (token_dtype < 0) return fail(INFV_ERR_INVALID, "vc_encode_img: unknown token dtype %d", token_dtype);
    if (frame_src && !fcu) return fail(INFV_ERR_INVALID, "vc_encode_img: bad arguments");
    const bool streams = frame_src != nullptr;                 // NULL: videos (F and fcu are not read)
    return vc_impl("vc_encode_img", h, ltm, V, cu, frames, token_dtype, streams ? F : 0, streams ? fcu : nullptr, frame_src, T, w, hidden_in,
                   text_len, u, new_video, hidden_out, proj_out, proj_mean, stream_, front);
}

int infv_vqf_encode_frames(infv_vqf_handle h, int32_t F, const void* vision, int32_t token_dtype, int32_t n_tokens,
                           const infv_vqf_vc_weights* w, const infv_vqf_vision_ln* ln, const float* query_rows, void* out, int32_t out_dtype,
                           void* stream_) {
    // ---- what vc_impl does not see; everything else is refused there, before any launch or memory change ----
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
    const int rc = vc_impl(name, h, nullptr, F, cu.data(), vision, token_dtype, 0, nullptr, nullptr, 1, w, query_rows, text_len.data(), nullptr, 0,
                           out_dtype == INFV_TOKENS_F32 ? static_cast<float*>(out) : nullptr, nullptr, nullptr, stream_, &front, &fc);
    h->tap_layer = -1; h->tap_dst = nullptr;                  // a tap serves one call
    return rc;
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
    if ((size_t)n_rows * 2 * sizeof(float) > stats->bytes) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(stats->reserve((size_t)n_rows * 2 * sizeof(float))); }
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
