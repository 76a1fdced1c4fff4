// The VideoChat2 / frame calls of include/infv_vqf.h: vc_impl, a short driver over stages that read one call descriptor (VcCall), its
// six entry points, infv_vqf_encode_frames and infv_vqf_frame_cross_attention.
#include "vqf_handle.h"
#include <algorithm>

using namespace infv;

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
    const CallBlocks blocks = vc_call_blocks(h, C, k.n_tokens);
    k.RB = blocks.RB; k.NB = blocks.NB;
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
    k.TB = text_ffn_block(Tt);
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
        TokenPass p{k.frames, k.tok, k.Cf, k.n_tokens, k.have_kbar ? kbar : nullptr, true};
        p.ln = k.ln; p.n_live = k.pad ? k.n_live : 0;
        if (int rc = prepare_split(h, p, &k.wref, k.stream)) return rc;
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
            TokenPass p{op.frames, k.tok, nb, k.n_tokens};
            p.ln = ln ? &lc : nullptr; p.n_live = k.pad ? k.n_live : 0;
            op.rc = prepare_split(h, p, &op.pre, k.stream);
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
        TokenPass p{tok_at(k.frames, k.tok, (long)src[b0] * k.chunk_k), k.tok, b1 - b0, k.n_tokens};
        p.dst0 = b0; p.cap = nb; p.ln = ln ? &lc : nullptr;
        op.rc = prepare_split(h, p, &op.pre, k.stream);
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
        ShortAttn a{op.frames, k.tok, b.nb, k.n_tokens, xq + b.r0, false, key, value};
        a.merged = out + b.r0; a.pre = op.has_pre ? &op.pre : nullptr; a.inv_nb = kInvariantNb;
        a.b_map = op.map; a.t_identity = op.t_identity; a.n_live = k.pad ? k.n_live : 0;
        if (int rc = short_attention(h, a, k.stream)) return rc;
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
        const BlockRows r{b.nb * Q, true, k.fc != nullptr, k.stream};
        if (int rc = cross_output(h, r, &L.x_o, &L.x_ln, vmerged + b.r0, h->v1.as<float>() + b.r0, r.rows, h->v2.as<float>() + b.r0)) return rc;
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
    // the frame tokens leave in the type their consumer reads: no fp32 row is written
    const bool out16 = k.fc && last && k.fc->out_dtype != INFV_TOKENS_F32;
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)Q * Hd}) {
        const BlockRows r{b.nb * Q, true, k.fc != nullptr, k.stream};
        if (int rc = ffn_rows(h, r, FfnRef{&L.q_ffn_in, &L.q_ffn_out, &L.q_ffn_ln}, qin + b.r0, h->vinter.as<float>(), h->vA.as<float>() + b.r0,
                              out16 ? static_cast<char*>(k.fc->out) + 2 * b.r0 : nullptr, out16 ? k.fc->out_dtype : INFV_TOKENS_F32)) return rc;
    }
    if (!(k.Tt > 0 && (!last || k.hidden_out))) return INFV_OK;   // the last layer's text rows feed nothing but hidden_out
    float* tA = h->tA.as<float>(); float* t1 = h->t1.as<float>();
    const long Tt = k.Tt, TB = k.TB;
    for (long m0 = 0; m0 < Tt; m0 += TB) {
        const BlockRows r{(int)(Tt - m0 < TB ? Tt - m0 : TB), true, false, k.stream};
        if (int rc = ffn_rows(h, r, FfnRef{&L.t_ffn_in, &L.t_ffn_out, &L.t_ffn_ln}, t1 + m0 * Hd, h->tinter.as<float>(), tA + m0 * Hd)) return rc;
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
        return project_and_mean(h, RowBlocks{k.C, k.RB, (long)h->cfg.n_query * Hd}, &k.w->mistral_proj, true, k.proj_out, k.proj_mean,
                                VideoSegs{k.cu, k.V}, k.stream);
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

extern "C" {

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

}  // extern "C"
