// The video Q-former calls of include/infv_vqf.h: the per-chunk infv_vqf_encode_chunk, and the layer-major infv_vqf_encode_video /
// infv_vqf_encode_videos -- encode_impl, a short driver over stages that read one call descriptor (EncCall).
#include "vqf_handle.h"
#include <algorithm>
#include <cstdlib>

using namespace infv;

static int check_layer_cfg(const infv_vqf_config& c) {       // what the fused per-layer kernels of encode_chunk / encode_video are built for
    if (c.n_query > 32) return fail(INFV_ERR_UNSUPPORTED, "encode_chunk / encode_video need n_query <= 32 (this handle: %d)", c.n_query);
    if (c.tokens_per_frame % 32) return fail(INFV_ERR_UNSUPPORTED, "encode_chunk / encode_video need tokens_per_frame %% 32 == 0");
    return INFV_OK;
}

static infv_ltm_proj cross_proj(const infv_vqf_layer& L) {   // the key / value projections a layer's memory shares with its cross-attention
    infv_ltm_proj pr{};
    pr.wk = L.x_k.w; pr.bk = L.x_k.b; pr.wv = L.x_v.w; pr.bv = L.x_v.b;
    return pr;
}

// One call of infv_vqf_encode_video (one video, ltm [n_layers]) or infv_vqf_encode_videos (packed: V videos packed by the host array
// cu, ltm [V][n_layers]; every choice that shapes a GEMM or contraction is taken from per-chunk quantities or constants, and each
// layer's memories step through infv_ltm_steps_videos).  The entry points fill the arguments by name; enc_validate adds what it
// decides from them, the token pass what it leaves for the layers.
struct EncCall {
    // ---- arguments
    const char* name = nullptr;                                // names the call in the refusals
    const infv_ltm_handle* ltm = nullptr;
    int32_t V = 1; const int32_t* cu = nullptr;
    const void* frames = nullptr;                              // (fp32_tokens_unless_split may replace frames and tok by an fp32 copy)
    int32_t n_chunks = 0, T = 0;
    const infv_vqf_weights* w = nullptr;
    const double* u = nullptr;
    int32_t new_video = 0;
    float* hidden_out = nullptr; float* llama_out = nullptr; float* llama_mean = nullptr;
    hipStream_t stream = nullptr;
    bool packed = false;                                       // packed videos (encode_videos), else one video (encode_video)
    // ---- decided by enc_validate
    tok_code tok = INFV_TOKENS_F32;
    bool use_ltm = false;
    bool inv = false; int inv_nb = 0;                          // batch invariant: the row count does not shape the GEMMs; short_attention's inv_nb
    bool pool_first = false;                                   // the frame means every layer's memories step from are pooled up front
    int C = 0;                                                 // chunks (0 after validation: the call is complete)
    long M = 0;                                                // rows of the whole-call activations
    int n_tokens = 0; long chunk_k = 0;                        // tokens and elements of a chunk
    int RB = 0, NB = 0;                                        // chunks per row block of the query-token GEMMs, per sub-batch of the short-term attention
    // ---- left by enc_token_pass
    SplitRef wref{}; bool have_w = false, have_kbar = false;   // the planes of all C chunks, kept for the call; the frame means came with them
    std::vector<infv_ltm_handle> hs_l;                         // scratch of the memory steps: layer l's handles of every video [V]
};

// ---- validation before any device work or memory change.  Returns with k.C == 0 where nothing is left to do.
static int enc_validate(const infv_vqf_s* h, EncCall& k) {
    if (k.packed) {
        if (!h || !k.cu || !k.w || k.V < 0) return fail(INFV_ERR_INVALID, "encode_videos: bad arguments");
        if (k.V == 0) return INFV_OK;
        if (int rc = check_offsets(k.name, "cu", k.cu, k.V)) return rc;
        if (int rc = refuse_reduced(h, k.name)) return rc;      // (the first read of the handle)
        k.use_ltm = h->cfg.alpha != 1.0f;
        const int n_h = k.use_ltm ? k.V * h->cfg.n_layers : 0;
        if (k.use_ltm) {
            if (!k.ltm) return fail(INFV_ERR_INVALID, "encode_videos: alpha != 1 needs the per-layer LTM handles of every video");
            if (int rc = check_distinct_handles(k.name, k.ltm, n_h, "layer")) return rc;
        }
        if (k.cu[k.V] == 0) {                                  // no chunk: new_video still starts every memory afresh
            if (k.use_ltm && k.new_video)
                for (int i = 0; i < n_h; ++i) infv_ltm_reset(k.ltm[i]);
            return INFV_OK;
        }
        if (!k.frames) return fail(INFV_ERR_INVALID, "encode_videos: null frames");
        k.n_chunks = k.cu[k.V];
    } else {
        if (!h || !k.frames || !k.w || k.n_chunks < 1) return fail(INFV_ERR_INVALID, "bad argument");
        if (int rc = refuse_reduced(h, k.name)) return rc;
    }
    const infv_vqf_config& c = h->cfg;
    if (int rc = check_layer_cfg(c)) return rc;
    k.use_ltm = c.alpha != 1.0f;
    if (k.use_ltm && !k.ltm) return fail(INFV_ERR_INVALID, "alpha != 1 needs the per-layer LTM handles");
    if (k.T < 1) return fail(INFV_ERR_INVALID, "T must be >= 1");
    if ((k.llama_out || k.llama_mean) && (c.proj_out <= 0 || !k.w->llama_proj.w)) return fail(INFV_ERR_INVALID, "llama output without llama_proj");
    k.tok = h->tok;
    if (k.tok != INFV_TOKENS_F32 && !aligned16(k.frames)) return fail(INFV_ERR_INVALID, "fp16 / bf16 / fp8 frames must be 16-byte aligned");
    // ---- what the stages read
    k.inv = k.packed; k.inv_nb = k.packed ? kInvariantNb : 0; k.pool_first = k.packed && k.use_ltm;
    k.C = k.n_chunks;
    k.M = (long)k.C * c.n_query;
    k.n_tokens = k.T * c.tokens_per_frame;
    k.chunk_k = (long)k.n_tokens * c.enc_width;
    const CallBlocks blocks = video_call_blocks(h, k.C, k.n_tokens, k.packed);
    k.RB = blocks.RB; k.NB = blocks.NB;
    return INFV_OK;
}

// whole-call activations + per-block scratch
static int enc_workspaces(infv_vqf_s* h, const EncCall& k) {
    const infv_vqf_config& c = h->cfg;
    const size_t act = (size_t)k.M * c.hidden * sizeof(float), row = (size_t)c.n_query * c.hidden * sizeof(float), f = sizeof(float);
    const bool use_ltm = k.use_ltm;
    HIP_TRY(reserve_all({{h->vA, act}, {h->v1, act}, {h->v2, act}, {h->vxq, act}, {h->vshort, act}, {h->vmerged, act},
                         {h->valong, use_ltm ? act : 0}, {h->vu, use_ltm ? (size_t)k.C * c.nb_samples * sizeof(double) : 0},
                         {h->vkbar, use_ltm ? (size_t)k.C * k.T * c.enc_width * f : 0}, {h->vqkv, (size_t)k.RB * 3 * row},
                         {h->vsa, (size_t)k.RB * row}, {h->vinter, (size_t)k.RB * c.n_query * c.inter * f}, {h->v_h1s, row}, {h->v_xqs, row}}));
    return INFV_OK;
}

// ONE pass over the whole call's frame tokens: split-bf16 operands of every layer's short-term attention and the frame means of
// every layer's memory.  The copies take 2 x the tokens' bytes (12.7 GB for the headline's 252 chunks): kept for the call when
// they fit INFV_VQF_SPLIT_CACHE_GB (default 64 of the 288 GB).  Packed videos without means from the pass: pooled here, up front.
static int enc_token_pass(infv_vqf_s* h, EncCall& k) {
    const infv_vqf_config& c = h->cfg;
    const double need_gb = plane_bytes(k.tok, false) * (double)k.C * (double)k.chunk_k / 1e9;
    if (h->fuse && split_path(h, k.n_tokens) && need_gb <= h->split_cache_gb) {
        k.have_kbar = k.use_ltm && 64 % c.tokens_per_frame == 0;
        TokenPass p{k.frames, k.tok, k.C, k.n_tokens, k.have_kbar ? h->vkbar.as<float>() : nullptr, true};
        if (int rc = prepare_split(h, p, &k.wref, k.stream)) return rc;
        k.have_w = true;
    }
    if (k.pool_first && !k.have_kbar) {
        if (int rc = infv_ltm_set_token_dtype(k.ltm[0], k.tok)) return rc;
        if (int rc = infv_ltm_pool(k.ltm[0], k.frames, (int64_t)k.C * k.T, h->vkbar.as<float>(), k.stream)) return rc;
    }
    k.hs_l = std::vector<infv_ltm_handle>(k.pool_first ? k.V : 0);
    return INFV_OK;
}

// Layer l's memory step with the constant query of layer 0: all chunks at once, on the caller's stream -> valong
static int enc_memory_shared_query(infv_vqf_s* h, EncCall& k, int l, const infv_ltm_proj& pr) {
    const infv_vqf_config& c = h->cfg;
    if (int rc = ltm_u_slice(h, k.u, l, c.n_layers, k.C, k.stream)) return rc;
    const double* u = k.u ? h->vu.as<double>() : nullptr;
    float* kbar = h->vkbar.as<float>(); float* xq = h->v_xqs.as<float>(); float* valong = h->valong.as<float>();
    if (k.packed) {                                            // every video's memory with the shared query, in lockstep
        for (int v = 0; v < k.V; ++v) k.hs_l[v] = k.ltm[(size_t)v * c.n_layers + l];
        return infv_ltm_steps_videos(k.hs_l.data(), k.V, k.cu, kbar, k.T, xq, 0, c.n_query, &pr, u, k.new_video, valong, k.stream);
    }
    if (k.have_kbar)                                           // the whole-video fast path
        return infv_ltm_consolidate_pooled(k.ltm[l], kbar, k.C, k.T, xq, c.n_query, &pr, u, k.new_video, valong, k.stream);
    if (int rc = infv_ltm_set_token_dtype(k.ltm[l], k.tok)) return rc;
    return infv_ltm_consolidate(k.ltm[l], k.frames, k.C, k.T, xq, c.n_query, &pr, u, k.new_video, valong, k.stream);
}

// Layer l's memory step with per-chunk queries: the sequential chain, on the worker stream between ev_main and ev_side, while the
// caller's stream runs the layer's short-term attention -> valong
static int enc_memory_chunk_queries(infv_vqf_s* h, EncCall& k, int l, const infv_ltm_proj& pr) {
    const infv_vqf_config& c = h->cfg;
    if (int rc = ltm_u_slice(h, k.u, l, c.n_layers, k.C, k.stream)) return rc;
    const double* u = k.u ? h->vu.as<double>() : nullptr;
    float* kbar = h->vkbar.as<float>(); float* vxq = h->vxq.as<float>(); float* valong = h->valong.as<float>();
    HIP_TRY(hipEventRecord(h->ev_main, k.stream));
    HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
    if (k.packed) {                                            // every video's memory with its chunks' queries, in lockstep
        for (int v = 0; v < k.V; ++v) k.hs_l[v] = k.ltm[(size_t)v * c.n_layers + l];
        if (int rc = infv_ltm_steps_videos(k.hs_l.data(), k.V, k.cu, kbar, k.T, vxq, 1, c.n_query, &pr, u, k.new_video, valong, h->side)) return rc;
    } else {
        if (k.new_video)
            if (int rc = infv_ltm_reset(k.ltm[l])) return rc;
        if (!k.have_kbar) {
            if (int rc = infv_ltm_set_token_dtype(k.ltm[l], k.tok)) return rc;
            if (int rc = infv_ltm_pool(k.ltm[l], k.frames, (int64_t)k.C * k.T, kbar, h->side)) return rc;
        }
        // new-row projections of all chunks in one GEMM, then the chain chunk by chunk
        if (int rc = infv_ltm_steps(k.ltm[l], kbar, k.C, k.T, vxq, c.n_query, &pr, u, valong, h->side)) return rc;
    }
    HIP_TRY(hipEventRecord(h->ev_side, h->side));
    return INFV_OK;
}

// The short-term attention of every chunk, in sub-batches: xq (shared: one block for all) -> out, merged with `along` (nullptr: none)
// in the epilogue.  The cached split of chunks c0.. where the token pass kept it, else split per sub-batch.
static int enc_short_attention(infv_vqf_s* h, const EncCall& k, const infv_vqf_layer& L, const float* xq, bool shared, const float* along,
                               float* out) {
    for (RowBlock b : RowBlocks{k.C, k.NB, (long)h->cfg.n_query * h->cfg.hidden}) {
        const SplitRef sr = split_ref_at(k.wref, b.c0, k.chunk_k);
        ShortAttn a{tok_at(k.frames, k.tok, b.c0 * k.chunk_k), k.tok, b.nb, k.n_tokens, shared ? xq : xq + b.r0, shared, &L.x_k, &L.x_v};
        a.along = along ? along + b.r0 : nullptr; a.merged = out + b.r0;
        a.pre = k.have_w ? &sr : nullptr; a.inv_nb = k.inv_nb;
        if (int rc = short_attention(h, a, k.stream)) return rc;
    }
    return INFV_OK;
}

// Layer 0: the hidden states entering it do not depend on the chunk -- self-attention block + cross query once, the whole-call
// memory step, the short-term attention with the merge in its epilogue
static int enc_layer0(infv_vqf_s* h, EncCall& k) {
    const infv_vqf_layer& L = k.w->layer[0];
    float* xqs = h->v_xqs.as<float>();
    const BlockRows one{h->cfg.n_query, k.inv, false, k.stream};
    if (int rc = query_self_block(h, one, L, h->h_a.as<float>(), false, h->v_h1s.as<float>(), xqs)) return rc;
    if (k.use_ltm)
        if (int rc = enc_memory_shared_query(h, k, 0, cross_proj(L))) return rc;
    return enc_short_attention(h, k, L, xqs, true, k.use_ltm ? h->valong.as<float>() : nullptr, h->vmerged.as<float>());
}

// Layer l > 0: self-attention block + cross query of every chunk (row blocks), the memory step on the worker stream beside the
// short-term attention, alpha_merge of the two
static int enc_later_layer(infv_vqf_s* h, EncCall& k, int l) {
    const infv_vqf_layer& L = k.w->layer[l];
    float* vA = h->vA.as<float>(); float* v1 = h->v1.as<float>(); float* vxq = h->vxq.as<float>();
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)h->cfg.n_query * h->cfg.hidden})
        if (int rc = query_self_block(h, BlockRows{b.nb * h->cfg.n_query, k.inv, false, k.stream}, L, vA + b.r0, true, v1 + b.r0, vxq + b.r0)) return rc;
    if (k.use_ltm)
        if (int rc = enc_memory_chunk_queries(h, k, l, cross_proj(L))) return rc;
    if (int rc = enc_short_attention(h, k, L, vxq, false, nullptr, (k.use_ltm ? h->vshort : h->vmerged).as<float>())) return rc;
    if (!k.use_ltm) return INFV_OK;
    HIP_TRY(hipStreamWaitEvent(k.stream, h->ev_side, 0));
    return alpha_merge(h, k.M, k.stream);
}

// The tail of layer l: cross output + query FFN of every chunk, row block by row block (the residual of layer 0 is one shared block)
static int enc_layer_tail(infv_vqf_s* h, const EncCall& k, int l) {
    const infv_vqf_config& c = h->cfg;
    const infv_vqf_layer& L = k.w->layer[l];
    const int Q = c.n_query;
    float* vA = h->vA.as<float>(); float* v2 = h->v2.as<float>(); const float* vmerged = h->vmerged.as<float>();
    for (RowBlock b : RowBlocks{k.C, k.RB, (long)Q * c.hidden}) {
        const BlockRows r{b.nb * Q, k.inv, false, k.stream};
        const float* res = l == 0 ? h->v_h1s.as<float>() : h->v1.as<float>() + b.r0;
        if (int rc = cross_output(h, r, &L.x_o, &L.x_ln, vmerged + b.r0, res, l == 0 ? Q : r.rows, v2 + b.r0)) return rc;
        if (int rc = ffn_rows(h, r, FfnRef{&L.ffn_in, &L.ffn_out, &L.ffn_ln}, v2 + b.r0, h->vinter.as<float>(), vA + b.r0)) return rc;
    }
    return INFV_OK;
}

static int enc_outputs(infv_vqf_s* h, const EncCall& k) {
    const infv_vqf_config& c = h->cfg;
    if (k.hidden_out)
        HIP_TRY(hipMemcpyAsync(k.hidden_out, h->vA.p, (size_t)k.M * c.hidden * sizeof(float), hipMemcpyDeviceToDevice, k.stream));
    if (!k.llama_out && !k.llama_mean) return INFV_OK;
    return project_and_mean(h, RowBlocks{k.C, k.RB, (long)c.n_query * c.hidden}, &k.w->llama_proj, k.inv, k.llama_out, k.llama_mean,
                            VideoSegs{k.cu, k.V}, k.stream);
}

// The layer-major body of infv_vqf_encode_video and infv_vqf_encode_videos: the stages above, in call order
static int encode_impl(infv_vqf_handle h, EncCall& k) {
    if (int rc = enc_validate(h, k)) return rc;
    if (k.C == 0) return INFV_OK;                              // no video or no chunk
    if (int rc = ensure_streams(h)) return rc;
    if (int rc = fp32_tokens_unless_split(h, k.frames, k.tok, k.n_tokens, (size_t)k.C * k.chunk_k, k.stream)) return rc;
    if (int rc = enc_workspaces(h, k)) return rc;
    if (int rc = enc_token_pass(h, k)) return rc;
    if (int rc = embed_query_tokens(h, k.w, k.stream)) return rc;
    for (int l = 0; l < h->cfg.n_layers; ++l) {
        if (int rc = l == 0 ? enc_layer0(h, k) : enc_later_layer(h, k, l)) return rc;
        if (int rc = enc_layer_tail(h, k, l)) return rc;
    }
    return enc_outputs(h, k);
}

extern "C" {

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
        const TokenPass p{frames, tok, 1, n_tokens, use_ltm && fused_pool ? h->kbar.as<float>() : nullptr};
        if (int rc = prepare_split(h, p, &sref, stream)) return rc;
        pre = &sref;
    }
    if (use_ltm && !fused_pool) {
        // (the LTM handle's token dtype is sticky state an earlier caller may have set)
        if (int rc = infv_ltm_set_token_dtype(ltm[0], tok)) return rc;
        if (int rc = infv_ltm_pool(ltm[0], frames, T, h->kbar.as<float>(), stream_)) return rc;   // shared by all layers
    }

    const BlockRows one{Q, false, false, stream};
    for (int l = 0; l < c.n_layers; ++l) {
        const infv_vqf_layer& L = w->layer[l];
        const bool l0c = caching && l == 0;                   // this layer's prefix lives in the cache buffers
        float* h1 = l0c ? h->c_h1.as<float>() : h->h1.as<float>();
        float* xqb = l0c ? h->c_xq.as<float>() : h->xq.as<float>();
        if (!(l0c && prefix_cached)) {
            if (int rc = query_self_block(h, one, L, hcur, false, h1, xqb)) return rc;
            if (l0c) { h->c_valid = true; h->c_epoch = h->epoch; }
        }
        ShortAttn a{frames, tok, 1, n_tokens, xqb, false, &L.x_k, &L.x_v};
        a.merged = h->merged.as<float>(); a.use_cache = l0c; a.pre = pre;
        if (use_ltm) {
            // The memory step and the short-term attention both start from the cross query and meet only in the merge
            // (Qformer.py:216-223 vs :225-302, :303-304): the step's three launches go to the shared worker stream and run
            // beside the attention's contractions; the merge epilogue waits for them.
            const infv_ltm_proj pr = cross_proj(L);
            const double* ul = u ? u + (size_t)l * c.nb_samples : nullptr;
            HIP_TRY(hipEventRecord(h->ev_main, stream));              // cross query, pooled frames, the previous layer's merge
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_main, 0));
            if (int rc = infv_ltm_step(ltm[l], h->kbar.as<float>(), T, xqb, Q, &pr, ul,
                                       h->along.as<float>(), h->side)) return rc;
            HIP_TRY(hipEventRecord(h->ev_side, h->side));
            a.along = h->along.as<float>();
            a.along_ready = h->ev_side;
        }
        if (int rc = short_attention(h, a, stream)) return rc;
        if (int rc = cross_output(h, one, &L.x_o, &L.x_ln, h->merged.as<float>(), h1, Q, h->h2.as<float>())) return rc;
        if (int rc = ffn_rows(h, one, FfnRef{&L.ffn_in, &L.ffn_out, &L.ffn_ln}, h->h2.as<float>(), h->inter.as<float>(), hnext)) return rc;
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

int infv_vqf_encode_video(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t n_chunks,
                          int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, float* llama_mean, void* stream_) {
    EncCall k;
    k.name = "encode_video"; k.ltm = ltm; k.frames = frames; k.n_chunks = n_chunks; k.T = T; k.w = w; k.u = u; k.new_video = new_video;
    k.hidden_out = hidden_out; k.llama_out = llama_out; k.llama_mean = llama_mean; k.stream = static_cast<hipStream_t>(stream_);
    return encode_impl(h, k);
}

int infv_vqf_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                           int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video, float* hidden_out,
                           float* llama_out, float* llama_mean, void* stream_) {
    EncCall k;
    k.name = "encode_videos"; k.packed = true; k.ltm = ltm; k.V = V; k.cu = cu; k.frames = frames; k.T = T; k.w = w; k.u = u;
    k.new_video = new_video; k.hidden_out = hidden_out; k.llama_out = llama_out; k.llama_mean = llama_mean;
    k.stream = static_cast<hipStream_t>(stream_);
    return encode_impl(h, k);
}

}  // extern "C"
