// C ABI of the video Q-former path (include/infv_vqf.h): the handle, its weight-plane caches, the steps the call paths share
// (vqf_handle.h; the paths: vqf_video.hip, vqf_vc.hip) and the stand-alone entry points.
#include "vqf_handle.h"
#include <algorithm>
#include <mutex>

#include <cstdlib>
#include <new>

namespace infv {

static int check_cfg(const infv_vqf_config& c) {
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

// Drops the cached weight planes (work in flight may still read them: the device is synchronised first)
static int drop_linear_planes(infv_vqf_s* h) {
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

bool split_path(const infv_vqf_s* h, int n_tokens) {
    static const bool want_fp32 = [] { const char* e = getenv("INFV_VQF_FP32"); return e && atoi(e) != 0; }();
    return !want_fp32 && !h->exact_fp32 && h->cfg.enc_width % 64 == 0 && n_tokens % 64 == 0;   // (odd frame counts: exact-fp32 kernels)
}

int fp32_tokens_unless_split(infv_vqf_s* h, const void*& frames, tok_code& tok, int n_tokens, size_t elems, hipStream_t stream) {
    if (tok == INFV_TOKENS_F32 || split_path(h, n_tokens)) return INFV_OK;
    HIP_TRY(reserve_all({{h->up, elems * sizeof(float)}}));
    HIP_TRY(launch_upcast(frames, tok, h->up.as<float>(), (long)elems, stream));
    frames = h->up.p; tok = INFV_TOKENS_F32;
    return INFV_OK;
}

int prepare_split(infv_vqf_s* h, const TokenPass& p, SplitRef* ref, hipStream_t stream) {
    const void* frames_ = p.frames; const tok_code tok = p.tok; const TokLn* ln = p.ln; float* kbar = p.kbar;
    const int nb = p.nb, n_tokens = p.n_tokens, dst0 = p.dst0, cap = p.cap, n_live = p.n_live; const bool whole = p.whole;
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

int short_attention(infv_vqf_s* h, const ShortAttn& a, hipStream_t stream) {
    const void* frames_ = a.frames; const tok_code tok = a.tok; const int nb = a.nb, n_tokens = a.n_tokens, inv_nb = a.inv_nb, n_live = a.n_live;
    const float* xq = a.xq; const float* along = a.along; float* merged = a.merged; const infv_linear* key = a.key; const infv_linear* value = a.value;
    const bool shared_q = a.shared_q, use_cache = a.use_cache, t_identity = a.t_identity;
    const SplitRef* pre = a.pre; const int32_t* b_map = a.b_map; const hipEvent_t along_ready = a.along_ready;
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
        else if (int rc = prepare_split(h, TokenPass{frames_, tok, nb, n_tokens}, &sr, stream)) return rc;
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
        QfGemm g{};                                           // S[b] = qt[b] . frames[b]^T
        g.A = qt; g.lda = d; g.strideA = shared_q ? 0 : (long)rows * d;
        g.B[0] = frames; g.ldb = d; g.strideB = (long)n_tokens * d; g.seg_rows = n_tokens;
        g.C = h->S.as<float>(); g.ldc = ldS; g.strideC = (long)rows * ldS; g.split_stride = 0;
        g.M = rows; g.N = n_tokens; g.k_per_split = d; g.splitk = 1; g.nbatch = nb; g.b_map = b_map;
        HIP_TRY(launch_qf_gemm(g, false, stream));
        HIP_TRY(launch_qf_softmax_rows(h->S.as<float>(), (long)nb * rows, n_tokens, ldS, stream));
        QfGemm p{};                                           // O[b] = P[b] . frames[b]
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
int query_self_block(infv_vqf_s* h, const BlockRows& r, const infv_vqf_layer& L, const float* x, bool whole, float* h1, float* xq) {
    const int Q = h->cfg.n_query, Hd = h->cfg.hidden, nb = r.rows / Q;
    const bool inv = r.inv; hipStream_t stream = r.stream;
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

int cross_output(infv_vqf_s* h, const BlockRows& r, const infv_linear* x_o, const infv_layernorm* ln, const float* x, const float* residual,
                 int res_rows, float* y) {
    const int Hd = h->cfg.hidden;
    LinearCall xo{x, r.rows, Hd, {x_o}, 1, Hd};
    xo.inv = r.inv; xo.reduced = r.reduced; xo.residual = residual; xo.res_rows = res_rows; xo.ln = ln; xo.y = y;
    return run_linear(h, xo, r.stream);
}

int ffn_rows(infv_vqf_s* h, const BlockRows& r, const FfnRef& f, const float* x, float* inter, float* y, void* y16, tok_code y16_dtype) {
    const int Hd = h->cfg.hidden, In = h->cfg.inter;
    LinearCall fi{x, r.rows, Hd, {f.in}, 1, In};
    fi.inv = r.inv; fi.reduced = r.reduced; fi.act = QF_ACT_GELU; fi.y = inter;
    if (int rc = run_linear(h, fi, r.stream)) return rc;
    LinearCall fo{inter, r.rows, In, {f.out}, 1, Hd};
    fo.inv = r.inv; fo.reduced = r.reduced; fo.residual = x; fo.res_rows = r.rows; fo.ln = f.ln; fo.y = y;
    fo.y16 = y16; fo.y16_dtype = y16_dtype;
    return run_linear(h, fo, r.stream);
}

// chunks per sub-batch of the short-term attention of a layer-major call over C chunks: the second contraction has few, long tiles
// per chunk (rows/128 x d/128 = 18 at the headline shape, K = T*P), so pick the count whose tile total fills whole rounds of the
// 256 CUs (16 chunks = 288 tiles ran at 56 % of 14 chunks' rate per tile)
int pick_short_nb(const infv_vqf_s* h, int C, int n_tokens) {
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

CallBlocks video_call_blocks(const infv_vqf_s* h, int C, int n_tokens, bool multi) {
    const int rb_max = multi ? kRowBlockVideos : kRowBlockVideo;   // (batch invariant: the row count does not shape the GEMMs)
    return CallBlocks{C < rb_max ? C : rb_max, pick_short_nb(h, C, n_tokens)};
}

CallBlocks vc_call_blocks(const infv_vqf_s* h, int C, int n_tokens) {
    const int RB = C < kRowBlockVideos ? C : kRowBlockVideos;
    return CallBlocks{RB, pick_short_nb(h, C, n_tokens)};
}

long text_ffn_block(long Tt) {
    const long TB = Tt < kTextFfnRows ? Tt : kTextFfnRows;
    return TB;
}

// u[:, l, :] of u [C][n_layers_in_u][S] -> contiguous [C][S] in h->vu, for the one-layer memory handles (u == nullptr: nothing)
int ltm_u_slice(infv_vqf_s* h, const double* u, int l, int n_layers_in_u, int C, hipStream_t stream) {
    if (!u) return INFV_OK;
    const size_t S = (size_t)h->cfg.nb_samples;
    HIP_TRY(hipMemcpy2DAsync(h->vu.p, S * sizeof(double), u + (size_t)l * S, (size_t)n_layers_in_u * S * sizeof(double), S * sizeof(double),
                             (size_t)C, hipMemcpyDeviceToDevice, stream));
    return INFV_OK;
}

// vmerged = alpha * vshort + (1 - alpha) * valong over the M rows of the whole call
int alpha_merge(infv_vqf_s* h, long M, hipStream_t stream) {
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
// mean (nullptr: none) = the mean of every video's chunks (videos.cu [V + 1]), or of all chunks (cu == nullptr).
int project_and_mean(infv_vqf_s* h, RowBlocks blocks, const infv_linear* proj, bool inv, float* out, float* mean, VideoSegs videos,
                     hipStream_t stream) {
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
    if (mean && videos.cu) HIP_TRY(launch_qf_mean_segments(out, videos.cu, videos.V, row, mean, stream));
    else if (mean) HIP_TRY(launch_qf_mean(out, blocks.C, row, mean, stream));
    return INFV_OK;
}

}  // namespace infv

using namespace infv;

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
    ShortAttn a{frames, tok, 1, n_tokens, xq, false, key, value};
    a.along = a_long; a.merged = merged;
    return short_attention(h, a, static_cast<hipStream_t>(stream));
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
