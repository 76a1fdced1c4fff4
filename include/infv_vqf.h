/* infv_vqf.h -- C ABI of the video Q-former path around the LTM (libinfv_ltm.so), MI355X / gfx950.
 *
 * The reference has no FFI for this path either: the boundary is Python (`video_Qformer.bert(...)` called by
 * `encode_video`, infty-Video-LLaMA/InfVideoLLaMA/models/infinityqa.py:280-344).  These entry points are what the
 * Python mirror (infinite_video_amd/video_qformer.py) binds with ctypes.  Plain pointers and sizes only; all
 * pointers are DEVICE pointers (fp32, row-major) unless stated; every call is asynchronous on `stream`.  Only the frame tokens
 * (`frames`) may be fp16, bf16 or fp8 e4m3 instead (infv_vqf_set_token_dtype).
 * `stream` may be a non-blocking side stream, under the contract of infv_ltm.h (Conventions): inputs are read behind the work queued
 * on `stream` before the call, and inputs, outputs and the memories belong to `stream` again when the call returns -- the layer-major
 * calls run the later layers' memories on the library's shared worker stream behind an event of `stream` and join it before the
 * merge.  Host waits beside workspace growth: infv_vqf_vc_embed and infv_vqf_vc_encode_img stage the instruction ids through one
 * pinned buffer per handle and wait for the previous call's copy out of it before rewriting it; under a reduced linear or
 * attention precision the first call of a NEW weights epoch drops the cached weight planes (device synchronisation) and
 * allocates the new ones, later calls of that epoch reuse them without a host wait; infv_vqf_layernorm_tokens keeps its row
 * statistics in one process-wide buffer and orders calls on different streams with an event (no host wait, but such calls
 * serialise); infv_vqf_destroy synchronises the device.  Not promised: one handle on two streams without the caller ordering them.
 * Errors: int status as in infv_ltm.h, message via infv_ltm_last_error().
 *
 * Scope: the query-token-only, eval-mode, all-ones-mask case the video Q-former is run in
 * (Qformer.py:197-312 BertSelfAttention, :322-326 BertSelfOutput, :442-522 BertLayer with the query FFN,
 * :85-112 BertEmbeddings on query_embeds), head size 64, <= 32 query tokens, tokens_per_frame a multiple of 32.
 */
#ifndef INFV_VQF_H
#define INFV_VQF_H

#include "infv_ltm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INFV_VQF_MAX_LAYERS 8

typedef struct infv_vqf_s* infv_vqf_handle;

typedef struct {
    int32_t n_layers;          /* BertConfig.num_hidden_layers of the video Q-former (infinityqa.py:38: 2) */
    int32_t n_heads;           /* 12 */
    int32_t hidden;            /* 768 = n_heads * 64 */
    int32_t inter;             /* 3072, intermediate_query width */
    int32_t enc_width;         /* width of the frame tokens (encoder_width, infinityqa.py:39) */
    int32_t tokens_per_frame;  /* 32 */
    int32_t n_query;           /* video query tokens (32) */
    int32_t proj_out;          /* llama_proj output width (4096); 0 = no projection */
    int32_t nb_samples;        /* S = 512: stride of the per-layer Gibbs uniforms in `u` */
    float   alpha;             /* merge weight of the short-term context (Qformer.py:129,304) */
    float   ln_eps;            /* BertConfig.layer_norm_eps = 1e-12 */
} infv_vqf_config;

typedef struct { const float* w; const float* b; } infv_linear;          /* nn.Linear: w [out][in], b [out] */
typedef struct { const float* gamma; const float* beta; } infv_layernorm;

/* One BertLayer of the video Q-former (Qformer.py:420-441; the text FFN is removed, infinityqa.py:206-208). */
typedef struct {
    infv_linear self_q, self_k, self_v, self_o;   infv_layernorm self_ln;   /* layer.attention            */
    infv_linear x_q, x_k, x_v, x_o;               infv_layernorm x_ln;      /* layer.crossattention       */
    infv_linear ffn_in, ffn_out;                  infv_layernorm ffn_ln;    /* intermediate_query / output_query */
} infv_vqf_layer;

typedef struct {
    const float*   query_tokens;                  /* video_query_tokens [n_query][hidden] (infinityqa.py:52-55) */
    infv_layernorm emb_ln;                        /* bert.embeddings.LayerNorm */
    infv_vqf_layer layer[INFV_VQF_MAX_LAYERS];
    infv_linear    llama_proj;                    /* infinityqa.py:342 */
} infv_vqf_weights;

int infv_vqf_create(const infv_vqf_config* cfg, infv_vqf_handle* out);
int infv_vqf_destroy(infv_vqf_handle h);

/* Arithmetic of the two big contractions of the short-term attention ([H*Q x d x T*P] each):
 *   0 (default)  split-bf16: every fp32 operand as hi + lo bf16, three bf16 MFMA products, fp32 accumulation
 *                (error ~1e-5 relative, inside the path's 1e-3 budget, ~2.5x faster);
 *   1            exact fp32 MFMA (bitwise an fp32 fma chain). */
int infv_vqf_set_precision(infv_vqf_handle h, int32_t exact_fp32);

/* Element type of every `frames` argument below: an infv_token_dtype (infv_ltm.h), default INFV_TOKENS_F32; anything else is
 * refused with INFV_ERR_INVALID and the handle keeps its setting.  An fp16 or bf16 `frames` pointer must be 16-byte aligned
 * (refused otherwise, before any device work).  With fp16 tokens (INFV_TOKENS_F16, what the reference's fp16 producer holds)
 * one pass reads the caller's buffer at 2 bytes per element and writes the hi / lo planes, their transposed copies and the
 * frame means -- an fp16 value is exactly hi + lo (11 = 8 + 3 significand bits), so planes, means and every result are bit for
 * bit those of the same values passed as fp32, and the contractions are the three-product ones.  With bf16 tokens the split-bf16 contractions read the caller's buffer in place (a bf16
 * token is its own hi plane and its lo plane is exactly zero): one pass writes the transposed copy and the frame means, and
 * both contractions run two bf16 MFMA products instead of three.  Results are bit for bit those of the same values passed as
 * fp32.  Where the split path does not apply (exact fp32, token counts that are no multiple of 64) the tokens are copied to
 * fp32 in a workspace of the handle first (fp16 and bf16 alike).  Every shape accepted with fp32 tokens is accepted with
 * fp16 and with bf16 tokens.
 * Code 4 = INFV_TOKENS_F8E4M3 (OCP e4m3fn at 1 byte per element, 16-byte aligned; infv_ltm.h) is accepted too: fp8 is the caller's
 * storage choice and the contract is equality with the run on the tokens widened to fp32.  An e4m3 value is exactly its own bf16
 * hi piece, so the token pass writes the two hi planes and no lo planes, both contractions run the two-product form as for bf16
 * tokens, and the plane cache counts 4 bytes per element (2 for bf16, 8 for fp32 / fp16); off the split path the tokens are
 * widened to fp32 in a workspace of the handle first. */
int infv_vqf_set_token_dtype(infv_vqf_handle h, int32_t dtype);

/* Layer 0's hidden states entering the cross-attention come from the learned query tokens and the weights only, so
 * infv_vqf_encode_chunk can reuse them (embedding LayerNorm, self-attention block, cross query, pre-multiplied query)
 * from one chunk to the next.  The host vouches for the weights with an epoch: while the same non-zero epoch is set,
 * the cached prefix is reused; change it whenever any weight of that prefix changes; 0 (default) disables reuse. */
int infv_vqf_set_weights_epoch(infv_vqf_handle h, uint64_t epoch);

/* Short-term cross-attention of one layer over one chunk's frame tokens, merged with the long-term context:
 *   merged = alpha * softmax((xq W-free restatement, see vqf_kernels.hip)) ... = Qformer.py:232-304 for a cross layer.
 * frames [n_tokens][enc_width], xq [n_query][hidden] (= self.query(hidden_states), bias applied),
 * a_long [n_query][hidden] or NULL (then merged = short-term context, the alpha == 1.0 / image-Q-former case). */
int infv_vqf_short_attention(infv_vqf_handle h, const void* frames, int32_t n_tokens, const float* xq,
                             const infv_linear* key, const infv_linear* value, const float* a_long,
                             float* merged, void* stream);

/* One chunk through the whole video Q-former + llama_proj (the device side of encode_video, infinityqa.py:325-343):
 *   ltm[l]      LTM handle of cross-attention layer l (n_layers = 1 each, plan for T set); ignored if alpha == 1
 *   frames      [T * tokens_per_frame][enc_width]
 *   u           [n_layers][nb_samples] float64 Gibbs uniforms (device) or NULL (first chunk / non-sticky / alpha == 1)
 *   new_video   resets the memories first (Qformer.py:221 new_doc=new_video)
 *   hidden_out  [n_query][hidden]    last_hidden_state        (may be NULL)
 *   llama_out   [n_query][proj_out]  llama_proj(last_hidden)  (may be NULL)
 * The chunk's frame tokens are read ONCE: one pass yields the split-bf16 operands of every layer's short-term attention
 * (Qformer.py:278-291) and the frame means every layer's memory pools (long_term_attention_gibbs.py:304). */
int infv_vqf_encode_chunk(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t T,
                          const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, void* stream);

/* A whole video (n_chunks chunks of T frames each) through the video Q-former, layer-major:
 *   - layer 0's hidden states do not depend on the chunk (they come from the learned query tokens only), so its LTM
 *     runs as ONE infv_ltm_consolidate over all chunks (constant query) and its short-term attention shares one
 *     pre-multiplied query block;
 *   - later layers have per-chunk queries: their LTM is the sequential per-call chain, issued on an internal side
 *     stream while the caller's stream runs the layer's short-term attention for all chunks;
 *   - every query-token block (linear / LayerNorm / GELU / self-attention) is batched over chunks;
 *   - the frame tokens of the whole video are read once: their split-bf16 copies (2 x the tokens' bytes; bf16 tokens: the
 *     transposed copy only, 1 x) are kept for the call when they fit INFV_VQF_SPLIT_CACHE_GB (default 64), and layer 0's memory runs from the frame means of that pass
 *     (infv_ltm_consolidate_pooled).
 * Results equal n_chunks calls of infv_vqf_encode_chunk (new_video on the first only).
 *   frames [n_chunks][T * tokens_per_frame][enc_width], u [n_chunks][n_layers][nb_samples] or NULL,
 *   hidden_out [n_chunks][n_query][hidden] / llama_out [n_chunks][n_query][proj_out] / llama_mean [n_query][proj_out]
 *   (the eval loop's mean over chunks, run_inference_inf_video_llama_nextqa.py:194); each may be NULL. */
int infv_vqf_encode_video(infv_vqf_handle h, const infv_ltm_handle* ltm, const void* frames, int32_t n_chunks,
                          int32_t T, const infv_vqf_weights* w, const double* u, int32_t new_video,
                          float* hidden_out, float* llama_out, float* llama_mean, void* stream);

/* infv_vqf_encode_video over V videos in one call (evaluation harnesses over many short videos).  Chunks are PACKED, video v
 * owning chunks [cu[v], cu[v+1]) (cu: HOST array [V+1], cu[0] = 0, non-decreasing; a video may have no chunk):
 *   frames     [cu[V]][T*P][enc_width]   u [cu[V]][n_layers][S] float64 (may be NULL when not sticky, or when every video is
 *                                        new and has one chunk)
 *   hidden_out [cu[V]][Q][hidden], llama_out [cu[V]][Q][proj_out] (either may be NULL)
 *   llama_mean [V][Q][proj_out]: video v's mean over its chunks, bitwise infv_vqf_mean over its own llama rows (NULL: none)
 *   ltm        [V][n_layers] one-layer handles, video-major (NULL when alpha == 1); all distinct
 * new_video = 1 starts every memory afresh; 0 continues each video's memories.  The schedule is infv_vqf_encode_video's over
 * all packed chunks: layer 0's chunk-independent prefix once, one token pass (split operands + frame means), layer 0's memories
 * through infv_ltm_steps_videos with the shared query, short-term attention over all chunks; for later layers the query-token
 * blocks batched over all chunks and their memories through infv_ltm_steps_videos with per-chunk queries on the side stream
 * while the caller's stream runs the short-term attention; then merge, FFN, llama_proj and the per-video means.
 * BATCH INVARIANCE: a video's hidden states, llama rows, mean and memories (B, bin masses, draws) do not depend on what else is
 * in the call.  The GEMMs over row blocks of chunks take 128 x 128 tiles without split-K; the short-term contractions take
 * their kernel shape and split-K counts from the chunk's shape and a constant (split-K partials are summed in a fixed order;
 * no float atomics); sub-batch sizes still vary for occupancy, which changes no summation order.  So the
 * values agree with infv_vqf_encode_video to fp32 rounding, not bit for bit; a Gibbs uniform within rounding of a cdf edge can
 * flip a draw.  Refusals (INFV_ERR_INVALID: bad cu, null or repeated handle) happen before any device work. */
int infv_vqf_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu,
                           const void* frames, int32_t T, const infv_vqf_weights* w, const double* u,
                           int32_t new_video, float* hidden_out, float* llama_out, float* llama_mean, void* stream);

/* ---- VideoChat2 Q-former (infty-VideoChat2/models/blip2/Qformer.py): query tokens + instruction text tokens ---- */

#define INFV_VQF_VC_MAX_LAYERS 24
#define INFV_VQF_VC_MAX_TOKENS 608   /* 96 query tokens + max_txt_len = 512 instruction tokens */

/* Self-attention over the query + text tokens of nb chunks (Qformer.py:232-300 with all-ones masks, eval mode), the building
 * block beside infv_vqf_short_attention:  ctx = softmax(q k^T / sqrt(64)) v  per head of the handle's n_heads.
 *   qkv     [nb][n_max][3 * hidden]  query | key | value of every token, bias applied (device)
 *   n_valid HOST int32[nb], each in 1..n_max: chunk b attends over its first n_valid[b] tokens; NULL = n_max everywhere
 *   ctx     [nb][n_max][hidden]      rows at or beyond n_valid[b] are written as zeros
 * n_max <= INFV_VQF_VC_MAX_TOKENS (INFV_ERR_UNSUPPORTED above).  Keys at or beyond n_valid[b] are never read.  Arithmetic is
 * fp32 FMA; the summation order of an output element depends on its chunk's n_valid alone, so a chunk's result is the same
 * bits whatever else is in the call.  Row tiles of 32 go across workgroups (grid: head x chunk x row tile). */
int infv_vqf_self_attention(infv_vqf_handle h, const float* qkv, int32_t nb, int32_t n_max, const int32_t* n_valid,
                            float* ctx, void* stream);

/* One BertLayer of the VideoChat2 Q-former (Qformer.py:419-505): self-attention over query + text tokens (:195-310, :320-324),
 * cross-attention of the query part in every cross_attention_freq-th layer (:463-481), the query FFN and the text FFN
 * (:483-496).  The x_* members are read only when has_cross is set. */
typedef struct {
    infv_linear self_q, self_k, self_v, self_o;   infv_layernorm self_ln;    /* layer.attention                      */
    int32_t has_cross;                                                        /* layer.has_cross_attention            */
    int32_t reserved;                                                         /* 0                                    */
    infv_linear x_q, x_k, x_v, x_o;               infv_layernorm x_ln;       /* layer.crossattention                 */
    infv_linear q_ffn_in, q_ffn_out;              infv_layernorm q_ffn_ln;   /* intermediate_query / output_query    */
    infv_linear t_ffn_in, t_ffn_out;              infv_layernorm t_ffn_ln;   /* intermediate / output (text rows)    */
} infv_vqf_vc_layer;

typedef struct {
    int32_t n_layers;                    /* 1..INFV_VQF_VC_MAX_LAYERS (Qformer.py:544-640: the encoder loop; 12) */
    int32_t reserved;                    /* 0 */
    const infv_vqf_vc_layer* layers;     /* HOST array [n_layers] */
    infv_linear mistral_proj;            /* videochat2_it_mistral.py:252; w == NULL: absent (proj_out / proj_mean must be NULL) */
} infv_vqf_vc_weights;

/* The VideoChat2 Q-former over the packed chunks of V >= 1 videos, layer-major (the device side of encode_img after the
 * vision encoder, videochat2_it_mistral.py:199-252, inside the eval loop of eval_code/run_nextqa_mistral.py:141-152; one video
 * is V = 1).  The handle's config gives n_heads, hidden, inter, enc_width, tokens_per_frame, n_query, proj_out, nb_samples,
 * alpha and ln_eps; its n_layers is not read (the weights carry the layer count).  n_cross = number of layers with has_cross.
 *   ltm        [V][n_cross] one-layer LTM handles, video-major, all distinct (NULL when alpha == 1)
 *   cu         HOST [V+1], cu[0] = 0, non-decreasing: video v owns chunks [cu[v], cu[v+1])
 *   frames     [cu[V]][T * tokens_per_frame][enc_width] fp32
 *   hidden_in  the encoder input rows of every video, packed: video v's [n_query + text_len[v]][hidden] (query rows first)
 *              start at row  sum_{w<v} (n_query + text_len[w]);  every chunk of a video starts from the same rows
 *   text_len   HOST [V], each >= 0 with n_query + text_len[v] <= INFV_VQF_VC_MAX_TOKENS
 *   u          [cu[V]][n_cross][nb_samples] float64, or NULL under infv_vqf_encode_videos's rules (not sticky; every video new
 *              with one chunk; the device rng of every memory on)
 *   new_video  1 starts every memory afresh, 0 continues each video's memories
 *   hidden_out last hidden states, packed per CHUNK: chunk c of video v holds n_query + text_len[v] rows (query rows first)
 *              starting at row  sum over earlier chunks of their row counts        (may be NULL)
 *   proj_out   [cu[V]][n_query][proj_out] mistral_proj of the query rows           (may be NULL)
 *   proj_mean  [V][n_query][proj_out] per-video mean over its chunks (run_nextqa_mistral.py:150), undefined for a video
 *              without chunks                                                        (may be NULL)
 * Schedule: every chunk's frames are pooled once (all cross layers step from that one copy) and split once into the bf16
 * operands of the short-term attention when they fit INFV_VQF_SPLIT_CACHE_GB; per layer, over all packed chunks, the QKV
 * projection, infv_vqf_self_attention's kernel, output dense + LayerNorm; on cross layers the cross query, that layer's V
 * memories through infv_ltm_steps_videos with per-chunk queries on the shared worker stream while the caller's stream runs the
 * short-term attention, the merge and its output block; then the query FFN on the query rows and the text FFN on the text
 * rows (text rows are kept packed: no padding enters any kernel); last mistral_proj and the per-video means.
 * BATCH INVARIANCE as in infv_vqf_encode_videos: a video's hidden rows, projected rows, mean and memories (B, bin masses,
 * draws, probabilities) are the same bits whatever else is in the call, at whatever position, whatever the neighbours' text
 * lengths, and whether its chunks come in one call or in two (new_video = 0 on the second).  Values agree with the per-chunk
 * binding to fp32 rounding.  Token counts that are a multiple of 32 but not of 64 take the exact-fp32 contractions.
 * Refused before any device work or memory change: bad cu, a null or repeated LTM handle, negative text_len (INFV_ERR_INVALID);
 * n_query + text_len[v] > 608, n_layers > 24, T * tokens_per_frame not a multiple of 32, fp16 or bf16 tokens set on the handle
 * (INFV_ERR_UNSUPPORTED).
 * This call and infv_vqf_vc_encode_streams read fp32 tokens only: fp16 / bf16 tokens go to infv_vqf_vc_encode_videos_tok /
 * infv_vqf_vc_encode_streams_tok below, which take the element type as an argument and read the tokens in place. */
int infv_vqf_vc_encode_videos(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                              int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len,
                              const double* u, int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean,
                              void* stream);

/* infv_vqf_vc_encode_videos over V STREAMS that read their frame tokens from F distinct blocks (additive): several instructions
 * asked of one video.  The Q-former takes the instruction as input (encode_img with qformer_text_input,
 * videochat2_it_mistral.py:199-252, :204-223), so the queries, densities, draws and memories of a video depend on it -- the
 * frame tokens do not.  Asking K questions of one video (run_nextqa_mistral.py:141-152 with a different `instruction` per
 * stream) is K streams over ONE copy of its tokens.  A stream has its own instruction (hidden_in rows, text_len), its own
 * n_cross memories, its own rows of u and of the outputs.
 *   frames     [fcu[F]][T * tokens_per_frame][enc_width] fp32: the F blocks, packed
 *   fcu        HOST [F+1], fcu[0] = 0, non-decreasing: block f owns chunks [fcu[f], fcu[f+1])
 *   frame_src  HOST [V], each in [0, F), in any order (streams of one block need not be adjacent); stream v has as many chunks
 *              as its block: cu[v+1] - cu[v] == fcu[s+1] - fcu[s], s = frame_src[v]
 * Everything else -- ltm [V][n_cross], cu, hidden_in, text_len [V], u [cu[V]][n_cross][nb_samples], the outputs packed per stream
 * and chunk, new_video -- is infv_vqf_vc_encode_videos's, with "video" read as "stream".
 * Bits: every result (hidden rows, projected rows, per-stream means, each memory's B, bin masses, draws and probabilities) is
 * bit for bit that of infv_vqf_vc_encode_videos on V videos where video v's frames are a copy of block frame_src[v].
 * Schedule: the one token pass (split planes, their transposed copies, the frame means; else infv_ltm_pool) runs over the fcu[F]
 * distinct chunks only, and the planes fit INFV_VQF_SPLIT_CACHE_GB by the distinct bytes.  The short-term contractions read
 * stream-chunk c's B operand at chunk  fcu[frame_src[v]] + i  through a device map written from kernel arguments (no host buffer
 * outlives the call, no host synchronisation beyond workspace growth); each cross layer's memories step through
 * infv_ltm_steps_videos_from with kbar_chunk0[v] = fcu[frame_src[v]].  On the exact-fp32 path (token counts that are a multiple
 * of 32 but not of 64) the map applies to the caller's `frames` directly.  Where the split path is in use and the planes of
 * the distinct chunks do NOT fit the budget, every sub-batch splits each contiguous run of its source chunks into its own plane
 * buffers and contracts with the identity map: correct, but the split work is not shared between streams in that case.
 * Refused before any device work or memory change: bad cu or fcu, frame_src out of range, a chunk-count mismatch between a
 * stream and its block, a null or repeated LTM handle, negative text_len (INFV_ERR_INVALID); the token-count, layer-count and
 * token-dtype cases of infv_vqf_vc_encode_videos (INFV_ERR_UNSUPPORTED). */
int infv_vqf_vc_encode_streams(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const float* frames,
                               int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T, const infv_vqf_vc_weights* w,
                               const float* hidden_in, const int32_t* text_len, const double* u, int32_t new_video,
                               float* hidden_out, float* proj_out, float* proj_mean, void* stream);

/* infv_vqf_vc_encode_videos / infv_vqf_vc_encode_streams with the frame tokens' element type as an ARGUMENT of the call
 * (additive): token_dtype is an infv_token_dtype code -- 0 fp32, 1 bf16, 3 fp16 -- or 4 (INFV_TOKENS_F8E4M3: OCP e4m3fn at 1 byte
 * per element, the caller's storage choice; its hi planes F_hi / FT_hi are written, no lo planes, two-product contractions, the
 * bits of the call on the tokens widened to fp32) and `frames` holds that type.  The handle's
 * infv_vqf_set_token_dtype setting is neither read nor changed.  Code 0 is the call without the argument: its bits, its
 * launches.  fp16 / bf16 tokens are read in place at 2 bytes per element (no fp32 copy) and give the bits of the fp32 call on
 * the same values: an fp16 value is exactly its bf16 hi + lo planes, a bf16 value is its own hi plane (the contractions then take
 * two products instead of three), and the frame means are summed in token order in fp32 either way.  Where T * tokens_per_frame
 * is a multiple of 64 the token pass writes the planes, and the frame means too where a frame divides its 64-token tile; other
 * frame sizes (tokens_per_frame = 196) pool through infv_ltm_pool at the token type, then split -- a one-launch form for them was
 * measured slower than these two and is not shipped.  Token counts that are a multiple of 32 only, infv_vqf_set_precision(h, 1)
 * and INFV_VQF_FP32 take the fp32 contractions from an fp32 copy of the distinct chunks in the handle's workspace.
 * Refused before any device work or memory change, beside the refusals of the calls without the argument: an unknown code,
 * fp16 / bf16 `frames` that are not 16-byte aligned (INFV_ERR_INVALID). */
int infv_vqf_vc_encode_videos_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                  int32_t token_dtype, int32_t T, const infv_vqf_vc_weights* w, const float* hidden_in,
                                  const int32_t* text_len, const double* u, int32_t new_video, float* hidden_out, float* proj_out,
                                  float* proj_mean, void* stream);

int infv_vqf_vc_encode_streams_tok(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                                   int32_t token_dtype, int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T,
                                   const infv_vqf_vc_weights* w, const float* hidden_in, const int32_t* text_len, const double* u,
                                   int32_t new_video, float* hidden_out, float* proj_out, float* proj_mean, void* stream);

/* ---- encode_img from what a pipeline holds: the vision encoder's output and the tokenizer's ids (additive) ----
 * Two pieces of the reference's encode_img stand between the vision encoder and the calls above:
 *   vision_layernorm (videochat2_it_mistral.py:195; nn.LayerNorm(width, eps = 1e-12), blip2.py:88) over the vision encoder's fp16
 *     output -- under autocast it hands over an fp32 tensor, twice the bytes of what it read;
 *   the embedding layer (Qformer.py:54-111, called from videochat2_it_mistral.py:204-223): word_embeddings(input_ids) +
 *     position_embeddings behind the query tokens, ONE LayerNorm over query and text rows together.
 * infv_vqf_vc_front carries both; either may be off. */
typedef struct {
    const float* gamma;                  /* device fp32 [enc_width]; NULL: no vision LayerNorm (beta is then not read) */
    const float* beta;                   /* device fp32 [enc_width] */
    float eps;                           /* 1e-12 in the reference */
} infv_vqf_vision_ln;

typedef struct {
    const float* word;                   /* device fp32 [vocab][hidden]; NULL: no embedding layer (hidden_in is read as before) */
    const float* pos;                    /* device fp32 [max_pos][hidden] */
    infv_layernorm ln;                   /* bert.embeddings.LayerNorm, eps = the handle's ln_eps */
    int32_t vocab, max_pos;
    const float* query_tokens;           /* device fp32 [n_query][hidden]: the raw query tokens (query + extra, concatenated) */
} infv_vqf_vc_emb;

typedef struct {
    infv_vqf_vision_ln vision_ln;
    infv_vqf_vc_emb emb;
    const int32_t* input_ids;            /* HOST, packed by text_len as cu packs chunks: video v's ids start at sum_{w<v} text_len[w] */
    int32_t reserved;                    /* 0 */
} infv_vqf_vc_front;

/* infv_vqf_vc_encode_videos_tok (frame_src == NULL; F and fcu are not read) or infv_vqf_vc_encode_streams_tok (frame_src given)
 * with `front` in front.  With front NULL, or both of its parts off, it IS that call: its bits, its launches.
 *   vision LayerNorm on: `frames` is the vision encoder's output in its own type (fp32 / fp16 / bf16, 16-byte aligned; fp8 tokens,
 *     code 4, are INFV_ERR_UNSUPPORTED here before any device work: no vision encoder emits fp8), read in place.  One launch writes (mean, 1 / sqrt(var + eps)) per distinct token row (8 bytes a token; two-pass, biased variance,
 *     fixed-order wave reductions); the token pass and the pooling then normalise on load:  y = fma((x - mean) * rstd, gamma, beta)
 *     with x widened exactly.  No fp32 copy of the tokens is made.  A normalised value is a general fp32 number, so every source
 *     type writes all four planes and takes the three-product contractions (bf16 too; the planes count 4 x towards
 *     INFV_VQF_SPLIT_CACHE_GB).  Where the split path does not apply (token counts that are a multiple of 32 only,
 *     infv_vqf_set_precision(h, 1), INFV_VQF_FP32) the normalised tokens of the distinct chunks are written as fp32 into the
 *     handle's workspace and the fp32 contractions run from there.
 *     BITS: for any source type the call equals, bit for bit, the call without the LayerNorm on the fp32 tensor
 *     infv_vqf_layernorm_tokens writes from the same `frames`.
 *   embedding layer on: hidden_in must be NULL; video v's encoder input rows are LN(query_tokens[q]) for q < n_query and
 *     LN(word[ids_v[t]] + pos[t]) for t < text_len[v] (positions start at 0 at the first text token; no padding, no mask).  A
 *     video's rows do not depend on the batch.  The ids are checked on the host, then staged through a pinned buffer of the handle
 *     whose reuse waits on an event recorded behind the copy.  BITS: those of the call with hidden_in = infv_vqf_vc_embed's rows.
 * Refused before any launch or memory change, beside the refusals of the _tok calls (INFV_ERR_INVALID): reserved != 0, gamma
 * without beta, frames not 16-byte aligned under the LayerNorm, the embedding layer together with a non-NULL hidden_in, a table or
 * input_ids missing, text_len[v] > max_pos, an id outside [0, vocab) (the message names the video);  INFV_ERR_UNSUPPORTED: the
 * LayerNorm with enc_width no multiple of 64 or above 4096. */
int infv_vqf_vc_encode_img(infv_vqf_handle h, const infv_ltm_handle* ltm, int32_t V, const int32_t* cu, const void* frames,
                           int32_t token_dtype, int32_t F, const int32_t* fcu, const int32_t* frame_src, int32_t T,
                           const infv_vqf_vc_weights* w, const infv_vqf_vc_front* front, const float* hidden_in,
                           const int32_t* text_len, const double* u, int32_t new_video, float* hidden_out, float* proj_out,
                           float* proj_mean, void* stream);

/* ---- the per-frame image Q-former: the producer of the Video-LLaMA frame tokens (additive) ----
 * The image Q-former of encode_short_memory_frame (infinityqa.py:259-270; Qformer.py BertEncoder with
 * position_embedding_ext == None, so no long-term memory is called whatever alpha is) over F frames: bert-base with a
 * cross-attention in every layer whose has_cross is set, n_query learned queries, no text rows.  It is the layer loop of
 * infv_vqf_vc_encode_videos over F one-chunk "videos" that all start from query_rows.
 *   vision      device [F][n_tokens][enc_width] in token_dtype (0 fp32, 1 bf16, 3 fp16, 4 fp8 e4m3), 16-byte aligned, read in place.
 *               With `ln` on it is the vision encoder's output before ln_vision, normalised on load exactly as
 *               infv_vqf_vc_encode_img does, eps from the struct (the reference's ln_vision is nn.LayerNorm's default 1e-5); fp8
 *               input with the LayerNorm on is INFV_ERR_UNSUPPORTED.
 *   n_tokens    >= 1, any value (a ViT hands over 257 = class token + 16 x 16 patches).  It is an argument: the handle's
 *               tokens_per_frame is not read, nor are its alpha and proj_out.  Where n_tokens is no multiple of 64 the split-bf16
 *               planes are kept at n_pad = ceil(n_tokens / 64) * 64 tokens a frame with zero rows behind the frame's own; exactly
 *               n_tokens rows of a frame are read.  The row softmax runs over the first n_tokens columns and writes zeros into
 *               the pad columns, so the pad keys carry no mass.  bf16 tokens without LayerNorm then get their hi plane written
 *               too (another stride than the caller's buffer).  n_tokens % 64 == 0: the kernels and launches of
 *               infv_vqf_vc_encode_videos_tok, bit for bit.
 *   precision   enc_width must be a multiple of 64.  The call takes the split-bf16 contractions; with infv_vqf_set_precision(h, 1)
 *               or INFV_VQF_FP32 set it is INFV_ERR_UNSUPPORTED unless n_tokens % 32 == 0, where the fp32 kernels run.
 *   w           the text FFN members are never read (no text rows exist); mistral_proj must be absent (w and b NULL).
 *   query_rows  device fp32 [n_query][hidden], 16-byte aligned: the embedded query tokens (embeddings.LayerNorm(query_tokens)).
 *   out         device [F][n_query][hidden] in out_dtype (0 fp32, 1 bf16, 3 fp16), 16-byte aligned.  bf16 / fp16: the last layer's
 *               query-FFN LayerNorm epilogue rounds to nearest even and writes the 2-byte rows itself -- the bits of
 *               (fp32 result).to(dtype), no fp32 copy of the output is made.  fp32: the rows are copied out of the workspace as
 *               infv_vqf_vc_encode_videos copies hidden_out (its launches, one for one).  fp8 output: INFV_ERR_UNSUPPORTED (the
 *               library does not quantise).
 * A frame's output bits do not depend on F, on the frame's position or on the other frames' contents.
 * Refused before any launch or memory change (INFV_ERR_INVALID unless noted): a null h, w, query_rows, or (F > 0) vision / out;
 * F < 0 (F == 0 returns INFV_OK); an unknown token or output dtype; vision, out or query_rows not 16-byte aligned; n_tokens < 1;
 * w->n_layers < 1 or above INFV_VQF_VC_MAX_LAYERS (INFV_ERR_UNSUPPORTED); a projection present; gamma without beta; for bf16 / fp16
 * output a last-layer q_ffn_out.b / q_ffn_ln that is not 16-byte aligned. */
int infv_vqf_encode_frames(infv_vqf_handle h, int32_t F, const void* vision, int32_t token_dtype, int32_t n_tokens,
                           const infv_vqf_vc_weights* w, const infv_vqf_vision_ln* ln /* NULL or gamma NULL: off */,
                           const float* query_rows /* device [n_query][hidden]: the embedded query tokens, shared by all frames */,
                           void* out /* [F][n_query][hidden] */, int32_t out_dtype /* 0 fp32, 1 bf16, 3 fp16 */, void* stream);

/* The arithmetic of the QUERY-SIDE linears of infv_vqf_encode_frames (additive: the ABI version stays 6).  mode:
 *   0 (default)  fp32 MFMA: the path and the bits of a handle that never called this.
 *   1            split-bf16: the fp32 activation and the fp32 weight are each carried as hi = bf16(x), lo = bf16(x - hi); per k-step
 *                three bf16 MFMA products in the order lo.hi, hi.lo, hi.hi, fp32 accumulation (the scheme of the short-term
 *                attention's contractions).  fp32-class: about 1e-5 of a sum of |x w| at K = 3072.
 *   2            fp16: activation and weight rounded to nearest-even fp16, as `.half()` does (beyond 65504: inf, as under autocast);
 *                one f16 MFMA product, fp32 accumulation.  Bias, GELU, residual and LayerNorm stay fp32.  The f16 MFMA KEEPS
 *                subnormal fp16 operands (magnitudes below 2^-14) on gfx950: 2^-20 x 2^10 through this mode gives 2^-10, not 0
 *                (tests/test_attention_precision_gpu.py, one MI355X); whether subnormal operands cost it time is not measured.
 * The mode governs the eight linears per layer on the query rows -- the stacked self q/k/v, the self output, the cross query, the
 * cross output, q_ffn_in and q_ffn_out (with its 2-byte cast epilogue) -- and nothing else: the short-term attention and the token
 * pass run as before, a linear stays two launches (GEMM + epilogue), the activations are split / rounded between the registers and
 * LDS (no activation plane in memory), and a frame's bits still do not depend on F or on the other frames.
 * The weights arrive as fp32; their 2-byte planes ([N][K], a stacked q/k/v as one [3 * hidden][K] set) are made on the device and
 * cached in the handle, keyed on (weight pointers, shape), while the NON-ZERO weights epoch (infv_vqf_set_weights_epoch) stands;
 * a change of the epoch or of the mode drops them, infv_vqf_destroy frees them.  With epoch 0 every linear rebuilds its planes into
 * one scratch pair (correct, and 1 or 2 more launches per weight matrix).  Cost for the model's image Q-former (12 layers, hidden 768,
 * inter 3072: about 92 M weight elements): about 370 MB in mode 1 (two planes), about 185 MB in mode 2.
 * While the mode is not 0, EVERY OTHER entry point that takes the handle -- infv_vqf_short_attention, infv_vqf_encode_chunk /
 * _video / _videos, the infv_vqf_vc_encode_* family, infv_vqf_vc_embed -- returns INFV_ERR_UNSUPPORTED before any launch or workspace
 * change, naming this function: those calls feed their cross query into the long-term memories' Gibbs draw, and reduced products
 * never feed the scores of the draw (csrc/split_gemm.hip).  (infv_vqf_self_attention runs no linear and is not refused.)
 * A null handle or a mode outside 0..2 is INFV_ERR_INVALID and leaves the setting as it was. */
int infv_vqf_set_linear_precision(infv_vqf_handle h, int32_t mode);

/* One linear of the layer-major calls in its batch-invariant form, under the handle's linear precision (exported for tests and
 * measurements, as infv_vqf_self_attention and infv_vqf_token_pass are):
 *   y [M][n_lin * n_out] = LN?( act( x [M][K] . [lin[0].w; ...; lin[n_lin-1].w]^T + bias ) + residual[m % res_rows] )
 * lin: HOST array of n_lin linears with device pointers, each w [n_out][K] (b may be NULL); act 0 none, 1 GELU; residual NULL or
 * device [res_rows][n_lin * n_out]; ln NULL or gamma / beta [n_lin * n_out] (eps: the handle's ln_eps).  128 x 128 tiles, no split-K,
 * whatever M is.  Refused before any launch or memory change: a null h, x, lin, y or lin[i].w; M < 1; n_lin outside 1..4; an
 * unknown act; res_rows < 1 with a residual; gamma without beta; a pointer that is not 16-byte aligned (INFV_ERR_INVALID); K or
 * n_out no positive multiple of 64, K or n_lin * n_out above 4096 (INFV_ERR_UNSUPPORTED). */
int infv_vqf_linear(infv_vqf_handle h, const float* x, int32_t M, int32_t K, const infv_linear* lin, int32_t n_lin, int32_t n_out,
                    int32_t act, const float* residual, int32_t res_rows, const infv_layernorm* ln, float* y, void* stream);

/* The arithmetic of the CROSS-ATTENTION of infv_vqf_encode_frames (additive: the ABI version stays 6).  mode:
 *   0 (default)  the split-bf16 (or, with infv_vqf_set_precision(h, 1), fp32) contractions: the path, the launches and the bits of a
 *                handle that never called this.
 *   1            fp16 operands, fp32 accumulation, one f16 MFMA product per contraction -- what the reference's fp16 autocast runs.
 *                Per frame and head (dh = 64), with q the fp32 output of the cross-query linear (in the handle's linear precision):
 *                  x^  = fp16(LN(x)) with the vision LayerNorm on (its fp32 arithmetic, from the same statistics launch), else
 *                        fp16(float(x)); round to nearest even AFTER widening, so fp16, bf16 and fp8 sources give the bits of the
 *                        run on the same values as fp32; rows n_tokens .. n_pad - 1 (n_pad = ceil(n_tokens / 64) * 64) exact zeros
 *                  q~' = fp16(32 * sum_c fp16(q[c]) * fp16(Wk[c][:]))          32 = 2^8 / sqrt(64); the key bias is dropped, as in mode 0
 *                  s   = 2^-8 * sum_e q~'[e] * x^[j][e];  p = softmax over the first n_tokens columns in fp32, maximum subtracted
 *                  p'  = fp16(2^10 * p), exact zeros in the pad columns
 *                  o'  = fp16(2^-10 * sum_j p'[j] * x^[j][:])
 *                  ctx = sum_e o'[e] * fp16(Wv[c][e]) + bv[c]                   fp32 bias, added once
 *                The two powers of two keep q~' and p' out of fp16's subnormal range (an unscaled q~ of the test models has about
 *                1 % of its entries below 2^-14, a peaked row most of its p), so the result does not rest on how the MFMA treats
 *                subnormal operands.  Beyond fp16's range a value becomes inf, as `.half()` gives: |q~| >= 256, or a token above
 *                65504 in magnitude without the LayerNorm; nothing guards against it.  The score matrix never reaches memory, the
 *                context product has no split-K; a frame's tiles and summation orders depend on n_tokens alone, so a frame's bits
 *                do not depend on F or on the other frames.  n_tokens above 512 is INFV_ERR_UNSUPPORTED in this mode;
 *                infv_vqf_set_precision and INFV_VQF_FP32, which choose between the two forms of mode 0, are not read in it.
 *                Bias, merge, output dense, LayerNorms and the query-side linears are unchanged.
 * One pass over the vision output writes the fp16 plane [F][n_pad][enc_width] and its transposed copy (4 bytes per padded token
 * element, written once per call and shared by all its cross layers; 461 MB at 256 x 257 x 1408); a sub-batch of up to 256
 * frames keeps its q~' and o' rows as fp16 (2 x 277 MB at 12 heads x 32 queries x 1408).  All four are workspaces of the handle, grown
 * on demand like the split-bf16 planes of mode 0 and NOT released after the call: about 1 GB at that shape until infv_vqf_destroy.  The key and value weights arrive as fp32; their fp16 planes
 * (Wk per head transposed [H][enc_width][64], Wv as it lies) are made on the device and kept in the cache of the linears' planes, by
 * its rules: keyed on the weight pointers while the NON-ZERO weights epoch stands, dropped by a change of the epoch, of this mode or
 * of the linear precision, rebuilt in every call with epoch 0 (two more launches per cross layer).  Cost for the model's image
 * Q-former (6 cross layers of 768 x 1408): 26 MB.
 * Independent of infv_vqf_set_linear_precision: all six combinations run.  While the mode is not 0, every other entry point that
 * takes the handle -- the list of infv_vqf_set_linear_precision -- returns INFV_ERR_UNSUPPORTED before any launch or workspace change,
 * naming this function; infv_vqf_set_context_tap works in both modes.  A null handle or a mode outside 0..1 is INFV_ERR_INVALID and
 * leaves the setting as it was. */
int infv_vqf_set_attention_precision(infv_vqf_handle h, int32_t mode);

/* One cross-attention of infv_vqf_encode_frames alone, under the handle's attention precision (exported for tests and measurements,
 * as infv_vqf_linear and infv_vqf_token_pass are): the vision statistics and the token pass of that call, then one layer's attention.
 *   vision, token_dtype, n_tokens, ln   as in infv_vqf_encode_frames
 *   xq     device fp32 [F][n_query][hidden]: the cross query (bias applied), 16-byte aligned
 *   key, value   the layer's linears (HOST structs, device pointers; key->b is not read, value->b may be NULL)
 *   ctx    device fp32 [F][n_query][hidden]: the context, value bias included, before the output dense -- what the context tap copies
 * Mode 0 issues the launches of the default path (its bits: the context tap of the same layer), mode 1 the fp16 ones.
 * Refused before any launch or memory change (INFV_ERR_INVALID unless noted): a null h, key, value or weight, or (F > 0) vision, xq or
 * ctx; F < 0 (F == 0 returns INFV_OK); an unknown token dtype; a pointer that is not 16-byte aligned; n_tokens < 1; gamma without
 * beta; fp8 tokens with the LayerNorm, enc_width no multiple of 64, n_tokens % 32 != 0 on the fp32 contractions, n_tokens > 512 in
 * mode 1 (INFV_ERR_UNSUPPORTED). */
int infv_vqf_frame_cross_attention(infv_vqf_handle h, int32_t F, const void* vision, int32_t token_dtype, int32_t n_tokens,
                                   const infv_vqf_vision_ln* ln /* NULL or gamma NULL: off */, const float* xq, const infv_linear* key,
                                   const infv_linear* value, float* ctx, void* stream);

/* A tap for tests (exported as infv_vqf_self_attention is): the NEXT infv_vqf_encode_frames call on h also copies the cross-attention
 * context of encoder layer `layer` (Qformer.py:303-304: softmax(q k^T / sqrt(dh)) v with the value bias, before the output dense),
 * [F][n_query][hidden] fp32, to dst (device) on the call's stream; the tap is cleared when that call returns.  dst NULL: off.  A layer
 * that is no cross-attention layer of the call's weights makes that call INFV_ERR_INVALID before any launch.  No kernel is added. */
int infv_vqf_set_context_tap(infv_vqf_handle h, int32_t layer, float* dst);

/* The vision LayerNorm alone (exported for tests and measurements): out_f32 [n_rows][d] = LayerNorm(frames [n_rows][d]) with the
 * kernels and the arithmetic of infv_vqf_vc_encode_img -- the reference form of its bits.  d a multiple of 64 up to 4096; frames,
 * gamma, beta and out_f32 16-byte aligned.  The row statistics go through a process-wide device buffer. */
int infv_vqf_layernorm_tokens(const void* frames, int32_t token_dtype, int64_t n_rows, int32_t d, const float* gamma,
                              const float* beta, float eps, float* out_f32, void* stream);

/* The embedding layer alone (exported for tests and measurements): out_rows = the packed encoder input rows of V videos, video v's
 * n_query + text_len[v] rows of width hidden (query rows first), from front->emb and front->input_ids (front->vision_ln is not
 * read).  The handle gives n_query, hidden and ln_eps and owns the pinned staging buffer.  Refusals as in infv_vqf_vc_encode_img. */
int infv_vqf_vc_embed(infv_vqf_handle h, const infv_vqf_vc_front* front, int32_t V, const int32_t* text_len, float* out_rows,
                      void* stream);

/* The token pass alone (exported for tests and measurements, as infv_vqf_self_attention is): the launches the encoders issue for
 * frames [nb][n_tokens][d] of element type token_dtype.
 *   Fh, Fl [nb][n_tokens][d], Th, Tl [nb][d][n_tokens] bf16: the hi / lo planes and their transposed copies.  bf16 tokens are
 *          their own hi plane: Fh, Fl and Tl must be NULL and only Th is written.  fp8 tokens (code 4) have no lo piece: Fl and
 *          Tl must be NULL, Fh and Th are written.
 *   kbar   [nb][n_tokens / tokens_per_frame][d] fp32 frame means, the bits of infv_ltm_pool; NULL: planes only
 * n_tokens a multiple of 32, d a multiple of 64, every pointer 16-byte aligned, tokens_per_frame dividing n_tokens where kbar is
 * given (INFV_ERR_INVALID otherwise).  INFV_ERR_UNSUPPORTED, and no launch, where no one-pass form with the means exists:
 * kbar given and tokens_per_frame not dividing 64. */
int infv_vqf_token_pass(const void* frames, int32_t token_dtype, int32_t nb, int32_t n_tokens, int32_t d, int32_t tokens_per_frame,
                        void* Fh, void* Fl, void* Th, void* Tl, float* kbar, void* stream);

/* out[i] = mean over n of in[n][i]  (the eval loop's mean over chunk embeddings,
 * run_inference_inf_video_llama_nextqa.py:194) */
int infv_vqf_mean(const float* in, int32_t n, int64_t elems, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
