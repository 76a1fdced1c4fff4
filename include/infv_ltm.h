/*
 * infv_ltm.h -- C ABI of the MI355X-native long-term-memory (LTM) consolidation path of
 * infinity-Video (deep-spin/Infinite-Video).  Implemented by libinfv_ltm.so
 * (infinite-video_amd/csrc/, hand-written HIP for gfx950).
 *
 * The reference has no FFI for this path: its operator boundary is the Python nn.Module
 *     LongTermAttention.forward(k, q, new_doc, layer_n)
 *         infty-Video-LLaMA/InfVideoLLaMA/models/long_term_attention_gibbs.py:288-346
 * called once per cross-attention layer per chunk from
 *     BertSelfAttention.forward   infty-Video-LLaMA/InfVideoLLaMA/models/Qformer.py:216-223.
 * The entry points below are what a binding for that boundary needs; each cites the
 * reference lines it replaces.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every pointer documented "device" is a HIP device pointer owned by the caller;
 *     the handle owns only the consolidated memory (coefficients B, their projections,
 *     the sticky histogram) and its workspaces;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*,
 *     NULL = the null stream); no entry point synchronises except infv_ltm_sync and the
 *     get calls that copy to HOST buffers, with the host waits listed below;
 *   - `stream` may be any stream, a non-blocking side stream included (tests/test_stream_order_gpu.py runs every entry point
 *     that takes one behind a delay on such a stream).  What a caller may rely on: a call reads its device inputs no earlier than
 *     the work queued on `stream` before it, and when it returns, work queued on `stream` behind it may overwrite every input and
 *     read every output and every exported state -- the worker streams the library forks over (infv_ltm_consolidate*: three
 *     process-wide non-blocking streams shared by all handles of a device) start behind `stream` and are joined into it before the
 *     call returns.  Handles on different streams do not disturb each other's results.
 *     Host waits, none of which changes a result: a call that has to GROW a workspace synchronises the device first (the first
 *     call of a handle, or of a larger shape; a handle that has run a shape once runs it again without a host wait);
 *     infv_ltm_set_plan / _set_dense_plan / _set_psi_plan / _set_grid_plan upload host tables; infv_ltm_set_probs and
 *     infv_ltm_set_bins, which take no stream, synchronise the device and then copy, so they take effect in PROGRAM order: steps
 *     issued before the setter use the old override (or none), steps issued after it the new one; infv_ltm_destroy waits for
 *     the handle's work.
 *     Not promised: ordering between calls of ONE handle on DIFFERENT streams.  The memory, the workspaces and the override
 *     buffers are ordered by the stream of the call alone, so a caller who moves a handle to another stream orders the two
 *     streams itself (an event, or infv_ltm_sync) before the first call on the new one;
 *   - a failure that only shows on the device (the persistent chain kernel of
 *     infv_ltm_consolidate timed out waiting for workgroups that never became resident, e.g.
 *     on a partitioned or shared GPU) is latched in host-visible memory: infv_ltm_sync and
 *     every later entry point on the handle return INFV_ERR_STATE once, the memory is reset;
 *   - return value: 0 on success, negative infv_status on failure; nothing throws across
 *     the ABI.  infv_ltm_last_error() returns a thread-local description;
 *   - a handle is not re-entrant (the reference module is mutable, single-threaded state);
 *   - all floating-point data is fp32, row-major, batch size 1 (reference
 *     long_term_attention_gibbs.py:208,346); only the frame tokens may be fp16, bf16 or fp8 e4m3 (infv_ltm_set_token_dtype).
 */
#ifndef INFV_LTM_H
#define INFV_LTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INFV_LTM_ABI_VERSION 6
#define INFV_LTM_MAX_LAYERS 8

typedef enum {
    INFV_OK = 0,
    INFV_ERR_INVALID = -1,      /* bad argument / shape */
    INFV_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels implement */
    INFV_ERR_NO_PLAN = -3,      /* no plan registered for this chunk length */
    INFV_ERR_STATE = -4,        /* call not valid in the handle's current state */
    INFV_ERR_HIP = -5,          /* a HIP runtime call failed (see last_error) */
    INFV_ERR_NOMEM = -6
} infv_status;

typedef struct infv_ltm_s* infv_ltm_handle;

/* Constructor knobs = the kwargs the Q-former passes (Qformer.py:135-158) that the active
 * path reads, plus the frame-pooling shape the reference hard-codes
 * (long_term_attention_gibbs.py:291,304: 32 x 768; VideoChat2 twin: 196 x 1024). */
typedef struct {
    int32_t num_basis;         /* N, attn_num_basis                                    */
    int32_t n_heads;           /* H                                                    */
    int32_t head_size;         /* dh (64)                                              */
    int32_t d_in;              /* d, encoder width of the frame tokens                 */
    int32_t tokens_per_frame;  /* P                                                    */
    int32_t n_layers;          /* LTM instances stepped together by this handle (>=1)  */
    int32_t nb_samples;        /* S, 1..1024; the reference hard-codes 512 (long_term_attention_gibbs.py:55).  More than
                                  1024: INFV_ERR_UNSUPPORTED at create (the draw kernels hold the S slots in LDS).  Every
                                  entry point takes any S in range; infv_ltm_consolidate's fused chain takes S <= 512 and
                                  runs the per-chunk step above it (same results to fp32 rounding)       */
    int32_t sticky;            /* sticky_memories                                      */
    int32_t max_q;             /* largest query length that will be passed             */
    int32_t max_batch_chunks;  /* chunks pooled/projected per sub-batch by consolidate */
} infv_ltm_config;

/* Host-built tables for one chunk length T ("plan").  They are the sparse form of what
 * get_basis()/compute_G() rebuild on every forward (long_term_attention_gibbs.py:67-165):
 * with box basis functions F F^T is diagonal, so each row of G has one non-zero
 * 1/(count+ridge).  All pointers are HOST pointers; the call copies them to the device.
 *   rows:  for r in [0,rows): box row_box[r] receives val[box] * sum of frames
 *          [row_begin[r], row_end[r])                      ("new" coefficient rows)
 *   old:   CSR over boxes of the S resampled-memory slots that land in the box
 *          (infinite-memory operator only; positions tau*s/S, :137)                      */
typedef struct {
    int32_t T;
    int32_t first_rows;
    const int32_t* first_row_box;
    const int32_t* first_row_begin;
    const int32_t* first_row_end;
    const float*   first_box_val;     /* [N] */
    int32_t inf_rows;
    const int32_t* inf_row_box;
    const int32_t* inf_row_begin;
    const int32_t* inf_row_end;
    const float*   inf_box_val;       /* [N] */
    const int32_t* inf_old_ptr;       /* [N+1] */
    const int32_t* inf_old_slot;      /* [inf_old_ptr[N]] values in [0,S) */
    const float*   readout_w;         /* [N]  trapezoid weight of the 1000-point grid in box n (:264-282) */
    float          readout_w_out;     /* weight of grid points in no box (t = 1.0)          */
    int32_t        n_bins;            /* 128 (:163)                                          */
    const int32_t* edge_box;          /* [n_bins+1] box evaluated at each modified edge, -1 = none (:197-200) */
    const float*   edge_dx;           /* [n_bins]   fp32 spacing of the modified edges              */
    const int32_t* bin_box;           /* [n_bins]   box of the unmodified left edge of bin b (:207-208) */
    const int32_t* uniform_idx;       /* [S] non-sticky resample rows, -1 = zero row (:153-157,212)  */
} infv_ltm_plan;

/* Borrowed projection weights of one cross-attention layer (device pointers): the layer's
 * own key/value nn.Linear (Qformer.py:133-134,156-157), read at call time. */
typedef struct {
    const float* wk;   /* [dm, d] */
    const float* bk;   /* [dm]    */
    const float* wv;   /* [dm, d] */
    const float* bv;   /* [dm]    */
} infv_ltm_proj;

int         infv_ltm_abi_version(void);
const char* infv_ltm_last_error(void);

/* LongTermAttention.__init__ (long_term_attention_gibbs.py:26-65).  Refused HERE, before any device work (INFV_ERR_UNSUPPORTED /
 * INFV_ERR_INVALID, message in infv_ltm_last_error): head_size other than 64, num_basis that is no positive multiple of 16 (the
 * Python wrapper pads any other value), d_in that is no positive multiple of 32, n_heads < 1, tokens_per_frame < 1, nb_samples
 * outside 1..1024, n_layers outside 1..INFV_LTM_MAX_LAYERS, max_q < 1.  num_basis and max_q have no upper bound here; what the
 * suite has run is num_basis up to 512 and query lengths up to 384 (tests/golden/sweep_cases.py lists every swept shape).
 * infv_ltm_consolidate runs queries longer than 256 rows through the per-chunk step. */
int infv_ltm_create(const infv_ltm_config* cfg, infv_ltm_handle* out);
int infv_ltm_destroy(infv_ltm_handle h);

/* get_basis() (long_term_attention_gibbs.py:67-165), cached per chunk length. */
int infv_ltm_set_plan(infv_ltm_handle h, const infv_ltm_plan* plan);
int infv_ltm_has_plan(infv_ltm_handle h, int32_t T);          /* 1 / 0 */

/* Dense form of the operators of one chunk length, for num_basis values whose fp32 box bounds
 * (basis_functions.py:248-250) overlap or leave gaps at a sample position, histogram edge or resampling point: psi(t)
 * then has two ones, F F^T is not diagonal and G (long_term_attention_gibbs.py:68-84) has two non-zeros in some rows.
 * The host computes G with the reference's own fp32 sequence (F^T (F F^T + ridge I)^-1 via LAPACK, trimmed) and hands
 * it over transposed, together with the (up to two) boxes of every point the step evaluates psi at.  Registered IN
 * ADDITION to infv_ltm_set_plan for the same T (whose readout_w / edge_dx / n_bins stay in force; its one-box tables
 * are ignored).  With a dense plan every entry point runs the per-call step with dense kernels (update = x . G on fp32
 * MFMA); infv_ltm_consolidate loops over chunks.  All pointers are HOST pointers. */
typedef struct {
    int32_t T;
    int32_t first_K;                  /* rows of the first-chunk operator (= T)                       */
    const float*   first_GT;          /* [N][first_K]  G_first transposed                             */
    int32_t inf_K;                    /* rows of the infinite-memory operator (= S + T)               */
    const float*   inf_GT;            /* [N][inf_K]    G_inf transposed; rows 0..S-1 = resampled, then the T frames */
    const int32_t* bin_box2;          /* [n_bins][2]   boxes containing the unmodified left edge of bin b, -1 = none (:207-208) */
    const int32_t* edge_box2;         /* [n_bins+1][2] boxes containing each modified histogram edge (:197-200)      */
    const int32_t* uniform_box2;      /* [S][2]        boxes of the non-sticky resample positions (:153-157,212)     */
} infv_ltm_dense_plan;
int infv_ltm_set_dense_plan(infv_ltm_handle h, const infv_ltm_dense_plan* plan);

/* General-psi plan of chunk length T, on top of its dense plan: a basis family whose psi(t) is a dense row -- the reference's
 * GaussianBasisFunctions (basis_functions.py:135-164, built by add_gaussian_basis_functions,
 * long_term_attention_gibbs.py:167-174).  Besides the dense ridge operators (infv_ltm_set_dense_plan: compute_G :68-84) the
 * step then needs psi itself wherever the reference evaluates it (batch_evaluate / evaluate):
 *   psi_edge    at the modified histogram edges (update_inf :197-200 -> score :224-230): the sticky density
 *   psi_bin     at the unmodified left edge of every bin, ts = bins[b] (:207-208): the resampled rows B_past^T psi(ts)
 *   psi_uniform at the non-sticky resample positions (get_basis :153-157, used at :212)
 *   psi_grid    on linspace(0, 1, n_grid) with the trapezoid weights grid_w (expected_value :251-286): the read-out
 * Steps of that length take the per-call path with dense contractions for all of these (ltm_psi.hip).  All arrays are
 * host pointers, copied. */
typedef struct {
    int32_t T;
    int32_t n_grid;                   /* points of the read-out grid (1000, long_term_attention_gibbs.py:251) */
    const float* psi_edge;            /* [n_bins+1][N] */
    const float* psi_bin;             /* [n_bins][N]   */
    const float* psi_uniform;         /* [S][N]        */
    const float* psi_grid;            /* [n_grid][N]   */
    const float* grid_w;              /* [n_grid]      */
} infv_ltm_psi_plan;
int infv_ltm_set_psi_plan(infv_ltm_handle h, const infv_ltm_psi_plan* plan);

/* new_doc=True (long_term_attention_gibbs.py:300-302): forget the memory. */
int infv_ltm_reset(infv_ltm_handle h);
int infv_ltm_has_memory(infv_ltm_handle h);                    /* 1 / 0 */

/* Element type of the frame tokens `k` handed to pool / forward / consolidate.  The reference concatenates fp32
 * tensors (infinityqa.py:317-322), but their values come out of an fp16 producer: the ViT is .half() and the image
 * Q-former runs under fp16 autocast (blip2.py:37-43, infinityqa.py:256-259).  Four layouts are read in place:
 *   INFV_TOKENS_F32   4 bytes per element.
 *   INFV_TOKENS_F16   2 bytes per element and nothing lost: every fp16 value (subnormals included) is exact in fp32, it
 *                     is widened by the hardware conversion, and the sum, the division by P and everything after run
 *                     in fp32 in the same order -- every result has the bits of the fp32-token run on the same values.
 *   INFV_TOKENS_BF16  2 bytes per element; results differ from the fp32-token run only by the rounding of the tokens
 *                     themselves where the producer rounded them (2^-9 relative each, averaged over P tokens).
 *   INFV_TOKENS_F8E4M3  (code 4, declared below the enum) 1 byte per element: OCP FP8 e4m3fn, what torch.float8_e4m3fn holds
 *                     -- not e5m2, not the e4m3fnuz encoding, no scale factor.  fp8 is the CALLER's storage choice (e.g.
 *                     tokens.to(torch.float8_e4m3fn) when caching features): the library neither quantises nor scales nor
 *                     judges that choice.  Its contract is equality: each of the 254 finite codes is an exact fp32 number
 *                     (and exact in bf16), the two NaN codes 0x7F / 0xFF widen to NaN, the hardware conversion widens
 *                     them, and everything after runs in fp32 in the same order -- every result has the bits of the run on
 *                     the tokens widened to fp32.  `k` must be 16-byte aligned (INFV_ERR_INVALID before any launch).
 * Either half format halves the bytes of the only HBM-heavy stream of the path; fp8 quarters them; the pooled frames and everything after
 * stay fp32.  fp16 and bf16 tokens must be 16-byte aligned where the video Q-former reads them (infv_vqf.h).  Codes not
 * listed here (2 among them) are refused.  Default fp32; set before the first call that takes `k`. */
typedef enum { INFV_TOKENS_F32 = 0, INFV_TOKENS_BF16 = 1, INFV_TOKENS_F16 = 3 } infv_token_dtype;
#define INFV_TOKENS_F8E4M3 4   /* accepted wherever an infv_token_dtype code is; entry points take the code as int32_t */
int infv_ltm_set_token_dtype(infv_ltm_handle h, int32_t dtype);

/* Frame mean-pool, long_term_attention_gibbs.py:304:  k [n_frames, P, d] -> kbar [n_frames, d] (fp32). */
int infv_ltm_pool(infv_ltm_handle h, const void* k, int64_t n_frames, float* kbar, void* stream);

/* Frame mean-pool and the memory's new rows in one pass (what infv_ltm_consolidate runs per sub-batch): for each of
 * n_chunks chunks of T frames, R[c][r] = sum over the frames f of box row r of val_r * mean_P(k[c][f]) -- the rows
 * `G_inf^T`'s new-signal half contributes in update_inf (long_term_attention_gibbs.py:216 applied to the means of :304);
 * k [n_chunks, T*P, d], R [n_chunks, rows, d] fp32 with rows = infv_ltm_new_rows(h, T).  Same bits as infv_ltm_pool
 * followed by the per-row sums of infv_ltm_step.  Needs infv_ltm_set_plan(T) (sparse plans only). */
int infv_ltm_pool_rows(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T, float* R, void* stream);
int infv_ltm_new_rows(infv_ltm_handle h, int32_t T);           /* rows per chunk of the plan for T, or a negative error */

/* One consolidation step of all n_layers instances on one chunk, from pooled frames:
 * update_inf + proj_key/proj_value + expected_value (long_term_attention_gibbs.py:194-222,
 * 312-318).  kbar [T,d]; q [L,Q,dm]; proj[L]; u [L,S] float64 Gibbs uniforms (device;
 * may be NULL when the handle has no memory yet or is not sticky); ctx [L,Q,dm]. */
int infv_ltm_step(infv_ltm_handle h, const float* kbar, int32_t T, const float* q, int32_t Q,
                  const infv_ltm_proj* proj, const double* u, float* ctx, void* stream);

/* `n_chunks` consecutive consolidation steps with a DIFFERENT query per chunk (what a cross-attention layer
 * after the first sees: its query is self.query(hidden_states), Qformer.py:211, and hidden_states depend on the
 * chunk).  kbar [C,T,d]; q [C,L,Q,dm]; u [C,L,S] (rows of chunks that resample nothing are ignored; may be NULL
 * when not sticky); ctx [C,L,Q,dm].  The new-row projections of all chunks are batched into one GEMM; the
 * memory chain (draw, update, attend per chunk) stays sequential.  Equals C calls of infv_ltm_step. */
int infv_ltm_steps(infv_ltm_handle h, const float* kbar, int32_t n_chunks, int32_t T, const float* q, int32_t Q,
                   const infv_ltm_proj* proj, const double* u, float* ctx, void* stream);

/* The per-chunk loop with per-chunk queries: infv_ltm_consolidate's arguments except q [C,L,Q,dm].
 * reset if new_doc, pool every chunk (batched), infv_ltm_steps. */
int infv_ltm_consolidate_q(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T, const float* q,
                           int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                           void* stream);

/* LongTermAttention.forward (long_term_attention_gibbs.py:288-346) for all layers of the
 * handle on one chunk: reset if new_doc, pool, step.  k [T*P, d].  What the step would refuse (a null argument, Q outside (0, max_q],
 * no plan for T, a sticky step on a memory without u -- any chunk after the first of infv_ltm_consolidate_q --, no sticky
 * histogram, a partial forced draw on a dense plan, a latched device error) is refused BEFORE the reset and the pooling launch --
 * here, in infv_ltm_forward_into and in infv_ltm_consolidate_q: such a call launches no kernel and leaves the memory as it was. */
int infv_ltm_forward(infv_ltm_handle h, const void* k, int32_t T, const float* q, int32_t Q,
                     const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                     void* stream);

/* infv_ltm_forward for a caller that keeps the pooled frames: pool k (element type `token_dtype`, an infv_token_dtype) into the
 * caller's DEVICE buffer kbar [T,d] (long_term_attention_gibbs.py:304), then step from it (:306-346) -- infv_ltm_set_token_dtype +
 * infv_ltm_pool + infv_ltm_step behind ONE call (round 6: the drop-in module's steady-state forward was three ctypes calls; its
 * second cross-attention layer of the same chunk steps from the same kbar without pooling again).  No reset: new_doc is the
 * caller's infv_ltm_reset. */
int infv_ltm_forward_into(infv_ltm_handle h, const void* k, int32_t token_dtype, int32_t T, float* kbar, const float* q, int32_t Q,
                          const infv_ltm_proj* proj, const double* u, float* ctx, void* stream);

/* The per-chunk loop of the eval drivers (run_inference_inf_video_llama_nextqa.py:179-196)
 * with the LLM/Q-former stubbed: n_chunks chunks of T frames, k [C, T*P, d], the same
 * q [L,Q,dm] for every chunk, u [C,L,S], ctx [C,L,Q,dm].  new_doc applies to chunk 0.
 * Pooling and new-row projections are batched over chunks; the memory chain is sequential. */
int infv_ltm_consolidate(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T,
                         const float* q, int32_t Q, const infv_ltm_proj* proj, const double* u,
                         int32_t new_doc, float* ctx, void* stream);

/* infv_ltm_consolidate from frame means the caller already holds: kbar [C,T,d] fp32 instead of k.  Same results bit
 * for bit as infv_ltm_consolidate on tokens whose infv_ltm_pool output is kbar; the pooling stage and its stream drop
 * out.  The video Q-former's single pass over the frame tokens (split + transpose + mean, Qformer.py:236,278-291)
 * produces these means, so the tokens are not read a second time for the memory. */
int infv_ltm_consolidate_pooled(infv_ltm_handle h, const float* kbar, int32_t n_chunks, int32_t T,
                                const float* q, int32_t Q, const infv_ltm_proj* proj, const double* u,
                                int32_t new_doc, float* ctx, void* stream);

/* Several independent videos stepped together (ABI 6).  hs[V]: distinct handles with identical configuration (N, H, dh, d,
 * P, L, S, sticky, token dtype) and the SAME plan for T (identical tables in infv_ltm_set_plan: same tau and num_basis).  Chunks are PACKED: video v owns chunks [cu[v], cu[v+1]) of
 *   k   [cu[V], T*P, d]   (device, the handles' token dtype)
 *   u   [cu[V], L, S]     float64 (device; may be NULL when not sticky)
 *   ctx [cu[V], L, Q, dm] (device, output)
 * q [L,Q,dm] and proj[L] are shared by every video and chunk (infv_ltm_consolidate's contract).  cu is a HOST array [V+1].
 * new_doc = 1 resets every handle first; new_doc = 0 continues each handle's memory (every handle must hold one).  With
 * new_doc = 0, cu[v+1] == cu[v] leaves video v untouched.  Afterwards each handle is in the state that infv_ltm_consolidate on
 * its own chunks would have left it in, so export_state, get_draw, forward, ... keep working per video, and a handle with an
 * armed trace (infv_ltm_set_trace) records its chunks' draws.
 * The videos advance in lockstep, one chunk each per step: one launch per stage and step for all of them, a video index in every
 * grid, nothing reduced across videos -- a video's results do not depend on the rest of the batch.  Per video the arithmetic is
 * the per-call step's (infv_ltm_forward) except the new-row projection, which runs without split-K.  Shapes the lockstep kernels
 * do not take (dense or psi plans, N above 256 or not a multiple of 16, S above 1024) run each handle's infv_ltm_consolidate in
 * turn.  Everything is enqueued on `stream` (the video table travels in kernel arguments: no host buffer, capture-safe); no
 * host synchronisation except workspace growth of the first handle, which owns the workspaces (one step of up to 256 videos:
 * pooled frames, projected rows; more videos run in groups of 256).
 * Refusals (INFV_ERR_INVALID: bad cu, duplicate handle, mismatched configuration or plan, missing u; INFV_ERR_NO_PLAN; INFV_ERR_STATE:
 * new_doc = 0 on a handle without memory) leave every handle as it was. */
int infv_ltm_consolidate_videos(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const void* k, int32_t T, const float* q,
                                int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx, void* stream);

/* infv_ltm_consolidate_videos from frame means the caller already holds, with an optional query per chunk (additive in ABI 6;
 * the video Q-former's layers after the first query the memory with chunk-dependent hidden states, Qformer.py:211).
 *   kbar [cu[V], T, d]  fp32 (device, 16-byte aligned: read as float4): frame means (infv_ltm_pool of the tokens); the
 *                       handles' token dtype does not enter
 *   q    q_per_chunk = 0: [L, Q, dm] shared by every chunk;  q_per_chunk = 1: [cu[V], L, Q, dm], one per chunk (infv_ltm_steps)
 * Everything else -- handles, packed cu, u, ctx, new_doc, refusals, groups of 256 videos, the caller's stream only -- is
 * infv_ltm_consolidate_videos's contract.  The lockstep step copies each running video's kbar rows of the step into the call's
 * workspace (plain copies) where consolidate_videos pools tokens, and reads chunk c's query at q + c * L*Q*dm when q_per_chunk.
 * Bits:
 *   (a) q_per_chunk = 0 and kbar = infv_ltm_pool(k): ctx, B, bin masses and draws equal infv_ltm_consolidate_videos(k, q)'s;
 *   (b) a video's bits do not depend on the rest of the batch (which videos, their order, their lengths);
 *   (c) per video, the results agree with infv_ltm_consolidate_q on that handle to fp32 rounding (its projection may take
 *       split-K; this one never does), the draws apart from uniforms within rounding of a cdf edge.
 * Shapes the lockstep kernels do not take (dense or psi plans, N above 256 or not a multiple of 16) run each handle's
 * infv_ltm_steps (q_per_chunk = 1) or infv_ltm_consolidate_pooled (q_per_chunk = 0) in turn, after the reset when new_doc. */
int infv_ltm_steps_videos(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const float* kbar, int32_t T,
                          const float* q, int32_t q_per_chunk, int32_t Q, const infv_ltm_proj* proj,
                          const double* u, int32_t new_doc, float* ctx, void* stream);

/* infv_ltm_steps_videos with the frame means read through a per-video base (additive in ABI 6): several memories may step from
 * ONE block of frame means, as when several instructions are asked of one video (the VideoChat2 Q-former's queries, and so its
 * memories, depend on the instruction; the frames do not: videochat2_it_mistral.py:199-252).
 *   kbar_chunk0 [V]  HOST int32: chunk i of video v reads its frame means at kbar + (kbar_chunk0[v] + i) * T * d instead of at
 *                    chunk cu[v] + i.  Entries may repeat and come in any order; kbar must hold kbar_chunk0[v] + cu[v+1] - cu[v]
 *                    chunks for every v.  NULL: cu[v], which is infv_ltm_steps_videos itself.
 * u, q (q_per_chunk = 1) and ctx stay packed by cu.  A negative entry is refused (INFV_ERR_INVALID) before any handle changes;
 * everything else is infv_ltm_steps_videos's contract.  The new-row projection of a step is computed per video even where videos
 * share frame means.
 * Bits: those of infv_ltm_steps_videos on a kbar in which video v's chunks are copies of chunks kbar_chunk0[v].. (the lockstep
 * step gathers through the base; the per-handle fallback hands each handle the pointer at its base). */
int infv_ltm_steps_videos_from(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const float* kbar,
                               const int32_t* kbar_chunk0, int32_t T, const float* q, int32_t q_per_chunk, int32_t Q,
                               const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx, void* stream);

/* The lockstep calls for videos whose LAST chunk is short (additive in ABI 6).  The reference's drivers cut a video with
 * torch.split(video, n_frames, dim=1) (run_inference_inf_video_llama_nextqa.py:228): a video whose frame count is no multiple of T
 * ends in a chunk of fewer frames, which steps with the plan for ITS length.  One descriptor serves both forms of the call: frame
 * tokens (`k`, pooled per step: infv_ltm_consolidate_videos) or frame means (`kbar`, infv_ltm_steps_videos); exactly one is set.
 *   tail_T [V]  HOST int32: frames of video v's last chunk; 0 or T: a full chunk.  Ignored for a video with no chunk.
 * Layout.  k and kbar are packed by FRAME: video v has frames(v) = (len_v - 1) * T + tail(v) frames (len_v = cu[v+1] - cu[v], 0
 * without a chunk) and they start at frame sum_{w<v} frames(w): k is [sum frames, P, d], kbar [sum frames, d].  With no short
 * tail that is byte for byte the layout of the calls above.  u, ctx and a per-chunk q stay packed by CHUNK through cu.
 * Contract.  Per video, every output and every piece of handle state equals BIT FOR BIT what two of the calls above leave:
 *   infv_ltm_consolidate_videos (k) or infv_ltm_steps_videos (kbar) on the video's full chunks, then the same entry point with
 *   new_doc = 0 and T = tail(v) on its last chunk (with the call's new_doc if that chunk is the video's only one)
 * -- ctx, B and K'/V', the sticky bin partials, probs / bins / idx / scores of the last step (infv_ltm_get_draw), the rows of an
 * armed draw trace and of the lead's packed mass trace, the rng position and what the handle remembers of its last step (its plan
 * is the one for tail(v)).  A video's bits do not depend on the rest of the batch.  Everything is enqueued on hip_stream; no host
 * buffer outlives the call (the per-video frame counts travel in kernel arguments beside the video table, the operator of a short
 * chunk is read from its plan on the device).
 * A step is still five launches (six with the packed mass trace) whatever mix of tail lengths it holds: pooling / gather, the
 * new-row projection and the update take the frames and the operator per video; the draw, the attend and the box masses do not
 * depend on T.  The projected-row workspace holds, per video, the most rows of any plan involved rounded up to 64.
 * Shapes the lockstep kernels do not take (a dense or psi plan for T or for any tail length, N above 256 or not a multiple of 16,
 * S above 1024) run per handle: infv_ltm_consolidate / infv_ltm_steps / infv_ltm_consolidate_pooled on the full chunks, then one
 * chunk at the tail length.
 * The stream is a FIELD of the descriptor, not a `void* stream` parameter, as in infv_ltm_sources_videos_desc and for its reason
 * (tests/golden/stream_cases.py lists every function that declares such a parameter); this call's stream-order scenario lives in
 * tests/test_videos_tail_gpu.py.
 * Refused before any handle changes (the resets of new_doc included): a null descriptor or tail_T; both k and kbar, or neither;
 * tail_T[v] outside {0} and [2, T] (a chunk of one frame has an empty operator, LTM.py:79-82); a handle without a plan for its
 * tail length (INFV_ERR_NO_PLAN); handles that share a tail length but whose plans for it differ; a tail plan that differs from the
 * plan for T in a table that does not depend on the chunk length (read-out weights, sticky histogram, uniform resampling table);
 * reserved != 0; and everything infv_ltm_consolidate_videos / infv_ltm_steps_videos refuse.  kbar_chunk0 is not offered here. */
typedef struct {
    const infv_ltm_handle* hs;   /* HOST [V] */
    int32_t V;
    int32_t T;                   /* frames of a full chunk */
    const int32_t* cu;           /* HOST [V+1], in chunks, as the lockstep calls take it */
    const int32_t* tail_T;       /* HOST [V] */
    const void*    k;            /* DEVICE [sum frames, P, d] in the handles' token dtype, or NULL */
    const float*   kbar;         /* DEVICE [sum frames, d] fp32, 16-byte aligned, or NULL */
    const float*   q;            /* DEVICE [L, Q, dm], or [cu[V], L, Q, dm] with q_per_chunk */
    int32_t q_per_chunk;         /* 0 / 1 */
    int32_t Q;
    const infv_ltm_proj* proj;   /* HOST [L] */
    const double*  u;            /* DEVICE [cu[V], L, S] or NULL */
    int32_t new_doc;
    int32_t reserved;            /* 0 */
    float*         ctx;          /* DEVICE [cu[V], L, Q, dm], output */
    void*          hip_stream;   /* the stream of every launch (see above) */
} infv_ltm_videos_tail_desc;
int infv_ltm_videos_tail(const infv_ltm_videos_tail_desc* d);

/* The hand-over payload of a consolidate call in ONE kernel launch: everything a peer needs from this handle after
 * infv_ltm_consolidate, as one fp32 DEVICE buffer
 *   B [L][n_basis][d] | sticky bin masses [L][n_bins-1] | (with_scores: bias-free scores [L][H][Q][n_basis]) |
 *   ctx_sum [L][Q][dm] | count
 * -- the first n_basis (<= num_basis) rows / columns of the handle's padded basis; B and the masses are the bits of
 * infv_ltm_export_state, the scores those of the blob of infv_ltm_export_chain_state, count = (float)n_chunks, and ctx_sum is
 * the sum over the call's chunks of ctx [n_chunks][L][Q][dm].  The call refuses where infv_ltm_export_state would, and with
 * with_scores where infv_ltm_export_chain_state would.  Asynchronous on `stream`, which must be the consolidate call's.
 * ctx_sum, order of the fp32 additions.  With infv_ltm_set_ctx_sum(h, 1) the update + read-out kernels of a fused
 * infv_ltm_consolidate / _pooled call with Q <= 32 add up the values they store, and pack_memory only copies the result:
 *   sum = (...((0 + S_0) + S_1) + ...) over the call's update + read-out launches in launch order; S_b is the left-to-right sum of
 *   launch b's chunks, starting from the first one.  Launch 0 is the document's first chunk when the call starts a document;
 *   the sub-batches follow (max_batch_chunks chunks each, 32 for calls under 768 chunks, the last one shorter).
 * That sum is valid for exactly the (ctx, n_chunks, Q) of the call that produced it, until any entry point steps, resets or
 * imports the memory.  In every other case -- sums off, the chunk-by-chunk path (dense / psi plans, shapes the fused chain does
 * not hold), another ctx -- one extra launch adds ctx up first:
 *   left-to-right sums over blocks of 64 consecutive chunks, each from 0, then the block sums left to right from 0.
 * The two orders agree to fp32 rounding, not bit for bit. */
int infv_ltm_set_ctx_sum(infv_ltm_handle h, int32_t on);
int infv_ltm_pack_memory(infv_ltm_handle h, int32_t n_basis, int32_t Q, const float* ctx, int32_t n_chunks, int32_t with_scores,
                         float* payload, void* stream);

/* Consolidated memory of one layer: B_past [N,d] (long_term_attention_gibbs.py:220) and the
 * unnormalised sticky bin masses p[n_bins-1] derived from the last scores (:200-202).
 * Export copies device -> caller's DEVICE buffers (async on stream). */
int infv_ltm_export_state(infv_ltm_handle h, int32_t layer, float* B, float* bin_mass, void* stream);
/* Import + recompute the projected memory with the given weights. */
int infv_ltm_import_state(infv_ltm_handle h, int32_t layer, const float* B, const float* bin_mass,
                          const infv_ltm_proj* proj, void* stream);
/* Exact hand-off of the memory chain between handles (multi-GPU correctness mode: rank r continues where rank r-1
 * stopped, reference semantics of one process walking the whole video, long_term_attention_gibbs.py:194-222).
 * The blob is a 64-byte header (magic, version, L, N, d, dm, H, Q, n_bins as int32) and everything infv_ltm_consolidate
 * carries from chunk to chunk, in fp32:
 *   B [L][N][d] | projected memory [L][N][2][dm] | bias-free scores under the call's query [L][H][Q][N] | sticky bin
 *   masses [L][n_bins] | key-bias term of those scores [L][H][Q] (q_h . b_k,h / sqrt(dh): what infv_ltm_density, infv_ltm_masses
 *   and the scores of infv_ltm_get_draw add back on the importing side)
 * so a consolidate call that follows an import (new_doc = 0) continues BIT FOR BIT as if the exporting handle had gone on
 * itself -- unlike export_state/import_state, which hand over B and the masses only and re-derive the rest (same values up
 * to fp32 rounding).  Conditions, none of which the library can check for the caller: the SAME q and proj on both sides (the
 * blob carries the scores under the exporter's query), and blocks that do not end in a short sub-batch -- a sub-batch of
 * fewer than 1024 new rows (16 chunks at the headline shape) takes the split-K form of the projection, whose sums are
 * ordered differently (same values to fp32 rounding, not the same bits; tests/test_sharding_gpu.py cuts 129 chunks as 65 + 64).
 * import checks the header on the device: a blob of another shape latches an error that the next entry point returns as
 * INFV_ERR_STATE (the memory is reset).  export needs a memory whose last step ran in infv_ltm_consolidate with query
 * length Q; blob = DEVICE buffer of infv_ltm_chain_state_bytes(h, Q) bytes; both are asynchronous on `stream`. */
int64_t infv_ltm_chain_state_bytes(infv_ltm_handle h, int32_t Q);
int infv_ltm_export_chain_state(infv_ltm_handle h, int32_t Q, void* blob, void* stream);
int infv_ltm_import_chain_state(infv_ltm_handle h, int32_t Q, const void* blob, void* stream);
/* Recompute projected memory of every layer from B (weights changed since the last step). */
int infv_ltm_reproject(infv_ltm_handle h, const infv_ltm_proj* proj, void* stream);

/* Diagnostics of the last step of one layer, copied to HOST buffers (synchronises stream):
 * bins [S] drawn histogram bins, idx [S] resampled rows, probs [n_bins-1] as fed to the draw,
 * scores [H,Q,N] (any pointer may be NULL). */
int infv_ltm_get_draw(infv_ltm_handle h, int32_t layer, int32_t* bins, int32_t* idx, float* probs,
                      float* scores, void* stream);
/* Teacher forcing for tests: the next step of `layer` draws from these HOST probs[n_bins-1]
 * instead of the ones derived from its own scores (one-shot).  No stream argument: this setter and infv_ltm_set_bins synchronise
 * the device, then copy -- steps already queued on any stream keep the override they were issued under (see Conventions). */
int infv_ltm_set_probs(infv_ltm_handle h, int32_t layer, const float* probs);
/* Forced draw (one-shot, per-call step/forward only): the next step of `layer` resamples the
 * rows of these HOST bins[S] (values in [0, n_bins-1)) instead of its own draw.  The step still
 * derives its own probabilities and draw; infv_ltm_get_draw then returns the step's OWN bins
 * next to the idx actually used, so a long chain can be compared draw by draw with another path
 * without the two diverging at the first uniform that falls within rounding of a cdf edge. */
int infv_ltm_set_bins(infv_ltm_handle h, int32_t layer, const int32_t* bins);
/* Draw trace of infv_ltm_consolidate: while set, chunk c of a call (c < capacity_chunks) writes
 * the bins it drew to bins_all[c][L][S] and its probabilities to probs_all[c][L][n_bins]
 * (DEVICE buffers owned by the caller, either may be NULL; rows of a document's first chunk,
 * which draws nothing, are left untouched).  capacity_chunks = 0 clears the trace. */
int infv_ltm_set_trace(infv_ltm_handle h, int32_t* bins_all, float* probs_all, int64_t capacity_chunks);

/* ---- Read-outs of the memory's attention density (additive in ABI 6) ----
 * The reference's Video-LLaMA operator evaluates, on every forward, the density of the step it just took on a 768-point grid and
 * pickles it to ./alphas_uniform (long_term_attention_gibbs.py:320-343; relevant_frames.py reads that file).  Neither read-out
 * below is on a default path: with no trace set and no density call, no entry point launches, records or allocates anything more
 * than before.  General-psi plans (infv_ltm_set_psi_plan) have no box density: all four calls refuse a handle that holds one
 * (INFV_ERR_UNSUPPORTED), and infv_ltm_set_psi_plan refuses a handle with a grid plan or a trace set.  Sparse and dense box plans
 * are taken.
 *
 * The grid (:328-334: three torch.linspace segments of 256 points) as host tables, copied: n_points M <= 4096 in n_segments
 * G <= 16 consecutive segments, segment g = points [seg_begin[g], seg_begin[g+1]) (at least two each); pt_weight[m] the
 * trapezoid weight of point m inside its own segment (torch.trapz, :248, over the fp32 grid values); and psi at every point as a
 * CSR over boxes: entries [pt_ptr[m], pt_ptr[m+1]) of pt_box / pt_val.  A box partition gives one entry of value 1, a point where
 * two fp32 boxes overlap (num_basis 96, ...) two, a point in no box (t = 1.0) none.  s(t_m) = sum of pt_val * S[pt_box] is added
 * in CSR order in fp32.  Refused with INFV_ERR_INVALID before any device work: null tables, M outside [2, 4096], G outside
 * [1, 16], seg_begin not running from 0 to M or a segment of fewer than two points, pt_ptr not starting at 0 or not monotone,
 * a pt_box outside [0, num_basis), a weight that is negative or not finite, a value that is not finite, num_basis + M above
 * 16384 (a wave keeps the score row and the grid in LDS). */
typedef struct {
    int32_t n_points;
    int32_t n_segments;
    const int32_t* seg_begin;         /* [n_segments+1] */
    const float*   pt_weight;         /* [n_points]     */
    const int32_t* pt_ptr;            /* [n_points+1]   */
    const int32_t* pt_box;            /* [pt_ptr[n_points]] */
    const float*   pt_val;            /* [pt_ptr[n_points]] */
} infv_ltm_grid_plan;
int infv_ltm_set_grid_plan(infv_ltm_handle h, const infv_ltm_grid_plan* plan);

/* The reference's `alphas` (:328-337) of the memory's LAST step, one layer: with S[h,q,n] the step's full scores (key-bias term
 * included: a grid point in no box enters as exp(0)) and s(t) as above,
 *     e = exp(s - max of s over the point's segment);  z_g = sum over segment g of pt_weight * e;  dens = e / z_g;
 *     alphas[q][h][m] = dens_m / sum_m' dens_m'
 * written to the DEVICE buffer alphas [Q][H][M] -- the [Q, 1, H, M] of the permute at :337.  (The reference subtracts no
 * maximum, :248, and overflows where this does not; dens is normalised inside a segment, so the segment's own maximum keeps it in range.)  One launch on `stream`: a wave per (h, q) row, exp is expf, the sums run in
 * float64.  Works after every single-handle entry point that leaves a memory: step, steps, forward, forward_into, consolidate,
 * consolidate_pooled, consolidate_q, import_chain_state -- and after the lockstep calls.  INFV_ERR_STATE: no memory, no grid plan,
 * a Q other than the last step's, or after infv_ltm_import_state, which keeps no scores. */
int infv_ltm_density(infv_ltm_handle h, int32_t layer, int32_t Q, float* alphas, void* stream);

/* What the read-out of the last step actually used, one layer: mass[n] = mean over (h, q) of alpha[h,q,n] with
 * alpha[h,q,n] = w_n e^{S_n} / (sum_m w_m e^{S_m} + w_out), the `integral` of expected_value (:282); w and w_out are the plan's
 * readout_w and readout_w_out.  mass: DEVICE [num_basis].  One launch; same conditions and refusals as infv_ltm_density except
 * that no grid plan is needed; num_basis above 512 is INFV_ERR_UNSUPPORTED.
 * Order of the sum over the H*Q rows r = h * Q + q (both this call and the trace below): eight partial sums, partial k adds rows
 * k, k + 8, k + 16, ... in increasing order from 0; the partials are added in order 0..7 from 0; the total is multiplied by
 * 1 / (H*Q).  All in float64, rounded to fp32 once -- so the order is part of the description, not of the result. */
int infv_ltm_masses(infv_ltm_handle h, int32_t layer, int32_t Q, float* mass, void* stream);

/* Box-mass trace of the multi-chunk calls, modelled on infv_ltm_set_trace: while set, chunk c < capacity_chunks of an
 * infv_ltm_steps / infv_ltm_consolidate / infv_ltm_consolidate_pooled / infv_ltm_consolidate_q call writes the masses of its
 * step, every layer, to mass_all[c][L][num_basis] (DEVICE buffer owned by the caller).  Every chunk writes, a document's first
 * included; rows at and beyond capacity_chunks are not touched; capacity_chunks = 0 clears the trace.  The single-chunk calls
 * (step, forward, forward_into) leave the trace alone: read them with infv_ltm_masses.
 * Added launches while set, none otherwise: the fused chain of consolidate / consolidate_pooled adds exactly ONE per update +
 * read-out launch -- one per sub-batch, plus one for a document's first chunk, which is a launch of its own -- on the stream of
 * those launches, behind the sub-batch's softmax weights and ahead of the reuse of their ring slots; it reads the weights the
 * update + read-out kernel reads.  The per-chunk stages (steps, consolidate_q, and consolidate where it runs them: dense plans,
 * shapes the fused chain does not hold) add exactly ONE per chunk, from the chunk's full scores: there the last row has the
 * bits of infv_ltm_masses called afterwards.  No existing kernel changes, no event or allocation is added.
 * infv_ltm_consolidate_videos, infv_ltm_steps_videos and infv_ltm_steps_videos_from refuse a handle with a trace set
 * (INFV_ERR_UNSUPPORTED before any device work, every memory untouched; their own trace is the packed one of
 * infv_ltm_set_videos_mass_trace below).  The video Q-former drives these same handles:
 * infv_vqf_encode_video steps each layer's handle with infv_ltm_consolidate / _pooled / infv_ltm_steps (infv_vqf.h), so a trace
 * set on a layer's handle is honoured by it without further work; its batched calls run the lockstep entry points and refuse. */
int infv_ltm_set_mass_trace(infv_ltm_handle h, float* mass_all, int64_t capacity_chunks);

/* Packed box-mass trace of the LOCKSTEP calls (additive in ABI 6) -- a call-level trace with its own setter; the refusal above
 * stays.  While set, every infv_ltm_consolidate_videos / infv_ltm_steps_videos / infv_ltm_steps_videos_from call whose handle 0
 * is `lead` writes mass_all[c][L][num_basis] (DEVICE buffer owned by the caller) for every packed chunk c < capacity_chunks,
 * where c indexes the call's packed arrays exactly as ctx does: chunk i of video v is row cu[v] + i, whatever the number of
 * videos (calls of more than 256 run in groups; the row index does not depend on group or rank).  Every chunk writes, a video's
 * first included; rows at and beyond the capacity are not touched; capacity_chunks = 0 clears the trace.
 * ONE added launch per lockstep step while set, none otherwise (a workgroup per 64 columns, layer and video still running, 8
 * waves), issued directly behind the step's attend launch on the call's stream: it reads each video's full score rows, key bias
 * included, which stream order protects from the next step's attend.  The per-row arithmetic and the order of the sums are those
 * stated at infv_ltm_masses, so the last row of each video has the bits of infv_ltm_masses called on that video's handle after
 * the call, and a video's rows do not depend on what else is in the batch.  No existing kernel changes.
 * Shapes the lockstep kernels do not take (dense plans, num_basis above 256, ...) run each video's own per-call path; there the
 * trace is served through that path's per-chunk trace on the video's slice mass_all + cu[v] * L * num_basis with the capacity
 * that remains, so the rows have the bits infv_ltm_set_mass_trace would have given that video's own call.
 * Refusals, before any device work, every memory untouched: by the setter, a handle with a general-psi plan or num_basis above
 * 512 (INFV_ERR_UNSUPPORTED, as infv_ltm_set_mass_trace), a negative capacity or a NULL buffer with a positive one
 * (INFV_ERR_INVALID); by the lockstep calls, a handle other than hs[0] that carries a videos trace (INFV_ERR_INVALID: a trace
 * that would silently stay empty is worse than a refusal); infv_ltm_set_psi_plan refuses a handle with a videos trace set.
 * The batched video Q-formers (infv_vqf_encode_videos, infv_vqf_vc_encode_videos*, infv_vqf_vc_encode_streams*,
 * infv_vqf_vc_encode_img) drive these same entry points with video 0's handle of the layer as handle 0, so a trace set on that
 * handle is honoured by them without further work. */
int infv_ltm_set_videos_mass_trace(infv_ltm_handle lead, float* mass_all, int64_t capacity_chunks);

/* ---- Source weights: the memory traced back to its frames (additive in ABI 6) ----
 * The masses above say how much the read-out attends to each BASIS FUNCTION.  The reference's relevant_frames.py:53-69 turns that
 * into frames by taking grid point m of segment i of `alphas` for frame m + 256 * i of the video -- right only for a memory that
 * was never consolidated: after the first sticky update every basis function mixes resampled older content with new frames.
 * The update is linear in the frame means (long_term_attention_gibbs.py:207-216 in closed form: B_new[n] = val[n] * (sum of the
 * resampled old rows of box n + sum of its new frames)), so there is a W with B[n] = sum over sources of W[n][source] *
 * kbar[source], and W obeys the same recurrence with one-hot rows in place of the frame means.
 * Columns of W are SOURCES: groups of g = frames_per_source consecutive frames (g >= 1, g divides T).  Frame f of chunk c of the
 * call belongs to column col_begin + (c * T + f) / g.  For one layer and chunk c, W_old being the matrix before the chunk:
 *   first chunk of a document (new_doc and c == 0):
 *       W_new[n][m] = first_box_val[n] * cnt_first(n, m)
 *     cnt_first = number of frames of box n's [first_row_begin, first_row_end) whose column is m; every column below col_begin
 *     becomes 0 (the document's memory was reset);
 *   otherwise, with idx[s] = bin_box[bins[c][l][s]] on a sticky handle and uniform_idx[s] on others:
 *       acc = 0
 *       for s in inf_old_slot[inf_old_ptr[n] : inf_old_ptr[n+1]], in stored order:
 *           if idx[s] >= 0: acc += W_old[idx[s]][m]
 *       acc += float(cnt_inf(n, m))          -- the box's new frames that fall in column m, added LAST as one fp32 number
 *       W_new[n][m] = inf_box_val[n] * acc
 * This order is part of the contract: fp32 additions in that order and one multiplication, nothing an FMA could contract;
 * density.source_weights(dtype=float32) restates it in numpy and equals the device bit for bit.  Boxes with no rows and the pad
 * basis functions of a padded num_basis keep W = 0.
 * A bin outside [0, n_bins - 1) -- an unwritten trace row holds -1 -- is never used as an index: it resamples a zero row.
 * bad_bins[l] (if given) is increased by the number of such bins among the S bins of every resampling chunk of layer l (every
 * chunk but a document's first), counted once per layer whatever the number of columns; the caller zeroes it.
 * With mass_all (the trace infv_ltm_set_mass_trace wrote during the same call) the pass also writes the attention map of the
 * video while it holds W_c, the matrix after chunk c:
 *       attn_all[c][l][m] = sum_n mass_all[c][l][n] * W_c[n][m]
 * accumulated in float64 (eight partial sums on num_basis <= 256, sixteen above: partial k adds rows k, k + 8 (16), ... in
 * increasing order; the partials are added in order from 0) and rounded once.  It is raw, not normalised: rows do not sum to 1
 * because of the ridge and readout_w_out.
 *   bins_all   DEVICE [C][L][S], the layout infv_ltm_set_trace writes -- which the fused chain, the per-chunk stages and the
 *              lockstep calls all fill; NULL iff the handle is not sticky
 *   W          DEVICE [L][num_basis][ld], 16-byte aligned, in/out: columns < col_begin are read unless new_doc; columns
 *              [col_begin, col_begin + C * T / g) need no initialisation; columns beyond are not touched
 *   mass_all   DEVICE [C][L][num_basis] or NULL;  attn_all DEVICE [C][L][ld] or NULL (NULL iff mass_all is NULL): every column
 *              below col_begin + C * T / g of every chunk is written, the rest not touched
 * ONE launch on `stream`: a workgroup per (tile of 64 columns -- 32 when num_basis > 256 --, layer) keeps its slice of W in LDS
 * over the whole call.  It reads nothing of the handle but the plan tables for T, and neither reads nor changes the memory.
 * Carrying W and col_begin + C * T / g from one call into the next equals one call over all the chunks, bit for bit.
 * Refused before any device work, nothing written -- INFV_ERR_INVALID: null descriptor or W, C < 1, g < 1 or g not dividing T,
 * negative col_begin, ld below col_begin + C * T / g or no multiple of 4, W not 16-byte aligned, bins_all NULL on a sticky handle
 * (or given on another), exactly one of mass_all / attn_all; INFV_ERR_STATE: no plan registered for T; INFV_ERR_UNSUPPORTED: a
 * dense or general-psi plan for T (they resample psi-combinations of two boxes through a dense operator: another kernel), or
 * num_basis above 512. */
typedef struct {
    int32_t n_chunks;           /* C >= 1 */
    int32_t T;                  /* frames per chunk */
    int32_t new_doc;            /* chunk 0 starts a document */
    int32_t frames_per_source;  /* g */
    int64_t col_begin;          /* column of the call's first source */
    int64_t ld;                 /* row stride of W and attn_all in floats: multiple of 4, >= col_begin + C*T/g */
} infv_ltm_sources_desc;
int infv_ltm_source_weights(infv_ltm_handle h, const infv_ltm_sources_desc* d, const int32_t* bins_all, float* W,
                            const float* mass_all, float* attn_all, int32_t* bad_bins, void* stream);

/* The source weights of MANY videos in one launch (additive in ABI 6): the pass above over the packed bins and masses of a
 * lockstep call.  Every video is a new document with col_begin = 0 (continuing a document stays the single-video call's job).
 * For every video v of len_v = cu[v+1] - cu[v] chunks and M_v = len_v * T / g columns, W_all[v] equals bit for bit what
 * infv_ltm_source_weights writes for that video's slice of the packed arrays (new_doc = 1, col_begin = 0, the same ld), and its
 * rows [cu[v], cu[v+1]) of attn_all equal that call's attn_all bit for bit; columns at and beyond M_v are not touched, and a video
 * with no chunk writes nothing.  bad_bins[l] is increased by the count over all videos.  `h` supplies only the plan tables for T.
 * The packed bins come for free: the draw trace is per handle and indexed by step, so infv_ltm_set_trace(h_v, bins + cu[v]*L*S,
 * probs + cu[v]*L*n_bins, len_v) on every handle makes a lockstep call fill one packed [cu[V]][L][S] tensor; the packed masses
 * are infv_ltm_set_videos_mass_trace's.
 * ONE launch for up to 512 videos (ceil(V / 512) launches beyond): grid (tiles of the longest video, L, videos); workgroup
 * (tile, l, v) walks chunks [cu[v], cu[v+1]) and returns at once when its tile starts at or beyond M_v.  cu is read on the host
 * during the call and travels in the kernel's arguments: nothing is copied to the device, nothing outlives the call, and the call
 * may be captured.
 * The stream is a FIELD of the descriptor, not a `void* stream` parameter, on purpose: the table of stream-order cases
 * (tests/golden/stream_cases.py) lists every function that declares such a parameter; this call's stream-order scenario lives in
 * tests/test_videos_trace_gpu.py instead.  Do not move it into the parameter list.
 * Refused before any device work, nothing written: everything infv_ltm_source_weights refuses (g, ld below the longest video's
 * columns or no multiple of 4, alignment of W_all, the sticky / bins_all pairing, the mass_all / attn_all pairing, no plan for T,
 * a dense or general-psi plan for T, num_basis above 512), and INFV_ERR_INVALID for a null descriptor, cu or W_all, V < 1, cu not
 * non-decreasing from a non-negative start, cu[V] = 0, reserved != 0. */
typedef struct {
    int32_t n_videos;            /* V >= 1 */
    int32_t T;                   /* frames per chunk */
    int32_t frames_per_source;   /* g >= 1, divides T */
    int32_t reserved;            /* 0 */
    int64_t ld;                  /* row stride of W_all and attn_all in floats: multiple of 4, >= max_v len_v * T / g */
    const int32_t* cu;           /* HOST [V+1], as the lockstep calls take it */
    const int32_t* bins_all;     /* DEVICE packed [cu[V]][L][S]; NULL iff the handle is not sticky */
    float*         W_all;        /* DEVICE [V][L][num_basis][ld], 16-byte aligned */
    const float*   mass_all;     /* DEVICE packed [cu[V]][L][num_basis] or NULL */
    float*         attn_all;     /* DEVICE packed [cu[V]][L][ld] or NULL (NULL iff mass_all is NULL) */
    int32_t*       bad_bins;     /* DEVICE [L] or NULL, summed over videos */
    void*          hip_stream;   /* the stream of the launch (see above) */
} infv_ltm_sources_videos_desc;
int infv_ltm_source_weights_videos(infv_ltm_handle h, const infv_ltm_sources_videos_desc* d);

/* Synchronises `stream`, then reports a latched device-side failure (see Conventions). */
int infv_ltm_sync(infv_ltm_handle h, void* stream);

/* Measurement (bench.py's roofline leg): while enabled, every kernel launch the handle issues
 * is bracketed by HIP events on the launch stream.  profile_read synchronises, returns the
 * number of launches and their summed device time for one kernel family, and clears it. */
typedef enum {
    INFV_KERNEL_POOL = 0,     /* frame mean-pool (the HBM-bound kernel)   */
    INFV_KERNEL_ROWS = 1,     /* new coefficient rows                     */
    INFV_KERNEL_PROJECT = 2,  /* fp32 MFMA projection GEMM                */
    INFV_KERNEL_DRAW = 3,     /* Gibbs draw                               */
    INFV_KERNEL_UPDATE = 4,   /* memory update                            */
    INFV_KERNEL_ATTEND = 5,   /* scores / softmax / read-out              */
    INFV_KERNEL_SCORES = 6,   /* batched new-row scores (fast path)       */
    INFV_KERNEL_CHAIN = 7,    /* per-chunk chain step: draw, score recurrence, softmax weights (fast path) */
    INFV_KERNEL_UC = 8,       /* state update + read-out of a sub-batch (fast path) */
    INFV_KERNEL_COUNT = 9
} infv_kernel;
int infv_ltm_profile_enable(infv_ltm_handle h, int32_t on);
int infv_ltm_profile_read(infv_ltm_handle h, int32_t kernel, int64_t* launches, double* total_ms);
/* Kernel launches this library has issued in this process so far (every handle, both headers' entry points): a
 * benchmark reads it before and after a call to state "launches per chunk".  Host-side counter, no device work. */
int64_t infv_ltm_launch_count(void);

/* ---- Device rng for the Gibbs uniforms (additive in ABI 6) ----
 * The reference samples the sticky memory with torch.rand(nb_samples) on the memory's device
 * (long_term_attention_gibbs.py:204-206); on its CUDA deployment that is torch's Philox device generator.  With the rng on, every
 * entry point that takes `u` accepts u == NULL on an existing sticky memory and the kernels generate the uniforms themselves,
 * in registers, with a counter-based Philox4x32-10 (csrc/philox.h) -- no more launches than with explicit u.  (The reference's
 * second nb_samples uniforms, :206, place the sample inside the drawn bin; they are degenerate and not generated.)
 *   key = (seed & 0xffffffff, seed >> 32)
 *   ctr = (s >> 1, layer, pos, stream_id)      s: sample slot in [0, S); layer: index inside the handle
 *   one block (w0, w1, w2, w3) serves two slots: u[s even] = u53(w0, w1), u[s odd] = u53(w2, w3)
 *   u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53, a double in [0, 1)
 * pos is the number of steps the handle has taken since its last reset: the index of the chunk within the document.  The first
 * chunk of a document has pos = 0 and draws nothing.  pos advances on EVERY step of every entry point, explicit-u steps included;
 * infv_ltm_reset and new_doc set it to 0.  A video's draws therefore depend only on (seed, stream_id) and its own content, not
 * on what the handle or the process did before.  infv_ltm_import_state / infv_ltm_import_chain_state leave pos alone: a caller
 * who continues a document on another handle sets it with infv_ltm_set_rng_position.  The chain-state blob does not carry it.
 * Precedence: a non-NULL u is always used as given (same bits as with the rng off); NULL u with the rng on is generated; NULL u
 * with the rng off is refused as before.  The multi-handle calls (infv_ltm_consolidate_videos, infv_ltm_steps_videos) need the
 * rng on for EVERY handle when u is NULL (INFV_ERR_INVALID before any handle changes); each handle draws from its own
 * (seed, stream_id) at its own position.  One-layer handles that stand for the layers of one model (infv_vqf_*) are told apart
 * by their stream_id, since `layer` is 0 for each.
 * pos travels in the launch arguments, so a captured graph replays the position it was captured with.
 * on = 0 restores the default (the seed and stream are kept but unused).  set_rng touches neither the memory nor pos. */
int infv_ltm_set_rng(infv_ltm_handle h, int32_t on, uint64_t seed, uint32_t stream_id);
int infv_ltm_get_rng_position(infv_ltm_handle h, uint32_t* pos);
int infv_ltm_set_rng_position(infv_ltm_handle h, uint32_t pos);
/* The uniforms the kernels would generate for steps pos0 .. pos0 + n_steps - 1 (pos wraps at 2^32) of a handle of n_layers layers
 * and S samples: u [n_steps][n_layers][S] float64, written to a DEVICE buffer by one launch on `stream` ... */
int infv_ltm_rng_fill(uint64_t seed, uint32_t stream_id, uint32_t pos0, int32_t n_steps, int32_t n_layers, int32_t S,
                      double* u_device, void* stream);
/* ... or to a HOST buffer by the CPU, from the same header, with no device work: feeding them back as explicit u (or to a CPU
 * reference) replays a device-rng run draw for draw. */
int infv_ltm_rng_fill_host(uint64_t seed, uint32_t stream_id, uint32_t pos0, int32_t n_steps, int32_t n_layers, int32_t S,
                           double* u_host);

#ifdef __cplusplus
}
#endif
#endif /* INFV_LTM_H */
