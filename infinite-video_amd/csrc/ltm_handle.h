// Private to the LTM host units (ltm_capi.hip: create / plans / per-call path / lockstep multi-video calls / rng / state;
// ltm_consolidate.hip: the whole-video fast path): the handle, what a plan uploads, and the checks they share.
#pragma once
#include "../../include/infv_ltm.h"
#include "ltm_internal.h"
#include "capi_common.h"
#include "ltm_memory_state.h"
#include "vqf_internal.h"

#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace infv {

// Timing experiments only (results become garbage): INFV_SKIP bit 0 = no pooling launches, bit 1 = no projection GEMM,
// bit 2 = no UC launches, bit 3 = no role-S launches.  Shows how much each stream slows the others.
inline int skip_mask() { static const int m = exp_int("INFV_SKIP", 0); return m; }

struct Operator {
    int rows = 0;
    DeviceBuf row_box, row_begin, row_end, box_val, box_row, old_ptr, old_slot, slot_tab;
    bool has_old = false;
    int tabw = 4;                      // max slots per box, rounded up to a multiple of 4
    OperatorView view() const {
        OperatorView v;
        v.rows = rows;
        v.row_box = row_box.as<int32_t>();
        v.row_begin = row_begin.as<int32_t>();
        v.row_end = row_end.as<int32_t>();
        v.box_val = box_val.as<float>();
        v.box_row = box_row.as<int32_t>();
        v.old_ptr = has_old ? old_ptr.as<int32_t>() : nullptr;
        v.old_slot = has_old ? old_slot.as<int32_t>() : nullptr;
        v.slot_tab = has_old ? slot_tab.as<int32_t>() : nullptr;
        v.tabw = tabw;
        return v;
    }
};

// Dense form of a plan's operators (infv_ltm_set_dense_plan): num_basis whose fp32 boxes overlap
struct DensePlan {
    bool on = false;
    int first_K = 0, inf_K = 0;
    DeviceBuf first_GT, inf_GT;        // [N][K]
    DeviceBuf bin_box2, edge_box2, uniform_box2;
    // general-psi plan (infv_ltm_set_psi_plan): psi where the reference evaluates it, and the step's scratch
    bool psi_on = false;
    int n_grid = 0;
    DeviceBuf psi_edge, psi_bin, psi_uniform, psi_grid, grid_w;
};

struct Plan {
    int T = 0;
    DensePlan dense;
    Operator first, inf;
    DeviceBuf w, edge_box, edge_dx, bin_box, uniform_idx;
    float w_out = 0.f;
    int n_bins = 0;
    bool points_ok = false;            // the histogram edges are the bins' left edges (what chain_batch3_kernel assumes)
    uint64_t digest = 0;               // FNV-1a of every table infv_ltm_set_plan received (infv_ltm_consolidate_videos: same plan on every handle)
    // FNV-1a of the tables that do not depend on T for one (num_basis, tau, nb_samples) -- read-out weights, sticky histogram,
    // uniform resampling table: infv_ltm_videos_tail draws and attends every video of a step with ONE copy of them, whatever
    // the length of its chunk, and refuses handles whose plans disagree here
    uint64_t shared_digest = 0;
    DeviceBuf views;                   // OperatorView[2] on the device: {first.view(), inf.view()} (VideoTail.op_last points here)
    const OperatorView* device_view(bool inf_op) const { return views.as<OperatorView>() + (inf_op ? 1 : 0); }
    StickyView sticky() const {
        StickyView s;
        s.points_ok = points_ok ? 1 : 0;
        s.n_bins = n_bins;
        s.edge_box = edge_box.as<int32_t>();
        s.edge_dx = edge_dx.as<float>();
        s.bin_box = bin_box.as<int32_t>();
        return s;
    }
};

// Grid of infv_ltm_density (infv_ltm_set_grid_plan): the host tables, uploaded
struct GridPlan {
    bool on = false;
    int M = 0, G = 0;
    DeviceBuf seg_begin, pt_weight, pt_ptr, pt_box, pt_val;
    GridView view() const {
        GridView g;
        g.M = M; g.G = G;
        g.seg_begin = seg_begin.as<int32_t>(); g.pt_weight = pt_weight.as<float>();
        g.pt_ptr = pt_ptr.as<int32_t>(); g.pt_box = pt_box.as<int32_t>(); g.pt_val = pt_val.as<float>();
        return g;
    }
};

struct Profiler {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[INFV_KERNEL_COUNT];
    ~Profiler() { clear_all(); }
    void clear(int k) {
        for (auto& p : ev[k]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        ev[k].clear();
    }
    void clear_all() { for (int k = 0; k < INFV_KERNEL_COUNT; ++k) clear(k); }
};

// Brackets one launch with events when profiling is on.
struct Timed {
    Profiler& prof; int kernel; hipStream_t stream; hipEvent_t a = nullptr, b = nullptr;
    Timed(Profiler& p, int k, hipStream_t s) : prof(p), kernel(k), stream(s) {
        if (prof.on && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, stream);
    }
    ~Timed() {
        if (prof.on && a && b) { (void)hipEventRecord(b, stream); prof.ev[kernel].emplace_back(a, b); }
    }
};

// New-row buffers R of the sub-batch pipeline: the pooling stream fills set b % kRSets for sub-batch b and may run that many
// sub-batches ahead of the UC kernel, the last reader of a set (three sets coupled the pooling to the UC stream's progress).
constexpr int kRSets = 8;
#ifndef INFV_PSETS
#define INFV_PSETS 5
#endif
constexpr int kPSets = INFV_PSETS;            // rotating sets of the sub-batch workspaces (projections, pooled frames) and their events

}  // namespace infv

struct infv_ltm_s {
    infv_ltm_config cfg;
    int N, H, dh, d, dm, P, L, S, maxQ, maxC;
    std::map<int, infv::Plan*> plans;
    infv::MemoryState mem;             // which buffers are live, what the last step left behind, the rng position (ltm_memory_state.h)
    infv::DeviceBuf B[2], KV[2];       // [L][N][d], [L][N][2][dm]   ping-pong (mem.cur())
    infv::DeviceBuf bin_part;          // [L][max_parts][n_bins]  sticky partials, mem.parts() rows per layer in use
    infv::DeviceBuf probs, probs_override, bins, idx, scores;
    unsigned override_mask = 0;        // layers whose next draw uses probs_override (teacher forcing)
    // workspaces of the chunk-parallel stage.  consolidate() fills P set b % kPSets (projections; pooled frames when the rows
    // kernel runs apart) and R set b % kRSets (new rows) for sub-batch b on the worker streams while role S of the sub-batches
    // before it runs on the caller's stream; R set kRSets holds the first chunk of a document.  The per-call path uses set 0.
    infv::DeviceBuf kbar_ws, kbar_side[infv::kPSets], R_ws[infv::kRSets + 1], P_ws[infv::kPSets];
    infv::DeviceBuf kbar_all;          // pooled frames of a whole consolidate_q call
    infv::DeviceBuf wv_hi, wv_lo, R_hi, R_lo;  // split-bf16 operands of the V' half of the new-row projection (fast path)
    bool wv_split_valid = false;       // the value weights of this consolidate call have been split
    // The projection GEMM of the whole-video path runs on the bf16 MFMA pipe, fp32-accurate (three exact bf16 pieces per operand,
    // six products, fp32 accumulation: split_gemm.hip, gemm_x6_wide_kernel); INFV_PROJ_X6=0 at create selects gemm_nt_lw_kernel's
    // fp32 MFMAs instead (rounds 1-3's default).  Planes of [Wv ; q~] are made once per call, of a sub-batch's new rows per launch.
    infv::DeviceBuf w3[3], r3[3];
    infv::DeviceBuf r3_ring[infv::kRSets][3];   // bf16 planes of the new rows written by the pooling kernel itself, one set per R set
    bool proj_x6 = true, w3_valid = false;
    hipStream_t side = nullptr;        // stream of the projection GEMMs; != nullptr: the streams and events below exist (ensure_side_stream)
    hipStream_t pools = nullptr;       // stream of the pooling kernels (HBM-bound; runs ahead of the GEMM stream)
    hipStream_t ucs = nullptr;         // stream of the UC kernels (state update + read-out of a sub-batch)
    // events of a fused call, one per rotating set: pooled (pools), projected (side), role S done (caller's stream), UC done with
    // the P set / with the R set (ucs).  Their `recorded` flags are cleared when a fused call starts (clear_call_events).
    infv::CallEvent ev_pool[infv::kPSets], ev_p[infv::kPSets], ev_s[infv::kPSets], ev_uc[infv::kPSets], ev_r[infv::kRSets];
    hipEvent_t ev_start = nullptr, ev_q = nullptr;   // the call's set-up has begun / its queries and weight planes are ready
    void clear_call_events() {
        for (int i = 0; i < infv::kPSets; ++i) { ev_pool[i].clear(); ev_p[i].clear(); ev_s[i].clear(); ev_uc[i].clear(); }
        for (int i = 0; i < infv::kRSets; ++i) ev_r[i].clear();
    }
    // fast path (consolidate): bias-free scores (ping-pong); per-chunk outputs of role S for the UC kernel -- softmax weights,
    // row sums, resolved gather tables -- in rings of `ring` = kPSets * maxC + 2 slots (a slot is rewritten kPSets sub-batches
    // after the one whose UC kernel read it)
    infv::DeviceBuf Sp[2], cqbuf;
    infv::DeviceBuf qt_buf;            // fast path: pre-multiplied queries qt[(l*H+h)*Q+q][d] of the current call
    infv::DeviceBuf alpha_ring, asum_ring, tab_ring;
    infv::DeviceBuf crit_ring, tabb_ring;        // chain_batch3_kernel -> alpha_rows2_kernel: point scores, drawn-bin tables
    int ring = 0;
    infv::DeviceBuf sync_words;        // [0..7] arrival counters per layer
    // error word of the persistent chain kernel: pinned host memory mapped into the device, so a time-out is
    // visible to the host without any synchronisation or copy
    unsigned int* err_host = nullptr; unsigned int* err_dev = nullptr;
    infv::tok_code tok = INFV_TOKENS_F32;   // element type of the frame tokens `k` (infv_ltm_set_token_dtype)
    bool v_split = false;              // INFV_VPROJ_SPLIT=1 at create: V' half of the sub-batch projection as a split-bf16 contraction
    // Where the V' half of a sub-batch's projection runs.  Default (round 3): inside the side stream's one [V' | S'] GEMM.  The
    // UC stream (V' GEMM -> softmax weights -> update, serial per sub-batch) was the second-longest stream of the pipeline
    // and a GEMM workgroup cannot share a CU with a UC workgroup (272 + 320 of the 512 registers per SIMD), so the V' GEMM
    // only ever delayed the UC kernel behind it; with 16-row chain tiles (48 role-S workgroups instead of 96) the merged
    // GEMM has the CUs to finish well before the chain needs its score half.  Round 2 ran long calls (>= 768 chunks) with the
    // V' half on the UC stream (INFV_VPROJ_ON_UC=1 restores that; the split-bf16 V' projection implies it): then only the
    // SCORE half stays on the side stream (role S waits for it) and the V' half is issued on the UC stream before that kernel.
    int v_on_uc_mode = -1;
    bool vproj_on_uc() const { return v_on_uc_mode >= 0 ? v_on_uc_mode != 0 : v_split; }
    int spin_limit = 1 << 22; int expect_extra = 0;     // INFV_CHAIN_FAULT=1 (tests): expect one arrival too many -> every wait times out
    int32_t* trace_bins = nullptr; float* trace_probs = nullptr; long trace_cap = 0;   // draw trace of consolidate (caller's device buffers)
    infv::DeviceBuf bins_forced; unsigned forced_mask = 0;    // one-shot forced draw of the per-call path
    infv::DeviceBuf mass_acc[3];       // fixed-point sticky bin masses [L][kAccShards][128] u64, ring of 3 (read / accumulate / being cleared)
    infv::DeviceBuf uf_all;            // a consolidate call's Gibbs uniforms as fp32 round-ups [n_chunks][L][S] (chain_batch3_kernel's search)
    infv::DeviceBuf step_tab;          // per-call path: resolved gather table of the step [L][N][tabw] (written by the draw plane of step_project)
    infv::DeviceBuf psi_Y, psi_E, psi_Eg, psi_alpha;   // general-psi step: resampled rows, edge scores, grid scores / probabilities, read-out weights
    infv::DeviceBuf R_all, planes_all[3];    // one pooling launch per call: every new row of the call (fp32, and as three bf16 planes per sub-batch for the projection GEMM)
    infv::DeviceBuf pool_done;         // ... and its per-sub-batch completion counts
    // Sum of a consolidate call's outputs, kept by the UC kernels as they store them (infv_ltm_set_ctx_sum; the hand-over payload
    // of infv_ltm_pack_memory): valid for exactly the (ctx, n_chunks, Q) that mem holds for it (mem.ctx_sum_holds)
    bool ctx_sum_on = false;
    infv::DeviceBuf ctx_sum;           // [L][Q][dm]
    infv::DeviceBuf vid_tab, vid_kbar, vid_P;   // infv_ltm_consolidate_videos with this handle first: video table, pooled frames and projected rows of one step
    infv::DeviceBuf vid_tail;          // infv_ltm_videos_tail with this handle first: the side table beside vid_tab (VideoTail per rank)
    int n_bins = 128;
    // device rng (infv_ltm_set_rng): with it on, a NULL u is generated by the kernels (philox.h), at position mem.pos()
    bool rng_on = false; uint64_t rng_seed = 0; uint32_t rng_stream = 0;
    bool gen(const void* u) const { return !u && rng_on; }                       // this call's uniforms are generated
    infv::RngView rng_view(uint32_t at) const { infv::RngView g = infv::make_rng_view(rng_seed, rng_stream, at); g.on = rng_on ? 1u : 0u; return g; }
    // read-outs of the attention density (ltm_density.hip), which need mem.last_scores_readable()
    infv::GridPlan grid;
    float* mass_trace = nullptr; long mass_cap = 0;   // box-mass trace of the multi-chunk calls (caller's device buffer [cap][L][N])
    long mass_at = -1;                 // chunk index inside the multi-chunk call that is running its per-chunk stages, or -1
    float* vmass_trace = nullptr; long vmass_cap = 0; // packed box-mass trace of the lockstep calls this handle leads ([cap][L][N], infv_ltm_set_videos_mass_trace)
    infv::Profiler prof;
    ~infv_ltm_s() {
        for (auto& kv : plans) delete kv.second;
        // (the streams belong to the process-wide pool, see shared_streams(): synchronise, do not destroy)
        if (side) (void)hipStreamSynchronize(side);
        if (ucs) (void)hipStreamSynchronize(ucs);
        if (pools) (void)hipStreamSynchronize(pools);
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_q) (void)hipEventDestroy(ev_q);
        if (err_host) (void)hipHostFree(err_host);
    }
};

namespace infv {

inline int check_handle(infv_ltm_handle h) {
    if (!h) return fail(INFV_ERR_INVALID, "null handle");
    return INFV_OK;
}

constexpr unsigned int kErrBlobMismatch = 0x100u;  // error-latch code (1 = chain time-out)

// A time-out of the persistent chain kernel leaves garbage in the memory: report it once (at the next entry point
// that would use or extend the memory, or at infv_ltm_sync) and forget the memory.
int check_chain_error(infv_ltm_handle h);
int find_plan(infv_ltm_handle h, int T, Plan** out);
// one launch: the masses of the step that just left its full scores in h->scores -> row h->mass_at of the trace (per-chunk stages)
int trace_masses_of_step(infv_ltm_handle h, const Plan& plan, int Q, hipStream_t stream);
// brackets the per-chunk stages of a multi-chunk call: chunk `c` of the call is about to step
struct MassTraceChunk {
    infv_ltm_handle h;
    MassTraceChunk(infv_ltm_handle h_, long c) : h(h_) { h->mass_at = h->mass_trace ? c : -1; }
    ~MassTraceChunk() { h->mass_at = -1; }
};

inline int check_q(infv_ltm_handle h, int Q) {
    if (Q <= 0 || Q > h->maxQ) return fail(INFV_ERR_INVALID, "Q=%d outside (0, max_q=%d]", Q, h->maxQ);
    return INFV_OK;
}

// fp8 tokens are read in place in 4-byte vectors at offsets that are multiples of 4: `k` must be 16-byte aligned, refused before any
// launch or memory change (the other token types keep the alignment rules they had)
inline int check_k_aligned(const char* name, tok_code tok, const void* k) {
    if (k && !token_ptr_ok(tok, k)) return fail(INFV_ERR_INVALID, "%s: fp8 frame tokens must be 16-byte aligned", name);
    return INFV_OK;
}

inline ProjPtrs make_proj(const infv_ltm_proj* proj, int L) {
    ProjPtrs p;
    memset(&p, 0, sizeof(p));
    for (int l = 0; l < L; ++l) { p.wk[l] = proj[l].wk; p.bk[l] = proj[l].bk; p.wv[l] = proj[l].wv; p.bv[l] = proj[l].bv; }
    return p;
}

}  // namespace infv
