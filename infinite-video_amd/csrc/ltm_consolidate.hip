// infv_ltm_consolidate / infv_ltm_consolidate_pooled: the whole-video fast path (handle and shared checks: ltm_handle.h).
// Per chunk ONE small launch of chain_kernel's role S (draw -> score recurrence -> alpha, sticky
// histogram, gather table); per sub-batch ONE launch of uc_kernel (memory update + read-out of all its
// chunks) on its own stream, overlapping role S of the next sub-batch.
#include "ltm_handle.h"

#include <chrono>
#include <cstdio>
#include <mutex>
#include <vector>

using namespace infv;

namespace {

struct StepS {                       // critical work of the chunk entering the chain
    const Operator* op; bool inf; const float* Snew; const double* u; int sk; long ss;   // Snew: scores part of the chunk's first output row
};

// One sub-batch of a call (chunks [c0, c0 + nb)) and where its stages find their data: filled once by sub_batch_of(), read by
// field name by the pooling, projection, role-S and UC stages.  The first chunk of a document fills one of its own.
struct SubBatch {
    int b = 0, c0 = 0, nb = 0;
    int set = 0, rset = 0;               // its P workspace set (and the events of that set); its R set
    float* r_rows = nullptr;             // its new rows: R_ws[rset], or its slice of the call-long pooling launch's R_all
    bool rows_done = false;              // the pooling stage writes r_rows itself (else the projection stage builds them from frame means)
    void* planes[3] = {};                // bf16 planes of r_rows for the six-product GEMM ...
    bool planes_ready = false;           // ... written by the call-long pooling launch, by this sub-batch's own (stage_pool sets it), or not at all
    int splitk = 1; long split_stride = 0;   // of its projection (set by project_chunks_fast)
    bool defer_values = false;           // the projection on the side stream makes the score half only (V' half: project_values_on_uc)
    bool small_tiles = false;            // the six-product GEMM runs 128 x 128 tiles
    int gemm_pad = 0;                    // padding LDS of its GEMM launches
};

constexpr int kPollDelay = 0;       // units of 64 clocks between role S's deposit and its first poll (INFV_S_POLL_DELAY in the experiments build)

// the stamp read-outs of the experiments build (tools/stamps*.sh and tools/uc_stamps.sh parse these lines)
void print_s_stamps(const long long* hb) {
    fprintf(stderr, "[stamps x10ns] S:");
    for (int i = 1; i <= 5; ++i) fprintf(stderr, " %lld", hb[i] - hb[i - 1]);
    fprintf(stderr, " [draw: sync %lld probs %lld scan %lld search %lld tab %lld] | clk %.0f MHz | S total %lld\n",
            hb[12] - hb[1], hb[13] - hb[12], hb[14] - hb[13], hb[15] - hb[14], hb[2] - hb[15],
            100.0 * (double)(hb[29] - hb[24]) / (double)(hb[5] - hb[0]), hb[5] - hb[0]);
}
void print_batch_s_stamps(const long long* hb, int prev_n) {
    fprintf(stderr, "[batch-S stamps x10ns] wait+read %lld draw %lld tab %lld recurrence %lld row-phase+add %lld - %lld alpha-out %lld | step %lld\n",
            hb[1] - hb[0], hb[2] - hb[1], hb[3] - hb[2], hb[4] - hb[3], hb[5] - hb[4], hb[6] - hb[5], hb[7] - hb[6], hb[7] - hb[0]);
    // shader cycles of the same step (s_memtime): cycles / (10 ns ticks) = effective clock in units of 100 MHz
    fprintf(stderr, "[batch-S clock] step %lld shader cycles over %lld x10ns -> %.2f GHz\n", hb[15] - hb[8], hb[7] - hb[0],
            (hb[7] - hb[0]) > 0 ? 0.1 * (double)(hb[15] - hb[8]) / (double)(hb[7] - hb[0]) : 0.0);
    if (prev_n > 2) fprintf(stderr, "[batch-S avg] %.3f us per step over steps 1..%d of the previous launch\n",
                            0.01 * (double)(hb[17] - hb[16]) / (prev_n - 2), prev_n - 1);
    fprintf(stderr, "[batch-S launch] previous end -> entry %.2f us, set-up %.2f us, step 0 %.2f us, last step + exit %.2f us, entry -> end %.2f us\n",
            0.01 * (double)(hb[18] - hb[21]), 0.01 * (double)(hb[19] - hb[18]), 0.01 * (double)(hb[16] - hb[19]),
            0.01 * (double)(hb[20] - hb[17]), 0.01 * (double)(hb[20] - hb[18]));
}
void print_uc_stamps(const long long* hb) {
    fprintf(stderr, "[uc stamps x10ns] park %lld prefetch-issue %lld barrier %lld gather %lld mfma %lld red-barrier %lld epilogue %lld | chunk total %lld\n",
            hb[1] - hb[0], hb[2] - hb[1], hb[3] - hb[2], hb[4] - hb[3], hb[5] - hb[4], hb[6] - hb[5], hb[7] - hb[6], hb[7] - hb[0]);
}

struct FastPipe {
    infv_ltm_handle h; const Plan& plan; int Q; const ProjPtrs& pp; hipStream_t stream;
    long counter = 0;                // chunks that entered the chain in this call
    float* ctx_sum = nullptr;        // the handle's output sum, when this call keeps it (every UC launch adds its chunks)

    size_t alpha_slot() const { return (size_t)h->L * h->H * Q * h->N; }
    size_t asum_slot() const { return (size_t)h->L * h->H * Q; }
    size_t tab_slot() const { return (size_t)h->L * h->N * 16; }
    size_t crit_slot() const { return (size_t)h->L * h->H * Q * 128; }
    int v_cols() const { return h->L * h->dm; }                    // a projected row is [ V' (L*dm) | scores (L*H*Q) ] ...
    int p_ld() const { return h->L * h->dm + h->L * h->H * Q; }    // ... of this pitch
    bool last_v2 = false;            // the last persistent launch ran chain_batch3_kernel (scores rebuilt by alpha_rows2)
    const float* last_snew = nullptr; int last_sk = 1; long last_ss = 0; float* last_sp_out = nullptr; int batch_launches = 0;

    // what a sticky draw cannot do without, checked in front of every role-S launch
    int refuse_draw(int draw_mode, const double* u) const {
        if (draw_mode != 1) return INFV_OK;
        if (!u && !h->rng_on) return fail(INFV_ERR_INVALID, "sticky consolidation needs the Gibbs uniforms u");
        if (counter == 0 && h->mem.parts() <= 0) return fail(INFV_ERR_STATE, "no sticky histogram available");
        return INFV_OK;
    }
    // the fields ChainRoleS and ChainBatchArgs share by name: the draw's inputs and outputs, the trace rows, the new-row scores
    template <class A> void fill_role_s(A& a, const float* Snew, int sk, long ss, const double* u) const {
        a.part_prev = h->bin_part.as<float>(); a.parts = h->mem.parts();
        a.probs_override = h->probs_override.as<float>(); a.override_mask = h->override_mask;
        a.u = u; a.rng = h->rng_view(h->mem.pos()); a.uniform_idx = plan.uniform_idx.as<int32_t>();
        a.probs_out = h->probs.as<float>(); a.bins_out = h->bins.as<int32_t>(); a.idx_out = h->idx.as<int32_t>();
        if (h->trace_cap > counter) {
            a.probs_tr = h->trace_probs ? h->trace_probs + (size_t)counter * h->L * h->n_bins : nullptr;
            a.bins_tr = h->trace_bins ? h->trace_bins + (size_t)counter * h->L * h->S : nullptr;
        }
        a.Snew = Snew; a.snew_ld = p_ld(); a.snew_splitk = sk; a.snew_split_stride = ss;
        a.cq = h->cqbuf.as<float>(); a.w = plan.w.as<float>(); a.w_out = plan.w_out;
    }
    // the handle's host state after role S of `n` steps
    void after_role_s(int draw_mode, int n) {
        if (draw_mode == 1) h->override_mask = 0;
        h->mem.role_s_done(&plan, Q, n);
        counter += n;
    }

    int launch_s(const StepS& st) {
        ChainArgs a;
        memset(&a, 0, sizeof(a));
        const int QT = (Q + kQTile - 1) / kQTile, QS = chain_s_tiles(Q);
        a.N = h->N; a.H = h->H; a.Q = Q; a.QT = QT; a.QS = QS; a.L = h->L; a.S = h->S; a.d4 = h->d / 4; a.dm4 = h->dm / 4;
        a.st = plan.sticky();
        ChainRoleS& s = a.s;
        s.n_blocks = h->H * QS * h->L;
        s.op = st.op->view();
        s.draw_mode = st.inf ? (h->cfg.sticky ? 1 : 2) : 0;
        if (int rc = refuse_draw(s.draw_mode, st.u)) return rc;
        const long slot = counter % h->ring;
        // sticky histogram: the first step of a call may inherit float partials from the per-call path;
        // afterwards the totals live in the fixed-point ring (read slot k-1, accumulate k, clear k+1)
        fill_role_s(s, st.Snew, st.sk, st.ss, st.u);
        s.acc_prev = (counter > 0) ? h->mass_acc[(counter + 2) % 3].as<unsigned long long>() : nullptr;
        s.acc_next = h->mass_acc[counter % 3].as<unsigned long long>();
        s.acc_clear = h->mass_acc[(counter + 1) % 3].as<unsigned long long>();
        s.tab_out = h->tab_ring.as<int32_t>() + slot * tab_slot();
        s.Sp_prev = h->Sp[h->mem.sc()].as<float>(); s.Sp_next = h->Sp[h->mem.sc() ^ 1].as<float>();
        s.alpha_out = h->alpha_ring.as<float>() + slot * alpha_slot();
        s.asum_out = h->asum_ring.as<float>() + slot * asum_slot();
        static StampBuf stamps("INFV_CHAIN_STAMPS", 32);
        a.dbg = stamps.dev;
        long long hb[32];
        if (stamps.read(300, stream, hb)) print_s_stamps(hb);
        {
            Timed t_(h->prof, INFV_KERNEL_CHAIN, stream);
            HIP_TRY(launch_chain(a, stream));
        }
        after_role_s(s.draw_mode, 1);
        return INFV_OK;
    }

    // role S of the sub-batch's `nb` consecutive infinite-memory chunks in one persistent launch
    int launch_s_batch(const SubBatch& sb, const double* u, const float* uf) {
        static int prev_n = 0;                     // (experiments: steps of the previous launch, for the stamps' average)
        ChainBatchArgs b;
        memset(&b, 0, sizeof(b));
        b.N = h->N; b.H = h->H; b.Q = Q; b.QS = chain_s_tiles(Q); b.L = h->L; b.S = h->S;
        b.st = plan.sticky();
        b.op = plan.inf.view();
        b.draw_mode = h->cfg.sticky ? 1 : 2;
        if (int rc = refuse_draw(b.draw_mode, u)) return rc;
        b.n_steps = sb.nb; b.step0 = counter; b.ring = h->ring;
        b.first_from_parts = (counter == 0) ? 1 : 0;
        fill_role_s(b, h->P_ws[sb.set].as<float>() + v_cols(), sb.splitk, sb.split_stride, u);
        for (int i = 0; i < 3; ++i) b.acc[i] = h->mass_acc[i].as<unsigned long long>();
        b.arrive = h->sync_words.as<unsigned int>(); b.error = h->err_dev;
        b.spin_limit = h->spin_limit; b.expect_extra = h->expect_extra;
        { static const int pd = exp_int("INFV_S_POLL_DELAY", kPollDelay); b.poll_delay = pd; }
        { static const int fl = exp_int("INFV_S_FLAGS", 0); b.exp_flags = fl; }
        if (h->trace_cap > counter) b.trace_steps = (int)((h->trace_cap - counter < sb.nb) ? h->trace_cap - counter : sb.nb);
        b.uf = uf;
        b.tab_ring = h->tab_ring.as<int32_t>(); b.tab_slot = (long)tab_slot();
        b.tabb_ring = h->tabb_ring.as<int32_t>();
        b.crit_ring = h->crit_ring.as<float>(); b.crit_slot = (long)crit_slot();
        b.publish_init = (batch_launches == 0) ? 1 : 0;
        b.alpha_ring = h->alpha_ring.as<float>(); b.alpha_slot = (long)alpha_slot();
        b.asum_ring = h->asum_ring.as<float>(); b.asum_slot = (long)asum_slot();
        b.Sp_in = h->Sp[h->mem.sc()].as<float>(); b.Sp_out = h->Sp[h->mem.sc() ^ 1].as<float>();
        static StampBuf stamps("INFV_CHAIN_STAMPS", 32);
        b.dbg = stamps.dev;
        long long hb[32];
        if (stamps.read(8, stream, hb)) print_batch_s_stamps(hb, prev_n);
        {
            Timed t_(h->prof, INFV_KERNEL_CHAIN, stream);
            if (!(skip_mask() & 8)) HIP_TRY(launch_chain_batch(b, stream));
        }
        last_v2 = chain_batch2_applies(b);
        prev_n = sb.nb;
        last_snew = b.Snew; last_sk = sb.splitk; last_ss = sb.split_stride; last_sp_out = b.Sp_out;
        ++batch_launches;
        after_role_s(b.draw_mode, sb.nb);
        return INFV_OK;
    }

    // the persistent role S leaves SCORES in the alpha ring: turn the `n` slots from slot0 into softmax weights + row sums
    int launch_alpha(int n, long slot0, hipStream_t s, bool last_batch) {
        if (skip_mask() & (4 | 16)) return INFV_OK;                 // (timing experiments: 4 = no UC and no alpha launches, 16 = no alpha, 32 = no UC)
        if (last_v2) {
            // chain_batch3_kernel published point scores + drawn bins: rebuild the full score rows, then the weights
            AlphaRows2Args r;
            memset(&r, 0, sizeof(r));
            r.N = h->N; r.H = h->H; r.Q = Q; r.L = h->L; r.rows = plan.inf.rows; r.tabw = plan.inf.tabw; r.n_steps = n;
            r.slot0 = slot0 % h->ring; r.ring = h->ring;
            r.crit_ring = h->crit_ring.as<float>(); r.crit_slot = (long)crit_slot();
            r.tabb_ring = h->tabb_ring.as<int32_t>(); r.tab_slot = (long)tab_slot();
            r.Snew = last_snew; r.snew_ld = p_ld(); r.snew_splitk = last_sk; r.snew_split_stride = last_ss;
            r.cq = h->cqbuf.as<float>(); r.w = plan.w.as<float>(); r.w_out = plan.w_out;
            r.box_val = plan.inf.box_val.as<float>(); r.box_row = plan.inf.box_row.as<int32_t>();
            r.alpha_ring = h->alpha_ring.as<float>(); r.alpha_slot = (long)alpha_slot();
            r.asum_ring = h->asum_ring.as<float>(); r.asum_slot = (long)asum_slot();
            r.Sp_out = last_batch ? last_sp_out : nullptr;
            HIP_TRY(launch_alpha_rows2(r, s));
            return INFV_OK;
        }
        HIP_TRY(launch_alpha_rows(h->alpha_ring.as<float>(), (long)alpha_slot(), h->asum_ring.as<float>(), (long)asum_slot(),
                                  slot0 % h->ring, h->ring, n, h->L * h->H * Q, h->N, plan.w.as<float>(), plan.w_out, s));
        return INFV_OK;
    }

    // memory update + read-out of the sub-batch's chunks, whose role S used ring slots slot0.. , on the UC stream; flips the
    // B / KV ping-pong
    int launch_uc(const Operator& op, bool inf, const SubBatch& sb, long slot0, float* ctx) {
        hipStream_t ucs = h->ucs;
        UcArgs u;
        memset(&u, 0, sizeof(u));
        u.N = h->N; u.H = h->H; u.Q = Q; u.L = h->L; u.d = h->d; u.dm = h->dm; u.tabw = op.tabw;
        u.op = op.view();
        u.gather = inf ? 1 : 0;
        u.have_state = h->mem.has_memory() ? 1 : 0;
        u.n_chunks = sb.nb; u.slot0 = slot0 % h->ring; u.ring = h->ring;
        u.tab = h->tab_ring.as<int32_t>(); u.tab_slot = (long)tab_slot();
        u.alpha = h->alpha_ring.as<float>(); u.asum = h->asum_ring.as<float>();
        u.R = sb.r_rows; u.Pnew = h->P_ws[sb.set].as<float>(); u.p_ld = p_ld(); u.splitk = sb.splitk; u.split_stride = sb.split_stride;
        u.B_prev = h->B[h->mem.cur()].as<float>(); u.KV_prev = h->KV[h->mem.cur()].as<float>();
        u.B_next = h->B[h->mem.cur() ^ 1].as<float>(); u.KV_next = h->KV[h->mem.cur() ^ 1].as<float>();
        for (int l = 0; l < h->L; ++l) u.bv[l] = pp.bv[l];
        u.ctx = ctx; u.ctx_sum = ctx_sum;
        static StampBuf stamps("INFV_UC_STAMPS", 16);
        u.dbg = stamps.dev;
        long long hb[16];
        if (stamps.read(8, ucs, hb)) print_uc_stamps(hb);
        {
            Timed t_(h->prof, INFV_KERNEL_UC, ucs);
            if (!(skip_mask() & (4 | 32))) HIP_TRY(::infv::launch_uc(u, ucs));
        }
        h->mem.memory_written(1);                               // (consolidate_join declares the finished call's output sum valid)
        return INFV_OK;
    }

    // mass trace (infv_ltm_set_mass_trace): rows [c0, c0 + n) of the call from the softmax weights in ring slots slot0.., one launch
    // on the UC stream between the weights and the UC kernel that reads the same slots (ev_uc, recorded behind it, guards their reuse)
    int launch_mass_trace(long c0, int n, long slot0) {
        if (!h->mass_trace || c0 >= h->mass_cap) return INFV_OK;
        BoxMassArgs a;
        memset(&a, 0, sizeof(a));
        a.src = h->alpha_ring.as<float>(); a.item_stride = (long)alpha_slot(); a.slot0 = slot0 % h->ring; a.ring = h->ring;
        a.from_alpha = 1;
        a.n_items = (int)(h->mass_cap - c0 < n ? h->mass_cap - c0 : n); a.L = h->L; a.rows = h->H * Q; a.N = h->N;
        a.out = h->mass_trace + (size_t)c0 * h->L * h->N; a.out_item_stride = (long)h->L * h->N;
        HIP_TRY(launch_box_mass(a, h->ucs));
        return INFV_OK;
    }
};

// The worker streams are shared by every handle of a device.  The HIP runtime multiplexes a process's streams onto a few
// hardware queues (4 by default, GPU_MAX_HW_QUEUES): a second handle with four more streams of its own shared queues with
// the first one's and its pipeline ran 12 % slower (107 k against 120 k chunks/s for the second engine of bench.py).
// Handles are not re-entrant and their calls are issued from one host thread at a time, so FIFO order within a shared
// stream is the order the host issued the work in; cross-stream dependencies are events, as before.  No lock orders the calls
// of different handles: the one kernel that spins, flag_wait_kernel on the `side` stream, waits only for a pooling launch
// submitted before it (on `pools`, behind the call's own ev_start), and that pooling launch depends on nothing submitted later,
// so whatever interleaving two handles' calls take, every wait is for work already ahead of it and ends.  (A second handle's
// flag_wait_kernel can still hold the shared `side` stream for the other handle's whole pooling launch: a delay, not a deadlock.)
struct SharedStreams { hipStream_t side = nullptr, pools = nullptr, ucs = nullptr; };
bool host_serial() { static const bool v = exp_set("INFV_SERIAL"); return v; }   // timing experiments: the host synchronises the streams (no overlap)
int shared_streams(int dev, SharedStreams** out) {
    static std::mutex mu;
    static SharedStreams pool[64];
    if (dev < 0 || dev >= 64) return fail(INFV_ERR_INVALID, "device index out of range");
    std::lock_guard<std::mutex> lock(mu);
    SharedStreams& p = pool[dev];
    if (!p.side) {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least urgent
        // INFV_PRIO_UCS / _POOL / _SIDE (experiments): -1 most urgent, 0 normal, 1 least urgent
        auto prio = [&](const char* name, int dflt) { const int v = exp_int(name, dflt); return v < hi ? hi : (v > lo ? lo : v); };
        const int prio_ucs = prio("INFV_PRIO_UCS", 0), prio_pool = prio("INFV_PRIO_POOL", lo), prio_side = prio("INFV_PRIO_SIDE", lo);
        HIP_TRY(hipStreamCreateWithPriority(&p.ucs, hipStreamNonBlocking, prio_ucs));
        HIP_TRY(hipStreamCreateWithPriority(&p.pools, hipStreamNonBlocking, prio_pool));
        HIP_TRY(hipStreamCreateWithPriority(&p.side, hipStreamNonBlocking, prio_side));   // last: marks the set complete
    }
    *out = &p;
    return INFV_OK;
}

}  // namespace

namespace infv {
// the normal-priority worker stream of the shared set, for the video Q-former's layer-major schedule (its side stream
// runs the per-call LTM chain of the later layers while the caller's stream runs their short-term attention)
int shared_worker_stream(hipStream_t* out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    SharedStreams* sh = nullptr;
    if (int rc = shared_streams(dev, &sh)) return rc;
    *out = sh->ucs;
    return INFV_OK;
}
}  // namespace infv

namespace {
int ensure_side_stream(infv_ltm_handle h) {
    if (h->side) return INFV_OK;
    SharedStreams* sh = nullptr;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));                              // (the caller's current device: where the handle was created)
    if (int rc = shared_streams(dev, &sh)) return rc;
    h->ucs = sh->ucs; h->pools = sh->pools;
    for (int i = 0; i < kPSets; ++i) {
        HIP_TRY(h->ev_s[i].create());
        HIP_TRY(h->ev_uc[i].create());
        HIP_TRY(h->ev_p[i].create());
        HIP_TRY(h->ev_pool[i].create());
    }
    for (int i = 0; i < kRSets; ++i) HIP_TRY(h->ev_r[i].create());
    if (!h->ev_start) HIP_TRY(hipEventCreateWithFlags(&h->ev_start, hipEventDisableTiming));
    if (!h->ev_q) HIP_TRY(hipEventCreateWithFlags(&h->ev_q, hipEventDisableTiming));
    h->side = sh->side;                                       // last: h->side != nullptr means "streams and events exist"
    return INFV_OK;
}

// ---- infv_ltm_consolidate: the stages of one call, in the order it runs them ----
// The call's inputs and the decisions its stages take, one stage after the other.
struct ConsolidateCall {
    const Plan* plan; const char* k; const float* kbar_pre;   // k: frame tokens (byte addressing), or kbar_pre: the caller's frame means
    int n_chunks, T, Q; const float* q; const infv_ltm_proj* proj; const ProjPtrs* pp; const double* u; float* ctx;
    hipStream_t stream; void* stream_;
    size_t chunk_k, chunk_ctx, chunk_u;            // bytes of one chunk's tokens; floats of one chunk's ctx / uniforms
    // set-up
    bool pool_call_wanted = false;                 // ONE pooling launch for the call, if the schedule allows it
    const float* uf = nullptr;                     // the call's uniforms as fp32 round-ups (chain_batch3_kernel), or nullptr
    // schedule: sub-batch b holds chunks [c0(b), c0(b) + nb(b))
    bool persistent = false;                       // role S in one persistent launch per sub-batch (else one launch per chunk)
    int first_c = 0, sub = 0, n_batches = 0;
    size_t rows = 0;                               // new rows per chunk
    bool split_pool = false; hipStream_t pools = nullptr;   // the pooling stream (the side stream when not split)
    bool use_pr2 = false;                          // pool + rows in one kernel (pool_rows2_kernel)
    int pr_u = 8, pr_pad = 0, pr_wgs = 0;          // its load width, LDS pad, grid cap
    int pool_pad = 0, gemm_pad = 0;                // padding LDS of the pooling kernel of frame means / of the GEMMs
    bool use_pool_call = false;                    // one pooling launch for the call ...
    bool planes_call = false;                      // ... that also writes the bf16 planes of the projection GEMM
    bool planes_in_pool = false;                   // the per-sub-batch pooling launches write those planes
    int small_mask = 0, small_below = 0;           // which sub-batches project in small tiles (small_tiles())
    int drop_waits = 1;                            // (experiments) waits between two role-S launches that are left out
    std::vector<SubBatch> batches;                 // the sub-batches (sub_batch_of), filled when the workspaces exist
    int c0(int b) const { return first_c + b * sub; }
    int nb(int b) const { return n_chunks - c0(b) < sub ? n_chunks - c0(b) : sub; }
};

// fast-path chunk-parallel stage after the pool: new rows R (unless the pooling stage wrote them), then ONE GEMM whose output rows are
// [ V' projection of the row (L*dm) | its scores under the call's pre-multiplied queries (L*H*Q) ], into workspace set sb.set
int project_chunks_fast(infv_ltm_handle h, const ConsolidateCall& cc, bool inf, const float* kbar, SubBatch& sb, hipStream_t stream) {
    const Plan& plan = *cc.plan;
    const Operator& op = inf ? plan.inf : plan.first;
    const long M = (long)sb.nb * op.rows;
    const int n_out = h->L * h->H * cc.Q;
    const long ld = (long)h->L * h->dm + n_out;
    const int sk_max = 8;
    const size_t needP = (size_t)(M ? M : 1) * ld * sizeof(float) * (M < 1024 ? sk_max : 1);
    HIP_TRY(reserve_all({{h->P_ws[sb.set], needP}}));
    float* P = h->P_ws[sb.set].as<float>();
    if (!sb.rows_done) {
        Timed t_(h->prof, INFV_KERNEL_ROWS, stream);
        HIP_TRY(launch_rows(kbar, sb.nb, cc.T, h->d, op.view(), sb.r_rows, stream));
    }
    const int v_cols = h->L * h->dm;
    if (skip_mask() & 2) {
        sb.splitk = project_splitk((int)M, h->d);
    } else if (sb.defer_values && M >= 1024) {
        Timed t_(h->prof, INFV_KERNEL_PROJECT, stream);
        HIP_TRY(launch_project_scores((int)M, h->d, n_out, h->qt_buf.as<float>(), sb.r_rows, P + v_cols, (int)ld, stream, sb.gemm_pad));
        sb.splitk = 1;
    } else if (h->proj_x6 && h->w3_valid && inf && M >= 1024 && h->d % 32 == 0 && !sb.defer_values) {
        // [V'new | S'new] = R . [Wv ; q~]^T from three bf16 planes per operand (the weights' planes were made once for the call)
        Timed t_(h->prof, INFV_KERNEL_PROJECT, stream);
        SplitGemm6 g{};
        if (sb.planes_ready) {
            for (int i = 0; i < 3; ++i) g.A[i] = static_cast<const __bf16*>(sb.planes[i]);
        } else {
            const size_t szR = (size_t)M * h->d * sizeof(__bf16), szC = (size_t)h->maxC * op.rows * h->d * sizeof(__bf16);
            HIP_TRY(reserve_all(BufList().add_each(h->r3, szC > szR ? szC : szR)));
            HIP_TRY(launch_split3_rows(sb.r_rows, h->d, M, h->d, h->r3[0].p, h->r3[1].p, h->r3[2].p, 0, M, stream));
            for (int i = 0; i < 3; ++i) g.A[i] = h->r3[i].as<__bf16>();
        }
        for (int i = 0; i < 3; ++i) g.B[i] = h->w3[i].as<__bf16>();
        g.lda = h->d; g.ldb = h->d; g.C = P; g.ldc = ld; g.M = (int)M; g.N = (int)ld; g.K = h->d;
        g.narrow = sb.small_tiles ? 1 : 0;                      // 128 x 128 tiles (many short workgroups: the same bits) instead of 384 x 256
        HIP_TRY(launch_gemm_x6(g, stream));
        sb.splitk = 1;
    } else {
        Timed t_(h->prof, INFV_KERNEL_PROJECT, stream);
        HIP_TRY(launch_project_fast((int)M, h->d, h->dm, h->L, n_out, *cc.pp, h->qt_buf.as<float>(), sb.r_rows, P, &sb.splitk, stream, sb.gemm_pad));
    }
    sb.split_stride = M * ld;
    return INFV_OK;
}

// Shapes the fused chain kernel cannot hold in LDS (or whose query block qtilde_kernel does not take) run chunk by chunk
// through the per-call stage kernels.
bool fused_chain_holds(infv_ltm_handle h, const Plan& plan, int Q) {
    const int rows_max = plan.first.rows > plan.inf.rows ? plan.first.rows : plan.inf.rows;
    return !plan.dense.on && chain_supported(h->N, h->S, rows_max, plan.inf.tabw) && (h->L * h->H * Q) % 128 == 0 &&
           (h->L * h->dm) % 128 == 0 && uc_supported(h->N, h->d, h->dm, plan.inf.tabw, rows_max) && qtilde_supported(Q);
}

int consolidate_per_chunk(infv_ltm_handle h, const ConsolidateCall& cc) {
    for (int c = 0; c < cc.n_chunks; ++c) {
        MassTraceChunk tr_(h, c);
        const double* uc = cc.u ? cc.u + c * cc.chunk_u : nullptr;
        if (cc.kbar_pre) {
            if (int rc = infv_ltm_step(h, cc.kbar_pre + (size_t)c * cc.T * h->d, cc.T, cc.q, cc.Q, cc.proj, uc, cc.ctx + c * cc.chunk_ctx,
                                       cc.stream_)) return rc;
        } else if (int rc = infv_ltm_forward(h, cc.k + c * cc.chunk_k, cc.T, cc.q, cc.Q, cc.proj, uc, 0, cc.ctx + c * cc.chunk_ctx,
                                             cc.stream_)) return rc;
    }
    return INFV_OK;
}

// Per-call set-up on the caller's stream: the pooling launch's counters, the rings of role S's outputs, the pre-multiplied
// queries, the weight planes of the projection GEMM and the fp32 uniforms.
int consolidate_setup(infv_ltm_handle h, ConsolidateCall& cc, const FastPipe& pipe) {
    const Plan& plan = *cc.plan;
    hipStream_t stream = cc.stream;
    const ProjPtrs& pp = *cc.pp;
    h->wv_split_valid = false;                                // the caller's value weights may have changed since the last call
    // ONE pooling launch per call (round 6, shipped for calls of 768 chunks and more): the pooling stream is what bounds a long call,
    // and between its per-sub-batch launches sat an event record, a wait for the R set's last reader and the ramp of 2688 fresh
    // workgroups (13 us per boundary by the residency stamps).  The launch walks every (chunk, row) of the call in order, writes rows
    // and bf16 planes write-through and counts them into one word per sub-batch; the GEMM stream holds on that word with a one-wave
    // flag_wait_kernel (bounded, latches the handle's error word) instead of an event.  Role S, the GEMM, alpha and UC keep their
    // per-sub-batch launches: 13.3 against 13.7 ms per video on one box, four rounds (profiles/r06_matrix.txt, block 12), same bits.
    // Rows + planes of the whole call live in HBM (0.49 MB per chunk: 1 GB at 2048 chunks); above kPoolCallBudget the call keeps its
    // per-sub-batch pooling launches.  INFV_POOL_CALL (experiments build): 0 never, 2 always.
    static const int pool_call_env = exp_int("INFV_POOL_CALL", -1);
    constexpr size_t kPoolCallBudget = (size_t)16 << 30;
    const size_t pool_call_bytes = (size_t)cc.n_chunks * (size_t)plan.inf.rows * h->d * (sizeof(float) + 3 * sizeof(__bf16));
    cc.pool_call_wanted = pool_call_env >= 0 ? pool_call_env == 2 : (cc.n_chunks >= 768 && pool_call_bytes <= kPoolCallBudget);
    if (cc.pool_call_wanted) {   // its completion counts restart with the call (before ev_start: the pooling stream starts behind it)
        const size_t need_pd = ((size_t)cc.n_chunks + 1) * sizeof(unsigned int);
        HIP_TRY(reserve_all({{h->pool_done, need_pd < 32768 ? 32768 : need_pd}}));
        HIP_TRY(hipMemsetAsync(h->pool_done.p, 0, need_pd, stream));
    }
    HIP_TRY(hipEventRecord(h->ev_start, stream));
    HIP_TRY(hipMemsetAsync(h->mass_acc[0].p, 0, h->mass_acc[0].bytes, stream));   // slot of the call's first step
    // the call's output sum restarts: behind the previous call's pack on this stream, ahead of the first UC launch (ev_s)
    if (pipe.ctx_sum) HIP_TRY(hipMemsetAsync(pipe.ctx_sum, 0, cc.chunk_ctx * sizeof(float), stream));
    // rings of role S's per-chunk outputs (sized for this call's Q)
    HIP_TRY(reserve_all({{h->alpha_ring, (size_t)h->ring * pipe.alpha_slot() * sizeof(float)},
                         {h->asum_ring, (size_t)h->ring * pipe.asum_slot() * sizeof(float)},
                         {h->tab_ring, (size_t)h->ring * pipe.tab_slot() * sizeof(int32_t)},
                         {h->tabb_ring, (size_t)h->ring * pipe.tab_slot() * sizeof(int32_t)},
                         {h->crit_ring, (size_t)h->ring * pipe.crit_slot() * sizeof(float)}}));
    // pre-multiplied queries qt = (q/sqrt(dh)) . Wk_h and the bias term cq = q_h . bk_h / sqrt(dh), once per call
    HIP_TRY(launch_qtilde(cc.q, cc.Q, h->H, h->d, h->L, pp, h->qt_buf.as<float>(), h->cqbuf.as<float>(), stream));
    h->w3_valid = false;
    const long n_rows = pipe.p_ld();
    if (h->proj_x6 && h->d % 32 == 0 && n_rows % 8 == 0) {
        // bf16 planes of the projection GEMM's weight rows [Wv_0 ; ... ; Wv_{L-1} ; q~] (the caller's weights may change between calls)
        HIP_TRY(reserve_all(BufList().add_each(h->w3, (size_t)n_rows * h->d * sizeof(__bf16))));
        for (int l = 0; l < h->L; ++l)
            HIP_TRY(launch_split3_rows(pp.wv[l], h->d, h->dm, h->d, h->w3[0].p, h->w3[1].p, h->w3[2].p, (long)l * h->dm, n_rows, stream));
        HIP_TRY(launch_split3_rows(h->qt_buf.as<float>(), h->d, (long)h->L * h->H * cc.Q, h->d, h->w3[0].p, h->w3[1].p, h->w3[2].p,
                                   (long)h->L * h->dm, n_rows, stream));
        h->w3_valid = true;
    }
    HIP_TRY(hipEventRecord(h->ev_q, stream));                 // the side stream's projections need no more than this
    // the persistent role S searches in fp32 against the round-ups of the f64 uniforms (equivalent to the f64 compare):
    // converted once per call, off the chain
    // With the handle's device rng on and no u, this pass IS the generator: chunk c of the call sits at position pos + c, and
    // the round-up is the same function of the double (philox.h, round_up_f32), so the launch count does not change and the
    // search sees the floats an explicit run of the same uniforms would.  The kernels that read doubles (the per-chunk role S,
    // chain_batch_kernel) generate their own.
    if ((cc.u || h->rng_on) && h->cfg.sticky && chain_batch3_shape_ok(1, plan.sticky().points_ok, plan.inf.rows, h->S, cc.Q)) {
        const size_t need_u = (size_t)cc.n_chunks * cc.chunk_u * sizeof(float);
        HIP_TRY(reserve_all({{h->uf_all, need_u}}));
        if (cc.u) HIP_TRY(launch_round_up_uniforms(cc.u, h->uf_all.as<float>(), (long)cc.n_chunks * (long)cc.chunk_u, stream));
        else HIP_TRY(launch_rng_fill(h->rng_view(h->mem.pos()), cc.n_chunks, h->L, h->S, nullptr, h->uf_all.as<float>(), stream));
        cc.uf = h->uf_all.as<float>();
    }
    return INFV_OK;
}

// The schedule (host decisions only): role S's form, the sub-batches, the pooling form, the padding and tiling knobs.
void consolidate_schedule(infv_ltm_handle h, ConsolidateCall& cc) {
    const Plan& plan = *cc.plan;
    const int mode = h->cfg.sticky ? 1 : 2;
    // INFV_PERSISTENT=0 falls back to one role-S launch per chunk
    static const bool want_persistent = exp_int("INFV_PERSISTENT", 1) != 0;
    cc.persistent = want_persistent &&
        chain_batch_supported(h->N, h->S, plan.inf.rows, plan.inf.tabw, h->H * chain_s_tiles(cc.Q) * h->L) &&
        chain_batch_resident(h->N, h->S, plan.inf.rows, plan.inf.tabw,
                             chain_batch_blocks(h->H, cc.Q, h->L, mode, plan.sticky().points_ok, plan.inf.rows, h->S),
                             mode, plan.sticky().points_ok, cc.Q);
    cc.first_c = h->mem.has_memory() ? 0 : 1;                // the first chunk of a document runs on its own (consolidate_first_chunk)
    // sub-batch size: long calls amortise the per-launch gap of role S over more chunks (42 x 64 new rows = 21 row tiles:
    // 126 score tiles, 252 V' tiles); short ones (e.g. a 256-chunk shard of a multi-GPU run) keep 32 so that the
    // pipeline fills and drains quickly.  INFV_SUB_BATCH overrides.  Every sub-batch but the last has `sub` chunks.
    static const int sub_env = exp_int("INFV_SUB_BATCH", 0);
    cc.sub = h->maxC;
    if (sub_env > 0) cc.sub = sub_env < h->maxC ? sub_env : h->maxC;
    else if (cc.n_chunks < 768 && cc.sub > 32) cc.sub = 32;  // (28 while the V' GEMM ran on the UC stream; 2.84 -> 2.68 ms per 256 chunks)
    cc.n_batches = (cc.n_chunks - cc.first_c + cc.sub - 1) / cc.sub;
    cc.rows = plan.inf.rows;
    // The pooling has its own stream so that the HBM-bound pooling of batch b+2 overlaps the MFMA-bound projection of
    // batch b+1 (pooled frames are triple-buffered either way); INFV_SPLIT_POOL=0 puts it back on the side stream.
    // (Round 1 measured this worse, 87 k vs 95 k chunks/s, because role S was then sensitive to every concurrent
    // kernel; with chain_batch2_kernel and no padding LDS on the GEMMs it is better: 112 k vs 102 k.)
    static const bool split_pool_env = exp_int("INFV_SPLIT_POOL", 1) != 0;
    cc.split_pool = split_pool_env && !cc.kbar_pre;           // (frame means handed in: there is no pooling stage)
    cc.pools = cc.split_pool ? h->pools : h->side;
    // Pool + rows in one kernel: the pooling stream writes the sub-batch's new rows R straight from the tokens -- in this path
    // the frame means are consumed by the rows kernel only; same bits either way.  Default: pool_rows2_kernel (one short-lived
    // workgroup per (chunk, row), a wave per frame and slice): no kbar round trip through HBM, no rows kernel on the side
    // stream, and the pooling stream runs up to kRSets sub-batches ahead instead of three.  Measured in situ (round 3,
    // tools/sweep_r03s.sh, alternating on one box): 132.5 k against 130.5 k chunks/s, pooling stream 14.65 against 15.05 ms.
    // The experiments build keeps INFV_POOL_ROWS=0 (pool_frames_kernel + build_rows_kernel, the round-2 form, still used when
    // frame means are handed in or the width has no pool_rows2 shape).  (Round 3's long-lived grid-stride form, pool_rows_kernel,
    // streamed faster alone -- 218-270 us per launch against 304 -- but cost the chain launches their CUs, 116-121 k: deleted.)
    static const int pr_env = exp_int("INFV_POOL_ROWS", 2);
    static const int pr_u = exp_int("INFV_PR_U", 8);
    static const int pr_pad = exp_int("INFV_PR_PAD", 84 * 1024);
    static const int pr_wgs = exp_int("INFV_PR_WGS", 0);
    cc.use_pr2 = pr_env == 2 && !cc.kbar_pre && pool_rows2_supported(h->d);
    cc.pr_u = pr_u; cc.pr_pad = pr_pad; cc.pr_wgs = pr_wgs;
    // Padding LDS caps the pooling kernel's occupancy at ONE 512-thread workgroup (84 KB: two do not fit, one leaves room for
    // a 74 KB workgroup of the loader-wave GEMM) per CU, so a role-S workgroup
    // always finds LDS and wave slots and the pool's bytes in flight stay bounded.  The GEMMs carry no padding any more
    // (INFV_GEMM_PAD): their workgroups (36 KB, one wave per SIMD) co-reside with a pooling workgroup -- MFMA work beside
    // memory work -- instead of taking the CU away from it.
    static const int pool_pad = exp_int("INFV_POOL_PAD", 84 * 1024);
    static const int gemm_pad = exp_int("INFV_GEMM_PAD", 0);
    cc.pool_pad = pool_pad; cc.gemm_pad = gemm_pad;
    // the one pooling launch (see consolidate_setup): rows and their bf16 planes for the whole call in HBM (402 + 604 MB at 2048
    // chunks), the GEMM stream follows it through per-sub-batch completion counts
    cc.use_pool_call = cc.pool_call_wanted && cc.persistent && cc.n_batches > 0 && !host_serial() && cc.use_pr2 && cc.pr_wgs == 0 &&
                       !(skip_mask() & 1);
    cc.planes_call = cc.use_pool_call && h->proj_x6 && h->d % 32 == 0 && !h->vproj_on_uc();
    // per-sub-batch pooling launches: the kernel writes the bf16 planes of its rows too (no split3_rows_kernel, no re-read of R).
    // Long calls only (round 6, same-box A/B, `profiles/r06_matrix.txt` block 10): a call of 768 chunks and more is bound by the role-S
    // stream and the planes cost the pooling nothing (150.4 against 149.0 k chunks/s, four rounds); a short call -- the 256-chunk
    // shard of the 8-GPU split -- is bound by its pooling launches, which the extra stores lengthen: 2.14-2.17 ms with
    // split3_rows_kernel on the side stream against 2.20-2.24 with the planes written by the pooling kernel.  Same bits either way.
    // (INFV_POOL_PLANES, experiments build: 0 = never, 2 = always.)
    static const int planes_env = exp_int("INFV_POOL_PLANES", 1);
    cc.planes_in_pool = (planes_env == 2 || (planes_env == 1 && cc.n_chunks >= 768)) && cc.use_pr2 && !cc.use_pool_call && h->proj_x6 &&
                        h->w3_valid && h->d % 32 == 0 && !h->vproj_on_uc() && cc.n_batches > 0;
    // (experiments) INFV_SMALL_TILES=<mask>: bit 0 / 1 / 2 = the call's first / second / last sub-batch runs the projection as
    // 128 x 128 tiles (hundreds of short workgroups: faster while the chip is still -- or again -- empty)
    // Shipped (bit 3, round 6): the LAST sub-batch of a long call -- behind the pooling launch the call's tail is serial (GEMM -> role S ->
    // alpha -> UC of the last sub-batch) and the chip is emptying: 288 short workgroups finish sooner than 54 of 120 us.  13.45
    // against 13.63 ms per video over five alternating rounds on one box; the two tilings give the same bits (test-enforced).
    static const int small_mask = exp_int("INFV_SMALL_TILES", 8);
    static const int small_below = exp_int("INFV_SMALL_BELOW", 0);   // sub-batches of fewer chunks than this
    cc.small_mask = small_mask; cc.small_below = small_below;
    // (experiments) INFV_DROP_WAITS=<mask>: what the packets between two role-S launches cost.  1: no wait for the UC kernel of
    // sub-batch b - 5 on the caller's stream (redundant: the GEMM of sub-batch b waited for it, and this stream waits for that GEMM);
    // 2: no event record behind role S / no wait of the UC stream for it (WRONG results: timing only); 4: no wait for the GEMM (WRONG)
    static const int drop_waits = exp_int("INFV_DROP_WAITS", 1);   // (round 6: bit 0 is the default -- 13.62 against 13.72 ms, tighter)
    cc.drop_waits = drop_waits;
}

bool small_tiles(const ConsolidateCall& cc, int b) {
    const int m = cc.small_mask, last = cc.n_batches - 1;
    if (cc.n_chunks >= 768) return (m & 8) && b == last;     // bit 3: the LAST sub-batch of a long call (the chip is emptying: the serial tail)
    return ((m & 1) && b == 0) || ((m & 2) && b == 1) || ((m & 4) && b == last) || cc.nb(b) < cc.small_below;
}

// Sub-batch b of the call.  (After consolidate_workspaces: the workspaces it points into do not move any more.)
SubBatch sub_batch_of(infv_ltm_handle h, const ConsolidateCall& cc, int b) {
    SubBatch sb;
    sb.b = b; sb.c0 = cc.c0(b); sb.nb = cc.nb(b);
    sb.set = b % kPSets; sb.rset = b % kRSets;
    const size_t off = (size_t)(sb.c0 - cc.first_c) * cc.rows * h->d;   // of its rows in the call-long pooling launch's output
    sb.r_rows = cc.use_pool_call ? h->R_all.as<float>() + off : h->R_ws[sb.rset].as<float>();
    sb.rows_done = cc.use_pr2;
    for (int i = 0; i < 3; ++i) {
        if (cc.planes_call) sb.planes[i] = h->planes_all[i].as<__bf16>() + off;
        else if (!cc.use_pool_call) sb.planes[i] = h->r3_ring[sb.rset][i].p;   // (where its own pooling launch would write them)
    }
    sb.planes_ready = cc.planes_call;
    sb.defer_values = h->vproj_on_uc();
    sb.small_tiles = small_tiles(cc, b);
    sb.gemm_pad = cc.gemm_pad;
    return sb;
}

// The first chunk of a document (first-chunk operator, workspace set 2, R set kRSets) -- or, continuing a memory, the scores of
// its K' rows under this call's query.
int consolidate_first_chunk(infv_ltm_handle h, ConsolidateCall& cc, FastPipe& pipe) {
    const Plan& plan = *cc.plan;
    hipStream_t stream = cc.stream, ucs = h->ucs;
    if (!h->mem.has_memory()) {
        const float* kb0 = cc.kbar_pre;
        if (!kb0) {
            HIP_TRY(reserve_all({{h->kbar_ws, (size_t)cc.T * h->d * sizeof(float)}}));
            if (int rc = infv_ltm_pool(h, cc.k, cc.T, h->kbar_ws.as<float>(), cc.stream_)) return rc;
            kb0 = h->kbar_ws.as<float>();
        }
        HIP_TRY(reserve_all({{h->R_ws[kRSets], (size_t)(plan.first.rows ? plan.first.rows : 1) * h->d * sizeof(float)}}));
        SubBatch sb;
        sb.nb = 1; sb.set = 2; sb.rset = kRSets;
        sb.r_rows = h->R_ws[kRSets].as<float>();
        if (int rc = project_chunks_fast(h, cc, false, kb0, sb, stream)) return rc;
        const StepS st{&plan.first, false, h->P_ws[2].as<float>() + pipe.v_cols(), nullptr, sb.splitk, sb.split_stride};
        if (int rc = pipe.launch_s(st)) return rc;
        HIP_TRY(h->ev_s[2].record(stream));
        HIP_TRY(h->ev_s[2].wait_always(ucs));
        if (int rc = pipe.launch_mass_trace(0, 1, 0)) return rc;
        if (int rc = pipe.launch_uc(plan.first, false, sb, 0, cc.ctx)) return rc;
        HIP_TRY(h->ev_uc[2].record(ucs));
    } else if (h->mem.carry_fits(cc.Q)) {
        // ... handed over by infv_ltm_import_chain_state: the scores under this query and the projected memory are the
        // exporting handle's own; nothing is re-derived, the chain goes on bit for bit
    } else {
        // ... bias-free scores of the current K' rows under this query
        if (h->mem.k_stale())
            if (int rc = infv_ltm_reproject(h, cc.proj, cc.stream_)) return rc;
        Timed t_(h->prof, INFV_KERNEL_SCORES, stream);
        HIP_TRY(launch_new_scores(cc.q, cc.Q, h->H, h->L, 1, h->N, h->KV[h->mem.cur()].as<float>(), 0, 2L * h->dm,
                                  (long)h->N * 2 * h->dm, 1, 0, *cc.pp, h->Sp[h->mem.sc()].as<float>(), h->cqbuf.as<float>(), stream));
    }
    h->mem.carry_consumed();
    return INFV_OK;
}

// The workspaces of the sub-batches, sized ahead of their first launch (a growth synchronises the device), and the sub-batches.
int consolidate_workspaces(infv_ltm_handle h, ConsolidateCall& cc) {
    const size_t rows = cc.rows;
    const int sub = cc.sub, wide = h->maxC > sub ? h->maxC : sub;
    if (!cc.kbar_pre && !cc.use_pr2)
        HIP_TRY(reserve_all(BufList().add_each(h->kbar_side, (size_t)h->maxC * cc.T * h->d * sizeof(float))));
    if (cc.n_batches > 0)                                     // the rotating R sets are written off the side stream: size them here
        HIP_TRY(reserve_all(BufList().add_each(h->R_ws, (size_t)sub * rows * h->d * sizeof(float), kRSets)));
    if (cc.use_pool_call) {
        // every workspace the loop would grow (a growth synchronises the device: fatal beside a kernel that waits for the loop's work)
        const long ld = (long)h->L * h->dm + (long)h->L * h->H * cc.Q;
        size_t needP = 0;
        for (int b = 0; b < cc.n_batches; ++b) {
            const size_t M = (size_t)cc.nb(b) * rows;
            const size_t np = M * ld * sizeof(float) * (M < 1024 ? 8 : 1);
            if (np > needP) needP = np;
        }
        const size_t szW = (size_t)h->L * h->dm * h->d * 2, szR = (size_t)wide * rows * h->d * 2;
        const size_t needRall = (size_t)(cc.n_chunks - cc.first_c) * rows * h->d * sizeof(float);
        BufList l;
        l.add(h->R_all, needRall).add_each(h->planes_all, cc.planes_call ? needRall / 2 : 0).add_each(h->P_ws, needP);
        if (h->proj_x6) l.add_each(h->r3, (size_t)wide * rows * h->d * sizeof(__bf16));
        if (h->v_split) l.add(h->wv_hi, szW).add(h->wv_lo, szW).add(h->R_hi, szR).add(h->R_lo, szR);
        bool grew = false;
        HIP_TRY(reserve_all(l, &grew));
        if (grew && h->v_split) h->wv_split_valid = false;
    }
    if (cc.planes_in_pool) {
        BufList l;
        for (int i = 0; i < kRSets; ++i) l.add_each(h->r3_ring[i], (size_t)sub * rows * h->d * sizeof(__bf16));
        HIP_TRY(reserve_all(l));
    }
    cc.batches.clear();
    cc.batches.reserve(cc.n_batches > 0 ? cc.n_batches : 0);
    for (int b = 0; b < cc.n_batches; ++b) cc.batches.push_back(sub_batch_of(h, cc, b));
    return INFV_OK;
}

// The V' half of the sub-batch's projection as its own GEMM on the UC stream `vs`
// (INFV_VPROJ_ON_UC=1, or implied by the split-bf16 V' projection).
int project_values_on_uc(infv_ltm_handle h, const ConsolidateCall& cc, const SubBatch& sb, hipStream_t vs) {
    const Plan& plan = *cc.plan;
    const ProjPtrs& pp = *cc.pp;
    // V' half of this sub-batch's projection: needs the new rows (ev_p), feeds only the UC kernel below
    HIP_TRY(h->ev_p[sb.set].wait_always(vs));
    Timed t_(h->prof, INFV_KERNEL_PROJECT, vs);
    const long Mv = (long)sb.nb * plan.inf.rows;
    const int v_cols = h->L * h->dm, p_ld = h->L * h->dm + h->L * h->H * cc.Q;
    // exact fp32 MFMA by default.  INFV_VPROJ_SPLIT=1: V' only feeds the read-out (1e-3 budget), so it may run as a
    // split-bf16 contraction (three bf16 MFMA products, ~1e-5 relative); bench.py then labels its dtype accordingly
    if (h->v_split && h->d % 64 == 0 && v_cols % 128 == 0) {
        const size_t szW = (size_t)v_cols * h->d * 2, szR = (size_t)h->maxC * plan.inf.rows * h->d * 2;
        bool grew = false;
        HIP_TRY(reserve_all({{h->wv_hi, szW}, {h->wv_lo, szW}, {h->R_hi, szR}, {h->R_lo, szR}}, &grew));
        if (grew) h->wv_split_valid = false;
        if (!h->wv_split_valid) {
            for (int l = 0; l < h->L; ++l)
                HIP_TRY(launch_split_rows(pp.wv[l], h->d, h->dm, h->d, h->wv_hi.as<__bf16>() + (size_t)l * h->dm * h->d,
                                          h->wv_lo.as<__bf16>() + (size_t)l * h->dm * h->d, h->d, vs));
            h->wv_split_valid = true;
        }
        HIP_TRY(launch_split_rows(sb.r_rows, h->d, Mv, h->d, h->R_hi.p, h->R_lo.p, h->d, vs));
        SplitGemm g{};
        g.A_hi = h->R_hi.as<__bf16>(); g.A_lo = h->R_lo.as<__bf16>(); g.lda = h->d; g.strideA = 0;
        g.B_hi = h->wv_hi.as<__bf16>(); g.B_lo = h->wv_lo.as<__bf16>(); g.ldb = h->d; g.strideB = 0;
        g.C = h->P_ws[sb.set].as<float>(); g.ldc = p_ld; g.strideC = 0; g.split_stride = 0;
        g.M = (int)Mv; g.N = v_cols; g.K = h->d; g.k_per_split = h->d; g.splitk = 1; g.nbatch = 1;
        HIP_TRY(launch_split_gemm(g, vs, sb.gemm_pad));
    } else {
        HIP_TRY(launch_project_values((int)Mv, h->d, h->dm, h->L, pp, sb.r_rows, h->P_ws[sb.set].as<float>(), p_ld, vs, sb.gemm_pad));
    }
    return INFV_OK;
}

// ---- the sub-batches.  Streams: `pools` = pooling of batch b+2, `side` = projection GEMM of batch b+1, caller's stream = role S
// of batch b, `ucs` = softmax weights, memory update + read-out of batch b-1.

// frame means (or directly the new rows) of the sub-batch, on `pools`
int stage_pool(infv_ltm_handle h, const ConsolidateCall& cc, SubBatch& sb) {
    if (cc.kbar_pre || cc.use_pool_call) return INFV_OK;
    hipStream_t pools = cc.pools;
    const char* k = cc.k + sb.c0 * cc.chunk_k;
    if (cc.use_pr2) {
        // R set rset was last read by the UC kernel (and the projections) of batch b - kRSets
        HIP_TRY(h->ev_r[sb.rset].wait_on(pools));
        sb.planes_ready = false;
        if (!(skip_mask() & 1)) {
            // the pooling kernel also writes the rows' bf16 planes when the six-product GEMM will read them (>= 1024 rows)
            const bool want_planes = cc.planes_in_pool && (long)sb.nb * (long)cc.rows >= 1024;
            Timed t_(h->prof, INFV_KERNEL_POOL, pools);
            HIP_TRY(launch_pool_rows2(k, h->tok, sb.nb, cc.T, h->P, h->d, cc.plan->inf.view(), sb.r_rows, pools, cc.pr_u, cc.pr_pad,
                                      cc.pr_wgs, want_planes ? sb.planes : nullptr, &sb.planes_ready));
        }
    } else {
        // the rows kernel that read this set's pooled frames (batch b-3) is done once its projection is
        if (cc.split_pool) HIP_TRY(h->ev_p[sb.set].wait_on(pools));
        if (!(skip_mask() & 1)) {
            Timed t_(h->prof, INFV_KERNEL_POOL, pools);
            HIP_TRY(launch_pool(k, h->tok, h->kbar_side[sb.set].as<float>(), (int64_t)sb.nb * cc.T, h->P, h->d, pools, cc.pool_pad));
        }
    }
    if (cc.split_pool) HIP_TRY(h->ev_pool[sb.set].record(pools));
    return INFV_OK;
}

// rows -> [V'new | S'new] GEMM of the sub-batch, on `side`
int stage_project(infv_ltm_handle h, const ConsolidateCall& cc, SubBatch& sb) {
    hipStream_t side = h->side;
    HIP_TRY(h->ev_uc[sb.set].wait_on(side));                  // the UC kernel that read this set is done
    if (!cc.use_pr2) HIP_TRY(h->ev_r[sb.rset].wait_on(side)); // (the rows kernel writes R here)
    if (cc.split_pool && !cc.use_pool_call) HIP_TRY(h->ev_pool[sb.set].wait_always(side));
    const float* kb = cc.kbar_pre ? cc.kbar_pre + (size_t)sb.c0 * cc.T * h->d : h->kbar_side[sb.set].as<float>();
    if (cc.use_pool_call)   // the rows of the sub-batch are complete once every (chunk, row) workgroup of the pooling launch has counted itself in
        HIP_TRY(launch_flag_wait(h->pool_done.as<unsigned int>() + sb.b, (unsigned int)((size_t)sb.nb * cc.rows), h->spin_limit, h->err_dev, side));
    if (int rc = project_chunks_fast(h, cc, true, kb, sb, side)) return rc;
    HIP_TRY(h->ev_p[sb.set].record(side));
    return INFV_OK;
}

// the chunk-parallel work issued while the chain of the sub-batch before `sb` is about to start: the pooling of the one after
// `sb`, the projection of `sb`
int stage_parallel(infv_ltm_handle h, ConsolidateCall& cc, SubBatch& sb) {
    if (sb.b + 1 < cc.n_batches)
        if (int rc = stage_pool(h, cc, cc.batches[sb.b + 1])) return rc;
    return stage_project(h, cc, sb);
}

// what goes out before the first role S: the call-long pooling launch or the pooling of sub-batches 0 and 1, the projection of 0
int stage_prologue(infv_ltm_handle h, ConsolidateCall& cc) {
    HIP_TRY(hipStreamWaitEvent(h->side, h->ev_q, 0));
    if (cc.split_pool) HIP_TRY(hipStreamWaitEvent(cc.pools, h->ev_start, 0));
    if (cc.use_pool_call) {
        PoolCallDesc pc;
        memset(&pc, 0, sizeof(pc));
        pc.sub = cc.sub; pc.n_chunks = cc.n_chunks - cc.first_c;
        pc.R_all = h->R_all.as<float>();
        if (cc.planes_call) for (int i = 0; i < 3; ++i) pc.plane[i] = h->planes_all[i].p;
        pc.done = h->pool_done.as<unsigned int>();
        Timed t_(h->prof, INFV_KERNEL_POOL, cc.pools);
        HIP_TRY(launch_pool_rows2_call(cc.k + cc.first_c * cc.chunk_k, h->tok, cc.T, h->P, h->d, cc.plan->inf.view(), pc, cc.pools, cc.pr_u, cc.pr_pad));
    }
    if (int rc = stage_pool(h, cc, cc.batches[0])) return rc;
    if (cc.n_batches > 1)
        if (int rc = stage_pool(h, cc, cc.batches[1])) return rc;
    return stage_project(h, cc, cc.batches[0]);
}

// role S of sub-batch `sb` on the caller's stream; the chunk-parallel stage of the next sub-batch goes out first (persistent) or
// behind the first chunk's launch, so that it overlaps this sub-batch's chain
int role_s_of(infv_ltm_handle h, ConsolidateCall& cc, FastPipe& pipe, const SubBatch& sb) {
    hipStream_t stream = cc.stream, side = h->side, ucs = h->ucs, pools = cc.pools;
    SubBatch* next = sb.b + 1 < cc.n_batches ? &cc.batches[sb.b + 1] : nullptr;
    if (!(cc.drop_waits & 4)) HIP_TRY(h->ev_p[sb.set].wait_always(stream));
    // the ring slots this batch writes were last read by the UC kernel kPSets batches ago (same set)
    if (!(cc.drop_waits & 1)) HIP_TRY(h->ev_uc[sb.set].wait_on(stream));
    const bool serial = host_serial();                        // timing experiments: no overlap between the streams
    if (serial) { HIP_TRY(hipStreamSynchronize(pools)); HIP_TRY(hipStreamSynchronize(side)); HIP_TRY(hipStreamSynchronize(ucs)); }
    if (cc.persistent) {
        if (next)
            if (int rc = stage_parallel(h, cc, *next)) return rc;
        if (serial) { HIP_TRY(hipStreamSynchronize(pools)); HIP_TRY(hipStreamSynchronize(side)); }
        if (int rc = pipe.launch_s_batch(sb, cc.u ? cc.u + (size_t)sb.c0 * cc.chunk_u : nullptr, cc.uf ? cc.uf + (size_t)sb.c0 * cc.chunk_u : nullptr)) return rc;
        if (serial) HIP_TRY(hipStreamSynchronize(stream));
        return INFV_OK;
    }
    for (int i = 0; i < sb.nb; ++i) {
        const StepS st{&cc.plan->inf, true, h->P_ws[sb.set].as<float>() + (size_t)i * cc.rows * pipe.p_ld() + pipe.v_cols(),
                       cc.u ? cc.u + (size_t)(sb.c0 + i) * cc.chunk_u : nullptr, sb.splitk, sb.split_stride};
        if (int rc = pipe.launch_s(st)) return rc;
        if (i == 0 && next)
            if (int rc = stage_parallel(h, cc, *next)) return rc;
    }
    return INFV_OK;
}

// What the UC kernel needs besides role S's tables -- the softmax weights, and the V' half of the projection when it
// is not part of the side stream's GEMM -- runs on the UC stream itself (a stream of its own for it was measured much
// worse in rounds 1 and 2: every extra concurrent kernel slows role S and the GEMMs more than the shorter stream gains);
// then the memory update + read-out of the sub-batch, whose role S used the ring slots from slot0.
int uc_of(infv_ltm_handle h, const ConsolidateCall& cc, FastPipe& pipe, const SubBatch& sb, long slot0) {
    hipStream_t ucs = h->ucs;
    if (h->vproj_on_uc() && (long)sb.nb * cc.plan->inf.rows >= 1024 && !(skip_mask() & 2))
        if (int rc = project_values_on_uc(h, cc, sb, ucs)) return rc;
    if (!(cc.drop_waits & 2)) {
        HIP_TRY(h->ev_s[sb.set].record(cc.stream));
        HIP_TRY(h->ev_s[sb.set].wait_always(ucs));
    }
    if (cc.persistent)
        if (int rc = pipe.launch_alpha(sb.nb, slot0, ucs, sb.b == cc.n_batches - 1)) return rc;
    if (int rc = pipe.launch_mass_trace(sb.c0, sb.nb, slot0)) return rc;
    if (int rc = pipe.launch_uc(cc.plan->inf, true, sb, slot0, cc.ctx + (size_t)sb.c0 * cc.chunk_ctx)) return rc;
    HIP_TRY(h->ev_uc[sb.set].record(ucs));
    HIP_TRY(h->ev_r[sb.rset].record(ucs));
    return INFV_OK;
}

int consolidate_sub_batches(infv_ltm_handle h, ConsolidateCall& cc, FastPipe& pipe) {
    if (cc.n_batches > 0)
        if (int rc = stage_prologue(h, cc)) return rc;
    static const bool host_trace = exp_set("INFV_HOST_TRACE");   // host time of every loop iteration (is the host ahead of the device?)
    std::vector<double> host_us;
    const auto host_t0 = std::chrono::steady_clock::now();
    auto since_t0 = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - host_t0).count(); };
    for (int b = 0; b < cc.n_batches; ++b) {
        if (host_trace) host_us.push_back(since_t0());
        const long slot0 = pipe.counter;
        if (int rc = role_s_of(h, cc, pipe, cc.batches[b])) return rc;
        if (int rc = uc_of(h, cc, pipe, cc.batches[b], slot0)) return rc;
    }
    if (host_trace && !host_us.empty()) {
        fprintf(stderr, "[host trace] %d iterations, issue time us:", cc.n_batches);
        for (size_t i = 0; i < host_us.size(); i += 4) fprintf(stderr, " %.0f", host_us[i]);
        fprintf(stderr, " | end %.0f\n", since_t0());
    }
    return INFV_OK;
}

// The join: the memory and every ctx are complete once the last UC kernel is; then hand the sticky histogram back as one
// float partial row and bring the K' half of the projected memory up to date.
int consolidate_join(infv_ltm_handle h, const ConsolidateCall& cc, const FastPipe& pipe) {
    for (int i = 0; i < kPSets; ++i) HIP_TRY(h->ev_uc[i].wait_on(cc.stream));
    if (pipe.counter > 0)
        HIP_TRY(launch_acc_to_part(h->mass_acc[(pipe.counter + 2) % 3].as<unsigned long long>(), h->L, 1,
                                   h->bin_part.as<float>(), cc.stream));
    h->mem.fused_call_joined(pipe.counter > 0, pipe.ctx_sum ? cc.ctx : nullptr, cc.n_chunks, cc.Q);
    return INFV_OK;
}

// cc: the caller's arguments by name -- k: frame tokens (pooled here, on a stream of their own), or kbar_pre: frame means
// [n_chunks][T][d] the caller already holds (infv_ltm_consolidate_pooled: the video Q-former's one pass over the tokens produces them)
int consolidate_impl(infv_ltm_handle h, ConsolidateCall& cc, int32_t new_doc) {
    if (int rc = check_handle(h)) return rc;
    if ((!cc.k && !cc.kbar_pre) || !cc.q || !cc.proj || !cc.ctx || cc.n_chunks < 0) return fail(INFV_ERR_INVALID, "consolidate: bad arguments");
    if (int rc = check_k_aligned("consolidate", h->tok, cc.k)) return rc;
    if (int rc = check_chain_error(h)) return rc;
    if (int rc = check_q(h, cc.Q)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, cc.T, &plan)) return rc;
    const ProjPtrs pp = make_proj(cc.proj, h->L);
    cc.plan = plan; cc.pp = &pp;
    cc.stream = static_cast<hipStream_t>(cc.stream_);
    cc.chunk_k = (size_t)cc.T * h->P * h->d * token_bytes(h->tok);
    cc.chunk_ctx = (size_t)h->L * cc.Q * h->dm;
    cc.chunk_u = (size_t)h->L * h->S;
    if (new_doc) infv_ltm_reset(h);
    if (cc.n_chunks == 0) return INFV_OK;
    if (!fused_chain_holds(h, *plan, cc.Q)) return consolidate_per_chunk(h, cc);
    if (int rc = ensure_side_stream(h)) return rc;
    h->clear_call_events();
    FastPipe pipe{h, *plan, cc.Q, pp, cc.stream};
    h->mem.drop_ctx_sum();
    if (h->ctx_sum_on && uc_ctx_sum_supported(cc.Q)) pipe.ctx_sum = h->ctx_sum.as<float>();
    if (int rc = consolidate_setup(h, cc, pipe)) return rc;
    consolidate_schedule(h, cc);
    if (int rc = consolidate_first_chunk(h, cc, pipe)) return rc;
    if (int rc = consolidate_workspaces(h, cc)) return rc;
    if (int rc = consolidate_sub_batches(h, cc, pipe)) return rc;
    return consolidate_join(h, cc, pipe);
}

}  // namespace

extern "C" {

int infv_ltm_consolidate(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T, const float* q,
                         int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                         void* stream) {
    if (!k) return fail(INFV_ERR_INVALID, "consolidate: bad arguments");
    ConsolidateCall cc{};
    cc.k = static_cast<const char*>(k);                       // byte addressing: the token element size depends on the handle
    cc.n_chunks = n_chunks; cc.T = T; cc.q = q; cc.Q = Q; cc.proj = proj; cc.u = u; cc.ctx = ctx; cc.stream_ = stream;
    return consolidate_impl(h, cc, new_doc);
}

int infv_ltm_consolidate_pooled(infv_ltm_handle h, const float* kbar, int32_t n_chunks, int32_t T, const float* q,
                                int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                                void* stream) {
    if (!kbar) return fail(INFV_ERR_INVALID, "consolidate_pooled: bad arguments");
    ConsolidateCall cc{};
    cc.kbar_pre = kbar;
    cc.n_chunks = n_chunks; cc.T = T; cc.q = q; cc.Q = Q; cc.proj = proj; cc.u = u; cc.ctx = ctx; cc.stream_ = stream;
    return consolidate_impl(h, cc, new_doc);
}

}  // extern "C"
