// C ABI of libinfv_ltm.so (include/infv_ltm.h): create / destroy, plans, the per-call entry points, the lockstep multi-video
// calls (the per-call step over many handles), the device rng and state import / export.  The whole-video fast path is
// ltm_consolidate.hip; the handle and the checks the two units share are ltm_handle.h.
#include "ltm_handle.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

using namespace infv;

namespace infv {
thread_local char g_err[512] = "";
std::atomic<long long> g_kernel_launches{0};

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_chain_error(infv_ltm_handle h) {
    if (h->err_host && *reinterpret_cast<volatile unsigned int*>(h->err_host)) {
        const unsigned int code = *reinterpret_cast<volatile unsigned int*>(h->err_host);
        *reinterpret_cast<volatile unsigned int*>(h->err_host) = 0;
        h->mem.forget();
        if (code == kErrBlobMismatch)
            return fail(INFV_ERR_STATE, "the blob handed to an earlier infv_ltm_import_chain_state was not exported by a handle of "
                                        "this shape (magic / version / L, N, d, dm, H, Q, n_bins in its header); the memory has been reset");
        return fail(INFV_ERR_STATE, "the persistent chain kernel of an earlier infv_ltm_consolidate timed out waiting for the "
                                    "other workgroups of its layer (not all co-resident: partitioned or shared GPU?); "
                                    "its outputs and the memory are invalid, the memory has been reset");
    }
    return INFV_OK;
}

int find_plan(infv_ltm_handle h, int T, Plan** out) {
    auto it = h->plans.find(T);
    if (it == h->plans.end()) return fail(INFV_ERR_NO_PLAN, "no plan registered for chunk length T=%d", T);
    *out = it->second;
    return INFV_OK;
}
}  // namespace infv

namespace {

// header of a chain-state blob (infv_ltm_export_chain_state): 16 int32 in front of the fp32 payload
constexpr int kBlobHeaderInts = 16;
constexpr int kBlobMagic = 0x43464E49;             // "INFC"
constexpr int kBlobVersion = 1;
struct BlobHeader { int v[kBlobHeaderInts]; };
__global__ void blob_header_write_kernel(int* out, BlobHeader hd) { if (threadIdx.x < kBlobHeaderInts) out[threadIdx.x] = hd.v[threadIdx.x]; }
__global__ void blob_header_check_kernel(const int* in, BlobHeader hd, unsigned int* err) {
    bool bad = false;
    for (int i = 0; i < kBlobHeaderInts; ++i) bad = bad || in[i] != hd.v[i];
    if (bad) __hip_atomic_store(err, kErrBlobMismatch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int upload_operator(Operator& op, int N, int rows, const int32_t* row_box, const int32_t* row_begin,
                    const int32_t* row_end, const float* box_val, const int32_t* old_ptr,
                    const int32_t* old_slot, int T, int S) {
    if (rows < 0 || rows > N) return fail(INFV_ERR_INVALID, "plan: rows=%d outside [0,%d]", rows, N);
    std::vector<int32_t> box_row(N, -1);
    for (int r = 0; r < rows; ++r) {
        if (row_box[r] < 0 || row_box[r] >= N || box_row[row_box[r]] != -1)
            return fail(INFV_ERR_INVALID, "plan: bad or duplicate row_box[%d]=%d", r, row_box[r]);
        if (row_begin[r] < 0 || row_end[r] > T || row_begin[r] >= row_end[r])
            return fail(INFV_ERR_INVALID, "plan: bad frame range of row %d", r);
        box_row[row_box[r]] = r;
    }
    op.rows = rows;
    HIP_TRY(upload(op.row_box, row_box, rows));
    HIP_TRY(upload(op.row_begin, row_begin, rows));
    HIP_TRY(upload(op.row_end, row_end, rows));
    HIP_TRY(upload(op.box_val, box_val, N));
    HIP_TRY(upload(op.box_row, box_row.data(), N));
    op.has_old = old_ptr != nullptr;
    if (old_ptr) {
        const int nnz = old_ptr[N];
        if (old_ptr[0] != 0 || nnz < 0 || nnz > S) return fail(INFV_ERR_INVALID, "plan: bad old_ptr");
        for (int i = 0; i < nnz; ++i)
            if (old_slot[i] < 0 || old_slot[i] >= S) return fail(INFV_ERR_INVALID, "plan: old_slot out of range");
        int mx = 0;
        for (int n = 0; n < N; ++n) {
            if (old_ptr[n + 1] < old_ptr[n]) return fail(INFV_ERR_INVALID, "plan: old_ptr not monotone");
            if (old_ptr[n + 1] - old_ptr[n] > mx) mx = old_ptr[n + 1] - old_ptr[n];
        }
        op.tabw = mx < 4 ? 4 : (mx + 3) & ~3;
        std::vector<int32_t> tab((size_t)N * op.tabw, -1);
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < old_ptr[n + 1] - old_ptr[n]; ++k) tab[(size_t)n * op.tabw + k] = old_slot[old_ptr[n] + k];
        HIP_TRY(upload(op.slot_tab, tab.data(), tab.size()));
        HIP_TRY(upload(op.old_ptr, old_ptr, N + 1));
        HIP_TRY(upload(op.old_slot, old_slot, nnz));
    }
    return INFV_OK;
}

// draw (if the memory exists) -> update -> attend, for all layers, on one chunk's new rows.
// kbar_rows != nullptr (single-chunk step): R is null and the update builds the new rows of B from the pooled frames;
// draw_done: the draw already ran inside the projection launch (launch_step_project).
int chain_step(infv_ltm_handle h, const Plan& plan, const float* R, const float* Pnew, int splitk,
               long split_stride, const float* q, int Q, const ProjPtrs& pp, const double* u, float* ctx,
               hipStream_t stream, const float* kbar_rows = nullptr, bool draw_done = false, const int32_t* tab = nullptr) {
    const bool inf = h->mem.has_memory();
    const Operator& op = inf ? plan.inf : plan.first;
    const int32_t* idx = nullptr;
    int idx_stride = 0;
    if (inf) {
        if (h->cfg.sticky) {
            if (!draw_done) {
                if (!u && !h->rng_on) return fail(INFV_ERR_INVALID, "sticky step on an existing memory needs the Gibbs uniforms u");
                if (h->mem.parts() <= 0) return fail(INFV_ERR_STATE, "no sticky histogram available (import_state or step first)");
                Timed t_(h->prof, INFV_KERNEL_DRAW, stream);
                HIP_TRY(launch_draw(h->bin_part.as<float>(), h->mem.parts(), h->probs_override.as<float>(),
                                    h->override_mask, plan.sticky(), u, h->S, h->L,
                                    h->probs.as<float>(), h->bins.as<int32_t>(), h->idx.as<int32_t>(), stream,
                                    h->bins_forced.as<int32_t>(), h->forced_mask, h->rng_view(h->mem.pos())));
            }
            h->override_mask = 0;
            h->forced_mask = 0;
            idx = h->idx.as<int32_t>();
            idx_stride = h->S;
        } else {
            idx = plan.uniform_idx.as<int32_t>();
            idx_stride = 0;
        }
    }
    const int nxt = h->mem.cur() ^ 1;
    {
    Timed t_(h->prof, INFV_KERNEL_UPDATE, stream);
    HIP_TRY(launch_update(op.view(), h->N, h->d, h->dm, h->L, h->S, idx, idx_stride, R, Pnew, splitk, split_stride,
                          h->B[h->mem.cur()].as<float>(), h->KV[h->mem.cur()].as<float>(), h->B[nxt].as<float>(),
                          h->KV[nxt].as<float>(), stream, kbar_rows, (inf && h->cfg.sticky && draw_done) ? tab : nullptr));
    }
    h->mem.memory_written(1);
    {
    Timed t_(h->prof, INFV_KERNEL_ATTEND, stream);
    HIP_TRY(launch_attend(q, Q, h->N, h->H, h->L, h->KV[h->mem.cur()].as<float>(), pp, plan.w.as<float>(), plan.w_out,
                          plan.sticky(), ctx, h->bin_part.as<float>(), h->scores.as<float>(), stream));
    }
    h->mem.attended(&plan, Q, attend_parts(Q, h->H, h->N), 1);
    return trace_masses_of_step(h, plan, Q, stream);
}

// One step with dense operators (ltm_dense.hip): draw -> B = x . G -> project the whole memory -> scores, softmax weights,
// read-out -> sticky masses with two-box edges.  Same state layout as chain_step; the K'/V' rows are re-projected from B.
int dense_step(infv_ltm_handle h, const Plan& plan, const float* kbar, int T, const float* q, int Q, const ProjPtrs& pp,
               const double* u, float* ctx, hipStream_t stream) {
    const bool inf = h->mem.has_memory();
    const DensePlan& dp = plan.dense;
    const int32_t* bins = nullptr;
    int bins_stride = 0;
    const int32_t* pos_box2 = dp.uniform_box2.as<int32_t>();
    if (inf && h->cfg.sticky) {
        if (!u && !h->rng_on) return fail(INFV_ERR_INVALID, "sticky step on an existing memory needs the Gibbs uniforms u");
        if (h->mem.parts() <= 0) return fail(INFV_ERR_STATE, "no sticky histogram available (import_state or step first)");
        // (checked BEFORE the draw consumes the one-shot masks: an unsupported request leaves the handle as it was)
        if (h->forced_mask && h->forced_mask != (1u << h->L) - 1u)
            return fail(INFV_ERR_UNSUPPORTED, "dense plans: infv_ltm_set_bins must force every layer of the handle or none");
        Timed t_(h->prof, INFV_KERNEL_DRAW, stream);
        HIP_TRY(launch_draw(h->bin_part.as<float>(), h->mem.parts(), h->probs_override.as<float>(), h->override_mask,
                            plan.sticky(), u, h->S, h->L, h->probs.as<float>(), h->bins.as<int32_t>(), h->idx.as<int32_t>(),
                            stream, h->bins_forced.as<int32_t>(), h->forced_mask, h->rng_view(h->mem.pos())));
        h->override_mask = 0;
        // a forced draw replaces the resampled bins (infv_ltm_set_bins); get_draw still returns the step's own
        bins = h->forced_mask ? h->bins_forced.as<int32_t>() : h->bins.as<int32_t>();
        h->forced_mask = 0;
        bins_stride = h->S;
        pos_box2 = dp.bin_box2.as<int32_t>();
    }
    const int nxt = h->mem.cur() ^ 1;
    if (dp.psi_on) {
        // psi(t) is a dense row: the resampled rows are rows of Y = Psi_pos . B_past (128 positions when sticky, S otherwise)
        Timed t_(h->prof, INFV_KERNEL_UPDATE, stream);
        const bool use_bins = bins != nullptr;
        const int n_pos = use_bins ? h->n_bins : h->S;
        if (inf) {
            HIP_TRY(h->psi_Y.reserve((size_t)h->L * n_pos * h->d * sizeof(float)));
            HIP_TRY(launch_psi_gemm(false, use_bins ? dp.psi_bin.as<float>() : dp.psi_uniform.as<float>(), h->N, 0,
                                    h->B[h->mem.cur()].as<float>(), h->d, (long)h->N * h->d, h->psi_Y.as<float>(), h->d, (long)n_pos * h->d,
                                    n_pos, h->d, h->N, h->L, stream));
        }
        HIP_TRY(launch_psi_update(inf ? dp.inf_GT.as<float>() : dp.first_GT.as<float>(), inf ? dp.inf_K : dp.first_K,
                                  inf ? dp.inf_K : dp.first_K, inf ? h->S : 0, bins, bins_stride, h->psi_Y.as<float>(), n_pos, kbar,
                                  h->B[nxt].as<float>(), h->N, h->d, h->L, stream));
    } else {
        Timed t_(h->prof, INFV_KERNEL_UPDATE, stream);
        HIP_TRY(launch_dense_update(inf ? dp.inf_GT.as<float>() : dp.first_GT.as<float>(), inf ? dp.inf_K : dp.first_K,
                                    inf ? dp.inf_K : dp.first_K, inf ? h->S : 0, bins, bins_stride, pos_box2,
                                    h->B[h->mem.cur()].as<float>(), kbar, h->B[nxt].as<float>(), h->N, h->d, h->L, stream));
    }
    h->mem.memory_written(1);
    HIP_TRY(launch_reproject(h->B[h->mem.cur()].as<float>(), h->N, h->d, h->dm, h->L, pp, h->KV[h->mem.cur()].as<float>(), stream));
    h->mem.reprojected();
    {
        Timed t_(h->prof, INFV_KERNEL_ATTEND, stream);
        HIP_TRY(launch_attend(q, Q, h->N, h->H, h->L, h->KV[h->mem.cur()].as<float>(), pp, plan.w.as<float>(), plan.w_out,
                              plan.sticky(), ctx, h->bin_part.as<float>(), h->scores.as<float>(), stream));
        if (dp.psi_on) {
            // the attend kernel above supplied the scores S = q K^T / sqrt(dh); its read-out and masses assume boxes.  Dense forms:
            const long rows_hq = (long)h->L * h->H * Q;
            const int ldE = h->n_bins + 4, ldG = (dp.n_grid + 3) & ~3;
            HIP_TRY(h->psi_E.reserve((size_t)rows_hq * ldE * sizeof(float)));
            HIP_TRY(h->psi_Eg.reserve((size_t)rows_hq * ldG * sizeof(float)));
            HIP_TRY(h->psi_alpha.reserve((size_t)rows_hq * h->N * sizeof(float)));
            // edge scores z(t_j) = sum_n S[n] psi_n(t_j) -> sticky masses (LTM.py:197-203,224-230)
            HIP_TRY(launch_psi_gemm(true, h->scores.as<float>(), h->N, 0, dp.psi_edge.as<float>(), h->N, 0, h->psi_E.as<float>(), ldE, 0,
                                    (int)rows_hq, h->n_bins + 1, h->N, 1, stream));
            HIP_TRY(launch_psi_masses(h->psi_E.as<float>(), ldE, Q, h->H, h->L, plan.edge_dx.as<float>(), h->bin_part.as<float>(), stream));
            // read-out on the 1000-point grid (LTM.py:251-286): z -> w o prob -> alpha = (w o prob) . Psi_grid -> ctx = alpha . (V' + bv)
            HIP_TRY(launch_psi_gemm(true, h->scores.as<float>(), h->N, 0, dp.psi_grid.as<float>(), h->N, 0, h->psi_Eg.as<float>(), ldG, 0,
                                    (int)rows_hq, dp.n_grid, h->N, 1, stream));
            HIP_TRY(launch_psi_grid(h->psi_Eg.as<float>(), ldG, dp.n_grid, rows_hq, dp.grid_w.as<float>(), stream));
            HIP_TRY(launch_psi_gemm(false, h->psi_Eg.as<float>(), ldG, 0, dp.psi_grid.as<float>(), h->N, 0, h->psi_alpha.as<float>(), h->N, 0,
                                    (int)rows_hq, h->N, dp.n_grid, 1, stream));
            HIP_TRY(launch_psi_ctx(h->psi_alpha.as<float>(), h->KV[h->mem.cur()].as<float>(), pp, Q, h->N, h->H, h->dm / h->H, h->L, ctx, stream));
        } else {
        // the attend kernel's partials assume one box per edge: recompute them from the scores with the two-box table
        HIP_TRY(launch_dense_masses(h->scores.as<float>(), Q, h->N, h->H, h->L, dp.edge_box2.as<int32_t>(),
                                    plan.edge_dx.as<float>(), h->bin_part.as<float>(), stream));
        }
    }
    h->mem.attended(&plan, Q, h->H, 1);
    return trace_masses_of_step(h, plan, Q, stream);
}

// What infv_ltm_step would refuse over the `n_chunks` chunks of a call, for the entry points that reset the memory or pool the
// tokens in front of it (forward, forward_into, consolidate_q): checked first, so that a refused call launches nothing and
// leaves the handle as it was.  `keeps_memory`: the first step runs on the handle's present memory (no reset in front of it).
// (Its callers refuse null q / proj / ctx just before it.)
int precheck_step(infv_ltm_handle h, int T, int Q, const void* u, bool keeps_memory, int n_chunks = 1) {
    if (int rc = check_chain_error(h)) return rc;
    if (int rc = check_q(h, Q)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, T, &plan)) return rc;
    const bool on_memory = keeps_memory && h->mem.has_memory();    // the call's first step resamples an existing memory
    if (h->cfg.sticky && !u && !h->rng_on && (on_memory || n_chunks > 1))   // (every step after the call's first one does)
        return fail(INFV_ERR_INVALID, "sticky step on an existing memory needs the Gibbs uniforms u");
    if (h->cfg.sticky && on_memory) {
        if (h->mem.parts() <= 0) return fail(INFV_ERR_STATE, "no sticky histogram available (import_state or step first)");
        if (plan->dense.on && h->forced_mask && h->forced_mask != (1u << h->L) - 1u)
            return fail(INFV_ERR_UNSUPPORTED, "dense plans: infv_ltm_set_bins must force every layer of the handle or none");
    }
    return INFV_OK;
}

}  // namespace

extern "C" {

int infv_ltm_abi_version(void) { return INFV_LTM_ABI_VERSION; }
int64_t infv_ltm_launch_count(void) { return (int64_t)::infv::g_kernel_launches.load(std::memory_order_relaxed); }
const char* infv_ltm_last_error(void) { return g_err; }

int infv_ltm_create(const infv_ltm_config* cfg, infv_ltm_handle* out) {
    if (!cfg || !out) return fail(INFV_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->head_size != kHeadSize) return fail(INFV_ERR_UNSUPPORTED, "head_size=%d (kernels are built for %d)", cfg->head_size, kHeadSize);
    if (cfg->num_basis <= 0 || cfg->num_basis % 16) return fail(INFV_ERR_UNSUPPORTED, "num_basis=%d must be a positive multiple of 16", cfg->num_basis);
    if (cfg->n_layers < 1 || cfg->n_layers > INFV_LTM_MAX_LAYERS) return fail(INFV_ERR_INVALID, "n_layers=%d outside [1,%d]", cfg->n_layers, INFV_LTM_MAX_LAYERS);
    if (cfg->d_in <= 0 || cfg->d_in % 32) return fail(INFV_ERR_UNSUPPORTED, "d_in=%d must be a positive multiple of 32", cfg->d_in);
    if (cfg->n_heads <= 0 || (cfg->n_heads * cfg->head_size) % 64) return fail(INFV_ERR_UNSUPPORTED, "n_heads*head_size must be a multiple of 64");
    if (cfg->tokens_per_frame <= 0 || cfg->nb_samples <= 0 || cfg->max_q <= 0) return fail(INFV_ERR_INVALID, "tokens_per_frame, nb_samples, max_q must be positive");
    // the draw kernels hold the S resampled slots of a layer in LDS (draw_kernel, step_project_kernel, draw_videos_kernel: 1024)
    if (cfg->nb_samples > kMaxSamples) return fail(INFV_ERR_UNSUPPORTED, "nb_samples=%d (the draw kernels hold at most %d samples)", cfg->nb_samples, kMaxSamples);
    infv_ltm_s* h = new (std::nothrow) infv_ltm_s();
    if (!h) return fail(INFV_ERR_NOMEM, "out of host memory");
    h->cfg = *cfg;
    h->N = cfg->num_basis; h->H = cfg->n_heads; h->dh = cfg->head_size; h->d = cfg->d_in;
    h->dm = cfg->n_heads * cfg->head_size; h->P = cfg->tokens_per_frame; h->L = cfg->n_layers;
    h->S = cfg->nb_samples; h->maxQ = cfg->max_q; h->maxC = cfg->max_batch_chunks > 0 ? cfg->max_batch_chunks : 32;
    const size_t nb = (size_t)h->L * h->N;
    const int max_parts = h->H * ((h->maxQ + 3) / 4);      // finest partial granularity (4-row tiles of the per-call attend kernel)
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = h->B[i].reserve(nb * h->d * sizeof(float));
        if (e == hipSuccess) e = h->KV[i].reserve(nb * 2 * h->dm * sizeof(float));
    }
    const size_t nsq = (size_t)h->L * h->H * h->maxQ * h->N;
    if (e == hipSuccess) e = h->bin_part.reserve((size_t)h->L * max_parts * h->n_bins * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->bin_part.p, 0, h->bin_part.bytes);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = h->Sp[i].reserve(nsq * sizeof(float));
    for (int i = 0; i < 3 && e == hipSuccess; ++i) {
        e = h->mass_acc[i].reserve((size_t)h->L * kAccShards * 128 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(h->mass_acc[i].p, 0, h->mass_acc[i].bytes);
    }
    if (e == hipSuccess) e = h->sync_words.reserve(16 * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(h->sync_words.p, 0, 16 * sizeof(unsigned int));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->err_host), 64, hipHostMallocMapped);
    if (e == hipSuccess) { memset(h->err_host, 0, 64); e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->err_dev), h->err_host, 0); }
    if (e == hipSuccess) e = h->bins_forced.reserve((size_t)h->L * h->S * sizeof(int32_t));
    if (exp_int("INFV_CHAIN_FAULT", 0) != 0) { h->expect_extra = 1; h->spin_limit = 1 << 12; }
    if (const char* f = getenv("INFV_VPROJ_SPLIT")) h->v_split = atoi(f) != 0;
    if (const char* f = getenv("INFV_PROJ_X6")) h->proj_x6 = atoi(f) != 0;
    if (exp_set("INFV_VPROJ_ON_UC")) h->v_on_uc_mode = exp_int("INFV_VPROJ_ON_UC", 0) != 0 ? 1 : 0;
    h->ring = kPSets * h->maxC + 2;         // a slot is rewritten kPSets sub-batches after the one whose UC kernel read it
    if (e == hipSuccess) e = h->cqbuf.reserve((size_t)h->L * h->H * h->maxQ * sizeof(float));
    if (e == hipSuccess) e = h->qt_buf.reserve((size_t)h->L * h->H * h->maxQ * h->d * sizeof(float));
    if (e == hipSuccess) e = h->probs.reserve((size_t)h->L * h->n_bins * sizeof(float));
    if (e == hipSuccess) e = h->probs_override.reserve((size_t)h->L * h->n_bins * sizeof(float));
    if (e == hipSuccess) e = h->bins.reserve((size_t)h->L * h->S * sizeof(int32_t));
    if (e == hipSuccess) e = h->idx.reserve((size_t)h->L * h->S * sizeof(int32_t));
    if (e == hipSuccess) e = h->scores.reserve((size_t)h->L * h->H * h->maxQ * h->N * sizeof(float));
    // what infv_ltm_get_draw returns before any draw has happened (non-sticky handles never draw) is defined: zeros
    if (e == hipSuccess) e = hipMemset(h->probs.p, 0, h->probs.bytes);
    if (e == hipSuccess) e = hipMemset(h->bins.p, 0, h->bins.bytes);
    if (e == hipSuccess) e = hipMemset(h->idx.p, 0, h->idx.bytes);
    if (e != hipSuccess) {
        delete h;
        return fail(INFV_ERR_HIP, "device allocation failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return INFV_OK;
}

int infv_ltm_destroy(infv_ltm_handle h) {
    delete h;
    return INFV_OK;
}

int infv_ltm_set_plan(infv_ltm_handle h, const infv_ltm_plan* p) {
    if (int rc = check_handle(h)) return rc;
    if (!p || p->T < 2) return fail(INFV_ERR_INVALID, "plan: T must be >= 2 (the reference operator is empty for T=1)");
    if (p->n_bins != h->n_bins) return fail(INFV_ERR_UNSUPPORTED, "plan: n_bins=%d (kernels are built for %d)", p->n_bins, h->n_bins);
    Plan* plan = new (std::nothrow) Plan();
    if (!plan) return fail(INFV_ERR_NOMEM, "out of host memory");
    plan->T = p->T;
    int rc = upload_operator(plan->first, h->N, p->first_rows, p->first_row_box, p->first_row_begin,
                             p->first_row_end, p->first_box_val, nullptr, nullptr, p->T, h->S);
    if (rc == INFV_OK)
        rc = upload_operator(plan->inf, h->N, p->inf_rows, p->inf_row_box, p->inf_row_begin, p->inf_row_end,
                             p->inf_box_val, p->inf_old_ptr, p->inf_old_slot, p->T, h->S);
    if (rc != INFV_OK) { delete plan; return rc; }
    for (int j = 0; j <= p->n_bins; ++j)
        if (p->edge_box[j] < -1 || p->edge_box[j] >= h->N) { delete plan; return fail(INFV_ERR_INVALID, "plan: edge_box out of range"); }
    for (int j = 0; j < p->n_bins; ++j)
        if (p->bin_box[j] < -1 || p->bin_box[j] >= h->N) { delete plan; return fail(INFV_ERR_INVALID, "plan: bin_box out of range"); }
    for (int s = 0; s < h->S; ++s)
        if (p->uniform_idx[s] < -1 || p->uniform_idx[s] >= h->N) { delete plan; return fail(INFV_ERR_INVALID, "plan: uniform_idx out of range"); }
    plan->w_out = p->readout_w_out;
    plan->n_bins = p->n_bins;
    plan->points_ok = p->edge_box[0] == -1 && p->edge_box[p->n_bins] == -1;
    for (int j = 0; j < p->n_bins; ++j) {
        if (p->bin_box[j] < 0) plan->points_ok = false;
        if (j > 0 && p->edge_box[j] != p->bin_box[j]) plan->points_ok = false;
    }
    {
        uint64_t x = 1469598103934665603ull;
        auto mix = [&x](const void* a, size_t bytes) {
            const unsigned char* b = static_cast<const unsigned char*>(a);
            for (size_t i = 0; i < bytes; ++i) { x ^= b[i]; x *= 1099511628211ull; }
        };
        const int32_t head[4] = {p->T, p->first_rows, p->inf_rows, p->n_bins};
        mix(head, sizeof(head));
        mix(p->first_row_box, p->first_rows * 4); mix(p->first_row_begin, p->first_rows * 4); mix(p->first_row_end, p->first_rows * 4);
        mix(p->first_box_val, (size_t)h->N * 4);
        mix(p->inf_row_box, p->inf_rows * 4); mix(p->inf_row_begin, p->inf_rows * 4); mix(p->inf_row_end, p->inf_rows * 4);
        mix(p->inf_box_val, (size_t)h->N * 4);
        mix(p->inf_old_ptr, (size_t)(h->N + 1) * 4); mix(p->inf_old_slot, (size_t)p->inf_old_ptr[h->N] * 4);
        mix(p->readout_w, (size_t)h->N * 4); mix(&p->readout_w_out, 4);
        mix(p->edge_box, (size_t)(p->n_bins + 1) * 4); mix(p->edge_dx, (size_t)p->n_bins * 4); mix(p->bin_box, (size_t)p->n_bins * 4);
        mix(p->uniform_idx, (size_t)h->S * 4);
        plan->digest = x;
        // the tables basis_maps builds from (num_basis, tau, nb_samples) alone, whatever T
        x = 1469598103934665603ull;
        mix(&p->n_bins, 4);
        mix(p->readout_w, (size_t)h->N * 4); mix(&p->readout_w_out, 4);
        mix(p->edge_box, (size_t)(p->n_bins + 1) * 4); mix(p->edge_dx, (size_t)p->n_bins * 4); mix(p->bin_box, (size_t)p->n_bins * 4);
        mix(p->uniform_idx, (size_t)h->S * 4);
        plan->shared_digest = x;
    }
    hipError_t e = upload(plan->w, p->readout_w, h->N);
    if (e == hipSuccess) e = upload(plan->edge_box, p->edge_box, p->n_bins + 1);
    if (e == hipSuccess) e = upload(plan->edge_dx, p->edge_dx, p->n_bins);
    if (e == hipSuccess) e = upload(plan->bin_box, p->bin_box, p->n_bins);
    if (e == hipSuccess) e = upload(plan->uniform_idx, p->uniform_idx, h->S);
    if (e == hipSuccess) {
        const OperatorView views[2] = {plan->first.view(), plan->inf.view()};
        e = upload(plan->views, views, 2);
    }
    if (e != hipSuccess) { delete plan; return fail(INFV_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e)); }
    auto it = h->plans.find(p->T);
    if (it != h->plans.end()) {
        h->mem.plan_erased(it->second);
        delete it->second; h->plans.erase(it);
    }
    h->plans[p->T] = plan;
    return INFV_OK;
}

int infv_ltm_has_plan(infv_ltm_handle h, int32_t T) {
    if (int rc = check_handle(h)) return rc;
    return h->plans.count(T) ? 1 : 0;
}

int infv_ltm_set_dense_plan(infv_ltm_handle h, const infv_ltm_dense_plan* p) {
    if (int rc = check_handle(h)) return rc;
    if (!p || !p->first_GT || !p->inf_GT || !p->bin_box2 || !p->edge_box2 || !p->uniform_box2)
        return fail(INFV_ERR_INVALID, "dense plan: null argument");
    Plan* plan = nullptr;
    if (int rc = find_plan(h, p->T, &plan)) return rc;          // the regular plan of this T carries readout_w / edge_dx
    if (p->first_K != p->T || p->inf_K != h->S + p->T)
        return fail(INFV_ERR_INVALID, "dense plan: first_K=%d inf_K=%d, expected %d and %d", p->first_K, p->inf_K, p->T, h->S + p->T);
    auto check_pairs = [&](const int32_t* t, int n) {
        for (int i = 0; i < 2 * n; ++i) if (t[i] < -1 || t[i] >= h->N) return false;
        return true;
    };
    if (!check_pairs(p->bin_box2, h->n_bins) || !check_pairs(p->edge_box2, h->n_bins + 1) || !check_pairs(p->uniform_box2, h->S))
        return fail(INFV_ERR_INVALID, "dense plan: box index out of range");
    DensePlan& d = plan->dense;
    HIP_TRY(upload(d.first_GT, p->first_GT, (size_t)h->N * p->first_K));
    HIP_TRY(upload(d.inf_GT, p->inf_GT, (size_t)h->N * p->inf_K));
    HIP_TRY(upload(d.bin_box2, p->bin_box2, (size_t)2 * h->n_bins));
    HIP_TRY(upload(d.edge_box2, p->edge_box2, (size_t)2 * (h->n_bins + 1)));
    HIP_TRY(upload(d.uniform_box2, p->uniform_box2, (size_t)2 * h->S));
    d.first_K = p->first_K; d.inf_K = p->inf_K;
    d.on = true;
    return INFV_OK;
}

int infv_ltm_set_psi_plan(infv_ltm_handle h, const infv_ltm_psi_plan* p) {
    if (int rc = check_handle(h)) return rc;
    if (!p || !p->psi_edge || !p->psi_bin || !p->psi_uniform || !p->psi_grid || !p->grid_w || p->n_grid < 2)
        return fail(INFV_ERR_INVALID, "psi plan: null argument");
    Plan* plan = nullptr;
    if (int rc = find_plan(h, p->T, &plan)) return rc;
    DensePlan& d = plan->dense;
    if (!d.on) return fail(INFV_ERR_STATE, "psi plan: set the dense plan of T=%d first (infv_ltm_set_dense_plan)", p->T);
    if (h->grid.on || h->mass_trace || h->vmass_trace)
        return fail(INFV_ERR_UNSUPPORTED, "psi plan: the handle has a grid plan or a mass trace set (box plans only: infv_ltm_set_grid_plan)");
    HIP_TRY(hipDeviceSynchronize());                            // a step of this length may still be reading the old tables
    HIP_TRY(upload(d.psi_edge, p->psi_edge, (size_t)(h->n_bins + 1) * h->N));
    HIP_TRY(upload(d.psi_bin, p->psi_bin, (size_t)h->n_bins * h->N));
    HIP_TRY(upload(d.psi_uniform, p->psi_uniform, (size_t)h->S * h->N));
    HIP_TRY(upload(d.psi_grid, p->psi_grid, (size_t)p->n_grid * h->N));
    HIP_TRY(upload(d.grid_w, p->grid_w, (size_t)p->n_grid));
    d.n_grid = p->n_grid;
    d.psi_on = true;
    return INFV_OK;
}

int infv_ltm_reset(infv_ltm_handle h) {
    if (int rc = check_handle(h)) return rc;
    h->mem.forget();
    return INFV_OK;
}

int infv_ltm_has_memory(infv_ltm_handle h) {
    if (int rc = check_handle(h)) return rc;
    return h->mem.has_memory() ? 1 : 0;
}

int infv_ltm_set_token_dtype(infv_ltm_handle h, int32_t dtype) {
    if (int rc = check_handle(h)) return rc;
    if (!token_dtype_known(dtype)) return fail(INFV_ERR_INVALID, "set_token_dtype: unknown dtype %d", dtype);
    h->tok = static_cast<tok_code>(dtype);
    return INFV_OK;
}

int infv_ltm_pool(infv_ltm_handle h, const void* k, int64_t n_frames, float* kbar, void* stream) {
    if (int rc = check_handle(h)) return rc;
    if (!k || !kbar || n_frames < 0) return fail(INFV_ERR_INVALID, "pool: bad arguments");
    if (int rc = check_k_aligned("pool", h->tok, k)) return rc;
    Timed t_(h->prof, INFV_KERNEL_POOL, static_cast<hipStream_t>(stream));
    HIP_TRY(launch_pool(k, h->tok, kbar, n_frames, h->P, h->d, static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

int infv_ltm_new_rows(infv_ltm_handle h, int32_t T) {
    if (int rc = check_handle(h)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, T, &plan)) return rc;
    if (plan->dense.on) return fail(INFV_ERR_UNSUPPORTED, "new_rows: the plan for T = %d is dense (no box rows)", T);
    return plan->inf.rows;
}

int infv_ltm_pool_rows(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T, float* R, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!k || !R || n_chunks < 0) return fail(INFV_ERR_INVALID, "pool_rows: bad arguments");
    if (int rc = check_k_aligned("pool_rows", h->tok, k)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, T, &plan)) return rc;
    if (plan->dense.on) return fail(INFV_ERR_UNSUPPORTED, "pool_rows: the plan for T = %d is dense (no box rows)", T);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Timed t_(h->prof, INFV_KERNEL_POOL, stream);
    if (pool_rows2_supported(h->d)) {
        static const int wgs = exp_int("INFV_PR_WGS", 0);      // (tools/pool_cus.py)
        static const int pad = exp_int("INFV_PR_PAD", 84 * 1024);
        HIP_TRY(launch_pool_rows2(k, h->tok, n_chunks, T, h->P, h->d, plan->inf.view(), R, stream, 8, pad, wgs));
        return INFV_OK;
    }
    // widths without a pool_rows2 shape: the two kernels, one chunk group at a time through the pooled-frame workspace
    const size_t need = (size_t)n_chunks * T * h->d * sizeof(float);
    HIP_TRY(reserve_all({{h->kbar_side[0], need}}));
    HIP_TRY(launch_pool(k, h->tok, h->kbar_side[0].as<float>(), (int64_t)n_chunks * T, h->P, h->d, stream));
    HIP_TRY(launch_rows(h->kbar_side[0].as<float>(), n_chunks, T, h->d, plan->inf.view(), R, stream));
    return INFV_OK;
}

int infv_ltm_step(infv_ltm_handle h, const float* kbar, int32_t T, const float* q, int32_t Q,
                  const infv_ltm_proj* proj, const double* u, float* ctx, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!kbar || !q || !proj || !ctx) return fail(INFV_ERR_INVALID, "step: null argument");
    if (int rc = check_chain_error(h)) return rc;
    if (int rc = check_q(h, Q)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, T, &plan)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const ProjPtrs pp = make_proj(proj, h->L);
    if (plan->dense.on) return dense_step(h, *plan, kbar, T, q, Q, pp, u, ctx, stream);
    if (h->mem.k_stale() && h->mem.has_memory())
        if (int rc = infv_ltm_reproject(h, proj, stream_)) return rc;
    // Three launches per step (six in round 2): [new-row projection with the rows built on the fly + the draw] -> update
    // (its new B rows built from the pooled frames too) -> attend.  Same arithmetic in the same order as the batched path.
    const bool inf = h->mem.has_memory();
    const Operator& op = inf ? plan->inf : plan->first;
    const long n_cols = (long)h->L * 2 * h->dm;
    const int sk_max = project_splitk(op.rows > 0 ? op.rows : 1, h->d);
    const size_t needP = (size_t)(op.rows ? op.rows : 1) * n_cols * sk_max * sizeof(float);
    HIP_TRY(reserve_all({{h->P_ws[0], needP}}));
    StepDraw dr;
    memset(&dr, 0, sizeof(dr));
    if (inf && h->cfg.sticky) {
        if (!u && !h->rng_on) return fail(INFV_ERR_INVALID, "sticky step on an existing memory needs the Gibbs uniforms u");
        if (h->mem.parts() <= 0) return fail(INFV_ERR_STATE, "no sticky histogram available (import_state or step first)");
        dr.rng = h->rng_view(h->mem.pos());
        dr.n_layers = h->L; dr.bin_part = h->bin_part.as<float>(); dr.parts = h->mem.parts();
        dr.probs_override = h->probs_override.as<float>(); dr.override_mask = h->override_mask; dr.sticky = plan->sticky();
        dr.u = u; dr.S = h->S; dr.probs_out = h->probs.as<float>(); dr.bins_out = h->bins.as<int32_t>(); dr.idx_out = h->idx.as<int32_t>();
        dr.bins_forced = h->bins_forced.as<int32_t>(); dr.forced_mask = h->forced_mask;
        // the draw also resolves the gather table of the step (per layer: source box of every (box, slot) entry)
        const size_t need_t = (size_t)h->L * h->N * op.tabw * sizeof(int32_t);
        if (op.tabw > 0 && op.slot_tab.p != nullptr) {
            HIP_TRY(reserve_all({{h->step_tab, need_t}}));
            dr.slot_tab = op.slot_tab.as<int32_t>(); dr.tab_entries = h->N * op.tabw; dr.tab_out = h->step_tab.as<int32_t>();
        }
    }
    int sk = 1;
    {
        Timed t_(h->prof, INFV_KERNEL_PROJECT, stream);
        HIP_TRY(launch_step_project(kbar, h->d, h->dm, h->L, op.view(), pp, h->P_ws[0].as<float>(), &sk, dr, stream));
    }
    return chain_step(h, *plan, nullptr, h->P_ws[0].as<float>(), sk, (long)op.rows * n_cols, q, Q, pp, u, ctx, stream, kbar,
                      dr.n_layers > 0, dr.tab_out);
}

int infv_ltm_steps(infv_ltm_handle h, const float* kbar, int32_t n_chunks, int32_t T, const float* q, int32_t Q,
                   const infv_ltm_proj* proj, const double* u, float* ctx, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!kbar || !q || !proj || !ctx || n_chunks < 0) return fail(INFV_ERR_INVALID, "steps: bad arguments");
    if (int rc = check_chain_error(h)) return rc;
    if (int rc = check_q(h, Q)) return rc;
    Plan* plan = nullptr;
    if (int rc = find_plan(h, T, &plan)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const ProjPtrs pp = make_proj(proj, h->L);
    const size_t chunk_kbar = (size_t)T * h->d, chunk_q = (size_t)h->L * Q * h->dm, chunk_u = (size_t)h->L * h->S;
    int c = 0;
    if (plan->dense.on) {                                     // dense operators: chunk by chunk
        for (; c < n_chunks; ++c) {
            MassTraceChunk tr_(h, c);
            if (int rc = infv_ltm_step(h, kbar + c * chunk_kbar, T, q + c * chunk_q, Q, proj, u ? u + c * chunk_u : nullptr,
                                       ctx + c * chunk_q, stream_)) return rc;
        }
        return INFV_OK;
    }
    if (!h->mem.has_memory() && n_chunks > 0) {               // first chunk of a document: its own operator
        MassTraceChunk tr_(h, 0);
        if (int rc = infv_ltm_step(h, kbar, T, q, Q, proj, u, ctx, stream_)) return rc;
        c = 1;
    }
    if (c < n_chunks && h->mem.k_stale())
        if (int rc = infv_ltm_reproject(h, proj, stream_)) return rc;
    const size_t rows = plan->inf.rows;
    const long n_cols = (long)h->L * 2 * h->dm;
    // sub-batches of at least 16 chunks: 1024 new rows take the large-tile GEMM without split-K
    const int sub = h->maxC > 16 ? h->maxC : 16;
    while (c < n_chunks) {
        const int nb = n_chunks - c < sub ? n_chunks - c : sub;
        // project the new rows of the sub-batch's pooled chunks into workspace set 0, which every sub-batch reuses: its readers
        // (the update kernels of the previous one) are earlier on this same stream
        const long M = (long)nb * rows;
        const int sk = project_splitk((int)M, h->d);
        const long ss = M * n_cols;
        HIP_TRY(reserve_all({{h->R_ws[0], (size_t)(M ? M : 1) * h->d * sizeof(float)},
                             {h->P_ws[0], (size_t)(M ? M : 1) * n_cols * sk * sizeof(float)}}));   // growing frees: nothing may still read it
        {
            Timed t_(h->prof, INFV_KERNEL_ROWS, stream);
            HIP_TRY(launch_rows(kbar + c * chunk_kbar, nb, T, h->d, plan->inf.view(), h->R_ws[0].as<float>(), stream));
        }
        {
            Timed t_(h->prof, INFV_KERNEL_PROJECT, stream);
            HIP_TRY(launch_project(nb, h->d, h->dm, h->L, plan->inf.view(), pp, h->R_ws[0].as<float>(), h->P_ws[0].as<float>(), stream, 0));
        }
        for (int i = 0; i < nb; ++i) {
            MassTraceChunk tr_(h, c + i);
            if (int rc = chain_step(h, *plan, h->R_ws[0].as<float>() + (size_t)i * rows * h->d,
                                    h->P_ws[0].as<float>() + (size_t)i * rows * n_cols, sk, ss, q + (c + i) * chunk_q, Q, pp,
                                    u ? u + (c + i) * chunk_u : nullptr, ctx + (c + i) * chunk_q, stream)) return rc;
        }
        c += nb;
    }
    return INFV_OK;
}

int infv_ltm_consolidate_q(infv_ltm_handle h, const void* k, int32_t n_chunks, int32_t T, const float* q,
                           int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                           void* stream) {
    if (int rc = check_handle(h)) return rc;
    if (!k || n_chunks < 0) return fail(INFV_ERR_INVALID, "consolidate_q: bad arguments");
    if (int rc = check_k_aligned("consolidate_q", h->tok, k)) return rc;
    if (n_chunks > 0) {
        if (!q || !proj || !ctx) return fail(INFV_ERR_INVALID, "step: null argument");
        if (int rc = precheck_step(h, T, Q, u, !new_doc, n_chunks)) return rc;
    }
    if (new_doc) infv_ltm_reset(h);
    if (n_chunks == 0) return INFV_OK;
    const size_t need = (size_t)n_chunks * T * h->d * sizeof(float);
    HIP_TRY(reserve_all({{h->kbar_all, need}}));
    if (int rc = infv_ltm_pool(h, k, (int64_t)n_chunks * T, h->kbar_all.as<float>(), stream)) return rc;
    return infv_ltm_steps(h, h->kbar_all.as<float>(), n_chunks, T, q, Q, proj, u, ctx, stream);
}

int infv_ltm_forward(infv_ltm_handle h, const void* k, int32_t T, const float* q, int32_t Q,
                     const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx, void* stream) {
    if (int rc = check_handle(h)) return rc;
    if (!k) return fail(INFV_ERR_INVALID, "forward: null k");
    if (int rc = check_k_aligned("forward", h->tok, k)) return rc;
    if (!q || !proj || !ctx) return fail(INFV_ERR_INVALID, "step: null argument");
    if (int rc = precheck_step(h, T, Q, u, !new_doc)) return rc;
    if (new_doc) infv_ltm_reset(h);
    HIP_TRY(h->kbar_ws.reserve((size_t)T * h->d * sizeof(float)));
    if (int rc = infv_ltm_pool(h, k, T, h->kbar_ws.as<float>(), stream)) return rc;
    return infv_ltm_step(h, h->kbar_ws.as<float>(), T, q, Q, proj, u, ctx, stream);
}

int infv_ltm_forward_into(infv_ltm_handle h, const void* k, int32_t token_dtype, int32_t T, float* kbar, const float* q, int32_t Q,
                          const infv_ltm_proj* proj, const double* u, float* ctx, void* stream) {
    if (int rc = check_handle(h)) return rc;
    if (!token_dtype_known(token_dtype)) return fail(INFV_ERR_INVALID, "forward_into: unknown token dtype %d", token_dtype);
    if (T <= 0 || !k || !kbar) return fail(INFV_ERR_INVALID, "forward_into: T must be positive, k and kbar non-null");
    if (int rc = check_k_aligned("forward_into", token_dtype, k)) return rc;
    if (!q || !proj || !ctx) return fail(INFV_ERR_INVALID, "step: null argument");
    if (int rc = precheck_step(h, T, Q, u, true)) return rc;
    if (int rc = infv_ltm_set_token_dtype(h, token_dtype)) return rc;
    if (int rc = infv_ltm_pool(h, k, T, kbar, stream)) return rc;
    return infv_ltm_step(h, kbar, T, q, Q, proj, u, ctx, stream);
}


}  // extern "C"

// ---- several independent videos in lockstep (infv_ltm_consolidate_videos / infv_ltm_steps_videos / infv_ltm_steps_videos_from) ----
// Step s advances every video that still has a chunk: ONE pooling, projection, draw, update and attend launch for all of them
// (ltm_kernels.hip section 7), ordered by launch order on the caller's stream.  The state stays in the handles; the lead
// handle (hs[0]) owns the call's workspaces: the video table and the pooled frames / projected rows of one step of at most
// kVideoGroup videos.  Larger calls run their videos in groups of that size, one group after the other.
namespace {
constexpr int kVideoGroup = 256;

// tokens: the handles also agree on their token dtype (infv_ltm_consolidate_videos pools tokens; infv_ltm_steps_videos reads
// frame means, so the dtype does not enter)
bool same_config(infv_ltm_handle a, infv_ltm_handle b, bool tokens) {
    return a->N == b->N && a->H == b->H && a->dh == b->dh && a->d == b->d && a->P == b->P && a->L == b->L && a->S == b->S &&
           (a->cfg.sticky != 0) == (b->cfg.sticky != 0) && (!tokens || a->tok == b->tok);
}

bool same_plan(const Plan& a, const Plan& b) {
    return a.digest == b.digest && a.dense.on == b.dense.on && a.first.rows == b.first.rows && a.inf.rows == b.inf.rows &&
           a.inf.tabw == b.inf.tabw && a.n_bins == b.n_bins && a.w_out == b.w_out;
}

// One lockstep call: the caller's arguments by name, and what validation derives from them.  tokens: `k` holds frame tokens,
// pooled per step (infv_ltm_consolidate_videos); else `kbar` holds frame means, gathered per step (infv_ltm_steps_videos*), video
// v's from chunk kbar_chunk0[v] (cu[v] without the table).  Chunk c of the packed arrays reads its query at q + c * q_stride:
// q_stride 0 shares one [L,Q,dm] query, L*Q*dm (q_per_chunk) gives every chunk its own.  `name` prefixes the refusals.
struct VideosCall {
    const char* name; const infv_ltm_handle* hs; int V; const int32_t* cu;
    bool tokens; const char* k; const float* kbar; const int32_t* kbar_chunk0;
    int T; const float* q; bool q_per_chunk; int Q; const infv_ltm_proj* proj; const double* u; int new_doc; float* ctx; void* stream_;
    // infv_ltm_videos_tail: frames of every video's LAST chunk (0 or T: full), k / kbar then packed by FRAME; nullptr for the other calls
    const int32_t* tail_T = nullptr;
    // derived by videos_validate
    int total = 0; bool sticky = false; std::vector<Plan*> plans;
    size_t chunk_k = 0, chunk_kbar = 0, chunk_ctx = 0, chunk_u = 0;
    bool ragged = false;               // some video's last chunk is short: the stages that depend on T take it per video
    std::vector<Plan*> last_plans;     // plan of video v's last chunk (ragged only)
    std::vector<long long> frame0;     // first frame of video v in the packed k / kbar (ragged only)
    int rows_max = 0;                  // most new rows of any operator the call may use
    int tail(int v) const { return (tail_T && tail_T[v] != 0 && len(v) > 0) ? tail_T[v] : T; }
    bool short_tail(int v) const { return len(v) > 0 && tail(v) != T; }
    const Plan* last_plan(int v) const { return ragged ? last_plans[v] : plans[v]; }
    // the lockstep stages
    hipStream_t stream = nullptr; ProjPtrs pp; int parts = 0;
    std::vector<int> order;            // the present group's videos by decreasing length: those still running at step s are ranks [0, n_s)
    int len(int v) const { return cu[v + 1] - cu[v]; }
    size_t kbar_base(int v) const { return (size_t)(kbar_chunk0 ? kbar_chunk0[v] : cu[v]); }   // first chunk of video v's frame means
    int mask_step() const { return new_doc ? 1 : 0; }
};

// Every check of the call; nothing before its end changes a handle (the resets of new_doc come last).
int videos_validate(VideosCall& vc) {
    const char* name = vc.name; const infv_ltm_handle* hs = vc.hs; const int V = vc.V; const int32_t* cu = vc.cu;
    if (cu[0] < 0) return fail(INFV_ERR_INVALID, "%s: cu[0] = %d is negative", name, cu[0]);
    for (int v = 0; v < V; ++v)
        if (cu[v + 1] < cu[v]) return fail(INFV_ERR_INVALID, "%s: cu is not non-decreasing (cu[%d] = %d > cu[%d] = %d)",
                                            name, v, cu[v], v + 1, cu[v + 1]);
    vc.total = cu[V];
    if (vc.kbar_chunk0)
        for (int v = 0; v < V; ++v)
            if (vc.kbar_chunk0[v] < 0) return fail(INFV_ERR_INVALID, "%s: kbar_chunk0[%d] = %d is negative", name, v, vc.kbar_chunk0[v]);
    for (int v = 0; v < V; ++v) {                  // (before any handle is read)
        if (!hs[v]) return fail(INFV_ERR_INVALID, "%s: handle %d is null", name, v);
        for (int w = 0; w < v; ++w)
            if (hs[w] == hs[v]) return fail(INFV_ERR_INVALID, "%s: handle %d is also handle %d (a memory steps once per step)", name, v, w);
    }
    if (vc.total > 0 && ((vc.tokens ? !vc.k : !vc.kbar) || !vc.q || !vc.proj || !vc.ctx)) return fail(INFV_ERR_INVALID, "%s: null argument", name);
    for (int v = 0; v < V; ++v)                    // (the first read of a handle: the checks above refuse without one)
        if (hs[v]->mass_trace)
            return fail(INFV_ERR_UNSUPPORTED, "%s: handle %d has a mass trace set (infv_ltm_set_mass_trace): the lockstep calls do not write it", name, v);
    for (int v = 1; v < V; ++v)                    // (a trace that would silently stay empty: only the lead's is served)
        if (hs[v]->vmass_trace)
            return fail(INFV_ERR_INVALID, "%s: handle %d has a videos mass trace set (infv_ltm_set_videos_mass_trace): only handle 0's is written", name, v);
    for (int v = 1; v < V; ++v)
        if (!same_config(hs[0], hs[v], vc.tokens))
            return fail(INFV_ERR_INVALID, "%s: handle %d's configuration (N, H, dh, d, P, L, S, sticky%s) differs from handle 0's",
                        name, v, vc.tokens ? ", token dtype" : "");
    infv_ltm_handle h0 = hs[0];
    if (vc.tokens)
        if (int rc = check_k_aligned(name, h0->tok, vc.k)) return rc;
    vc.sticky = h0->cfg.sticky != 0;
    int max_len = 0;
    for (int v = 0; v < V; ++v) max_len = vc.len(v) > max_len ? vc.len(v) : max_len;
    if (vc.sticky && !vc.u && (vc.new_doc ? max_len > 1 : vc.total > 0)) {
        // generated uniforms: every handle draws from its own stream, so every handle needs its device rng on
        bool all_on = true;
        for (int v = 0; v < V; ++v) all_on = all_on && hs[v]->rng_on;
        if (!all_on) return fail(INFV_ERR_INVALID, "%s: sticky steps on an existing memory need the Gibbs uniforms u", name);
    }
    vc.plans.assign(V, nullptr);
    for (int v = 0; v < V; ++v) {
        infv_ltm_handle h = hs[v];
        if (int rc = check_chain_error(h)) return rc;
        if (int rc = check_q(h, vc.Q)) return rc;
        if (int rc = find_plan(h, vc.T, &vc.plans[v])) return rc;
        if (!same_plan(*vc.plans[0], *vc.plans[v]))
            return fail(INFV_ERR_INVALID, "%s: handle %d's plan for T = %d differs from handle 0's (tau, num_basis or "
                                          "the tables themselves): every video steps with one plan", name, v, vc.T);
        if (!vc.new_doc && !h->mem.has_memory())
            return fail(INFV_ERR_STATE, "%s: new_doc = 0 but handle %d holds no memory", name, v);
        if (!vc.new_doc && vc.sticky && h->mem.parts() <= 0)
            return fail(INFV_ERR_STATE, "%s: handle %d has no sticky histogram (import_state or step first)", name, v);
    }
    if (vc.tail_T) {
        // a short last chunk steps with the handle's plan for ITS length; videos that share a length share that plan, and every
        // plan of the call agrees on the tables the draw and the attend take once per step (Plan::shared_digest)
        vc.last_plans = vc.plans;
        vc.frame0.assign(V, 0);
        std::map<int, Plan*> by_tail;
        long long frame = 0;
        for (int v = 0; v < V; ++v) {
            vc.frame0[v] = frame;
            if (vc.len(v) == 0) continue;                        // (its tail_T entry is ignored)
            const int t = vc.tail_T[v];
            if (t != 0 && (t < 2 || t > vc.T))
                return fail(INFV_ERR_INVALID, "%s: tail_T[%d] = %d is neither 0 nor in [2, T = %d] (a chunk of one frame has an empty "
                                              "operator)", name, v, t, vc.T);
            frame += (long long)(vc.len(v) - 1) * vc.T + vc.tail(v);
            if (!vc.short_tail(v)) continue;
            if (int rc = find_plan(hs[v], t, &vc.last_plans[v])) return rc;
            const Plan& lp = *vc.last_plans[v];
            auto seen = by_tail.emplace(t, vc.last_plans[v]);
            if (!same_plan(*seen.first->second, lp))
                return fail(INFV_ERR_INVALID, "%s: handle %d's plan for its tail length %d differs from that of an earlier handle "
                                              "with the same tail length", name, v, t);
            if (lp.shared_digest != vc.plans[0]->shared_digest || lp.n_bins != vc.plans[0]->n_bins || lp.w_out != vc.plans[0]->w_out)
                return fail(INFV_ERR_INVALID, "%s: handle %d's plan for its tail length %d differs from the plan for T = %d in a table "
                                              "that does not depend on the chunk length (read-out weights, sticky histogram, uniform "
                                              "resampling): were they built for one (num_basis, tau, nb_samples)?", name, v, t, vc.T);
            vc.ragged = true;
        }
    }
    if (vc.new_doc)
        for (int v = 0; v < V; ++v) infv_ltm_reset(hs[v]);
    vc.chunk_k = (size_t)vc.T * h0->P * h0->d * token_bytes(h0->tok); vc.chunk_kbar = (size_t)vc.T * h0->d;
    vc.chunk_ctx = (size_t)h0->L * vc.Q * h0->dm; vc.chunk_u = (size_t)h0->L * h0->S;
    return INFV_OK;
}

// shapes the lockstep kernels do not take (dense / psi plans, N above 256, ...): each video's own per-call path, in turn
// (the handles were reset by videos_validate when new_doc is set).  The lead's packed mass trace is served through each handle's
// own per-chunk trace (infv_ltm_set_mass_trace's fields, empty here: videos_validate refuses a handle that has one) on the
// video's slice of the packed buffer, for the length of its call.
struct MassTraceSlice {
    infv_ltm_handle h; float* was; long was_cap;
    MassTraceSlice(infv_ltm_handle h_, float* slice, long cap) : h(h_), was(h_->mass_trace), was_cap(h_->mass_cap) {
        if (slice && cap > 0) { h->mass_trace = slice; h->mass_cap = cap; }
    }
    ~MassTraceSlice() { h->mass_trace = was; h->mass_cap = was_cap; }
};
// the handle's draw trace (infv_ltm_set_trace) is indexed by the chunk of the per-handle call: a video's second per-handle call
// (its short last chunk, infv_ltm_videos_tail) goes on at row `c0`, where the first one stopped
struct DrawTraceShift {
    infv_ltm_handle h; int32_t* bins; float* probs; long cap;
    DrawTraceShift(infv_ltm_handle h_, long c0) : h(h_), bins(h_->trace_bins), probs(h_->trace_probs), cap(h_->trace_cap) {
        if (c0 <= 0) return;
        if (bins) h->trace_bins = bins + (size_t)c0 * h->L * h->S;
        if (probs) h->trace_probs = probs + (size_t)c0 * h->L * h->n_bins;
        h->trace_cap = cap > c0 ? cap - c0 : 0;
    }
    ~DrawTraceShift() { h->trace_bins = bins; h->trace_probs = probs; h->trace_cap = cap; }
};

int videos_per_video(const VideosCall& vc) {
    infv_ltm_handle h0 = vc.hs[0];
    float* const vmass = h0->vmass_trace;
    const long vcap = h0->vmass_cap;
    // chunks [c0, c0 + n) of video v, all of T frames, the first of them `frame` frames into the packed k / kbar
    auto run = [&](int v, int c0, int n, int T, size_t frame) {
        infv_ltm_handle h = vc.hs[v];
        const size_t chunk = (size_t)vc.cu[v] + c0;
        MassTraceSlice tr_(h, vmass ? vmass + chunk * h0->L * h0->N : nullptr, vcap - (long)chunk);
        DrawTraceShift dt_(h, c0);
        const double* uv = vc.u ? vc.u + chunk * vc.chunk_u : nullptr;
        float* cv = vc.ctx + chunk * vc.chunk_ctx;
        if (vc.tokens)
            return infv_ltm_consolidate(h, vc.k + frame * (vc.chunk_k / vc.T), n, T, vc.q, vc.Q, vc.proj, uv, 0, cv, vc.stream_);
        if (vc.q_per_chunk)
            return infv_ltm_steps(h, vc.kbar + frame * h0->d, n, T, vc.q + chunk * vc.chunk_ctx, vc.Q, vc.proj, uv, cv, vc.stream_);
        return infv_ltm_consolidate_pooled(h, vc.kbar + frame * h0->d, n, T, vc.q, vc.Q, vc.proj, uv, 0, cv, vc.stream_);
    };
    for (int v = 0; v < vc.V; ++v) {
        const int n = vc.len(v);
        if (n == 0) continue;
        const size_t frame = vc.ragged ? (size_t)vc.frame0[v] : vc.kbar_base(v) * (size_t)vc.T;
        const int n_full = vc.short_tail(v) ? n - 1 : n;          // (infv_ltm_videos_tail: the full chunks, then one at the tail length)
        if (n_full > 0)
            if (int rc = run(v, 0, n_full, vc.T, frame)) return rc;
        if (n_full < n)
            if (int rc = run(v, n_full, 1, vc.tail(v), frame + (size_t)n_full * vc.T)) return rc;
    }
    return INFV_OK;
}

// The table of group [g0, g0 + gn): the videos ranked by decreasing length (vc.order), one VideoDesc per rank, written to the
// lead handle's vid_tab.  Returns the group's longest video in *g_len.
int videos_group_table(VideosCall& vc, int g0, int gn, int* g_len) {
    const int32_t* cu = vc.cu;
    vc.order.resize(gn);
    for (int i = 0; i < gn; ++i) vc.order[i] = g0 + i;
    std::stable_sort(vc.order.begin(), vc.order.end(), [&](int a, int b) { return cu[a + 1] - cu[a] > cu[b + 1] - cu[b]; });
    std::vector<VideoDesc> tab(gn, VideoDesc{});
    *g_len = 0;
    for (int j = 0; j < gn; ++j) {
        const int v = vc.order[j];
        infv_ltm_handle h = vc.hs[v];
        VideoDesc& e = tab[j];
        for (int i = 0; i < 2; ++i) { e.B[i] = h->B[i].as<float>(); e.KV[i] = h->KV[i].as<float>(); }
        e.bin_part = h->bin_part.as<float>();
        e.probs = h->probs.as<float>(); e.bins = h->bins.as<int32_t>(); e.idx = h->idx.as<int32_t>(); e.scores = h->scores.as<float>();
        e.probs_override = h->probs_override.as<float>(); e.bins_forced = h->bins_forced.as<int32_t>();
        e.override_mask = h->override_mask; e.forced_mask = h->forced_mask;
        e.trace_bins = h->trace_bins; e.trace_probs = h->trace_probs; e.trace_cap = h->trace_cap;
        e.chunk0 = cu[v];
        e.kbar0 = (long long)vc.kbar_base(v);
        e.cur0 = h->mem.cur();
        e.parts0 = vc.new_doc ? vc.parts : h->mem.parts();
        e.rng = h->rng_view(h->mem.pos());    // (reset by videos_validate when new_doc: step s of the call draws at position pos + s)
        *g_len = vc.len(v) > *g_len ? vc.len(v) : *g_len;
    }
    // the table travels in kernel arguments (launch_video_table): no host buffer outlives the call, nothing waits on the host,
    // and a captured graph holds its own copy; the group's launches and the next group's table write follow in stream order
    if (!vc.ragged) {
        HIP_TRY(launch_video_table(vc.hs[0]->vid_tab.as<VideoDesc>(), tab.data(), gn, vc.stream));
        return INFV_OK;
    }
    // ... and with it, in the same launches, the side table of the stages that depend on the chunk length (VideoTail)
    std::vector<VideoTail> tails(gn, VideoTail{});
    for (int j = 0; j < gn; ++j) {
        const int v = vc.order[j];
        VideoTail& t = tails[j];
        t.frame0 = vc.frame0[v];
        t.len = vc.len(v);
        t.tail = vc.tail(v);
        // a short chunk that starts a document (the video's only one, new_doc) takes its plan's first-chunk operator
        t.op_last = vc.short_tail(v) ? vc.last_plans[v]->device_view(!(vc.new_doc && t.len == 1)) : nullptr;
    }
    HIP_TRY(launch_video_tables(vc.hs[0]->vid_tab.as<VideoDesc>(), tab.data(), vc.hs[0]->vid_tail.as<VideoTail>(), tails.data(), gn,
                                vc.stream));
    return INFV_OK;
}

// The lockstep steps of the present group (vc.order): five launches per step, for the videos still running -- six while the lead
// carries a packed mass trace (infv_ltm_set_videos_mass_trace): the masses follow the attend launch whose scores they read, and
// stream order keeps the next step's attend behind them
int videos_steps(const VideosCall& vc, int g_len) {
    infv_ltm_handle h0 = vc.hs[0];
    const Plan& plan = *vc.plans[0];
    hipStream_t stream = vc.stream;
    const int N = h0->N, d = h0->d, dm = h0->dm, L = h0->L, S = h0->S, T = vc.T;
    const long q_stride = vc.q_per_chunk ? (long)vc.chunk_ctx : 0;
    int n = (int)vc.order.size();
    // ragged: the most new rows of any operator at work in step s -- the step's own, and those of the short chunks that end there.
    // The projected rows of a step are packed with THAT many row slots per video (in whole tiles), not with the call's maximum:
    // a tile without rows still costs a workgroup, and workgroups that do nothing at a regular stride of the grid leave the
    // workgroups that do work on few of the XCDs (256 x (7 + tail) at the headline shape, 4 tiles per video of which 3 are empty
    // in every step but the first: 31.7 ms of projection per call against 12.5 ms with the step's own count).
    std::vector<int> step_rows;
    if (vc.ragged) {
        step_rows.resize(g_len);
        for (int s = 0; s < g_len; ++s) step_rows[s] = (vc.new_doc && s == 0) ? plan.first.rows : plan.inf.rows;
        for (int v : vc.order)
            if (vc.short_tail(v)) {
                const Plan& lp = *vc.last_plans[v];
                const int rows = (vc.new_doc && vc.len(v) == 1) ? lp.first.rows : lp.inf.rows;
                step_rows[vc.len(v) - 1] = std::max(step_rows[vc.len(v) - 1], rows);
            }
    }
    for (int s = 0; s < g_len; ++s) {
        while (n > 0 && vc.len(vc.order[n - 1]) <= s) --n;
        const bool inf = !(vc.new_doc && s == 0);
        const Operator& op = inf ? plan.inf : plan.first;
        const VideoStep vs{h0->vid_tab.as<VideoDesc>(), s, n, vc.mask_step()};
        // ragged (infv_ltm_videos_tail with a short last chunk somewhere): the three stages that depend on the chunk length take it,
        // and the operator, per video rank; `op` is then the operator of the step's full chunks.  Every video of a call starts at
        // step 0, so "first chunk of a document" stays a property of the step.
        const TailStep ts{h0->vid_tail.as<VideoTail>(), T};
        const int row_slots = vc.ragged ? tail_row_slots(step_rows[s]) : 0;
        const int32_t* idx_shared = (inf && !vc.sticky) ? plan.uniform_idx.as<int32_t>() : nullptr;
        {
            Timed t_(h0->prof, INFV_KERNEL_POOL, stream);
            if (vc.ragged) {
                if (vc.tokens) HIP_TRY(launch_pool_videos_tail(vc.k, h0->tok, vs, ts, h0->P, d, h0->vid_kbar.as<float>(), stream));
                else HIP_TRY(launch_gather_videos_tail(vc.kbar, vs, ts, d, h0->vid_kbar.as<float>(), stream));
            }
            else if (vc.tokens) HIP_TRY(launch_pool_videos(vc.k, h0->tok, vs, T, h0->P, d, h0->vid_kbar.as<float>(), stream));
            else HIP_TRY(launch_gather_videos(vc.kbar, vs, T, d, h0->vid_kbar.as<float>(), stream));
        }
        {
            Timed t_(h0->prof, INFV_KERNEL_PROJECT, stream);
            if (vc.ragged)
                HIP_TRY(launch_project_videos_tail(h0->vid_kbar.as<float>(), vs, ts, d, dm, L, op.view(), row_slots, vc.pp,
                                                   h0->vid_P.as<float>(), stream));
            else
                HIP_TRY(launch_project_videos(h0->vid_kbar.as<float>(), n, T, d, dm, L, op.view(), vc.pp, h0->vid_P.as<float>(), stream));
        }
        if (inf && vc.sticky) {
            Timed t_(h0->prof, INFV_KERNEL_DRAW, stream);
            HIP_TRY(launch_draw_videos(vs, vc.parts, plan.sticky(), vc.u, S, L, stream));
        }
        {
            Timed t_(h0->prof, INFV_KERNEL_UPDATE, stream);
            if (vc.ragged)
                HIP_TRY(launch_update_videos_tail(vs, ts, op.view(), row_slots, N, d, dm, L, S, idx_shared, h0->vid_kbar.as<float>(),
                                                  h0->vid_P.as<float>(), stream));
            else
                HIP_TRY(launch_update_videos(vs, op.view(), N, T, d, dm, L, S, idx_shared, h0->vid_kbar.as<float>(), h0->vid_P.as<float>(),
                                             stream));
        }
        {
            Timed t_(h0->prof, INFV_KERNEL_ATTEND, stream);
            HIP_TRY(launch_attend_videos(vs, vc.q, q_stride, vc.Q, N, h0->H, L, vc.pp, plan.w.as<float>(), plan.w_out, plan.sticky(), vc.ctx,
                                         stream));
        }
        if (h0->vmass_trace)
            HIP_TRY(launch_box_mass_videos(vs, h0->H * vc.Q, N, L, plan.w.as<float>(), plan.w_out, h0->vmass_trace, h0->vmass_cap, stream));
    }
    return INFV_OK;
}

// the handles' host state after their chunks (chain_step's transitions, `len` steps at once), for the present group
void videos_bookkeeping(const VideosCall& vc) {
    for (int v : vc.order) {
        infv_ltm_handle h = vc.hs[v];
        const int len = vc.len(v);
        if (len == 0) continue;
        h->mem.memory_written(len);
        h->mem.attended(vc.last_plan(v), vc.Q, vc.parts, len);
        if (vc.sticky && len > vc.mask_step()) { h->override_mask = 0; h->forced_mask = 0; }
    }
}

int videos_impl(VideosCall& vc) {
    if (!vc.hs || !vc.cu || vc.V < 0) return fail(INFV_ERR_INVALID, "%s: bad arguments", vc.name);
    if (vc.V == 0) return INFV_OK;
    if (int rc = videos_validate(vc)) return rc;
    if (vc.total == 0) return INFV_OK;
    infv_ltm_handle h0 = vc.hs[0];
    const Plan& plan = *vc.plans[0];
    const int V = vc.V;
    bool dense = plan.dense.on;
    vc.rows_max = plan.first.rows > plan.inf.rows ? plan.first.rows : plan.inf.rows;
    if (vc.ragged)
        for (int v = 0; v < V; ++v) {
            const Plan& lp = *vc.last_plans[v];
            dense = dense || lp.dense.on;                        // (whether the boxes overlap at a sample position depends on T too)
            vc.rows_max = std::max(vc.rows_max, std::max(lp.first.rows, lp.inf.rows));
        }
    if (!videos_supported(h0->N, h0->d, h0->dm, h0->L, h0->S) || dense) return videos_per_video(vc);
    vc.stream = static_cast<hipStream_t>(vc.stream_);
    vc.pp = make_proj(vc.proj, h0->L);
    for (int v = 0; v < V; ++v)                    // the per-call step re-derives a stale K' half before stepping (infv_ltm_step)
        if (vc.len(v) > 0 && vc.hs[v]->mem.k_stale() && vc.hs[v]->mem.has_memory())
            if (int rc = infv_ltm_reproject(vc.hs[v], vc.proj, vc.stream_)) return rc;
    // row slots per video of the projected rows: the plan's most rows; ragged, the most of any plan involved, in whole 64-row tiles
    const int row_slots = vc.ragged ? tail_row_slots(vc.rows_max) : (vc.rows_max > 0 ? vc.rows_max : 1);
    const int group = V < kVideoGroup ? V : kVideoGroup;
    // workspaces of one step (grown, never shrunk; released with the lead handle)
    HIP_TRY(reserve_all({{h0->vid_tab, (size_t)group * sizeof(VideoDesc)},
                         {h0->vid_tail, vc.ragged ? (size_t)group * sizeof(VideoTail) : 0},
                         {h0->vid_kbar, (size_t)group * vc.T * h0->d * sizeof(float)},
                         {h0->vid_P, (size_t)group * row_slots * h0->L * 2 * h0->dm * sizeof(float)}}));
    vc.parts = attend_parts(vc.Q, h0->H, h0->N);
    for (int g0 = 0; g0 < V; g0 += group) {
        int g_len = 0;
        if (int rc = videos_group_table(vc, g0, V - g0 < group ? V - g0 : group, &g_len)) return rc;
        if (int rc = videos_steps(vc, g_len)) return rc;
        videos_bookkeeping(vc);
    }
    return INFV_OK;
}
}  // namespace

extern "C" {

int infv_ltm_consolidate_videos(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const void* k, int32_t T, const float* q,
                                int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx, void* stream) {
    VideosCall vc{};
    vc.name = "consolidate_videos"; vc.hs = hs; vc.V = V; vc.cu = cu; vc.tokens = true; vc.k = static_cast<const char*>(k);
    vc.T = T; vc.q = q; vc.Q = Q; vc.proj = proj; vc.u = u; vc.new_doc = new_doc; vc.ctx = ctx; vc.stream_ = stream;
    return videos_impl(vc);
}

int infv_ltm_steps_videos(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const float* kbar, int32_t T, const float* q,
                          int32_t q_per_chunk, int32_t Q, const infv_ltm_proj* proj, const double* u, int32_t new_doc, float* ctx,
                          void* stream) {
    if (q_per_chunk != 0 && q_per_chunk != 1) return fail(INFV_ERR_INVALID, "steps_videos: q_per_chunk must be 0 or 1");
    VideosCall vc{};
    vc.name = "steps_videos"; vc.hs = hs; vc.V = V; vc.cu = cu; vc.kbar = kbar; vc.q_per_chunk = q_per_chunk != 0;
    vc.T = T; vc.q = q; vc.Q = Q; vc.proj = proj; vc.u = u; vc.new_doc = new_doc; vc.ctx = ctx; vc.stream_ = stream;
    return videos_impl(vc);
}

int infv_ltm_steps_videos_from(const infv_ltm_handle* hs, int32_t V, const int32_t* cu, const float* kbar, const int32_t* kbar_chunk0,
                               int32_t T, const float* q, int32_t q_per_chunk, int32_t Q, const infv_ltm_proj* proj, const double* u,
                               int32_t new_doc, float* ctx, void* stream) {
    if (q_per_chunk != 0 && q_per_chunk != 1) return fail(INFV_ERR_INVALID, "steps_videos_from: q_per_chunk must be 0 or 1");
    VideosCall vc{};
    vc.name = "steps_videos_from"; vc.hs = hs; vc.V = V; vc.cu = cu; vc.kbar = kbar; vc.kbar_chunk0 = kbar_chunk0; vc.q_per_chunk = q_per_chunk != 0;
    vc.T = T; vc.q = q; vc.Q = Q; vc.proj = proj; vc.u = u; vc.new_doc = new_doc; vc.ctx = ctx; vc.stream_ = stream;
    return videos_impl(vc);
}

int infv_ltm_videos_tail(const infv_ltm_videos_tail_desc* d) {
    if (!d) return fail(INFV_ERR_INVALID, "videos_tail: null descriptor");
    if (!d->tail_T) return fail(INFV_ERR_INVALID, "videos_tail: null tail_T");
    if ((d->k != nullptr) == (d->kbar != nullptr)) return fail(INFV_ERR_INVALID, "videos_tail: exactly one of k (frame tokens) and kbar (frame means) must be given");
    if (d->q_per_chunk != 0 && d->q_per_chunk != 1) return fail(INFV_ERR_INVALID, "videos_tail: q_per_chunk must be 0 or 1");
    if (d->reserved != 0) return fail(INFV_ERR_INVALID, "videos_tail: reserved must be 0");
    VideosCall vc{};
    vc.name = "videos_tail"; vc.hs = d->hs; vc.V = d->V; vc.cu = d->cu; vc.tail_T = d->tail_T;
    vc.tokens = d->k != nullptr; vc.k = static_cast<const char*>(d->k); vc.kbar = d->kbar; vc.q_per_chunk = d->q_per_chunk != 0;
    vc.T = d->T; vc.q = d->q; vc.Q = d->Q; vc.proj = d->proj; vc.u = d->u; vc.new_doc = d->new_doc; vc.ctx = d->ctx; vc.stream_ = d->hip_stream;
    return videos_impl(vc);
}

// ---- device rng (philox.h) ----
int infv_ltm_set_rng(infv_ltm_handle h, int32_t on, uint64_t seed, uint32_t stream_id) {
    if (int rc = check_handle(h)) return rc;
    h->rng_on = on != 0;
    h->rng_seed = seed;
    h->rng_stream = stream_id;
    return INFV_OK;
}

int infv_ltm_get_rng_position(infv_ltm_handle h, uint32_t* pos) {
    if (int rc = check_handle(h)) return rc;
    if (!pos) return fail(INFV_ERR_INVALID, "get_rng_position: null pos");
    *pos = h->mem.pos();
    return INFV_OK;
}

int infv_ltm_set_rng_position(infv_ltm_handle h, uint32_t pos) {
    if (int rc = check_handle(h)) return rc;
    h->mem.set_rng_position(pos);
    return INFV_OK;
}

static int rng_fill_check(const char* name, int32_t n_steps, int32_t n_layers, int32_t S, const void* out) {
    if (n_steps < 0 || n_layers < 1 || S < 1) return fail(INFV_ERR_INVALID, "%s: n_steps must not be negative, n_layers and S positive", name);
    if (n_steps > 0 && !out) return fail(INFV_ERR_INVALID, "%s: null output", name);
    if ((uint64_t)n_steps * (uint64_t)n_layers * (uint64_t)S > ((uint64_t)1 << 40)) return fail(INFV_ERR_INVALID, "%s: too many uniforms", name);
    return INFV_OK;
}

int infv_ltm_rng_fill(uint64_t seed, uint32_t stream_id, uint32_t pos0, int32_t n_steps, int32_t n_layers, int32_t S,
                      double* u_device, void* stream) {
    if (int rc = rng_fill_check("rng_fill", n_steps, n_layers, S, u_device)) return rc;
    HIP_TRY(launch_rng_fill(make_rng_view(seed, stream_id, pos0), n_steps, n_layers, S, u_device, nullptr,
                            static_cast<hipStream_t>(stream)));
    return INFV_OK;
}

int infv_ltm_rng_fill_host(uint64_t seed, uint32_t stream_id, uint32_t pos0, int32_t n_steps, int32_t n_layers, int32_t S,
                           double* u_host) {
    if (int rc = rng_fill_check("rng_fill_host", n_steps, n_layers, S, u_host)) return rc;
    const RngView g = make_rng_view(seed, stream_id, pos0);
    for (int32_t i = 0; i < n_steps; ++i)
        for (int l = 0; l < n_layers; ++l) {
            double* row = u_host + ((size_t)i * n_layers + l) * S;
            for (int s = 0; s < S; s += 2) {
                const Philox4 b = gibbs_block(g, (uint32_t)l, pos0 + (uint32_t)i, (uint32_t)(s >> 1));
                row[s] = philox_u53(b.w[0], b.w[1]);
                if (s + 1 < S) row[s + 1] = philox_u53(b.w[2], b.w[3]);
            }
        }
    return INFV_OK;
}

int infv_ltm_export_state(infv_ltm_handle h, int32_t layer, float* B, float* bin_mass, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L) return fail(INFV_ERR_INVALID, "layer out of range");
    if (int rc = check_chain_error(h)) return rc;
    if (!h->mem.has_memory()) return fail(INFV_ERR_STATE, "no memory to export (B_past is None)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (B) HIP_TRY(hipMemcpyAsync(B, h->B[h->mem.cur()].as<float>() + (size_t)layer * h->N * h->d,
                                  (size_t)h->N * h->d * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (bin_mass) {
        HIP_TRY(launch_sum_parts(h->bin_part.as<float>() + (size_t)layer * h->mem.parts() * h->n_bins, h->mem.parts(), h->n_bins,
                                 bin_mass, stream));
    }
    return INFV_OK;
}

int infv_ltm_set_ctx_sum(infv_ltm_handle h, int32_t on) {
    if (int rc = check_handle(h)) return rc;
    if (on) HIP_TRY(h->ctx_sum.reserve((size_t)h->L * h->maxQ * h->dm * sizeof(float)));
    h->ctx_sum_on = on != 0;
    h->mem.drop_ctx_sum();
    return INFV_OK;
}

int infv_ltm_pack_memory(infv_ltm_handle h, int32_t n_basis, int32_t Q, const float* ctx, int32_t n_chunks, int32_t with_scores,
                         float* payload, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!ctx || !payload || n_chunks < 0 || n_basis <= 0 || n_basis > h->N) return fail(INFV_ERR_INVALID, "pack_memory: bad arguments");
    if (int rc = check_q(h, Q)) return rc;
    if (int rc = check_chain_error(h)) return rc;
    if (!h->mem.has_memory()) return fail(INFV_ERR_STATE, "no memory to export (B_past is None)");
    if (with_scores && !h->mem.chain_exportable(Q))          // (has_memory, which the predicate includes, holds here: refused above)
        return fail(INFV_ERR_STATE, "pack_memory: the scores need a memory whose last step came from infv_ltm_consolidate with Q=%d", Q);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t nC = (size_t)h->L * Q * h->dm;
    if (!h->mem.ctx_sum_holds(ctx, n_chunks, Q)) {
        // no sum kept for these outputs (dense / psi plans, the per-chunk path, sums switched off, someone else's ctx): add them up
        // now, in ctx_sum_kernel's fixed order; that overwrites whatever sum the handle held
        h->mem.drop_ctx_sum();
        HIP_TRY(reserve_all({{h->ctx_sum, (size_t)h->L * h->maxQ * h->dm * sizeof(float)}}));
        HIP_TRY(launch_ctx_sum(ctx, n_chunks, (long)nC, h->ctx_sum.as<float>(), stream));
    }
    PackMemoryArgs a;
    memset(&a, 0, sizeof(a));
    a.B = h->B[h->mem.cur()].as<float>(); a.N = n_basis; a.Np = h->N; a.d = h->d;
    a.part = h->bin_part.as<float>(); a.parts = h->mem.parts(); a.pitch = h->n_bins; a.n_mass = h->n_bins - 1;
    a.scores = with_scores ? h->Sp[h->mem.sc()].as<float>() : nullptr;
    a.ctx_sum = h->ctx_sum.as<float>(); a.count = (float)n_chunks;
    a.nB = (long)h->L * n_basis * h->d; a.nM = (long)h->L * a.n_mass; a.nS = with_scores ? (long)h->L * h->H * Q * n_basis : 0; a.nC = (long)nC;
    a.out = payload;
    HIP_TRY(launch_pack_memory(a, stream));
    return INFV_OK;
}

int64_t infv_ltm_chain_state_bytes(infv_ltm_handle h, int32_t Q) {
    if (!h || Q <= 0 || Q > h->maxQ) return -1;
    return (int64_t)sizeof(float) * (kBlobHeaderInts + (int64_t)h->L * h->N * h->d + (int64_t)h->L * h->N * 2 * h->dm +
                                     (int64_t)h->L * h->H * Q * h->N + (int64_t)h->L * h->n_bins + (int64_t)h->L * h->H * Q);
}

namespace {
BlobHeader blob_header(infv_ltm_handle h, int Q) {
    BlobHeader hd{};
    const int v[] = {kBlobMagic, kBlobVersion, h->L, h->N, h->d, h->dm, h->H, Q, h->n_bins};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) hd.v[i] = v[i];
    return hd;
}
}  // namespace

int infv_ltm_export_chain_state(infv_ltm_handle h, int32_t Q, void* blob, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!blob) return fail(INFV_ERR_INVALID, "export_chain_state: null blob");
    if (int rc = check_q(h, Q)) return rc;
    if (int rc = check_chain_error(h)) return rc;
    if (!h->mem.chain_exportable(Q))
        return fail(INFV_ERR_STATE, "export_chain_state: the memory's last step must come from infv_ltm_consolidate with Q=%d", Q);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    INFV_LAUNCH(blob_header_write_kernel, dim3(1), dim3(64), 0, stream, static_cast<int*>(blob), blob_header(h, Q));
    HIP_TRY(hipGetLastError());
    float* out = static_cast<float*>(blob) + kBlobHeaderInts;
    const size_t nB = (size_t)h->L * h->N * h->d, nKV = (size_t)h->L * h->N * 2 * h->dm, nS = (size_t)h->L * h->H * Q * h->N,
                 nM = (size_t)h->L * h->n_bins;
    HIP_TRY(hipMemcpyAsync(out, h->B[h->mem.cur()].p, nB * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(out + nB, h->KV[h->mem.cur()].p, nKV * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(out + nB + nKV, h->Sp[h->mem.sc()].p, nS * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(out + nB + nKV + nS, h->bin_part.p, nM * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(out + nB + nKV + nS + nM, h->cqbuf.p, (size_t)h->L * h->H * Q * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return INFV_OK;
}

int infv_ltm_import_chain_state(infv_ltm_handle h, int32_t Q, const void* blob, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!blob) return fail(INFV_ERR_INVALID, "import_chain_state: null blob");
    if (int rc = check_q(h, Q)) return rc;
    if (int rc = check_chain_error(h)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the header is checked on the device (the call stays asynchronous): a mismatch latches an error that the next entry point reports
    INFV_LAUNCH(blob_header_check_kernel, dim3(1), dim3(1), 0, stream, static_cast<const int*>(blob), blob_header(h, Q), h->err_dev);
    HIP_TRY(hipGetLastError());
    const float* in = static_cast<const float*>(blob) + kBlobHeaderInts;
    const size_t nB = (size_t)h->L * h->N * h->d, nKV = (size_t)h->L * h->N * 2 * h->dm, nS = (size_t)h->L * h->H * Q * h->N,
                 nM = (size_t)h->L * h->n_bins;
    HIP_TRY(hipMemcpyAsync(h->B[h->mem.cur()].p, in, nB * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(h->KV[h->mem.cur()].p, in + nB, nKV * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(h->Sp[h->mem.sc()].p, in + nB + nKV, nS * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(h->bin_part.p, in + nB + nKV + nS, nM * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(h->cqbuf.p, in + nB + nKV + nS + nM, (size_t)h->L * h->H * Q * sizeof(float), hipMemcpyDeviceToDevice, stream));
    h->mem.chain_imported(Q);
    return INFV_OK;
}

int infv_ltm_reproject(infv_ltm_handle h, const infv_ltm_proj* proj, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (!proj) return fail(INFV_ERR_INVALID, "reproject: null proj");
    if (!h->mem.has_memory()) return INFV_OK;
    const ProjPtrs pp = make_proj(proj, h->L);
    HIP_TRY(launch_reproject(h->B[h->mem.cur()].as<float>(), h->N, h->d, h->dm, h->L, pp, h->KV[h->mem.cur()].as<float>(),
                             static_cast<hipStream_t>(stream_)));
    h->mem.reprojected();
    return INFV_OK;
}

int infv_ltm_import_state(infv_ltm_handle h, int32_t layer, const float* B, const float* bin_mass,
                          const infv_ltm_proj* proj, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L) return fail(INFV_ERR_INVALID, "layer out of range");
    if (!B || !proj) return fail(INFV_ERR_INVALID, "import: null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipMemcpyAsync(h->B[h->mem.cur()].as<float>() + (size_t)layer * h->N * h->d, B,
                           (size_t)h->N * h->d * sizeof(float), hipMemcpyDeviceToDevice, stream));
    h->mem.layer_import_begins();
    float* part = h->bin_part.as<float>() + (size_t)layer * h->mem.parts() * h->n_bins;
    HIP_TRY(hipMemsetAsync(part, 0, (size_t)h->mem.parts() * h->n_bins * sizeof(float), stream));
    if (bin_mass)
        HIP_TRY(hipMemcpyAsync(part, bin_mass, (size_t)(h->n_bins - 1) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    // re-project this layer's memory with its weights
    ProjPtrs one;
    memset(&one, 0, sizeof(one));
    one.wk[0] = proj->wk; one.bk[0] = proj->bk; one.wv[0] = proj->wv; one.bv[0] = proj->bv;
    HIP_TRY(launch_reproject(h->B[h->mem.cur()].as<float>() + (size_t)layer * h->N * h->d, h->N, h->d, h->dm, 1, one,
                             h->KV[h->mem.cur()].as<float>() + (size_t)layer * h->N * 2 * h->dm, stream));
    h->mem.layer_imported();
    return INFV_OK;
}

int infv_ltm_get_draw(infv_ltm_handle h, int32_t layer, int32_t* bins, int32_t* idx, float* probs,
                      float* scores, void* stream_) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L) return fail(INFV_ERR_INVALID, "layer out of range");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipStreamSynchronize(stream));
    if (int rc = check_chain_error(h)) return rc;
    if (bins) HIP_TRY(hipMemcpy(bins, h->bins.as<int32_t>() + (size_t)layer * h->S, h->S * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (idx) HIP_TRY(hipMemcpy(idx, h->idx.as<int32_t>() + (size_t)layer * h->S, h->S * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (probs) HIP_TRY(hipMemcpy(probs, h->probs.as<float>() + (size_t)layer * h->n_bins, (h->n_bins - 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (scores) {
        if (h->mem.lastQ() <= 0) return fail(INFV_ERR_STATE, "no scores yet");
        const size_t n = (size_t)h->H * h->mem.lastQ() * h->N;
        if (h->mem.last_fast()) {
            std::vector<float> cq((size_t)h->H * h->mem.lastQ());
            HIP_TRY(hipMemcpy(scores, h->Sp[h->mem.sc()].as<float>() + (size_t)layer * n, n * sizeof(float), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cq.data(), h->cqbuf.as<float>() + (size_t)layer * cq.size(), cq.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t r = 0; r < cq.size(); ++r)
                for (int j = 0; j < h->N; ++j) scores[r * h->N + j] += cq[r];
        } else {
            HIP_TRY(hipMemcpy(scores, h->scores.as<float>() + (size_t)layer * n, n * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return INFV_OK;
}

int infv_ltm_set_probs(infv_ltm_handle h, int32_t layer, const float* probs) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L || !probs) return fail(INFV_ERR_INVALID, "set_probs: bad arguments");
    // The setter has no stream: it takes effect in PROGRAM order.  A step queued on a non-blocking stream may still be waiting to
    // read an earlier override, and the null stream's copy below would overtake it.
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->probs_override.as<float>() + (size_t)layer * h->n_bins, probs,
                      (h->n_bins - 1) * sizeof(float), hipMemcpyHostToDevice));
    h->override_mask |= 1u << layer;
    return INFV_OK;
}

int infv_ltm_set_bins(infv_ltm_handle h, int32_t layer, const int32_t* bins) {
    if (int rc = check_handle(h)) return rc;
    if (layer < 0 || layer >= h->L || !bins) return fail(INFV_ERR_INVALID, "set_bins: bad arguments");
    for (int s = 0; s < h->S; ++s)
        if (bins[s] < 0 || bins[s] >= h->n_bins - 1) return fail(INFV_ERR_INVALID, "set_bins: bins[%d]=%d outside [0,%d)", s, bins[s], h->n_bins - 1);
    HIP_TRY(hipDeviceSynchronize());                            // program order, as in infv_ltm_set_probs: a queued step may still read the old bins
    HIP_TRY(hipMemcpy(h->bins_forced.as<int32_t>() + (size_t)layer * h->S, bins, h->S * sizeof(int32_t), hipMemcpyHostToDevice));
    h->forced_mask |= 1u << layer;
    return INFV_OK;
}

int infv_ltm_set_trace(infv_ltm_handle h, int32_t* bins_all, float* probs_all, int64_t capacity_chunks) {
    if (int rc = check_handle(h)) return rc;
    if (capacity_chunks < 0) return fail(INFV_ERR_INVALID, "set_trace: negative capacity");
    h->trace_bins = capacity_chunks ? bins_all : nullptr;
    h->trace_probs = capacity_chunks ? probs_all : nullptr;
    h->trace_cap = (h->trace_bins || h->trace_probs) ? (long)capacity_chunks : 0;
    return INFV_OK;
}

int infv_ltm_sync(infv_ltm_handle h, void* stream) {
    if (int rc = check_handle(h)) return rc;
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return check_chain_error(h);
}

int infv_ltm_profile_enable(infv_ltm_handle h, int32_t on) {
    if (int rc = check_handle(h)) return rc;
    h->prof.on = on != 0;
    if (!on) h->prof.clear_all();
    return INFV_OK;
}

int infv_ltm_profile_read(infv_ltm_handle h, int32_t kernel, int64_t* launches, double* total_ms) {
    if (int rc = check_handle(h)) return rc;
    if (kernel < 0 || kernel >= INFV_KERNEL_COUNT || !launches || !total_ms) return fail(INFV_ERR_INVALID, "profile_read: bad arguments");
    double ms = 0.0;
    for (auto& p : h->prof.ev[kernel]) {
        HIP_TRY(hipEventSynchronize(p.second));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, p.first, p.second));
        ms += t;
    }
    *launches = (int64_t)h->prof.ev[kernel].size();
    *total_ms = ms;
    h->prof.clear(kernel);
    return INFV_OK;
}

}  // extern "C"
